"""CPU tier: the built gfx950 code objects of the two graph-query kernels (csrc/query.hip), read from the library's metadata as
tests/test_code_objects_cpu.py reads it.  The hops kernel keeps four table rows in flight per lane and the tail four MFMA
accumulators per wave: neither may spill a VGPR or use scratch."""
from test_code_objects_cpu import _kernels, code_objects  # noqa: F401  (the module-scoped fixture)


def test_graph_query_kernels_neither_spill_nor_use_scratch(code_objects):  # noqa: F811
    for pat in (r"graph_query_hops_kernel", r"graph_query_tail_kernel"):
        found = _kernels(code_objects, pat)
        assert found, pat
        for name, m in found.items():
            assert m["vgpr_spill"] == 0 and m["scratch"] == 0, (name, m)
            assert m["vgpr"] <= 128, (name, m)   # two workgroups of 256 threads per SIMD set at least
