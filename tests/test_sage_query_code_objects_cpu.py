"""CPU tier: the built gfx950 code object of the SAGE query gather (csrc/query.hip, sage_query_gather_kernel; one instantiation),
read from the library's metadata as tests/test_code_objects_cpu.py reads it.  A lane keeps four table rows and the row's root float4
in flight beside the row's accumulator and the wave's partial: it may not spill a VGPR or use scratch, and stays within the 128
VGPRs the GCN gather is held to."""
from test_code_objects_cpu import _kernels, code_objects  # noqa: F401  (the module-scoped fixture)


def test_sage_query_kernel_neither_spills_nor_uses_scratch(code_objects):  # noqa: F811
    hits = _kernels(code_objects, r"sage_query_gather_kernel")
    assert len(hits) == 1, sorted(hits)
    for name, m in hits.items():
        assert m["vgpr_spill"] == 0 and m["scratch"] == 0, (name, m)
        assert m["vgpr"] <= 128, (name, m)   # two workgroups of 256 threads per SIMD set at least
