"""CPU tier: the built gfx950 code objects of the two GIN graph-query kernels (csrc/query.hip: gin_graph_query_hops_kernel<NS>, one or
two 256-column slots of Ha, and gin_graph_query_tail_kernel), read from the library's metadata as tests/test_code_objects_cpu.py reads
it.  A lane of the hops kernel keeps four table rows of NS float4 and the row's root in flight, then four MFMA accumulators: no kernel
may spill a VGPR or use scratch, and each stays within 128 VGPRs."""
from test_code_objects_cpu import _kernels, code_objects  # noqa: F401  (the module-scoped fixture)


def _held(hits):
    for name, m in hits.items():
        assert m["vgpr_spill"] == 0 and m["scratch"] == 0, (name, m)
        assert m["vgpr"] <= 128, (name, m)


def test_gin_graph_hops_kernels_neither_spill_nor_use_scratch(code_objects):  # noqa: F811
    hits = _kernels(code_objects, r"gin_graph_query_hops_kernel")
    assert len(hits) == 2, sorted(hits)
    _held(hits)


def test_gin_graph_tail_kernel_neither_spills_nor_uses_scratch(code_objects):  # noqa: F811
    hits = _kernels(code_objects, r"gin_graph_query_tail_kernel")
    assert len(hits) == 1, sorted(hits)
    _held(hits)
