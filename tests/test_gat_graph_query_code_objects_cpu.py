"""CPU tier: the built gfx950 code objects of the GAT graph-query kernel (csrc/query.hip: gat_graph_query_hops_kernel<NS>, one or two
256-column slots of H), read from the library's metadata as tests/test_code_objects_cpu.py reads it.  In phase 1 a lane keeps four
table rows of NS float4 in flight beside the row's accumulators, the bias and both score vectors; in phase 2 its sum of NS float4: no
instance may spill a VGPR or use scratch, and each stays within 128 VGPRs."""
from test_code_objects_cpu import _kernels, code_objects  # noqa: F401  (the module-scoped fixture)


def test_gat_graph_hops_kernels_neither_spill_nor_use_scratch(code_objects):  # noqa: F811
    hits = _kernels(code_objects, r"gat_graph_query_hops_kernel")
    assert len(hits) == 2, sorted(hits)
    for name, m in hits.items():
        assert m["vgpr_spill"] == 0 and m["scratch"] == 0, (name, m)
        assert m["vgpr"] <= 128, (name, m)
