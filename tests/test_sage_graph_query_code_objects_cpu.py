"""CPU tier: the built gfx950 code object of the SAGE graph-query kernel (csrc/query.hip: sage_graph_query_hops_kernel, one 256-column
slab of H per workgroup), read from the library's metadata as tests/test_code_objects_cpu.py reads it.  In phase 1 a lane keeps four
table float4 and the root float4 in flight beside the row's accumulator and the bias; in phase 2 its sum of one float4: the kernel may
not spill a VGPR or use scratch, and stays within 128 VGPRs, the bound the GCN graph hops kernel is held to."""
from test_code_objects_cpu import _kernels, code_objects  # noqa: F401  (the module-scoped fixture)


def test_sage_graph_hops_kernel_neither_spills_nor_uses_scratch(code_objects):  # noqa: F811
    hits = _kernels(code_objects, r"sage_graph_query_hops_kernel")
    assert len(hits) == 1, sorted(hits)
    for name, m in hits.items():
        assert m["vgpr_spill"] == 0 and m["scratch"] == 0, (name, m)
        assert m["vgpr"] <= 128, (name, m)
