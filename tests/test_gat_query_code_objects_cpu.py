"""CPU tier: the built gfx950 code objects of the attention query kernel (csrc/query.hip, gat_query_hops_kernel<1> for H <= 256 and
<2> for H <= 512), read from the library's metadata as tests/test_code_objects_cpu.py reads it.  A lane keeps four table rows of up
to two float4 in flight beside the row's accumulator and the wave's online-softmax state: neither instantiation may spill a VGPR
or use scratch, and both stay within the 128 VGPRs the GCN gather is held to."""
from test_code_objects_cpu import _kernels, code_objects  # noqa: F401  (the module-scoped fixture)


def test_gat_query_kernel_neither_spills_nor_uses_scratch(code_objects):  # noqa: F811
    hits = _kernels(code_objects, r"gat_query_hops_kernel")
    assert len(hits) == 2, sorted(hits)   # one and two column slots per lane
    for name, m in hits.items():
        assert m["vgpr_spill"] == 0 and m["scratch"] == 0, (name, m)
        assert m["vgpr"] <= 128, (name, m)   # two workgroups of 256 threads per SIMD set at least
