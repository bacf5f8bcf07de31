"""CPU tier: the built gfx950 code objects of the multi-head attention query kernels (csrc/query.hip: mhgat_hops_kernel<1> for
H <= 256, <2> for H <= 512, and mhgat_tail_kernel), read from the library's metadata as tests/test_code_objects_cpu.py reads it.
The hops kernel keeps four table rows of up to two float4 and their per-slot weights in flight beside the row's accumulator; the
heads' accumulators live in LDS and the per-head scalars on lanes, so the head count costs no registers: no instantiation may
spill a VGPR or use scratch (a condition), and each is held to the occupancy step (64 / 96 / 128 / 168 / 256 VGPRs, those of
tests/test_gat_heads_code_objects_cpu.py) above the count this build reports: 68, 102 and 68 (DESIGN.md section 4 quotes them; the
tail's workgroups per CU are set by its LDS, not by its registers)."""
from test_code_objects_cpu import _kernels, code_objects  # noqa: F401  (the module-scoped fixture)

CEILINGS = {
    r"mhgat_hops_kernelILi1E": (1, 96),
    r"mhgat_hops_kernelILi2E": (1, 128),
    r"mhgat_tail_kernel": (1, 96),
}


def test_every_instantiation_is_listed(code_objects):  # noqa: F811
    hits = _kernels(code_objects, r"mhgat_")
    assert len(hits) == len(CEILINGS) == 3, sorted(hits)


def test_mhgat_query_kernels_neither_spill_nor_use_scratch(code_objects):  # noqa: F811
    for pattern, (count, ceiling) in CEILINGS.items():
        hits = _kernels(code_objects, pattern)
        assert len(hits) == count, (pattern, sorted(hits))
        for name, m in hits.items():
            assert m["vgpr_spill"] == 0 and m["scratch"] == 0, (name, m)
            assert m["vgpr"] <= ceiling, (name, m)
