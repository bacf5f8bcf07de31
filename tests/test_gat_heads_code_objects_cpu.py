"""CPU tier: the built gfx950 code objects of the multi-head attention kernels (csrc/gat_heads.hip), read from the library's metadata
as tests/test_code_objects_cpu.py reads it.  Every instantiation keeps its registers: no VGPR spill, no scratch.  The ceilings are
the occupancy steps of a SIMD lane's 512 VGPRs (allocated in blocks of 8: 64 -> 8 waves, 96 -> 5, 128 -> 4, 168 -> 3) that each
kernel is held to:

  aggregate / sddmm <1>     a float4 of four operand rows in flight beside the accumulator / the row of dOut: 64 (8 waves per SIMD)
  aggregate / sddmm <2>     twice that, eight 16-byte loads per lane in flight: 96 (5 waves)
  aggregate <4>             sixteen loads in flight, 16 accumulator values, 16 weights: 128 (4 waves)
  sddmm <4>                 sixteen loads in flight, the 16 values of dOut and the 16 per-slot partial sums of four entries live
                            through their butterflies: 168 (3 waves; each already keeps 16 row fetches per lane in flight)
  their scalar twins, scores, the two softmax passes: a handful of values (a short row's 8 or 16 in registers): 64 (8 waves)
"""
from test_code_objects_cpu import _kernels, code_objects  # noqa: F401  (the module-scoped fixture)

CEILINGS = {
    r"gat_heads_scores_kernel": (1, 64),
    r"gat_heads_edge_softmax_kernel": (1, 64),
    r"gat_heads_softmax_bwd_kernel": (1, 64),
    r"gat_heads_aggregate_scalar_kernel": (1, 64),
    r"gat_heads_sddmm_scalar_kernel": (1, 64),
    r"gat_heads_aggregate_kernelILi1E": (1, 64),
    r"gat_heads_aggregate_kernelILi2E": (1, 96),
    r"gat_heads_aggregate_kernelILi4E": (1, 128),
    r"gat_heads_sddmm_kernelILi1E": (1, 64),
    r"gat_heads_sddmm_kernelILi2E": (1, 96),
    r"gat_heads_sddmm_kernelILi4E": (1, 168),
}


def test_every_instantiation_is_listed(code_objects):  # noqa: F811
    hits = _kernels(code_objects, r"gat_heads_")
    assert len(hits) == len(CEILINGS), sorted(hits)


def test_gat_heads_kernels_neither_spill_nor_use_scratch(code_objects):  # noqa: F811
    for pattern, (count, ceiling) in CEILINGS.items():
        hits = _kernels(code_objects, pattern)
        assert len(hits) == count, (pattern, sorted(hits))
        for name, m in hits.items():
            assert m["vgpr_spill"] == 0 and m["scratch"] == 0, (name, m)
            assert m["vgpr"] <= ceiling, (name, m)
