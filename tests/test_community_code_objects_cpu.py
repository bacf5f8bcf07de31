"""CPU tier: the built gfx950 code objects of the community detection sweep (csrc/community.hip; one kernel per launch branch),
read from the library's metadata as tests/test_code_objects_cpu.py reads it.  A lane holds an int64 score, a community id and
its node's few scalars: none of the three may spill a VGPR or use scratch, and each stays within the 64 VGPRs that leave a SIMD
its eight waves (the hash tables, not registers, bound the occupancy of the LDS branches)."""
from test_code_objects_cpu import _kernels, code_objects  # noqa: F401  (the module-scoped fixture)


def test_sweep_kernels_neither_spill_nor_use_scratch(code_objects):  # noqa: F811
    for pat in (r"louvain_sweep_wave_kernel", r"louvain_sweep_block_kernel", r"louvain_sweep_global_kernel"):
        hits = _kernels(code_objects, pat)
        assert len(hits) == 1, sorted(hits)
        for name, m in hits.items():
            assert m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0 and m["scratch"] == 0, (name, m)
            assert m["vgpr"] <= 64, (name, m)


def test_stats_and_component_kernels_do_not_spill(code_objects):  # noqa: F811
    for pat in (r"louvain_stats_rows_kernel", r"louvain_stats_tot2_kernel", r"louvain_bucket_kernel", r"components_hook_kernel",
                r"components_jump_kernel"):
        for name, m in _kernels(code_objects, pat).items():
            assert m["vgpr_spill"] == 0 and m["scratch"] == 0, (name, m)
