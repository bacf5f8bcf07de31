"""CPU tier: the loss-row kernels of the GCN step (csrc/gcn_ops.hip) in the BUILT gfx950 code object.

The head backward holds U rows of `out`, of dy @ Wl and of dy in registers at once, the narrow column sum a 64-entry accumulator, and
the loss kernel and the column sum stage their rows through an LDS row tile with eight loads in flight per thread: each of them is a
stream that must not spill or touch scratch (a private segment would put a trip through memory into every row).  The fused store
epilogue of the exact GEMM (gemm_f32_kernel<..., true>) falls under test_code_objects_cpu.py's rule for every gemm_f32_kernel.
"""
import re

from test_code_objects_cpu import _kernels, code_objects  # noqa: F401  (the fixture: metadata of every kernel of the library)


def test_loss_row_kernels_use_no_scratch(code_objects):  # noqa: F811
    # mangled names: epilogue_bwd_kernel<4, true, 0> is ...epilogue_bwd_kernelILi4ELb1ELi0EE...
    head = _kernels(code_objects, r"epilogue_bwd_kernelILi4ELb1ELi0EE")
    assert len(head) == 1, sorted(head)
    nll = _kernels(code_objects, r"softmax_nll_kernel")
    assert len(nll) == 2, sorted(nll)   # the LDS-tile form and the row-walking form for a wide C
    col = _kernels(code_objects, r"narrow_colsum_kernel")
    assert len(col) == 1, sorted(col)
    for hits in (head, nll, col):
        for name, m in hits.items():
            assert m["vgpr_spill"] == 0 and m["scratch"] == 0, (name, m)


def test_fused_store_gemm_kernels_exist_and_do_not_spill(code_objects):  # noqa: F811
    # gemm_f32_kernel<WM, WN, MI, NJ, false, false, true>: the six tile shapes of the forward form
    hits = {k: v for k, v in _kernels(code_objects, r"gemm_f32_kernel").items() if re.search(r"Lb0ELb0ELb1EE", k)}
    assert len(hits) == 6, sorted(hits)
    for name, m in hits.items():
        assert m["vgpr_spill"] == 0 and m["scratch"] == 0, (name, m)
