"""CPU tier: _lib.call, the one checked path from Python into the library.  Every case returns inside the library's argument
checks (or before the library is entered), so nothing here touches a device."""
import ast
import ctypes
import glob
import os
import re

import pytest
import torch

from fitgnn_amd import _lib

PKG = os.path.dirname(os.path.abspath(_lib.__file__))

# fitgnn_head_rows_f32(out, ldo, rows, n_rows, Wl, bl, C, H, y, ldy, out_compact, stream): with n_rows = 0 it returns 0 before it
# looks at a pointer, and it never looks at out_compact's range
HEAD = "fitgnn_head_rows_f32"
HEAD_OK = (None, 512, None, 0, None, None, 3, 512, None, 3, 0, None)
# fitgnn_epilogue_bwd_f32(dOut, out, dZ, n_rows, H, epilogue u32, p, seed u64, mask, db, work, work_bytes size_t, stream)
EPI = "fitgnn_epilogue_bwd_f32"
EPI_OK = (None, None, None, 0, 0, 0, 0.0, 0, None, None, None, 0, None)


def _with(args, i, v):
    return args[:i] + (v,) + args[i + 1:]


def test_bad_argument_carries_the_symbol_name_and_the_library_text():
    assert _lib.call(HEAD, *HEAD_OK) is None
    with pytest.raises(_lib.FitgnnError) as e:
        _lib.call(HEAD, *_with(HEAD_OK, 3, -1))
    bad = _lib.lib().fitgnn_error_string(-1).decode()
    assert "bad argument" in bad and HEAD in str(e.value) and bad in str(e.value)


@pytest.mark.parametrize("pos", [i for i, t in enumerate(_lib.SIGNATURES[HEAD][1]) if t is _lib.ptr])
def test_host_tensor_is_refused_before_the_library_is_entered(pos):
    # the library would return 0 for these arguments whatever the pointer: a return without an exception is the miss
    with pytest.raises(_lib.FitgnnError, match="no CPU fallback"):
        _lib.call(HEAD, *_with(HEAD_OK, pos, torch.zeros(4)))
    with pytest.raises(_lib.FitgnnError, match="no CPU fallback"):
        _lib.call(HEAD, *_with(HEAD_OK, pos, torch.nn.Parameter(torch.zeros(4))))


def test_integer_range():
    sig = _lib.SIGNATURES
    assert sig[HEAD][1][3] is _lib.c_i32 and sig[HEAD][1][10] is _lib.c_i32 and sig[HEAD][1][9] is _lib.c_i64
    assert (sig[EPI][1][5], sig[EPI][1][7], sig[EPI][1][11]) == (_lib.c_u32, _lib.c_u64, _lib.c_size)
    for v in (2 ** 31, 2 ** 32 + 5, -2 ** 31 - 1):          # ctypes alone would pass these on as -2^31, 5 and 2^31 - 1
        with pytest.raises(_lib.FitgnnError, match=r"%s: argument 3 = %d\b" % (HEAD, v)):
            _lib.call(HEAD, *_with(HEAD_OK, 3, v))
    assert _lib.call(EPI, *EPI_OK) is None
    for pos in (5, 7, 11):
        with pytest.raises(_lib.FitgnnError, match=r"%s: argument %d = -1\b" % (EPI, pos)):
            _lib.call(EPI, *_with(EPI_OK, pos, -1))
    for pos, v in ((5, 2 ** 32), (7, 2 ** 64), (11, 2 ** 64)):
        with pytest.raises(_lib.FitgnnError, match="argument %d" % pos):
            _lib.call(EPI, *_with(EPI_OK, pos, v))
    # the ends of each range are taken: the library returns 0 for them
    for v in (2 ** 31 - 1, -2 ** 31, True, False):
        assert _lib.call(HEAD, *_with(HEAD_OK, 10, v)) is None
    assert _lib.call(HEAD, *_with(HEAD_OK, 9, 2 ** 63 - 1)) is None
    for pos, v in ((5, 2 ** 32 - 1), (7, 2 ** 64 - 1), (11, 2 ** 64 - 1)):
        assert _lib.call(EPI, *_with(EPI_OK, pos, v)) is None
    with pytest.raises(_lib.FitgnnError, match="argument 9"):
        _lib.call(HEAD, *_with(HEAD_OK, 9, 2 ** 63))


def test_wrong_argument_count():
    for args in (HEAD_OK[:-1], HEAD_OK + (None,), ()):
        with pytest.raises(_lib.FitgnnError, match=HEAD):
            _lib.call(HEAD, *args)


def test_unknown_name_is_a_fitgnn_error():
    with pytest.raises(_lib.FitgnnError, match="fitgnn_no_such_thing"):
        _lib.call("fitgnn_no_such_thing", None)


def _cpu_wrapper_cases():
    from fitgnn_amd import ops, torch_ops
    f = lambda *s: torch.zeros(*s)                                    # noqa: E731
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)                # noqa: E731
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64)                # noqa: E731
    rp, col, val, T, rows = i32(5), i32(8), f(8), f(4, 16), i64(2)
    seg, prow, pptr, none = i64(1, 2), i64(2), i64(2), i64(0)
    w, b = f(16, 16), f(16)
    return {
        "gemm_exact": lambda: ops.gemm_exact(f(8, 16), f(8, 16), "nt"),
        "gemm_exact_epi": lambda: ops.gemm_exact_epi(f(8, 16), f(8, 16), None, None, 0),
        "spmm_raw": lambda: ops.spmm_raw(rp, col, val, i32(1, 4), T, 4),
        "spmm_blocks_raw": lambda: ops.spmm_blocks_raw(rp, col, val, i32(1, 8), i32(1), T, f(4, 16)),
        "gcn_query_gather": lambda: ops.gcn_query_gather(rp, col, val, T, rows),
        "gcn_query_tail": lambda: ops.gcn_query_tail(T, w, b, w, b),
        "gcn_graph_query_hops": lambda: ops.gcn_graph_query_hops(rp, col, val, T, seg, prow, pptr, 4),
        "gcn_graph_query_hops, nothing pooled": lambda: ops.gcn_graph_query_hops(rp, col, val, T, seg, none, pptr, 4),
        "gcn_graph_query_tail": lambda: ops.gcn_graph_query_tail(T, pptr, w, b, w, b),
        "gat_query_gather": lambda: ops.gat_query_gather(rp, col, T, f(4), f(4), b, b, rows),
        "gat_graph_query_hops": lambda: ops.gat_graph_query_hops(rp, col, T, f(4), f(4), b, b, seg, prow, pptr, 4),
        "gat_graph_query_hops, nothing pooled": lambda: ops.gat_graph_query_hops(rp, col, T, f(4), f(4), b, b, seg, none, pptr, 4),
        "sage_query_gather": lambda: ops.sage_query_gather(rp, col, val, T, rows),
        "sage_graph_query_hops": lambda: ops.sage_graph_query_hops(rp, col, val, T, seg, prow, pptr, 4),
        "sage_graph_query_hops, nothing pooled": lambda: ops.sage_graph_query_hops(rp, col, val, T, seg, none, pptr, 4),
        "gin_query_hops": lambda: ops.gin_query_hops(rp, col, val, T, f(1), w, b, f(1), rows),
        "gin_query_tail": lambda: ops.gin_query_tail(T, w, b, w, b, w, b),
        "gin_graph_query_hops": lambda: ops.gin_graph_query_hops(rp, col, val, T, f(1), w, b, f(1), seg, prow, pptr, 4),
        "gin_graph_query_hops, nothing pooled": lambda: ops.gin_graph_query_hops(rp, col, val, T, f(1), w, b, f(1), seg, none, pptr, 4),
        "gin_graph_query_tail": lambda: ops.gin_graph_query_tail(T, pptr, w, b, w, b, w, b),
        "segment_sum": lambda: ops.segment_sum(i32(3), i32(4), T, 2),
        "torch_ops._gcn_norm_csr": lambda: torch_ops._gcn_norm_csr(rp, col, val),
    }


def test_wrappers_refuse_cpu_tensors_with_the_package_error():
    """Every operand on the CPU, the usual mistake: the wrapper raises FitgnnError, not torch's error about the device that its
    output or its stream is taken from -- also where nothing is pooled and the wrapper returns without a launch."""
    for name, fn in _cpu_wrapper_cases().items():
        try:
            fn()
        except _lib.FitgnnError as e:
            assert "no CPU fallback" in str(e), name
        except Exception as e:
            pytest.fail("%s: %s: %s" % (name, type(e).__name__, e))
        else:
            pytest.fail(name + " returned")


def test_what_is_no_tensor_passes_through_to_ctypes():
    counts = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    assert _lib.call("fitgnn_louvain_bucket_rows", None, 0, 0, counts, None, 0, None) is None
    assert list(counts) == [0, 0, 0, 0]
    # a byref, a c_void_p and an int address in pointer positions
    shape, nchunks, main_rows = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int64(-1)
    _lib.call("fitgnn_gemm_exact_plan", 4096, 64, 64, 0, 0, ctypes.byref(shape), ctypes.c_void_p(ctypes.addressof(nchunks)),
              ctypes.addressof(main_rows))
    assert nchunks.value >= 1 and main_rows.value >= 0 and shape.value >= 0


def test_the_package_calls_the_library_through_call_alone():
    pair = "torch.cuda.Event(enable_timing=True), torch.cuda.Event"
    files = sorted(glob.glob(os.path.join(PKG, "*.py")))
    assert len(files) > 10
    for path in files:
        name = os.path.basename(path)
        if name == "_lib.py":
            continue
        text = open(path).read()
        assert not re.search(r"\bdptr\(", text), name
        assert not re.search(r"\bcheck\(", text), name
        if pair not in text:
            continue
        assert name == "ops.py", name
        homes = {n.name: (n.lineno, n.end_lineno) for n in ast.parse(text).body if isinstance(n, (ast.ClassDef, ast.FunctionDef))}
        for i, line in enumerate(text.split("\n"), 1):
            if pair in line:
                assert any(homes[h][0] <= i <= homes[h][1] for h in ("_timed", "_gemm_events")), (name, i)
