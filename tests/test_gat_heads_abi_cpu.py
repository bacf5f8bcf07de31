"""CPU tier: the multi-head attention entry points (csrc/gat_heads.hip) load, and every refusal include/fitgnn_hip.h lists for them
is decided on the host before any launch: FITGNN_E_BADARG with no GPU present.

The size refusals are told apart from the NULL refusal by calls with n = 0: valid sizes return 0 there (nothing to do, pointers not
looked at), a bad size still returns FITGNN_E_BADARG.  The NULL refusals use n = 1 with every other pointer set (a host buffer: a
refused call never reaches a launch)."""
import ctypes

import pytest

from fitgnn_amd import _lib

BAD = -1   # FITGNN_E_BADARG
NAMES = ["fitgnn_gat_heads_scores_f32", "fitgnn_gat_heads_edge_softmax_f32", "fitgnn_gat_heads_aggregate_f32",
         "fitgnn_gat_heads_sddmm_f32", "fitgnn_gat_heads_softmax_bwd_f32"]
BIG = 1 << 31


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


@pytest.fixture(scope="module")
def buf():
    return ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)


def _calls(L, P, n=0, nnz=0, heads=2, C=4, ld=8):
    """The five entry points with one set of sizes and every pointer = P -> their return codes, in NAMES' order."""
    return [L.fitgnn_gat_heads_scores_f32(P, ld, n, heads, C, P, P, P, P, None),
            L.fitgnn_gat_heads_edge_softmax_f32(P, P, P, P, 0.2, n, nnz, heads, P, None),
            L.fitgnn_gat_heads_aggregate_f32(P, P, P, P, ld, P, ld, n, nnz, heads, C, P, None),
            L.fitgnn_gat_heads_sddmm_f32(P, P, P, ld, P, ld, n, nnz, heads, C, P, None),
            L.fitgnn_gat_heads_softmax_bwd_f32(P, P, P, P, P, P, 0.2, n, nnz, heads, P, P, None)]


def test_symbols_load_with_their_signatures(L):
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1]


def test_nothing_to_do_returns_zero_without_looking_at_the_pointers(L):
    assert _calls(L, None) == [0] * 5
    assert _calls(L, None, heads=1, C=1, ld=1) == [0] * 5
    assert _calls(L, None, heads=16, C=64, ld=1024) == [0] * 5


def test_size_refusals(L):
    """heads < 1, C < 1, negative sizes, ld < W, and 32-bit index overflow -- all with n = 0 or less, where valid sizes return 0."""
    assert _calls(L, None, heads=0) == [BAD] * 5
    assert _calls(L, None, heads=-3) == [BAD] * 5
    assert _calls(L, None, n=-1) == [BAD] * 5
    has_C = [0, 2, 3]          # scores, aggregate, sddmm take C and leading dimensions
    has_nnz = [1, 2, 3, 4]
    for C in (0, -1):
        got = _calls(L, None, C=C, ld=8)
        assert [got[i] for i in has_C] == [BAD] * 3, C
    got = _calls(L, None, heads=2, C=4, ld=7)     # ld < W = 8
    assert [got[i] for i in has_C] == [BAD] * 3
    got = _calls(L, None, heads=3, C=5, ld=14)    # W = 15
    assert [got[i] for i in has_C] == [BAD] * 3
    assert _calls(L, None, heads=3, C=5, ld=15) == [0] * 5
    got = _calls(L, None, nnz=-1)
    assert [got[i] for i in has_nnz] == [BAD] * 4
    # nnz * heads >= 2^31 (entry-major [nnz, heads] arrays are indexed with 32 bits)
    got = _calls(L, None, nnz=BIG // 2, heads=2)
    assert [got[i] for i in has_nnz] == [BAD] * 4
    got = _calls(L, None, nnz=BIG // 2 - 1, heads=2)
    assert [got[i] for i in has_nnz] == [0] * 4
    got = _calls(L, None, nnz=BIG, heads=1, C=4, ld=4)
    assert [got[i] for i in has_nnz] == [BAD] * 4
    # heads * C >= 2^31
    got = _calls(L, None, heads=1 << 16, C=1 << 15, ld=1 << 40)
    assert [got[i] for i in has_C] == [BAD] * 3


def test_node_index_overflow_is_refused(L, buf):
    """n * heads >= 2^31 needs n > 0: every pointer is set, so only the size check can refuse."""
    assert _calls(L, buf, n=BIG // 2, nnz=4, heads=2, C=4, ld=8) == [BAD] * 5
    assert _calls(L, buf, n=(1 << 31) - 1, nnz=4, heads=2, C=4, ld=8) == [BAD] * 5


def test_null_pointers_are_refused(L, buf):
    """n = 1, nnz = 1, valid sizes: each required pointer NULL in turn, the others set.  (bias may be NULL: not among them.)"""
    P = buf

    def each(fn, args, ptr_positions):
        for i in ptr_positions:
            a = list(args)
            a[i] = None
            assert fn(*a) == BAD, (fn.__name__, i)

    each(L.fitgnn_gat_heads_scores_f32, [P, 8, 1, 2, 4, P, P, P, P, None], [0, 5, 6, 7, 8])
    each(L.fitgnn_gat_heads_edge_softmax_f32, [P, P, P, P, 0.2, 1, 1, 2, P, None], [0, 1, 2, 3, 8])
    each(L.fitgnn_gat_heads_aggregate_f32, [P, P, P, P, 8, P, 8, 1, 1, 2, 4, None, None], [0, 1, 2, 3, 5])
    each(L.fitgnn_gat_heads_sddmm_f32, [P, P, P, 8, P, 8, 1, 1, 2, 4, P, None], [0, 1, 2, 4, 10])
    each(L.fitgnn_gat_heads_softmax_bwd_f32, [P, P, P, P, P, P, 0.2, 1, 1, 2, P, P, None], [0, 1, 2, 3, 4, 5, 10, 11])
