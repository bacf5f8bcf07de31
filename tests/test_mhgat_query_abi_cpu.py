"""CPU tier: the multi-head attention query entry points (csrc/query.hip: fitgnn_mhgat_query_gather_f32, fitgnn_mhgat_query_tail_f32)
load with their signatures, and every refusal include/fitgnn_hip.h lists for them is decided on the host before any launch:
FITGNN_E_BADARG / FITGNN_E_ALIGN with no GPU present (the convention of tests/test_gat_heads_abi_cpu.py: pointers are NULL or a host
buffer, a refused call never reaches a launch)."""
import ctypes

import pytest

from fitgnn_amd import _lib

BAD, ALIGN = -1, -3   # FITGNN_E_BADARG, FITGNN_E_ALIGN
GATHER, TAIL = "fitgnn_mhgat_query_gather_f32", "fitgnn_mhgat_query_tail_f32"


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


@pytest.fixture(scope="module")
def buf():
    return ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)


def _gather(L, P=None, heads=4, H=64, Q=4, ldt=None, ldg=None):
    ldt = H if ldt is None else ldt
    ldg = heads * H if ldg is None else ldg
    #                                        rowptr col T  ldt xrow a_s a_d heads b0  sl0  U_s U_d sl1 rows Q  H  G  ldg  stream
    return L.fitgnn_mhgat_query_gather_f32(P, P, P, ldt, None, P, P, heads, None, 0.2, P, P, 0.2, P, Q, H, P, ldg, None)


def _tail(L, P=None, heads=4, H=64, H2=64, C=5, Q=4, ldg=None, ldo=None):
    ldg = heads * H if ldg is None else ldg
    #                                     G  ldg  Q  W1 b1   Wl bl    H  H2  heads  C  out ldo              log_softmax stream
    return L.fitgnn_mhgat_query_tail_f32(P, ldg, Q, P, None, P, None, H, H2, heads, C, P, C if ldo is None else ldo, 1, None)


def test_symbols_load_with_their_signatures(L):
    for name in (GATHER, TAIL):
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
        assert getattr(L, name).argtypes == _lib.SIGNATURES[name][1]
        assert getattr(L, name).restype == _lib.SIGNATURES[name][0]
    assert len(_lib.SIGNATURES[GATHER][1]) == 19 and len(_lib.SIGNATURES[TAIL][1]) == 15
    lds = L.fitgnn_mhgat_query_tail_lds_bytes
    assert lds.argtypes == _lib.SIGNATURES["fitgnn_mhgat_query_tail_lds_bytes"][1] and lds.restype == ctypes.c_size_t


def test_tail_lds_bytes(L):
    """The GCN tail's LDS plus one staged 16 x 36 tile of G per head past the first; 0 for sizes the launcher refuses."""
    lds, gcn = L.fitgnn_mhgat_query_tail_lds_bytes, L.fitgnn_gcn_query_tail_lds_bytes
    for H2, C, heads in ((32, 3, 2), (64, 7, 4), (80, 5, 5), (512, 47, 8)):
        assert lds(H2, C, heads) == gcn(H2, C) + (heads - 1) * 16 * 36 * 4
    assert lds(512, 48, 8) <= 160 * 1024
    assert lds(64, 7, 1) == 0 and lds(64, 7, 9) == 0 and lds(0, 7, 4) == 0 and lds(64, 0, 4) == 0


def test_nothing_to_do_returns_zero_without_looking_at_the_pointers(L):
    for heads, H in ((2, 8), (4, 64), (8, 256), (5, 260), (2, 512), (8, 512)):
        assert _gather(L, heads=heads, H=H, Q=0) == 0, (heads, H)
    assert _gather(L, Q=0, ldt=68, ldg=264) == 0
    for heads, H, H2 in ((2, 8, 32), (4, 64, 64), (5, 260, 80), (8, 512, 512)):
        assert _tail(L, heads=heads, H=H, H2=H2, Q=0) == 0, (heads, H, H2)


def test_gather_size_refusals(L):
    assert _gather(L, heads=1, H=64) == BAD
    assert _gather(L, heads=9, H=72) == BAD
    assert _gather(L, heads=0, H=64) == BAD
    assert _gather(L, heads=2, H=12) == BAD        # C0 = 6: a float4 would straddle two heads
    assert _gather(L, heads=3, H=64) == BAD        # H % heads
    assert _gather(L, heads=2, H=4) == BAD         # H < 8
    assert _gather(L, heads=2, H=516) == BAD       # H > 512
    assert _gather(L, heads=4, H=516) == BAD
    assert _gather(L, heads=4, H=64, ldg=4 * 64 - 4) == BAD    # ldg < heads H
    assert _gather(L, heads=4, H=64, ldg=64) == BAD            # (the single-head kernel's ldg)
    assert _gather(L, heads=4, H=64, ldt=60) == BAD
    assert _gather(L, Q=-1) == BAD
    assert _gather(L, ldt=66) == ALIGN and _gather(L, ldg=258) == ALIGN
    # the refusals above hold with Q = 0 as well, where valid sizes return 0: they are size checks, not the NULL check
    assert _gather(L, heads=1, H=64, Q=0) == BAD and _gather(L, heads=2, H=12, Q=0) == BAD and _gather(L, heads=4, ldg=252, Q=0) == BAD


def test_tail_size_refusals(L):
    assert _tail(L, heads=8, H=64, H2=64) == BAD      # C1 = 8: not a multiple of the 16-column MFMA block
    assert _tail(L, heads=4, H=64, H2=96) == BAD      # C1 = 24
    assert _tail(L, heads=3, H=48, H2=64) == BAD      # H2 % heads
    assert _tail(L, heads=1, H=64, H2=64) == BAD and _tail(L, heads=9, H=72, H2=144) == BAD
    assert _tail(L, heads=2, H=6, H2=32) == BAD       # H % 4
    assert _tail(L, C=0) == BAD and _tail(L, Q=-1) == BAD
    assert _tail(L, ldg=4 * 64 - 4) == BAD and _tail(L, ldo=4) == BAD
    assert _tail(L, ldg=258) == ALIGN
    assert _tail(L, heads=2, H=8, H2=4096, C=48) == BAD    # z of a tile does not fit LDS
    assert _tail(L, heads=8, H=64, H2=64, Q=0) == BAD


def test_null_pointers_are_refused(L, buf):
    """Q > 0, valid sizes: each required pointer NULL in turn, the others set (xrow, b0, b1, bl may be NULL: not among them)."""
    P = buf
    good = [P, P, P, 64, None, P, P, 4, None, 0.2, P, P, 0.2, P, 1, 64, P, 256, None]
    for i in (0, 1, 2, 5, 6, 10, 11, 13, 16):
        a = list(good)
        a[i] = None
        assert L.fitgnn_mhgat_query_gather_f32(*a) == BAD, i
    good = [P, 256, 1, P, None, P, None, 64, 64, 4, 5, P, 5, 1, None]
    for i in (0, 3, 5, 11):
        a = list(good)
        a[i] = None
        assert L.fitgnn_mhgat_query_tail_f32(*a) == BAD, i


def test_misaligned_pointers_are_refused_on_the_host(L):
    """T, G, U_src, U_dst (gather) and G, W1, Wl, out (tail) 4 bytes past a 16-byte boundary: FITGNN_E_ALIGN before any launch."""
    raw = (ctypes.c_float * 72)()
    base = (ctypes.addressof(raw) + 15) & ~15
    P, off = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)
    good = [P, P, P, 64, None, P, P, 4, None, 0.2, P, P, 0.2, P, 1, 64, P, 256, None]
    for i in (2, 10, 11, 16):
        a = list(good)
        a[i] = off
        assert L.fitgnn_mhgat_query_gather_f32(*a) == ALIGN, i
    good = [P, 256, 1, P, None, P, None, 64, 64, 4, 5, P, 5, 1, None]
    for i in (0, 3, 5, 11):
        a = list(good)
        a[i] = off
        assert L.fitgnn_mhgat_query_tail_f32(*a) == ALIGN, i
