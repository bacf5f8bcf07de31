"""CPU tier of the in-order whole-component matching coarsening (fitgnn_match_small, coarsening.coarsen_in_order) and of the
graph-level matching methods: the ABI's symbols, size queries and argument checks, the np.random bookkeeping of DrawPool, the
kernel's code objects, and GraphSet's refusals -- all without a GPU."""
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from fitgnn_amd import _lib, coarsening, graph_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fit-gnn_amd", "lib", "libfitgnn_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"


def test_match_small_symbols_exported_and_sized_without_a_gpu():
    L = _lib.lib()
    for n in ("fitgnn_match_small_lds_bytes", "fitgnn_match_small"):
        assert hasattr(L, n) and n in _lib.SIGNATURES, n
    he, jc = _lib.MATCH_HEAVY_EDGE, _lib.MATCH_ALGEBRAIC_JC
    full = L.fitgnn_match_small_lds_bytes(he, 128, 1024, 0)
    assert 0 < full <= _lib.MATCH_SMALL_LDS_BUDGET
    assert 0 < L.fitgnn_match_small_lds_bytes(he, 29, 64, 0) < full // 8     # a molecule's workgroup is small
    assert L.fitgnn_match_small_lds_bytes(jc, 20, 40, 10) == L.fitgnn_match_small_lds_bytes(jc, 128, 1024, 12) <= _lib.MATCH_SMALL_LDS_BUDGET
    assert L.fitgnn_match_small_lds_bytes(he, 129, 64, 0) == 0               # over the node cap
    assert L.fitgnn_match_small_lds_bytes(he, 64, 1025, 0) == 0              # over the entry cap
    assert L.fitgnn_match_small_lds_bytes(jc, 64, 64, 13) == 0               # K over FITGNN_MATCH_SMALL_MAX_K
    assert L.fitgnn_match_small_lds_bytes(7, 64, 64, 10) == 0                # unknown method


def _call(method=_lib.MATCH_HEAVY_EDGE, c0=0, c1=1, r=0.5, K=10, levels=10, mlr=0.99, sqrt_n=None, cap_n=16, cap_z=32, progress=None):
    L = _lib.lib()
    return L.fitgnn_match_small(method, None, None, None, None, c0, c1, r, K, levels, mlr, None, 0, sqrt_n, cap_n, cap_z,
                                None, None, None, None, None, None, None, None, progress, None)


def test_match_small_argument_errors_return_before_device_work():
    assert _call(method=5) == -1
    assert _call(c0=2, c1=1) == -1
    assert _call(r=1.5) == -1 and _call(r=float("nan")) == -1 and _call(mlr=-0.1) == -1
    assert _call(levels=-1) == -1
    assert _call(cap_n=129) == -1 and _call(cap_z=2048) == -1
    assert _call(method=_lib.MATCH_ALGEBRAIC_JC) == -1                       # no sqrt table / progress word
    assert _call(method=_lib.MATCH_ALGEBRAIC_JC, K=13) == -1
    assert _call() == -1                                                     # NULL graph / outputs
    assert _call(c0=3, c1=3) == 0                                            # nothing to do (heavy_edge): no device work


@pytest.mark.parametrize("chunk", [1, 7, 64, 1 << 12])
def test_draw_pool_leaves_the_state_of_one_straight_randn(chunk):
    """DrawPool over many forced chunk boundaries: the draws it hands out are the stream's, in order, and after sync() the
    global state is the one a single randn(total) leaves -- also across a rebase mid-way (a fallback coarsen() call)."""
    rng = np.random.default_rng(3)
    np.random.seed(11)
    pool = coarsening.DrawPool(chunk)
    got, total = [], 0
    for step in range(40):
        need = int(rng.integers(1, 30))
        avail = pool.ensure(need)
        assert avail.size >= need
        k = int(rng.integers(0, need + 1))
        got.append(avail[:k].copy())
        pool.consume(k)
        total += k
        if step == 20:                   # a fallback: the global state must sit at exactly `total`
            pool.sync()
            got.append(np.random.randn(5))
            total += 5
            pool.rebase()
    pool.sync()
    after = np.random.get_state()
    np.random.seed(11)
    want = np.random.randn(total)
    ref = np.random.get_state()
    assert np.array_equal(np.concatenate(got), want)
    assert after[0] == ref[0] and np.array_equal(after[1], ref[1]) and after[2:] == ref[2:]
    with pytest.raises(ValueError):
        pool.consume(1)                  # nothing drawn ahead after sync()


@pytest.fixture(scope="module")
def code_objects(tmp_path_factory):
    if not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))):
        pytest.skip("ROCm's llvm tools are not installed")
    d = tmp_path_factory.mktemp("co")
    shutil.copy(LIB, d / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=d, check=True, stdout=subprocess.DEVNULL)
    files = sorted(glob.glob(str(d / "lib.so.*gfx950*")))
    assert files, "no gfx950 code object in libfitgnn_hip.so"
    meta = {}
    for f in files:
        txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f], check=True, stdout=subprocess.PIPE, text=True).stdout
        for blk in re.split(r"\n\s*- \.agpr_count:|\n\s*- \.args:", txt):
            name = re.search(r"\.name:\s+(\S+)", blk)
            if not name:
                continue
            vals = {k: int(m.group(1)) for k in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")
                    for m in [re.search(r"\.%s:\s+(\d+)" % k, blk)] if m}
            meta[name.group(1)] = vals
    return meta


def test_match_small_kernels_neither_spill_nor_use_scratch(code_objects):
    hits = {k: v for k, v in code_objects.items() if "match_small_kernel" in k}
    assert len(hits) == 2, sorted(hits)                                      # heavy_edge and algebraic_JC instantiations
    for name, m in hits.items():
        assert m.get("vgpr_spill_count") == 0 and m.get("sgpr_spill_count") == 0, (name, m)
        assert m.get("private_segment_fixed_size") == 0, (name, m)


def _two_graphs(connected_second):
    # graph 0: triangle; graph 1: a path of 3 (or a pair plus an isolated node)
    e = [(0, 1), (1, 2), (0, 2), (3, 4)] + ([(4, 5)] if connected_second else [])
    e = np.array(e).T
    ei = np.concatenate([e, e[::-1]], 1)
    return dict(node_ptr=np.array([0, 3, 6]), edge_index=ei, x=np.zeros((6, 2), np.float32), y=np.zeros((2, 1), np.float32))


@pytest.mark.parametrize("method", graph_data.GRAPH_MATCHING_METHODS)
def test_graph_set_refuses_a_disconnected_graph_for_the_matching_methods(method):
    with pytest.raises(ValueError, match="graph 1 is not"):
        graph_data.GraphSet(_two_graphs(False), method=method)


@pytest.mark.parametrize("method", ["affinity_GS", "variation_cliques", "kron"])
def test_graph_set_refuses_methods_outside_the_graph_level_set(method):
    with pytest.raises(NotImplementedError):
        graph_data.GraphSet(_two_graphs(True), method=method)


def test_coarsen_in_order_refuses_what_it_does_not_implement():
    W = sp.csr_matrix(np.ones((3, 3)) - np.eye(3))
    for m in ("affinity_GS", "variation_edges", "variation_neighborhoods"):
        with pytest.raises(NotImplementedError, match="heavy_edge, algebraic_JC"):
            coarsening.coarsen_in_order(W, [0, 3], method=m)


def test_graph_method_of_the_cli():
    import argparse

    from fitgnn_amd import pipeline
    for m in ("variation_neighborhoods", "heavy_edge", "algebraic_JC", "variation_edges"):
        assert pipeline.graph_method(argparse.Namespace(coarsening_method=m)) == m
    with pytest.raises(NotImplementedError, match="affinity_GS"):
        pipeline.graph_method(argparse.Namespace(coarsening_method="affinity_GS"))
