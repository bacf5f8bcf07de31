"""CPU tier: the community detection entry points (csrc/community.hip) load, size their workspaces on the host, and refuse what
the rule's int64 arithmetic cannot hold -- N or M2 of 2^31 and more -- before any GPU work; main.py takes --community_method."""
import ctypes
import os
import sys

import pytest

from fitgnn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fitgnn_louvain_sweep_workspace_bytes", "fitgnn_louvain_bucket_rows", "fitgnn_louvain_sweep", "fitgnn_louvain_stats",
         "fitgnn_louvain_components_workspace_bytes", "fitgnn_louvain_components"]
BADARG = -1


def test_symbols_load_and_the_abi_version_stays_1():
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert L.fitgnn_abi_version() == 1


def test_workspace_queries():
    L = _lib.lib()
    ws = L.fitgnn_louvain_sweep_workspace_bytes
    assert ws(1000, 100) >= 3 * 1000 * 4                       # the three node lists
    assert ws(1000, 128) == ws(1000, 129) == ws(1000, 1000)   # no table below the third branch's cut-off ...
    assert ws(10000, 4096) == ws(10000, 100)
    assert ws(10000, 4097) - ws(10000, 4096) == 16 * 2 * 8192 * 2 * 4            # ... then 16 tables of 2 * pow2ceil(max_row) slots
    assert ws(10000, 8193) - ws(10000, 4096) == 16 * 2 * 16384 * 2 * 4
    assert ws(0, 0) > 0
    for n, max_row in ((-1, 0), (2 ** 31, 5), (2 ** 40, 5), (100, -1), (100, 101), (2 ** 31 - 1, 2 ** 30 + 1)):
        assert ws(n, max_row) == 0, (n, max_row)
    cw = L.fitgnn_louvain_components_workspace_bytes
    assert cw(1000) > 0 and cw(-1) == 0 and cw(2 ** 31) == 0


def test_sizes_of_2_pow_31_are_refused_without_touching_the_gpu():
    L = _lib.lib()
    counts = (ctypes.c_int32 * 4)()
    for n, m2 in ((2 ** 31, 10), (10, 2 ** 31), (2 ** 33, 2 ** 33), (-1, 10), (10, -1)):
        assert L.fitgnn_louvain_sweep(None, None, None, None, n, m2, None, None, None, 0, counts, 0, None, None, 0, None) == BADARG, (n, m2)
        assert L.fitgnn_louvain_stats(None, None, None, None, n, m2, None, None, None, None, None, None) == BADARG, (n, m2)
    for n in (2 ** 31, -1):
        assert L.fitgnn_louvain_bucket_rows(None, n, 0, counts, None, 0, None) == BADARG
        assert L.fitgnn_louvain_components(None, None, n, None, None, None, None, 0, None) == BADARG
    # in range but without buffers, a negative sweep index, a longest row the workspace was not sized for
    assert L.fitgnn_louvain_sweep(None, None, None, None, 10, 20, None, None, None, 0, counts, 2, None, None, 0, None) == BADARG
    assert L.fitgnn_louvain_sweep(None, None, None, None, 10, 20, None, None, None, -1, counts, 2, None, None, 0, None) == BADARG
    assert L.fitgnn_louvain_sweep(None, None, None, None, 10, 20, None, None, None, 0, None, 2, None, None, 0, None) == BADARG
    assert L.fitgnn_louvain_bucket_rows(None, 10, 11, counts, None, 0, None) == BADARG
    assert L.fitgnn_louvain_components(None, None, 10, None, None, None, None, 0, None) == BADARG
    # nothing to do
    assert L.fitgnn_louvain_sweep(None, None, None, None, 0, 0, None, None, None, 0, counts, 0, None, None, 0, None) == 0
    assert L.fitgnn_louvain_bucket_rows(None, 0, 0, counts, None, 0, None) == 0 and list(counts) == [0, 0, 0, 0]
    assert L.fitgnn_louvain_components(None, None, 0, None, None, None, None, 0, None) == 0


def test_python_layer_refuses_before_any_gpu_work():
    from fitgnn_amd import community, pipeline

    with pytest.raises(_lib.FitgnnError, match="2\\^31"):
        community.modularity_communities([[0], [1]], 2 ** 31)
    with pytest.raises(_lib.FitgnnError, match="no CPU path"):
        community.modularity_communities([[0], [1]], 2, device="cpu")
    with pytest.raises(ValueError, match="unknown method"):
        pipeline.detect_communities([[0], [1]], 2, method="leiden")


def test_modularity_is_exact_on_the_host():
    from fitgnn_amd import community

    ei = [[0, 1, 2, 3, 4, 5, 2], [1, 2, 0, 4, 5, 3, 3]]                       # two triangles and a bridge: M2 = 14
    assert community.modularity(ei, 6, [0, 0, 0, 1, 1, 1]) == (14 * 12 - 2 * 49) / (14 * 14)
    assert community.modularity(ei, 6, [5, 5, 5, 5, 5, 5]) == 0.0
    assert community.modularity([[0, 0], [0, 0]], 3, [0, 1, 2]) == 0.0           # self-loops only: no edge


def test_main_takes_community_method():
    sys.path.insert(0, os.path.join(ROOT, "fit-gnn_amd"))
    import main as cli

    p = cli.build_parser()
    assert p.parse_args(["--output_dir", "x"]).community_method == "label_propagation"
    assert p.parse_args(["--output_dir", "x", "--community_method", "modularity"]).community_method == "modularity"
    with pytest.raises(SystemExit):
        p.parse_args(["--output_dir", "x", "--community_method", "leiden"])
