"""CPU tests of the argument checks of DynamicGraph.common_neighbors and
DynamicGraph.temporal_degree (dynamic_graph.check_common_neighbors_args,
check_temporal_degree_args) and of NeighborOverlap's constructor: every TypeError and ValueError is
raised before anything is allocated or launched and needs no device; the two native entries reject
a null graph and out-of-range bounds with a status code; the Python limit is the header's."""
import os
import re

import numpy as np
import pytest
import torch

import gnnflow_amd
from gnnflow_amd import CommonNeighbors, NeighborOverlap, _capi
from gnnflow_amd.dynamic_graph import (CN_MAX_HISTORY, DynamicGraph, check_common_neighbors_args,
                                       check_temporal_degree_args)
from tests import common_neighbors_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(N=4, **over):
    a = dict(src=torch.zeros(N, dtype=torch.int64), dst=torch.ones(N, dtype=torch.int64),
             ts=torch.zeros(N, dtype=torch.float32), since=None, max_history=64, max_common=32)
    a.update(over)
    return a


def test_names_are_exported():
    assert {"CommonNeighbors", "NeighborOverlap"} <= set(gnnflow_amd.__all__)
    assert gnnflow_amd.CommonNeighbors is CommonNeighbors
    assert gnnflow_amd.NeighborOverlap is NeighborOverlap
    assert CommonNeighbors._fields == ("n_src", "n_dst", "u_src", "u_dst", "common", "nodes",
                                       "cnt_src", "cnt_dst")


def test_the_limit_is_the_headers():
    text = open(os.path.join(ROOT, "include", "gnnflow_hip.h")).read()
    assert int(re.search(r"#define GF_CN_MAX_HISTORY (\d+)", text).group(1)) == CN_MAX_HISTORY
    assert CN_MAX_HISTORY == R.MAX_HISTORY == 512


def test_good_arguments_return_rows_and_bounds():
    assert check_common_neighbors_args(**_args()) == (4, 64, 32)
    assert check_common_neighbors_args(**_args(N=0)) == (0, 64, 32)
    assert check_common_neighbors_args(**_args(since=40.0)) == (4, 64, 32)
    assert check_common_neighbors_args(**_args(since=float("nan"))) == (4, 64, 32)
    assert check_common_neighbors_args(**_args(since=torch.zeros(4))) == (4, 64, 32)
    a = _args()
    assert check_common_neighbors_args(a["src"], a["dst"], a["ts"]) == (4, 64, 32)


@pytest.mark.parametrize("H", [1, 512])
@pytest.mark.parametrize("K", [0, 1, 512])
def test_bounds_that_are_legal(H, K):
    assert check_common_neighbors_args(**_args(max_history=H, max_common=K)) == (4, H, K)


@pytest.mark.parametrize("H", [0, 513, -1])
def test_max_history_out_of_range(H):
    with pytest.raises(ValueError, match="max_history"):
        check_common_neighbors_args(**_args(max_history=H))


@pytest.mark.parametrize("K", [513, -1])
def test_max_common_out_of_range(K):
    with pytest.raises(ValueError, match="max_common"):
        check_common_neighbors_args(**_args(max_common=K))


@pytest.mark.parametrize("name", ["max_history", "max_common"])
@pytest.mark.parametrize("bad", [True, False, 1.0, None, "3", np.float32(2)])
def test_bounds_must_be_ints(name, bad):
    with pytest.raises(TypeError, match=name):
        check_common_neighbors_args(**_args(**{name: bad}))


@pytest.mark.parametrize("name", ["src", "dst", "ts"])
def test_not_a_tensor(name):
    with pytest.raises(TypeError, match=name):
        check_common_neighbors_args(**_args(**{name: np.zeros(4)}))
    with pytest.raises(TypeError, match=name):
        check_common_neighbors_args(**_args(**{name: [0, 1, 2, 3]}))


@pytest.mark.parametrize("name,bad", [("src", torch.int32), ("src", torch.float32),
                                      ("dst", torch.int32), ("dst", torch.float32),
                                      ("ts", torch.float64), ("ts", torch.int64),
                                      ("since", torch.float64), ("since", torch.int64)])
def test_wrong_dtype(name, bad):
    with pytest.raises(TypeError, match=name):
        check_common_neighbors_args(**_args(**{name: torch.zeros(4, dtype=bad)}))


@pytest.mark.parametrize("bad", [True, "3", [0.0] * 4, np.zeros(4, np.float32), (1.0,)])
def test_since_must_be_none_a_float_or_a_tensor(bad):
    with pytest.raises(TypeError, match="since"):
        check_common_neighbors_args(**_args(since=bad))
    with pytest.raises(TypeError, match="since"):
        check_temporal_degree_args(torch.zeros(4, dtype=torch.int64), torch.zeros(4), bad)


@pytest.mark.parametrize("name", ["src", "dst", "ts", "since"])
def test_not_one_dimensional(name):
    good = _args(since=torch.zeros(4))[name]
    with pytest.raises(ValueError, match=name):
        check_common_neighbors_args(**_args(**{name: good.reshape(-1, 1)}))
    with pytest.raises(ValueError, match=name):
        check_common_neighbors_args(**_args(**{name: good[0]}))


@pytest.mark.parametrize("name,dtype", [("dst", torch.int64), ("ts", torch.float32),
                                        ("since", torch.float32)])
def test_lengths_differ(name, dtype):
    with pytest.raises(ValueError, match=name):
        check_common_neighbors_args(**_args(**{name: torch.zeros(3, dtype=dtype)}))


def test_too_many_rows():
    # 2^31 rows without their 16 GiB: a zero-stride view has the shape and no storage
    i64 = torch.zeros(1, dtype=torch.int64).expand(2 ** 31)
    f32 = torch.zeros(1, dtype=torch.float32).expand(2 ** 31)
    with pytest.raises(ValueError, match="2\\*\\*31"):
        check_common_neighbors_args(i64, i64, f32)
    with pytest.raises(ValueError, match="2\\*\\*31"):
        check_temporal_degree_args(i64, f32)
    n = 2 ** 31 - 1
    assert check_common_neighbors_args(i64[:n], i64[:n], f32[:n], f32[:n])[0] == n
    assert check_temporal_degree_args(i64[:n], f32[:n], f32[:n]) == n


@pytest.mark.parametrize("name,dtype", [("dst", torch.int64), ("ts", torch.float32),
                                        ("since", torch.float32)])
def test_devices_differ(name, dtype):
    with pytest.raises(ValueError, match=name + " is on meta"):
        check_common_neighbors_args(**_args(**{name: torch.zeros(4, dtype=dtype, device="meta")}))


def test_method_checks_before_it_touches_the_graph():
    """The method raises on bad arguments and on CPU tensors without a graph handle."""
    g = DynamicGraph.__new__(DynamicGraph)      # no native handle: nothing can be launched
    g._device = 0
    with pytest.raises(TypeError, match="src"):
        g.common_neighbors(**_args(src=torch.zeros(4, dtype=torch.int32)))
    with pytest.raises(TypeError, match="since"):
        g.common_neighbors(**_args(since="yesterday"))
    with pytest.raises(ValueError, match="max_history"):
        g.common_neighbors(**_args(max_history=0))
    with pytest.raises(ValueError, match="max_common"):
        g.common_neighbors(**_args(max_common=513))
    with pytest.raises(ValueError, match="the graph is on device"):
        g.common_neighbors(**_args())
    with pytest.raises(TypeError):
        g.common_neighbors(*_args().values())      # since and the bounds are keyword-only
    with pytest.raises(ValueError, match="the graph is on device"):
        g.temporal_degree(torch.zeros((2, 3), dtype=torch.int64), torch.zeros((2, 3)))
    with pytest.raises(TypeError):
        g.temporal_degree(torch.zeros(2, dtype=torch.int64), torch.zeros(2), 0.0)


# ---- temporal_degree's own checks ------------------------------------------------------------

def test_temporal_degree_good_arguments():
    n, t = torch.zeros((3, 5), dtype=torch.int64), torch.zeros((3, 5))
    assert check_temporal_degree_args(n, t) == 15
    assert check_temporal_degree_args(n, t, 2.0) == 15
    assert check_temporal_degree_args(n, t, torch.zeros((3, 5))) == 15
    assert check_temporal_degree_args(n[:, :0], t[:, :0]) == 0
    assert check_temporal_degree_args(n[0, 0], t[0, 0]) == 1


def test_temporal_degree_bad_arguments():
    n, t = torch.zeros((3, 5), dtype=torch.int64), torch.zeros((3, 5))
    with pytest.raises(TypeError, match="nodes"):
        check_temporal_degree_args(n.int(), t)
    with pytest.raises(TypeError, match="nodes"):
        check_temporal_degree_args(np.zeros((3, 5), np.int64), t)
    with pytest.raises(TypeError, match="ts"):
        check_temporal_degree_args(n, t.double())
    with pytest.raises(TypeError, match="since"):
        check_temporal_degree_args(n, t, t.double())
    with pytest.raises(ValueError, match="ts has"):
        check_temporal_degree_args(n, t[:, :4])
    with pytest.raises(ValueError, match="ts has"):
        check_temporal_degree_args(n, t.reshape(5, 3))
    with pytest.raises(ValueError, match="since has"):
        check_temporal_degree_args(n, t, t[0])
    with pytest.raises(ValueError, match="ts is on meta"):
        check_temporal_degree_args(n, torch.zeros((3, 5), device="meta"))
    with pytest.raises(ValueError, match="since is on meta"):
        check_temporal_degree_args(n, t, torch.zeros((3, 5), device="meta"))


# ---- the native entries: bound, and refusing without a launch -------------------------------

def test_native_entries_are_bound_and_reject_a_null_graph():
    assert len(_capi.PROTOTYPES["gf_graph_common_neighbors"][1]) == 18
    assert len(_capi.PROTOTYPES["gf_graph_temporal_degree"][1]) == 8
    lib = _capi.load()
    rc = lib.gf_graph_common_neighbors(None, None, None, None, None, 0, 64, 32, None, None, None,
                                       None, None, None, None, None, 0, None)
    assert rc == _capi.GF_ERR_INVALID_ARGUMENT
    assert b"null graph" in lib.gf_last_error()
    rc = lib.gf_graph_temporal_degree(None, None, None, None, 0, None, 0, None)
    assert rc == _capi.GF_ERR_INVALID_ARGUMENT
    assert b"null graph" in lib.gf_last_error()


# ---- NeighborOverlap's constructor: no device, no graph handle -------------------------------

def test_neighbor_overlap_defaults_and_good_arguments():
    b = NeighborOverlap(None)
    assert (b.score, b.max_history, b.max_common, b.window) == ("cn", 64, 64, None)
    b = NeighborOverlap(None, "aa", max_history=512, max_common=0, window=3)
    assert b.window == 3.0 and isinstance(b.window, float)
    assert (b.score, b.max_history, b.max_common) == ("aa", 512, 0)
    for score in R.SCORES:
        assert NeighborOverlap(None, score).score == score
    assert not isinstance(b, torch.nn.Module) and not isinstance(b, gnnflow_amd.EdgeBank)


@pytest.mark.parametrize("score", ["bogus", "CN", "", None, 0])
def test_neighbor_overlap_score(score):
    with pytest.raises(ValueError, match="score"):
        NeighborOverlap(None, score)


@pytest.mark.parametrize("window", [0, 0.0, -1.0, float("inf"), float("nan"), "3", True])
def test_neighbor_overlap_window(window):
    with pytest.raises(ValueError, match="window"):
        NeighborOverlap(None, window=window)


@pytest.mark.parametrize("max_history", [0, 513, -1, 1.5, True, None])
def test_neighbor_overlap_max_history(max_history):
    with pytest.raises(ValueError, match="max_history"):
        NeighborOverlap(None, max_history=max_history)


@pytest.mark.parametrize("max_common", [513, -1, 1.5, True, None])
def test_neighbor_overlap_max_common(max_common):
    with pytest.raises(ValueError, match="max_common"):
        NeighborOverlap(None, max_common=max_common)
    assert NeighborOverlap(None, max_common=0).max_common == 0
    assert NeighborOverlap(None, max_history=1, max_common=512).max_history == 1


def test_neighbor_overlap_predict_checks_the_layout_before_the_graph():
    b = NeighborOverlap(None)
    with pytest.raises(ValueError, match="neg_sample_ratio"):
        b.predict(torch.zeros(6, dtype=torch.int64), torch.zeros(6), neg_sample_ratio=-1)
    with pytest.raises(TypeError, match="roots and ts"):
        NeighborOverlap(DynamicGraph.__new__(DynamicGraph)).predict([0, 1, 2], torch.zeros(3))
