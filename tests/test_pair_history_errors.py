"""CPU tests of DynamicGraph.pair_history's argument checks
(dynamic_graph.check_pair_history_args) and of EdgeBank's constructor: every TypeError and
ValueError is raised before anything is launched and needs no device; and gf_graph_pair_history
rejects a null graph with a status code."""
import numpy as np
import pytest
import torch

import gnnflow_amd
from gnnflow_amd import EdgeBank, PairHistory, _capi
from gnnflow_amd.dynamic_graph import DynamicGraph, check_pair_history_args


def _args(N=4, **over):
    a = dict(src=torch.zeros(N, dtype=torch.int64), dst=torch.ones(N, dtype=torch.int64),
             ts=torch.zeros(N, dtype=torch.float32), since=None, max_history=0)
    a.update(over)
    return a


def test_names_are_exported():
    assert {"PairHistory", "EdgeBank"} <= set(gnnflow_amd.__all__)
    assert gnnflow_amd.PairHistory is PairHistory and gnnflow_amd.EdgeBank is EdgeBank
    assert PairHistory._fields == ("count", "last_ts", "last_eid")


def test_good_arguments_return_the_rows():
    assert check_pair_history_args(**_args()) == 4
    assert check_pair_history_args(**_args(N=0)) == 0
    assert check_pair_history_args(**_args(max_history=7)) == 4
    assert check_pair_history_args(**_args(since=40.0)) == 4
    assert check_pair_history_args(**_args(since=float("nan"))) == 4
    assert check_pair_history_args(**_args(since=torch.zeros(4))) == 4
    a = _args()
    assert check_pair_history_args(a["src"], a["dst"], a["ts"]) == 4


@pytest.mark.parametrize("name", ["src", "dst", "ts"])
def test_not_a_tensor(name):
    with pytest.raises(TypeError, match=name):
        check_pair_history_args(**_args(**{name: np.zeros(4)}))
    with pytest.raises(TypeError, match=name):
        check_pair_history_args(**_args(**{name: [0, 1, 2, 3]}))


@pytest.mark.parametrize("name,bad", [("src", torch.int32), ("src", torch.float32),
                                      ("dst", torch.int32), ("dst", torch.float32),
                                      ("ts", torch.float64), ("ts", torch.int64),
                                      ("since", torch.float64), ("since", torch.int64)])
def test_wrong_dtype(name, bad):
    with pytest.raises(TypeError, match=name):
        check_pair_history_args(**_args(**{name: torch.zeros(4, dtype=bad)}))


@pytest.mark.parametrize("bad", [True, "3", [0.0] * 4, np.zeros(4, np.float32), (1.0,)])
def test_since_must_be_none_a_float_or_a_tensor(bad):
    with pytest.raises(TypeError, match="since"):
        check_pair_history_args(**_args(since=bad))


@pytest.mark.parametrize("bad", [True, False, 1.0, None, "3", np.float32(2)])
def test_max_history_must_be_an_int(bad):
    with pytest.raises(TypeError, match="max_history"):
        check_pair_history_args(**_args(max_history=bad))


def test_negative_max_history():
    with pytest.raises(ValueError, match="max_history"):
        check_pair_history_args(**_args(max_history=-1))


@pytest.mark.parametrize("name", ["src", "dst", "ts", "since"])
def test_not_one_dimensional(name):
    good = _args(since=torch.zeros(4))[name]
    with pytest.raises(ValueError, match=name):
        check_pair_history_args(**_args(**{name: good.reshape(-1, 1)}))
    with pytest.raises(ValueError, match=name):
        check_pair_history_args(**_args(**{name: good[0]}))


@pytest.mark.parametrize("name,dtype", [("dst", torch.int64), ("ts", torch.float32),
                                        ("since", torch.float32)])
def test_lengths_differ(name, dtype):
    with pytest.raises(ValueError, match=name):
        check_pair_history_args(**_args(**{name: torch.zeros(3, dtype=dtype)}))


def test_too_many_rows():
    # 2^31 rows without their 16 GiB: a zero-stride view has the shape and no storage
    i64 = torch.zeros(1, dtype=torch.int64).expand(2 ** 31)
    f32 = torch.zeros(1, dtype=torch.float32).expand(2 ** 31)
    with pytest.raises(ValueError, match="2\\*\\*31"):
        check_pair_history_args(i64, i64, f32)
    n = 2 ** 31 - 1
    assert check_pair_history_args(i64[:n], i64[:n], f32[:n], f32[:n]) == n


@pytest.mark.parametrize("name,dtype", [("dst", torch.int64), ("ts", torch.float32),
                                        ("since", torch.float32)])
def test_devices_differ(name, dtype):
    with pytest.raises(ValueError, match=name + " is on meta"):
        check_pair_history_args(**_args(**{name: torch.zeros(4, dtype=dtype, device="meta")}))


def test_method_checks_before_it_touches_the_graph():
    """The method raises on bad arguments and on CPU tensors without a graph handle."""
    g = DynamicGraph.__new__(DynamicGraph)      # no native handle: nothing can be launched
    g._device = 0
    with pytest.raises(TypeError, match="src"):
        g.pair_history(**_args(src=torch.zeros(4, dtype=torch.int32)))
    with pytest.raises(TypeError, match="since"):
        g.pair_history(**_args(since="yesterday"))
    with pytest.raises(ValueError, match="max_history"):
        g.pair_history(**_args(max_history=-2))
    with pytest.raises(ValueError, match="the graph is on device"):
        g.pair_history(**_args())
    with pytest.raises(TypeError):
        g.pair_history(*_args().values())      # since and max_history are keyword-only


def test_native_entry_is_bound_and_rejects_a_null_graph():
    assert len(_capi.PROTOTYPES["gf_graph_pair_history"][1]) == 12
    lib = _capi.load()
    rc = lib.gf_graph_pair_history(None, None, None, None, None, 0, 0, None, None, None, 0, None)
    assert rc == _capi.GF_ERR_INVALID_ARGUMENT
    assert b"null graph" in lib.gf_last_error()


# ---- EdgeBank's constructor: no device, no graph handle -------------------------------------

def test_edge_bank_defaults_and_good_arguments():
    b = EdgeBank(None)
    assert (b.mode, b.window, b.min_count, b.max_history, b.score) == \
        ("unlimited", None, 1, 0, "seen")
    b = EdgeBank(None, "time_window", window=3, min_count=2, max_history=64, score="count")
    assert b.window == 3.0 and isinstance(b.window, float)
    assert (b.mode, b.min_count, b.max_history, b.score) == ("time_window", 2, 64, "count")
    assert not isinstance(b, torch.nn.Module)


@pytest.mark.parametrize("mode", ["bogus", "UNLIMITED", "", None, 1])
def test_edge_bank_mode(mode):
    with pytest.raises(ValueError, match="mode"):
        EdgeBank(None, mode)


@pytest.mark.parametrize("score", ["bogus", "Seen", "", None, 0])
def test_edge_bank_score(score):
    with pytest.raises(ValueError, match="score"):
        EdgeBank(None, score=score)


@pytest.mark.parametrize("window", [None, 0, 0.0, -1.0, float("inf"), float("nan"), "3", True])
def test_edge_bank_window(window):
    with pytest.raises(ValueError, match="window"):
        EdgeBank(None, "time_window", window=window)


def test_edge_bank_window_without_the_mode():
    with pytest.raises(ValueError, match="window"):
        EdgeBank(None, "unlimited", window=5.0)


@pytest.mark.parametrize("min_count", [0, -1, 1.0, True, None, "2"])
def test_edge_bank_min_count(min_count):
    with pytest.raises(ValueError, match="min_count"):
        EdgeBank(None, min_count=min_count)


@pytest.mark.parametrize("max_history", [-1, 1.5, True, None])
def test_edge_bank_max_history(max_history):
    with pytest.raises(ValueError, match="max_history"):
        EdgeBank(None, max_history=max_history)


def test_edge_bank_predict_checks_the_layout_before_the_graph():
    b = EdgeBank(None)
    with pytest.raises(ValueError, match="neg_sample_ratio"):
        b.predict(torch.zeros(6, dtype=torch.int64), torch.zeros(6), neg_sample_ratio=-1)
    with pytest.raises(TypeError, match="roots and ts"):
        EdgeBank(DynamicGraph.__new__(DynamicGraph)).predict([0, 1, 2], torch.zeros(3))
