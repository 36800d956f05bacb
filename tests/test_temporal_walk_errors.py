"""CPU tests of the argument checks of DynamicGraph.temporal_random_walk
(dynamic_graph.check_temporal_walk_args) and ops.walk_position_counts
(ops.check_walk_position_counts_args): every TypeError and ValueError is raised before anything is
launched or allocated and needs no device; and the two native entries reject bad calls with a
status code."""
import numpy as np
import pytest
import torch

import gnnflow_amd
from gnnflow_amd import _capi, ops
from gnnflow_amd.dynamic_graph import DynamicGraph, TemporalWalks, check_temporal_walk_args
from gnnflow_amd.ops import check_walk_position_counts_args


def _args(B=4, **over):
    a = dict(src=torch.zeros(B, dtype=torch.int64), ts=torch.zeros(B, dtype=torch.float32),
             length=3, num_walks=2, recency=1, max_history=0, seed=0, epoch=0, first_row=0)
    a.update(over)
    return a


def _huge(*shape, dtype=torch.int64):
    """A tensor of this shape without its storage: a zero-stride view."""
    return torch.zeros(1, dtype=dtype).expand(*shape)


def test_good_arguments_return_the_sizes():
    assert check_temporal_walk_args(**_args()) == (4, 2, 3)
    assert check_temporal_walk_args(**_args(B=0)) == (0, 2, 3)
    a = _args()
    assert check_temporal_walk_args(a["src"], a["ts"], 1) == (4, 1, 1)
    assert check_temporal_walk_args(**_args(length=32, num_walks=2 ** 16 - 1, recency=8,
                                            max_history=5, seed=2 ** 64 - 1, epoch=2 ** 64 - 1,
                                            first_row=2 ** 64 - 1)) == (4, 2 ** 16 - 1, 32)
    assert check_temporal_walk_args(**_args(length=np.int64(2))) == (4, 2, 2)
    assert "TemporalWalks" in gnnflow_amd.__all__ and gnnflow_amd.TemporalWalks is TemporalWalks
    assert TemporalWalks._fields == ("nodes", "eids", "times")


@pytest.mark.parametrize("name", ["src", "ts"])
def test_not_a_tensor(name):
    with pytest.raises(TypeError, match=name):
        check_temporal_walk_args(**_args(**{name: np.zeros(4)}))
    with pytest.raises(TypeError, match=name):
        check_temporal_walk_args(**_args(**{name: [0, 1, 2, 3]}))


@pytest.mark.parametrize("name,bad", [("src", torch.int32), ("src", torch.float32),
                                      ("ts", torch.float64), ("ts", torch.int64)])
def test_wrong_dtype(name, bad):
    with pytest.raises(TypeError, match=name):
        check_temporal_walk_args(**_args(**{name: torch.zeros(4, dtype=bad)}))


@pytest.mark.parametrize("name", ["length", "num_walks", "recency", "max_history", "seed", "epoch",
                                  "first_row"])
@pytest.mark.parametrize("bad", [True, 1.0, None, "3", np.float32(2)])
def test_counts_must_be_ints(name, bad):
    with pytest.raises(TypeError, match=name):
        check_temporal_walk_args(**_args(**{name: bad}))


@pytest.mark.parametrize("name,bad", [("length", 0), ("length", 33), ("length", -1),
                                      ("num_walks", 0), ("num_walks", 2 ** 16),
                                      ("recency", 0), ("recency", 9), ("max_history", -1),
                                      ("seed", -1), ("seed", 2 ** 64), ("epoch", 2 ** 64),
                                      ("first_row", -1)])
def test_out_of_range(name, bad):
    with pytest.raises(ValueError, match=name):
        check_temporal_walk_args(**_args(**{name: bad}))


@pytest.mark.parametrize("name", ["src", "ts"])
def test_not_one_dimensional(name):
    good = _args()[name]
    with pytest.raises(ValueError, match=name):
        check_temporal_walk_args(**_args(**{name: good.reshape(-1, 1)}))
    with pytest.raises(ValueError, match=name):
        check_temporal_walk_args(**_args(**{name: good[0]}))


def test_lengths_differ():
    with pytest.raises(ValueError, match="ts"):
        check_temporal_walk_args(**_args(ts=torch.zeros(3)))


def test_too_many_walks():
    B = 2 ** 16
    src, ts = _huge(B), _huge(B, dtype=torch.float32)
    with pytest.raises(ValueError, match="2\\*\\*31"):
        check_temporal_walk_args(**_args(src=src, ts=ts, num_walks=2 ** 15))
    assert check_temporal_walk_args(**_args(src=src, ts=ts, num_walks=2 ** 15 - 1))[0] == B
    with pytest.raises(ValueError, match="2\\*\\*31"):
        check_temporal_walk_args(**_args(src=_huge(2 ** 31), ts=_huge(2 ** 31, dtype=torch.float32),
                                         num_walks=1))


def test_devices_differ():
    with pytest.raises(ValueError, match="ts is on meta"):
        check_temporal_walk_args(**_args(ts=torch.zeros(4, device="meta")))


def test_method_checks_before_it_touches_the_graph():
    """The method raises on bad arguments and on CPU tensors without a graph handle."""
    g = DynamicGraph.__new__(DynamicGraph)      # no native handle: nothing can be launched
    g._device = 0
    a = _args()
    src, ts, length, num_walks = (a.pop(k) for k in ("src", "ts", "length", "num_walks"))
    with pytest.raises(TypeError, match="src"):
        g.temporal_random_walk(src.int(), ts, length, num_walks, **a)
    with pytest.raises(ValueError, match="length"):
        g.temporal_random_walk(src, ts, 0)
    with pytest.raises(ValueError, match="recency"):
        g.temporal_random_walk(src, ts, length, num_walks, recency=9)
    with pytest.raises(TypeError):              # the options are keyword-only
        g.temporal_random_walk(src, ts, length, num_walks, 1)
    with pytest.raises(ValueError, match="the graph is on device"):
        g.temporal_random_walk(src, ts, length, num_walks, **a)


def _walks(B=3, W=4, L1=3, dtype=torch.int64):
    return torch.zeros((B, W, L1), dtype=dtype)


def test_position_counts_good_arguments_return_the_sizes():
    assert check_walk_position_counts_args(_walks()) == (3, 4, 3, 4, 3)
    assert check_walk_position_counts_args(_walks(), _walks(3, 7, 2)) == (3, 4, 3, 7, 2)
    assert check_walk_position_counts_args(_walks(0), None) == (0, 4, 3, 4, 3)
    assert check_walk_position_counts_args(_walks(L1=33), _walks(3, 124, 33)) == (3, 4, 33, 124, 33)
    # W is not bounded by the set that goes to LDS when another one is counted in
    assert check_walk_position_counts_args(_huge(3, 5000, 3), _walks(3, 4096, 1))[1] == 5000


@pytest.mark.parametrize("name", ["nodes", "ref"])
def test_position_counts_types(name):
    for bad in (np.zeros((3, 4, 3), np.int64), [[[0]]]):
        with pytest.raises(TypeError, match=name):
            check_walk_position_counts_args(**{"nodes": _walks(), name: bad})
    for bad in (torch.int32, torch.float32):
        with pytest.raises(TypeError, match=name):
            check_walk_position_counts_args(**{"nodes": _walks(), name: _walks(dtype=bad)})


@pytest.mark.parametrize("name", ["nodes", "ref"])
def test_position_counts_ranks_and_lengths(name):
    for bad in (torch.zeros((3, 12), dtype=torch.int64), torch.zeros((3, 4, 3, 1), dtype=torch.int64),
                _walks(L1=0), _walks(L1=34)):
        with pytest.raises(ValueError, match=name):
            check_walk_position_counts_args(**{"nodes": _walks(), name: bad})


def test_position_counts_rows_differ():
    with pytest.raises(ValueError, match="ref has 2"):
        check_walk_position_counts_args(_walks(), _walks(2))


def test_position_counts_reference_set_too_large():
    assert check_walk_position_counts_args(_walks(), _walks(3, 1024, 4))[3:] == (1024, 4)
    with pytest.raises(ValueError, match="4096"):
        check_walk_position_counts_args(_walks(), _walks(3, 1025, 4))
    with pytest.raises(ValueError, match="4096"):               # ref=None: nodes is the set
        check_walk_position_counts_args(_walks(3, 1366, 3))
    with pytest.raises(ValueError, match="2\\*\\*31"):
        check_walk_position_counts_args(_huge(1, 2 ** 22, 33), _walks(1, 4, 33))
    with pytest.raises(ValueError, match="2\\*\\*31"):
        check_walk_position_counts_args(_huge(2 ** 31, 1, 1))


def test_position_counts_devices():
    with pytest.raises(ValueError, match="ref is on meta"):
        check_walk_position_counts_args(_walks(), _walks().to("meta"))
    with pytest.raises(ValueError, match="runs on the GPU"):
        ops.walk_position_counts(_walks())
    with pytest.raises(TypeError, match="nodes"):
        ops.walk_position_counts(_walks(dtype=torch.int32))


def test_native_entries_are_bound_and_reject_bad_calls():
    assert len(_capi.PROTOTYPES["gf_graph_temporal_walks"][1]) == 16
    assert len(_capi.PROTOTYPES["gf_walk_position_counts"][1]) == 10
    lib = _capi.load()
    rc = lib.gf_graph_temporal_walks(None, None, None, 0, 1, 1, 1, 0, 0, 0, 0, None, None, None,
                                     0, None)
    assert rc == _capi.GF_ERR_INVALID_ARGUMENT and b"null graph" in lib.gf_last_error()
    for args, what in (((1, 1, 34, 1, 1), b"32 steps"), ((1, 1, 3, 1, 34), b"32 steps"),
                       ((1, 1, 3, 1025, 4), b"4096"), ((1, 2 ** 22, 33, 4, 33), b"2^31"),
                       ((1, 1, 3, 1, 3), b"null")):
        rc = lib.gf_walk_position_counts(None, None, *args, None, 0, None)
        assert rc == _capi.GF_ERR_INVALID_ARGUMENT and what in lib.gf_last_error(), args
    # nothing to do: no launch, no device needed
    assert lib.gf_walk_position_counts(None, None, 0, 4, 3, 4, 3, None, 0, None) == _capi.GF_OK
