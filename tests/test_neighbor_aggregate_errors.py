"""CPU tests of DynamicGraph.neighbor_aggregate's argument checks
(dynamic_graph.check_neighbor_aggregate_args): every TypeError and ValueError is raised before
anything is launched or allocated and needs no device; and gf_graph_neighbor_aggregate rejects a
null graph with a status code."""
import numpy as np
import pytest
import torch

import gnnflow_amd
from gnnflow_amd import NeighborAggregate, _capi
from gnnflow_amd.dynamic_graph import (AGG_MAX_WIDTH, DynamicGraph,
                                       check_neighbor_aggregate_args)


def _args(N=4, **over):
    a = dict(nodes=torch.zeros(N, dtype=torch.int64), ts=torch.zeros(N, dtype=torch.float32),
             node_feats=torch.zeros(10, 8), edge_feats=None, since=None, max_history=0,
             reduce="mean")
    a.update(over)
    return a


def test_names_are_exported():
    assert {"NeighborAggregate", "FixedTimeEncode"} <= set(gnnflow_amd.__all__)
    assert gnnflow_amd.NeighborAggregate is NeighborAggregate
    assert NeighborAggregate._fields == ("count", "node", "edge")
    from gnnflow_amd import models
    assert "GraphMixer" in models.__all__ and models.GraphMixer.__name__ == "GraphMixer"
    assert AGG_MAX_WIDTH == 1024


def test_good_arguments_return_the_rows_and_the_widths():
    assert check_neighbor_aggregate_args(**_args()) == (4, 8, 0)
    assert check_neighbor_aggregate_args(**_args(N=0)) == (0, 8, 0)
    assert check_neighbor_aggregate_args(**_args(edge_feats=torch.zeros(3, 5))) == (4, 8, 5)
    assert check_neighbor_aggregate_args(
        **_args(node_feats=None, edge_feats=torch.zeros(3, 1))) == (4, 0, 1)
    assert check_neighbor_aggregate_args(**_args(node_feats=torch.zeros(2, 1024))) == (4, 1024, 0)
    assert check_neighbor_aggregate_args(**_args(max_history=7, reduce="sum")) == (4, 8, 0)
    assert check_neighbor_aggregate_args(**_args(since=40.0)) == (4, 8, 0)
    assert check_neighbor_aggregate_args(**_args(since=float("nan"))) == (4, 8, 0)
    assert check_neighbor_aggregate_args(**_args(since=torch.zeros(4))) == (4, 8, 0)
    a = _args()
    assert check_neighbor_aggregate_args(a["nodes"], a["ts"], a["node_feats"]) == (4, 8, 0)
    # a row slice of a table is contiguous and is taken as it is
    assert check_neighbor_aggregate_args(**_args(node_feats=torch.zeros(10, 8)[2:7])) == (4, 8, 0)


@pytest.mark.parametrize("name", ["nodes", "ts", "node_feats", "edge_feats"])
def test_not_a_tensor(name):
    with pytest.raises(TypeError, match=name):
        check_neighbor_aggregate_args(**_args(**{name: np.zeros((4, 4), np.float32)}))
    with pytest.raises(TypeError, match=name):
        check_neighbor_aggregate_args(**_args(**{name: [0, 1, 2, 3]}))


@pytest.mark.parametrize("name,bad", [("nodes", torch.int32), ("nodes", torch.float32),
                                      ("ts", torch.float64), ("ts", torch.int64),
                                      ("since", torch.float64), ("since", torch.int64)])
def test_wrong_dtype(name, bad):
    with pytest.raises(TypeError, match=name):
        check_neighbor_aggregate_args(**_args(**{name: torch.zeros(4, dtype=bad)}))


@pytest.mark.parametrize("name", ["node_feats", "edge_feats"])
@pytest.mark.parametrize("bad", [torch.float16, torch.bfloat16, torch.float64, torch.int64])
def test_tables_are_float32_and_the_message_says_so(name, bad):
    with pytest.raises(TypeError, match=name + ".*float32"):
        check_neighbor_aggregate_args(**_args(**{name: torch.zeros(4, 8, dtype=bad)}))


@pytest.mark.parametrize("bad", [True, "3", [0.0] * 4, np.zeros(4, np.float32), (1.0,)])
def test_since_must_be_none_a_float_or_a_tensor(bad):
    with pytest.raises(TypeError, match="since"):
        check_neighbor_aggregate_args(**_args(since=bad))


@pytest.mark.parametrize("bad", [True, False, 1.0, None, "3", np.float32(2)])
def test_max_history_must_be_an_int(bad):
    with pytest.raises(TypeError, match="max_history"):
        check_neighbor_aggregate_args(**_args(max_history=bad))


def test_negative_max_history():
    with pytest.raises(ValueError, match="max_history"):
        check_neighbor_aggregate_args(**_args(max_history=-1))


@pytest.mark.parametrize("bad", [None, 1, True, b"mean"])
def test_reduce_must_be_a_str(bad):
    with pytest.raises(TypeError, match="reduce"):
        check_neighbor_aggregate_args(**_args(reduce=bad))


@pytest.mark.parametrize("bad", ["max", "MEAN", "", "avg"])
def test_reduce_must_be_sum_or_mean(bad):
    with pytest.raises(ValueError, match="reduce"):
        check_neighbor_aggregate_args(**_args(reduce=bad))


@pytest.mark.parametrize("name", ["nodes", "ts", "since"])
def test_not_one_dimensional(name):
    good = _args(since=torch.zeros(4))[name]
    with pytest.raises(ValueError, match=name):
        check_neighbor_aggregate_args(**_args(**{name: good.reshape(-1, 1)}))
    with pytest.raises(ValueError, match=name):
        check_neighbor_aggregate_args(**_args(**{name: good[0]}))


@pytest.mark.parametrize("name", ["ts", "since"])
def test_lengths_differ(name):
    with pytest.raises(ValueError, match=name):
        check_neighbor_aggregate_args(**_args(**{name: torch.zeros(3)}))


def test_too_many_rows():
    i64 = torch.zeros(1, dtype=torch.int64).expand(2 ** 31)
    f32 = torch.zeros(1, dtype=torch.float32).expand(2 ** 31)
    with pytest.raises(ValueError, match="2\\*\\*31"):
        check_neighbor_aggregate_args(i64, f32, torch.zeros(2, 2))
    n = 2 ** 31 - 1
    assert check_neighbor_aggregate_args(i64[:n], f32[:n], torch.zeros(2, 2)) == (n, 2, 0)


def test_no_table_at_all():
    with pytest.raises(ValueError, match="node_feats or edge_feats"):
        check_neighbor_aggregate_args(**_args(node_feats=None))


@pytest.mark.parametrize("name", ["node_feats", "edge_feats"])
def test_table_shapes(name):
    for bad in (torch.zeros(8), torch.zeros(2, 3, 4), torch.zeros(())):
        with pytest.raises(ValueError, match=name + " must be 2-D"):
            check_neighbor_aggregate_args(**_args(**{name: bad}))
    with pytest.raises(ValueError, match=name + " has no rows"):
        check_neighbor_aggregate_args(**_args(**{name: torch.zeros(0, 4)}))
    for width in (0, AGG_MAX_WIDTH + 1, 4096):
        with pytest.raises(ValueError, match=name + " must have 1 to 1024 columns"):
            check_neighbor_aggregate_args(**_args(**{name: torch.zeros(2, width)}))


@pytest.mark.parametrize("name", ["node_feats", "edge_feats"])
def test_a_table_that_is_not_contiguous_is_not_copied(name):
    for bad in (torch.zeros(8, 10).t(), torch.zeros(10, 16)[:, :8], torch.zeros(10, 8)[::2]):
        assert not bad.is_contiguous()
        with pytest.raises(ValueError, match=name + " must be contiguous"):
            check_neighbor_aggregate_args(**_args(**{name: bad}))


@pytest.mark.parametrize("name,shape,dtype", [("ts", (4,), torch.float32),
                                              ("since", (4,), torch.float32),
                                              ("node_feats", (10, 8), torch.float32),
                                              ("edge_feats", (10, 8), torch.float32)])
def test_devices_differ(name, shape, dtype):
    with pytest.raises(ValueError, match=name + " is on meta"):
        check_neighbor_aggregate_args(
            **_args(**{name: torch.zeros(shape, dtype=dtype, device="meta")}))


def test_method_checks_before_it_touches_the_graph():
    """The method raises on bad arguments and on CPU tensors without a graph handle."""
    g = DynamicGraph.__new__(DynamicGraph)      # no native handle: nothing can be launched
    g._device = 0
    with pytest.raises(TypeError, match="nodes"):
        g.neighbor_aggregate(**_args(nodes=torch.zeros(4, dtype=torch.int32)))
    with pytest.raises(TypeError, match="float32"):
        g.neighbor_aggregate(**_args(node_feats=torch.zeros(4, 4, dtype=torch.bfloat16)))
    with pytest.raises(ValueError, match="reduce"):
        g.neighbor_aggregate(**_args(reduce="max"))
    with pytest.raises(ValueError, match="the graph is on device"):
        g.neighbor_aggregate(**_args())
    with pytest.raises(TypeError):
        g.neighbor_aggregate(*_args().values())      # everything past ts is keyword-only


def test_native_entry_is_bound_and_rejects_a_null_graph():
    assert len(_capi.PROTOTYPES["gf_graph_neighbor_aggregate"][1]) == 18
    lib = _capi.load()
    rc = lib.gf_graph_neighbor_aggregate(None, None, None, None, 0, 0, None, 0, 0, None, 0, 0, 0,
                                         None, None, None, 0, None)
    assert rc == _capi.GF_ERR_INVALID_ARGUMENT
    assert b"null graph" in lib.gf_last_error()
