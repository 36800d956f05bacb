"""CPU tests of DynamicGraph.neighbor_sequence's argument checks
(dynamic_graph.check_neighbor_sequence_args): every TypeError and ValueError is raised before
anything is launched or allocated and needs no device; and gf_graph_neighbor_sequence rejects a
null graph with a status code."""
import numpy as np
import pytest
import torch

import gnnflow_amd
from gnnflow_amd import NeighborSequence, _capi
from gnnflow_amd.dynamic_graph import (SEQ_MAX_LENGTH, SEQ_MAX_WIDTH, DynamicGraph,
                                       check_neighbor_sequence_args)
from gnnflow_amd.nn import FixedTimeEncode, TimeEncode


def _args(N=4, **over):
    a = dict(nodes=torch.zeros(N, dtype=torch.int64), ts=torch.zeros(N, dtype=torch.float32),
             since=None, length=32, edge_feats=torch.zeros(10, 8), node_feats=None,
             time_encoder=None)
    a.update(over)
    return a


def _pair(dT=6):
    return torch.zeros(dT, 1), torch.zeros(dT)


def test_names_are_exported():
    assert "NeighborSequence" in gnnflow_amd.__all__
    assert gnnflow_amd.NeighborSequence is NeighborSequence
    assert NeighborSequence._fields == ("lengths", "nodes", "eids", "times", "delta_t", "tokens")
    assert SEQ_MAX_LENGTH == 512 and SEQ_MAX_WIDTH == 1024
    from gnnflow_amd import models
    assert callable(models.GraphMixer.forward_tokens)


def test_good_arguments_return_the_rows_the_length_and_the_widths():
    assert check_neighbor_sequence_args(**_args()) == (4, 32, 8, 0, 0)
    assert check_neighbor_sequence_args(**_args(N=0)) == (0, 32, 8, 0, 0)
    assert check_neighbor_sequence_args(**_args(edge_feats=None)) == (4, 32, 0, 0, 0)
    assert check_neighbor_sequence_args(**_args(node_feats=torch.zeros(3, 5))) == (4, 32, 8, 5, 0)
    assert check_neighbor_sequence_args(
        **_args(edge_feats=None, node_feats=torch.zeros(3, 1))) == (4, 32, 0, 1, 0)
    assert check_neighbor_sequence_args(
        **_args(edge_feats=torch.zeros(2, 1024), length=512)) == (4, 512, 1024, 0, 0)
    assert check_neighbor_sequence_args(**_args(length=1)) == (4, 1, 8, 0, 0)
    assert check_neighbor_sequence_args(**_args(length=np.int64(7))) == (4, 7, 8, 0, 0)
    for since in (40.0, float("nan"), 3, torch.zeros(4)):
        assert check_neighbor_sequence_args(**_args(since=since)) == (4, 32, 8, 0, 0)
    a = _args()
    assert check_neighbor_sequence_args(a["nodes"], a["ts"]) == (4, 32, 0, 0, 0)
    # a row slice of a table is contiguous and is taken as it is
    assert check_neighbor_sequence_args(
        **_args(edge_feats=torch.zeros(10, 8)[2:7])) == (4, 32, 8, 0, 0)


def test_every_form_of_time_encoder():
    assert check_neighbor_sequence_args(**_args(time_encoder=_pair())) == (4, 32, 8, 0, 6)
    assert check_neighbor_sequence_args(**_args(time_encoder=list(_pair(1)))) == (4, 32, 8, 0, 1)
    assert check_neighbor_sequence_args(
        **_args(time_encoder=(torch.zeros(6), torch.zeros(6)))) == (4, 32, 8, 0, 6)
    assert check_neighbor_sequence_args(
        **_args(edge_feats=None, time_encoder=FixedTimeEncode(100))) == (4, 32, 0, 0, 100)
    assert check_neighbor_sequence_args(
        **_args(node_feats=torch.zeros(2, 3), time_encoder=TimeEncode(4))) == (4, 32, 8, 3, 4)
    assert check_neighbor_sequence_args(**_args(time_encoder=_pair(1024))) == (4, 32, 8, 0, 1024)


@pytest.mark.parametrize("name", ["nodes", "ts", "edge_feats", "node_feats"])
def test_not_a_tensor(name):
    with pytest.raises(TypeError, match=name):
        check_neighbor_sequence_args(**_args(**{name: np.zeros((4, 4), np.float32)}))
    with pytest.raises(TypeError, match=name):
        check_neighbor_sequence_args(**_args(**{name: [0, 1, 2, 3]}))


@pytest.mark.parametrize("name,bad", [("nodes", torch.int32), ("nodes", torch.float32),
                                      ("ts", torch.float64), ("ts", torch.int64),
                                      ("since", torch.float64), ("since", torch.int64)])
def test_wrong_dtype(name, bad):
    with pytest.raises(TypeError, match=name):
        check_neighbor_sequence_args(**_args(**{name: torch.zeros(4, dtype=bad)}))


@pytest.mark.parametrize("name", ["edge_feats", "node_feats"])
@pytest.mark.parametrize("bad", [torch.float16, torch.bfloat16, torch.float64, torch.int64])
def test_tables_are_float32_and_the_message_says_so(name, bad):
    with pytest.raises(TypeError, match=name + ".*float32"):
        check_neighbor_sequence_args(**_args(**{name: torch.zeros(4, 8, dtype=bad)}))


@pytest.mark.parametrize("bad", [True, "3", [0.0] * 4, np.zeros(4, np.float32), (1.0,)])
def test_since_must_be_none_a_float_or_a_tensor(bad):
    with pytest.raises(TypeError, match="since"):
        check_neighbor_sequence_args(**_args(since=bad))


@pytest.mark.parametrize("bad", [True, False, 1.0, None, "3", np.float32(2)])
def test_length_must_be_an_int(bad):
    with pytest.raises(TypeError, match="length"):
        check_neighbor_sequence_args(**_args(length=bad))


@pytest.mark.parametrize("bad", [0, -1, SEQ_MAX_LENGTH + 1, 4096])
def test_length_outside_1_to_512(bad):
    with pytest.raises(ValueError, match="length"):
        check_neighbor_sequence_args(**_args(length=bad))


@pytest.mark.parametrize("bad", [3, "cos", torch.zeros(4), (torch.zeros(4, 1),),
                                 (torch.zeros(4, 1), torch.zeros(4), torch.zeros(4)),
                                 torch.nn.ReLU()])
def test_time_encoder_must_hold_a_weight_and_a_bias(bad):
    with pytest.raises(TypeError, match="time_encoder"):
        check_neighbor_sequence_args(**_args(time_encoder=bad))


@pytest.mark.parametrize("which", [0, 1])
def test_time_encoder_tensors_are_float32_tensors(which):
    for bad in (np.zeros(6, np.float32), None, torch.zeros(6, dtype=torch.float64),
                torch.zeros(6, dtype=torch.bfloat16)):
        pair = list(_pair())
        pair[which] = bad
        with pytest.raises(TypeError, match="time_encoder's " + ("weight", "bias")[which]):
            check_neighbor_sequence_args(**_args(time_encoder=tuple(pair)))


def test_time_encoder_shapes():
    for weight, bias in ((torch.zeros(6, 1), torch.zeros(5)), (torch.zeros(5), torch.zeros(6)),
                         (torch.zeros(1, 6), torch.zeros(6)), (torch.zeros(6, 2), torch.zeros(6)),
                         (torch.zeros(6, 1, 1), torch.zeros(6))):
        with pytest.raises(ValueError, match="time_encoder's weight"):
            check_neighbor_sequence_args(**_args(time_encoder=(weight, bias)))
    for bias in (torch.zeros(6, 1), torch.zeros(())):
        with pytest.raises(ValueError, match="time_encoder's bias"):
            check_neighbor_sequence_args(**_args(time_encoder=(torch.zeros(6, 1), bias)))
    for dT in (0, SEQ_MAX_WIDTH + 1):
        with pytest.raises(ValueError, match="time_encoder must have 1 to 1024 columns"):
            check_neighbor_sequence_args(**_args(time_encoder=_pair(dT)))


@pytest.mark.parametrize("name", ["nodes", "ts", "since"])
def test_not_one_dimensional(name):
    good = _args(since=torch.zeros(4))[name]
    with pytest.raises(ValueError, match=name):
        check_neighbor_sequence_args(**_args(**{name: good.reshape(-1, 1)}))
    with pytest.raises(ValueError, match=name):
        check_neighbor_sequence_args(**_args(**{name: good[0]}))


@pytest.mark.parametrize("name", ["ts", "since"])
def test_lengths_differ(name):
    with pytest.raises(ValueError, match=name):
        check_neighbor_sequence_args(**_args(**{name: torch.zeros(3)}))


def test_too_many_rows():
    i64 = torch.zeros(1, dtype=torch.int64).expand(2 ** 31)
    f32 = torch.zeros(1, dtype=torch.float32).expand(2 ** 31)
    with pytest.raises(ValueError, match="2\\*\\*31"):
        check_neighbor_sequence_args(i64, f32)
    n = 2 ** 31 - 1
    assert check_neighbor_sequence_args(i64[:n], f32[:n], length=2) == (n, 2, 0, 0, 0)


@pytest.mark.parametrize("name", ["edge_feats", "node_feats"])
def test_table_shapes(name):
    for bad in (torch.zeros(8), torch.zeros(2, 3, 4), torch.zeros(())):
        with pytest.raises(ValueError, match=name + " must be 2-D"):
            check_neighbor_sequence_args(**_args(**{name: bad}))
    with pytest.raises(ValueError, match=name + " has no rows"):
        check_neighbor_sequence_args(**_args(**{name: torch.zeros(0, 4)}))
    for width in (0, SEQ_MAX_WIDTH + 1, 4096):
        with pytest.raises(ValueError, match=name + " must have 1 to 1024 columns"):
            check_neighbor_sequence_args(**_args(**{name: torch.zeros(2, width)}))


@pytest.mark.parametrize("name", ["edge_feats", "node_feats"])
def test_a_table_that_is_not_contiguous_is_not_copied(name):
    for bad in (torch.zeros(8, 10).t(), torch.zeros(10, 16)[:, :8], torch.zeros(10, 8)[::2]):
        assert not bad.is_contiguous()
        with pytest.raises(ValueError, match=name + " must be contiguous"):
            check_neighbor_sequence_args(**_args(**{name: bad}))


@pytest.mark.parametrize("name,shape", [("ts", (4,)), ("since", (4,)), ("edge_feats", (10, 8)),
                                        ("node_feats", (10, 8))])
def test_devices_differ(name, shape):
    with pytest.raises(ValueError, match=name + " is on meta"):
        check_neighbor_sequence_args(**_args(**{name: torch.zeros(shape, device="meta")}))


def test_the_encoder_is_on_the_rows_device():
    weight, bias = _pair()
    with pytest.raises(ValueError, match="time_encoder's weight is on meta"):
        check_neighbor_sequence_args(**_args(time_encoder=(weight.to("meta"), bias)))
    with pytest.raises(ValueError, match="time_encoder's bias is on meta"):
        check_neighbor_sequence_args(**_args(time_encoder=(weight, bias.to("meta"))))
    with pytest.raises(ValueError, match="is on meta"):
        check_neighbor_sequence_args(**_args(time_encoder=FixedTimeEncode(4).to("meta")))


def test_method_checks_before_it_touches_the_graph():
    """The method raises on bad arguments and on CPU tensors without a graph handle."""
    g = DynamicGraph.__new__(DynamicGraph)      # no native handle: nothing can be launched
    g._device = 0
    with pytest.raises(TypeError, match="nodes"):
        g.neighbor_sequence(**_args(nodes=torch.zeros(4, dtype=torch.int32)))
    with pytest.raises(TypeError, match="float32"):
        g.neighbor_sequence(**_args(edge_feats=torch.zeros(4, 4, dtype=torch.bfloat16)))
    with pytest.raises(ValueError, match="length"):
        g.neighbor_sequence(**_args(length=513))
    with pytest.raises(ValueError, match="the graph is on device"):
        g.neighbor_sequence(**_args())
    with pytest.raises(TypeError):
        g.neighbor_sequence(*_args().values())      # everything past ts is keyword-only


def test_native_entry_is_bound_and_rejects_a_null_graph():
    assert len(_capi.PROTOTYPES["gf_graph_neighbor_sequence"][1]) == 23
    lib = _capi.load()
    rc = lib.gf_graph_neighbor_sequence(None, None, None, None, 0, 1, None, 0, 0, None, 0, 0,
                                        None, None, 0, None, None, None, None, None, None, 0,
                                        None)
    assert rc == _capi.GF_ERR_INVALID_ARGUMENT
    assert b"null graph" in lib.gf_last_error()
