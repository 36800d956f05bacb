"""CPU tests of DynamicGraph.pair_sequence's argument checks
(dynamic_graph.check_pair_sequence_args): every TypeError and ValueError is raised before
anything is launched or allocated and needs no device; and gf_graph_pair_sequence rejects a
null graph with a status code."""
import numpy as np
import pytest
import torch

import gnnflow_amd
from gnnflow_amd import PairSequence, _capi
from gnnflow_amd.dynamic_graph import (PAIRSEQ_MAX_LENGTH, PAIRSEQ_MAX_WIDTH, DynamicGraph,
                                       check_pair_sequence_args)
from gnnflow_amd.nn import FixedTimeEncode, TimeEncode


def _args(N=4, **over):
    a = dict(src=torch.zeros(N, dtype=torch.int64), dst=torch.zeros(N, dtype=torch.int64),
             ts=torch.zeros(N, dtype=torch.float32), since=None, length=32,
             node_feats=None, edge_feats=torch.zeros(10, 8), time_encoder=None)
    a.update(over)
    return a


def _pair(dT=6):
    return torch.zeros(dT, 1), torch.zeros(dT)


def test_names_are_exported():
    assert "PairSequence" in gnnflow_amd.__all__
    assert gnnflow_amd.PairSequence is PairSequence
    assert PairSequence._fields == ("lengths", "nodes", "eids", "times", "delta_t", "counts",
                                    "node", "edge", "time")
    assert PAIRSEQ_MAX_LENGTH == 512 and PAIRSEQ_MAX_WIDTH == 1024
    from gnnflow_amd import models
    assert "DyGFormer" in models.__all__ and models.DyGFormer.__name__ == "DyGFormer"
    assert callable(models.DyGFormer.forward_parts) and callable(models.DyGFormer.forward_graph)
    assert callable(DynamicGraph.pair_sequence)


def test_good_arguments_return_the_rows_the_length_and_the_widths():
    assert check_pair_sequence_args(**_args()) == (4, 32, 0, 8, 0)
    assert check_pair_sequence_args(**_args(N=0)) == (0, 32, 0, 8, 0)
    assert check_pair_sequence_args(**_args(edge_feats=None)) == (4, 32, 0, 0, 0)
    assert check_pair_sequence_args(**_args(node_feats=torch.zeros(3, 5))) == (4, 32, 5, 8, 0)
    assert check_pair_sequence_args(
        **_args(edge_feats=None, node_feats=torch.zeros(3, 1))) == (4, 32, 1, 0, 0)
    assert check_pair_sequence_args(
        **_args(edge_feats=torch.zeros(2, 1024), length=512)) == (4, 512, 0, 1024, 0)
    assert check_pair_sequence_args(**_args(length=2)) == (4, 2, 0, 8, 0)
    assert check_pair_sequence_args(**_args(length=np.int64(7))) == (4, 7, 0, 8, 0)
    for since in (40.0, float("nan"), 3, torch.zeros(4)):
        assert check_pair_sequence_args(**_args(since=since)) == (4, 32, 0, 8, 0)
    a = _args()
    assert check_pair_sequence_args(a["src"], a["dst"], a["ts"]) == (4, 32, 0, 0, 0)
    # a row slice of a table is contiguous and is taken as it is
    assert check_pair_sequence_args(
        **_args(edge_feats=torch.zeros(10, 8)[2:7])) == (4, 32, 0, 8, 0)


def test_every_form_of_time_encoder():
    assert check_pair_sequence_args(**_args(time_encoder=_pair())) == (4, 32, 0, 8, 6)
    assert check_pair_sequence_args(**_args(time_encoder=list(_pair(1)))) == (4, 32, 0, 8, 1)
    assert check_pair_sequence_args(
        **_args(time_encoder=(torch.zeros(6), torch.zeros(6)))) == (4, 32, 0, 8, 6)
    assert check_pair_sequence_args(
        **_args(edge_feats=None, time_encoder=FixedTimeEncode(100))) == (4, 32, 0, 0, 100)
    assert check_pair_sequence_args(
        **_args(node_feats=torch.zeros(2, 3), time_encoder=TimeEncode(4))) == (4, 32, 3, 8, 4)
    assert check_pair_sequence_args(**_args(time_encoder=_pair(1024))) == (4, 32, 0, 8, 1024)


@pytest.mark.parametrize("name", ["src", "dst", "ts", "edge_feats", "node_feats"])
def test_not_a_tensor(name):
    with pytest.raises(TypeError, match=name + " must be a tensor"):
        check_pair_sequence_args(**_args(**{name: np.zeros((4, 4), np.float32)}))
    with pytest.raises(TypeError, match=name + " must be a tensor"):
        check_pair_sequence_args(**_args(**{name: [0, 1, 2, 3]}))


@pytest.mark.parametrize("name,bad", [("src", torch.int32), ("dst", torch.float32),
                                      ("ts", torch.float64), ("ts", torch.int64),
                                      ("since", torch.float64), ("since", torch.int64)])
def test_wrong_dtype(name, bad):
    with pytest.raises(TypeError, match=name + " must be torch"):
        check_pair_sequence_args(**_args(**{name: torch.zeros(4, dtype=bad)}))


@pytest.mark.parametrize("name", ["edge_feats", "node_feats"])
@pytest.mark.parametrize("bad", [torch.float16, torch.bfloat16, torch.float64, torch.int64])
def test_tables_are_float32_and_the_message_says_so(name, bad):
    with pytest.raises(TypeError, match=name + ".*float32"):
        check_pair_sequence_args(**_args(**{name: torch.zeros(4, 8, dtype=bad)}))


@pytest.mark.parametrize("bad", [torch.float16, torch.bfloat16])
def test_half_precision_tables_are_named_as_unsupported(bad):
    with pytest.raises(TypeError, match="half-precision tables are not supported"):
        check_pair_sequence_args(**_args(node_feats=torch.zeros(4, 8, dtype=bad)))


@pytest.mark.parametrize("bad", [True, "3", [0.0] * 4, np.zeros(4, np.float32), (1.0,)])
def test_since_must_be_none_a_float_or_a_tensor(bad):
    with pytest.raises(TypeError, match="since must be None, a float or a tensor"):
        check_pair_sequence_args(**_args(since=bad))


@pytest.mark.parametrize("bad", [True, False, 1.0, None, "3", np.float32(2)])
def test_length_must_be_an_int(bad):
    with pytest.raises(TypeError, match="length must be an int"):
        check_pair_sequence_args(**_args(length=bad))


@pytest.mark.parametrize("bad", [1, 0, -1, PAIRSEQ_MAX_LENGTH + 1, 4096])
def test_length_outside_2_to_512(bad):
    with pytest.raises(ValueError, match="length must be in \\[2, 513\\)"):
        check_pair_sequence_args(**_args(length=bad))


@pytest.mark.parametrize("bad", [3, "cos", torch.zeros(4), (torch.zeros(4, 1),),
                                 (torch.zeros(4, 1), torch.zeros(4), torch.zeros(4)),
                                 torch.nn.ReLU()])
def test_time_encoder_must_hold_a_weight_and_a_bias(bad):
    with pytest.raises(TypeError, match="time_encoder must be a module"):
        check_pair_sequence_args(**_args(time_encoder=bad))


@pytest.mark.parametrize("which", [0, 1])
def test_time_encoder_tensors_are_float32_tensors(which):
    for bad in (np.zeros(6, np.float32), None, torch.zeros(6, dtype=torch.float64),
                torch.zeros(6, dtype=torch.bfloat16)):
        pair = list(_pair())
        pair[which] = bad
        with pytest.raises(TypeError, match="time_encoder's " + ("weight", "bias")[which]):
            check_pair_sequence_args(**_args(time_encoder=tuple(pair)))


def test_time_encoder_shapes():
    for weight, bias in ((torch.zeros(6, 1), torch.zeros(5)), (torch.zeros(5), torch.zeros(6)),
                         (torch.zeros(1, 6), torch.zeros(6)), (torch.zeros(6, 2), torch.zeros(6)),
                         (torch.zeros(6, 1, 1), torch.zeros(6))):
        with pytest.raises(ValueError, match="time_encoder's weight must be \\[dT, 1\\] or \\[dT\\]"):
            check_pair_sequence_args(**_args(time_encoder=(weight, bias)))
    for bias in (torch.zeros(6, 1), torch.zeros(())):
        with pytest.raises(ValueError, match="time_encoder's bias must be \\[dT\\]"):
            check_pair_sequence_args(**_args(time_encoder=(torch.zeros(6, 1), bias)))
    for dT in (0, PAIRSEQ_MAX_WIDTH + 1):
        with pytest.raises(ValueError, match="time_encoder must have 1 to 1024 columns"):
            check_pair_sequence_args(**_args(time_encoder=_pair(dT)))


@pytest.mark.parametrize("name", ["src", "dst", "ts", "since"])
def test_not_one_dimensional(name):
    good = _args(since=torch.zeros(4))[name]
    with pytest.raises(ValueError, match=name + " must be 1-D"):
        check_pair_sequence_args(**_args(**{name: good.reshape(-1, 1)}))
    with pytest.raises(ValueError, match=name + " must be 1-D"):
        check_pair_sequence_args(**_args(**{name: good[0]}))


@pytest.mark.parametrize("name,dtype", [("dst", torch.int64), ("ts", torch.float32),
                                        ("since", torch.float32)])
def test_lengths_differ(name, dtype):
    with pytest.raises(ValueError, match="src has 4 rows, {} has 3".format(name)):
        check_pair_sequence_args(**_args(**{name: torch.zeros(3, dtype=dtype)}))


def test_too_many_rows():
    i64 = torch.zeros(1, dtype=torch.int64).expand(2 ** 31)
    f32 = torch.zeros(1, dtype=torch.float32).expand(2 ** 31)
    with pytest.raises(ValueError, match="pair_sequence takes fewer than 2\\*\\*31 rows"):
        check_pair_sequence_args(i64, i64, f32)
    n = 2 ** 31 - 1
    assert check_pair_sequence_args(i64[:n], i64[:n], f32[:n], length=2) == (n, 2, 0, 0, 0)


@pytest.mark.parametrize("name", ["edge_feats", "node_feats"])
def test_table_shapes(name):
    for bad in (torch.zeros(8), torch.zeros(2, 3, 4), torch.zeros(())):
        with pytest.raises(ValueError, match=name + " must be 2-D"):
            check_pair_sequence_args(**_args(**{name: bad}))
    with pytest.raises(ValueError, match=name + " has no rows"):
        check_pair_sequence_args(**_args(**{name: torch.zeros(0, 4)}))
    for width in (0, PAIRSEQ_MAX_WIDTH + 1, 4096):
        with pytest.raises(ValueError, match=name + " must have 1 to 1024 columns"):
            check_pair_sequence_args(**_args(**{name: torch.zeros(2, width)}))


@pytest.mark.parametrize("name", ["edge_feats", "node_feats"])
def test_a_table_that_is_not_contiguous_is_not_copied(name):
    for bad in (torch.zeros(8, 10).t(), torch.zeros(10, 16)[:, :8], torch.zeros(10, 8)[::2]):
        assert not bad.is_contiguous()
        with pytest.raises(ValueError, match=name + " must be contiguous"):
            check_pair_sequence_args(**_args(**{name: bad}))


@pytest.mark.parametrize("name,shape,dtype", [
    ("dst", (4,), torch.int64), ("ts", (4,), torch.float32), ("since", (4,), torch.float32),
    ("edge_feats", (10, 8), torch.float32), ("node_feats", (10, 8), torch.float32)])
def test_devices_differ(name, shape, dtype):
    with pytest.raises(ValueError, match=name + " is on meta"):
        check_pair_sequence_args(**_args(**{name: torch.zeros(shape, dtype=dtype,
                                                              device="meta")}))


def test_the_encoder_is_on_the_rows_device():
    weight, bias = _pair()
    with pytest.raises(ValueError, match="time_encoder's weight is on meta"):
        check_pair_sequence_args(**_args(time_encoder=(weight.to("meta"), bias)))
    with pytest.raises(ValueError, match="time_encoder's bias is on meta"):
        check_pair_sequence_args(**_args(time_encoder=(weight, bias.to("meta"))))
    with pytest.raises(ValueError, match="is on meta"):
        check_pair_sequence_args(**_args(time_encoder=FixedTimeEncode(4).to("meta")))


def test_type_errors_come_before_value_errors():
    with pytest.raises(TypeError, match="ts must be"):
        check_pair_sequence_args(**_args(ts=torch.zeros(3, dtype=torch.float64), length=1))
    with pytest.raises(ValueError, match="length"):      # then length, then the rows
        check_pair_sequence_args(**_args(ts=torch.zeros(3), length=1))


def test_method_checks_before_it_touches_the_graph():
    """The method raises on bad arguments and on CPU tensors without a graph handle."""
    g = DynamicGraph.__new__(DynamicGraph)      # no native handle: nothing can be launched
    g._device = 0
    with pytest.raises(TypeError, match="src"):
        g.pair_sequence(**_args(src=torch.zeros(4, dtype=torch.int32)))
    with pytest.raises(TypeError, match="float32"):
        g.pair_sequence(**_args(edge_feats=torch.zeros(4, 4, dtype=torch.bfloat16)))
    with pytest.raises(ValueError, match="length"):
        g.pair_sequence(**_args(length=513))
    with pytest.raises(ValueError, match="the graph is on device"):
        g.pair_sequence(**_args())
    with pytest.raises(TypeError):
        g.pair_sequence(*_args().values())      # everything past ts is keyword-only


def test_native_entry_is_bound_and_rejects_a_null_graph():
    assert len(_capi.PROTOTYPES["gf_graph_pair_sequence"][1]) == 27
    lib = _capi.load()
    rc = lib.gf_graph_pair_sequence(None, None, None, None, None, 0, 2, None, 0, 0, None, 0, 0,
                                    None, None, 0, None, None, None, None, None, None, None,
                                    None, None, 0, None)
    assert rc == _capi.GF_ERR_INVALID_ARGUMENT
    assert b"null graph" in lib.gf_last_error()
