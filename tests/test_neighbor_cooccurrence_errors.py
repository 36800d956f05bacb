"""CPU tests of the argument checks of DynamicGraph.neighbor_cooccurrence
(dynamic_graph.check_neighbor_cooccurrence_args) and of nn.NeighborCooccurrenceEncoder's own: every
TypeError and ValueError is raised before anything is allocated or launched and needs no device;
the native entry rejects a null graph with a status code; the Python limit is the header's."""
import os
import re

import numpy as np
import pytest
import torch

import gnnflow_amd
from gnnflow_amd import NeighborCooccurrence, NeighborCooccurrenceEncoder, _capi
from gnnflow_amd.dynamic_graph import (COOC_MAX_LENGTH, DynamicGraph,
                                       check_neighbor_cooccurrence_args)
from tests import neighbor_cooccurrence_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 2 ** 31


def _args(N=4, **over):
    a = dict(src=torch.zeros(N, dtype=torch.int64), dst=torch.ones(N, dtype=torch.int64),
             ts=torch.zeros(N, dtype=torch.float32), since=None, length=32, include_self=True)
    a.update(over)
    return a


def test_names_are_exported():
    assert {"NeighborCooccurrence", "NeighborCooccurrenceEncoder"} <= set(gnnflow_amd.__all__)
    assert gnnflow_amd.NeighborCooccurrence is NeighborCooccurrence
    assert NeighborCooccurrence._fields == R.FIELDS == ("lengths", "nodes", "eids", "times",
                                                        "counts")


def test_the_limit_is_the_headers():
    text = open(os.path.join(ROOT, "include", "gnnflow_hip.h")).read()
    assert int(re.search(r"#define GF_COOC_MAX_LENGTH (\d+)", text).group(1)) == COOC_MAX_LENGTH
    assert COOC_MAX_LENGTH == R.MAX_LENGTH == 512


def test_good_arguments_return_rows_length_and_self():
    assert check_neighbor_cooccurrence_args(**_args()) == (4, 32, 1)
    assert check_neighbor_cooccurrence_args(**_args(N=0)) == (0, 32, 1)
    assert check_neighbor_cooccurrence_args(**_args(include_self=False)) == (4, 32, 0)
    assert check_neighbor_cooccurrence_args(**_args(since=40.0)) == (4, 32, 1)
    assert check_neighbor_cooccurrence_args(**_args(since=float("nan"))) == (4, 32, 1)
    assert check_neighbor_cooccurrence_args(**_args(since=torch.zeros(4))) == (4, 32, 1)
    a = _args()
    assert check_neighbor_cooccurrence_args(a["src"], a["dst"], a["ts"]) == (4, 32, 1)
    assert check_neighbor_cooccurrence_args(**_args(length=np.int64(7))) == (4, 7, 1)


@pytest.mark.parametrize("L,self_slot", [(1, False), (2, True), (2, False), (512, True),
                                         (512, False)])
def test_lengths_that_are_legal(L, self_slot):
    assert check_neighbor_cooccurrence_args(**_args(length=L, include_self=self_slot)) == \
        (4, L, int(self_slot))


@pytest.mark.parametrize("self_slot", [False, True])
@pytest.mark.parametrize("L", [0, 513, -1])
def test_length_out_of_range(L, self_slot):
    with pytest.raises(ValueError, match="length must be in"):
        check_neighbor_cooccurrence_args(**_args(length=L, include_self=self_slot))


def test_length_one_has_no_room_beside_the_self_slot():
    """length - include_self bounds the window, and a bound of 0 would read as "no bound"."""
    with pytest.raises(ValueError, match="length must be in \\[2, 513\\), got 1"):
        check_neighbor_cooccurrence_args(**_args(length=1, include_self=True))
    with pytest.raises(ValueError, match="length must be in \\[2, 513\\), got 1"):
        check_neighbor_cooccurrence_args(**_args(length=1))      # the default is True


@pytest.mark.parametrize("bad", [True, False, 1.0, None, "3", np.float32(2)])
def test_length_must_be_an_int(bad):
    with pytest.raises(TypeError, match="length must be an int"):
        check_neighbor_cooccurrence_args(**_args(length=bad))


@pytest.mark.parametrize("bad", [1, 0, None, "yes", 1.0, np.bool_(True)])
def test_include_self_must_be_a_bool(bad):
    with pytest.raises(TypeError, match="include_self must be a bool"):
        check_neighbor_cooccurrence_args(**_args(include_self=bad))


@pytest.mark.parametrize("name", ["src", "dst", "ts"])
def test_not_a_tensor(name):
    with pytest.raises(TypeError, match=name):
        check_neighbor_cooccurrence_args(**_args(**{name: np.zeros(4)}))
    with pytest.raises(TypeError, match=name):
        check_neighbor_cooccurrence_args(**_args(**{name: [0, 1, 2, 3]}))


@pytest.mark.parametrize("name,bad", [("src", torch.int32), ("src", torch.float32),
                                      ("dst", torch.int32), ("dst", torch.float32),
                                      ("ts", torch.float64), ("ts", torch.int64),
                                      ("since", torch.float64), ("since", torch.int64)])
def test_wrong_dtype(name, bad):
    with pytest.raises(TypeError, match=name):
        check_neighbor_cooccurrence_args(**_args(**{name: torch.zeros(4, dtype=bad)}))


@pytest.mark.parametrize("bad", [True, "3", [0.0] * 4, np.zeros(4, np.float32), (1.0,)])
def test_since_must_be_none_a_float_or_a_tensor(bad):
    with pytest.raises(TypeError, match="since"):
        check_neighbor_cooccurrence_args(**_args(since=bad))


@pytest.mark.parametrize("name", ["src", "dst", "ts", "since"])
def test_not_one_dimensional(name):
    good = _args(since=torch.zeros(4))[name]
    with pytest.raises(ValueError, match=name + " must be 1-D"):
        check_neighbor_cooccurrence_args(**_args(**{name: good.reshape(-1, 1)}))
    with pytest.raises(ValueError, match=name + " must be 1-D"):
        check_neighbor_cooccurrence_args(**_args(**{name: good[0]}))


@pytest.mark.parametrize("name,dtype", [("dst", torch.int64), ("ts", torch.float32),
                                        ("since", torch.float32)])
def test_lengths_differ(name, dtype):
    with pytest.raises(ValueError, match="src has 4 rows, {} has 3".format(name)):
        check_neighbor_cooccurrence_args(**_args(**{name: torch.zeros(3, dtype=dtype)}))


def test_too_many_rows():
    # 2^31 rows without their 16 GiB: a zero-stride view has the shape and no storage
    i64 = torch.zeros(1, dtype=torch.int64).expand(BIG)
    f32 = torch.zeros(1, dtype=torch.float32).expand(BIG)
    with pytest.raises(ValueError, match="neighbor_cooccurrence takes fewer than 2\\*\\*31 rows"):
        check_neighbor_cooccurrence_args(i64, i64, f32)
    n = BIG - 1
    assert check_neighbor_cooccurrence_args(i64[:n], i64[:n], f32[:n], f32[:n])[0] == n


@pytest.mark.parametrize("name,dtype", [("dst", torch.int64), ("ts", torch.float32),
                                        ("since", torch.float32)])
def test_devices_differ(name, dtype):
    with pytest.raises(ValueError, match=name + " is on meta"):
        check_neighbor_cooccurrence_args(
            **_args(**{name: torch.zeros(4, dtype=dtype, device="meta")}))


# which error wins when two arguments are wrong: common_neighbors' order -- the tensors' types and
# since's, include_self's type, length's type and then its range, 1-D, equal rows, 2**31 rows,
# devices
ORDER = [
    (dict(dst=torch.zeros(4, dtype=torch.int32), include_self=1), TypeError,
     "dst must be torch.int64"),
    (dict(since=(1.0,), include_self=None), TypeError, "since must be None, a float or"),
    (dict(include_self=1, length=1.0), TypeError, "include_self must be a bool"),
    (dict(length=None, src=torch.zeros((2, 2), dtype=torch.int64)), TypeError,
     "length must be an int"),
    (dict(length=513, src=torch.zeros((2, 2), dtype=torch.int64)), ValueError,
     "length must be in \\[2, 513\\)"),
    (dict(length=0, include_self=False, ts=torch.zeros(3)), ValueError,
     "length must be in \\[1, 513\\)"),
    (dict(ts=torch.zeros((2, 2)), dst=torch.zeros(3, dtype=torch.int64)), ValueError,
     "ts must be 1-D"),
    (dict(dst=torch.zeros(3, dtype=torch.int64), ts=torch.zeros(4, device="meta")), ValueError,
     "src has 4 rows, dst has 3"),
    (dict(src=torch.zeros(1, dtype=torch.int64).expand(BIG),
          dst=torch.zeros(1, dtype=torch.int64).expand(BIG),
          ts=torch.zeros(1, device="meta").expand(BIG)), ValueError,
     "neighbor_cooccurrence takes fewer than 2\\*\\*31 rows"),
    (dict(ts=torch.zeros(4, device="meta"), since=torch.zeros(4, device="meta")), ValueError,
     "ts is on meta, src on"),
]


@pytest.mark.parametrize("case", range(len(ORDER)))
def test_the_earlier_check_wins(case):
    faults, exc, message = ORDER[case]
    with pytest.raises(exc, match="^" + message):
        check_neighbor_cooccurrence_args(**_args(**faults))


def test_method_checks_before_it_touches_the_graph():
    """The method raises on bad arguments and on CPU tensors without a graph handle."""
    g = DynamicGraph.__new__(DynamicGraph)      # no native handle: nothing can be launched
    g._device = 0
    with pytest.raises(TypeError, match="src"):
        g.neighbor_cooccurrence(**_args(src=torch.zeros(4, dtype=torch.int32)))
    with pytest.raises(TypeError, match="since"):
        g.neighbor_cooccurrence(**_args(since="yesterday"))
    with pytest.raises(ValueError, match="length"):
        g.neighbor_cooccurrence(**_args(length=1))
    with pytest.raises(TypeError, match="include_self"):
        g.neighbor_cooccurrence(**_args(include_self=1))
    with pytest.raises(ValueError, match="the graph is on device"):
        g.neighbor_cooccurrence(**_args())
    with pytest.raises(TypeError):
        g.neighbor_cooccurrence(*_args().values())      # since and the rest are keyword-only


def test_native_entry_is_bound_and_rejects_a_null_graph():
    assert len(_capi.PROTOTYPES["gf_graph_neighbor_cooccurrence"][1]) == 15
    lib = _capi.load()
    rc = lib.gf_graph_neighbor_cooccurrence(None, None, None, None, None, 0, 32, 1, None, None,
                                            None, None, None, 0, None)
    assert rc == _capi.GF_ERR_INVALID_ARGUMENT
    assert b"null graph" in lib.gf_last_error()


# ---- the encoder: plain torch, so its shapes and its checks run here -------------------------

def test_encoder_shapes_padding_and_checks():
    torch.manual_seed(0)
    enc = NeighborCooccurrenceEncoder(6)
    counts = torch.randint(0, 6, (3, 2, 5, 2), dtype=torch.int32)
    lengths = torch.tensor([[5, 0], [2, 3], [1, 5]], dtype=torch.int32)
    out = enc(counts, lengths)
    assert out.dtype == torch.float32 and tuple(out.shape) == (3, 2, 5, 6)
    assert (out[0, 1] == 0).all() and (out[1, 0, 2:] == 0).all() and (out[2, 0, 1:] == 0).all()
    assert (out[0, 0] != 0).any(1).all() and tuple(enc.table(5).shape) == (6, 6)
    same =NeighborCooccurrenceEncoder(6, max_count=9)
    same.load_state_dict(enc.state_dict())
    # a larger table, the same rows of it (another GEMM shape: to rounding)
    assert torch.allclose(same(counts, lengths), out, rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError, match="counts must be"):
        enc(counts[..., 0], lengths)
    with pytest.raises(ValueError, match="lengths must be"):
        enc(counts, lengths[:2])
    with pytest.raises(ValueError, match="max_count is 4"):
        NeighborCooccurrenceEncoder(6, max_count=4)(counts, lengths)
    for bad in (0, -1, True, 2.0):
        with pytest.raises(ValueError, match="max_count"):
            NeighborCooccurrenceEncoder(6, max_count=bad)
