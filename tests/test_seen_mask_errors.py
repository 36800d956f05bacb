"""CPU tests of DynamicGraph.seen_mask's argument checks (dynamic_graph.check_seen_mask_args):
every TypeError and ValueError is raised before anything is launched and needs no device; and
gf_graph_seen_mask rejects a null graph with a status code."""
import numpy as np
import pytest
import torch

from gnnflow_amd import _capi
from gnnflow_amd.dynamic_graph import DynamicGraph, check_seen_mask_args


def _args(B=4, C=5, **over):
    a = dict(src=torch.zeros(B, dtype=torch.int64), ts=torch.zeros(B, dtype=torch.float32),
             cand_ids=torch.arange(C, dtype=torch.int64), max_history=0)
    a.update(over)
    return a


def test_good_arguments_return_the_sizes():
    assert check_seen_mask_args(**_args()) == (4, 5)
    assert check_seen_mask_args(**_args(B=0)) == (0, 5)
    assert check_seen_mask_args(**_args(max_history=7)) == (4, 5)
    a = _args()
    assert check_seen_mask_args(a["src"], a["ts"], a["cand_ids"]) == (4, 5)


@pytest.mark.parametrize("name", ["src", "ts", "cand_ids"])
def test_not_a_tensor(name):
    with pytest.raises(TypeError, match=name):
        check_seen_mask_args(**_args(**{name: np.zeros(4)}))
    with pytest.raises(TypeError, match=name):
        check_seen_mask_args(**_args(**{name: [0, 1, 2, 3]}))


@pytest.mark.parametrize("name,bad", [("src", torch.int32), ("src", torch.float32),
                                      ("ts", torch.float64), ("ts", torch.int64),
                                      ("cand_ids", torch.int32), ("cand_ids", torch.float32)])
def test_wrong_dtype(name, bad):
    with pytest.raises(TypeError, match=name):
        check_seen_mask_args(**_args(**{name: torch.zeros(4, dtype=bad)}))


@pytest.mark.parametrize("bad", [True, False, 1.0, None, "3", np.float32(2)])
def test_max_history_must_be_an_int(bad):
    with pytest.raises(TypeError, match="max_history"):
        check_seen_mask_args(**_args(max_history=bad))


def test_negative_max_history():
    with pytest.raises(ValueError, match="max_history"):
        check_seen_mask_args(**_args(max_history=-1))


@pytest.mark.parametrize("name", ["src", "ts", "cand_ids"])
def test_not_one_dimensional(name):
    good = _args()[name]
    with pytest.raises(ValueError, match=name):
        check_seen_mask_args(**_args(**{name: good.reshape(-1, 1)}))
    with pytest.raises(ValueError, match=name):
        check_seen_mask_args(**_args(**{name: good[0]}))


def test_lengths_differ():
    with pytest.raises(ValueError, match="ts"):
        check_seen_mask_args(**_args(ts=torch.zeros(3)))


def test_no_candidates():
    with pytest.raises(ValueError, match="candidate"):
        check_seen_mask_args(**_args(C=0))


def test_too_many_candidates():
    # 2^31 ids without their 16 GiB: a zero-stride view has the shape and no storage
    huge = torch.zeros(1, dtype=torch.int64).expand(2 ** 31)
    with pytest.raises(ValueError, match="2\\*\\*31"):
        check_seen_mask_args(**_args(cand_ids=huge))
    assert check_seen_mask_args(**_args(cand_ids=huge[:2 ** 31 - 1])) == (4, 2 ** 31 - 1)


def test_devices_differ():
    with pytest.raises(ValueError, match="cand_ids is on meta"):
        check_seen_mask_args(**_args(cand_ids=torch.zeros(5, dtype=torch.int64, device="meta")))


def test_method_checks_before_it_touches_the_graph():
    """The method raises on bad arguments and on CPU tensors without a graph handle."""
    g = DynamicGraph.__new__(DynamicGraph)      # no native handle: nothing can be launched
    g._device = 0
    with pytest.raises(TypeError, match="src"):
        g.seen_mask(**_args(src=torch.zeros(4, dtype=torch.int32)))
    with pytest.raises(ValueError, match="candidate"):
        g.seen_mask(**_args(C=0))
    with pytest.raises(ValueError, match="the graph is on device"):
        g.seen_mask(**_args())


def test_native_entry_is_bound_and_rejects_a_null_graph():
    assert len(_capi.PROTOTYPES["gf_graph_seen_mask"][1]) == 11
    lib = _capi.load()
    rc = lib.gf_graph_seen_mask(None, None, None, 0, None, None, 1, 0, None, 0, None)
    assert rc == _capi.GF_ERR_INVALID_ARGUMENT
    assert b"null graph" in lib.gf_last_error()
