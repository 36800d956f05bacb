"""CPU tests of ops.edge_rank's argument checks: every TypeError and ValueError is raised before
any native call, the constants equal the header's and the entry points are declared on both
sides of the C boundary."""
import re

import pytest
import torch

from gnnflow_amd import _capi, ops
from tests import edge_rank_ref as R


@pytest.fixture(autouse=True)
def no_native_call(monkeypatch):
    def refuse():
        raise AssertionError("the checks must come before the native library is loaded")
    monkeypatch.setattr(_capi, "load", refuse)


def _args(B=4, C=6, D=8, **over):
    a = dict(src=torch.zeros(B, D), cand=torch.zeros(C, D), weight=torch.zeros(D),
             bias=torch.zeros(1))
    a.update(over)
    return a


@pytest.mark.parametrize("name", ["src", "cand", "weight", "bias", "ref_score", "skip"])
def test_non_tensors_are_refused(name):
    with pytest.raises(TypeError, match=name):
        ops.edge_rank(**_args(**{name: [0.0]}))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float16])
@pytest.mark.parametrize("name", ["src", "cand", "weight", "bias", "ref_score"])
def test_only_float32_is_taken(name, dtype):
    a = _args(ref_score=torch.zeros(4))
    a[name] = a[name].to(dtype)
    with pytest.raises(TypeError, match="float32"):
        ops.edge_rank(**a)


def test_skip_must_be_int64():
    with pytest.raises(TypeError, match="int64"):
        ops.edge_rank(**_args(skip=torch.zeros(4, dtype=torch.int32)))
    with pytest.raises(TypeError, match="k must be an int"):
        ops.edge_rank(**_args(), k=1.0)


@pytest.mark.parametrize("over", [
    dict(src=torch.zeros(4)), dict(cand=torch.zeros(6, 8, 1)), dict(cand=torch.zeros(6, 7)),
    dict(src=torch.zeros(4, 0), cand=torch.zeros(6, 0), weight=torch.zeros(0)),
    dict(cand=torch.zeros(0, 8)), dict(weight=torch.zeros(7)), dict(weight=torch.zeros(8, 1)),
    dict(bias=torch.zeros(2)), dict(bias=torch.zeros(())), dict(ref_score=torch.zeros(5)),
    dict(ref_score=torch.zeros(4, 2)), dict(skip=torch.zeros(5, dtype=torch.int64)),
    dict(skip=torch.zeros(4, 1, dtype=torch.int64)),
])
def test_bad_shapes_are_refused(over):
    with pytest.raises(ValueError):
        ops.edge_rank(**_args(**over))


@pytest.mark.parametrize("C,k", [(6, -1), (6, 7), (100, 65), (1, 2)])
def test_k_out_of_range(C, k):
    with pytest.raises(ValueError, match="k must be"):
        ops.edge_rank(**_args(C=C), k=k)


def test_too_many_candidates():
    cand = torch.empty(2 ** 31, 1, device="meta")
    a = dict(src=torch.empty(1, 1, device="meta"), cand=cand,
             weight=torch.empty(1, device="meta"), bias=torch.empty(1, device="meta"))
    with pytest.raises(ValueError, match="2\\*\\*31"):
        ops.edge_rank(**a)


@pytest.mark.parametrize("name", ["cand", "weight", "bias", "ref_score", "skip"])
def test_devices_must_agree(name):
    a = _args(ref_score=torch.zeros(4), skip=torch.zeros(4, dtype=torch.int64))
    a[name] = a[name].to("meta")
    with pytest.raises(ValueError, match=name + " is on meta"):
        ops.edge_rank(**a)


def test_the_cpu_is_refused_last():
    with pytest.raises(ValueError, match="runs on the GPU"):
        ops.edge_rank(**_args(), k=3, ref_score=torch.zeros(4),
                      skip=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="runs on the GPU"):      # skip without ref_score
        ops.edge_rank(**_args(), k=3, skip=torch.zeros(4, dtype=torch.int64))


def test_constants_and_symbols():
    assert ops.EDGE_RANK_MAX_K == R.header_constant("GF_EDGE_RANK_MAX_K") == 64
    assert ops.EDGE_RANK_CHUNK == R.header_constant("GF_EDGE_RANK_CHUNK")
    header = open(R._HEADER).read()
    for sym in ("gf_edge_rank_scratch", "gf_edge_rank"):
        assert re.search(r"GF_API int {}\(".format(sym), header)
        assert sym in _capi.PROTOTYPES
    assert len(_capi.PROTOTYPES["gf_edge_rank"][1]) == 18
    assert len(_capi.PROTOTYPES["gf_edge_rank_scratch"][1]) == 4


def test_edge_rank_result_type():
    r = ops.EdgeRank(torch.zeros(2, 0), torch.zeros(2, 0, dtype=torch.int64), None, None)
    assert r.rank is None and r._fields == ("values", "indices", "greater", "equal")
    r = ops.EdgeRank(r.values, r.indices, torch.tensor([0, 3]), torch.tensor([1, 2]))
    assert r.rank.dtype == torch.float64 and r.rank.tolist() == [1.5, 5.0]
