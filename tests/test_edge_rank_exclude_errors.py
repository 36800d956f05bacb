"""CPU tests of ops.edge_rank's checks of `exclude`: the TypeError and the ValueErrors are raised
where the other shape and type errors are, before the inputs are asked to be on a GPU."""
import numpy as np
import pytest
import torch

from gnnflow_amd import _capi, ops
from tests import edge_rank_ref as R


def _args(B=4, C=70, D=8):
    inp = R.make_grid((B, C, D))
    return {n: torch.from_numpy(inp[n]) for n in ("src", "cand", "w", "bias")} | \
        {"weight": torch.from_numpy(inp["w"])}


def _call(exclude, B=4, C=70, **kw):
    a = _args(B, C)
    return ops.edge_rank(a["src"], a["cand"], a["weight"], a["bias"], k=3, exclude=exclude, **kw)


def test_not_a_tensor():
    with pytest.raises(TypeError, match="exclude"):
        _call(np.zeros((4, 2), np.int64))


@pytest.mark.parametrize("bad", [torch.int32, torch.uint8, torch.bool, torch.float32])
def test_wrong_dtype(bad):
    with pytest.raises(TypeError, match="exclude must be int64"):
        _call(torch.zeros((4, 2), dtype=bad))


@pytest.mark.parametrize("shape", [(4, 1), (4, 3), (4, 70)], ids=str)
def test_wrong_number_of_words(shape):
    with pytest.raises(ValueError, match="exclude must be"):
        _call(torch.zeros(shape, dtype=torch.int64))


@pytest.mark.parametrize("rows", [3, 5, 0])
def test_wrong_number_of_rows(rows):
    with pytest.raises(ValueError, match="exclude must be"):
        _call(torch.zeros((rows, 2), dtype=torch.int64))


def test_one_dimensional():
    with pytest.raises(ValueError, match="exclude must be"):
        _call(torch.zeros(8, dtype=torch.int64))
    with pytest.raises(ValueError, match="exclude must be"):
        _call(torch.zeros(2, dtype=torch.int64), B=1)


def test_a_good_mask_reaches_the_gpu_check():
    """Nothing about a well-formed exclude is refused: the call gets as far as every well-formed
    call on CPU tensors does."""
    with pytest.raises(ValueError, match="runs on the GPU"):
        _call(torch.zeros((4, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="runs on the GPU"):
        _call(torch.zeros((4, 2), dtype=torch.int64), skip=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="runs on the GPU"):
        _call(torch.zeros((4, 1), dtype=torch.int64), C=64)


def test_device_mismatch():
    with pytest.raises(ValueError, match="exclude is on meta"):
        _call(torch.zeros((4, 2), dtype=torch.int64, device="meta"))


def test_native_entries():
    lib = _capi.load()
    assert hasattr(lib, "gf_edge_rank_masked")
    # gf_edge_rank's argument list plus the mask; gf_edge_rank itself keeps its prototype
    assert len(_capi.PROTOTYPES["gf_edge_rank_masked"][1]) == 19
    assert len(_capi.PROTOTYPES["gf_edge_rank"][1]) == 18
    assert len(_capi.PROTOTYPES["gf_edge_rank_scratch"][1]) == 4
