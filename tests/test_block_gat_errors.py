"""Error paths of ops.block_gat and of the gf_block_gat entry points.  ops.block_gat validates
every argument before it touches the device (or the block's segments), so all of this runs on
CPU tensors without a GPU."""
import ctypes
import os
import re

import pytest
import torch

from gnnflow_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Block:
    """What block_gat reads before it launches anything."""

    def __init__(self, num_src, num_dst, num_edges):
        self.n = (num_src, num_dst, num_edges)

    def num_src_nodes(self):
        return self.n[0]

    def num_dst_nodes(self):
        return self.n[1]

    def num_edges(self):
        return self.n[2]

    def segments(self):
        raise AssertionError("block_gat looked at the block's edges before validating")


B = _Block(12, 5, 20)


def _inputs(H=2, D=3, num_src=12, num_dst=5):
    return torch.zeros(num_src, H, D), torch.zeros(num_src, H), torch.zeros(num_dst, H)


def test_wrong_dtype():
    feat, el, er = _inputs()
    for bad in ((feat.double(), el, er), (feat, el.half(), er), (feat, el, er.to(torch.bfloat16)),
                (feat.long(), el, er)):
        with pytest.raises(TypeError, match="float32"):
            ops.block_gat(B, *bad)
    with pytest.raises(TypeError):
        ops.block_gat(B, feat.numpy(), el, er)


def test_wrong_ranks_and_rows():
    feat, el, er = _inputs()
    for bad in ((feat.reshape(12, 6), el, er), (feat, el.reshape(12, 2, 1), er),
                (feat, el, er.reshape(-1)), (feat[:, :, :, None], el, er)):
        with pytest.raises(ValueError, match="must be"):
            ops.block_gat(B, *bad)
    for bad in ((feat[:-1], el, er), (feat, el[:-1], er), (feat, el, er[:-1]),
                (feat, el, torch.zeros(12, 2))):
        with pytest.raises(ValueError, match="one row per"):
            ops.block_gat(B, *bad)


def test_mismatched_heads_and_widths():
    feat, el, er = _inputs()
    for bad in ((feat, el[:, :1], er), (feat, el, er[:, :1]), (feat[:, :1], el, er),
                (feat, torch.zeros(12, 3), torch.zeros(5, 3))):
        with pytest.raises(ValueError, match="differ in H"):
            ops.block_gat(B, *bad)
    with pytest.raises(ValueError, match="D >= 1"):
        ops.block_gat(B, torch.zeros(12, 2, 0), el, er)


def test_width_limit():
    assert ops.MAX_ATTENTION_WIDTH == 1024
    for H, D in ((1, 1025), (2, 513), (33, 32)):
        with pytest.raises(ValueError, match="limit"):
            ops.block_gat(B, *_inputs(H, D))


def test_dropout_p_and_seed():
    feat, el, er = _inputs()
    for p in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="dropout_p"):
            ops.block_gat(B, feat, el, er, dropout_p=p, dropout_seed=1)
    with pytest.raises(ValueError, match="rounds to 1"):
        ops.block_gat(B, feat, el, er, dropout_p=1.0 - 2.0 ** -30, dropout_seed=1)
    with pytest.raises(ValueError, match="needs a dropout_seed"):
        ops.block_gat(B, feat, el, er, dropout_p=0.5)
    for seed in (-1, 2 ** 64):
        with pytest.raises(ValueError, match="dropout_seed"):
            ops.block_gat(B, feat, el, er, dropout_p=0.5, dropout_seed=seed)
        with pytest.raises(ValueError, match="dropout_seed"):
            ops.block_gat(B, feat, el, er, dropout_seed=seed)


def test_valid_arguments_get_as_far_as_the_device_check():
    """Everything above passes: the last check is where the tensors live."""
    feat, el, er = _inputs()
    with pytest.raises(ValueError, match="runs on the GPU"):
        ops.block_gat(B, feat, el, er, dropout_p=0.5, dropout_seed=2 ** 64 - 1)
    with pytest.raises(ValueError, match="is on"):
        ops.block_gat(B, feat, el.to("meta"), er)


def test_symbols_in_header_and_capi():
    from gnnflow_amd import _capi
    text = open(os.path.join(ROOT, "include", "gnnflow_hip.h")).read()
    for name in ("gf_block_gat", "gf_block_gat_backward"):
        assert re.search(r"GF_API int {}\(".format(name), text)
        assert name in _capi.PROTOTYPES
    assert len(_capi.PROTOTYPES["gf_block_gat"][1]) == 18
    assert len(_capi.PROTOTYPES["gf_block_gat_backward"][1]) == 21


def test_entry_points_reject_bad_arguments_before_any_pointer():
    from gnnflow_amd import _build, _capi
    _build.build()
    lib = _capi.load()
    f = ctypes.c_float

    def fwd(H, D, p, num_src=0):
        return lib.gf_block_gat(None, 0, 0, None, num_src, H, D, None, None, None, f(0.2), f(p),
                                1, None, None, None, 0, None)

    def bwd(H, D, p, num_src=0):
        return lib.gf_block_gat_backward(None, 0, 0, None, num_src, H, D, None, None, None, None,
                                         None, f(0.2), f(p), 1, None, None, None, None, 0, None)

    for call in (fwd, bwd):
        for H, D in ((1, 1025), (1025, 1), (33, 32), (0, 4), (4, 0)):
            assert call(H, D, 0.0) == _capi.GF_ERR_INVALID_ARGUMENT, (H, D)
            assert b"block_gat" in lib.gf_last_error()
        for p in (1.0, -0.1, 1.5, float("nan")):
            assert call(2, 4, p) == _capi.GF_ERR_INVALID_ARGUMENT, p
            assert b"dropout" in lib.gf_last_error()
        # valid shapes and p get as far as the next check
        assert call(2, 4, 0.5) == _capi.GF_ERR_INVALID_ARGUMENT
        assert b"offsets" in lib.gf_last_error()
    # without col the source rows are the destinations followed by one row per edge
    off = (ctypes.c_int64 * 1)(0)
    rc = lib.gf_block_gat(off, 0, 0, None, 3, 2, 4, None, None, None, f(0.2), f(0.0), 1, None,
                          None, None, 0, None)
    assert rc == _capi.GF_ERR_INVALID_ARGUMENT and b"num_src" in lib.gf_last_error()
