"""Dtype errors of the ops that take bfloat16 (block_attention, time_encode_cat, edge_score): a
mixture of float32 and bfloat16, float16, and an out_dtype other than float32 / bfloat16 are
refused before the device, the block's segments or the native library are touched, so all of
this runs on CPU tensors without a GPU."""
import os
import re

import pytest
import torch

from gnnflow_amd import _capi, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


class _Block:
    """What block_attention reads before it launches anything."""

    def num_dst_nodes(self):
        return 5

    def num_edges(self):
        return 20

    def segments(self):
        raise AssertionError("block_attention looked at the block's edges before validating")


@pytest.fixture(autouse=True)
def no_native_call(monkeypatch):
    def load():
        raise AssertionError("the native library was touched")
    monkeypatch.setattr(_capi, "load", load)


def _qkv(*dtypes):
    shapes = ((5, 2, 3), (20, 2, 3), (20, 2, 3))
    return [torch.zeros(s, dtype=d) for s, d in zip(shapes, dtypes)]


@pytest.mark.parametrize("dtypes", [(F32, BF16, BF16), (BF16, F32, BF16), (BF16, BF16, F32),
                                    (F32, F32, BF16)])
def test_block_attention_mixture_names_the_three_dtypes(dtypes):
    with pytest.raises(TypeError) as e:
        ops.block_attention(_Block(), *_qkv(*dtypes))
    for d in dtypes:
        assert str(d) in str(e.value)
    assert re.search(r"{}, {} and {}".format(*dtypes), str(e.value))


@pytest.mark.parametrize("dtypes", [(F16, F16, F16), (F32, F16, F32), (torch.float64,) * 3])
def test_block_attention_refuses_other_dtypes(dtypes):
    with pytest.raises(TypeError, match="float16|float64"):
        ops.block_attention(_Block(), *_qkv(*dtypes))


def test_block_attention_bfloat16_gets_as_far_as_the_shape_checks():
    q, k, v = _qkv(BF16, BF16, BF16)
    with pytest.raises(ValueError, match="one row per destination"):
        ops.block_attention(_Block(), q[:-1], k, v)


def _te(**kw):
    return ops.time_encode_cat((torch.zeros(3, 2),), torch.zeros(3), torch.ones(4), torch.zeros(4),
                               **kw)


@pytest.mark.parametrize("bad", [F16, torch.float64, torch.int32, "bfloat16"])
def test_time_encode_cat_out_dtype(bad):
    with pytest.raises(ValueError, match="out_dtype"):
        _te(out_dtype=bad)
    with pytest.raises(ValueError, match="out_dtype"):
        ops.time_encode(torch.zeros(3), torch.ones(4), torch.zeros(4), out_dtype=bad)


@pytest.mark.parametrize("ok", [None, F32, BF16])
def test_time_encode_cat_valid_out_dtype_gets_as_far_as_the_device_check(ok):
    with pytest.raises(ValueError, match="runs on the GPU"):
        _te(out_dtype=ok)


def test_time_encode_cat_inputs_stay_float32():
    for dtype in (BF16, F16):
        with pytest.raises(TypeError, match="float32"):
            ops.time_encode_cat((torch.zeros(3, 2, dtype=dtype),), torch.zeros(3), torch.ones(4),
                                torch.zeros(4), out_dtype=BF16)


def _es(src, dst, w=F32, bias=F32):
    return ops.edge_score(torch.zeros(4, 6, dtype=src), torch.zeros(8, 6, dtype=dst),
                          torch.zeros(6, dtype=w), torch.zeros(1, dtype=bias))


@pytest.mark.parametrize("src,dst", [(F32, BF16), (BF16, F32)])
def test_edge_score_mixture_names_the_dtypes(src, dst):
    with pytest.raises(TypeError) as e:
        _es(src, dst)
    assert "src is {}".format(src) in str(e.value) and "dst is {}".format(dst) in str(e.value)


def test_edge_score_refuses_other_dtypes():
    for src, dst in ((F16, F16), (F16, F32), (torch.float64, torch.float64)):
        with pytest.raises(TypeError, match="float16|float64"):
            _es(src, dst)
    for kw in (dict(w=BF16), dict(bias=BF16), dict(w=F16)):
        with pytest.raises(TypeError, match="float32"):
            _es(BF16, BF16, **kw)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_edge_score_valid_dtypes_get_as_far_as_the_device_check(dtype):
    with pytest.raises(ValueError, match="runs on the GPU"):
        _es(dtype, dtype)


def test_symbols_in_header_and_capi():
    text = open(os.path.join(ROOT, "include", "gnnflow_hip.h")).read()
    for name, f32 in (("gf_block_attention_bf16", "gf_block_attention"),
                      ("gf_block_attention_bf16_backward", "gf_block_attention_backward"),
                      ("gf_block_attention_dropout_bf16", "gf_block_attention_dropout"),
                      ("gf_block_attention_dropout_bf16_backward",
                       "gf_block_attention_dropout_backward"),
                      ("gf_time_encode_cat_bf16", "gf_time_encode_cat"),
                      ("gf_time_encode_backward_bf16", "gf_time_encode_backward"),
                      ("gf_edge_score_bf16", "gf_edge_score"),
                      ("gf_edge_score_backward_bf16", "gf_edge_score_backward")):
        assert re.search(r"GF_API int {}\(".format(name), text)
        # the same argument order as the float32 sibling
        assert _capi.PROTOTYPES[name] == _capi.PROTOTYPES[f32]
