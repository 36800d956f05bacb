"""Dtype errors of block_reduce, block_max and block_gat now that they take bfloat16 source rows:
what autocast leaves float32 (edge weights, el, er) must be float32, float16 and float64 are
refused anywhere, and a gradient must have its output's dtype.  All of it is refused before the
block's segments or the native library are touched, so this runs on CPU tensors without a GPU."""
import os
import re

import pytest
import torch

from gnnflow_amd import _capi, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
NUM_SRC, NUM_DST, E = 12, 5, 20


class _Block:
    """What the ops read before they launch anything."""

    def num_src_nodes(self):
        return NUM_SRC

    def num_dst_nodes(self):
        return NUM_DST

    def num_edges(self):
        return E

    def segments(self):
        raise AssertionError("the op looked at the block's edges before validating")


@pytest.fixture(autouse=True)
def no_native_call(monkeypatch):
    def load():
        raise AssertionError("the native library was touched")
    monkeypatch.setattr(_capi, "load", load)


def _src(dtype, rows=NUM_SRC):
    return torch.zeros(rows, 6, dtype=dtype)


@pytest.mark.parametrize("src,w", [(F32, BF16), (BF16, BF16), (BF16, F16), (F32, F64)])
def test_block_reduce_weight_must_be_float32(src, w):
    with pytest.raises(TypeError) as e:
        ops.block_reduce(_Block(), _src(src), torch.zeros(E, 2, dtype=w))
    assert "src is {}".format(src) in str(e.value)
    assert "edge_weight is {}".format(w) in str(e.value)


@pytest.mark.parametrize("bad", [F16, F64, torch.int64])
def test_block_reduce_and_block_max_refuse_other_source_dtypes(bad):
    for call in (lambda s: ops.block_reduce(_Block(), s),
                 lambda s: ops.block_reduce(_Block(), s, torch.zeros(E, 2)),
                 lambda s: ops.block_max(_Block(), s)):
        with pytest.raises(TypeError) as e:
            call(_src(bad))
        assert "src is {}".format(bad) in str(e.value) and "float32" in str(e.value)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_valid_source_dtypes_get_as_far_as_the_shape_check(dtype):
    for call in (lambda s: ops.block_reduce(_Block(), s),
                 lambda s: ops.block_reduce(_Block(), s, torch.zeros(E, 2)),
                 lambda s: ops.block_max(_Block(), s)):
        with pytest.raises(ValueError, match="one row per source node"):
            call(_src(dtype, NUM_SRC - 1))


def _gat(feat=F32, el=F32, er=F32):
    return (torch.zeros(NUM_SRC, 2, 3, dtype=feat), torch.zeros(NUM_SRC, 2, dtype=el),
            torch.zeros(NUM_DST, 2, dtype=er))


@pytest.mark.parametrize("dtypes", [(BF16, BF16, F32), (BF16, F32, BF16), (F32, BF16, F32),
                                    (F32, F32, BF16), (BF16, BF16, BF16), (F16, F32, F32),
                                    (F16, F16, F16), (F64, F32, F32), (BF16, F16, F32)])
def test_block_gat_mixtures_name_the_three_dtypes(dtypes):
    with pytest.raises(TypeError) as e:
        ops.block_gat(_Block(), *_gat(*dtypes))
    assert re.search(r"feat is {}, el is {} and er is {}".format(*dtypes), str(e.value))
    assert "float32" in str(e.value)


@pytest.mark.parametrize("feat", [F32, BF16])
def test_block_gat_valid_dtypes_get_as_far_as_the_device_check(feat):
    with pytest.raises(ValueError, match="runs on the GPU"):
        ops.block_gat(_Block(), *_gat(feat))
    with pytest.raises(ValueError, match="one row per source"):
        f, el, er = _gat(feat)
        ops.block_gat(_Block(), f[:-1], el, er)


def test_a_gradient_must_have_its_outputs_dtype():
    for out, grad in ((BF16, F32), (F32, BF16), (BF16, F16)):
        with pytest.raises(TypeError) as e:
            ops._grad_as(torch.zeros(3, dtype=grad), out)
        assert str(out) in str(e.value) and str(grad) in str(e.value)
    g = torch.zeros(3, 2, dtype=BF16).t()
    assert ops._grad_as(g, BF16).is_contiguous()


def test_no_edge_gat_returns_the_inputs_dtype():
    for feat in (F32, BF16):
        f, el, er = _gat(feat)
        f.requires_grad_()
        out = ops._NoEdgeGat.apply(f, el, er)
        assert out.dtype == feat and out.shape == (NUM_DST, 2, 3) and not out.any()
        out.sum().backward()
        assert f.grad.dtype == feat and not f.grad.any()


SIBLINGS = (("gf_block_reduce_bf16", "gf_block_reduce", 0),
            ("gf_block_reduce_backward_bf16", "gf_block_reduce_backward", 1),
            ("gf_block_reduce_max_bf16", "gf_block_reduce_max", 0),
            ("gf_block_reduce_max_backward_bf16", "gf_block_reduce_max_backward", 1),
            ("gf_block_gat_bf16", "gf_block_gat", 1),
            ("gf_block_gat_backward_bf16", "gf_block_gat_backward", 1))


def test_symbols_in_header_and_capi():
    text = open(os.path.join(ROOT, "include", "gnnflow_hip.h")).read()
    for name, f32, extra in SIBLINGS:
        assert re.search(r"GF_API int {}\(".format(name), text), name
        res, args = _capi.PROTOTYPES[name]
        res32, args32 = _capi.PROTOTYPES[f32]
        # the float32 sibling's arguments in its order, then the extra trailing pointers
        assert res == res32 and args[:len(args32)] == args32, name
        assert args[len(args32):] == [_capi.C.c_void_p] * extra, name
