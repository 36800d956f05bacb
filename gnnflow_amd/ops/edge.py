"""edge_score (csrc/edge_score.hip) and edge_rank (csrc/edge_rank.hip): the EdgePredictor's
score of pairs of rows, and of every source against one candidate set."""
from typing import NamedTuple, Optional

import torch

from .. import _capi
from ._common import (_bwd, _check_on_gpu, _check_same_device, _check_tensors, _f32, _fwd,
                      _grads_like, _launch, _partial_rows, _ptr)


class _EdgeScore(torch.autograd.Function):
    @staticmethod
    @_fwd
    def forward(ctx, src, dst, weight, bias):
        # src [B, D], dst [M, D] contiguous, both fp32 or both bf16; weight [D], bias [1] fp32
        M = dst.shape[0]
        out = torch.empty((M, 1), dtype=torch.float32, device=dst.device)
        if M:
            _launch(dst.device, "gf_edge_score", "gf_edge_score_bf16", dst.dtype,
                    (src.data_ptr(), dst.data_ptr(), weight.data_ptr(), bias.data_ptr(),
                     src.shape[0], M, dst.shape[1], out.data_ptr()))
        ctx.save_for_backward(src, dst, weight)
        return out

    @staticmethod
    @_bwd
    def backward(ctx, grad):
        src, dst, weight = ctx.saved_tensors
        (B, D), M = src.shape, dst.shape[0]
        needs = ctx.needs_input_grad
        need_w, need_b = needs[2:]
        f32 = dict(dtype=torch.float32, device=dst.device)
        if M == 0:      # zeros, and nothing to launch
            return _grads_like((src, dst, weight), needs, zero=True) + \
                (torch.zeros(1, **f32) if need_b else None,)
        if not any(needs):
            return None, None, None, None
        g = _f32(grad)
        gs, gd, gw = _grads_like((src, dst, weight), needs)
        gb = torch.empty(1, **f32) if need_b else None
        partials, rows = None, 0
        if need_w or need_b:
            rows = _partial_rows(_capi.load().gf_edge_score_backward_partial_rows, B)
            partials = torch.empty((rows, D + 1), **f32)
        _launch(dst.device, "gf_edge_score_backward", "gf_edge_score_backward_bf16", dst.dtype,
                (src.data_ptr(), dst.data_ptr(), weight.data_ptr(), B, M, D, g.data_ptr(),
                 _ptr(partials), rows, _ptr(gs), _ptr(gd), _ptr(gw), _ptr(gb)))
        return gs, gd, gw, gb


def edge_score(src: torch.Tensor, dst: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor):
    """out[j, 0] = bias + sum_d weight[d] * relu(src[j mod B, d] + dst[j, d]): the tail of the
    reference's EdgePredictor (layers.py:195-197) for every block of dst rows in one kernel.

    src: [B, D]; dst: [M, D] with M = r * B, block k of B rows paired with src (r = 2: the
    positive and the negative half; r > 2: several negatives per positive, block after block);
    weight: [D] or [1, D] (out_fc.weight); bias: [1]; all float32 on one GPU (row slices such as
    h[B:] are taken as they are; any other non-contiguous input is copied first).  Returns
    [M, 1].  Differentiable in all four; every gradient is summed in a fixed order:
    bit-identical from run to run.

    src and dst may instead both be bfloat16 (the Linear outputs under autocast) with weight and
    bias float32; any other dtype or a mixture raises TypeError.  The module's rule -- float32
    arithmetic, one rounding on store -- applies: the scores and the gradients of weight and bias
    are float32 and equal, bit for bit, the float32 op's on src.float() and dst.float(); the
    gradients of src and dst are bfloat16, its float32 gradients rounded once."""
    _check_tensors(("src", src), ("dst", dst), ("weight", weight), ("bias", bias))
    if (src.dtype, dst.dtype) not in ((torch.float32,) * 2, (torch.bfloat16,) * 2):
        raise TypeError("edge_score computes in float32 and takes src and dst both float32 or "
                        "both bfloat16, src is {} and dst is {}".format(src.dtype, dst.dtype))
    for name, x in (("weight", weight), ("bias", bias)):
        if x.dtype != torch.float32:
            raise TypeError("edge_score computes in float32, {} is {}".format(name, x.dtype))
    if src.dim() != 2 or dst.dim() != 2:
        raise ValueError("src and dst must be [B, D] and [M, D], got {} and {}".format(
            tuple(src.shape), tuple(dst.shape)))
    (B, D), M = (int(n) for n in src.shape), int(dst.shape[0])
    if dst.shape[1] != D:
        raise ValueError("src has {} columns, dst has {}".format(D, dst.shape[1]))
    if D == 0:
        raise ValueError("edge_score needs D >= 1")
    if tuple(weight.shape) not in ((D,), (1, D)):
        raise ValueError("weight must be [D] or [1, D] with D = {}, got {}".format(
            D, tuple(weight.shape)))
    if tuple(bias.shape) != (1,):
        raise ValueError("bias must be [1], got {}".format(tuple(bias.shape)))
    if M % B if B else M:
        raise ValueError("dst has {} rows, not a multiple of the {} rows of src".format(M, B))
    _check_same_device("dst", dst, ("src", src), ("weight", weight), ("bias", bias))
    _check_on_gpu("edge_score", dst.device)
    return _EdgeScore.apply(src.contiguous(), dst.contiguous(), weight.reshape(D).contiguous(),
                            bias.contiguous())


EDGE_RANK_MAX_K = 64                 # GF_EDGE_RANK_MAX_K: the longest top-k list
EDGE_RANK_CHUNK = 256                # GF_EDGE_RANK_CHUNK: candidates per workgroup pass of the kernel


class EdgeRank(NamedTuple):
    """What edge_rank returns.  values, indices: [B, k] (float32, int64); greater, equal: [B]
    (int64) or None without a reference score."""
    values: torch.Tensor
    indices: torch.Tensor
    greater: Optional[torch.Tensor]
    equal: Optional[torch.Tensor]

    @property
    def rank(self) -> Optional[torch.Tensor]:
        """float64 [B]: 1 + greater + equal / 2, the mean of the optimistic and the pessimistic
        rank (the convention of link_metrics); None without a reference score."""
        if self.greater is None:
            return None
        return 1.0 + self.greater.double() + self.equal.double() / 2


def edge_rank(src: torch.Tensor, cand: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
              k: int = 0, ref_score: Optional[torch.Tensor] = None,
              skip: Optional[torch.Tensor] = None,
              exclude: Optional[torch.Tensor] = None) -> EdgeRank:
    """Scores every source against ONE shared candidate set and keeps, per source, the k best
    candidates and the number of candidates that beat or tie a reference score:

        score(i, c) = bias + sum_d weight[d] * relu(src[i, d] + cand[c, d])

    in one streaming kernel (csrc/edge_rank.hip) that stores neither the [B * C, D] rows that
    edge_score(src, cand.repeat_interleave(B, 0)) would need nor the [B, C] scores.  score(i, c)
    is the float32 value edge_score returns for that pair of rows, bit for bit, so a ref_score
    taken from edge_score ties exactly with the same candidate here; the one exception is a NaN
    in src[i, d] + cand[c, d], which makes the score NaN (torch.relu keeps a NaN, edge_score's
    relu turns it into 0).

    src: [B, D]; cand: [C, D]; weight: [D] or [1, D]; bias: [1]; ref_score: [B] or [B, 1] or
    None; all float32 on one GPU.  skip: int64 [B] or None.  exclude: int64 [B, W] with
    W = (C + 63) // 64, or None.  0 <= k <= min(C, EDGE_RANK_MAX_K), D >= 1, 1 <= C < 2**31.  Inputs are detached: there is no autograd.  Row slices are taken as
    they are; any other non-contiguous input is copied.

    Returns EdgeRank(values, indices, greater, equal):
      values, indices [B, k]  the k best candidates of each source, score descending, then
          candidate index ascending among equal scores.  A NaN score sorts below -inf (by
          ascending index among NaNs) and is returned as NaN.  A row with fewer than k candidates
          left (k == C with a valid skip, or exclusions) ends in (-inf, -1).  [B, 0] when k == 0.
      greater, equal [B]  the candidates with score > / == ref_score[i]; a NaN score is neither,
          and a NaN ref_score gives two zeros.  None without ref_score.  .rank is
          1 + greater + equal / 2.
    Candidate skip[i] is left out of row i's counts and list (the "filtered" setting: the true
    destination); a value outside [0, C) excludes nothing.  skip works without ref_score too.
    Candidate c is left out of row i in exactly the same way when bit c % 64 of
    exclude[i, c // 64] is set: a per-source SET of candidates, such as the nodes the source has
    already interacted with (DynamicGraph.seen_mask returns this layout).  skip and exclude may
    both be given; bits at positions >= C are ignored; a row with every candidate excluded gets a
    list of (-inf, -1) and, with ref_score, zero counts.

    Runs on the current stream and never synchronises; selection under a total order and
    integer counts: the same inputs give the same bits.

    A candidate set too large for one call is cut into shards cand[a:b]: the counts of the
    shards add, and the lists (indices + a) are concatenated and go through one
    torch.topk(values, k) -- after which equal scores are no longer in index order across
    shards, unless the shards' lists are merged by (value, index) instead.  A shard cand[a:b]
    with a % 64 == 0 takes exclude[:, a // 64:(b + 63) // 64]."""
    named = (("src", src), ("cand", cand), ("weight", weight), ("bias", bias))
    if ref_score is not None:
        named += (("ref_score", ref_score),)
    ints = tuple((name, x) for name, x in (("skip", skip), ("exclude", exclude)) if x is not None)
    _check_tensors(*named, *ints)
    for name, x in named:
        if x.dtype != torch.float32:
            raise TypeError("edge_rank computes in float32, {} is {}".format(name, x.dtype))
    for name, x in ints:
        if x.dtype != torch.int64:
            raise TypeError("{} must be int64, got {}".format(name, x.dtype))
    if isinstance(k, bool) or not isinstance(k, int):
        raise TypeError("k must be an int, got {}".format(type(k).__name__))
    if src.dim() != 2 or cand.dim() != 2:
        raise ValueError("src and cand must be [B, D] and [C, D], got {} and {}".format(
            tuple(src.shape), tuple(cand.shape)))
    (B, D), Cn = (int(n) for n in src.shape), int(cand.shape[0])
    if cand.shape[1] != D:
        raise ValueError("src has {} columns, cand has {}".format(D, cand.shape[1]))
    if D == 0:
        raise ValueError("edge_rank needs D >= 1")
    if Cn == 0:
        raise ValueError("edge_rank needs at least one candidate")
    if Cn >= 2 ** 31:
        raise ValueError("edge_rank takes fewer than 2**31 candidates per call, got {}".format(Cn))
    if tuple(weight.shape) not in ((D,), (1, D)):
        raise ValueError("weight must be [D] or [1, D] with D = {}, got {}".format(
            D, tuple(weight.shape)))
    if tuple(bias.shape) != (1,):
        raise ValueError("bias must be [1], got {}".format(tuple(bias.shape)))
    if k < 0 or k > min(Cn, EDGE_RANK_MAX_K):
        raise ValueError("k must be in [0, min(C, {})] with C = {}, got {}".format(
            EDGE_RANK_MAX_K, Cn, k))
    if ref_score is not None and tuple(ref_score.shape) not in ((B,), (B, 1)):
        raise ValueError("ref_score must be [B] or [B, 1] with B = {}, got {}".format(
            B, tuple(ref_score.shape)))
    if skip is not None and tuple(skip.shape) != (B,):
        raise ValueError("skip must be [B] with B = {}, got {}".format(B, tuple(skip.shape)))
    if exclude is not None and tuple(exclude.shape) != (B, (Cn + 63) // 64):
        raise ValueError("exclude must be [B, (C + 63) // 64] = [{}, {}], got {}".format(
            B, (Cn + 63) // 64, tuple(exclude.shape)))
    _check_same_device("src", src, *named[1:], *ints)
    _check_on_gpu("edge_rank", src.device)
    dev = src.device
    s, c = src.detach().contiguous(), cand.detach().contiguous()
    w, b = weight.detach().reshape(D).contiguous(), bias.detach().contiguous()
    ref = None if ref_score is None else ref_score.detach().reshape(B).contiguous()
    sk = None if skip is None else skip.detach().contiguous()
    ex = None if exclude is None else exclude.detach().contiguous()
    values = torch.empty((B, k), dtype=torch.float32, device=dev)
    indices = torch.empty((B, k), dtype=torch.int64, device=dev)
    greater = equal = None
    if ref is not None:
        greater = torch.empty(B, dtype=torch.int64, device=dev)
        equal = torch.empty(B, dtype=torch.int64, device=dev)
    if B and (k or ref is not None):
        nbytes = _partial_rows(_capi.load().gf_edge_rank_scratch, B, Cn, k)
        scratch = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
        _launch(dev, "gf_edge_rank_masked", None, None,
                (s.data_ptr(), c.data_ptr(), w.data_ptr(), b.data_ptr(), B, Cn, D, k, _ptr(ref),
                 _ptr(sk), _ptr(ex), scratch.data_ptr(), scratch.numel() * 8, _ptr(values),
                 _ptr(indices), _ptr(greater), _ptr(equal)))
    return EdgeRank(values, indices, greater, equal)
