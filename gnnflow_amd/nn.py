"""dgl.nn.SAGEConv / dgl.nn.GATConv for MFGBlocks — the two DGL layers the
reference's static models instantiate (gnnflow/models/graphsage.py:27-31, gat.py:28-46), with
dgl's constructor arguments, parameter names and formulas, on the block ops of
gnnflow_amd.ops.  dgl (requirements.txt: dgl >= 0.7) is not vendored in the reference; these
follow its documented layer definitions.  Both run under torch.autocast('cuda',
dtype=torch.bfloat16) with no cast by the caller: ops.block_reduce, block_max and block_gat take
the bfloat16 rows the Linear layers return (models.SAGE and models.GAT are built from them).

TimeEncode / TemporalAttentionLayer are the reference's own temporal attention
(gnnflow/models/modules/layers.py:16-168, the layer of TGN, TGAT and DySAT) with its constructor
arguments and parameter names, on ops.block_attention and ops.time_encode_cat.

GRUMemoryUpdater is TGN's memory updater (gnnflow/models/modules/memory_updater.py, there
spelled GRUMemeoryUpdater), the consumer of gnnflow_amd.memory.Memory.prepare_input.

EdgePredictor / MLP are the reference's heads (layers.py:171-214); EdgePredictor's tail can run as
one ops.edge_score call.  LinkLoss is the training criterion that follows them, on ops.link_loss."""
from typing import Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops


class SAGEConv(nn.Module):
    """GraphSAGE layer: h_i' = W_self h_i + W_neigh * AGG_{j in N(i)} h_j + b.
    aggregator_type 'mean', 'gcn' or 'pool' ('lstm' is not built).

    Under torch.autocast('cuda', dtype=torch.bfloat16) every aggregator runs on either side of
    `lin_before_mp`, with and without edge weights.  fc_neigh / fc_pool return bfloat16, and
    ops.block_reduce / ops.block_max take the rows as they come, float32 features or bfloat16
    Linear outputs: float32 arithmetic inside, one rounding on store (ops/).  Edge weights stay
    float32.  Two small operands are brought to the large one's dtype so that torch's promotion
    does not widen a [num_dst, out_feats] tensor only for the next Linear to narrow it again (the
    h_dst.to(agg.dtype) of TemporalAttentionLayer): the bias, and in 'gcn' the degrees, where
    degree + 1 is added as integers first so that bfloat16 rounds it once.  The output has the
    dtype of the Linear outputs, bfloat16.  Outside autocast these are no-ops and nothing
    differs."""

    def __init__(self, in_feats, out_feats, aggregator_type, feat_drop=0., bias=True, norm=None,
                 activation=None):
        super().__init__()
        if aggregator_type not in ('mean', 'gcn', 'pool'):
            raise NotImplementedError(
                "SAGEConv aggregator '{}' (only 'mean', 'gcn' and 'pool')".format(aggregator_type))
        self._in_src_feats = self._in_dst_feats = in_feats
        self._out_feats = out_feats
        self._aggre_type = aggregator_type
        self.norm = norm
        self.feat_drop = nn.Dropout(feat_drop)
        self.activation = activation
        if aggregator_type == 'pool':
            self.fc_pool = nn.Linear(in_feats, in_feats)
        self.fc_neigh = nn.Linear(in_feats, out_feats, bias=False)
        if aggregator_type != 'gcn':
            self.fc_self = nn.Linear(in_feats, out_feats, bias=False)
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_feats))
        else:
            self.register_buffer('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain('relu')
        if self._aggre_type == 'pool':
            nn.init.xavier_uniform_(self.fc_pool.weight, gain=gain)
        if self._aggre_type != 'gcn':
            nn.init.xavier_uniform_(self.fc_self.weight, gain=gain)
        nn.init.xavier_uniform_(self.fc_neigh.weight, gain=gain)

    def forward(self, graph, feat, edge_weight=None):
        feat_src = self.feat_drop(feat)
        feat_dst = feat_src[:graph.num_dst_nodes()]
        h_self = feat_dst
        if graph.num_edges() == 0:
            h_neigh = torch.zeros((graph.num_dst_nodes(), self._in_src_feats),
                                  dtype=feat_dst.dtype, device=feat_dst.device)
            if self._aggre_type != 'gcn':
                h_neigh = self.fc_neigh(h_neigh)
        else:
            w = None if edge_weight is None else edge_weight.reshape(graph.num_edges(), 1)
            # linear before message passing when it shrinks the rows
            lin_before_mp = self._in_src_feats > self._out_feats
            if self._aggre_type == 'mean':
                src = self.fc_neigh(feat_src) if lin_before_mp else feat_src
                h_neigh = ops.block_reduce(graph, src, w, mean=True)
                if not lin_before_mp:
                    h_neigh = self.fc_neigh(h_neigh)
            elif self._aggre_type == 'pool':   # max over relu(fc_pool(h_j))
                if w is not None:
                    raise NotImplementedError("SAGEConv('pool') with edge weights")
                h_neigh = self.fc_neigh(ops.block_max(graph, F.relu(self.fc_pool(feat_src))))
            else:   # gcn: (sum of neighbours + self) / (degree + 1)
                src = self.fc_neigh(feat_src) if lin_before_mp else feat_src
                dst = src[:graph.num_dst_nodes()]
                total = ops.block_reduce(graph, src, w, mean=False)
                # degree + 1 in integers, then one cast: exact in float32 as before, and rounded
                # once where total is bfloat16
                degs1 = (graph.in_degrees() + 1).to(total.dtype)
                h_neigh = (total + dst) / degs1.unsqueeze(-1)
                if not lin_before_mp:
                    h_neigh = self.fc_neigh(h_neigh)
        rst = h_neigh if self._aggre_type == 'gcn' else self.fc_self(h_self) + h_neigh
        if self.bias is not None:
            rst = rst + self.bias.to(rst.dtype)      # a no-op unless rst is bfloat16 (autocast)
        if self.activation is not None:
            rst = self.activation(rst)
        if self.norm is not None:
            rst = self.norm(rst)
        return rst


# Defaults of `fused_attention` and `fused_attention_dropout` in GATConv.  Each becomes True only
# once scripts/block_gat_bench.py (the second with --dropout) has shown the fused op, forward +
# backward, ahead of the composed chain at every one of its shapes by more than the chain's own
# round-to-round spread in that run (profiles/block_gat_bench.jsonl).
FUSED_GAT_DEFAULT = False
FUSED_GAT_DROPOUT_DEFAULT = False


class GATConv(nn.Module):
    """Graph attention layer: e_ij = LeakyReLU(a_l . W h_j + a_r . W h_i),
    alpha = edge_softmax(e), h_i' = sum_j alpha_ij W h_j (+ residual, bias, activation);
    returns [num_dst, num_heads, out_feats].

    The attention is the chain el[col] + er[row] -> leaky_relu -> ops.edge_softmax -> attn_drop
    -> ops.block_reduce.  With `fused_attention` set and get_attention false it is ONE
    ops.block_gat call instead (one kernel each way, no [E, H] intermediates), whenever attention
    dropout is inactive (attn_drop.p == 0 or eval mode).  With `fused_attention_dropout` set as
    well, training with 0 < attn_drop.p < 1 is one ops.block_gat call too: the dropout happens
    inside the kernels, from the op's stateless Philox mask, with a seed drawn per forward from
    torch's default CPU generator (no device sync; reproducible under torch.manual_seed, but not
    the mask torch's own dropout would draw).  get_attention=True always takes the composed
    chain, where the returned attention stays differentiable.  Both attributes are plain Python
    attributes, not part of the state dict; their defaults are FUSED_GAT_DEFAULT and
    FUSED_GAT_DROPOUT_DEFAULT.

    Under torch.autocast('cuda', dtype=torch.bfloat16) every one of these paths runs.  fc
    returns bfloat16; el and er come out float32 (bfloat16 * float32 parameter promotes, and sum
    is on autocast's float32 list), so ops.edge_softmax sees float32 as always, and
    ops.block_reduce / ops.block_gat take the bfloat16 rows with the float32 attention: float32
    arithmetic inside, one rounding on store (ops/).  The bias and the residual (float32 when
    res_fc is the identity) are brought to the aggregate's dtype, as TemporalAttentionLayer does
    with h_dst.to(agg.dtype), so that promotion does not widen the [num_dst, H, D] result only for
    the next Linear to narrow it again; the output is bfloat16, and the attention
    get_attention=True returns float32.  Outside autocast the casts are no-ops and nothing
    differs."""

    def __init__(self, in_feats, out_feats, num_heads, feat_drop=0., attn_drop=0.,
                 negative_slope=0.2, residual=False, activation=None,
                 allow_zero_in_degree=False, bias=True):
        super().__init__()
        self._num_heads = num_heads
        self._in_src_feats = self._in_dst_feats = in_feats
        self._out_feats = out_feats
        self._allow_zero_in_degree = allow_zero_in_degree
        self.fc = nn.Linear(in_feats, out_feats * num_heads, bias=False)
        self.attn_l = nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.attn_r = nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.feat_drop = nn.Dropout(feat_drop)
        self.attn_drop = nn.Dropout(attn_drop)
        self.leaky_relu = nn.LeakyReLU(negative_slope)
        if bias:
            self.bias = nn.Parameter(torch.zeros(num_heads * out_feats))
        else:
            self.register_buffer('bias', None)
        if residual:
            if in_feats != out_feats * num_heads:
                self.res_fc = nn.Linear(in_feats, num_heads * out_feats, bias=False)
            else:
                self.res_fc = nn.Identity()
        else:
            self.register_buffer('res_fc', None)
        self.activation = activation
        # True: the attention is one ops.block_gat call (not part of the state)
        self.fused_attention = FUSED_GAT_DEFAULT
        # True: attention dropout in training inside ops.block_gat (not part of the state)
        self.fused_attention_dropout = FUSED_GAT_DROPOUT_DEFAULT
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain('relu')
        nn.init.xavier_normal_(self.fc.weight, gain=gain)
        nn.init.xavier_normal_(self.attn_l, gain=gain)
        nn.init.xavier_normal_(self.attn_r, gain=gain)
        if isinstance(self.res_fc, nn.Linear):
            nn.init.xavier_normal_(self.res_fc.weight, gain=gain)

    def set_allow_zero_in_degree(self, set_value):
        self._allow_zero_in_degree = set_value

    def forward(self, graph, feat, get_attention=False):
        if not self._allow_zero_in_degree and graph.num_dst_nodes() and \
                bool((graph.in_degrees() == 0).any()):
            raise RuntimeError(
                "There are 0-in-degree nodes in the graph, output for those nodes will be "
                "invalid. Set allow_zero_in_degree=True to suppress this check.")
        num_dst, H, D = graph.num_dst_nodes(), self._num_heads, self._out_feats
        h_src = self.feat_drop(feat)
        feat_src = self.fc(h_src).view(-1, H, D)
        feat_dst = feat_src[:num_dst]
        el = (feat_src * self.attn_l).sum(dim=-1)        # [num_src, H]
        er = (feat_dst * self.attn_r).sum(dim=-1)        # [num_dst, H]
        p = self.attn_drop.p
        drop = self.training and p > 0
        a = None
        if self.fused_attention and not get_attention and not drop:
            rst = ops.block_gat(graph, feat_src, el, er,
                                negative_slope=self.leaky_relu.negative_slope)
        elif self.fused_attention and not get_attention and self.fused_attention_dropout \
                and p < 1:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64))
            rst = ops.block_gat(graph, feat_src, el, er,
                                negative_slope=self.leaky_relu.negative_slope,
                                dropout_p=p, dropout_seed=seed)
        else:
            col, row = graph.edges()
            e = self.leaky_relu(el[col] + er[row])           # u_add_v
            a = self.attn_drop(ops.edge_softmax(graph, e))   # [E, H]
            rst = ops.block_reduce(graph, feat_src, a)       # u_mul_e + sum -> [num_dst, H, D]
        if self.res_fc is not None:
            # an identity res_fc hands on the float32 input: one cast of the [num_dst, H * D] side
            rst = rst + self.res_fc(h_src[:num_dst]).view(num_dst, H, D).to(rst.dtype)
        if self.bias is not None:
            rst = rst + self.bias.to(rst.dtype).view(1, H, D)      # a no-op outside autocast
        if self.activation:
            rst = self.activation(rst)
        if get_attention:
            return rst, a.unsqueeze(-1)
        return rst


# Default of `fused_time_encode` in TemporalAttentionLayer and GRUMemoryUpdater.  True only once
# scripts/time_encode_bench.py has shown the fused op ahead of the torch chain at all three epoch
# shapes by more than the chain's own spread (profiles/time_encode_bench.jsonl);
# that has not been measured yet.
FUSED_TIME_ENCODE_DEFAULT = False

# Default of `fused_attention_dropout` in TemporalAttentionLayer.  True only once
# scripts/block_attention_bench.py --dropout 0.2 has shown the fused op, forward + backward, ahead
# of the composed chain at both of its shapes by more than the chain's own round-to-round spread
# (profiles/block_attention_bench.jsonl).
FUSED_ATTENTION_DROPOUT_DEFAULT = False

# Default of `fused_score` in EdgePredictor.  True because scripts/bench_edge_score.py shows
# ops.edge_score, forward + backward, ahead of the torch expression at B = 600, D = 100, as the op
# alone (about 4x) and inside the module (about 1.65x), far beyond the rounds' spread
# (profiles/edge_score_microbench.txt).
FUSED_EDGE_SCORE_DEFAULT = True

# Default of `fused_epilogue` in TemporalAttentionLayer.  True only once
# scripts/layer_epilogue_bench.py has shown ops.dropout_relu_layer_norm, forward + backward, ahead
# of the torch line at every one of its shapes by more than the torch chain's own round-to-round
# spread (profiles/layer_epilogue_bench.jsonl).  It did not hold on the run
# recorded there.  Medians per iteration: the op 62.3-92.8 us (62-67 us in its quietest rounds at
# every shape: the pace at which the host enqueues its three launches), torch 53.5-128.9 us.  The
# op is ahead by more than torch's spread on 6 of the 12 lines (R = 19 800: float32 p = 0 and
# bfloat16 at both p; D = 172: float32 p = 0.1 and bfloat16 at both p), ahead by less than the
# spread on 4, and behind at float32 without dropout at R = 1 800 (0.71x at D = 100, 0.86x at
# D = 172).  So the default stays False.
FUSED_EPILOGUE_DEFAULT = False


# Default of `fused_gru` in GRUMemoryUpdater.  True only once scripts/gru_cell_bench.py has shown
# the module with ops.gru_cell, forward + backward, ahead of the module with torch's GRU cell on
# every one of its lines by more than the torch side's own round-to-round spread
# (profiles/gru_cell_bench.jsonl).  It did not hold on the run recorded there:
# medians 352-638 us against torch's 334-634 us at N = 1 800 and 19 800 alike (the host's pace of
# enqueueing 17-31 launches), ahead by more than torch's spread on 1 of the 8 lines, behind at
# N = 1 800 without node features in float32 (0.949x).  So the default stays False.
FUSED_GRU_DEFAULT = False


class TimeEncode(nn.Module):
    """TGAT's time encoding cos(w * dt + b): w = 1 / 10^linspace(0, 9, dim_time), b = 0 at
    initialisation, both trainable; held as a Linear(1, dim_time) named `w`.  float32 input on
    the GPU takes ops.time_encode (one kernel); anything else the torch expression."""

    def __init__(self, dim_time: int):
        super().__init__()
        self.w = nn.Linear(1, dim_time)
        freq = 1 / 10 ** np.linspace(0, 9, dim_time, dtype=np.float32)
        self.w.weight = nn.Parameter(torch.from_numpy(freq).reshape(dim_time, 1))
        self.w.bias = nn.Parameter(torch.zeros(dim_time))

    def forward(self, delta_time: torch.Tensor) -> torch.Tensor:
        if delta_time.is_cuda and delta_time.dtype == torch.float32 and \
                self.w.weight.dtype == torch.float32:
            return ops.time_encode(delta_time.reshape(-1), self.w.weight, self.w.bias)
        return torch.cos(self.w(delta_time.reshape(-1, 1)))


class FixedTimeEncode(nn.Module):
    """GraphMixer's frozen time encoding cos(dt * w), w_i = 10^(-9 i / (dim - 1)) (w = 1 for
    dim == 1): TimeEncode's initial frequencies, never trained.  `weight` [dim, 1] and the zero
    `bias` [dim] are buffers, so the module has no parameters and they follow .to() and the
    state dict.  forward(dt of any shape) -> dt.shape + (dim,); float32 input on the GPU takes
    ops.time_encode (one kernel), anything else the torch expression."""

    def __init__(self, dim: int):
        super().__init__()
        freq = 1 / 10 ** np.linspace(0, 9, dim, dtype=np.float32)
        self.dim = int(dim)
        self.register_buffer("weight", torch.from_numpy(freq).reshape(dim, 1))
        self.register_buffer("bias", torch.zeros(dim))

    def forward(self, delta_time: torch.Tensor) -> torch.Tensor:
        flat = delta_time.reshape(-1)
        if flat.is_cuda and flat.dtype == torch.float32 and self.weight.dtype == torch.float32:
            out = ops.time_encode(flat, self.weight, self.bias)
        else:
            out = torch.cos(flat.unsqueeze(1) * self.weight.reshape(1, -1) + self.bias)
        return out.reshape(tuple(delta_time.shape) + (self.dim,))


class _GatherCountPair(torch.autograd.Function):
    """out[r] = tab[i0[r]] + tab[i1[r]] where filled[r], else 0.  The table's gradient is a sum
    of all rows into a handful: it is accumulated in float64 and rounded once, so that it neither
    loses bits as the batch grows nor depends on the order of the adds beyond that rounding."""

    @staticmethod
    def forward(ctx, tab, i0, i1, filled):
        ctx.save_for_backward(i0, i1, filled)
        ctx.rows = tab.shape[0]
        out = tab.index_select(0, i0) + tab.index_select(0, i1)
        return out.masked_fill(~filled.unsqueeze(1), 0.0)

    @staticmethod
    def backward(ctx, grad):
        i0, i1, filled = ctx.saved_tensors
        g = grad.masked_fill(~filled.unsqueeze(1), 0.0).double()
        d_tab = torch.zeros((ctx.rows, g.shape[1]), dtype=torch.float64, device=g.device)
        d_tab.index_add_(0, i0, g)
        d_tab.index_add_(0, i1, g)
        return d_tab.to(grad.dtype), None, None, None


class NeighborCooccurrenceEncoder(nn.Module):
    """DyGFormer's neighbour co-occurrence encoder over DynamicGraph.neighbor_cooccurrence's
    counts: f(c) = Linear(dim, dim)(ReLU(Linear(1, dim)(c))), and the feature of a sequence
    element is f(its count in src's sequence) + f(its count in dst's).

    forward(counts int [N, 2, L, 2], lengths int [N, 2]) -> float32 [N, 2, L, dim], the positions
    at and past lengths[i, side] exactly zero.  A count is an integer in [0, L], so f is evaluated
    once on arange(M + 1) and gathered: two tiny GEMMs and two index_selects instead of a GEMM over
    N * 2 * L * 2 rows, and the gradient goes back through the gather (summed into the table's
    M + 1 rows in float64, rounded once).  M = max_count
    when given (the table then has the same size in every call; L above it is a ValueError), else
    the call's own L.  Plain torch: no kernel of its own."""

    def __init__(self, dim: int, max_count: Optional[int] = None):
        super().__init__()
        if max_count is not None and (isinstance(max_count, bool) or
                                      not isinstance(max_count, int) or max_count < 1):
            raise ValueError("max_count must be None or an int >= 1, got {!r}".format(max_count))
        self.dim, self.max_count = int(dim), max_count
        self.lift = nn.Linear(1, dim)
        self.proj = nn.Linear(dim, dim)

    def table(self, max_count: int) -> torch.Tensor:
        """f(0), f(1), .. f(max_count): float [max_count + 1, dim]"""
        c = torch.arange(max_count + 1, device=self.lift.weight.device,
                         dtype=self.lift.weight.dtype)
        return self.proj(F.relu(self.lift(c.unsqueeze(1))))

    def forward(self, counts: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
        if counts.dim() != 4 or counts.shape[1] != 2 or counts.shape[3] != 2:
            raise ValueError("counts must be [N, 2, L, 2], got shape {}".format(
                tuple(counts.shape)))
        N, _, L, _ = counts.shape
        if tuple(lengths.shape) != (N, 2):
            raise ValueError("lengths must be [{}, 2], got shape {}".format(
                N, tuple(lengths.shape)))
        M = L if self.max_count is None else self.max_count
        if L > M:
            raise ValueError("sequences of {} slots, max_count is {}".format(L, M))
        idx = counts.reshape(-1, 2).long()
        filled = torch.arange(L, device=lengths.device) < lengths.unsqueeze(2)
        out = _GatherCountPair.apply(self.table(M), idx[:, 0].contiguous(),
                                     idx[:, 1].contiguous(), filled.reshape(-1))
        return out.reshape(N, 2, L, self.dim)


class TemporalAttentionLayer(nn.Module):
    """Temporal multi-head attention over a sampled block (reads b.srcdata['h'], b.edata['f'],
    b.edata['dt']):

        Q = w_q([h_dst | time_enc(0)])            per destination
        K, V = w_k, w_v([h_src | f | time_enc(dt)])   per edge
        att = edge_softmax(leaky_relu(<Q, K> per head, 0.2)), dropped out with att_dropout
        out = layer_norm(relu(dropout(w_out([sum_e att V | h_dst]))))

    A width of 0 leaves that part out: without node features the query is the time encoding
    alone, or a row of ones (and w_q the identity) without a time encoding either.  With
    attention dropout inactive (p = 0 or eval mode) the attention is one ops.block_attention
    call; otherwise edge_softmax -> dropout -> block_reduce, so that dropout acts on the
    attention weights as in the reference.  With `fused_attention_dropout` (and
    `fused_attention`) training with 0 < att_dropout.p < 1 is one ops.block_attention call too:
    the dropout happens inside the kernels, from the op's stateless Philox mask, with a seed
    drawn per forward from torch's default CPU generator (no device sync; reproducible under
    torch.manual_seed, but not the mask torch's own dropout would draw).  With `fused_time_encode` the rows [h_src | f |
    time_enc(dt)] and [h_dst | time_enc(0)] are one ops.time_encode_cat call each.

    Under torch.autocast('cuda', dtype=torch.bfloat16) every flag combination runs.  The Linear
    layers return bfloat16, and ops.block_attention takes q, k, v as they come: float32
    arithmetic inside, one rounding on store (ops/).  With `fused_time_encode` the rows are
    asked for in bfloat16 (out_dtype), the type w_q / w_k / w_v want, so autocast has nothing to
    cast in front of them.  The bfloat16 aggregate is concatenated with h_dst.to(bfloat16): one
    cast of the [R, dim_node] side and a bfloat16 cat, one kernel fewer than letting torch.cat
    promote (which widens the aggregate, concatenates in float32 and leaves w_out's input to be
    cast again).  The composed chain edge_softmax -> dropout -> block_reduce is float32 only:
    where it is taken (`fused_attention` off, or dropout active with `fused_attention_dropout`
    off) q, k, v are widened with .float() in front of it.  The output is float32, layer_norm's
    type under autocast.  Outside autocast nothing differs.

    With `fused_epilogue` the last line after w_out, layer_norm(relu(dropout(.))), is one
    ops.dropout_relu_layer_norm call each way instead of torch's dropout, relu, cast and
    layer_norm kernels: it takes w_out's rows as they come (float32, or bfloat16 under autocast),
    returns float32 and writes no mask.  In training with 0 < dropout.p < 1 the dropout happens
    inside the kernel, from the op's stateless Philox mask with a seed drawn per forward from
    torch's default CPU generator, after the attention's when both are drawn: reproducible under
    torch.manual_seed, but not the mask nn.Dropout would draw.  With the flag off no seed is
    drawn.  dropout.p == 1, a layer_norm without affine parameters, rows that are not on the GPU
    or not float32 / bfloat16, and dim_out above ops.LAYER_EPILOGUE_MAX_WIDTH take the torch
    line."""

    def __init__(self, dim_node: int, dim_edge: int, dim_time: int, dim_out: int, num_head: int,
                 dropout: float, att_dropout: float):
        super().__init__()
        self.use_node_feat = dim_node > 0
        self.use_edge_feat = dim_edge > 0
        self.use_time_enc = dim_time > 0
        self.dim_node, self.dim_time, self.dim_out, self.num_head = \
            dim_node, dim_time, dim_out, num_head
        self.dropout = nn.Dropout(dropout)
        self.att_dropout = nn.Dropout(att_dropout)
        self.att_act = nn.LeakyReLU(0.2)
        if self.use_time_enc:
            self.time_enc = TimeEncode(dim_time)
        if self.use_node_feat or self.use_time_enc:
            self.w_q = nn.Linear(dim_node + dim_time, dim_out)
        else:
            self.w_q = nn.Identity()
        self.w_k = nn.Linear(dim_node + dim_edge + dim_time, dim_out)
        self.w_v = nn.Linear(dim_node + dim_edge + dim_time, dim_out)
        self.w_out = nn.Linear(dim_node + dim_out, dim_out)
        self.layer_norm = nn.LayerNorm(dim_out)
        # False: always the composed edge_softmax -> block_reduce chain (not part of the state)
        self.fused_attention = True
        # True: attention dropout in training inside ops.block_attention (not part of the state)
        self.fused_attention_dropout = FUSED_ATTENTION_DROPOUT_DEFAULT
        # False: time_enc + torch.cat instead of ops.time_encode_cat (not part of the state)
        self.fused_time_encode = FUSED_TIME_ENCODE_DEFAULT
        # True: dropout, relu and layer_norm after w_out as one ops.dropout_relu_layer_norm call
        # (not part of the state)
        self.fused_epilogue = FUSED_EPILOGUE_DEFAULT

    def forward(self, b):
        E, R, dev = b.num_edges(), b.num_dst_nodes(), b.device
        if E == 0:
            return torch.zeros((R, self.dim_out), device=dev)
        fused_te = self.fused_time_encode and self.use_time_enc
        amp = dev.type == 'cuda' and torch.is_autocast_enabled('cuda') and \
            torch.get_autocast_dtype('cuda') == torch.bfloat16
        parts_q, parts_kv = [], []
        if self.use_node_feat:
            h = b.srcdata['h']
            h_dst = h[:R]
            parts_q.append(h_dst)
            parts_kv.append(h[R:])
        elif not self.use_time_enc:
            parts_q.append(torch.ones((R, self.dim_out), device=dev))
        if self.use_edge_feat:
            parts_kv.append(b.edata['f'])
        if fused_te:      # [parts | time_enc] in one launch each
            w = self.time_enc.w
            rows = torch.bfloat16 if amp else None      # the GEMMs' input type under autocast
            q_in = ops.time_encode_cat(parts_q, torch.zeros(R, dtype=torch.float32, device=dev),
                                       w.weight, w.bias, out_dtype=rows)
            kv = ops.time_encode_cat(parts_kv, b.edata['dt'], w.weight, w.bias, out_dtype=rows)
        else:
            if self.use_time_enc:
                parts_q.append(self.time_enc(torch.zeros(R, dtype=torch.float32, device=dev)))
                parts_kv.append(self.time_enc(b.edata['dt']))
            kv = torch.cat(parts_kv, dim=1) if parts_kv else torch.zeros((E, 0), device=dev)
            q_in = torch.cat(parts_q, dim=1)
        H = self.num_head
        q = self.w_q(q_in).reshape(R, H, -1)
        k = self.w_k(kv).reshape(E, H, -1)
        v = self.w_v(kv).reshape(E, H, -1)
        if q.dtype != k.dtype:      # w_q the identity: a row of ones, exact in any float type
            q = q.to(k.dtype)
        p = self.att_dropout.p
        if self.fused_attention and (p == 0 or not self.training):
            agg = ops.block_attention(b, q, k, v, negative_slope=self.att_act.negative_slope)
        elif self.fused_attention and self.fused_attention_dropout and 0 < p < 1:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64))
            agg = ops.block_attention(b, q, k, v, negative_slope=self.att_act.negative_slope,
                                      dropout_p=p, dropout_seed=seed)
        else:
            if q.dtype == torch.bfloat16:      # the composed chain is float32 only
                q, k, v = q.float(), k.float(), v.float()
            row = b.edges()[1]
            att = ops.edge_softmax(b, self.att_act((q[row] * k).sum(dim=2)))
            msg = (v * self.att_dropout(att)[:, :, None]).reshape(E, -1)
            agg = ops.block_reduce(b, torch.cat([torch.zeros((R, msg.shape[1]), device=dev), msg]))
        agg = agg.reshape(R, -1)
        rst = torch.cat([agg, h_dst.to(agg.dtype)], dim=1) if self.use_node_feat else agg
        z = self.w_out(rst)
        ln, p = self.layer_norm, self.dropout.p
        if self.fused_epilogue and z.is_cuda and z.dtype in (torch.float32, torch.bfloat16) and \
                self.dim_out <= ops.LAYER_EPILOGUE_MAX_WIDTH and ln.weight is not None and \
                ln.bias is not None and ln.weight.dtype == torch.float32 and \
                (0 <= p < 1 or not self.training):
            if p == 0 or not self.training:
                return ops.dropout_relu_layer_norm(z, ln.weight, ln.bias, ln.eps)
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64))
            return ops.dropout_relu_layer_norm(z, ln.weight, ln.bias, ln.eps, dropout_p=p,
                                               dropout_seed=seed)
        return ln(F.relu(self.dropout(z)))


TransfomerAttentionLayer = TemporalAttentionLayer      # the reference's own spelling


class GRUMemoryUpdater(nn.Module):
    """TGN's GRU memory updater over a block prepared by Memory.prepare_input (reads
    b.srcdata['ts', 'mem_ts', 'mem_input', 'mem', 'ID'], and 'h' when dim_node > 0):

        updated = GRUCell([mem_input | time_enc(ts - mem_ts)], mem)
        b.srcdata['h'] = h + updated                      dim_node == dim_embed
                         updated + node_feat_proj(h)      other dim_node > 0
                         updated                          no node features

    Returns {'last_updated_nid', 'last_updated_memory', 'last_updated_ts'} of the first
    num_dst_nodes rows as detached clones, the arguments of Memory.update_mem_mail.  Unlike the
    reference it leaves b.srcdata['mem_input'] as prepare_input wrote it.  With
    `fused_time_encode` the GRU input is one ops.time_encode_cat call.  Under bfloat16 autocast the
    GRU cell returns bfloat16; it is widened once, so 'last_updated_memory' (Memory stores
    float32) and b.srcdata['h'] come out float32 as they do outside autocast.

    With `fused_gru` and float32 memory rows on the GPU, the cell is its two GEMMs (F.linear with
    the parameters of `updater`, which stays an nn.GRUCell: state dicts do not change) and one
    ops.gru_cell call that takes b.srcdata['mem'] as stored -- float32, never rounded, under
    autocast too -- adds the residual and writes 'last_updated_memory' as an output of its own:
    no cast, no clone of the memory rows and no add behind it."""

    def __init__(self, dim_node: int, dim_edge: int, dim_time: int, dim_embed: int,
                 dim_memory: int):
        super().__init__()
        self.dim_message = 2 * dim_memory + dim_edge
        self.dim_node, self.dim_time, self.dim_embed = dim_node, dim_time, dim_embed
        self.updater = nn.GRUCell(self.dim_message + dim_time, dim_memory)
        self.use_time_enc = dim_time > 0
        if self.use_time_enc:
            self.time_enc = TimeEncode(dim_time)
        if dim_node > 0 and dim_node != dim_memory:
            self.node_feat_proj = nn.Linear(dim_node, dim_memory)
        # False: time_enc + torch.cat instead of ops.time_encode_cat (not part of the state)
        self.fused_time_encode = FUSED_TIME_ENCODE_DEFAULT
        # True: ops.gru_cell behind the two GEMMs instead of nn.GRUCell (not part of the state)
        self.fused_gru = FUSED_GRU_DEFAULT

    def _forward_fused(self, b, x):
        """The rest of forward() through ops.gru_cell."""
        cell, mem, R = self.updater, b.srcdata['mem'], b.num_dst_nodes()
        gi = F.linear(x, cell.weight_ih, cell.bias_ih)
        gh = F.linear(mem, cell.weight_hh, cell.bias_hh)
        residual = None
        if self.dim_node > 0:
            residual = b.srcdata['h']
            if self.dim_node != self.dim_embed:
                residual = self.node_feat_proj(residual)
        h, last_mem = ops.gru_cell(gi, gh, mem, residual=residual, num_last=R)
        last = {"last_updated_nid": b.srcdata['ID'][:R].detach().clone(),
                "last_updated_memory": last_mem,
                "last_updated_ts": b.srcdata['ts'][:R].detach().clone()}
        b.srcdata['h'] = h
        return last

    def forward(self, b):
        x = b.srcdata['mem_input']
        if self.use_time_enc:
            dt = b.srcdata['ts'] - b.srcdata['mem_ts']
            if self.fused_time_encode:
                x = ops.time_encode_cat((x,), dt, self.time_enc.w.weight, self.time_enc.w.bias)
            else:
                x = torch.cat([x, self.time_enc(dt)], dim=1)
        mem = b.srcdata['mem']
        if self.fused_gru and mem.is_cuda and mem.dtype == torch.float32 and \
                self.updater.weight_ih.dtype == torch.float32 and \
                x.dtype in (torch.float32, torch.bfloat16) and \
                (self.dim_node == 0 or b.srcdata['h'].dtype in (torch.float32, torch.bfloat16)):
            return self._forward_fused(b, x)
        updated = self.updater(x, mem)
        if updated.dtype == torch.bfloat16:      # bfloat16 autocast: memory and 'h' stay float32
            updated = updated.float()
        R = b.num_dst_nodes()
        last = {"last_updated_nid": b.srcdata['ID'][:R].detach().clone(),
                "last_updated_memory": updated[:R].detach().clone(),
                "last_updated_ts": b.srcdata['ts'][:R].detach().clone()}
        if self.dim_node > 0:
            if self.dim_node == self.dim_embed:
                b.srcdata['h'] = b.srcdata['h'] + updated
            else:
                b.srcdata['h'] = updated + self.node_feat_proj(b.srcdata['h'])
        else:
            b.srcdata['h'] = updated
        return last


GRUMemeoryUpdater = GRUMemoryUpdater                   # the reference's own spelling


class EdgePredictor(nn.Module):
    """The reference's link-prediction head over h = [src | pos dst | neg dst] (three equal row
    blocks):

        pos = out_fc(relu(src_fc(src) + dst_fc(pos dst)))
        neg = out_fc(relu(src_fc(src) + dst_fc(neg dst)))        -> (pos, neg), [B, 1] each

    With `fused_score`, float32 rows on the GPU take dst_fc as one GEMM over both destination
    blocks and everything behind it as one ops.edge_score call; anything else the torch
    expression.  The call is made when what src_fc and dst_fc return is float32 or, as under
    bfloat16 autocast, bfloat16 (ops.edge_score: float32 arithmetic, float32 scores); any other
    type they return (float16 autocast) takes the torch expression on the same two results."""

    def __init__(self, dim_embed: int):
        super().__init__()
        self.src_fc = nn.Linear(dim_embed, dim_embed)
        self.dst_fc = nn.Linear(dim_embed, dim_embed)
        self.out_fc = nn.Linear(dim_embed, 1)
        # True: the tail as one ops.edge_score call (not part of the state)
        self.fused_score = FUSED_EDGE_SCORE_DEFAULT

    def forward(self, h: torch.Tensor):
        if h.shape[0] % 3:
            raise ValueError("EdgePredictor takes [src | pos dst | neg dst] rows, {} is not a "
                             "multiple of 3".format(h.shape[0]))
        B = h.shape[0] // 3
        if self.fused_score and h.is_cuda and h.dtype in (torch.float32, torch.bfloat16) and \
                self.out_fc.weight.dtype == torch.float32:
            src_h, dst_h = self.src_fc(h[:B]), self.dst_fc(h[B:])
            if src_h.dtype == dst_h.dtype and src_h.dtype in (torch.float32, torch.bfloat16):
                out = ops.edge_score(src_h, dst_h, self.out_fc.weight, self.out_fc.bias)
                return out[:B], out[B:]
            return (self.out_fc(F.relu(src_h + dst_h[:B])), self.out_fc(F.relu(src_h + dst_h[B:])))
        src_h = self.src_fc(h[:B])
        pos_edge = F.relu(src_h + self.dst_fc(h[B:2 * B]))
        neg_edge = F.relu(src_h + self.dst_fc(h[2 * B:]))
        return self.out_fc(pos_edge), self.out_fc(neg_edge)

    _RANK_TORCH_CHUNK = 4096      # candidates per step of the torch expression of rank()

    @torch.no_grad()
    def rank(self, h_src: torch.Tensor, h_cand: torch.Tensor, k: int = 0,
             target: Optional[torch.Tensor] = None,
             exclude: Optional[torch.Tensor] = None) -> "ops.EdgeRank":
        """Ranks the candidates h_cand [C, dim_embed] for every source h_src [B, dim_embed]:
        the score of forward() for every (source, candidate) pair, of which the k best
        candidates per source (ops.EdgeRank.values / .indices, [B, k]) are kept and, with
        `target` (int64 [B], the index of each source's true destination among the candidates,
        all in range, not checked), the counts .greater / .equal of the OTHER candidates that
        beat / tie the target's score; .rank is 1 + greater + equal / 2.  The target is left
        out of its own row's list too (the filtered setting).  No gradient, no state.

        `exclude` (int64 [B, (C + 63) // 64], ops.edge_rank's bit layout, what
        DynamicGraph.seen_mask returns) leaves a per-source set of candidates out of the list and
        the counts as well.  The target's score is still taken from its own row of h_cand, so
        with `target` the rank is the target's rank among the candidates that are neither
        excluded nor the target, also when the target's own bit is set -- the usual case on a
        stream with repeat interactions, and the filtered setting of the temporal
        link-prediction protocols.

        float32 rows on the GPU with `fused_score` take ops.edge_rank, whose scores are those of
        ops.edge_score bit for bit: the target's score is ops.edge_score's and is compared
        exactly.  Anything else (the CPU, fused_score off, bfloat16 under autocast, widened to
        float32) takes the torch expression over chunks of the candidates, with the same order
        (score descending, then index ascending; NaN last) and the same (-inf, -1) fill."""
        src_p, cand_p = self.src_fc(h_src), self.dst_fc(h_cand)
        w, b = self.out_fc.weight, self.out_fc.bias
        if self.fused_score and src_p.is_cuda and src_p.dtype == cand_p.dtype == torch.float32 \
                and w.dtype == torch.float32:
            ref = None
            if target is not None:
                ref = ops.edge_score(src_p, cand_p[target], w, b)
            return ops.edge_rank(src_p, cand_p, w, b, k=k, ref_score=ref, skip=target,
                                 exclude=exclude)
        return _rank_torch(src_p.float(), cand_p.float(), w.float().reshape(-1), b.float(), k,
                           target, self._RANK_TORCH_CHUNK, exclude)


def _rank_torch(src, cand, w, b, k, target, step, exclude=None):
    """ops.edge_rank's semantics as a torch expression, `step` candidates at a time."""
    (B, D), Cn = src.shape, cand.shape[0]
    if not 0 <= k <= min(Cn, ops.EDGE_RANK_MAX_K):
        raise ValueError("k must be in [0, min(C, {})] with C = {}, got {}".format(
            ops.EDGE_RANK_MAX_K, Cn, k))
    if exclude is not None and (exclude.dtype != torch.int64 or
                                tuple(exclude.shape) != (B, (Cn + 63) // 64)):
        raise ValueError("exclude must be int64 [B, (C + 63) // 64] = [{}, {}], got {} {}".format(
            B, (Cn + 63) // 64, exclude.dtype, tuple(exclude.shape)))
    dev = src.device
    ref = None
    if target is not None:
        ref = (F.relu(src + cand[target]) * w).sum(-1) + b
    greater = torch.zeros(B, dtype=torch.int64, device=dev) if ref is not None else None
    equal = torch.zeros(B, dtype=torch.int64, device=dev) if ref is not None else None
    neg_inf = float("-inf")
    # the running list: (is a number, value, -index) ascending under lexsort = the kernel's key
    vals = torch.full((B, 0), neg_inf, dtype=torch.float32, device=dev)
    idx = torch.full((B, 0), -1, dtype=torch.int64, device=dev)
    for a in range(0, Cn, step):
        c = cand[a:a + step]
        score = (F.relu(src[:, None, :] + c[None, :, :]) * w).sum(-1) + b      # [B, n]
        ids = torch.arange(a, a + c.shape[0], device=dev).expand(B, -1)
        keep = torch.ones_like(ids, dtype=torch.bool) if target is None \
            else ids != target[:, None]
        if exclude is not None:
            keep = keep & (((exclude[:, ids[0] >> 6] >> (ids[0] & 63)) & 1) == 0)
        if ref is not None:
            greater += ((score > ref[:, None]) & keep).sum(1)
            equal += ((score == ref[:, None]) & keep).sum(1)
        if k:
            vals = torch.cat([vals, torch.where(keep, score, torch.full_like(score, neg_inf))], 1)
            idx = torch.cat([idx, torch.where(keep, ids, torch.full_like(ids, -1))], 1)
            # three stable sorts, least significant key first: index ascending, value
            # descending (NaN as the smallest), skipped entries last
            order = torch.argsort(torch.where(idx < 0, torch.full_like(idx, Cn), idx), dim=1,
                                  stable=True)
            vals, idx = vals.gather(1, order), idx.gather(1, order)
            sort_v = torch.where(torch.isnan(vals), torch.full_like(vals, neg_inf), vals)
            tier = torch.where(idx < 0, 2, torch.where(torch.isnan(vals), 1, 0))
            order = torch.argsort(sort_v, dim=1, descending=True, stable=True)
            vals, idx, tier = vals.gather(1, order), idx.gather(1, order), tier.gather(1, order)
            order = torch.argsort(tier, dim=1, stable=True)[:, :k]
            vals, idx = vals.gather(1, order), idx.gather(1, order)
    if not k:
        vals, idx = vals[:, :0], idx[:, :0]
    return ops.EdgeRank(vals, idx, greater, equal)


class LinkLoss(nn.Module):
    """The reference's training criterion for link prediction,

        criterion(pred_pos, ones_like(pred_pos)) + criterion(pred_neg, zeros_like(pred_neg))

    with BCEWithLogitsLoss, as one ops.link_loss call that also keeps the epoch's running sums
    on the device, so that a training epoch reads its loss with one synchronisation:

        criterion = LinkLoss()
        for ...:                                   # the training batches
            loss = criterion(pred_pos, pred_neg)   # float32 scalar, no sync
            loss.backward()
        result = criterion.compute()               # {'mean_loss', ...}, one sync

    The accumulator is a float64 [5] buffer (sum_loss, sum_loss_times_P, batches, nonfinite,
    sum_P; P the number of positives of a batch), created on the device of the first GPU inputs.
    It is not persistent: state_dict() does not hold it.

    Inputs that are not float32 or bfloat16 on the GPU (CPU tensors, float64, float16) take the
    torch expression, F.binary_cross_entropy_with_logits twice, and are NOT accumulated."""

    _FIELDS = ("sum_loss", "sum_loss_times_P", "batches", "nonfinite", "sum_P")

    def __init__(self):
        super().__init__()
        self.register_buffer("state", None, persistent=False)

    def forward(self, pred_pos: torch.Tensor, pred_neg: torch.Tensor) -> torch.Tensor:
        if not (pred_pos.is_cuda and pred_neg.is_cuda and pred_pos.dtype == pred_neg.dtype and
                pred_pos.dtype in (torch.float32, torch.bfloat16)):
            return F.binary_cross_entropy_with_logits(pred_pos, torch.ones_like(pred_pos)) + \
                F.binary_cross_entropy_with_logits(pred_neg, torch.zeros_like(pred_neg))
        if self.state is None or self.state.device != pred_pos.device:
            self.state = torch.zeros(ops.LINK_LOSS_ACC_FIELDS, dtype=torch.float64,
                                     device=pred_pos.device)
        return ops.link_loss(pred_pos, pred_neg, accumulator=self.state)

    def compute(self) -> dict:
        """The epoch so far (one device-to-host copy, which waits for the batches issued):
        'mean_loss' = sum_loss / batches, what the mean of float(loss) over the batches gives;
        'edge_weighted_loss' = sum_loss_times_P / sum_P, each batch weighted by its positives;
        NaN where the count is 0; 'batches'; 'nonfinite' counts the batches left out because
        their loss was NaN or infinite."""
        s = dict(zip(self._FIELDS, self.state.tolist() if self.state is not None else [0.0] * 5))
        nan = float("nan")
        b = int(s["batches"])
        return {"mean_loss": s["sum_loss"] / b if b else nan,
                "edge_weighted_loss": s["sum_loss_times_P"] / s["sum_P"] if s["sum_P"] else nan,
                "batches": b, "nonfinite": int(s["nonfinite"])}

    def reset(self) -> None:
        if self.state is not None:
            self.state.zero_()


class MLP(nn.Module):
    """The reference's node-classification head: fc2(relu(fc1(x)))."""

    def __init__(self, dim_in, dim_hid, num_class):
        super().__init__()
        self.fc1 = nn.Linear(dim_in, dim_hid)
        self.fc2 = nn.Linear(dim_hid, num_class)

    def forward(self, x):
        return self.fc2(F.relu(self.fc1(x)))
