"""DyGFormer (Yu et al., "Towards Better Dynamic Graph Learning: New Architecture and Unified
Library", NeurIPS 2023) per pair, on the readers of DynamicGraph: the newest interactions of both
ends of a pair, the node itself in front, as four channels -- node features, edge features, time
encoding and the neighbour co-occurrence feature -- which are patched, projected channel by
channel, concatenated and run through one transformer encoder over both sides' patches.  The
channels come finished from DynamicGraph.pair_sequence(..., node_feats=, edge_feats=,
time_encoder=model.time_enc) -- one kernel, padding already zero -- into forward_parts; forward
builds the same parts in torch from ids, time deltas and lengths.  Plain torch modules; the GEMMs
are torch's -- except with fused_patches=True, where the node, edge and time channels are never
built: ops.patch_project gathers (encodes) their rows and applies proj in one kernel, from the id
and time planes alone -- and with fused_attention=True, where the encoder blocks' self-attention
between in_proj and out_proj is one ops.sequence_attention call -- and with
fused_feed_forward=True, where the blocks' Linear-GELU-dropout-Linear is one ops.feed_forward
call."""
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..nn import EdgePredictor, FixedTimeEncode, NeighborCooccurrenceEncoder, TimeEncode
from ..ops.feed_forward import _fused_route


class EncoderBlock(nn.Module):
    """One pre-norm transformer encoder block over x [n, S, C]: x + drop(MHA(LN(x))), then
    x + drop(W2 drop(gelu(W1 LN(x)))) with a hidden width of 4 C.  No padding mask.

    fused_attention=True (a route, not state: the same parameters and state_dict) computes the
    attention of a float32 x on a GPU as out_proj(ops.sequence_attention(in_proj(h), num_heads,
    p, seed)): p is att.dropout in training and 0 otherwise, the seed is drawn per forward from
    torch's default CPU generator (no device sync; reproducible under torch.manual_seed, but not
    the mask torch's own dropout would draw).  Any other x takes the torch route.

    fused_feed_forward=True (a route too) makes the second residual of such an x
    x + drop(ops.feed_forward(ff_norm(x), w1.weight, w1.bias, w2.weight, w2.bias, p, seed)), with
    p = drop.p in training and 0 otherwise and a seed drawn the same way: the inner dropout is
    inside the kernel and the [n, S, 4 C] hidden tensors are never stored; LayerNorm, the outer
    dropout and the residual stay in torch.  fused_feed_forward="bfloat16" is that route with
    compute_dtype=torch.bfloat16 (the products on the bfloat16 matrix instruction, float32
    tensors in and out); it is taken inside a bfloat16 autocast region as well, where ff_norm(x)
    is float32 already, while True falls back to torch there.  Any other value: ValueError."""

    def __init__(self, dim: int, num_heads: int, dropout: float, fused_attention: bool = False,
                 fused_feed_forward=False):
        super().__init__()
        self.fused_attention = bool(fused_attention)
        self.fused_feed_forward, self._ff_dtype = _fused_route(fused_feed_forward)
        if self.fused_feed_forward and dim > ops.FEED_FORWARD_MAX_WIDTH:
            raise ValueError("fused_feed_forward takes a dim of up to {}, got {}".format(
                ops.FEED_FORWARD_MAX_WIDTH, dim))
        if self.fused_attention and dim // num_heads > ops.SEQ_ATTENTION_MAX_HEAD_DIM:
            raise ValueError("fused_attention takes heads of up to {} columns, got dim {} / "
                             "num_heads {}".format(ops.SEQ_ATTENTION_MAX_HEAD_DIM, dim, num_heads))
        self.att_norm = nn.LayerNorm(dim)
        self.att = nn.MultiheadAttention(dim, num_heads, dropout=dropout, batch_first=True)
        self.ff_norm = nn.LayerNorm(dim)
        self.w1 = nn.Linear(dim, 4 * dim)
        self.w2 = nn.Linear(4 * dim, dim)
        self.drop = nn.Dropout(dropout)

    @staticmethod
    def _seed(p):
        return int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64)) if p > 0 else None

    def forward(self, x):
        h = self.att_norm(x)
        on_gpu = x.is_cuda and x.dtype == torch.float32
        fusable = on_gpu and not torch.is_autocast_enabled()
        if self.fused_attention and fusable:
            att = self.att
            p = att.dropout if self.training else 0.0
            seed = self._seed(p)
            qkv = F.linear(h, att.in_proj_weight, att.in_proj_bias)
            a = att.out_proj(ops.sequence_attention(qkv, att.num_heads, p, seed))
        else:
            a = self.att(h, h, h, need_weights=False)[0]
        x = x + self.drop(a)
        if self.fused_feed_forward and (fusable or on_gpu and self._ff_dtype == torch.bfloat16):
            p = self.drop.p if self.training else 0.0
            return x + self.drop(ops.feed_forward(
                self.ff_norm(x).contiguous(), self.w1.weight, self.w1.bias, self.w2.weight,
                self.w2.bias, p, self._seed(p), compute_dtype=self._ff_dtype))
        return x + self.drop(self.w2(self.drop(F.gelu(self.w1(self.ff_norm(x))))))


def _table_rows(table: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """table[ids] with the zero row for an id without a row (negative, >= the table's rows)."""
    known = (ids >= 0) & (ids < table.shape[0])
    return table[ids.clamp(0, table.shape[0] - 1)].masked_fill(~known.unsqueeze(-1), 0.0)


class DyGFormer(nn.Module):
    """
    DyGFormer, one score per pair, with L = max_length slots per side and P = patch_size:

        channels = node_x, edge_x, time_x [N, 2, L, d], the slots p >= lengths set to zero, and
                   cooc_enc(counts, lengths) [N, 2, L, channel_dim]
        patches  = each channel as [N, 2, L / P, P d] through its own Linear(P d, channel_dim),
                   concatenated: [N, 2, L / P, C], C = channels * channel_dim
        x        = blocks(patches as one sequence [N, 2 L / P, C])
        emb      = out_fc(mean over each side's L / P patches)            [N, 2, dim_embed]
        score    = edge_predictor's out_fc(relu(src_fc(emb_src) + dst_fc(emb_dst)))     [N, 1]

        time_enc         FixedTimeEncode(dim_time), frozen; TimeEncode(dim_time) with learn_time
        cooc_enc         NeighborCooccurrenceEncoder(channel_dim, max_count=max_length)
        proj             the channels' Linear(P d, channel_dim), by name
        blocks           num_layers EncoderBlocks, no padding mask (the published model has none)
        out_fc           Linear(C, dim_embed)
        edge_predictor   the link-prediction head; row i pairs src[i] with dst[i]

    dim_node == 0 or dim_edge == 0 drops that channel (node_x / edge_x are then ignored).

    fused_patches=True (off by default; README "patch_project" has the measurements) makes
    forward and forward_graph, on a GPU, take the node and edge channels' patches from
    ops.patch_project and the time channel's from ops.patch_project_time (with learn_time the
    time channel stays on the torch route, so that TimeEncode trains); forward_graph then asks
    pair_sequence for the planes only.  The parameters, the state_dict and forward_parts are the
    same either way.

    fused_attention=True (off by default; README "sequence_attention" has the measurements) makes
    every EncoderBlock take its self-attention from ops.sequence_attention on a GPU, with the
    attention dropout inside the kernel.  A route too: nothing in the state changes.

    fused_feed_forward=True (off by default; README "feed_forward" has the measurements) makes
    every EncoderBlock take its feed-forward from ops.feed_forward on a GPU, with the inner
    dropout inside the kernel and no [N, S, 4 C] tensor stored.  A route as well.
    fused_feed_forward="bfloat16" runs that kernel's products on the bfloat16 matrix instruction
    (ops.feed_forward's compute_dtype), under bfloat16 autocast too; see EncoderBlock.
    """

    def __init__(self, dim_node: int, dim_edge: int, dim_time: int = 100, channel_dim: int = 50,
                 patch_size: int = 1, num_layers: int = 2, num_heads: int = 2,
                 dropout: float = 0.1, max_length: int = 32, dim_embed: int = 100,
                 learn_time: bool = False, fused_patches: bool = False,
                 fused_attention: bool = False, fused_feed_forward=False):
        super().__init__()
        for name, value, lo in (("dim_node", dim_node, 0), ("dim_edge", dim_edge, 0),
                                ("dim_time", dim_time, 1), ("channel_dim", channel_dim, 1),
                                ("patch_size", patch_size, 1), ("num_layers", num_layers, 1),
                                ("num_heads", num_heads, 1), ("max_length", max_length, 2),
                                ("dim_embed", dim_embed, 1)):
            if isinstance(value, bool) or not isinstance(value, int) or value < lo:
                raise ValueError("{} must be an int >= {}, got {!r}".format(name, lo, value))
        if max_length % patch_size:
            raise ValueError("max_length {} is not a multiple of patch_size {}".format(
                max_length, patch_size))
        widths = {"node": dim_node, "edge": dim_edge, "time": dim_time, "cooc": channel_dim}
        self.channels = [name for name in ("node", "edge", "time", "cooc") if widths[name]]
        dim = len(self.channels) * channel_dim
        if dim % num_heads:
            raise ValueError("{} channels of {} columns are not a multiple of num_heads {}".format(
                len(self.channels), channel_dim, num_heads))
        self.dim_node, self.dim_edge, self.dim_time = dim_node, dim_edge, dim_time
        self.channel_dim, self.patch_size, self.max_length = channel_dim, patch_size, max_length
        self.dim_embed, self.learn_time = dim_embed, bool(learn_time)
        self.fused_patches = bool(fused_patches)      # a route, not state: no parameter or buffer
        if self.fused_patches:      # ops.patch_project's limits, here and not at the first call
            fused = [n for n in self.channels if n in ("node", "edge") or
                     (n == "time" and not learn_time)]
            wide = [n for n in fused if widths[n] > ops.PATCH_MAX_WIDTH or
                    patch_size * widths[n] > ops.PATCH_MAX_PATCH_WIDTH]
            if wide or channel_dim > ops.PATCH_MAX_CHANNELS or max_length > ops.PATCH_MAX_LENGTH:
                raise ValueError(
                    "fused_patches takes channels of up to {} columns and patch_size * columns "
                    "up to {}, channel_dim up to {} and max_length up to {}; got {}, "
                    "patch_size {}, channel_dim {}, max_length {}".format(
                        ops.PATCH_MAX_WIDTH, ops.PATCH_MAX_PATCH_WIDTH, ops.PATCH_MAX_CHANNELS,
                        ops.PATCH_MAX_LENGTH, {n: widths[n] for n in fused}, patch_size,
                        channel_dim, max_length))
        self.fused_attention = bool(fused_attention)
        if self.fused_attention and (2 * max_length // patch_size > ops.SEQ_ATTENTION_MAX_LENGTH
                                     or dim // num_heads > ops.SEQ_ATTENTION_MAX_HEAD_DIM):
            raise ValueError(
                "fused_attention takes sequences of up to {} patches and heads of up to {} "
                "columns; got 2 * max_length / patch_size = {} and dim / num_heads = {}".format(
                    ops.SEQ_ATTENTION_MAX_LENGTH, ops.SEQ_ATTENTION_MAX_HEAD_DIM,
                    2 * max_length // patch_size, dim // num_heads))
        self.fused_feed_forward = _fused_route(fused_feed_forward)[0]
        if self.fused_feed_forward and dim > ops.FEED_FORWARD_MAX_WIDTH:
            raise ValueError(
                "fused_feed_forward takes up to {} columns; got {} channels of channel_dim "
                "{}".format(ops.FEED_FORWARD_MAX_WIDTH, len(self.channels), channel_dim))
        self.time_enc = TimeEncode(dim_time) if learn_time else FixedTimeEncode(dim_time)
        self.cooc_enc = NeighborCooccurrenceEncoder(channel_dim, max_count=max_length)
        self.proj = nn.ModuleDict({name: nn.Linear(patch_size * widths[name], channel_dim)
                                   for name in self.channels})
        self.blocks = nn.ModuleList(EncoderBlock(dim, num_heads, dropout, self.fused_attention,
                                                 self.fused_feed_forward)
                                    for _ in range(num_layers))
        self.out_fc = nn.Linear(dim, dim_embed)
        self.edge_predictor = EdgePredictor(dim_embed)

    def _check_length(self, L: int):
        if L != self.max_length:
            raise ValueError("sequences of {} slots per side, max_length is {}".format(
                L, self.max_length))

    def _padding(self, lengths: torch.Tensor, L: int) -> torch.Tensor:
        """bool [N, 2, L, 1]: the slots at and past lengths[i, side]"""
        return (torch.arange(L, device=lengths.device) >= lengths.unsqueeze(2)).unsqueeze(3)

    def _encode_time(self, delta_t: torch.Tensor, padding: torch.Tensor) -> torch.Tensor:
        time_x = self.time_enc(delta_t).reshape(tuple(delta_t.shape) + (self.dim_time,))
        return time_x.masked_fill(padding, 0.0)

    def forward(self, nodes: torch.Tensor, eids: torch.Tensor, delta_t: torch.Tensor,
                counts: torch.Tensor, lengths: torch.Tensor,
                node_feats: Optional[torch.Tensor] = None,
                edge_feats: Optional[torch.Tensor] = None, return_embed: bool = False):
        """
        Args:
            nodes, eids: int64 [N, 2, L], DynamicGraph.neighbor_cooccurrence(..., length=L,
                include_self=True)'s; an id without a row in its table (the self slot's eid, the
                padding's -1) takes the zero row
            delta_t: float [N, 2, L], the query time minus the slots' times
            counts: int [N, 2, L, 2], lengths: int [N, 2], that call's
            node_feats: float [rows, dim_node], edge_feats: float [rows, dim_edge], the tables
            return_embed: return (emb_src, emb_dst), [N, dim_embed] each, instead of the scores
        """
        self._check_length(delta_t.shape[2])
        if self.fused_patches and delta_t.is_cuda:
            return self._forward_fused(nodes, eids, delta_t, counts, lengths, node_feats,
                                       edge_feats, return_embed)
        padding = self._padding(lengths, delta_t.shape[2])
        node_x = edge_x = None
        if self.dim_node:
            node_x = _table_rows(node_feats, nodes).masked_fill(padding, 0.0)
        if self.dim_edge:
            edge_x = _table_rows(edge_feats, eids).masked_fill(padding, 0.0)
        return self.forward_parts(node_x, edge_x, self._encode_time(delta_t, padding), counts,
                                  lengths, return_embed)

    def forward_graph(self, graph, src: torch.Tensor, dst: torch.Tensor, ts: torch.Tensor,
                      node_feats: Optional[torch.Tensor] = None,
                      edge_feats: Optional[torch.Tensor] = None, since=None,
                      return_embed: bool = False):
        """forward() on what graph.pair_sequence(src, dst, ts, since=since, length=max_length)
        reads: one launch gives the planes and the finished parts.  With learn_time the reader
        is asked for no time part and the returned delta_t is encoded here, so that the
        encoder trains; no gradient flows to the tables either way.  With fused_patches the
        reader is asked for the planes alone and forward() projects from them."""
        if self.fused_patches and src.is_cuda:
            seq = graph.pair_sequence(src, dst, ts, since=since, length=self.max_length)
            return self._forward_fused(seq.nodes, seq.eids, seq.delta_t, seq.counts, seq.lengths,
                                       node_feats, edge_feats, return_embed)
        seq = graph.pair_sequence(
            src, dst, ts, since=since, length=self.max_length,
            node_feats=node_feats if self.dim_node else None,
            edge_feats=edge_feats if self.dim_edge else None,
            time_encoder=None if self.learn_time else self.time_enc)
        time_x = seq.time
        if self.learn_time:
            time_x = self._encode_time(seq.delta_t, self._padding(seq.lengths, self.max_length))
        return self.forward_parts(seq.node, seq.edge, time_x, seq.counts, seq.lengths,
                                  return_embed)

    def _forward_fused(self, nodes, eids, delta_t, counts, lengths, node_feats, edge_feats,
                       return_embed):
        """forward() without the node, edge and time parts: each of those channels' patches
        [N, 2, L / P, channel_dim] comes from ops.patch_project(_time) on the planes."""
        if counts.dim() != 4:
            raise ValueError("counts must be [N, 2, L, 2], got shape {}".format(
                tuple(counts.shape)))
        N, L, P = counts.shape[0], counts.shape[2], self.patch_size
        self._check_length(L)
        planes = {"node": (nodes, node_feats), "edge": (eids, edge_feats)}
        projected = []
        for name in self.channels:
            proj = self.proj[name]
            if name in planes:
                ids, table = planes[name]
                projected.append(ops.patch_project(ids, lengths, table, proj.weight, proj.bias, P))
            elif name == "time" and not self.learn_time:
                projected.append(ops.patch_project_time(
                    delta_t, lengths, self.time_enc.weight, self.time_enc.bias, proj.weight,
                    proj.bias, P))
            else:
                x = self.cooc_enc(counts, lengths) if name == "cooc" else \
                    self._encode_time(delta_t, self._padding(lengths, L))
                projected.append(proj(x.reshape(N, 2, L // P, P * x.shape[3])))
        return self._encode_patches(projected, N, L, return_embed)

    def forward_parts(self, node_x: Optional[torch.Tensor], edge_x: Optional[torch.Tensor],
                      time_x: torch.Tensor, counts: torch.Tensor, lengths: torch.Tensor,
                      return_embed: bool = False):
        """
        forward() from finished parts, whose padded slots are already zero.

        Args:
            node_x: float [N, 2, L, dim_node], edge_x: float [N, 2, L, dim_edge], time_x: float
                [N, 2, L, dim_time]: DynamicGraph.pair_sequence(...).node / .edge / .time
            counts: int [N, 2, L, 2], lengths: int [N, 2]: that call's
            return_embed: as in forward()
        """
        if counts.dim() != 4:
            raise ValueError("counts must be [N, 2, L, 2], got shape {}".format(
                tuple(counts.shape)))
        N, L, P = counts.shape[0], counts.shape[2], self.patch_size
        self._check_length(L)
        parts = {"node": node_x, "edge": edge_x, "time": time_x}
        projected = []
        for name in self.channels:
            x = self.cooc_enc(counts, lengths) if name == "cooc" else parts[name]
            width = self.proj[name].in_features // P
            if tuple(x.shape) != (N, 2, L, width):
                raise ValueError("the {} part must be [{}, 2, {}, {}], got {}".format(
                    name, N, L, width, tuple(x.shape)))
            projected.append(self.proj[name](x.reshape(N, 2, L // P, P * width)))
        return self._encode_patches(projected, N, L, return_embed)

    def _encode_patches(self, projected, N: int, L: int, return_embed: bool):
        """the model behind the channels' projections, [N, 2, L / P, channel_dim] each"""
        P = self.patch_size
        x = torch.cat(projected, dim=3)                       # [N, 2, L / P, C]
        x = x.reshape(N, 2 * (L // P), x.shape[3])
        for block in self.blocks:
            x = block(x)
        emb = self.out_fc(x.reshape(N, 2, L // P, x.shape[2]).mean(dim=2))
        emb_src, emb_dst = emb[:, 0], emb[:, 1]
        if return_embed:
            return emb_src, emb_dst
        return self.score(emb_src, emb_dst)

    def score(self, emb_src: torch.Tensor, emb_dst: torch.Tensor) -> torch.Tensor:
        """[N, 1]: edge_predictor's expression on row i of both, out_fc(relu(src_fc(emb_src) +
        dst_fc(emb_dst))); one ops.edge_score call where EdgePredictor would make one."""
        head = self.edge_predictor
        src_h, dst_h = head.src_fc(emb_src), head.dst_fc(emb_dst)
        if head.fused_score and src_h.is_cuda and src_h.shape[0] and \
                src_h.dtype == dst_h.dtype and \
                src_h.dtype in (torch.float32, torch.bfloat16) and \
                head.out_fc.weight.dtype == torch.float32:
            return ops.edge_score(src_h, dst_h, head.out_fc.weight, head.out_fc.bias)
        return head.out_fc(F.relu(src_h + dst_h))
