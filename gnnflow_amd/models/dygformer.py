"""DyGFormer (Yu et al., "Towards Better Dynamic Graph Learning: New Architecture and Unified
Library", NeurIPS 2023) per pair, on the readers of DynamicGraph: the newest interactions of both
ends of a pair, the node itself in front, as four channels -- node features, edge features, time
encoding and the neighbour co-occurrence feature -- which are patched, projected channel by
channel, concatenated and run through one transformer encoder over both sides' patches.  The
channels come finished from DynamicGraph.pair_sequence(..., node_feats=, edge_feats=,
time_encoder=model.time_enc) -- one kernel, padding already zero -- into forward_parts; forward
builds the same parts in torch from ids, time deltas and lengths.  Plain torch modules; the GEMMs
are torch's."""
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..nn import EdgePredictor, FixedTimeEncode, NeighborCooccurrenceEncoder, TimeEncode


class EncoderBlock(nn.Module):
    """One pre-norm transformer encoder block over x [n, S, C]: x + drop(MHA(LN(x))), then
    x + drop(W2 drop(gelu(W1 LN(x)))) with a hidden width of 4 C.  No padding mask."""

    def __init__(self, dim: int, num_heads: int, dropout: float):
        super().__init__()
        self.att_norm = nn.LayerNorm(dim)
        self.att = nn.MultiheadAttention(dim, num_heads, dropout=dropout, batch_first=True)
        self.ff_norm = nn.LayerNorm(dim)
        self.w1 = nn.Linear(dim, 4 * dim)
        self.w2 = nn.Linear(4 * dim, dim)
        self.drop = nn.Dropout(dropout)

    def forward(self, x):
        h = self.att_norm(x)
        x = x + self.drop(self.att(h, h, h, need_weights=False)[0])
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
    """

    def __init__(self, dim_node: int, dim_edge: int, dim_time: int = 100, channel_dim: int = 50,
                 patch_size: int = 1, num_layers: int = 2, num_heads: int = 2,
                 dropout: float = 0.1, max_length: int = 32, dim_embed: int = 100,
                 learn_time: bool = False):
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
        self.time_enc = TimeEncode(dim_time) if learn_time else FixedTimeEncode(dim_time)
        self.cooc_enc = NeighborCooccurrenceEncoder(channel_dim, max_count=max_length)
        self.proj = nn.ModuleDict({name: nn.Linear(patch_size * widths[name], channel_dim)
                                   for name in self.channels})
        self.blocks = nn.ModuleList(EncoderBlock(dim, num_heads, dropout)
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
        encoder trains; no gradient flows to the tables either way."""
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
