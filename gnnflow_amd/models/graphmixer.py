"""GraphMixer (Cong et al., "Do We Really Need Complicated Model Architectures For Temporal
Networks?", ICLR 2023) per node, on the readers of DynamicGraph: the link encoder is an MLP-Mixer
over a node's newest K interactions, the node encoder is the node's own features plus the mean of
the features of the nodes it met (DynamicGraph.neighbor_aggregate).  The link encoder's tokens
come finished from DynamicGraph.neighbor_sequence(..., edge_feats=, time_encoder=model.time_enc)
-- one kernel, padding already zero -- into forward_tokens; forward builds the same tokens in
torch from edge features, time deltas and lengths.  Plain torch modules; the GEMMs are torch's."""
from typing import Optional

import torch
import torch.nn as nn

from ..nn import EdgePredictor, FixedTimeEncode


class _FeedForward(nn.Module):
    """Linear -> GELU -> dropout -> Linear -> dropout over the last dimension."""

    def __init__(self, dim: int, expansion: float, dropout: float):
        super().__init__()
        hidden = max(1, int(expansion * dim))
        self.net = nn.Sequential(nn.Linear(dim, hidden), nn.GELU(), nn.Dropout(dropout),
                                 nn.Linear(hidden, dim), nn.Dropout(dropout))

    def forward(self, x):
        return self.net(x)


class MixerBlock(nn.Module):
    """One MLP-Mixer block over x [n, K, C]: x + token MLP over K of LayerNorm(x), then
    x + channel MLP over C of LayerNorm(x)."""

    def __init__(self, num_tokens: int, dim: int, token_expansion: float,
                 channel_expansion: float, dropout: float):
        super().__init__()
        self.token_norm = nn.LayerNorm(dim)
        self.token_mlp = _FeedForward(num_tokens, token_expansion, dropout)
        self.channel_norm = nn.LayerNorm(dim)
        self.channel_mlp = _FeedForward(dim, channel_expansion, dropout)

    def forward(self, x):
        x = x + self.token_mlp(self.token_norm(x).transpose(1, 2)).transpose(1, 2)
        return x + self.channel_mlp(self.channel_norm(x))


class GraphMixer(nn.Module):
    """
    GraphMixer, one embedding per node:

        tokens   = [edge_x | time_enc(delta_t)], the slots p >= lengths set to zero   [n, K, .]
        link     = mean over K of mixers(link_in(tokens))                           [n, dim_embed]
        node     = node_x + nbr_mean                                                [n, dim_node]
        embed    = out_fc([link | node])                                            [n, dim_embed]

        time_enc         FixedTimeEncode(dim_time), frozen
        link_in          Linear(dim_edge + dim_time, dim_embed)
        mixers           num_layers MixerBlocks over K = num_tokens tokens
        out_fc           Linear(dim_embed + dim_node, dim_embed)
        edge_predictor   the link-prediction head, over rows laid out [src | dst | negatives]

    The padded slots are replaced, not multiplied: whatever they hold (NaN too) leaves the result
    unchanged.  dim_node == 0 drops the node part (node_x and nbr_mean are then ignored), and
    dim_edge == 0 leaves the time encoding as the token (edge_x is then ignored).
    """

    def __init__(self, dim_node: int, dim_edge: int, dim_time: int = 100, dim_embed: int = 100,
                 num_tokens: int = 32, num_layers: int = 2, token_expansion: float = 0.5,
                 channel_expansion: float = 4.0, dropout: float = 0.1):
        super().__init__()
        self.dim_node, self.dim_edge, self.dim_time = dim_node, dim_edge, dim_time
        self.dim_embed, self.num_tokens, self.num_layers = dim_embed, num_tokens, num_layers
        self.time_enc = FixedTimeEncode(dim_time)
        self.link_in = nn.Linear(dim_edge + dim_time, dim_embed)
        self.mixers = nn.ModuleList(
            MixerBlock(num_tokens, dim_embed, token_expansion, channel_expansion, dropout)
            for _ in range(num_layers))
        self.out_fc = nn.Linear(dim_embed + dim_node, dim_embed)
        self.edge_predictor = EdgePredictor(dim_embed)

    def forward(self, edge_x: Optional[torch.Tensor], delta_t: torch.Tensor,
                lengths: torch.Tensor, node_x: Optional[torch.Tensor] = None,
                nbr_mean: Optional[torch.Tensor] = None, return_embed: bool = False):
        """
        Args:
            edge_x: float [n, K, dim_edge], the features of each node's newest K edges
            delta_t: float [n, K], the query time minus the edges' times
            lengths: int [n], the filled slots of each row; slots p >= lengths[i] are padding
            node_x: float [n, dim_node], the nodes' own features
            nbr_mean: float [n, dim_node], DynamicGraph.neighbor_aggregate(...).node
            return_embed: return the embeddings [n, dim_embed] instead of the edge predictor's
                (pos, neg), for which n is a multiple of 3 laid out [src | dst | negatives]
        """
        n, K = delta_t.shape
        if K != self.num_tokens:
            raise ValueError("delta_t has {} slots per row, num_tokens is {}".format(
                K, self.num_tokens))
        parts = [self.time_enc(delta_t)]
        if self.dim_edge > 0:
            parts.insert(0, edge_x)
        tokens = torch.cat(parts, dim=2)
        padding = torch.arange(K, device=delta_t.device) >= lengths.reshape(n, 1)
        return self.forward_tokens(tokens.masked_fill(padding.unsqueeze(2), 0.0), node_x,
                                   nbr_mean, return_embed)

    def forward_tokens(self, tokens: torch.Tensor, node_x: Optional[torch.Tensor] = None,
                       nbr_mean: Optional[torch.Tensor] = None, return_embed: bool = False):
        """
        forward() from finished tokens, whose padded slots are already zero.

        Args:
            tokens: float [n, K, dim_edge + dim_time], [edge_x | time_enc(delta_t)] with zeros in
                the padding: DynamicGraph.neighbor_sequence(nodes, ts, length=K,
                edge_feats=..., time_encoder=self.time_enc).tokens (without edge_feats when
                dim_edge == 0)
            node_x, nbr_mean, return_embed: as in forward()
        """
        if tokens.dim() != 3 or tokens.shape[1] != self.num_tokens or \
                tokens.shape[2] != self.dim_edge + self.dim_time:
            raise ValueError("tokens must be [n, {}, {}], got {}".format(
                self.num_tokens, self.dim_edge + self.dim_time, tuple(tokens.shape)))
        x = self.link_in(tokens)
        for mixer in self.mixers:
            x = mixer(x)
        h = x.mean(dim=1)
        if self.dim_node > 0:
            h = torch.cat([h, node_x + nbr_mean], dim=1)
        embed = self.out_fc(h)
        if return_embed:
            return embed
        return self.edge_predictor(embed)
