"""GraphMixer (Cong et al., "Do We Really Need Complicated Model Architectures For Temporal
Networks?", ICLR 2023) per node, on the readers of DynamicGraph: the link encoder is an MLP-Mixer
over a node's newest K interactions, the node encoder is the node's own features plus the mean of
the features of the nodes it met (DynamicGraph.neighbor_aggregate).  The link encoder's tokens
come finished from DynamicGraph.neighbor_sequence(..., edge_feats=, time_encoder=model.time_enc)
-- one kernel, padding already zero -- into forward_tokens; forward builds the same tokens in
torch from edge features, time deltas and lengths.  Plain torch modules; the GEMMs are torch's --
except with fused_feed_forward=True, where each mixer block's channel MLP is one ops.feed_forward
call, and with fused_token_mix=True, where its token half is one ops.token_mix call."""
from typing import Optional

import torch
import torch.nn as nn

from .. import ops
from ..nn import EdgePredictor, FixedTimeEncode
from ..ops.feed_forward import _fused_route


class _FeedForward(nn.Module):
    """Linear -> GELU -> dropout -> Linear -> dropout over the last dimension.

    fused=True (a route, not state: the same parameters and state_dict keys) takes everything but
    the trailing dropout of a float32 x on a GPU, outside autocast, from ops.feed_forward: the
    inner Dropout's p in training and 0 otherwise, the seed drawn per forward from torch's
    default CPU generator (no device sync).  Any other x takes the torch route.
    fused="bfloat16" is that route with compute_dtype=torch.bfloat16, taken inside a bfloat16
    autocast region too (the LayerNorm output it is given there is float32); any other value of
    the flag raises ValueError."""

    def __init__(self, dim: int, expansion: float, dropout: float, fused=False):
        super().__init__()
        hidden = max(1, int(expansion * dim))
        self.fused, self._dtype = _fused_route(fused)
        if self.fused and dim > ops.FEED_FORWARD_MAX_WIDTH:
            raise ValueError("fused_feed_forward takes a width of up to {}, got {}".format(
                ops.FEED_FORWARD_MAX_WIDTH, dim))
        self.net = nn.Sequential(nn.Linear(dim, hidden), nn.GELU(), nn.Dropout(dropout),
                                 nn.Linear(hidden, dim), nn.Dropout(dropout))

    def forward(self, x):
        if self.fused and x.is_cuda and x.dtype == torch.float32 and \
                (self._dtype == torch.bfloat16 or not torch.is_autocast_enabled()):
            w1, _, drop, w2, last = self.net
            p = drop.p if self.training else 0.0
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64)) if p > 0 else None
            return last(ops.feed_forward(x.contiguous(), w1.weight, w1.bias, w2.weight, w2.bias,
                                         p, seed, compute_dtype=self._dtype))
        return self.net(x)


class MixerBlock(nn.Module):
    """One MLP-Mixer block over x [n, K, C]: x + token MLP over K of LayerNorm(x), then
    x + channel MLP over C of LayerNorm(x).  fused_feed_forward=True routes the channel MLP
    through ops.feed_forward, "bfloat16" through its bfloat16 kernels.
    fused_token_mix=True (a route too, independent of the other: the
    same parameters and state_dict keys) takes the whole first line -- token_norm, the token MLP
    over the K tokens with its hidden width of K / 2, both dropouts and the residual -- of a
    float32 x on a GPU, outside autocast, from ops.token_mix, without the transposed [n, C, K]
    copy: the token Dropout's p in training and 0 otherwise, the seed drawn per forward from
    torch's default CPU generator (no device sync).  Any other x takes the torch route.  With both
    flags a block is two native calls and one LayerNorm."""

    def __init__(self, num_tokens: int, dim: int, token_expansion: float,
                 channel_expansion: float, dropout: float, fused_feed_forward=False,
                 fused_token_mix: bool = False):
        super().__init__()
        self.fused_token_mix = bool(fused_token_mix)
        hidden = max(1, int(token_expansion * num_tokens))
        if self.fused_token_mix and max(num_tokens, hidden) > ops.TOKEN_MIX_MAX_TOKENS:
            raise ValueError("fused_token_mix takes up to {} tokens and hidden units, got {} and "
                             "{}".format(ops.TOKEN_MIX_MAX_TOKENS, num_tokens, hidden))
        if self.fused_token_mix and dim > ops.TOKEN_MIX_MAX_WIDTH:
            raise ValueError("fused_token_mix takes a width of up to {}, got {}".format(
                ops.TOKEN_MIX_MAX_WIDTH, dim))
        self.token_norm = nn.LayerNorm(dim)
        self.token_mlp = _FeedForward(num_tokens, token_expansion, dropout)
        self.channel_norm = nn.LayerNorm(dim)
        self.channel_mlp = _FeedForward(dim, channel_expansion, dropout, fused_feed_forward)

    def forward(self, x):
        if self.fused_token_mix and x.is_cuda and x.dtype == torch.float32 and \
                not torch.is_autocast_enabled():
            w1, _, drop, w2, _ = self.token_mlp.net
            p = drop.p if self.training else 0.0
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64)) if p > 0 else None
            x = ops.token_mix(x.contiguous(), self.token_norm.weight, self.token_norm.bias,
                              w1.weight, w1.bias, w2.weight, w2.bias, self.token_norm.eps, p, seed)
        else:
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

    fused_feed_forward=True (off by default; README "feed_forward" has the measurements) takes
    every mixer block's channel MLP from ops.feed_forward on a GPU, the [n, K, 4 C] hidden
    tensors never stored.  A route, not state: the parameters and the state_dict are the same.
    dim_embed may then be at most ops.FEED_FORWARD_MAX_WIDTH.  fused_feed_forward="bfloat16" runs
    that kernel's products on the bfloat16 matrix instruction (ops.feed_forward's compute_dtype),
    under bfloat16 autocast too, where True falls back to torch.

    fused_token_mix=True (off by default, independent of the other flag; README "token_mix" has
    the measurements) takes every mixer block's token half -- LayerNorm, the MLP over the K
    tokens, both dropouts and the residual -- from ops.token_mix on a GPU, with no transposed
    copy and no [n, C, K / 2] hidden tensor.  A route too.  num_tokens and its hidden width may
    then be at most ops.TOKEN_MIX_MAX_TOKENS, dim_embed at most ops.TOKEN_MIX_MAX_WIDTH.
    """

    def __init__(self, dim_node: int, dim_edge: int, dim_time: int = 100, dim_embed: int = 100,
                 num_tokens: int = 32, num_layers: int = 2, token_expansion: float = 0.5,
                 channel_expansion: float = 4.0, dropout: float = 0.1,
                 fused_feed_forward=False, fused_token_mix: bool = False):
        super().__init__()
        self.fused_feed_forward = _fused_route(fused_feed_forward)[0]
        self.fused_token_mix = bool(fused_token_mix)
        self.dim_node, self.dim_edge, self.dim_time = dim_node, dim_edge, dim_time
        self.dim_embed, self.num_tokens, self.num_layers = dim_embed, num_tokens, num_layers
        self.time_enc = FixedTimeEncode(dim_time)
        self.link_in = nn.Linear(dim_edge + dim_time, dim_embed)
        self.mixers = nn.ModuleList(
            MixerBlock(num_tokens, dim_embed, token_expansion, channel_expansion, dropout,
                       self.fused_feed_forward, self.fused_token_mix)
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
