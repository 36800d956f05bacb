"""The reference's static GAT link predictor (gnnflow/models/gat.py): a stack of nn.GATConv
layers over the blocks of one snapshot and the MLP of models.SAGE on source * destination.
Trains under torch.autocast('cuda', dtype=torch.bfloat16) as it is (nn.GATConv)."""
import torch.nn as nn
import torch.nn.functional as F

from ..nn import GATConv
from .graphsage import link_predictor, score_roots


class GAT(nn.Module):
    """`num_layers` GATConv layers named layers['l{l}h0'], layer l with attn_head[l] heads of
    dim_out columns; the heads are flattened between layers and averaged after the last, and
    only the first layer has an activation (ELU)."""

    def __init__(self, dim_in: int, dim_out: int, num_layers: int = 2, attn_head=[8, 1],
                 feat_drop: float = 0, attn_drop: float = 0, allow_zero_in_degree: bool = True):
        if num_layers != len(attn_head):
            raise ValueError("length of attn head {} must equal to num_layers {}".format(
                attn_head, num_layers))
        super().__init__()
        self.num_layers = num_layers
        self.dim_out = dim_out
        self.layers = nn.ModuleDict()
        for l in range(num_layers):
            self.layers['l{}h0'.format(l)] = GATConv(
                dim_in if l == 0 else dim_out * attn_head[l - 1], dim_out, attn_head[l],
                feat_drop=feat_drop, attn_drop=attn_drop, activation=F.elu if l == 0 else None,
                allow_zero_in_degree=allow_zero_in_degree)
        self.predictor = link_predictor(dim_out)

    def reset(self):
        """Nothing to reset: the model keeps no state between batches."""

    def forward(self, mfgs, neg_sample_ratio: int = 1, *args, **kwargs):
        """As SAGE.forward: mfgs[l][0] the block of layer l, roots [src | pos dst | neg dst x
        neg_sample_ratio]; returns (h_pos, h_neg)."""
        for l in range(self.num_layers):
            b = mfgs[l][0]
            h = self.layers['l{}h0'.format(l)](b, b.srcdata['h'])
            if l != self.num_layers - 1:
                h = h.flatten(1)
                mfgs[l + 1][0].srcdata['h'] = h
            else:
                h = h.mean(1)
        return score_roots(self.predictor, h, neg_sample_ratio)
