"""The reference's static GraphSAGE link predictor (gnnflow/models/graphsage.py): a stack of
nn.SAGEConv layers over the blocks of one snapshot and an MLP that scores source * destination.
Trains under torch.autocast('cuda', dtype=torch.bfloat16) as it is (nn.SAGEConv)."""
import torch.nn as nn
import torch.nn.functional as F

from ..nn import SAGEConv

AGGREGATORS = ['mean', 'gcn', 'pool', 'lstm']


def link_predictor(dim: int) -> nn.Sequential:
    """Linear-ReLU-Linear-ReLU-Linear(dim, 1): the scorer SAGE and GAT share."""
    return nn.Sequential(nn.Linear(dim, dim), nn.ReLU(), nn.Linear(dim, dim), nn.ReLU(),
                         nn.Linear(dim, 1))


def score_roots(predictor, h, neg_sample_ratio):
    """h = [src | pos dst | neg dst x ratio] rows -> (h_pos [B, 1], h_neg [B * ratio, 1]): the
    predictor on src * dst, the sources repeated block after block for the negatives."""
    B = h.shape[0] // (neg_sample_ratio + 2)
    src, pos, neg = h[:B], h[B:2 * B], h[2 * B:]
    return predictor(src * pos), predictor(src.tile(neg_sample_ratio, 1) * neg)


class SAGE(nn.Module):
    """`num_layers` SAGEConv layers (dim_node -> dim_out -> ... -> dim_out) with ReLU between
    them, named layers['l{l}h0'] (a static graph has one snapshot), and `predictor`.
    aggregator: 'mean', 'gcn', 'pool' or 'lstm'; the last is a name the model accepts and the
    layer does not build (NotImplementedError)."""

    def __init__(self, dim_node: int, dim_out: int, num_layers: int = 2, aggregator='mean'):
        if aggregator not in AGGREGATORS:
            raise ValueError("aggregator {} is not in {}".format(aggregator, AGGREGATORS))
        super().__init__()
        self.num_layers = num_layers
        self.dim_out = dim_out
        self.layers = nn.ModuleDict()
        for l in range(num_layers):
            self.layers['l{}h0'.format(l)] = SAGEConv(dim_node if l == 0 else dim_out, dim_out,
                                                      aggregator)
        self.predictor = link_predictor(dim_out)

    def reset(self):
        """Nothing to reset: the model keeps no state between batches."""

    def forward(self, mfgs, neg_sample_ratio: int = 1, *args, **kwargs):
        """mfgs[l][0]: the block of layer l, outermost first, with mfgs[0][0].srcdata['h'] set;
        the roots of the last block are [src | pos dst | neg dst x neg_sample_ratio].  Returns
        (h_pos, h_neg).  Writes srcdata['h'] of the inner blocks."""
        for l in range(self.num_layers):
            b = mfgs[l][0]
            h = self.layers['l{}h0'.format(l)](b, b.srcdata['h'])
            if l != self.num_layers - 1:
                h = F.relu(h)
                mfgs[l + 1][0].srcdata['h'] = h
        return score_roots(self.predictor, h, neg_sample_ratio)
