"""Message passing on an MFGBlock: the DGL calls the reference's layers
make on a sampled block, on HIP segment kernels (csrc/block_ops.hip) with autograd.

    edge_softmax(block, logits)            dgl.ops.edge_softmax      (layers.py:153)
    block.update_all(fn.copy_src('v','m'), fn.sum('m','h'))          (layers.py:159)
    copy_u / u_mul_e messages, sum / mean reducers                   (dgl.nn.SAGEConv / GATConv)
    block_attention(block, q, k, v)        layers.py:144-159 in one launch (csrc/block_attention.hip)
      ... dropout_p=, dropout_seed=        with the attention dropout of layers.py:155 inside it, from a
                                           stateless Philox mask (no mask tensor, reproducible on the CPU)
    block_gat(block, feat, el, er)         dgl.nn.GATConv's u_add_v -> leaky_relu -> edge_softmax ->
                                           (attn_drop) -> u_mul_e + sum in one launch each way
                                           (csrc/block_gat.hip), the same dropout_p= / dropout_seed=
    time_encode_cat(parts, t, w, b)        torch.cat([*parts, TimeEncode(t)], 1) in one launch
                                           (layers.py:16-42, 118-137; csrc/time_encode.hip)
    edge_score(src, dst, w, b)             out_fc(relu(src + dst)) of EdgePredictor (layers.py:195-197),
                                           every dst block against the one src block, in one launch
                                           (csrc/edge_score.hip)
    dropout_relu_layer_norm(x, w, b)       layer_norm(relu(dropout(x))), the last line of
                                           TemporalAttentionLayer.forward after w_out, in one launch
                                           with the Philox mask of block_attention, redrawn in the
                                           backward (csrc/layer_epilogue.hip)
    gru_cell(gi, gh, hx, residual)         everything torch.nn.GRUCell does behind its two GEMMs, the
                                           residual add of the memory updater and the copy of the
                                           first rows for Memory.update_mem_mail
                                           (memory_updater.py:62-85), one launch each way without a
                                           workspace (csrc/gru_cell.hip)
    link_metrics(pos, neg)                 average_precision_score / roc_auc_score of the reference's
                                           evaluate() (scripts/offline_edge_prediction.py:141-146) and
                                           the MRR, counted on the GPU without a sort, a sync or a copy
                                           to the host (csrc/link_metrics.hip)
    link_loss(pos, neg)                    criterion(pred_pos, ones) + criterion(pred_neg, zeros) of the
                                           reference's training step (BCEWithLogitsLoss), one launch
                                           each way, with a running epoch sum on the device
                                           (csrc/link_loss.hip)
    edge_rank(src, cand, w, b, k, ...)     the edge score of every source against one shared candidate
                                           set, of which the top k and the rank counts of a reference
                                           score are kept and nothing else is stored
                                           (csrc/edge_rank.hip); no autograd
    walk_position_counts(nodes, ref)       the position-count ("anonymous") encoding of the walks
                                           DynamicGraph.temporal_random_walk returns, CAWN's
                                           set-based anonymisation (csrc/walk_positions.hip); integers,
                                           no autograd

block_attention, block_reduce, block_max, block_gat, time_encode_cat, edge_score, link_loss,
gru_cell and dropout_relu_layer_norm also run on bfloat16 (the tensors autocast hands them), by one rule: float32 arithmetic, one rounding on
store.  Every bfloat16 element is widened to float32 where it is loaded (exact), the arithmetic is
the float32 kernels' own in the same order, and each bfloat16 result is rounded once, to nearest
even.  So op(x.bfloat16()) == op(x.bfloat16().float()).to(torch.bfloat16) bit for bit, forward and
backward, and the float32 outputs (attention, scores, parameter gradients) are equal.  The ops
choose by the dtypes they are given and behave the same inside and outside an autocast region.
What may be bfloat16 is what autocast makes bfloat16, the rows a Linear returns: q / k / v, the
source rows of block_reduce and block_max, feat of block_gat.  What autocast leaves float32 stays
float32 only: edge weights (a softmax output), el and er (a float32 sum), and edge_softmax
altogether.  A gradient of a source may meet several edges (an explicit col): it is summed in a
float32 scratch and rounded once, never once per edge.

A block's edges are grouped by destination (the sampler emits them that way); blocks built by
hand with unordered edges are handled through a stable permutation.

The ops live in one module per kernel family, split as the csrc/ sources are: block.py
(block_ops.hip), attention.py (block_attention.hip, block_gat.hip), time_encoding.py
(time_encode.hip; not time_encode.py, which the op of that name would shadow), edge.py
(edge_score.hip, edge_rank.hip), layer.py (layer_epilogue.hip, gru_cell.hip), link.py
(link_loss.hip, link_metrics.hip), walks.py (walk_positions.hip); _common.py holds the one path
to a native launch and the argument checks they share.  This file only re-exports: callers look
an op up as an attribute of this package at call time (`ops.block_attention(...)`), which is
where a replacement of it is seen; nothing binds an op with `from .ops import ...`.
"""
# Tests and scripts reach for private names too (ops._grad_as, ops._NoEdgeGat, ops.torch): the
# whole of what `gnnflow_amd.ops.<name>` resolves is kept, the imported modules included.
import ctypes as C
from typing import NamedTuple, Optional

import torch

from .. import _capi
from ..dynamic_graph import WALK_MAX_LENGTH
from ._common import _bwd, _f32, _fwd, _grad_as, _ptr, _scratch, _stream
from .attention import (MAX_ATTENTION_WIDTH, _BlockAttention, _BlockGat, _NoEdgeAttention,
                        _NoEdgeGat, block_attention, block_gat)
from .block import (_BlockMax, _BlockReduce, _EdgeSoftmax, _src_dtype, block_max, block_reduce,
                    edge_softmax)
from .edge import EDGE_RANK_CHUNK, EDGE_RANK_MAX_K, EdgeRank, _EdgeScore, edge_rank, edge_score
from .layer import (LAYER_EPILOGUE_MAX_WIDTH, _DropoutReluLayerNorm, _GruCell,
                    dropout_relu_layer_norm, gru_cell)
from .link import (_LINK_METRICS_PARTIAL_WORDS, LINK_LOSS_ACC_FIELDS,
                   LINK_LOSS_MAX_PARTIAL_ROWS, LINK_LOSS_SINGLE_TILES, LINK_LOSS_TILE,
                   LINK_METRICS_MAX_SCORES, LINK_METRICS_TILE, _LinkLoss, link_loss,
                   link_metrics)
from .time_encoding import _time_encode_cat, _TimeEncodeCat, time_encode, time_encode_cat
from .walks import WALK_MAX_REF_ENTRIES, check_walk_position_counts_args, walk_position_counts

_BlockAttentionDropout = _BlockAttention      # the dropout path is the same Function (p > 0)
