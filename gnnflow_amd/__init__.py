"""gnnflow_amd — MI355X-native temporal neighbour sampler + feature gather for GNNFlow.

Drop-in for the hot path of jasperzhong/GNNFlow: `DynamicGraph`, `TemporalSampler`,
`cache.LRUCache` keep the reference's Python API; the work runs in hand-written HIP
kernels (gfx950) behind the C ABI of include/gnnflow_hip.h.
"""
from .baselines import EdgeBank, NeighborOverlap
from .data import DeviceBatchStream, DeviceDstSet
from .dynamic_graph import (CommonNeighbors, DynamicGraph, NeighborAggregate,
                            NeighborCooccurrence, NeighborSequence, PairHistory,
                            PairSequence, TemporalWalks)
from .metrics import LinkMetrics
from .mfg import MFGBlock
from .nn import (MLP, EdgePredictor, FixedTimeEncode, GATConv, GRUMemeoryUpdater,
                 GRUMemoryUpdater, LinkLoss, NeighborCooccurrenceEncoder, SAGEConv,
                 TemporalAttentionLayer, TimeEncode, TransfomerAttentionLayer)
from .temporal_sampler import SamplingResult, TemporalSampler

__all__ = ["DynamicGraph", "TemporalSampler", "SamplingResult", "MFGBlock", "SAGEConv", "GATConv",
           "TimeEncode", "TemporalAttentionLayer", "TransfomerAttentionLayer", "GRUMemoryUpdater",
           "GRUMemeoryUpdater", "EdgePredictor", "MLP", "LinkMetrics", "LinkLoss",
           "DeviceDstSet", "DeviceBatchStream", "TemporalWalks", "PairHistory", "EdgeBank",
           "CommonNeighbors", "NeighborOverlap", "NeighborCooccurrence",
           "NeighborCooccurrenceEncoder", "NeighborAggregate", "FixedTimeEncode",
           "NeighborSequence", "PairSequence"]
