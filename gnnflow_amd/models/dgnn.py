"""DGNN, the reference's temporal model (gnnflow/models/dgnn.py; TGN, TGAT and DySAT are its
configurations) with the same constructor, attributes, sub-module names and methods, on the
layers of gnnflow_amd.nn and the HBM-resident gnnflow_amd.memory.Memory."""
from typing import Dict, List, Optional, Union

import torch

from ..memory import Memory
from ..nn import EdgePredictor, GRUMemoryUpdater, TemporalAttentionLayer


class DGNN(torch.nn.Module):
    """
    Dynamic Graph Neural Model (DGNN)

        layers['l{l}h{h}']   one TemporalAttentionLayer per layer l and snapshot h
        combiner             torch.nn.RNN over the snapshots' embeddings (num_snapshots > 1)
        memory, memory_updater   TGN's memory and its GRU updater (use_memory)
        edge_predictor       the link-prediction head

    As in the reference, forward() runs the layers, the combiner and the head; with memory the
    caller runs memory.prepare_input and memory_updater on the input block before it, keeps
    the updater's result in `last_updated`, and calls memory.update_mem_mail after it.
    """

    def __init__(self, dim_node: int, dim_edge: int, dim_time: int,
                 dim_embed: int, num_layers: int, num_snapshots: int,
                 att_head: int, dropout: float, att_dropout: float,
                 use_memory: bool, dim_memory: Optional[int] = None,
                 num_nodes: Optional[int] = None,
                 memory_device: Union[torch.device, str] = 'cuda',
                 memory_shared: bool = False,
                 kvstore_client=None,
                 *args, **kwargs):
        """
        Args:
            dim_node: dimension of node features/embeddings
            dim_edge: dimension of edge features
            dim_time: dimension of time features
            dim_embed: dimension of output embeddings
            num_layers: number of layers
            num_snapshots: number of snapshots
            att_head: number of heads for attention
            dropout: dropout rate
            att_dropout: dropout rate for attention
            use_memory: whether to use memory
            dim_memory: dimension of memory
            num_nodes: number of nodes in the graph
            memory_device: device of the memory; 'cuda' (the default) is the current GPU, since
                the memory lives in HBM
            memory_shared: accepted and ignored (every rank keeps its own tables)
            kvstore_client: must be None (the multi-machine KVStore memory is out of scope)
        """
        super().__init__()
        self.dim_node = dim_node
        self.dim_node_input = dim_node
        self.dim_edge = dim_edge
        self.dim_time = dim_time
        self.dim_embed = dim_embed
        self.num_layers = num_layers
        self.num_snapshots = num_snapshots
        self.att_head = att_head
        self.dropout = dropout
        self.att_dropout = att_dropout
        self.use_memory = use_memory

        if self.use_memory:
            assert num_snapshots == 1, 'memory is not supported for multiple snapshots'
            assert dim_memory is not None, 'dim_memory should be specified'
            assert num_nodes is not None, 'num_nodes is required when using memory'
            self.memory = Memory(num_nodes, dim_edge, dim_memory, memory_device, memory_shared,
                                 kvstore_client)
            self.memory_updater = GRUMemoryUpdater(dim_node, dim_edge, dim_time, dim_embed,
                                                   dim_memory)
            dim_node = dim_memory

        self.layers = torch.nn.ModuleDict()
        for l in range(num_layers):
            for h in range(num_snapshots):
                key = 'l' + str(l) + 'h' + str(h)
                self.layers[key] = TemporalAttentionLayer(
                    dim_node if l == 0 else dim_embed, dim_edge, dim_time, dim_embed, att_head,
                    dropout, att_dropout)

        if self.num_snapshots > 1:
            self.combiner = torch.nn.RNN(dim_embed, dim_embed)

        self.last_updated = None
        self.edge_predictor = EdgePredictor(dim_embed)

    def reset(self):
        if self.use_memory:
            self.memory.reset()

    def resize(self, num_nodes: int):
        if self.use_memory:
            self.memory.resize(num_nodes)

    def has_memory(self):
        return self.use_memory

    def backup_memory(self) -> Dict:
        if self.use_memory:
            return self.memory.backup()
        return {}

    def restore_memory(self, backup: Dict):
        if self.use_memory:
            self.memory.restore(backup)

    def forward(self, mfgs: List[List], return_embed: bool = False):
        """
        Args:
            mfgs: list (layers) of list (snapshots) of blocks, input layer first
            return_embed: return the embeddings instead of the edge predictor's (pos, neg)
        """
        out = list()
        for l in range(self.num_layers):
            for h in range(self.num_snapshots):
                key = 'l' + str(l) + 'h' + str(h)
                rst = self.layers[key](mfgs[l][h])
                if l != self.num_layers - 1:
                    mfgs[l + 1][h].srcdata['h'] = rst
                else:
                    out.append(rst)

        if self.num_snapshots == 1:
            embed = out[0]
        else:
            embed = torch.stack(out, dim=0)
            embed = self.combiner(embed)[0][-1, :, :]

        if return_embed:
            return embed
        return self.edge_predictor(embed)
