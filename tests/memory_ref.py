"""
memory_ref.py — TEST INFRASTRUCTURE, NOT PRODUCT CODE.

A sequential restatement of the TGN memory module, independent of oracle/memory_oracle.py: the
same four tables, and update_mem_mail as two plain loops that apply one write per position, in
order.  The last writer of a node wins because it writes last; there is no "unique" step and no
winner selection to get wrong.  Ids outside [0, num_nodes) are skipped by the update (for the
table whose loop meets them) and read back as all-zero rows.
"""
import numpy as np


class RefMemory:
    def __init__(self, num_nodes, dim_edge, dim_memory):
        self.num_nodes, self.dim_edge, self.dim_memory = num_nodes, dim_edge, dim_memory
        self.dim_raw_message = 2 * dim_memory + dim_edge
        self.node_memory = np.zeros((num_nodes, dim_memory), np.float32)
        self.node_memory_ts = np.zeros(num_nodes, np.float32)
        self.mailbox = np.zeros((num_nodes, self.dim_raw_message), np.float32)
        self.mailbox_ts = np.zeros(num_nodes, np.float32)

    def tables(self):
        return self.node_memory, self.mailbox, self.node_memory_ts, self.mailbox_ts

    def reset(self):
        for t in self.tables():
            t[...] = 0

    def resize(self, num_nodes):
        if num_nodes <= self.num_nodes:
            return
        def grow(t):
            n = np.zeros((num_nodes,) + t.shape[1:], np.float32)
            n[:t.shape[0]] = t
            return n
        self.node_memory, self.mailbox = grow(self.node_memory), grow(self.mailbox)
        self.node_memory_ts, self.mailbox_ts = grow(self.node_memory_ts), grow(self.mailbox_ts)
        self.num_nodes = num_nodes

    def backup(self):
        return [t.copy() for t in self.tables()]

    def restore(self, backup):
        for t, b in zip(self.tables(), backup):
            t[...] = b

    def prepare_input(self, ids):
        """(mem, mem_ts, mail_ts, mem_input) = rows of the tables, zero rows for unknown ids."""
        ids = [int(v) for v in np.asarray(ids).reshape(-1)]
        n = len(ids)
        mem = np.zeros((n, self.dim_memory), np.float32)
        mem_ts = np.zeros(n, np.float32)
        mail_ts = np.zeros(n, np.float32)
        mem_input = np.zeros((n, self.dim_raw_message), np.float32)
        for r, v in enumerate(ids):
            if 0 <= v < self.num_nodes:
                mem[r] = self.node_memory[v]
                mem_ts[r] = self.node_memory_ts[v]
                mail_ts[r] = self.mailbox_ts[v]
                mem_input[r] = self.mailbox[v]
        return mem, mem_ts, mail_ts, mem_input

    def update_mem_mail(self, nid, memory, ts, edge_feats=None, neg_sample_ratio=1):
        nid = [int(v) for v in np.asarray(nid).reshape(-1)]
        memory = np.asarray(memory, np.float32)
        ts = np.asarray(ts, np.float32)
        B = len(nid) // (2 + neg_sample_ratio)
        if edge_feats is None:
            edge_feats = np.zeros((B, self.dim_edge), np.float32)
        edge_feats = np.asarray(edge_feats, np.float32)
        dm = self.dim_memory
        # the mailbox: positions interleaved src0, dst0, src1, dst1, ...
        for j in range(2 * B):
            i = j // 2
            me, other = (i, B + i) if j % 2 == 0 else (B + i, i)
            node = nid[me]
            if not 0 <= node < self.num_nodes:
                continue
            self.mailbox[node, :dm] = memory[me]
            self.mailbox[node, dm:2 * dm] = memory[other]
            self.mailbox[node, 2 * dm:] = edge_feats[i]
            self.mailbox_ts[node] = ts[j]
        # the memory: positions in the order of nid[:2B], src.. then dst..
        for j in range(2 * B):
            node = nid[j]
            if not 0 <= node < self.num_nodes:
                continue
            self.node_memory[node] = memory[j]
            self.node_memory_ts[node] = ts[j]
