"""tests/memory_ref.py (the sequential restatement the GPU edge tests compare against) is itself
pinned three ways: to the reference module's recorded run, to the numpy oracle on random valid
sequences, and to hand-written tables for the ids outside [0, num_nodes) that neither of the
other two covers."""
import os

import numpy as np

from oracle.memory_oracle import OracleMemory
from tests.memory_ref import RefMemory

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "memory_reference.npz")


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and \
        np.array_equal(a.view(np.int32), b.view(np.int32))


def test_replays_the_reference_module():
    z = np.load(FIX)
    N, de, dm, B, steps = (int(x) for x in z["meta"])
    m = RefMemory(N, de, dm)
    for s in range(steps):
        ef = z["s%d/ef" % s] if ("s%d/ef" % s) in z.files else None
        m.update_mem_mail(z["s%d/nid" % s], z["s%d/memory" % s], z["s%d/ts" % s], ef,
                          int(z["s%d/neg" % s][0]))
        got = m.prepare_input(z["s%d/query" % s])
        for k, g in zip(("mem", "mem_ts", "mail_ts", "mem_input"), got):
            assert _same(g, z["s%d/%s" % (s, k)]), (s, k)
        for k, g in zip(("node_memory", "mailbox", "node_memory_ts", "mailbox_ts"), m.tables()):
            assert _same(g, z["s%d/%s" % (s, k)]), (s, k)


def test_equals_the_oracle_on_random_valid_sequences():
    for seed in range(50):
        rng = np.random.RandomState(1000 + seed)
        N, dm, de = rng.randint(1, 201), rng.randint(1, 71), rng.randint(0, 10)
        ref, ora = RefMemory(N, de, dm), OracleMemory(N, de, dm)
        for step in range(3):
            B, neg = rng.randint(1, 121), rng.randint(0, 4)
            n = (2 + neg) * B
            # heavy duplicates: the ids come from a small part of the table
            nid = rng.randint(0, max(1, min(N, rng.randint(1, 40))), n).astype(np.int64)
            mem = rng.randn(n, dm).astype(np.float32)
            ts = rng.rand(n).astype(np.float32) + step
            ef = None if rng.randint(4) == 0 else rng.randn(B, de).astype(np.float32)
            ref.update_mem_mail(nid, mem, ts, ef, neg)
            ora.update_mem_mail(nid, mem, ts, ef, neg)
            for k, a, b in zip("abcd", ref.tables(),
                               (ora.node_memory, ora.mailbox, ora.node_memory_ts, ora.mailbox_ts)):
                assert _same(a, b), (seed, step, k)
            q = rng.randint(0, N, rng.randint(1, 300)).astype(np.int64)
            for k, a, b in zip("abcd", ref.prepare_input(q), ora.prepare_input(q)):
                assert _same(a, b), (seed, step, k)


def test_out_of_range_ids_by_hand():
    """N=3, dm=1, de=1, B=3, neg=1.  nid = src (0, 7, 1) ++ dst (-1, 0, 3) ++ neg (2, 2, 2);
    memory row j is [10 + j], ts[j] = 100 + j, edge feature i is [50 + i].

    Mailbox, interleaved positions 0..5 = nodes 0, -1, 7, 0, 1, 3: position 0 writes node 0
    ([mem 0, mem 3, ef 0], ts[0]); 1 (-1) and 2 (7) are skipped; 3 writes node 0 again as a
    destination ([mem 4, mem 1, ef 1], ts[3]) — the edge's skipped source does not keep its
    destination from being written; 4 writes node 1 ([mem 2, mem 5, ef 2], ts[4]); 5 (3 == N) is
    skipped.  Memory, positions 0..5 = nodes 0, 7, 1, -1, 0, 3: node 0 last at position 4,
    node 1 at position 2.  The negatives (node 2) are never written."""
    m = RefMemory(3, 1, 1)
    nid = np.array([0, 7, 1, -1, 0, 3, 2, 2, 2], np.int64)
    mem = (10 + np.arange(9, dtype=np.float32)).reshape(9, 1)
    ts = 100 + np.arange(9, dtype=np.float32)
    ef = np.array([[50], [51], [52]], np.float32)
    m.update_mem_mail(nid, mem, ts, ef, 1)
    assert m.mailbox.tolist() == [[14, 11, 51], [12, 15, 52], [0, 0, 0]]
    assert m.mailbox_ts.tolist() == [103, 104, 0]
    assert m.node_memory.tolist() == [[14], [12], [0]]
    assert m.node_memory_ts.tolist() == [104, 102, 0]
    got = m.prepare_input(np.array([1, -1, 3, 0, 2 ** 40, -3, 2], np.int64))
    assert got[0].tolist() == [[12], [0], [0], [14], [0], [0], [0]]
    assert got[1].tolist() == [102, 0, 0, 104, 0, 0, 0]
    assert got[2].tolist() == [104, 0, 0, 103, 0, 0, 0]
    assert got[3].tolist() == [[12, 15, 52], [0, 0, 0], [0, 0, 0], [14, 11, 51], [0, 0, 0],
                               [0, 0, 0], [0, 0, 0]]
    # a batch that is entirely out of range changes nothing; edge_feats=None means zeros
    before = m.backup()
    m.update_mem_mail(np.array([3, -1, 2 ** 40, -2 ** 40], np.int64),
                      np.ones((4, 1), np.float32), np.ones(4, np.float32), None, 0)
    assert all(_same(a, b) for a, b in zip(m.tables(), before))
    m.update_mem_mail(np.array([2, 9], np.int64), np.array([[7], [8]], np.float32),
                      np.array([5, 6], np.float32), None, 0)
    assert m.mailbox.tolist() == [[14, 11, 51], [12, 15, 52], [7, 8, 0]]
    assert m.mailbox_ts.tolist() == [103, 104, 5]
    assert m.node_memory.tolist() == [[14], [12], [7]]


def test_keeps_payload_bits():
    """Signalling and quiet NaNs, -0.0 and denormals go through the restatement's row and scalar
    copies unchanged (the GPU tests compare bits, so the reference must not launder them)."""
    bits = np.array([0x7F800001, 0xFF80ABCD, 0x7FC12345, 0x80000000, 0x00000001, 0x807FFFFF],
                    np.uint32)
    x = bits.view(np.float32)
    m = RefMemory(3, 2, 2)
    m.update_mem_mail(np.array([0, 2], np.int64), x[:4].reshape(2, 2), x[4:6], x[2:4].reshape(1, 2),
                      0)
    assert m.node_memory.view(np.uint32).tolist() == [bits[:2].tolist(), [0, 0], bits[2:4].tolist()]
    assert m.node_memory_ts.view(np.uint32).tolist() == [bits[4], 0, bits[5]]
    assert m.mailbox_ts.view(np.uint32).tolist() == [bits[4], 0, bits[5]]
    assert m.mailbox.view(np.uint32)[2].tolist() == bits[[2, 3, 0, 1, 2, 3]].tolist()
    got = m.prepare_input(np.array([2, 5], np.int64))
    assert got[0].view(np.uint32).tolist() == [bits[2:4].tolist(), [0, 0]]
    assert got[1].view(np.uint32).tolist() == [bits[5], 0]
    assert got[2].view(np.uint32).tolist() == [bits[5], 0]
    assert got[3].view(np.uint32)[0].tolist() == bits[[2, 3, 0, 1, 2, 3]].tolist()


def test_resize_reset_backup_restore():
    m = RefMemory(2, 0, 1)
    m.update_mem_mail(np.array([0, 1], np.int64), np.array([[1], [2]], np.float32),
                      np.array([3, 4], np.float32), None, 0)
    bk = m.backup()
    m.resize(1)                                     # never shrinks
    assert m.num_nodes == 2
    m.resize(4)
    assert m.num_nodes == 4 and m.mailbox.shape == (4, 2) and m.node_memory_ts.shape == (4,)
    assert m.node_memory.tolist() == [[1], [2], [0], [0]]
    assert m.mailbox.tolist() == [[1, 2], [2, 1], [0, 0], [0, 0]]
    m.update_mem_mail(np.array([3, 0], np.int64), np.array([[5], [6]], np.float32),
                      np.array([7, 8], np.float32), None, 0)
    assert m.node_memory.tolist() == [[6], [2], [0], [5]]
    m.reset()
    assert all(not t.any() for t in m.tables())
    m2 = RefMemory(2, 0, 1)
    m2.restore(bk)
    assert m2.node_memory.tolist() == [[1], [2]] and m2.mailbox_ts.tolist() == [3, 4]
    bk[0][...] = 9                                  # the backup is a copy, and so is the restore
    assert m2.node_memory.tolist() == [[1], [2]]
