"""gnnflow_amd.memory.Memory (csrc/memory_ops.hip, and csrc/gather.hip through
gather_rows_multi) against tests/memory_ref.py at the edges the reference fixture does not reach:
row widths on every gather path and around the 64-lane column loops, batches larger than the write
kernel's grid, ids outside [0, num_nodes), orderings that tell the two winner tables apart,
payload bits, the epoch tag across its restart and across resize / reset / restore, inputs as
callers hand them over, a side stream, and a seeded fuzz.

Everything here is data movement: every comparison is on the int32 view of the float arrays, the
four whole tables after every update (so rows that must stay untouched are covered) and a
prepare_input over a query."""
import numpy as np
import pytest

from tests.memory_ref import RefMemory

pytestmark = pytest.mark.gpu

KEYS = ("mem", "mem_ts", "mail_ts", "mem_input")
TABLES = ("node_memory", "mailbox", "node_memory_ts", "mailbox_ts")


class _Blk:
    def __init__(self, ids):
        self.srcdata = {"ID": ids}


def _same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype == np.float32 and got.shape == want.shape and \
        np.array_equal(got.view(np.int32), want.view(np.int32))


def _hip_tables(m):
    return tuple(getattr(m, k).cpu().numpy() for k in TABLES)


def _outside(N):
    return np.array([-1, -N, N, N + 1, 2 ** 40, -2 ** 40], np.int64)


def _ids(rng, N, n, bad=0.0, hi=None):
    """n ids below min(N, hi) (duplicates wherever n is not small against that), a share `bad`
    of them replaced by ids outside [0, N)."""
    ids = rng.randint(0, min(N, hi or N), n).astype(np.int64)
    if bad:
        out = _outside(N)
        pick = rng.rand(n) < bad
        ids[pick] = out[rng.randint(0, len(out), int(pick.sum()))]
    return ids


def _payload(rng, n, dm, B, de, t0=0.0):
    return (rng.randn(n, dm).astype(np.float32), (rng.rand(n) + t0).astype(np.float32),
            rng.randn(B, de).astype(np.float32))


class _Pair:
    """A Memory on the GPU and its sequential restatement, driven together."""

    def __init__(self, N, de, dm, tag=None):
        import torch
        from gnnflow_amd.memory import Memory
        self.torch = torch
        N, de, dm = int(N), int(de), int(dm)
        self.hip = Memory(N, de, dm, device="cuda:0")
        self.ref = RefMemory(N, de, dm)
        self.tag = tag
        self.saved = None

    def check_tables(self, *where):
        for k, got, want in zip(TABLES, _hip_tables(self.hip), self.ref.tables()):
            assert _same(got, want), (self.tag, k) + where

    def update(self, nid, mem, ts, ef, neg, *where):
        t = self.torch
        self.hip.update_mem_mail(t.from_numpy(nid).cuda(), t.from_numpy(mem).cuda(),
                                 t.from_numpy(ts).cuda(),
                                 None if ef is None else t.from_numpy(ef).cuda(),
                                 neg_sample_ratio=neg)
        self.ref.update_mem_mail(nid, mem, ts, ef, neg)
        self.check_tables(*where)

    def query(self, q, *where):
        b = _Blk(self.torch.from_numpy(q).cuda())
        self.hip.prepare_input(b)
        got = [b.srcdata[k].cpu().numpy() for k in KEYS]
        for k, g, w in zip(KEYS, got, self.ref.prepare_input(q)):
            assert _same(g, w), (self.tag, k, len(q)) + where
        return got

    def random_step(self, rng, B, neg, bad=0.0, with_ef=True, hi=None, t0=0.0, *where):
        N, dm, de = self.ref.num_nodes, self.ref.dim_memory, self.ref.dim_edge
        n = (2 + neg) * B
        mem, ts, ef = _payload(rng, n, dm, B, de, t0)
        self.update(_ids(rng, N, n, bad, hi), mem, ts, ef if with_ef else None, neg, *where)

    def resize(self, N):
        self.hip.resize(N)
        self.ref.resize(N)
        assert self.hip.num_nodes == self.ref.num_nodes

    def reset(self):
        self.hip.reset()
        self.ref.reset()

    def backup(self):
        self.saved = (self.hip.backup(), self.ref.backup())

    def restore(self):
        self.hip.restore(self.saved[0])
        self.ref.restore(self.saved[1])


# ---- widths -------------------------------------------------------------------------------------
QUERY_LENGTHS = (1, 15, 16, 17, 63, 64, 65, 257)


@pytest.mark.parametrize("with_ef", [True, False])
@pytest.mark.parametrize("dm,de", [(1, 0), (3, 2), (5, 1), (9, 0), (64, 0), (65, 3), (128, 1)])
def test_width_grid(dm, de, with_ef):
    """Mailbox rows of 2 / 8 / 11 / 18 / 128 / 133 / 257 and memory rows of 1 / 3 / 5 / 9 / 64 /
    65 / 128 floats beside the two 1-float timestamp columns: scalar, float4 and overlapping-vector
    contexts (tails 1, 2, 3) in one gather launch, and column loops of the write kernel of less
    than, exactly, and one more than 64 lanes."""
    N, B = 97, 40
    rng = np.random.RandomState(dm * 16 + de)
    for neg in (0, 1, 3):
        p = _Pair(N, de, dm, (dm, de, with_ef, neg))
        for step in range(3):
            p.random_step(rng, B, neg, 0.0, with_ef, None, float(step), step)
            for qn in QUERY_LENGTHS:
                q = _ids(rng, N, qn)
                q[-1] = q[0]            # a duplicate for certain, across the whole query
                p.query(q, step)


# ---- more positions than the write kernel has waves --------------------------------------------
def test_grid_stride_every_position_writes():
    """2B = 16400 positions on 16384 waves, every id distinct: a second trip that is skipped, or
    that starts at the wrong position, leaves rows at zero or writes another row's payload."""
    B, dm, de = 8200, 4, 1
    rng = np.random.RandomState(1)
    p = _Pair(2 * B, de, dm)
    mem, ts, ef = _payload(rng, 2 * B, dm, B, de)
    p.update(rng.permutation(2 * B).astype(np.int64), mem, ts, ef, 0)
    assert np.all(p.hip.node_memory.cpu().numpy().view(np.int32) != 0)      # every row written
    p.query(rng.randint(0, 2 * B, 3000).astype(np.int64))


def test_grid_stride_with_contention():
    B, dm, de, N = 8200, 4, 1, 5000
    rng = np.random.RandomState(2)
    p = _Pair(N, de, dm)
    for step in range(2):
        p.random_step(rng, B, 1, 0.0, True, None, float(step), step)
    p.query(rng.randint(0, N, 3000).astype(np.int64))


def test_query_above_the_tile_threshold():
    """70 001 ids: past the block size at which the gather goes from 32 to 64 rows per wave;
    rows of 5 (scalar), 11 (overlapping vectors), 1 and 1 floats, the last tile a single row."""
    N, dm, de = 5000, 5, 1
    rng = np.random.RandomState(3)
    p = _Pair(N, de, dm)
    p.random_step(rng, 3000, 1)
    p.query(_ids(rng, N, 70001, 0.1))


# ---- ids outside [0, num_nodes) -----------------------------------------------------------------
def test_out_of_range_ids():
    N, dm, de, B = 97, 9, 2, 60
    rng = np.random.RandomState(4)
    p = _Pair(N, de, dm)
    for step, neg in enumerate((1, 0, 3)):
        p.random_step(rng, B, neg, 0.1, step != 1, None, float(step), step)
        for qn in (1, 17, 64, 300):
            q = _ids(rng, N, qn, 0.1)
            if qn == 1:
                q[0] = 2 ** 40
            got = p.query(q, step)
            unknown = (q < 0) | (q >= N)
            for g in got:       # said once more without the restatement: unknown ids read as zero
                assert not g[unknown].view(np.int32).any()


def test_last_occurrence_just_before_an_invalid_id():
    """Nodes 3 and 4 have their last occurrence right before an id outside the range, in the
    memory order (3 3 8 4 [3 N] 8 [4 -1] 2^40) and in the interleaved order
    (3 N 3 8 8 4 [4 -1] [3 2^40]) alike: the skipped neighbour must not take the write with it."""
    N, dm, de = 20, 3, 2
    rng = np.random.RandomState(5)
    p = _Pair(N, de, dm)
    nid = np.array([3, 3, 8, 4, 3, N, 8, 4, -1, 2 ** 40], np.int64)
    mem, ts, ef = _payload(rng, 10, dm, 5, de)
    p.update(nid, mem, ts, ef, 0)
    assert _same(p.hip.node_memory[3].cpu().numpy(), mem[4])
    assert _same(p.hip.node_memory[4].cpu().numpy(), mem[7])
    assert _same(p.hip.mailbox[3].cpu().numpy(), np.concatenate([mem[4], mem[9], ef[4]]))
    assert _same(p.hip.mailbox[4].cpu().numpy(), np.concatenate([mem[3], mem[8], ef[3]]))
    p.query(np.arange(-2, N + 2, dtype=np.int64))


def test_a_batch_that_is_entirely_invalid_changes_nothing():
    N, dm, de, B = 50, 5, 1, 33
    rng = np.random.RandomState(6)
    p = _Pair(N, de, dm)
    p.random_step(rng, B, 1)
    before = _hip_tables(p.hip)
    out = _outside(N)
    for neg in (0, 1):
        n = (2 + neg) * B
        mem, ts, ef = _payload(rng, n, dm, B, de, 5.0)
        p.update(out[rng.randint(0, len(out), n)], mem, ts, ef, neg)
        assert all(_same(a, b) for a, b in zip(_hip_tables(p.hip), before))
    got = p.query(out[rng.randint(0, len(out), 70)])
    assert not any(g.view(np.int32).any() for g in got)
    p.random_step(rng, B, 1, 0.0, True, None, 9.0)      # and the next valid batch lands


# ---- who is last ----------------------------------------------------------------------------------
def test_self_loops():
    """src[i] == dst[i]: the mailbox keeps the destination's message of the node's last edge
    (interleaved order), the memory the row of the last destination position."""
    N, dm, de, B = 30, 5, 2, 64
    rng = np.random.RandomState(7)
    p = _Pair(N, de, dm)
    for neg in (0, 1):
        n = (2 + neg) * B
        loop = rng.randint(0, N, B).astype(np.int64)
        nid = np.concatenate([loop, loop, rng.randint(0, N, neg * B).astype(np.int64)])
        mem, ts, ef = _payload(rng, n, dm, B, de)
        p.update(nid, mem, ts, ef, neg)
        p.query(np.arange(N, dtype=np.int64))
    last = B - 1 - int(np.argmax(loop[::-1] == loop[0]))    # last edge of the node of edge 0
    v = int(loop[0])
    assert _same(p.hip.mailbox[v].cpu().numpy(),
                 np.concatenate([mem[B + last], mem[last], ef[last]]))
    assert _same(p.hip.node_memory[v].cpu().numpy(), mem[B + last])


def test_every_position_names_one_node():
    N, dm, de, B, v = 11, 7, 3, 300, 6
    rng = np.random.RandomState(8)
    p = _Pair(N, de, dm)
    for step in range(2):
        mem, ts, ef = _payload(rng, 3 * B, dm, B, de, float(step))
        p.update(np.full(3 * B, v, np.int64), mem, ts, ef, 1, step)
    assert _same(p.hip.node_memory[v].cpu().numpy(), mem[2 * B - 1])
    assert _same(p.hip.mailbox_ts[v].cpu().numpy(), ts[2 * B - 1])
    p.query(np.arange(N, dtype=np.int64))


def test_position_decides_not_time():
    N, dm, de, B = 40, 4, 1, 100
    rng = np.random.RandomState(9)
    p = _Pair(N, de, dm)
    for step in range(2):
        mem, _, ef = _payload(rng, 3 * B, dm, B, de)
        ts = (1000.0 * (2 - step) - np.arange(3 * B)).astype(np.float32)    # strictly decreasing
        p.update(_ids(rng, N, 3 * B), mem, ts, ef, 1, step)
    p.query(np.arange(N, dtype=np.int64))


def test_source_early_destination_late_and_the_other_way_round():
    """a = src[0] = dst[B-1], b = dst[0] = src[B-1], every other id distinct.  The mailbox
    (interleaved) keeps a's message as a destination and b's as a source, both of the last edge;
    the memory (src.. ++ dst..) keeps a's row of position 2B-1 and b's row of position B — b's
    two tables take their rows from different edges."""
    N, dm, de, B, a, b = 64, 6, 2, 9, 40, 41
    rng = np.random.RandomState(10)
    p = _Pair(N, de, dm)
    other = rng.permutation(40)[:2 * B - 4].astype(np.int64)
    src = np.concatenate([[a], other[:B - 2], [b]])
    dst = np.concatenate([[b], other[B - 2:], [a]])
    mem, ts, ef = _payload(rng, 2 * B, dm, B, de)
    p.update(np.concatenate([src, dst]).astype(np.int64), mem, ts, ef, 0)
    row = lambda t, v: getattr(p.hip, t)[v].cpu().numpy()
    assert _same(row("mailbox", a), np.concatenate([mem[2 * B - 1], mem[B - 1], ef[B - 1]]))
    assert _same(row("mailbox", b), np.concatenate([mem[B - 1], mem[2 * B - 1], ef[B - 1]]))
    assert _same(row("mailbox_ts", a), ts[2 * B - 1]) and _same(row("mailbox_ts", b), ts[2 * B - 2])
    assert _same(row("node_memory", a), mem[2 * B - 1]) and _same(row("node_memory", b), mem[B])
    assert _same(row("node_memory_ts", b), ts[B])
    p.query(np.arange(N, dtype=np.int64))


# ---- bits ---------------------------------------------------------------------------------------
SPECIAL_BITS = np.array([0x7FC00000, 0x7FC00001, 0x7FC12345, 0xFFC00000, 0xFFFFFFFF, 0x7F800001,
                         0xFF80ABCD, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x80000001,
                         0x007FFFFF, 0x807FFFFF, 0x00400000], np.uint32).view(np.float32)


def test_payload_bits():
    """NaNs with distinct payloads (quiet and signalling), +-inf, -0.0 and denormals go through
    the update and come back out of the tables and of prepare_input bit for bit."""
    N, dm, de, B = 50, 9, 5, 45
    rng = np.random.RandomState(11)
    p = _Pair(N, de, dm)

    def special(shape):
        x = rng.randn(*shape).astype(np.float32)
        pick = rng.rand(*shape) < 0.6
        x[pick] = SPECIAL_BITS[rng.randint(0, len(SPECIAL_BITS), int(pick.sum()))]
        return x

    for step in range(2):
        mem, ts, ef = special((3 * B, dm)), special((3 * B,)), special((B, de))
        kept = [a.view(np.int32).copy() for a in (mem, ts, ef)]
        p.update(_ids(rng, N, 3 * B), mem, ts, ef, 1, step)
        assert all(np.array_equal(a.view(np.int32), k) for a, k in zip((mem, ts, ef), kept))
        p.query(np.arange(N, dtype=np.int64), step)
    seen = set(p.hip.mailbox.cpu().numpy().view(np.uint32).reshape(-1).tolist())
    assert seen >= set(SPECIAL_BITS.view(np.uint32).tolist())       # the test did carry them all


# ---- the epoch tag --------------------------------------------------------------------------------
def test_epoch_crosses_its_restart():
    N, dm, de, B = 80, 5, 2, 50
    rng = np.random.RandomState(12)
    p = _Pair(N, de, dm)
    p.random_step(rng, B, 1)
    assert p.hip._epoch == 1
    p.hip._epoch = 2 ** 31 - 3
    epochs = []
    for step in range(4):
        p.random_step(rng, B, 1, 0.0, True, None, float(step), step)
        epochs.append(p.hip._epoch)
        p.query(np.arange(N, dtype=np.int64), step)
    assert epochs == [2 ** 31 - 2, 2 ** 31 - 1, 1, 2]


def test_restart_clears_stale_tags():
    """v is tagged (epoch 1, position 2B-1) by the first update.  The first update after the
    restart runs at epoch 1 again and has v at position 0 only: a tag that survived the restart
    would outrank it, and v's rows would stay as they were."""
    N, dm, de, B, v = 200, 5, 2, 50, 199
    rng = np.random.RandomState(13)
    p = _Pair(N, de, dm)
    nid = np.concatenate([rng.permutation(150)[:2 * B - 1], [v]]).astype(np.int64)
    mem, ts, ef = _payload(rng, 2 * B, dm, B, de)
    p.update(nid, mem, ts, ef, 0)
    p.hip._epoch = 2 ** 31 - 1
    nid = np.concatenate([[v], rng.permutation(150)[:2 * B - 1]]).astype(np.int64)
    mem, ts, ef = _payload(rng, 2 * B, dm, B, de, 1.0)
    p.update(nid, mem, ts, ef, 0)
    assert p.hip._epoch == 1
    assert _same(p.hip.node_memory[v].cpu().numpy(), mem[0])
    assert _same(p.hip.mailbox_ts[v].cpu().numpy(), ts[0])


def test_resize_between_updates():
    N, dm, de, B = 60, 5, 2, 40
    rng = np.random.RandomState(14)
    p = _Pair(N, de, dm)
    for step in range(4):
        p.random_step(rng, B, 1, 0.05, True, None, float(step), step)
        p.query(_ids(rng, p.ref.num_nodes + 50, 100), step)     # also ids of rows still to come
        p.resize(p.ref.num_nodes + 50)
        p.check_tables("resized", step)
        # old and new nodes in one batch, the new ones tagged for the first time
        n = 3 * B
        nid = np.concatenate([_ids(rng, N, n // 2), rng.randint(p.ref.num_nodes - 50,
                                                                p.ref.num_nodes, n - n // 2)])
        mem, ts, ef = _payload(rng, n, dm, B, de, step + 0.5)
        p.update(rng.permutation(nid).astype(np.int64), mem, ts, ef, 1, "after resize", step)
    p.hip.resize(10)        # never shrinks
    assert p.hip.num_nodes == N + 200
    p.query(np.arange(-1, N + 201, dtype=np.int64))


def test_reset_backup_restore_between_updates():
    N, dm, de, B = 60, 5, 2, 40
    rng = np.random.RandomState(15)
    p = _Pair(N, de, dm)
    p.random_step(rng, B, 1)
    p.backup()
    p.random_step(rng, B, 1, 0.0, True, 10, 1.0)
    p.reset()
    p.check_tables("reset")
    assert not any(t.view(np.int32).any() for t in _hip_tables(p.hip))
    p.random_step(rng, B, 0, 0.0, True, 10, 2.0)     # tags of before the reset are stale, rows zero
    p.query(np.arange(N, dtype=np.int64))
    p.restore()
    p.check_tables("restored")
    p.random_step(rng, B, 3, 0.0, False, None, 3.0)
    p.restore()
    p.check_tables("restored twice")
    p.random_step(rng, B, 1, 0.0, True, None, 4.0)
    p.query(np.arange(N, dtype=np.int64))


def test_two_memories_in_turn():
    rng = np.random.RandomState(16)
    a, b = _Pair(70, 2, 5, "a"), _Pair(45, 0, 12, "b")
    for step in range(4):
        a.random_step(rng, 40, 1, 0.0, True, None, float(step), step)
        b.random_step(rng, 25, 0, 0.0, step % 2 == 0, None, float(step), step)
        a.check_tables("after b", step)
        b.query(np.arange(45, dtype=np.int64), step)
        a.query(np.arange(70, dtype=np.int64), step)
    assert a.hip._epoch == b.hip._epoch == 4


# ---- inputs as callers hand them over ----------------------------------------------------------
@pytest.mark.parametrize("dm,de", [(6, 3), (5, 0)])
def test_inputs_as_they_come(dm, de):
    """CPU tensors, int32 ids, float64 memory / ts (values float32 holds exactly), memory a
    column slice of a wider tensor, ts every other element of a longer one, edge_feats [B, 0]
    for dim_edge 0; nothing handed over is written to."""
    import torch
    N, B, neg = 40, 30, 1
    n = (2 + neg) * B
    rng = np.random.RandomState(17 + de)
    p = _Pair(N, de, dm)
    for step in range(2):
        nid = torch.from_numpy(_ids(rng, N, n, 0.1).clip(-2 ** 31, 2 ** 31 - 1).astype(np.int32))
        wide = torch.from_numpy(rng.randint(-4096, 4096, (n, dm + 5)) / 16.0)
        long_ts = torch.from_numpy(rng.randint(0, 1 << 20, 2 * n) / 4.0)
        ef = torch.from_numpy(rng.randint(-4096, 4096, (B, de)) / 16.0)
        mem, ts = wide[:, 2:2 + dm], long_ts[1::2]
        assert wide.dtype == long_ts.dtype == ef.dtype == torch.float64
        assert not mem.is_contiguous() and not ts.is_contiguous() and tuple(ef.shape) == (B, de)
        raw = lambda t: t.numpy().reshape(-1).view(np.uint8)
        kept = [raw(t).copy() for t in (nid, wide, long_ts, ef)]
        p.hip.update_mem_mail(nid, mem, ts, ef, neg_sample_ratio=neg)
        p.ref.update_mem_mail(nid.numpy().astype(np.int64), mem.numpy().astype(np.float32),
                              ts.numpy().astype(np.float32), ef.numpy().astype(np.float32), neg)
        p.check_tables(step)
        for t, k in zip((nid, wide, long_ts, ef), kept):
            assert np.array_equal(raw(t), k)
        # the query: int32 ids on the CPU, every third element of a longer tensor
        long_q = torch.from_numpy(_ids(rng, N, 150, 0.1).clip(-2 ** 31, 2 ** 31 - 1)
                                  .astype(np.int32))
        q, kept_q = long_q[::3], long_q.clone()
        blk = _Blk(q)
        p.hip.prepare_input(blk)
        for k, w in zip(KEYS, p.ref.prepare_input(q.numpy().astype(np.int64))):
            assert _same(blk.srcdata[k].cpu().numpy(), w), (k, step)
        assert blk.srcdata["ID"] is q and torch.equal(long_q, kept_q)


def test_side_stream():
    import torch
    N, dm, de, B = 90, 9, 3, 70
    rng = np.random.RandomState(19)
    p = _Pair(N, de, dm)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())      # the tables were zeroed on the current stream
    outs, host = [], []
    with torch.cuda.stream(s):
        for step in range(3):
            nid = _ids(rng, N, 3 * B, 0.1)
            mem, ts, ef = _payload(rng, 3 * B, dm, B, de, float(step))
            q = _ids(rng, N, 200, 0.1)
            host.append((nid, mem, ts, ef, q))
            up = lambda a: torch.from_numpy(a).pin_memory().to("cuda:0", non_blocking=True)
            # inputs produced on s: uploaded there, and passed through a kernel of s
            p.hip.update_mem_mail(up(nid) + 0, up(mem) * 1.0, up(ts) * 1.0, up(ef) * 1.0)
            b = _Blk(up(q) + 0)
            p.hip.prepare_input(b)
            outs.append(b)
    s.synchronize()
    for step, (b, (nid, mem, ts, ef, q)) in enumerate(zip(outs, host)):
        p.ref.update_mem_mail(nid, mem, ts, ef, 1)
        for k, w in zip(KEYS, p.ref.prepare_input(q)):
            assert _same(b.srcdata[k].cpu().numpy(), w), (k, step)
    p.check_tables()


def test_validation_reaches_the_launch_path():
    """edge_feats with one row too many (harmless if it went through): refused with the shape in
    the message, before the epoch moves or a table changes."""
    import torch
    N, dm, de, B = 30, 4, 3, 10
    rng = np.random.RandomState(20)
    p = _Pair(N, de, dm)
    p.random_step(rng, B, 1)
    before, epoch = _hip_tables(p.hip), p.hip._epoch
    mem, ts, _ = _payload(rng, 3 * B, dm, B, de)
    with pytest.raises(ValueError, match=r"edge_feats must be \[10, 3\] or None, got shape \(11, 3\)"):
        p.hip.update_mem_mail(torch.from_numpy(_ids(rng, N, 3 * B)).cuda(),
                              torch.from_numpy(mem).cuda(), torch.from_numpy(ts).cuda(),
                              torch.zeros(B + 1, de, device="cuda:0"))
    torch.cuda.synchronize()
    assert p.hip._epoch == epoch
    assert all(_same(a, b) for a, b in zip(_hip_tables(p.hip), before))
    p.check_tables()


# ---- fuzz -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(24))
def test_seeded_fuzz(seed):
    rng = np.random.RandomState(5000 + seed)
    N, dm, de = rng.randint(1, 301), rng.randint(1, 71), rng.randint(0, 10)
    p = _Pair(N, de, dm, (seed, N, dm, de))
    for step in range(4):
        B, neg = rng.randint(1, 201), rng.randint(0, 4)
        hi = None if rng.randint(2) else rng.randint(1, 40)     # half the steps: heavy duplicates
        p.random_step(rng, B, neg, 0.1, rng.randint(4) != 0, hi, float(step), step)
        p.query(_ids(rng, p.ref.num_nodes, rng.randint(1, 400), 0.1), step)
        if rng.randint(4) == 0:
            if rng.randint(2):
                p.resize(p.ref.num_nodes + rng.randint(1, 60))
            elif p.saved is None or p.saved[1][0].shape[0] != p.ref.num_nodes or rng.randint(2):
                p.backup()
            else:
                p.restore()
            p.check_tables("between", step)
