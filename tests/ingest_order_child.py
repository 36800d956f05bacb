"""Child process of tests/test_gpu_ingest_order.py: the order add_edges leaves a node's run in,
(source, timestamp under float `<`, input position), on whichever of its three orderings a batch
takes — the device radix sort, the host counting sort + per-group stable sort, the host std::sort
for sparse ids.  The threshold between device and host is read once per process
(GNNFLOW_INGEST_DEVICE_SORT_MIN), hence a fresh process per arrangement; GNNFLOW_INGEST_PROFILE=1
makes every accepted add_edges print its phase line on stderr ("dsort" = device path), and the
`@@ tag` lines written here tell the parent which call a phase line belongs to.

Every scenario builds the same store in gnnflow_amd.DynamicGraph and oracle.OracleGraph and
compares accessors, every source's neighbour list and samples bit for bit.

  python tests/ingest_order_child.py [scenario ...]      (default: all of a b c d e f t)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
assert os.environ.get("GNNFLOW_INGEST_DEVICE_SORT_MIN") is not None
assert os.environ.get("GNNFLOW_INGEST_PROFILE") is not None

import gnnflow_amd  # noqa: E402
from oracle import oracle as O  # noqa: E402

T = 4096                                   # the low threshold of the "4096" arrangement
F32 = np.finfo(np.float32)
FMAX, DEN = np.float32(F32.max), np.float32(F32.smallest_subnormal)
PZ, NZ = np.float32(0.0), np.float32(-0.0)
SPECIAL = np.array([PZ, NZ, DEN, -DEN, FMAX, -FMAX], np.float32)


def mark(tag):
    print("@@ " + tag, file=sys.stderr, flush=True)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Pair:
    """The same store twice: HIP and oracle."""

    def __init__(self, min_block=8, policy="insert", adaptive=True):
        self.g = gnnflow_amd.DynamicGraph(1 << 20, 1 << 30, "cuda", min_block, 128, policy,
                                          adaptive_block_size=adaptive)
        self.o = O.OracleGraph(minimum_block_size=min_block, insertion_policy=policy,
                               adaptive_block_size=adaptive)

    def add(self, tag, src, dst, ts, eid, add_reverse=False):
        mark(tag)
        self.g.add_edges(src, dst, ts, eid, add_reverse=add_reverse)
        self.o.add_edges(src, dst, ts, eid, add_reverse=add_reverse)

    def same(self, tag):
        g, o = self.g, self.o
        assert g.num_edges() == o.num_edges(), tag
        assert g.num_vertices() == o.num_vertices(), tag
        assert g.num_source_vertices() == o.num_source_vertices(), tag
        assert g.max_vertex_id() == o.max_vertex_id(), tag
        assert np.array_equal(g.nodes(), o.nodes()), tag
        assert np.array_equal(g.src_nodes(), o.src_nodes()), tag
        assert np.array_equal(np.sort(g.edges()), np.sort(o.edges())), tag
        ids = np.arange(0, o.max_vertex_id() + 1)
        assert np.array_equal(g.out_degree(ids), o.out_degree(ids)), tag
        assert abs(g.avg_linked_list_length() - o.avg_linked_list_length()) < 1e-4, tag
        assert g.get_graph_memory_usage() == o.get_graph_memory_usage(), tag
        for v in o.src_nodes():
            gd, gt, ge = g.get_temporal_neighbors(int(v))
            od, ot, oe = o.get_temporal_neighbors(int(v))
            assert np.array_equal(gd, od), (tag, "dst", int(v))
            assert np.array_equal(u32(gt), u32(ot)), (tag, "ts bits", int(v))
            assert np.array_equal(ge, oe), (tag, "eid", int(v))

    def same_samples(self, tag, nodes, ts, **cfg):
        """recent [7, 3] and one uniform sample, every array bit for bit; returns the oracle's
        recent blocks."""
        nodes = np.ascontiguousarray(nodes, np.int64)
        ts = np.ascontiguousarray(ts, np.float32)
        recent = None
        for strategy, extra in (("recent", {}), ("uniform", {"seed": 8})):
            hs = gnnflow_amd.TemporalSampler(self.g, [7, 3], strategy, **cfg, **extra)
            os_ = O.OracleSampler(self.o, [7, 3], strategy, **cfg, **extra)
            want = os_.sample(nodes, ts)
            same_blocks(hs.sample(nodes, ts), want, "{} {} {}".format(tag, strategy, cfg))
            recent = recent or want
        return recent


def same_blocks(hip, ora, tag):
    assert len(hip) == len(ora), tag
    for li, (hl, ol) in enumerate(zip(hip, ora)):
        assert len(hl) == len(ol), tag
        for si, (hb, ob) in enumerate(zip(hl, ol)):
            w = "{} block[{}][{}]".format(tag, li, si)
            assert hb.num_src_nodes() == ob.num_src_nodes(), w
            assert hb.num_dst_nodes() == ob.num_dst_nodes(), w
            assert np.array_equal(hb.srcdata["ID"].cpu().numpy(), ob.srcdata["ID"]), w + " nodes"
            assert np.array_equal(u32(hb.srcdata["ts"].cpu().numpy()), u32(ob.srcdata["ts"])), \
                w + " ts bits"
            assert np.array_equal(u32(hb.edata["dt"].cpu().numpy()), u32(ob.edata["dt"])), \
                w + " dt bits"
            assert np.array_equal(hb.edata["ID"].cpu().numpy(), ob.edata["ID"]), w + " eids"
            assert np.array_equal(hb.edges()[0].cpu().numpy(), ob.edges()[0]), w + " col"
            assert np.array_equal(hb.edges()[1].cpu().numpy(), ob.edges()[1]), w + " row"


def roots_around_newest(o, sources):
    """Three roots per source: just before, at and just after its newest edge."""
    nodes, ts = [], []
    for v in sources:
        t = o.get_temporal_neighbors(int(v))[1]
        tn = t[0] if len(t) else np.float32(100.0)           # (every edge offloaded)
        after = tn if tn == FMAX else np.nextafter(tn, np.float32(np.inf), dtype=np.float32)
        before = tn if tn == -FMAX else np.nextafter(tn, np.float32(-np.inf), dtype=np.float32)
        nodes += [int(v)] * 3
        ts += [before, tn, after]
    return np.array(nodes, np.int64), np.array(ts, np.float32)


def some(ids, k, rng):
    ids = np.asarray(ids)
    return ids if len(ids) <= k else rng.choice(ids, size=k, replace=False)


def permuted(rng, *arrays):
    p = rng.permutation(len(arrays[0]))
    return [np.ascontiguousarray(a[p]) for a in arrays]


# ---- (a) unsorted batch, heavy ties, signed zeros, denormals, +-FLT_MAX -----------------------
def scenario_a():
    rng = np.random.RandomState(101)
    N, E = 300, 12000
    src = rng.randint(0, N, E)
    ts = (rng.randint(-25, 25, E) * 20.0).astype(np.float32)          # 50 levels in [-500, 500)
    # zero sources: only negative times besides several zeros of either sign, so that the zeros
    # are their newest edges; two of them also carry the negative denormal and -FLT_MAX
    zsrc = np.arange(N, N + 8)
    for i, v in enumerate(zsrc):
        zs = np.array([PZ, NZ] * 3, np.float32)
        neg = (-20.0 * rng.randint(1, 6, 6)).astype(np.float32)
        if i < 2:
            neg = np.concatenate([neg, [-DEN, -FMAX, -DEN]]).astype(np.float32)
        src = np.concatenate([src, np.full(len(zs) + len(neg), v)])
        ts = np.concatenate([ts, zs, neg])
    # mixed sources: every special value twice among ordinary times
    msrc = np.arange(N + 8, N + 12)
    for v in msrc:
        vals = np.concatenate([SPECIAL, SPECIAL, (rng.randint(-5, 5, 8) * 20.0)]).astype(np.float32)
        src = np.concatenate([src, np.full(len(vals), v)])
        ts = np.concatenate([ts, vals])
    # a fresh block of the reference starts with end_timestamp = 0 and refuses a batch whose
    # newest edge is older (utils.cu:42-43): one closing edge at t >= 0 for the ordinary sources
    src = np.concatenate([src, np.arange(N)])
    ts = np.concatenate([ts, np.full(N, 480.0, np.float32)])
    n = len(src)
    dst = rng.randint(0, N + 12, n)
    src, dst, ts = permuted(rng, src, dst, ts.astype(np.float32))
    eid = np.arange(n, dtype=np.int64)
    assert T < n <= 40000

    p = Pair(min_block=8)
    p.add("a", src, dst, ts, eid)
    p.same("a")

    # not vacuous, from the inputs and the oracle alone: both input orders of the two zeros
    # occur, the oracle keeps input order among them, and at a root just after 0 the newest
    # candidate is a zero whose eid differs under the bit order (-0.0 before +0.0)
    orders, divergent = set(), []
    for v in np.concatenate([zsrc, msrc]):
        at = np.flatnonzero((src == v) & (ts == 0))               # input order, both signs
        sign = np.signbit(ts[at])
        assert sign.any() and not sign.all()
        for a, b in zip(sign[:-1], sign[1:]):
            if a != b:
                orders.add("+-" if b else "-+")
        od, ot, oe = p.o.get_temporal_neighbors(int(v))
        zero = ot == 0
        assert oe[zero].tolist() == eid[at][::-1].tolist()        # newest first = input reversed
        assert np.array_equal(u32(ot[zero]), u32(ts[at][::-1]))   # each keeps its own sign
        newest_by_bits = eid[at][~sign][-1]                       # the last +0.0 of the input
        if eid[at][-1] != newest_by_bits:
            divergent.append((int(v), int(eid[at][-1]), int(newest_by_bits)))
    assert orders == {"+-", "-+"}, orders
    assert len(divergent) >= 2, divergent

    srcs = np.unique(src)
    nodes, rts = roots_around_newest(p.o, srcs)
    sp_nodes = np.repeat(np.concatenate([zsrc, msrc]), len(SPECIAL) + 1)
    sp_ts = np.tile(np.concatenate([SPECIAL, [np.float32(1.0)]]), len(zsrc) + len(msrc))
    first_special = len(nodes)
    nodes = np.concatenate([nodes, sp_nodes])
    rts = np.concatenate([rts, sp_ts]).astype(np.float32)
    recent = p.same_samples("a", nodes, rts)
    # the expected sample itself shows the tie: the root (v, smallest denormal) of a divergent
    # source takes the zero that came LAST in the input first
    block, den_at = recent[-1][0], list(SPECIAL).index(DEN)
    rows, eids = block.edges()[1], block.edata["ID"]
    order = np.concatenate([zsrc, msrc]).tolist()
    for v, want, other in divergent:
        r = first_special + order.index(v) * (len(SPECIAL) + 1) + den_at
        assert nodes[r] == v and u32(rts[r]) == u32(DEN)
        got = eids[np.flatnonzero(rows == r)[0]]
        assert got == want and got != other, (v, got, want, other)
    # with a window the negative half is reachable too (a window of 0 starts at t = 0)
    p.same_samples("a window", nodes, rts, snapshot_time_window=2000.0)


# ---- (b) unix-second times: float32 spacing 128, most edges tie ---------------------------------
def scenario_b():
    rng = np.random.RandomState(202)
    N, DAY, base = 400, 86400, 1.6e9
    p = Pair(min_block=16)
    lo = 0
    for k, (n, t0, t1) in enumerate(((12000, 0, 2 * DAY + 1), (8000, 2 * DAY, 3 * DAY))):
        src = rng.zipf(1.5, n) % N
        dst = rng.randint(0, N, n)
        ts = (base + rng.randint(t0, t1, n)).astype(np.float32)
        assert len(np.unique(ts)) < n // 4                        # most edges tie
        p.add("b%d" % k, src, dst, ts, np.arange(lo, lo + n))     # (randint: already unsorted)
        lo += n
        p.same("b%d" % k)
    srcs = some(p.o.src_nodes(), 300, rng)
    nodes, rts = roots_around_newest(p.o, srcs)
    more = rng.randint(0, N, 400)
    nodes = np.concatenate([nodes, more])
    rts = np.concatenate([rts, (base + rng.randint(0, 4 * DAY, 400)).astype(np.float32)])
    p.same_samples("b", nodes, rts, num_snapshots=3, snapshot_time_window=float(DAY))


# ---- (c) widely spread ids: a hub, one-edge sources, a far id, empty groups ---------------------
def scenario_c():
    rng = np.random.RandomState(303)
    hub, first, singles = 5, 100, 12000
    far = first + singles + 70000
    src = np.concatenate([np.full(9000, hub), np.arange(first, first + singles), [far] * 3])
    n = len(src)
    dst = rng.randint(0, first + singles, n)
    ts = (rng.randint(0, 200, n) * 5.0).astype(np.float32)
    src, dst, ts = permuted(rng, src, dst, ts)
    p = Pair(min_block=4)
    p.add("c", src, dst, ts, np.arange(n))
    p.same("c")
    # 1 000 edges whose far id is 300 000: on the host this is the std::sort branch
    # (table_len > 4 n + 65536)
    m = 1000
    src2 = np.concatenate([np.full(100, hub), rng.randint(first, first + 1000, m - 110),
                           [300000] * 10])
    dst2 = rng.randint(0, first + singles, m)
    ts2 = (1000.0 + rng.randint(0, 20, m)).astype(np.float32)
    src2, dst2, ts2 = permuted(rng, src2, dst2, ts2)
    assert 300001 > 4 * m + 65536
    p.add("c sparse", src2, dst2, ts2, np.arange(n, n + m))
    p.same("c sparse")
    srcs = np.concatenate([[hub, far, 300000], some(np.arange(first, first + singles), 500, rng)])
    nodes, rts = roots_around_newest(p.o, srcs)
    p.same_samples("c", nodes, rts)


# ---- (d) a second ordered batch on existing segments, an offload, a third batch -----------------
def scenario_d():
    for policy in ("insert", "replace"):
        rng = np.random.RandomState(404)
        N, n = 800, 9000
        p = Pair(min_block=4, policy=policy)
        for k in range(3):
            src = rng.zipf(1.3, n) % N
            dst = rng.randint(0, N, n)
            ts = (300.0 * k + rng.randint(0, 61, n) * 5.0).astype(np.float32)   # ends meet
            p.add("d %s %d" % (policy, k), src, dst, ts, np.arange(k * n, (k + 1) * n))
            p.same("d %s %d" % (policy, k))
            if k == 1:
                assert p.g.offload_old_blocks(150.0) == p.o.offload_old_blocks(150.0)
                p.same("d %s offload" % policy)
        nodes, rts = roots_around_newest(p.o, some(p.o.src_nodes(), 400, rng))
        p.same_samples("d " + policy, nodes, rts)


# ---- (e) a rejected batch, (f) NaN timestamps ---------------------------------------------------
def expect_value_error(p, tag, contains, *batch, **kw):
    mark(tag + " (rejected)")
    try:
        p.g.add_edges(*batch, **kw)
    except ValueError as e:
        assert contains in str(e), (tag, str(e))
    else:
        raise AssertionError(tag + ": the batch was accepted")
    p.same(tag)


def scenario_e_f(which):
    rng = np.random.RandomState(505)
    N, n = 500, 6000
    p = Pair(min_block=8)
    src = rng.zipf(1.3, n) % N
    p.add(which + "0", src, rng.randint(0, N, n),
          (100.0 + rng.randint(0, 101, n)).astype(np.float32), np.arange(n))
    p.same(which + "0")
    nodes, rts = roots_around_newest(p.o, some(p.o.src_nodes(), 200, rng))
    p.same_samples(which + "0", nodes, rts)
    # the next batch: old and new vertices (ids up to 899), all at or after the newest stored time
    src1 = rng.randint(0, 900, n)
    dst1 = rng.randint(0, 900, n)
    ts1 = (200.0 + rng.randint(0, 50, n)).astype(np.float32)
    eid1 = np.arange(n, 2 * n)
    if "e" in which:
        victim = int(np.bincount(src).argmax())
        assert p.o.get_temporal_neighbors(victim)[1][0] > 150.0 and (src1 == victim).sum() > 1
        bad = ts1.copy()
        bad[np.flatnonzero(src1 == victim)[-1]] = 150.0       # its group's oldest edge: too old
        expect_value_error(p, "e", "older than its newest stored edge", src1, dst1, bad, eid1)
        expect_value_error(p, "e small", "older than its newest stored edge",
                           np.array([901, victim, 3]), np.array([1, 2, 3]),
                           np.array([500.0, 150.0, 500.0], np.float32), np.array([1, 2, 3]) + 2 * n)
        p.same_samples("e", nodes, rts)
    if "f" in which:
        nan = np.float32(np.nan)
        for name, bits in (("", None), (" negative", 0xFFC00000), (" signalling", 0x7F800001)):
            bad = ts1.copy()
            bad[[T + 1, 5000]] = nan if bits is None else np.array([bits], np.uint32).view(np.float32)
            expect_value_error(p, "f" + name, "position %d" % (T + 1), src1, dst1, bad, eid1)
        bad = ts1[:n // 2].copy()
        bad[77] = nan
        expect_value_error(p, "f reverse", "position 77", src1[:n // 2], dst1[:n // 2], bad,
                           eid1[:n // 2], add_reverse=True)
        expect_value_error(p, "f small", "position 2", np.array([1, 2, 3]), np.array([4, 5, 6]),
                           np.array([300.0, 300.0, nan], np.float32), np.array([1, 2, 3]) + 2 * n)
        expect_value_error(p, "f sparse", "position 0", np.array([300000, 2, 3]),
                           np.array([4, 5, 6]), np.array([nan, 300.0, nan], np.float32),
                           np.array([1, 2, 3]) + 2 * n)
        p.same_samples("f", nodes, rts)
    # a valid batch then succeeds
    p.add(which + " after", src1, dst1, ts1, eid1)
    p.same(which + " after")
    nodes, rts = roots_around_newest(p.o, some(p.o.src_nodes(), 200, rng))
    p.same_samples(which + " after", nodes, rts)


# ---- (t) batches just below, at and above the low threshold -------------------------------------
def scenario_t():
    rng = np.random.RandomState(606)
    N = 300
    p = Pair(min_block=8)
    lo = 0
    for k, (tag, n, rev) in enumerate((("T-1", T - 1, False), ("T", T, False), ("T+1", T + 1, False),
                                       ("T/2 reverse", T // 2, True))):
        src = rng.zipf(1.4, n) % N
        dst = rng.randint(0, N, n)
        ts = (100.0 * k + rng.randint(0, 21, n) * 5.0).astype(np.float32)
        p.add("t " + tag, src, dst, ts, np.arange(lo, lo + n), add_reverse=rev)
        lo += n
        p.same("t " + tag)
    nodes, rts = roots_around_newest(p.o, p.o.src_nodes())
    p.same_samples("t", nodes, rts)


SCENARIOS = {"a": scenario_a, "b": scenario_b, "c": scenario_c, "d": scenario_d,
             "e": lambda: scenario_e_f("e"), "f": lambda: scenario_e_f("f"), "t": scenario_t}


def main():
    failed = []
    for name in sys.argv[1:] or sorted(SCENARIOS):
        mark("scenario " + name)
        try:
            SCENARIOS[name]()
            print("ok", name, flush=True)
        except AssertionError as e:        # a wrong answer: report it and go on with the rest
            failed.append(name)
            print("FAILED {}: {!r}".format(name, e), flush=True)
    mark("end")
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
