"""Fuzz of the four edge-history readers (DynamicGraph.pair_history, DynamicGraph.seen_mask,
DeviceBatchStream's historical negatives, DynamicGraph.temporal_random_walk) on the stores the
sampler is tested on: power-law graphs, negative and signed-zero times, both block policies,
small chunks, reverse edges, an offload in the middle of the stream, unsorted chunks, a source id
far past the dense range, a hub of more than 8192 edges.  Everything is exact: ids, counts and
mask words equal, last_ts and walk times bit for bit.

  python scripts/fuzz_history.py [--seeds 200]

`draw(seed)` is pure numpy (tests/test_history_fuzz_inputs.py imports it without a GPU);
`run(seed)` builds the store and calls `check_readers`, which holds the two checks:

A  every reader against its numpy restatement (tests/*_ref.py) over histories read with
   graph.get_temporal_neighbors, called through the helpers of the readers' own GPU tests.

B  every reader against TemporalSampler(graph, [k], "recent"), which answers the same question
   (the newest k edges before t) without get_temporal_neighbors.  The sampler's upper end is
   strict, ts < t, as the readers': oracle/gnnflow_oracle.c block_range takes
   lower_bound_ts(end), the first timestamp >= end, as the exclusive end of a block's candidates,
   and csrc/sampler_ctx.hpp window_bounds takes hi = lower_bound_fenced(end) (or hi = size for
   end > the newest edge).  So check B runs on rows that tie with an edge too.  The LOWER end is
   where sampler and readers differ by definition: without a window the sampler's window is
   [0, t), as the reference's (time_window: start = 0), which on a store without negative times
   is every edge before t, and with negative times is not.  On a store with negative times check
   B therefore samples with snapshot_time_window = 4e6, a window [t - 4e6, t) that holds every
   edge before t for every finite t of the queries, and leaves out the rows at t = +inf, whose
   window [inf, inf) is empty while the readers consider every edge.  Nothing else is left out.
   k = max_history, or 70 without a bound, then on the rows whose node has at most 70 live edges
   (graph.out_degree).
"""
import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import hist_negatives_ref as H      # noqa: E402
from tests import pair_history_ref as P        # noqa: E402
from tests import seen_mask_ref as S           # noqa: E402
from tests import synth                        # noqa: E402
from tests import temporal_walk_ref as T       # noqa: E402

T_MAX = 1000.0
LATE = 1e6                # later than everything
FAR = 70000               # a far source id is N + FAR
HUB_EDGES = 8192          # a hub's extra edges, at least
UNBOUNDED_K = 70          # check B's fanout where max_history is 0
WINDOW = 4e6              # check B's sampler window on a store with negative times
FEATURES = ("negative", "replace", "offload", "shuffle", "far", "hub")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the draw -----------------------------------------------------------------------------
def draw(seed):
    """Everything run(seed) uses, from np.random.RandomState(seed) alone: the edge stream as
    add_edges will be given it (src, dst, ts, eid; chunk boundaries every `chunk` edges), how
    the store is configured, the query rows and the readers' arguments."""
    rng = np.random.RandomState(seed)
    d = types.SimpleNamespace(seed=seed)
    d.N = N = int(rng.choice([5, 50, 700, 4000]))
    E = int(rng.choice([40, 900, 20000]))
    d.alpha = float(rng.choice([0.0, 1.0, 1.6]))
    d.ties = int(rng.choice([3, 60, 5000]))
    d.min_block = int(rng.choice([1, 4, 62]))
    d.policy = str(rng.choice(["insert", "replace"]))
    d.adaptive = bool(rng.randint(2))
    d.chunk = int(rng.choice([7, 333, 6000]))
    d.reverse = bool(rng.randint(2))
    d.offload = bool(rng.randint(2))
    d.negative = bool(rng.randint(2))
    d.shuffle = rng.randint(4) == 0
    d.far = rng.randint(4) == 0
    hub = rng.randint(4) == 0
    if hub:
        E = min(E, 20000 - HUB_EDGES - 300)      # the largest store stays at 20 000 edges
    src, dst, ts, _ = synth.powerlaw_graph(N, E, seed=seed, alpha=d.alpha, tie_levels=d.ties)
    d.hub = -1
    if hub:
        d.hub = int(rng.randint(N))
        n = HUB_EDGES + int(rng.randint(300))
        h_dst = rng.randint(0, N, 20)[rng.randint(0, 20, n)]
        h_ts = np.sort(rng.uniform(0, T_MAX, n))
        h_ts = np.floor(h_ts / T_MAX * d.ties) * (T_MAX / d.ties)
        src = np.concatenate([src, np.full(n, d.hub, np.int64)])
        dst = np.concatenate([dst, h_dst.astype(np.int64)])
        ts = np.concatenate([ts, h_ts.astype(np.float32)])
        order = np.argsort(ts, kind="stable")
        src, dst, ts = src[order], dst[order], ts[order]
    d.E = E = len(src)
    if d.far:
        src[rng.choice(E, 3, replace=False)] = N + FAR
    d.zero_node, d.zero_rows = -1, np.empty(0, np.int64)
    if d.negative:
        ts = (ts - np.float32(T_MAX / 2)).astype(np.float32)      # about half are negative
        # six neighbouring edges across the sign change become one node's, at -0.0 and +0.0:
        # the stream still ascends
        z = int(np.searchsorted(ts, 0.0))
        lo, hi = max(z - 3, 0), min(z + 3, E)
        d.zero_node = int(src[min(z, E - 1)])
        d.zero_rows = np.arange(lo, hi)
        src[lo:hi] = d.zero_node
        ts[lo:z], ts[z:hi] = np.float32(-0.0), np.float32(0.0)
    d.half = (E // 2 // d.chunk) * d.chunk
    d.cut = float(ts[d.half // 2]) if d.half else 0.0
    d.offload = d.offload and d.half > 0
    eid = np.arange(E, dtype=np.int64)
    # the newest edge of every node that has one, while the stream is still in time order
    by_node = np.lexsort((ts, src))
    last = np.flatnonzero(np.append(src[by_node][1:] != src[by_node][:-1], True))
    newest = by_node[last]
    if d.shuffle:                                                 # any order inside a call
        for i in range(0, E, d.chunk):
            p = i + rng.permutation(min(d.chunk, E - i))
            src[i:i + len(p)], dst[i:i + len(p)], ts[i:i + len(p)], eid[i:i + len(p)] = \
                src[p], dst[p], ts[p], eid[p]
            went_to = np.empty(len(p), np.int64)                  # old position - i -> new one
            went_to[p - i] = np.arange(i, i + len(p))
            for marked in (newest, d.zero_rows):
                inside = (marked >= i) & (marked < i + len(p))
                marked[inside] = went_to[marked[inside] - i]
    d.src, d.dst, d.ts, d.eid = src, dst, ts, eid
    d.dl = np.unique(dst)
    _draw_queries(d, rng, newest)
    _draw_arguments(d, rng)
    return d


def _draw_queries(d, rng, newest):
    src, dst, ts, E, N = d.src, d.dst, d.ts, d.E, d.N
    d.B = B = int(rng.choice([1, 63, 600, 1500]))
    t_lo, t_hi = float(ts.min()), float(ts.max())
    q_src, _ = synth.random_roots(N, B, T_MAX, seed=int(rng.randint(1 << 30)),
                                  extra_ids=[N + 2, -1])
    q_dst = dst[rng.randint(0, E, B)]
    q_ts = rng.uniform(t_lo - 100.0, t_hi + 100.0, B).astype(np.float32)
    # 0: at an edge of the row's node, 1: later than everything, 2: anywhere, 3: special times
    r = rng.rand(B)
    kind = np.where(r < 0.33, 0, np.where(r < 0.66, 1, 2))
    kind[:2][kind[:2] == 0] = 2                                  # rows 0, 1 keep the unknown ids
    pick = rng.randint(0, E, B)
    at = np.flatnonzero(kind == 0)
    some = rng.permutation(newest)[:(len(at) + 1) // 2]          # the newest edges first
    pick[at[:len(some)]] = some
    q_ts[kind == 1] = np.float32(LATE)
    # about half of the other rows ask for a pair that an edge of the stream names
    own = (kind == 0) | ((rng.rand(B) < 0.5) & (np.arange(B) >= 2))
    q_src[own], q_dst[own] = src[pick[own]], dst[pick[own]]
    q_ts[kind == 0] = ts[pick[kind == 0]]
    if B >= 63:
        sp = np.arange(B - 5, B)
        kind[sp] = 3
        with np.errstate(invalid="ignore"):
            q_ts[sp] = np.array([-np.inf, np.inf, np.nan, -0.0, 0.0], np.float32)
        if d.negative:                                           # the node with the zero times
            q_src[sp] = d.zero_node
            q_dst[sp] = dst[d.zero_rows[np.arange(5) % len(d.zero_rows)]]
        else:
            q_src[sp], q_dst[sp] = src[pick[sp]], dst[pick[sp]]
    d.q_src, d.q_dst, d.q_ts, d.kind = q_src.astype(np.int64), q_dst.astype(np.int64), q_ts, kind
    d.t_lo, d.t_hi = t_lo, t_hi


def since_tensor(q_ts):
    """-inf, NaN, the row's own time and time + 10, in turn."""
    n = len(q_ts)
    with np.errstate(invalid="ignore"):
        cols = np.stack([np.full(n, -np.inf), np.full(n, np.nan), q_ts, q_ts + np.float32(10.0)])
    return cols[np.arange(n) % 4, np.arange(n)].astype(np.float32)


def _draw_arguments(d, rng):
    d.max_history = int(rng.choice([0, 1, 5, 64, 65, 1000]))
    d.since_kind = str(rng.choice(["none", "scalar", "tensor"]))
    scalar = float(np.float32(rng.uniform(d.t_lo, d.t_hi)))
    d.since = {"none": None, "scalar": scalar, "tensor": since_tensor(d.q_ts)}[d.since_kind]
    d.C = C = int(rng.choice([1, 64, 65, 130]))
    d.cands = d.dl[rng.randint(0, len(d.dl), C)].astype(np.int64)
    if C > 1:
        d.cands[C // 2] = d.N + FAR + 20000                      # nobody meets it
    d.K, d.Kh = [(1, 1), (3, 1), (3, 3)][rng.randint(3)]
    d.batch_size = int(rng.choice([64, 257]))
    d.L, d.W = int(rng.choice([1, 3, 8])), int(rng.choice([1, 4]))
    d.recency = int(rng.choice([1, 2, 4]))
    moved = bool(rng.randint(2))
    d.first_row = int(rng.randint(1, 1 << 30)) if moved else 0
    d.epoch = int(rng.randint(1, 1000)) if moved else 0
    d.walk_seed = int(rng.randint(1, 1 << 62, dtype=np.int64))


def arguments(q_src, q_dst, q_ts, dl, negative, **given):
    """What check_readers takes, for a store and queries that were not drawn: the fields of a
    draw, with plain values for whatever `given` does not name."""
    a = types.SimpleNamespace(
        q_src=np.asarray(q_src, np.int64), q_dst=np.asarray(q_dst, np.int64),
        q_ts=np.asarray(q_ts, np.float32), dl=np.unique(dl), negative=negative, max_history=0,
        since=None, K=3, Kh=3, batch_size=257, L=3, W=4, recency=2, first_row=0, epoch=0,
        walk_seed=0x5EED0123456789AB)
    a.cands = a.dl[:130].copy()
    for name, value in given.items():
        assert hasattr(a, name), name
        setattr(a, name, value)
    return a


def features(d):
    """The store features a draw has, of FEATURES."""
    has = dict(negative=d.negative, replace=d.policy == "replace", offload=d.offload,
               shuffle=d.shuffle, far=d.far, hub=d.hub >= 0)
    return [f for f in FEATURES if has[f]]


def describe(d):
    return ("seed %3d N %4d E %5d B %4d %s adaptive=%d min_block %2d chunk %4d reverse=%d "
            "max_history %4d since %-6s C %3d K,Kh %d,%d L %d W %d recency %d [%s]" % (
                d.seed, d.N, d.E, d.B, d.policy, d.adaptive, d.min_block, d.chunk, d.reverse,
                d.max_history, d.since_kind, d.C, d.K, d.Kh, d.L, d.W, d.recency,
                " ".join(features(d))))


def edge_histories(d):
    """{node: (dst, ts, eid)} oldest first from the drawn edge lists alone (no offload)."""
    return T.from_chunks(d.src, d.dst, d.ts, d.eid, d.chunk, add_reverse=d.reverse)[0]


# ---- are the comparisons vacuous?  From a restatement alone ------------------------------
def restate(histories, src, dst, ts, max_history=0, wrong=None):
    """pair_history without `since`, written once more so that it can be made wrong on purpose:
    "le" counts a tie as history, "oldest" bounds to the oldest n, "off_by_one" takes
    max_history + 1 for the bound."""
    N = len(src)
    count = np.zeros(N, np.int64)
    last_ts = np.full(N, -np.inf, np.float32)
    last_eid = np.full(N, -1, np.int64)
    bound = max_history + 1 if wrong == "off_by_one" else max_history
    for i in range(N):
        h = histories.get(int(src[i]))
        if h is None or len(h[0]) == 0:
            continue
        with np.errstate(invalid="ignore"):
            c = int(np.count_nonzero(h[1] <= ts[i] if wrong == "le" else h[1] < ts[i]))
        n = min(c, bound) if bound else c
        lo = 0 if wrong == "oldest" else c - n
        hits = np.flatnonzero(h[0][lo:lo + n] == dst[i]) + lo
        count[i] = len(hits)
        if len(hits):
            last_ts[i], last_eid[i] = h[1][hits[-1]], h[2][hits[-1]]
    return count, last_ts, last_eid


def rows_that_differ(a, b):
    return (a[0] != b[0]) | (bits(a[1]) != bits(b[1])) | (a[2] != b[2])


def check_inputs(d, histories):
    """The conditions under which the exact comparisons of a draw mean something, computed from
    `histories` ({node: (dst, ts, eid)} oldest first) and the draw alone.  Returns the figures."""
    q = (d.q_src, d.q_dst, d.q_ts)
    m = d.max_history
    want = P.pair_history(histories, *q, None, m)
    mine = restate(histories, *q, m)
    assert not rows_that_differ(want, mine).any(), "the second restatement is not the first"
    B = len(d.q_src)
    out = dict(hit=float(np.mean(want[0] > 0)), miss=float(np.mean(want[0] == 0)))
    assert out["hit"] >= 0.10 and out["miss"] >= 0.10, (d.seed, out)
    for wrong in ("le", "oldest", "off_by_one"):
        out[wrong] = float(np.mean(rows_that_differ(want, restate(histories, *q, m, wrong))))
        assert out[wrong] >= 0.01, (d.seed, wrong, out)
    if d.negative:
        # a window taken to start at the node's first edge whenever since <= 0
        out["since_le_0"] = int(np.count_nonzero(rows_that_differ(
            P.pair_history(histories, *q, 0.0, m), want)))
        assert out["since_le_0"] >= 1, (d.seed, out)
        zero = (d.q_ts == 0) & (d.q_src == d.zero_node)
        assert (zero & np.signbit(d.q_ts)).any() and (zero & ~np.signbit(d.q_ts)).any(), d.seed
        h_ts = histories[d.zero_node][1]
        assert ((h_ts == 0) & np.signbit(h_ts)).any() and ((h_ts == 0) & ~np.signbit(h_ts)).any()
    if B >= 63:
        tie = [i for i in np.flatnonzero(d.kind == 0) if int(d.q_src[i]) in histories and
               len(histories[int(d.q_src[i])][1]) and
               histories[int(d.q_src[i])][1][-1] == d.q_ts[i]]
        out["newest_tie"] = len(tie)
        assert len(tie) >= 1, d.seed
    return out


# ---- the store ----------------------------------------------------------------------------
def new_graph(min_block, policy, adaptive):
    import gnnflow_amd
    return gnnflow_amd.DynamicGraph(1 << 20, 1024 << 20, "cuda", min_block, 128, policy,
                                    adaptive_block_size=adaptive)


def build_store(d):
    """No reader has been launched on this graph yet: nothing to synchronise with."""
    g = new_graph(d.min_block, d.policy, d.adaptive)
    h = d.half
    synth.ingest_chunks(g, d.src[:h], d.dst[:h], d.ts[:h], d.eid[:h], d.chunk, add_reverse=d.reverse)
    d.offloaded = g.offload_old_blocks(d.cut) if d.offload else 0
    synth.ingest_chunks(g, d.src[h:], d.dst[h:], d.ts[h:], d.eid[h:], d.chunk, add_reverse=d.reverse)
    return g


# ---- check A ------------------------------------------------------------------------------
def check_against_restatements(g, a, tag):
    import torch
    from gnnflow_amd import DeviceDstSet
    from tests import test_gpu_hist_negatives as TH
    from tests import test_gpu_pair_history as TP
    from tests import test_gpu_seen_mask as TS
    from tests import test_gpu_temporal_walk as TW
    src, dst, ts, m = a.q_src, a.q_dst, a.q_ts, a.max_history
    hist = P.from_graph(g, src)
    lower_ends = [a.since] + ([None] if a.since is not None else []) + \
        ([0.0] if a.negative else [])
    out = {}
    for since in lower_ends:
        got = TP._call(g, src, dst, ts, since, m)
        want = P.pair_history(hist, src, dst, ts, since, m)
        if since is None:
            out["pair"] = got
        try:
            TP._same(got, want)
        except AssertionError:
            bad = np.flatnonzero(rows_that_differ(got, want))
            raise AssertionError("%s pair_history since=%s: rows %s got %s want %s" % (
                tag, "tensor" if isinstance(since, np.ndarray) else since, bad[:5],
                [x[bad[:5]] for x in got], [x[bad[:5]] for x in want]))
    out["mask"] = TS._call(g, src, ts, a.cands, m)
    want = S.seen_mask(S.from_graph(g, src), src, ts, a.cands, m)
    assert np.array_equal(out["mask"], want), \
        "%s seen_mask: rows %s" % (tag, np.flatnonzero((out["mask"] != want).any(1))[:5])
    walk_hist, table_len = T.from_graph(g)
    kw = dict(recency=a.recency, max_history=m, seed=a.walk_seed, epoch=a.epoch,
              first_row=a.first_row)
    got = TW._call(g, src, ts, a.L, a.W, **kw)
    want = T.walks(walk_hist, table_len, src, ts, a.L, a.W, **kw)
    assert TW._same(got, want), \
        "%s temporal_random_walk: rows %s" % (tag, np.flatnonzero((got[1] != want[1]).any((1, 2)))[:5])
    # the historical negatives: the query rows are the stream
    toy = types.SimpleNamespace(src=src, dst=dst, time=ts, rows=len(src), graph=g, dl=a.dl,
                                eid=np.arange(len(src), dtype=np.int64))
    toy.dst_set = DeviceDstSet(int(a.dl.max()) + 1, "cuda:0", a.dl)
    neg_hist, neg_len = TH._histories(g)
    assert neg_len == table_len
    ref = TH._reference(toy, neg_hist, neg_len, a.K, epoch=a.epoch, first_row=a.first_row)
    stream = TH._stream(toy, a.batch_size, a.K, a.Kh, first_row=a.first_row)
    plain = TH._stream(toy, a.batch_size, a.K, 0, first_row=a.first_row)
    stream.set_epoch(a.epoch), plain.set_epoch(a.epoch)
    changed = np.zeros((a.Kh, len(src)), bool)
    negs = np.zeros((a.Kh, len(src)), np.int64)
    for b in range(len(stream)):
        lo, hi = int(stream.borders[b]), int(stream.borders[b + 1])
        roots = stream.batch(b)[0].cpu().numpy()
        assert np.array_equal(roots, TH._want_roots(toy, ref, lo, hi, a.K, a.Kh)), \
            "%s hist_negatives batch %d" % (tag, b)
        got = roots[2 * (hi - lo):].reshape(a.K, hi - lo)[:a.Kh]
        base = plain.batch(b)[0].cpu().numpy()[2 * (hi - lo):].reshape(a.K, hi - lo)[:a.Kh]
        negs[:, lo:hi], changed[:, lo:hi] = got, got != base
    assert int(stream.hist_filled.item()) == H.filled(ref[2][:a.Kh]), tag + " hist_filled"
    out["negs"], out["neg_changed"] = negs, changed
    torch.cuda.synchronize()
    return out


# ---- check B ------------------------------------------------------------------------------
def sampled_sets(g, src, ts, k, window):
    """Per row, what TemporalSampler(g, [k], "recent") sampled: (neighbour ids, timestamps,
    edge ids), read off the block the way the sampler's parity test reads it."""
    import gnnflow_amd
    kw = dict(snapshot_time_window=window) if window else {}
    block = gnnflow_amd.TemporalSampler(g, [k], "recent", **kw).sample(src, ts)[0][0]
    R = len(src)
    assert block.num_dst_nodes() == R
    ids = block.srcdata["ID"].cpu().numpy()
    times = block.srcdata["ts"].cpu().numpy()
    col, row = (x.cpu().numpy() for x in block.edges())
    eid = block.edata["ID"].cpu().numpy()
    assert np.array_equal(ids[:R], src) and len(col) == len(row) == len(eid) == len(ids) - R
    order = np.argsort(row, kind="stable")
    ends = np.searchsorted(row[order], np.arange(R + 1))
    nbr, t, e = ids[col][order], times[col][order], eid[order]
    return [(nbr[ends[i]:ends[i + 1]], t[ends[i]:ends[i + 1]], e[ends[i]:ends[i + 1]])
            for i in range(R)]


def check_against_sampler(g, a, got, tag):
    from tests import test_gpu_temporal_walk as TW
    src, dst, ts, m = a.q_src, a.q_dst, a.q_ts, a.max_history
    k = m if m else UNBOUNDED_K
    known = (src >= 0) & (src <= g.max_vertex_id())
    degree = np.zeros(len(src), np.int64)
    degree[known] = g.out_degree(src[known]).astype(np.int64)
    whole = degree <= k                        # the sample holds the node's whole history
    rows = np.ones(len(src), bool) if m else whole.copy()
    if a.negative:
        rows &= ~np.isposinf(ts)
    sets = sampled_sets(g, src, ts, k, WINDOW if a.negative else 0.0)
    walks = TW._call(g, src, ts, 1, a.W, recency=a.recency, max_history=m, seed=a.walk_seed,
                     epoch=a.epoch, first_row=a.first_row)
    count, last_ts, last_eid = got["pair"]
    seen = S.unpack(got["mask"], len(a.cands))
    for i in np.flatnonzero(rows):
        nbr, t, e = sets[i]
        where = "%s row %d (src %d dst %d t %r)" % (tag, i, src[i], dst[i], ts[i])
        assert len(nbr) <= k, where
        hit = nbr == dst[i]
        assert count[i] == hit.sum(), where + " count"
        if count[i]:
            # the maximum by value; -0.0 and +0.0 are one value with two bit patterns, so the
            # bits are those of the sampled edge that last_eid names
            last = hit & (e == last_eid[i])
            assert last.any(), where + " last_eid"
            assert last_ts[i] == t[hit].max() and \
                (bits(t[last]) == bits(last_ts[i:i + 1])[0]).all(), where + " last_ts"
        assert np.array_equal(seen[i], np.isin(a.cands, nbr)), where + " seen_mask"
        for w in range(a.W):
            if walks[1][i, w, 0] == -1:
                assert len(nbr) == 0 and walks[0][i, w, 1] == -1, where + " walk ended"
                continue
            at = np.flatnonzero(e == walks[1][i, w, 0])
            assert len(at) and (nbr[at] == walks[0][i, w, 1]).any(), where + " walk edge"
            assert (bits(t[at]) == bits(walks[2][i, w, :1])[0]).any(), where + " walk time"
        if whole[i]:
            filled = got["negs"][got["neg_changed"][:, i], i]
            assert np.isin(filled, nbr).all(), where + " historical negative"
    return int(rows.sum())


def check_readers(g, a, tag):
    """Checks A and B of the readers on graph `g` for the queries and arguments in `a` (the
    fields draw() sets: q_src, q_dst, q_ts, max_history, since, cands, dl, K, Kh, batch_size, L,
    W, recency, first_row, epoch, walk_seed, negative).  Returns the rows check B covered."""
    got = check_against_restatements(g, a, tag)
    return check_against_sampler(g, a, got, tag)


def run(seed, conditions=False, verbose=True):
    """One seed: draw, build, check.  conditions=True also asserts check_inputs on the histories
    the store holds (the CPU test asserts them on histories built from the edge lists)."""
    d = draw(seed)
    g = build_store(d)
    tag = "seed %d" % seed
    if not d.offload:      # the store's order restated from the edge lists, a third reference
        want = edge_histories(d)
        have, _ = T.from_graph(g)
        assert sorted(v for v in have if len(have[v][0])) == sorted(want), tag
        for v, h in want.items():
            assert all(np.array_equal(x, y) for x, y in zip(h, have[v])) and \
                np.array_equal(bits(h[1]), bits(have[v][1])), (tag, v)
    if conditions:
        check_inputs(d, P.from_graph(g, d.q_src))
    covered = check_readers(g, d, tag)
    if verbose:
        print(describe(d) + " ok, check B on %d rows" % covered, flush=True)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=30)
    ap.add_argument("--first", type=int, default=0)
    args = ap.parse_args()
    for seed in range(args.first, args.first + args.seeds):
        run(seed)
    print("all ok")


if __name__ == "__main__":
    main()
