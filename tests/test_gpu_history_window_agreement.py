"""One history window, the same number from every reader that can express it
(csrc/history_window.hpp): temporal_degree, pair_history(...).count, common_neighbors(...).n_src
and n_dst, whether seen_mask sets a bit, and whether temporal_random_walk takes step 0, each
against tests/pair_history_ref.py's count.

Every edge of node v leads to DST + v, so that pair_history's count of (v, DST + v) is the size
of v's window, seen_mask's row has a bit iff the window has an edge, and a walk's first step
exists iff it has one.  Nodes 0 .. 5 hold 0, 1, 63, 64, 65 and 129 live edges, the boundaries of
the 64-lane stride of the wave-per-row kernels; node 0 had nine edges, all in a block that
offload_old_blocks took.  The times of a node are 100, 100, 100, 101, 101, 101, ...: ties.
Expected values are computed once per (since, max_history) and left unchanged.

Only the SIZE of a window is compared here.  With one destination per node a window of the right
size in the wrong place (a wrong c - n under max_history) gives the same numbers: which records a
window holds is checked by the per-reader tests and by test_gpu_history_readers_fuzz.py."""
import itertools

import numpy as np
import pytest
import torch

from tests import pair_history_ref as P

pytestmark = pytest.mark.gpu

LIVE = [0, 1, 63, 64, 65, 129]      # live edges of nodes 0 .. 5
DST = 10                            # node v's edges lead to DST + v; DST + 5 ends the node table
OLD = 9                             # node 0's edges, all before the offload
T_TIE, T_TIE_OF_ONE, T_AFTER = 110.0, 100.0, 1e9
SINCE_TIE, SINCE_ABOVE = 105.0, 2e9
HISTORIES = [0, 1, 64, 65]


class Toy:
    pass


@pytest.fixture(scope="module")
def toy():
    import gnnflow_amd
    t = Toy()
    g = gnnflow_amd.DynamicGraph(1 << 20, 1 << 28, "cuda", 8, 128, "insert")
    g.add_edges(np.zeros(OLD, np.int64), np.full(OLD, DST, np.int64),
                np.arange(1, OLD + 1, dtype=np.float32))
    src = np.concatenate([np.full(n, v, np.int64) for v, n in enumerate(LIVE)])
    ts = np.concatenate([100 + np.arange(n) // 3 for n in LIVE]).astype(np.float32)
    order = np.argsort(ts, kind="stable")
    g.add_edges(src[order], DST + src[order], ts[order])
    t.edges_before = g.num_edges()
    torch.cuda.synchronize()
    t.offloaded = g.offload_old_blocks(50.0)
    t.graph = g
    t.past_table = g.max_vertex_id() + 1
    nodes = list(range(len(LIVE))) + [-1, t.past_table]
    times = [T_TIE, T_TIE_OF_ONE, T_AFTER, np.nan]
    sinces = [np.nan, SINCE_TIE, SINCE_ABOVE, -np.inf]
    rows = list(itertools.product(nodes, times, sinces))
    t.src = np.array([r[0] for r in rows], np.int64)
    t.ts = np.array([r[1] for r in rows], np.float32)
    t.since = np.array([r[2] for r in rows], np.float32)
    t.dst = DST + t.src
    t.hist = P.from_graph(g, t.src)
    t.d_src, t.d_dst = torch.from_numpy(t.src).cuda(), torch.from_numpy(t.dst).cuda()
    t.d_ts, t.d_since = torch.from_numpy(t.ts).cuda(), torch.from_numpy(t.since).cuda()
    t.d_cands = torch.arange(DST, DST + len(LIVE), dtype=torch.int64, device="cuda")
    t.ref = {}
    return t


def _want(toy, with_since, max_history):
    """the window's size per row, from the numpy reference"""
    key = (with_since, max_history)
    if key not in toy.ref:
        toy.ref[key] = P.pair_history(toy.hist, toy.src, toy.dst, toy.ts,
                                      toy.since if with_since else None, max_history)[0]
    return toy.ref[key]


def test_the_store_and_the_queries_hold_every_case(toy):
    """From the store and the reference alone: the comparisons below are not vacuous."""
    assert toy.offloaded > 0 and toy.graph.num_edges() == toy.edges_before - OLD == sum(LIVE)
    assert toy.past_table == DST + len(LIVE)
    for v, n in enumerate(LIVE):
        d, t, _ = toy.graph.get_temporal_neighbors(v)
        assert len(d) == n and (d == DST + v).all()                    # one destination per node
        if n >= 63:
            assert (t == np.float32(T_TIE)).sum() == 3                 # t at a tie
            assert (t == np.float32(SINCE_TIE)).sum() == 3             # since at a tie
        if n:
            assert (t == np.float32(T_TIE_OF_ONE)).sum() == min(n, 3) and t.max() < T_AFTER
    src, ts, since = toy.src, toy.ts, toy.since
    assert (src == -1).any() and (src == toy.past_table).any()
    assert np.isnan(ts).any() and np.isnan(since).any() and np.isneginf(since).any()
    with np.errstate(invalid="ignore"):
        assert (since > ts).any() and ((since == SINCE_TIE) & (ts == T_TIE)).any()
    whole = _want(toy, False, 0)
    after = ts == np.float32(T_AFTER)
    assert [int(whole[after & (src == v)][0]) for v in range(len(LIVE))] == LIVE    # the shortcut
    tie = ts == np.float32(T_TIE)
    assert [int(whole[tie & (src == v)][0]) for v in range(len(LIVE))] == [0, 1, 30, 30, 30, 30]
    assert (whole[ts == np.float32(T_TIE_OF_ONE)] == 0).all()          # strictly before
    assert (whole[np.isnan(ts)] == 0).all()
    assert (whole[(src < 0) | (src >= toy.past_table)] == 0).all()
    lower = _want(toy, True, 0)
    assert (lower[np.isnan(since)] == whole[np.isnan(since)]).all()    # a NaN since: no lower end
    assert (lower[since == np.float32(SINCE_ABOVE)] == 0).all()        # since > t: nothing
    at_tie = after & (since == np.float32(SINCE_TIE))                  # inclusive: the tie counts
    assert [int(lower[at_tie & (src == v)][0]) for v in (2, 3, 4, 5)] == [48, 49, 50, 114]
    # the bounds cut where they should: 65 -> 64, 129 -> 65
    assert int(_want(toy, False, 64)[after & (src == 4)][0]) == 64
    assert int(_want(toy, False, 65)[after & (src == 5)][0]) == 65
    assert int(_want(toy, False, 1).max()) == 1


@pytest.mark.parametrize("with_since", [False, True])
@pytest.mark.parametrize("max_history", HISTORIES)
def test_every_reader_reports_the_same_window(toy, max_history, with_since):
    g, H = toy.graph, max_history
    want = _want(toy, with_since, H)
    since = toy.d_since if with_since else None
    got = {}
    degree = g.temporal_degree(toy.d_src, toy.d_ts, since=since)
    got["temporal_degree"] = torch.clamp(degree, max=H) if H else degree
    got["pair_history"] = g.pair_history(toy.d_src, toy.d_dst, toy.d_ts, since=since,
                                         max_history=H).count
    if H:                                        # common_neighbors needs a bound
        cn = g.common_neighbors(toy.d_src, toy.d_src, toy.d_ts, since=since, max_history=H,
                                max_common=1)
        got["common_neighbors.n_src"], got["common_neighbors.n_dst"] = cn.n_src, cn.n_dst
    for name, n in got.items():
        assert np.array_equal(n.cpu().numpy().astype(np.int64), want), name
    if with_since:                               # seen_mask and the walks have no lower end
        return
    mask = g.seen_mask(toy.d_src, toy.d_ts, toy.d_cands, max_history=H).cpu().numpy()
    assert mask.shape == (len(toy.src), 1)
    bits = np.array([bin(int(w) & (2 ** 64 - 1)).count("1") for w in mask[:, 0]])
    assert np.array_equal(bits > 0, want > 0)
    own = np.where(want > 0, 1 << np.clip(toy.src, 0, len(LIVE) - 1), 0)
    assert np.array_equal(mask[:, 0], own)       # and the one bit is the node's own destination
    walks = g.temporal_random_walk(toy.d_src, toy.d_ts, 1, max_history=H)
    stepped = walks.nodes[:, 0, 1].cpu().numpy()
    assert np.array_equal(stepped != -1, want > 0)
    assert np.array_equal(stepped[want > 0], toy.dst[want > 0])
