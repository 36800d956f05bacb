"""Which error wins when two arguments of an edge-history reader are wrong at once.

The seven checkers (dynamic_graph.check_seen_mask_args, check_pair_history_args,
check_common_neighbors_args, check_temporal_degree_args, check_temporal_walk_args,
check_neighbor_aggregate_args, check_neighbor_sequence_args) report their errors in a fixed order,
and callers see that order: the per-reader error tests pin every message, this file pins the
order.  Each case breaks two checks that are adjacent in a checker's order and
names the one reported; the expected winners were written from the checkers as they stood before
they were folded onto shared helpers.  CPU only: a tensor on `meta` stands for another device, and
a zero-stride view for 2**31 rows without their memory."""
import numpy as np
import pytest
import torch

from gnnflow_amd.dynamic_graph import (check_common_neighbors_args, check_neighbor_aggregate_args,
                                       check_neighbor_sequence_args, check_pair_history_args,
                                       check_seen_mask_args, check_temporal_degree_args,
                                       check_temporal_walk_args)

BIG = 2 ** 31


def i64(n=4, device="cpu"):
    return torch.zeros(n, dtype=torch.int64, device=device)


def f32(n=4, device="cpu"):
    return torch.zeros(n, dtype=torch.float32, device=device)


def big(dtype, device="cpu"):
    return torch.zeros(1, dtype=dtype, device=device).expand(BIG)


def tab(rows=6, cols=8, device="cpu"):
    return torch.zeros((rows, cols), dtype=torch.float32, device=device)


def seen(**over):
    a = dict(src=i64(), ts=f32(), cand_ids=i64(5), max_history=0)
    a.update(over)
    return check_seen_mask_args(**a)


def pair(**over):
    a = dict(src=i64(), dst=i64(), ts=f32(), since=None, max_history=0)
    a.update(over)
    return check_pair_history_args(**a)


def common(**over):
    a = dict(src=i64(), dst=i64(), ts=f32(), since=None, max_history=64, max_common=32)
    a.update(over)
    return check_common_neighbors_args(**a)


def degree(**over):
    a = dict(nodes=torch.zeros((3, 5), dtype=torch.int64), ts=torch.zeros((3, 5)), since=None)
    a.update(over)
    return check_temporal_degree_args(**a)


def walk(**over):
    a = dict(src=i64(), ts=f32(), length=3, num_walks=2, recency=1, max_history=0, seed=0, epoch=0,
             first_row=0)
    a.update(over)
    return check_temporal_walk_args(**a)


def agg(**over):
    # one table: taking it away is then a fault of its own
    a = dict(nodes=i64(), ts=f32(), node_feats=tab(), edge_feats=None, since=None, max_history=0,
             reduce="mean")
    a.update(over)
    return check_neighbor_aggregate_args(**a)


def seq(**over):
    a = dict(nodes=i64(), ts=f32(), since=None, length=8, edge_feats=tab(), node_feats=tab(),
             time_encoder=(tab(4, 1), f32()))
    a.update(over)
    return check_neighbor_sequence_args(**a)


# (checker, the two faults, the exception, what its message starts with)
CASES = [
    # seen_mask: types of src, ts, cand_ids; max_history's type; 1-D; ts's length; no candidate;
    # 2**31 candidates; 2**31 rows; max_history's sign; devices of ts, cand_ids
    (seen, dict(src=i64().int(), ts=f32().double()), TypeError, "src must be torch.int64"),
    (seen, dict(src=[0, 1], ts=f32().double()), TypeError, "src must be a tensor"),
    (seen, dict(ts=np.zeros(4, np.float32), cand_ids=i64(5).int()), TypeError,
     "ts must be a tensor"),
    (seen, dict(cand_ids=i64(5).int(), max_history=1.0), TypeError, "cand_ids must be torch.int64"),
    (seen, dict(max_history=True, src=i64().reshape(2, 2)), TypeError,
     "max_history must be an int"),
    (seen, dict(max_history=np.int64(3), ts=f32(3)), TypeError, "max_history must be an int"),
    (seen, dict(src=i64().reshape(2, 2), ts=f32()[0]), ValueError, "src must be 1-D"),
    (seen, dict(cand_ids=i64(6).reshape(2, 3), ts=f32(3)), ValueError, "cand_ids must be 1-D"),
    (seen, dict(ts=f32(3), cand_ids=i64(0)), ValueError, "src has 4 rows, ts has 3"),
    (seen, dict(ts=f32(3), max_history=-1), ValueError, "src has 4 rows, ts has 3"),
    (seen, dict(cand_ids=i64(0), src=big(torch.int64), ts=big(torch.float32)), ValueError,
     "seen_mask needs at least one candidate"),
    (seen, dict(cand_ids=big(torch.int64), src=big(torch.int64), ts=big(torch.float32)),
     ValueError, "seen_mask takes fewer than 2\\*\\*31 candidates"),
    (seen, dict(src=big(torch.int64), ts=big(torch.float32), max_history=-1), ValueError,
     "seen_mask takes fewer than 2\\*\\*31 rows"),
    (seen, dict(max_history=-1, ts=f32(4, "meta")), ValueError, "max_history must be >= 0"),
    (seen, dict(ts=f32(4, "meta"), cand_ids=i64(5, "meta")), ValueError, "ts is on meta, src on"),
    # pair_history: types of src, dst, ts, since; max_history's type; 1-D; lengths; 2**31 rows;
    # max_history's sign; devices
    (pair, dict(src=i64().int(), dst=f32()), TypeError, "src must be torch.int64"),
    (pair, dict(ts=f32().double(), since="yesterday"), TypeError, "ts must be torch.float32"),
    (pair, dict(since=f32().double(), max_history=None), TypeError, "since must be torch.float32"),
    (pair, dict(since=True, max_history=None), TypeError, "since must be None, a float or"),
    (pair, dict(max_history=2.0, dst=i64()[0]), TypeError, "max_history must be an int"),
    (pair, dict(max_history=np.int64(2), ts=f32(3)), TypeError, "max_history must be an int"),
    (pair, dict(since=f32().reshape(2, 2), dst=i64(3)), ValueError, "since must be 1-D"),
    (pair, dict(dst=i64(3), ts=f32(5)), ValueError, "src has 4 rows, dst has 3"),
    (pair, dict(src=big(torch.int64), dst=i64(3)), ValueError,
     "src has 2147483648 rows, dst has 3"),
    (pair, dict(ts=f32(3), max_history=-1), ValueError, "src has 4 rows, ts has 3"),
    (pair, dict(src=big(torch.int64), dst=big(torch.int64), ts=big(torch.float32),
                max_history=-1), ValueError, "pair_history takes fewer than 2\\*\\*31 rows"),
    (pair, dict(max_history=-1, dst=i64(4, "meta")), ValueError, "max_history must be >= 0"),
    (pair, dict(dst=i64(4, "meta"), since=f32(4, "meta")), ValueError, "dst is on meta, src on"),
    # common_neighbors: types; max_history's type, then range; max_common's type, then range;
    # 1-D; lengths; 2**31 rows; devices
    (common, dict(dst=i64().int(), max_history=1.0), TypeError, "dst must be torch.int64"),
    (common, dict(since=(1.0,), max_history=0), TypeError, "since must be None, a float or"),
    (common, dict(max_history=None, max_common=-1), TypeError, "max_history must be an int"),
    (common, dict(max_history=0, max_common=1.0), ValueError,
     "max_history must be in \\[1, 513\\)"),
    (common, dict(max_history=513, src=i64()[0]), ValueError, "max_history must be in"),
    (common, dict(max_common="3", src=i64()[0]), TypeError, "max_common must be an int"),
    (common, dict(max_common=513, ts=f32().reshape(2, 2)), ValueError,
     "max_common must be in \\[0, 513\\)"),
    (common, dict(ts=f32().reshape(2, 2), dst=i64(3)), ValueError, "ts must be 1-D"),
    (common, dict(dst=i64(3), ts=f32(3, "meta")), ValueError, "src has 4 rows, dst has 3"),
    (common, dict(src=big(torch.int64), dst=big(torch.int64), ts=big(torch.float32, "meta")),
     ValueError, "common_neighbors takes fewer than 2\\*\\*31 rows"),
    (common, dict(ts=f32(4, "meta"), since=f32(4, "meta")), ValueError, "ts is on meta, src on"),
    # temporal_degree: types of nodes, ts, since; shapes of ts, since; 2**31 elements; devices
    (degree, dict(nodes=torch.zeros((3, 5), dtype=torch.int32), ts=torch.zeros((5, 3))),
     TypeError, "nodes must be torch.int64"),
    (degree, dict(since="3", ts=torch.zeros((5, 3))), TypeError, "since must be None, a float or"),
    (degree, dict(ts=torch.zeros((5, 3)), since=torch.zeros(15)), ValueError,
     "nodes has shape \\(3, 5\\), ts has \\(5, 3\\)"),
    (degree, dict(since=torch.zeros(15), ts=torch.zeros((3, 5), device="meta")), ValueError,
     "nodes has shape \\(3, 5\\), since has \\(15,\\)"),
    (degree, dict(nodes=big(torch.int64), ts=f32(3)), ValueError,
     "nodes has shape \\(2147483648,\\), ts has \\(3,\\)"),
    (degree, dict(nodes=big(torch.int64), ts=big(torch.float32, "meta")), ValueError,
     "temporal_degree takes fewer than 2\\*\\*31 elements"),
    (degree, dict(ts=torch.zeros((3, 5), device="meta"),
                  since=torch.zeros((3, 5), device="meta")), ValueError, "ts is on meta, nodes on"),
    # temporal_random_walk: types of src, ts; then length, num_walks, recency, max_history, seed,
    # epoch, first_row, each its type and then its range; 1-D; ts's length; 2**31 walks; device
    (walk, dict(ts=f32().double(), length=1.0), TypeError, "ts must be torch.float32"),
    (walk, dict(length=True, num_walks=0), TypeError, "length must be an int"),
    (walk, dict(length=33, num_walks=1.0), ValueError, "length must be in \\[1, 33\\)"),
    (walk, dict(num_walks=2 ** 16, recency=None), ValueError, "num_walks must be in"),
    (walk, dict(recency=9, max_history=-1), ValueError, "recency must be in \\[1, 9\\)"),
    (walk, dict(max_history=-1, seed=-1), ValueError, "max_history must be in"),
    (walk, dict(seed=2 ** 64, epoch="0"), ValueError, "seed must be in"),
    (walk, dict(epoch=-1, first_row=1.5), ValueError, "epoch must be in"),
    (walk, dict(first_row=-1, src=i64().reshape(2, 2)), ValueError, "first_row must be in"),
    (walk, dict(src=i64().reshape(2, 2), ts=f32(3)), ValueError, "src must be 1-D"),
    (walk, dict(ts=f32(3, "meta")), ValueError, "src has 4 rows, ts has 3"),
    (walk, dict(src=big(torch.int64), ts=f32(3)), ValueError, "src has 2147483648 rows, ts has 3"),
    (walk, dict(src=big(torch.int64), ts=big(torch.float32, "meta")), ValueError,
     "temporal_random_walk takes fewer than 2\\*\\*31 walks"),
    (walk, dict(src=i64(2 ** 15), ts=f32(2 ** 15, "meta"), num_walks=2 ** 16 - 1), ValueError,
     "ts is on meta, src on"),
    # neighbor_aggregate: half-precision node_feats, edge_feats; types of nodes, ts, node_feats,
    # edge_feats, since; max_history's type; reduce's type; 1-D; lengths; 2**31 rows; no table;
    # per table, node_feats first: 2-D, no rows, columns, contiguous; reduce's value;
    # max_history's sign; devices
    (agg, dict(node_feats=tab().half(), nodes=i64().int()), TypeError,
     "node_feats must be float32, got torch.float16: half-precision"),
    (agg, dict(node_feats=tab().half(), edge_feats=tab().bfloat16()), TypeError,
     "node_feats must be float32, got torch.float16"),
    (agg, dict(edge_feats=tab().bfloat16(), nodes=[0, 1]), TypeError,
     "edge_feats must be float32, got torch.bfloat16: half-precision"),
    (agg, dict(nodes=i64().int(), ts=f32().double()), TypeError, "nodes must be torch.int64"),
    (agg, dict(ts=f32().double(), node_feats=tab().double()), TypeError,
     "ts must be torch.float32"),
    (agg, dict(node_feats=tab().double(), edge_feats=tab().int()), TypeError,
     "node_feats must be torch.float32"),
    (agg, dict(edge_feats=np.zeros((6, 8), np.float32), since=f32().double()), TypeError,
     "edge_feats must be a tensor"),
    (agg, dict(since=f32().double(), max_history=None), TypeError, "since must be torch.float32"),
    (agg, dict(since="yesterday", max_history=1.0), TypeError, "since must be None, a float or"),
    (agg, dict(max_history=True, reduce=None), TypeError, "max_history must be an int"),
    (agg, dict(max_history=np.int64(3), reduce=None), TypeError, "max_history must be an int"),
    (agg, dict(reduce=None, nodes=i64().reshape(2, 2)), TypeError, "reduce must be a str"),
    (agg, dict(nodes=i64().reshape(2, 2), ts=f32(3)), ValueError, "nodes must be 1-D"),
    (agg, dict(since=f32().reshape(2, 2), ts=f32(3)), ValueError, "since must be 1-D"),
    (agg, dict(ts=f32(3), since=f32(5)), ValueError, "nodes has 4 rows, ts has 3"),
    (agg, dict(since=f32(5), node_feats=None), ValueError, "nodes has 4 rows, since has 5"),
    (agg, dict(nodes=big(torch.int64), ts=f32(3)), ValueError,
     "nodes has 2147483648 rows, ts has 3"),
    (agg, dict(nodes=big(torch.int64), ts=big(torch.float32), node_feats=None), ValueError,
     "neighbor_aggregate takes fewer than 2\\*\\*31 rows"),
    (agg, dict(node_feats=None, reduce="max"), ValueError,
     "neighbor_aggregate needs node_feats or edge_feats"),
    (agg, dict(node_feats=None, max_history=-1), ValueError,
     "neighbor_aggregate needs node_feats or edge_feats"),
    (agg, dict(node_feats=torch.zeros(0)), ValueError, "node_feats must be 2-D"),
    (agg, dict(node_feats=tab(0, 2000)), ValueError, "node_feats has no rows"),
    (agg, dict(node_feats=tab(2000, 6).t()), ValueError,
     "node_feats must have 1 to 1024 columns, got 2000"),
    (agg, dict(node_feats=tab().t(), edge_feats=f32(6)), ValueError,
     "node_feats must be contiguous"),
    (agg, dict(edge_feats=f32(6), reduce="max"), ValueError, "edge_feats must be 2-D"),
    (agg, dict(edge_feats=tab().t(), reduce="max"), ValueError, "edge_feats must be contiguous"),
    (agg, dict(reduce="max", max_history=-1), ValueError, "reduce must be 'sum' or 'mean'"),
    (agg, dict(max_history=-1, ts=f32(4, "meta")), ValueError, "max_history must be >= 0"),
    (agg, dict(ts=f32(4, "meta"), node_feats=tab(device="meta")), ValueError,
     "ts is on meta, nodes on"),
    (agg, dict(node_feats=tab(device="meta"), since=f32(4, "meta")), ValueError,
     "node_feats is on meta, nodes on"),
    # neighbor_sequence: half-precision edge_feats, node_feats; what time_encoder is; types of
    # nodes, ts, edge_feats, node_feats, the encoder's weight and bias, since; length's type, then
    # range; 1-D; lengths; 2**31 rows; per table, edge_feats first: 2-D, no rows, columns,
    # contiguous; the encoder's bias, width, weight; devices
    (seq, dict(edge_feats=tab().half(), nodes=i64().int()), TypeError,
     "edge_feats must be float32, got torch.float16: half-precision"),
    (seq, dict(edge_feats=tab().bfloat16(), node_feats=tab().half()), TypeError,
     "edge_feats must be float32, got torch.bfloat16"),
    (seq, dict(node_feats=tab().half(), time_encoder=3), TypeError,
     "node_feats must be float32, got torch.float16: half-precision"),
    (seq, dict(time_encoder=(f32(), f32(), f32()), nodes=i64().int()), TypeError,
     "time_encoder must be a module or a \\(weight, bias\\) pair, got 3 elements"),
    (seq, dict(time_encoder=3, nodes=[0, 1]), TypeError,
     "time_encoder must be a module with weight and bias or"),
    (seq, dict(nodes=i64().int(), ts=f32().double()), TypeError, "nodes must be torch.int64"),
    (seq, dict(ts=f32().double(), edge_feats=tab().double()), TypeError,
     "ts must be torch.float32"),
    (seq, dict(edge_feats=tab().double(), node_feats=tab().int()), TypeError,
     "edge_feats must be torch.float32"),
    (seq, dict(node_feats=tab().int(), time_encoder=(tab(4, 1).double(), f32())), TypeError,
     "node_feats must be torch.float32"),
    (seq, dict(time_encoder=(tab(4, 1).double(), f32().double())), TypeError,
     "time_encoder's weight must be torch.float32"),
    (seq, dict(time_encoder=(tab(4, 1), [0.0] * 4), since=f32().double()), TypeError,
     "time_encoder's bias must be a tensor"),
    (seq, dict(since=f32().double(), length=1.0), TypeError, "since must be torch.float32"),
    (seq, dict(since="yesterday", length=None), TypeError, "since must be None, a float or"),
    (seq, dict(length=True, nodes=i64().reshape(2, 2)), TypeError, "length must be an int"),
    (seq, dict(length=513, nodes=i64().reshape(2, 2)), ValueError,
     "length must be in \\[1, 513\\)"),
    (seq, dict(nodes=i64().reshape(2, 2), ts=f32(3)), ValueError, "nodes must be 1-D"),
    (seq, dict(since=f32().reshape(2, 2), ts=f32(3)), ValueError, "since must be 1-D"),
    (seq, dict(ts=f32(3), since=f32(5)), ValueError, "nodes has 4 rows, ts has 3"),
    (seq, dict(since=f32(5), edge_feats=f32(6)), ValueError, "nodes has 4 rows, since has 5"),
    (seq, dict(nodes=big(torch.int64), ts=f32(3)), ValueError,
     "nodes has 2147483648 rows, ts has 3"),
    (seq, dict(nodes=big(torch.int64), ts=big(torch.float32), edge_feats=f32(6)), ValueError,
     "neighbor_sequence takes fewer than 2\\*\\*31 rows"),
    (seq, dict(edge_feats=torch.zeros(0)), ValueError, "edge_feats must be 2-D"),
    (seq, dict(edge_feats=tab(0, 2000)), ValueError, "edge_feats has no rows"),
    (seq, dict(edge_feats=tab(2000, 6).t()), ValueError,
     "edge_feats must have 1 to 1024 columns, got 2000"),
    (seq, dict(edge_feats=tab().t(), node_feats=f32(6)), ValueError,
     "edge_feats must be contiguous"),
    (seq, dict(node_feats=f32(6), time_encoder=(tab(4, 1), tab(4, 1))), ValueError,
     "node_feats must be 2-D"),
    (seq, dict(node_feats=tab().t(), time_encoder=(tab(4, 1), tab(4, 1))), ValueError,
     "node_feats must be contiguous"),
    (seq, dict(time_encoder=(tab(3, 1), tab(2000, 1))), ValueError,
     "time_encoder's bias must be \\[dT\\], got shape \\(2000, 1\\)"),
    (seq, dict(time_encoder=(tab(3, 1), f32(2000))), ValueError,
     "time_encoder must have 1 to 1024 columns, got 2000"),
    (seq, dict(time_encoder=(tab(3, 1), f32()), ts=f32(4, "meta")), ValueError,
     "time_encoder's weight must be \\[dT, 1\\] or \\[dT\\] with dT = 4"),
    (seq, dict(ts=f32(4, "meta"), edge_feats=tab(device="meta")), ValueError,
     "ts is on meta, nodes on"),
    (seq, dict(edge_feats=tab(device="meta"), time_encoder=(tab(4, 1), f32(4, "meta"))),
     ValueError, "edge_feats is on meta, nodes on"),
    (seq, dict(time_encoder=(tab(4, 1), f32(4, "meta")), since=f32(4, "meta")), ValueError,
     "time_encoder's bias is on meta, nodes on"),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_the_earlier_check_wins(case):
    checker, faults, exc, message = CASES[case]
    with pytest.raises(exc, match="^" + message):
        checker(**faults)


def test_each_fault_alone_is_an_error_too():
    """A case pins an order only if its second fault would have been reported: every argument a
    case breaks is an error on its own (cases whose faults need each other, such as 2**31 rows in
    every tensor, are left whole)."""
    for checker, faults, _, _ in CASES:
        sizes = {int(v.numel()) for v in faults.values() if isinstance(v, torch.Tensor)}
        if BIG in sizes or 2 ** 15 in sizes:
            continue
        for name, value in faults.items():
            with pytest.raises((TypeError, ValueError)):
                checker(**{name: value})


def test_numpy_integers_where_they_are_taken():
    """common_neighbors and the walks take numpy integers for their bounds; seen_mask and
    pair_history do not (cases above)."""
    assert common(max_history=np.int64(5), max_common=np.int32(2)) == (4, 5, 2)
    assert walk(length=np.int64(3), num_walks=np.int32(2)) == (4, 2, 3)
