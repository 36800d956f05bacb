"""Which error wins when two arguments of an edge-history reader are wrong at once.

The five checkers (dynamic_graph.check_seen_mask_args, check_pair_history_args,
check_common_neighbors_args, check_temporal_degree_args, check_temporal_walk_args) report their
errors in a fixed order, and callers see that order: the per-reader error tests pin every message,
this file pins the order.  Each case breaks two checks that are adjacent in a checker's order and
names the one reported; the expected winners were written from the checkers as they stood before
they were folded onto shared helpers.  CPU only: a tensor on `meta` stands for another device, and
a zero-stride view for 2**31 rows without their memory."""
import numpy as np
import pytest
import torch

from gnnflow_amd.dynamic_graph import (check_common_neighbors_args, check_pair_history_args,
                                       check_seen_mask_args, check_temporal_degree_args,
                                       check_temporal_walk_args)

BIG = 2 ** 31


def i64(n=4, device="cpu"):
    return torch.zeros(n, dtype=torch.int64, device=device)


def f32(n=4, device="cpu"):
    return torch.zeros(n, dtype=torch.float32, device=device)


def big(dtype, device="cpu"):
    return torch.zeros(1, dtype=dtype, device=device).expand(BIG)


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
