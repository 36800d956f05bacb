"""ops.walk_position_counts (csrc/walk_positions.hip) on the GPU against
tests/temporal_walk_ref.position_counts, bit for bit.

The walks are the reference's own over the toy graph of tests/test_gpu_temporal_walk.py with
reverse edges (so the kernel under test is this one alone): 167 roots of which seven go nowhere,
with ended slots in most rows and nodes that repeat inside and across the walks of a root."""
import numpy as np
import pytest
import torch

from gnnflow_amd import ops
from tests import temporal_walk_ref as T
from tests.test_gpu_temporal_walk import _edges, _queries

pytestmark = pytest.mark.gpu


class Walks:
    pass


@pytest.fixture(scope="module")
def walks():
    w = Walks()
    hist, table_len = T.from_edges(*_edges(), add_reverse=True)
    src, ts = _queries()
    # (W, L) = (70, 2): above one wave of entries per walk set; (9, 4): another Wr and Lr
    w.a = T.walks(hist, table_len, src, ts, 2, 70, 2, 0, seed=21)[0]
    w.b = T.walks(hist, table_len, src, ts, 4, 9, 1, 5, seed=22)[0]
    w.d_a, w.d_b = torch.from_numpy(w.a).cuda(), torch.from_numpy(w.b).cuda()
    return w


def _check(nodes, ref=None):
    """nodes, ref: numpy.  The op's output on the device against the restatement."""
    d_nodes = torch.from_numpy(nodes).cuda()
    d_ref = None if ref is None else torch.from_numpy(ref).cuda()
    out = ops.walk_position_counts(d_nodes, d_ref)
    lr1 = (nodes if ref is None else ref).shape[2]
    assert out.dtype == torch.int32 and out.is_cuda and out.is_contiguous()
    assert tuple(out.shape) == tuple(nodes.shape) + (lr1,) and not out.requires_grad
    got = out.cpu().numpy()
    assert np.array_equal(got, T.position_counts(nodes, ref))
    return got


def test_the_walks_exercise_every_case(walks):
    """From the reference alone: ended slots, rows of ended walks only, nodes that repeat."""
    a, b = walks.a, walks.b
    assert a.shape == (167, 70, 3) and b.shape == (167, 9, 5)
    assert (a[-7:, :, 1:] == -1).all() and (a[:, :, 1:] == -1).any(axis=(1, 2)).sum() > 7
    assert (a[:, :, 2] >= 0).any() and (b[:, :, 4] >= 0).any()
    own = T.position_counts(a)
    assert own.max() > 8 and (own[a < 0] == 0).all()
    known = a[:, 0, 0] >= 0                                # all but the sources -3 and -1
    assert known.sum() == 165
    assert (own[known, :, 0, 0] == 70).all()               # the root stands first in all its walks
    other = T.position_counts(a, b)
    assert other.shape == (167, 70, 3, 5) and (other[known, :, 0, 0] == 9).all()
    assert (other[:, :, 1:, 1:] > 1).any()                 # and nodes met on the way repeat


def test_counts_in_the_walks_themselves(walks):
    got = _check(walks.a)
    assert got.sum() > 0
    _check(walks.b)


def test_counts_in_a_partner_set_of_other_sizes(walks):
    _check(walks.a, walks.b)
    _check(walks.b, walks.a)
    # the same tensor passed as ref is ref=None
    assert torch.equal(ops.walk_position_counts(walks.d_a, walks.d_a),
                       ops.walk_position_counts(walks.d_a))


def test_one_row_and_a_row_of_ended_walks(walks):
    hub = 3 * 40
    _check(walks.a[hub:hub + 1])
    _check(walks.a[hub:hub + 1], walks.b[hub:hub + 1])
    ended = walks.a[-5:]                                   # sources the table does not hold
    assert (ended[:, :, 1:] == -1).all()
    got = _check(ended)
    assert (got[:, :, 1:] == 0).all() and (got[:2] == 0).all()       # -3 and -1 count nothing
    assert (got[2:, :, 0, 0] == 70).all()                  # 2^40 is an id like any other
    got = _check(walks.a[:3], np.full((3, 4, 2), -1, np.int64))
    assert (got == 0).all()


def test_a_reference_set_of_exactly_4096_entries(walks):
    rng = np.random.RandomState(7)
    for wr, lr1 in ((4096, 1), (128, 32), (124, 33)):
        assert wr * lr1 <= 4096
        ref = rng.randint(-1, 12, (2, wr, lr1)).astype(np.int64)
        nodes = rng.randint(-2, 14, (2, 5, 33)).astype(np.int64)
        nodes[0, 0, 0], ref[0, -1, -1], ref[0, -2, -1] = 11, 11, 11      # the set's last entry counts
        got = _check(nodes, ref)
        assert got[0, 0, 0, lr1 - 1] >= 2
    with pytest.raises(ValueError, match="4096"):
        ops.walk_position_counts(walks.d_a[:, :5], torch.zeros((167, 4097, 1), dtype=torch.int64,
                                                               device="cuda"))


def test_empty_inputs_views_and_a_side_stream(walks):
    out = ops.walk_position_counts(walks.d_a[:0], walks.d_b[:0])
    assert tuple(out.shape) == (0, 70, 3, 5) and out.dtype == torch.int32
    out = ops.walk_position_counts(walks.d_a[:, :0], walks.d_b)
    assert tuple(out.shape) == (167, 0, 3, 5)
    whole = ops.walk_position_counts(walks.d_a, walks.d_b)
    # rows are independent; a strided view is taken for what it holds
    assert torch.equal(ops.walk_position_counts(walks.d_a[::2], walks.d_b[::2]), whole[::2])
    assert torch.equal(ops.walk_position_counts(walks.d_a[:, :, :2], walks.d_b), whole[:, :, :2])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = ops.walk_position_counts(walks.d_a, walks.d_b)
    side.synchronize()
    assert torch.equal(again, whole)


def test_rows_past_the_grid_limit_are_grid_strided(walks):
    """The launch has at most 4096 workgroups, one row each: more rows than that, the walks
    repeated, so that the expected rows are the reference's rows repeated."""
    rows = 4096 + 37
    idx = torch.arange(rows, device="cuda") % 167
    got = ops.walk_position_counts(walks.d_a[idx, :6], walks.d_b[idx])
    want = T.position_counts(walks.a[:, :6], walks.b)
    assert np.array_equal(got.cpu().numpy(), want[idx.cpu().numpy()])


def test_temporal_walks_example():
    """examples/temporal_walks.py on a small graph: the shapes it prints, and its encodings are
    the restatement's of its walks."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "temporal_walks_example", os.path.join(root, "examples", "temporal_walks.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    r, wu, wv, enc = example.main(batch_size=40, num_walks=6, length=3, num_edges=4000,
                                  verbose=False)
    assert r["nodes"] == (40, 6, 4) and r["eids"] == r["times"] == (40, 6, 3)
    assert r["encoding"] == (40, 6, 4, 4) and 0 < r["mean_steps"] <= 3
    u, v = wu.nodes.cpu().numpy(), wv.nodes.cpu().numpy()
    assert np.array_equal(enc["u|u"].cpu().numpy(), T.position_counts(u))
    assert np.array_equal(enc["u|v"].cpu().numpy(), T.position_counts(u, v))
    assert np.array_equal(enc["v|u"].cpu().numpy(), T.position_counts(v, u))
    t, taken = wu.times.cpu().numpy(), wu.eids.cpu().numpy() >= 0
    assert (t[:, :, 1:] < t[:, :, :-1])[taken[:, :, 1:]].all()      # time strictly decreases
