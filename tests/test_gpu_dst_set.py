"""DeviceDstSet on the GPU against np.unique (tests/batch_stream_ref.union): num_nodes at the
word edge (1, 64, 65), past one tile's 64-bit word count times 4 (4097 bits: the last thread of
a tile has words the bitmap does not) and past one compaction tile (65 536 bits: two tiles)."""
import numpy as np
import pytest

from tests import batch_stream_ref as R

pytestmark = pytest.mark.gpu

TILE_BITS = 1024 * 64


def _ids(s):
    import torch
    n = int(s.count.item())
    assert n == len(s)
    ids = s.ids[:n].cpu().numpy()
    assert ids.dtype == np.int64 and s.count.dtype == torch.int64 and tuple(s.count.shape) == (1,)
    assert np.array_equal(ids, s.to_numpy())
    return ids


@pytest.mark.parametrize("num_nodes", [1, 64, 65, 4097, TILE_BITS + 3])
def test_three_adds_equal_np_unique(num_nodes):
    import torch
    from gnnflow_amd import DeviceDstSet
    rng = np.random.RandomState(num_nodes)
    a = np.concatenate([rng.randint(0, num_nodes, 40), [0, num_nodes - 1]])      # both ends
    b = rng.randint(0, num_nodes, 300)                                            # overlaps a
    b[:20] = a[:20]
    s = DeviceDstSet(num_nodes, "cuda:0", a)
    assert np.array_equal(_ids(s), R.union(num_nodes, a)[0])
    s.add(torch.from_numpy(b).cuda())                    # a device tensor
    s.add(np.empty(0, np.int64))                         # an empty add changes nothing
    s.add(torch.empty(0, dtype=torch.int32))
    want, bad = R.union(num_nodes, a, b)
    got = _ids(s)
    assert np.array_equal(got, want) and bad == 0
    assert got[0] == 0 and got[-1] == num_nodes - 1
    assert s.upper_bound() >= len(want)
    s.check()
    s.add(a.astype(np.int32))                            # all there already
    assert np.array_equal(_ids(s), want)


def test_every_id_of_two_tiles():
    from gnnflow_amd import DeviceDstSet
    n = 2 * TILE_BITS
    s = DeviceDstSet(n, "cuda:0", np.arange(n))
    assert np.array_equal(_ids(s), np.arange(n))


def test_resize_keeps_members():
    from gnnflow_amd import DeviceDstSet
    s = DeviceDstSet(65, "cuda:0", [3, 64, 0, 3])
    s.resize(TILE_BITS + 100)
    assert s.num_nodes == TILE_BITS + 100
    assert _ids(s).tolist() == [0, 3, 64]
    s.add([TILE_BITS + 99, 70, 64])
    assert _ids(s).tolist() == [0, 3, 64, 70, TILE_BITS + 99]
    s.check()
    empty = DeviceDstSet(0, "cuda:0")
    assert len(empty) == 0 and int(empty.count.item()) == 0
    empty.resize(10)
    empty.add([9, 9])
    assert _ids(empty).tolist() == [9]


def test_check_reports_ids_out_of_range():
    from gnnflow_amd import DeviceDstSet
    s = DeviceDstSet(100, "cuda:0", [5, 6])
    s.check()
    s.add([7, 100, -1, 99, 1 << 40])
    assert _ids(s).tolist() == [5, 6, 7, 99]             # the in-range ids of that call are in
    with pytest.raises(ValueError, match=r"3 id\(s\) outside \[0, 100\)"):
        s.check()


@pytest.mark.parametrize("size", [0, 1, 5, 257, 600])
def test_sample_matches_reference(size):
    from gnnflow_amd import DeviceDstSet
    members = np.array([2, 3, 5, 7, 11, 13, 17])
    s = DeviceDstSet(64, "cuda:0", members)
    for first, call in ((0, 0), (3 * 10 ** 9, 1), ((1 << 64) - 3, (1 << 32) + 1)):
        got = s.sample(size, seed=99, first=first, call=call)
        assert got.is_cuda and got.dtype.is_floating_point is False and tuple(got.shape) == (size,)
        if size:
            assert np.array_equal(got.cpu().numpy(), R.sample(members, size, 99, first, call))
