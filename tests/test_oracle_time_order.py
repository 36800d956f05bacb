"""The oracle's rule for the timestamps where float bits and float `<` part ways, pinned
without a GPU: a batch is ordered by (source, timestamp under `<`, input position)
(oracle/gnnflow_oracle.c sortkey_cmp; the reference stable-sorts a source's edges by timestamp,
dynamic_graph.cu:105-128).  +0.0 and -0.0 tie under `<`, so they keep their input order and each
keeps its own sign bit; the denormals and +-FLT_MAX are ordinary values.  tests/
test_gpu_ingest_order.py holds the HIP store to exactly this on every ingest path."""
import numpy as np

from oracle import oracle as O

F = np.finfo(np.float32)
DEN = np.float32(F.smallest_subnormal)
PZ, NZ = np.float32(0.0), np.float32(-0.0)


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _one_source(ts):
    ts = np.asarray(ts, np.float32)
    n = len(ts)
    o = O.OracleGraph(minimum_block_size=4)
    o.add_edges(np.zeros(n, np.int64), np.arange(1, n + 1), ts, np.arange(100, 100 + n))
    return o.get_temporal_neighbors(0)


def test_signed_zeros_tie_and_keep_input_order_and_sign():
    for first, second in ((PZ, NZ), (NZ, PZ)):
        # position:  0     1      2       3      4
        ts = [np.float32(1.0), first, np.float32(-1.0), second, first]
        dst, t, eid = _one_source(ts)
        # the reference reports a node's edges newest first
        assert eid.tolist() == [100, 104, 103, 101, 102]
        assert dst.tolist() == [1, 5, 4, 2, 3]
        assert _bits(t).tolist() == _bits([1.0, first, second, first, -1.0]).tolist()
    assert _bits(PZ) != _bits(NZ)


def test_denormals_and_flt_max_are_ordered_by_less_than():
    ts = np.array([F.max, DEN, NZ, -F.max, -DEN, PZ, 1.0, -1.0, DEN, -F.max], np.float32)
    dst, t, eid = _one_source(ts)
    # -FLT_MAX < -1 < -denormal < the zeros < denormal < 1 < FLT_MAX, ties by input position
    asc = [3, 9, 7, 4, 2, 5, 1, 8, 6, 0]
    assert asc == sorted(range(len(ts)), key=lambda i: (float(ts[i]), i))
    assert eid.tolist() == [100 + i for i in reversed(asc)]          # reported newest first
    assert dst.tolist() == [1 + i for i in reversed(asc)]
    assert _bits(t).tolist() == _bits(ts[asc[::-1]]).tolist()


def test_a_second_batch_at_the_other_zero_is_not_older():
    """The stored newest edge at +0.0 admits a batch whose oldest edge is -0.0 (and the other
    way round): neither is `<` the other."""
    for first, second in ((PZ, NZ), (NZ, PZ)):
        o = O.OracleGraph(minimum_block_size=4)
        o.add_edges(np.array([0, 0]), np.array([1, 2]), np.array([-1.0, first], np.float32),
                    np.array([0, 1]))
        o.add_edges(np.array([0]), np.array([3]), np.array([second], np.float32), np.array([2]))
        dst, t, eid = o.get_temporal_neighbors(0)
        assert eid.tolist() == [2, 1, 0]
        assert _bits(t).tolist() == _bits([second, first, -1.0]).tolist()
