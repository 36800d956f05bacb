"""Every ValueError / TypeError of DeviceDstSet and DeviceBatchStream is raised before anything
touches the GPU: these pass on a machine without one."""
import numpy as np
import pandas as pd
import pytest

import gnnflow_amd
from gnnflow_amd.data import DeviceBatchStream, DeviceDstSet

DEV = "cuda:0"
SRC = np.arange(10, dtype=np.int64)
DST = np.arange(10, 20, dtype=np.int64)
TIME = np.arange(10, dtype=np.float32)
EID = np.arange(10, dtype=np.int64)


def nonempty(num_nodes=100):
    """A set that believes it was given ids, without the device state an add() would create."""
    s = DeviceDstSet(num_nodes, DEV)
    s._added = 5
    return s


def test_exported():
    assert {"DeviceDstSet", "DeviceBatchStream"} <= set(gnnflow_amd.__all__)
    assert gnnflow_amd.DeviceBatchStream is DeviceBatchStream


def test_negative_neg_ratio():
    with pytest.raises(ValueError, match="neg_ratio"):
        DeviceBatchStream(SRC, DST, TIME, EID, 4, nonempty(), neg_ratio=-1)
    with pytest.raises(TypeError, match="neg_ratio"):
        DeviceBatchStream(SRC, DST, TIME, EID, 4, nonempty(), neg_ratio=1.5)


def test_empty_destination_set():
    empty = DeviceDstSet(100, DEV)
    with pytest.raises(ValueError, match="empty destination set"):
        DeviceBatchStream(SRC, DST, TIME, EID, 4, empty, neg_ratio=1)
    with pytest.raises(ValueError, match="empty destination set"):
        empty.sample(3, seed=0)
    with pytest.raises(ValueError, match="destination set"):
        DeviceBatchStream(SRC, DST, TIME, EID, 4, None, neg_ratio=1, device=DEV)
    assert len(empty) == 0 and empty.to_numpy().shape == (0,)      # nothing allocated, no GPU
    empty.check()


def test_destination_set_too_large_to_draw_from():
    big = DeviceDstSet(1 << 33, DEV)
    big._added = 1 << 32
    with pytest.raises(ValueError, match=r"2\*\*32"):
        DeviceBatchStream(SRC, DST, TIME, EID, 4, big)
    with pytest.raises(ValueError, match=r"2\*\*32"):
        big.sample(3, seed=0)


def test_unequal_columns():
    for cols in ((SRC[:9], DST, TIME, EID), (SRC, DST[:9], TIME, EID), (SRC, DST, TIME[:9], EID),
                 (SRC, DST, TIME, EID[:9])):
        with pytest.raises(ValueError, match="differ in length"):
            DeviceBatchStream(*cols, 4, nonempty())
    with pytest.raises(ValueError, match="one-dimensional"):
        DeviceBatchStream(SRC.reshape(2, 5), DST, TIME, EID, 4, nonempty())


@pytest.mark.parametrize("batch_size", [0, -3])
def test_batch_size_not_positive(batch_size):
    with pytest.raises(ValueError, match="batch_size"):
        DeviceBatchStream(SRC, DST, TIME, EID, batch_size, nonempty())
    df = pd.DataFrame({"src": SRC, "dst": DST, "time": TIME, "eid": EID})
    with pytest.raises(ValueError, match="batch_size"):
        DeviceBatchStream.from_dataframe(df, batch_size, nonempty())


@pytest.mark.parametrize("seed", [-1, 1 << 64])
def test_seed_out_of_range(seed):
    with pytest.raises(ValueError, match="seed"):
        DeviceBatchStream(SRC, DST, TIME, EID, 4, nonempty(), seed=seed)
    with pytest.raises(ValueError, match="seed"):
        nonempty().sample(3, seed=seed)
    with pytest.raises(ValueError, match="first_row"):
        DeviceBatchStream(SRC, DST, TIME, EID, 4, nonempty(), first_row=seed)


def test_non_integer_ids():
    for cols in ((SRC.astype(np.float64), DST, TIME, EID), (SRC, DST.astype(np.float32), TIME, EID),
                 (SRC, DST, TIME, EID.astype(np.float64))):
        with pytest.raises(TypeError, match="integers"):
            DeviceBatchStream(*cols, 4, nonempty())
    with pytest.raises(TypeError, match="integers"):
        DeviceDstSet(100, DEV, dst=np.array([1.0, 2.0]))
    with pytest.raises(TypeError, match="integers"):
        DeviceDstSet(100, DEV).add(np.array([True, False]))
    with pytest.raises(TypeError, match="seed"):
        DeviceBatchStream(SRC, DST, TIME, EID, 4, nonempty(), seed=1.0)


def test_borders_must_ascend_inside_the_stream():
    for borders in ([0, 5, 4, 10], [0, 11], [-1, 10]):
        with pytest.raises(ValueError, match="borders"):
            DeviceBatchStream(SRC, DST, TIME, EID, 4, nonempty(), borders=borders)
    with pytest.raises(TypeError, match="borders"):
        DeviceBatchStream(SRC, DST, TIME, EID, 4, nonempty(), borders=[0.0, 10.0])


def test_frame_whose_index_does_not_ascend():
    index = np.arange(10)
    index[[2, 7]] = index[[7, 2]]      # batches of 4 by index // 4 are no longer row ranges
    df = pd.DataFrame({"src": SRC, "dst": DST, "time": TIME, "eid": EID}, index=index)
    with pytest.raises(ValueError, match="contiguous"):
        DeviceBatchStream.from_dataframe(df, 4, nonempty())


def test_set_arguments():
    with pytest.raises(ValueError, match="num_nodes"):
        DeviceDstSet(-1, DEV)
    with pytest.raises(ValueError, match="num_nodes"):
        DeviceDstSet(1 << 40, DEV)
    with pytest.raises(ValueError, match="GPU"):
        DeviceDstSet(10, "cpu")
    with pytest.raises(ValueError, match="shrink"):
        DeviceDstSet(10, DEV).resize(5)
    with pytest.raises(ValueError, match="size"):
        nonempty().sample(-1, seed=0)
    s = DeviceDstSet(10, DEV)
    s.resize(1000)                     # nothing allocated yet: just a number
    assert s.num_nodes == 1000 and s.upper_bound() == 0
