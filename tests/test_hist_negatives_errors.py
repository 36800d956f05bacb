"""The ValueError / TypeError cases of DeviceBatchStream(graph=, hist_ratio=) are raised before
anything touches the GPU, and gf_batch_hist_negatives rejects a null graph with a status code and
a message: these pass on a machine without a GPU."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

from gnnflow_amd import _capi
from gnnflow_amd.data import DeviceBatchStream, DeviceDstSet

DEV = "cuda:0"
SRC = np.arange(10, dtype=np.int64)
DST = np.arange(10, 20, dtype=np.int64)
TIME = np.arange(10, dtype=np.float32)
EID = np.arange(10, dtype=np.int64)


def nonempty(device=DEV):
    """A set that believes it was given ids, without the device state an add() would create."""
    s = DeviceDstSet(100, device)
    s._added = 5
    return s


class GraphOn:
    """What DeviceBatchStream looks at in a DynamicGraph before it uses the GPU: the handle
    attribute and the device number.  (A real graph allocates on the device when it is made.)"""

    def __init__(self, device):
        self._h = C.c_void_p()
        self.device = device


@pytest.mark.parametrize("hist_ratio", [1.0, 1.5, "1", True, None])
def test_hist_ratio_must_be_an_integer(hist_ratio):
    with pytest.raises(TypeError, match="hist_ratio"):
        DeviceBatchStream(SRC, DST, TIME, EID, 4, nonempty(), neg_ratio=2, graph=GraphOn(0),
                          hist_ratio=hist_ratio)


def test_hist_ratio_range():
    with pytest.raises(ValueError, match="hist_ratio"):
        DeviceBatchStream(SRC, DST, TIME, EID, 4, nonempty(), neg_ratio=2, graph=GraphOn(0),
                          hist_ratio=-1)
    with pytest.raises(ValueError, match="hist_ratio"):
        DeviceBatchStream(SRC, DST, TIME, EID, 4, nonempty(), neg_ratio=2, graph=GraphOn(0),
                          hist_ratio=3)
    with pytest.raises(ValueError, match="hist_ratio"):
        DeviceBatchStream(SRC, DST, TIME, EID, 4, None, neg_ratio=0, graph=GraphOn(0),
                          hist_ratio=1, device=DEV)
    with pytest.raises(ValueError, match="hist_ratio"):      # numpy integers are integers
        DeviceBatchStream(SRC, DST, TIME, EID, 4, nonempty(), neg_ratio=np.int64(2),
                          graph=GraphOn(0), hist_ratio=np.int32(3))


def test_hist_ratio_needs_a_graph():
    with pytest.raises(ValueError, match="graph"):
        DeviceBatchStream(SRC, DST, TIME, EID, 4, nonempty(), neg_ratio=2, hist_ratio=1)
    df = pd.DataFrame({"src": SRC, "dst": DST, "time": TIME, "eid": EID})
    with pytest.raises(ValueError, match="graph"):
        DeviceBatchStream.from_dataframe(df, 4, nonempty(), neg_ratio=2, hist_ratio=2)


def test_graph_must_be_a_graph():
    for graph in (5, "graph", object(), np.zeros(3)):
        with pytest.raises(TypeError, match="DynamicGraph"):
            DeviceBatchStream(SRC, DST, TIME, EID, 4, nonempty(), neg_ratio=2, graph=graph,
                              hist_ratio=1)


def test_graph_on_another_device():
    with pytest.raises(ValueError, match="device"):
        DeviceBatchStream(SRC, DST, TIME, EID, 4, nonempty("cuda:0"), neg_ratio=2,
                          graph=GraphOn(1), hist_ratio=1)
    with pytest.raises(ValueError, match="device"):
        DeviceBatchStream(SRC, DST, TIME, EID, 4, nonempty("cuda:1"), neg_ratio=2,
                          graph=GraphOn(0), hist_ratio=2)
    df = pd.DataFrame({"src": SRC, "dst": DST, "time": TIME, "eid": EID})
    with pytest.raises(ValueError, match="device"):
        DeviceBatchStream.from_dataframe(df, 4, nonempty("cuda:1"), neg_ratio=1, graph=GraphOn(0),
                                         hist_ratio=1)


def test_null_graph_is_an_invalid_argument():
    lib = _capi.load()
    rc = lib.gf_batch_hist_negatives(None, None, None, None, 0, None, 1, 0, 2, 1, 0, 0, 0, None, 0,
                                     None, 0, None)
    assert rc == _capi.GF_ERR_INVALID_ARGUMENT
    assert b"null graph" in lib.gf_last_error()
    # also when nothing would be launched: the handle is looked at first
    rc = lib.gf_batch_hist_negatives(None, None, None, None, 0, None, 0, 0, 0, 0, 0, 0, 0, None, 0,
                                     None, 0, None)
    assert rc == _capi.GF_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError, match="null graph"):
        _capi.check(rc)
