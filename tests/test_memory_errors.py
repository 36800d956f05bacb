"""Shape rules of gnnflow_amd.memory that need no device: check_update_shapes / check_ids refuse
every shape the kernels would read past (they take raw pointers), with the offending shape in the
message, and Memory calls them before it touches its epoch or the native library."""
import pytest
import torch

from gnnflow_amd import memory as M

DM, DE = 5, 3


def _args(n=12, B=4, nid=None, mem=None, ts=None, ef="default", neg=1):
    nid = torch.zeros(n, dtype=torch.int64) if nid is None else nid
    mem = torch.zeros(n, DM) if mem is None else mem
    ts = torch.zeros(n) if ts is None else ts
    ef = torch.zeros(B, DE) if isinstance(ef, str) else ef
    return (DM, DE, nid, mem, ts, ef, neg)


def test_passing_cases():
    assert M.check_update_shapes(*_args()) == (12, 4)
    assert M.check_update_shapes(*_args(ef=None)) == (12, 4)
    assert M.check_update_shapes(*_args(n=8, B=4, neg=0)) == (8, 4)
    assert M.check_update_shapes(*_args(n=20, B=4, neg=3)) == (20, 4)
    assert M.check_update_shapes(*_args(n=0, B=0)) == (0, 0)
    # what Memory converts itself: other integer ids, other float types, strided views
    assert M.check_update_shapes(*_args(nid=torch.zeros(12, dtype=torch.int32),
                                        mem=torch.zeros(12, 9, dtype=torch.float64)[:, 2:7],
                                        ts=torch.zeros(24, dtype=torch.float64)[::2])) == (12, 4)
    assert M.check_update_shapes(DM, 0, torch.zeros(4, dtype=torch.int64), torch.zeros(4, DM),
                                 torch.zeros(4), torch.zeros(2, 0), 0) == (4, 2)
    for dt in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        M.check_ids(torch.zeros(7, dtype=dt))
    M.check_ids(torch.zeros(0, dtype=torch.int64))


def test_nid_is_1d_and_integer():
    with pytest.raises(ValueError, match=r"last_updated_nid must be 1-D, got shape \(6, 2\)"):
        M.check_update_shapes(*_args(nid=torch.zeros(6, 2, dtype=torch.int64)))
    with pytest.raises(ValueError, match=r"last_updated_nid must be 1-D, got shape \(\)"):
        M.check_update_shapes(*_args(nid=torch.zeros((), dtype=torch.int64)))
    for dt in (torch.float32, torch.float64, torch.bool):
        with pytest.raises(ValueError, match="last_updated_nid must have an integer dtype"):
            M.check_update_shapes(*_args(nid=torch.zeros(12, dtype=dt)))
    with pytest.raises(TypeError, match="last_updated_nid must be a tensor"):
        M.check_update_shapes(*_args(nid=[0] * 12))


def test_neg_sample_ratio():
    with pytest.raises(ValueError, match="neg_sample_ratio must be >= 0, got -1"):
        M.check_update_shapes(*_args(neg=-1))
    with pytest.raises(TypeError):
        M.check_update_shapes(*_args(neg=1.0))
    # tensor_split + cat of the reference fails when the ids do not split evenly
    with pytest.raises(ValueError, match=r"has 13 ids, not a multiple of 2 \+ neg_sample_ratio = 3"):
        M.check_update_shapes(*_args(n=13))
    with pytest.raises(ValueError, match="has 12 ids, not a multiple"):
        M.check_update_shapes(*_args(neg=3))
    with pytest.raises(ValueError, match="has 1 ids, not a multiple"):
        M.check_update_shapes(*_args(n=1, B=0, neg=0))


def test_memory_shape():
    for shape in ((11, DM), (13, DM), (12, DM - 1), (12, DM + 1), (12 * DM,), (12, DM, 1), (0, DM)):
        with pytest.raises(ValueError, match=r"last_updated_memory must be \[12, 5\], got shape "
                           + r"\(" + ", ".join(str(s) for s in shape)):
            M.check_update_shapes(*_args(mem=torch.zeros(shape)))
    with pytest.raises(TypeError, match="last_updated_memory must be a tensor"):
        M.check_update_shapes(*_args(mem=[[0.0] * DM] * 12))


def test_ts_shape():
    for shape in ((11,), (13,), (12, 1), (1, 12), ()):
        with pytest.raises(ValueError, match=r"last_updated_ts must be \[12\], got shape"):
            M.check_update_shapes(*_args(ts=torch.zeros(shape)))
    with pytest.raises(TypeError, match="last_updated_ts must be a tensor"):
        M.check_update_shapes(*_args(ts=0.0))


def test_edge_feats_shape():
    for shape in ((3, DE), (5, DE), (12, DE), (4, DE - 1), (4, DE + 1), (4 * DE,), (4, DE, 1)):
        with pytest.raises(ValueError, match=r"edge_feats must be \[4, 3\] or None, got shape"):
            M.check_update_shapes(*_args(ef=torch.zeros(shape)))
    with pytest.raises(ValueError, match=r"edge_feats must be \[2, 0\] or None, got shape \(2, 1\)"):
        M.check_update_shapes(DM, 0, torch.zeros(4, dtype=torch.int64), torch.zeros(4, DM),
                              torch.zeros(4), torch.zeros(2, 1), 0)
    with pytest.raises(TypeError, match="edge_feats must be a tensor or None"):
        M.check_update_shapes(*_args(ef=[[0.0] * DE] * 4))


def test_query_ids():
    with pytest.raises(ValueError, match=r"ids must be 1-D, got shape \(3, 1\)"):
        M.check_ids(torch.zeros(3, 1, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"ids must be 1-D, got shape \(\)"):
        M.check_ids(torch.zeros((), dtype=torch.int64))
    for dt in (torch.float32, torch.bool):
        with pytest.raises(ValueError, match="ids must have an integer dtype, got torch"):
            M.check_ids(torch.zeros(3, dtype=dt))
    with pytest.raises(TypeError, match="ids must be a tensor"):
        M.check_ids([1, 2])


class _Blk:
    def __init__(self, ids):
        self.srcdata = {"ID": ids}


def test_memory_checks_before_it_touches_anything():
    """A Memory whose tables and library were never made (no device here): a refused call must
    not get as far as needing them, and leaves the epoch alone."""
    m = M.Memory.__new__(M.Memory)
    m.dim_memory, m.dim_edge, m._epoch = DM, DE, 41
    _, _, nid, mem, ts, ef, _ = _args()
    with pytest.raises(ValueError, match=r"edge_feats must be \[4, 3\]"):
        m.update_mem_mail(nid, mem, ts, torch.zeros(5, DE))
    with pytest.raises(ValueError, match="last_updated_memory must be"):
        m.update_mem_mail(nid, mem[:, :4], ts, ef)
    with pytest.raises(ValueError, match="last_updated_ts must be"):
        m.update_mem_mail(nid, mem, ts[:11], ef)
    with pytest.raises(ValueError, match="not a multiple"):
        m.update_mem_mail(nid, mem, ts, ef, neg_sample_ratio=3)
    with pytest.raises(ValueError, match="neg_sample_ratio must be >= 0"):
        m.update_mem_mail(nid, mem, ts, ef, neg_sample_ratio=-2)
    with pytest.raises(ValueError, match="ids must be 1-D"):
        m.prepare_input(_Blk(torch.zeros(3, 2, dtype=torch.int64)))
    assert m._epoch == 41
    assert m.update_mem_mail(nid[:0], mem[:0], ts[:0], ef[:0]) is None      # nothing to do
    assert m._epoch == 41
