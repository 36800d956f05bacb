"""CPU: ops.patch_project / ops.patch_project_time refuse bad arguments in Python, before native
code is touched (every tensor here is on the CPU, so a call that passed its checks would end in
"runs on the GPU"), and DyGFormer(fused_patches=True) holds the same state."""
import pytest
import torch

from gnnflow_amd import ops
from gnnflow_amd.models import DyGFormer

L, P, D, C, ROWS = 8, 2, 4, 5, 7


def _table_args(**over):
    a = dict(ids=torch.zeros(3, 2, L, dtype=torch.int64),
             lengths=torch.zeros(3, 2, dtype=torch.int32), table=torch.zeros(ROWS, D),
             weight=torch.zeros(C, P * D), bias=torch.zeros(C), patch_size=P)
    a.update(over)
    return a


def _time_args(**over):
    a = dict(delta_t=torch.zeros(3, 2, L), lengths=None, time_weight=torch.zeros(D, 1),
             time_bias=torch.zeros(D), weight=torch.zeros(C, P * D), bias=torch.zeros(C),
             patch_size=P)
    a.update(over)
    return a


TABLE_CASES = [
    (dict(ids=[1, 2]), TypeError, "ids must be a tensor"),
    (dict(ids=torch.zeros(3, 2, L, dtype=torch.int32)), TypeError, "ids must be torch.int64"),
    (dict(lengths=torch.zeros(3, 2, dtype=torch.int64)), TypeError, "lengths must be int32"),
    (dict(table=torch.zeros(ROWS, D, dtype=torch.bfloat16)), TypeError, "table is"),
    (dict(weight=torch.zeros(C, P * D, dtype=torch.float16)), TypeError, "weight is"),
    (dict(bias=torch.zeros(C, dtype=torch.float64)), TypeError, "bias is"),
    (dict(patch_size=2.0), TypeError, "patch_size must be an int"),
    (dict(table=torch.zeros(ROWS)), ValueError, r"table must be \[rows, d\]"),
    (dict(table=torch.zeros(ROWS, 2 * D)[:, ::2]), ValueError, "contiguous"),
    (dict(lengths=torch.zeros(3, dtype=torch.int32)), ValueError, "lengths must be"),
    (dict(table=torch.zeros(ROWS, 1025), weight=torch.zeros(C, 2050)), ValueError, "1 to 1024"),
    (dict(table=torch.zeros(ROWS, 0), weight=torch.zeros(C, 0)), ValueError, "1 to 1024"),
    (dict(ids=torch.zeros(3, 513, dtype=torch.int64), lengths=None), ValueError, "1 to 512"),
    (dict(patch_size=3), ValueError, "not a multiple of patch_size 3"),
    (dict(patch_size=0), ValueError, "not a multiple of patch_size 0"),
    (dict(table=torch.zeros(ROWS, 1024), patch_size=8, weight=torch.zeros(C, 8192)), ValueError,
     "up to 4096"),
    (dict(weight=torch.zeros(C, P * D + 1)), ValueError, r"weight must be \[C, patch_size \* d\]"),
    (dict(weight=torch.zeros(129, P * D), bias=torch.zeros(129)), ValueError, "1 to 128"),
    (dict(bias=torch.zeros(C + 1)), ValueError, r"bias must be \[5\]"),
    (dict(ids=torch.zeros(1, dtype=torch.int64).expand(2 ** 31, 1), lengths=None, patch_size=1,
          weight=torch.zeros(C, D)), ValueError, "fewer than 2\\*\\*31 patches"),
    (dict(), ValueError, "runs on the GPU"),
]

TIME_CASES = [
    (dict(delta_t=torch.zeros(3, 2, L, dtype=torch.float64)), TypeError, "delta_t must be"),
    (dict(time_weight=torch.zeros(D, 1, dtype=torch.float64)), TypeError, "time_weight is"),
    (dict(time_bias=torch.zeros(D, 1)), ValueError, r"time_bias must be \[dT\]"),
    (dict(time_weight=torch.zeros(1, D)), ValueError, "time_weight must be"),
    (dict(lengths=torch.zeros(3, 2)), TypeError, "lengths must be int32"),
    (dict(), ValueError, "runs on the GPU"),
]


@pytest.mark.parametrize("over,exc,match", TABLE_CASES)
def test_patch_project_checks(over, exc, match):
    with pytest.raises(exc, match=match):
        ops.patch_project(**_table_args(**over))


@pytest.mark.parametrize("over,exc,match", TIME_CASES)
def test_patch_project_time_checks(over, exc, match):
    with pytest.raises(exc, match=match):
        ops.patch_project_time(**_time_args(**over))


def test_the_flag_changes_no_state():
    kw = dict(dim_node=8, dim_edge=6, dim_time=10, channel_dim=12, patch_size=2, max_length=8)
    plain, fused = DyGFormer(**kw), DyGFormer(fused_patches=True, **kw)
    assert fused.fused_patches and not plain.fused_patches
    assert list(plain.state_dict()) == list(fused.state_dict())
    fused.load_state_dict(plain.state_dict())
    DyGFormer(fused_patches=False, **dict(kw, channel_dim=256))
    for over in (dict(channel_dim=256), dict(dim_node=2048), dict(dim_edge=1024, patch_size=8),
                 dict(max_length=1024)):
        with pytest.raises(ValueError, match="fused_patches takes"):
            DyGFormer(fused_patches=True, **dict(kw, **over))
    DyGFormer(fused_patches=True, learn_time=True, **dict(kw, dim_time=2048))
