"""walk_position_counts: the anonymous encoding of temporal walks (csrc/walk_positions.hip)."""
from typing import Optional

import torch

from ..dynamic_graph import WALK_MAX_LENGTH
from ._common import _check_on_gpu, _check_same_device, _check_tensors, _launch, _ptr

WALK_MAX_REF_ENTRIES = 4096          # GF_WALK_MAX_REF_ENTRIES: Wr * (Lr + 1), one row's set in LDS


def check_walk_position_counts_args(nodes, ref=None):
    """Arguments of walk_position_counts, checked before anything is launched or allocated.
    Needs no device.  Returns (B, W, L + 1, Wr, Lr + 1)."""
    for name, x in (("nodes", nodes), ("ref", ref)):
        if x is None and name == "ref":
            continue
        _check_tensors((name, x))      # everything about nodes before anything about ref
        if x.dtype != torch.int64:
            raise TypeError("{} must be torch.int64, got {}".format(name, x.dtype))
        if x.dim() != 3:
            raise ValueError("{} must be [rows, walks, length + 1], got shape {}".format(
                name, tuple(x.shape)))
        if not 1 <= int(x.shape[2]) <= WALK_MAX_LENGTH + 1:
            raise ValueError("{} must hold walks of 0 to {} steps (1 to {} nodes), got {} nodes"
                             .format(name, WALK_MAX_LENGTH, WALK_MAX_LENGTH + 1, int(x.shape[2])))
    B, W, L1 = (int(n) for n in nodes.shape)
    Br, Wr, Lr1 = (B, W, L1) if ref is None else (int(n) for n in ref.shape)
    if Br != B:
        raise ValueError("nodes has {} rows, ref has {}".format(B, Br))
    if Wr * Lr1 > WALK_MAX_REF_ENTRIES:
        raise ValueError("walk_position_counts counts in at most {} entries per row, got "
                         "{} x {}".format(WALK_MAX_REF_ENTRIES, Wr, Lr1))
    if B >= 2 ** 31:
        raise ValueError("walk_position_counts takes fewer than 2**31 rows, got {}".format(B))
    if W * L1 * Lr1 >= 2 ** 31:
        raise ValueError("walk_position_counts writes fewer than 2**31 counts per row, got "
                         "{} x {} x {}".format(W, L1, Lr1))
    _check_same_device("nodes", nodes, ("ref", ref))
    return B, W, L1, Wr, Lr1


def walk_position_counts(nodes: torch.Tensor, ref: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The position-count ("anonymous") encoding of temporal walks, CAWN's set-based
    anonymisation: an int32 tensor [B, W, L + 1, Lr + 1] with

        out[i, w, j, p] = #{w' < Wr : ref[i, w', p] == nodes[i, w, j]}   if nodes[i, w, j] >= 0
                          0                                              otherwise

    nodes: int64 [B, W, L + 1], the walks to encode (TemporalWalks.nodes); ref: int64
    [B, Wr, Lr + 1], the walks to count in, nodes itself when None.  With ref=None a node is
    encoded by how often it stands at each position of its own root's walks; for a link (u, v) a
    second call with the partner's walks as ref gives the counts relative to the other side.
    Negative entries (the slots of ended walks) encode to zeros and are never counted.  L and Lr
    are at most 32 and Wr * (Lr + 1) at most WALK_MAX_REF_ENTRIES; B == 0 or W == 0 returns an
    empty tensor without a launch.  The outputs are integers and carry no autograd.

    One kernel (csrc/walk_positions.hip) on the current stream, never synchronises: a workgroup
    per row holds ref[i] in LDS and compares every entry of nodes[i] with every entry of it,
    W (L + 1) * Wr (Lr + 1) compares per row."""
    B, W, L1, Wr, Lr1 = check_walk_position_counts_args(nodes, ref)
    dev = nodes.device
    _check_on_gpu("walk_position_counts", dev)
    n = nodes.detach().contiguous()
    r = n if ref is None else ref.detach().contiguous()
    out = torch.empty((B, W, L1, Lr1), dtype=torch.int32, device=dev)
    if B and W:
        _launch(dev, "gf_walk_position_counts", None, None,
                (n.data_ptr(), _ptr(r), B, W, L1, Wr, Lr1, out.data_ptr()))
    return out
