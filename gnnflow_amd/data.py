"""Datasets and batch samplers in front of the sampler, same classes and
arguments as gnnflow/data.py: `EdgePredictionDataset`, `RandomStartBatchSampler`,
`DistributedBatchSampler`, `default_collate_ndarray`.

Used the way scripts/offline_edge_prediction.py:190-229 does: the batch sampler yields lists
of row positions, `DataLoader(dataset, sampler=batch_sampler, collate_fn=
default_collate_ndarray)` hands each list to `dataset[list]`, which returns the batch's
(roots, ts, eid) in the layout `TemporalSampler.sample` takes.

`DeviceDstSet` and `DeviceBatchStream` are this project's own: the same batches with the edge
stream and the destination set in HBM, one kernel launch per batch (csrc/batch_stream.hip).
"""
import collections.abc
import ctypes as C
import os
import re
from typing import Iterable, Iterator, List, Optional, Union

import numpy as np
import torch
import torch.distributed
from torch.utils.data import BatchSampler, Dataset, Sampler

from . import _capi
from .utils import DstRandEdgeSampler


class EdgePredictionDataset(Dataset):
    """Positive edges of a dataframe (columns src, dst, time, eid) plus, with a negative
    sampler, one random destination per edge: item = (roots int64 [src|dst|neg],
    ts float32 [t|t|t], eid).  gnnflow/data.py:17-55."""

    def __init__(self, data, neg_sampler: Optional[DstRandEdgeSampler] = None):
        super(EdgePredictionDataset, self).__init__()
        self.data = data
        self.length = np.max(np.array(data['dst'], dtype=int))
        self.neg_sampler = neg_sampler

    def __getitem__(self, index):
        rows = self.data.iloc[index]
        src, dst, t = rows.src.values, rows.dst.values, rows.time.values
        parts = [src, dst]
        if self.neg_sampler is not None:
            parts.append(self.neg_sampler.sample(len(src)))
        roots = np.concatenate(parts).astype(np.int64)
        ts = np.concatenate([t] * len(parts)).astype(np.float32)
        return roots, ts, rows['eid'].values

    def __len__(self):
        return len(self.data)


def _chunked_batches(indices, first_size, batch_size, drop_last):
    """Lists of `batch_size` consecutive indices; when `first_size` > 0 the first list is
    that long instead (the random start of an epoch)."""
    want = first_size if first_size > 0 else batch_size
    batch = []
    for idx in indices:
        batch.append(idx)
        if len(batch) == want:
            yield batch
            batch, want = [], batch_size
    if batch and not drop_last:
        yield batch


def _local_device():
    if torch.cuda.is_available():
        return torch.device('cuda', int(os.environ.get("LOCAL_RANK", "0")))
    return torch.device('cpu')


class RandomStartBatchSampler(BatchSampler):
    """Sequential batches whose first one is cut to a random multiple of
    `batch_size // num_chunks` each epoch, so that successive epochs see differently aligned
    batches.  gnnflow/data.py:58-118."""

    def __init__(self, sampler: Union[Sampler[int], Iterable[int]], batch_size: int,
                 drop_last: bool, num_chunks: int = 1, world_size: int = 1):
        super(RandomStartBatchSampler, self).__init__(sampler, batch_size, drop_last)
        assert 0 < num_chunks < batch_size, "num_chunks must be in (0, batch_size)"
        self.num_chunks = num_chunks
        self.chunk_size = batch_size // num_chunks
        self.reorder = self.num_chunks > 1
        self.random_size = batch_size
        # the draw is broadcast with the process group's backend when there are several ranks
        self.device = _local_device() if world_size > 1 else torch.device('cpu')
        self.world_size = world_size

    def __iter__(self) -> Iterator[List[int]]:
        self.reset()
        first = self.random_size if self.reorder else 0
        for batch in _chunked_batches(self.sampler, first, self.batch_size, self.drop_last):
            self.reorder = False
            yield batch

    def reset(self):
        self.reorder = self.num_chunks > 1
        randint = torch.randint(0, self.num_chunks, size=(1,), device=self.device)
        if self.world_size > 1:
            torch.distributed.broadcast(randint, src=0)
        self.random_size = int(randint) * self.chunk_size
        if self.random_size == 0:
            self.reorder = False


class DistributedBatchSampler(BatchSampler):
    """Rank r takes the indices with `idx % world_size == r`, batched as above; rank 0 draws
    the random start and broadcasts it.  gnnflow/data.py:121-185."""

    def __init__(self, sampler: Union[Sampler[int], Iterable[int]], batch_size: int,
                 drop_last: bool, rank: int, world_size: int, num_chunks: int = 1):
        super(DistributedBatchSampler, self).__init__(sampler, batch_size, drop_last)
        self.rank = rank
        self.world_size = world_size
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        self.device = _local_device()
        assert 0 < num_chunks < batch_size, "num_chunks must be in (0, batch_size)"
        self.num_chunks = num_chunks
        self.chunk_size = batch_size // num_chunks
        self.reorder = False
        self.random_size = batch_size

    def __iter__(self) -> Iterator[List[int]]:
        self.reset()
        mine = (idx for idx in self.sampler if idx % self.world_size == self.rank)
        first = self.random_size if self.reorder else 0
        for batch in _chunked_batches(mine, first, self.batch_size, self.drop_last):
            self.reorder = False
            yield batch

    def reset(self):
        self.reorder = self.num_chunks > 1
        if not self.reorder:
            return
        if self.rank == 0:
            randint = torch.randint(0, self.num_chunks, size=(1,), device=self.device)
        else:
            randint = torch.zeros(1, dtype=torch.int64, device=self.device)
        torch.distributed.broadcast(randint, src=0)
        self.random_size = int(randint.item() * self.chunk_size)
        if self.random_size == 0:
            self.reorder = False


_STRING_OR_OBJECT = re.compile(r'[SaUO]')


def default_collate_ndarray(batch):
    """torch's default_collate with numpy outputs (gnnflow/data.py:193-293): arrays are
    stacked and flattened column-major (so a batch of one array is that array), numbers
    become arrays, strings stay lists, mappings / namedtuples / sequences recurse."""
    elem = batch[0]
    kind = type(elem)
    if isinstance(elem, np.ndarray):
        if kind.__name__ in ('ndarray', 'memmap') and \
                _STRING_OR_OBJECT.search(elem.dtype.str) is not None:
            raise TypeError("default_collate_ndarray: batch must contain tensors, numpy arrays, "
                            "numbers, dicts or lists; found {}".format(elem.dtype))
        return np.stack(batch, 0).flatten('F')
    if kind.__module__ == 'numpy' and kind.__name__ not in ('str_', 'string_'):
        if getattr(elem, 'shape', None) == ():
            return np.array(batch)
    if isinstance(elem, float):
        return np.array(batch, dtype=np.float64)
    if isinstance(elem, int):
        return np.array(batch)
    if isinstance(elem, (str, bytes)):
        return batch
    if isinstance(elem, collections.abc.Mapping):
        merged = {key: default_collate_ndarray([d[key] for d in batch]) for key in elem}
        try:
            return kind(merged)
        except TypeError:
            return merged
    if isinstance(elem, tuple) and hasattr(elem, '_fields'):
        return kind(*(default_collate_ndarray(samples) for samples in zip(*batch)))
    if isinstance(elem, collections.abc.Sequence):
        size = len(elem)
        if any(len(e) != size for e in batch):
            raise RuntimeError('each element in list of batch should be of equal size')
        columns = [default_collate_ndarray(samples) for samples in zip(*batch)]
        if isinstance(elem, tuple):
            return columns
        try:
            return kind(columns)
        except TypeError:
            return columns
    raise TypeError("default_collate_ndarray: batch must contain tensors, numpy arrays, numbers, "
                    "dicts or lists; found {}".format(kind))


# ---- device-resident batches (csrc/batch_stream.hip) -----------------------------------
_U64 = 1 << 64


def _u64(value, name):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise TypeError("{} must be an integer, got {}".format(name, type(value).__name__))
    value = int(value)
    if not 0 <= value < _U64:
        raise ValueError("{} must be in [0, 2**64), got {}".format(name, value))
    return value


def _count(value, name, least):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise TypeError("{} must be an integer, got {}".format(name, type(value).__name__))
    if int(value) < least:
        raise ValueError("{} must be at least {}, got {}".format(name, least, value))
    return int(value)


_INT_TENSORS = (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8)


def _id_column(x, name) -> torch.Tensor:
    """`x` (numpy, a pandas column or a tensor) as a 1-d contiguous int64 tensor where it is;
    TypeError for anything but integers — a float id is a bug upstream, not something to round."""
    if isinstance(x, torch.Tensor):
        if x.dtype not in _INT_TENSORS:
            raise TypeError("{} must hold integers, got {}".format(name, x.dtype))
        t = x
    else:
        a = np.asarray(x)
        if a.dtype.kind not in "iu":
            raise TypeError("{} must hold integers, got dtype {}".format(name, a.dtype))
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64))
    if t.dim() != 1:
        raise ValueError("{} must be one-dimensional, got shape {}".format(name, tuple(t.shape)))
    return t.to(torch.int64).contiguous()


def _time_column(x) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(
        np.ascontiguousarray(np.asarray(x), dtype=np.float32))
    if t.dim() != 1:
        raise ValueError("time must be one-dimensional, got shape {}".format(tuple(t.shape)))
    return t.to(torch.float32).contiguous()


def _cuda_device(device) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("a device-resident batch source needs a GPU device, got {}".format(device))
    return device


class _NoStream:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


class DeviceDstSet:
    """The distinct destination ids seen so far, on the device: the counterpart of
    `DstRandEdgeSampler.dst_list`.  A bitmap of `num_nodes` bits plus the ascending id list,
    kept equal to `np.unique(np.concatenate(everything added))`.

    `add` marks and recompacts on the current stream and never waits for the GPU; `ids` is the
    list's buffer (its first `count[0]` entries are the set, ascending) and `count` a device
    int64[1] — kernels that draw from the set read the length from there, so the host need not
    know it.  Only `__len__`, `to_numpy` and `check` synchronise.  Nothing is allocated before
    the first use.  Everything runs on the stream current at the call: order `add` against
    readers on other streams yourself."""

    def __init__(self, num_nodes: int, device, dst=None):
        self.num_nodes = self._checked_nodes(num_nodes)
        self.device = _cuda_device(device)
        self._bitmap = self._ids = self._count = self._oob = self._scratch = None
        self._added = 0          # ids handed to add(): an upper bound of len(self), known here
        if dst is not None:
            self.add(dst)

    @staticmethod
    def _checked_nodes(num_nodes):
        num_nodes = _count(num_nodes, "num_nodes", 0)
        if num_nodes >= 1 << 40:
            raise ValueError("num_nodes must be below 2**40, got {}".format(num_nodes))
        return num_nodes

    def upper_bound(self) -> int:
        """The most ids the set can hold now, without asking the GPU."""
        return min(self.num_nodes, self._added)

    # -- device state ---------------------------------------------------------------------
    def _words(self):
        return (self.num_nodes + 63) // 64

    def _alloc(self):
        if self._count is not None:
            return
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._lib = _capi.load()
        dev = self.device
        self._bitmap = torch.zeros(max(self._words(), 1), dtype=torch.int64, device=dev)
        self._count = torch.zeros(1, dtype=torch.int64, device=dev)
        self._oob = torch.zeros(1, dtype=torch.int64, device=dev)
        self._ids = torch.empty(0, dtype=torch.int64, device=dev)
        self._alloc_scratch()

    def _alloc_scratch(self):
        n = C.c_size_t(0)
        _capi.check(self._lib.gf_dst_set_scratch_bytes(self.num_nodes, C.byref(n)))
        self._scratch = torch.empty(max((n.value + 7) // 8, 1), dtype=torch.int64,
                                    device=self.device)

    @property
    def ids(self) -> torch.Tensor:
        """int64 buffer whose first `count[0]` entries are the set, ascending."""
        self._alloc()
        return self._ids

    @property
    def count(self) -> torch.Tensor:
        self._alloc()
        return self._count

    def add(self, dst):
        """Adds ids (numpy or a tensor on any device).  An id outside [0, num_nodes) is left out
        and counted; `check()` reports it."""
        col = _id_column(dst, "dst")
        n = int(col.shape[0])
        if n == 0:
            return
        self._alloc()
        col = col.to(self.device)
        stream = _capi.current_stream(self.device)
        with torch.cuda.device(self.device):
            _capi.check(self._lib.gf_dst_set_mark(
                col.data_ptr(), n, self._bitmap.data_ptr(), self.num_nodes, self._oob.data_ptr(),
                self.device.index, stream))
            self._added += n
            self._compact(stream)

    def _compact(self, stream):
        need = self.upper_bound()
        if self._ids.shape[0] < need:
            # rewritten in full below; queued readers of the old buffer are ahead on the stream
            self._ids = torch.empty(min(self.num_nodes, max(need, 2 * self._ids.shape[0])),
                                    dtype=torch.int64, device=self.device)
        _capi.check(self._lib.gf_dst_set_compact(
            self._bitmap.data_ptr(), self.num_nodes, self._ids.data_ptr(), self._ids.shape[0],
            self._count.data_ptr(), self._scratch.data_ptr(), self._scratch.shape[0] * 8,
            self.device.index, stream))

    def resize(self, num_nodes: int):
        """Makes room for ids below a larger `num_nodes`; the members stay."""
        num_nodes = self._checked_nodes(num_nodes)
        if num_nodes < self.num_nodes:
            raise ValueError("resize: cannot shrink from {} to {} nodes".format(
                self.num_nodes, num_nodes))
        old_words = self._words()
        self.num_nodes = num_nodes
        if self._count is None or num_nodes == 0:
            return
        if self._words() > self._bitmap.shape[0]:
            grown = torch.zeros(self._words(), dtype=torch.int64, device=self.device)
            grown[:old_words] = self._bitmap[:old_words]
            self._bitmap = grown
        self._alloc_scratch()

    def check(self):
        """Raises ValueError if any id handed to `add` was outside [0, num_nodes).  Waits for
        the GPU."""
        if self._oob is None:
            return
        bad = int(self._oob.item())
        if bad:
            raise ValueError("DeviceDstSet: {} id(s) outside [0, {}) were left out".format(
                bad, self.num_nodes))

    def __len__(self):
        return 0 if self._count is None else int(self._count.item())

    def to_numpy(self) -> np.ndarray:
        n = len(self)
        return self._ids[:n].cpu().numpy() if n else np.empty(0, np.int64)

    def sample(self, size: int, seed: int, first: int = 0, call: int = 0) -> torch.Tensor:
        """`size` uniform draws from the set as a device tensor:
        `ids[(philox(seed, first + i, call) * count) >> 32]`, the negatives of
        `DeviceBatchStream` with one negative per row (same kernel)."""
        size = _count(size, "size", 0)
        seed, first, call = _u64(seed, "seed"), _u64(first, "first"), _u64(call, "call")
        _check_drawable(self)
        self._alloc()
        out = torch.empty(size, dtype=torch.int64, device=self.device)
        if size:
            with torch.cuda.device(self.device):
                _capi.check(self._lib.gf_batch_assemble(
                    None, None, None, size, 0, size, 1, self._ids.data_ptr(),
                    self._count.data_ptr(), seed, call, first, out.data_ptr(), None,
                    self.device.index, _capi.current_stream(self.device)))
        return out


def _check_drawable(dst_set):
    bound = dst_set.upper_bound()
    if bound == 0:
        raise ValueError("negatives asked for from an empty destination set")
    if bound >= 1 << 32:
        raise ValueError("a destination set of 2**32 ids or more cannot be drawn from "
                         "(32-bit multiply-shift range reduction)")


class DeviceBatchStream:
    """`utils.get_batch` with the edge stream in HBM: batch i is `(roots, ts, eids)` as device
    tensors in get_batch's layout, produced by ONE kernel launch — no host-to-device copy, no
    host synchronisation, no host RNG.

        roots = [src | dst | neg_0 | ... | neg_{K-1}]   int64,   K = neg_ratio
        ts    = [t | t | ... ]                          float32, 2 + K copies
        eids  = eid[lo:hi]                              a view

    Negative k of the edge in row r of the stream is
    `dst_set.ids[(philox(seed, (first_row + r) * K + k, epoch) * len(dst_set)) >> 32]`
    (include/gnnflow_rng.h; `set_epoch` sets the call word).  The key is the edge's global row,
    so an edge draws the same negatives whatever the batch size or the random start, and ranks
    that pass the `first_row` of their slice draw what one process would have drawn for those
    rows, without talking to each other.  As in the reference a negative may equal the true
    destination.  The set's length is read on the device when the batch is assembled: ids added
    to `dst_set` (in stream order) are drawn from at once.  `neg_ratio=0` is `get_batch_no_neg`.

    `borders` are the row positions where batches begin plus the end (ascending, host
    integers); the default cuts every `batch_size` rows.  The columns are copied to the device
    once, here.

    `hist_ratio=Kh` (with `graph`, a `DynamicGraph` on the same device) makes the first Kh of
    the K negatives *historical*: a destination the source interacted with strictly before the
    edge's time that is not the true one, drawn with replacement from the source's live edges in
    the graph's temporal edge store (include/gnnflow_hip.h, gf_batch_hist_negatives; up to four
    attempts per slot under a seed tag of their own).  A second launch directly behind the
    assemble launch, same stream, overwrites those slots; a slot whose source has no earlier
    edge, is unknown to the graph, or drew the true destination four times keeps its random
    negative.  `hist_filled` is a device int64[1] that accumulates the number of slots
    overwritten (`reset_hist_filled()` zeroes it); divided by the slots asked for, rows x Kh, it
    is the share of historical negatives — read it once per pass.  Edges added to the graph are
    drawn from by batches launched after `add_edges` returns.  `add_edges` and
    `offload_old_blocks` move and free segments: synchronise the streams that batches were
    launched on before calling either, as for `TemporalSampler.sample`.  On a graph built with
    reverse edges the history includes nodes that pointed at the source."""

    def __init__(self, src, dst, time, eid, batch_size: int, dst_set: Optional[DeviceDstSet],
                 neg_ratio: int = 1, seed: int = 0, first_row: int = 0, borders=None,
                 device=None, graph=None, hist_ratio: int = 0):
        batch_size = _count(batch_size, "batch_size", 1)
        neg_ratio = _count(neg_ratio, "neg_ratio", 0)
        if neg_ratio >= 1 << 16:
            raise ValueError("neg_ratio must be below 65536, got {}".format(neg_ratio))
        hist_ratio = _count(hist_ratio, "hist_ratio", 0)
        if hist_ratio > neg_ratio:
            raise ValueError("hist_ratio must not exceed neg_ratio = {}, got {}".format(
                neg_ratio, hist_ratio))
        if graph is None:
            if hist_ratio:
                raise ValueError("hist_ratio > 0 needs the graph to draw the history from")
        elif not (hasattr(graph, "_h") and isinstance(getattr(graph, "device", None), int)):
            raise TypeError("graph must be a DynamicGraph, got {}".format(type(graph).__name__))
        seed, first_row = _u64(seed, "seed"), _u64(first_row, "first_row")
        src, dst, eid = _id_column(src, "src"), _id_column(dst, "dst"), _id_column(eid, "eid")
        time = _time_column(time)
        rows = int(src.shape[0])
        if not (dst.shape[0] == rows and time.shape[0] == rows and eid.shape[0] == rows):
            raise ValueError("src, dst, time and eid differ in length: {}, {}, {}, {}".format(
                rows, dst.shape[0], time.shape[0], eid.shape[0]))
        if neg_ratio:
            if dst_set is None:
                raise ValueError("neg_ratio > 0 needs a destination set")
            _check_drawable(dst_set)
        if dst_set is not None:
            if device is not None and torch.device(device) != dst_set.device:
                raise ValueError("device {} is not the destination set's {}".format(
                    device, dst_set.device))
            device = dst_set.device
        elif device is None:
            raise ValueError("without a destination set a device must be given")
        device = _cuda_device(device)
        self._check_graph_device(graph, device)
        if borders is None:
            borders = np.append(np.arange(0, rows, batch_size, dtype=np.int64), rows)
        else:
            b = np.asarray(borders)
            if b.dtype.kind not in "iu":
                raise TypeError("borders must hold integers, got dtype {}".format(b.dtype))
            borders = np.ascontiguousarray(b, dtype=np.int64)
            if borders.ndim != 1 or len(borders) < 1 or borders[0] < 0 or \
                    borders[-1] > rows or np.any(np.diff(borders) < 0):
                raise ValueError("borders must ascend within [0, {}]".format(rows))
        # ---- from here on the GPU is used ------------------------------------------------
        if dst_set is not None:
            dst_set._alloc()
            device = dst_set.device
        elif device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self._check_graph_device(graph, device)      # "cuda" without an index is known only now
        self._lib = _capi.load()
        self.device, self.dst_set = device, dst_set
        self.batch_size, self.neg_ratio = batch_size, neg_ratio
        self.graph, self.hist_ratio = graph, hist_ratio
        self.hist_filled = torch.zeros(1, dtype=torch.int64, device=device) if hist_ratio else None
        self.seed, self.first_row, self.epoch = seed, first_row, 0
        self.rows = rows
        self.src, self.dst = src.to(device), dst.to(device)
        self.time, self.eid = time.to(device), eid.to(device)
        self.borders = borders
        self._d_borders = torch.from_numpy(borders).to(device)

    @classmethod
    def from_dataframe(cls, df, batch_size: int, dst_set: Optional[DeviceDstSet],
                       num_chunks: int = 0, world_size: int = 1, **kwargs):
        """The batches `utils.get_batch(df, batch_size, num_chunks, ...)` cuts: borders stay
        aligned to multiples of `batch_size` in *index* space, and `num_chunks` > 0 drops the
        same random multiple of `batch_size / num_chunks` leading rows (one draw from torch's
        generator, as there).  Computed on the host once.  ValueError when a batch is not a
        contiguous range of rows, i.e. the frame's index does not ascend."""
        from .utils import _random_start, _row_groups
        batch_size = _count(batch_size, "batch_size", 1)
        skip = _random_start(num_chunks, batch_size, world_size)
        borders, end = [], skip
        for pos in _row_groups(df, batch_size, skip):
            if pos[0] != end or pos[-1] - pos[0] + 1 != len(pos) or np.any(np.diff(pos) != 1):
                raise ValueError("from_dataframe: a batch is not a contiguous range of rows; "
                                 "the frame's index must ascend")
            borders.append(int(pos[0]))
            end = int(pos[-1]) + 1
        borders.append(end)
        return cls(df['src'].values, df['dst'].values, df['time'].values, df['eid'].values,
                   batch_size, dst_set, borders=np.asarray(borders, dtype=np.int64), **kwargs)

    @staticmethod
    def _check_graph_device(graph, device):
        if graph is not None and device.index is not None and device.index != graph.device:
            raise ValueError("the graph is on device {}, the stream on {}".format(
                graph.device, device))

    def set_epoch(self, epoch: int):
        """The Philox call word of the negatives: another epoch, other draws for every row."""
        self.epoch = _u64(epoch, "epoch")

    def reset_hist_filled(self):
        """Zeroes `hist_filled` on the current stream."""
        if self.hist_filled is not None:
            self.hist_filled.zero_()

    def _hist_negatives(self, d_borders, count, max_rows, roots, capacity):
        """The launch behind an assemble launch that overwrote `roots` (same borders)."""
        _capi.check(self._lib.gf_batch_hist_negatives(
            self.graph._h, self.src.data_ptr(), self.dst.data_ptr(), self.time.data_ptr(),
            self.rows, d_borders, count, max_rows, self.neg_ratio, self.hist_ratio, self.seed,
            self.epoch, self.first_row, roots.data_ptr(), capacity, self.hist_filled.data_ptr(),
            self.device.index, _capi.current_stream(self.device)))

    def __len__(self):
        return len(self.borders) - 1

    def __iter__(self):
        for i in range(len(self)):
            yield self.batch(i)

    def __getitem__(self, i):
        return self.batch(i)

    def _index(self, i):
        n = len(self)
        i = int(i)
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError("batch {} of {}".format(i, n))
        return i

    def _dl(self):
        if not self.neg_ratio:
            return None, None
        return self.dst_set.ids.data_ptr(), self.dst_set.count.data_ptr()

    def batch(self, i: int, stream=None):
        """(roots, ts, eids) of batch i: one launch on `stream` (default: the current stream),
        two with historical negatives, none for an empty batch."""
        i = self._index(i)
        lo, hi = int(self.borders[i]), int(self.borders[i + 1])
        planes, dev = 2 + self.neg_ratio, self.device
        with torch.cuda.stream(stream) if stream is not None else _NoStream():
            roots = torch.empty(planes * (hi - lo), dtype=torch.int64, device=dev)
            ts = torch.empty(planes * (hi - lo), dtype=torch.float32, device=dev)
            if hi > lo:
                dl, dl_count = self._dl()
                with torch.cuda.device(dev):
                    _capi.check(self._lib.gf_batch_assemble(
                        self.src.data_ptr(), self.dst.data_ptr(), self.time.data_ptr(), self.rows,
                        lo, hi, self.neg_ratio, dl, dl_count, self.seed, self.epoch,
                        self.first_row, roots.data_ptr(), ts.data_ptr(), dev.index,
                        _capi.current_stream(dev)))
                    if self.hist_ratio:
                        self._hist_negatives(self._d_borders.data_ptr() + 8 * i, 1, hi - lo,
                                             roots, planes * (hi - lo))
        return roots, ts, self.eid[lo:hi]

    def materialize(self, first: int = 0, count: Optional[int] = None, stream=None):
        """Batches first .. first + count - 1 (default: to the end) in ONE launch (one more for
        all their historical negatives), as a list of
        (roots, ts, eids) tuples of views into one roots and one ts buffer: the form
        `ReplayPipeline(batches=...)` takes.  The pipeline reads its batches on side streams,
        so synchronise the producing stream (the current one, or `stream`) ONCE after this
        call — once per `materialize`, not per batch — before handing the list over."""
        n = len(self)
        first = _count(first, "first", 0)
        count = n - first if count is None else _count(count, "count", 0)
        if first + count > n:
            raise IndexError("batches {}..{} of {}".format(first, first + count - 1, n))
        b = self.borders[first:first + count + 1]
        planes, dev = 2 + self.neg_ratio, self.device
        total = planes * int(b[-1] - b[0]) if count else 0
        with torch.cuda.stream(stream) if stream is not None else _NoStream():
            roots = torch.empty(total, dtype=torch.int64, device=dev)
            ts = torch.empty(total, dtype=torch.float32, device=dev)
            if total:
                dl, dl_count = self._dl()
                with torch.cuda.device(dev):
                    _capi.check(self._lib.gf_batch_assemble_many(
                        self.src.data_ptr(), self.dst.data_ptr(), self.time.data_ptr(), self.rows,
                        self._d_borders.data_ptr() + 8 * first, count, int(np.diff(b).max()),
                        self.neg_ratio, dl, dl_count, self.seed, self.epoch, self.first_row,
                        roots.data_ptr(), ts.data_ptr(), total, dev.index,
                        _capi.current_stream(dev)))
                    if self.hist_ratio:
                        self._hist_negatives(self._d_borders.data_ptr() + 8 * first, count,
                                             int(np.diff(b).max()), roots, total)
        out = []
        for k in range(count):
            lo, hi = int(b[k]), int(b[k + 1])
            at, size = planes * (lo - int(b[0])), planes * (hi - lo)
            out.append((roots[at:at + size], ts[at:at + size], self.eid[lo:hi]))
        return out
