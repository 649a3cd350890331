"""Autograd-aware Python front of the C ABI (include/kagnn_hip.h).

torch is plumbing here: it owns device memory, the current stream and the autograd tape.  Every
arithmetic step of the hot path is a call into libkagnn_hip.so through ctypes.  CPU tensors are
refused -- there is no CPU implementation in this package (the CPU restatement lives in
``oracle/`` and is test infrastructure only).
"""
from __future__ import annotations

import ctypes
import functools
import inspect
import math
import os
import threading
import weakref
from ctypes import byref, c_int64, c_size_t
from typing import NamedTuple, Optional, Tuple

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import FUSED_MAX_SPLINE_ORDER, HIGH_ORDER_MAX_KNOTS, MAX_SPLINE_ORDER, PREC_FP32, PREC_FP32_GRID, PREC_HALF, PREC_SPLIT

HUB_THRESHOLD = int(os.environ.get("KAGNN_HUB_THRESHOLD", "96"))       # rows above this many edges are split into segments
_LAYER_ABI = os.environ.get("KAGNN_LAYER_ABI", "1") != "0"     # 1: kagnn_gin_kan_layer_fwd / _bwd (one library call each way)
_FOLD_NORM_STATS = os.environ.get("KAGNN_FOLD_NORM_STATS", "1") != "0"


def default_precision() -> int:
    """`KAGNN_PRECISION=fp32|split|half` (default split: fp16 hi/lo operands, three products, fp32 accumulate; `half`: the same
    kernels with ONE fp16 product per fp32 product -- the build-defined reduced-precision mode of BASELINE config 2)."""
    v = os.environ.get("KAGNN_PRECISION", "split").lower()
    if v in ("fp32", "exact", "0"):
        return PREC_FP32
    if v in ("split", "1"):
        return PREC_SPLIT
    if v in ("half", "fp16", "3"):
        return PREC_HALF
    raise ValueError(f"KAGNN_PRECISION={v!r}: expected 'fp32', 'split' or 'half'")


def high_order(spline_order) -> bool:
    """orders 5..16: the exact-fp32 per-operation kernels only (kan_high_order.hip) -- no split / reduced precision, no fused
    layer / stack / model call, no parts or moments forward, no refit, no sharding"""
    return int(spline_order) > FUSED_MAX_SPLINE_ORDER


def split_like(mode) -> bool:
    """the modes that run on the split-precision kernels (and their packs, fused nodes and shape limits): PREC_SPLIT and its
    single-product variant PREC_HALF"""
    return mode == PREC_SPLIT or mode == PREC_HALF


class EntryPointTimer:
    """Optional per-entry-point device timing (HIP events on the launch stream), used by bench.py
    to report the dominant kernel's duration live.  Off by default: zero overhead."""

    def __init__(self, only: Optional[str] = None):
        self.records = []
        self.only = only                 # time just this entry point (None: all of them)

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, a, b in self.records:
            d = out.setdefault(name, [0, 0.0])
            d[0] += 1
            d[1] += a.elapsed_time(b)
        return {k: {"launches": v[0], "total_ms": v[1], "avg_ms": v[1] / v[0]} for k, v in out.items()}


class LibraryStageTimer:
    """Per-stage device timing INSIDE the library (``kagnn_stage_timer_*``): HIP events on the launch stream around every
    per-operation entry point, also when it runs inside the one-call layer entry points -- what ``bench.py`` uses to time the
    dominant kernel live on the product's default path (``KAGNN_LAYER_ABI=1``).  ``only``: record just this stage."""

    def __init__(self, only: Optional[str] = None):
        self.only = only

    def __enter__(self):
        _lib.call("kagnn_stage_timer_enable", None if self.only is None else self.only.encode())
        return self

    def __exit__(self, *exc):
        _lib.call("kagnn_stage_timer_disable")
        return False

    @staticmethod
    def collect(capacity: int = 64):
        """{stage: {"launches", "total_ms", "avg_ms"}} of everything recorded since the last collect (waits for the events)"""
        names = ctypes.create_string_buffer(64 * capacity)
        launches = (c_int64 * capacity)()
        total = (ctypes.c_double * capacity)()
        n = ctypes.c_int32(0)
        _lib.call("kagnn_stage_timer_collect", names, launches, total, capacity, byref(n))
        out = {}
        for i in range(n.value):
            name = names.raw[64 * i:64 * (i + 1)].split(b"\0", 1)[0].decode()
            out[name] = {"launches": int(launches[i]), "total_ms": float(total[i]), "avg_ms": float(total[i]) / max(1, int(launches[i]))}
        return out


_timer: Optional[EntryPointTimer] = None


def set_timer(t: Optional[EntryPointTimer]) -> None:
    global _timer
    _timer = t


def _call(name: str, *args) -> None:
    if _timer is None or (_timer.only is not None and _timer.only != name):
        _lib.call(name, *args)
        return
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    _lib.call(name, *args)
    b.record()
    _timer.records.append((name, a, b))


_SIZE_CACHE: dict = {}


def _sizes(name: str, *args, outputs: int = 1):
    """Size queries (``*_bytes`` entry points) are pure functions of their integer arguments: ask the library
    once per distinct shape.  On small graphs the ctypes round trips were a measurable part of a step."""
    key = (name, args)
    hit = _SIZE_CACHE.get(key)
    if hit is None:
        outs = [c_size_t(0) for _ in range(outputs)]
        cargs = [(ctypes.c_int32 * len(a))(*a) if isinstance(a, tuple) else a for a in args]     # (int tuples: int32 arrays)
        _call(name, *cargs, *[byref(o) for o in outs])
        hit = tuple(o.value for o in outs)
        _SIZE_CACHE[key] = hit
    return hit if outputs > 1 else hit[0]


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """hipStream_t of torch's current stream.  ``torch.cuda.current_stream()`` builds a Stream object through several
    Python layers (~14 us a call, ten calls a layer step: most of the host time of a small graph's step); the raw
    getter is one C call."""
    if _RAW_STREAM is not None:
        return ctypes.c_void_p(_RAW_STREAM(torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_cuda(*ts):
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "kagnn_amd ops run only on MI355X device tensors (libkagnn_hip.so); got a CPU tensor. "
                "There is no CPU fallback in this package.")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"kagnn_amd ops need all operands on one device; got {dev} and {t.device}")


class _NoGuard:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def _device_of(t):
    """Context that makes ``t``'s GPU the current device (kernels launch on the CURRENT device's stream: a model moved
    to ``cuda:1`` without ``torch.cuda.set_device(1)`` would otherwise launch on device 0).  Free when it already is."""
    if t is None or not t.is_cuda or t.device.index == torch.cuda.current_device():
        return _NO_GUARD
    return torch.cuda.device(t.device)


def _on_operand_device(fn):
    """Decorator for ``Function.forward`` / ``.backward``: run on the device of the first CUDA tensor argument."""
    @functools.wraps(fn)
    def run(ctx, *args):
        for a in args:
            if isinstance(a, torch.Tensor) and a.is_cuda:
                if a.device.index != torch.cuda.current_device():
                    with torch.cuda.device(a.device):
                        return fn(ctx, *args)
                break
        return fn(ctx, *args)
    return run


def default_activation_dtype() -> torch.dtype:
    """`KAGNN_ACT=fp32|bf16` (default fp32).  bf16: the rows the neighbour aggregation GATHERS (conv inputs on the way
    forward, d loss / d h0 on the way back) are stored as bf16 -- fp32 accumulation, KAN layers unchanged; a
    build-defined mode for BASELINE.json's config 2, outside the 1e-4 fp32 contract (tests: 4e-3)."""
    v = os.environ.get("KAGNN_ACT", "fp32").lower()
    if v in ("fp32", "f32", "float32"):
        return torch.float32
    if v in ("bf16", "bfloat16"):
        return torch.bfloat16
    raise ValueError(f"KAGNN_ACT={v!r}: expected 'fp32' or 'bf16'")


def _rows(t: torch.Tensor, allow_bf16: bool = False) -> torch.Tensor:
    """2-D fp32 (or, where the entry point takes them, bf16) rows with unit column stride (row stride is passed to the
    kernels as ld)."""
    if t.dim() != 2:
        raise AssertionError(f"expected a 2-D tensor, got shape {tuple(t.shape)}")
    if t.dtype != torch.float32 and not (allow_bf16 and t.dtype == torch.bfloat16):
        raise TypeError(f"kagnn_amd kernels are fp32{' / bf16 gather operands' if allow_bf16 else ''}; got {t.dtype}")
    if t.stride(1) != 1 or (t.size(0) > 1 and t.stride(0) < t.size(1)):
        t = t.contiguous()
    return t


def _ld(t: torch.Tensor) -> int:
    return t.stride(0) if t.size(0) > 1 else max(t.size(1), t.stride(0))


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


# ======================================================================== graph structure
class GraphIndex:
    """CSR (by destination) and its transpose (by source) of one ``edge_index``, int32, on device.

    Built once per edge list by ``kagnn_csr_build`` (stable radix sort => ``perm`` equals
    ``argsort(dst, stable=True)`` bit for bit) and cached; replaces the index bookkeeping
    torch_geometric redoes on every ``propagate`` call.
    """

    def __init__(self, edge_index: torch.Tensor, num_nodes: int, hub_threshold: int = HUB_THRESHOLD, defer_validation: bool = False):
        _need_cuda(edge_index)
        if edge_index.dim() != 2 or edge_index.size(0) != 2 or edge_index.dtype != torch.int64:
            raise ValueError("edge_index must be an int64 tensor of shape [2, E]")
        self.num_nodes = int(num_nodes)
        self.num_edges = int(edge_index.size(1))
        self.hub_threshold = int(hub_threshold)
        self.device = edge_index.device
        src = edge_index[0].contiguous()
        dst = edge_index[1].contiguous()
        self._flags = None
        with _device_of(edge_index):
            if _SMALL_CSR and _lib.load().kagnn_csr_small_ok(self.num_edges, self.num_nodes):
                self._build_small(src, dst)
            else:
                self.rowptr, self.col, self.perm, self.hub_seg, self.num_hub_seg = self._build(dst, src)
                self.rowptr_t, self.col_t, self.perm_t, self.hub_seg_t, self.num_hub_seg_t = self._build(src, dst)
        self._dis = None
        self._edge_list, self._edge_keys = (src, dst), None
        if not defer_validation:
            self.validate()             # (small path: waits for its flags -- graphs that are indexed once pay one synchronisation, as
                                        # the rocPRIM path does; the per-batch graphs of the graph-level models defer it)

    def _build_small(self, src, dst):
        """E, N <= 65 536 (the graph-level models' mini-batches, rebuilt per batch): both structures from ONE launch and without
        blocking the stream (``kagnn_csr_build_small``); same arrays, bit for bit; no hub segments.  Out-of-range node ids are
        clamped on the device (nothing reads out of bounds) and the flags travel to pinned host memory behind the launch;
        ``validate()`` reads them: at once (one synchronisation, like the rocPRIM path) unless the caller asked to defer it
        (``graph_index(..., cache=False)``: the per-batch graphs) -- then without waiting when the next small graph is indexed, or
        by whoever calls ``validate()``."""
        n, e, dev = self.num_nodes, self.num_edges, self.device
        i32 = dict(dtype=torch.int32, device=dev)
        _validate_pending(dev)
        self.rowptr, self.col, self.perm = torch.empty(n + 1, **i32), torch.empty(e, **i32), torch.empty(e, **i32)
        self.rowptr_t, self.col_t, self.perm_t = torch.empty(n + 1, **i32), torch.empty(e, **i32), torch.empty(e, **i32)
        self.hub_seg = self.hub_seg_t = torch.empty(0, **i32)
        self.num_hub_seg = self.num_hub_seg_t = 0
        ws = _ws(_sizes("kagnn_csr_small_workspace_bytes", e), dev)
        flags = torch.empty(2, **i32)
        _call("kagnn_csr_build_small", _ptr(src), _ptr(dst), e, n, _ptr(self.rowptr), _ptr(self.col), _ptr(self.perm),
              _ptr(self.rowptr_t), _ptr(self.col_t), _ptr(self.perm_t), _ptr(flags), _ptr(ws), ws.numel(), _stream())
        self._flags = _defer_flag_check(flags)

    @classmethod
    def from_arrays(cls, rowptr, col, perm, rowptr_t, col_t, perm_t, num_nodes: int, num_edges: int) -> "GraphIndex":
        """A GraphIndex around six int32 device arrays that already ARE the two structures (``kagnn_batch_assemble``: slices of a
        dataset's CSR -- ``kagnn_amd.data``).  Nothing is launched and nothing is validated here: no hub segments (as on the
        small-graph path) and no pending flags -- whoever made the arrays vouches for them."""
        g = cls.__new__(cls)
        g.num_nodes, g.num_edges, g.hub_threshold, g.device = int(num_nodes), int(num_edges), HUB_THRESHOLD, rowptr.device
        g.rowptr, g.col, g.perm, g.rowptr_t, g.col_t, g.perm_t = rowptr, col, perm, rowptr_t, col_t, perm_t
        g.hub_seg = g.hub_seg_t = _no_hub_segments(rowptr.device)
        g.num_hub_seg = g.num_hub_seg_t = 0
        g._flags = None
        g._dis = None
        g._edge_list = g._edge_keys = None
        return g

    def validate(self, wait: bool = True) -> None:
        """raise if the edge list named node ids outside [0, num_nodes) (small-graph path; the rocPRIM path has already raised)"""
        if self._flags is not None:
            _check_flags(self._flags, wait)

    def _build(self, key, val):
        n, e, dev = self.num_nodes, self.num_edges, self.device
        nbytes = c_size_t(0)
        _call("kagnn_csr_workspace_bytes", e, n, byref(nbytes))
        ws = _ws(nbytes.value, dev)
        rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        col = torch.empty(e, dtype=torch.int32, device=dev)
        perm = torch.empty(e, dtype=torch.int32, device=dev)
        seg_len = max(self.hub_threshold // 4, 32)                  # as in csr.hip
        cap = e // seg_len + e // self.hub_threshold + 1
        hub = torch.empty(3 * cap, dtype=torch.int32, device=dev)
        nseg = c_int64(0)
        _call("kagnn_csr_build", _ptr(key), _ptr(val), e, n, _ptr(rowptr), _ptr(col), _ptr(perm),
                  self.hub_threshold, _ptr(hub), cap, byref(nseg), _ptr(ws), ws.numel(), _stream())
        return rowptr, col, perm, hub, int(nseg.value)

    @property
    def gcn_dis(self) -> torch.Tensor:
        """deg^-1/2 with one self loop per node (gcn_norm, add_remaining_self_loops)."""
        if self._dis is None:
            dis = torch.empty(self.num_nodes, dtype=torch.float32, device=self.device)
            with _device_of(self.rowptr):
                _call("kagnn_gcn_deg_inv_sqrt", _ptr(self.rowptr), _ptr(self.col), self.num_nodes,
                      _ptr(dis), _stream())
            self._dis = dis
        return self._dis

    @property
    def edge_keys(self) -> torch.Tensor:
        """the edge set as ascending, duplicate-free int64 keys ``src * num_nodes + dst`` (``kagnn_edge_keys_build``): what
        ``negative_sample`` searches.  Built at the first use and kept -- one read of the key count then, none afterwards."""
        if self._edge_keys is None:
            if self._edge_list is None:
                raise RuntimeError("GraphIndex.edge_keys: an index made from arrays (from_arrays, a subgraph's index) carries no edge "
                                   "list; build the keys with ops.edge_keys(edge_index, num_nodes)")
            self._edge_keys = _edge_keys_raw(self._edge_list[0], self._edge_list[1], self.num_nodes)
        return self._edge_keys

    def side(self, transposed: bool):
        if transposed:
            return self.rowptr_t, self.col_t, self.perm_t, self.hub_seg_t, self.num_hub_seg_t
        return self.rowptr, self.col, self.perm, self.hub_seg, self.num_hub_seg


_NO_HUB: "dict[int, torch.Tensor]" = {}


def _no_hub_segments(dev) -> torch.Tensor:
    """the empty hub-segment list of an index that has none, one per device (``from_arrays`` runs once per mini-batch)"""
    t = _NO_HUB.get(dev.index)
    if t is None:
        t = _NO_HUB[dev.index] = torch.empty(0, dtype=torch.int32, device=dev)
    return t


_CSR_FLAG_MESSAGE = "kagnn_csr_build_small: edge_index holds node ids outside [0, num_nodes)"


def _defer_flag_check(flags: torch.Tensor, message: str = _CSR_FLAG_MESSAGE):
    """the out-of-range-id flags of a small-graph CSR build (2 ints on the device) travel to pinned host memory behind the launches
    queued so far; the entry joins ``_pending_checks`` and is looked at -- without waiting -- when a later small graph is indexed, or
    by ``flush_graph_checks()`` / ``GraphIndex.validate()``.  ``message``: what a raised flag means (the two flags of
    ``kagnn_batch_assemble`` travel the same way)"""
    dev = flags.device
    host = torch.empty(flags.shape, dtype=torch.int32, pin_memory=True)       # (2 ints; [batches, 2] for a loader's epoch)
    host.copy_(flags, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    entry = [host, ev, flags, False, message]
    _pending_checks.setdefault(dev.index, []).append(entry)
    return entry


_SMALL_CSR = True      # False: always the rocPRIM build (a module attribute for the bitwise tests; identical arrays)
_pending_checks: "dict[int, list]" = {}


def _check_flags(entry, wait: bool) -> bool:
    """``entry`` = [pinned flags, event, device flags, done]: True once the flags have been looked at (each entry reports ONCE)"""
    if entry[3]:
        return True
    host, ev = entry[0], entry[1]
    if not ev.query():                # (an event that has completed is not waited for: a loop that indexes a pair list per epoch never waits)
        if not wait:
            return False
        ev.synchronize()
    entry[3] = True
    if (int(host[0]) or int(host[1])) if host.dim() == 1 else bool(host.any()):
        raise RuntimeError(entry[4])
    return True


def _validate_pending(dev) -> None:
    """the deferred range checks of earlier small graphs on this device whose flags have arrived (never waits)"""
    lst = _pending_checks.get(dev.index)
    if lst:
        keep, bad = [], []
        for en in lst:
            try:
                if not _check_flags(en, False):
                    keep.append(en)
            except RuntimeError:
                bad.append(en[4])
        _pending_checks[dev.index] = keep
        if bad:
            raise RuntimeError(_earlier_failures(bad))


def _earlier_failures(messages) -> str:
    out = []
    for m in messages:
        m = "kagnn_csr_build_small: an edge_index indexed earlier held node ids outside [0, num_nodes)" if m == _CSR_FLAG_MESSAGE else m
        if m not in out:
            out.append(m)
    return "; ".join(out)


def flush_graph_checks(device=None) -> None:
    """WAIT for the deferred node-id range checks of every small graph indexed so far (``graph_index(cache=False)``:
    ``kagnn_csr_build_small`` clamps out-of-range ids and raises a flag that is otherwise only looked at when a LATER graph is
    indexed) and raise if any failed.  Call it at a natural synchronisation point -- the end of an epoch or an evaluation loop,
    before reading outputs back on the host (the last batch of a loop, or a single inference call, was never
    validated).  ``harness.train_graph_batches`` does so at the end of every epoch."""
    devs = list(_pending_checks) if device is None else [torch.device(device).index]
    for flags, message in ((_nll_flags, _NLL_FLAG_MESSAGE), (_node_eval_flags, _NODE_EVAL_FLAG_MESSAGE)):
        if flags:
            if device is None:
                devs += [d for d in flags if d not in devs]
            _defer_label_flags(flags, devs, message)     # the bad-label flag of every nll_loss / node_eval launch so far joins the checks waited for below
    bad = []
    for d in devs:
        for en in _pending_checks.get(d) or []:
            try:
                _check_flags(en, True)
            except RuntimeError:
                bad.append(en[4])
        _pending_checks[d] = []
    if bad:
        raise RuntimeError(_earlier_failures(bad))


_graph_cache: "dict[tuple, GraphIndex]" = {}
_GRAPH_CACHE_MAX = 8
def graph_index(edge_index: torch.Tensor, num_nodes: int, cache: bool = True) -> GraphIndex:
    """Cached GraphIndex keyed on the identity and version of ``edge_index`` (SURVEY 8(b) ownership): full-batch node
    models see the same ``edge_index`` every epoch.  ``cache=False`` (the graph-level models' mini-batches, which never
    repeat): build and drop -- a cache that never hits only pins the last 8 batches and both of their CSRs."""
    if not cache:
        return GraphIndex(edge_index, num_nodes, defer_validation=True)
    key = (edge_index.data_ptr(), edge_index._version, tuple(edge_index.shape), int(num_nodes),
           edge_index.device.index)
    g = _graph_cache.get(key)
    if g is None:
        if len(_graph_cache) >= _GRAPH_CACHE_MAX:
            _graph_cache.pop(next(iter(_graph_cache)))
        g = GraphIndex(edge_index, num_nodes)
        g._keepalive = edge_index     # the key holds a raw pointer: pin the tensor it names
        _graph_cache[key] = g
    return g


def batch_graph_index(data, num_nodes: int) -> GraphIndex:
    """The index of a mini-batch object of the graph-level models: ``data.graph_index`` when the loader assembled one with the batch
    (``kagnn_amd.data.DeviceBatchLoader``: slices of the dataset's CSR, the same bits as a build from ``data.edge_index``) and it
    describes this ``edge_index``; else built from ``data.edge_index`` as for any other batch object (never cached: mini-batches
    do not repeat)."""
    g = getattr(data, "graph_index", None)
    ei = data.edge_index
    if isinstance(g, GraphIndex) and g.num_nodes == int(num_nodes) and g.num_edges == int(ei.size(1)) and g.device == ei.device:
        return g
    return graph_index(ei, num_nodes, cache=False)


def clear_graph_cache() -> None:
    _graph_cache.clear()
    _gcn_cache.clear()


class Subgraph(NamedTuple):
    """What ``k_hop_subgraph`` / ``induced_subgraph`` return: the subgraph of a parent ``GraphIndex`` induced by a node selection,
    relabelled to ``0 .. num_nodes - 1`` in ascending order of the original ids (torch_geometric's ``relabel_nodes=True``)."""
    nodes: torch.Tensor                  # int64 [num_nodes]: original node ids, ascending
    edge_index: torch.Tensor             # int64 [2, num_edges]: relabelled edge list, in original edge order
    edge_ids: torch.Tensor               # int64 [num_edges]: original edge ids, ascending (the set bits of torch_geometric's edge_mask)
    mapping: Optional[torch.Tensor]      # int64, one entry per entry of the node ids handed in: its position in ``nodes`` (None: a bool mask)
    hops: Optional[torch.Tensor]         # int32 [num_nodes]: hops from each node to the nearest seed (None: an induced subgraph)
    index: GraphIndex                    # both CSR structures of ``edge_index``, the bits a build would give; nothing was sorted; no hub segments
    num_nodes: int
    num_edges: int


def _subgraph_operands(what, ids, g):
    """the refusals ``k_hop_subgraph`` and ``induced_subgraph`` share, before anything is launched; returns the ids as an int64
    device vector, or a bool mask of length N as it is"""
    if not isinstance(g, GraphIndex):
        raise TypeError(f"{what}: the graph must be an ops.GraphIndex (ops.graph_index(edge_index, num_nodes))")
    if isinstance(ids, torch.Tensor) and ids.dtype == torch.bool:
        if ids.dim() != 1 or ids.numel() != g.num_nodes:
            raise ValueError(f"{what}: a node mask must have shape [{g.num_nodes}], got {tuple(ids.shape)}")
    elif isinstance(ids, torch.Tensor):
        if ids.dtype != torch.int64 or ids.dim() > 1:
            raise ValueError(f"{what}: node ids must be an int64 scalar or vector (or a bool mask of length num_nodes)")
        ids = ids.reshape(-1)
    _need_cuda(g.rowptr, ids if isinstance(ids, torch.Tensor) else None)
    if not isinstance(ids, torch.Tensor):
        ids = torch.tensor([ids] if isinstance(ids, int) else list(ids), dtype=torch.int64, device=g.device).reshape(-1)
    return ids.contiguous()


def _subgraph_extract(what, hop, rec, g: GraphIndex, ids, keep_hops: bool, keep=None) -> Subgraph:
    """``hop`` [N] int32 selects the nodes (>= 0); ``rec`` = device int32 [n_sub, e_sub, bad-seed flag]: count, the ONE read-back
    (pinned memory), fill with exact sizes.  ``keep`` [E] uint8: the subgraph of that edge selection (the ``kagnn_edge_subgraph_*``
    pair) in place of the induced one"""
    n, e, dev = g.num_nodes, g.num_edges, g.device
    i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
    ws = _ws(_sizes("kagnn_subgraph_workspace_bytes", n, e), dev)
    parent = [_ptr(t) for t in (g.rowptr, g.col, g.perm, g.rowptr_t, g.col_t, g.perm_t)]
    if keep is None:
        _call("kagnn_subgraph_count", _ptr(hop), *parent, n, e, _ptr(ws), ws.numel(), _ptr(rec), _stream())
    else:
        _call("kagnn_edge_subgraph_count", _ptr(hop), _ptr(keep), *parent, n, e, _ptr(ws), ws.numel(), _ptr(rec), _stream())
    host = torch.empty(3, dtype=torch.int32, pin_memory=True)
    host.copy_(rec, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    ev.synchronize()
    n_sub, e_sub, bad = (int(v) for v in host)
    if bad:
        raise ValueError(f"{what}: node ids outside [0, {n})")
    nodes, edge_ids, ei = torch.empty(n_sub, **i64), torch.empty(e_sub, **i64), torch.empty((2, e_sub), **i64)
    rowptr, col, perm = torch.empty(n_sub + 1, **i32), torch.empty(e_sub, **i32), torch.empty(e_sub, **i32)
    rowptr_t, col_t, perm_t = torch.empty(n_sub + 1, **i32), torch.empty(e_sub, **i32), torch.empty(e_sub, **i32)
    outs = [_ptr(t) for t in (nodes, edge_ids, ei, rowptr, col, perm, rowptr_t, col_t, perm_t)]
    if keep is None:
        _call("kagnn_subgraph_fill", _ptr(ws), ws.numel(), *parent, n, e, n_sub, e_sub, *outs, _stream())
    else:
        _call("kagnn_edge_subgraph_fill", _ptr(ws), ws.numel(), _ptr(keep), *parent, n, e, n_sub, e_sub, *outs, _stream())
    mapping = None
    if ids is not None:
        relabel = ws[:4 * n].view(torch.int32)             # (the workspace begins with relabel[N]: kagnn_hip.h)
        mapping = relabel.index_select(0, ids).to(torch.int64) if ids.numel() else torch.empty(0, **i64)
    hops = hop.index_select(0, nodes) if keep_hops else None
    index = GraphIndex.from_arrays(rowptr, col, perm, rowptr_t, col_t, perm_t, n_sub, e_sub)
    return Subgraph(nodes, ei, edge_ids, mapping, hops, index, n_sub, e_sub)


def _mark_hops(ids, num_hops: int, g: GraphIndex):
    n, dev = g.num_nodes, g.device
    hop = torch.empty(n, dtype=torch.int32, device=dev)
    rec = torch.empty(3, dtype=torch.int32, device=dev)
    _call("kagnn_k_hop_mark", _ptr(g.rowptr), _ptr(g.col), n, _ptr(ids), ids.numel(), int(num_hops), _ptr(hop), _ptr(rec[2:]), _stream())
    return hop, rec


def k_hop_subgraph(node_idx, num_hops: int, g: GraphIndex) -> Subgraph:
    """torch_geometric's ``k_hop_subgraph(node_idx, num_hops, edge_index, relabel_nodes=True)`` (``flow='source_to_target'``) on
    the parent's index ``g``: the nodes from which some node of ``node_idx`` (an int, a sequence or an int64 device vector;
    duplicates allowed) is reached along at most ``num_hops`` edges, and every edge between two of them -- what the prediction of
    a ``num_hops``-layer message-passing model at ``node_idx`` rests on (``kagnn_amd.receptive_hops``: a GCN-normalised model needs
    one hop more than it has layers).  ``kagnn_k_hop_mark`` -> ``kagnn_subgraph_count`` -> one read of the two counts and the
    bad-seed flag from pinned memory -> ``kagnn_subgraph_fill``; the parent's rows are compacted in place of a sort, so
    ``.index`` holds the bits ``GraphIndex(sub.edge_index, sub.num_nodes)`` would, without hub segments.  Raises ``ValueError``
    for a seed outside ``[0, N)`` (after the read) and for ``num_hops < 0``; empty seeds give an empty subgraph."""
    if isinstance(num_hops, bool) or int(num_hops) != num_hops or num_hops < 0:
        raise ValueError(f"k_hop_subgraph: num_hops must be a non-negative integer, got {num_hops!r}")
    if isinstance(node_idx, torch.Tensor) and node_idx.dtype == torch.bool:
        raise ValueError("k_hop_subgraph: node_idx must be node ids, not a mask")
    ids = _subgraph_operands("k_hop_subgraph", node_idx, g)
    with _device_of(g.rowptr):
        hop, rec = _mark_hops(ids, int(num_hops), g)
        return _subgraph_extract("k_hop_subgraph", hop, rec, g, ids, True)


def induced_subgraph(nodes, g: GraphIndex) -> Subgraph:
    """torch_geometric's ``subgraph(nodes, edge_index, relabel_nodes=True, return_edge_mask=True)`` on the parent's index ``g``:
    ``nodes`` is a sequence / int64 device vector of ids (duplicates allowed) or a bool mask ``[N]``.  The same calls and the same
    single read as ``k_hop_subgraph`` (the mark call with ``num_hops = 0``; a mask needs no mark call); ``.hops`` is ``None``."""
    ids = _subgraph_operands("induced_subgraph", nodes, g)
    with _device_of(g.rowptr):
        if ids.dtype == torch.bool:
            hop = ids.to(torch.int32) - 1                                   # selected: 0, else -1
            rec = torch.zeros(3, dtype=torch.int32, device=g.device)
            return _subgraph_extract("induced_subgraph", hop, rec, g, None, False)
        hop, rec = _mark_hops(ids, 0, g)
        return _subgraph_extract("induced_subgraph", hop, rec, g, ids, False)


def _fanouts(what, fanouts) -> list:
    """the fan-outs of ``sample_neighbors`` as a list of ints: 1 .. 16 integers, each a count (>= 0) or -1 (all)"""
    if isinstance(fanouts, torch.Tensor):
        fanouts = fanouts.tolist() if fanouts.dim() == 1 and not fanouts.is_cuda else None
    try:
        out = list(fanouts)
    except TypeError:
        out = None
    if out is None or not 1 <= len(out) <= _lib.SAMPLE_MAX_LEVELS:
        raise ValueError(f"{what}: fanouts must be a sequence of 1 to {_lib.SAMPLE_MAX_LEVELS} integers, got {fanouts!r}")
    for k in out:
        if isinstance(k, bool) or not isinstance(k, (int, float)) or int(k) != k or k < -1 or k > 2147483647:
            raise ValueError(f"{what}: every fan-out must be an integer >= 0, or -1 for all neighbours; got {k!r}")
    return [int(k) for k in out]


def sample_neighbors(node_idx, fanouts, g: GraphIndex, seed: int = 0) -> Subgraph:
    """Fan-out-limited neighbour sampling on the parent's index ``g`` (GraphSAGE; what torch_geometric's ``NeighborLoader`` draws
    per batch, directed and without replacement): level ``d`` of a backward BFS from ``node_idx`` (an int, a sequence or an int64
    device vector; duplicates allowed) keeps, for every node first reached at level ``d``, ``min(in-degree, fanouts[d])`` of its
    in-edges -- ``-1``: all of them -- and reaches their sources.  Returns the ``Subgraph`` of the kept EDGES (not the induced
    one): ``nodes`` ascending, ``edge_ids`` the kept edges in original order, ``hops`` the level at which a node was first reached,
    ``mapping`` the seeds' rows, ``index`` the bits ``GraphIndex(sub.edge_index, sub.num_nodes)`` would hold, nothing sorted.
    Which edges a row keeps is a pure function of ``(seed, original edge id)`` (``kagnn_hip.h``: the ``k`` smallest ``(key32, e)``
    of the row): the result does not depend on the order or duplication of the seeds, and two calls return the same bits.
    ``kagnn_neighbor_sample_mark`` -> ``kagnn_edge_subgraph_count`` -> one read of the two counts and the bad-seed flag ->
    ``kagnn_edge_subgraph_fill``.  ``seed``: any int, taken mod 2^64.  Raises ``ValueError`` for a mask as seeds, ``len(fanouts)``
    outside 1..16, an entry below -1 or not an integer (all before any launch) and for a seed outside ``[0, N)`` (after the read);
    empty seeds give an empty subgraph."""
    fan = _fanouts("sample_neighbors", fanouts)
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError(f"sample_neighbors: seed must be an int, got {seed!r}")
    if isinstance(node_idx, torch.Tensor) and node_idx.dtype == torch.bool:
        raise ValueError("sample_neighbors: node_idx must be node ids, not a mask")
    ids = _subgraph_operands("sample_neighbors", node_idx, g)
    with _device_of(g.rowptr):
        hop, keep, rec = _mark_sampled(ids, fan, g, seed)
        return _subgraph_extract("sample_neighbors", hop, rec, g, ids, True, keep)


def _mark_sampled(ids, fan, g: GraphIndex, seed: int):
    n, e, dev = g.num_nodes, g.num_edges, g.device
    hop = torch.empty(n, dtype=torch.int32, device=dev)
    keep = torch.empty(e, dtype=torch.uint8, device=dev)
    rec = torch.empty(3, dtype=torch.int32, device=dev)
    fan_host = (ctypes.c_int32 * len(fan))(*fan)
    _call("kagnn_neighbor_sample_mark", _ptr(g.rowptr), _ptr(g.col), _ptr(g.perm), n, e, _ptr(ids), ids.numel(), fan_host, len(fan),
          int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(hop), _ptr(keep), _ptr(rec[2:]), _stream())
    return hop, keep, rec


class WeightedGcnGraph:
    """``gcn_norm`` with edge weights (torch_geometric 2.5.3 semantics, restated in oracle/kan_oracle.py).

    Dense ``edge_index`` (``gcn_norm`` -> ``add_remaining_self_loops``): non-loop edges keep their weight, every node
    gets exactly one self loop (an existing loop keeps its weight, otherwise 1).  Sparse adjacency
    (``sparse_loops=True``; ``gcn_norm`` -> ``add_self_loops`` + coalesce): every node gets a weight-1 loop ADDED to
    whatever its diagonal entry already holds.  Either way ``deg`` = weighted in-degree, ``dis = deg^-1/2`` (inf -> 0).
    The augmented edge list is indexed once (CSR + transpose); built with a handful of torch ops -- per graph, not
    per step."""

    def __init__(self, edge_index: torch.Tensor, edge_weight: Optional[torch.Tensor], num_nodes: int,
                 sparse_loops: bool = False):
        _need_cuda(edge_index)
        dev = edge_index.device
        src, dst = edge_index[0], edge_index[1]
        w = (torch.ones(src.numel(), dtype=torch.float32, device=dev) if edge_weight is None
             else edge_weight.to(device=dev, dtype=torch.float32))
        keep = src != dst
        if sparse_loops:         # coalesced input: at most one (i, i) entry per node
            loop_w = torch.ones(num_nodes, dtype=torch.float32, device=dev).index_add_(0, src[~keep], w[~keep])
        else:
            loop_w = torch.ones(num_nodes, dtype=torch.float32, device=dev)
            loop_w[src[~keep]] = w[~keep]
        ar = torch.arange(num_nodes, dtype=src.dtype, device=dev)
        ei = torch.stack([torch.cat([src[keep], ar]), torch.cat([dst[keep], ar])]).contiguous()
        self.weight = torch.cat([w[keep], loop_w]).contiguous()
        deg = torch.zeros(num_nodes, dtype=torch.float32, device=dev).index_add_(0, ei[1], self.weight)
        dis = deg.pow(-0.5)
        self.dis = torch.where(torch.isinf(dis), torch.zeros_like(dis), dis).contiguous()
        self.graph = GraphIndex(ei, num_nodes)
        self._keepalive = (ei,)


_gcn_cache: "dict[tuple, WeightedGcnGraph]" = {}


def weighted_gcn_graph(edge_index: torch.Tensor, edge_weight: Optional[torch.Tensor], num_nodes: int) -> WeightedGcnGraph:
    """Cached per (edge_index, edge_weight) identity / version.  ``edge_index`` may also be a torch sparse COO
    matrix, read the way torch_geometric reads a sparse ``adj_t``: entry (i, j) = weight of the edge j -> i (the
    form the reference's gcn timing branch passes, ``time_model.py:70-80``); its self loops follow
    ``add_self_loops`` (+1 on the diagonal), see ``WeightedGcnGraph``."""
    if isinstance(edge_index, torch.Tensor) and edge_index.is_sparse:
        key = (id(edge_index), int(num_nodes))
        hit = _gcn_cache.get(key)
        if hit is not None and hit._owner is edge_index:
            return hit
        adj = edge_index.coalesce()
        idx = adj.indices()
        hit = WeightedGcnGraph(torch.stack([idx[1], idx[0]]).contiguous(), adj.values(), num_nodes, sparse_loops=True)
        hit._owner = edge_index
    else:
        key = (edge_index.data_ptr(), edge_index._version, tuple(edge_index.shape), int(num_nodes),
               None if edge_weight is None else (edge_weight.data_ptr(), edge_weight._version))
        hit = _gcn_cache.get(key)
        if hit is not None:
            return hit
        hit = WeightedGcnGraph(edge_index, edge_weight, num_nodes)
        hit._owner = (edge_index, edge_weight)
    if len(_gcn_cache) >= _GRAPH_CACHE_MAX:
        _gcn_cache.pop(next(iter(_gcn_cache)))
    _gcn_cache[key] = hit
    return hit


# ======================================================================== aggregation
def _aggregate_raw(x, g: GraphIndex, transposed, self_scale, edge_weight, in_scale, out_scale, bias,
                   skip_self, out_dtype=torch.float32, addend=None) -> torch.Tensor:
    x = _rows(x, allow_bf16=True)
    if x.size(0) != g.num_nodes:
        raise ValueError(f"x has {x.size(0)} rows but the graph has {g.num_nodes} nodes")
    rowptr, col, _, hub, nhub = g.side(transposed)
    if addend is not None and (x.dtype != torch.float32 or out_dtype != torch.float32):
        return _aggregate_csr(x, rowptr, col, hub, nhub, g.hub_threshold, self_scale, edge_weight, in_scale, out_scale, bias,
                              skip_self, out_dtype) + addend.to(out_dtype)
    return _aggregate_csr(x, rowptr, col, hub, nhub, g.hub_threshold, self_scale, edge_weight, in_scale, out_scale, bias,
                          skip_self, out_dtype, addend)


def aggregate_sum_affine(x, g: GraphIndex, self_scale: float, affine: torch.Tensor, transposed: bool = False) -> torch.Tensor:
    """``aggregate_sum(x * affine[0] + affine[1], g, self_scale)`` without that matrix (``kagnn_aggregate_sum_affine``: the affine is
    applied to the row sums -- ``a * (self * x_i + sum_j x_j) + (self + deg_i) * b``).  Forward only (no autograd): inside the
    fused convolution node the library makes this call itself; this wrapper serves tests and the C-ABI documentation."""
    _need_cuda(x, affine)
    x = _rows(x.detach())
    rowptr, col, _, hub, nhub = g.side(transposed)
    n, f = x.shape
    out = torch.empty((n, f), dtype=torch.float32, device=x.device)
    ws = _ws(_sizes("kagnn_aggregate_workspace_bytes", nhub, f), x.device) if nhub else None
    with _device_of(x):
        _call("kagnn_aggregate_sum_affine", _ptr(x), _ld(x), _ptr(out), f, _ptr(rowptr), _ptr(col), n, f, float(self_scale),
              _ptr(affine[0]), _ptr(affine[1]), _ptr(hub) if nhub else None, nhub, g.hub_threshold, None, 0,
              _ptr(ws), ws.numel() if ws is not None else 0, _stream())
    return out


def _bf16_gather_width_ok(f: int) -> bool:
    """a row width the bf16 aggregation takes (the rule is api.hip's; this is its one copy on the Python side)"""
    return f % 8 == 0 and f <= 512


def _bf16_rows_ok(t: torch.Tensor) -> bool:
    return _bf16_gather_width_ok(t.size(1)) and _ld(t) % 8 == 0 and t.data_ptr() % 16 == 0


def to_bf16_rows(x: torch.Tensor) -> torch.Tensor:
    """fp32 rows -> bf16 (round to nearest even) in one pass (kagnn_rows_to_bf16)"""
    x = _rows(x)
    if not _bf16_rows_ok(x.new_empty((1, x.size(1)), dtype=torch.bfloat16)) or _ld(x) % 4 or x.data_ptr() % 16:
        return x.to(torch.bfloat16)
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    _call("kagnn_rows_to_bf16", _ptr(x), _ld(x), _ptr(y), x.size(1), x.size(0), x.size(1), _stream())
    return y


def _aggregate_csr(x, rowptr, col, hub, nhub, hub_threshold, self_scale, edge_weight, in_scale, out_scale, bias,
                   skip_self, out_dtype=torch.float32, addend=None) -> torch.Tensor:
    n, f = x.shape
    if rowptr.numel() != n + 1:
        raise ValueError(f"x has {n} rows but the graph has {rowptr.numel() - 1} nodes")
    if x.dtype == torch.bfloat16 or out_dtype == torch.bfloat16:
        if x.dtype != torch.bfloat16:
            x = to_bf16_rows(x)
        out = torch.empty((n, f), dtype=out_dtype, device=x.device)
        if not (_bf16_rows_ok(x) and (out_dtype != torch.bfloat16 or _bf16_rows_ok(out))):
            # widths the bf16 kernels do not take: through fp32 (same values, one more pass)
            return _aggregate_csr(x.float(), rowptr, col, hub, nhub, hub_threshold, self_scale, edge_weight, in_scale,
                                  out_scale, bias, skip_self).to(out_dtype)
        ws = _ws(_sizes("kagnn_aggregate_workspace_bytes", nhub, f), x.device) if nhub else None
        _call("kagnn_aggregate_sum_bf16", _ptr(x), _ld(x), _ptr(out), f,
              _lib.DTYPE_BF16 if out_dtype == torch.bfloat16 else _lib.DTYPE_F32, _ptr(rowptr), _ptr(col),
              _ptr(edge_weight), n, f, float(self_scale), _ptr(in_scale), _ptr(out_scale), _ptr(bias), int(skip_self),
              _ptr(hub) if nhub else None, nhub, hub_threshold, _ptr(ws), ws.numel() if nhub else 0, _stream())
        return out
    out = torch.empty((n, f), dtype=torch.float32, device=x.device)
    ws = _ws(_sizes("kagnn_aggregate_workspace_bytes", nhub, f), x.device) if nhub else None   # per-segment partial sums
    if addend is None:
        _call("kagnn_aggregate_sum", _ptr(x), _ld(x), _ptr(out), f, _ptr(rowptr), _ptr(col),
              _ptr(edge_weight), n, f, float(self_scale), _ptr(in_scale), _ptr(out_scale), _ptr(bias),
              int(skip_self), _ptr(hub) if nhub else None, nhub, hub_threshold, _ptr(ws), ws.numel() if nhub else 0, _stream())
    else:
        _call("kagnn_aggregate_sum_add", _ptr(x), _ld(x), _ptr(out), f, _ptr(rowptr), _ptr(col),
              _ptr(edge_weight), n, f, float(self_scale), _ptr(in_scale), _ptr(out_scale), _ptr(bias),
              int(skip_self), _ptr(hub) if nhub else None, nhub, hub_threshold, _ptr(addend), _ld(addend), _ptr(ws),
              ws.numel() if nhub else 0, _stream())
    return out


def aggregate_edge_grad(x, gout, g: GraphIndex, in_scale=None, out_scale=None, skip_self_loops: bool = False, out=None) -> torch.Tensor:
    """d loss / d edge_weight of ``aggregate_sum(x, g, edge_weight=w, in_scale=, out_scale=, skip_self_loops=)`` given the gradient
    ``gout`` of its result: ``[E]`` fp32 in ORIGINAL edge order, ``out_scale[dst] * in_scale[src] * <gout[dst], x[src]>`` per edge and
    exactly 0 for a dropped self loop (``kagnn_aggregate_edge_grad``: no atomics, bit-reproducible).  Raw and non-differentiable:
    ``aggregate_sum`` calls it in its backward when the weights require a gradient.  ``out``: write into the first ``E`` elements of
    this contiguous fp32 vector instead of a new one."""
    _need_cuda(x, gout, in_scale, out_scale, out)
    x, gout = _rows(x.detach()), _rows(gout.detach())
    n, f = x.shape
    if n != g.num_nodes or gout.shape != x.shape:
        raise ValueError(f"x {tuple(x.shape)} and gout {tuple(gout.shape)} must both be [{g.num_nodes}, F]")
    scales = []
    for s in (in_scale, out_scale):
        if s is not None:
            s = s.detach().to(torch.float32).contiguous()
            if s.shape != (n,):
                raise ValueError(f"in_scale / out_scale must be [{n}]")
        scales.append(s)
    e = g.num_edges
    if out is not None and (out.dtype != torch.float32 or out.dim() != 1 or out.numel() < e or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous fp32 vector of at least {e} elements")
    with _device_of(x):
        return _aggregate_edge_grad_csr(x, gout, g.rowptr, g.col, g.perm, g.hub_seg if g.num_hub_seg else None, g.num_hub_seg,
                                        g.hub_threshold, e, scales[0], scales[1], skip_self_loops, out)


def _aggregate_edge_grad_csr(x, gout, rowptr, col, perm, hub, nhub, hub_threshold, num_edges, in_scale, out_scale, skip_self, out=None):
    """the launch of ``aggregate_edge_grad`` on the arrays of the by-destination CSR (also what ``kagnn::aggregate_edge_grad`` of
    ``kagnn_amd.library`` runs): fp32 rows with unit column stride, fp32 scales or None"""
    n, f = x.shape
    if out is None:
        out = torch.empty(num_edges, dtype=torch.float32, device=x.device)
    _call("kagnn_aggregate_edge_grad", _ptr(x), _ld(x), _ptr(gout), _ld(gout), _ptr(rowptr), _ptr(col), _ptr(perm), n, num_edges, f,
          _ptr(in_scale), _ptr(out_scale), int(bool(skip_self)), _ptr(hub) if nhub else None, nhub, hub_threshold, _ptr(out), _stream())
    return out


class _AggregateFn(Function):
    """out = out_scale * (self_scale*s*x_i + sum_e w_e * s_j * x_j) + bias over the by-dst CSR;
    backward is the same kernel on the transposed CSR with in/out scales swapped, and -- only when the edge weights require a
    gradient, the one case in which the gathered rows are kept -- ``aggregate_edge_grad`` for theirs."""

    @staticmethod
    @_on_operand_device
    def forward(ctx, x, bias, g, self_scale, edge_weight, in_scale, out_scale, skip_self):
        _need_cuda(x)
        ctx.g, ctx.self_scale, ctx.skip_self = g, self_scale, skip_self
        ctx.in_scale, ctx.out_scale = in_scale, out_scale
        ctx.edge_weight_t = None
        if edge_weight is not None:
            if ctx.needs_input_grad[4]:
                if edge_weight.shape != (g.num_edges,):
                    raise ValueError(f"edge_weight must be [{g.num_edges}] to receive a gradient, got {tuple(edge_weight.shape)}")
                rows = _rows(x, allow_bf16=True)
                ctx.save_for_backward(rows if rows.dtype == torch.float32 else rows.float())    # (bf16 rows: the values that were summed)
                ctx.edge_weight_dtype = edge_weight.dtype
            w = edge_weight.to(torch.float32)
            ctx.edge_weight_t = w[g.perm_t.long()].contiguous()
            edge_weight = w[g.perm.long()].contiguous()
        ctx.x_dtype = x.dtype
        return _aggregate_raw(x, g, False, self_scale, edge_weight, in_scale, out_scale, bias, skip_self)

    @staticmethod
    @once_differentiable
    @_on_operand_device
    def backward(ctx, gout):
        gx = gb = gw = None
        if ctx.needs_input_grad[0]:
            gx = _aggregate_raw(gout, ctx.g, True, ctx.self_scale, ctx.edge_weight_t, ctx.out_scale,
                                ctx.in_scale, None, ctx.skip_self, out_dtype=ctx.x_dtype)
        if ctx.needs_input_grad[1]:
            gb = gout.sum(0)
        if ctx.needs_input_grad[4]:
            gw = aggregate_edge_grad(ctx.saved_tensors[0], gout, ctx.g, ctx.in_scale, ctx.out_scale, ctx.skip_self).to(ctx.edge_weight_dtype)
        return gx, gb, None, None, gw, None, None, None


def aggregate_sum(x, g: GraphIndex, self_scale: float = 1.0, edge_weight=None, in_scale=None,
                  out_scale=None, bias=None, skip_self_loops: bool = False) -> torch.Tensor:
    if torch.compiler.is_compiling():
        from . import library
        return library.aggregate(x, g, self_scale, edge_weight, in_scale, out_scale, bias, skip_self_loops)
    return _AggregateFn.apply(x, bias, g, float(self_scale), edge_weight, in_scale, out_scale,
                              bool(skip_self_loops))


class _GineFn(Function):
    @staticmethod
    @_on_operand_device
    def forward(ctx, x, edge_attr, g, self_scale):
        _need_cuda(x, edge_attr)
        x, ea = _rows(x), _rows(edge_attr)
        n, f = x.shape
        if ea.shape != (g.num_edges, f):
            raise ValueError("edge_attr must be [E, F] with F == x.size(1)")
        out = torch.empty((n, f), dtype=torch.float32, device=x.device)
        _call("kagnn_aggregate_gine", _ptr(x), _ld(x), _ptr(ea), _ld(ea), _ptr(out), f,
                  _ptr(g.rowptr), _ptr(g.col), _ptr(g.perm), n, f, float(self_scale), _stream())
        ctx.save_for_backward(x, ea)
        ctx.g, ctx.self_scale = g, self_scale
        return out

    @staticmethod
    @once_differentiable
    @_on_operand_device
    def backward(ctx, gout):
        x, ea = ctx.saved_tensors
        g = ctx.g
        gout = _rows(gout)
        n, f = x.shape
        gx = torch.empty((n, f), dtype=torch.float32, device=x.device)
        gea = torch.empty((g.num_edges, f), dtype=torch.float32, device=x.device) \
            if ctx.needs_input_grad[1] else None
        _call("kagnn_aggregate_gine_bwd", _ptr(x), _ld(x), _ptr(ea), _ld(ea), _ptr(gout), _ld(gout),
                  _ptr(gx), f, _ptr(gea), f, _ptr(g.rowptr_t), _ptr(g.col_t), _ptr(g.perm_t), n, f,
                  float(ctx.self_scale), _stream())
        return gx, gea, None, None


def aggregate_gine(x, edge_attr, g: GraphIndex, self_scale: float = 1.0) -> torch.Tensor:
    return _GineFn.apply(x, edge_attr, g, float(self_scale))


# ======================================================================== pooling
def segment_ptr(batch: torch.Tensor, num_graphs: int) -> torch.Tensor:
    """Offsets of a SORTED batch vector (torch_geometric's DataLoader emits it sorted): ptr[b] = the first node of graph b.
    One binary search per offset (round 5: bincount + cumsum + zero-fill + slice copy were four launches per mini-batch)."""
    marks = torch.arange(num_graphs + 1, dtype=batch.dtype, device=batch.device)
    return torch.searchsorted(batch, marks, out_int32=True)


def _segment_pool_raw(x, seg, mean):
    b, f = seg.numel() - 1, x.size(1)
    out = torch.empty((b, f), dtype=torch.float32, device=x.device)
    _call("kagnn_segment_pool", _ptr(x), _ld(x), _ptr(out), f, _ptr(seg), b, f, int(mean), _stream())
    return out


_ZERO_ROWS: "dict[tuple, torch.Tensor]" = {}


def _segment_broadcast_raw(gout, seg, n, mean):
    """the gradient of ``_segment_pool_raw``.  The kernel writes the rows of ``[seg[0], seg[B])`` only; nothing pooled depends on
    rows before ``seg[0]`` or from ``seg[B]`` on (a ``seg_ptr`` that does not span all ``n`` rows: ``segment_ptr`` with fewer graphs
    than the batch vector names, or any caller-made one), so their gradient is zero: the same kernel broadcasts a zero row over
    the two ranges ``[0, seg[0])`` and ``[seg[B], n)``, whose ends stay on the device (no host read of ``seg``, no pass over a
    covered row)."""
    b, f = gout.shape
    dev = gout.device
    if b == 0:
        return torch.zeros((n, f), dtype=torch.float32, device=dev)
    gx = torch.empty((n, f), dtype=torch.float32, device=dev)
    _call("kagnn_segment_broadcast", _ptr(gout), _ld(gout), _ptr(gx), f, _ptr(seg), b, f, int(mean), _stream())
    zero = _ZERO_ROWS.get((dev.index, f))
    if zero is None:
        zero = _ZERO_ROWS[(dev.index, f)] = torch.zeros((1, f), dtype=torch.float32, device=dev)
    ends = torch.full((4,), n, dtype=torch.int32, device=dev)          # [0, seg[0]] and [seg[B], n]: two one-segment pointers
    ends[0:1].zero_()
    ends[1:3].copy_(seg[::b])
    _call("kagnn_segment_broadcast", _ptr(zero), f, _ptr(gx), f, _ptr(ends), 1, f, 0, _stream())
    _call("kagnn_segment_broadcast", _ptr(zero), f, _ptr(gx), f, ctypes.c_void_p(ends.data_ptr() + 8), 1, f, 0, _stream())
    return gx


class _SegmentPoolFn(Function):
    @staticmethod
    @_on_operand_device
    def forward(ctx, x, seg, mean):
        _need_cuda(x, seg)
        x = _rows(x)
        ctx.seg, ctx.mean, ctx.n = seg, mean, x.size(0)
        return _segment_pool_raw(x, seg, mean)

    @staticmethod
    @once_differentiable
    @_on_operand_device
    def backward(ctx, gout):
        return _segment_broadcast_raw(_rows(gout), ctx.seg, ctx.n, ctx.mean), None, None


def segment_pool(x, seg_ptr, mean: bool = False) -> torch.Tensor:
    if torch.compiler.is_compiling():
        from . import library
        return library.segment_pool(x, seg_ptr, bool(mean))
    return _SegmentPoolFn.apply(x, seg_ptr, bool(mean))


# ======================================================================== dense layer (MLP baselines)
class _LinearFn(Function):
    """y = x W^T (+ b) (then ReLU): torch.nn.Linear and the torch.nn.ReLU that follows it in the reference's make_mlp chains,
    exact fp32 in every precision mode (csrc/linear.hip).  Saves x and, for the fused ReLU only, y (the mask of the backward
    is y > 0: torch's threshold_backward on the result)."""

    @staticmethod
    @_on_operand_device
    def forward(ctx, x, weight, bias, relu):
        _need_cuda(x, weight, bias)
        x = _rows(x)
        w = _rows(weight).contiguous()
        b = None if bias is None else bias.contiguous()
        n, fin = x.shape
        fout = w.size(0)
        if w.size(1) != fin or (b is not None and (b.dim() != 1 or b.numel() != fout or b.dtype != torch.float32)):
            raise ValueError(f"linear: x {tuple(x.shape)}, weight {tuple(w.shape)}, bias {None if b is None else tuple(b.shape)} do not fit")
        y = torch.empty((n, fout), dtype=torch.float32, device=x.device)
        if n > 0:
            _call("kagnn_linear_fwd", _ptr(x), _ld(x), n, fin, _ptr(w), _ptr(b), fout, int(relu), _ptr(y), fout, _stream())
        ctx.save_for_backward(x, w, y if relu else None)
        ctx.has_bias = b is not None
        return y

    @staticmethod
    @once_differentiable
    @_on_operand_device
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        gy = _rows(gy)
        n, fin = x.shape
        fout = w.size(0)
        dev = x.device
        gx = gw = gb = None
        ldy = 0 if y is None else _ld(y)
        if ctx.needs_input_grad[0]:
            gx = torch.empty((n, fin), dtype=torch.float32, device=dev)
            if n > 0:
                _call("kagnn_linear_bwd_input", _ptr(gy), _ld(gy), _ptr(y), ldy, n, fout, _ptr(w), fin, _ptr(gx), fin, _stream())
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_b:
            if n == 0:
                gw = torch.zeros((fout, fin), dtype=torch.float32, device=dev)
                gb = torch.zeros((fout,), dtype=torch.float32, device=dev) if want_b else None
            else:
                gw = torch.empty((fout, fin), dtype=torch.float32, device=dev)
                gb = torch.empty((fout,), dtype=torch.float32, device=dev) if want_b else None
                ws = _ws(_sizes("kagnn_linear_bwd_weight_workspace_bytes", n, fin, fout), dev)
                _call("kagnn_linear_bwd_weight", _ptr(x), _ld(x), _ptr(gy), _ld(gy), _ptr(y), ldy, n, fin, fout, _ptr(gw), _ptr(gb),
                      _ptr(ws), ws.numel(), _stream())
            if not ctx.needs_input_grad[1]:
                gw = None
        return gx, gw, gb, None


def linear(x, weight, bias=None, relu: bool = False) -> torch.Tensor:
    """``F.linear(x, weight, bias)``, followed by ``F.relu`` when ``relu``, as one library call each way.  x [..., in], weight
    [out, in], bias [out] or None."""
    if torch.compiler.is_compiling():
        y = torch.nn.functional.linear(x, weight, bias)
        return torch.nn.functional.relu(y) if relu else y
    if x.dim() == 2:
        return _LinearFn.apply(x, weight, bias, bool(relu))
    _need_cuda(x, weight, bias)
    y = _LinearFn.apply(x.reshape(-1, x.size(-1)), weight, bias, bool(relu))
    return y.view(*x.shape[:-1], weight.size(0))


# ======================================================================== dense attention (bias after the softmax)
def _att_rows(t: torch.Tensor, what: str):
    """``[B, R, W]`` fp32 as the kernels' ``[B * R, W]`` rows with ONE row stride: ``(tensor, ld)``.  Copies only where the
    strides cannot be described that way (a column slice of a wider matrix is passed as it is)."""
    if t.dim() != 3:
        raise ValueError(f"dense_attention: {what} must be [batch, rows, num_heads * head_dim], got shape {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise TypeError(f"kagnn_amd kernels are fp32; got {t.dtype} for {what}")
    b, r, w = t.shape
    for _ in range(2):
        ld = t.stride(1) if r > 1 else (t.stride(0) if b > 1 else w)
        if (w == 1 or t.stride(2) == 1) and ld >= w and (b <= 1 or r <= 1 or t.stride(0) == r * ld):
            return t, ld
        t = t.contiguous()
    raise AssertionError("unreachable")


class _DenseAttentionFn(Function):
    """o = (softmax_k(scale <wq, wk>) + bias) wv per head, times sigmoid(gate): csrc/attention.hip.  Saves the operands, the row
    statistics [2, B, Q, H] and the ungated o; nothing of size Q * K except the bias gradient, which is a result."""

    @staticmethod
    @_on_operand_device
    def forward(ctx, wq, wk, wv, bias, gate, num_heads, scale):
        _need_cuda(wq, wk, wv, bias, gate)
        wq, ldq = _att_rows(wq, "wq")
        wk, ldk = _att_rows(wk, "wk")
        wv, ldv = _att_rows(wv, "wv")
        B, Q, hc = wq.shape
        K = wk.size(1)
        H = int(num_heads)
        if H < 1 or hc % H or wk.shape != (B, K, hc) or wv.shape != (B, K, hc):
            raise ValueError(f"dense_attention: wq {tuple(wq.shape)}, wk {tuple(wk.shape)}, wv {tuple(wv.shape)} do not fit {H} heads")
        c = hc // H
        ldg = 0
        if gate is not None:
            gate, ldg = _att_rows(gate, "gate")
            if gate.shape != wq.shape:
                raise ValueError(f"dense_attention: gate {tuple(gate.shape)} is not wq's shape {tuple(wq.shape)}")
        bbs = brs = 0
        if bias is not None:
            if bias.dtype != torch.float32:
                raise TypeError(f"kagnn_amd kernels are fp32; got {bias.dtype} for bias")
            if bias.shape != (B, Q, K):
                raise ValueError(f"dense_attention: bias {tuple(bias.shape)} is not [batch, num_queries, num_keys] = {(B, Q, K)}")
            if K > 1 and bias.stride(2) != 1:
                bias = bias.contiguous()
            bbs, brs = (bias.stride(0) if B > 1 else 0), (bias.stride(1) if Q > 1 else 0)
        dev = wq.device
        need = any(ctx.needs_input_grad[:5])
        o = torch.empty((B, Q, hc), dtype=torch.float32, device=dev)
        stats = torch.empty((2, B, Q, H), dtype=torch.float32, device=dev) if need else None
        oung = torch.empty((B, Q, hc), dtype=torch.float32, device=dev) if need and gate is not None else None
        _call("kagnn_attention_fwd", _ptr(wq), ldq, _ptr(wk), ldk, _ptr(wv), ldv, _ptr(bias), bbs, brs, _ptr(gate), ldg, B, Q, K, H, c,
              float(scale), _ptr(o), hc, _ptr(oung), hc, _ptr(stats), _stream())
        if need:
            ctx.save_for_backward(wq, wk, wv, bias, gate, stats, o if oung is None else oung)
            ctx.dims = (B, Q, K, H, c, float(scale), ldq, ldk, ldv, ldg, bbs, brs)
        return o

    @staticmethod
    @once_differentiable
    @_on_operand_device
    def backward(ctx, gout):
        wq, wk, wv, bias, gate, stats, oung = ctx.saved_tensors
        B, Q, K, H, c, scale, ldq, ldk, ldv, ldg, bbs, brs = ctx.dims
        hc = H * c
        gout, ldgo = _att_rows(gout, "the upstream gradient")
        dev = wq.device
        g_wq = torch.empty((B, Q, hc), dtype=torch.float32, device=dev)
        g_wk = torch.empty((B, K, hc), dtype=torch.float32, device=dev)
        g_wv = torch.empty((B, K, hc), dtype=torch.float32, device=dev)
        g_bias = torch.empty((B, Q, K), dtype=torch.float32, device=dev) if bias is not None and ctx.needs_input_grad[3] else None
        g_gate = None if gate is None else torch.empty((B, Q, hc), dtype=torch.float32, device=dev)
        ws = _ws(_sizes("kagnn_attention_bwd_workspace_bytes", B, Q, K, H, c, int(gate is not None)), dev)
        _call("kagnn_attention_bwd", _ptr(gout), ldgo, _ptr(wq), ldq, _ptr(wk), ldk, _ptr(wv), ldv, _ptr(bias), bbs, brs, _ptr(gate), ldg,
              _ptr(oung), hc, _ptr(stats), B, Q, K, H, c, scale, _ptr(g_wq), hc, _ptr(g_wk), hc, _ptr(g_wv), hc, _ptr(g_bias), Q * K, K,
              _ptr(g_gate), hc, _ptr(ws), ws.numel(), _stream())
        return g_wq, g_wk, g_wv, g_bias, g_gate, None, None


def dense_attention(wq, wk, wv, num_heads: int, scale: float, bias=None, gate=None) -> torch.Tensor:
    """Multi-head attention with the bias added AFTER the softmax, the core of the reference's ``AttentionWithFastKANTransform``:
    ``o[b,q,h,:] = sum_k (softmax_k(scale <wq[b,q,h,:], wk[b,k,h,:]>) + bias[b,q,k]) wv[b,k,h,:]``, times ``sigmoid(gate)`` when a
    gate is given.  ``wq``, ``gate`` ``[B, Q, H*c]``; ``wk``, ``wv`` ``[B, K, H*c]``; ``bias`` ``[B, Q, K]`` (an ``expand``ed view is read in
    place).  ``1 <= c <= 128``.  One fused kernel each way plus the bias-gradient product: nothing of size ``Q*K`` is stored but the
    bias gradient.  Exact fp32 in every precision mode, bit-reproducible.  Gradients: ``wq, wk, wv, bias, gate``."""
    return _DenseAttentionFn.apply(wq, wk, wv, bias, gate, int(num_heads), float(scale))


# ======================================================================== efficient-KAN layer
def kan_pack_chain(layers, grid_size: int, spline_order: int, mode: int):
    """Pack the weights of all layers of a KAN chain in ONE launch (``kagnn_kan_pack_batch``): ``layers`` is a list of
    ``(base_weight, spline_weight, spline_scaler_or_None)``.  Returns ``[(pack_fwd, pack_dx, key), ...]`` to hand to
    ``kan_linear(..., packed=)``, or ``None`` when the shapes are not covered (each layer then packs itself)."""
    n = len(layers)
    if not (2 <= n <= 8) or not split_like(mode) or spline_order != 3 or grid_size + spline_order > 8:
        return None
    if any(sw.size(0) > 64 or not sw.is_cuda for _, sw, _ in layers):
        return None
    dev = layers[0][1].device
    keep, packs = [], []
    arr = lambda vals, ty: (ty * n)(*vals)
    bws, sws, scs, ins, outs, pfs, pds = [], [], [], [], [], [], []
    for bw, sw, sc in layers:
        bw_c, sw_c = bw.detach().contiguous(), sw.detach().contiguous()
        sc_c = None if sc is None else sc.detach().contiguous()
        keep += [bw_c, sw_c, sc_c]
        fout, fin = sw_c.size(0), sw_c.size(1)
        fb, db = _sizes("kagnn_kan_pack_bytes", fin, fout, grid_size, spline_order, mode, outputs=2)
        pf, pd = _ws(fb, dev), _ws(db, dev)
        packs.append((pf, pd, _weights_key(bw, sw, sc)))
        bws.append(bw_c.data_ptr()); sws.append(sw_c.data_ptr()); scs.append(0 if sc_c is None else sc_c.data_ptr())
        ins.append(fin); outs.append(fout); pfs.append(pf.data_ptr()); pds.append(pd.data_ptr())
    vp = ctypes.c_void_p
    with _device_of(layers[0][1]):
        _call("kagnn_kan_pack_batch", n, arr(bws, vp), arr(sws, vp), arr(scs, vp), arr(ins, ctypes.c_int32),
              arr(outs, ctypes.c_int32), int(grid_size), int(spline_order), int(mode), arr(pfs, vp), arr(pds, vp), _stream())
    return packs


def _weights_key(bw, sw, sc):
    return tuple((t.data_ptr(), t._version) for t in (bw, sw, sc) if t is not None)


# raw (no autograd) pieces of the KANLinear forward / backward: shared by the autograd.Function below (eager) and by the
# torch.library ops of kagnn_amd/library.py (torch.compile sees those as opaque ops)
def _kan_fwd_raw(x, bw, sw, sc, knots, grid_size, spline_order, mode, packed=None, pack_key=None, moments=False, out=None,
                 zero_pack=False):
    """-> (y, pack_dx): forward output and the input-gradient pack of the current weights; with ``moments`` also the
    column moments of y, ``(mean [out], M2 [out])`` (``kagnn_kan_linear_fwd_moments``: the BatchNorm1d statistics).
    ``zero_pack``: the bytes of pack_dx that the pack kernel skips (padding nothing reads) are 0 instead of whatever the
    allocator handed out -- for ``kagnn::kan_linear``, which RETURNS the pack: an op's output must be a function of its inputs"""
    n, fin = x.shape
    fout = sw.size(0)
    if packed is not None and packed[2] == pack_key:
        pack_f, pack_d = packed[0], packed[1]         # packed with its chain (kan_pack_chain), weights unchanged since
    else:
        fb, db = _sizes("kagnn_kan_pack_bytes", fin, fout, grid_size, spline_order, mode, outputs=2)
        pack_f, pack_d = _ws(fb, x.device), _ws(db, x.device)
        if zero_pack:
            pack_d.zero_()
        _call("kagnn_kan_pack", _ptr(bw), _ptr(sw), _ptr(sc), fin, fout, grid_size, spline_order, mode,
              _ptr(pack_f), _ptr(pack_d), _stream())
    if out is not None and (out.shape != (n, fout) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device):
        raise ValueError("out must be a contiguous fp32 [rows, out_features] tensor on the input's device")
    y = out if out is not None else torch.empty((n, fout), dtype=torch.float32, device=x.device)
    if moments:
        mom = torch.empty((2, fout), dtype=torch.float32, device=x.device)
        wb = _sizes("kagnn_kan_fwd_moments_workspace_bytes", n, fin, fout, grid_size, spline_order, mode)
        ws = _ws(wb, x.device) if wb else None
        _call("kagnn_kan_linear_fwd_moments", _ptr(x), _ld(x), n, _ptr(knots), fin, fout, grid_size, spline_order, mode,
              _ptr(pack_f), _ptr(y), fout, _ptr(mom[0]), _ptr(mom[1]), _ptr(ws), wb, _stream())
        return y, pack_d, mom
    wb = _sizes("kagnn_kan_fwd_workspace_bytes", n, fin, fout, grid_size, spline_order, mode)
    ws = _ws(wb, x.device) if wb else None
    _call("kagnn_kan_linear_fwd", _ptr(x), _ld(x), n, _ptr(knots), fin, fout, grid_size,
          spline_order, mode, _ptr(pack_f), _ptr(y), fout, _ptr(ws), wb, _stream())
    return y, pack_d


def _kan_bwd_input_raw(x, gy, knots, pack_d, fin, fout, G, K, mode, bf16_out=False, x_affine=None):
    n = x.size(0)
    gx = torch.empty((n, fin), dtype=torch.bfloat16 if bf16_out else torch.float32, device=x.device)
    if x_affine is not None:           # the layer input is x_affine[0] * x + x_affine[1] (AffineRows); gx is w.r.t. that input
        _call("kagnn_kan_linear_bwd_input_affine", _ptr(x), _ld(x), _ptr(x_affine), _ptr(gy), _ld(gy), n, _ptr(knots), fin,
              fout, G, K, mode, _ptr(pack_d), _ptr(gx), fin, _lib.DTYPE_F32, _stream())
        return gx
    _call("kagnn_kan_linear_bwd_input", _ptr(x), _ld(x), _ptr(gy), _ld(gy), n, _ptr(knots), fin,
          fout, G, K, mode, _ptr(pack_d), _ptr(gx), fin, _lib.DTYPE_BF16 if bf16_out else _lib.DTYPE_F32, _stream())
    return gx


def _kan_bwd_input_sums_raw(x, gy, knots, pack_d, fin, fout, G, K, mode, x_affine, ns):
    """``_kan_bwd_input_raw(x_affine=)`` + the two column sums of gx the folded norm's backward starts from (``ns``: its NormSums)"""
    n = x.size(0)
    gx = torch.empty((n, fin), dtype=torch.float32, device=x.device)
    sums = torch.empty((2, fin), dtype=torch.float32, device=x.device)
    wb = _sizes("kagnn_kan_bwd_input_sums_workspace_bytes", n, fin)
    ws = _ws(wb, x.device)
    _call("kagnn_kan_linear_bwd_input_affine_sums", _ptr(x), _ld(x), _ptr(x_affine), _ptr(ns.mean), _ptr(ns.rstd), _ptr(gy), _ld(gy), n,
          _ptr(knots), fin, fout, G, K, mode, _ptr(pack_d), _ptr(gx), fin, _ptr(sums), _ptr(ws), ws.numel(), _stream())
    return gx, sums


def _kan_bwd_weight_raw(x, gy, knots, sw, sc, fin, fout, G, K, mode, has_base, x_affine=None):
    n = x.size(0)
    ws = _ws(_sizes("kagnn_kan_bwd_weight_workspace_bytes", n, fin, fout, G, K, mode), x.device)
    gbw = torch.empty((fout, fin), dtype=torch.float32, device=x.device) if has_base else None
    gsw = torch.empty((fout, fin, G + K), dtype=torch.float32, device=x.device)
    gsc = None if sc is None else torch.empty((fout, fin), dtype=torch.float32, device=x.device)
    if x_affine is not None:
        _call("kagnn_kan_linear_bwd_weight_affine", _ptr(x), _ld(x), _ptr(x_affine), _ptr(gy), _ld(gy), n, _ptr(knots), fin,
              fout, G, K, mode, _ptr(sw), _ptr(sc), _ptr(gbw), _ptr(gsw), _ptr(gsc), _ptr(ws), ws.numel(), _stream())
        return gbw, gsw, gsc
    _call("kagnn_kan_linear_bwd_weight", _ptr(x), _ld(x), _ptr(gy), _ld(gy), n, _ptr(knots), fin,
          fout, G, K, mode, _ptr(sw), _ptr(sc), _ptr(gbw), _ptr(gsw), _ptr(gsc), _ptr(ws),
          ws.numel(), _stream())
    return gbw, gsw, gsc


class _OutBuffer:
    """a caller-owned destination for a forward output, hidden from autograd (see _KANLinearFn.forward)"""

    def __init__(self, t: torch.Tensor):
        self.t = t

    def view(self, n: int, f: int) -> torch.Tensor:
        if self.t.numel() < n * f or self.t.dtype != torch.float32 or not self.t.is_contiguous():
            raise ValueError("out must be a contiguous fp32 buffer of at least rows * out_features elements")
        return self.t.detach().view(-1)[: n * f].view(n, f)


class _KANLinearFn(Function):
    @staticmethod
    @_on_operand_device
    def forward(ctx, x, base_weight, spline_weight, spline_scaler, knots, grid_size, spline_order, mode, packed=None, out=None):
        _need_cuda(x, base_weight, spline_weight, spline_scaler, knots)
        x = _rows(x)
        fin = x.size(1)
        fout = spline_weight.size(0)
        bw = None if base_weight is None else base_weight.contiguous()     # None: no SiLU branch (coefficient groups)
        sw = spline_weight.contiguous()
        sc = None if spline_scaler is None else spline_scaler.contiguous()
        # out: an _OutBuffer (NOT a tensor argument: autograd must not see the caller's buffer -- e.g. a peer-mapped exchange
        # buffer -- as an input modified in place); the output is a fresh view of it made here, under the forward's no_grad
        y, pack_d = _kan_fwd_raw(x, bw, sw, sc, knots, grid_size, spline_order, mode, packed,
                                 _weights_key(base_weight, spline_weight, spline_scaler) if packed is not None else None,
                                 out=None if out is None else out.view(x.size(0), fout))
        ctx.save_for_backward(x, sw, sc, knots, pack_d)
        ctx.dims = (fin, fout, grid_size, spline_order, mode)
        ctx.has_base = bw is not None
        return y

    @staticmethod
    @once_differentiable
    @_on_operand_device
    def backward(ctx, gy):
        x, sw, sc, knots, pack_d = ctx.saved_tensors
        fin, fout, G, K, mode = ctx.dims
        gy = _rows(gy)
        gx = gbw = gsw = gsc = None
        if ctx.needs_input_grad[0]:
            gx = _kan_bwd_input_raw(x, gy, knots, pack_d, fin, fout, G, K, mode)
        if any(ctx.needs_input_grad[1:4]):
            gbw, gsw, gsc = _kan_bwd_weight_raw(x, gy, knots, sw, sc, fin, fout, G, K, mode, ctx.has_base)
        return gx, gbw, gsw, gsc, None, None, None, None, None, None


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


# ------------------------------------------------------------------------ one "aggregate + KAN chain (+ BatchNorm)" library call:
# the host side that _GinKanLayerFn, _GinKanBnLayerFn and graph_ops._GineKanLayerFn share

def _fixed_args(node) -> int:
    """how many arguments ``node.forward`` takes in front of ``*params`` (``ctx`` not counted): its backward returns that many
    gradients before the parameters', and the parameters' ``needs_input_grad`` entries start there"""
    return len(inspect.signature(node.forward).parameters) - 2


def _chain_layers(params):
    """a node's ``*params`` (``base_weight, spline_weight, spline_scaler`` per layer) -> (contiguous triples per layer, the
    chain's widths ``[in, out_0, ..., out]``)"""
    nl = len(params) // 3
    layers = [(params[3 * i].contiguous(), params[3 * i + 1].contiguous(), params[3 * i + 2].contiguous()) for i in range(nl)]
    return layers, [layers[0][1].size(1)] + [sw.size(0) for _, sw, _ in layers]


def _chain_fwd_call(name, head, n, dev, layers, widths, knots, grid_size, spline_order, mode, hub_segs, moments):
    """One chain forward entry point: allocates what it writes, then calls ``name`` with ``head`` (the arguments up to the layer
    count: the rows, the graph) and the arguments all of them end with -> (acts ``[h0, ..., y]``, input-gradient packs per layer,
    the [2, out] column moments of y or None).  ``hub_segs``: the graph's hub segments by destination and by source."""
    nl = len(layers)
    acts = [torch.empty((n, w), dtype=torch.float32, device=dev) for w in widths]
    pfs, pds = [], []
    for i in range(nl):
        fb, db = _sizes("kagnn_kan_pack_bytes", widths[i], widths[i + 1], grid_size, spline_order, mode, outputs=2)
        pfs.append(_ws(fb, dev)); pds.append(_ws(db, dev))
    warr = (ctypes.c_int32 * (nl + 1))(*widths)
    wf, _ = _sizes("kagnn_gin_kan_layer_workspace_bytes", n, nl, tuple(widths), grid_size, spline_order, mode, *hub_segs, outputs=2)
    ws = _ws(wf, dev)
    mom = torch.empty((2, widths[nl]), dtype=torch.float32, device=dev) if moments else None
    _call(name, *head, nl, warr, _ptr_array([l[0] for l in layers]), _ptr_array([l[1] for l in layers]),
          _ptr_array([l[2] for l in layers]), _ptr(knots), grid_size, spline_order, mode, _ptr_array(acts), _ptr_array(pfs),
          _ptr_array(pds), _ptr(mom[0]) if moments else None, _ptr(mom[1]) if moments else None, _ptr(ws), ws.numel(), _stream())
    return acts, pds, mom


def _chain_saved(acts, layers, pds, knots, *extras):
    """the tensors a chain node saves: per layer its input, spline weight, spline scaler and input-gradient pack; the knot
    vector; then the node's own ``extras``"""
    saved = []
    for h, (_, sw, sc), pack_d in zip(acts, layers, pds):
        saved += [h, sw, sc, pack_d]
    return (*saved, knots, *extras)


def _chain_unsaved(t, nl):
    """``_chain_saved`` read back -> (acts, sws, scs, pds, knots, extras)"""
    return t[0:4 * nl:4], t[1:4 * nl:4], t[2:4 * nl:4], t[3:4 * nl:4], t[4 * nl], t[4 * nl + 1:]


def _chain_bwd_buffers(n, dev, widths, G, K, mode, hub_segs):
    """-> (the gradients of base weight, spline weight and spline scaler per layer, the widths as int32[], the bytes of the
    chain's backward workspace)"""
    nl = len(widths) - 1
    f32 = dict(dtype=torch.float32, device=dev)
    gbw = [torch.empty((widths[i + 1], widths[i]), **f32) for i in range(nl)]
    gsw = [torch.empty((widths[i + 1], widths[i], G + K), **f32) for i in range(nl)]
    gsc = [torch.empty((widths[i + 1], widths[i]), **f32) for i in range(nl)]
    warr = (ctypes.c_int32 * (nl + 1))(*widths)
    _, wb = _sizes("kagnn_gin_kan_layer_workspace_bytes", n, nl, tuple(widths), G, K, mode, *hub_segs, outputs=2)
    return gbw, gsw, gsc, warr, wb


def _chain_bwd_result(fixed, lead, gbw, gsw, gsc):
    """what a chain node's backward returns: ``lead`` for its first forward arguments, None for the rest of the ``fixed`` ones
    (``_fixed_args``), then the parameter gradients in the order of ``*params``"""
    return (*lead, *(None,) * (fixed - len(lead)), *[t for trio in zip(gbw, gsw, gsc) for t in trio])


def _gin_chain_prepare(ctx, x, g, self_scale, grid_size, spline_order, mode, act_bf16, skip_gradient, params):
    """Forward opening of the two GIN nodes -> (the rows the aggregation gathers, layers, widths); leaves ``ctx.meta`` and
    ``ctx.skip_gradient`` for ``_gin_bwd_prepare``"""
    layers, widths = _chain_layers(params)
    xg = _rows(x, allow_bf16=True)
    if xg.size(0) != g.num_nodes:            # (the library call indexes rowptr / x by this count)
        raise ValueError(f"x has {xg.size(0)} rows but the graph has {g.num_nodes} nodes")
    if act_bf16 and xg.dtype != torch.bfloat16 and _bf16_gather_width_ok(xg.size(1)):
        xg = to_bf16_rows(xg)                # (rows the bf16 aggregation cannot take stay fp32 -- unrounded)
    if xg.dtype == torch.bfloat16 and not _bf16_rows_ok(xg):
        xg = xg.float()
    ctx.meta = (g, self_scale, grid_size, spline_order, mode, act_bf16, len(layers), x.dtype, widths)
    # a second gradient of x that another tape node (the skip-concat read-out) hands over outside the tape: this node's
    # backward adds it inside the transposed aggregation's epilogue (SkipGradient)
    ctx.skip_gradient = None
    if (skip_gradient is not None and x.requires_grad and x.dtype == torch.float32 and xg.dtype == torch.float32
            and not act_bf16):
        skip_gradient.consumer = True
        ctx.skip_gradient = skip_gradient
    return xg, layers, widths


def _take_skip_gradient(ctx, gy, fin):
    """the gradient a ``SkipGradient`` holds for this node's input (as many rows as ``gy``, ``fin`` columns), or None"""
    if ctx.skip_gradient is None:
        return None
    addend = ctx.skip_gradient.take()
    if addend is not None:
        addend = _rows(addend)
        if addend.shape != (gy.size(0), fin) or not ctx.needs_input_grad[0]:
            raise RuntimeError("SkipGradient: the gradient handed over does not belong to this convolution's input")
    return addend


def _gin_bwd_prepare(ctx, gy, addend, acts, sws, scs, pds, knots):
    """Opening of the two GIN nodes' one-call backward -> (gx or None, gbw, gsw, gsc, the bytes of the chain's workspace, ``tail``:
    the arguments ``kagnn_gin_kan_layer_bwd_add`` / ``_bwd_bn`` / ``_bwd_bn_sums`` share, from the row count to the last gradient
    pointer).  ``gx`` has the input's dtype, or fp32 at widths the bf16 kernels do not take (``_gx_as_input`` converts it)."""
    g, self_scale, G, K, mode, act_bf16, nl, x_dtype, widths = ctx.meta
    n, dev = gy.size(0), gy.device
    if n != g.num_nodes:
        raise ValueError(f"the incoming gradient has {n} rows but the graph has {g.num_nodes} nodes")
    gbw, gsw, gsc, warr, wb = _chain_bwd_buffers(n, dev, widths, G, K, mode, (g.num_hub_seg, g.num_hub_seg_t))
    gx = torch.empty((n, widths[0]), dtype=x_dtype, device=dev) if ctx.needs_input_grad[0] else None
    if gx is not None and x_dtype == torch.bfloat16 and not _bf16_rows_ok(gx):
        gx = torch.empty((n, widths[0]), dtype=torch.float32, device=dev)      # widths the bf16 kernels do not take
    tail = (n, _ptr(g.rowptr_t), _ptr(g.col_t), _ptr(g.hub_seg_t) if g.num_hub_seg_t else None, g.num_hub_seg_t, g.hub_threshold,
            float(self_scale), nl, warr, _ptr_array(sws), _ptr_array(scs), _ptr(knots), G, K, mode, _ptr_array(acts), _ptr_array(pds),
            _ptr(gx), _lib.DTYPE_BF16 if (gx is not None and gx.dtype == torch.bfloat16) else _lib.DTYPE_F32, widths[0],
            int(bool(act_bf16) and _bf16_gather_width_ok(widths[0])), _ptr(addend), _ld(addend) if addend is not None else 0,
            _ptr_array(gbw), _ptr_array(gsw), _ptr_array(gsc))
    return gx, gbw, gsw, gsc, wb, tail


def _gx_as_input(gx, x_dtype):
    return gx if gx is None or gx.dtype == x_dtype else gx.to(x_dtype)


def _gin_kan_layer_fwd_raw(xg, g, self_scale, knots, grid_size, spline_order, mode, layers, widths, moments, in_affine=None):
    """``kagnn_gin_kan_layer_fwd``: -> (acts [h0, ..., y], input-gradient packs per layer, column moments of y or None)"""
    n = xg.size(0)
    graph = (n, _ptr(g.rowptr), _ptr(g.col), _ptr(g.hub_seg) if g.num_hub_seg else None, g.num_hub_seg, g.hub_threshold,
             float(self_scale))
    if in_affine is not None:          # the gathered rows are in_affine[0] * xg + in_affine[1]: a folded BatchNorm1d (AffineRows)
        name, head = "kagnn_gin_kan_layer_fwd_affine", (_ptr(xg), _ld(xg), *graph, _ptr(in_affine[0]), _ptr(in_affine[1]))
    else:
        name, head = "kagnn_gin_kan_layer_fwd", (_ptr(xg), _lib.DTYPE_BF16 if xg.dtype == torch.bfloat16 else _lib.DTYPE_F32, _ld(xg), *graph)
    return _chain_fwd_call(name, head, n, xg.device, layers, widths, knots, grid_size, spline_order, mode,
                           (g.num_hub_seg, g.num_hub_seg_t), moments)


def _gin_kan_layer_fwd_composed(xg, g, self_scale, knots, grid_size, spline_order, mode, layers, moments):
    """``_gin_kan_layer_fwd_raw`` composed from the per-operation entry points (``KAGNN_LAYER_ABI=0``; ``knots``: per layer):
    the same kernels, the same return"""
    nl = len(layers)
    acts, pds, mom = [_aggregate_raw(xg, g, False, self_scale, None, None, None, None, False)], [], None
    packs = kan_pack_chain(layers, grid_size, spline_order, mode) if nl > 1 else None
    for i, (bw, sw, sc) in enumerate(layers):
        out = _kan_fwd_raw(acts[i], bw, sw, sc, knots[i], grid_size, spline_order, mode,
                           None if packs is None else packs[i], None if packs is None else packs[i][2],
                           moments=moments and i == nl - 1)
        acts.append(out[0]); pds.append(out[1])
        mom = out[2] if len(out) > 2 else mom
    return acts, pds, mom


def _gin_kan_layer_bwd_composed(ctx, gy, addend, acts, sws, scs, pds, knots):
    """the backward of ``_GinKanLayerFn`` composed from the per-operation entry points -> (gx, gbw, gsw, gsc)"""
    g, self_scale, G, K, mode, act_bf16, nl, x_dtype, widths = ctx.meta
    need_x = ctx.needs_input_grad[0]
    gbw, gsw, gsc = [None] * nl, [None] * nl, [None] * nl
    for i in reversed(range(nl)):
        fin, fout = widths[i], widths[i + 1]
        if any(ctx.needs_input_grad[_GIN_FIXED + 3 * i:_GIN_FIXED + 3 * i + 3]):
            gbw[i], gsw[i], gsc[i] = _kan_bwd_weight_raw(acts[i], gy, knots, sws[i], scs[i], fin, fout, G, K, mode, True)
        if i > 0 or need_x:
            bf16_out = (i == 0 and act_bf16 and split_like(mode) and K == 3 and G + K <= 8 and fout <= 128
                        and _bf16_gather_width_ok(fin) and _fits32(acts[i], fout))     # the dX variant that stores bf16 rows
            gy = _kan_bwd_input_raw(acts[i], gy, knots, pds[i], fin, fout, G, K, mode, bf16_out)
    gx = _aggregate_raw(gy, g, True, self_scale, None, None, None, None, False, out_dtype=x_dtype, addend=addend) if need_x else None
    return gx, gbw, gsw, gsc


class AffineRows:
    """A matrix that exists only as ``y * affine[0] + affine[1]`` (per-column scale and shift) -- the output of a training-mode
    ``BatchNorm1d`` whose normalising pass is folded into the kernels that read it (reference
    ``node_classification_clean/models.py:198-203``).  ``y`` is the convolution's raw output, on the tape; ``affine`` is a [2, F]
    fp32 tensor outside it.  CONVENTION: whoever consumes this object treats ``y``'s gradient slot as the gradient with respect
    to the NORMALISED rows -- the producing node (``_GinKanBnLayerFn`` in lazy mode) runs the norm's backward from there.  Only
    ``kagnn_amd.models._NodeModel.forward`` builds these, and only between nodes that follow the convention."""
    __slots__ = ("y", "affine", "stats")

    def __init__(self, y: torch.Tensor, affine: torch.Tensor, stats: Optional["NormSums"] = None):
        self.y, self.affine, self.stats = y, affine, stats     # stats: the producing norm's NormSums (or None)

    def size(self, d):
        return self.y.size(d)

    def materialise(self) -> torch.Tensor:
        """the normalised rows as an ordinary tensor (for consumers that cannot fold the affine); the gradient passes through
        unchanged, as the convention above requires"""
        return _MaterialiseAffineFn.apply(self.y, self.affine)


class NormSums:
    """Side channel between two fused convolution + norm nodes (``_GinKanBnLayerFn``), outside the tape like ``SkipGradient``:
    the backward of layer l's norm starts from two column sums of its incoming gradient g -- ``sum g`` and ``sum g * xhat`` -- which
    used to take a pass over g and the norm's input.  In the node models g is exactly what layer l+1's transposed aggregation
    writes (reference ``node_classification_clean/models.py:198-200``), so that kernel forms the sums in its epilogue
    (``kagnn_gin_kan_layer_bwd_bn_sums``).  The PRODUCING node (layer l) creates this object in its forward and fills ``mean`` /
    ``rstd``; the CONSUMING node (layer l+1) gets it with the ``AffineRows``, parks ``sums`` for the gradient tensor it returns;
    layer l's backward takes them only if the gradient it receives IS that tensor (same storage, same engine run) -- any other
    consumer of the activation makes autograd sum into a new tensor and the statistics pass runs as before."""
    __slots__ = ("mean", "rstd", "sums", "grad", "task", "version")

    def __init__(self):
        self.mean = self.rstd = self.sums = self.grad = None
        self.task = self.version = -1

    def park(self, sums: torch.Tensor, grad: torch.Tensor) -> None:
        # (holding ``grad`` keeps its storage from being reused; its version counter is recorded so that an engine that
        # accumulated another consumer's gradient INTO it in place -- same storage, new contents -- is noticed: ADVICE r04)
        self.sums, self.grad, self.task, self.version = sums, grad, graph_task_id(), grad._version

    def take(self, grad: torch.Tensor):
        sums, parked, t, ver = self.sums, self.grad, self.task, self.version
        self.sums = self.grad = None
        self.task = self.version = -1
        if sums is None or t != graph_task_id() or parked is None:
            return None
        same = (parked.data_ptr() == grad.data_ptr() and parked.shape == grad.shape and parked.stride() == grad.stride()
                and parked.dtype == grad.dtype and parked.device == grad.device
                and parked._version == ver and grad._version == ver)
        return sums if same else None


class _MaterialiseAffineFn(Function):
    @staticmethod
    def forward(ctx, y, affine):
        return torch.addcmul(affine[1], y, affine[0])

    @staticmethod
    def backward(ctx, g):
        return g, None


class _GinKanLayerFn(Function):
    """One KAN-GIN convolution -- ``KAN((1 + eps) x_i + sum_{j->i} x_j)`` -- as a single tape node over
    ``kagnn_gin_kan_layer_fwd / _bwd`` (the ``gin_kan_fused_fwd / _bwd`` of SURVEY.md 8(b)): forward = aggregation + ONE
    weight-pack launch + the chain's KANLinear forwards, backward = per layer dW / dX, then the transposed aggregation --
    one library call each way.  Saves the layer inputs only.  With ``act_bf16`` the two matrices the aggregation GATHERS
    travel as bf16: ``x`` on the way forward and ``d loss / d h0`` on the way back (written as bf16 by the
    input-gradient kernel itself, no extra pass).  ``KAGNN_LAYER_ABI=0`` composes the same kernels from the per-op entry
    points instead (bit-identical; kept for A/B)."""

    @staticmethod
    @_on_operand_device
    def forward(ctx, x, g, self_scale, knots, grid_size, spline_order, mode, act_bf16, moments, skip_gradient, *params):
        _need_cuda(x, *params)
        xg, layers, widths = _gin_chain_prepare(ctx, x, g, self_scale, grid_size, spline_order, mode, act_bf16, skip_gradient, params)
        if _LAYER_ABI:
            acts, pds, mom = _gin_kan_layer_fwd_raw(xg, g, self_scale, knots[0], grid_size, spline_order, mode, layers, widths, moments)
        else:
            acts, pds, mom = _gin_kan_layer_fwd_composed(xg, g, self_scale, knots, grid_size, spline_order, mode, layers, moments)
        ctx.save_for_backward(*_chain_saved(acts, layers, pds, knots[0]))
        if moments:
            ctx.mark_non_differentiable(mom)
            return acts[-1], mom
        return acts[-1]

    @staticmethod
    @once_differentiable
    @_on_operand_device
    def backward(ctx, gy, _g_moments=None):
        g, self_scale, G, K, mode, act_bf16, nl, x_dtype, widths = ctx.meta
        acts, sws, scs, pds, knots, _ = _chain_unsaved(ctx.saved_tensors, nl)
        gy = _rows(gy)
        addend = _take_skip_gradient(ctx, gy, widths[0])
        if not _LAYER_ABI:
            gx, gbw, gsw, gsc = _gin_kan_layer_bwd_composed(ctx, gy, addend, acts, sws, scs, pds, knots)
            return _chain_bwd_result(_GIN_FIXED, (gx,), gbw, gsw, gsc)
        gx, gbw, gsw, gsc, wb, tail = _gin_bwd_prepare(ctx, gy, addend, acts, sws, scs, pds, knots)
        ws = _ws(wb, gy.device)
        _call("kagnn_gin_kan_layer_bwd_add", _ptr(gy), _ld(gy), *tail, _ptr(ws), ws.numel(), _stream())
        return _chain_bwd_result(_GIN_FIXED, (_gx_as_input(gx, x_dtype),), gbw, gsw, gsc)


_GIN_FIXED = _fixed_args(_GinKanLayerFn)


class _GinKanBnLayerFn(Function):
    """``BatchNorm1d(KAN((1 + eps) x_i + sum_j x_j))`` in training mode -- a KAN-GIN convolution and the norm that follows it in
    every node model (reference ``node_classification_clean/models.py:198-200``) -- as ONE tape node.  Forward:
    ``kagnn_gin_kan_layer_fwd`` (column moments from the last kernel's epilogue) + the normalising pass.  Backward:
    ``kagnn_gin_kan_layer_bwd_bn`` -- the norm's statistics pass, then its element-wise backward INSIDE the last layer's
    input-gradient kernel (the rows are transformed as they are loaded and left for the weight gradient), so the separate
    normalisation-backward pass over [N, out] is gone.  Same values as the two nodes (``_GinKanLayerFn`` -> ``_BatchNormFn``)."""

    @staticmethod
    @_on_operand_device
    def forward(ctx, x, bn_weight, bn_bias, g, self_scale, knots, grid_size, spline_order, mode, act_bf16, skip_gradient, in_affine, lazy,
                in_stats, out_stats, running_mean, running_var, momentum, eps, *params):
        """``in_affine``: the input is an ``AffineRows`` (``x`` = its y): the aggregation folds the previous layer's norm.
        ``lazy``: do not write the normalised rows -- return ``(y, affine)`` for an ``AffineRows`` (see its convention).
        ``in_stats`` / ``out_stats``: the ``NormSums`` of the input ``AffineRows`` / a fresh one for the output (lazy mode)."""
        _need_cuda(x, bn_weight, bn_bias, running_mean, running_var, in_affine, *params)
        xg, layers, widths = _gin_chain_prepare(ctx, x, g, self_scale, grid_size, spline_order, mode, act_bf16, skip_gradient, params)
        acts, pds, mom = _gin_kan_layer_fwd_raw(xg, g, self_scale, knots[0], grid_size, spline_order, mode, layers, widths, True,
                                                in_affine=in_affine)
        y = acts[-1]
        affine = None
        if lazy:
            f = widths[-1]
            mean = torch.empty(f, dtype=torch.float32, device=y.device)
            rstd = torch.empty(f, dtype=torch.float32, device=y.device)
            affine = torch.empty((2, f), dtype=torch.float32, device=y.device)
            _call("kagnn_batchnorm_stats_affine", _ptr(mom[0]), _ptr(mom[1]), y.size(0), f, _ptr(bn_weight), _ptr(bn_bias),
                  _ptr(running_mean), _ptr(running_var), float(momentum), float(eps), _ptr(mean), _ptr(rstd), _ptr(affine), _stream())
        else:
            h, mean, rstd = _batchnorm_fwd_raw(y, bn_weight, bn_bias, running_mean, running_var, True, momentum, eps, mom)
        # the norms' backward statistics travel with the gradients (NormSums): this node's own, and the previous norm's that
        # this node's transposed aggregation can produce -- fp32 rows of 17..256 columns (a multiple of 4), gradient wanted
        ctx.out_stats = ctx.in_stats = None
        if _FOLD_NORM_STATS and lazy and out_stats is not None:
            out_stats.mean, out_stats.rstd = mean, rstd
            ctx.out_stats = out_stats
        extra = []
        if (_FOLD_NORM_STATS and in_affine is not None and in_stats is not None and in_stats.mean is not None and x.requires_grad
                and x.dtype == torch.float32 and xg is x and not act_bf16 and 16 < widths[0] <= 256 and widths[0] % 4 == 0
                and x.data_ptr() % 16 == 0 and _ld(x) % 4 == 0):
            ctx.in_stats = in_stats
            extra = [x]                                   # x = the previous norm's input
        ctx.save_for_backward(*_chain_saved(acts, layers, pds, knots[0], y, mean, rstd, bn_weight, *extra))
        ctx.has_bias = bn_bias is not None
        if lazy:
            ctx.mark_non_differentiable(affine)
            ctx.set_materialize_grads(False)          # (no zero-filled [2, F] "gradient" of the affine per backward: two tiny launches)
            return y, affine
        return h

    @staticmethod
    @once_differentiable
    @_on_operand_device
    def backward(ctx, gh, _g_affine=None):
        g, self_scale, G, K, mode, act_bf16, nl, x_dtype, widths = ctx.meta
        acts, sws, scs, pds, knots, (y, mean, rstd, bn_w, *norm_input) = _chain_unsaved(ctx.saved_tensors, nl)
        if gh is None:                                # (lazy mode does not materialise absent gradients: an unused output)
            gh = torch.zeros_like(y)
        gh_in = gh
        gh = _rows(gh)
        addend = _take_skip_gradient(ctx, gh, widths[0])
        gx, gbw, gsw, gsc, wb, tail = _gin_bwd_prepare(ctx, gh, addend, acts, sws, scs, pds, knots)
        n, dev = gh.size(0), gh.device
        f32 = dict(dtype=torch.float32, device=dev)
        gbn_w = torch.empty(widths[nl], **f32) if bn_w is not None else None
        gbn_b = torch.empty(widths[nl], **f32) if ctx.has_bias else None
        # statistics that came with the gradient (the next layer's aggregation made them for exactly this tensor), and the ones
        # this call makes for the previous norm
        my_sums = ctx.out_stats.take(gh_in) if ctx.out_stats is not None else None
        prev = ctx.in_stats if (ctx.in_stats is not None and gx is not None and gx.dtype == torch.float32) else None
        wbn = _sizes("kagnn_gin_kan_layer_bwd_bn_workspace_bytes", n, widths[nl])
        if my_sums is None and prev is None:
            ws = _ws(wb + wbn, dev)
            _call("kagnn_gin_kan_layer_bwd_bn", _ptr(gh), _ld(gh), _ptr(y), _ld(y), _ptr(bn_w), _ptr(mean), _ptr(rstd), _ptr(gbn_w),
                  _ptr(gbn_b), *tail, _ptr(ws), ws.numel(), _stream())
        else:
            prev_sums = prev_y = None
            wst = 0
            if prev is not None:
                prev_y = norm_input[0]
                prev_sums = torch.empty((2, widths[0]), **f32)
                wst = _sizes("kagnn_gin_kan_layer_bwd_bn_sums_workspace_bytes", n, widths[0], g.num_hub_seg_t)
            ws = _ws(wb + wbn + wst, dev)
            _call("kagnn_gin_kan_layer_bwd_bn_sums", _ptr(gh), _ld(gh), _ptr(y), _ld(y), _ptr(bn_w), _ptr(mean), _ptr(rstd), _ptr(gbn_w),
                  _ptr(gbn_b), _ptr(my_sums), _ptr(prev_y), _ld(prev_y) if prev_y is not None else 0,
                  _ptr(prev.mean) if prev is not None else None, _ptr(prev.rstd) if prev is not None else None, _ptr(prev_sums),
                  *tail, _ptr(ws), ws.numel(), _stream())
            if prev is not None:
                prev.park(prev_sums, gx)
        return _chain_bwd_result(_GIN_BN_FIXED, (_gx_as_input(gx, x_dtype), gbn_w, gbn_b), gbw, gsw, gsc)


_GIN_BN_FIXED = _fixed_args(_GinKanBnLayerFn)


_GRAPH_TASK_ID = getattr(torch._C, "_current_graph_task_id", None)


def graph_task_id() -> int:
    """id of the autograd engine run this is called from (-1 outside a backward pass; always -1 on a torch build without the
    hook: the tags below then compare equal and the objects behave as before they were tagged)"""
    return _GRAPH_TASK_ID() if _GRAPH_TASK_ID is not None else -1


class SkipGradient:
    """A gradient that travels from one tape node to another OUTSIDE the tape.  In the skip-concat node models an activation
    ``h_l`` feeds the next convolution AND the read-out (reference ``node_classification_clean/models.py:196-202``); autograd
    would materialise both gradients and add them in a pass of its own (0.12 ms per layer at 1M x 64).  Instead: the
    convolution's fused node registers as the ``consumer`` of this object in its forward; the read-out's node
    (``_KANLinearPartsFn``) -- whose backward always runs first, the convolution's output feeds it -- leaves its gradient of
    ``h_l`` in ``grad`` and reports none to the tape; the convolution's backward adds it inside the transposed aggregation's
    epilogue (``kagnn_gin_kan_layer_bwd_add``).  Bit-identical to the separate sum."""
    __slots__ = ("grad", "consumer", "task")

    def __init__(self):
        self.grad = None
        self.consumer = False
        self.task = -1                  # the engine run (graph task id) that parked ``grad``

    def park(self, grad) -> None:
        self.grad, self.task = grad, graph_task_id()

    def take(self):
        """the parked gradient if THIS backward pass parked it, else None; always leaves the object empty.  A pass that
        prunes the consumer (``backward(inputs=[...])``) leaves a parked gradient behind: a later pass must not add it to a
        loss it does not belong to -- it is dropped here instead."""
        g, t = self.grad, self.task
        self.grad, self.task = None, -1
        return g if t == graph_task_id() else None


_KNOTS_EQUAL: dict = {}


def _same_knots(layers, knots) -> bool:
    """all layers of the chain on ONE knot vector (``KAN`` hands every layer the same grid_range)?  One host comparison per
    distinct set of knot tensors, cached."""
    key = tuple((k.data_ptr(), k._version) for k in knots)
    hit = _KNOTS_EQUAL.get(key)
    if hit is None:
        hit = all(bool(torch.equal(k, knots[0])) for k in knots[1:])
        if len(_KNOTS_EQUAL) > 256:
            _KNOTS_EQUAL.clear()
        _KNOTS_EQUAL[key] = hit
    return hit


def _hook_free(mods) -> bool:
    """no hook, global or on one of ``mods`` (a hook must see a tensor the fused calls never expose): the global tables once, then the modules"""
    mod = torch.nn.modules.module
    if (mod._global_forward_hooks or mod._global_forward_pre_hooks or mod._global_backward_hooks
            or getattr(mod, "_global_backward_pre_hooks", None)):
        return False
    for m in mods:
        if m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or m._backward_pre_hooks:
            return False
    return True


def _uniform_chain(layers):
    """What a one-call node over several ``KANLinear`` layers needs of them (``_chain_plan``, ``graph_ops._gine_stack_plan``): each
    the plain layer (``KANLinear._plain_knots``) with the stand-alone spline scale, ONE precision, grid size and spline order, and --
    the library evaluates them all on ONE knot vector -- grids that ARE equal, verified: uniform but different grids (another
    grid_range, update_grid with grid_eps = 1) must not be folded onto the first layer's.  ``None``, or ``(mode, one knot vector per
    layer)``.  Reads no parameter: the stack plan runs once per step of a host-bound model."""
    precision, G, K = layers[0].precision, layers[0].grid_size, layers[0].spline_order
    knots = []
    for l in layers:
        k = l._plain_knots()
        if k is None or l.precision != precision or l.grid_size != G or l.spline_order != K or not l.enable_standalone_scale_spline:
            return None
        knots.append(k)
    if not _same_knots(layers, knots):
        return None
    return (precision if precision is not None else default_precision()), knots


def _chain_plan(layers):
    """Can the fused convolution nodes run this chain of ``KANLinear`` layers as one library call?  ``None``, or ``(mode, one knot
    vector per layer -- all equal --, the flat parameter list)``.  What ``gin_kan_layer`` and ``graph_ops.gine_kan_layer`` both
    ask: a uniform chain (``_uniform_chain``) of at most 16 coefficients within the split kernels' addressing."""
    plan = None if layers[0].grid_size + layers[0].spline_order > 16 else _uniform_chain(layers)
    if plan is None:
        return None
    mode, knots = plan
    # (gin_kan_layer's condition: the split kernels' 32-bit addressing, see _fits32; gine_kan_layer takes split-like modes only)
    if split_like(mode) and max(max(l.in_features, l.out_features) for l in layers) > 7680:
        return None
    params = []
    for l in layers:
        params += [l.base_weight, l.spline_weight, l.spline_scaler]
    return mode, knots, params


def gin_kan_layer(x, g: GraphIndex, self_scale: float, chain, act_dtype: Optional[torch.dtype] = None,
                  moments: bool = False, skip_gradient: Optional["SkipGradient"] = None, batch_norm=None,
                  in_affine: Optional[torch.Tensor] = None, lazy_norm: bool = False, in_stats: Optional["NormSums"] = None):
    """``chain(aggregate_sum(x, g, self_scale))`` for a ``kagnn_amd.KAN`` chain as ONE autograd node, or ``None`` when the
    chain is outside what the fused node covers (adaptive grids, > 16 coefficients, mixed precisions): the caller then
    composes the ops.  ``moments=True`` -> ``(y, moments)`` with the [2, out] column moments (mean, M2) of y from the
    last forward kernel's epilogue, for ``batch_norm(..., moments=...)``.
    ``batch_norm=(weight, bias, running_mean, running_var, momentum, eps)``: the training-mode BatchNorm1d that follows the
    convolution joins the node (``_GinKanBnLayerFn``: its element-wise backward runs inside the last input-gradient kernel)
    and the normalised rows are returned."""
    if layer_inputs_visible():        # a collect_edge_l1 block: the composed form, every KANLinear.forward sees its input
        return None
    if aggregation_visible():         # an edge_mask block: the aggregation runs on its own, with the mask as edge weights
        return None
    layers = list(chain.layers)
    act = default_activation_dtype() if act_dtype is None else act_dtype
    plan = _chain_plan(layers)
    if plan is None:
        return None
    mode, knots, params = plan
    first = layers[0]
    if batch_norm is not None:
        # (the library call keeps the norm's transformed rows in the chain's ping-pong gradient matrices, which are as wide as
        # the widest layer INPUT: a chain whose output is wider than every input stays on the two nodes)
        if not _LAYER_ABI or x.size(0) < 2 or layers[-1].out_features > max(l.in_features for l in layers):
            return None
        bw_, bb_, rm_, rv_, mom_, eps_ = batch_norm() if callable(batch_norm) else batch_norm      # (callable: evaluated only now that the node is certain -- the caller's per-call bookkeeping)
        out_stats = NormSums() if lazy_norm else None
        out = _GinKanBnLayerFn.apply(x, bw_, bb_, g, float(self_scale), knots, first.grid_size, first.spline_order, int(mode),
                                     act == torch.bfloat16 or x.dtype == torch.bfloat16, skip_gradient, in_affine, bool(lazy_norm),
                                     in_stats, out_stats, rm_, rv_, float(mom_), float(eps_), *params)
        return AffineRows(out[0], out[1], out_stats) if lazy_norm else out
    return _GinKanLayerFn.apply(x, g, float(self_scale), knots, first.grid_size, first.spline_order, int(mode),
                                act == torch.bfloat16 or x.dtype == torch.bfloat16, bool(moments), skip_gradient, *params)


def kan_linear(x, base_weight, spline_weight, spline_scaler, knots, grid_size: int, spline_order: int,
               mode: Optional[int] = None, packed=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = silu(x) @ base_weight.T + bases(x) @ (spline_weight*scaler).T  (ekan.py:154-162).
    ``knots`` is ONE row of the layer's grid buffer (uniform), fp32 [G+2k+1] on the device -- or the whole
    buffer [in, G+2k+1] when its rows differ / are non-uniform (after ``update_grid``): that runs the exact-fp32
    kernels on per-feature knots (``KAGNN_PREC_FP32_GRID``)."""
    if knots.dim() == 2:
        if knots.size(0) != x.size(-1):
            raise AssertionError("grid must be [in_features, G+2k+1]")
        mode = PREC_FP32_GRID
    if mode is None:
        mode = default_precision()
    if high_order(spline_order):
        # orders 5..16: the exact-fp32 kernels whatever precision was asked for (the rule of every other uncovered shape: the more
        # accurate kernels, never less), so every mode gives the same bits; never the coefficient-group split below
        if packed is not None or out is not None:
            raise ValueError("packed= and out= are not supported at spline_order above 4")
        if mode != PREC_FP32_GRID:
            mode = PREC_FP32
    if split_like(mode) and not _fits32(x, base_weight.size(0)):
        mode = PREC_FP32
    if not split_like(mode):
        packed = None                                    # chain packs are in the split kernels' layout
    n_coef = int(grid_size) + int(spline_order)
    if out is not None and ((split_like(mode) and n_coef > 16 and knots.dim() == 1) or torch.compiler.is_compiling()):
        raise ValueError("out= is not supported for layers with more than 16 coefficients or under torch.compile")
    if split_like(mode) and n_coef > 16 and knots.dim() == 1:
        # More than 16 coefficients per feature (the reference's search space goes to grid_size 32): a uniform
        # B-spline basis function only depends on its own k+2 knots, so the layer is the SUM of layers over
        # consecutive coefficient groups, each on its slice of the knot vector -- every group has <= 16 coefficients
        # and runs on the split-precision kernels (the SiLU branch rides with the first group).
        groups = -(-n_coef // 16)
        size, extra = divmod(n_coef, groups)
        y, c0 = None, 0
        one_group = _KANLinearFn.apply
        if torch.compiler.is_compiling():                 # traced code: every group is one opaque kagnn::kan_linear op
            from . import library
            one_group = lambda *a: library.kan_linear(*a)[0]
        for g in range(groups):
            cg = size + (1 if g < extra else 0)
            part = one_group(x, base_weight if g == 0 else None, spline_weight[:, :, c0:c0 + cg], spline_scaler,
                             knots[c0:c0 + cg + int(spline_order) + 1], cg - int(spline_order),
                             int(spline_order), int(mode))
            y = part if y is None else y + part
            c0 += cg
        return y
    if torch.compiler.is_compiling():
        from . import library
        return library.kan_linear(x, base_weight, spline_weight, spline_scaler, knots, int(grid_size), int(spline_order),
                                  int(mode))[0]
    return _KANLinearFn.apply(x, base_weight, spline_weight, spline_scaler, knots, int(grid_size),
                              int(spline_order), int(mode), packed, None if out is None else _OutBuffer(out))


_PARTS_OK: dict = {}
_PARTS_ONE_LAUNCH = True      # False: per-block layers summed (a module attribute for the bitwise A/B tests, no longer an environment switch)


def parts_one_launch_widths_ok(widths: tuple, fout: int, grid_size: int, spline_order: int, mode: int) -> bool:
    """block widths ``kagnn_kan_linear_fwd_parts`` covers (asked once per shape)"""
    key = (widths, fout, grid_size, spline_order, mode)
    hit = _PARTS_OK.get(key)
    if hit is None:
        hit = bool(getattr(_lib.load(), "kagnn_kan_fwd_parts_ok")((ctypes.c_int32 * len(widths))(*widths), len(widths), sum(widths),
                                                                    fout, grid_size, spline_order, mode))
        _PARTS_OK[key] = hit
    return hit


def _parts_one_launch(parts, fout: int, grid_size: int, spline_order: int, mode: int) -> bool:
    """the column blocks qualify for ``kagnn_kan_linear_fwd_parts`` (one forward launch over all of them)"""
    p0 = parts[0]
    if not all(t.is_cuda and t.dim() == 2 and t.dtype == torch.float32 and t.stride(1) == 1 and t.stride(0) % 4 == 0
               and t.size(1) <= t.stride(0) <= 7680 and t.size(0) == p0.size(0) and t.device == p0.device and t.data_ptr() % 16 == 0
               for t in parts):
        return False
    return parts_one_launch_widths_ok(tuple(int(t.size(1)) for t in parts), fout, grid_size, spline_order, mode)


class _KANLinearPartsFn(Function):
    """``KANLinear`` on ``[x_0 | x_1 | ...]`` as ONE tape node: the forward is a single launch that reads every block where
    it lies (``kagnn_kan_linear_fwd_parts``: no concatenation, no partial outputs to add up); the backward runs the
    input-gradient kernel per block that needs it and the weight-gradient kernel per block, and assembles the parameter
    gradients with one concatenation each."""

    @staticmethod
    @_on_operand_device
    def forward(ctx, base_weight, spline_weight, spline_scaler, knots, grid_size, spline_order, mode, skip_gradients, affines, norm_stats,
                *parts):
        """``affines``: ``None`` or per block ``None`` / a [2, width] tensor -- the block is read as scale * x + shift
        (``AffineRows``: a BatchNorm1d output that was never written); ``norm_stats``: ``None`` or per block ``None`` / the
        ``NormSums`` of that norm (its backward statistics can then come out of this node's input-gradient kernel)"""
        _need_cuda(base_weight, spline_weight, spline_scaler, knots, *parts)
        ctx.skip_gradients = skip_gradients
        ctx.affines = affines
        ctx.norm_stats = norm_stats
        n, fout = parts[0].size(0), spline_weight.size(0)
        widths = [int(t.size(1)) for t in parts]
        fin = sum(widths)
        bw, sw = base_weight.contiguous(), spline_weight.contiguous()
        sc = None if spline_scaler is None else spline_scaler.contiguous()
        fb, db = _sizes("kagnn_kan_pack_bytes", fin, fout, grid_size, spline_order, mode, outputs=2)
        pack_f, pack_d = _ws(fb, bw.device), _ws(db, bw.device)
        _call("kagnn_kan_pack", _ptr(bw), _ptr(sw), _ptr(sc), fin, fout, grid_size, spline_order, mode, _ptr(pack_f), _ptr(pack_d),
              _stream())
        y = torch.empty((n, fout), dtype=torch.float32, device=bw.device)
        wb = _sizes("kagnn_kan_fwd_workspace_bytes", n, fin, fout, grid_size, spline_order, mode)
        ws = _ws(wb, bw.device) if wb else None
        _call("kagnn_kan_linear_fwd_parts_affine", _ptr_array(parts), (ctypes.c_int32 * len(widths))(*widths),
              (ctypes.c_int64 * len(widths))(*[_ld(t) for t in parts]), None if affines is None else _ptr_array(list(affines)),
              len(widths), n, _ptr(knots), fin, fout, grid_size, spline_order, mode, _ptr(pack_f), _ptr(y), fout, _ptr(ws), wb, _stream())
        ctx.save_for_backward(bw, sw, sc, knots, *parts)
        ctx.dims = (widths, fout, grid_size, spline_order, mode)
        return y

    @staticmethod
    @once_differentiable
    @_on_operand_device
    def backward(ctx, gy):
        bw, sw, sc, knots, *parts = ctx.saved_tensors
        widths, fout, G, K, mode = ctx.dims
        gy = _rows(gy)
        want_w = any(ctx.needs_input_grad[0:3])
        gxs, gbws, gsws, gscs, f0 = [], [], [], [], 0
        slices = []                          # per block: contiguous (base, spline, scaler) columns, or None when nothing needs them
        npart, w0 = len(parts), widths[0]
        if npart > 1 and all(w == w0 for w in widths) and (want_w or all(ctx.needs_input_grad[10:10 + npart])):
            # equal blocks (the node models on hidden-wide inputs): ONE strided copy per parameter tensor -- [out, P, w(, C)] ->
            # [P, out, w(, C)] -- instead of one per block and tensor (12 four-microsecond launches per read-out backward)
            out_f = bw.size(0)
            bwb = bw.view(out_f, npart, w0).permute(1, 0, 2).contiguous()
            swb = sw.view(out_f, npart, w0, sw.size(2)).permute(1, 0, 2, 3).contiguous()
            scb = None if sc is None else sc.view(out_f, npart, w0).permute(1, 0, 2).contiguous()
            slices = [(bwb[i], swb[i], None if scb is None else scb[i]) for i in range(npart)]
        else:
            for i in range(npart):
                f1 = f0 + widths[i]
                if ctx.needs_input_grad[10 + i] or want_w:
                    slices.append((bw[:, f0:f1].contiguous(), sw[:, f0:f1].contiguous(), None if sc is None else sc[:, f0:f1].contiguous()))
                else:
                    slices.append(None)
                f0 = f1
        # the input-gradient packs of all blocks that need one: ONE launch when the batch entry point covers them
        need = [i for i in range(len(parts)) if ctx.needs_input_grad[10 + i]]
        packs = kan_pack_chain([slices[i] for i in need], G, K, mode) if sc is not None and len(need) >= 2 else None
        pack_of = {} if packs is None else {i: packs[k][1] for k, i in enumerate(need)}
        for i, part in enumerate(parts):
            want_x = ctx.needs_input_grad[10 + i]
            aff = None if ctx.affines is None else ctx.affines[i]
            bwp, swp, scp = slices[i] if slices[i] is not None else (None, None, None)
            gx = None
            if want_x:
                pack_d = pack_of.get(i)
                if pack_d is None:
                    fb, db = _sizes("kagnn_kan_pack_bytes", widths[i], fout, G, K, mode, outputs=2)
                    pack_f, pack_d = _ws(fb, part.device), _ws(db, part.device)
                    _call("kagnn_kan_pack", _ptr(bwp), _ptr(swp), _ptr(scp), widths[i], fout, G, K, mode, _ptr(pack_f), _ptr(pack_d),
                          _stream())
                sk = ctx.skip_gradients[i] if ctx.skip_gradients is not None else None
                handed = sk is not None and sk.consumer    # the convolution that consumed this block adds it in its own backward
                ns = None if (ctx.norm_stats is None or handed or aff is None) else ctx.norm_stats[i]
                if (ns is not None and ns.mean is not None and _FOLD_NORM_STATS and part.data_ptr() % 16 == 0
                        and getattr(_lib.load(), "kagnn_kan_bwd_input_sums_ok")(part.size(0), widths[i], fout, G, K, mode)):
                    # this gradient goes STRAIGHT to the norm whose folded output the block is (the last convolution's): the
                    # kernel also leaves the two column sums that norm's backward starts from (no statistics pass there)
                    gx, sums = _kan_bwd_input_sums_raw(part, gy, knots, pack_d, widths[i], fout, G, K, mode, aff, ns)
                    ns.park(sums, gx)
                else:
                    gx = _kan_bwd_input_raw(part, gy, knots, pack_d, widths[i], fout, G, K, mode, x_affine=aff)
                if handed:
                    sk.park(gx)
                    gx = None
            gxs.append(gx)
            if want_w:
                gbw, gsw, gsc = _kan_bwd_weight_raw(part, gy, knots, swp, scp, widths[i], fout, G, K, mode, True, x_affine=aff)
                gbws.append(gbw); gsws.append(gsw); gscs.append(gsc)
        gbw = torch.cat(gbws, dim=1) if want_w else None
        gsw = torch.cat(gsws, dim=1) if want_w else None
        gsc = torch.cat(gscs, dim=1) if want_w and sc is not None else None
        return (gbw, gsw, gsc, None, None, None, None, None, None, None, *gxs)


def parts_affine_ok(fout: int, grid_size: int, spline_order: int, parts, lazy) -> bool:
    """can the read-out kernels apply a folded BatchNorm1d to these blocks?  (``kagnn_kan_linear_*_affine``: cubic layers of
    <= 8 coefficients and <= 64 outputs; the weight-gradient kernel needs blocks wider than 32 columns)"""
    return parts_affine_widths_ok(fout, grid_size, spline_order, [int(t.size(1)) for t, z in zip(parts, lazy) if z])


def parts_affine_widths_ok(fout: int, grid_size: int, spline_order: int, lazy_widths) -> bool:
    """``parts_affine_ok`` before the blocks exist: ``lazy_widths`` are the widths of the blocks that would arrive folded"""
    return spline_order == 3 and grid_size + spline_order <= 8 and fout <= 64 and all(w > 32 for w in lazy_widths)


def kan_linear_parts(parts, base_weight, spline_weight, spline_scaler, knots, grid_size: int, spline_order: int,
                     mode: Optional[int] = None, skip_gradients=None) -> torch.Tensor:
    """``kan_linear`` on the column-concatenation of ``parts`` without building it: both branches of the layer are
    sums over input features, so the output is the sum of the layer restricted to each part's columns of the
    weights.  For the skip-concat read-out of the node models this saves the concatenation, and -- in the backward --
    the strided gradient slices that had to be copied contiguous for every branch.  Blocks the forward kernel can read
    in place (``kagnn_kan_fwd_parts_ok``) run as ONE launch and one tape node; anything else is the sum of per-block
    layers.  ``skip_gradients``: per block ``None`` or a ``SkipGradient`` whose consumer adds this layer's gradient of
    the block itself (only honoured by the one-node form; everywhere else the tape sums as usual)."""
    parts = list(parts)
    if sum(int(t.size(1)) for t in parts) != base_weight.size(1):
        raise AssertionError("parts do not add up to in_features")
    m = default_precision() if mode is None else int(mode)
    if high_order(spline_order):                         # no parts forward at these orders: write lazy blocks out and concatenate
        rows = concat_columns([t.materialise() if isinstance(t, AffineRows) else t for t in parts])
        return kan_linear(rows, base_weight, spline_weight, spline_scaler, knots, grid_size, spline_order, mode)
    lazy = [isinstance(t, AffineRows) for t in parts]
    raw = [t.y if z else t for t, z in zip(parts, lazy)]
    if (_PARTS_ONE_LAUNCH and split_like(m) and knots.dim() == 1 and len(parts) > 1 and not torch.compiler.is_compiling()
            and _parts_one_launch(raw, spline_weight.size(0), int(grid_size), int(spline_order), m)
            and (not any(lazy) or parts_affine_ok(spline_weight.size(0), int(grid_size), int(spline_order), raw, lazy))):
        sk = None if skip_gradients is None or not any(k is not None and k.consumer for k in skip_gradients) else tuple(skip_gradients)
        affines = tuple(t.affine if z else None for t, z in zip(parts, lazy)) if any(lazy) else None
        stats = tuple(t.stats if z else None for t, z in zip(parts, lazy)) if any(lazy) else None
        return _KANLinearPartsFn.apply(base_weight, spline_weight, spline_scaler, knots, int(grid_size), int(spline_order), m, sk,
                                       affines, stats, *raw)
    parts = [t.materialise() if z else t for t, z in zip(parts, lazy)]        # (blocks no kernel folds: write them out)
    y, f0 = None, 0
    for part in parts:
        f1 = f0 + part.size(1)
        sc = None if spline_scaler is None else spline_scaler[:, f0:f1]
        out = kan_linear(part, base_weight[:, f0:f1], spline_weight[:, f0:f1], sc, knots, grid_size, spline_order, mode)
        y = out if y is None else y + out
        f0 = f1
    return y


def kan_bsplines(x, grid, grid_size: int, spline_order: int) -> torch.Tensor:
    """Dense B-spline bases ``[N, in, G+k]`` of ``x[N, in]`` on the per-feature knot rows ``grid[in, G+2k+1]``
    (``KANLinear.b_splines``, ekan.py:79-112).  Not differentiable (the layer never stores this tensor)."""
    _need_cuda(x, grid)
    x = _rows(x.detach())
    g = grid.detach().to(torch.float32).contiguous()
    n, fin = x.shape
    if g.shape != (fin, grid_size + 2 * spline_order + 1):
        raise AssertionError("grid must be [in_features, G+2k+1]")
    out = torch.empty((n, fin, grid_size + spline_order), dtype=torch.float32, device=x.device)
    with _device_of(x):
        _call("kagnn_kan_bsplines", _ptr(x), _ld(x), n, _ptr(g), fin, int(grid_size), int(spline_order), _ptr(out),
              _stream())
    return out


def kan_grid_refit(x, grid_old, grid_new, spline_weight, spline_scaler, grid_size: int,
                   spline_order: int) -> torch.Tensor:
    """Coefficients on ``grid_new`` that reproduce, in the least-squares sense over the rows of ``x``, the
    per-feature curves the layer had on ``grid_old`` (the refit inside ``update_grid``, ekan.py:169-177,211):
    ``kan_grid_resize`` between two grids of one size, every row taking part."""
    return kan_grid_resize(x, grid_old, grid_new, spline_weight, spline_scaler, grid_size, grid_size, spline_order, window=None)[0]


MAX_KNOTS = 48                     # grid_size + 2 * spline_order + 1 at orders 1..4 (kMaxKnots of the kernels)


def kan_grid_resize(x, grid_old, grid_new, spline_weight, spline_scaler, grid_size_old: int, grid_size_new: int,
                    spline_order: int, window=None):
    """The least-squares coefficient refit between grids of TWO sizes (grid extension: a coarse grid's curves moved onto a finer one,
    or back; ``kan_grid_refit`` is the equal-size case):
    ``grid_old [in, G_old+2k+1]``, ``grid_new [in, G_new+2k+1]``, ``spline_weight [out, in, G_old+k]``; returns
    ``(new_spline_weight [out, in, G_new+k], untouched [in] int32)``.  ``window [in, 2]``: row ``n`` takes part in feature ``f``'s
    fit only when ``window[f, 0] <= x[n, f] < window[f, 1]``.  ``untouched[f]``: the new bases of feature ``f`` no participating
    row reached (their coefficients are 0).  Orders 1..4, ``G + 2k + 1 <= 48`` on either side."""
    g0, g1, k = int(grid_size_old), int(grid_size_new), int(spline_order)
    if high_order(k) or k < 1:
        raise NotImplementedError(f"kan_grid_resize: spline_order must be in 1..{FUSED_MAX_SPLINE_ORDER} (got {spline_order})")
    for g in (g0, g1):
        if g < 1 or g + 2 * k + 1 > MAX_KNOTS:
            raise ValueError(f"kan_grid_resize: grid_size must be >= 1 with grid_size + 2 * spline_order + 1 <= {MAX_KNOTS} (got {g} at order {k})")
    _need_cuda(x, grid_old, grid_new, spline_weight, spline_scaler, window)
    x = _rows(x.detach())
    n, fin = x.shape
    fout = spline_weight.size(0)
    if n < 1:
        raise ValueError("kan_grid_resize: no rows to fit on")
    go = grid_old.detach().to(torch.float32).contiguous()
    gn = grid_new.detach().to(torch.float32).contiguous()
    if go.shape != (fin, g0 + 2 * k + 1) or gn.shape != (fin, g1 + 2 * k + 1):
        raise AssertionError("grids must be [in_features, G+2k+1]")
    if tuple(spline_weight.shape) != (fout, fin, g0 + k):
        raise AssertionError("spline_weight must be [out_features, in_features, G_old+k]")
    sw = spline_weight.detach().to(torch.float32).contiguous()
    sc = None if spline_scaler is None else spline_scaler.detach().to(torch.float32).contiguous()
    win = None if window is None else window.detach().to(torch.float32).contiguous()
    if win is not None and win.shape != (fin, 2):
        raise AssertionError("window must be [in_features, 2]")
    ws = _ws(_sizes("kagnn_kan_grid_resize_workspace_bytes", n, fin, g0, g1, k), x.device)
    out = torch.empty((fout, fin, g1 + k), dtype=torch.float32, device=x.device)
    untouched = torch.empty((fin,), dtype=torch.int32, device=x.device)
    with _device_of(x):
        _call("kagnn_kan_grid_resize", _ptr(x), _ld(x), n, _ptr(go), _ptr(gn), _ptr(win), fin, fout, g0, g1, k, _ptr(sw), _ptr(sc),
              _ptr(out), _ptr(untouched), _ptr(ws), ws.numel(), _stream())
    return out, untouched


# ======================================================================== per-edge activations (kan_edge.hip)
# phi_{o,i}(t) = base_weight[o,i] silu(t) + spline_scaler[o,i] sum_c spline_weight[o,i,c] B_c(t): what a KAN user inspects and
# regularises.  Exact fp32 in every precision mode; spline orders 1..FUSED_MAX_SPLINE_ORDER.

_EDGE_STATE = threading.local()      # .collectors: the calling thread's active kagnn_amd.collect_edge_l1 blocks, innermost last


def _edge_collectors() -> list:
    """the collect_edge_l1 blocks open on THIS thread (a block opened by another thread -- a replica, a loader thread running a
    model -- neither changes this thread's routing nor receives its statistics)"""
    got = getattr(_EDGE_STATE, "collectors", None)
    if got is None:
        got = _EDGE_STATE.collectors = []
    return got


def layer_inputs_visible() -> bool:
    """True inside a ``kagnn_amd.collect_edge_l1`` block of the calling thread: every route that hides a KANLinear's input from ``KANLinear.forward``
    (the fused layer / stack / model nodes, the chain pack, the concatenation-free read-out) then takes its composed
    per-layer form, so each layer sees -- and can take statistics of -- its own input."""
    return bool(getattr(_EDGE_STATE, "collectors", None)) or getattr(_EDGE_STATE, "refine", None) is not None


def _refine_walk():
    """the ``kagnn_amd.refine_grids`` walk open on THIS thread, or None.  While one is open ``layer_inputs_visible()`` holds, exactly
    as inside a ``collect_edge_l1`` block: every KANLinear.forward sees its own input and refines itself on it first."""
    return getattr(_EDGE_STATE, "refine", None)


def _set_refine_walk(walk) -> None:
    _EDGE_STATE.refine = walk


def edge_mask_of(g: Optional[GraphIndex] = None):
    """the mask of the ``kagnn_amd.edge_mask`` block open on THIS thread, or None.  With the graph a convolution is about to
    aggregate over: checked against its edge count."""
    mask = getattr(_EDGE_STATE, "mask", None)
    if mask is not None and g is not None and mask.numel() != g.num_edges:
        raise ValueError(f"edge_mask: the mask has {mask.numel()} entries but this convolution's graph has {g.num_edges} edges")
    return mask


def _set_edge_mask(mask) -> None:
    _EDGE_STATE.mask = mask


def aggregation_visible() -> bool:
    """True inside a ``kagnn_amd.edge_mask`` block of the calling thread -- the sibling of ``layer_inputs_visible()``: every route
    that hides a convolution's aggregation step (the fused ``gin_kan_layer`` node with or without its norm, the lazy-norm
    ``AffineRows`` form whose folded aggregation is unit-weight only) then takes its per-operation form, so the step runs as
    ``aggregate_sum(..., edge_weight=mask)``."""
    return getattr(_EDGE_STATE, "mask", None) is not None


def gcn_norm_weights(edge_index: torch.Tensor, edge_weight: torch.Tensor, num_nodes: int):
    """``(graph, w_hat)``: the augmented edge list of ``WeightedGcnGraph`` (non-loop edges, then one self loop per node -- an
    existing loop keeps its weight, otherwise 1) and its normalised weights ``w_hat[e] = dis[src] * w[e] * dis[dst]``,
    ``dis = deg^-1/2`` (inf -> 0) of the weighted in-degree, in differentiable torch ops: the form ``_NormalisedConv`` takes for
    weights that require a gradient, which then reaches them through the message AND the degrees, as in torch_geometric's
    ``gcn_norm``.  Only the index of the augmented list (weight-independent) comes from the per-``edge_index`` cache."""
    _need_cuda(edge_index, edge_weight)
    if edge_weight.shape != (edge_index.size(1),):
        raise ValueError(f"edge_weight must be [{edge_index.size(1)}], got {tuple(edge_weight.shape)}")
    src, dst = edge_index[0], edge_index[1]
    w = edge_weight.to(torch.float32)
    keep = src != dst
    loop_w = torch.ones(num_nodes, dtype=torch.float32, device=w.device).index_put((src[~keep],), w[~keep])
    wa = torch.cat([w[keep], loop_w])
    ar = torch.arange(num_nodes, dtype=src.dtype, device=src.device)
    a_src, a_dst = torch.cat([src[keep], ar]), torch.cat([dst[keep], ar])
    deg = torch.zeros(num_nodes, dtype=torch.float32, device=w.device).index_add(0, a_dst, wa)
    dis = deg.pow(-0.5)
    dis = torch.where(torch.isinf(dis), torch.zeros_like(dis), dis)
    return weighted_gcn_graph(edge_index, None, num_nodes).graph, dis[a_src] * wa * dis[a_dst]


def _edge_operands(what, rows, base_weight, spline_weight, spline_scaler, knots, grid_size, spline_order):
    if high_order(spline_order) or int(spline_order) < 1:
        raise NotImplementedError(f"{what}: spline_order must be in 1..{FUSED_MAX_SPLINE_ORDER} (got {spline_order}); the per-edge "
                                  "activation kernels do not cover the orders above")
    _need_cuda(rows, base_weight, spline_weight, spline_scaler, knots)
    fout, fin, coef = spline_weight.shape
    if coef != int(grid_size) + int(spline_order):
        raise AssertionError("spline_weight must be [out_features, in_features, G+k]")
    kn = knots.detach().to(torch.float32).contiguous()
    if kn.dim() == 2 and kn.size(0) != fin or kn.size(-1) != int(grid_size) + 2 * int(spline_order) + 1:
        raise AssertionError("knots must be [G+2k+1] or [in_features, G+2k+1]")
    bw = None if base_weight is None else base_weight.detach().contiguous()
    sw = spline_weight.detach().contiguous()
    sc = None if spline_scaler is None else spline_scaler.detach().contiguous()
    for t in (bw, sw, sc):
        if t is not None and t.dtype != torch.float32:
            raise TypeError(f"kagnn_amd kernels are fp32; got {t.dtype}")
    if (bw is not None and bw.shape != (fout, fin)) or (sc is not None and sc.shape != (fout, fin)):
        raise AssertionError("base_weight / spline_scaler must be [out_features, in_features]")
    return bw, sw, sc, kn, int(kn.dim() == 2), fin, fout


def _kan_edge_abs_sum_raw(x, bw, sw, sc, kn, pf, fin, fout, G, K, out=None):
    n = x.size(0)
    S = torch.empty((fout, fin), dtype=torch.float32, device=x.device) if out is None else out
    ws = _ws(_sizes("kagnn_kan_edge_abs_sum_workspace_bytes", n, fin, fout, G, K), x.device)
    _call("kagnn_kan_edge_abs_sum", _ptr(x), _ld(x), n, _ptr(kn), pf, fin, fout, G, K, _ptr(bw), _ptr(sw), _ptr(sc), _ptr(S),
          _ld(S) if out is not None else fin, _ptr(ws), ws.numel(), _stream())
    return S


def _kan_edge_abs_sum_bwd_raw(x, bw, sw, sc, kn, pf, fin, fout, G, K, gS, want_bw, want_sw, want_sc, want_x):
    n = x.size(0)
    dev = x.device
    gbw = torch.empty((fout, fin), dtype=torch.float32, device=dev) if want_bw and bw is not None else None
    gsw = torch.empty((fout, fin, G + K), dtype=torch.float32, device=dev) if want_sw else None
    gsc = torch.empty((fout, fin), dtype=torch.float32, device=dev) if want_sc and sc is not None else None
    gx = torch.empty((n, fin), dtype=torch.float32, device=dev) if want_x else None
    ws = None
    if gbw is not None or gsw is not None or gsc is not None:
        ws = _ws(_sizes("kagnn_kan_edge_abs_sum_bwd_workspace_bytes", n, fin, fout, G, K), dev)
    _call("kagnn_kan_edge_abs_sum_bwd", _ptr(x), _ld(x), n, _ptr(kn), pf, fin, fout, G, K, _ptr(bw), _ptr(sw), _ptr(sc), _ptr(gS),
          _ld(gS), _ptr(gbw), _ptr(gsw), _ptr(gsc), _ptr(gx), fin, _ptr(ws), 0 if ws is None else ws.numel(), _stream())
    return gbw, gsw, gsc, gx


class _KanEdgeAbsSumFn(Function):
    """``S[o,i] = sum_n |phi_{o,i}(x[n,i])|``.  Saves the rows and the parameters, not phi: the backward evaluates it again."""

    @staticmethod
    @_on_operand_device
    def forward(ctx, x, base_weight, spline_weight, spline_scaler, knots, grid_size, spline_order):
        bw, sw, sc, kn, pf, fin, fout = _edge_operands("kan_edge_abs_sum", x, base_weight, spline_weight, spline_scaler, knots,
                                                       grid_size, spline_order)
        x = _rows(x.detach())
        if x.size(1) != fin:
            raise AssertionError("x must be [rows, in_features]")
        ctx.save_for_backward(x, bw, sw, sc, kn)
        ctx.dims = (pf, fin, fout, int(grid_size), int(spline_order))
        return _kan_edge_abs_sum_raw(x, bw, sw, sc, kn, pf, fin, fout, int(grid_size), int(spline_order))

    @staticmethod
    @once_differentiable
    @_on_operand_device
    def backward(ctx, gS):
        x, bw, sw, sc, kn = ctx.saved_tensors
        pf, fin, fout, G, K = ctx.dims
        need = ctx.needs_input_grad
        gbw, gsw, gsc, gx = _kan_edge_abs_sum_bwd_raw(x, bw, sw, sc, kn, pf, fin, fout, G, K, _rows(gS), need[1], need[2], need[3],
                                                      need[0])
        return gx, gbw, gsw, gsc, None, None, None


def kan_edge_abs_sum(x, base_weight, spline_weight, spline_scaler, knots, grid_size: int, spline_order: int) -> torch.Tensor:
    """``S[out, in] = sum_n |phi_{o,i}(x[n,i])|`` -- the per-edge activation magnitude the KAN regulariser is defined on, as a
    SUM over the rows (sums over a partition of the rows add; ``KANLinear.edge_l1`` divides by the row count).  ``knots`` as
    for ``kan_linear``: one row [G+2k+1] or the whole grid buffer [in, G+2k+1].  ``base_weight`` / ``spline_scaler`` may be
    ``None``.  Differentiable in the three parameters and ``x``; nothing of size [N, out, in] (or [N, out]) is stored."""
    return _KanEdgeAbsSumFn.apply(x, base_weight, spline_weight, spline_scaler, knots, int(grid_size), int(spline_order))


def kan_edge_moments(x, base_weight, spline_weight, spline_scaler, knots, grid_size: int, spline_order: int, out=None):
    """``(mean, m2)``, both ``[out, in]``: ``mean[o,i] = mean_n phi_{o,i}(x[n,i])`` and the centred sum of squares
    ``m2[o,i] = sum_n (phi_{o,i}(x[n,i]) - mean[o,i])^2`` -- a SUM, so the caller chooses the divisor, and results over a partition
    of the rows merge pairwise.  Operands as for ``kan_edge_abs_sum``.  Accumulated about a pivot row (an edge on a large offset
    keeps its scale); exact fp32; the same inputs give the same bits.  Not differentiable.  ``out = (mean, m2)``: row-strided
    [out, in] views to write into."""
    bw, sw, sc, kn, pf, fin, fout = _edge_operands("kan_edge_moments", x, base_weight, spline_weight, spline_scaler, knots, grid_size,
                                                   spline_order)
    x = _rows(x.detach())
    if x.size(1) != fin:
        raise AssertionError("x must be [rows, in_features]")
    n, G, K = x.size(0), int(grid_size), int(spline_order)
    mean, m2 = out if out is not None else (torch.empty((fout, fin), dtype=torch.float32, device=x.device) for _ in range(2))
    for t in (mean, m2):                          # (the kernel writes [out, in] blocks with a row stride and unit column stride)
        if t.shape != (fout, fin) or t.dtype != torch.float32 or t.device != x.device or t.stride(1) != 1 or (fout > 1 and t.stride(0) < fin):
            raise AssertionError("kan_edge_moments: out must be two fp32 [out_features, in_features] views on x's device with unit column stride")
    with _device_of(x):
        ws = _ws(_sizes("kagnn_kan_edge_moments_workspace_bytes", n, fin, fout, G, K), x.device)
        _call("kagnn_kan_edge_moments", _ptr(x), _ld(x), n, _ptr(kn), pf, fin, fout, G, K, _ptr(bw), _ptr(sw), _ptr(sc), _ptr(mean),
              _ld(mean), _ptr(m2), _ld(m2), _ptr(ws), ws.numel(), _stream())
    return mean, m2


def kan_edge_curves(points, base_weight, spline_weight, spline_scaler, knots, grid_size: int, spline_order: int) -> torch.Tensor:
    """``phi[P, out, in]``: every edge function sampled at ``points`` -- ``[P]`` (the same abscissae for every input feature)
    or ``[P, in]``.  Not differentiable."""
    bw, sw, sc, kn, pf, fin, fout = _edge_operands("kan_edge_curves", points, base_weight, spline_weight, spline_scaler, knots,
                                                   grid_size, spline_order)
    t = points.detach()
    if t.dtype != torch.float32:
        raise TypeError(f"kagnn_amd kernels are fp32; got {t.dtype}")
    if t.dim() == 1:
        t, ldt = t.contiguous(), 0
    elif t.dim() == 2 and t.size(1) == fin:
        t = _rows(t)
        ldt = _ld(t)
    else:
        raise AssertionError("points must be [P] or [P, in_features]")
    out = torch.empty((t.size(0), fout, fin), dtype=torch.float32, device=t.device)
    with _device_of(t):
        _call("kagnn_kan_edge_curves", _ptr(t), ldt, t.size(0), _ptr(kn), pf, fin, fout, int(grid_size), int(spline_order), _ptr(bw),
              _ptr(sw), _ptr(sc), _ptr(out), _stream())
    return out


# ======================================================================== FastKAN layer
def _fastkan_fwd_raw(x, ln_w, ln_b, spline_w, base_w, base_b, centers, denominator, ln_eps, mode):
    """-> (y, row_stats or None)"""
    n, fin = x.shape
    fout = spline_w.size(0)
    ng = centers.numel()
    if spline_w.size(1) != fin * ng:
        raise AssertionError("spline_linear.weight must be [out, in*num_grids]")
    sw = spline_w.contiguous()
    lw = None if ln_w is None else ln_w.contiguous()
    lb = None if ln_b is None else ln_b.contiguous()
    bw = None if base_w is None else base_w.contiguous()
    bb = None if base_b is None else base_b.contiguous()
    ws = _ws(_sizes("kagnn_fastkan_fwd_workspace_bytes", n, fin, fout, ng, mode), x.device)
    stats = torch.empty((n, 2), dtype=torch.float32, device=x.device) if lw is not None else None
    y = torch.empty((n, fout), dtype=torch.float32, device=x.device)
    _call("kagnn_fastkan_fwd", _ptr(x), _ld(x), n, fin, fout, ng, _ptr(centers), float(denominator),
          _ptr(lw), _ptr(lb), float(ln_eps), _ptr(sw), _ptr(bw), _ptr(bb), _ptr(y), fout,
          _ptr(stats), mode, _ptr(ws), ws.numel(), _stream())
    return y, stats


def _fastkan_bwd_raw(x, gy, ln_w, ln_b, spline_w, base_w, centers, stats, denominator, ln_eps, mode):
    """-> (gx, g_ln_weight, g_ln_bias, g_spline_weight, g_base_weight, g_base_bias); absent ones are None"""
    n, fin = x.shape
    fout = spline_w.size(0)
    ng = centers.numel()
    dev = x.device
    sw = spline_w.contiguous()
    lw = None if ln_w is None else ln_w.contiguous()
    lb = None if ln_b is None else ln_b.contiguous()
    bw = None if base_w is None else base_w.contiguous()
    ws = _ws(_sizes("kagnn_fastkan_bwd_workspace_bytes", n, fin, fout, ng, mode), dev)
    f32 = dict(dtype=torch.float32, device=dev)
    gx = torch.empty((n, fin), **f32)
    glw = torch.empty(fin, **f32) if lw is not None else None
    glb = torch.empty(fin, **f32) if lw is not None else None
    gsw = torch.empty((fout, fin * ng), **f32)
    gbw = torch.empty((fout, fin), **f32) if bw is not None else None
    gbb = torch.empty(fout, **f32) if bw is not None else None
    _call("kagnn_fastkan_bwd", _ptr(x), _ld(x), _ptr(gy), _ld(gy), n, fin, fout, ng, _ptr(centers), float(denominator),
          _ptr(lw), _ptr(lb), float(ln_eps), _ptr(sw), _ptr(bw), _ptr(stats), _ptr(gx), fin, _ptr(glw),
          _ptr(glb), _ptr(gsw), _ptr(gbw), _ptr(gbb), mode, _ptr(ws), ws.numel(), _stream())
    return gx, glw, glb, gsw, gbw, gbb


class _FastKANFn(Function):
    @staticmethod
    @_on_operand_device
    def forward(ctx, x, ln_w, ln_b, spline_w, base_w, base_b, centers, denominator, ln_eps, mode):
        _need_cuda(x, spline_w, centers)
        x = _rows(x)
        y, stats = _fastkan_fwd_raw(x, ln_w, ln_b, spline_w, base_w, base_b, centers, denominator, ln_eps, mode)
        ctx.save_for_backward(x, ln_w, ln_b, spline_w, base_w, centers, stats)
        ctx.meta = (float(denominator), float(ln_eps), base_b is not None, mode)
        return y

    @staticmethod
    @once_differentiable
    @_on_operand_device
    def backward(ctx, gy):
        x, lw, lb, sw, bw, centers, stats = ctx.saved_tensors
        den, eps, has_bb, mode = ctx.meta
        gx, glw, glb, gsw, gbw, gbb = _fastkan_bwd_raw(x, _rows(gy), lw, lb, sw, bw, centers, stats, den, eps, mode)
        return gx, glw, glb, gsw, gbw, (gbb if has_bb else None), None, None, None, None


# ------------------------------------------------------------------------ per-edge activations of a FastKAN layer (fastkan_edge.hip)
# phi_{o,i}(n) = sum_g spline_weight[o, i*G+g] exp(-((u[n,i] - c_g) / h)^2) + base_weight[o,i] silu(x[n,i]),  u = LayerNorm(x) or x:
# the FastKAN twin of kan_edge_abs_sum / kan_edge_curves above.  Exact fp32 in every precision mode.
def _fastkan_edge_operands(ln_weight, ln_bias, spline_weight, base_weight, centers, *rows):
    _need_cuda(*rows, ln_weight, ln_bias, spline_weight, base_weight, centers)
    if (ln_weight is None) != (ln_bias is None):
        raise AssertionError("layernorm weight and bias must both be given or both be None")
    c = centers.detach().to(torch.float32).contiguous()
    ng = c.numel()
    ts = [None if t is None else t.detach().contiguous() for t in (ln_weight, ln_bias, spline_weight, base_weight)]
    for t in ts:
        if t is not None and t.dtype != torch.float32:
            raise TypeError(f"kagnn_amd kernels are fp32; got {t.dtype}")
    lw, lb, sw, bw = ts
    if sw is not None and (sw.dim() != 2 or sw.size(1) % max(ng, 1)):
        raise AssertionError("spline_linear.weight must be [out, in*num_grids]")
    if sw is None and bw is None:
        raise AssertionError("neither spline_weight nor base_weight is given")
    fout, fin = (bw.size(0), bw.size(1)) if bw is not None else (sw.size(0), sw.size(1) // ng)
    if (sw is not None and sw.shape != (fout, fin * ng)) or (lw is not None and (lw.shape != (fin,) or lb.shape != (fin,))):
        raise AssertionError("spline_weight must be [out, in*num_grids], base_weight [out, in], layernorm weight and bias [in]")
    return lw, lb, sw, bw, c, ng, fin, fout


def _fastkan_edge_abs_sum_raw(x, lw, lb, sw, bw, c, ng, fin, fout, denominator, ln_eps, out=None):
    n = x.size(0)
    S = torch.empty((fout, fin), dtype=torch.float32, device=x.device) if out is None else out
    ws = _ws(_sizes("kagnn_fastkan_edge_abs_sum_workspace_bytes", n, fin, fout, ng, int(lw is not None)), x.device)
    _call("kagnn_fastkan_edge_abs_sum", _ptr(x), _ld(x), n, fin, fout, ng, _ptr(c), float(denominator), _ptr(lw), _ptr(lb),
          float(ln_eps), _ptr(sw), _ptr(bw), _ptr(S), _ld(S) if out is not None else fin, _ptr(ws), ws.numel(), _stream())
    return S


def _fastkan_edge_abs_sum_bwd_raw(x, lw, lb, sw, bw, c, ng, fin, fout, denominator, ln_eps, gS, want_sw, want_bw, want_x):
    """-> (g_spline_weight, g_base_weight, gx, g_ln_weight, g_ln_bias); with a layernorm the last three come together"""
    n, dev = x.size(0), x.device
    f32 = dict(dtype=torch.float32, device=dev)
    gsw = torch.empty((fout, fin * ng), **f32) if want_sw else None
    gbw = torch.empty((fout, fin), **f32) if want_bw and bw is not None else None
    gx = torch.empty((n, fin), **f32) if want_x else None
    glw = torch.empty(fin, **f32) if want_x and lw is not None else None
    glb = torch.empty(fin, **f32) if want_x and lw is not None else None
    ws = _ws(_sizes("kagnn_fastkan_edge_abs_sum_bwd_workspace_bytes", n, fin, fout, ng, int(lw is not None)), dev)
    _call("kagnn_fastkan_edge_abs_sum_bwd", _ptr(x), _ld(x), n, fin, fout, ng, _ptr(c), float(denominator), _ptr(lw), _ptr(lb),
          float(ln_eps), _ptr(sw), _ptr(bw), _ptr(gS), _ld(gS), _ptr(gsw), _ptr(gbw), _ptr(gx), fin, _ptr(glw), _ptr(glb), _ptr(ws),
          ws.numel(), _stream())
    return gsw, gbw, gx, glw, glb


class _FastKANEdgeAbsSumFn(Function):
    """``S[o,i] = sum_n |phi_{o,i}(n)|``.  Saves the rows and the parameters, not phi: the backward evaluates it again."""

    @staticmethod
    @_on_operand_device
    def forward(ctx, x, ln_weight, ln_bias, spline_weight, base_weight, centers, denominator, ln_eps):
        if spline_weight is None:
            raise AssertionError("fastkan_edge_abs_sum needs spline_weight")
        lw, lb, sw, bw, c, ng, fin, fout = _fastkan_edge_operands(ln_weight, ln_bias, spline_weight, base_weight, centers, x)
        x = _rows(x.detach())
        if x.size(1) != fin:
            raise AssertionError("x must be [rows, input_dim]")
        ctx.save_for_backward(x, lw, lb, sw, bw, c)
        ctx.dims = (ng, fin, fout, float(denominator), float(ln_eps))
        return _fastkan_edge_abs_sum_raw(x, lw, lb, sw, bw, c, ng, fin, fout, denominator, ln_eps)

    @staticmethod
    @once_differentiable
    @_on_operand_device
    def backward(ctx, gS):
        x, lw, lb, sw, bw, c = ctx.saved_tensors
        ng, fin, fout, den, eps = ctx.dims
        need = ctx.needs_input_grad
        want_x = need[0] or (lw is not None and (need[1] or need[2]))
        gsw, gbw, gx, glw, glb = _fastkan_edge_abs_sum_bwd_raw(x, lw, lb, sw, bw, c, ng, fin, fout, den, eps, _rows(gS), need[3], need[4],
                                                               want_x)
        return (gx if need[0] else None), (glw if need[1] else None), (glb if need[2] else None), gsw, gbw, None, None, None


def fastkan_edge_abs_sum(x, ln_weight, ln_bias, spline_weight, base_weight, centers, denominator: float,
                         ln_eps: float = 1e-5) -> torch.Tensor:
    """``S[out, in] = sum_n |phi_{o,i}(n)|`` of a FastKAN layer -- the per-edge activation magnitude the KAN regulariser is defined
    on, as a SUM over the rows (sums over a partition of the rows add; ``FastKANLayer.edge_l1`` divides by the row count).
    ``ln_weight`` / ``ln_bias`` ``None``: no LayerNorm in front of the RBFs; ``base_weight`` ``None``: no base branch.
    Differentiable in ``x``, both LayerNorm parameters and both weights; nothing of size [N, out, in] (or [N, out]) is stored."""
    return _FastKANEdgeAbsSumFn.apply(x, ln_weight, ln_bias, spline_weight, base_weight, centers, float(denominator), float(ln_eps))


def _edge_points(t, fin, what):
    """-> (points with unit column stride, ld or 0 for one shared column)"""
    if t.dtype != torch.float32:
        raise TypeError(f"kagnn_amd kernels are fp32; got {t.dtype}")
    t = t.detach()
    if t.dim() == 1:
        return t.contiguous(), 0
    if t.dim() == 2 and t.size(1) == fin:
        t = _rows(t)
        return t, _ld(t)
    raise AssertionError(f"{what} must be [P] or [P, input_dim]")


def fastkan_edge_curves(points, spline_weight, base_weight, centers, denominator: float, base_points=None) -> torch.Tensor:
    """``phi[P, out, in]``: every edge function of a FastKAN layer sampled at ``points`` -- ``[P]`` (the same abscissae for every
    input feature) or ``[P, in]``; they are the RBFs' argument, i.e. the value AFTER any LayerNorm.  ``base_points`` (same shape):
    other abscissae for the base branch, which in a LayerNorm layer sees the row before the normalisation; ``None``: ``points``.
    ``spline_weight`` or ``base_weight`` ``None`` leaves that branch out (``points`` may then be ``None`` too).  Not differentiable."""
    lw, lb, sw, bw, c, ng, fin, fout = _fastkan_edge_operands(None, None, spline_weight, base_weight, centers, points, base_points)
    if points is None and (sw is not None or base_points is None):
        raise AssertionError("points may be None only for the base branch alone, sampled at base_points")
    t, ldt = (None, 0) if points is None else _edge_points(points, fin, "points")
    tb, ldtb = (None, 0) if base_points is None else _edge_points(base_points, fin, "base_points")
    first = t if t is not None else tb
    if t is not None and tb is not None and tb.shape != t.shape:
        raise AssertionError("base_points must have the shape of points")
    out = torch.empty((first.size(0), fout, fin), dtype=torch.float32, device=first.device)
    with _device_of(first):
        _call("kagnn_fastkan_edge_curves", _ptr(t), ldt, _ptr(tb), ldtb, first.size(0), fin, fout, ng, _ptr(c), float(denominator),
              _ptr(sw), _ptr(bw), _ptr(out), _stream())
    return out


# ------------------------------------------------------------------------ feature-sharded FastKAN layer
# The local-compute half of kagnn_amd.sharded.ShardedFastKANLayer: a rank holds `w` of the row's P*w input columns.  LayerNorm
# (fastkan.py:77-78) is the only reduction over the sharded axis -- 2 floats per row each way; the collectives themselves are the
# caller's (torch.distributed), these are the library calls around them (include/kagnn_hip.h: kagnn_fastkan_row_moments ...).
def fastkan_row_moments(x: torch.Tensor) -> torch.Tensor:
    """[N, 2] = (mean, sum of squared deviations from it) of every row over the LOCAL columns"""
    _need_cuda(x)
    x = _rows(x)
    mom = torch.empty((x.size(0), 2), dtype=torch.float32, device=x.device)
    with _device_of(x):
        _call("kagnn_fastkan_row_moments", _ptr(x), _ld(x), x.size(0), x.size(1), _ptr(mom), _stream())
    return mom


def fastkan_merge_moments(gathered: torch.Tensor, width: int, ln_eps: float) -> torch.Tensor:
    """``gathered`` [P, N, 2]: every rank's ``fastkan_row_moments`` (``width`` columns each), merged per row in rank order ->
    [N, 2] = (mean, 1 / sqrt(biased variance + eps)) over all P * width columns: torch.nn.LayerNorm's statistics"""
    _need_cuda(gathered)
    gathered = gathered.contiguous()
    p, n = gathered.size(0), gathered.size(1)
    stats = torch.empty((n, 2), dtype=torch.float32, device=gathered.device)
    with _device_of(gathered):
        _call("kagnn_fastkan_merge_moments", _ptr(gathered), p, n, int(width), float(ln_eps), _ptr(stats), _stream())
    return stats


def _fastkan_shard_mode(x, spline_w, ng, mode):
    if mode is None:
        mode = default_precision()
    if split_like(mode) and (ng > 16 or not _fits32(x, spline_w.size(0))):
        mode = PREC_FP32                    # (more than 16 centres / very wide rows: the exact-fp32 kernels)
    return int(mode)


def fastkan_shard_fwd(x, stats, ln_w, ln_b, spline_w, base_w, base_b, centers, denominator: float, mode=None, out=None):
    """this rank's partial sums ``[N, out]`` of FastKANLayer.forward over its input columns, LayerNorm on the MERGED row
    statistics ``stats`` (``None`` with ``ln_w is None``); ``base_b``: on one rank only"""
    _need_cuda(x, spline_w, centers)
    x = _rows(x)
    n, fin = x.shape
    fout, ng = spline_w.size(0), centers.numel()
    if spline_w.size(1) != fin * ng:
        raise AssertionError("spline_linear.weight slice must be [out, in_local*num_grids]")
    mode = _fastkan_shard_mode(x, spline_w, ng, mode)
    sw = spline_w.contiguous()
    lw, lb = (None, None) if ln_w is None else (ln_w.contiguous(), ln_b.contiguous())
    bw = None if base_w is None else base_w.contiguous()
    bb = None if base_b is None else base_b.contiguous()
    ws = _ws(_sizes("kagnn_fastkan_fwd_workspace_bytes", n, fin, fout, ng, mode), x.device)
    y = torch.empty((n, fout), dtype=torch.float32, device=x.device) if out is None else out
    with _device_of(x):
        _call("kagnn_fastkan_shard_fwd", _ptr(x), _ld(x), n, fin, fout, ng, _ptr(centers), float(denominator), _ptr(lw), _ptr(lb),
              _ptr(stats), _ptr(sw), _ptr(bw), _ptr(bb), _ptr(y), _ld(y), mode, _ptr(ws), ws.numel(), _stream())
    return y


class FastKANShardBackward:
    """the state between ``fastkan_shard_bwd`` and ``fastkan_shard_bwd_finish``: the library workspace holding d loss / dz, the
    partially written input gradient, and the shape the second call has to repeat"""
    __slots__ = ("x", "stats", "lw", "lb", "gx", "ws", "dims", "mode", "wgrads")


def fastkan_shard_bwd(x, gy, stats, ln_w, ln_b, spline_w, base_w, centers, denominator: float, mode=None, want_bias=False):
    """everything of the layer's backward but the LayerNorm backward, from the gathered gradient ``gy`` [N, out]:
    ``(state, row_sums [N, 2] or None, g_spline_weight, g_base_weight, g_base_bias)``.  ``row_sums`` = (sum_f gz*gamma,
    sum_f gz*gamma*zhat) over the local columns: to be summed over the ranks, then ``fastkan_shard_bwd_finish``."""
    st, sums = fastkan_shard_bwd_halves(x, gy, stats, ln_w, ln_b, spline_w, base_w, centers, denominator, mode, part="both",
                                        want_bias=want_bias)
    return (st, sums) + st.wgrads


def fastkan_shard_bwd_halves(x, gy, stats, ln_w, ln_b, spline_w, base_w, centers, denominator: float, mode=None, part="input",
                             state=None, want_bias=False):
    """``kagnn_fastkan_shard_bwd`` in its two halves: ``part="input"`` -> ``(state, row_sums)`` (gx's base-branch part and
    d loss / dz are in ``state``); ``part="weight", state=...`` -> ``(g_spline_weight, g_base_weight, g_base_bias)`` -- the
    caller's all-reduce of ``row_sums`` runs between / beside them.  ``part="both"``: one call, ``state.wgrads`` holds the three."""
    _need_cuda(x, gy, spline_w, centers)
    x, gy = _rows(x), _rows(gy)
    n, fin = x.shape
    fout, ng = spline_w.size(0), centers.numel()
    mode = _fastkan_shard_mode(x, spline_w, ng, mode)
    dev = x.device
    sw = spline_w.contiguous()
    lw, lb = (None, None) if ln_w is None else (ln_w.contiguous(), ln_b.contiguous())
    bw = None if base_w is None else base_w.contiguous()
    f32 = dict(dtype=torch.float32, device=dev)
    st = state
    if st is None:
        st = FastKANShardBackward()
        st.x, st.stats, st.lw, st.lb, st.mode, st.dims = x, stats, lw, lb, mode, (n, fin, fout, ng)
        st.ws = _ws(_sizes("kagnn_fastkan_bwd_workspace_bytes", n, fin, fout, ng, mode), dev)
        st.gx = torch.empty((n, fin), **f32)
        st.wgrads = None
    parts = {"input": 1, "weight": 2, "both": 3}[part]
    sums = gsw = gbw = gbb = None
    if parts & 1:
        sums = torch.empty((n, 2), **f32) if lw is not None else None
    if parts & 2:
        gsw = torch.empty((fout, fin * ng), **f32)
        gbw = torch.empty((fout, fin), **f32) if bw is not None else None
        gbb = torch.empty(fout, **f32) if (want_bias and bw is not None) else None
    with _device_of(x):
        _call("kagnn_fastkan_shard_bwd", _ptr(x), _ld(x), _ptr(gy), _ld(gy), n, fin, fout, ng, _ptr(centers), float(denominator),
              _ptr(lw), _ptr(lb), _ptr(sw), _ptr(bw), _ptr(stats), _ptr(st.gx), fin, _ptr(sums), _ptr(gsw), _ptr(gbw), _ptr(gbb),
              parts, mode, _ptr(st.ws), st.ws.numel(), _stream())
    if parts == 2:
        return gsw, gbw, gbb
    st.wgrads = (gsw, gbw, gbb)
    return st, sums


def fastkan_shard_bwd_finish(st: FastKANShardBackward, row_sums: Optional[torch.Tensor], width_total: int):
    """-> ``(gx, g_ln_weight, g_ln_bias)`` with ``row_sums`` summed over the ranks (``None``: the layer has no LayerNorm)"""
    if st.lw is None:
        return st.gx, None, None
    n, fin, fout, ng = st.dims
    glw = torch.empty(fin, dtype=torch.float32, device=st.gx.device)
    glb = torch.empty_like(glw)
    with _device_of(st.gx):
        _call("kagnn_fastkan_shard_bwd_finish", _ptr(st.x), _ld(st.x), n, fin, int(width_total), fout, ng, _ptr(st.lw), _ptr(st.lb),
              _ptr(st.stats), _ptr(row_sums), _ptr(st.gx), fin, _ptr(glw), _ptr(glb), st.mode, _ptr(st.ws), st.ws.numel(), _stream())
    return st.gx, glw, glb


# ======================================================================== harness loss
class _SoftmaxXentFn(Function):
    @staticmethod
    @_on_operand_device
    def forward(ctx, logits, labels, mask, pre_softmax):
        _need_cuda(logits, labels, mask)
        z = _rows(logits)
        n, c = z.shape
        y = labels.to(torch.int64).contiguous()
        m = None if mask is None else mask.contiguous()
        ws = _ws(_sizes("kagnn_softmax_xent_workspace_bytes", n), z.device)
        out = torch.empty(2, dtype=torch.float32, device=z.device)          # (loss, row count)
        stats = torch.empty((n, 3), dtype=torch.float32, device=z.device)
        _call("kagnn_softmax_xent_fwd", _ptr(z), _ld(z), n, c, _ptr(y), _ptr(m), int(pre_softmax), _ptr(out),
              _ptr(stats), ctypes.c_void_p(out.data_ptr() + 4), _ptr(ws), ws.numel(), _stream())
        ctx.save_for_backward(z, y, m, stats, out)
        ctx.pre = int(pre_softmax)
        return out[0]

    @staticmethod
    @once_differentiable
    @_on_operand_device
    def backward(ctx, gloss):
        z, y, m, stats, out = ctx.saved_tensors
        n, c = z.shape
        g = gloss.to(torch.float32).contiguous()
        gz = torch.empty((n, c), dtype=torch.float32, device=z.device)
        _call("kagnn_softmax_xent_bwd", _ptr(z), _ld(z), n, c, _ptr(y), _ptr(m), ctx.pre, _ptr(stats),
              ctypes.c_void_p(out.data_ptr() + 4), _ptr(g), _ptr(gz), c, _stream())
        return gz, None, None, None


def softmax_cross_entropy(logits, labels, mask=None, pre_softmax: bool = False) -> torch.Tensor:
    """``CrossEntropyLoss()(f(logits)[mask], labels[mask])`` (mean over the masked rows) in one kernel each way, with
    ``f = softmax(dim=1)`` when ``pre_softmax`` (the reference harness, ``time_model.py:43-45``) and the identity
    otherwise.  ``mask``: bool ``[N]`` or ``None``; an int64 index tensor of distinct rows is accepted too.  No
    device-to-host sync (boolean indexing has one), so a whole epoch can be captured in a HIP graph."""
    if mask is not None and mask.dtype != torch.bool:
        picked = torch.zeros(logits.size(0), dtype=torch.bool, device=logits.device)
        picked[mask] = True
        mask = picked
    return _SoftmaxXentFn.apply(logits, labels, mask, bool(pre_softmax))


class _L1LossFn(Function):
    @staticmethod
    @_on_operand_device
    def forward(ctx, pred, target):
        _need_cuda(pred, target)
        p = pred.to(torch.float32).contiguous()
        t = target.to(torch.float32).contiguous()
        out = torch.empty(1, dtype=torch.float32, device=p.device)
        _call("kagnn_l1_loss_fwd", _ptr(p), _ptr(t), p.numel(), _ptr(out), _stream())
        ctx.save_for_backward(p, t)
        return out[0]

    @staticmethod
    @once_differentiable
    @_on_operand_device
    def backward(ctx, gloss):
        p, t = ctx.saved_tensors
        g = gloss.to(torch.float32).contiguous()
        gp = torch.empty_like(p)
        _call("kagnn_l1_loss_bwd", _ptr(p), _ptr(t), p.numel(), _ptr(g), _ptr(gp), _stream())
        return gp, None


class RegressionMeter:
    """The running figures of one pass of the reference's graph-regression loops (``graph_regression/optuna_zinc.py:64,72,81``:
    ``loss.item() * data.num_graphs`` per batch; ``optuna_qm9.py:69-75``: a ``[1, 12]`` per-target absolute error) as a 272-byte
    DEVICE record ``{int64 graphs; int64 targets; double abs_sum[32]}`` that ``l1_loss(..., accumulate=meter)`` adds to inside its
    one launch.  ``reset()`` is two asynchronous fills (the target count stays), ``read()`` ONE read-back: ``(abs_sum[num_targets]`` as a float64
    CPU tensor, ``graphs)``."""

    def __init__(self, num_targets: int = 1, device="cuda"):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("kagnn_amd.ops.RegressionMeter keeps its record on an MI355X (kagnn_l1_loss_meter_fwd adds to it there); "
                               f"got device '{device}'. There is no CPU fallback in this package.")
        if not 1 <= int(num_targets) <= _lib.REGRESSION_MAX_TARGETS:
            raise ValueError(f"RegressionMeter: num_targets must be 1..{_lib.REGRESSION_MAX_TARGETS}, got {num_targets}")
        self.num_targets = int(num_targets)
        host = torch.zeros(2 + _lib.REGRESSION_MAX_TARGETS, dtype=torch.int64)
        host[1] = self.num_targets
        self.record = host.to(device)

    def reset(self) -> None:
        self.record[0].zero_()
        self.record[2:].zero_()

    def read(self) -> Tuple[torch.Tensor, int]:
        host = self.record.cpu()
        return host[2:2 + self.num_targets].view(torch.float64).clone(), int(host[0])


class _L1LossMeterFn(Function):
    @staticmethod
    @_on_operand_device
    def forward(ctx, pred, target, meter, scale):
        p = pred.to(torch.float32)
        t = target.to(torch.float32)
        p = _rows(p if p.dim() == 2 else p.reshape(-1, 1))
        t = _rows(t if t.dim() == 2 else t.reshape(-1, 1))
        b, c = p.shape
        out = torch.empty(1, dtype=torch.float32, device=p.device)
        _call("kagnn_l1_loss_meter_fwd", _ptr(p), _ld(p), _ptr(t), _ld(t), b, c, _ptr(scale), _ptr(out),
              None if meter is None else _ptr(meter.record), _stream())
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(p.contiguous(), t.contiguous())
        ctx.pred_shape = pred.shape
        return out[0]

    @staticmethod
    @once_differentiable
    @_on_operand_device
    def backward(ctx, gloss):
        p, t = ctx.saved_tensors
        g = gloss.to(torch.float32).contiguous()
        gp = torch.empty_like(p)
        _call("kagnn_l1_loss_bwd", _ptr(p), _ptr(t), p.numel(), _ptr(g), _ptr(gp), _stream())
        return gp.view(ctx.pred_shape), None, None, None


def l1_loss(pred, target, accumulate: Optional[RegressionMeter] = None, scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``torch.nn.L1Loss()(pred, target)`` (mean absolute error; the loss of the reference's graph-regression scripts,
    ``graph_regression/optuna_zinc.py:58``) as one kernel each way; same shapes required (no broadcasting -- L1Loss warns about it
    and the scripts squeeze the prediction for that reason); the target gets no gradient.
    ``accumulate``: a ``RegressionMeter`` on the same device to which the same launch adds the batch's per-target sums of absolute
    errors and its number of rows (``kagnn_l1_loss_meter_fwd``: ``[B]`` or ``[B, T]`` operands, ``T <= 32``; the column sums and the
    returned mean are taken in fp64 and rounded once; the gradient is the plain path's, bit for bit).  ``scale``: fp32 ``[T]`` -- the
    QM9 script's de-standardised error ``(y * std - pred * std).abs() / std`` (``optuna_qm9.py:72``) with torch's fp32 roundings;
    an evaluation figure: refused when ``pred`` requires a gradient.  With neither, the call is what it always was."""
    if pred.shape != target.shape:
        raise ValueError(f"l1_loss: prediction {tuple(pred.shape)} and target {tuple(target.shape)} must have the same shape")
    if accumulate is None and scale is None:
        return _L1LossFn.apply(pred, target)
    _need_cuda(pred, target, None if accumulate is None else accumulate.record, scale)
    if pred.dim() not in (1, 2):
        raise ValueError(f"l1_loss: with accumulate / scale the operands are [B] or [B, T]; got {tuple(pred.shape)}")
    targets = 1 if pred.dim() == 1 else int(pred.size(1))
    if not 1 <= targets <= _lib.REGRESSION_MAX_TARGETS:
        raise ValueError(f"l1_loss: with accumulate / scale the number of targets must be 1..{_lib.REGRESSION_MAX_TARGETS} "
                         f"(KAGNN_REGRESSION_MAX_TARGETS), got {targets}")
    if accumulate is not None and accumulate.num_targets != targets:
        raise ValueError(f"l1_loss: the meter was made for {accumulate.num_targets} targets, the prediction has {targets}")
    if scale is not None:
        if pred.requires_grad:
            raise ValueError("l1_loss: scale is an evaluation figure (optuna_qm9.py:72); it is refused when pred requires a gradient")
        if scale.dtype != torch.float32 or scale.numel() != targets:
            raise ValueError(f"l1_loss: scale is an fp32 tensor of {targets} elements, got {scale.dtype} {tuple(scale.shape)}")
        scale = scale.detach().reshape(-1).contiguous()
    return _L1LossMeterFn.apply(pred, target, accumulate, scale)


# ======================================================================== graph classification: Degree, nll_loss, the epoch's meter
_NLL_FLAG_MESSAGE = "kagnn_nll_loss_fwd: a target holds a class outside [0, num_classes) (the loss of that mini-batch is NaN)"
_nll_flags: "dict[int, list]" = {}       # device index -> [int32[2] on the device (the kernel only ever SETS it), launches since the last flush]


def _nll_flag(dev, flags=None) -> torch.Tensor:
    """the device's bad-label flag of ``kagnn_nll_loss_fwd`` (``flags``: another entry point's table -- ``kagnn_node_eval`` keeps its
    own flag, with its own message, in the same way).  One per device, not one per launch: a launch only ever sets it, and
    ``flush_graph_checks`` sends it through ``_defer_flag_check`` behind everything queued so far and clears it -- a training step
    pays nothing for the check.  ONE STREAM per device is assumed, as everywhere in the loops of ``kagnn_amd.harness``: the copy and
    the clearing fill run on the stream that is current when ``flush_graph_checks`` is called, so an ``nll_loss`` launched on
    another stream has to be ordered before that call by its caller (``stream.synchronize()`` or ``wait_stream``), or its flag can
    be missed"""
    flags = _nll_flags if flags is None else flags
    en = flags.get(dev.index)
    if en is None:
        en = flags[dev.index] = [torch.zeros(2, dtype=torch.int32, device=dev), 0]
    en[1] += 1
    return en[0]


def _defer_label_flags(flags, devs, message) -> None:
    for d in devs:
        en = flags.get(d)
        if en is not None and en[1]:
            with torch.cuda.device(d):
                _defer_flag_check(en[0], message)
                en[0].zero_()                    # (behind the copy on the same stream: the next epoch starts clean)
            en[1] = 0


class ClassificationMeter:
    """The running figures of one epoch of the reference's classification loops (``graph_classification_utils.py:45-72``:
    ``loss_all += ...item()`` and ``correct += ...item()`` per batch) as a 24-byte DEVICE record ``{double nll_sum; int64 correct;
    int64 graphs}`` that ``nll_loss(..., accumulate=meter)`` adds to inside its one launch.  ``reset()`` is one asynchronous fill,
    ``read()`` ONE read-back: ``(nll_sum, correct, graphs)`` as Python numbers."""

    def __init__(self, device="cuda"):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("kagnn_amd.ops.ClassificationMeter keeps its record on an MI355X (kagnn_nll_loss_fwd adds to it there); "
                               f"got device '{device}'. There is no CPU fallback in this package.")
        self.record = torch.zeros(3, dtype=torch.int64, device=device)

    def reset(self) -> None:
        self.record.zero_()

    def read(self) -> Tuple[float, int, int]:
        host = self.record.cpu()
        return float(host[:1].view(torch.float64)[0]), int(host[1]), int(host[2])


_REDUCTIONS = {"mean": 0, "sum": 1}      # KAGNN_REDUCTION_MEAN / _SUM


class _NllLossFn(Function):
    @staticmethod
    @_on_operand_device
    def forward(ctx, logp, target, reduction, meter):
        z = _rows(logp)
        b, c = z.shape
        y = target.contiguous()
        out = torch.empty(2, dtype=torch.float32, device=z.device)          # (mean, sum)
        _call("kagnn_nll_loss_fwd", _ptr(z), _ld(z), b, c, _ptr(y), _ptr(out), ctypes.c_void_p(out.data_ptr() + 4),
              None if meter is None else _ptr(meter.record), _ptr(_nll_flag(z.device)), _stream())
        ctx.save_for_backward(y)
        ctx.classes, ctx.reduction = c, reduction
        return out[reduction]

    @staticmethod
    @once_differentiable
    @_on_operand_device
    def backward(ctx, gloss):
        y, = ctx.saved_tensors
        b, c = y.numel(), ctx.classes
        g = gloss.to(torch.float32).contiguous()
        gz = torch.empty((b, c), dtype=torch.float32, device=y.device)
        _call("kagnn_nll_loss_bwd", _ptr(y), b, c, _ptr(g), ctx.reduction, _ptr(gz), c, _stream())
        return gz, None, None, None


def nll_loss(logp, target, reduction: str = "mean", accumulate: Optional[ClassificationMeter] = None) -> torch.Tensor:
    """``F.nll_loss(logp, target, reduction=...)`` for the fp32 ``[B, C]`` log-probabilities every graph-classification model here
    returns and int64 targets ``[B]`` (the loss of the reference's loops, ``graph_classification_utils.py:50,62``): one launch each
    way, the sum taken in fp64 and rounded once.  ``accumulate``: a ``ClassificationMeter`` on the same device to which the same
    launch adds this batch's loss SUM (whatever ``reduction`` is), its number of correct arg-max predictions (``:70-71``) and its
    number of graphs.  No read-back: a target outside ``[0, C)`` gives a NaN loss at once and raises at the next
    ``flush_graph_checks()`` (called on the stream the losses were launched on: see ``_nll_flag``)."""
    if reduction not in _REDUCTIONS:
        raise ValueError(f"nll_loss: reduction must be 'mean' or 'sum' (one launch makes one number), got {reduction!r}")
    _need_cuda(logp, target, None if accumulate is None else accumulate.record)
    if logp.dim() != 2 or target.dim() != 1 or target.size(0) != logp.size(0):
        raise ValueError(f"nll_loss: log-probabilities [B, C] and targets [B]; got {tuple(logp.shape)} and {tuple(target.shape)}")
    if target.dtype != torch.int64:
        raise TypeError(f"nll_loss: targets are int64 class indices, got {target.dtype}")
    return _NllLossFn.apply(logp, target, _REDUCTIONS[reduction], accumulate)


def _degree_one_hot_raw(rowptr_by_source: Optional[torch.Tensor], num_nodes: int, num_classes: int, device) -> torch.Tensor:
    x = torch.empty((num_nodes, num_classes), dtype=torch.float32, device=device)
    with _device_of(x):
        _call("kagnn_degree_one_hot", _ptr(rowptr_by_source), num_nodes, num_classes, _ptr(x), num_classes, _stream())
    return x


def degree_one_hot(graph, num_nodes: int, num_classes: int = 36) -> torch.Tensor:
    """The reference's ``Degree`` transform (``graph_classification_utils.py:31-36``), the node features of the unlabeled TU
    datasets: ``F.one_hot(clip(degree(edge_index[0], num_nodes), 0, num_classes - 1), num_classes).float()`` in one launch.
    ``graph``: a ``GraphIndex`` or an int64 ``edge_index [2, E]`` on the device (indexed here, uncached).  The degree is the OUT-degree
    -- edges counted at their source -- read off the index's by-source offsets (``rowptr_t``)."""
    num_nodes, num_classes = int(num_nodes), int(num_classes)
    if num_classes < 1:
        raise ValueError("degree_one_hot: num_classes >= 1")
    if isinstance(graph, GraphIndex):
        if graph.num_nodes != num_nodes:
            raise ValueError(f"degree_one_hot: the index describes {graph.num_nodes} nodes, not {num_nodes}")
        return _degree_one_hot_raw(graph.rowptr_t, num_nodes, num_classes, graph.device)
    _need_cuda(graph)
    if graph.dim() != 2 or graph.size(0) != 2 or graph.dtype != torch.int64:
        raise ValueError("edge_index must be an int64 tensor of shape [2, E]")
    if graph.size(1) == 0:
        return _degree_one_hot_raw(None, num_nodes, num_classes, graph.device)
    g = GraphIndex(graph, num_nodes)
    return _degree_one_hot_raw(g.rowptr_t, num_nodes, num_classes, graph.device)


# ======================================================================== node classification: split metrics, early stopping, snapshot
_NODE_EVAL_FLAG_MESSAGE = "kagnn_node_eval: a row of a split holds a label outside [0, num_classes) (that split's loss is NaN)"
_node_eval_flags: "dict[int, list]" = {}     # as _nll_flags: device index -> [int32[2] on the device, launches since the last flush]
NODE_EVAL_MAX_SPLITS = 8


def split_bits(*masks, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One byte per node for ``node_eval``: bit ``s`` is set where ``masks[s]`` is.  Up to 8 boolean ``[N]`` masks of one length
    on one device, overlapping or not (``test_mask=None`` of the reference's loop is the validation mask passed twice).  Plain
    torch, built once per split; ``out``: a uint8 ``[N]`` tensor to refill."""
    if not 1 <= len(masks) <= NODE_EVAL_MAX_SPLITS:
        raise ValueError(f"split_bits: 1 to {NODE_EVAL_MAX_SPLITS} masks (one bit of the row's byte each), got {len(masks)}")
    n = masks[0].numel()
    for m in masks:
        if m.dim() != 1 or m.dtype != torch.bool:
            raise TypeError(f"split_bits: masks are 1-D bool tensors, got {m.dtype} of shape {tuple(m.shape)}")
        if m.numel() != n or m.device != masks[0].device:
            raise ValueError("split_bits: the masks must have one length and one device; "
                             f"got {[int(q.numel()) for q in masks]} on {[str(q.device) for q in masks]}")
    if out is None:
        out = torch.zeros(n, dtype=torch.uint8, device=masks[0].device)
    else:
        if out.dtype != torch.uint8 or out.shape != (n,) or out.device != masks[0].device or not out.is_contiguous():
            raise ValueError("split_bits: out must be a contiguous uint8 [N] tensor on the masks' device")
        out.zero_()
    for s, m in enumerate(masks):
        out |= m.to(torch.uint8) << s
    return out


def node_eval(logits, labels, bits, num_splits: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Loss and accuracy figures of up to 8 node splits from ONE pass over the fp32 ``[N, C]`` logits (``kagnn_node_eval``): what
    the reference's loop takes per epoch with a masked ``CrossEntropyLoss`` and three ``pred[mask] == y[mask]`` counts
    (``node_classification_clean/utils.py:150-160,171-178``).  ``bits``: ``split_bits(...)``; ``labels`` int64 ``[N]``.  Returns the
    records as an int64 ``[num_splits, 3]`` device tensor -- per split ``(xent_sum, correct, rows)``, the first as the bits of a
    double (``records[:, 0].view(torch.float64)``); ``out`` is overwritten and returned when given.  No read-back: a label outside
    ``[0, C)`` in a row of some split makes that split's sum NaN at once and raises at the next ``flush_graph_checks()``, exactly
    as ``nll_loss``'s flag does (one stream per device: see ``_nll_flag``)."""
    _need_cuda(logits, labels, bits, out)
    num_splits = int(num_splits)
    if logits.dim() != 2 or labels.dim() != 1 or bits.dim() != 1 or labels.size(0) != logits.size(0) or bits.size(0) != logits.size(0):
        raise ValueError(f"node_eval: logits [N, C], labels [N] and bits [N]; got {tuple(logits.shape)}, {tuple(labels.shape)}, {tuple(bits.shape)}")
    if labels.dtype != torch.int64 or bits.dtype != torch.uint8:
        raise TypeError(f"node_eval: labels are int64 class indices and bits uint8 (split_bits), got {labels.dtype} and {bits.dtype}")
    if not 1 <= num_splits <= NODE_EVAL_MAX_SPLITS:
        raise ValueError(f"node_eval: num_splits must be 1..{NODE_EVAL_MAX_SPLITS}, got {num_splits}")
    z = _rows(logits.detach())
    n, c = z.shape
    if out is None:
        out = torch.empty((num_splits, 3), dtype=torch.int64, device=z.device)
    elif out.dtype != torch.int64 or out.shape != (num_splits, 3) or not out.is_contiguous():
        raise ValueError("node_eval: out must be a contiguous int64 [num_splits, 3] tensor")
    y, b = labels.contiguous(), bits.contiguous()
    nbytes = _sizes("kagnn_node_eval_workspace_bytes", n, c, num_splits)
    ws = _ws(nbytes, z.device) if nbytes else None
    with _device_of(z):
        _call("kagnn_node_eval", _ptr(z), _ld(z), n, c, _ptr(y), _ptr(b), num_splits, _ptr(out), _ptr(_nll_flag(z.device, _node_eval_flags)),
              _ptr(ws), nbytes, _stream())
    return out


class EarlyStopState(NamedTuple):
    """what ``EarlyStop.read()`` returns: the device record's fields and ``history`` -- the eval records of the counted epochs as a
    CPU int64 ``[epochs, num_splits, 3]`` tensor (``None`` when not asked for)"""
    min_loss: float
    min_delta: float
    patience: int
    counter: int
    epochs: int
    best_epoch: int
    improved: bool
    stopped: bool
    history: Optional[torch.Tensor]


class EarlyStop:
    """The reference's ``EarlyStopper(patience, min_delta)`` (``node_classification_clean/utils.py:68-86``) as a 32-byte DEVICE record
    that ``update(records)`` advances with one tiny launch (``kagnn_early_stop_update``): the validation split's mean loss against
    the running minimum in fp32, the miss counter, the stop.  It also counts the epochs, remembers the best one and keeps every
    counted epoch's ``node_eval`` records in ``history``, so the whole run's curves come back with ``read()`` -- ONE read-back.
    ``improved`` is the device word ``copy_if`` takes as its flag.  Once stopped (or after ``max_epochs`` updates) further updates
    only clear ``improved``."""

    def __init__(self, patience: int, min_delta: float = 0.0, max_epochs: int = 1000, num_splits: int = 3, device="cuda"):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("kagnn_amd.ops.EarlyStop keeps its record on an MI355X (kagnn_early_stop_update advances it there); "
                               f"got device '{device}'. There is no CPU fallback in this package.")
        if not 1 <= int(num_splits) <= NODE_EVAL_MAX_SPLITS or int(max_epochs) < 0:
            raise ValueError(f"EarlyStop: num_splits 1..{NODE_EVAL_MAX_SPLITS} and max_epochs >= 0")
        self.num_splits, self.max_epochs = int(num_splits), int(max_epochs)
        # one buffer: the record (32 bytes = 4 words of 8) in front of history, so read() is one copy
        host = torch.zeros(4 + self.max_epochs * self.num_splits * 3, dtype=torch.int64)
        head = host[:4].view(torch.int32)
        host[:1].view(torch.float32)[0] = float("inf")
        host[:1].view(torch.float32)[1] = float(min_delta)
        head[2], head[5] = int(patience), -1
        self._buf = host.to(device)
        self.state = self._buf[:4].view(torch.int32)
        self.improved = self.state[6:7]
        self.history = self._buf[4:].view(self.max_epochs, self.num_splits, 3)

    def update(self, records: torch.Tensor, val_split: int = 1) -> None:
        _need_cuda(records)
        if records.dtype != torch.int64 or records.shape != (self.num_splits, 3) or not records.is_contiguous() or records.device != self._buf.device:
            raise ValueError(f"EarlyStop.update: records are node_eval's contiguous int64 [{self.num_splits}, 3] tensor on {self._buf.device}")
        if not 0 <= int(val_split) < self.num_splits:
            raise ValueError(f"EarlyStop.update: val_split must be in [0, {self.num_splits})")
        with _device_of(self._buf):
            _call("kagnn_early_stop_update", _ptr(records), self.num_splits, int(val_split), _ptr(self.state),
                  _ptr(self.history) if self.max_epochs else None, self.max_epochs, _stream())

    def read(self, history: bool = True) -> EarlyStopState:
        """ONE read-back: the record, and with ``history`` the counted rows of the history (a poll needs the record alone)"""
        host = (self._buf if history else self._buf[:4]).cpu()
        f, i = host[:1].view(torch.float32).tolist(), host[:4].view(torch.int32).tolist()
        hist = host[4:].view(self.max_epochs, self.num_splits, 3)[:i[4]] if history else None
        return EarlyStopState(f[0], f[1], i[2], i[3], i[4], i[5], bool(i[6]), bool(i[7]), hist)


class RegressionStopState(NamedTuple):
    """what ``RegressionStop.read()`` returns: the device record's fields and ``history`` -- the per-target mean absolute errors of
    the counted epochs as a CPU float64 ``[epochs, 3, num_targets]`` tensor, splits in the order train, val, test (``None`` when
    not asked for)"""
    min_loss: float
    min_delta: float
    best_val: float
    test_at_best: float
    patience: int
    counter: int
    epochs: int
    best_epoch: int
    test_epoch: int
    improved: bool
    stopped: bool
    history: Optional[torch.Tensor]


class RegressionStop:
    """What the reference's graph-regression scripts decide once per epoch (``graph_regression/optuna_zinc.py:75-86``: ``if
    best_val_loss >= val_loss`` take the test figure; ``EarlyStopper(patience)``, ``graph_regression/utils.py:8-16``) as a 48-byte
    DEVICE record that ``update(train, val, test, sizes)`` advances with one tiny launch (``kagnn_regression_epoch_update``) from
    the three splits' ``RegressionMeter``s -- which the launch also zeroes for the next epoch.  Every counted epoch's per-target
    figures are kept in ``history`` behind the record, in ONE buffer, so ``read()`` is one copy.  ``improved`` is the device word
    ``copy_if`` takes as its flag.  Once stopped (or after ``max_epochs`` updates) further updates only clear ``improved``."""
    _HEAD = 6                                                    # the record: 48 bytes = 6 words of 8

    def __init__(self, patience: int, min_delta: float = 0.0, max_epochs: int = 1000, num_targets: int = 1, device="cuda"):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("kagnn_amd.ops.RegressionStop keeps its record on an MI355X (kagnn_regression_epoch_update advances it "
                               f"there); got device '{device}'. There is no CPU fallback in this package.")
        if not 1 <= int(num_targets) <= _lib.REGRESSION_MAX_TARGETS or int(max_epochs) < 0:
            raise ValueError(f"RegressionStop: num_targets 1..{_lib.REGRESSION_MAX_TARGETS} and max_epochs >= 0")
        self.num_targets, self.max_epochs = int(num_targets), int(max_epochs)
        host = torch.zeros(self._HEAD + self.max_epochs * 3 * _lib.REGRESSION_MAX_TARGETS, dtype=torch.int64)
        f, i = host[:2].view(torch.float32), host[:self._HEAD].view(torch.int32)
        f[0], f[1], f[2], f[3] = float("inf"), float(min_delta), float("inf"), float("nan")
        i[4], i[7], i[8] = int(patience), -1, -1
        self._buf = host.to(device)
        self.state = self._buf[:self._HEAD].view(torch.int32)
        self.improved = self.state[9:10]
        self.history = self._buf[self._HEAD:].view(torch.float64).view(self.max_epochs, 3, _lib.REGRESSION_MAX_TARGETS)

    def update(self, train: RegressionMeter, val: RegressionMeter, test: Optional[RegressionMeter], sizes) -> None:
        """``sizes``: the three ``len(loader.dataset)`` divisors (train, val, test); ``test=None``: the validation meter"""
        n_train, n_val, n_test = (int(n) for n in sizes)
        for m in (train, val, test):
            if m is not None and (not isinstance(m, RegressionMeter) or m.record.device != self._buf.device):
                raise ValueError(f"RegressionStop.update: the meters are RegressionMeters on {self._buf.device}")
        with _device_of(self._buf):
            _call("kagnn_regression_epoch_update", _ptr(train.record), _ptr(val.record), None if test is None else _ptr(test.record),
                  n_train, n_val, n_test, _ptr(self.state), _ptr(self.history) if self.max_epochs else None, self.max_epochs, _stream())

    def read(self, history: bool = True) -> RegressionStopState:
        """ONE read-back: the record, and with ``history`` the counted rows of the history (a poll needs the record alone)"""
        host = (self._buf if history else self._buf[:self._HEAD]).cpu()
        f, i = host[:2].view(torch.float32).tolist(), host[:self._HEAD].view(torch.int32).tolist()
        hist = None
        if history:
            hist = host[self._HEAD:].view(torch.float64).view(self.max_epochs, 3, _lib.REGRESSION_MAX_TARGETS)[:i[6], :, :self.num_targets]
        return RegressionStopState(f[0], f[1], f[2], f[3], i[4], i[5], i[6], i[7], i[8], bool(i[9]), bool(i[10]), hist)


_COPY_IF_TABLES: dict = {}
_COPY_IF_TABLES_MAX = 16


def copy_if(flag: torch.Tensor, dsts, srcs) -> None:
    """``dst.copy_(src)`` for every pair if the device word ``flag`` (int32, e.g. ``EarlyStop.improved``) is non-zero, else nothing
    -- decided ON the device, one launch per 32 tensors (``kagnn_copy_if``).  The tensors go as bytes: parameters and buffers of
    any dtype alike, contiguous, pairwise the same dtype and shape, their sizes multiples of 4 bytes (an int64 counter is 8).  The
    pointer tables are cached per set of tensors, as ``harness.Adam`` caches its own."""
    dsts, srcs = list(dsts), list(srcs)
    _need_cuda(flag, *dsts, *srcs)
    if flag.dtype != torch.int32 or flag.numel() != 1:
        raise TypeError(f"copy_if: the flag is one int32 on the device, got {flag.dtype} x {flag.numel()}")
    if len(dsts) != len(srcs):
        raise ValueError(f"copy_if: {len(dsts)} destinations for {len(srcs)} sources")
    key = (tuple(t.data_ptr() for t in dsts), tuple(t.data_ptr() for t in srcs), tuple(t.numel() * t.element_size() for t in srcs))
    tables = _COPY_IF_TABLES.get(key)
    if tables is None:
        for d, t in zip(dsts, srcs):
            if d.dtype != t.dtype or d.shape != t.shape or not d.is_contiguous() or not t.is_contiguous():
                raise ValueError(f"copy_if: pairs of contiguous tensors of one dtype and shape; got {d.dtype} {tuple(d.shape)} <- {t.dtype} {tuple(t.shape)}")
            if (t.numel() * t.element_size()) % 4 or d.data_ptr() % 4 or t.data_ptr() % 4:
                raise ValueError("copy_if: tensors are 4-byte aligned and their sizes multiples of 4 bytes")
        n = len(dsts)
        if len(_COPY_IF_TABLES) >= _COPY_IF_TABLES_MAX:
            _COPY_IF_TABLES.clear()
        tables = _COPY_IF_TABLES[key] = ((ctypes.c_void_p * n)(*key[0]), (ctypes.c_void_p * n)(*key[1]), (ctypes.c_int64 * n)(*key[2]))
    with _device_of(flag):
        _call("kagnn_copy_if", _ptr(flag), len(dsts), *tables, _stream())


# ======================================================================== link prediction: edge keys, negatives, pair scores, BCE, ranking
def _edge_keys_raw(src, dst, num_nodes: int) -> torch.Tensor:
    e, dev = int(src.numel()), src.device
    keys = torch.empty(e, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    ws = _ws(_sizes("kagnn_edge_keys_workspace_bytes", e), dev)
    with _device_of(src):
        _call("kagnn_edge_keys_build", _ptr(src), _ptr(dst), e, int(num_nodes), _ptr(keys), _ptr(count), _ptr(ws), ws.numel(), _stream())
        return keys[:int(count.item())] if e else keys


def edge_keys(edge_index: torch.Tensor, num_nodes: int) -> torch.Tensor:
    """The edge set of an int64 ``[2, E]`` device ``edge_index`` as ascending, duplicate-free int64 keys ``src * num_nodes + dst``
    (``kagnn_edge_keys_build``: a rocPRIM radix sort and a unique pass) -- what ``negative_sample`` tests membership against.  One
    read of the number of keys; ``GraphIndex.edge_keys`` keeps the result per graph."""
    if edge_index.dim() != 2 or edge_index.size(0) != 2 or edge_index.dtype != torch.int64:
        raise ValueError("edge_index must be an int64 tensor of shape [2, E]")
    num_nodes = int(num_nodes)
    if not 0 <= num_nodes < 1 << 31 or (edge_index.size(1) and not num_nodes):
        raise ValueError(f"edge_keys: num_nodes must lie in [0, 2^31) and be positive when there are edges, got {num_nodes}")
    _need_cuda(edge_index)
    return _edge_keys_raw(edge_index[0].contiguous(), edge_index[1].contiguous(), num_nodes)


def negative_sample(num: int, g_or_keys, num_nodes: int, seed: int = 0, attempts: int = 8):
    """``num`` uniform negative pairs of a graph of ``num_nodes`` nodes (torch_geometric's ``negative_sampling``, dense-free) as a
    FIXED-SIZE result, on the device, without compaction or read-back: ``(pairs, valid)`` = int64 ``[2, num]`` and uint8 ``[num]``.
    ``g_or_keys``: a ``GraphIndex`` (its ``edge_keys``) or the int64 key vector of ``edge_keys``.  Slot ``p`` tries the attempts
    ``t = 0 .. attempts - 1`` with the counter ``c = p * attempts + t``: ``u = (key32(seed, 2c) * N) >> 32``, ``v = (key32(seed,
    2c + 1) * N) >> 32`` (``key32``: the sampler's, ``kagnn_hip.h``); an attempt is valid iff ``u != v`` and ``(u, v)`` is not an
    edge; the slot takes its first valid attempt.  A slot without one is EMPTY: the pair ``(0, 0)`` with ``valid = 0`` -- give it
    weight 0 (``bce_with_logits(weight_u8=valid)``).  The share of empty slots is ``(1 - free / N^2) ** attempts``, ``free`` the
    number of ordered non-edge, non-self pairs.  A pure function of ``(seed, keys, N, attempts)``: two calls return the same bits.
    ``seed``: any int, taken mod 2^64.  Refused before any launch: ``attempts`` outside 1..32, ``2 * num * attempts >= 2^32``,
    ``num_nodes >= 2^31``."""
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError(f"negative_sample: seed must be an int, got {seed!r}")
    num, num_nodes, attempts = int(num), int(num_nodes), int(attempts)
    if not 1 <= attempts <= _lib.NEGATIVE_MAX_ATTEMPTS:
        raise ValueError(f"negative_sample: attempts must be 1..{_lib.NEGATIVE_MAX_ATTEMPTS}, got {attempts}")
    if num < 0 or 2 * num * attempts >= 1 << 32:
        raise ValueError(f"negative_sample: num >= 0 and 2 * num * attempts below 2^32; got num = {num}, attempts = {attempts}")
    if not 0 <= num_nodes < 1 << 31:
        raise ValueError(f"negative_sample: num_nodes must lie in [0, 2^31), got {num_nodes}")
    if isinstance(g_or_keys, GraphIndex):
        if g_or_keys.num_nodes != num_nodes:
            raise ValueError(f"negative_sample: the index describes {g_or_keys.num_nodes} nodes, not {num_nodes}")
        _need_cuda(g_or_keys.rowptr)
        keys = g_or_keys.edge_keys
    else:
        keys = g_or_keys
        if not isinstance(keys, torch.Tensor) or keys.dtype != torch.int64 or keys.dim() != 1:
            raise TypeError("negative_sample: a GraphIndex or the int64 key vector of ops.edge_keys")
        _need_cuda(keys)
        keys = keys.contiguous()
    dev = keys.device
    if num_nodes == 0:
        return torch.zeros((2, num), dtype=torch.int64, device=dev), torch.zeros(num, dtype=torch.uint8, device=dev)
    pairs = torch.empty((2, num), dtype=torch.int64, device=dev)
    valid = torch.empty(num, dtype=torch.uint8, device=dev)
    with _device_of(keys):
        _call("kagnn_negative_sample", _ptr(keys), keys.numel(), num_nodes, num, int(seed) & 0xFFFFFFFFFFFFFFFF, attempts, _ptr(pairs),
              _ptr(valid), _stream())
    return pairs, valid


class _PairScoresFn(Function):
    """s[p] = <z[u_p], z[v_p]> over a pair index (u = source, v = destination): ``kagnn_aggregate_edge_grad`` with x = gout = z; the
    backward is the two weighted aggregations of the upstream gradient, one over each structure of the index"""

    @staticmethod
    @_on_operand_device
    def forward(ctx, z, g):
        rows = _rows(z)
        ctx.g = g
        ctx.save_for_backward(rows)
        if g is None or g.num_edges == 0:                              # (no pair: nothing is indexed and nothing launched)
            return torch.empty(0, dtype=torch.float32, device=z.device)
        return _aggregate_edge_grad_csr(rows, rows, g.rowptr, g.col, g.perm, g.hub_seg if g.num_hub_seg else None, g.num_hub_seg,
                                        g.hub_threshold, g.num_edges, None, None, False)

    @staticmethod
    @once_differentiable
    @_on_operand_device
    def backward(ctx, gs):
        rows, = ctx.saved_tensors
        g = ctx.g
        if g is None or g.num_edges == 0:
            return torch.zeros(rows.shape, dtype=torch.float32, device=rows.device), None
        gs = gs.to(torch.float32)
        # d s_p / d z[v_p] = z[u_p]: rows = destinations gather their sources;  d s_p / d z[u_p] = z[v_p]: the transposed structure
        by_dst = _aggregate_csr(rows, g.rowptr, g.col, g.hub_seg, g.num_hub_seg, g.hub_threshold, 0.0, gs[g.perm.long()].contiguous(),
                                None, None, None, False)
        return _aggregate_csr(rows, g.rowptr_t, g.col_t, g.hub_seg_t, g.num_hub_seg_t, g.hub_threshold, 0.0,
                              gs[g.perm_t.long()].contiguous(), None, None, None, False, addend=by_dst), None


def pair_index(pairs: torch.Tensor, num_nodes: int) -> GraphIndex:
    """the ``GraphIndex`` of a pair list for ``pair_scores``: int64 ``[2, P]``, ``u = pairs[0]`` the source, ``v = pairs[1]`` the
    destination.  Never cached and validated later (``flush_graph_checks``): index a fixed list once and keep the result."""
    return graph_index(pairs, num_nodes, cache=False)


def pair_scores(z, pairs) -> torch.Tensor:
    """The dot-product decoder of link prediction: ``s[p] = <z[u_p], z[v_p]>`` as fp32 ``[P]``, with autograd.  ``pairs``: an int64
    ``[2, P]`` device tensor or an ``ops.GraphIndex`` built over it for ``z.size(0)`` nodes (``u`` = source, ``v`` = destination;
    duplicate and self pairs are fine).
    No kernel of its own.  The forward is ``kagnn_aggregate_edge_grad`` with ``x = gout = z`` on the pairs' by-destination
    structure, which writes the products in the pairs' original order.  The backward is one ``kagnn_aggregate_sum`` over the
    by-destination structure plus one ``kagnn_aggregate_sum_add`` over the by-source structure, both with ``self_scale = 0`` and the
    upstream gradient as edge weights -- deterministic, no atomics.
    What it costs: one CSR build per NEW pair list.  On the small-graph path (up to 65 536 pairs and nodes) the build is one
    launch and does not synchronise; above it the rocPRIM path synchronises the stream ONCE per structure's build call.  So pass a
    ``GraphIndex`` (``pair_index``) for the lists that stay fixed -- the positives, the evaluation negatives -- and a tensor only for
    pairs drawn anew, such as each epoch's training negatives."""
    if z.dim() != 2:
        raise ValueError(f"pair_scores: z is [N, d], got shape {tuple(z.shape)}")
    if isinstance(pairs, GraphIndex):
        g = pairs
        if g.num_nodes != z.size(0):
            raise ValueError(f"pair_scores: the pair index describes {g.num_nodes} nodes, z has {z.size(0)} rows")
        _need_cuda(z, g.rowptr)
    else:
        if not isinstance(pairs, torch.Tensor) or pairs.dim() != 2 or pairs.size(0) != 2 or pairs.dtype != torch.int64:
            raise ValueError("pair_scores: pairs must be an int64 tensor of shape [2, P] or a GraphIndex")
        _need_cuda(z, pairs)
        with _device_of(z):
            g = pair_index(pairs, z.size(0)) if pairs.size(1) else None
    return _PairScoresFn.apply(z, g)


def _bce_operands(what, scores, labels_u8, weight_u8):
    if scores.dim() != 1 or scores.dtype != torch.float32:
        raise TypeError(f"{what}: scores are an fp32 vector [P], got {scores.dtype} of shape {tuple(scores.shape)}")
    for name, t in (("labels_u8", labels_u8), ("weight_u8", weight_u8)):
        if t is None and name == "weight_u8":
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 1:
            raise TypeError(f"{what}: {name} is a uint8 vector [P]")
        if t.numel() != scores.numel():
            raise ValueError(f"{what}: {name} has {t.numel()} entries for {scores.numel()} scores")
    _need_cuda(scores, labels_u8, weight_u8)


class _BceLogitsFn(Function):
    @staticmethod
    @_on_operand_device
    def forward(ctx, scores, labels, weight, record):
        s = scores.contiguous()
        p, dev = s.numel(), s.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        divisor = torch.empty(1, dtype=torch.int64, device=dev)
        ws = _ws(_lib.BCE_WORKSPACE_BYTES, dev) if p > 4096 else None
        _call("kagnn_bce_logits_fwd", _ptr(s), _ptr(labels), _ptr(weight), p, _ptr(loss), _ptr(divisor), _ptr(record), _ptr(ws),
              ws.numel() if ws is not None else 0, _stream())
        ctx.save_for_backward(s, labels, divisor)
        ctx.weight = weight
        return loss[0]

    @staticmethod
    @once_differentiable
    @_on_operand_device
    def backward(ctx, gloss):
        s, labels, divisor = ctx.saved_tensors
        g = gloss.to(torch.float32).contiguous()
        gs = torch.empty_like(s)
        _call("kagnn_bce_logits_bwd", _ptr(s), _ptr(labels), _ptr(ctx.weight), s.numel(), _ptr(divisor), _ptr(g), _ptr(gs), _stream())
        return gs, None, None, None


def bce_with_logits(scores, labels_u8, weight_u8=None, accumulate: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``F.binary_cross_entropy_with_logits(scores, labels)`` over the rows of weight 1 (``weight_u8=None``: all rows) as one call
    each way: the mean of ``max(s, 0) - s * y + log1p(exp(-|s|))``, the term in fp32, the sum in fp64 partials added in a fixed
    order, divided by the number of such rows (at least 1: no row gives 0) and rounded once; the gradient is ``(sigmoid(s) - y) * w /
    rows``.  ``scores`` fp32 ``[P]``; ``labels_u8`` / ``weight_u8`` uint8 ``[P]`` (non-zero = 1) -- ``negative_sample``'s ``valid``
    is a weight.  ``accumulate``: a contiguous int64 device tensor of 3 elements (``[3]`` or ``[1, 3]``) that the same call
    OVERWRITES with one record of ``node_eval``'s format -- the loss sum as the bits of a double, the rows with ``(s > 0) == y``,
    the rows -- so that ``EarlyStop.update(record.view(1, 3), 0)`` and ``copy_if`` serve a link-prediction loop as they are.  A
    NaN score makes the sum NaN; it counts like any other score."""
    if accumulate is not None and (not isinstance(accumulate, torch.Tensor) or accumulate.dtype != torch.int64 or accumulate.numel() != 3
                                   or not accumulate.is_contiguous()):
        raise ValueError("bce_with_logits: accumulate is a contiguous int64 tensor of 3 elements (one node_eval record)")
    _bce_operands("bce_with_logits", scores, labels_u8, weight_u8)
    _need_cuda(scores, accumulate)
    return _BceLogitsFn.apply(scores, labels_u8.contiguous(), None if weight_u8 is None else weight_u8.contiguous(), accumulate)


LINK_RANK_MAX_KS = 3


def link_rank(scores, labels_u8, weight_u8=None, ks=(20, 50, 100), out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The ranking figures of a scored pair set as an int64 ``[8]`` device record ``{2U, n_pos, n_neg, nan_rows, hits[ks[0]],
    hits[ks[1]], hits[ks[2]], 0}`` (``kagnn_link_rank``; exact integers, no read-back): ``2U`` = over positives ``i`` and negatives
    ``j``, 2 where ``s_i > s_j`` and 1 where ``s_i == s_j``, so ROC-AUC is ``2U / (2 * n_pos * n_neg)`` (``link_rank_figures``);
    ``hits[k]`` = the positives strictly above the ``k``-th largest negative score, all of them when there are fewer than ``k``
    negatives.  Rows of weight 0 and rows with a NaN score take no part (the latter are counted in ``nan_rows``); ``-0.0`` and
    ``+0.0`` tie, ``+-Inf`` are ordinary values.  ``ks``: up to 3 integers >= 1.  ``out``: a contiguous int64 ``[8]`` device tensor
    to overwrite (a row of a history)."""
    ks = [int(k) for k in ks]
    if len(ks) > LINK_RANK_MAX_KS or any(k < 1 or k >= 1 << 31 for k in ks):
        raise ValueError(f"link_rank: ks holds at most {LINK_RANK_MAX_KS} values, each in [1, 2^31); got {ks}")
    _bce_operands("link_rank", scores, labels_u8, weight_u8)
    s = scores.detach().contiguous()
    p, dev = s.numel(), s.device
    if out is None:
        out = torch.empty(8, dtype=torch.int64, device=dev)
    elif out.dtype != torch.int64 or out.shape != (8,) or not out.is_contiguous() or out.device != dev:
        raise ValueError("link_rank: out must be a contiguous int64 [8] tensor on the scores' device")
    nbytes = _sizes("kagnn_link_rank_workspace_bytes", p)
    ws = _ws(nbytes, dev)
    ks_host = (ctypes.c_int32 * max(len(ks), 1))(*ks)
    with _device_of(s):
        _call("kagnn_link_rank", _ptr(s), _ptr(labels_u8.contiguous()), None if weight_u8 is None else _ptr(weight_u8.contiguous()), p,
              ks_host, len(ks), _ptr(out), _ptr(ws), nbytes, _stream())
    return out


def link_rank_figures(record, ks=(20, 50, 100)) -> dict:
    """a ``link_rank`` record (any device; read here) as numbers: ``auc`` (NaN without a positive or a negative), ``hits`` -- the
    share of positives above the ``k``-th negative, per ``k`` -- and the four counts"""
    r = [int(v) for v in record.reshape(-1).tolist()]
    u2, n_pos, n_neg = r[0], r[1], r[2]
    auc = u2 / (2 * n_pos * n_neg) if n_pos and n_neg else float("nan")
    hits = {int(k): (r[4 + j] / n_pos if n_pos else float("nan")) for j, k in enumerate(ks)}
    return {"auc": auc, "hits": hits, "two_u": u2, "n_pos": n_pos, "n_neg": n_neg, "nan_rows": r[3]}


# ======================================================================== GAT attention aggregation
class _GatFn(Function):
    @staticmethod
    @_on_operand_device
    def forward(ctx, xh, att_src, att_dst, bias, g, heads, channels):
        _need_cuda(xh, att_src, att_dst)
        xh = _rows(xh)
        n = xh.size(0)
        dev = xh.device
        a_s = att_src.reshape(heads, channels).contiguous()
        a_d = att_dst.reshape(heads, channels).contiguous()
        b = None if bias is None else bias.contiguous()
        ls = torch.empty((n, heads), dtype=torch.float32, device=dev)
        ld_ = torch.empty((n, heads), dtype=torch.float32, device=dev)
        _call("kagnn_gat_logits", _ptr(xh), _ld(xh), n, heads, channels, _ptr(a_s), _ptr(a_d), _ptr(ls), _ptr(ld_), _stream())
        out = torch.empty((n, heads * channels), dtype=torch.float32, device=dev)
        m = torch.empty((n, heads), dtype=torch.float32, device=dev)
        z = torch.empty((n, heads), dtype=torch.float32, device=dev)
        _call("kagnn_gat_fwd", _ptr(xh), _ld(xh), _ptr(ls), _ptr(ld_), _ptr(g.rowptr), _ptr(g.col), n, heads, channels,
              _ptr(b), _ptr(out), heads * channels, _ptr(m), _ptr(z), _ptr(g.hub_seg) if g.num_hub_seg else None,
              g.num_hub_seg, g.hub_threshold, _stream())
        ctx.save_for_backward(xh, a_s, a_d, b, ls, ld_, m, z, out)
        ctx.g, ctx.hc = g, (heads, channels)
        ctx.att_shape = att_src.shape
        return out

    @staticmethod
    @once_differentiable
    @_on_operand_device
    def backward(ctx, gout):
        xh, a_s, a_d, b, ls, ld_, m, z, out = ctx.saved_tensors
        g = ctx.g
        heads, channels = ctx.hc
        gout = _rows(gout)
        n, dev = xh.size(0), xh.device
        f32 = dict(dtype=torch.float32, device=dev)
        gpre = torch.empty(max(g.num_edges, 1) * heads, **f32)
        gself = torch.empty((n, heads), **f32)
        gd = torch.empty((n, heads), **f32)
        gs = torch.empty((n, heads), **f32)
        gx = torch.empty((n, heads * channels), **f32)
        _call("kagnn_gat_bwd", _ptr(xh), _ld(xh), _ptr(gout), _ld(gout), _ptr(out), heads * channels, _ptr(b), _ptr(ls),
              _ptr(ld_), _ptr(m), _ptr(z), _ptr(g.rowptr), _ptr(g.col), _ptr(g.perm), _ptr(g.rowptr_t), _ptr(g.col_t),
              _ptr(g.perm_t), _ptr(a_s), _ptr(a_d), n, heads, channels, _ptr(gpre), _ptr(gself), _ptr(gd), _ptr(gs),
              _ptr(gx), heads * channels, _ptr(g.hub_seg) if g.num_hub_seg else None, g.num_hub_seg, g.hub_threshold,
              _stream())
        if heads * channels <= 1024:                      # [H, C] contractions over the nodes: one pass over xh
            ws = _ws(_sizes("kagnn_gat_att_grad_workspace_bytes", n, heads, channels), dev)
            g_att = torch.empty((2, heads * channels), **f32)
            _call("kagnn_gat_att_grad", _ptr(xh), _ld(xh), _ptr(gs), _ptr(gd), n, heads, channels, _ptr(g_att),
                  ctypes.c_void_p(g_att.data_ptr() + 4 * heads * channels), _ptr(ws), ws.numel(), _stream())
            g_att_src, g_att_dst = g_att[0].reshape(ctx.att_shape), g_att[1].reshape(ctx.att_shape)
        else:
            x3 = xh.reshape(n, heads, channels) if xh.is_contiguous() else xh.contiguous().view(n, heads, channels)
            g_att_src = torch.einsum("nh,nhc->hc", gs, x3).reshape(ctx.att_shape)
            g_att_dst = torch.einsum("nh,nhc->hc", gd, x3).reshape(ctx.att_shape)
        g_bias = gout.sum(0) if b is not None else None
        return gx, g_att_src, g_att_dst, g_bias, None, None, None


def gat_aggregate(xh, att_src, att_dst, bias, g: GraphIndex, heads: int, channels: int) -> torch.Tensor:
    """GATConv message passing on ``xh = lin(x)`` (heads concatenated): see csrc/gat.hip."""
    return _GatFn.apply(xh, att_src, att_dst, bias, g, int(heads), int(channels))


# ======================================================================== BatchNorm1d (conv epilogue)
def _batchnorm_fwd_raw(x, weight, bias, running_mean, running_var, training, momentum, eps, moments=None,
                       dropout_p=0.0, dropout_seed=0):
    """-> (y, save_mean, save_rstd); running statistics are updated in place by the kernel.  ``moments``: the [2, F]
    column moments of x from its producer (no statistics pass); ``dropout_p`` > 0: y = dropout(bn(x)) in the same pass"""
    n, f = x.shape
    ws = _ws(_sizes("kagnn_batchnorm_workspace_bytes", n, f), x.device)
    y = torch.empty((n, f), dtype=torch.float32, device=x.device)
    mean = torch.empty(f, dtype=torch.float32, device=x.device)
    rstd = torch.empty(f, dtype=torch.float32, device=x.device)
    w = None if weight is None else weight.contiguous()
    b = None if bias is None else bias.contiguous()
    use_mom = moments is not None and training
    _call("kagnn_batchnorm_fwd", _ptr(x), _ld(x), n, f, _ptr(w), _ptr(b), _ptr(running_mean), _ptr(running_var),
          float(momentum), float(eps), int(bool(training)), _ptr(moments[0]) if use_mom else None,
          _ptr(moments[1]) if use_mom else None, float(dropout_p), int(dropout_seed), _ptr(y), f, _ptr(mean),
          _ptr(rstd), _ptr(ws), ws.numel(), _stream())
    return y, mean, rstd


def _batchnorm_bwd_raw(x, gy, weight, mean, rstd, training, want_gx, want_bias, dropout_p=0.0, dropout_seed=0):
    n, f = x.shape
    w = None if weight is None else weight.contiguous()
    ws = _ws(_sizes("kagnn_batchnorm_workspace_bytes", n, f), x.device)
    gx = torch.empty((n, f), dtype=torch.float32, device=x.device) if want_gx else None
    gw = torch.empty(f, dtype=torch.float32, device=x.device) if w is not None else None
    gb = torch.empty(f, dtype=torch.float32, device=x.device) if want_bias else None
    _call("kagnn_batchnorm_bwd", _ptr(x), _ld(x), _ptr(gy), _ld(gy), n, f, _ptr(w), _ptr(mean), _ptr(rstd),
          int(training), float(dropout_p), int(dropout_seed), _ptr(gx), f, _ptr(gw), _ptr(gb), _ptr(ws), ws.numel(),
          _stream())
    return gx, gw, gb


class _BatchNormFn(Function):
    @staticmethod
    @_on_operand_device
    def forward(ctx, x, weight, bias, running_mean, running_var, training, momentum, eps, moments=None, dropout_p=0.0,
                dropout_seed=0):
        _need_cuda(x, weight, bias, running_mean, running_var, moments)
        x = _rows(x)
        y, mean, rstd = _batchnorm_fwd_raw(x, weight, bias, running_mean, running_var, training, momentum, eps, moments,
                                           dropout_p, dropout_seed)
        ctx.save_for_backward(x, weight, mean, rstd)
        ctx.training = bool(training)
        ctx.dropout = (float(dropout_p), int(dropout_seed))
        ctx.has_bias = bias is not None
        return y                      # running statistics are grad-free buffers, updated in place by the kernel

    @staticmethod
    @once_differentiable
    @_on_operand_device
    def backward(ctx, gy):
        x, w, mean, rstd = ctx.saved_tensors
        gx, gw, gb = _batchnorm_bwd_raw(x, _rows(gy), w, mean, rstd, ctx.training, ctx.needs_input_grad[0], ctx.has_bias,
                                        *ctx.dropout)
        return gx, gw, gb, None, None, None, None, None, None, None, None


def dropout_seed() -> int:
    """a fresh 63-bit seed for the fused dropout, drawn from torch's CPU default generator (``torch.manual_seed``
    reproduces it; no device work)"""
    return int(torch.empty((), dtype=torch.int64).random_().item()) & 0x7FFFFFFFFFFFFFFF


def batch_norm(x, weight, bias, running_mean, running_var, training: bool, momentum: float, eps: float,
               moments: Optional[torch.Tensor] = None, dropout_p: float = 0.0, seed: Optional[int] = None):
    """torch.nn.functional.batch_norm on [N, F] rows (reference ``models.py:195-202`` epilogue).

    The fused epilogue of SURVEY.md 8(f) rank 1: ``moments`` = the [2, F] column moments of ``x`` left by the kernel
    that produced it (``gin_kan_layer(..., moments=True)``) replaces the statistics pass in training; ``dropout_p`` > 0
    (training) returns ``dropout(batch_norm(x), p)`` from the same kernel, the mask being a hash of (seed, row, column)
    that the backward regenerates -- same distribution as ``F.dropout``, not torch's random stream."""
    if x.size(0) == 0:
        return x.new_empty(x.shape)
    if not 0.0 <= dropout_p <= 1.0:
        raise ValueError(f"dropout probability has to be between 0 and 1, but got {dropout_p}")
    p = float(dropout_p) if training else 0.0
    if torch.compiler.is_compiling():
        from . import library
        y = library.batch_norm_traced(x, weight, bias, running_mean, running_var, bool(training), float(momentum), float(eps))
        return torch.nn.functional.dropout(y, p, True) if p > 0.0 else y
    if p > 0.0 and seed is None:
        seed = dropout_seed()
    return _BatchNormFn.apply(x, weight, bias, running_mean, running_var, training, momentum, eps, moments, p,
                              seed if p > 0.0 else 0)


class _ConcatColumnsFn(Function):
    """torch.cat(dim=1) whose backward hands every branch a CONTIGUOUS gradient (stock cat backward returns
    strided column slices, which sends BatchNorm1d's backward down a ~15x slower non-contiguous kernel)."""

    @staticmethod
    @_on_operand_device
    def forward(ctx, *parts):
        ctx.widths = [p.size(1) for p in parts]
        return torch.cat(parts, dim=1)

    @staticmethod
    @once_differentiable
    @_on_operand_device
    def backward(ctx, g):
        return tuple(c.contiguous() for c in torch.split(g, ctx.widths, dim=1))


def concat_columns(parts) -> torch.Tensor:
    """Skip-concatenation of the node models (reference ``models.py:200-201``: ``torch.cat(outs, dim=1)``)."""
    return _ConcatColumnsFn.apply(*parts)


def _fits32(x, width) -> bool:
    """The split kernels address activations with 32-bit byte offsets inside per-tile buffer windows: any number of
    rows, row strides up to 7680 floats (wider inputs take the exact-fp32 kernels)."""
    return max(x.stride(0) if x.dim() == 2 else 0, x.size(-1), width) <= 7680


def fastkan_layer(x, ln_weight, ln_bias, spline_weight, base_weight, base_bias, centers,
                  denominator: float, ln_eps: float = 1e-5, mode: Optional[int] = None) -> torch.Tensor:
    """FastKANLayer.forward (fastkan.py:76-85) on 2-D input."""
    if mode is None:
        mode = default_precision()
    if split_like(mode) and not _fits32(x, spline_weight.size(0)):
        mode = PREC_FP32
    ng = centers.numel()
    if split_like(mode) and ng > 16:
        # more than 16 centres: the layer is a sum over groups of centres (each <= 16, split-precision kernels);
        # every group normalises x the same way, the base branch rides with the first
        fout, fin = spline_weight.size(0), spline_weight.size(1) // ng
        w3 = spline_weight.view(fout, fin, ng)
        groups = -(-ng // 16)
        size, extra = divmod(ng, groups)
        y, c0 = None, 0
        one_group = _FastKANFn.apply
        if torch.compiler.is_compiling():                 # traced code: every group is one opaque kagnn::fastkan_layer op
            from . import library
            one_group = lambda *a: library.fastkan_layer(*a)[0]
        for g in range(groups):
            cg = size + (1 if g < extra else 0)
            part = one_group(x, ln_weight, ln_bias, w3[:, :, c0:c0 + cg].reshape(fout, fin * cg),
                             base_weight if g == 0 else None, base_bias if g == 0 else None,
                             centers[c0:c0 + cg], float(denominator), float(ln_eps), int(mode))
            y = part if y is None else y + part
            c0 += cg
        return y
    if torch.compiler.is_compiling():
        from . import library
        return library.fastkan_layer(x, ln_weight, ln_bias, spline_weight, base_weight, base_bias, centers,
                                     float(denominator), float(ln_eps), int(mode))[0]
    return _FastKANFn.apply(x, ln_weight, ln_bias, spline_weight, base_weight, base_bias, centers,
                            float(denominator), float(ln_eps), int(mode))


# ======================================================================== symbolic fits of edge functions (csrc/symbolic.hip)
# the fixed library of kagnn_symbolic_fit, in id order (include/kagnn_hip.h)
SYMBOLIC_FUNCTIONS = ("x", "x^2", "x^3", "x^4", "1/x", "1/x^2", "sqrt", "1/sqrt(x)", "exp", "log", "abs", "sin", "cos", "tan", "tanh",
                      "sgn", "arctan", "gaussian", "silu")


class SymbolicFit(NamedTuple):
    """what ``symbolic_fit`` returns.  ``functions``: the fitted names, the order of dimension 0 of ``params [F, out, in, 4]``
    (``a, b, c, d`` of ``phi ~ c f(a x + b) + d``) and ``r2 [F, out, in]``.  With ``tables=True`` also every iteration's score
    table ``[iterations, F, out, in, Gn, Gn]``, ranges ``[iterations, F, out, in, 4]`` (``a_lo, a_hi, b_lo, b_hi``) and winning
    flat index ``a_id * Gn + b_id``, int32 ``[iterations, F, out, in]``; else ``None``."""
    functions: Tuple[str, ...]
    params: torch.Tensor
    r2: torch.Tensor
    tables: Optional[torch.Tensor] = None
    ranges: Optional[torch.Tensor] = None
    winners: Optional[torch.Tensor] = None


def symbolic_fit(x, phi, functions=None, a_range=(-10, 10), b_range=(-10, 10), grid_number: int = 101, iterations: int = 3,
                 tables: bool = False) -> SymbolicFit:
    """For every edge function ``phi[:, o, i]`` sampled on the rows ``x[:, i]`` and every function ``f`` of ``functions`` (names of
    ``SYMBOLIC_FUNCTIONS``; default: all), the best ``c f(a x + b) + d`` and its ``R^2`` -- pykan's ``suggest_symbolic`` /
    ``fit_params`` for all edges of a layer at once, on the device.  ``x [N, in]`` fp32 (a row stride is allowed), ``phi [N, out, in]``
    fp32 contiguous: what ``kan_edge_curves(x, ...)`` / ``fastkan_edge_curves(x, ...)`` return.  The search is a ``grid_number`` x
    ``grid_number`` grid over ``(a, b)`` on ``a_range`` x ``b_range``, zoomed ``iterations - 1`` times around the winner, per axis;
    the rule (scores, degenerate candidates, ties, zoom) is stated at ``kagnn_symbolic_fit`` in include/kagnn_hip.h.  Deterministic.
    ``tables=True`` (tests, debugging, small shapes) also returns every iteration's score table, ranges and winner.
    Not differentiable."""
    names = tuple(SYMBOLIC_FUNCTIONS if functions is None else functions)
    if not names:
        raise ValueError("symbolic_fit: no functions given")
    for nm in names:
        if nm not in SYMBOLIC_FUNCTIONS:
            raise ValueError(f"symbolic_fit: unknown function {nm!r}; the library is {', '.join(SYMBOLIC_FUNCTIONS)}")
    if len(set(names)) != len(names):
        raise ValueError("symbolic_fit: a function is listed twice")
    gn, its = int(grid_number), int(iterations)
    if not 3 <= gn <= _lib.SYMBOLIC_MAX_GRID:
        raise ValueError(f"symbolic_fit: grid_number must be 3..{_lib.SYMBOLIC_MAX_GRID} (got {grid_number})")
    if not 1 <= its <= _lib.SYMBOLIC_MAX_ITERATIONS:
        raise ValueError(f"symbolic_fit: iterations must be 1..{_lib.SYMBOLIC_MAX_ITERATIONS} (got {iterations})")
    if x.dtype != torch.float32 or phi.dtype != torch.float32:
        raise TypeError(f"kagnn_amd kernels are fp32; got {x.dtype} and {phi.dtype}")
    if x.dim() != 2 or phi.dim() != 3 or phi.size(0) != x.size(0) or phi.size(2) != x.size(1) or x.size(1) < 1 or phi.size(1) < 1:
        raise ValueError(f"symbolic_fit: x must be [N, in] and phi [N, out, in]; got {tuple(x.shape)} and {tuple(phi.shape)}")
    if not phi.is_contiguous():
        raise ValueError("symbolic_fit: phi must be contiguous [N, out, in] (what edge_curves returns)")
    ranges_host = [float(a_range[0]), float(a_range[1]), float(b_range[0]), float(b_range[1])]
    if not all(math.isfinite(v) for v in ranges_host):
        raise ValueError("symbolic_fit: a_range and b_range must be finite")
    _need_cuda(x, phi)
    x, phi = _rows(x.detach()), phi.detach()
    n, fout, fin = phi.shape
    f, dev = len(names), x.device
    ids = (ctypes.c_int32 * f)(*[SYMBOLIC_FUNCTIONS.index(nm) for nm in names])
    params = torch.empty((f, fout, fin, 4), dtype=torch.float32, device=dev)
    r2 = torch.empty((f, fout, fin), dtype=torch.float32, device=dev)
    tab = rng = win = None
    if tables:
        tab = torch.zeros((its, f, fout, fin, gn, gn), dtype=torch.float32, device=dev)
        rng = torch.zeros((its, f, fout, fin, 4), dtype=torch.float32, device=dev)
        win = torch.zeros((its, f, fout, fin), dtype=torch.int32, device=dev)
    if n == 0:                           # nothing to fit: zeros, and no call
        return SymbolicFit(names, params.zero_(), r2.zero_(), tab, rng, win)
    ws = _ws(_sizes("kagnn_symbolic_fit_workspace_bytes", n, fin, fout, f), dev)
    with _device_of(x):
        _call("kagnn_symbolic_fit", _ptr(x), _ld(x), _ptr(phi), n, fin, fout, ids, f, *ranges_host, gn, its, _ptr(params), _ptr(r2),
              _ptr(tab), _ptr(rng), _ptr(win), _ptr(ws), ws.numel(), _stream())
    return SymbolicFit(names, params, r2, tab, rng, win)


# ======================================================================== fixed symbolic edges (csrc/symbolic_edges.hip)
class SymbolicEdges:
    """A validated list of fixed symbolic edges of one layer: ``edges`` = ``(o, i, name)`` triples (any order; a pair at most once),
    sorted here by ``(o, i)``.  ``triples``: the sorted host tuples ``(o, i, function id)``; ``index``: the same as int32 ``[E, 3]`` on
    ``device``; ``plan_host`` / ``plan``: the library's plan of the list (``kagnn_symbolic_edges_plan``: validated once, here) on the
    host and on the device.  Build one per change of the list; row ``e`` of the ``affine [E, 4]`` operand of ``symbolic_edges``
    belongs to ``triples[e]``."""

    def __init__(self, edges, in_features: int, out_features: int, device):
        fin, fout = int(in_features), int(out_features)
        if fin < 1 or fout < 1:
            raise ValueError(f"SymbolicEdges: in_features and out_features must be >= 1 (got {in_features}, {out_features})")
        triples = []
        for rec in edges:
            o, i, f = rec
            if isinstance(f, str):
                if f not in SYMBOLIC_FUNCTIONS:
                    raise ValueError(f"SymbolicEdges: unknown function {f!r}; the library is {', '.join(SYMBOLIC_FUNCTIONS)}")
                f = SYMBOLIC_FUNCTIONS.index(f)
            triples.append((int(o), int(i), int(f)))
        triples.sort()
        self.triples: Tuple[Tuple[int, int, int], ...] = tuple(triples)
        self.in_features, self.out_features = fin, fout
        self._build(torch.device(device))

    @classmethod
    def from_sorted(cls, triples, in_features: int, out_features: int, device) -> "SymbolicEdges":
        """the list AS GIVEN, ``(o, i, function id)`` integer triples: an unsorted list, a repeated pair, an edge outside the layer
        or an unknown id are refused by the library's own validation"""
        self = cls.__new__(cls)
        self.triples = tuple((int(o), int(i), int(f)) for o, i, f in triples)
        self.in_features, self.out_features = int(in_features), int(out_features)
        self._build(torch.device(device))
        return self

    def _build(self, device) -> None:
        e = len(self.triples)
        host = torch.tensor(self.triples, dtype=torch.int32).reshape(e, 3).contiguous()
        if self.in_features < 1 or self.out_features < 1 or e > self.in_features * self.out_features:
            raise ValueError(f"SymbolicEdges: {e} edges do not fit a layer of {self.out_features} x {self.in_features}")
        nbytes = _sizes("kagnn_symbolic_edges_plan_bytes", e, self.in_features, self.out_features)
        self.plan_host = torch.zeros(nbytes // 4, dtype=torch.int32)
        try:
            _call("kagnn_symbolic_edges_plan", _ptr(host), e, self.in_features, self.out_features, _ptr(self.plan_host), nbytes)
        except RuntimeError as ex:
            raise ValueError(str(ex)) from None
        self.index = host.to(device)
        self.plan = self.plan_host.to(device)

    def __len__(self):
        return len(self.triples)

    @property
    def device(self):
        return self.plan.device


def symbolic_edges_workspace_bytes(num_rows: int, num_edges: int) -> int:
    """the backward's workspace (``kagnn_symbolic_edges_bwd_workspace_bytes``): a function of the two counts, no device needed"""
    return _sizes("kagnn_symbolic_edges_bwd_workspace_bytes", int(num_rows), int(num_edges))


class _SymbolicEdgesFn(Function):
    @staticmethod
    @_on_operand_device
    def forward(ctx, x, affine, y_in, edges):
        x = _rows(x.detach())
        aff = affine.detach().contiguous()
        yi = None if y_in is None else _rows(y_in.detach())
        n, fout = x.size(0), edges.out_features
        y = torch.empty((n, fout), dtype=torch.float32, device=x.device)
        _call("kagnn_symbolic_edges_fwd", _ptr(x), _ld(x), n, edges.in_features, fout, _ptr(edges.plan_host), _ptr(edges.plan),
              _ptr(aff), _ptr(yi), 0 if yi is None else _ld(yi), _ptr(y), fout, _stream())
        ctx.save_for_backward(x, aff)
        ctx.edges = edges
        return y

    @staticmethod
    @once_differentiable
    @_on_operand_device
    def backward(ctx, gy):
        x, aff = ctx.saved_tensors
        edges = ctx.edges
        need = ctx.needs_input_grad
        gaff = gx = None
        if need[0] or need[1]:
            g = _rows(gy)
            n, e = x.size(0), len(edges)
            gx = torch.empty((n, edges.in_features), dtype=torch.float32, device=x.device) if need[0] else None
            gaff = torch.empty((e, 4), dtype=torch.float32, device=x.device)
            ws = _ws(symbolic_edges_workspace_bytes(n, e), x.device)
            _call("kagnn_symbolic_edges_bwd", _ptr(x), _ld(x), _ptr(g), _ld(g), n, edges.in_features, edges.out_features,
                  _ptr(edges.plan_host), _ptr(edges.plan), _ptr(aff), _ptr(gx), edges.in_features, _ptr(gaff), _ptr(ws), ws.numel(),
                  _stream())
        return gx, (gaff if need[1] else None), (gy if need[2] else None), None


def symbolic_edges(x, edges: SymbolicEdges, affine, out_features: int, y: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``y[n,o] + sum over the fixed edges (o, i, f) of c f(a x[n,i] + b) + d`` (``y`` absent: the sum alone) -- the symbolic part
    of a layer with fixed edges, ``[N, out_features]``.  ``x [N, in]`` fp32 (a row stride is allowed), ``edges``: a
    ``SymbolicEdges``, ``affine [E, 4]`` = ``(a, b, c, d)`` per edge of ``edges.triples``, ``y [N, out_features]`` typically the spline
    part's output.  One tape node, differentiable in ``x``, ``affine`` and ``y`` (whose gradient is the incoming one itself); exact
    fp32, deterministic, nothing of size ``N x E``; the formulae are stated at ``kagnn_symbolic_edges_fwd`` in include/kagnn_hip.h.
    The plain functions: ``sqrt`` / ``log`` outside their domain and ``1/x`` at 0 give what IEEE gives.  No edge or no row: no
    launch (``y`` or zeros; zero gradients)."""
    if not isinstance(edges, SymbolicEdges):
        raise TypeError("symbolic_edges: edges must be an ops.SymbolicEdges")
    fout = int(out_features)
    if fout != edges.out_features:
        raise ValueError(f"symbolic_edges: the list was built for {edges.out_features} outputs, not {out_features}")
    if x.dim() != 2 or x.size(1) != edges.in_features:
        raise ValueError(f"symbolic_edges: x must be [N, {edges.in_features}]; got {tuple(x.shape)}")
    if affine.shape != (len(edges), 4):
        raise ValueError(f"symbolic_edges: affine must be [{len(edges)}, 4]; got {tuple(affine.shape)}")
    if y is not None and y.shape != (x.size(0), fout):
        raise ValueError(f"symbolic_edges: y must be [{x.size(0)}, {fout}]; got {tuple(y.shape)}")
    for t in (x, affine, y):
        if t is not None and t.dtype != torch.float32:
            raise TypeError(f"kagnn_amd kernels are fp32; got {t.dtype}")
    _need_cuda(x, affine, y, edges.plan)
    if x.size(0) == 0 or len(edges) == 0:                     # nothing to evaluate: no launch
        base = y.clone() if y is not None else torch.zeros((x.size(0), fout), dtype=torch.float32, device=x.device)
        if len(edges) and affine.requires_grad and torch.is_grad_enabled():
            base = base + 0.0 * affine.sum()                   # (no row: the tape still reaches affine, with zeros)
        return base
    return _SymbolicEdgesFn.apply(x, affine, y, edges)
