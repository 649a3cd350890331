"""Device-resident graph datasets and a mini-batch loader that assembles every batch in one kernel launch.

The reference's graph-level scripts draw a reshuffled mini-batch per step from torch_geometric's ``DataLoader``
(``graph_regression/optuna_zinc.py:59-60``, ``graph_classification/graph_classification_utils.py:48-49,109-128``): collated on the
host (``Batch.from_data_list``) and copied over with ``data.to(device)``.  Here the whole dataset lives on the device, collated ONCE
as "one giant batch in dataset order" and indexed once (``kagnn_csr_build``); a mini-batch -- ``x, edge_index, edge_attr, y, batch,
ptr`` and both CSR structures the convolutions need -- is per-graph slices of those arrays with three offsets rebased, made by ONE
``kagnn_batch_assemble`` launch (``csrc/batch.hip``).  No collation on the host, no host-to-device copy per step, no sort per batch.

torch_geometric is not imported: ``DeviceGraphDataset.from_graphs`` takes any objects with ``x / edge_index / edge_attr / y``.
CPU tensors as the place to keep the dataset are refused like everywhere else in this package.

The node-level side: ``NeighborLoader`` cuts the input nodes of ONE graph into mini-batches and samples a fan-out-limited
neighbourhood around each on the device (``ops.sample_neighbors``, ``csrc/subgraph.hip``) -- a ``NodeBatch`` per step for the node
models, again without host collation.

The edge-level side: ``random_link_split`` cuts ONE graph's edges into training / validation / test positives with the
message-passing graph each split may see (torch_geometric's ``RandomLinkSplit``, plain torch ops), and ``LinkSplit.with_negatives``
draws the fixed evaluation negatives on the device (``ops.negative_sample``, ``csrc/linkpred.hip``).
"""
from __future__ import annotations

import ctypes
from typing import Iterable, Optional

import torch

from . import _lib, ops

_ASSEMBLE_FLAG_MESSAGE = ("kagnn_batch_assemble: a mini-batch named a graph id outside the dataset, or its node / edge totals differ from "
                          "the host's figures (the batch's contents are meaningless)")


# ------------------------------------------------------------------------------------------------ host-side arithmetic (no device)
def epoch_order(n: int, shuffle: bool, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """the order in which one epoch visits ``n`` graphs: 0 .. n-1, or ``torch.randperm(n, generator=generator)`` drawn the way
    ``torch.utils.data.RandomSampler`` draws it -- hence the order of torch_geometric's ``DataLoader(shuffle=True, generator=g)``,
    epoch after epoch: without a generator the sampler seeds a fresh one from the global stream, and it ends every epoch with a
    second, unused draw (its empty tail ``randperm(n)[:0]``), which advances the generator for the next epoch"""
    if not shuffle:
        return torch.arange(n, dtype=torch.int64)
    if generator is None:
        generator = torch.Generator()
        generator.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
    order = torch.randperm(n, generator=generator)
    torch.randperm(n, generator=generator)
    return order


def num_batches(n: int, batch_size: int, drop_last: bool) -> int:
    return n // batch_size if drop_last else (n + batch_size - 1) // batch_size


def batch_plan(node_ptr: torch.Tensor, edge_ptr: torch.Tensor, ids: torch.Tensor, batch_size: int, drop_last: bool = False):
    """``(starts, sizes, num_nodes, num_edges)`` -- four lists, one entry per mini-batch -- of the batches that cut ``ids`` (graph ids
    of the dataset, int64, CPU) into runs of ``batch_size``: one vectorised pass over the CPU copies of the dataset's offsets"""
    n = int(ids.numel())
    nb = num_batches(n, batch_size, drop_last)
    starts = torch.arange(nb, dtype=torch.int64) * batch_size
    ends = torch.clamp(starts + batch_size, max=n)
    zero = torch.zeros(1, dtype=torch.int64)
    cn = torch.cat([zero, torch.cumsum(node_ptr[ids + 1] - node_ptr[ids], 0)])
    ce = torch.cat([zero, torch.cumsum(edge_ptr[ids + 1] - edge_ptr[ids], 0)])
    return starts.tolist(), (ends - starts).tolist(), (cn[ends] - cn[starts]).tolist(), (ce[ends] - ce[starts]).tolist()


def random_split_ids(n: int, fractions_or_lengths, generator: Optional[torch.Generator] = None):
    """The index tensors of ``torch.utils.data.random_split(range(n), fractions_or_lengths, generator)`` -- its subsets' ``.indices``,
    int64, CPU -- as the graph-regression scripts draw their train / validation / test sets (``graph_regression/optuna_qm9.py``:
    ``random_split(dataset, [0.8, 0.1, 0.1], generator)``): ``ds[ids]`` is the reference's subset.  Fractions that sum to 1 become
    ``floor(n * fraction)`` each, the remainder handed out one by one from the first split on; explicit lengths must sum to ``n``;
    one ``torch.randperm(n, generator=generator)`` is cut into consecutive runs.  ``generator=None``: torch's default generator, as
    ``random_split`` uses.  Host only."""
    import math
    n, parts = int(n), list(fractions_or_lengths)
    if n < 0 or not parts:
        raise ValueError("random_split_ids: n >= 0 and at least one split")
    if math.isclose(sum(parts), 1) and sum(parts) <= 1:
        if any(f < 0 or f > 1 for f in parts):
            raise ValueError("random_split_ids: fractions lie between 0 and 1")
        lengths = [math.floor(n * f) for f in parts]
        for k in range(n - sum(lengths)):
            lengths[k % len(lengths)] += 1
    else:
        lengths = [int(v) for v in parts]
        if any(v != int(v) or v < 0 for v in parts):
            raise ValueError("random_split_ids: lengths are non-negative integers (or fractions that sum to 1)")
    if sum(lengths) != n:
        raise ValueError(f"random_split_ids: the lengths {lengths} do not add up to n = {n}")
    order = torch.randperm(n, generator=generator) if generator is not None else torch.randperm(n)
    return list(torch.split(order, lengths))


def read_splits(path):
    """The reference's 10-fold split files (``graph_classification/data_splits/<dataset>_splits.json``, read at
    ``graph_classification_utils.py:88-91`` and used at ``:103-124``): ONE line of JSON,
    ``[{"test": [...], "model_selection": [{"train": [...], "validation": [...]}]}, ...]``.  Returns one ``(train, validation, test)``
    triple of int64 index tensors per fold -- ``dataset[train]`` etc. are the reference's ``dataset[train_index]`` views.  Like the
    reference, the LAST non-empty line of the file counts and the first ``model_selection`` entry of a fold is the one used.  Host only."""
    import json
    splits = None
    with open(path, "rt") as f:
        for line in f:
            if line.strip():
                try:
                    splits = json.loads(line)
                except ValueError as ex:
                    raise ValueError(f"{path}: not a split file (one line of JSON, a list of folds): {ex}") from None

    def ids(fold, value, what):
        if not isinstance(value, list) or not all(isinstance(i, int) and not isinstance(i, bool) and i >= 0 for i in value):
            raise ValueError(f"{path}: fold {fold}: '{what}' must be a list of non-negative graph indices")
        return torch.tensor(value, dtype=torch.int64)

    if not isinstance(splits, list) or not splits:
        raise ValueError(f"{path}: not a split file: expected a non-empty JSON list of folds "
                         '[{"test": [...], "model_selection": [{"train": [...], "validation": [...]}]}, ...]')
    out = []
    for k, fold in enumerate(splits):
        sel = fold.get("model_selection") if isinstance(fold, dict) else None
        if not isinstance(fold, dict) or "test" not in fold or not isinstance(sel, list) or not sel or not isinstance(sel[0], dict) \
                or "train" not in sel[0] or "validation" not in sel[0]:
            raise ValueError(f"{path}: fold {k} is not {{'test': [...], 'model_selection': [{{'train': [...], 'validation': [...]}}]}}")
        out.append((ids(k, sel[0]["train"], "train"), ids(k, sel[0]["validation"], "validation"), ids(k, fold["test"], "test")))
    return out


def _normalise_index(index, n: int) -> torch.Tensor:
    """``index`` (slice, list, int64 / bool tensor, anything ``torch.as_tensor`` takes) as int64 positions in [0, n)"""
    if isinstance(index, slice):
        return torch.arange(n, dtype=torch.int64)[index]
    idx = torch.as_tensor(index).detach().cpu()
    if idx.dtype == torch.bool:
        if idx.numel() != n:
            raise IndexError(f"a boolean mask of {idx.numel()} entries indexes a dataset of {n} graphs")
        return idx.nonzero().reshape(-1)
    idx = idx.reshape(-1).to(torch.int64)
    if idx.numel() and (int(idx.min()) < -n or int(idx.max()) >= n):
        raise IndexError(f"graph index out of range for a dataset of {n} graphs")
    return torch.where(idx < 0, idx + n, idx)


def _row_bytes(t: torch.Tensor) -> int:
    rb = (t[0].numel() if t.dim() > 1 else 1) * t.element_size()
    if rb == 0 or rb % 4:
        raise TypeError(f"kagnn_batch_assemble copies rows of a multiple of 4 bytes; one row of a {tuple(t.shape)} {t.dtype} tensor has {rb}")
    return rb


class _Storage:
    """the device-resident arrays of one dataset (shared by every subset view of it)"""
    __slots__ = ("device", "num_graphs", "num_nodes", "num_edges", "x", "src", "dst", "edge_attr", "y", "node_ptr", "edge_ptr",
                 "node_ptr_cpu", "edge_ptr_cpu", "index", "x_row_bytes", "edge_attr_row_bytes", "y_row_bytes", "num_classes")


# ------------------------------------------------------------------------------------------------ the dataset
class DeviceGraphDataset:
    """A dataset of disjoint graphs held on the device in the flat form torch_geometric's ``InMemoryDataset`` stores: ``x [N, ...]``,
    ``edge_index [2, E]`` with node ids in DATASET order, ``node_ptr [G + 1]`` (graph g owns nodes ``node_ptr[g] : node_ptr[g+1]``),
    optional ``edge_attr [E, ...]`` and per-graph targets ``y [G]`` / ``[G, T]``.  Edges must be grouped by graph, in graph order;
    ``edge_ptr [G + 1]`` is derived from that when not given and checked when given.  Construction validates on the host (every
    edge inside its own graph), moves everything to ``device`` once, keeps CPU copies of the two offset arrays only, and indexes
    the whole dataset once (both CSR structures; no hub segments, as for any mini-batch of small graphs).
    ``ds[list / tensor / slice]`` is a subset VIEW on the same storage (the reference's ``dataset[train_index]``)."""

    def __init__(self, x, edge_index, node_ptr, edge_ptr=None, edge_attr=None, y=None, device="cuda", degree_features=None):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("kagnn_amd.data.DeviceGraphDataset keeps the dataset on an MI355X and assembles mini-batches there "
                               f"(libkagnn_hip.so); got device '{device}'. There is no CPU fallback in this package.")
        if (x is None) == (degree_features is None):
            raise ValueError("give node features x, or x=None with degree_features=K (one-hot out-degree features, the reference's "
                             "Degree transform for datasets without node features: K = 36)")
        if degree_features is not None and int(degree_features) < 1:
            raise ValueError("degree_features must be a positive number of classes")
        if x is not None:
            x = torch.as_tensor(x)
        edge_index = torch.as_tensor(edge_index)
        node_ptr = torch.as_tensor(node_ptr).detach().cpu().to(torch.int64).reshape(-1)
        if edge_index.dim() != 2 or edge_index.size(0) != 2 or edge_index.dtype != torch.int64:
            raise ValueError("edge_index must be an int64 tensor of shape [2, E]")
        G, E = node_ptr.numel() - 1, int(edge_index.size(1))
        N = int(x.size(0)) if x is not None else (int(node_ptr[-1]) if node_ptr.numel() else 0)
        if G < 1 or int(node_ptr[0]) != 0 or int(node_ptr[-1]) != N or bool((node_ptr[1:] < node_ptr[:-1]).any()):
            raise ValueError("node_ptr must be non-decreasing offsets [G + 1] from 0 to the number of nodes, G >= 1")
        if N >= 2 ** 31 - 1 or E >= 2 ** 31 - 1:
            raise ValueError("the dataset's node and edge counts must fit int32 (the library's index type)")
        ei = edge_index.detach().cpu()
        if E and (int(ei.min()) < 0 or int(ei.max()) >= N):
            raise ValueError("edge_index holds node ids outside [0, num_nodes)")
        owner = torch.searchsorted(node_ptr, ei[0].contiguous(), right=True) - 1          # graph of every edge's source
        if E and not torch.equal(owner, torch.searchsorted(node_ptr, ei[1].contiguous(), right=True) - 1):
            raise ValueError("an edge joins two different graphs: the graphs of a dataset are disjoint")
        counts = torch.bincount(owner, minlength=G) if E else torch.zeros(G, dtype=torch.int64)
        derived = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts, 0)])
        if E and bool((owner[1:] < owner[:-1]).any()):
            raise ValueError("edges must be grouped by graph, in graph order (torch_geometric's collated storage is)")
        if edge_ptr is not None:
            edge_ptr = torch.as_tensor(edge_ptr).detach().cpu().to(torch.int64).reshape(-1)
            if not torch.equal(edge_ptr, derived):
                raise ValueError("edge_ptr disagrees with the graphs the edges belong to")
        st = _Storage()
        st.device, st.num_graphs, st.num_nodes, st.num_edges = device, G, N, E
        st.node_ptr_cpu, st.edge_ptr_cpu = node_ptr, derived
        if x is not None:
            st.x = x.detach().contiguous().to(device)
            st.x_row_bytes = _row_bytes(x)
        st.edge_attr, st.edge_attr_row_bytes = None, 0
        if edge_attr is not None:
            edge_attr = torch.as_tensor(edge_attr)
            if edge_attr.size(0) != E:
                raise ValueError(f"edge_attr has {edge_attr.size(0)} rows for {E} edges")
            st.edge_attr_row_bytes = _row_bytes(edge_attr)
            st.edge_attr = edge_attr.detach().contiguous().to(device)
        st.y, st.y_row_bytes, st.num_classes = None, 0, None
        if y is not None:
            y = torch.as_tensor(y)
            if y.size(0) != G:
                raise ValueError(f"y has {y.size(0)} rows for {G} graphs (per-graph targets)")
            st.y_row_bytes = _row_bytes(y)
            if not (y.is_floating_point() or y.is_complex()) and y.dim() == 1 and G:
                st.num_classes = int(y.max()) + 1
            st.y = y.detach().contiguous().to(device)
        eid = ei.to(device)
        st.src, st.dst = eid[0].contiguous(), eid[1].contiguous()
        st.node_ptr, st.edge_ptr = node_ptr.to(device), derived.to(device)
        # both structures of the whole dataset, once; the hub threshold is out of reach: a mini-batch's index carries no hub segments
        st.index = ops.GraphIndex(eid, N, hub_threshold=2 ** 31 - 1) if E else None
        if x is None:
            # the reference's Degree transform, once, from the dataset's own by-source offsets (kagnn_degree_one_hot)
            st.x = ops._degree_one_hot_raw(None if st.index is None else st.index.rowptr_t, N, int(degree_features), device)
            st.x_row_bytes = 4 * int(degree_features)
        self._store = st
        self._index = None                      # None = the whole dataset, else int64 graph ids (CPU) of this view

    @classmethod
    def from_graphs(cls, graphs: Iterable, device="cuda", degree_features=None) -> "DeviceGraphDataset":
        """from per-graph objects with ``x``, ``edge_index`` (LOCAL node ids), optionally ``edge_attr`` and ``y`` (one target row per
        graph) -- duck-typed: torch_geometric ``Data`` objects work.  ``degree_features=K``: the graphs' ``x`` is not read (the
        unlabeled TU datasets have none; the node count is ``num_nodes``, else ``x.size(0)``) and the dataset's node features are
        the one-hot out-degrees"""
        if torch.device(device).type != "cuda":
            cls(torch.zeros(1, 1), torch.zeros(2, 0, dtype=torch.int64), [0, 1], device=device)      # (raises: no CPU fallback)
        xs, eis, eas, ys, node_ptr = [], [], [], [], [0]
        for g in graphs:
            ei = torch.as_tensor(g.edge_index)
            if degree_features is None:
                x = torch.as_tensor(g.x)
                n = int(x.size(0))
            else:
                x, n = None, getattr(g, "num_nodes", None)
                if n is None:
                    if getattr(g, "x", None) is None:
                        raise ValueError(f"graph {len(xs)}: neither num_nodes nor x says how many nodes it has")
                    n = torch.as_tensor(g.x).size(0)
                n = int(n)
            if ei.numel() and (int(ei.min()) < 0 or int(ei.max()) >= n):
                raise ValueError(f"graph {len(xs)}: edge_index holds node ids outside [0, {n})")
            xs.append(x)
            eis.append(ei.reshape(2, -1).to(torch.int64) + node_ptr[-1])
            node_ptr.append(node_ptr[-1] + n)
            ea, y = getattr(g, "edge_attr", None), getattr(g, "y", None)
            if ea is not None:
                eas.append(torch.as_tensor(ea))
            if y is not None:
                y = torch.as_tensor(y)
                ys.append(y.reshape(1) if y.dim() == 0 else y)
        if not xs:
            raise ValueError("no graphs")
        if (eas and len(eas) != len(xs)) or (ys and len(ys) != len(xs)):
            raise ValueError("edge_attr / y must be present on every graph or on none")
        return cls(torch.cat(xs) if degree_features is None else None, torch.cat(eis, dim=1), node_ptr,
                   edge_attr=torch.cat(eas) if eas else None, y=torch.cat(ys) if ys else None, device=device,
                   degree_features=degree_features)

    # -- views
    def __len__(self) -> int:
        return self._store.num_graphs if self._index is None else int(self._index.numel())

    def __getitem__(self, index) -> "DeviceGraphDataset":
        if isinstance(index, int):
            index = [index]
        sel = _normalise_index(index, len(self))
        view = object.__new__(type(self))
        view._store = self._store
        view._index = sel if self._index is None else self._index[sel]
        return view

    def global_ids(self, positions: torch.Tensor) -> torch.Tensor:
        """the storage's graph ids of this view's ``positions`` (int64, CPU)"""
        return positions if self._index is None else self._index[positions]

    @property
    def storage(self) -> _Storage:
        return self._store

    @property
    def device(self) -> torch.device:
        return self._store.device

    def standardize_targets(self, columns=None):
        """``(dataset, mean, std)``: the targets of the WHOLE storage standardised as the QM9 script does before it splits
        (``graph_regression/optuna_qm9.py:145-149``): ``y = y[:, columns]`` when ``columns`` (a slice or a list of column indices)
        is given, ``mean = y.mean(0, keepdim=True)``, ``std = y.std(0, keepdim=True)`` (unbiased), ``y = (y - mean) / std``.  The
        returned dataset shares every other array with this one (and keeps this view's selection); ``mean`` and ``std`` are
        ``[1, T]`` device tensors -- ``std`` is what ``l1_loss(scale=...)`` and ``train_graph_regression(target_scale=...)`` take.
        Plain torch on the device, once per dataset."""
        st = self._store
        if st.y is None or not st.y.is_floating_point():
            raise TypeError("standardize_targets: the dataset needs floating-point targets y [G] or [G, T]")
        y = st.y if st.y.dim() > 1 else st.y.reshape(-1, 1)
        if y.dim() != 2:
            raise TypeError(f"standardize_targets: targets are [G] or [G, T], got {tuple(st.y.shape)}")
        if columns is not None:
            y = y[:, columns]
        mean, std = y.mean(dim=0, keepdim=True), y.std(dim=0, keepdim=True)
        new = _Storage()
        for k in _Storage.__slots__:
            if hasattr(st, k):
                setattr(new, k, getattr(st, k))
        new.y = ((y - mean) / std).contiguous()
        new.y_row_bytes = _row_bytes(new.y)
        out = object.__new__(type(self))
        out._store, out._index = new, self._index
        return out, mean, std

    # -- the descriptive attributes the reference's scripts read off a dataset
    @property
    def num_node_features(self) -> int:
        x = self._store.x
        return 1 if x.dim() == 1 else int(x.size(1))

    num_features = num_node_features

    @property
    def num_edge_features(self) -> int:
        ea = self._store.edge_attr
        return 0 if ea is None else (1 if ea.dim() == 1 else int(ea.size(1)))

    @property
    def num_classes(self) -> int:
        """``max(y) + 1`` over the STORAGE's integer targets (a subset view reports its parent's figure)"""
        if self._store.num_classes is None:
            raise AttributeError("num_classes is defined for integer targets y [G]")
        return self._store.num_classes


# ------------------------------------------------------------------------------------------------ a mini-batch
class DeviceBatch:
    """What ``DeviceBatchLoader`` yields: the attributes of a torch_geometric ``Batch`` that the graph-level models and the
    reference's loops read (``x, edge_index, edge_attr, y, batch, ptr, num_graphs``), plus ``graph_index`` -- the batch's two CSR
    structures, assembled with it (absent when the batch has no edges or is beyond the small-graph limits: the model then indexes
    ``edge_index`` itself)."""
    __slots__ = ("x", "edge_index", "edge_attr", "y", "batch", "ptr", "num_graphs", "num_nodes", "num_edges", "graph_index")

    def to(self, device, *args, **kwargs) -> "DeviceBatch":
        """the reference loops call ``data = data.to(device)``: the batch already is on its device"""
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if dev != self.x.device:
            raise RuntimeError(f"this mini-batch was assembled on {self.x.device} and cannot move to {dev}: build the dataset there")
        return self


# ------------------------------------------------------------------------------------------------ the loader
class DeviceBatchLoader:
    """``torch_geometric.loader.DataLoader(dataset, batch_size, shuffle, drop_last=..., generator=...)`` for a
    ``DeviceGraphDataset``: re-iterable, ``len()`` = batches per epoch, ``.dataset``.  Every ``__iter__`` draws the epoch's order on
    the host (``epoch_order``: the sequence torch's ``RandomSampler`` draws for the same generator), sends it to the device in
    ONE non-blocking copy, computes every batch's node / edge totals from the CPU offsets, and then per batch allocates the outputs
    and makes ONE ``kagnn_batch_assemble`` call.  The kernel re-derives the totals and checks the ids; its verdict travels with
    the deferred graph checks (``ops.flush_graph_checks()`` -- ``harness.train_graph_batches`` calls it every epoch)."""

    def __init__(self, dataset: DeviceGraphDataset, batch_size: int = 1, shuffle: bool = False, drop_last: bool = False,
                 generator: Optional[torch.Generator] = None, attach_graph_index: bool = True):
        if not 1 <= int(batch_size) <= _lib.BATCH_MAX_GRAPHS:
            raise ValueError(f"batch_size must be in [1, {_lib.BATCH_MAX_GRAPHS}] (KAGNN_BATCH_MAX_GRAPHS)")
        self.dataset, self.batch_size, self.shuffle, self.drop_last, self.generator = dataset, int(batch_size), shuffle, drop_last, generator
        self.attach_graph_index = attach_graph_index     # False: the model rebuilds the CSR per batch (for A/B measurements)

    def __len__(self) -> int:
        return num_batches(len(self.dataset), self.batch_size, self.drop_last)

    def order(self) -> torch.Tensor:
        """draw one epoch's order: the dataset's (storage) graph ids in the sequence the epoch visits them (int64, CPU)"""
        return self.dataset.global_ids(epoch_order(len(self.dataset), self.shuffle, self.generator))

    def __iter__(self):
        return self.batches_of(self.order())

    def batches_of(self, ids: torch.Tensor):
        """the mini-batches that cut ``ids`` (graph ids of the storage, int64, CPU; repeats allowed) into runs of ``batch_size``"""
        st = self.dataset.storage
        dev = st.device
        ids = torch.as_tensor(ids, dtype=torch.int64).reshape(-1)
        starts, sizes, nodes, edges = batch_plan(st.node_ptr_cpu, st.edge_ptr_cpu, torch.clamp(ids, 0, st.num_graphs - 1), self.batch_size,
                                                 self.drop_last)
        if not starts:
            return
        # the pinned block comes from torch's caching host allocator, which does not hand it out again while the copy is in flight
        pinned = torch.empty(ids.numel(), dtype=torch.int64, pin_memory=True)
        pinned.copy_(ids)
        with ops._device_of(st.x):
            ids_dev = pinned.to(dev, non_blocking=True)
            flags = torch.zeros((len(starts), 2), dtype=torch.int32, device=dev)
        a = _lib.BatchAssemble()
        a.struct_bytes = ctypes.sizeof(_lib.BatchAssemble)
        a.num_graphs_total = st.num_graphs
        a.x_row_bytes, a.edge_attr_row_bytes, a.y_row_bytes = st.x_row_bytes, st.edge_attr_row_bytes, st.y_row_bytes
        a.node_ptr, a.edge_ptr = st.node_ptr.data_ptr(), st.edge_ptr.data_ptr()
        a.x_all = st.x.data_ptr()
        a.edge_attr_all = None if st.edge_attr is None else st.edge_attr.data_ptr()
        a.y_all = None if st.y is None else st.y.data_ptr()
        a.src_all, a.dst_all = st.src.data_ptr(), st.dst.data_ptr()
        gi = st.index
        small_ok = _lib.load().kagnn_csr_small_ok
        x_tail, ea_tail = tuple(st.x.shape[1:]), (() if st.edge_attr is None else tuple(st.edge_attr.shape[1:]))
        y_tail = () if st.y is None else tuple(st.y.shape[1:])
        ids_ptr, flags_ptr = ids_dev.data_ptr(), flags.data_ptr()
        i64, i32 = dict(dtype=torch.int64, device=dev), dict(dtype=torch.int32, device=dev)
        ref = ctypes.byref(a)
        try:
            for b, (s, B, n, e) in enumerate(zip(starts, sizes, nodes, edges)):
                out = DeviceBatch()
                out.num_graphs, out.num_nodes, out.num_edges = B, n, e
                with ops._device_of(st.x):
                    out.x = torch.empty((n, *x_tail), dtype=st.x.dtype, device=dev)
                    out.edge_index = torch.empty((2, e), **i64)
                    out.edge_attr = None if st.edge_attr is None else torch.empty((e, *ea_tail), dtype=st.edge_attr.dtype, device=dev)
                    out.y = None if st.y is None else torch.empty((B, *y_tail), dtype=st.y.dtype, device=dev)
                    out.batch = torch.empty(n, **i64)
                    out.ptr = torch.empty(B + 1, **i64)
                    a.num_graphs, a.num_nodes, a.num_edges = B, n, e
                    a.ids = ids_ptr + 8 * s
                    a.x, a.edge_index, a.batch, a.ptr = out.x.data_ptr(), out.edge_index.data_ptr(), out.batch.data_ptr(), out.ptr.data_ptr()
                    a.edge_attr = None if out.edge_attr is None else out.edge_attr.data_ptr()
                    a.y = None if out.y is None else out.y.data_ptr()
                    a.flags = flags_ptr + 8 * b
                    # the assembled index is attached exactly when the model would have taken the small-graph build: same bits
                    if self.attach_graph_index and gi is not None and small_ok(e, n):
                        rp, co, pe = torch.empty(n + 1, **i32), torch.empty(e, **i32), torch.empty(e, **i32)
                        rpt, cot, pet = torch.empty(n + 1, **i32), torch.empty(e, **i32), torch.empty(e, **i32)
                        a.rowptr_all, a.col_all, a.perm_all = gi.rowptr.data_ptr(), gi.col.data_ptr(), gi.perm.data_ptr()
                        a.rowptr_t_all, a.col_t_all, a.perm_t_all = gi.rowptr_t.data_ptr(), gi.col_t.data_ptr(), gi.perm_t.data_ptr()
                        a.rowptr, a.col, a.perm = rp.data_ptr(), co.data_ptr(), pe.data_ptr()
                        a.rowptr_t, a.col_t, a.perm_t = rpt.data_ptr(), cot.data_ptr(), pet.data_ptr()
                        out.graph_index = ops.GraphIndex.from_arrays(rp, co, pe, rpt, cot, pet, n, e)
                    else:
                        a.rowptr = a.col = a.perm = a.rowptr_t = a.col_t = a.perm_t = None
                        out.graph_index = None
                    ops._call("kagnn_batch_assemble", ref, ops._stream())
                yield out
        finally:
            # one deferred check for the epoch's batches (also when the consumer stops early: rows of batches never assembled are 0)
            with ops._device_of(st.x):
                ops._defer_flag_check(flags, _ASSEMBLE_FLAG_MESSAGE)


# ------------------------------------------------------------------------------------------------ neighbour-sampled node batches
_SEED_STRIDE = 0x9E3779B97F4A7C15      # 2^64 / golden ratio, odd: the multiples i * stride mod 2^64 are distinct for i < 2^64


class NodeBatch:
    """What ``NeighborLoader`` yields: the sampled subgraph around ``seeds`` (``ops.sample_neighbors``) -- ``nodes`` (int64, original
    ids, ascending), ``edge_index`` (int64 ``[2, num_edges]``, relabelled), ``edge_ids`` (original edge ids), ``index`` (the
    ``GraphIndex`` of ``edge_index``: ``model(batch.x, batch.index)``), ``hops`` (int32: the level at which a node was first
    reached) -- and the batch's own rows: ``seeds`` (original ids, in the epoch's order), ``seed_rows`` (their positions in
    ``nodes``: the loss is taken on ``out[batch.seed_rows]``), ``num_seeds``, ``x = x[nodes]`` and ``y = y[seeds]`` where the loader
    was given ``x`` / ``y`` (else ``None``)."""
    __slots__ = ("nodes", "edge_index", "edge_ids", "index", "hops", "seed_rows", "seeds", "num_seeds", "num_nodes", "num_edges", "x", "y")


class NeighborLoader:
    """torch_geometric's ``NeighborLoader(data, num_neighbors=fanouts, input_nodes=..., batch_size=..., shuffle=...)`` on the device:
    re-iterable, ``len()`` = batches per epoch.  ``graph``: an ``ops.GraphIndex`` or ``(edge_index, num_nodes)``; ``input_nodes``:
    int64 ids or a bool mask ``[N]``.  Every ``__iter__`` draws the epoch's order on the host (``epoch_order``, applied to the
    input nodes), sends it to the device in ONE non-blocking copy, and per batch calls ``ops.sample_neighbors`` on a slice of it
    (whose read of the two counts is the batch's only synchronisation) and gathers ``x[nodes]`` / ``y[seeds]``.  No host
    collation, no sort.

    Sampling seeds: batch ``b`` of epoch ``t`` (``t`` counts the orders drawn from this loader, from 0) samples under
    ``(seed + 0x9E3779B97F4A7C15 * (1 + t * len(loader) + b)) mod 2^64`` -- ``sampling_seed(t, b)``.  One ``seed`` therefore
    reproduces a run (together with ``generator`` when ``shuffle``), and no two batches of a run share a sampling seed: the stride
    is odd, so its multiples are distinct mod 2^64.  Which edges a seed keeps: ``kagnn_neighbor_sample_mark`` (kagnn_hip.h)."""

    def __init__(self, graph, input_nodes, fanouts, batch_size: int, shuffle: bool = False, drop_last: bool = False,
                 generator: Optional[torch.Generator] = None, seed: int = 0, x=None, y=None):
        self.fanouts = ops._fanouts("NeighborLoader", fanouts)
        if isinstance(batch_size, bool) or int(batch_size) != batch_size or batch_size < 1:
            raise ValueError(f"NeighborLoader: batch_size must be a positive integer, got {batch_size!r}")
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"NeighborLoader: seed must be an int, got {seed!r}")
        if isinstance(graph, (tuple, list)) and len(graph) == 2 and isinstance(graph[0], torch.Tensor):
            graph = ops.graph_index(graph[0], int(graph[1]))
        if not isinstance(graph, ops.GraphIndex):
            raise TypeError("NeighborLoader: the graph must be an ops.GraphIndex or (edge_index, num_nodes)")
        n = graph.num_nodes
        if not isinstance(input_nodes, torch.Tensor):
            input_nodes = torch.as_tensor(input_nodes)
        if input_nodes.dtype == torch.bool:
            if input_nodes.dim() != 1 or input_nodes.numel() != n:
                raise ValueError(f"NeighborLoader: a node mask must have shape [{n}], got {tuple(input_nodes.shape)}")
            input_nodes = input_nodes.nonzero().flatten()
        elif input_nodes.dtype != torch.int64 or input_nodes.dim() != 1:
            raise ValueError("NeighborLoader: input_nodes must be an int64 vector of node ids or a bool mask of length num_nodes")
        for name, t in (("x", x), ("y", y)):
            if t is not None and (not isinstance(t, torch.Tensor) or t.dim() < 1 or t.size(0) != n):
                raise ValueError(f"NeighborLoader: {name} must have {n} rows, one per node of the graph")
        self.graph, self.input_nodes = graph, input_nodes.cpu().contiguous()        # (the order is drawn on the host)
        self.batch_size, self.shuffle, self.drop_last, self.generator = int(batch_size), bool(shuffle), bool(drop_last), generator
        self.seed, self.x, self.y = seed, x, y
        self.epoch = 0                                    # the number of epoch orders drawn so far: the `t` of the seed formula

    def __len__(self) -> int:
        return num_batches(int(self.input_nodes.numel()), self.batch_size, self.drop_last)

    def sampling_seed(self, epoch: int, batch: int) -> int:
        """the 64-bit seed under which batch ``batch`` of epoch ``epoch`` is sampled (the class docstring's formula)"""
        return (self.seed + _SEED_STRIDE * (1 + int(epoch) * len(self) + int(batch))) & 0xFFFFFFFFFFFFFFFF

    def order(self) -> torch.Tensor:
        """draw one epoch's order -- the input nodes in the sequence the epoch visits them (int64, CPU) -- and count the epoch"""
        self.epoch += 1
        return self.input_nodes[epoch_order(int(self.input_nodes.numel()), self.shuffle, self.generator)]

    def __iter__(self):
        epoch = self.epoch
        return self.batches_of(self.order(), epoch)

    def batches_of(self, ids: torch.Tensor, epoch: int):
        """the mini-batches that cut ``ids`` (node ids, int64, CPU) into runs of ``batch_size``, sampled under ``epoch``'s seeds"""
        g = self.graph
        ops._need_cuda(g.rowptr, self.x, self.y)
        ids = torch.as_tensor(ids, dtype=torch.int64).reshape(-1)
        nb = num_batches(int(ids.numel()), self.batch_size, self.drop_last)
        if nb == 0:
            return
        pinned = torch.empty(ids.numel(), dtype=torch.int64, pin_memory=True)
        pinned.copy_(ids)
        with ops._device_of(g.rowptr):
            ids_dev = pinned.to(g.device, non_blocking=True)
        for b in range(nb):
            seeds = ids_dev[b * self.batch_size:(b + 1) * self.batch_size]
            sub = ops.sample_neighbors(seeds, self.fanouts, g, seed=self.sampling_seed(epoch, b))
            out = NodeBatch()
            out.nodes, out.edge_index, out.edge_ids, out.index, out.hops = sub.nodes, sub.edge_index, sub.edge_ids, sub.index, sub.hops
            out.seed_rows, out.seeds, out.num_seeds = sub.mapping, seeds, int(seeds.numel())
            out.num_nodes, out.num_edges = sub.num_nodes, sub.num_edges
            with ops._device_of(g.rowptr):
                out.x = None if self.x is None else self.x.index_select(0, sub.nodes)
                out.y = None if self.y is None else self.y.index_select(0, seeds)
            yield out


# ------------------------------------------------------------------------------------------------ link prediction: the edge split
class LinkSplit:
    """What ``random_link_split`` returns.  Per split a message-passing graph (int64 ``[2, E]``) and the positive pairs it is
    scored on (int64 ``[2, P]``, ``u`` = row 0, ``v`` = row 1; with ``is_undirected`` the ``u < v`` representative of each edge):
    ``train_edge_index / val_edge_index / test_edge_index`` and ``train_pos / val_pos / test_pos``.  ``edge_index`` is the full edge
    list the split was drawn from, ``num_nodes`` its node count.  ``with_negatives`` adds ``val_neg / test_neg`` (int64 ``[2, P]``)
    and ``val_neg_valid / test_neg_valid`` (uint8 ``[P]``: 0 marks an EMPTY slot of ``ops.negative_sample``, to be given weight 0);
    they are ``None`` before."""
    _FIELDS = ("edge_index", "num_nodes", "is_undirected", "train_edge_index", "val_edge_index", "test_edge_index", "train_pos",
               "val_pos", "test_pos", "val_neg", "val_neg_valid", "test_neg", "test_neg_valid")

    def __init__(self, **kw):
        for k in self._FIELDS:
            setattr(self, k, kw.get(k))

    def __repr__(self):
        sizes = ", ".join(f"{k}={int(getattr(self, k).size(1))}" for k in ("train_pos", "val_pos", "test_pos"))
        return f"LinkSplit(num_nodes={self.num_nodes}, is_undirected={self.is_undirected}, {sizes}, negatives={self.val_neg is not None})"

    def with_negatives(self, seed: int, ratio: float = 1.0) -> "LinkSplit":
        """a copy with FIXED evaluation negatives: ``round(ratio * P)`` slots per split from ``ops.negative_sample`` against the
        FULL edge set (no validation or test edge can be drawn as a negative), seeds ``seed + 1`` (validation) and ``seed + 2``
        (test); drawn once, on the device"""
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"LinkSplit.with_negatives: seed must be an int, got {seed!r}")
        keys = ops.edge_keys(self.edge_index, self.num_nodes)
        out = LinkSplit(**{k: getattr(self, k) for k in self._FIELDS})
        out.val_neg, out.val_neg_valid = ops.negative_sample(round(ratio * self.val_pos.size(1)), keys, self.num_nodes, seed + 1)
        out.test_neg, out.test_neg_valid = ops.negative_sample(round(ratio * self.test_pos.size(1)), keys, self.num_nodes, seed + 2)
        return out


def random_link_split(edge_index: torch.Tensor, num_nodes: int, val_ratio: float = 0.05, test_ratio: float = 0.1,
                      is_undirected: bool = True, generator: Optional[torch.Generator] = None) -> LinkSplit:
    """torch_geometric's ``RandomLinkSplit`` restated in plain torch ops on ``edge_index``'s device (CPU tensors work too, as for
    ``random_split_ids``).  With ``is_undirected`` only the ``u < v`` representative of every edge is split (the list is taken to
    hold both directions; self loops take no part), else every edge is its own representative.  Of the ``E_rep`` representatives,
    in the order of one ``torch.randperm(E_rep, generator=generator)`` drawn on the HOST (the same split on every device),
    ``int(val_ratio * E_rep)`` become validation positives, ``int(test_ratio * E_rep)`` test positives and the rest, which come
    first, training positives.  Message passing: training and validation see the training edges (both directions when
    undirected), the test split sees training plus validation edges -- no pair a split is scored on, nor its reverse, is in the
    graph that split's encoder sees before its turn."""
    if edge_index.dim() != 2 or edge_index.size(0) != 2 or edge_index.dtype != torch.int64:
        raise ValueError("edge_index must be an int64 tensor of shape [2, E]")
    if not (0.0 <= val_ratio and 0.0 <= test_ratio and val_ratio + test_ratio < 1.0):
        raise ValueError(f"random_link_split: ratios are >= 0 and sum to less than 1; got {val_ratio} and {test_ratio}")
    rep = edge_index[:, edge_index[0] < edge_index[1]] if is_undirected else edge_index
    e_rep = int(rep.size(1))
    n_val, n_test = int(val_ratio * e_rep), int(test_ratio * e_rep)
    n_train = e_rep - n_val - n_test
    order = (torch.randperm(e_rep, generator=generator) if generator is not None else torch.randperm(e_rep)).to(edge_index.device)
    train, val, test = (rep[:, ids].contiguous() for ids in torch.split(order, [n_train, n_val, n_test]))

    def graph(pairs):
        return torch.cat([pairs, pairs.flip(0)], dim=1).contiguous() if is_undirected else pairs
    train_graph = graph(train)
    return LinkSplit(edge_index=edge_index, num_nodes=int(num_nodes), is_undirected=bool(is_undirected), train_edge_index=train_graph,
                     val_edge_index=train_graph, test_edge_index=graph(torch.cat([train, val], dim=1)), train_pos=train, val_pos=val,
                     test_pos=test)
