"""Host side of kagnn_amd.data (device-resident datasets, one-launch mini-batch assembly): everything that needs no GPU.

The yardstick for collation is ``collate`` below: a plain torch restatement (``torch.cat`` of per-graph slices, ``edge_index`` +
node offset, ``repeat_interleave`` for ``batch``, ``cumsum`` for ``ptr``) -- the definition of torch_geometric's
``Batch.from_data_list`` for these attributes; tests/test_gpu_data.py holds the same function and compares the kernel with it."""
import ctypes
import os
import re

import pytest
import torch

import kagnn_amd
from kagnn_amd import _lib, data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def collate(x, edge_index, node_ptr, edge_ptr, ids, edge_attr=None, y=None):
    ids = [int(g) for g in ids]
    sizes = torch.tensor([int(node_ptr[g + 1] - node_ptr[g]) for g in ids], dtype=torch.int64)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)])
    out = {"x": torch.cat([x[node_ptr[g]:node_ptr[g + 1]] for g in ids]),
           "edge_index": torch.cat([edge_index[:, edge_ptr[g]:edge_ptr[g + 1]] - node_ptr[g] + ptr[k] for k, g in enumerate(ids)], dim=1),
           "batch": torch.repeat_interleave(torch.arange(len(ids)), sizes), "ptr": ptr}
    if edge_attr is not None:
        out["edge_attr"] = torch.cat([edge_attr[edge_ptr[g]:edge_ptr[g + 1]] for g in ids])
    if y is not None:
        out["y"] = torch.cat([y[g:g + 1] for g in ids])
    return out


def _lib_loaded():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_batch_assemble_struct_mirror_matches_the_header():
    """kagnn_batch_assemble_t (include/kagnn_hip.h) against its ctypes mirror kagnn_amd._lib.BatchAssemble: the same field names in
    the same order (every field is 8 bytes wide, so name order + size pin the layout) and the size of the built library's struct"""
    src = open(os.path.join(ROOT, "include", "kagnn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    body = re.search(r"typedef struct kagnn_batch_assemble \{(.*?)\} kagnn_batch_assemble_t;", src, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        for part in decl.strip().split(","):
            if part.strip():
                names.append(re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*(\[[^\]]*\])?$", part.strip()).group(1))
    mirror = [f[0] for f in _lib.BatchAssemble._fields_]
    assert names == mirror, [(a, b) for a, b in zip(names, mirror) if a != b][:5]
    assert all(ctypes.sizeof(f[1]) == 8 for f in _lib.BatchAssemble._fields_)
    lib = _lib_loaded()
    assert lib.kagnn_batch_assemble_struct_bytes() == ctypes.sizeof(_lib.BatchAssemble) == 8 * len(mirror)
    limit = int(re.search(r"#define KAGNN_BATCH_MAX_GRAPHS (\d+)", src).group(1))
    assert limit == _lib.BATCH_MAX_GRAPHS >= 4096


def test_batch_assemble_refuses_bad_arguments_before_any_device_call():
    lib = _lib_loaded()
    assert lib.kagnn_batch_assemble(None, None) == -1                                   # KAGNN_ERR_ARG: null struct
    assert b"null" in lib.kagnn_last_error()
    a = _lib.BatchAssemble()
    a.struct_bytes = ctypes.sizeof(a) - 8
    assert lib.kagnn_batch_assemble(ctypes.byref(a), None) == -1                        # KAGNN_ERR_ARG: another header's struct
    assert b"struct_bytes" in lib.kagnn_last_error()
    a.struct_bytes = ctypes.sizeof(a)
    a.num_graphs_total, a.num_graphs = 10 ** 6, _lib.BATCH_MAX_GRAPHS + 1
    assert lib.kagnn_batch_assemble(ctypes.byref(a), None) == -3                        # KAGNN_ERR_UNSUPPORTED: B above the limit
    assert b"KAGNN_BATCH_MAX_GRAPHS" in lib.kagnn_last_error()
    a.num_graphs = 4
    assert lib.kagnn_batch_assemble(ctypes.byref(a), None) == -1                        # null arrays
    with pytest.raises(ValueError, match="KAGNN_BATCH_MAX_GRAPHS"):
        data.DeviceBatchLoader(_Stub(10), batch_size=_lib.BATCH_MAX_GRAPHS + 1)


def test_dataset_refuses_cpu_only_use():
    x, ei = torch.zeros(3, 1), torch.zeros(2, 2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kagnn_amd.DeviceGraphDataset(x, ei, [0, 3], device="cpu")
    from types import SimpleNamespace
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kagnn_amd.DeviceGraphDataset.from_graphs([SimpleNamespace(x=x, edge_index=ei)], device="cpu")


class _Stub:
    """what DeviceBatchLoader asks of a dataset before it touches the device: a length and the view's graph ids"""

    def __init__(self, n, index=None):
        self.n, self.index = n, index

    def __len__(self):
        return self.n if self.index is None else int(self.index.numel())

    def global_ids(self, positions):
        return positions if self.index is None else self.index[positions]


def test_epoch_order_is_the_random_samplers():
    from torch.utils.data import RandomSampler
    n = 1237
    for seed in (0, 5):
        g1, g2, g3 = (torch.Generator().manual_seed(seed) for _ in range(3))
        loader = data.DeviceBatchLoader(_Stub(n), batch_size=64, shuffle=True, generator=g1)
        for _epoch in range(3):                                    # the generator's state carries over from epoch to epoch
            got = loader.order()
            assert torch.equal(got, torch.randperm(n, generator=g2))
            torch.randperm(n, generator=g2)                        # (the sampler's unused second draw at the end of an epoch)
            assert got.tolist() == list(RandomSampler(range(n), generator=g3))
    torch.manual_seed(11)                                          # no generator: the sampler seeds one from the global stream
    got = data.DeviceBatchLoader(_Stub(n), batch_size=64, shuffle=True).order()
    torch.manual_seed(11)
    assert got.tolist() == list(RandomSampler(range(n)))
    assert torch.equal(data.DeviceBatchLoader(_Stub(n), batch_size=64).order(), torch.arange(n))
    # through a subset view: positions of the view in sampler order, mapped to the storage's graph ids
    index = torch.tensor([9, 3, 3, 7, 0])
    got = data.DeviceBatchLoader(_Stub(10, index), batch_size=2, shuffle=True, generator=torch.Generator().manual_seed(1)).order()
    assert torch.equal(got, index[torch.randperm(5, generator=torch.Generator().manual_seed(1))])


def test_loader_len_with_and_without_drop_last():
    for n, bs in ((1000, 256), (1024, 256), (5, 8), (1, 1), (0, 4)):
        assert len(data.DeviceBatchLoader(_Stub(n), batch_size=bs)) == -(-n // bs)
        assert len(data.DeviceBatchLoader(_Stub(n), batch_size=bs, drop_last=True)) == n // bs


def test_a_subset_of_a_subset_names_the_storages_graphs():
    ds = object.__new__(kagnn_amd.DeviceGraphDataset)              # (the view arithmetic is host-only: no storage needed)
    ds._store, ds._index = type("S", (), {"num_graphs": 20})(), None
    assert len(ds) == 20
    a = ds[torch.arange(19, -1, -2)]                               # 19, 17, ..., 1
    assert len(a) == 10 and a._store is ds._store
    b = a[[0, 3, -1]]
    assert b._index.tolist() == [19, 13, 1]
    assert b[1:]._index.tolist() == [13, 1] and b[torch.tensor([True, False, True])]._index.tolist() == [19, 1]
    assert b.global_ids(torch.tensor([2, 2, 0])).tolist() == [1, 1, 19]
    with pytest.raises(IndexError):
        a[[10]]


def test_batch_plan_matches_the_restatement():
    g = torch.Generator().manual_seed(3)
    G = 300
    sizes = torch.randint(0, 9, (G,), generator=g)                 # (graphs without nodes and without edges included)
    esizes = torch.where(sizes > 0, torch.randint(0, 14, (G,), generator=g), torch.zeros(G, dtype=torch.int64))
    node_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)])
    edge_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(esizes, 0)])
    x = torch.arange(int(node_ptr[-1])).reshape(-1, 1)
    lo = torch.repeat_interleave(node_ptr[:-1], esizes)
    ei = torch.stack([lo, lo])
    for bs, drop in ((64, False), (64, True), (1, False), (300, False), (7, True)):
        ids = torch.randint(0, G, (G,), generator=g)               # repeats allowed
        starts, counts, nodes, edges = data.batch_plan(node_ptr, edge_ptr, ids, bs, drop)
        assert len(starts) == data.num_batches(G, bs, drop)
        for s, c, n, e in zip(starts, counts, nodes, edges):
            ref = collate(x, ei, node_ptr, edge_ptr, ids[s:s + c])
            assert c == min(bs, G - s) and n == ref["x"].size(0) and e == ref["edge_index"].size(1)
