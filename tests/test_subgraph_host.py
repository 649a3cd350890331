"""Subgraph extraction, host side (no GPU): the four entry points' place in the C ABI and their argument checks, what
``ops.k_hop_subgraph`` / ``ops.induced_subgraph`` / ``explain_edges(num_hops=...)`` refuse before anything is launched, and
``kagnn_amd.receptive_hops``."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

import kagnn_amd
from kagnn_amd import _lib, ops
from kagnn_amd import baselines as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"kagnn_subgraph_workspace_bytes": 3, "kagnn_k_hop_mark": 9, "kagnn_subgraph_count": 13, "kagnn_subgraph_fill": 22}


def _cpu_graph(n, e):
    """a GraphIndex around host arrays: nothing is launched by ``from_arrays``, which is all the refusals below need"""
    i32 = dict(dtype=torch.int32)
    rp, col, perm = torch.zeros(n + 1, **i32), torch.zeros(e, **i32), torch.arange(e, **i32)
    rp[1:] = e
    return ops.GraphIndex.from_arrays(rp, col, perm, rp, col, perm, n, e)


class _NoLaunch:
    """every library call made while the block is open is an error: a refusal has to come first"""

    def __enter__(self):
        self.real = ops._call

        def refuse(name, *args):
            raise AssertionError(f"{name} was called before the refusal")
        ops._call = refuse
        return self

    def __exit__(self, *exc):
        ops._call = self.real
        return False


def test_the_four_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    assert lib.kagnn_version() >= 276
    header = open(os.path.join(ROOT, "include", "kagnn_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, nargs in NAMES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name) and name in _lib.EXPORTED and len(_lib._SIGNATURES[name][1]) == nargs, name
    assert callable(ops.k_hop_subgraph) and callable(ops.induced_subgraph) and callable(kagnn_amd.receptive_hops)
    assert ops.Subgraph._fields == ("nodes", "edge_index", "edge_ids", "mapping", "hops", "index", "num_nodes", "num_edges")


def test_the_size_query_is_monotone_and_refuses_bad_arguments():
    lib = _lib.load()
    out = ctypes.c_size_t(0)

    def size(n, e):
        assert lib.kagnn_subgraph_workspace_bytes(n, e, ctypes.byref(out)) == 0, lib.kagnn_last_error()
        return out.value
    shapes = [(0, 0), (1, 0), (5, 0), (300, 900), (300, 2513), (70_001, 400_000), (1_000_000, 10_000_000), (1_000_000, 2_000_000_000)]
    sizes = [size(n, e) for n, e in shapes]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[3] < sizes[4] < sizes[5] < sizes[6] < sizes[7]
    assert size(300, 900) <= size(301, 900) and size(300, 900) <= size(300, 901) and size(1 << 20, 0) > size(1 << 10, 0)
    # what the two calls keep there: relabel, the node scan, two row-pointer pairs (int32, N + 1 each) and edge_rank + keep (5 E bytes)
    assert sizes[6] >= 6 * 4 * 1_000_001 + 5 * 10_000_000
    for n, e in [(-1, 0), (0, -1), (1 << 31, 0), (0, 1 << 31)]:
        assert lib.kagnn_subgraph_workspace_bytes(n, e, ctypes.byref(out)) != 0
        assert b"kagnn_subgraph_workspace_bytes" in lib.kagnn_last_error()
    assert lib.kagnn_subgraph_workspace_bytes(3, 3, None) != 0


def test_argument_checks_need_no_gpu():
    lib = _lib.load()
    mark, count, fill = lib.kagnn_k_hop_mark, lib.kagnn_subgraph_count, lib.kagnn_subgraph_fill
    assert mark(None, None, -1, None, 0, 1, None, None, None) != 0
    assert mark(None, None, 10, None, -1, 1, None, None, None) != 0
    assert mark(None, None, 10, None, 0, -1, None, None, None) != 0 and b"num_hops" in lib.kagnn_last_error()
    assert mark(None, None, 10, None, 0, 1, None, None, None) != 0 and b"null array" in lib.kagnn_last_error()
    assert count(None, None, None, None, None, None, None, -1, 0, None, 0, None, None) != 0
    assert count(None, None, None, None, None, None, None, 0, 5, None, 0, None, None) != 0 and b"edges without nodes" in lib.kagnn_last_error()
    assert count(None, None, None, None, None, None, None, 10, 5, None, 0, None, None) != 0 and b"null array" in lib.kagnn_last_error()
    nulls = [None] * 9
    assert fill(None, 0, None, None, None, None, None, None, -1, 0, 0, 0, *nulls, None) != 0
    assert fill(None, 0, None, None, None, None, None, None, 10, 5, 11, 0, *nulls, None) != 0 and b"n_sub" in lib.kagnn_last_error()
    assert fill(None, 0, None, None, None, None, None, None, 10, 5, 3, 6, *nulls, None) != 0 and b"n_sub" in lib.kagnn_last_error()
    assert fill(None, 0, None, None, None, None, None, None, 10, 5, 0, 2, *nulls, None) != 0
    assert fill(None, 0, None, None, None, None, None, None, 10, 5, 3, 2, *nulls, None) != 0 and b"null array" in lib.kagnn_last_error()


def test_refusals_come_before_any_launch():
    g = _cpu_graph(5, 7)
    with _NoLaunch():
        for bad in (-1, -3, 1.5, True):
            with pytest.raises(ValueError, match="num_hops"):
                ops.k_hop_subgraph(torch.tensor([1]), bad, g)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.k_hop_subgraph(torch.tensor([1, 2]), 2, g)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.k_hop_subgraph([1, 2], 2, g)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.k_hop_subgraph(1, 0, g)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.induced_subgraph(torch.tensor([0, 0, 3]), g)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.induced_subgraph(torch.ones(5, dtype=torch.bool), g)
        for mask in (torch.ones(4, dtype=torch.bool), torch.ones(6, dtype=torch.bool), torch.ones(5, 1, dtype=torch.bool)):
            with pytest.raises(ValueError, match=r"shape \[5\]"):
                ops.induced_subgraph(mask, g)
        with pytest.raises(ValueError, match="mask"):
            ops.k_hop_subgraph(torch.ones(5, dtype=torch.bool), 1, g)
        for ids in (torch.tensor([1.0]), torch.tensor([1], dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int64)):
            with pytest.raises(ValueError, match="int64"):
                ops.k_hop_subgraph(ids, 1, g)
        with pytest.raises(TypeError, match="GraphIndex"):
            ops.k_hop_subgraph([1], 1, torch.zeros(2, 3, dtype=torch.int64))


def test_a_graph_on_another_device_is_refused_before_any_launch():
    """the parent's arrays and the ids must share a device: ``_need_cuda`` over both, as for every other op"""
    class _Elsewhere:
        is_cuda, device = True, torch.device("cuda", 1)
    g = _cpu_graph(5, 7)
    g.rowptr = _Elsewhere()
    ids = torch.tensor([1])
    with _NoLaunch():
        with pytest.raises(RuntimeError, match="no CPU fallback|one device"):
            ops.k_hop_subgraph(ids, 1, g)


def test_receptive_hops_counts_convolutions_and_adds_one_for_gcn():
    hops = kagnn_amd.receptive_hops
    for make in (lambda k, l: kagnn_amd.GKAN_Nodes(k, l, 4, 8, 3), lambda k, l: kagnn_amd.GFASTKAN_Nodes(k, l, 4, 8, 3),
                 lambda k, l: B.GNN_Nodes(k, l, 4, 8, 3)):
        for layers in (1, 2, 3):
            assert hops(make("gin", layers)) == layers and hops(make("gat", layers)) == layers
            assert hops(make("gcn", layers)) == layers + 1
    assert hops(kagnn_amd.GIKANLayer(4, 4)) == 1 and hops(kagnn_amd.KAGCNConv(4, 4)) == 2 and hops(kagnn_amd.KAGATConv(4, 4, 2)) == 1
    assert hops(B.GCNConv(4, 4)) == 2 and hops(B.GINConv(B.make_mlp_nodes(4, 4, 4, 2))) == 1 and hops(B.GATConv(4, 4, 2)) == 1
    assert hops(kagnn_amd.GINEKANLayer(kagnn_amd.KAN([4, 4]))) == 1
    # graph-level models: gnn_layers convolutions (3 here), one hop more for the GCN-normalised stacks
    from kagnn_amd import graph_models as G
    assert hops(G.KAGIN(3, 4, 8, 3, 2, 4, 3, 0.0)) == 3 and hops(G.FASTKAGIN(3, 4, 8, 3, 2, 4, 0.0)) == 3
    assert hops(G.KAGCN(3, 4, 8, 3, 4, 3, 0.0)) == 4 and hops(G.FASTKAGCN(3, 4, 8, 3, 4, 0.0)) == 4
    assert hops(G.KAGAT(3, 4, 8, 3, 4, 3, 0.0, 2)) == 3 and hops(G.KAGINRegression(4, 4, 3, 8, 2, 4, 3, 1, 0.0)) == 3
    for empty in (nn.Linear(3, 3), kagnn_amd.KAN([4, 4]), nn.Sequential()):
        with pytest.raises(ValueError, match="no message-passing convolution"):
            hops(empty)


def test_explain_edges_with_num_hops_needs_a_node_and_a_sane_number():
    model = kagnn_amd.GKAN_Nodes("gin", 2, 4, 8, 3)
    x, ei = torch.randn(6, 4), torch.randint(0, 6, (2, 9))
    with _NoLaunch():
        with pytest.raises(ValueError, match="node_idx"):
            kagnn_amd.explain_edges(model, x, ei, num_hops=2)
        with pytest.raises(ValueError, match="node_idx"):
            kagnn_amd.explain_edges(model, x, ei, num_hops="auto")
        for bad in (-1, 1.5, "two", True):
            with pytest.raises(ValueError, match="num_hops"):
                kagnn_amd.explain_edges(model, x, ei, node_idx=1, num_hops=bad)
    # on the CPU the extraction is refused like every other op, with nothing of the model touched
    model.train()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kagnn_amd.explain_edges(model, x, ei, node_idx=1, num_hops="auto", epochs=2)
    assert model.training and all(p.grad is None for p in model.parameters()) and ops.edge_mask_of() is None
