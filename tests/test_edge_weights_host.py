"""Differentiable edge weights, host side (no GPU): the new entry point's place in the C ABI and its argument checks, and what
``ops.aggregate_edge_grad``, ``kagnn_amd.edge_mask`` and ``kagnn_amd.explain_edges`` refuse or restore before anything is launched."""
import os
import re
import threading

import pytest
import torch

import kagnn_amd
from kagnn_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cpu_graph(n, e):
    """a GraphIndex around host arrays: nothing is launched by ``from_arrays``, which is all the refusals below need"""
    i32 = dict(dtype=torch.int32)
    rp, col, perm = torch.zeros(n + 1, **i32), torch.zeros(e, **i32), torch.arange(e, **i32)
    rp[1:] = e
    return ops.GraphIndex.from_arrays(rp, col, perm, rp, col, perm, n, e)


def _clean():
    return ops.edge_mask_of() is None and not ops.aggregation_visible() and not ops.layer_inputs_visible()


def test_symbol_is_declared_exported_and_bound():
    lib = _lib.load()
    assert lib.kagnn_version() >= 274
    header = open(os.path.join(ROOT, "include", "kagnn_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+kagnn_aggregate_edge_grad\s*\(", header)
    assert hasattr(lib, "kagnn_aggregate_edge_grad")
    assert "kagnn_aggregate_edge_grad" in _lib.EXPORTED and len(_lib._SIGNATURES["kagnn_aggregate_edge_grad"][1]) == 18
    assert callable(ops.aggregate_edge_grad) and callable(kagnn_amd.edge_mask) and callable(kagnn_amd.explain_edges)


def test_argument_checks_need_no_gpu():
    lib = _lib.load()
    call = lib.kagnn_aggregate_edge_grad
    # ldx < F, ldg < F, F < 1, negative sizes: refused with a message
    assert call(None, 4, None, 8, None, None, None, 10, 5, 8, None, None, 0, None, 0, 96, None, None) != 0
    assert b"leading dimension" in lib.kagnn_last_error()
    assert call(None, 8, None, 7, None, None, None, 10, 5, 8, None, None, 0, None, 0, 96, None, None) != 0
    assert call(None, 8, None, 8, None, None, None, 10, 5, 0, None, None, 0, None, 0, 96, None, None) != 0
    assert call(None, 8, None, 8, None, None, None, -1, 5, 8, None, None, 0, None, 0, 96, None, None) != 0
    # null arrays with work to do
    assert call(None, 8, None, 8, None, None, None, 10, 5, 8, None, None, 0, None, 0, 96, None, None) != 0
    assert b"null array" in lib.kagnn_last_error()
    # no nodes or no edges: nothing to launch, whatever the pointers
    assert call(None, 8, None, 8, None, None, None, 0, 5, 8, None, None, 0, None, 0, 96, None, None) == 0
    assert call(None, 8, None, 8, None, None, None, 10, 0, 8, None, None, 0, None, 0, 96, None, None) == 0


def test_cpu_tensors_are_refused():
    x, gout = torch.randn(5, 4), torch.randn(5, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.aggregate_edge_grad(x, gout, _cpu_graph(5, 7))
    w = torch.rand(7, requires_grad=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.aggregate_sum(x, _cpu_graph(5, 7), edge_weight=w)


def test_a_mask_of_the_wrong_length_raises():
    g = _cpu_graph(5, 7)
    x = torch.randn(5, 4)
    convs = [kagnn_amd.GIKANLayer(4, 4), kagnn_amd.GIFASTKANLayer(4, 4), kagnn_amd.KAGCNConv(4, 4), kagnn_amd.FASTKAGCNConv(4, 4),
             kagnn_amd.GCNConv(4, 4), kagnn_amd.GINConv(kagnn_amd.make_mlp_nodes(4, 4, 4, 2))]
    for conv in convs:
        with kagnn_amd.edge_mask(torch.ones(6)):
            with pytest.raises(ValueError, match="6 entries.*7 edges"):
                conv(x, g)
        assert _clean()
    for bad in (torch.ones(7, 1), torch.ones(7, dtype=torch.float64), [1.0] * 7):
        with pytest.raises(ValueError, match="float32"):
            with kagnn_amd.edge_mask(bad):
                pass
    assert _clean()


def test_attention_gine_sparse_and_explicit_weights_raise_inside_a_block():
    g = _cpu_graph(5, 7)
    x = torch.randn(5, 4)
    mask = torch.ones(7)
    gat, gine = kagnn_amd.KAGATConv(4, 4, 2), kagnn_amd.GINEKANLayer(kagnn_amd.KAN([4, 4]))
    gcn = kagnn_amd.KAGCNConv(4, 4)
    adj = torch.sparse_coo_tensor(torch.tensor([[0, 1], [1, 0]]), torch.ones(2), (5, 5))
    with kagnn_amd.edge_mask(mask):
        for conv in (gat, kagnn_amd.FASTKAGATConv(4, 4, 2), kagnn_amd.GATConv(4, 4, 2)):
            with pytest.raises(NotImplementedError, match="edge_mask"):
                conv(x, g)
        for conv in (gine, kagnn_amd.GINEConv(kagnn_amd.make_mlp(4, 4, 4, 2))):
            with pytest.raises(NotImplementedError, match="edge_mask"):
                conv(x, g, torch.randn(7, 4))
        with pytest.raises(NotImplementedError, match="edge_mask"):
            gine.forward_fused_norm(x, g, torch.randn(7, 4), kagnn_amd.BatchNorm1d(4))
        with pytest.raises(NotImplementedError, match="edge_mask"):
            gcn(x, adj)
        with pytest.raises(NotImplementedError, match="edge_mask"):
            gcn(x, g, torch.ones(7))
    assert _clean()
    # outside a block they are what they were: the CPU refusal, not the block's
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gat(x, torch.zeros(2, 3, dtype=torch.long))


def test_state_is_cleared_after_an_exception_inside_the_block():
    mask = torch.ones(3)
    with pytest.raises(KeyError):
        with kagnn_amd.edge_mask(mask):
            assert ops.edge_mask_of() is mask and ops.aggregation_visible()
            raise KeyError("inside")
    assert _clean()
    # nested blocks: the inner mask until it closes, then the outer one again -- also when the inner one is left by an exception
    inner = torch.zeros(3)
    with kagnn_amd.edge_mask(mask):
        with pytest.raises(KeyError):
            with kagnn_amd.edge_mask(inner):
                assert ops.edge_mask_of() is inner
                raise KeyError("inner")
        assert ops.edge_mask_of() is mask
    assert _clean()


def test_state_and_flags_are_restored_after_an_exception_inside_explain_edges():
    model = kagnn_amd.GKAN_Nodes("gin", 2, 4, 8, 3, dropout=0.5).train()
    model.bns[0].eval()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    x, ei = torch.randn(6, 4), torch.randint(0, 6, (2, 9))
    # the model's own prediction is asked for first: refused on the CPU before any block is open
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kagnn_amd.explain_edges(model, x, ei, epochs=2)
    assert _clean()
    # with a target given, the first forward is the masked one: refused INSIDE the block
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kagnn_amd.explain_edges(model, x, ei, target=torch.zeros(6, dtype=torch.long), epochs=2, generator=torch.Generator().manual_seed(0))
    assert _clean()
    assert model.training and model.convs[0].training and model.dropout.training and not model.bns[0].training and model.bns[1].training
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())
    assert all(p.grad is None for p in model.parameters())


def test_a_block_on_another_thread_does_not_affect_this_one():
    opened, release = threading.Event(), threading.Event()
    seen = {}

    def other():
        with kagnn_amd.edge_mask(torch.ones(4)):
            seen["inside"] = ops.aggregation_visible() and ops.edge_mask_of().numel() == 4
            opened.set()
            release.wait(30)
        seen["after"] = _clean()

    t = threading.Thread(target=other)
    t.start()
    try:
        assert opened.wait(30)
        assert _clean()                       # the other thread's block is open right now
        mine = torch.zeros(2)
        with kagnn_amd.edge_mask(mine):
            assert ops.edge_mask_of() is mine
        assert _clean()
    finally:
        release.set()
        t.join(30)
    assert seen == {"inside": True, "after": True}
