"""Host side of attribution and pruning (``kagnn_kan_edge_moments``, ``KAN.keep_nodes`` / ``prune_*``, ``kagnn_amd.apply_pruning``): ABI
surface, argument checks, what the Python surface refuses, the structural surgery of ``keep_nodes`` against the fp64 oracle, the
offset case a one-pass second moment cannot pass, and the register gate of the new kernels -- all without a GPU."""
import ctypes
import importlib.util
import os
import re
import shutil

import numpy as np
import pytest
import torch

import kagnn_amd
from kagnn_amd import _lib, ekan, ops
from helpers import assert_close, must_fail
import pruning_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAGNN_ERR_ARG, KAGNN_ERR_UNSUPPORTED = -1, -3


def _lib_or_build():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


# ---------------------------------------------------------------------------------- the C ABI
def test_version_symbols_and_signature():
    lib = _lib_or_build()
    assert lib.kagnn_version() >= 281
    header = open(os.path.join(ROOT, "include", "kagnn_hip.h")).read()
    for name in ("kagnn_kan_edge_moments_workspace_bytes", "kagnn_kan_edge_moments"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED and hasattr(lib, name), name
    P, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    res, args = _lib._SIGNATURES["kagnn_kan_edge_moments"]
    # x ldx N knots per_feature in out G K bw sw sc mean ld_mean m2 ld_m2 ws bytes stream
    assert res is i32 and args == [P, i64, i64, P, i32, i32, i32, i32, i32, P, P, P, P, i64, P, i64, P, ctypes.c_size_t, P]
    res, args = _lib._SIGNATURES["kagnn_kan_edge_moments_workspace_bytes"]
    assert res is i32 and args == [i64, i32, i32, i32, i32, ctypes.POINTER(ctypes.c_size_t)]


def test_workspace_query():
    lib = _lib_or_build()
    n, m = ctypes.c_size_t(0), ctypes.c_size_t(0)
    fn = lib.kagnn_kan_edge_moments_workspace_bytes
    sizes = {}
    for rows in (0, 1, 1000, 1 << 20, 1 << 24):
        assert fn(rows, 64, 64, 5, 3, ctypes.byref(n)) == 0
        assert lib.kagnn_kan_edge_abs_sum_workspace_bytes(rows, 64, 64, 5, 3, ctypes.byref(m)) == 0
        sizes[rows] = n.value
        assert n.value == 2 * m.value + 64 * 64 * 4            # two partials per slab of the abs sum's plan, and the pivots
    assert sizes[1 << 24] == sizes[1 << 20]                    # slab partials only: nothing proportional to N * out
    assert fn(10, 4, 4, 5, 3, None) == KAGNN_ERR_ARG
    assert fn(-1, 4, 4, 5, 3, ctypes.byref(n)) == KAGNN_ERR_ARG
    assert fn(10, 0, 4, 5, 3, ctypes.byref(n)) == KAGNN_ERR_ARG
    for order in range(5, 17):
        assert fn(10, 4, 4, 5, order, ctypes.byref(n)) == KAGNN_ERR_UNSUPPORTED
        assert b"spline_order must be 1..4" in lib.kagnn_last_error()


def test_argument_checks_need_no_device():
    lib = _lib_or_build()
    one = ctypes.c_void_p(16)       # never dereferenced: every call below fails its checks first
    mom = lib.kagnn_kan_edge_moments
    big = 1 << 20
    for order in range(5, 17):
        assert mom(one, 4, 8, one, 0, 4, 4, 5, order, one, one, one, one, 4, one, 4, one, big, None) == KAGNN_ERR_UNSUPPORTED
    assert mom(one, 4, 8, one, 0, 4, 4, 5, 3, one, one, one, None, 4, None, 4, one, big, None) == KAGNN_ERR_ARG       # both outputs NULL
    assert b"both null" in lib.kagnn_last_error()
    assert mom(one, 3, 8, one, 0, 4, 4, 5, 3, one, one, one, one, 4, one, 4, one, big, None) == KAGNN_ERR_ARG         # ldx < in
    assert mom(one, 4, 8, one, 0, 4, 4, 5, 3, one, one, one, one, 3, one, 4, one, big, None) == KAGNN_ERR_ARG         # ld_mean < in
    assert mom(one, 4, 8, one, 0, 4, 4, 5, 3, one, one, one, one, 4, one, 3, one, big, None) == KAGNN_ERR_ARG         # ld_m2 < in
    assert mom(one, 4, 8, one, 2, 4, 4, 5, 3, one, one, one, one, 4, one, 4, one, big, None) == KAGNN_ERR_ARG         # knot flag
    assert mom(one, 4, 8, one, 0, 4, 4, 5, 3, one, None, one, one, 4, one, 4, one, big, None) == KAGNN_ERR_ARG        # no spline_weight
    assert mom(one, 4, 8, one, 0, 4, 4, 5, 3, one, one, one, one, 4, one, 4, None, 0, None) == KAGNN_ERR_ARG          # no workspace
    assert mom(one, 4, 8, one, 0, 4, 4, 5, 3, one, one, one, one, 4, one, 4, one, 16, None) == KAGNN_ERR_ARG          # short workspace
    assert b"workspace too small" in lib.kagnn_last_error()
    assert mom(one, 4, -1, one, 0, 4, 4, 5, 3, one, one, one, one, 4, one, 4, one, big, None) == KAGNN_ERR_ARG        # negative rows


def test_moments_kernels_do_not_spill():
    objdir = os.path.join(ROOT, "kagnn_amd", "lib", "obj")
    if not os.path.isdir(objdir) or not shutil.which("c++filt") or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no build objects / LLVM tools on this machine (the library was shipped prebuilt)")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = [k for k in kr.collect(objdir) if "kan_phi_moments" in k["name"]]
    assert len(rows) == 8 + 1, len(rows)       # 4 orders x {shared, per-feature knots}, and the fp64 slab reduction
    bad = [k for k in rows if k["vgpr_spill_count"] or k["private_segment_fixed_size"]]
    assert not bad, [(k["name"], k["vgpr_spill_count"], k["private_segment_fixed_size"]) for k in bad]
    gated = [r for r in kr.hot_path_report(rows) if "kan_phi_moments_kernel<" in r[0]]
    assert len(gated) == 8 and all(r[3] == 0 and r[4] == 0 for r in gated)      # on the tool's own no-spill list


# ---------------------------------------------------------------------------------- what the Python surface refuses
@pytest.mark.parametrize("order", [5, 9, 16])
def test_python_surface_refuses_high_orders(order):
    layer = kagnn_amd.KANLinear(3, 2, grid_size=5, spline_order=order)
    chain = kagnn_amd.KAN([3, 4, 2], grid_size=5, spline_order=order)
    x = torch.zeros(4, 3)
    with pytest.raises(NotImplementedError, match="spline_order"):
        layer.edge_stats(x)
    for call in (chain.attribute, chain.prune_nodes, chain.prune_edges, chain.prune):
        with pytest.raises(NotImplementedError, match="spline_order"):
            call(x)


def test_python_surface_refuses_cpu_tensors():
    layer = kagnn_amd.KANLinear(3, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer.edge_stats(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kagnn_amd.KAN([3, 4, 2]).attribute(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.kan_edge_moments(torch.zeros(4, 3), None, torch.zeros(2, 3, 8), None, torch.linspace(-2.2, 2.2, 12), 5, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kagnn_amd.attribute(kagnn_amd.KAN([3, 4, 2]), torch.zeros(4, 3))
    assert not ops.layer_inputs_visible() and ops._edge_collectors() == []      # the block is closed again


# ---------------------------------------------------------------------------------- check 2: the offset case
def test_one_pass_second_moment_fails_the_offset_case():
    """phi ~ 5 +- 0.01: ``sum phi^2 - (sum phi)^2 / N`` in fp32 loses ~6e-8 x mean^2 / var of the variance.  The two-pass fp32 evaluation of
    the same quantity passes the bound the device result is held to; the one-pass form must not."""
    x, bw, sw, knots = pr.offset_case()
    mean, want, naive, e32 = pr.offset_reference(x, bw, sw, knots)
    assert 4.9 < float(mean.min()) and float(want.max()) < 0.02
    rel = float((naive.double() - want).abs().max() / want.max())
    print(f"offset case: one-pass fp32 error {rel:.3e} of the maximum, two-pass fp32 error {e32 / float(want.max()):.3e}")
    assert rel > 1e-2
    must_fail(naive, want, what="one-pass fp32 sqrt(m2/N) on the offset case")
    assert e32 <= 2e-5 * float(want.max())


# ---------------------------------------------------------------------------------- keep_nodes (pure host surgery)
def test_keep_nodes_shapes_fixed_edges_and_function():
    chain, x = pr.per_feature_chain()
    keep = [torch.tensor([0, 2, 3, 4])]                        # units 1 and 5 go
    before = [p for p in chain.parameters()]
    want = pr.chain_forward64(list(chain.layers), x, zero_out={1: [1, 5]})
    grid_rows = chain.layers[1].grid[keep[0]].clone()
    chain.keep_nodes(keep)
    l0, l1 = chain.layers
    assert (l0.in_features, l0.out_features, l1.in_features, l1.out_features) == (4, 4, 4, 3)
    assert l0.base_weight.shape == (4, 4) and l0.spline_weight.shape == (4, 4, 8) and l0.spline_scaler.shape == (4, 4)
    assert l1.base_weight.shape == (3, 4) and l1.spline_weight.shape == (3, 4, 8) and l1.grid.shape == (4, 12)
    assert torch.equal(l1.grid, grid_rows) and l1._knots().dim() == 2
    assert all(isinstance(p, torch.nn.Parameter) and p.requires_grad for p in chain.parameters())
    assert not {id(p) for p in chain.parameters()} & {id(p) for p in before}          # NEW Parameters: rebuild the optimizer
    names = [n for n, _ in chain.named_parameters()]
    assert names == ["layers.0.base_weight", "layers.0.spline_weight", "layers.0.spline_scaler", "layers.0.symbolic_affine",
                     "layers.1.base_weight", "layers.1.spline_weight", "layers.1.spline_scaler", "layers.1.symbolic_affine"]
    # layer 0: the "0" edge of removed row 1 is gone, that of row 3 is now row 2; layer 1: column 4 -> 3 kept, column 1 removed
    assert l0.fixed_edges() == {(2, 0): "0"}
    assert l1.fixed_edges() == {(2, 3): "sin"}
    assert torch.equal(l1.symbolic_affine.detach(), torch.tensor([[1.3, 0.2, 0.7, -0.1]]))
    got = pr.chain_forward64(list(chain.layers), x)
    assert_close(got, want, 1e-12, what="keep_nodes: the pruned chain in fp64 vs the unpruned one with zeroed edges")


def test_keep_nodes_without_the_grid_rows_must_fail():
    """mutation guard: slicing the next layer's columns but not its grid rows changes the function on per-feature knots"""
    chain, x = pr.per_feature_chain()
    keep = torch.tensor([0, 2, 3, 4])
    want = pr.chain_forward64(list(chain.layers), x, zero_out={1: [1, 5]})
    wrong_grid = chain.layers[1].grid[:4].clone()
    chain.keep_nodes([keep])
    chain.layers[1].grid = wrong_grid
    must_fail(pr.chain_forward64(list(chain.layers), x), want, what="columns sliced, grid rows not")


def test_keep_nodes_argument_checks_and_identity():
    chain, _ = pr.random_chain((4, 6, 5, 3), 1)
    with pytest.raises(ValueError, match="one index list per interior width"):
        chain.keep_nodes([[0, 1]])
    with pytest.raises(ValueError, match="nothing is kept"):
        chain.keep_nodes([[0, 1], []])
    for bad in ([1, 0], [0, 0], [0, 6], [-1, 2]):
        with pytest.raises(ValueError, match="sorted"):
            chain.keep_nodes([bad, [0]])
    assert [l.out_features for l in chain.layers] == [6, 5, 3]                          # nothing happened
    before = [id(p) for p in chain.parameters()]
    chain.keep_nodes([list(range(6)), torch.arange(5)])
    assert [id(p) for p in chain.parameters()] == before                                # everything kept: nothing is rebuilt
    chain.keep_nodes([[1, 4], [0, 2, 3]])
    assert [(l.in_features, l.out_features) for l in chain.layers] == [(4, 2), (2, 3), (3, 3)]
    one = kagnn_amd.KAN([3, 2])
    one.keep_nodes([])
    assert one.layers[0].base_weight.shape == (2, 3)


def test_keep_lists_and_edge_switching_from_an_attribution():
    """the decisions, on a hand-made attribution: a width where nothing passes keeps its best unit; fixed edges are left alone"""
    chain, _ = pr.random_chain((3, 4, 4, 2), 2)
    chain.layers[0].fix_symbolic(1, 1, "sin", params=(1.0, 0.0, 1.0, 0.0))
    chain.layers[0].fix_symbolic(0, 0, "0")
    es = [torch.full((4, 3), 0.5), torch.full((4, 4), 0.5), torch.full((2, 4), 0.5)]
    es[0][1, 1] = es[0][0, 0] = es[0][2, 2] = 1e-3
    es[2][1, 3] = 1e-3
    ns = [torch.ones(3), torch.tensor([0.5, 1e-3, 0.02, float("nan")]), torch.tensor([1e-3, 5e-3, 2e-3, 1e-4]), torch.ones(2)]
    att = ekan.Attribution(edge_std=es, out_std=[None] * 3, edge_scores=es, node_scores=ns)
    keep = ekan._keep_lists(att, 1e-2)
    assert [k.tolist() for k in keep] == [[0, 2], [1]] and all(k.dtype == torch.int64 for k in keep)
    pruned = ekan._switch_off_edges(list(chain.layers), att, 3e-2)
    assert [p.tolist() for p in pruned] == [[[2, 2]], [], [[1, 3]]]
    assert chain.layers[0].fixed_edges() == {(0, 0): "0", (1, 1): "sin", (2, 2): "0"}
    assert chain.layers[1]._symbolic is None and chain.layers[2].fixed_edges() == {(1, 3): "0"}


def test_apply_pruning_lets_a_pruned_checkpoint_load():
    torch.manual_seed(5)
    model = torch.nn.ModuleDict({"a": kagnn_amd.KAN([3, 6, 5, 2]), "b": kagnn_amd.KANLinear(4, 3)})
    report = kagnn_amd.PruneReport()
    model["a"].keep_nodes([[0, 3, 4], [1, 2]])
    model["a"].layers[1]._switch_off([(1, 0)])
    model["b"]._switch_off([(2, 1), (0, 3)])
    report.chains["a"] = {"keep": [torch.tensor([0, 3, 4]), torch.tensor([1, 2])], "edges": [torch.zeros((0, 2), dtype=torch.int64), torch.tensor([[1, 0]]), torch.zeros((0, 2), dtype=torch.int64)],
                          "widths_before": [3, 6, 5, 2], "widths_after": [3, 3, 2, 2]}
    report.chains["b"] = {"keep": [], "edges": [torch.tensor([[0, 3], [2, 1]])], "widths_before": [4, 3], "widths_after": [4, 3]}
    fresh = torch.nn.ModuleDict({"a": kagnn_amd.KAN([3, 6, 5, 2]), "b": kagnn_amd.KANLinear(4, 3)})
    with pytest.raises(RuntimeError, match="size mismatch"):
        fresh.load_state_dict(model.state_dict())
    fresh = torch.nn.ModuleDict({"a": kagnn_amd.KAN([3, 6, 5, 2]), "b": kagnn_amd.KANLinear(4, 3)})
    kagnn_amd.apply_pruning(fresh, report)
    fresh.load_state_dict(model.state_dict())
    for (n, p), (m, q) in zip(model.state_dict().items(), fresh.state_dict().items()):
        assert n == m and torch.equal(p, q), n
    assert fresh["a"].layers[1].fixed_edges() == {(1, 0): "0"} and fresh["b"].fixed_edges() == {(0, 3): "0", (2, 1): "0"}
    with pytest.raises(KeyError, match="no chain"):
        kagnn_amd.apply_pruning(kagnn_amd.KAN([3, 2]), report)


def test_attribution_rule_restatement_needs_its_normalisation():
    """mutation guard on the restatement itself: the rule without ``/ (s_l + 1e-4)`` is a different rule"""
    chain, x = pr.planted_chain(0)
    ref = pr.attribute64(list(chain.layers), x)
    wrong = pr.attribute64(list(chain.layers), x, normalise=False)
    must_fail(torch.from_numpy(wrong["node_scores"][0]), ref["node_scores"][0], what="input scores without the normalisation")
    assert pr.outside_band(ref["node_scores"][1], 1e-2)
    assert sorted(np.nonzero(ref["node_scores"][1] < 1e-2)[0].tolist()) == [2, 5]
