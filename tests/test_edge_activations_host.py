"""Host side of the per-edge activation entry points (csrc/kan_edge.hip): ABI surface, workspace queries, argument checks,
what the Python surface refuses, the spill gate, and the routing predicate of ``collect_edge_l1`` -- all without a GPU."""
import ctypes
import importlib.util
import os
import re
import shutil

import pytest
import torch

import kagnn_amd
from kagnn_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("kagnn_kan_edge_abs_sum_workspace_bytes", "kagnn_kan_edge_abs_sum", "kagnn_kan_edge_abs_sum_bwd_workspace_bytes",
           "kagnn_kan_edge_abs_sum_bwd", "kagnn_kan_edge_curves")
KAGNN_ERR_ARG, KAGNN_ERR_UNSUPPORTED = -1, -3


def _lib_or_build():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_version_and_symbols():
    lib = _lib_or_build()
    assert lib.kagnn_version() >= 269
    header = open(os.path.join(ROOT, "include", "kagnn_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED and hasattr(lib, name), name
    codes = dict(re.findall(r"#define\s+(KAGNN_ERR_[A-Z]+)\s+\(?(-?\d+)\)?", header))
    assert int(codes["KAGNN_ERR_ARG"]) == KAGNN_ERR_ARG and int(codes["KAGNN_ERR_UNSUPPORTED"]) == KAGNN_ERR_UNSUPPORTED


def test_workspace_queries():
    lib = _lib_or_build()
    n = ctypes.c_size_t(0)
    sizes = {}
    for rows in (0, 1, 1000, 1 << 20, 1 << 24):
        assert lib.kagnn_kan_edge_abs_sum_workspace_bytes(rows, 64, 64, 5, 3, ctypes.byref(n)) == 0
        sizes[rows] = n.value
        assert n.value >= 64 * 64 * 4 and n.value % (64 * 64 * 4) == 0          # whole [out, in] slab partials
        assert lib.kagnn_kan_edge_abs_sum_bwd_workspace_bytes(rows, 64, 64, 5, 3, ctypes.byref(n)) == 0
        assert n.value == sizes[rows] * 9                                        # [in, C + 1, out] per slab, C = 8
    # slab partials only: bounded in the row count (nothing proportional to N * out)
    assert sizes[1 << 24] == sizes[1 << 20] and sizes[1 << 20] <= 2048 * 64 * 64 * 4
    for fn in (lib.kagnn_kan_edge_abs_sum_workspace_bytes, lib.kagnn_kan_edge_abs_sum_bwd_workspace_bytes):
        assert fn(10, 4, 4, 5, 3, None) == KAGNN_ERR_ARG
        assert fn(-1, 4, 4, 5, 3, ctypes.byref(n)) == KAGNN_ERR_ARG
        assert fn(10, 0, 4, 5, 3, ctypes.byref(n)) == KAGNN_ERR_ARG
        assert fn(10, 4, 4, 40, 4, ctypes.byref(n)) == KAGNN_ERR_UNSUPPORTED     # 40 + 4 coefficients: beyond what the layer takes
        for order in range(5, 17):
            assert fn(10, 4, 4, 5, order, ctypes.byref(n)) == KAGNN_ERR_UNSUPPORTED
            assert b"spline_order must be 1..4" in lib.kagnn_last_error()


def test_argument_checks_need_no_device():
    lib = _lib_or_build()
    one = ctypes.c_void_p(16)       # never dereferenced: every call below fails its checks first
    for order in range(5, 17):
        assert lib.kagnn_kan_edge_abs_sum(one, 4, 8, one, 0, 4, 4, 5, order, one, one, one, one, 4, one, 1 << 20, None) == KAGNN_ERR_UNSUPPORTED
        assert lib.kagnn_kan_edge_abs_sum_bwd(one, 4, 8, one, 0, 4, 4, 5, order, one, one, one, one, 4, one, one, one, one, 4, one, 1 << 20,
                                             None) == KAGNN_ERR_UNSUPPORTED
        assert lib.kagnn_kan_edge_curves(one, 0, 8, one, 0, 4, 4, 5, order, one, one, one, one, None) == KAGNN_ERR_UNSUPPORTED
    assert lib.kagnn_kan_edge_abs_sum(one, 3, 8, one, 0, 4, 4, 5, 3, one, one, one, one, 4, one, 1 << 20, None) == KAGNN_ERR_ARG       # ldx < in
    assert lib.kagnn_kan_edge_abs_sum(one, 4, 8, one, 0, 4, 4, 5, 3, one, one, one, one, 3, one, 1 << 20, None) == KAGNN_ERR_ARG       # ld of S < in
    assert lib.kagnn_kan_edge_abs_sum(one, 4, 8, one, 2, 4, 4, 5, 3, one, one, one, one, 4, one, 1 << 20, None) == KAGNN_ERR_ARG       # knot flag
    assert lib.kagnn_kan_edge_abs_sum(one, 4, 8, one, 0, 4, 4, 5, 3, one, None, one, one, 4, one, 1 << 20, None) == KAGNN_ERR_ARG      # no spline_weight
    assert lib.kagnn_kan_edge_abs_sum(one, 4, 8, one, 0, 4, 4, 5, 3, one, one, one, None, 4, one, 1 << 20, None) == KAGNN_ERR_ARG      # no output
    assert lib.kagnn_kan_edge_abs_sum(one, 4, 8, one, 0, 4, 4, 5, 3, one, one, one, one, 4, one, 16, None) == KAGNN_ERR_ARG            # workspace too small
    assert b"workspace too small" in lib.kagnn_last_error()
    bwd = lib.kagnn_kan_edge_abs_sum_bwd
    assert bwd(one, 4, 8, one, 0, 4, 4, 5, 3, None, one, one, one, 4, one, one, one, one, 4, one, 1 << 20, None) == KAGNN_ERR_ARG       # g_bw without bw
    assert bwd(one, 4, 8, one, 0, 4, 4, 5, 3, one, one, None, one, 4, one, one, one, one, 4, one, 1 << 20, None) == KAGNN_ERR_ARG       # g_sc without sc
    assert bwd(one, 4, 8, one, 0, 4, 4, 5, 3, one, one, one, None, 4, one, one, one, one, 4, one, 1 << 20, None) == KAGNN_ERR_ARG       # no upstream
    assert bwd(one, 4, 8, one, 0, 4, 4, 5, 3, one, one, one, one, 4, one, one, one, one, 4, None, 0, None) == KAGNN_ERR_ARG             # no workspace
    assert bwd(one, 4, 8, one, 0, 4, 4, 5, 3, one, one, one, one, 4, one, one, one, one, 3, one, 1 << 20, None) == KAGNN_ERR_ARG        # ldgx < in
    assert lib.kagnn_kan_edge_curves(one, 3, 8, one, 0, 4, 4, 5, 3, one, one, one, one, None) == KAGNN_ERR_ARG                          # 0 < ldt < in
    assert lib.kagnn_kan_edge_curves(one, 0, 8, one, 0, 4, 4, 5, 3, one, one, one, None, None) == KAGNN_ERR_ARG                         # no output
    assert lib.kagnn_kan_edge_curves(None, 0, 0, None, 0, 4, 4, 5, 3, None, None, None, None, None) == 0                                # no points: nothing to do


@pytest.mark.parametrize("order", list(range(5, 17)))
def test_python_surface_refuses_high_orders(order):
    layer = kagnn_amd.KANLinear(3, 2, grid_size=5, spline_order=order)
    x = torch.zeros(4, 3)
    with pytest.raises(NotImplementedError, match="spline_order"):
        layer.edge_l1(x)
    with pytest.raises(NotImplementedError, match="spline_order"):
        layer.edge_curves(torch.zeros(4))
    with pytest.raises(NotImplementedError, match="spline_order"):
        layer.regularization_loss(x=x)
    assert torch.isfinite(layer.regularization_loss())          # the weight stand-in needs no kernel


def test_python_surface_refuses_cpu_tensors():
    layer = kagnn_amd.KANLinear(3, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer.edge_l1(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer.edge_curves(torch.zeros(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kagnn_amd.KAN([3, 4, 2]).regularization_loss(x=torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.kan_edge_abs_sum(torch.zeros(4, 3), None, torch.zeros(2, 3, 8), None, torch.linspace(-2.2, 2.2, 12), 5, 3)


def test_regularization_loss_without_rows_is_unchanged():
    torch.manual_seed(0)
    layer = kagnn_amd.KANLinear(6, 5)
    mag = layer.spline_weight.abs().mean(-1)
    total = mag.sum()
    share = mag / total
    assert torch.equal(layer.regularization_loss(0.5, 2.0), 0.5 * total - 2.0 * torch.sum(share * share.log()))


def test_edge_kernels_do_not_spill():
    objdir = os.path.join(ROOT, "kagnn_amd", "lib", "obj")
    if not os.path.isdir(objdir) or not shutil.which("c++filt") or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no build objects / LLVM tools on this machine (the library was shipped prebuilt)")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = [k for k in kr.collect(objdir) if "kan_edge_" in k["name"]]
    names = " ".join(k["demangled"] or k["name"] for k in rows)
    # 4 orders x {shared, per-feature knots} x {abs sum, gx, curves} row kernels, x 4 coefficient widths of the parameter kernel, 2 reductions
    assert len(rows) == 24 + 32 + 2, len(rows)
    for must in ("kan_edge_rows_kernel", "kan_edge_param_kernel", "kan_edge_sum_reduce_kernel", "kan_edge_param_reduce_kernel"):
        assert must in names, must
    bad = [k for k in rows if k["vgpr_spill_count"] or k["private_segment_fixed_size"]]
    assert not bad, [(k["name"], k["vgpr_spill_count"], k["private_segment_fixed_size"]) for k in bad]


def test_collect_edge_l1_restores_the_routing_predicate():
    model = kagnn_amd.KAN([3, 4, 2])
    high = kagnn_amd.KANLinear(3, 2, spline_order=6)
    both = torch.nn.ModuleDict({"kan": model, "high": high})
    assert not ops.layer_inputs_visible()
    with kagnn_amd.collect_edge_l1(both) as stats:
        assert ops.layer_inputs_visible() and stats == {}
        names, _ = ops._edge_collectors()[-1]
        assert sorted(names.values()) == ["kan.layers.0", "kan.layers.1"]       # the order-6 layer is not collected
        with kagnn_amd.collect_edge_l1(model):
            assert len(ops._edge_collectors()) == 2
        assert ops.layer_inputs_visible()
    assert not ops.layer_inputs_visible()
    with pytest.raises(ZeroDivisionError):
        with kagnn_amd.collect_edge_l1(model):
            assert ops.layer_inputs_visible()
            1 / 0
    assert not ops.layer_inputs_visible() and ops._edge_collectors() == []
    # a CPU forward inside the block reaches the collection, which refuses like every op
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        with kagnn_amd.collect_edge_l1(model):
            model(torch.zeros(4, 3))
    assert not ops.layer_inputs_visible()


def test_collect_edge_l1_belongs_to_the_thread_that_opened_it():
    import threading
    model = kagnn_amd.KAN([3, 4, 2])
    seen = {}

    def other():
        seen["visible"] = ops.layer_inputs_visible()
        seen["blocks"] = len(ops._edge_collectors())
        with kagnn_amd.collect_edge_l1(model):
            seen["own"] = ops.layer_inputs_visible()

    with kagnn_amd.collect_edge_l1(model):
        t = threading.Thread(target=other)
        t.start(); t.join()
        assert ops.layer_inputs_visible() and len(ops._edge_collectors()) == 1      # the other thread's block came and went unseen
    assert seen == {"visible": False, "blocks": 0, "own": True}


def test_parameter_gradients_cover_every_width_the_layer_checks_accept():
    """G + 2k + 1 <= 48 knots allows up to 46 coefficients (k = 1): the widest parameter-gradient kernel holds 48 dense columns, and the
    workspace grows with C + 1; one knot more is refused like everywhere else"""
    lib = _lib_or_build()
    n, m = ctypes.c_size_t(0), ctypes.c_size_t(0)
    for G, k in ((45, 1), (43, 2), (41, 3), (39, 4)):
        assert lib.kagnn_kan_edge_abs_sum_workspace_bytes(1000, 8, 8, G, k, ctypes.byref(n)) == 0
        assert lib.kagnn_kan_edge_abs_sum_bwd_workspace_bytes(1000, 8, 8, G, k, ctypes.byref(m)) == 0
        assert m.value == n.value * (G + k + 1)
        assert lib.kagnn_kan_edge_abs_sum_bwd_workspace_bytes(1000, 8, 8, G + 1, k, ctypes.byref(m)) == KAGNN_ERR_UNSUPPORTED
    src = open(os.path.join(ROOT, "kagnn_amd", "csrc", "kan_edge.hip")).read()
    assert "static_assert(kEdgeMaxNQ * 4 >= (kMaxKnots - 2) + 1" in src and "if (NQ * 4 < C + 1) return fail(" in src
