"""Host side of the FastKAN per-edge activation entry points (csrc/fastkan_edge.hip): ABI surface, workspace queries, argument
checks, what the Python surface refuses, the reference's ``plot_curve`` signature and the spill gate -- all without a GPU."""
import ctypes
import importlib.util
import inspect
import os
import re
import shutil

import pytest
import torch

import kagnn_amd
from kagnn_amd import _build, _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("kagnn_fastkan_edge_abs_sum_workspace_bytes", "kagnn_fastkan_edge_abs_sum", "kagnn_fastkan_edge_abs_sum_bwd_workspace_bytes",
           "kagnn_fastkan_edge_abs_sum_bwd", "kagnn_fastkan_edge_curves")
KAGNN_ERR_ARG, KAGNN_ERR_UNSUPPORTED = -1, -3


def _lib_or_build():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_version_and_symbols():
    lib = _lib_or_build()
    assert lib.kagnn_version() >= 270
    header = open(os.path.join(ROOT, "include", "kagnn_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED and hasattr(lib, name), name
    assert "fastkan_edge.hip" in _build.SOURCES


def test_workspace_queries():
    lib = _lib_or_build()
    n = ctypes.c_size_t(0)
    for fn, per_slab in ((lib.kagnn_fastkan_edge_abs_sum_workspace_bytes, 64 * 64 * 4),
                         (lib.kagnn_fastkan_edge_abs_sum_bwd_workspace_bytes, 64 * 64 * 9 * 4)):
        for layernorm in (0, 1):
            last = 0
            for rows in (0, 1, 1000, 1 << 20, 1 << 24):
                assert fn(rows, 64, 64, 8, layernorm, ctypes.byref(n)) == 0
                assert n.value >= per_slab and n.value >= last, (rows, layernorm)          # monotone in the rows
                last = n.value
            if not layernorm:       # slab partials only: bounded in the row count (nothing proportional to N * out)
                assert last <= 2048 * per_slab
        assert fn(10, 4, 4, 8, 0, None) == KAGNN_ERR_ARG
        assert fn(-1, 4, 4, 8, 0, ctypes.byref(n)) == KAGNN_ERR_ARG
        assert fn(10, 0, 4, 8, 0, ctypes.byref(n)) == KAGNN_ERR_ARG
        for ng in (0, 49):
            assert fn(10, 4, 4, ng, 0, ctypes.byref(n)) == KAGNN_ERR_UNSUPPORTED
            assert b"num_grids out of range" in lib.kagnn_last_error()
        for ng in (1, 32, 48):      # every centre count the layer takes, the 49 dense columns of the parameter kernel included
            assert fn(1000, 8, 8, ng, 1, ctypes.byref(n)) == 0
    m = ctypes.c_size_t(0)
    for ng in (1, 8, 48):           # the parameter partials grow with num_grids + 1 columns
        assert lib.kagnn_fastkan_edge_abs_sum_workspace_bytes(1000, 8, 8, ng, 0, ctypes.byref(n)) == 0
        assert lib.kagnn_fastkan_edge_abs_sum_bwd_workspace_bytes(1000, 8, 8, ng, 0, ctypes.byref(m)) == 0
        assert m.value == n.value * (ng + 1)


def test_argument_checks_need_no_device():
    lib = _lib_or_build()
    one = ctypes.c_void_p(16)       # never dereferenced: every call below fails its checks first
    big = 1 << 24
    fwd, bwd, curves = lib.kagnn_fastkan_edge_abs_sum, lib.kagnn_fastkan_edge_abs_sum_bwd, lib.kagnn_fastkan_edge_curves

    def f(x=one, ldx=4, n=8, fin=4, fout=4, ng=8, c=one, den=0.5, lw=one, lb=one, sw=one, bw=one, S=one, ldS=4, ws=one, nbytes=big):
        return fwd(x, ldx, n, fin, fout, ng, c, den, lw, lb, 1e-5, sw, bw, S, ldS, ws, nbytes, None)

    def b(x=one, ldx=4, n=8, fin=4, fout=4, ng=8, c=one, den=0.5, lw=one, lb=one, sw=one, bw=one, gS=one, ldgS=4, gsw=one, gbw=one, gx=one,
          ldgx=4, glw=one, glb=one, ws=one, nbytes=big):
        return bwd(x, ldx, n, fin, fout, ng, c, den, lw, lb, 1e-5, sw, bw, gS, ldgS, gsw, gbw, gx, ldgx, glw, glb, ws, nbytes, None)

    def cv(t=one, ldt=0, tb=None, ldtb=0, p=8, fin=4, fout=4, ng=8, c=one, den=0.5, sw=one, bw=one, phi=one):
        return curves(t, ldt, tb, ldtb, p, fin, fout, ng, c, den, sw, bw, phi, None)

    for ng in (0, 49, -1):
        assert f(ng=ng) == KAGNN_ERR_UNSUPPORTED and b(ng=ng) == KAGNN_ERR_UNSUPPORTED and cv(ng=ng) == KAGNN_ERR_UNSUPPORTED
    assert f(ldx=3) == KAGNN_ERR_ARG                       # ldx < in
    assert f(ldS=3) == KAGNN_ERR_ARG                       # ld of S < in
    assert f(sw=None) == KAGNN_ERR_ARG                     # no spline weight
    assert f(S=None) == KAGNN_ERR_ARG                      # no output
    assert f(lb=None) == KAGNN_ERR_ARG                     # half a layernorm
    assert f(den=0.0) == KAGNN_ERR_ARG
    assert f(nbytes=16) == KAGNN_ERR_ARG                   # workspace too small
    assert b"workspace too small" in lib.kagnn_last_error()
    assert f(lw=None, lb=None, nbytes=16) == KAGNN_ERR_ARG
    assert b(ldx=3) == KAGNN_ERR_ARG and b(ldgS=3) == KAGNN_ERR_ARG and b(ldgx=3) == KAGNN_ERR_ARG
    assert b(sw=None) == KAGNN_ERR_ARG                     # no spline weight
    assert b(gS=None) == KAGNN_ERR_ARG                     # no upstream
    assert b(bw=None) == KAGNN_ERR_ARG                     # g_bw without bw
    assert b(lw=None, lb=None) == KAGNN_ERR_ARG            # layernorm gradients without layernorm
    assert b(glb=None) == KAGNN_ERR_ARG                    # half a pair
    assert b(gx=None) == KAGNN_ERR_ARG                     # layernorm gradients without gx
    assert b(ws=None, nbytes=0) == KAGNN_ERR_ARG           # no workspace
    assert b(nbytes=16) == KAGNN_ERR_ARG                   # workspace too small
    assert b"workspace too small" in lib.kagnn_last_error()
    assert cv(ldt=3) == KAGNN_ERR_ARG                      # 0 < ldt < in
    assert cv(tb=one, ldtb=3) == KAGNN_ERR_ARG             # 0 < ld of the base points < in
    assert cv(phi=None) == KAGNN_ERR_ARG                   # no output
    assert cv(sw=None, bw=None) == KAGNN_ERR_ARG           # neither branch
    assert cv(t=None) == KAGNN_ERR_ARG                     # a spline branch without points
    assert cv(t=None, tb=None, p=0, c=None, sw=one, bw=None, phi=None) == 0                 # no points: nothing to do


def test_python_surface_refuses_cpu_tensors():
    layer = kagnn_amd.FastKANLayer(3, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer.edge_l1(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer.edge_curves(torch.zeros(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer.plot_curve(0, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer.regularization_loss(torch.zeros(4, 3))
    chain = kagnn_amd.FastKAN([3, 4, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        chain.regularization_loss(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        chain.edge_l1(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.fastkan_edge_abs_sum(torch.zeros(4, 3), None, None, torch.zeros(2, 24), None, torch.linspace(-2, 2, 8), 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.fastkan_edge_curves(torch.zeros(4), torch.zeros(2, 24), None, torch.linspace(-2, 2, 8), 0.5)
    # a CPU forward inside a collect_edge_l1 block reaches the collection, which refuses like every op
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        with kagnn_amd.collect_edge_l1(chain):
            chain(torch.zeros(4, 3))
    assert not ops.layer_inputs_visible()


def test_collect_edge_l1_names_fastkan_layers_beside_kanlinears():
    both = torch.nn.ModuleDict({"kan": kagnn_amd.KAN([3, 4, 2]), "fast": kagnn_amd.FastKAN([3, 4, 2]),
                                "high": kagnn_amd.KANLinear(3, 2, spline_order=6)})
    with kagnn_amd.collect_edge_l1(both) as stats:
        assert stats == {}
        names, _ = ops._edge_collectors()[-1]
        assert sorted(names.values()) == ["fast.layers.0", "fast.layers.1", "kan.layers.0", "kan.layers.1"]
    assert not ops.layer_inputs_visible()


def test_plot_curve_has_the_reference_signature():
    sig = inspect.signature(kagnn_amd.FastKANLayer.plot_curve)
    assert list(sig.parameters) == ["self", "input_index", "output_index", "num_pts", "num_extrapolate_bins"]
    assert sig.parameters["num_pts"].default == 1000 and sig.parameters["num_extrapolate_bins"].default == 2
    assert sig.parameters["input_index"].default is inspect.Parameter.empty
    reg = inspect.signature(kagnn_amd.FastKANLayer.regularization_loss)
    assert list(reg.parameters) == ["self", "x", "regularize_activation", "regularize_entropy"]
    assert reg.parameters["x"].default is inspect.Parameter.empty            # no weight stand-in: the rows are required
    assert reg.parameters["regularize_activation"].default == 1.0 and reg.parameters["regularize_entropy"].default == 1.0
    layer = kagnn_amd.FastKANLayer(3, 2)
    with pytest.raises(AssertionError):
        layer.plot_curve(3, 0)
    with pytest.raises(AssertionError):
        layer.plot_curve(0, 2)


def test_fastkan_edge_kernels_do_not_spill():
    objdir = os.path.join(ROOT, "kagnn_amd", "lib", "obj")
    if not os.path.isdir(objdir) or not shutil.which("c++filt") or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no build objects / LLVM tools on this machine (the library was shipped prebuilt)")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = [k for k in kr.collect(objdir) if "fastkan_edge" in k["demangled"]]
    names = sorted(k["demangled"] for k in rows)
    # {abs sum, gx, curves} x 5 centre bounds of the row kernel, 4 column widths of the parameter kernel (the widest: 52 >= 48 + 1)
    want = sorted(["fastkan_edge::rows_kernel<%d,%d>" % (gc, mode) for gc in (4, 8, 16, 32, 48) for mode in (0, 1, 2)]
                  + ["fastkan_edge::param_kernel<%d>" % nq for nq in (3, 5, 9, 13)])
    assert names == want, names
    assert all(k["tu"] == "fastkan_edge" for k in rows)
    bad = [k for k in rows if k["vgpr_spill_count"] or k["private_segment_fixed_size"]]
    assert not bad, [(k["name"], k["vgpr_spill_count"], k["private_segment_fixed_size"]) for k in bad]
    # the slab reductions are kan_edge.hip's, shared through edge_common.h: the new translation unit holds no kernel but the two above
    assert len(rows) == len([k for k in kr.collect(objdir) if k["tu"] == "fastkan_edge"])
