"""Grid refinement, host side (no GPU): the size query of ``kagnn_kan_grid_resize``, and what ``ops.kan_grid_resize``,
``KANLinear.refine``, ``KAN.refine`` and ``kagnn_amd.refine_grids`` refuse before anything is launched."""
import ctypes

import pytest
import torch

import kagnn_amd
from kagnn_amd import _lib, ops


def _query(lib, *args):
    out = ctypes.c_size_t(0)
    return lib.kagnn_kan_grid_resize_workspace_bytes(*args, ctypes.byref(out)), out.value


def test_version_and_symbols():
    lib = _lib.load()
    assert lib.kagnn_version() >= 272
    assert hasattr(lib, "kagnn_kan_grid_resize") and hasattr(lib, "kagnn_kan_grid_resize_workspace_bytes")
    assert callable(kagnn_amd.refine_grids) and callable(ops.kan_grid_resize)
    assert callable(kagnn_amd.KANLinear.refine) and callable(kagnn_amd.KAN.refine)


def test_size_query():
    lib = _lib.load()
    refit = ctypes.c_size_t(0)
    for n, fin, g0, g1, k in [(1, 1, 1, 2, 1), (4000, 6, 5, 20, 3), (1 << 20, 64, 8, 40, 3), (20000, 2, 9, 45, 1), (20000, 4, 13, 39, 4),
                              (4000, 6, 10, 5, 3)]:
        rc, nbytes = _query(lib, n, fin, g0, g1, k)
        assert rc == 0 and nbytes > 0, (n, fin, g0, g1, k)
    # the codes of the neighbouring query, kagnn_kan_grid_refit_workspace_bytes
    unsupported = lib.kagnn_kan_grid_refit_workspace_bytes(1000, 8, 5, 5, ctypes.byref(refit))
    no_rows = lib.kagnn_kan_grid_refit_workspace_bytes(0, 8, 5, 3, ctypes.byref(refit))
    assert unsupported != 0 and no_rows != 0
    assert _query(lib, 1000, 8, 5, 10, 5)[0] == unsupported             # order 5
    assert _query(lib, 1000, 8, 5, 42, 3)[0] == unsupported             # 49 knots on the new side
    assert _query(lib, 1000, 8, 42, 5, 3)[0] == unsupported             # ... and on the old side
    assert _query(lib, 1000, 8, 5, 41, 3)[0] == 0                       # 48 knots: the limit itself
    assert _query(lib, 20000, 4, 10, 40, 4)[0] == unsupported          # 44 coefficients at order 4 are 49 knots
    assert _query(lib, 1000, 8, 0, 5, 3)[0] != 0 and _query(lib, 1000, 8, 5, 0, 3)[0] != 0
    assert _query(lib, 0, 8, 5, 10, 3)[0] == no_rows
    assert lib.kagnn_kan_grid_resize_workspace_bytes(1000, 8, 5, 10, 3, None) != 0


def test_one_size_query():
    """``kagnn_kan_grid_refit`` is the resize between two grids of one size: its size query answers what the resize's does"""
    lib = _lib.load()
    refit = ctypes.c_size_t(0)
    for n, fin, g, k in [(1000, 8, 5, 3), (1000, 8, 32, 3), (100000, 64, 13, 3), (1, 1, 1, 1)]:
        rc, nbytes = _query(lib, n, fin, g, g, k)
        assert rc == 0 and nbytes > 0, (n, fin, g, k)
        assert lib.kagnn_kan_grid_refit_workspace_bytes(n, fin, g, k, ctypes.byref(refit)) == 0, (n, fin, g, k)
        assert refit.value == nbytes, (n, fin, g, k)
    rc = lib.kagnn_kan_grid_refit_workspace_bytes(1000, 8, 42, 3, ctypes.byref(refit))          # 49 knots
    assert rc == _query(lib, 1000, 8, 42, 42, 3)[0] == -3                                         # KAGNN_ERR_UNSUPPORTED


def test_a_finer_grid_needs_more_workspace_but_nothing_per_row():
    lib = _lib.load()
    small, big = _query(lib, 4096, 8, 5, 10, 3)[1], _query(lib, 4096, 8, 8, 40, 3)[1]
    assert big > small
    # nothing of size N x in x C: a 256-fold row count costs at most the slab cap, not 256 times the bytes
    assert _query(lib, 1 << 20, 8, 8, 40, 3)[1] <= 256 * big // 2
    assert _query(lib, 1 << 24, 64, 8, 40, 3)[1] == _query(lib, 1 << 22, 64, 8, 40, 3)[1]


def test_cpu_tensors_are_refused():
    layer = kagnn_amd.KANLinear(3, 2)
    x = torch.randn(10, 3)
    new_grid = kagnn_amd.KANLinear(3, 2, grid_size=10).grid
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.kan_grid_resize(x, layer.grid, new_grid, layer.spline_weight, None, 5, 10, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer.refine(x, 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kagnn_amd.KAN([3, 4, 2]).refine(x, 10)
    assert layer.grid_size == 5 and layer.spline_weight.shape == (2, 3, 8)


def test_orders_above_four_are_refused():
    layer = kagnn_amd.KANLinear(3, 2, grid_size=4, spline_order=6)
    with pytest.raises(NotImplementedError, match="spline_order"):
        layer.refine(torch.randn(10, 3), 8)
    with pytest.raises(NotImplementedError, match="spline_order"):
        ops.kan_grid_resize(torch.randn(10, 3), layer.grid, layer.grid, layer.spline_weight, None, 4, 4, 6)


@pytest.mark.parametrize("grid_size,order", [(0, 3), (-2, 3), (42, 3), (46, 1), (40, 4)])
def test_bad_grid_sizes_raise_before_any_launch(grid_size, order):
    """CPU tensors on purpose: the size check comes first, so it is a ValueError and not the CPU refusal"""
    layer = kagnn_amd.KANLinear(3, 2, grid_size=5, spline_order=order)
    x = torch.randn(10, 3)
    with pytest.raises(ValueError, match="grid_size"):
        layer.refine(x, grid_size)
    with pytest.raises(ValueError, match="grid_size"):
        ops.kan_grid_resize(x, layer.grid, layer.grid, layer.spline_weight, None, 5, grid_size, order)
    with pytest.raises(ValueError, match="grid_size"):
        kagnn_amd.refine_grids(torch.nn.Sequential(layer), grid_size, x)
    assert layer.grid_size == 5 and ops._refine_walk() is None and not ops.layer_inputs_visible()


def test_a_failed_walk_restores_the_flags_and_the_routing():
    model = torch.nn.Sequential(torch.nn.Dropout(0.5), kagnn_amd.KANLinear(3, 2)).train()
    model[1].eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kagnn_amd.refine_grids(model, 10, torch.randn(10, 3))
    assert model.training and model[0].training and not model[1].training
    assert ops._refine_walk() is None and not ops.layer_inputs_visible()
    assert model[1].grid_size == 5
