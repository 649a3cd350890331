"""KANLinear at spline orders 5..16, the host side: constructor and shapes, the widened C ABI, and the compiler's resource
report of the new kernels (kan_high_order.hip).  No GPU needed."""
import ctypes
import os
import sys

import pytest
import torch

import kagnn_amd
from kagnn_amd import _lib
from oracle import kan_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("g,k", [(5, 5), (3, 8), (16, 16), (1, 16)])
def test_constructor_accepts_orders_5_8_16(g, k):
    torch.manual_seed(0)
    layer = kagnn_amd.KANLinear(6, 4, grid_size=g, spline_order=k)
    assert layer.grid.shape == (6, g + 2 * k + 1)
    assert torch.equal(layer.grid, orc.make_knots(6, g, k))          # the reference's knot values, to the bit
    assert layer.spline_weight.shape == (4, 6, g + k)
    assert layer.base_weight.shape == (4, 6) and layer.spline_scaler.shape == (4, 6)
    for p in layer.parameters():
        assert bool(torch.isfinite(p).all())
    chain = kagnn_amd.KAN([6, 5, 3], grid_size=g, spline_order=k)
    assert [l.spline_order for l in chain.layers] == [k, k]


@pytest.mark.parametrize("g,k,word", [(3, 17, "16"), (32, 16, "64"), (3, 0, "16")])
def test_constructor_refuses_what_is_out_of_range(g, k, word):
    with pytest.raises(NotImplementedError, match=word):
        kagnn_amd.KANLinear(3, 3, grid_size=g, spline_order=k)
    with pytest.raises(NotImplementedError, match=word):
        kagnn_amd.KAN([3, 3, 3], grid_size=g, spline_order=k)


def test_the_largest_grid_of_every_order_constructs():
    for k in range(5, 17):
        g = 64 - 2 * k - 1
        assert kagnn_amd.KANLinear(2, 2, grid_size=g, spline_order=k).grid.shape == (2, 64)
        with pytest.raises(NotImplementedError):
            kagnn_amd.KANLinear(2, 2, grid_size=g + 1, spline_order=k)


def _err(lib):
    return lib.kagnn_last_error().decode()


def test_abi_sizes_answer_in_the_exact_modes_only():
    lib = _lib.load()
    assert lib.kagnn_version() >= 268
    assert _lib.MAX_SPLINE_ORDER == 16
    fb, db = ctypes.c_size_t(0), ctypes.c_size_t(0)
    for mode in (_lib.PREC_FP32, _lib.PREC_FP32_GRID):
        assert lib.kagnn_kan_pack_bytes(64, 64, 5, 7, mode, ctypes.byref(fb), ctypes.byref(db)) == 0, _err(lib)
        # the fp32 packs, generic in C: [P][C+1][OT][64] and [FT][C+1][16 OT][64] floats
        assert fb.value == 32 * 13 * 2 * 64 * 4 and db.value == 2 * 13 * 32 * 64 * 4
    for mode in (_lib.PREC_SPLIT, _lib.PREC_HALF):
        assert lib.kagnn_kan_pack_bytes(64, 64, 5, 7, mode, ctypes.byref(fb), ctypes.byref(db)) == -3
        assert "spline_order" in _err(lib)
    assert lib.kagnn_kan_pack_bytes(64, 64, 2, 17, _lib.PREC_FP32, ctypes.byref(fb), ctypes.byref(db)) == -3
    assert "spline_order" in _err(lib)
    assert lib.kagnn_kan_pack_bytes(64, 64, 32, 16, _lib.PREC_FP32, ctypes.byref(fb), ctypes.byref(db)) == -3
    assert "64" in _err(lib)
    wb = ctypes.c_size_t(123)
    assert lib.kagnn_kan_fwd_workspace_bytes(1000, 64, 64, 16, 16, _lib.PREC_FP32, ctypes.byref(wb)) == 0, _err(lib)
    assert wb.value == 0
    assert lib.kagnn_kan_bwd_weight_workspace_bytes(1000, 64, 64, 16, 16, _lib.PREC_FP32, ctypes.byref(wb)) == 0, _err(lib)
    assert wb.value >= 33 * 64 * 64 * 4 * 2                          # the reduced [C+1][in][out] block and at least one slab
    assert lib.kagnn_kan_bwd_weight_workspace_bytes(1000, 64, 64, 16, 16, _lib.PREC_SPLIT, ctypes.byref(wb)) == -3


def test_the_other_entry_points_refuse_the_order_with_a_message():
    lib = _lib.load()
    wb = ctypes.c_size_t(0)
    assert lib.kagnn_kan_fwd_moments_workspace_bytes(1000, 64, 64, 3, 8, _lib.PREC_FP32, ctypes.byref(wb)) == -3
    assert "spline_order" in _err(lib)
    assert lib.kagnn_kan_grid_refit_workspace_bytes(1000, 64, 3, 8, ctypes.byref(wb)) == -3
    assert "spline_order" in _err(lib)
    widths = (ctypes.c_int32 * 2)(64, 64)
    assert lib.kagnn_kan_fwd_parts_ok(widths, 2, 128, 64, 3, 8, _lib.PREC_SPLIT) == 0
    fws, bws = ctypes.c_size_t(0), ctypes.c_size_t(0)
    w3 = (ctypes.c_int32 * 3)(64, 64, 64)
    assert lib.kagnn_gin_kan_layer_workspace_bytes(1000, 2, w3, 3, 8, _lib.PREC_FP32, 0, 0, ctypes.byref(fws), ctypes.byref(bws)) == -3
    assert "spline_order" in _err(lib)


@pytest.mark.parametrize("conv_k,readout_k", [(3, 8), (8, 3)])
def test_the_model_call_refuses_the_order_in_the_stack_and_in_the_read_out(conv_k, readout_k):
    lib = _lib.load()
    m = _lib.KaginModel()
    m.num_nodes, m.num_edges, m.num_graphs, m.hidden = 100, 300, 4, 16
    m.num_atom_tables = m.num_bond_tables = m.x_stride = m.e_stride = 1
    m.num_convs, m.num_layers, m.grid_size, m.spline_order, m.mode = 2, 2, 3, conv_k, _lib.PREC_FP32
    m.num_readout, m.readout_grid_size, m.readout_spline_order = 1, 3, readout_k
    m.readout_widths[0], m.readout_widths[1] = 16, 1
    m.readout_modes[0] = _lib.PREC_FP32
    m.atom_rows[0], m.bond_rows[0] = 5, 4
    sizes = [ctypes.c_size_t(0) for _ in range(4)]
    good = (m.spline_order, m.readout_spline_order)
    assert lib.kagnn_kagin_model_sizes(ctypes.byref(m), *[ctypes.byref(v) for v in sizes]) == -3
    assert "spline_order" in _err(lib)
    m.spline_order = m.readout_spline_order = 3                     # the same struct at order 3 is sized: the refusal was the order's
    assert good != (3, 3) and lib.kagnn_kagin_model_sizes(ctypes.byref(m), *[ctypes.byref(v) for v in sizes]) == 0, _err(lib)


def test_routing_predicates_send_high_orders_to_the_composition():
    from kagnn_amd import ops
    chain = kagnn_amd.KAN([8, 8, 8], grid_size=3, spline_order=8)
    assert ops._chain_plan(list(chain.layers)) is None
    assert chain.layers[0].read_out_blocks_in_one_launch((4, 4)) is False
    assert ops.parts_affine_ok(8, 3, 8, [torch.zeros(4, 64)], [True]) is False
    with pytest.raises(NotImplementedError, match="ill-conditioned"):
        chain.layers[0].update_grid(torch.zeros(16, 8))
    from kagnn_amd.sharded import ShardedKANLinear
    with pytest.raises(ValueError, match="not supported"):
        ShardedKANLinear(chain.layers[0], 0, 1)


def test_new_kernels_use_no_scratch():
    objdir = os.path.join(ROOT, "kagnn_amd", "lib", "obj")
    if not os.path.exists(os.path.join(objdir, "kan_high_order.o")):
        pytest.skip("no build objects here (kagnn_amd/lib/obj): the resource report reads them")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = [r for r in kernel_resources.collect(objdir) if "kan_ho_" in r["demangled"]]
    names = {r["demangled"].split("<")[0].split("::")[-1].split()[-1] for r in rows}
    assert {"kan_ho_fwd_kernel", "kan_ho_dx_kernel", "kan_ho_dw_kernel", "kan_ho_bsplines_kernel"} <= names, names
    assert len(rows) >= 30
    for r in rows:
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, r
