"""The torch.compile route (kagnn_amd/library.py) against the fp64 oracle, op by op.

Every public function of ``kagnn_amd.ops`` has two host routes to the same kernels: the ``torch.autograd.Function`` nodes of eager
code and, while dynamo traces, the ``kagnn::*`` custom ops with their own autograd formulas, ``register_fake`` shape functions and
wrappers (``_AggregateBoth``, ``batch_norm_traced``).  Part A calls those ops eagerly under autograd -- exactly the traced route's
formulas, without the cost of tracing -- and holds forward and every gradient to fp64; part B runs ``torch.library.opcheck`` on every
op; part C compiles a handful of modules (``aot_eager``, ``fullgraph=True``) in the states the traced route used to get wrong.

Bounds.  ``TOL`` (2e-5 of the tensor's own maximum, ``helpers.assert_close``) for every single op and layer: the same kernels the
eager tests hold to it.  ``KAGNN_PREC_HALF``: ``helpers.half_parity`` against ``half_mode_oracle``, inputs built as in
tests/test_gpu_half.py.  Whole models: ``MODEL_TOL`` = 1e-4, the whole-model rule of tests/test_gpu_models.py (errors compound
through BatchNorm and several layers).  Everything else is derived in a comment where it is used.
"""
import re
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import kagnn_amd
from kagnn_amd import library, ops
from kagnn_amd._lib import PREC_FP32, PREC_FP32_GRID, PREC_HALF, PREC_SPLIT
from oracle import kan_oracle as orc
from helpers import (TOL, assert_close, half_mode_oracle, half_parity, must_fail, oracle_node_model_fwd_bwd, prenorm_bias_noise)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODEL_TOL = 1e-4
EPS32 = 2.0 ** -23
KAN_NAMES = ("base_weight", "spline_weight", "spline_scaler")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _dev(t, grad=False):
    return None if t is None else t.to(DEV).requires_grad_(grad)


# ================================================================================================ A. kagnn::kan_linear
def _jittered(grid, seed, share=0.3):
    """per-feature rows, every knot moved by up to ``share`` of a step (tests/test_gpu_grid_refine.py): rows stay strictly increasing"""
    step = float(grid[0, 1] - grid[0, 0])
    out = (grid + share * step * (2 * torch.rand(grid.shape, generator=_gen(seed)) - 1)).contiguous()
    assert bool((out[:, 1:] > out[:, :-1]).all()) and not torch.equal(out[0], out[1])
    return out


def _kan_case(n, fin, fout, G, k, seed, per_feature=False, nan_row=False, half=False):
    gen = _gen(seed)
    if half:                                              # the operands of tests/test_gpu_half.py: its bounds belong to them
        p = orc.init_kan_linear(fin, fout, G, k, gen)
        x = torch.randn(n, fin, generator=gen) * 0.8
        x[::7, 0] = 3.0
        gy = torch.randn(n, fout, generator=gen) * torch.logspace(-3, 2, n).unsqueeze(1)
        return x, gy, p
    grid = orc.make_knots(fin, G, k)
    if per_feature:
        grid = _jittered(grid, G)
    p = {"base_weight": 0.3 * torch.randn(fout, fin, generator=gen), "spline_weight": 0.3 * torch.randn(fout, fin, G + k, generator=gen),
         "spline_scaler": torch.randn(fout, fin, generator=gen), "grid": grid}
    x = torch.randn(n, fin, generator=gen) * 0.8
    x[::7, 0] = float(grid.max()) + 0.25                 # a column outside the spline support
    if nan_row:
        x[n // 2, :] = float("nan")
    return x, torch.randn(n, fout, generator=gen), p


def _kan_oracle(x, gy, p, k):
    """fp64: y and the gradient of every operand that is there (a missing base branch is a zero base weight)"""
    xr = x.double().requires_grad_(True)
    leaves = {nm: None if p[nm] is None else p[nm].double().requires_grad_(True) for nm in KAN_NAMES}
    bw = leaves["base_weight"] if leaves["base_weight"] is not None else torch.zeros(p["spline_weight"].shape[:2], dtype=torch.float64)
    y = orc.kan_linear_forward(xr, bw, leaves["spline_weight"], leaves["spline_scaler"], p["grid"].double(), k)
    y.backward(gy.double())
    return {"y": y.detach(), "x": xr.grad, **{nm: None if v is None else v.grad for nm, v in leaves.items()}}


def _kan_device(x, gy, p, G, k, mode, need=("x",) + KAN_NAMES):
    """the op under autograd; -> y and the .grad of every operand (None where there is none)"""
    xd = _dev(x, "x" in need)
    w = {nm: _dev(p[nm], nm in need) for nm in KAN_NAMES}
    grid = p["grid"].to(DEV)
    knots = grid.contiguous() if mode == PREC_FP32_GRID else grid[0].contiguous()
    y, pack = library.kan_linear(xd, w["base_weight"], w["spline_weight"], w["spline_scaler"], knots, G, k, mode)
    assert y.shape == (x.size(0), p["spline_weight"].size(0)) and pack.dtype == torch.uint8
    y.backward(gy.to(DEV))
    return {"y": y.detach(), "x": xd.grad, **{nm: None if w[nm] is None else w[nm].grad for nm in KAN_NAMES}}


KAN_CASES = [  # id, (n, fin, fout, G, k), mode, per-feature knots
    ("split-1037", (1037, 33, 17, 4, 3), PREC_SPLIT, False), ("fp32-1037", (1037, 33, 17, 4, 3), PREC_FP32, False),
    ("split-777", (777, 64, 40, 5, 3), PREC_SPLIT, False), ("fp32-777", (777, 64, 40, 5, 3), PREC_FP32, False),
    ("split-1row", (1, 33, 17, 4, 3), PREC_SPLIT, False), ("fp32-1row", (1, 33, 17, 4, 3), PREC_FP32, False),
    ("grid-1037", (1037, 33, 17, 4, 3), PREC_FP32_GRID, True), ("grid-777", (777, 64, 40, 5, 3), PREC_FP32_GRID, True),
    ("order5", (33, 2, 33, 5, 5), PREC_FP32, False), ("order8", (129, 33, 5, 3, 8), PREC_FP32, False),
    ("order8-grid", (129, 33, 5, 3, 8), PREC_FP32_GRID, True)]


@pytest.mark.parametrize("shape,mode,per_feature", [c[1:] for c in KAN_CASES], ids=[c[0] for c in KAN_CASES])
def test_kan_linear_op_and_formula_vs_fp64(shape, mode, per_feature):
    n, fin, fout, G, k = shape
    x, gy, p = _kan_case(n, fin, fout, G, k, sum(shape) + mode, per_feature)
    want, got = _kan_oracle(x, gy, p, k), _kan_device(x, gy, p, G, k, mode)
    for nm in want:
        assert_close(got[nm], want[nm], what=f"kagnn::kan_linear {shape} mode {mode}: {nm}")


@pytest.mark.parametrize("shape", [(1037, 33, 17, 4, 3), (777, 64, 40, 5, 3)], ids=str)
def test_kan_linear_op_half_mode_vs_rounding_oracle(shape):
    n, fin, fout, G, k = shape
    x, gy, p = _kan_case(n, fin, fout, G, k, n + fin, half=True)
    plain = _kan_oracle(x, gy, p, k)
    with half_mode_oracle():
        rounded = _kan_oracle(x, gy, p, k)
    got = _kan_device(x, gy, p, G, k, PREC_HALF)
    for nm in got:
        what = f"kagnn::kan_linear {shape} half: {nm}"
        if nm == "x":       # the rows' scales span five decades and each row is rounded at its own scale: row-normalised, as test_gpu_half.py
            rs = rounded[nm].abs().amax(1, keepdim=True).clamp(min=1e-300)
            half_parity(got[nm].cpu().double() / rs, rounded[nm] / rs, plain[nm] / rs, what + " (per row)")
        else:
            half_parity(got[nm], rounded[nm], plain[nm], what)


KAN_OPTIONS = {  # id -> (operands set to None, operands that require a gradient)
    "no-base": (("base_weight",), ("x", "spline_weight", "spline_scaler")),
    "no-scaler": (("spline_scaler",), ("x", "base_weight", "spline_weight")),
    "neither": (("base_weight", "spline_scaler"), ("x", "spline_weight")),
    "weights-only": ((), KAN_NAMES),
    "x-only": ((), ("x",)),
    "x-and-spline": ((), ("x", "spline_weight"))}


@pytest.mark.parametrize("mode", [PREC_SPLIT, PREC_FP32], ids=["split", "fp32"])
@pytest.mark.parametrize("option", list(KAN_OPTIONS))
def test_kan_linear_op_absent_operands_and_gradients(option, mode):
    absent, need = KAN_OPTIONS[option]
    shape = (1037, 33, 17, 4, 3)
    x, gy, p = _kan_case(*shape, 99)
    p = {nm: (None if nm in absent else v) for nm, v in p.items()}
    want, got = _kan_oracle(x, gy, p, 3), _kan_device(x, gy, p, 4, 3, mode, need)
    assert_close(got["y"], want["y"], what=f"kagnn::kan_linear {option}: y")
    for nm in ("x",) + KAN_NAMES:
        if nm in need:
            assert_close(got[nm], want[nm], what=f"kagnn::kan_linear {option} mode {mode}: {nm}")
        else:
            assert got[nm] is None, f"{option}: {nm} does not ask for a gradient"


@pytest.mark.parametrize("has_base,has_scaler,want_x", [(False, True, True), (True, False, True), (False, False, False), (True, True, False)])
def test_kan_formula_returns_none_for_absent_gradients(has_base, has_scaler, want_x):
    """the autograd formula itself: what it hands back for an absent operand is None, never the 0-element stand-in of the op"""
    x, gy, p = _kan_case(65, 9, 7, 4, 3, 5)
    xd, bw, sw, sc = _dev(x), _dev(p["base_weight"]) if has_base else None, _dev(p["spline_weight"]), _dev(p["spline_scaler"]) if has_scaler else None
    knots = p["grid"][0].contiguous().to(DEV)
    y, pack = torch.ops.kagnn.kan_linear(xd, bw, sw, sc, knots, 4, 3, PREC_FP32)
    ctx = SimpleNamespace(saved_tensors=(xd, sw, sc, knots, pack), meta=(7, 4, 3, PREC_FP32, has_base),
                          needs_input_grad=(want_x, has_base, True, has_scaler, False, False, False, False))
    out = library._kan_backward(ctx, gy.to(DEV), None)
    assert len(out) == 8 and all(o is None for o in out[4:])
    assert (out[0] is None) == (not want_x) and (out[1] is None) == (not has_base) and (out[3] is None) == (not has_scaler)
    assert out[2].shape == sw.shape and all(o is None or o.numel() > 0 for o in out)


NAN_ROW_CASES = [  # id, (n, fin, fout, G, k), mode, per-feature knots: every way the weight gradient leaves the device
    ("split", (1037, 33, 17, 4, 3), PREC_SPLIT, False), ("fp32", (1037, 33, 17, 4, 3), PREC_FP32, False),
    ("grid", (1037, 33, 17, 4, 3), PREC_FP32_GRID, True),
    ("split-11coef", (300, 33, 17, 8, 3), PREC_SPLIT, False), ("split-16coef-narrow", (300, 20, 10, 13, 3), PREC_SPLIT, False),
    ("order5", (33, 2, 33, 5, 5), PREC_FP32, False)]


@pytest.mark.parametrize("shape,mode,per_feature", [c[1:] for c in NAN_ROW_CASES], ids=[c[0] for c in NAN_ROW_CASES])
def test_kan_linear_op_nan_row(shape, mode, per_feature):
    """one NaN row: y and gx carry it in that row alone, as the oracle's do; the parameter gradients, sums over all rows, are NaN
    wherever the oracle's are (assert_close compares the patterns).  The oracle's dense basis table is NaN in EVERY coefficient of
    that row (NaN * 0), so all of its spline_weight gradient is NaN; the kernels evaluate the k + 1 bases of one span only (a
    non-finite x is put in span 0, where of the bases -k .. 0 only coefficient 0 exists: 561 of 3927 entries were NaN at
    (1037, 33, 17, G 4, k 3)) and the unpack kernels spread a NaN coefficient over its edge."""
    n, fin, fout, G, k = shape
    x, gy, p = _kan_case(n, fin, fout, G, k, 7, per_feature, nan_row=True)
    want, got = _kan_oracle(x, gy, p, k), _kan_device(x, gy, p, G, k, mode)
    rows = torch.isnan(want["y"]).any(1)
    assert int(rows.sum()) == 1 and bool(torch.isnan(want["x"]).any(1).eq(rows).all())
    assert bool(torch.isnan(want["spline_weight"]).all())
    nan = torch.isnan(got["spline_weight"]).cpu()
    print(f"NaN row {shape} mode {mode}: {int(nan.sum())} of {nan.numel()} entries of d/dspline_weight are NaN")
    for nm in want:
        assert_close(got[nm], want[nm], what=f"kagnn::kan_linear NaN row {shape} mode {mode}: {nm}")


def test_kan_linear_op_nan_in_one_column_poisons_that_column_only():
    """a NaN in x[n, f]: in d/dspline_weight every coefficient of the edges (., f) and nothing else, as the oracle"""
    shape = (1037, 33, 17, 4, 3)
    x, gy, p = _kan_case(*shape, 8)
    x[500, 5] = float("nan")
    want = _kan_oracle(x, gy, p, 3)
    assert bool(torch.isnan(want["spline_weight"][:, 5]).all()) and int(torch.isnan(want["spline_weight"]).sum()) == 17 * 7
    for mode in (PREC_SPLIT, PREC_FP32):
        got = _kan_device(x, gy, p, 4, 3, mode)
        for nm in KAN_NAMES:
            assert_close(got[nm], want[nm], what=f"kagnn::kan_linear one NaN entry mode {mode}: {nm}")


# ================================================================================================ A. kagnn::fastkan_layer
FK_NAMES = ("ln_weight", "ln_bias", "spline_weight", "base_weight", "base_bias")
FK_VARIANTS = {"full": (True, True, True), "no-ln": (False, True, True), "no-base": (True, False, False),
               "no-bias": (True, True, False), "bare": (False, False, False)}


@pytest.mark.parametrize("mode", [PREC_SPLIT, PREC_FP32], ids=["split", "fp32"])
@pytest.mark.parametrize("shape", [(1037, 33, 17), (777, 64, 40)], ids=str)
@pytest.mark.parametrize("variant", list(FK_VARIANTS))
def test_fastkan_layer_op_and_formula_vs_fp64(variant, shape, mode):
    ln, base, bias = FK_VARIANTS[variant]
    n, fin, fout = shape
    ng = 8
    gen = _gen(sum(shape) + 3 * len(variant))
    centers = torch.linspace(-2.0, 2.0, ng)
    den = 4.0 / (ng - 1)
    p = {"ln_weight": 1.0 + 0.3 * torch.randn(fin, generator=gen) if ln else None, "ln_bias": 0.3 * torch.randn(fin, generator=gen) if ln else None,
         "spline_weight": 0.1 * torch.randn(fout, fin * ng, generator=gen),
         "base_weight": 0.3 * torch.randn(fout, fin, generator=gen) if base else None, "base_bias": 0.3 * torch.randn(fout, generator=gen) if bias else None}
    x, gy = 0.8 * torch.randn(n, fin, generator=gen), torch.randn(n, fout, generator=gen)
    # fp64
    xr = x.double().requires_grad_(True)
    p64 = {nm: None if v is None else v.double().requires_grad_(True) for nm, v in p.items()}
    want = orc.fastkan_layer_forward(xr, p64["ln_weight"], p64["ln_bias"], centers.double(), den, p64["spline_weight"], p64["base_weight"], p64["base_bias"])
    want.backward(gy.double())
    # the op
    xd = _dev(x, True)
    w = {nm: _dev(v, True) for nm, v in p.items()}
    y, stats = library.fastkan_layer(xd, w["ln_weight"], w["ln_bias"], w["spline_weight"], w["base_weight"], w["base_bias"], centers.to(DEV), den, 1e-5, mode)
    assert stats.shape == ((n, 2) if ln else (0,))
    y.backward(gy.to(DEV))
    what = f"kagnn::fastkan_layer {variant} {shape} mode {mode}: "
    assert_close(y, want, what=what + "y")
    assert_close(xd.grad, xr.grad, what=what + "x")
    for nm in FK_NAMES:
        if p[nm] is not None:
            assert w[nm].grad is not None, nm
            assert_close(w[nm].grad, p64[nm].grad, what=what + nm)
    must_fail(torch.zeros_like(w["spline_weight"].grad), p64["spline_weight"].grad, what=what + "spline_weight zeroed")


# ================================================================================================ A. library.aggregate
@pytest.fixture(scope="module")
def graph():
    """the power-law graph of the compiled-model test: hub rows past hub_threshold (listed as segments by the rocPRIM build only),
    isolated nodes, self loops, duplicates"""
    n, e = 3000, 24000
    ei = orc.powerlaw_graph(n, e)
    small = ops._SMALL_CSR
    ops._SMALL_CSR = False
    try:
        g = ops.GraphIndex(ei.to(DEV), n)
    finally:
        ops._SMALL_CSR = small
    deg = torch.bincount(ei[1], minlength=n)
    assert g.num_hub_seg > 0 and int(deg.max()) > g.hub_threshold
    assert bool((deg == 0).any()) and bool((ei[0] == ei[1]).any())
    _ = g.gcn_dis                      # (host code: a library call dynamo cannot trace; cached on the graph)
    return SimpleNamespace(n=n, e=e, ei=ei, g=g)


def _agg64(x, ei, w, self_scale, in_scale, out_scale, skip, bias):
    """fp64: out[i] = out_scale[i] * (self_scale * s(i) x[i] + sum_{e: j -> i} w[e] s(j) x[j]) + bias, self loops dropped when ``skip``"""
    src, dst = ei[0], ei[1]
    s = torch.ones(x.size(0), dtype=torch.float64) if in_scale is None else in_scale
    ww = torch.ones(ei.size(1), dtype=torch.float64) if w is None else w
    if skip:
        ww = ww * (src != dst)
    out = (self_scale * s.unsqueeze(1) * x).index_add(0, dst, (ww * s[src]).unsqueeze(1) * x[src])
    if out_scale is not None:
        out = out_scale.unsqueeze(1) * out
    return out if bias is None else out + bias


AGG_OPTIONS = {  # id -> (self_scale, skip_self, in_scale, out_scale, bias, edge_weight)
    "self0": (0.0, False, False, False, False, False), "self1": (1.0, False, False, False, False, False),
    "self1.5": (1.5, False, False, False, False, False), "skip-self": (1.0, True, False, False, False, False),
    "in-scale": (1.0, False, True, False, False, False), "out-scale": (1.0, False, False, True, False, False),
    "bias": (1.0, False, False, False, True, False), "edge-weight": (1.0, False, False, False, False, True),
    "all": (1.5, True, True, True, True, True)}


def _agg_operands(graph, f, option, seed):
    self_scale, skip, use_in, use_out, use_b, use_w = AGG_OPTIONS[option]
    gen = _gen(seed)
    n = graph.n
    x, gout = 0.8 * torch.randn(n, f, generator=gen), 0.8 * torch.randn(n, f, generator=gen)
    s_in, s_out = 0.5 + torch.rand(n, generator=gen), 0.5 + torch.rand(n, generator=gen)
    b, w = torch.randn(f, generator=gen), 0.2 + torch.rand(graph.e, generator=gen)
    return SimpleNamespace(self_scale=self_scale, skip=skip, x=x, gout=gout, s_in=s_in if use_in else None, s_out=s_out if use_out else None,
                           b=b if use_b else None, w=w if use_w else None)


def _d(t):
    return None if t is None else t.double()


@pytest.mark.parametrize("f", [5, 16, 64])
@pytest.mark.parametrize("option", list(AGG_OPTIONS))
def test_aggregate_wrapper_and_transposed_formula_vs_fp64(graph, option, f):
    """out, d/dx (the same op on the transposed CSR: scales swapped, weights permuted) and d/dbias; the weights are constants"""
    c = _agg_operands(graph, f, option, 10 * f + len(option))
    x64 = c.x.double().requires_grad_(True)
    b64 = None if c.b is None else c.b.double().requires_grad_(True)
    want = _agg64(x64, graph.ei, _d(c.w), c.self_scale, _d(c.s_in), _d(c.s_out), c.skip, b64)
    want.backward(c.gout.double())
    xd, bd = _dev(c.x, True), _dev(c.b, True)
    got = library.aggregate(xd, graph.g, c.self_scale, _dev(c.w), _dev(c.s_in), _dev(c.s_out), bd, c.skip)
    got.backward(c.gout.to(DEV))
    what = f"library.aggregate {option} F={f}: "
    assert_close(got, want, what=what + "out")
    assert_close(xd.grad, x64.grad, what=what + "d/dx")
    if c.b is not None:
        assert_close(bd.grad, b64.grad, what=what + "d/dbias")
    if c.s_in is not None and c.s_out is not None:      # mutant: d/dx with the scales NOT swapped on the way back must be rejected
        ei_t = torch.stack([graph.ei[1], graph.ei[0]])
        unswapped = _agg64(c.gout.double(), ei_t, _d(c.w), c.self_scale, _d(c.s_in), _d(c.s_out), c.skip, None)
        must_fail(unswapped, x64.grad, what=what + "d/dx with in/out scales not swapped")


@pytest.mark.parametrize("option,f", [("edge-weight", 5), ("edge-weight", 64), ("all", 16), ("all", 64)])
def test_aggregate_wrapper_differentiates_through_edge_weight(graph, option, f):
    """weights that require a gradient get it (kagnn::aggregate_edge_grad), in original edge order, 0 on a dropped self loop"""
    c = _agg_operands(graph, f, option, 7 * f + 1)
    x64, w64 = c.x.double().requires_grad_(True), c.w.double().requires_grad_(True)
    want = _agg64(x64, graph.ei, w64, c.self_scale, _d(c.s_in), _d(c.s_out), c.skip, _d(c.b))
    want.backward(c.gout.double())
    xd, wd = _dev(c.x, True), _dev(c.w, True)
    got = library.aggregate(xd, graph.g, c.self_scale, wd, _dev(c.s_in), _dev(c.s_out), _dev(c.b), c.skip)
    got.backward(c.gout.to(DEV))
    what = f"library.aggregate {option} F={f}: "
    assert_close(got, want, what=what + "out")
    assert_close(xd.grad, x64.grad, what=what + "d/dx")
    assert wd.grad is not None, "edge_weight.requires_grad: the traced route must hand it a gradient"
    assert_close(wd.grad, w64.grad, what=what + "d/dedge_weight")
    if c.skip:
        assert bool((wd.grad.cpu()[graph.ei[0] == graph.ei[1]] == 0).all())
    must_fail(wd.grad[graph.g.perm.long()], w64.grad, what=what + "d/dedge_weight in CSR order")


# ================================================================================================ A. kagnn::batch_norm
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def _bn64(x, w, b, rm, rv, training, momentum, eps):
    """torch.nn.functional.batch_norm in fp64 (it updates rm / rv in place).  One row in training mode, which it refuses, is written
    out with the same formulas: biased variance 0, so y = bias, and the unbiased factor n / max(n - 1, 1) = 1 of batch_norm_traced"""
    if training and x.size(0) == 1:
        mean, var = x[0], torch.zeros_like(x[0])
        y = (x - mean) * torch.rsqrt(var + eps)
        if rm is not None:
            rm.mul_(1 - momentum).add_(mean.detach(), alpha=momentum)
            rv.mul_(1 - momentum).add_(var.detach(), alpha=momentum)
        return (y if w is None else y * w) + (0.0 if b is None else b)
    return F.batch_norm(x, rm, rv, w, b, training, momentum, eps)


def _bn_noise(x, gy, w, training, eps):
    """(noise of y, of d/dx, of d/dweight): what fp32 rounding alone leaves in a training-mode batch norm, to first order, from the
    fp64 operands -- the ``noise`` helpers.assert_close takes for cancelling fp32 sums.  Negligible beside TOL at a thousand rows;
    at one or two rows rstd reaches eps^-1/2 = 316 and multiplies the rounding of the cancelling differences.
      xhat = (x - mean) rstd: the subtraction cancels, |d xhat| <= eps32 (|x| + |mean|) rstd =: A;  rstd = (var + eps)^-1/2 with
      var = E[x^2] - mean^2 cancelling too: |d rstd| / rstd <= eps32 (E[x^2] + mean^2) / 2 (var + eps) =: B;  |d xhat| <= A + |xhat| B
      y = w xhat + b:                         |w| |d xhat|
      d/dweight = sum_n gy xhat:              sum_n |gy| |d xhat|
      d/dx = rstd w (gy - mean(gy) - xhat m), m = mean(gy xhat): each of the three terms went through up to four roundings
              (4 eps32 x their magnitudes), plus |d xhat| |m| + |xhat| |d m| + |gy - mean(gy) - xhat m| B"""
    if not training:
        return 0.0, 0.0, 0.0
    mean, var = x.mean(0), x.var(0, unbiased=False)
    rstd = torch.rsqrt(var + eps)
    xhat = (x - mean) * rstd
    wa = torch.ones_like(mean) if w is None else w.abs()
    B = EPS32 * 0.5 * ((x * x).mean(0) + mean * mean) / (var + eps)
    dxhat = EPS32 * (x.abs() + mean.abs()) * rstd + xhat.abs() * B
    m, dm = (gy * xhat).mean(0), (gy.abs() * dxhat).mean(0)
    core = gy - gy.mean(0) - xhat * m
    terms = gy.abs() + gy.mean(0).abs() + xhat.abs() * m.abs()
    gx = rstd * wa * (4.0 * EPS32 * terms + dxhat * m.abs() + xhat.abs() * dm + core.abs() * B)
    return float((wa * dxhat).max()), float(gx.max()), float((gy.abs() * dxhat).sum(0).max())


@pytest.mark.parametrize("n", [1, 2, 1037])
@pytest.mark.parametrize("f", [17, 64])
@pytest.mark.parametrize("mode", ["train", "train-plain", "train-norunning", "train-plain-norunning", "eval", "eval-plain"])
def test_batch_norm_op_formula_and_running_statistics_vs_fp64(mode, f, n):
    training, affine, running = mode.startswith("train"), "plain" not in mode, "norunning" not in mode
    gen = _gen(100 * n + f + len(mode))
    x = 0.7 * torch.randn(n, f, generator=gen) * (0.5 + torch.rand(f, generator=gen)) + torch.randn(f, generator=gen)
    gy = torch.randn(n, f, generator=gen)
    w, b = (1.0 + 0.3 * torch.randn(f, generator=gen), 0.3 * torch.randn(f, generator=gen)) if affine else (None, None)
    rm, rv = (0.3 * torch.randn(f, generator=gen), 0.5 + torch.rand(f, generator=gen)) if running else (None, None)
    x64, w64, b64 = x.double().requires_grad_(True), None if w is None else w.double().requires_grad_(True), None if b is None else b.double().requires_grad_(True)
    rm64, rv64 = _d(rm), _d(rv)
    want = _bn64(x64, w64, b64, rm64, rv64, training, BN_MOMENTUM, BN_EPS)
    want.backward(gy.double())
    xd, wd, bd, rmd, rvd = _dev(x, True), _dev(w, True), _dev(b, True), _dev(rm), _dev(rv)
    got = library.batch_norm_traced(xd, wd, bd, rmd, rvd, training, BN_MOMENTUM, BN_EPS)
    got.backward(gy.to(DEV))
    what = f"kagnn::batch_norm {mode} [{n}, {f}]: "
    noise_y, noise_gx, noise_gw = _bn_noise(x.double(), gy.double(), _d(w), training, BN_EPS)
    assert_close(got, want, what=what + "y", noise=noise_y)
    assert_close(xd.grad, x64.grad, what=what + "d/dx", noise=noise_gx)
    if affine:
        assert_close(wd.grad, w64.grad, what=what + "d/dweight", noise=noise_gw)
        assert_close(bd.grad, b64.grad, what=what + "d/dbias")
    if running:
        assert_close(rmd, rm64, what=what + "running_mean")
        assert_close(rvd, rv64, what=what + "running_var")
        if not training:
            assert torch.equal(rmd.cpu(), rm) and torch.equal(rvd.cpu(), rv), "eval mode only reads the running statistics"


def test_batch_norm_running_var_of_a_near_constant_column():
    """batch_norm_traced rebuilds the batch variance as 1 / rstd^2 - eps.  Where var << eps that difference cancels: its absolute
    error is that of 1 / rstd^2, a number of size eps.  In units of eps32 = 2^-23 relative to eps: fl(var + eps) 0.5; the reciprocal
    square root halves that and adds its own <= 1 (1.25); squaring doubles and rounds (3); the reciprocal <= 1 (4); the subtraction of
    the same fp32 eps is exact (Sterbenz) and the factor n / (n - 1) rounds a number 1000x smaller.  4, doubled for the headroom
    between a unit in the last place and eps32 of the two device approximations: C = 8, absolute bound 8 eps eps32 = 9.5e-12.
    Momentum 1 so that running_var IS the rebuilt variance (at momentum 0.1 the rounding of 0.9 running_var, ~6e-8, would hide it)."""
    n, f, col = 1037, 17, 3
    gen = _gen(5)
    x = 0.7 * torch.randn(n, f, generator=gen) + torch.randn(f, generator=gen)
    x[:, col] = 0.5 + 1e-4 * torch.randn(n, generator=gen)
    var64 = x.double().var(0, unbiased=True)
    assert float(var64[col]) < 1e-3 * BN_EPS
    rm, rv = torch.zeros(f, device=DEV), torch.ones(f, device=DEV)
    y = library.batch_norm_traced(x.to(DEV), None, None, rm, rv, True, 1.0, BN_EPS)
    assert_close(y, F.batch_norm(x.double(), None, None, None, None, True, 0.0, BN_EPS), what="near-constant column: y")
    err = abs(float(rv[col]) - float(var64[col]))
    print(f"near-constant column: running_var {float(rv[col]):.6e} vs {float(var64[col]):.6e}, error {err:.3e} = {err / (BN_EPS * EPS32):.2f} eps eps32")
    assert err <= 8.0 * BN_EPS * EPS32, err
    others = [c for c in range(f) if c != col]
    assert_close(rv[others], var64[others], what="near-constant column: running_var of the other columns")
    assert_close(rm, x.double().mean(0), what="near-constant column: running_mean")


# ================================================================================================ A. kagnn::segment_pool / segment_broadcast
SEGMENTS = {"ragged": [5, 5, 40, 40, 700, 703, 990], "one": [0, 1000], "one-row-each": [10, 11, 12, 13]}


def _pool64(x, seg, mean):
    rows = []
    for lo, hi in zip(seg[:-1], seg[1:]):
        s = x[lo:hi].sum(0)
        rows.append(s / max(hi - lo, 1) if mean else s)
    return torch.stack(rows)


@pytest.mark.parametrize("f", [17, 64])
@pytest.mark.parametrize("mean", [False, True], ids=["sum", "mean"])
@pytest.mark.parametrize("name", list(SEGMENTS))
def test_segment_pool_op_and_broadcast_vs_fp64(name, mean, f):
    """empty segments, rows before the first and after the last segment (gradient exactly 0), one segment holding everything"""
    seg, n = SEGMENTS[name], 1000
    gen = _gen(len(name) + f)
    x, gout = torch.randn(n, f, generator=gen), torch.randn(len(seg) - 1, f, generator=gen)
    x64 = x.double().requires_grad_(True)
    want = _pool64(x64, seg, mean)
    want.backward(gout.double())
    xd, ptr = _dev(x, True), torch.tensor(seg, dtype=torch.int32, device=DEV)
    got = library.segment_pool(xd, ptr, mean)
    got.backward(gout.to(DEV))
    what = f"kagnn::segment_pool {name} mean={mean} F={f}: "
    assert_close(got, want, what=what + "out")
    assert_close(xd.grad, x64.grad, what=what + "d/dx")
    outside = torch.ones(n, dtype=torch.bool)
    outside[seg[0]:seg[-1]] = False
    assert bool((xd.grad.cpu()[outside] == 0).all())
    assert torch.equal(library.segment_broadcast(gout.to(DEV), ptr, n, mean), xd.grad)


# ================================================================================================ B. torch.library.opcheck
def _opcheck_inputs(graph):
    """one representative input set per op, from part A"""
    n, fin, fout, G, k = 129, 33, 17, 4, 3
    x, gy, p = _kan_case(n, fin, fout, G, k, 1)
    xd, gyd = _dev(x, True), gy.to(DEV)
    bw, sw, sc = (_dev(p[nm], True) for nm in KAN_NAMES)
    knots = p["grid"][0].contiguous().to(DEV)
    with torch.no_grad():
        pack = torch.ops.kagnn.kan_linear(xd, bw, sw, sc, knots, G, k, PREC_SPLIT)[1]
    ng = 8
    gen = _gen(2)
    centers, den = torch.linspace(-2.0, 2.0, ng).to(DEV), 4.0 / (ng - 1)
    lw, lb = _dev(1.0 + 0.3 * torch.randn(fin, generator=gen), True), _dev(0.3 * torch.randn(fin, generator=gen), True)
    fsw, fbw, fbb = (_dev(t, True) for t in (0.1 * torch.randn(fout, fin * ng, generator=gen), 0.3 * torch.randn(fout, fin, generator=gen), 0.3 * torch.randn(fout, generator=gen)))
    with torch.no_grad():
        stats = torch.ops.kagnn.fastkan_layer(xd, lw, lb, fsw, fbw, fbb, centers, den, 1e-5, PREC_SPLIT)[1]
    g = graph.g
    c = _agg_operands(graph, 16, "all", 3)
    ax, agout, aw = c.x.to(DEV), c.gout.to(DEV), c.w.to(DEV)[g.perm.long()].contiguous()
    s_in, s_out, ab = c.s_in.to(DEV), c.s_out.to(DEV), c.b.to(DEV)
    bx = _dev(torch.randn(n, fout, generator=gen), True)
    w1, b1 = _dev(1.0 + 0.3 * torch.randn(fout, generator=gen), True), _dev(0.3 * torch.randn(fout, generator=gen), True)
    rm, rv = torch.zeros(fout, device=DEV), torch.ones(fout, device=DEV)
    with torch.no_grad():
        _, mean, rstd = torch.ops.kagnn.batch_norm(bx, w1, b1, rm, rv, True, BN_EPS)
    ptr = torch.tensor([5, 5, 40, 100, n - 3], dtype=torch.int32, device=DEV)
    d = lambda t: t.detach()
    return {
        "aggregate_sum": (d(ax), g.rowptr, g.col, aw, s_in, s_out, ab, g.hub_seg, g.num_hub_seg, g.hub_threshold, 1.5, True),
        "aggregate_edge_grad": (d(ax), agout, g.rowptr, g.col, g.perm, s_in, s_out, g.hub_seg, g.num_hub_seg, g.hub_threshold, g.num_edges, True),
        "kan_linear": (xd, bw, sw, sc, knots, G, k, PREC_SPLIT),
        "kan_linear_bwd_input": (d(xd), gyd, knots, pack, fout, G, k, PREC_SPLIT),
        "kan_linear_bwd_weight": (d(xd), gyd, knots, d(sw), d(sc), G, k, PREC_SPLIT, True),
        "fastkan_layer": (xd, lw, lb, fsw, fbw, fbb, centers, den, 1e-5, PREC_SPLIT),
        "fastkan_layer_bwd": (d(xd), gyd, d(lw), d(lb), d(fsw), d(fbw), centers, stats, den, 1e-5, PREC_SPLIT),
        "batch_norm": (bx, w1, b1, rm, rv, True, BN_EPS),
        "batch_norm_bwd": (d(bx), gyd, d(w1), mean, rstd, True, True),
        "segment_pool": (_dev(x, True), ptr, True),
        "segment_broadcast": (torch.randn(4, fin, generator=gen).to(DEV), ptr, n, True)}


OPS = ("aggregate_sum", "aggregate_edge_grad", "kan_linear", "kan_linear_bwd_input", "kan_linear_bwd_weight", "fastkan_layer",
       "fastkan_layer_bwd", "batch_norm", "batch_norm_bwd", "segment_pool", "segment_broadcast")
_OPCHECK_INPUTS = {}


@pytest.mark.parametrize("name", OPS)
def test_opcheck(graph, name):
    """schema (nothing mutates or aliases an argument), autograd registration, fake tensor (every register_fake promises the shape,
    dtype, device and strides of the real op) and aot dispatch with dynamic shapes: the default test_utils, none dropped.  Two runs of
    an op give the same bits except where a gradient is reduced through a workspace in an order the hardware picks; the tolerance
    handed to opcheck for those is TOL, relative and -- the operands being of order 1 -- absolute.  kagnn::kan_linear's second
    output is an opaque uint8 pack with padding bytes the pack kernel skips (247 of 55 552 differed between two runs here): the op
    zeroes the buffer first (``_kan_fwd_raw(zero_pack=True)``, the traced route only), so the pack is compared like every other
    output and no sub-check is dropped."""
    if not hasattr(torch.ops.kagnn, name):
        pytest.fail(f"kagnn::{name} is not registered")
    if not _OPCHECK_INPUTS:
        _OPCHECK_INPUTS.update(_opcheck_inputs(graph))
    torch.library.opcheck(getattr(torch.ops.kagnn, name).default, _OPCHECK_INPUTS[name], atol=TOL, rtol=TOL)


# ================================================================================================ C. compiled modules
def _compile(module):
    """torch.compile(backend=aot_eager, fullgraph=True) through a backend that first notes the call_function targets of the graph
    dynamo hands over (the spy of test_models_trace_into_one_graph_of_kagnn_ops, without tracing twice); -> (compiled, targets)"""
    import torch._dynamo
    from torch._dynamo.backends.registry import lookup_backend
    torch._dynamo.reset()
    seen = []

    def backend(gm, example_inputs):
        for sub in gm.modules():                      # (a traced autograd.Function keeps its ops in sub-graphs)
            if isinstance(sub, torch.fx.GraphModule):
                seen.extend(str(nd.target) for nd in sub.graph.nodes if nd.op == "call_function")
        return lookup_backend("aot_eager")(gm, example_inputs)
    return torch.compile(module, backend=backend, fullgraph=True), seen


def _count(seen, op):
    """how many call_function nodes are kagnn::<op> (whichever way the target prints: kagnn.op.default, kagnn::op)"""
    return sum(1 for t in seen if "kagnn" in t and op in re.split(r"[.:]+", t))


def _trained_like(layer, seed):
    """parameters of the size part A uses in place of the constructor's (its spline coefficients are noise of 1e-2)"""
    gen = _gen(seed)
    with torch.no_grad():
        layer.base_weight.copy_(0.3 * torch.randn(layer.base_weight.shape, generator=gen))
        layer.spline_weight.copy_(0.3 * torch.randn(layer.spline_weight.shape, generator=gen))
        layer.spline_scaler.copy_(1.0 + 0.5 * torch.randn(layer.spline_scaler.shape, generator=gen))
    return layer


def _layer_state(layer):
    return {k: v.detach().cpu().clone() for k, v in layer.state_dict().items()}


def _check_compiled_kanlinear(layer, x, gy, what, count=1, state=None):
    """compile the layer as it stands -- no eager forward first -- and hold y and every gradient to the oracle on ``state`` (default:
    the state the layer holds)"""
    p = _layer_state(layer) if state is None else state
    want = _kan_oracle(x, gy, p, layer.spline_order)
    compiled, seen = _compile(layer)
    layer.zero_grad()
    xd = _dev(x, True)
    y = compiled(xd)
    y.backward(gy.to(DEV))
    assert _count(seen, "kan_linear") == count, seen
    assert_close(y, want["y"], what=what + ": y")
    assert_close(xd.grad, want["x"], what=what + ": d/dx")
    for nm in KAN_NAMES:
        assert_close(getattr(layer, nm).grad, want[nm], what=f"{what}: {nm}")
    return p


@pytest.fixture(scope="module")
def grid_case():
    """the batch of test_update_grid_vs_oracle: every column with its own spread and centre"""
    gen = _gen(41)
    x = torch.randn(1037, 33, generator=gen) * torch.linspace(0.3, 2.0, 33) + torch.linspace(-1, 1, 33)
    return SimpleNamespace(x=x, gy=torch.randn(1037, 17, generator=gen))


def _fresh_layer(seed=42, trained=True):
    torch.manual_seed(seed)
    layer = kagnn_amd.KANLinear(33, 17, grid_size=5)
    return (_trained_like(layer, seed) if trained else layer).to(DEV)


def test_compiled_kanlinear_right_after_update_grid(grid_case):
    """update_grid, then the compiled call, no eager forward in between: y and every gradient against oracle.update_grid (its fit
    solved in fp64) plus the oracle's forward, at TOL; knots (5e-7) and refitted coefficients (5e-5) as test_update_grid_vs_oracle
    holds them, on that test's kind of layer (the constructor's parameters) and batch."""
    layer = _fresh_layer(trained=False)
    p = _layer_state(layer)
    layer.update_grid(grid_case.x.to(DEV))
    p["grid"], p["spline_weight"] = orc.update_grid(grid_case.x, p, 5, 3, solve_dtype=torch.float64)
    assert_close(layer.grid, p["grid"], 5e-7, what="update_grid: knots")
    assert_close(layer.spline_weight, p["spline_weight"], 5e-5, what="update_grid: coefficients")
    assert not torch.equal(layer.grid[0], layer.grid[1])
    _check_compiled_kanlinear(layer, grid_case.x, grid_case.gy, "compiled KANLinear after update_grid", state=p)


def test_compiled_kanlinear_right_after_adaptive_refine(grid_case):
    layer = _fresh_layer()
    before = _layer_state(layer)
    layer.refine(grid_case.x.to(DEV), 10, adaptive=True)
    grid64, _ = orc.update_grid(grid_case.x, before, 10, 3, solve_dtype=torch.float64)       # (the same quantile knots at the new size)
    assert layer.grid.shape == (33, 17) and layer.spline_weight.shape == (17, 33, 13)
    assert_close(layer.grid, grid64, 5e-7, what="refine(adaptive): knots")
    _check_compiled_kanlinear(layer, grid_case.x, grid_case.gy, "compiled KANLinear after refine(adaptive=True)")


def test_compiled_kanlinear_right_after_loading_per_feature_rows(grid_case):
    layer = _fresh_layer()
    state = _layer_state(layer)
    state["grid"] = _jittered(state["grid"], 5)
    layer.load_state_dict(state)
    p = _check_compiled_kanlinear(layer, grid_case.x, grid_case.gy, "compiled KANLinear after load_state_dict")
    assert torch.equal(p["grid"], state["grid"])


def test_compiled_layers_with_more_than_16_coefficients_or_centres():
    """grid_size 16 at order 3 is 19 coefficients, 20 centres are 20: two groups each on the split kernels, every group one opaque op"""
    gen = _gen(43)
    x, gy = 0.8 * torch.randn(300, 20, generator=gen), torch.randn(300, 10, generator=gen)
    torch.manual_seed(44)
    layer = _trained_like(kagnn_amd.KANLinear(20, 10, grid_size=16), 44).to(DEV)
    layer.precision = PREC_SPLIT
    _check_compiled_kanlinear(layer, x, gy, "compiled KANLinear, 19 coefficients", count=2)
    fk = kagnn_amd.FastKANLayer(20, 10, num_grids=20).to(DEV)
    fk.precision = PREC_SPLIT
    with torch.no_grad():
        fk.layernorm.weight.add_(0.3 * torch.randn(20, generator=gen).to(DEV))
        fk.layernorm.bias.add_(0.3 * torch.randn(20, generator=gen).to(DEV))
        fk.base_linear.bias.add_(0.3 * torch.randn(10, generator=gen).to(DEV))
    p64 = {k: v.detach().cpu().double().requires_grad_(v.requires_grad) for k, v in fk.named_parameters()}
    xr = x.double().requires_grad_(True)
    want = orc.fastkan_forward(xr, [p64])
    want.backward(gy.double())
    compiled, seen = _compile(fk)
    xd = _dev(x, True)
    y = compiled(xd)
    y.backward(gy.to(DEV))
    assert _count(seen, "fastkan_layer") == 2, seen
    assert_close(y, want, what="compiled FastKANLayer, 20 centres: y")
    assert_close(xd.grad, xr.grad, what="compiled FastKANLayer, 20 centres: d/dx")
    for name, prm in fk.named_parameters():
        if prm.requires_grad:
            assert_close(prm.grad, p64[name].grad, what=f"compiled FastKANLayer, 20 centres: {name}")


class _masked_gcn_oracle:
    """inside the block ``oracle.gcn_conv`` multiplies the message of original edge e by ``mask[e]`` (kagnn_amd.edge_mask's
    semantics, as in tests/test_gpu_edge_weights.py): the normalisation is ``oracle.gcn_norm`` of the unmasked graph, the added
    self loops are not masked, self loops of the edge list are dropped"""

    def __init__(self, mask):
        self.mask = mask

    def __enter__(self):
        self._orig = orc.gcn_conv
        mask = self.mask

        def gcn_conv(x, edge_index, lin_fn, bias):
            n = x.size(0)
            ei2, w2 = orc.gcn_norm(edge_index, n, x.dtype)
            keep = edge_index[0] != edge_index[1]
            out = orc.sum_aggregate(lin_fn(x), ei2, n, w2 * torch.cat([mask.to(x.dtype)[keep], torch.ones(n, dtype=x.dtype)]))
            return out if bias is None else out + bias
        orc.gcn_conv = gcn_conv
        return self

    def __exit__(self, *exc):
        orc.gcn_conv = self._orig
        return False


def _state64(model):
    return {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in model.state_dict().items()}


def _node_inputs(n, fin, classes, seed):
    gen = _gen(seed)
    return 0.5 * torch.randn(n, fin, generator=gen), torch.randn(n, classes, generator=gen) / n


def test_compiled_gcn_model_hands_the_edge_weights_their_gradient(graph):
    """a GKAN_Nodes takes edge weights as the mask of a kagnn_amd.edge_mask block: the compiled model inside the block, the mask
    requiring a gradient.  mask.grad against fp64 (oracle.gcn_norm in fp64 under autograd); None is the old silence"""
    fin, classes = 24, 5
    torch.manual_seed(45)
    model = kagnn_amd.GKAN_Nodes("gcn", 2, fin, 16, classes).to(DEV).train()
    x, gout = _node_inputs(graph.n, fin, classes, 46)
    mask = 0.2 + 0.8 * torch.rand(graph.e, generator=_gen(47))
    m64 = mask.double().requires_grad_(True)
    with _masked_gcn_oracle(m64):
        want = orc.node_model_forward(x.double(), graph.ei, _state64(model), "kan", "gcn", 2, 3)
    (want * gout.double()).sum().backward()
    compiled, seen = _compile(model)
    md = _dev(mask, True)
    with kagnn_amd.edge_mask(md):
        got = compiled(x.to(DEV), graph.g)
    (got * gout.to(DEV)).sum().backward()
    assert _count(seen, "aggregate_sum") and _count(seen, "kan_linear"), seen
    assert_close(got, want, MODEL_TOL, what="compiled masked GCN model: logits")
    assert md.grad is not None, "edge weights that require a gradient got none from the compiled model"
    assert_close(md.grad, m64.grad, MODEL_TOL, what="compiled masked GCN model: mask.grad")
    must_fail(torch.zeros_like(md.grad), m64.grad, MODEL_TOL, what="compiled masked GCN model: mask.grad zeroed")


def test_compiled_gin_models_order5_training_and_cubic_eval(graph):
    fin, classes = 24, 5
    x, gout = _node_inputs(graph.n, fin, classes, 48)
    # spline order 5, training mode: logits and every gradient
    torch.manual_seed(49)
    model = kagnn_amd.GKAN_Nodes("gin", 2, fin, 16, classes, grid_size=4, spline_order=5).to(DEV).train()
    state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    want, want_gx, wants = oracle_node_model_fwd_bwd(x, graph.ei, state, gout, "kan", "gin", 2, spline_order=5)
    compiled, seen = _compile(model)
    xd = _dev(x, True)
    got = compiled(xd, graph.g)
    got.backward(gout.to(DEV))
    assert _count(seen, "kan_linear") and _count(seen, "batch_norm") and _count(seen, "aggregate_sum"), seen
    assert_close(got, want, MODEL_TOL, what="compiled GIN order 5: logits")
    assert_close(xd.grad, want_gx, MODEL_TOL, what="compiled GIN order 5: d/dx")
    for name, prm in model.named_parameters():
        if prm.requires_grad:
            assert_close(prm.grad, wants[name], MODEL_TOL, what=f"compiled GIN order 5: {name}", noise=prenorm_bias_noise(name, wants))
    # eval mode: the running statistics are read, and are not the constructor's
    torch.manual_seed(50)
    model = kagnn_amd.GKAN_Nodes("gin", 2, fin, 16, classes, grid_size=4).to(DEV)
    with torch.no_grad():
        for bn in model.bns:
            bn.running_mean.normal_(std=0.3)
            bn.running_var.uniform_(0.5, 1.5)
            bn.weight.normal_(1.0, 0.3)
            bn.bias.normal_(std=0.3)
    model.eval()
    before = {k: v.clone() for k, v in model.state_dict().items() if "running" in k}
    want = orc.node_model_forward(x.double(), graph.ei, _state64(model), "kan", "gin", 2, 3, training=False)
    compiled, seen = _compile(model)
    got = compiled(x.to(DEV), graph.g)
    assert _count(seen, "kan_linear") and _count(seen, "batch_norm"), seen
    assert_close(got, want, MODEL_TOL, what="compiled GIN eval: logits")
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in before.items())
