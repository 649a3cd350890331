"""KANLinear at spline orders 5..16 on the device (kan_high_order.hip): the dense basis table, the layer and its gradients, the
routing around the entry points that stay at orders 1..4, and whole models -- against the fp64 oracle.

Bounds.  Basis table: 2e-6 of the table's own maximum, the bound of ``test_adaptive_grid_layer_golden``.  Layer: ``assert_close``'s
default (2e-5 of the tensor's own maximum, 1e-4 relative on its large elements).  Whole models: 1e-4 of each tensor's own maximum,
the whole-model rule of ``tests/test_gpu_models.py``.  Every figure is printed before it is asserted."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import kagnn_amd
from kagnn_amd import harness, ops
from kagnn_amd._lib import PREC_FP32, PREC_HALF, PREC_SPLIT
from oracle import kan_oracle as orc
from helpers import assert_close, must_fail, oracle_kan_linear_fwd_bwd, prenorm_bias_noise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _jittered(in_features, g, k, seed):
    """the uniform grid plus uniform jitter of +-0.15 knot steps per knot and feature: strictly increasing (0.3 < 1 step)"""
    base = orc.make_knots(in_features, g, k)
    step = 2.0 / g
    grid = (base + (torch.rand(base.shape, generator=_gen(seed)) * 2.0 - 1.0) * 0.15 * step).contiguous()
    assert bool((grid[:, 1:] > grid[:, :-1]).all())
    return grid


# ------------------------------------------------------------------------------------------------ 1. the basis table
def _probe_points(grid):
    """per feature: every knot, every knot +-1 ulp, span midpoints, two points beyond each end, NaN and +-Inf -> [P, in]"""
    t = grid.t().contiguous()                                                   # [nknots, in]
    inf = torch.full_like(t[:1], float("inf"))
    h = (t[-1:] - t[:1]) / (t.size(0) - 1)
    rows = [t, torch.nextafter(t, inf.expand_as(t)), torch.nextafter(t, -inf.expand_as(t)), 0.5 * (t[1:] + t[:-1]),
            t[:1] - 0.5 * h, t[:1] - 3.0 * h, t[-1:] + 0.5 * h, t[-1:] + 3.0 * h,
            torch.full_like(t[:1], float("nan")), inf, -inf]
    return torch.cat(rows, dim=0).contiguous()


@pytest.mark.parametrize("per_feature", [False, True], ids=["uniform", "jittered"])
@pytest.mark.parametrize("g,k", [(5, 5), (1, 8), (3, 8), (2, 12), (1, 16), (16, 16)])
def test_basis_table_against_fp64(g, k, per_feature):
    fin = 5
    grid = _jittered(fin, g, k, 100 * g + k) if per_feature else orc.make_knots(fin, g, k)
    x = _probe_points(grid)
    want = orc.bspline_bases(x.double(), grid.double(), k)        # the fp32 knots cast to double: the half-open span tests agree exactly
    layer = kagnn_amd.KANLinear(fin, 2, grid_size=g, spline_order=k)
    layer.grid.copy_(grid)
    got = layer.to(DEV).b_splines(x.to(DEV)).cpu()
    assert got.shape == (x.size(0), fin, g + k)
    assert torch.equal(torch.isnan(got), torch.isnan(want)), "NaN pattern differs"
    assert bool(torch.isnan(got[-3:]).all()) and not bool(torch.isnan(got[:-3]).any())
    err, own = float((torch.nan_to_num(got.double()) - torch.nan_to_num(want)).abs().max()), float(torch.nan_to_num(want).abs().max())
    print(f"bases G={g} K={k} per_feature={per_feature}: max abs err {err:.3e}, {err / (2e-6 * own):.3f} of the bound")
    assert_close(got, want, tol=2e-6, what=f"bases.{g}.{k}.{int(per_feature)}")
    sums = torch.nan_to_num(got[: 4 * grid.size(1) - 1].double()).sum(-1)       # partition of unity inside [t_k, t_{G+k})
    inside = (x[: 4 * grid.size(1) - 1] >= grid[:, k]) & (x[: 4 * grid.size(1) - 1] < grid[:, g + k])
    assert float((sums[inside] - 1.0).abs().max()) <= 2e-6 * (g + k)


@pytest.mark.parametrize("g,k", [(5, 5), (1, 8), (3, 8), (2, 12), (1, 16), (16, 16)])
def test_uniform_path_span_search_on_the_knot_probes(g, k):
    """The basis table above always runs the per-feature evaluation (the entry point takes a grid matrix).  The shared-knot-row
    evaluation of the layer kernels has its own span search and half-open decision, so the same probes -- every knot, +-1 ulp,
    midpoints, beyond both ends, NaN, +-Inf -- go through the LAYER on the uniform grid: two input features, no base branch,
    unit scaler and one-hot spline weights (output f * C + c reads coefficient c of feature f), so y IS the basis table (same
    bound, 2e-6 of its maximum, against the oracle's layer in fp64: a non-finite x gives a NaN row on both sides), and gx under a
    random gy holds the derivative of every basis at those points at the layer bound."""
    fin, C = 2, g + k
    grid = orc.make_knots(fin, g, k)
    x = _probe_points(grid)
    p = {"base_weight": torch.zeros(fin * C, fin), "spline_weight": torch.zeros(fin * C, fin, C), "spline_scaler": torch.ones(fin * C, fin),
         "grid": grid}
    for f in range(fin):
        for c in range(C):
            p["spline_weight"][f * C + c, f, c] = 1.0
    gy = torch.randn(x.size(0), fin * C, generator=_gen(1000 + 17 * g + k))
    xr = x.double().requires_grad_(True)
    want = orc.kan_linear_forward(xr, p["base_weight"].double(), p["spline_weight"].double(), p["spline_scaler"].double(), grid.double(), k)
    want.backward(gy.double())
    table = orc.bspline_bases(x[:-3].double(), grid.double(), k).reshape(x.size(0) - 3, fin * C)
    assert float((want.detach()[:-3] - table).abs().max()) <= 1e-14          # the layer with these weights is the table
    layer = _layer((x.size(0), fin, fin * C, g, k), p)
    assert layer._knots().dim() == 1
    y, gx, _gp = _run(layer, x, gy)
    fy = assert_close(y, want.detach(), tol=2e-6, what=f"ho.probe.{g}.{k}.y") / 2e-6
    fg = assert_close(gx, xr.grad, what=f"ho.probe.{g}.{k}.gx") / 2e-5
    print(f"ho.probe G={g} K={k}: y {fy:.3f} of the table bound, gx {fg:.3f} of the layer bound")
    assert bool(torch.isnan(y[-3:]).all()) and not bool(torch.isnan(y[:-3]).any())


# ------------------------------------------------------------------------------------------------ 2. the layer
SHAPES = [(1, 1, 1, 1, 5), (33, 2, 33, 5, 5), (129, 33, 5, 3, 8), (257, 65, 129, 2, 9), (300, 20, 10, 16, 16), (257, 7, 5, 1, 16),
          (300, 20, 10, 2, 12), (1000, 64, 64, 8, 6), (70, 3, 2, 4, 7)]
_CASES: dict = {}


def _case(shape, per_feature, scaler=True):
    """inputs, parameters and the fp64 oracle's (y, gx, parameter gradients) of one layer case: computed once, shared, left unchanged"""
    key = (shape, per_feature, scaler)
    hit = _CASES.get(key)
    if hit is None:
        n, fin, fout, g, k = shape
        gen = _gen(sum(shape) * 7 + int(per_feature))
        grid = _jittered(fin, g, k, sum(shape)) if per_feature else orc.make_knots(fin, g, k)
        x = torch.randn(n, fin, generator=gen) * 0.6
        flat = x.view(-1)
        flat[0] = -1.0
        if flat.numel() > 1:
            flat[flat.numel() // 2] = 1.0
        if flat.numel() > 2:
            flat[-1] = float(grid.max()) + 0.25                                # outside the knot range
        p = {"base_weight": torch.randn(fout, fin, generator=gen) * 0.3, "spline_weight": torch.randn(fout, fin, g + k, generator=gen) * 0.3,
             "spline_scaler": torch.randn(fout, fin, generator=gen), "grid": grid}
        gy = torch.randn(n, fout, generator=gen)
        if scaler:
            want = oracle_kan_linear_fwd_bwd(x, gy, p, k)
        else:
            xr = x.double().requires_grad_(True)
            bw, sw = p["base_weight"].double().requires_grad_(True), p["spline_weight"].double().requires_grad_(True)
            y = orc.kan_linear_forward(xr, bw, sw, None, grid.double(), k)
            y.backward(gy.double())
            want = (y.detach(), xr.grad, {"base_weight": bw.grad, "spline_weight": sw.grad})
        hit = (x, gy, p, want)
        _CASES[key] = hit
    return hit


def _layer(shape, p, scaler=True, precision=None):
    _n, fin, fout, g, k = shape
    layer = kagnn_amd.KANLinear(fin, fout, grid_size=g, spline_order=k, enable_standalone_scale_spline=scaler)
    sd = {q: v.clone() for q, v in p.items() if scaler or q != "spline_scaler"}
    layer.load_state_dict(sd)
    layer.precision = precision
    return layer.to(DEV)


def _run(layer, x, gy):
    xd = x.to(DEV).requires_grad_(True)
    y = layer(xd)
    y.backward(gy.to(DEV))
    grads = {q: v.grad for q, v in layer.named_parameters()}
    return y.detach(), xd.grad, grads


def _check(tag, got, want):
    (y, gx, gp), (yw, gxw, gpw) = got, want
    worst = 0.0
    for name, a, b in [("y", y, yw), ("gx", gx, gxw)] + [(f"g_{q}", gp[q], gpw[q]) for q in gpw]:
        frac = assert_close(a, b, what=f"{tag}.{name}") / 2e-5
        print(f"{tag}.{name}: {frac:.3f} of the bound")
        worst = max(worst, frac)
    return worst


@pytest.mark.parametrize("per_feature", [False, True], ids=["uniform", "jittered"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layer_against_fp64(shape, per_feature):
    x, gy, p, want = _case(shape, per_feature)
    layer = _layer(shape, p)
    assert (layer._knots().dim() == 2) == per_feature
    _check(f"ho.{'x'.join(map(str, shape))}.{int(per_feature)}", _run(layer, x, gy), want)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layer_without_the_standalone_scale(shape):
    x, gy, p, want = _case(shape, False, scaler=False)
    layer = _layer(shape, p, scaler=False)
    assert not hasattr(layer, "spline_scaler")
    _check(f"ho.noscale.{'x'.join(map(str, shape))}", _run(layer, x, gy), want)


# ------------------------------------------------------------------------------------------------ 3. one path for every mode
@pytest.mark.parametrize("shape", [(129, 33, 5, 3, 8), (300, 20, 10, 16, 16)], ids=lambda s: "x".join(map(str, s)))
def test_every_precision_gives_the_same_bits(shape, monkeypatch):
    x, gy, p, _want = _case(shape, False)
    runs = [_run(_layer(shape, p, precision=mode), x, gy) for mode in (None, PREC_SPLIT, PREC_HALF, PREC_FP32, PREC_FP32)]
    monkeypatch.setenv("KAGNN_PRECISION", "half")
    runs.append(_run(_layer(shape, p), x, gy))
    for y, gx, gp in runs[1:]:
        assert torch.equal(y, runs[0][0]) and torch.equal(gx, runs[0][1])
        for q in gp:
            assert torch.equal(gp[q], runs[0][2][q]), q                          # (runs[3] and runs[4]: the same mode twice)


# ------------------------------------------------------------------------------------------------ 4. buffers
@pytest.mark.parametrize("per_feature", [False, True], ids=["uniform", "jittered"])
def test_strided_operands_and_a_wider_output_buffer(per_feature):
    shape = (129, 33, 5, 3, 8)
    n, fin, fout, g, k = shape
    x, gy, p, want = _case(shape, per_feature)
    layer = _layer(shape, p)
    xw = torch.full((n + 3, fin + 7), 9.0)
    xw[:n, 4:4 + fin] = x
    gw = torch.full((n + 3, fout + 5), 7.0)
    gw[:n, 2:2 + fout] = gy
    xs = xw.to(DEV)[:n, 4:4 + fin].requires_grad_(True)
    y = layer(xs)
    y.backward(gw.to(DEV)[:n, 2:2 + fout])
    assert_close(y, want[0], what="strided.y")
    assert_close(xs.grad, want[1], what="strided.gx")
    for q in want[2]:
        assert_close(dict(layer.named_parameters())[q].grad, want[2][q], what=f"strided.g_{q}")
    # the raw forward into a wider, sentinel-filled buffer: columns beyond `out` and rows beyond N stay as they were
    knots = layer._knots()
    mode = ops.PREC_FP32_GRID if per_feature else PREC_FP32
    bw, sw, sc = layer.base_weight.detach(), layer.spline_weight.detach(), layer.spline_scaler.detach()
    fb, db = ops._sizes("kagnn_kan_pack_bytes", fin, fout, g, k, mode, outputs=2)
    pf, pd = ops._ws(fb, DEV), ops._ws(db, DEV)
    ops._call("kagnn_kan_pack", ops._ptr(bw), ops._ptr(sw), ops._ptr(sc), fin, fout, g, k, mode, ops._ptr(pf), ops._ptr(pd), ops._stream())
    sentinel = -12345.5
    wide = torch.full((n + 4, fout + 6), sentinel, device=DEV)
    ops._call("kagnn_kan_linear_fwd", ops._ptr(xs.detach()), xw.size(1), n, ops._ptr(knots), fin, fout, g, k, mode, ops._ptr(pf),
              ops._ptr(wide), wide.size(1), None, 0, ops._stream())
    assert torch.equal(wide[:n, :fout], y.detach())
    assert bool((wide[:n, fout:] == sentinel).all()) and bool((wide[n:] == sentinel).all())
    gxw = torch.full((n + 4, fin + 6), sentinel, device=DEV)
    gyd = gw.to(DEV)
    ops._call("kagnn_kan_linear_bwd_input", ops._ptr(xs.detach()), xw.size(1), ops._ptr(gyd[:, 2:]), gw.size(1), n, ops._ptr(knots), fin,
              fout, g, k, mode, ops._ptr(pd), ops._ptr(gxw), gxw.size(1), 0, ops._stream())
    assert torch.equal(gxw[:n, :fin], xs.grad)
    assert bool((gxw[:n, fin:] == sentinel).all()) and bool((gxw[n:] == sentinel).all())
    gbw, gsw, gsc = ops._kan_bwd_weight_raw(xs.detach(), gyd[:n, 2:2 + fout], knots, sw.contiguous(), sc.contiguous(), fin, fout, g, k, mode, True)
    assert torch.equal(gbw, layer.base_weight.grad) and torch.equal(gsw, layer.spline_weight.grad) and torch.equal(gsc, layer.spline_scaler.grad)


@pytest.mark.parametrize("per_feature", [False, True], ids=["uniform", "jittered"])
def test_no_rows_make_no_launch(per_feature):
    """N = 0 through the C entry points: every buffer a kernel of these calls would write -- y, gx, the weight gradient's slab
    workspace -- is filled with a sentinel first and must keep it (x and gy are NULL, which the calls accept for no rows); the
    parameter gradients of no rows are zeros (a memset, not a launch).  Then the module on an empty input."""
    fin, fout, g, k = 6, 4, 3, 8
    layer = kagnn_amd.KANLinear(fin, fout, grid_size=g, spline_order=k)
    if per_feature:
        layer.grid.copy_(_jittered(fin, g, k, 77))
    layer = layer.to(DEV)
    knots = layer._knots()
    mode = ops.PREC_FP32_GRID if per_feature else PREC_FP32
    bw, sw, sc = layer.base_weight.detach(), layer.spline_weight.detach(), layer.spline_scaler.detach()
    fb, db = ops._sizes("kagnn_kan_pack_bytes", fin, fout, g, k, mode, outputs=2)
    pf, pd = ops._ws(fb, DEV), ops._ws(db, DEV)
    ops._call("kagnn_kan_pack", ops._ptr(bw), ops._ptr(sw), ops._ptr(sc), fin, fout, g, k, mode, ops._ptr(pf), ops._ptr(pd), ops._stream())
    sentinel = -12345.5
    y = torch.full((8, fout), sentinel, device=DEV)
    ops._call("kagnn_kan_linear_fwd", None, fin, 0, ops._ptr(knots), fin, fout, g, k, mode, ops._ptr(pf), ops._ptr(y), fout, None, 0, ops._stream())
    gx = torch.full((8, fin), sentinel, device=DEV)
    ops._call("kagnn_kan_linear_bwd_input", None, fin, None, fout, 0, ops._ptr(knots), fin, fout, g, k, mode, ops._ptr(pd), ops._ptr(gx), fin, 0,
              ops._stream())
    wb = ops._sizes("kagnn_kan_bwd_weight_workspace_bytes", 0, fin, fout, g, k, mode)
    ws = torch.full((wb // 4,), sentinel, device=DEV)
    gbw, gsw, gsc = (torch.full_like(t, sentinel) for t in (bw, sw, sc))
    ops._call("kagnn_kan_linear_bwd_weight", None, fin, None, fout, 0, ops._ptr(knots), fin, fout, g, k, mode, ops._ptr(sw), ops._ptr(sc),
              ops._ptr(gbw), ops._ptr(gsw), ops._ptr(gsc), ops._ptr(ws), wb, ops._stream())
    torch.cuda.synchronize()
    assert bool((y == sentinel).all()) and bool((gx == sentinel).all()) and bool((ws == sentinel).all())
    assert not bool(gbw.any()) and not bool(gsw.any()) and not bool(gsc.any())
    x = torch.zeros(0, fin, device=DEV, requires_grad=True)
    out = layer(x)
    assert out.shape == (0, fout)
    out.sum().backward()
    assert x.grad.shape == (0, fin)
    assert not bool(layer.spline_weight.grad.any()) and not bool(layer.base_weight.grad.any()) and not bool(layer.spline_scaler.grad.any())


# ------------------------------------------------------------------------------------------------ 5. mutation guards
def test_the_checks_can_fail():
    shape = (300, 20, 10, 16, 16)
    x, gy, p, want = _case(shape, False)
    y, _gx, gp = _run(_layer(shape, p), x, gy)
    assert_close(y, want[0], what="guard.y")
    bad = y.clone()
    bad[17] *= 1.0 + 1e-3
    must_fail(bad, want[0], what="guard.y")
    gsw = gp["spline_weight"]
    assert_close(gsw, want[2]["spline_weight"], what="guard.g_spline_weight")
    bad = gsw.clone()
    bad[:, :, 11] = 0.0
    must_fail(bad, want[2]["spline_weight"], what="guard.g_spline_weight")


# ------------------------------------------------------------------------------------------------ 6. refusals and routing
def test_update_grid_and_the_sharded_layer_refuse_order_8():
    layer = kagnn_amd.KANLinear(6, 4, grid_size=3, spline_order=8).to(DEV)
    with pytest.raises(NotImplementedError, match="ill-conditioned"):
        layer.update_grid(torch.randn(64, 6, device=DEV))
    from kagnn_amd.sharded import ShardedKANLinear
    with pytest.raises(ValueError, match="not supported"):
        ShardedKANLinear(layer, 0, 1)
    with pytest.raises(ValueError, match="out="):
        ops.kan_linear(torch.zeros(4, 6, device=DEV), layer.base_weight, layer.spline_weight, layer.spline_scaler, layer._knots(), 3, 8,
                       out=torch.empty(4, 4, device=DEV))


def _small_graph(n=200, e=800, seed=3):
    gen = _gen(seed)
    return torch.randint(0, n, (2, e), generator=gen)


def test_gin_convolution_takes_the_composed_path_to_the_bit():
    torch.manual_seed(4)
    conv = kagnn_amd.GIKANLayer(12, 16, 3, 8, 16, 2).to(DEV)
    ei = _small_graph().to(DEV)
    x = torch.randn(200, 12, generator=_gen(5)).to(DEV)
    timer = ops.EntryPointTimer()
    ops.set_timer(timer)
    try:
        xa = x.clone().requires_grad_(True)
        ya = conv(xa, ei)
        ya.sum().backward()
    finally:
        ops.set_timer(None)
    names = {r[0] for r in timer.records}
    assert not any(nm.startswith("kagnn_gin_kan_layer") for nm in names), names
    assert "kagnn_kan_linear_fwd" in names and "kagnn_kan_linear_bwd_weight" in names, names
    ga = [p.grad.clone() for p in conv.parameters()]
    conv.zero_grad()
    xb = x.clone().requires_grad_(True)
    g = ops.graph_index(ei, 200)
    yb = conv.nn(ops.aggregate_sum(xb, g, 1.0 + conv._eps()))
    yb.sum().backward()
    assert torch.equal(ya, yb) and torch.equal(xa.grad, xb.grad)
    for a, p in zip(ga, conv.parameters()):
        assert torch.equal(a, p.grad)


# ------------------------------------------------------------------------------------------------ 7. whole models
N_NODES, HID, G7, K7 = 200, 16, 3, 8


@pytest.mark.parametrize("skip", [True, False], ids=["skip", "noskip"])
@pytest.mark.parametrize("kind", ["gin", "gcn", "gat"])
def test_node_models_against_fp64(kind, skip):
    torch.manual_seed(11)
    model = kagnn_amd.GKAN_Nodes(kind, 2, 9, HID, 5, skip=skip, grid_size=G7, spline_order=K7, hidden_layers=2, dropout=0.0,
                                 **({"heads": 2} if kind == "gat" else {}))
    ei = _small_graph(seed=12)
    x = torch.randn(N_NODES, 9, generator=_gen(13)) * 0.5
    gout = torch.randn(N_NODES, 5, generator=_gen(14))
    state = {q: v.detach().clone() for q, v in model.state_dict().items()}
    frozen = ("grid", "eps", "running_mean", "running_var", "num_batches_tracked")
    st, leaves = {}, {}
    for q, v in state.items():
        v = v.double() if v.is_floating_point() else v
        if q.endswith(frozen):
            st[q] = v
        else:
            leaves[q] = v.clone().requires_grad_(True)
            st[q] = leaves[q]
    xr = x.double().requires_grad_(True)
    want = orc.node_model_forward(xr, ei, st, "kan", kind, 2, K7, skip=skip)
    want.backward(gout.double())
    g_want = {q: v.grad for q, v in leaves.items()}
    model = model.to(DEV).train()
    xd = x.to(DEV).requires_grad_(True)
    out = model(xd, ei.to(DEV))
    out.backward(gout.to(DEV))
    tag = f"ho.nodes.{kind}.{int(skip)}"
    worst = assert_close(out, want.detach(), 1e-4, what=f"{tag}.logits")
    worst = max(worst, assert_close(xd.grad, xr.grad, 1e-4, what=f"{tag}.gx"))
    checked = 0
    for name, p in model.named_parameters():
        # (convs.i.bias of the gcn / gat flavours sits in front of a training-mode BatchNorm1d: an identically zero gradient, held to
        # the noise floor helpers.prenorm_bias_noise states for exactly that name -- 1e-4 of the convolution's largest gradient)
        worst = max(worst, assert_close(p.grad, g_want[name], 1e-4, what=f"{tag}.grad.{name}", noise=prenorm_bias_noise(name, g_want)))
        checked += 1
    print(f"{tag}: worst {worst / 1e-4:.3f} of the bound over {checked} parameter gradients")
    assert checked >= 8


def _batch(seed, features=7, graphs=4):
    gen = _gen(seed)
    sizes = torch.tensor([50] * graphs)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)])
    per = 800 // graphs
    ei = torch.cat([torch.randint(0, 50, (2, per), generator=gen) + int(ptr[i]) for i in range(graphs)], dim=1)
    x = torch.randn(N_NODES, features, generator=gen) * 0.5
    batch = torch.repeat_interleave(torch.arange(graphs), sizes)
    return x, ei, batch, ptr


def _oracle_state(model):
    frozen = ("grid", "eps", "running_mean", "running_var", "num_batches_tracked")
    return {q: (v.detach().cpu().double().requires_grad_(True) if v.is_floating_point() and not q.endswith(frozen)
                else v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for q, v in model.state_dict().items()}


def _kagat_restated(x, ei, batch, st, layers, k):
    def one(prefix, h):
        return orc.kan_linear_forward(h, st[prefix + "base_weight"], st[prefix + "spline_weight"], st[prefix + "spline_scaler"],
                                      st[prefix + "grid"], k)
    h = x
    for l in range(layers):
        h = F.silu(orc.gat_conv(h, ei, lambda t: one(f"conv.{l}.lin.", t), st[f"conv.{l}.att_src"], st[f"conv.{l}.att_dst"],
                                st[f"conv.{l}.bias"], st[f"conv.{l}.att_src"].shape[1]))
    return F.log_softmax(one("readout.layers.0.", orc.global_add_pool(h, batch, 4)), dim=1)


@pytest.mark.parametrize("name", ["KAGIN", "KAGCN", "KAGAT", "KAGINRegression"])
def test_graph_level_models_against_fp64(name):
    torch.manual_seed(21)
    x, ei, batch, ptr = _batch(22)
    data = SimpleNamespace(edge_index=ei.to(DEV), batch=batch.to(DEV), ptr=ptr.to(DEV), num_graphs=4)
    if name == "KAGIN":
        model = kagnn_amd.KAGIN(2, 7, HID, 3, 2, G7, K7, 0.0)
        fwd = lambda st: orc.graph_classification_forward(x.double(), ei, batch, 4, st, "kan", "gin", 2, K7)
    elif name == "KAGCN":
        model = kagnn_amd.KAGCN(2, 7, HID, 3, G7, K7, 0.0)
        fwd = lambda st: orc.graph_classification_forward(x.double(), ei, batch, 4, st, "kan", "gcn", 2, K7)
    elif name == "KAGAT":
        model = kagnn_amd.KAGAT(2, 7, HID, 3, G7, K7, 0.0, 2)
        fwd = lambda st: _kagat_restated(x.double(), ei, batch, st, 2, K7)
    else:
        from kagnn_amd.graph_models import ATOM_FEATURE_DIMS, BOND_FEATURE_DIMS
        model = kagnn_amd.KAGINRegression(1, 1, 2, HID, 2, G7, K7, 1, 0.0, True)
        gen = _gen(23)
        x = torch.stack([torch.randint(0, d, (N_NODES,), generator=gen) for d in ATOM_FEATURE_DIMS], dim=1)
        ea = torch.stack([torch.randint(0, d, (ei.size(1),), generator=gen) for d in BOND_FEATURE_DIMS], dim=1)
        data.edge_attr = ea.to(DEV)
        fwd = lambda st: orc.graph_regression_forward(x, ei, ea, batch, 4, st, "kan", 2, K7)
    data.x = x.to(DEV)
    st = _oracle_state(model)
    want = fwd(st)
    gout = torch.randn(want.shape, generator=_gen(24))
    want.backward(gout.double())
    model = model.to(DEV).train()
    out = model(data)
    out.backward(gout.to(DEV))
    tag = f"ho.graph.{name}"
    worst = assert_close(out, want.detach(), 1e-4, what=f"{tag}.out")
    checked = 0
    for pname, p in model.named_parameters():
        assert p.grad is not None and st[pname].grad is not None, pname
        worst = max(worst, assert_close(p.grad, st[pname].grad, 1e-4, what=f"{tag}.grad.{pname}"))
        checked += 1
    print(f"{tag}: worst {worst / 1e-4:.3f} of the bound over {checked} parameter gradients")
    assert checked >= 8


def test_one_node_classification_step_and_graph_classification_run():
    torch.manual_seed(31)
    model = kagnn_amd.GKAN_Nodes("gin", 2, 9, HID, 5, skip=True, grid_size=G7, spline_order=K7, hidden_layers=2, dropout=0.0).to(DEV)
    ei = _small_graph(seed=32).to(DEV)
    x = (torch.randn(N_NODES, 9, generator=_gen(33)) * 0.5).to(DEV)
    y = torch.randint(0, 5, (N_NODES,), generator=_gen(34)).to(DEV)
    mask = torch.zeros(N_NODES, dtype=torch.bool)
    mask[:120] = True
    before = [p.detach().clone() for p in model.parameters()]
    harness.train_node_classification(model, x, ei, y, mask.to(DEV), (~mask).to(DEV), epochs=1)
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())

    from test_gpu_data import _tu
    d = _tu(G=8, seed=35)
    ds = kagnn_amd.DeviceGraphDataset(d.x, d.edge_index, d.node_ptr, y=d.y, device=DEV)
    gm = kagnn_amd.KAGIN(2, d.x.size(1), HID, int(d.y.max()) + 1, 2, G7, K7, 0.0).to(DEV)
    _t, losses = harness.train_graph_classification(gm, kagnn_amd.DeviceBatchLoader(ds, 4), nb_epochs=1)
    assert len(losses) == 1 and losses[0] == losses[0]
