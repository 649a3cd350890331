"""Per-edge activations of a KANLinear -- ``ops.kan_edge_abs_sum`` / ``ops.kan_edge_curves`` (csrc/kan_edge.hip), ``KANLinear.edge_l1`` /
``edge_curves`` / ``regularization_loss(x=)``, ``KAN.edge_l1`` / ``regularization_loss(x=)`` and ``kagnn_amd.collect_edge_l1`` -- against an
fp64 reference built here from ``oracle.kan_oracle.bspline_bases``:

    phi64[n, o, i] = einsum('nic,oic->noi', B, sw * sc) + silu(x)[:, None, :] * bw

Inputs: ``bw, sw ~ 0.3 randn``, ``sc ~ 1 + 0.5 randn``, ``x ~ 0.8 randn`` (part of x lies outside the grid's support; with the default
init phi ~ bw silu(x), which crowds the kink of |.| at 0).

Forward: ``helpers.assert_close`` at its default (2e-5 of the tensor's maximum, no allowance).

Gradients: |phi| has a kink and an fp32 evaluation may take the other side of it.  With tau = 2e-6 max|phi64| (the fp32 evaluation
error is ~1.4e-7 of that maximum: ~15x head-room) the fp64 gradient is formed WITHOUT the terms of the elements |phi64| < tau, and
each entry is allowed the fp32 bound plus the sum of the absolute values of its own removed terms.  At most 5 % of the (o, i) pairs,
and of the gx entries, may carry such an allowance: asserted, and the count is printed.
"""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import kagnn_amd
from kagnn_amd import ops
from oracle import kan_oracle as orc
from helpers import TOL, assert_close, must_fail, prenorm_bias_noise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(1, 1, 1, 1, 1), (67, 3, 2, 2, 1), (257, 33, 17, 4, 3), (1000, 64, 64, 5, 3), (513, 16, 70, 8, 2), (300, 5, 130, 32, 4)]
SHAPE_IDS = ["%dx%d-%d_G%dk%d" % s for s in SHAPES]
# the widest layers the argument checks accept (G + 2k + 1 = 48 knots): 46, 44 and 43 coefficients
LIMIT_SHAPES = [(130, 5, 70, 45, 1), (130, 6, 9, 41, 3), (130, 5, 70, 39, 4)]
LIMIT_IDS = ["%dx%d-%d_G%dk%d" % s for s in LIMIT_SHAPES]
TAU_REL = 2e-6
LOOSE_CAP = 0.05


# ---------------------------------------------------------------------------------- inputs and the fp64 reference
def make_case(n, fin, fout, G, k, seed=0, jitter=False, scaler=True, base=True):
    gen = torch.Generator().manual_seed(1000 * seed + 7 * n + fin + 3 * fout + G + k)
    knots = orc.make_knots(fin, G, k)
    if jitter:      # per-feature rows: every knot moved by less than 0.15 of the spacing (rows stay strictly increasing)
        knots = (knots + (2.0 / G) * 0.3 * (torch.rand(knots.shape, generator=gen) - 0.5)).contiguous()
    return SimpleNamespace(
        n=n, fin=fin, fout=fout, G=G, k=k,
        x=0.8 * torch.randn(n, fin, generator=gen),
        bw=0.3 * torch.randn(fout, fin, generator=gen) if base else None,
        sw=0.3 * torch.randn(fout, fin, G + k, generator=gen),
        sc=1.0 + 0.5 * torch.randn(fout, fin, generator=gen) if scaler else None,
        knots=knots, jitter=jitter)


def dev_knots(c):
    """what the ops take: one shared row (uniform) or the whole buffer (per-feature rows)"""
    return (c.knots if c.jitter else c.knots[0]).contiguous().to(DEV)


def dev_args(c):
    d = lambda t: None if t is None else t.to(DEV)
    return d(c.bw), d(c.sw), d(c.sc), dev_knots(c), c.G, c.k


def bases_and_derivatives(x, knots, k):
    """B[n, i, c] and dB/dx[n, i, c] in the dtype of x: dB_{j,k} = k (B_{j,k-1} / (t_{j+k} - t_j) - B_{j+1,k-1} / (t_{j+k+1} - t_{j+1}))"""
    B = orc.bspline_bases(x, knots, k)
    lower = orc.bspline_bases(x, knots, k - 1)                     # [n, i, C + 1]
    t = knots
    dB = k * (lower[:, :, :-1] / (t[:, k:-1] - t[:, :-(k + 1)]) - lower[:, :, 1:] / (t[:, k + 1:] - t[:, 1:-k]))
    return B, dB


def phi64(c, x=None):
    """-> phi [n, out, in], spl = sum_c sw B (unscaled) [n, out, in], B, dphi/dx -- all fp64"""
    x = (c.x if x is None else x).double()
    B, dB = bases_and_derivatives(x, c.knots.double(), c.k)
    sw = c.sw.double()
    w = sw if c.sc is None else sw * c.sc.double().unsqueeze(-1)
    phi = torch.einsum("nic,oic->noi", B, w)
    dphi = torch.einsum("nic,oic->noi", dB, w)
    spl = torch.einsum("nic,oic->noi", B, sw)
    if c.bw is not None:
        phi = phi + F.silu(x)[:, None, :] * c.bw.double()
        sg = torch.sigmoid(x)
        dphi = dphi + (sg * (1 + x * (1 - sg)))[:, None, :] * c.bw.double()
    return phi, spl, B, dphi


def grad_reference(c, gS):
    """fp64 gradients of sum(gS * S) with the terms of |phi| < tau removed, and per entry the sum of |removed terms|.
    -> {name: (gradient, allowance)}, share of loosened (o, i) pairs, share of loosened gx entries"""
    phi, spl, B, dphi = phi64(c)
    x = c.x.double()
    gS = gS.double().cpu()
    tau = TAU_REL * float(phi.abs().max())
    keep = phi.abs() >= tau
    s = torch.sign(phi) * keep
    drop = (~keep).double()
    out = {}
    if c.bw is not None:
        silu = F.silu(x)[:, None, :]
        out["bw"] = (gS * (s * silu).sum(0), gS.abs() * (drop * silu.abs()).sum(0))
    scale = torch.ones_like(gS) if c.sc is None else c.sc.double()
    out["sw"] = ((gS * scale).unsqueeze(-1) * torch.einsum("noi,nic->oic", s, B),
                 (gS * scale).abs().unsqueeze(-1) * torch.einsum("noi,nic->oic", drop, B.abs()))
    if c.sc is not None:
        out["sc"] = (gS * (s * spl).sum(0), gS.abs() * (drop * spl.abs()).sum(0))
    out["x"] = ((gS * s * dphi).sum(1), (gS.abs() * drop * dphi.abs()).sum(1))
    pairs = float((~keep).any(0).double().mean()) if phi.numel() else 0.0
    rows = float((~keep).any(1).double().mean()) if phi.numel() else 0.0
    return out, pairs, rows


def check_grad(got, want, allow, what):
    """every entry within the fp32 bound (2e-5 of the tensor's maximum) plus its own allowance"""
    got, want, allow = got.detach().double().cpu(), want.double(), allow.double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), what
    if not want.numel():
        return
    bound = TOL * float(want.abs().max()) + allow
    err = (got - want).abs()
    worst = float((err - allow).clamp(min=0).max()) / max(float(want.abs().max()), 1e-300)
    print(f"{what}: err/max {worst:.2e}, entries with an allowance {int((allow > 0).sum())}/{allow.numel()}")
    assert bool((err <= bound).all()), (what, float(err.max()), float(want.abs().max()), float(allow.max()))


def run_device(c, gS=None, x=None):
    """S and, with gS, the four gradients on the device"""
    bw, sw, sc, knots, G, k = dev_args(c)
    xd = (c.x if x is None else x).to(DEV).requires_grad_(gS is not None)
    leaves = [t.requires_grad_(gS is not None) for t in (bw, sw, sc) if t is not None]
    S = ops.kan_edge_abs_sum(xd, bw, sw, sc, knots, G, k)
    if gS is None:
        return S
    S.backward(gS.to(DEV))
    g = {"x": xd.grad, "sw": sw.grad}
    if bw is not None:
        g["bw"] = bw.grad
    if sc is not None:
        g["sc"] = sc.grad
    return S.detach(), g


_CASES = {}


def cached(shape, jitter):
    """one case, its fp64 reference and its device result per (shape, grid kind), shared by the tests below and left unchanged"""
    key = (shape, jitter)
    if key not in _CASES:
        c = make_case(*shape, jitter=jitter)
        gS = torch.randn(c.fout, c.fin, generator=torch.Generator().manual_seed(99))
        ref, pairs, rows = grad_reference(c, gS)
        S, g = run_device(c, gS)
        _CASES[key] = (c, gS, phi64(c)[0].abs().sum(0), ref, pairs, rows, S, g)
    return _CASES[key]


# ---------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("jitter", [False, True], ids=["uniform", "per-feature"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_abs_sum_matches_fp64(shape, jitter):
    c, gS, want, ref, pairs, rows, S, g = cached(shape, jitter)
    assert S.shape == (c.fout, c.fin) and S.dtype == torch.float32
    assert_close(S, want, what=f"abs sum {shape} jitter={jitter}")


@pytest.mark.parametrize("variant", ["no_scaler", "no_base", "column_slice"])
def test_abs_sum_optional_operands_and_strided_rows(variant):
    c = make_case(257, 33, 17, 4, 3, seed=2, scaler=variant != "no_scaler", base=variant != "no_base")
    if variant == "column_slice":
        wide = torch.randn(c.n, c.fin + 9, generator=torch.Generator().manual_seed(5)).to(DEV)
        wide[:, 4:4 + c.fin] = c.x.to(DEV)
        x = wide[:, 4:4 + c.fin]
        assert not x.is_contiguous()
        S = ops.kan_edge_abs_sum(x, *dev_args(c))
    else:
        S = run_device(c)
    assert_close(S, phi64(c)[0].abs().sum(0), what=f"abs sum {variant}")


def test_precision_setting_does_not_reach_the_edge_kernels():
    c = make_case(257, 33, 17, 4, 3, seed=3)
    layer = kagnn_amd.KANLinear(c.fin, c.fout, grid_size=c.G, spline_order=c.k).to(DEV)
    with torch.no_grad():
        layer.base_weight.copy_(c.bw); layer.spline_weight.copy_(c.sw); layer.spline_scaler.copy_(c.sc)
    x = c.x.to(DEV)
    res = []
    for mode in (None, ops.PREC_SPLIT, ops.PREC_HALF, ops.PREC_FP32):
        layer.precision = mode
        res.append((layer.edge_l1(x), layer.edge_curves(x)))
    for l1, curves in res[1:]:
        assert torch.equal(l1, res[0][0]) and torch.equal(curves, res[0][1])
    assert_close(res[0][0], phi64(c)[0].abs().mean(0), what="edge_l1")


# ---------------------------------------------------------------------------------- gradients
@pytest.mark.parametrize("jitter", [False, True], ids=["uniform", "per-feature"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_abs_sum_gradients_match_fp64(shape, jitter):
    c, gS, want, ref, pairs, rows, S, g = cached(shape, jitter)
    print(f"{shape} jitter={jitter}: loosened (o, i) pairs {pairs:.4f}, loosened gx entries {rows:.4f}")
    assert pairs <= LOOSE_CAP and rows <= LOOSE_CAP, (pairs, rows)
    assert set(g) == set(ref)
    for name, (grad, allow) in ref.items():
        check_grad(g[name], grad, allow, f"g_{name} {shape} jitter={jitter}")


@pytest.mark.parametrize("jitter", [False, True], ids=["uniform", "per-feature"])
@pytest.mark.parametrize("shape", LIMIT_SHAPES, ids=LIMIT_IDS)
def test_abs_sum_and_gradients_at_the_knot_limit(shape, jitter):
    """more than 39 coefficients: the parameter-gradient kernel's widest form (48 dense columns per lane)"""
    c, gS, want, ref, pairs, rows, S, g = cached(shape, jitter)
    assert c.G + 2 * c.k + 1 == 48
    assert_close(S, want, what=f"abs sum {shape} jitter={jitter}")
    print(f"{shape} jitter={jitter}: loosened (o, i) pairs {pairs:.4f}, loosened gx entries {rows:.4f}")
    assert pairs <= LOOSE_CAP and rows <= LOOSE_CAP, (pairs, rows)
    assert set(g) == set(ref)
    for name, (grad, allow) in ref.items():
        check_grad(g[name], grad, allow, f"g_{name} {shape} jitter={jitter}")
    S2, g2 = run_device(c, gS)
    assert torch.equal(S2, S)
    for name in g:
        assert torch.equal(g2[name], g[name]), name
    t = torch.cat([probe_points(c.knots[0])[:-1], c.x[:, 0]])
    if not jitter:
        assert_close(ops.kan_edge_curves(t.to(DEV), *dev_args(c)), phi64(c, t.unsqueeze(1).expand(-1, c.fin))[0], what=f"curves {shape}")


def test_gradient_check_rejects_mutants():
    """a zeroed g_spline_scaler and an abs sum that lost one row's contribution must not pass the checks above"""
    c, gS, want, ref, pairs, rows, S, g = cached(SHAPES[2], False)
    with pytest.raises(AssertionError):
        check_grad(torch.zeros_like(g["sc"]), ref["sc"][0], ref["sc"][1], "zeroed g_sc [mutant]")
    must_fail(S - phi64(c)[0][100].abs().float().to(DEV), want, what="abs sum without row 100")


# ---------------------------------------------------------------------------------- many slabs
@pytest.mark.parametrize("shape", [(70001, 3, 5, 5, 3), (8193, 64, 64, 5, 3)], ids=["70001x3-5", "8193x64-64"])
def test_many_slabs_strict_additive_and_rowwise_identical(shape):
    c = make_case(*shape, seed=4)
    gS = torch.randn(c.fout, c.fin, generator=torch.Generator().manual_seed(98))
    want = torch.zeros(c.fout, c.fin, dtype=torch.float64)
    for r0 in range(0, c.n, 4096):                                 # (the fp64 reference in pieces: [N, out, in] at once is 270 MB)
        want += phi64(c, c.x[r0:r0 + 4096])[0].abs().sum(0)
    S, g = run_device(c, gS)
    assert_close(S, want, what=f"abs sum {shape}")
    parts = [run_device(c, gS, c.x[r0:r0 + 1000]) for r0 in range(0, c.n, 1000)]
    # sums over a partition of the rows add, up to the order of summation (2e-6: the project's figure for it)
    assert_close(sum(p[0].double() for p in parts), S.double(), 2e-6, what="abs sum over row chunks", elementwise=False)
    for name in ("bw", "sw", "sc"):
        assert_close(sum(p[1][name].double() for p in parts), g[name].double(), 2e-6, what=f"g_{name} over row chunks", elementwise=False)
    # gx is per row: the same kernel takes the same sign decisions whatever rows surround it
    assert torch.equal(torch.cat([p[1]["x"] for p in parts]), g["x"])


# ---------------------------------------------------------------------------------- run to run
def test_two_runs_give_the_same_bits():
    for jitter in (False, True):
        c = make_case(8193, 20, 70, 5, 3, seed=5, jitter=jitter)
        gS = torch.randn(c.fout, c.fin, generator=torch.Generator().manual_seed(97))
        a, b = run_device(c, gS), run_device(c, gS)
        assert torch.equal(a[0], b[0])
        for name in a[1]:
            assert torch.equal(a[1][name], b[1][name]), name
        t = c.x[:500].to(DEV)
        assert torch.equal(ops.kan_edge_curves(t, *dev_args(c)), ops.kan_edge_curves(t, *dev_args(c)))


# ---------------------------------------------------------------------------------- special cases
def test_non_finite_rows_poison_exactly_their_column():
    c = make_case(300, 6, 70, 5, 3, seed=6)
    clean = run_device(c)
    x = c.x.clone()
    x[5, 2], x[70, 2], x[299, 2] = float("nan"), float("inf"), float("-inf")
    S = run_device(c, x=x)
    assert bool(torch.isnan(S[:, 2]).all())
    others = [i for i in range(c.fin) if i != 2]
    assert torch.equal(S[:, others], clean[:, others])
    for bad in (float("nan"), float("inf"), float("-inf")):
        x = c.x.clone()
        x[17, 4] = bad
        S = run_device(c, x=x)
        assert bool(torch.isnan(S[:, 4]).all()) and int(torch.isnan(S).sum()) == c.fout, bad


def test_zero_weights_give_zero_sum_and_zero_gradients():
    c = make_case(257, 9, 17, 4, 3, seed=7)
    c.bw, c.sw = torch.zeros_like(c.bw), torch.zeros_like(c.sw)
    S, g = run_device(c, torch.randn(c.fout, c.fin))
    assert not bool(S.any())
    for name, t in g.items():
        assert not bool(t.any()), name


def test_no_rows():
    c = make_case(0, 5, 7, 4, 3, seed=8)
    S, g = run_device(c, torch.randn(c.fout, c.fin))
    assert S.shape == (7, 5) and not bool(S.any())
    assert g["x"].shape == (0, 5)
    for name in ("bw", "sw", "sc"):
        assert g[name].shape == getattr(c, name).shape and not bool(g[name].any()), name
    assert ops.kan_edge_curves(torch.empty(0, device=DEV), *dev_args(c)).shape == (0, 7, 5)


def test_output_with_a_leading_dimension_is_written_inside_its_block_only():
    c = make_case(300, 5, 70, 5, 3, seed=9)
    bw, sw, sc, knots, G, k = dev_args(c)
    buf = torch.full((c.fout + 2, c.fin + 3), -777.0, device=DEV)
    ops._kan_edge_abs_sum_raw(c.x.to(DEV), bw, sw, sc, knots, 0, c.fin, c.fout, G, k, out=buf[1:1 + c.fout, 2:2 + c.fin])
    assert torch.equal(buf[1:1 + c.fout, 2:2 + c.fin], run_device(c))
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[1:1 + c.fout, 2:2 + c.fin] = False
    assert bool((buf[mask] == -777.0).all())


# ---------------------------------------------------------------------------------- curves
def probe_points(row):
    """every knot, one ulp either side, the span midpoints, points beyond both ends, NaN (fp32 row of knots)"""
    inf = torch.tensor(float("inf"))
    h = row[1] - row[0]
    return torch.cat([row, torch.nextafter(row, inf), torch.nextafter(row, -inf), (row[1:] + row[:-1]) / 2,
                      torch.stack([row[0] - 3 * h, row[0] - 0.25 * h, row[-1] + 0.25 * h, row[-1] + 3 * h]), torch.tensor([float("nan")])])


@pytest.mark.parametrize("shape", [(3, 2, 2, 1), (33, 17, 4, 3), (16, 70, 8, 2), (5, 130, 32, 4)], ids=["3-2k1", "33-17k3", "16-70k2", "5-130k4"])
@pytest.mark.parametrize("form", ["shared-uniform", "per-feature"])
def test_curves_at_the_knot_probes(shape, form):
    c = make_case(1, *shape, seed=10, jitter=form == "per-feature")
    if form == "shared-uniform":
        t = probe_points(c.knots[0])
        tt = t.unsqueeze(1).expand(-1, c.fin)
    else:
        tt = torch.stack([probe_points(c.knots[i]) for i in range(c.fin)], dim=1).contiguous()
        t = tt
    got = ops.kan_edge_curves(t.to(DEV), *dev_args(c))
    want = phi64(c, tt)[0]
    assert got.shape == (tt.size(0), c.fout, c.fin)
    assert bool(torch.isnan(got[-1]).all())
    assert_close(got, want, what=f"curves {shape} {form}")


def test_curves_average_to_edge_l1():
    c = make_case(700, 16, 70, 8, 2, seed=11)
    layer = kagnn_amd.KANLinear(c.fin, c.fout, grid_size=c.G, spline_order=c.k).to(DEV)
    with torch.no_grad():
        layer.base_weight.copy_(c.bw); layer.spline_weight.copy_(c.sw); layer.spline_scaler.copy_(c.sc)
    x = c.x.to(DEV)
    curves = layer.edge_curves(x)
    assert_close(curves, phi64(c)[0], what="edge_curves")
    assert_close(layer.edge_l1(x), curves.double().abs().mean(0), what="edge_l1 vs the curves' mean")


# ---------------------------------------------------------------------------------- regulariser
def reg_formula(mag, a, e):
    total = mag.sum()
    p = mag / total
    return a * total - e * torch.sum(p * p.log())


def _load(layer, c):
    with torch.no_grad():
        layer.base_weight.copy_(c.bw); layer.spline_weight.copy_(c.sw); layer.spline_scaler.copy_(c.sc)
    return layer


def test_regularization_loss_on_activations_kanlinear():
    c = make_case(257, 33, 17, 4, 3, seed=12)
    layer = _load(kagnn_amd.KANLinear(c.fin, c.fout, grid_size=c.G, spline_order=c.k), c).to(DEV)
    a, e = 0.7, 1.3
    x = c.x.to(DEV).requires_grad_(True)
    loss = layer.regularization_loss(a, e, x=x)
    loss.backward()
    mag = (phi64(c)[0].abs().mean(0)).requires_grad_(True)
    want = reg_formula(mag, a, e)
    want.backward()
    assert_close(loss.reshape(1), want.detach().reshape(1), what="regulariser")
    ref, pairs, rows = grad_reference(c, mag.grad / c.n)           # d loss / d S = (d loss / d mag) / N
    assert pairs <= LOOSE_CAP and rows <= LOOSE_CAP, (pairs, rows)
    got = {"bw": layer.base_weight.grad, "sw": layer.spline_weight.grad, "sc": layer.spline_scaler.grad, "x": x.grad}
    for name, (grad, allow) in ref.items():
        check_grad(got[name], grad, allow, f"regulariser g_{name}")


def test_regularization_loss_without_rows_is_the_weight_stand_in_bit_for_bit():
    torch.manual_seed(3)
    layer = kagnn_amd.KANLinear(20, 7).to(DEV)
    mag = layer.spline_weight.abs().mean(-1)
    total = mag.sum()
    share = mag / total
    want = 1.0 * total - 1.0 * torch.sum(share * share.log())
    assert torch.equal(layer.regularization_loss(), want)
    chain = kagnn_amd.KAN([5, 6, 3]).to(DEV)
    assert torch.equal(chain.regularization_loss(0.5, 2.0), sum(l.regularization_loss(0.5, 2.0) for l in chain.layers))


def test_regularization_loss_on_activations_three_layer_chain():
    """fp64 through autograd, |.| replaced by phi * sign(phi) [|phi| >= tau] so that the removed terms are removed along the whole
    chain.  The case (64 rows, widths 5-6-4-3) is one where the fp64 reference removes nothing: no allowance anywhere."""
    widths, G, k, n = [5, 6, 4, 3], 5, 3, 64
    cs = [make_case(n, a, b, G, k, seed=20 + i) for i, (a, b) in enumerate(zip(widths[:-1], widths[1:]))]
    chain = kagnn_amd.KAN(widths, grid_size=G, spline_order=k)
    for layer, c in zip(chain.layers, cs):
        _load(layer, c)
    for layer in chain.layers:
        layer.precision = ops.PREC_FP32          # (the layers between the statistics in exact fp32: the bound below is the fp32 one)
    chain = chain.to(DEV)
    x = cs[0].x.to(DEV)
    loss = chain.regularization_loss(0.9, 1.1, x=x)
    loss.backward()
    l1 = chain.edge_l1(x)

    leaves, h, want, removed = [], cs[0].x.double(), 0.0, 0
    for c in cs:
        p = {name: getattr(c, name).double().requires_grad_(True) for name in ("bw", "sw", "sc")}
        leaves.append(p)
        B = orc.bspline_bases(h, c.knots.double(), k)
        phi = torch.einsum("nic,oic->noi", B, p["sw"] * p["sc"].unsqueeze(-1)) + F.silu(h)[:, None, :] * p["bw"]
        keep = phi.detach().abs() >= TAU_REL * float(phi.detach().abs().max())
        removed += int((~keep).sum())
        want = want + reg_formula((phi * (torch.sign(phi.detach()) * keep)).sum(0) / n, 0.9, 1.1)
        h = phi.sum(2)
    assert removed == 0, removed
    want.backward()
    assert_close(loss.reshape(1), want.detach().reshape(1), what="chain regulariser")
    for layer, p, stat, c in zip(chain.layers, leaves, l1, cs):
        assert stat.shape == (c.fout, c.fin)
        for name, t in (("bw", layer.base_weight), ("sw", layer.spline_weight), ("sc", layer.spline_scaler)):
            assert_close(t.grad, p[name].grad, what=f"chain regulariser g_{name} {c.fin}->{c.fout}")


def test_chain_walks_inside_a_block_do_not_record():
    torch.manual_seed(4)
    chain = kagnn_amd.KAN([5, 6, 3]).to(DEV)
    x = 0.8 * torch.randn(40, 5, device=DEV)
    with kagnn_amd.collect_edge_l1(chain) as stats:
        chain.regularization_loss(x=x)
        chain.edge_l1(x)
        assert stats == {}
        chain(x)
        assert set(stats) == {"layers.0", "layers.1"}
        assert_close(stats["layers.1"], chain.layers[1].edge_l1(chain.layers[0](x)), what="the chain's forward records")


# ---------------------------------------------------------------------------------- collection over a model
def _node_inputs(seed=0, n=300, e=2000, f=12):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, f, generator=gen).to(DEV), torch.randint(0, n, (2, e), generator=gen).to(DEV)


def _graph_batch(seed=0, B=16, integer=False, f=7):
    gen = torch.Generator().manual_seed(seed)
    sizes = torch.randint(9, 30, (B,), generator=gen)
    off = torch.cumsum(sizes, 0) - sizes
    src, dst, batch = [], [], []
    for b in range(B):
        nb = int(sizes[b]); eb = 2 * nb + 1
        src.append(torch.randint(0, nb, (eb,), generator=gen) + off[b]); dst.append(torch.randint(0, nb, (eb,), generator=gen) + off[b])
        batch.append(torch.full((nb,), b))
    n, e = int(sizes.sum()), sum(len(s) for s in src)
    d = SimpleNamespace(edge_index=torch.stack([torch.cat(src), torch.cat(dst)]).to(DEV), batch=torch.cat(batch).to(DEV), num_graphs=B)
    if integer:
        d.x = torch.randint(0, 21, (n, 1), generator=gen).to(DEV)
        d.edge_attr = torch.randint(0, 4, (e,), generator=gen).to(DEV)
    else:
        d.x = torch.randn(n, f, generator=gen).to(DEV)
    return d


def _models():
    out = {}
    for conv in ("gin", "gcn"):
        for skip in (True, False):
            def build(conv=conv, skip=skip):
                torch.manual_seed(11)
                m = kagnn_amd.GKAN_Nodes(conv, 2, 12, 16, 5, skip=skip, grid_size=5, spline_order=3, hidden_layers=2, dropout=0.0)
                x, ei = _node_inputs()
                return m.to(DEV).train(), (lambda mod: mod(x, ei))
            out[f"GKAN_Nodes-{conv}-skip{int(skip)}"] = build

    def kagin():
        torch.manual_seed(12)
        d = _graph_batch()
        return kagnn_amd.KAGIN(2, 7, 16, 3, 2, 4, 3, 0.0).to(DEV).train(), (lambda mod: mod(d))

    def kagin_regression():
        torch.manual_seed(13)
        H = 32
        d = _graph_batch(integer=True)
        m = kagnn_amd.KAGINRegression(1, 1, 3, H, 2, 4, 3, 1, 0.0, True)
        m.atom_encoder = kagnn_amd.graph_models.AtomEncoder(H, [21])
        m.bond_encoder.bond_embedding_list = torch.nn.ModuleList([torch.nn.Embedding(4, H)])
        return m.to(DEV).train(), (lambda mod: mod(d))
    out["KAGIN"], out["KAGINRegression"] = kagin, kagin_regression
    return out


MODELS = _models()
FUSED_ENTRY_POINTS = ("kagnn_gin_kan_layer_fwd", "kagnn_gin_kan_layer_fwd_affine", "kagnn_gine_kan_layer_fwd", "kagnn_gine_kan_stack_fwd",
                      "kagnn_kagin_model_fwd")


def _timed(fn):
    timer = ops.EntryPointTimer()
    ops.set_timer(timer)
    try:
        out = fn()
    finally:
        ops.set_timer(None)
    return out, [r[0] for r in timer.records]


@pytest.mark.parametrize("which", list(MODELS), ids=list(MODELS))
def test_collect_edge_l1_over_a_model(which):
    model, call = MODELS[which]()
    layers = {n: m for n, m in model.named_modules() if isinstance(m, kagnn_amd.KANLinear) and m.spline_order <= 4}
    assert layers
    outside, names_before = _timed(lambda: call(model))
    # the scalar whose gradients are compared inside against outside the block: the output under a fixed random upstream gradient, as
    # the A/B tests of the fused routes do (test_gpu_models.py: y.backward(gy)).  Not out.sum(): KAGIN ends in log_softmax, whose
    # row sums have the upstream gradient 1 - C softmax(z) -- it sums to zero over every row, so the parameter gradients are small
    # differences of large terms (max 0.07 here against terms of order 1) and rounding-level differences of the logits show at
    # 2.07e-5 of that small maximum (measured once, on kan.layers.0.spline_weight); the bound is for a gradient that is not a
    # cancelling sum
    upstream = torch.randn(outside.shape, generator=torch.Generator().manual_seed(31)).to(DEV)
    model.zero_grad()
    (outside * upstream).sum().backward()
    grads_outside = {n: p.grad.clone() for n, p in model.named_parameters()}
    fused_before = [n for n in names_before if n in FUSED_ENTRY_POINTS]
    assert fused_before or "gcn" in which, names_before           # the default route is a fused one (gcn: transform first, nothing fused)

    model.zero_grad()
    with kagnn_amd.collect_edge_l1(model) as stats:
        assert ops.layer_inputs_visible()
        inside, names_inside = _timed(lambda: call(model))
        assert set(stats) == set(layers), (sorted(stats), sorted(layers))
        assert not any(n in FUSED_ENTRY_POINTS for n in names_inside), names_inside
        (inside.sum() + sum(s.sum() for s in stats.values())).backward()
    assert not ops.layer_inputs_visible()
    assert_close(inside, outside, 2e-5, what=f"{which}: output inside the block vs outside", elementwise=False)
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    for name, layer in layers.items():
        assert stats[name].shape == (layer.out_features, layer.in_features)
        assert bool(layer.spline_weight.grad.any()), name

    # each statistic is edge_l1 of that layer on the input it saw: a second composed run with a forward pre-hook on every layer
    seen, hooks = {}, []
    for name, layer in layers.items():
        hooks.append(layer.register_forward_pre_hook(lambda mod, args, name=name: seen.__setitem__(name, args[0].detach().clone())))
    model.zero_grad()
    try:
        with kagnn_amd.collect_edge_l1(model):
            (call(model) * upstream).sum().backward()
    finally:
        for h in hooks:
            h.remove()
    assert set(seen) == set(layers)
    for name, layer in layers.items():
        assert_close(stats[name], layer.edge_l1(seen[name]), what=f"{which}: {name}")

    # the gradients of (out * upstream).sum() on the composed routes inside a block against the fused routes outside it, at the
    # tolerance the A/B switch of each route documents for gradients: 2e-5 of the tensor's maximum for the node models
    # (test_gpu_models.py: fused epilogue / norm backward on and off), 1e-4 for the graph-level models KAGIN and KAGINRegression
    # (README "fused forms of the graph-level model", test_gine_one_library_call_each_way_matches_the_composition,
    # tools/fuzz_graph_models.py: the fused and composed forms round the batch statistics differently).  Measured on KAGIN: 2.06e-5
    # on kan.layers.0.spline_scaler (maximum 0.0098).  A bias added right in front of a training-mode norm has a gradient that is
    # rounding noise on both sides (helpers.prenorm_bias_noise)
    tol = 1e-4 if which in ("KAGIN", "KAGINRegression") else 2e-5
    for name, p in model.named_parameters():
        assert_close(p.grad, grads_outside[name], tol, what=f"{which}: gradient of {name} inside vs outside", elementwise=False,
                     noise=prenorm_bias_noise(name, grads_outside))

    # after the block the fused routes are taken again, and give what they gave before
    again, names_after = _timed(lambda: call(model))
    assert [n for n in names_after if n in FUSED_ENTRY_POINTS] == fused_before, (names_after, names_before)
    assert torch.equal(again, outside)
