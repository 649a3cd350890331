"""Per-edge activations of a FastKANLayer -- ``ops.fastkan_edge_abs_sum`` / ``ops.fastkan_edge_curves`` (csrc/fastkan_edge.hip),
``FastKANLayer.edge_l1`` / ``edge_curves`` / ``plot_curve`` / ``regularization_loss``, ``FastKAN.edge_l1`` / ``regularization_loss`` and
``kagnn_amd.collect_edge_l1`` over FastKAN models -- against an fp64 torch evaluation written here:

    u = LayerNorm(x) or x;   phi64[n, o, i] = sum_g sw[o, i*G+g] exp(-((u[n,i] - c_g) / h)^2) + bw[o, i] silu(x[n, i])

Inputs: ``x ~ 0.8 randn``, weights ``~ 0.3 randn``, ``gamma ~ 1 + 0.3 randn``, ``beta ~ 0.2 randn``, centres ``linspace(-2, 2, G)``.

Forward: ``helpers.assert_close`` at its default (2e-5 of the tensor's maximum, no allowance).

Gradients of x and the two weights: |phi| has a kink and an fp32 evaluation may take the other side of it.  With
tau = 2e-6 max|phi64| the fp64 gradient is formed by autograd WITHOUT the terms of the elements |phi64| < tau (|phi| is replaced by
phi * sign(phi) [|phi| >= tau]), and each entry is allowed the fp32 bound plus the sum of the absolute values of its own removed
terms.  Behind a LayerNorm a removed term of column j reaches every gx entry of its row, through the normalisation's Jacobian at about
1 / in of its size.  An allowance on all of them would leave whole rows loose (5.2 % of the gx entries at (1000, 64, 64, 8), 5.8 % at
(8193, 64, 64, 8): the share of rows with a removed term, in * out * P(|phi| < tau)), so the one thing the kink leaves open, a sign in
{-1, 0, +1} per removed element, is taken from the device: the signs that fit the row best are added to the fp64 reference and every
entry of the row is then held to the plain fp32 bound (``resolve_kinks``; the entries of a row share the few signs, which is stricter
than the allowance).  What counts as carrying an allowance there are the entries of the removed elements' own columns, whose terms
are the ones resolved that way (and every entry of a row with more than 6 removed elements, which keeps the allowance; none here).

The caps on the allowances are asserted in tests of their own: at most 5 % of the (o, i) pairs and 5 % of the gx entries on the
listed shapes (``test_allowance_shares_stay_under_the_cap``), at most 0.1 % of the gx entries over many slabs
(``test_many_slabs_gx_allowance_share``).  The fp64 reference alone gives at most 1.3 % of the pairs and 0.13 % of the gx entries on
the listed shapes, 0.092 % of the gx entries at (8193, 64, 64, 8).

Without the base branch phi underflows to 0, together with its derivative, wherever the argument leaves the centres' reach (a
LayerNorm output does: 10 % to 66 % of the pairs have such an element), so the run without it, at (257, 33, 17, 8), checks the forward
with and without LayerNorm, the gradients without LayerNorm, and the gradients behind a LayerNorm whose gamma and beta are 0.3 of
their usual size, so that its output stays within the centres' reach (``no_base_ln_near``).

Gradients of gamma and beta: signed sums over rows and outputs, held to ``max(fp32 bound, 4 x E32)``, E32 = the error of torch's own
fp32 CPU autograd of the same composed formula against the same fp64 gradient (the rule of tests/test_gpu_node_classification.py for
its loss sums).

Observed on MI355X (library version 270), worst fraction of each bound over the listed shapes: abs sum 0.01; gx 0.11, g_spline_weight
0.02, g_base_weight 0.02; g_gamma and g_beta 0.25 of max(fp32 bound, 4 x E32); gx over many slabs 0.71 (70001 rows of 3 columns under
a LayerNorm).
"""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import kagnn_amd
from kagnn_amd import ops
from helpers import TOL, assert_close, must_fail, prenorm_bias_noise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(1, 1, 1, 1), (7, 3, 2, 2), (130, 5, 3, 4), (257, 33, 17, 8), (300, 5, 130, 32), (1000, 64, 64, 8), (64, 70, 9, 48)]
VARIANTS = ["ln", "plain"]
TAU_REL = 2e-6
LOOSE_CAP = 0.05
EPS = 1e-5


# ---------------------------------------------------------------------------------- inputs and the fp64 reference
def make_case(n, fin, fout, G, ln=True, base=True, seed=0, ln_scale=1.0):
    gen = torch.Generator().manual_seed(1000 * seed + 7 * n + fin + 3 * fout + G)
    ln = ln and fin > 1                                     # (the layer itself refuses a layernorm over one column)
    return SimpleNamespace(
        n=n, fin=fin, fout=fout, G=G,
        x=0.8 * torch.randn(n, fin, generator=gen),
        sw=0.3 * torch.randn(fout, fin * G, generator=gen),
        bw=0.3 * torch.randn(fout, fin, generator=gen) if base else None,
        gamma=ln_scale * (1.0 + 0.3 * torch.randn(fin, generator=gen)) if ln else None,
        beta=ln_scale * 0.2 * torch.randn(fin, generator=gen) if ln else None,
        centers=torch.linspace(-2.0, 2.0, G),
        den=4.0 / (G - 1) if G > 1 else 1.0)                # one centre: an explicit denominator


def layer_norm(x, gamma, beta):
    mean = x.mean(1, keepdim=True)
    rstd = ((x - mean).square().mean(1, keepdim=True) + EPS).rsqrt()
    return (x - mean) * rstd * gamma + beta


def phi_of(x, sw, bw, gamma, beta, centers, den, G):
    """phi [n, out, in], the RBF table [n, in, G] and u, in the dtype of the operands"""
    u = x if gamma is None else layer_norm(x, gamma, beta)
    rbf = torch.exp(-((u.unsqueeze(-1) - centers) / den) ** 2)
    phi = torch.einsum("nig,oig->noi", rbf, sw.view(sw.size(0), -1, G))
    if bw is not None:
        phi = phi + F.silu(x)[:, None, :] * bw
    return phi, rbf, u


def leaves_of(c, dtype):
    p = {"x": c.x, "sw": c.sw, "bw": c.bw, "gamma": c.gamma, "beta": c.beta}
    return {k: v.to(dtype).clone().requires_grad_(True) for k, v in p.items() if v is not None}


def phi64(c, x=None):
    x = (c.x if x is None else x).double()
    d = lambda t: None if t is None else t.double()
    return phi_of(x, d(c.sw), d(c.bw), d(c.gamma), d(c.beta), c.centers.double(), c.den, c.G)[0]


def grad_reference(c, gS, x=None, want=("x", "sw", "bw", "gamma", "beta")):
    """fp64 gradients of sum(gS * S) by autograd with the terms of |phi| < tau removed, and per entry of gx / g_sw / g_bw the sum of
    |removed terms|.  -> S64, {name: (gradient, allowance or None)} -- behind a layernorm ("x": (gradient, allowance, kinks), see
    ``resolve_kinks``) --, share of (o, i) pairs with a removed term, share of gx entries (n, i) with a removed term phi[n, :, i],
    share of gx entries that carry an allowance"""
    cc = c if x is None else SimpleNamespace(**{**vars(c), "x": x})
    p = leaves_of(cc, torch.float64)
    phi, rbf, u = phi_of(p["x"], p["sw"], p.get("bw"), p.get("gamma"), p.get("beta"), c.centers.double(), c.den, c.G)
    gS = gS.double().cpu()
    pd = phi.detach()
    tau = TAU_REL * float(pd.abs().max()) if pd.numel() else 0.0
    keep = pd.abs() >= tau
    names = [k for k in want if k in p]
    grads = torch.autograd.grad((gS * (phi * (torch.sign(pd) * keep)).sum(0)).sum(), [p[k] for k in names])
    drop = (~keep).double()
    xd, ud, rd = p["x"].detach(), u.detach(), rbf.detach()
    w3 = p["sw"].detach().view(c.fout, c.fin, c.G)
    allow = {"sw": (gS.abs().unsqueeze(-1) * torch.einsum("noi,nig->oig", drop, rd)).reshape(c.fout, -1)}
    if c.bw is not None:
        allow["bw"] = gS.abs() * (drop * F.silu(xd).abs()[:, None, :]).sum(0)
    # gx: a removed element (n, o, j) is the term  s (t_u d u_j / d x + t_b e_j)  of row n, s its sign,  t_u = gS dphi/du,
    # t_b = gS bw silu'(x[n, j]);  d u_j / d x_i = gamma_j rstd (delta_ij - 1 / in - z_i z_j / in) behind a layernorm, else delta_ij
    dphi_du = torch.einsum("nig,oig->noi", rd * (-2.0 * (ud.unsqueeze(-1) - c.centers.double()) / c.den ** 2), w3)
    t_u = gS * dphi_du
    t_b = torch.zeros_like(t_u)
    if c.bw is not None:
        sg = torch.sigmoid(xd)
        t_b = gS * c.bw.double() * (sg * (1 + xd * (1 - sg)))[:, None, :]
    kinks = None
    if c.gamma is not None:
        mean = xd.mean(1, keepdim=True)
        rstd = ((xd - mean).square().mean(1, keepdim=True) + EPS).rsqrt()
        z = (xd - mean) * rstd
        own = c.gamma.double() * rstd * (1.0 - 1.0 / c.fin - z * z / c.fin)             # d u_i / d x_i  [n, in]
        ax = (drop * (t_u * own[:, None, :] + t_b).abs()).sum(1)                       # the entry's own terms
        kinks = {}
        for n, o, j in (~keep).nonzero().tolist():
            v = -(1.0 / c.fin + z[n] * z[n, j] / c.fin)
            v[j] += 1.0
            v = v * (t_u[n, o, j] * c.gamma.double()[j] * rstd[n, 0])
            v[j] += t_b[n, o, j]
            kinks.setdefault(n, []).append(v)
        for n, vs in kinks.items():                                                    # too many to resolve: the whole row is loose
            if len(vs) > MAX_KINKS:
                ax[n] = torch.stack(vs).abs().sum(0)
    else:
        ax = (drop * (t_u + t_b).abs()).sum(1)
    allow["x"] = ax
    ref = {k: (g, allow.get(k)) for k, g in zip(names, grads)}
    if kinks is not None and "x" in ref:
        ref["x"] = (ref["x"][0], ax, kinks)
    pairs = float((~keep).any(0).double().mean()) if pd.numel() else 0.0
    entries = float((~keep).any(1).double().mean()) if pd.numel() else 0.0
    reached = float((ax > 0).double().mean()) if ax.numel() else 0.0
    return pd.abs().sum(0), ref, pairs, entries, reached


MAX_KINKS = 6


def resolve_kinks(got, want, allow, kinks):
    """Behind a layernorm a removed element (n, o, j) reaches every gx entry of row n: as  s v,  v [in] known in fp64 and s in
    {-1, 0, +1} the one thing the kink leaves open.  An allowance on every entry of such a row would leave whole rows loose, so the
    sign is taken from the device instead: per row the s (one per removed element, at most MAX_KINKS of them) that fits the row
    best is added to the reference, and EVERY entry of the row is then held to the plain fp32 bound -- the entries of the row
    share the few signs, which is stricter than the allowance.  The allowance stays on the entries (n, j) of the removed elements'
    own columns for the count of loosened entries (their terms are the ones whose sign the device supplies), and on whole rows
    with more removed elements than that.  -> the completed reference and the allowance that is left"""
    import itertools
    want, allow = want.clone(), allow.clone()
    for n, vs in kinks.items():
        if len(vs) > MAX_KINKS:
            continue
        V = torch.stack(vs)                                                            # [d, in]
        resid = got[n] - want[n]
        best = min((torch.tensor(s, dtype=torch.float64) @ V for s in itertools.product((-1.0, 0.0, 1.0), repeat=len(vs))),
                   key=lambda fit: float((resid - fit).abs().max()))
        want[n] += best
        allow[n] = 0.0
    return want, allow


def fp32_autograd_error(c, gS, ref):
    """E32 per LayerNorm parameter: max |torch's fp32 CPU autograd of the composed formula - the fp64 gradient|"""
    p = leaves_of(c, torch.float32)
    phi = phi_of(p["x"], p["sw"], p.get("bw"), p["gamma"], p["beta"], c.centers, c.den, c.G)[0]
    g = torch.autograd.grad((gS * phi.abs().sum(0)).sum(), [p["gamma"], p["beta"]])
    return {k: float((t.double() - ref[k][0]).abs().max()) for k, t in zip(("gamma", "beta"), g)}


def check_grad(got, want, allow, what, kinks=None):
    """every entry within the fp32 bound (2e-5 of the tensor's maximum) plus its own allowance; -> worst error / bound"""
    got, want = got.detach().double().cpu(), want.double()
    allow = torch.zeros_like(want) if allow is None else allow.double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), what
    if not want.numel():
        return 0.0
    scale = float(want.abs().max())
    if kinks:
        want, allow = resolve_kinks(got, want, allow, kinks)
    err = (got - want).abs()
    worst = float((err - allow).clamp(min=0).max()) / max(TOL * scale, 1e-300)
    print(f"{what}: fraction of the fp32 bound {worst:.3f}, entries with an allowance {int((allow > 0).sum())}/{allow.numel()}")
    assert bool((err <= TOL * scale + allow).all()), (what, float(err.max()), scale, float(allow.max()))
    return worst


def check_ln_grad(got, want, e32, what):
    """a signed sum over rows and outputs: max(fp32 bound, 4 x E32)"""
    got, want = got.detach().double().cpu(), want.double()
    assert got.shape == want.shape and bool(torch.isfinite(got).all()), what
    bound = max(TOL * float(want.abs().max()), 4.0 * e32)
    err = float((got - want).abs().max())
    print(f"{what}: err {err:.3e}, fp32 bound {TOL * float(want.abs().max()):.3e}, 4 x E32 {4 * e32:.3e}, fraction of the bound {err / max(bound, 1e-300):.3f}")
    assert err <= bound, (what, err, bound)
    return err / max(bound, 1e-300)


def dev_args(c):
    d = lambda t: None if t is None else t.to(DEV)
    return d(c.gamma), d(c.beta), d(c.sw), d(c.bw), c.centers.to(DEV), c.den, EPS


def run_device(c, gS=None, x=None):
    """S and, with gS, the gradients on the device"""
    lw, lb, sw, bw, centers, den, eps = dev_args(c)
    xd = (c.x if x is None else x).to(DEV).requires_grad_(gS is not None)
    leaves = {"x": xd, "sw": sw, "bw": bw, "gamma": lw, "beta": lb}
    for t in leaves.values():
        if t is not None:
            t.requires_grad_(gS is not None)
    S = ops.fastkan_edge_abs_sum(xd, lw, lb, sw, bw, centers, den, eps)
    if gS is None:
        return S
    S.backward(gS.to(DEV))
    return S.detach(), {k: t.grad for k, t in leaves.items() if t is not None}


def variant_case(shape, variant):
    """"no_base_ln_near": gamma and beta at 0.3 of their usual size, so that the LayerNorm output stays within the centres' reach"""
    return make_case(*shape, ln=variant in ("ln", "no_base_ln", "no_base_ln_near"), base=not variant.startswith("no_base"),
                     ln_scale=0.3 if variant == "no_base_ln_near" else 1.0)


_CASES = {}


def cached(shape, variant):
    """one case, its fp64 reference and its device result per (shape, variant), shared by the tests below and left unchanged"""
    key = (shape, variant)
    if key not in _CASES:
        c = variant_case(shape, variant)
        gS = torch.randn(c.fout, c.fin, generator=torch.Generator().manual_seed(99))
        want, ref, pairs, entries, reached = grad_reference(c, gS)
        S, g = run_device(c, gS)
        _CASES[key] = (c, gS, want, ref, pairs, reached, S, g)
    return _CASES[key]


CASES = [(s, v) for s in SHAPES for v in VARIANTS if not (s[1] == 1 and v == "ln")] + [(SHAPES[3], "no_base"), (SHAPES[3], "no_base_ln_near")]
CASE_IDS = ["%dx%d-%d_G%d-%s" % (*s, v) for s, v in CASES]


# ---------------------------------------------------------------------------------- abs sum and gradients against fp64
@pytest.mark.parametrize("shape,variant", CASES + [(SHAPES[3], "no_base_ln")], ids=CASE_IDS + ["%dx%d-%d_G%d-no_base_ln" % SHAPES[3]])
def test_abs_sum_matches_fp64(shape, variant):
    if variant == "no_base_ln":
        c = variant_case(shape, variant)
        assert_close(run_device(c), phi64(c).abs().sum(0), what=f"abs sum {shape} {variant}")
        return
    c, gS, want, ref, pairs, entries, S, g = cached(shape, variant)
    assert S.shape == (c.fout, c.fin) and S.dtype == torch.float32
    rel = assert_close(S, want, what=f"abs sum {shape} {variant}")
    print(f"abs sum {shape} {variant}: fraction of the fp32 bound {rel / TOL:.3f}")


@pytest.mark.parametrize("shape,variant", CASES, ids=CASE_IDS)
def test_abs_sum_gradients_match_fp64(shape, variant):
    c, gS, want, ref, pairs, reached, S, g = cached(shape, variant)
    assert set(g) == set(ref)
    for name in ("x", "sw", "bw"):
        if name in ref:
            check_grad(g[name], ref[name][0], ref[name][1], f"g_{name} {shape} {variant}", *ref[name][2:])
    if c.gamma is not None:
        e32 = fp32_autograd_error(c, gS, ref)
        for name in ("gamma", "beta"):
            check_ln_grad(g[name], ref[name][0], e32[name], f"g_{name} {shape} {variant}")


@pytest.mark.parametrize("shape,variant", CASES, ids=CASE_IDS)
def test_allowance_shares_stay_under_the_cap(shape, variant):
    """at most 5 % of the (o, i) pairs and 5 % of the gx entries may carry an allowance: every entry whose allowance is not zero
    counts, so behind a LayerNorm every entry of a row that has a removed term"""
    c, gS, want, ref, pairs, reached, S, g = cached(shape, variant)
    print(f"{shape} {variant}: (o, i) pairs with an allowance {pairs:.4f}, gx entries with an allowance {reached:.4f}")
    assert pairs <= LOOSE_CAP and reached <= LOOSE_CAP, (pairs, reached)


def test_column_slice_in_and_wider_output():
    """x as a column slice of a wider activation, S written into a block of a wider sentinel-filled buffer"""
    c = make_case(257, 33, 17, 8, seed=2)
    wide = torch.randn(c.n, c.fin + 9, generator=torch.Generator().manual_seed(5)).to(DEV)
    wide[:, 4:4 + c.fin] = c.x.to(DEV)
    x = wide[:, 4:4 + c.fin]
    assert not x.is_contiguous()
    lw, lb, sw, bw, centers, den, eps = dev_args(c)
    buf = torch.full((c.fout + 2, c.fin + 3), -777.0, device=DEV)
    block = buf[1:1 + c.fout, 2:2 + c.fin]
    ops._fastkan_edge_abs_sum_raw(x, lw, lb, sw, bw, centers, c.G, c.fin, c.fout, den, eps, out=block)
    assert_close(block, phi64(c).abs().sum(0), what="abs sum of a column slice into a block")
    assert torch.equal(block, run_device(c))
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[1:1 + c.fout, 2:2 + c.fin] = False
    assert bool((buf[mask] == -777.0).all())
    # the gradients of the slice are those of its contiguous copy, bit for bit
    gS = torch.randn(c.fout, c.fin, generator=torch.Generator().manual_seed(96))
    wide.requires_grad_(True)
    ops.fastkan_edge_abs_sum(wide[:, 4:4 + c.fin], lw, lb, sw, bw, centers, den, eps).backward(gS.to(DEV))
    _, g = run_device(c, gS)
    assert torch.equal(wide.grad[:, 4:4 + c.fin], g["x"]) and not bool(wide.grad[:, :4].any()) and not bool(wide.grad[:, 4 + c.fin:].any())


# ---------------------------------------------------------------------------------- mutation guards
def test_checks_reject_mutants():
    shape = SHAPES[3]
    c, gS, want, ref, pairs, entries, S, g = cached(shape, "ln")
    e32 = fp32_autograd_error(c, gS, ref)
    with pytest.raises(AssertionError):
        check_ln_grad(torch.zeros_like(g["gamma"]), ref["gamma"][0], e32["gamma"], "zeroed g_gamma [mutant]")
    with pytest.raises(AssertionError):
        check_grad(g["x"] + 1e-3 * g["x"].abs().max(), ref["x"][0], ref["x"][1], "gx moved by 1e-3 of its maximum [mutant]", *ref["x"][2:])
    must_fail(S - phi64(c)[100].abs().float().to(DEV), want, what="abs sum without row 100")
    # a row whose removed term's sign is taken from the device is held to the plain bound on every entry: one entry of such a row
    # moved by 10 bounds (well inside the allowance a whole-row allowance would have granted nowhere near all rows) must fail
    kinks = ref["x"][2]
    n = next(iter(kinks))
    i = int(kinks[n][0].abs().argmin())
    moved = g["x"].clone()
    moved[n, i] += 10 * TOL * float(ref["x"][0].abs().max())
    with pytest.raises(AssertionError):
        check_grad(moved, ref["x"][0], ref["x"][1], "one entry of a resolved row moved by 10 bounds [mutant]", kinks)


# ---------------------------------------------------------------------------------- many slabs
MANY_SLABS = [(70001, 3, 5, 5), (8193, 64, 64, 8)]
MANY_SLAB_IDS = ["70001x3-5_G5", "8193x64-64_G8"]
_MANY = {}


def many_slab_case(shape):
    """the case, its upstream gradient and its fp64 abs sum, gx and gx allowance (computed once per shape, left unchanged)"""
    if shape not in _MANY:
        c = make_case(*shape, seed=4)
        gS = torch.randn(c.fout, c.fin, generator=torch.Generator().manual_seed(98))
        want = torch.zeros(c.fout, c.fin, dtype=torch.float64)
        gx, ax, kinks = [], [], {}
        for r0 in range(0, c.n, 2048):        # (the fp64 reference in pieces: [N, out, in] at once is 270 MB; gx is per row)
            s64, ref, _, _, _ = grad_reference(c, gS, c.x[r0:r0 + 2048], want=("x",))
            want += s64
            gx.append(ref["x"][0]); ax.append(ref["x"][1])
            kinks.update({r0 + n: vs for n, vs in ref["x"][2].items()})
        _MANY[shape] = (c, gS, want, torch.cat(gx), torch.cat(ax), kinks)
    return _MANY[shape]


@pytest.mark.parametrize("shape", MANY_SLABS, ids=MANY_SLAB_IDS)
def test_many_slabs_gx_allowance_share(shape):
    """at most 0.1 % of the gx entries may carry an allowance there: every entry whose allowance is not zero counts"""
    c, gS, want, gx, ax, kinks = many_slab_case(shape)
    share = float((ax > 0).double().mean())
    print(f"{shape}: gx entries with an allowance {share:.5f}")
    assert share <= 0.001, share


@pytest.mark.parametrize("shape", MANY_SLABS, ids=MANY_SLAB_IDS)
def test_many_slabs_strict_additive_and_rowwise_identical(shape):
    c, gS, want, gx, ax, kinks = many_slab_case(shape)
    S, g = run_device(c, gS)
    assert_close(S, want, what=f"abs sum {shape}")
    check_grad(g["x"], gx, ax, f"gx {shape}", kinks)
    parts = [run_device(c, gS, c.x[r0:r0 + 1000]) for r0 in range(0, c.n, 1000)]
    # sums over a partition of the rows add, up to the order of summation (2e-6: the project's figure for it)
    assert_close(sum(p[0].double() for p in parts), S.double(), 2e-6, what="abs sum over row chunks", elementwise=False)
    for name in ("sw", "bw", "gamma", "beta"):
        assert_close(sum(p[1][name].double() for p in parts), g[name].double(), 2e-6, what=f"g_{name} over row chunks", elementwise=False)
    # gx is per row, and the row statistics do not depend on the rows around: the same kernels take the same sign decisions
    assert torch.equal(torch.cat([p[1]["x"] for p in parts]), g["x"])


# ---------------------------------------------------------------------------------- reproducibility and precision
def test_two_runs_give_the_same_bits():
    for ln in (True, False):
        c = make_case(8193, 20, 70, 5, ln=ln, seed=5)
        gS = torch.randn(c.fout, c.fin, generator=torch.Generator().manual_seed(97))
        a, b = run_device(c, gS), run_device(c, gS)
        assert torch.equal(a[0], b[0])
        for name in a[1]:
            assert torch.equal(a[1][name], b[1][name]), name
        t = c.x[:500].to(DEV)
        lw, lb, sw, bw, centers, den, eps = dev_args(c)
        assert torch.equal(ops.fastkan_edge_curves(t, sw, bw, centers, den), ops.fastkan_edge_curves(t, sw, bw, centers, den))


def load_layer(c, use_layernorm=None):
    layer = kagnn_amd.FastKANLayer(c.fin, c.fout, num_grids=c.G, use_base_update=c.bw is not None,
                                   use_layernorm=c.gamma is not None if use_layernorm is None else use_layernorm)
    layer.rbf.denominator = c.den
    with torch.no_grad():
        layer.spline_linear.weight.copy_(c.sw)
        if c.bw is not None:
            layer.base_linear.weight.copy_(c.bw)
        if c.gamma is not None and layer.layernorm is not None:
            layer.layernorm.weight.copy_(c.gamma); layer.layernorm.bias.copy_(c.beta)
    return layer.to(DEV)


def test_precision_setting_does_not_reach_the_edge_kernels():
    c = make_case(257, 33, 17, 8, seed=3)
    layer = load_layer(c)
    x = c.x.to(DEV)
    res = []
    for mode in (None, ops.PREC_SPLIT, ops.PREC_HALF, ops.PREC_FP32):
        layer.precision = mode
        xg = x.clone().requires_grad_(True)
        l1 = layer.edge_l1(xg)
        l1.sum().backward()
        res.append((l1.detach(), layer.edge_curves(x), xg.grad, layer.spline_linear.weight.grad.clone(), layer.layernorm.weight.grad.clone()))
        layer.zero_grad()
    for other in res[1:]:
        for a, b in zip(other, res[0]):
            assert torch.equal(a, b)
    assert_close(res[0][0], phi64(c).abs().mean(0), what="edge_l1")


# ---------------------------------------------------------------------------------- non-finite inputs, zero weights, no rows
def test_non_finite_rows_poison_exactly_their_column_without_layernorm():
    c = make_case(300, 6, 70, 5, ln=False, seed=6)
    clean = run_device(c)
    others = [i for i in range(c.fin) if i != 4]
    for bad in (float("nan"), float("inf"), float("-inf")):
        x = c.x.clone()
        x[17, 4] = bad
        S = run_device(c, x=x)
        assert not bool(torch.isfinite(S[:, 4]).any()), bad
        assert torch.equal(S[:, others], clean[:, others]), bad
    # without the base branch an RBF of +-Inf is 0: only a NaN poisons
    nb = make_case(300, 6, 70, 5, ln=False, base=False, seed=6)
    clean = run_device(nb)
    x = nb.x.clone()
    x[17, 4] = float("nan")
    S = run_device(nb, x=x)
    assert bool(torch.isnan(S[:, 4]).all()) and torch.equal(S[:, others], clean[:, others])


def test_a_nan_behind_a_layernorm_poisons_every_column():
    c = make_case(300, 6, 70, 5, seed=6)
    x = c.x.clone()
    x[17, 4] = float("nan")
    assert not bool(torch.isfinite(run_device(c, x=x)).any())


@pytest.mark.parametrize("ln", [True, False], ids=["ln", "plain"])
def test_zero_weights_give_zero_sum_and_zero_gradients(ln):
    c = make_case(257, 9, 17, 4, ln=ln, seed=7)
    c.bw, c.sw = torch.zeros_like(c.bw), torch.zeros_like(c.sw)
    S, g = run_device(c, torch.randn(c.fout, c.fin))
    assert not bool(S.any())
    for name, t in g.items():
        assert not bool(t.any()), name


@pytest.mark.parametrize("ln", [True, False], ids=["ln", "plain"])
def test_no_rows(ln):
    c = make_case(0, 5, 7, 4, ln=ln, seed=8)
    S, g = run_device(c, torch.randn(c.fout, c.fin))
    assert S.shape == (7, 5) and not bool(S.any())
    assert g["x"].shape == (0, 5)
    for name in g:
        if name != "x":
            assert g[name].shape == getattr(c, name).shape and not bool(g[name].any()), name
    lw, lb, sw, bw, centers, den, eps = dev_args(c)
    assert ops.fastkan_edge_curves(torch.empty(0, device=DEV), sw, bw, centers, den).shape == (0, 7, 5)


# ---------------------------------------------------------------------------------- curves
def probe_points(centers, h):
    """every centre, one ulp either side, the midpoints, 8 h beyond both ends, NaN"""
    inf = torch.tensor(float("inf"))
    return torch.cat([centers, torch.nextafter(centers, inf), torch.nextafter(centers, -inf), (centers[1:] + centers[:-1]) / 2,
                      torch.stack([centers[0] - 8 * h, centers[-1] + 8 * h]), torch.tensor([float("nan")])])


@pytest.mark.parametrize("shape", [(2, 2, 2), (17, 33, 4), (70, 16, 8), (130, 5, 32)], ids=["2-2_G2", "17-33_G4", "70-16_G8", "130-5_G32"])
@pytest.mark.parametrize("form", ["shared", "per-feature"])
def test_curves_at_the_centre_probes(shape, form):
    c = make_case(1, *shape, ln=False, seed=10)
    t = probe_points(c.centers, c.den)
    if form == "per-feature":           # other abscissae per input: every column shifted by its own fraction of the spacing
        t = (t.unsqueeze(1) + c.den * torch.linspace(-0.4, 0.4, c.fin)).contiguous()
        tt = t
    else:
        tt = t.unsqueeze(1).expand(-1, c.fin)
    lw, lb, sw, bw, centers, den, eps = dev_args(c)
    got = ops.fastkan_edge_curves(t.to(DEV), sw, bw, centers, den)
    assert got.shape == (tt.size(0), c.fout, c.fin)
    assert bool(torch.isnan(got[-1]).all())
    assert_close(got, phi64(c, tt), what=f"curves {shape} {form}")
    # either branch alone, and the base branch at abscissae of its own
    nb = SimpleNamespace(**{**vars(c), "bw": None})
    assert_close(ops.fastkan_edge_curves(t.to(DEV), sw, None, centers, den), phi64(nb, tt), what=f"spline curves {shape} {form}")
    tb = (0.7 * tt + 0.1).contiguous()
    base = F.silu(tb.double())[:, None, :] * c.bw.double()
    assert_close(ops.fastkan_edge_curves(None, None, bw, centers, den, base_points=tb.to(DEV)), base, what=f"base curves {shape} {form}")
    assert_close(ops.fastkan_edge_curves(t.to(DEV), sw, bw, centers, den, base_points=(tb if form == "per-feature" else tb[:, 0].contiguous()).to(DEV)),
                 phi64(nb, tt) + (base if form == "per-feature" else F.silu(tb[:, :1].double())[:, None, :] * c.bw.double()),
                 what=f"curves with base points {shape} {form}")


def test_plot_curve_is_the_reference_formula_and_a_column_of_edge_curves():
    c = make_case(1, 17, 33, 8, seed=11)
    layer = load_layer(c)
    for i, o, kw in ((0, 0, {}), (16, 32, {}), (5, 7, dict(num_pts=257, num_extrapolate_bins=3))):
        x, y = layer.plot_curve(i, o, **kw)
        num_pts, ne = kw.get("num_pts", 1000), kw.get("num_extrapolate_bins", 2)
        assert x.device == y.device == layer.spline_linear.weight.device and x.shape == y.shape == (num_pts,)
        assert torch.equal(x.cpu(), torch.linspace(-2.0 - ne * c.den, 2.0 + ne * c.den, num_pts))
        w = c.sw.double()[o, i * c.G:(i + 1) * c.G]
        want = (w * torch.exp(-((x.cpu().double()[:, None] - c.centers.double()) / c.den) ** 2)).sum(-1)      # fastkan.py:114
        assert_close(y, want, what=f"plot_curve({i}, {o})")
        curves = ops.fastkan_edge_curves(x, layer.spline_linear.weight, None, layer.rbf.grid, layer.rbf.denominator)
        assert torch.equal(y, curves[:, o, i])


@pytest.mark.parametrize("ln", [True, False], ids=["ln", "plain"])
def test_curves_sum_to_the_layer_forward(ln):
    """sum_i edge_curves(LN64(x), base_points=x) + bias is the layer's own forward in exact-fp32 mode"""
    c = make_case(300, 33, 17, 8, ln=ln, seed=12)
    layer = load_layer(c)
    layer.precision = ops.PREC_FP32
    x = c.x.to(DEV)
    u = layer_norm(c.x.double(), c.gamma.double(), c.beta.double()).float().to(DEV) if ln else x
    curves = layer.edge_curves(u, base_points=x)
    with torch.no_grad():
        y = layer(x)
        assert_close(curves.double().sum(2) + layer.base_linear.bias.double(), y, what="sum of the curves + bias vs the layer")
    assert_close(y, phi64(c).sum(2) + layer.base_linear.bias.detach().double().cpu(), what="the layer vs fp64")


def test_curves_average_to_edge_l1():
    c = make_case(700, 16, 70, 8, ln=False, seed=13)
    layer = load_layer(c)
    x = c.x.to(DEV)
    curves = layer.edge_curves(x)
    assert_close(curves, phi64(c), what="edge_curves")
    assert_close(layer.edge_l1(x), curves.double().abs().mean(0), what="edge_l1 vs the curves' mean")
    # a layernorm layer asked for its statistic without the normalisation is the plain layer
    c2 = make_case(700, 16, 70, 8, ln=True, seed=13)
    both = load_layer(c2)
    plain = SimpleNamespace(**{**vars(c2), "gamma": None, "beta": None})
    assert_close(both.edge_l1(x, use_layernorm=False), phi64(plain).abs().mean(0), what="edge_l1(use_layernorm=False)")
    assert_close(both.edge_l1(x), phi64(c2).abs().mean(0), what="edge_l1 with the layernorm")


# ---------------------------------------------------------------------------------- regulariser
def reg_formula(mag, a, e):
    total = mag.sum()
    p = mag / total
    return a * total - e * torch.sum(p * p.log())


def test_regularization_loss_fastkan_layer():
    c = make_case(257, 33, 17, 8, seed=14)
    layer = load_layer(c)
    a, e = 0.7, 1.3
    x = c.x.to(DEV).requires_grad_(True)
    loss = layer.regularization_loss(x, a, e)
    loss.backward()
    mag = phi64(c).abs().mean(0).requires_grad_(True)
    want = reg_formula(mag, a, e)
    want.backward()
    assert_close(loss.reshape(1), want.detach().reshape(1), what="regulariser")
    gS = mag.grad / c.n                                             # d loss / d S = (d loss / d mag) / N
    _, ref, pairs, _, reached = grad_reference(c, gS)
    assert pairs <= LOOSE_CAP and reached <= LOOSE_CAP, (pairs, reached)
    got = {"x": x.grad, "sw": layer.spline_linear.weight.grad, "bw": layer.base_linear.weight.grad,
           "gamma": layer.layernorm.weight.grad, "beta": layer.layernorm.bias.grad}
    for name in ("x", "sw", "bw"):
        check_grad(got[name], ref[name][0], ref[name][1], f"regulariser g_{name}", *ref[name][2:])
    e32 = fp32_autograd_error(c, gS, ref)
    for name in ("gamma", "beta"):
        check_ln_grad(got[name], ref[name][0], e32[name], f"regulariser g_{name}")
    assert layer.base_linear.bias.grad is None                       # the bias is no part of phi


def test_regularization_loss_three_layer_chain():
    """fp64 through autograd, |.| replaced by phi * sign(phi) [|phi| >= tau] so that the removed terms are removed along the whole
    chain.  The case (64 rows, widths 5-6-4-3) is one where the fp64 reference removes nothing: no allowance anywhere."""
    widths, G, n = [5, 6, 4, 3], 5, 64
    cs = [make_case(n, a, b, G, seed=20 + i) for i, (a, b) in enumerate(zip(widths[:-1], widths[1:]))]
    chain = kagnn_amd.FastKAN(widths, num_grids=G)
    gen = torch.Generator().manual_seed(77)
    biases = [0.2 * torch.randn(b, generator=gen) for b in widths[1:]]
    with torch.no_grad():
        for layer, c, bias in zip(chain.layers, cs, biases):
            layer.spline_linear.weight.copy_(c.sw); layer.base_linear.weight.copy_(c.bw); layer.base_linear.bias.copy_(bias)
            layer.layernorm.weight.copy_(c.gamma); layer.layernorm.bias.copy_(c.beta)
            layer.precision = ops.PREC_FP32      # (the layers between the statistics in exact fp32: the bound below is the fp32 one)
    chain = chain.to(DEV)
    x = cs[0].x.to(DEV)
    loss = chain.regularization_loss(x, 0.9, 1.1)
    loss.backward()
    l1 = chain.edge_l1(x)

    leaves, h, want, removed = [], cs[0].x.double(), 0.0, 0
    for c, bias in zip(cs, biases):
        p = {k: v.double().requires_grad_(True) for k, v in (("sw", c.sw), ("bw", c.bw), ("gamma", c.gamma), ("beta", c.beta))}
        p["bias"] = bias.double().requires_grad_(True)
        leaves.append(p)
        phi = phi_of(h, p["sw"], p["bw"], p["gamma"], p["beta"], c.centers.double(), c.den, G)[0]
        keep = phi.detach().abs() >= TAU_REL * float(phi.detach().abs().max())
        removed += int((~keep).sum())
        want = want + reg_formula((phi * (torch.sign(phi.detach()) * keep)).sum(0) / n, 0.9, 1.1)
        h = phi.sum(2) + p["bias"]
    assert removed == 0, removed
    want.backward()
    assert_close(loss.reshape(1), want.detach().reshape(1), what="chain regulariser")
    for li, (layer, p, stat, c) in enumerate(zip(chain.layers, leaves, l1, cs)):
        assert stat.shape == (c.fout, c.fin)
        named = [("sw", layer.spline_linear.weight), ("bw", layer.base_linear.weight), ("gamma", layer.layernorm.weight),
                 ("beta", layer.layernorm.bias)]
        if li + 1 < len(cs):
            named.append(("bias", layer.base_linear.bias))          # (the last layer's output feeds no statistic)
        for name, t in named:
            assert_close(t.grad, p[name].grad, what=f"chain regulariser g_{name} {c.fin}->{c.fout}")


def test_chain_walks_inside_a_block_do_not_record():
    torch.manual_seed(4)
    chain = kagnn_amd.FastKAN([5, 6, 3]).to(DEV)
    x = 0.8 * torch.randn(40, 5, device=DEV)
    with kagnn_amd.collect_edge_l1(chain) as stats:
        chain.regularization_loss(x)
        chain.edge_l1(x)
        assert stats == {}
        chain(x)
        assert set(stats) == {"layers.0", "layers.1"}
        assert_close(stats["layers.1"], chain.layers[1].edge_l1(chain.layers[0](x)), what="the chain's forward records")
        # the use_layernorm the call passed is the one the statistic is taken with
        chain.layers[0](x, use_layernorm=False)
        assert torch.equal(stats["layers.0"], chain.layers[0].edge_l1(x, use_layernorm=False))
        assert not torch.equal(stats["layers.0"], chain.layers[0].edge_l1(x))


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
                m = kagnn_amd.GFASTKAN_Nodes(conv, 2, 12, 16, 5, skip=skip, grid_size=4, hidden_layers=2, dropout=0.0)
                x, ei = _node_inputs()
                return m.to(DEV).train(), (lambda mod: mod(x, ei))
            out[f"GFASTKAN_Nodes-{conv}-skip{int(skip)}"] = build

    def fastkagin():
        torch.manual_seed(12)
        d = _graph_batch()
        return kagnn_amd.FASTKAGIN(2, 7, 16, 3, 2, 4, 0.0).to(DEV).train(), (lambda mod: mod(d))

    def fastkagin_regression():
        torch.manual_seed(13)
        H = 32
        d = _graph_batch(integer=True)
        m = kagnn_amd.FASTKAGINRegression(1, 1, 3, H, 2, 4, 1, 0.0, True)
        m.atom_encoder = kagnn_amd.graph_models.AtomEncoder(H, [21])
        m.bond_encoder.bond_embedding_list = torch.nn.ModuleList([torch.nn.Embedding(4, H)])
        return m.to(DEV).train(), (lambda mod: mod(d))
    out["FASTKAGIN"], out["FASTKAGINRegression"] = fastkagin, fastkagin_regression
    return out


MODELS = _models()


@pytest.mark.parametrize("which", list(MODELS), ids=list(MODELS))
def test_collect_edge_l1_over_a_fastkan_model(which):
    model, call = MODELS[which]()
    layers = {n: m for n, m in model.named_modules() if isinstance(m, kagnn_amd.FastKANLayer)}
    assert layers
    outside = call(model)
    upstream = torch.randn(outside.shape, generator=torch.Generator().manual_seed(31)).to(DEV)
    model.zero_grad()
    (outside * upstream).sum().backward()
    grads_outside = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}

    model.zero_grad()
    with kagnn_amd.collect_edge_l1(model) as stats:
        assert ops.layer_inputs_visible()
        inside = call(model)
        assert set(stats) == set(layers), (sorted(stats), sorted(layers))
        (inside.sum() + sum(s.sum() for s in stats.values())).backward()
    assert not ops.layer_inputs_visible()
    tol = 1e-4 if which in ("FASTKAGIN", "FASTKAGINRegression") else 2e-5
    assert_close(inside, outside, tol, what=f"{which}: output inside the block vs outside", elementwise=False)
    for name, layer in layers.items():
        assert stats[name].shape == (layer.output_dim, layer.input_dim)
        assert bool(layer.spline_linear.weight.grad.any()), name

    # each statistic is edge_l1 of that layer on the input it saw: a second run with a forward pre-hook on every layer
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
    # the gradients of (out * upstream).sum() inside a block against outside it
    for name, p in model.named_parameters():
        if name in grads_outside:
            assert_close(p.grad, grads_outside[name], tol, what=f"{which}: gradient of {name} inside vs outside", elementwise=False,
                         noise=prenorm_bias_noise(name, grads_outside))
    assert torch.equal(call(model), outside)


def test_a_mixed_model_yields_both_kinds_of_entries():
    torch.manual_seed(5)
    mixed = torch.nn.ModuleDict({"kan": kagnn_amd.KANLinear(6, 5), "fast": kagnn_amd.FastKANLayer(5, 4)}).to(DEV)
    x = 0.8 * torch.randn(50, 6, device=DEV)
    with kagnn_amd.collect_edge_l1(mixed) as stats:
        h = mixed["kan"](x)
        y = mixed["fast"](h)
    assert set(stats) == {"kan", "fast"}
    assert torch.equal(stats["kan"], mixed["kan"].edge_l1(x)) and stats["kan"].shape == (5, 6)
    assert torch.equal(stats["fast"], mixed["fast"].edge_l1(h)) and stats["fast"].shape == (4, 5)
    (y.sum() + stats["kan"].sum() + stats["fast"].sum()).backward()
    for name, p in mixed.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
