"""Grid refinement -- ``ops.kan_grid_resize`` (csrc/kan_grid.hip), ``KANLinear.refine``, ``KAN.refine`` and ``kagnn_amd.refine_grids`` --
against an fp64 reference built here: ``oracle.kan_oracle.bspline_bases`` on fp64 copies of the knots and of ``x``, the old curves
``A_old @ spline_weight``, and ``torch.linalg.lstsq(..., driver="gelsd")`` over the rows that take part (all of them, or those inside
the window; the window comparison is the device's: fp32 ``lo <= x < hi``).

Inputs: ``spline_weight ~ 0.3 randn``; ``x`` uniform in [-0.99, 0.99], or ``0.8 randn`` together with the window.

Bound on the fitted coefficients: 5e-5 of ``max|reference|`` (what ``test_update_grid_vs_oracle`` holds the same computation to), no
allowance.  "Function kept" (nested refinements only): the refined layer's forward on 2048 fresh rows inside the range against
``oracle.kan_linear_forward`` of the OLD parameters in fp64, at ``helpers.assert_close``'s default fp32 bound.

The order-4 refinement is 13 -> 39 (43 coefficients, 48 knots).  10 -> 40 at order 4 would be 44 coefficients on 49 knots, one past
the 48-knot limit that the entry point, ``KANLinear`` itself and every kernel of orders 1..4 share; that it is refused is asserted
in tests/test_grid_refine_host.py.
"""
import copy
from types import SimpleNamespace

import pytest
import torch

import kagnn_amd
from kagnn_amd import ops
from oracle import kan_oracle as orc
from helpers import assert_close, must_fail

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIT_TOL = 5e-5

# (N, in, out, G_old, G_new, k)
REFINEMENTS = [(4000, 6, 5, 5, 10, 3), (4000, 6, 5, 5, 20, 3),
               (20000, 4, 3, 8, 40, 3),        # 43 coefficients: three 16-blocks
               (20000, 4, 3, 13, 39, 4),       # order 4 at the 48-knot limit: 43 coefficients, the worst-conditioned G1 here
               (20000, 2, 2, 9, 45, 1)]        # the 48-knot limit
LOW_ORDERS = [(4000, 3, 4, 4, 8, 1), (4000, 6, 5, 1, 2, 2), (4000, 5, 4, 3, 12, 4)]
NON_NESTED = [(4000, 6, 5, 5, 7, 3)]
COARSENING = [(4000, 6, 5, 10, 5, 3)]
FEW_ROWS = [(300, 4, 3, 5, 20, 3)]
ONE_ROW = [(1, 1, 1, 1, 2, 1)]
CASES = REFINEMENTS + LOW_ORDERS + NON_NESTED + COARSENING + FEW_ROWS + ONE_ROW
NESTED = REFINEMENTS + LOW_ORDERS + FEW_ROWS
WINDOWED = [(4000, 6, 5, 5, 10, 3), (4000, 6, 5, 5, 20, 3)]


def ids(cases):
    return ["%dx%d-%d_G%dto%d_k%d" % c for c in cases]


def make_case(n, fin, fout, g0, g1, k, dist="uniform", scaler=False, seed=0):
    gen = torch.Generator().manual_seed(100 * seed + 13 * n + 7 * fin + 3 * fout + 31 * g0 + g1 + k)
    x = 0.8 * torch.randn(n, fin, generator=gen) if dist == "randn" else 1.98 * torch.rand(n, fin, generator=gen) - 0.99
    c = SimpleNamespace(n=n, fin=fin, fout=fout, g0=g0, g1=g1, k=k, x=x, sw=0.3 * torch.randn(fout, fin, g0 + k, generator=gen),
                        bw=0.3 * torch.randn(fout, fin, generator=gen), go=orc.make_knots(fin, g0, k), gn=orc.make_knots(fin, g1, k))
    c.sc = None
    if scaler:                      # negative entries and one exact zero
        c.sc = 1.0 + 0.8 * torch.randn(fout, fin, generator=gen)
        c.sc[0, 0] = -abs(c.sc[0, 0]) - 0.1
        c.sc[-1, -1] = 0.0
    c.fresh = 1.98 * torch.rand(2048, fin, generator=gen) - 0.99
    return c


def inner_window(grid, k):
    return torch.stack([grid[:, k], grid[:, -k - 1]], dim=1).contiguous()


def participating(x, window):
    if window is None:
        return torch.ones_like(x, dtype=torch.bool)
    return (x >= window[:, 0]) & (x < window[:, 1])          # fp32 against fp32, as the kernel compares


def reference_fit(x, go, gn, sw, sc, k, window=None):
    """-> (coefficients [out, in, C_new] fp64, untouched [in]): per feature the gelsd least-squares fit over the participating rows"""
    xd = x.double()
    a_old, a_new = orc.bspline_bases(xd, go.double(), k), orc.bspline_bases(xd, gn.double(), k)
    w = sw.double() if sc is None else sw.double() * sc.double().unsqueeze(-1)
    part = participating(x, None if window is None else window.float())
    fit = torch.zeros(sw.size(0), sw.size(1), gn.size(1) - k - 1, dtype=torch.float64)
    untouched = torch.zeros(sw.size(1), dtype=torch.int32)
    for f in range(sw.size(1)):
        rows = part[:, f]
        an = a_new[rows, f]
        curves = a_old[rows, f] @ w[:, f].T
        fit[:, f] = torch.linalg.lstsq(an, curves, driver="gelsd").solution.T
        untouched[f] = int((an.abs().sum(0) == 0).sum())
    return fit, untouched


def device_fit(c, window=None, x=None):
    d = lambda t: None if t is None else t.to(DEV)
    return ops.kan_grid_resize(d(c.x if x is None else x), d(c.go), d(c.gn), d(c.sw), d(c.sc), c.g0, c.g1, c.k, window=d(window))


def layer_of(c, grid_size=None, sw=None, grid=None):
    """a KANLinear holding the case's parameters (old ones by default)"""
    g = c.g0 if grid_size is None else grid_size
    layer = kagnn_amd.KANLinear(c.fin, c.fout, grid_size=g, spline_order=c.k)
    sd = {"base_weight": c.bw, "spline_weight": c.sw if sw is None else sw, "grid": c.go if grid is None else grid,
          "spline_scaler": torch.ones(c.fout, c.fin) if c.sc is None else c.sc}
    layer.load_state_dict(sd)
    return layer.to(DEV)


def old_function(c, rows):
    sc = torch.ones(c.fout, c.fin) if c.sc is None else c.sc
    return orc.kan_linear_forward(rows.double(), c.bw.double(), c.sw.double(), sc.double(), c.go.double(), c.k)


# ---------------------------------------------------------------------------------- the kernel against the fp64 fit
@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_resize_matches_the_fp64_least_squares_fit(case):
    c = make_case(*case)
    want, want_untouched = reference_fit(c.x, c.go, c.gn, c.sw, None, c.k)
    got, untouched = device_fit(c)
    assert got.shape == (c.fout, c.fin, c.g1 + c.k) and untouched.shape == (c.fin,) and untouched.dtype == torch.int32
    err = assert_close(got, want, FIT_TOL, what="resize %dx%d-%d G%d->%d k%d" % case, elementwise=False)
    print("resize", case, "error / max|reference| = %.3e" % err)
    assert torch.equal(untouched.cpu(), want_untouched)


@pytest.mark.parametrize("case", WINDOWED, ids=ids(WINDOWED))
def test_resize_with_the_window_on_rows_beyond_the_range(case):
    c = make_case(*case, dist="randn", scaler=True)
    win = inner_window(c.gn, c.k)
    assert not bool(participating(c.x, win).all())
    want, want_untouched = reference_fit(c.x, c.go, c.gn, c.sw, c.sc, c.k, win)
    got, untouched = device_fit(c, win)
    assert_close(got, want, FIT_TOL, what="windowed resize (scaled curves)", elementwise=False)
    assert torch.equal(untouched.cpu(), want_untouched)


def test_dropping_the_off_diagonal_blocks_of_g2_is_caught():
    """mutation guard for the 43-coefficient case: normal equations whose A_new^T A_old keeps only its diagonal 16-blocks"""
    c = make_case(20000, 4, 3, 8, 40, 3)
    want, _ = reference_fit(c.x, c.go, c.gn, c.sw, None, c.k)
    xd = c.x.double()
    a_old, a_new = orc.bspline_bases(xd, c.go.double(), c.k), orc.bspline_bases(xd, c.gn.double(), c.k)
    g1 = torch.einsum("nfc,nfd->fcd", a_new, a_new)
    g2 = torch.einsum("nfc,nfd->fcd", a_new, a_old)
    blk = (torch.arange(g2.size(1)).unsqueeze(1) // 16) == (torch.arange(g2.size(2)).unsqueeze(0) // 16)
    mutant = torch.linalg.solve(g1, torch.einsum("fcd,ofd->fco", g2 * blk, c.sw.double())).permute(2, 0, 1)
    exact = torch.linalg.solve(g1, torch.einsum("fcd,ofd->fco", g2, c.sw.double())).permute(2, 0, 1)
    assert_close(exact, want, FIT_TOL, what="the unmutated normal equations", elementwise=False)
    must_fail(mutant, want, FIT_TOL, what="block-diagonal G2", elementwise=False)


# ---------------------------------------------------------------------------------- the layer keeps its function
@pytest.mark.parametrize("case", NESTED, ids=ids(NESTED))
@pytest.mark.parametrize("variant", ["in_range", "randn_window", "scaler"])
def test_nested_refinement_keeps_the_function(case, variant):
    c = make_case(*case, dist="randn" if variant == "randn_window" else "uniform", scaler=variant == "scaler")
    layer = layer_of(c)
    untouched = layer.refine(c.x.to(DEV), c.g1)
    assert layer.grid_size == c.g1 and layer.spline_weight.shape == (c.fout, c.fin, c.g1 + c.k) and layer.grid.shape == (c.fin, c.g1 + 2 * c.k + 1)
    assert isinstance(layer.spline_weight, torch.nn.Parameter) and layer._knots().dim() == 1         # still one shared uniform row
    assert_close(layer.grid, c.gn, 5e-7, what="uniform knots")
    assert int(untouched.sum()) == 0
    if c.sc is not None:
        assert torch.equal(layer.spline_scaler.cpu(), c.sc)
    err = assert_close(layer(c.fresh.to(DEV)), old_function(c, c.fresh), what=f"function kept ({variant})")
    print("function kept", case, variant, "error / max|reference| = %.3e" % err)


def test_without_the_window_rows_beyond_the_range_spoil_the_function():
    """mutation guard: the 0.8 randn rows with window=None must FAIL the check the windowed refinement passes"""
    c = make_case(4000, 6, 5, 5, 10, 3, dist="randn")
    want = old_function(c, c.fresh)
    for window, ok in ((inner_window(c.gn, c.k), True), (None, False)):
        fit, _ = device_fit(c, window)
        y = layer_of(c, c.g1, fit.cpu(), c.gn)(c.fresh.to(DEV))
        if ok:
            assert_close(y, want, what="windowed")
        else:
            must_fail(y, want, what="no window")


# ---------------------------------------------------------------------------------- adaptive knots, per-feature knots
@pytest.mark.parametrize("case", [(4000, 6, 5, 5, 10, 3), (4000, 5, 4, 3, 12, 4)], ids=ids([(4000, 6, 5, 5, 10, 3), (4000, 5, 4, 3, 12, 4)]))
def test_adaptive_refinement_matches_the_oracle_update_grid(case):
    c = make_case(*case, dist="randn", scaler=True)
    p = {"grid": c.go, "spline_weight": c.sw, "spline_scaler": None}
    grid, fit = orc.update_grid(c.x, p, c.g1, c.k, solve_dtype=torch.float64)
    layer = layer_of(c)
    untouched = layer.refine(c.x.to(DEV), c.g1, adaptive=True)
    assert_close(layer.grid, grid, 5e-7, what="adaptive knots")
    assert_close(layer.spline_weight, fit, FIT_TOL, what="adaptive refit", elementwise=False)
    assert int(untouched.sum()) == 0 and torch.equal(layer.spline_scaler.cpu(), c.sc) and layer._knots().dim() == 2


@pytest.mark.parametrize("adaptive", [False, True], ids=["uniform", "adaptive"])
def test_refining_a_layer_that_already_holds_per_feature_knots(adaptive):
    c = make_case(4000, 6, 5, 5, 10, 3, dist="randn")
    layer = layer_of(c)
    x = c.x.to(DEV)
    layer.update_grid(x)
    assert layer._knots().dim() == 2
    go, sw = layer.grid.detach().cpu().clone(), layer.spline_weight.detach().cpu().clone()
    layer.refine(x, c.g1, adaptive=adaptive)
    gn = layer.grid.detach().cpu()
    if adaptive:
        want_grid, _ = orc.update_grid(c.x, {"grid": go, "spline_weight": sw, "spline_scaler": None}, c.g1, c.k, solve_dtype=torch.float64)
        window = None
    else:
        lo, hi = go[:, c.k].double(), go[:, -c.k - 1].double()
        want_grid = lo.unsqueeze(1) + torch.arange(-c.k, c.g1 + c.k + 1).double().unsqueeze(0) * ((hi - lo) / c.g1).unsqueeze(1)
        window = inner_window(gn, c.k)
    assert_close(gn, want_grid, 5e-7, what="knots of the refined per-feature layer")
    want, _ = reference_fit(c.x, go, gn, sw, None, c.k, window)
    assert_close(layer.spline_weight, want, FIT_TOL, what="refit from per-feature knots", elementwise=False)
    assert bool(torch.isfinite(layer(x[:512])).all())


def test_column_slice_and_second_call_give_the_same_bits():
    c = make_case(4000, 6, 5, 5, 20, 3)
    first, u1 = device_fit(c)
    again, u2 = device_fit(c)
    assert torch.equal(first, again) and torch.equal(u1, u2)
    wide = torch.randn(c.n, c.fin + 7)
    wide[:, 3:3 + c.fin] = c.x
    sliced, u3 = device_fit(c, x=wide.to(DEV)[:, 3:3 + c.fin])
    assert torch.equal(first, sliced) and torch.equal(u1, u3)


@pytest.mark.parametrize("n,fin,fout,g,k,scaler", [(300, 4, 3, 5, 3, True), (300, 3, 2, 20, 3, False)],      # 8 coefficients; 23: two 16-blocks
                         ids=["300x4-3_G5_k3_scaler", "300x3-2_G20_k3"])
def test_refit_is_the_resize_between_two_grids_of_one_size(n, fin, fout, g, k, scaler):
    """``ops.kan_grid_refit`` (what ``update_grid`` calls) and ``ops.kan_grid_resize`` with equal sizes and no window: one arithmetic,
    the same bits.  The new knots are per-feature rows, each knot moved by up to 0.3 of a step."""
    c = make_case(n, fin, fout, g, g, k, dist="randn", scaler=scaler)
    assert (c.sc is not None and bool((c.sc < 0).any())) == scaler
    step = float(c.gn[0, 1] - c.gn[0, 0])
    c.gn = c.gn + 0.3 * step * (2 * torch.rand(c.gn.shape, generator=torch.Generator().manual_seed(g)) - 1)
    assert bool((c.gn[:, 1:] > c.gn[:, :-1]).all()) and not torch.equal(c.gn[0], c.gn[1])
    d = lambda t: None if t is None else t.to(DEV)
    refit = ops.kan_grid_refit(d(c.x), d(c.go), d(c.gn), d(c.sw), d(c.sc), g, k)
    resized, _ = device_fit(c)
    assert refit.shape == (fout, fin, g + k) and bool(torch.isfinite(refit).all())
    assert torch.equal(refit, resized)


def test_bases_no_sample_reaches_get_zero_and_are_counted():
    c = make_case(4000, 4, 3, 5, 20, 3)
    c.x = -0.99 * torch.rand(c.n, c.fin, generator=torch.Generator().manual_seed(5))            # half the range: (-0.99, 0]
    a_new = orc.bspline_bases(c.x.double(), c.gn.double(), c.k)
    empty = a_new.abs().sum(0) == 0                                                                # [in, C_new]
    assert int(empty.sum()) >= 4 * 8
    got, untouched = device_fit(c, inner_window(c.gn, c.k))
    assert torch.equal(untouched.cpu().long(), empty.sum(1))
    assert bool(torch.isfinite(got).all())
    assert bool((got.cpu()[:, empty] == 0).all())
    want, _ = reference_fit(c.x, c.go, c.gn, c.sw, None, c.k, inner_window(c.gn, c.k))
    assert_close(got, want, FIT_TOL, what="half-range fit", elementwise=False)


# ---------------------------------------------------------------------------------- the chain
def test_kan_chain_refine_against_the_fp64_walk():
    """``KAN.refine``: each layer on its own input, then evaluated refined; 5e-4 is the chain tolerance of test_kan_chain_update_grid_flag"""
    torch.manual_seed(3)
    net = kagnn_amd.KAN([6, 10, 4], grid_size=5, spline_order=3)
    layers = [{n: v.detach().clone() for n, v in l.state_dict().items()} for l in net.layers]
    x = torch.randn(600, 6) * 0.9
    h = x.double()
    for p in layers:
        gn = orc.make_knots(p["grid"].size(0), 10, 3)
        fit, _ = reference_fit(h.float(), p["grid"], gn, p["spline_weight"], None, 3, inner_window(gn, 3))
        h = orc.kan_linear_forward(h, p["base_weight"].double(), fit, p["spline_scaler"].double(), gn.double(), 3)
    net = net.to(DEV)
    untouched = net.refine(x.to(DEV), 10)
    assert net.grid_size == 10 and len(untouched) == 2 and all(l.grid_size == 10 and l.spline_weight.size(2) == 13 for l in net.layers)
    y = net(x.to(DEV))
    assert_close(y, h, tol=5e-4, what="chain after refine")
    assert torch.equal(net(x.to(DEV)), y)


# ---------------------------------------------------------------------------------- whole models
def _node_inputs(seed=0, n=300, e=2000, f=12):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, f, generator=gen), torch.randint(0, n, (2, e), generator=gen)


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
    d = SimpleNamespace(edge_index=torch.stack([torch.cat(src), torch.cat(dst)]), batch=torch.cat(batch), num_graphs=B)
    if integer:
        d.x = torch.randint(0, 21, (n, 1), generator=gen)
        d.edge_attr = torch.randint(0, 4, (e,), generator=gen)
    else:
        d.x = torch.randn(n, f, generator=gen)
    return d


def _on_device(d):
    return SimpleNamespace(**{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in vars(d).items()})


def _models():
    """name -> (builder(grid_size) -> (model on the device in training mode, its arguments, fp64 oracle forward(state)), old and new grid_size)"""
    out = {}
    for conv in ("gin", "gcn"):
        for skip in (True, False):
            def build(grid, conv=conv, skip=skip):
                torch.manual_seed(11)
                m = kagnn_amd.GKAN_Nodes(conv, 2, 12, 16, 5, skip=skip, grid_size=grid, spline_order=3, hidden_layers=2, dropout=0.0)
                x, ei = _node_inputs()
                xd, eid = x.to(DEV), ei.to(DEV)
                return (m.to(DEV).train(), (xd, eid),
                        (lambda st: orc.node_model_forward(x.double(), ei, st, "kan", conv, 2, 3, skip=skip)))
            out[f"GKAN_Nodes-{conv}-skip{int(skip)}"] = (build, 5, 10)

    def kagin(grid):
        torch.manual_seed(12)
        d = _graph_batch()
        dd = _on_device(d)
        return (kagnn_amd.KAGIN(2, 7, 16, 3, 2, grid, 3, 0.0).to(DEV).train(), (dd,),
                (lambda st: orc.graph_classification_forward(d.x.double(), d.edge_index, d.batch, d.num_graphs, st, "kan", "gin", 2, 3)))

    def kagin_regression(grid):
        torch.manual_seed(13)
        H = 32
        d = _graph_batch(integer=True)
        dd = _on_device(d)
        m = kagnn_amd.KAGINRegression(1, 1, 3, H, 2, grid, 3, 1, 0.0, True)
        m.atom_encoder = kagnn_amd.graph_models.AtomEncoder(H, [21])
        m.bond_encoder.bond_embedding_list = torch.nn.ModuleList([torch.nn.Embedding(4, H)])
        return (m.to(DEV).train(), (dd,),
                (lambda st: orc.graph_regression_forward(d.x, d.edge_index, d.edge_attr.view(-1, 1), d.batch, d.num_graphs, st, "kan", 3, 3)))
    out["KAGIN"] = (kagin, 4, 8)
    out["KAGINRegression"] = (kagin_regression, 2, 4)        # 4 + 3 coefficients: still within the one-call GINE stack / model routes
    return out


MODELS = _models()


def _state64(model):
    return {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in model.state_dict().items()}


_REFINED = {}


def _trained_like(model):
    """parameters of the size the kernel-level cases use (0.3 randn, scaler 1 + 0.5 randn) in place of the constructor's: its
    spline coefficients are noise of 1e-2, curves a refit has little to keep"""
    gen = torch.Generator().manual_seed(77)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, kagnn_amd.KANLinear):
                m.base_weight.copy_((0.3 * torch.randn(m.base_weight.shape, generator=gen)).to(DEV))
                m.spline_weight.copy_((0.3 * torch.randn(m.spline_weight.shape, generator=gen)).to(DEV))
                m.spline_scaler.copy_((1.0 + 0.5 * torch.randn(m.spline_scaler.shape, generator=gen)).to(DEV))


def refined(which, adaptive=False):
    """one ``refine_grids`` walk per model and knot rule, shared by the tests below (they read it; the one test that trains runs on a
    copy).  The adaptive walk runs on trained-like parameters."""
    key = (which, adaptive)
    if key not in _REFINED:
        build, g_old, g_new = MODELS[which]
        model, args, oracle = build(g_old)
        if adaptive:
            _trained_like(model)
        layers = {n: m for n, m in model.named_modules() if isinstance(m, kagnn_amd.KANLinear)}
        assert layers and all(l.grid_size == g_old for l in layers.values())
        model(*args)                                       # the fused routes run once on the old shapes: whatever they cache now exists
        before = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        flags = {n: m.training for n, m in model.named_modules()}
        report = kagnn_amd.refine_grids(model, g_new, *args, keep_inputs=True, adaptive=adaptive)
        _REFINED[key] = SimpleNamespace(adaptive=adaptive, model=model, args=args, oracle=oracle, layers=layers, before=before, flags=flags, report=report,
                                          g_old=g_old, g_new=g_new, build=build)
    return _REFINED[key]


def layer_fits(r, name):
    """-> (participating rows [N, in], fp64 bases on the new grid, device coefficients, fp64 reference coefficients, its untouched counts)"""
    layer, e = r.layers[name], r.report[name]
    x, gn = e["input"].cpu(), layer.grid.detach().cpu()
    win = None if r.adaptive else inner_window(gn, 3)
    want, want_untouched = reference_fit(x, r.before[name + ".grid"], gn, r.before[name + ".spline_weight"], None, 3, win)
    return participating(x, win), orc.bspline_bases(x.double(), gn.double(), 3), layer.spline_weight.detach().cpu().double(), want, want_untouched


@pytest.mark.parametrize("which", list(MODELS), ids=list(MODELS))
def test_refine_grids_over_a_model(which):
    r = refined(which)
    model, report, layers, g_old, g_new = r.model, dict(r.report), r.layers, r.g_old, r.g_new
    call = lambda mod: mod(*r.args)
    assert not ops.layer_inputs_visible() and all(r.flags.values())
    assert report.pop("skipped") == [] and set(report) == set(layers)
    assert {n: m.training for n, m in model.named_modules()} == r.flags
    for k, v in model.state_dict().items():                # the norms' running buffers (and everything that is not a refined tensor)
        if not k.endswith((".grid", ".spline_weight")):
            assert torch.equal(v.cpu(), r.before[k]), k
    for name, layer in layers.items():
        e = report[name]
        assert e["grid_size"] == (g_old, g_new) and layer.grid_size == g_new and e["rows"] == e["input"].size(0)
        assert layer.spline_weight.shape == (layer.out_features, layer.in_features, g_new + 3) and layer.grid.shape == (layer.in_features, g_new + 7)
        assert isinstance(layer.spline_weight, torch.nn.Parameter) and layer.spline_weight.requires_grad
        assert e["untouched"].shape == (layer.in_features,) and layer._knots().dim() == 1
    for m in model.modules():
        if isinstance(m, kagnn_amd.KAN):
            assert m.grid_size == g_new

    # the model afterwards: the fp64 oracle on the refined state_dict, and the fused routes against the composed ones
    out = call(model)
    assert_close(out, r.oracle(_state64(model)), 1e-4, what=f"{which}: output after refine_grids")
    with kagnn_amd.collect_edge_l1(model):
        composed = call(model)
    assert_close(out, composed, 2e-5, what=f"{which}: fused routes vs composed routes after refine_grids", elementwise=False)

    # the refined state_dict in a fresh model of the new grid_size: the same bits
    fresh, fresh_args, _ = r.build(g_new)
    fresh.load_state_dict(model.state_dict())
    assert torch.equal(fresh(*fresh_args), out)

    # one training step with a fresh optimizer (on the fresh copy: the shared model stays as refine_grids left it)
    opt = torch.optim.Adam(fresh.parameters(), lr=1e-3)
    upstream = torch.randn(out.shape, generator=torch.Generator().manual_seed(31)).to(DEV)
    (fresh(*fresh_args) * upstream).sum().backward()
    for name, p in fresh.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), name
    opt.step()
    assert bool(torch.isfinite(fresh(*fresh_args)).all())


@pytest.mark.parametrize("which", list(MODELS), ids=list(MODELS))
def test_refine_grids_fitted_curves_match_the_fp64_refit(which):
    """every refined layer against the fp64 refit on its recorded input, as CURVES: ``A_new @ coefficients`` on the participating rows,
    5e-5 of the largest fitted curve value of the layer, and the same ``untouched`` counts.  Unlike the coefficients (next test) the
    fitted curve is determined by the rows however few of them reach a basis; the largest figure seen on the device was 1.2e-5 (KAGIN, conv.1.nn.layers.1)"""
    r = refined(which)
    for name in r.layers:
        part, a_new, got, want, want_untouched = layer_fits(r, name)
        assert torch.equal(r.report[name]["untouched"].cpu(), want_untouched), name
        curves_got = torch.einsum("nfc,ofc->nfo", a_new, got)[part]
        curves_want = torch.einsum("nfc,ofc->nfo", a_new, want)[part]
        assert_close(curves_got, curves_want, FIT_TOL, what=f"{which}: fitted curves of {name}", elementwise=False)


@pytest.mark.parametrize("which", list(MODELS), ids=list(MODELS))
def test_refine_grids_layer_coefficients_match_the_fp64_refit(which):
    """with ``keep_inputs=True`` each layer's new ``spline_weight`` equals the fp64 ``gelsd`` refit of that layer on its recorded input at
    5e-5 of ``max|reference|`` -- on the walk with ``adaptive=True``.

    Why that walk.  A comparison of COEFFICIENTS holds the device to the reference only where the rows determine the coefficients:
    the reference's own answer moves by ``cond(A_new)`` times any perturbation of the bases (fp32 bases: 6e-8), so 5e-5 needs
    ``cond(A_new)`` of 1e2 .. 1e3 per feature.  Quantile knots give that by construction -- every knot interval holds ``N / grid_size``
    rows of the layer's input, whatever its distribution, and every row takes part: measured 6.1e-7 at most over all layers of the six
    models.  On the uniform grid a model's own activations do not: a few hundred rows cluster in part of the range, and beside the
    bases no row reaches there is a basis only the outermost rows reach, with values of 1e-4 and below (measured smallest / largest
    singular value of ``A_new`` per feature 1e-4 .. 1e-11).  There the coefficients of the fp64 reference and of the device differ by
    0.5 .. 17 of ``max|reference|`` in layers behind the first convolution, at 300 and at 900 nodes, with the constructor's parameters and with trained-like
    ones, while both draw the same curve on the rows: the uniform walk is held to the curves (previous test) and, at kernel level,
    to the coefficients on inputs that fill the range (``test_resize_matches_the_fp64_least_squares_fit``)."""
    r = refined(which, adaptive=True)
    assert set(r.report) - {"skipped"} == set(r.layers) and r.report["skipped"] == []
    for name, layer in r.layers.items():
        _, _, got, want, want_untouched = layer_fits(r, name)
        assert layer.grid_size == r.g_new and layer._knots().dim() == 2 and int(want_untouched.sum()) == 0
        assert torch.equal(r.report[name]["untouched"].cpu(), want_untouched), name
        assert_close(got, want, FIT_TOL, what=f"{which}: adaptive refit of {name}", elementwise=False)
    assert bool(torch.isfinite(r.model(*r.args)).all())


def test_refine_grids_skips_high_orders_and_fastkan_layers():
    torch.manual_seed(5)
    model = torch.nn.Sequential(kagnn_amd.KANLinear(6, 8, grid_size=5, spline_order=3), kagnn_amd.KANLinear(8, 8, grid_size=4, spline_order=6),
                                kagnn_amd.FastKANLayer(8, 4)).to(DEV)
    before = copy.deepcopy(model.state_dict())
    x = torch.rand(500, 6, device=DEV) * 1.8 - 0.9
    want = model(x)
    report = kagnn_amd.refine_grids(model, 10, x)
    assert report["skipped"] == ["1", "2"] and set(report) == {"0", "skipped"}
    assert model[0].grid_size == 10 and model[1].grid_size == 4
    for k, v in model.state_dict().items():
        if not k.startswith("0."):
            assert torch.equal(v, before[k]), k
    assert_close(model(x), want, 1e-4, what="nested refinement of the first layer keeps the model's output")
