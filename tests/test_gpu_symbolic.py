"""``ops.symbolic_fit`` (csrc/symbolic.hip) and the ``suggest_symbolic`` surface against the fp64 restatement of the rule in
tests/test_symbolic_host.py.

Scores lie in [0, 1], so the project's fp32 bound of 2e-5 of the maximum is an absolute 2e-5: ``tol = max(2e-5, 4 E32)``, ``E32`` the
worst error of a plain two-pass fp32 torch evaluation of the same tables on the CPU against the restatement (computed here, case by
case, over every table of the case; printed).  Every iteration's device table is compared with the restatement ON THE DEVICE'S OWN
RECORDED RANGES, so an arg-max that legitimately differs between fp32 and fp64 cannot cascade.  Candidates within a factor 2 of the
degeneracy threshold, or with ``sum u^2`` above 1e37, are compared either-or (the device's score is 0 or within tolerance).  On
the caller's ranges they are at most 2 % of each table: which candidates they are depends on ``x`` and the function alone, and the
function lists of the small grids are chosen for it (2 % of a 5 x 5 table is no candidate at all: ``tanh`` puts 2 .. 4 saturated
candidates within a factor 2 of the threshold at Gn 5 .. 11, ``gaussian`` 8 at Gn 9).  A zoomed table lies where the device's winners
put it and can lie across the threshold -- the identity's always ends there: ``c (a x + b) + d`` is the same line for every ``a != 0``,
so its table is flat, its winner is wherever rounding puts it, and its zoom walks into the degenerate wedge around ``a = 0`` (19 % of
the third table at Gn 21, on the restatement alone).  On zoomed tables the share that is held to 2 % is the one that could hide an
error: either-or candidates that the device scored 0 while fp64 did not.

Inputs: ``x`` uniform in [-1, 1]; ``phi`` from a real ``KANLinear`` (``bw, sw ~ 0.3 randn``, ``sc ~ 1 + 0.5 randn``, grid 5, order 3)
through ``edge_curves``, with one planted column ``0.8 sin(3.3 x + 0.7) + 1.5`` at edge (0, 0) where there is more than one edge."""
import functools

import numpy as np
import pytest
import torch

import kagnn_amd
from kagnn_amd import ops
from kagnn_amd.symbolic import SYMBOLIC_LIB, SymbolicSuggestion, strided_rows
from test_gpu_poison import DEV, _GuardedEmpty, _under_every_pattern
from test_subgraph_host import _NoLaunch
from test_symbolic_host import (ALL, F64, argmax_lowest, axis, closed_form, column_state, e32, fit_reference, score_table, zoom)

pytestmark = pytest.mark.gpu

# (N, in, out, Gn, functions, iterations)
THREE, FOUR = ("sin", "x^2", "exp"), ("sin", "exp", "1/x", "gaussian")
SHAPES = {
    "64x3x5 Gn21 all": (64, 3, 5, 21, ALL, 3),
    "one row": (1, 1, 1, 5, THREE, 3),
    "two rows": (2, 1, 1, 5, THREE, 3),
    "33x2x33 Gn11 partial tiles": (33, 2, 33, 11, FOUR, 3),
    "200x1x65 Gn7 two output tiles": (200, 1, 65, 7, ("cos", "x^3"), 3),
    "1030x2x3 Gn9 row chunks": (1030, 2, 3, 9, THREE, 3),
    "50x2x2 Gn101 default grid": (50, 2, 2, 101, ("sin", "log"), 3),
    "40x2x2 Gn128": (40, 2, 2, 128, ("arctan",), 3),
    "40x2x2 Gn3": (40, 2, 2, 3, ("sqrt",), 3),
    "1030x2x3 Gn9 one iteration": (1030, 2, 3, 9, THREE, 1),
    "64x2x2 Gn9 eight iterations": (64, 2, 2, 9, ("sin", "abs", "silu"), 8),
}


def _inputs(n, fin, fout, seed=1):
    gen = torch.Generator().manual_seed(seed + 7 * n + fin + 3 * fout)
    layer = kagnn_amd.KANLinear(fin, fout, grid_size=5, spline_order=3)
    with torch.no_grad():
        layer.base_weight.copy_(0.3 * torch.randn(fout, fin, generator=gen))
        layer.spline_weight.copy_(0.3 * torch.randn(fout, fin, 8, generator=gen))
        layer.spline_scaler.copy_(1 + 0.5 * torch.randn(fout, fin, generator=gen))
    x = (2 * torch.rand(n, fin, generator=gen) - 1).to(DEV)
    phi = layer.to(DEV).edge_curves(x)
    if fin * fout > 1:
        phi[:, 0, 0] = (0.8 * torch.sin(3.3 * x[:, 0].double() + 0.7) + 1.5).float()
    return x, phi.contiguous()


@functools.lru_cache(maxsize=None)
def _case(key):
    """the device's fit with tables and the restatement of every table on the device's ranges: computed once, shared"""
    n, fin, fout, gn, names, its = SHAPES[key]
    x, phi = _inputs(n, fin, fout)
    fit = ops.symbolic_fit(x, phi, names, grid_number=gn, iterations=its, tables=True)
    torch.cuda.synchronize()
    xs, ys = x.cpu().numpy(), phi.cpu().numpy()
    ranges = fit.ranges.cpu().numpy()
    ref = np.zeros((its, len(names), fout, fin, gn, gn))
    either = np.zeros(ref.shape, dtype=bool)
    worst = 0.0
    for it in range(its):
        for f, name in enumerate(names):
            for o in range(fout):
                for i in range(fin):
                    r = ranges[it, f, o, i]
                    av, bv = axis(r[0], r[1], gn), axis(r[2], r[3], gn)
                    ref[it, f, o, i], either[it, f, o, i] = score_table(name, xs[:, i], ys[:, o, i], av, bv)
                    worst = max(worst, e32(name, xs[:, i], ys[:, o, i], av, bv))
    tol = max(2e-5, 4 * worst)
    print(f"[{key}] E32 {worst:.3e} tol {tol:.3e} either-or share (worst table) {either.mean(axis=(-1, -2)).max():.4f}")
    return dict(x=x, phi=phi, xs=xs, ys=ys, fit=fit, ref=ref, either=either, tol=tol, e32=worst)


# ---------------------------------------------------------------------------------------------------------------- 1. tables
@pytest.mark.parametrize("key", list(SHAPES))
def test_tables_iteration_by_iteration(key):
    n, fin, fout, gn, names, its = SHAPES[key]
    c = _case(key)
    fit, ref, either, tol = c["fit"], c["ref"], c["either"], c["tol"]
    dev = fit.tables.cpu().double().numpy()
    winners, ranges = fit.winners.cpu().numpy(), fit.ranges.cpu().numpy()
    assert dev.shape == ref.shape and winners.shape == ref.shape[:4] and ranges.shape == ref.shape[:4] + (4,)
    diff = np.abs(dev - ref)
    # either-or candidates: at most 2 % of each table on the caller's ranges; on the zoomed tables, whose place the device's winners
    # decide, at most 2 % of each table are either-or candidates that the device scored 0 while fp64 did not (module docstring)
    share = either.mean(axis=(-1, -2))
    missed = (either & (dev == 0) & (ref != 0)).mean(axis=(-1, -2))
    print(f"[{key}] either-or share, worst table per iteration {share.max(axis=(1, 2, 3))}; of them 0 on the device only {missed.max(axis=(1, 2, 3))}")
    print(f"[{key}] either-or share per function (worst table) {dict(zip(names, np.round(share.max(axis=(0, 2, 3)), 4)))}")
    assert share[0].max() <= 0.02, share[0].max()
    assert missed.max() <= 0.02, missed.max()
    strict = np.where(either, 0.0, diff)
    print(f"[{key}] worst strict difference {strict.max():.3e}; either-or candidates {int(either.sum())}, of which scored 0 on the device: "
          f"{int((either & (dev == 0) & (ref != 0)).sum())}")
    assert strict.max() <= tol, np.unravel_index(strict.argmax(), strict.shape)
    assert (either <= ((dev == 0) | (diff <= tol))).all()
    assert (dev >= 0).all() and np.isfinite(dev).all()
    first = np.array([-10, 10, -10, 10], dtype=np.float32)
    for it in range(its):
        for f in range(len(names)):
            for o in range(fout):
                for i in range(fin):
                    w = int(winners[it, f, o, i])
                    assert w == argmax_lowest(dev[it, f, o, i]), (it, f, o, i)                       # exact: its own table's first maximum
                    assert ref[it, f, o, i].reshape(-1)[w] >= ref[it, f, o, i].max() - tol, (it, f, o, i)
                    want = first if it == 0 else zoom(ranges[it - 1, f, o, i], int(winners[it - 1, f, o, i]), gn)
                    assert np.array_equal(ranges[it, f, o, i], want), (it, f, o, i)                  # exact: the candidates are fp64-defined


def test_the_mutations_of_the_restatement_are_noticed():
    """an uncentred S_uy fails the tables on the column with d != 0; the restatement without the degeneracy rule fails the tanh table"""
    key = "64x3x5 Gn21 all"
    n, fin, fout, gn, names, its = SHAPES[key]
    c = _case(key)
    dev, ranges = c["fit"].tables.cpu().double().numpy(), c["fit"].ranges.cpu().numpy()
    f = names.index("sin")
    r = ranges[0, f, 0, 0]
    bent, _ = score_table("sin", c["xs"][:, 0], c["ys"][:, 0, 0], axis(r[0], r[1], gn), axis(r[2], r[3], gn), centred=False)
    assert np.abs(dev[0, f, 0, 0] - bent).max() > 100 * c["tol"]
    f = names.index("tanh")
    r = ranges[0, f, 1, 1]
    loose, either = score_table("tanh", c["xs"][:, 1], c["ys"][:, 1, 1], axis(r[0], r[1], gn), axis(r[2], r[3], gn), rule=False)
    assert np.where(either, 0.0, np.abs(dev[0, f, 1, 1] - loose)).max() > 100 * c["tol"]


# ---------------------------------------------------------------------------------------------------------------- 2. results
@pytest.mark.parametrize("key", list(SHAPES))
def test_results(key):
    n, fin, fout, gn, names, its = SHAPES[key]
    c = _case(key)
    fit, tol = c["fit"], c["tol"]
    plain = ops.symbolic_fit(c["x"], c["phi"], names, grid_number=gn, iterations=its)
    again = ops.symbolic_fit(c["x"], c["phi"], names, grid_number=gn, iterations=its)
    assert plain.tables is None and plain.ranges is None and plain.winners is None and plain.functions == tuple(names)
    assert plain.params.shape == (len(names), fout, fin, 4) and plain.r2.shape == (len(names), fout, fin)
    for a, b in ((plain.params, fit.params), (plain.r2, fit.r2), (again.params, plain.params), (again.r2, plain.r2)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    params, r2 = fit.params.cpu().numpy(), fit.r2.cpu().numpy()
    dev = fit.tables.cpu().numpy()
    winners, ranges = fit.winners.cpu().numpy(), fit.ranges.cpu().numpy()
    worst_c = worst_d = 0.0
    for f, name in enumerate(names):
        for o in range(fout):
            for i in range(fin):
                w, r = int(winners[-1, f, o, i]), ranges[-1, f, o, i]
                a, b, cc, d = params[f, o, i]
                assert a == axis(r[0], r[1], gn)[w // gn] and b == axis(r[2], r[3], gn)[w % gn]
                assert r2[f, o, i] == dev[-1, f, o, i].reshape(-1)[w]
                if r2[f, o, i] == 0:
                    ybar = column_state(c["xs"][:, i], c["ys"][:, o, i])[0]
                    assert w == 0 and cc == 0 and abs(d - ybar) <= 1e-6 * max(abs(ybar), 1e-30), (f, o, i)
                    continue
                c64, d64, suu, syy, ybar = closed_form(name, c["xs"][:, i], c["ys"][:, o, i], a, b)
                ec, ed = abs(cc - c64) / np.sqrt(syy / suu), abs(d - d64) / (abs(ybar) + np.sqrt(syy / n))
                worst_c, worst_d = max(worst_c, ec), max(worst_d, ed)
                assert ec <= tol and ed <= tol, (name, o, i, ec, ed)
    print(f"[{key}] c error / sqrt(Syy/Suu) {worst_c:.3e}; d error / (|ybar| + sqrt(Syy/N)) {worst_d:.3e}; tol {tol:.3e}")


# ---------------------------------------------------------------------------------------------------------------- 3. planted functions
# (a, b) on the first grid of Gn 21 over [-10, 10] (whole numbers) and off it; 1/x: the pole -b/a lies outside [-1, 1].
# sin, tanh, abs and 1/x are ranked against all seven.  x^2, exp and gaussian are ranked against the seven less those that ARE them
# to within the margin on [-1, 1]: exp(-t^2) at a
# small slope is 1 - t^2 (x^2 against gaussian) and at a large shift an exponential, and so is 1 + tanh(t) far to the left.
SEVEN = ("sin", "x^2", "exp", "tanh", "gaussian", "abs", "1/x")
PLANTED = {"sin": ((3.0, 1.0), (3.3, 0.7)), "x^2": ((2.0, 1.0), (1.7, 0.6)), "exp": ((2.0, -1.0), (1.6, -0.4)), "tanh": ((3.0, 1.0), (2.6, 0.3)),
           "gaussian": ((2.0, 1.0), (2.2, 0.9)), "abs": ((3.0, 1.0), (2.7, 0.8)), "1/x": ((1.0, 2.0), (0.9, 1.6))}
ALIASES = {"x^2": ("gaussian",), "exp": ("tanh", "gaussian"), "gaussian": ("x^2",)}


@pytest.mark.parametrize("planted", SEVEN)
def test_planted_functions_rank_first(planted):
    gn, its, n = 21, 3, 64
    names = tuple(f for f in SEVEN if f not in ALIASES.get(planted, ()))
    gen = torch.Generator().manual_seed(5)
    x = 2 * torch.rand(n, 1, generator=gen) - 1
    cols = []
    for k, (a, b) in enumerate(PLANTED[planted]):
        t = (np.float64(a) * x[:, 0].double().numpy() + np.float64(b)).astype(np.float32).astype(np.float64)
        cols.append(torch.from_numpy((0.7 - 0.2 * k) * F64[planted](t) - 0.4 + k))
    phi = torch.stack(cols, dim=1).float().unsqueeze(-1).contiguous()          # [N, 2, 1]: on the grid, off the grid
    fit = ops.symbolic_fit(x.to(DEV), phi.to(DEV), names, grid_number=gn, iterations=its)
    s = SymbolicSuggestion(fit, 2, x)
    xs, ys = x.numpy()[:, 0], phi.numpy()[:, :, 0]
    tol = 2e-5
    for o in range(2):
        ref = {f: fit_reference(f, xs, ys[:, o], gn=gn, iterations=its)["r2"] for f in names}
        ranked = sorted(names, key=lambda f: (-ref[f], SYMBOLIC_LIB[f][0]))
        assert ranked[0] == planted and ref[ranked[0]] - ref[ranked[1]] >= 10 * tol, (planted, o, ref)    # the precondition, on the restatement
        assert s.names[0][o][0] == planted, (o, planted, s.names[0][o][0], ref)
        assert abs(float(s.r2[0, o, 0]) - ref[planted]) <= tol, (o, planted, float(s.r2[0, o, 0]), ref[planted])


def test_an_exact_tie_goes_to_the_lower_index():
    """cos(a x + b) = cos(-a x - b) candidate by candidate: the device's winner is the lower of the two, the flipped rule's is not"""
    gen = torch.Generator().manual_seed(6)
    x = 2 * torch.rand(48, 1, generator=gen) - 1
    y = 0.5 * torch.cos(3.0 * x.double() + 1.0) + 0.25
    gn = 21
    fit = ops.symbolic_fit(x.to(DEV), y.float().reshape(48, 1, 1).to(DEV), ["cos", "x^2"], grid_number=gn, iterations=1, tables=True)
    for f, name in enumerate(("cos", "x^2")):
        table = fit.tables[0, f, 0, 0].cpu().numpy()
        assert np.array_equal(table, table[::-1, ::-1]), name                  # the tie is exact on the device too
        w = int(fit.winners[0, f, 0, 0])
        ref = fit_reference(name, x.numpy()[:, 0], y.float().numpy()[:, 0], gn=gn, iterations=1)
        flipped = fit_reference(name, x.numpy()[:, 0], y.float().numpy()[:, 0], gn=gn, iterations=1, lowest=False)
        assert w == argmax_lowest(table) and w < gn * gn - 1 - w and table.reshape(-1)[w] == table.reshape(-1)[gn * gn - 1 - w]
        assert ref["tables"][0].reshape(-1)[w] >= ref["tables"][0].max() - 2e-5 and flipped["winners"][0] > gn * gn // 2 > w


# ---------------------------------------------------------------------------------------------------------------- 4. edges of the rule
def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def test_edges_of_the_rule():
    n, fin, fout, gn = 40, 3, 4, 9
    names = ("sqrt", "log", "sin")
    x, phi = _inputs(n, fin, fout, seed=9)
    phi[:, 2, 1] = 0.37                                                   # a constant column
    clean = ops.symbolic_fit(x, phi, names, grid_number=gn, iterations=2, tables=True)
    assert bool((clean.tables[:, :, 2, 1] == 0).all()) and bool((clean.r2[:, 2, 1] == 0).all()) and bool((clean.winners[:, :, 2, 1] == 0).all())
    assert bool((clean.params[:, 2, 1, 2] == 0).all()) and torch.allclose(clean.params[:, 2, 1, 3], torch.full((3,), 0.37, device=DEV), rtol=1e-6, atol=0)
    # sqrt / log: exactly 0 wherever some t_n leaves the domain
    xs, ranges, tables = x.cpu().numpy(), clean.ranges.cpu().numpy(), clean.tables.cpu().numpy()
    for f, name in enumerate(names[:2]):
        for it in range(2):
            for o in range(fout):
                for i in range(fin):
                    r = ranges[it, f, o, i]
                    a, b = axis(r[0], r[1], gn).astype(np.float64), axis(r[2], r[3], gn).astype(np.float64)
                    t = (a[:, None, None] * xs[None, None, :, i].astype(np.float64) + b[None, :, None]).astype(np.float32)
                    outside = (t < 0).any(-1) if name == "sqrt" else (t <= 0).any(-1)
                    assert (tables[it, f, o, i][outside] == 0).all(), (name, it, o, i)
    assert bool((clean.tables[0, :2] > 0).any())
    # one NaN in x poisons exactly that column's edges, one Inf in phi exactly that edge
    xb, pb = x.clone(), phi.clone()
    xb[17, 1] = float("nan")
    pb[5, 3, 2] = float("inf")
    bad = ops.symbolic_fit(xb, pb, names, grid_number=gn, iterations=2, tables=True)
    hit = torch.zeros(fout, fin, dtype=torch.bool, device=DEV)
    hit[:, 1] = True
    hit[3, 2] = True
    assert bool((bad.tables[:, :, hit] == 0).all()) and bool((bad.r2[:, hit] == 0).all())
    assert bool(torch.isnan(bad.params[:, hit][..., 2:]).all()) and bool(torch.isfinite(bad.params[:, hit][..., :2]).all())
    for got, want, d in ((bad.params, clean.params, 1), (bad.r2, clean.r2, 1), (bad.tables, clean.tables, 2), (bad.ranges, clean.ranges, 2),
                         (bad.winners, clean.winners, 2)):
        a, b = got.movedim((d, d + 1), (0, 1))[~hit], want.movedim((d, d + 1), (0, 1))[~hit]
        assert torch.equal(_bits(a), _bits(b)), d
    # a strided x gives the bits of its contiguous copy
    wide = torch.zeros(n, fin + 5, device=DEV)
    wide[:, 2:2 + fin] = x
    strided = ops.symbolic_fit(wide[:, 2:2 + fin], phi, names, grid_number=gn, iterations=2)
    assert not wide[:, 2:2 + fin].is_contiguous()
    assert torch.equal(_bits(strided.params), _bits(clean.params)) and torch.equal(_bits(strided.r2), _bits(clean.r2))
    # no rows: zeros, and no library call
    with _NoLaunch():
        empty = ops.symbolic_fit(x[:0], phi[:0], names, grid_number=gn, iterations=2, tables=True)
    assert empty.params.shape == (3, fout, fin, 4) and not bool(empty.params.any()) and not bool(empty.r2.any()) and not bool(empty.tables.any())


# ---------------------------------------------------------------------------------------------------------------- 5. memory safety
@pytest.mark.parametrize("key,tables", [("33x2x33 Gn11 partial tiles", True), ("1030x2x3 Gn9 row chunks", False)])
def test_nothing_is_written_outside_the_outputs_and_the_heap_does_not_matter(monkeypatch, key, tables):
    n, fin, fout, gn, names, its = SHAPES[key]
    x, phi = _inputs(n, fin, fout)

    def run():
        fit = ops.symbolic_fit(x, phi, names, grid_number=gn, iterations=its, tables=tables)
        return [t for t in (fit.params, fit.r2, fit.tables, fit.ranges, fit.winners) if t is not None]
    ref = [t.clone() for t in run()]
    guarded = _GuardedEmpty().install(monkeypatch)
    out = run()
    count = guarded.check(key)
    monkeypatch.undo()
    assert count >= (6 if tables else 3)                                   # params, r2, the workspace (+ tables, ranges, winners)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(out, ref))
    _under_every_pattern(None, run, key)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(run(), ref))


# ---------------------------------------------------------------------------------------------------------------- 6. module level
SEARCH = dict(grid_number=11, iterations=2)
SOME = ("x", "x^2", "sin", "tanh", "exp")


def _same_suggestion(a, b):
    assert a.names == b.names and torch.equal(_bits(a.params), _bits(b.params)) and torch.equal(_bits(a.r2), _bits(b.r2))
    assert torch.equal(a.edge_l1, b.edge_l1) and torch.equal(a.x, b.x)


def _ranked(fit, topk):
    r2, params = fit.r2.cpu().numpy(), fit.params.cpu().numpy()
    ids = [SYMBOLIC_LIB[f][0] for f in fit.functions]
    names, p, r = [], np.zeros((topk,) + r2.shape[1:] + (4,), dtype=np.float32), np.zeros((topk,) + r2.shape[1:], dtype=np.float32)
    for k in range(topk):
        names.append([[None] * r2.shape[2] for _ in range(r2.shape[1])])
    for o in range(r2.shape[1]):
        for i in range(r2.shape[2]):
            order = sorted(range(len(ids)), key=lambda j: (-r2[j, o, i], ids[j]))[:topk]
            for k, j in enumerate(order):
                names[k][o][i], p[k, o, i], r[k, o, i] = fit.functions[j], params[j, o, i], r2[j, o, i]
    return names, p, r


def test_kanlinear_suggest_symbolic():
    torch.manual_seed(21)
    layer = kagnn_amd.KANLinear(3, 4, grid_size=5, spline_order=3).to(DEV)
    x = (2 * torch.rand(90, 3, device=DEV) - 1)
    before = [p.detach().clone() for p in layer.parameters()]
    s = layer.suggest_symbolic(x, functions=("tanh", "x", "sin", "x^2", "exp"), topk=3, **SEARCH)      # (not in library order)
    fit = ops.symbolic_fit(x, layer.edge_curves(x), ("tanh", "x", "sin", "x^2", "exp"), **SEARCH)
    names, p, r = _ranked(fit, 3)
    assert s.names == names and np.array_equal(s.params.cpu().numpy().view(np.int32), p.view(np.int32))
    assert np.array_equal(s.r2.cpu().numpy().view(np.int32), r.view(np.int32))
    assert torch.equal(s.edge_l1, layer.edge_l1(x).detach()) and torch.equal(s.x, x)
    assert all(torch.equal(a, b) for a, b in zip(before, layer.parameters()))
    # max_rows: the documented rows
    sub = layer.suggest_symbolic(x, functions=SOME, topk=2, max_rows=40, **SEARCH)
    _same_suggestion(sub, layer.suggest_symbolic(x[::3], functions=SOME, topk=2, **SEARCH))
    assert sub.x.size(0) == 30 and torch.equal(sub.x, strided_rows(x, 40))
    # the formula is what curves evaluates
    pts = torch.linspace(-1, 1, 9, device=DEV)
    assert s.curves(pts).shape == (9, 4, 3) and isinstance(s.formula(1, 2), str)
    for order in (1, 2, 4):
        other = kagnn_amd.KANLinear(2, 2, grid_size=4, spline_order=order).to(DEV)
        so = other.suggest_symbolic(x[:, :2], functions=SOME, **SEARCH)
        fo = ops.symbolic_fit(x[:, :2].contiguous(), other.edge_curves(x[:, :2].contiguous()), SOME, **SEARCH)
        assert so.names == _ranked(fo, 3)[0]
    with pytest.raises(NotImplementedError):
        kagnn_amd.KANLinear(2, 2, grid_size=4, spline_order=5).to(DEV).suggest_symbolic(x[:, :2])


@pytest.mark.parametrize("layernorm", [True, False])
def test_fastkan_layer_suggest_symbolic(layernorm):
    torch.manual_seed(22)
    layer = kagnn_amd.FastKANLayer(3, 4, use_layernorm=layernorm).to(DEV)
    if layernorm:
        with torch.no_grad():
            layer.layernorm.weight.copy_(1 + 0.3 * torch.randn(3))
            layer.layernorm.bias.copy_(0.2 * torch.randn(3))
    x = torch.randn(70, 3, device=DEV)
    s = layer.suggest_symbolic(x, functions=SOME, topk=2, **SEARCH)
    u = torch.nn.functional.layer_norm(x, (3,), layer.layernorm.weight, layer.layernorm.bias, layer.layernorm.eps) if layernorm else x
    fit = ops.symbolic_fit(u, layer.edge_curves(u, x if layernorm else None), SOME, **SEARCH)
    assert torch.equal(s.x, u) and s.names == _ranked(fit, 2)[0]                  # the fit variable is the normalised input
    assert np.array_equal(s.params.cpu().numpy().view(np.int32), _ranked(fit, 2)[1].view(np.int32))
    assert torch.equal(s.edge_l1, layer.edge_l1(x).detach())
    if layernorm:
        off = layer.suggest_symbolic(x, functions=SOME, topk=2, use_layernorm=False, **SEARCH)
        assert torch.equal(off.x, x) and torch.equal(off.edge_l1, layer.edge_l1(x, False).detach())


def test_chains_walk_their_layers():
    torch.manual_seed(23)
    x = 2 * torch.rand(50, 3, device=DEV) - 1
    for chain in (kagnn_amd.KAN([3, 4, 2]).to(DEV), kagnn_amd.FastKAN([3, 4, 2]).to(DEV)):
        got = chain.suggest_symbolic(x, functions=SOME, topk=2, **SEARCH)
        h = x
        assert len(got) == 2
        for layer, s in zip(chain.layers, got):
            _same_suggestion(s, layer.suggest_symbolic(h, functions=SOME, topk=2, **SEARCH))
            h = layer._forward(h)


def _node_inputs(n=60, e=240, f=6, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, f, generator=gen).to(DEV), torch.randint(0, n, (2, e), generator=gen).to(DEV)


def _toy_models():
    from types import SimpleNamespace
    out = {}
    for conv in ("gin", "gcn"):
        for skip in (True, False):
            def build(conv=conv, skip=skip):
                torch.manual_seed(31)
                x, ei = _node_inputs()
                return kagnn_amd.GKAN_Nodes(conv, 2, 6, 8, 3, skip=skip, grid_size=4, spline_order=3, hidden_layers=2, dropout=0.0).to(DEV), (x, ei)
            out[f"GKAN_Nodes-{conv}-skip{int(skip)}"] = build

    def fast():
        torch.manual_seed(32)
        x, ei = _node_inputs()
        return kagnn_amd.GFASTKAN_Nodes("gin", 2, 6, 8, 3, skip=True, grid_size=4, hidden_layers=2, dropout=0.0).to(DEV), (x, ei)
    out["GFASTKAN_Nodes-gin"] = fast

    def kagin():
        torch.manual_seed(33)
        gen = torch.Generator().manual_seed(3)
        sizes = [12, 15, 10, 13, 10]
        off = np.cumsum([0] + sizes[:-1])
        src = torch.cat([torch.randint(0, s, (3 * s,), generator=gen) + int(o) for s, o in zip(sizes, off)])
        dst = torch.cat([torch.randint(0, s, (3 * s,), generator=gen) + int(o) for s, o in zip(sizes, off)])
        d = SimpleNamespace(edge_index=torch.stack([src, dst]).to(DEV), num_graphs=5,
                            batch=torch.cat([torch.full((s,), b) for b, s in enumerate(sizes)]).to(DEV), x=torch.randn(60, 6, generator=gen).to(DEV))
        return kagnn_amd.KAGIN(2, 6, 8, 3, 2, 4, 3, 0.0).to(DEV), (d,)
    out["KAGIN"] = kagin
    return out


TOYS = _toy_models()


@pytest.mark.parametrize("which", list(TOYS))
def test_suggest_symbolic_over_a_model(which):
    model, args = TOYS[which]()
    model.train()
    layers = {n: m for n, m in model.named_modules()
              if (isinstance(m, kagnn_amd.KANLinear) and m.spline_order <= 4) or isinstance(m, kagnn_amd.FastKANLayer)}
    assert layers
    model.eval()
    with torch.no_grad():
        before = model(*args).clone()
    model.train()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    got = kagnn_amd.suggest_symbolic(model, *args, functions=SOME, topk=2, search=SEARCH, keep_inputs=True)
    assert set(got) == set(layers) and not ops.layer_inputs_visible() and model.training
    assert all(torch.equal(v, state[k]) for k, v in model.state_dict().items())
    # the inputs are those a collect_edge_l1 block sees in the same eval-mode forward: its statistics are edge_l1 of exactly them
    model.eval()
    with torch.no_grad(), kagnn_amd.collect_edge_l1(model) as stats:
        model(*args)
    for name, layer in layers.items():
        s = got[name]
        assert torch.equal(stats[name], layer.edge_l1(s.input).detach()) and torch.equal(s.edge_l1, stats[name].detach()), name
        _same_suggestion(s, layer.suggest_symbolic(s.input, functions=SOME, topk=2, **SEARCH))
    with torch.no_grad():
        after = model(*args)
    assert torch.equal(_bits(after), _bits(before))                          # the fused routes are back, nothing was modified


def test_a_sine_edge_is_reported_as_a_sine():
    """a 2-layer KAN whose edge (1, 2) of the first layer is sin(3 x) (``curve2coeff``, no base branch there) reports sin first.
    The candidate list leaves out cos, which IS sin up to the shift b = pi / 2 that the search finds."""
    names = ("x", "x^2", "x^3", "exp", "tanh", "sin", "abs", "gaussian")
    torch.manual_seed(41)
    chain = kagnn_amd.KAN([3, 4, 2], grid_size=12, spline_order=3)
    first = chain.layers[0]
    pts = torch.linspace(-1, 1, 200).unsqueeze(1).expand(-1, 3).contiguous()
    target = torch.zeros(200, 3, 4)
    target[:, 2, 1] = torch.sin(3.0 * pts[:, 2])
    with torch.no_grad():
        first.spline_weight[1, 2] = first.curve2coeff(pts, target)[1, 2]
        first.spline_scaler[1, 2] = 1.0
        first.base_weight[1, 2] = 0.0
    chain = chain.to(DEV)
    first = chain.layers[0]
    x = 2 * torch.rand(128, 3, device=DEV) - 1
    got = chain.suggest_symbolic(x, functions=names, topk=2, grid_number=21, iterations=3)
    xs, ys = x.cpu().numpy()[:, 2], first.edge_curves(x).cpu().numpy()[:, 1, 2]
    assert np.abs(ys - np.sin(3.0 * xs.astype(np.float64))).max() < 1e-3         # the layer really carries the sine
    ref = {f: fit_reference(f, xs, ys, gn=21, iterations=3)["r2"] for f in names}
    ranked = sorted(names, key=lambda f: (-ref[f], SYMBOLIC_LIB[f][0]))
    assert ranked[0] == "sin" and ref["sin"] - ref[ranked[1]] >= 10 * 2e-5, ref  # the precondition, on the restatement
    assert got[0].names[0][1][2] == "sin" and abs(float(got[0].r2[0, 1, 2]) - ref["sin"]) <= 2e-5
    a, b = got[0].params[0, 1, 2, :2].tolist()
    assert abs(abs(a) - 3.0) < 0.05 and "sin(" in got[0].formula(1, 2)
