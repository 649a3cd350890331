"""Fixed symbolic edges on the device: ``ops.symbolic_edges`` (csrc/symbolic_edges.hip), ``KANLinear.fix_symbolic`` / ``unfix_symbolic``,
``kagnn_amd.auto_symbolic`` and the routes of the models around a layer with fixed edges.

Kernel level.  The reference is the formula itself in fp64 torch ops on the CPU,

    y[n,o] = y_in[n,o] + sum over the edges (o, i, f) of c f(a x[n,i] + b) + d,

with autograd for gx, g_affine and the gradient of y_in.  x is uniform in [-1, 1]; the parameters are drawn per function so that the
argument stays inside the domain and off singularities (``draw_affine``).  For ``abs`` / ``sgn`` edges no fp64 argument may lie within
1e-5 of the kink at 0: asserted per case (the seeds were picked on the CPU so that it holds).  y and gx are held to
``helpers.assert_close`` at its default (2e-5 of the tensor's maximum) with no allowance; g_affine -- sums over all rows -- to the same
bound and, ONLY where that fails, to max(that bound, 4 x E32), E32 being the error of the same formula evaluated in fp32 torch on
the CPU; ``FALLBACKS`` lists the cases that needed it (printed by ``test_zz_report``; profiles/symbolic_edges.md records it).

Layer and model level: see the sections below."""
from types import SimpleNamespace

import pytest
import torch

import kagnn_amd
from kagnn_amd import graph_ops, ops
from kagnn_amd.symbolic import SYMBOLIC_LIB
from oracle import kan_oracle as orc
from helpers import TOL, assert_close, must_fail, oracle_kan_linear_fwd_bwd, prenorm_bias_noise
from test_gpu_poison import _GuardedEmpty, _under_every_pattern
from test_subgraph_host import _NoLaunch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = tuple(SYMBOLIC_LIB)
FN = [v[1] for v in SYMBOLIC_LIB.values()]
POSITIVE = ("1/x", "1/x^2", "sqrt", "1/sqrt(x)", "log")
FALLBACKS = []          # (case, E32 / max|want|) of the g_affine checks that needed the 4 x E32 bound
WORST = {}              # tensor kind -> worst error as a fraction of its bound


# ---------------------------------------------------------------------------------- cases and the fp64 reference
def draw_affine(fids, gen):
    rows = []
    u = lambda lo, hi: lo + (hi - lo) * float(torch.rand((), generator=gen))
    for f in fids:
        name = NAMES[f]
        if name in POSITIVE:
            a, b = u(0.3, 1.0), u(2.0, 3.0)
        elif name == "tan":
            a, b = u(0.3, 0.6), u(-0.5, 0.5)
        elif name == "exp":
            a, b = u(-1.5, 1.5), u(-1.5, 1.5)                  # t <= 3
        else:
            a, b = u(-3.0, 3.0), u(-3.0, 3.0)
        c = u(0.3, 1.5) * (1.0 if float(torch.rand((), generator=gen)) < 0.5 else -1.0)
        rows.append([a, b, c, 0.3 * float(torch.randn((), generator=gen))])
    return torch.tensor(rows, dtype=torch.float32).reshape(len(fids), 4)


def all_functions_case(fin, fout):
    """all 19 functions on output 0, one edge on each of the other outputs but the last two"""
    edges = [(0, 3 * f + 1, f) for f in range(19)]
    edges += [(o, (7 * o) % fin, (5 * o) % 19) for o in range(1, fout - 2)]
    return edges


def make_case(name, n, fin, fout, edges, seed):
    gen = torch.Generator().manual_seed(seed)
    if isinstance(edges, int):          # that many random pairs with random functions
        pairs = torch.randperm(fin * fout, generator=gen)[:edges].tolist()
        fids = torch.randint(0, 19, (edges,), generator=gen).tolist()
        edges = [(p // fin, p % fin, f) for p, f in zip(pairs, fids)]
    triples = tuple(sorted(edges))
    c = SimpleNamespace(name=name, n=n, fin=fin, fout=fout, triples=triples, affine=draw_affine([f for _, _, f in triples], gen),
                        x=2.0 * torch.rand(n, fin, generator=gen) - 1.0, y_in=torch.randn(n, fout, generator=gen),
                        gy=torch.randn(n, fout, generator=gen))
    # the precondition of the abs / sgn edges
    for e, (_, i, f) in enumerate(triples):
        if NAMES[f] in ("abs", "sgn"):
            t = c.affine[e, 0].double() * c.x[:, i].double() + c.affine[e, 1].double()
            assert float(t.abs().min()) > 1e-5, (name, e, "an fp64 argument of abs / sgn within 1e-5 of 0: pick another seed")
    return c


CASE_SPECS = {
    "1x1-1": (1, 1, 1, [(0, 0, 11)], 1),
    "63x3-5": (63, 3, 5, [(o, i, (3 * o + i) % 19) for o in range(5) for i in range(3)], 2),
    "64x3-5": (64, 3, 5, [(o, i, (3 * o + i + 4) % 19) for o in range(5) for i in range(3)], 3),
    "65x3-5": (65, 3, 5, [(o, i, (3 * o + i + 9) % 19) for o in range(5) for i in range(3)], 4),
    "257x70-9": (257, 70, 9, all_functions_case(70, 9), 5),
    "1000x64-64": (1000, 64, 64, 400, 6),
    "300x130-5": (300, 130, 5, 40, 7),
    "65x5-130": (65, 5, 130, 30, 8),        # more than 128 outputs: the backward's direct-gy variant
    "8193x6-4": (8193, 6, 4, 8, 9),
    "70001x6-4": (70001, 6, 4, 8, 10),
}
_CASES, _REFS = {}, {}


def case(name):
    if name not in _CASES:
        _CASES[name] = make_case(name, *CASE_SPECS[name])
    return _CASES[name]


def formula(x, triples, affine, y_in=None, fout=None, drop_d=False):
    """the formula in the dtype of x; ``drop_d``: a mutant of the mutation guards"""
    fout = fout if fout is not None else y_in.size(1)
    y = torch.zeros(x.size(0), fout, dtype=x.dtype) if y_in is None else y_in.clone()
    cols = []
    for e, (o, i, f) in enumerate(triples):
        a, b, c, d = affine[e]
        t = a * x[:, i] + b
        v = c * FN[f](t) + (0.0 if drop_d else d)
        cols.append((o, v))
    for o in sorted({o for o, _ in cols}):
        y[:, o] = y[:, o] + sum(v for oo, v in cols if oo == o)
    return y


def reference(c, with_y, dtype=torch.float64):
    key = (c.name, with_y, dtype)
    if key not in _REFS:
        x = c.x.to(dtype).requires_grad_(True)
        aff = c.affine.to(dtype).requires_grad_(True)
        yi = c.y_in.to(dtype).requires_grad_(True) if with_y else None
        y = formula(x, c.triples, aff, yi, c.fout)
        y.backward(c.gy.to(dtype))
        _REFS[key] = SimpleNamespace(y=y.detach(), gx=x.grad, gaff=aff.grad, gyin=None if yi is None else yi.grad)
    return _REFS[key]


def run_op(c, with_y, x=None, rows=None, want_gx=True):
    """forward + backward on the device -> y, gx, g_affine, gradient of y_in"""
    sl = slice(None) if rows is None else slice(*rows)
    edges = ops.SymbolicEdges.from_sorted(c.triples, c.fin, c.fout, DEV)
    xd = (c.x[sl].to(DEV) if x is None else x).requires_grad_(want_gx)
    aff = c.affine.to(DEV).requires_grad_(True)
    yi = c.y_in[sl].to(DEV).requires_grad_(True) if with_y else None
    y = ops.symbolic_edges(xd, edges, aff, c.fout, y=yi)
    y.backward(c.gy[sl].to(DEV))
    return y.detach(), xd.grad, aff.grad, None if yi is None else yi.grad


def note(kind, ratio):
    WORST[kind] = max(WORST.get(kind, 0.0), ratio / TOL)


def check_affine_gradient(c, with_y, got, want, what):
    try:
        note("g_affine", assert_close(got, want, what=what))
        return
    except AssertionError:
        pass
    ref32 = reference(c, with_y, torch.float32)
    e32 = float((ref32.gaff.double() - want).abs().max())
    own = float(want.abs().max())
    err = float((got.double().cpu() - want).abs().max())
    FALLBACKS.append((what, e32 / own))
    print(f"{what}: fp32 bound missed (err {err / own:.3e} of max); E32 {e32 / own:.3e} of max")
    assert err <= max(TOL * own, 4.0 * e32), (what, err / own, e32 / own)
    note("g_affine (4 x E32)", err / max(TOL * own, 4.0 * e32) * TOL)


# ---------------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize("with_y", [True, False], ids=["y_in", "alone"])
@pytest.mark.parametrize("name", list(CASE_SPECS))
def test_op_against_the_fp64_formula(name, with_y):
    c = case(name)
    ref = reference(c, with_y)
    y, gx, gaff, gyin = run_op(c, with_y)
    what = f"symbolic_edges {name} {'y_in' if with_y else 'alone'}"
    note("y", assert_close(y, ref.y, what=what + " y"))
    note("gx", assert_close(gx, ref.gx, what=what + " gx"))
    check_affine_gradient(c, with_y, gaff, ref.gaff, what + " g_affine")
    if with_y:
        assert torch.equal(gyin.cpu(), c.gy), "the gradient of y is the incoming gradient itself"
    # outputs without an edge: y_in bit for bit, or 0; inputs no edge reads: exactly 0
    used_o, used_i = {o for o, _, _ in c.triples}, {i for _, i, _ in c.triples}
    for o in set(range(c.fout)) - used_o:
        assert torch.equal(y[:, o].cpu(), c.y_in[:, o] if with_y else torch.zeros(c.n)), (what, o)
    for i in set(range(c.fin)) - used_i:
        assert not bool(gx[:, i].any()), (what, i)
    # a second call gives the same bits
    again = run_op(c, with_y)
    for a, b in zip((y, gx, gaff), again):
        assert torch.equal(a, b), what


def test_mutation_guards():
    """the checks above reject: f' of tanh replaced by f, d dropped, ga without its factor x, a list applied in input-major order"""
    c = case("257x70-9")
    ref = reference(c, True)
    x, aff = c.x.double(), c.affine.double()
    e_tanh = next(e for e, (_, _, f) in enumerate(c.triples) if NAMES[f] == "tanh")
    o, i, _ = c.triples[e_tanh]
    a, b, cc, _ = aff[e_tanh]
    t = a * x[:, i] + b
    gx = ref.gx.clone()
    gx[:, i] += c.gy[:, o].double() * cc * a * (torch.tanh(t) - (1 - torch.tanh(t) ** 2))
    must_fail(gx, ref.gx, what="f' of tanh replaced by f")
    must_fail(formula(x, c.triples, aff, c.y_in.double(), drop_d=True), ref.y, what="d dropped")
    gaff = ref.gaff.clone()
    gaff[:, 0] = gaff[:, 1]                                     # sum gy c f' without the factor x
    must_fail(gaff, ref.gaff, what="ga without x")
    by_input = sorted(range(len(c.triples)), key=lambda e: (c.triples[e][1], c.triples[e][0]))
    assert by_input != list(range(len(c.triples)))
    must_fail(formula(x, c.triples, aff[by_input], c.y_in.double()), ref.y, what="input-major list")


def test_column_sliced_x_and_a_wider_y_buffer():
    c = case("1000x64-64")
    ref = reference(c, True)
    wide = torch.full((c.n, c.fin + 7), 3.0, device=DEV)
    wide[:, 3:3 + c.fin] = c.x.to(DEV)
    xs = wide[:, 3:3 + c.fin].detach()                          # a row stride of in + 7 and a base address off the 16-byte grid
    assert not xs.is_contiguous() and xs.data_ptr() % 16 != 0
    y, gx, gaff, _ = run_op(c, True, x=xs)
    plain = run_op(c, True)
    for a, b in zip((y, gx, gaff), plain):
        assert torch.equal(a, b)
    assert_close(y, ref.y, what="sliced x: y")
    # y written into a sentinel-filled wider buffer through the C ABI: the padding stays bit-unchanged
    edges = ops.SymbolicEdges.from_sorted(c.triples, c.fin, c.fout, DEV)
    aff, yi = c.affine.to(DEV), c.y_in.to(DEV)
    for ld in (c.fout + 5, c.fout + 8):                         # the 4-byte and the 16-byte store paths
        buf = torch.full((c.n, ld), -7.25, device=DEV)
        ops._call("kagnn_symbolic_edges_fwd", ops._ptr(xs), xs.stride(0), c.n, c.fin, c.fout, ops._ptr(edges.plan_host),
                  ops._ptr(edges.plan), ops._ptr(aff), ops._ptr(yi), c.fout, ops._ptr(buf), ld, ops._stream())
        assert torch.equal(buf[:, :c.fout], y) and bool((buf[:, c.fout:] == -7.25).all()), ld


@pytest.mark.parametrize("name,r0,r1", [("1000x64-64", 37, 613), ("8193x6-4", 4000, 8193), ("300x130-5", 1, 66)])
def test_rows_do_not_depend_on_their_position(name, r0, r1):
    c = case(name)
    y, gx, _, _ = run_op(c, True)
    ys, gxs, _, _ = run_op(c, True, rows=(r0, r1))
    assert torch.equal(y[r0:r1], ys) and torch.equal(gx[r0:r1], gxs)


@pytest.mark.parametrize("name", ["8193x6-4", "70001x6-4"])
def test_affine_gradient_adds_over_row_chunks(name):
    c = case(name)
    _, _, gaff, _ = run_op(c, False)
    cut = (0, c.n // 3 + 5, 2 * c.n // 3 - 7, c.n)
    parts = sum(run_op(c, False, rows=(lo, hi))[2].double() for lo, hi in zip(cut[:-1], cut[1:]))
    scale = float(reference(c, False).gaff.abs().max())
    assert float((parts - gaff.double()).abs().max()) <= 2e-6 * scale
    assert torch.equal(run_op(c, False)[2], gaff)
    # without gx the parameter gradient is the same bits
    assert torch.equal(run_op(c, False, want_gx=False)[2], gaff)


def test_no_edge_and_no_row_launch_nothing():
    c = case("63x3-5")
    x, yi = c.x.to(DEV), c.y_in.to(DEV)
    none = ops.SymbolicEdges([], c.fin, c.fout, DEV)
    some = ops.SymbolicEdges.from_sorted(c.triples, c.fin, c.fout, DEV)
    aff0 = torch.zeros(0, 4, device=DEV, requires_grad=True)
    with _NoLaunch():
        xr, yr = x.clone().requires_grad_(True), yi.clone().requires_grad_(True)
        y = ops.symbolic_edges(xr, none, aff0, c.fout, y=yr)
        assert torch.equal(y, yi)
        y.backward(c.gy.to(DEV))
        assert torch.equal(yr.grad.cpu(), c.gy) and xr.grad is None
        assert not bool(ops.symbolic_edges(x, none, aff0, c.fout).any())
        aff = c.affine.to(DEV).requires_grad_(True)
        y = ops.symbolic_edges(x[:0], some, aff, c.fout, y=yi[:0])
        assert y.shape == (0, c.fout)
        y.sum().backward()
        assert aff.grad.shape == (len(c.triples), 4) and not bool(aff.grad.any())
    # the C ABI itself: y = y_in (or 0) and zero gradients, by copies and memsets
    out = torch.full((c.n, c.fout), 9.0, device=DEV)
    ops._call("kagnn_symbolic_edges_fwd", ops._ptr(x), c.fin, c.n, c.fin, c.fout, ops._ptr(none.plan_host), ops._ptr(none.plan), None,
              ops._ptr(yi), c.fout, ops._ptr(out), c.fout, ops._stream())
    assert torch.equal(out, yi)
    ops._call("kagnn_symbolic_edges_fwd", ops._ptr(x), c.fin, c.n, c.fin, c.fout, ops._ptr(none.plan_host), ops._ptr(none.plan), None,
              None, 0, ops._ptr(out), c.fout, ops._stream())
    assert not bool(out.any())


def test_nan_poisons_exactly_what_reads_it_and_log_of_a_negative():
    c = case("257x70-9")
    clean = run_op(c, True)
    n_bad, i_bad = 100, 7                                       # input 7 is read by an edge of output 0 and by output 1's edge
    x = c.x.clone()
    x[n_bad, i_bad] = float("nan")
    y, gx, gaff, _ = run_op(c, True, x=x.to(DEV))
    reads = [e for e, (_, i, _) in enumerate(c.triples) if i == i_bad]
    outs = {c.triples[e][0] for e in reads}
    bad_y = torch.isnan(y).nonzero().tolist()
    assert sorted(bad_y) == sorted([n_bad, o] for o in outs)
    keep = ~torch.isnan(y)
    assert torch.equal(y[keep], clean[0][keep])
    bad_e = sorted(set(torch.isnan(gaff).nonzero()[:, 0].tolist()))
    assert bad_e == reads and len(reads) == 2
    others = [e for e in range(len(c.triples)) if e not in reads]
    assert torch.equal(gaff[others], clean[2][others])
    assert torch.isnan(gx).nonzero().tolist() == [[n_bad, i_bad]]
    keep = ~torch.isnan(gx)
    assert torch.equal(gx[keep], clean[1][keep])
    # log of a negative argument: NaN there and nowhere else
    edges = ops.SymbolicEdges([(0, 0, "log"), (1, 1, "sin")], 2, 2, DEV)
    aff = torch.tensor([[1.0, 0.0, 1.0, 0.0], [1.0, 0.0, 1.0, 0.0]], device=DEV)
    x = torch.tensor([[0.5, 0.1], [-0.5, 0.2], [2.0, -0.3]], device=DEV)
    y = ops.symbolic_edges(x, edges, aff, 2)
    assert torch.isnan(y).tolist() == [[False, False], [True, False], [False, False]]
    assert_close(y[[0, 2]], torch.stack([torch.log(x[[0, 2], 0].double()), torch.sin(x[[0, 2], 1].double())], 1), what="log / sin")


def test_heap_patterns_and_guard_bands(monkeypatch):
    for name in ("65x3-5", "65x5-130"):
        c = case(name)
        _under_every_pattern(None, lambda: run_op(c, True)[:3], f"symbolic_edges {name}")
    for name in ("65x3-5", "257x70-9", "300x130-5", "65x5-130", "8193x6-4"):
        c = case(name)
        run_op(c, True)
        guarded = _GuardedEmpty().install(monkeypatch)
        out = run_op(c, True)
        n = guarded.check(name)
        monkeypatch.undo()
        assert n >= 4 and all(bool(torch.isfinite(t).all()) for t in out[:3]), name       # y, gx, g_affine, the workspace


def test_peak_memory_stays_far_below_a_dense_evaluation():
    n, fin, fout = 200_000, 64, 64
    gen = torch.Generator().manual_seed(11)
    triples = tuple((o, i, (o + 3 * i) % 19) for o in range(fout) for i in range(fin))
    aff = draw_affine([f for _, _, f in triples], gen).to(DEV).requires_grad_(True)
    edges = ops.SymbolicEdges.from_sorted(triples, fin, fout, DEV)
    x = (2.0 * torch.rand(n, fin, generator=gen) - 1.0).to(DEV).requires_grad_(True)
    gy = torch.randn(n, fout, generator=gen).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    y = ops.symbolic_edges(x, edges, aff, fout)
    y.backward(gy)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"peak of forward + backward at ({n}, {fin}, {fout}, all edges): {peak / 2**20:.1f} MiB; dense: {n * fout * fin * 4 / 2**20:.1f} MiB")
    assert peak < n * fout * fin * 4 // 2
    assert bool(torch.isfinite(aff.grad).all()) and bool(torch.isfinite(x.grad).all())


# ---------------------------------------------------------------------------------- layer level
def make_layer(fin, fout, G=5, k=3, seed=0, scale=True):
    torch.manual_seed(seed)
    layer = kagnn_amd.KANLinear(fin, fout, grid_size=G, spline_order=k, enable_standalone_scale_spline=scale)
    with torch.no_grad():
        layer.spline_weight.mul_(8.0)                           # edge functions with visible spline parts
    return layer.to(DEV)


def edge_functions64(layer, x):
    """phi[n, o, i] of the layer's SPLINE edges in fp64 from the oracle's bases, as tests/test_gpu_edge_activations.py builds it"""
    x = x.detach().cpu().double()
    B = orc.bspline_bases(x, layer.grid.detach().cpu().double(), layer.spline_order)
    w = layer.spline_weight.detach().cpu().double()
    if layer.enable_standalone_scale_spline:
        w = w * layer.spline_scaler.detach().cpu().double().unsqueeze(-1)
    return torch.einsum("nic,oic->noi", B, w) + torch.nn.functional.silu(x).unsqueeze(1) * layer.base_weight.detach().cpu().double().unsqueeze(0)


SEARCH = dict(grid_number=21, iterations=2)


def test_every_edge_fixed_to_its_best_suggestion():
    layer = make_layer(8, 5)
    x = (2.0 * torch.rand(300, 8, generator=torch.Generator().manual_seed(1)) - 1.0).to(DEV)
    sug = layer.suggest_symbolic(x, topk=1, **SEARCH)
    for o in range(5):
        for i in range(8):
            layer.fix_symbolic(o, i, sug.names[0][o][i], params=sug.params[0, o, i])
    want = torch.zeros(300, 5, dtype=torch.float64)
    xd = x.cpu().double()
    for o in range(5):
        for i in range(8):
            a, b, c, d = sug.params[0, o, i].cpu().double()
            want[:, o] += c * SYMBOLIC_LIB[sug.names[0][o][i]][1](a * xd[:, i] + b) + d
    assert_close(layer(x), want, what="all edges fixed: forward")
    assert layer.symbolic_formula(0).count("x") >= 8


@pytest.mark.parametrize("k,scale", [(3, True), (3, False), (8, True)], ids=["cubic", "no-scaler", "order8"])
def test_three_fixed_edges_beside_the_splines(k, scale):
    fin, fout, n = 6, 4, 300
    layer = make_layer(fin, fout, k=k, seed=2, scale=scale)
    gen = torch.Generator().manual_seed(3)
    x = (1.8 * torch.rand(n, fin, generator=gen) - 0.9).to(DEV)
    gy = torch.randn(n, fout, generator=gen).to(DEV)
    fixes = {(0, 1): ("sin", (2.0, 0.3, 0.7, -0.1)), (2, 5): ("0", None), (3, 0): ("gaussian", (1.5, -0.2, -1.1, 0.4))}
    phi = edge_functions64(layer, x)
    names = ["base_weight", "spline_weight"] + (["spline_scaler"] if scale else [])
    # the unfixed layer's own reference, through the oracle
    p = {n_: getattr(layer, n_) for n_ in names}
    p["spline_scaler"] = layer.spline_scaler if scale else torch.ones(fout, fin, device=DEV)
    p["grid"] = layer.grid
    _, _, gref = oracle_kan_linear_fwd_bwd(x, gy, p, k)
    for (o, i), (name, params) in fixes.items():
        layer.fix_symbolic(o, i, name, params=params)
    want = phi.clone()
    xd = x.cpu().double()
    for (o, i), (name, params) in fixes.items():
        want[:, o, i] = 0.0 if name == "0" else params[2] * SYMBOLIC_LIB[name][1](params[0] * xd[:, i] + params[1]) + params[3]
    xr = x.clone().requires_grad_(True)
    y = layer(xr)
    assert_close(y, want.sum(-1), what=f"3 fixed edges ({k}): forward")
    y.backward(gy)
    at = torch.tensor(sorted(fixes), device=DEV)
    free = layer.symbolic_keep.bool()
    for n_ in names:
        g = getattr(layer, n_).grad
        assert not bool(g[at[:, 0], at[:, 1]].any()), (n_, "a fixed edge's spline parameters must get exactly zero gradient")
        ref = gref[n_].clone()
        ref[at[:, 0].cpu(), at[:, 1].cpu()] = 0.0
        assert_close(g, ref, what=f"3 fixed edges ({k}): {n_}.grad elsewhere")
    assert layer.symbolic_affine.grad.shape == (2, 4) and bool(layer.symbolic_affine.grad.abs().sum() > 0)
    # the views describe the layer as it now is
    if k <= 4:
        assert_close(layer.edge_l1(x), want.abs().mean(0), what="edge_l1 with fixed edges")
        assert_close(layer.edge_curves(x), want, what="edge_curves with fixed edges")
        assert float(layer.edge_l1(x).detach()[2, 5]) == 0.0
    assert int(free.sum()) == fin * fout - 3


def test_fit_on_rows_gives_the_suggestions_parameters():
    layer = make_layer(4, 3, seed=4)
    x = (2.0 * torch.rand(200, 4, generator=torch.Generator().manual_seed(5)) - 1.0).to(DEV)
    sug = layer.suggest_symbolic(x, functions=["sin", "x^2", "tanh"], topk=3, **SEARCH)
    j = sug.fit.functions.index("x^2")
    r2 = layer.fix_symbolic(1, 2, "x^2", x=x, **SEARCH)
    assert torch.equal(layer.symbolic_affine[0], sug.fit.params[j, 1, 2]) and r2 == float(sug.fit.r2[j, 1, 2])


def test_unfix_restores_the_layer_bit_for_bit_and_state_dict_round_trip(monkeypatch):
    layer = make_layer(6, 4, seed=6)
    x = (2.0 * torch.rand(130, 6, generator=torch.Generator().manual_seed(7)) - 1.0).to(DEV)
    before = layer(x).detach()
    calls = []
    real = ops._call
    monkeypatch.setattr(ops, "_call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    layer.fix_symbolic(1, 1, "cos", params=(1.0, 0.5, 0.8, 0.0))
    layer.fix_symbolic(0, 3, "0")
    fixed = layer(x).detach()
    assert "kagnn_symbolic_edges_fwd" in calls and not torch.equal(fixed, before)
    other = kagnn_amd.KANLinear(6, 4).to(DEV)
    other.load_state_dict(layer.state_dict())
    assert torch.equal(other(x), fixed)
    moved = kagnn_amd.KANLinear(6, 4)
    moved.load_state_dict(layer.state_dict())                   # loaded on the CPU, then moved
    assert torch.equal(moved.to(DEV)(x), fixed)
    layer.unfix_symbolic(1, 1)
    layer.unfix_symbolic(0, 3)
    del calls[:]
    assert torch.equal(layer(x), before)
    assert "kagnn_symbolic_edges_fwd" not in calls and any(n.startswith("kagnn_kan_") for n in calls)


def test_training_the_four_numbers():
    def run():
        torch.manual_seed(0)
        layer = kagnn_amd.KANLinear(1, 1).to(DEV)
        layer.fix_symbolic(0, 0, "sin", params=(1.7, 0.1, 0.8, 0.1))
        assert [n for n, _ in layer.named_parameters()] == ["base_weight", "spline_weight", "spline_scaler", "symbolic_affine"]
        x = torch.linspace(-1, 1, 257, device=DEV).unsqueeze(1)
        target = torch.sin(2.0 * x + 0.3)
        opt = torch.optim.Adam([layer.symbolic_affine], lr=0.02)
        losses = []
        for _ in range(5):
            opt.zero_grad()
            loss = ((layer(x) - target) ** 2).mean()
            loss.backward()
            opt.step()
            losses.append(float(loss))
        return losses, layer.symbolic_affine.detach().clone()
    l1, p1 = run()
    l2, p2 = run()
    assert all(b < a for a, b in zip(l1[:-1], l1[1:])), l1
    assert l1 == l2 and torch.equal(p1, p2)


def test_routes_that_do_not_take_fixed_edges_raise():
    from kagnn_amd.sharded import ShardedKANLinear
    layer = make_layer(8, 8, seed=8)
    layer.fix_symbolic(0, 0, "x", params=(1, 0, 1, 0))
    with pytest.raises(NotImplementedError, match="fixed symbolic edges"):
        ShardedKANLinear(layer, 0, 2)                           # the shard every sharded layer, the RCCL ones included, is built from
    x = torch.zeros(4, 8, device=DEV)
    with pytest.raises(Exception, match="fixed symbolic edges|Observed exception"):       # (dynamo wraps what the traced forward raises)
        torch.compile(layer, fullgraph=True)(x)


# ---------------------------------------------------------------------------------- model level
# One edge of one convolution's first KANLinear gets zero spline coefficients and is fixed to silu with (1, 0, base_weight[o,i], 0):
# mathematically the unfixed model on that state_dict, so the existing fp64 oracle models are the reference.
MODEL_TOL = 1e-4
EDGE = (1, 2)
FUSED = ("gin_kan_layer", "gine_kan", "kagin_model", "pack_chain", "fwd_parts")


class _CallLog:
    def __init__(self, monkeypatch):
        self.names, real = [], ops._call
        logged = lambda name, *a: (self.names.append(name), real(name, *a))[1]
        monkeypatch.setattr(ops, "_call", logged)
        monkeypatch.setattr(graph_ops, "_call", logged)         # (graph_ops imported the function by name)

    def take(self):
        got, self.names[:] = list(self.names), []
        return got


def _fused(names):
    return [n for n in names if any(tag in n for tag in FUSED)]


def _work(names):
    """the calls of a step without what the host layer caches across steps (size queries, weight packs)"""
    return [n for n in names if not n.endswith("_bytes") and "pack" not in n]


def _first_kanlinear(module):
    return next(m for m in module.modules() if isinstance(m, kagnn_amd.KANLinear))


def _fix_one_edge_and_compare(model, layer_name, run, oracle, log, what, limits=None):
    """``run()`` -> (logits, backward done); ``oracle()`` -> (logits64, {name: grad64}) of the unfixed model on the same state.
    ``limits``: {part of an entry point's name: how many such calls the step with the fixed edge may make} -- for a model whose one
    call covers everything before the fix, so that the layers around the fixed one then run MORE fused calls than before, not fewer"""
    layer = dict(model.named_modules())[layer_name]
    o, i = EDGE
    with torch.no_grad():
        layer.spline_weight[o, i].zero_()
    want, wants = oracle()
    run()                                                       # (first use: the graph's structures, size queries, packs)
    model.zero_grad(set_to_none=True)
    log.take()
    untouched = run().detach().clone()
    calls_before = log.take()
    assert "kagnn_symbolic_edges_fwd" not in calls_before
    unfixed_c = float(layer.base_weight.grad[o, i])
    layer.fix_symbolic(o, i, "silu", params=(1.0, 0.0, float(layer.base_weight[o, i]), 0.0))
    model.zero_grad(set_to_none=True)
    log.take()
    out = run()
    calls_fixed = log.take()
    assert "kagnn_symbolic_edges_fwd" in calls_fixed and "kagnn_symbolic_edges_bwd" in calls_fixed, what
    if limits is not None:
        for tag, most in limits.items():
            assert sum(tag in n for n in calls_fixed) <= most, (what, tag, "the fixed layer still ran inside a fused entry point", calls_fixed)
    elif _fused(calls_before):
        assert len(_fused(calls_fixed)) < len(_fused(calls_before)), (what, "the fixed layer still ran inside a fused entry point")
    assert_close(out, want, MODEL_TOL, what=f"{what}: logits")
    checked = 0
    for name, prm in model.named_parameters():
        if name.endswith("symbolic_affine"):
            continue
        ref = wants[name].clone()
        if name.startswith(layer_name + ".") and name.split(".")[-1] in ("base_weight", "spline_weight", "spline_scaler"):
            assert not bool(prm.grad[o, i].any()), (what, name)
            ref[o, i] = 0.0                                     # the fixed edge's gradient now belongs to (a, b, c, d)
        assert_close(prm.grad, ref, MODEL_TOL, what=f"{what}: {name}.grad", noise=prenorm_bias_noise(name, wants))
        checked += 1
    assert checked >= 6
    bw64 = wants[layer_name + ".base_weight"]
    bound = MODEL_TOL * float(bw64.abs().max())
    gc = float(layer.symbolic_affine.grad[0, 2])
    assert abs(gc - float(bw64[o, i])) <= bound and abs(gc - unfixed_c) <= bound, (what, gc, float(bw64[o, i]), unfixed_c)
    layer.unfix_symbolic(o, i)
    model.zero_grad(set_to_none=True)
    log.take()
    again = run().detach()
    assert _work(log.take()) == _work(calls_before), (what, "the original entry points are back after unfix_symbolic")
    assert torch.equal(again, untouched), what


@pytest.mark.parametrize("skip", [True, False], ids=["skip", "noskip"])
@pytest.mark.parametrize("conv", ["gin", "gcn"])
def test_node_models_with_one_fixed_edge(monkeypatch, conv, skip):
    n, fin, classes = 300, 12, 4
    ei = orc.powerlaw_graph(n, 2000)
    g = ops.GraphIndex(ei.to(DEV), n)
    gen = torch.Generator().manual_seed(31)
    x, gout = 0.5 * torch.randn(n, fin, generator=gen), torch.randn(n, classes, generator=gen) / n
    torch.manual_seed(32)
    model = kagnn_amd.GKAN_Nodes(conv, 2, fin, 16, classes, skip=skip, grid_size=4).to(DEV).train()
    layer_name = next(nm for nm, m in model.named_modules() if nm.startswith("convs.1") and isinstance(m, kagnn_amd.KANLinear))

    def run():
        out = model(x.to(DEV), g)
        out.backward(gout.to(DEV))
        return out

    def oracle():
        frozen = ("grid", "eps", "running_mean", "running_var", "num_batches_tracked")      # (helpers.oracle_node_model_fwd_bwd, with skip)
        st = {q: (v.detach().cpu().double().requires_grad_(True) if v.is_floating_point() and not q.endswith(frozen)
                  else v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for q, v in model.state_dict().items()}
        want = orc.node_model_forward(x.double(), ei, st, "kan", conv, 2, 3, skip=skip)
        want.backward(gout.double())
        return want.detach(), {q: v.grad for q, v in st.items() if v.is_floating_point() and v.requires_grad}

    _fix_one_edge_and_compare(model, layer_name, run, oracle, _CallLog(monkeypatch), f"GKAN_Nodes {conv} skip={skip}")


def test_kagin_with_one_fixed_edge(monkeypatch):
    gen = torch.Generator().manual_seed(33)
    graphs, per = 4, 50
    ptr = torch.arange(graphs + 1) * per
    ei = torch.cat([torch.randint(0, per, (2, 200), generator=gen) + int(ptr[k]) for k in range(graphs)], dim=1)
    x = 0.5 * torch.randn(graphs * per, 7, generator=gen)
    batch = torch.repeat_interleave(torch.arange(graphs), per)
    data = SimpleNamespace(x=x.to(DEV), edge_index=ei.to(DEV), batch=batch.to(DEV), ptr=ptr.to(DEV), num_graphs=graphs)
    gout = torch.randn(graphs, 3, generator=gen)
    torch.manual_seed(34)
    model = kagnn_amd.KAGIN(2, 7, 16, 3, 2, 4, 3, 0.0).to(DEV).train()
    layer_name = next(nm for nm, m in model.named_modules() if nm.startswith("conv.1") and isinstance(m, kagnn_amd.KANLinear))

    def run():
        out = model(data)
        out.backward(gout.to(DEV))
        return out

    def oracle():
        frozen = ("grid", "eps", "running_mean", "running_var", "num_batches_tracked")
        st = {q: (v.detach().cpu().double().requires_grad_(True) if v.is_floating_point() and not q.endswith(frozen)
                  else v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for q, v in model.state_dict().items()}
        want = orc.graph_classification_forward(x.double(), ei, batch, graphs, st, "kan", "gin", 2, 3)
        want.backward(gout.double())
        return want.detach(), {q: v.grad for q, v in st.items() if v.is_floating_point() and v.requires_grad}

    _fix_one_edge_and_compare(model, layer_name, run, oracle, _CallLog(monkeypatch), "KAGIN")


# the fixed edge's place -> what the step with it may still run: never the whole-model call; with the edge in a convolution not the
# stack call either, and the one-call layer node for the OTHER convolution only; with it in the read-out no chain pack, and the convolutions as the ONE stack call each way
REGRESSION_PLACES = {
    "conv.1": ("conv.1.nn.layers.0", {"kagin_model": 0, "gine_kan_stack": 0, "gine_kan_layer_fwd": 1, "gine_kan_layer_bwd": 1}),
    "read-out": ("kan.layers.0", {"kagin_model": 0, "pack_chain": 0, "gine_kan_stack_fwd": 1, "gine_kan_stack_bwd": 1, "gine_kan_layer": 0}),
}


@pytest.mark.parametrize("place", list(REGRESSION_PLACES))
def test_kagin_regression_with_one_fixed_edge(monkeypatch, place):
    """``KAGINRegression`` with embedding encoders runs as ONE library call each way (``kagnn_kagin_model_fwd / _bwd``) before the fix and
    after ``unfix_symbolic``, and must leave that call -- and the stack call, for an edge in a convolution -- while the edge is fixed"""
    layer_name, limits = REGRESSION_PLACES[place]
    gen = torch.Generator().manual_seed(37)
    graphs, per, H = 4, 12, 16
    ptr = torch.arange(graphs + 1) * per
    ei = torch.cat([torch.randint(0, per, (2, 30), generator=gen) + int(ptr[k]) for k in range(graphs)], dim=1)
    x = torch.randint(0, 21, (graphs * per, 1), generator=gen)
    ea = torch.randint(0, 4, (ei.size(1),), generator=gen)
    batch = torch.repeat_interleave(torch.arange(graphs), per)
    data = SimpleNamespace(x=x.to(DEV), edge_index=ei.to(DEV), edge_attr=ea.to(DEV), batch=batch.to(DEV), ptr=ptr.to(DEV), num_graphs=graphs)
    gout = torch.randn(graphs, 1, generator=gen)
    torch.manual_seed(38)
    model = kagnn_amd.KAGINRegression(1, 1, 2, H, 2, 4, 3, 1, 0.0, True)
    model.atom_encoder = kagnn_amd.graph_models.AtomEncoder(H, [21])
    model.bond_encoder.bond_embedding_list = torch.nn.ModuleList([torch.nn.Embedding(4, H)])
    model = model.to(DEV).train()
    assert isinstance(dict(model.named_modules())[layer_name], kagnn_amd.KANLinear)
    log = _CallLog(monkeypatch)

    def run():
        out = model(data)
        out.backward(gout.to(DEV))
        return out

    def oracle():
        frozen = ("grid", "eps", "running_mean", "running_var", "num_batches_tracked")
        st = {q: (v.detach().cpu().double().requires_grad_(True) if v.is_floating_point() and not q.endswith(frozen)
                  else v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for q, v in model.state_dict().items()}
        want = orc.graph_regression_forward(x, ei, ea.view(-1, 1), batch, graphs, st, "kan", 2, 3)
        want.backward(gout.double())
        return want.detach(), {q: v.grad for q, v in st.items() if v.is_floating_point() and v.requires_grad}

    run()
    model.zero_grad(set_to_none=True)
    first = log.take()
    assert "kagnn_kagin_model_fwd" in first and "kagnn_kagin_model_bwd" in first, first     # this shape runs the whole-model call
    _fix_one_edge_and_compare(model, layer_name, run, oracle, log, f"KAGINRegression {place}", limits=limits)


def test_auto_symbolic_applies_the_rule_to_the_suggestions():
    torch.manual_seed(35)
    model = kagnn_amd.KAN([3, 4, 2], grid_size=4).to(DEV)
    with torch.no_grad():
        for l in model.layers:
            l.spline_weight.mul_(6.0)
        first = model.layers[0]
        first.base_weight[0, 1] = 0.0                           # a dead edge
        first.spline_weight[0, 1] = 0.0
        first.base_weight[2, 0] = 0.8                           # an edge that is a formula already: 0.8 silu(x)
        first.spline_weight[2, 0] = 0.0
    x = (2.0 * torch.rand(400, 3, generator=torch.Generator().manual_seed(36)) - 1.0).to(DEV)
    r2_thr, dead_thr = 0.999, 1e-4
    sug = kagnn_amd.suggest_symbolic(model, x, topk=1, search=SEARCH)
    expect = {}
    for name, s in sug.items():
        rows = []
        for o in range(s.r2.size(1)):
            for i in range(s.r2.size(2)):
                if float(s.edge_l1[o, i]) < dead_thr:
                    rows.append((o, i, "0", None))
                elif float(s.r2[0, o, i]) >= r2_thr:
                    rows.append((o, i, s.names[0][o][i], float(s.r2[0, o, i])))
        expect[name] = rows
    pieces = {name: (s.x.cpu().double(), s.params[0].cpu().double(), s.names[0]) for name, s in sug.items()}
    before = model(x).detach()
    report = kagnn_amd.auto_symbolic(model, x, r2_threshold=r2_thr, dead_threshold=dead_thr, search=SEARCH)
    assert report == expect
    assert (0, 1, "0", None) in report["layers.0"] and any(r[:2] == (2, 0) and r[2] != "0" for r in report["layers.0"])
    assert any((o, i) not in model.layers[0].fixed_edges() for o in range(4) for i in range(3)), "some edge stays a spline"
    for name, rows in report.items():
        layer = dict(model.named_modules())[name]
        assert layer.fixed_edges() == {(o, i): fn for o, i, fn, _ in rows}
    # the logits are the fp64 evaluation of the pieces: splines where nothing was fixed, formulas elsewhere
    h = x.cpu().double()
    for name, layer in (("layers.0", model.layers[0]), ("layers.1", model.layers[1])):
        B = orc.bspline_bases(h, layer.grid.detach().cpu().double(), 3)
        w = layer.spline_weight.detach().cpu().double() * layer.spline_scaler.detach().cpu().double().unsqueeze(-1)
        phi = torch.einsum("nic,oic->noi", B, w) + torch.nn.functional.silu(h).unsqueeze(1) * layer.base_weight.detach().cpu().double()
        _, params, names = pieces[name]
        for o, i, fn, _ in report[name]:
            a, b, c, d = params[o, i]
            phi[:, o, i] = 0.0 if fn == "0" else c * SYMBOLIC_LIB[fn][1](a * h[:, i] + b) + d
        h = phi.sum(-1)
    assert_close(model(x), h, what="auto_symbolic: logits against the fp64 pieces")
    assert not torch.equal(model(x), before)
    with pytest.raises(TypeError):
        kagnn_amd.auto_symbolic(model, x)                       # both thresholds are required


def test_zz_report():
    print("worst error as a fraction of each bound:", {k: f"{v:.3f}" for k, v in sorted(WORST.items())})
    print("g_affine checks that needed the 4 x E32 bound:", FALLBACKS or "none")
