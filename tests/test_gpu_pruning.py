"""Attribution and pruning on the device: ``ops.kan_edge_moments`` (csrc/kan_edge.hip), ``KANLinear.edge_stats``, ``KAN.attribute`` /
``keep_nodes`` / ``prune_nodes`` / ``prune_edges`` / ``prune`` and ``kagnn_amd.attribute`` / ``prune`` / ``apply_pruning``, against fp64
restatements built from ``oracle.kan_oracle.bspline_bases`` (tests/pruning_ref.py).

Bounds.  ``mean`` and ``sqrt(m2 / N)`` at ``helpers.assert_close``'s default (2e-5 of the reference tensor's maximum, 1e-4 relative on
its large elements).  ``sqrt(m2 / N)`` alone may instead meet ``max(bound, 4 x E32)`` where the plain bound failed, ``E32`` being the
error of a TWO-pass fp32 torch evaluation of the same quantity on the CPU: such cases are printed and listed in ``ALLOWANCE_USED``.
Pruning decisions are checked only on inputs whose every score lies outside ``[threshold / 3, 3 x threshold]`` (asserted on the fp64
restatement), so rounding cannot flip one."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kagnn_amd
from kagnn_amd import ops
from oracle import kan_oracle as orc
from helpers import TOL, assert_close, must_fail
import pruning_ref as pr
from test_gpu_edge_activations import FUSED_ENTRY_POINTS, _graph_batch, _node_inputs, _timed, dev_args, make_case
from test_gpu_poison import _guard_case, _heap_case
from test_gpu_poison_families import _ran, _randn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(1, 1, 1, 5, 3), (2, 3, 2, 5, 1), (64, 4, 65, 5, 3), (257, 33, 7, 8, 2), (1000, 64, 64, 5, 3), (300, 5, 130, 32, 4),
          (130, 5, 70, 45, 1)]            # the last: the 48-knot limit
SHAPE_IDS = ["%dx%d-%d_G%dk%d" % s for s in SHAPES]
ALLOWANCE_USED = []


# ---------------------------------------------------------------------------------- the kernel against fp64
def moments(c, x=None, **kw):
    return ops.kan_edge_moments((c.x if x is None else x).to(DEV), *dev_args(c), **kw)


def reference(c, x=None, chunk=4096):
    """(mean, m2) in fp64 by two passes over row chunks (the [N, out, in] tensor at once would not fit for the long cases)"""
    x = c.x if x is None else x
    n = x.size(0)
    phi = lambda r: pr.phi_of(x[r:r + chunk], c.knots, c.k, c.bw, c.sw, c.sc)
    mean = sum(phi(r).sum(0) for r in range(0, n, chunk)) / max(n, 1)
    return mean, sum((phi(r) - mean).square().sum(0) for r in range(0, n, chunk))


def e32_of(c, x, want_std, chunk=4096):
    """max error of the two-pass fp32 torch evaluation of sqrt(m2 / N) on the CPU"""
    n = x.size(0)
    phi = lambda r: pr.phi_of(x[r:r + chunk], c.knots, c.k, c.bw, c.sw, c.sc, torch.float32)
    mean = sum(phi(r).sum(0) for r in range(0, n, chunk)) / n
    std = (sum((phi(r) - mean).square().sum(0) for r in range(0, n, chunk)) / n).sqrt()
    return float((std.double() - want_std).abs().max())


def check_moments(c, got, what, x=None):
    x = c.x if x is None else x
    n = x.size(0)
    mean, m2 = got
    want_mean, want_m2 = reference(c, x)
    assert mean.shape == m2.shape == (c.fout, c.fin) and mean.dtype == m2.dtype == torch.float32
    r1 = assert_close(mean, want_mean, what=f"mean {what}")
    got_std, want_std = (m2.double().cpu() / n).sqrt(), (want_m2 / n).sqrt()
    try:
        r2 = assert_close(got_std, want_std, what=f"sqrt(m2/N) {what}")
    except AssertionError:
        e32 = e32_of(c, x, want_std)
        own = float(want_std.abs().max())
        ALLOWANCE_USED.append((what, e32 / own))
        print(f"sqrt(m2/N) {what}: the plain bound failed; two-pass fp32 error E32 = {e32 / own:.3e} of the maximum")
        r2 = assert_close(got_std, want_std, what=f"sqrt(m2/N) {what} [max(bound, 4 x E32)]", noise=max(0.0, 4 * e32 - TOL * own), elementwise=False)
    print(f"{what}: mean at {r1 / TOL:.3f} of its bound, sqrt(m2/N) at {r2 / TOL:.3f} of the plain bound")


@pytest.mark.parametrize("jitter", [False, True], ids=["uniform", "per-feature"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_moments_match_fp64(shape, jitter):
    c = make_case(*shape, jitter=jitter)
    check_moments(c, moments(c), f"{shape} jitter={jitter}")


@pytest.mark.parametrize("variant", ["no_scaler", "no_base", "column_slice"])
def test_moments_optional_operands_and_strided_rows(variant):
    c = make_case(257, 33, 7, 8, 2, seed=2, scaler=variant != "no_scaler", base=variant != "no_base")
    if variant == "column_slice":
        wide = torch.randn(c.n, c.fin + 9, generator=torch.Generator().manual_seed(5)).to(DEV)
        wide[:, 4:4 + c.fin] = c.x.to(DEV)
        x = wide[:, 4:4 + c.fin]
        assert not x.is_contiguous()
        got = ops.kan_edge_moments(x, *dev_args(c))
        assert all(torch.equal(a, b) for a, b in zip(got, moments(c)))
    else:
        got = moments(c)
    check_moments(c, got, variant)


def test_outputs_with_a_leading_dimension_are_written_inside_their_block_only():
    c = make_case(300, 5, 70, 5, 3, seed=9)
    bufs = [torch.full((c.fout + 2, c.fin + 3), -777.0, device=DEV) for _ in range(2)]
    moments(c, out=tuple(b[1:1 + c.fout, 2:2 + c.fin] for b in bufs))
    mask = torch.ones_like(bufs[0], dtype=torch.bool)
    mask[1:1 + c.fout, 2:2 + c.fin] = False
    for buf, want in zip(bufs, moments(c)):
        assert torch.equal(buf[1:1 + c.fout, 2:2 + c.fin], want)
        assert bool((buf[mask] == -777.0).all())


def _merge(a, b):
    """Chan's pairwise merge of (n, mean, m2) in fp64"""
    (na, ma, sa), (nb, mb, sb) = a, b
    d = mb - ma
    n = na + nb
    return n, ma + d * (nb / n), sa + sb + d * d * (na * nb / n)


def test_many_slabs_and_a_ragged_row_partition():
    c = make_case(70001, 6, 4, 5, 3, seed=4)
    one = moments(c)
    check_moments(c, one, "70001x6-4 over many slabs")
    parts = []
    for a, b in ((0, 1), (1, 30001), (30001, c.n)):                 # ragged: a single row, and two long pieces
        mean, m2 = moments(c, c.x[a:b])
        parts.append((b - a, mean.double().cpu(), m2.double().cpu()))
    n, mean, m2 = _merge(_merge(parts[0], parts[1]), parts[2])
    assert n == c.n
    assert_close(mean, one[0].double(), 2e-6, what="mean merged over a row partition", elementwise=False)
    assert_close(m2, one[1].double(), 2e-6, what="m2 merged over a row partition", elementwise=False)


# ---------------------------------------------------------------------------------- check 2: the offset case
def test_offset_case_keeps_the_scale_where_one_pass_fp32_loses_it():
    """phi ~ 5 +- 0.01 (bw = 0, sw = 5 + 0.01 randn, the bases sum to 1 inside the grid).  The device result meets the bound of the
    kernel checks; ``sum phi^2 - (sum phi)^2 / N`` in fp32 torch on the CPU must FAIL it (a relative loss of ~6e-8 x mean^2 / var)."""
    x, bw, sw, knots = pr.offset_case()
    c = SimpleNamespace(n=x.size(0), fin=4, fout=4, G=5, k=3, x=x, bw=bw, sw=sw, sc=None, knots=knots, jitter=False)
    check_moments(c, moments(c), "offset case 70001x4-4")
    mean, want, naive, e32 = pr.offset_reference(x, bw, sw, knots)
    print(f"offset case: one-pass fp32 error {float((naive.double() - want).abs().max() / want.max()):.3e} of the maximum")
    must_fail(naive, want, what="one-pass fp32 sqrt(m2/N) on the offset case")


# ---------------------------------------------------------------------------------- bitwise and special cases
def _layer_of(c):
    layer = kagnn_amd.KANLinear(c.fin, c.fout, grid_size=c.G, spline_order=c.k)
    with torch.no_grad():
        layer.base_weight.copy_(c.bw); layer.spline_weight.copy_(c.sw); layer.spline_scaler.copy_(c.sc)
    return layer.to(DEV)


def test_two_calls_and_every_precision_mode_give_the_same_bits():
    for jitter in (False, True):
        c = make_case(8193, 20, 70, 5, 3, seed=5, jitter=jitter)
        a, b = moments(c), moments(c)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = make_case(257, 33, 17, 4, 3, seed=3)
    layer, x = _layer_of(c), c.x.to(DEV)
    res = []
    for mode in (None, ops.PREC_SPLIT, ops.PREC_HALF, ops.PREC_FP32):
        layer.precision = mode
        res.append(layer.edge_stats(x))
    for stats in res[1:]:
        assert torch.equal(stats.mean, res[0].mean) and torch.equal(stats.std, res[0].std)


def test_non_finite_rows_poison_exactly_their_column():
    c = make_case(300, 6, 70, 5, 3, seed=6)
    clean = moments(c)
    x = c.x.clone()
    x[5, 2], x[70, 2], x[299, 2] = float("nan"), float("inf"), float("-inf")
    others = [i for i in range(c.fin) if i != 2]
    for got, ref in zip(moments(c, x), clean):
        assert bool(torch.isnan(got[:, 2]).all()) and torch.equal(got[:, others], ref[:, others])
    for row in (0, 17):                                              # row 0 is the pivot row
        for bad in (float("nan"), float("inf"), float("-inf")):
            x = c.x.clone()
            x[row, 4] = bad
            for got in moments(c, x):
                assert bool(torch.isnan(got[:, 4]).all()) and int(torch.isnan(got).sum()) == c.fout, (row, bad)


def test_zero_weights_and_constant_rows_give_exact_zeros():
    c = make_case(257, 9, 17, 4, 3, seed=7)
    c.bw, c.sw = torch.zeros_like(c.bw), torch.zeros_like(c.sw)
    mean, m2 = moments(c)
    assert not bool(mean.any()) and not bool(m2.any())
    c = make_case(257, 9, 17, 4, 3, seed=7)
    x = c.x[:1].expand(300, -1).contiguous()                         # every row the pivot row: no spread at all
    mean, m2 = moments(c, x)
    assert not bool(m2.any())
    assert_close(mean, pr.phi_of(c.x[:1], c.knots, c.k, c.bw, c.sw, c.sc)[0], what="mean of constant rows")


def test_no_rows():
    c = make_case(0, 5, 7, 4, 3, seed=8)
    (mean, m2), names = _timed(lambda: moments(c))
    assert mean.shape == m2.shape == (7, 5) and not bool(mean.any()) and not bool(m2.any())
    assert "kagnn_kan_edge_moments" in names


def _moments_case(n, fin, fout, jitter):
    def build():
        c = make_case(n, fin, fout, 5, 3, seed=13, jitter=jitter)
        args = dev_args(c)
        x = c.x.to(DEV)
        return None, _ran(lambda: list(ops.kan_edge_moments(x, *args)), "kagnn_kan_edge_moments")
    return build


POISON_CASES = {"moments 777x9->70": ("split", _moments_case(777, 9, 70, False), 3),
                "moments 8193x6->5 per-feature knots": ("split", _moments_case(8193, 6, 5, True), 3),
                "moments 1x3->130": ("split", _moments_case(1, 3, 130, False), 3)}


@pytest.mark.parametrize("case", list(POISON_CASES))
def test_moments_blind_to_the_heap(monkeypatch, case):
    _heap_case(monkeypatch, POISON_CASES, case)


@pytest.mark.parametrize("case", list(POISON_CASES))
def test_moments_writes_stay_inside_their_buffers(monkeypatch, case):
    _guard_case(monkeypatch, POISON_CASES, case)


# ---------------------------------------------------------------------------------- layer and chain
def test_edge_stats_with_fixed_edges_and_both_divisors():
    c = make_case(257, 5, 4, 5, 3, seed=21)
    layer = _layer_of(c)
    layer.fix_symbolic(0, 1, "0")
    layer.fix_symbolic(2, 3, "sin", params=(1.3, 0.2, 0.7, 2.5))
    layer.fix_symbolic(1, 0, "tanh", params=(0.9, -0.3, 1.1, -4.0))
    x = c.x.to(DEV)
    phi = pr.layer_phi64(layer, x)
    for unbiased in (True, False):
        stats, names = _timed(lambda: layer.edge_stats(x, unbiased=unbiased))
        assert "kagnn_kan_edge_moments" in names
        assert_close(stats.mean, phi.mean(0), what="edge_stats mean with fixed edges")
        assert_close(stats.std, phi.std(0, unbiased=unbiased), what=f"edge_stats std with fixed edges unbiased={unbiased}")
        assert float(stats.mean[0, 1]) == 0.0 and float(stats.std[0, 1]) == 0.0       # the "0" edge: exactly nothing
    one = layer.edge_stats(x[:1])
    assert bool(torch.isnan(one.std).all()) and bool(torch.isnan(torch.std(x[:1], dim=0)).all())     # as torch.std
    assert not bool(layer.edge_stats(x[:1], unbiased=False).std.any())
    assert_close(one.mean, phi[0], what="edge_stats mean of one row")


ATTRIBUTE_FIELDS = ("edge_std", "out_std", "edge_scores", "node_scores")


def _chain_on_device(chain):
    dev = copy.deepcopy(chain).to(DEV)
    for layer in dev.layers:
        layer.precision = ops.PREC_FP32          # (the layers between the statistics in exact fp32: the bound below is the fp32 one)
    return dev


@pytest.mark.parametrize("widths", [(5, 9, 4), (6, 7, 7, 3), (4, 3)], ids=["5-9-4", "6-7-7-3", "4-3"])
@pytest.mark.parametrize("scored", [False, True], ids=["ones", "out_scores"])
def test_chain_attribute_matches_the_rule_in_fp64(widths, scored):
    chain, gen = pr.random_chain(widths, seed=30 + len(widths))
    x = 0.8 * torch.randn(300, widths[0], generator=gen)
    scores = [0.5 + 0.25 * j for j in range(widths[-1])] if scored else None
    att = _chain_on_device(chain).attribute(x.to(DEV), out_scores=None if scores is None else torch.tensor(scores))
    ref = pr.attribute64(list(chain.layers), x, scores)
    for field in ATTRIBUTE_FIELDS:
        got = getattr(att, field)
        assert len(got) == len(ref[field]) == len(widths) - (field != "node_scores")
        for l, (g, w) in enumerate(zip(got, ref[field])):
            assert g.is_cuda
            assert_close(g, w, what=f"attribute {widths} {field}[{l}]")
    assert att.input_scores is att.node_scores[0]
    # mutation guard: the rule without the / (s_l + 1e-4) normalisation is not what was checked
    wrong = pr.attribute64(list(chain.layers), x, scores, normalise=False)
    must_fail(att.node_scores[0], wrong["node_scores"][0], what="input scores against the rule without normalisation")


def test_prune_nodes_removes_the_planted_dead_units():
    chain, x = pr.planted_chain(0)
    ref = pr.attribute64(list(chain.layers), x)
    assert pr.outside_band(ref["node_scores"][1], 1e-2), ref["node_scores"][1]        # a condition on the inputs: rounding cannot decide
    want_keep = np.nonzero(ref["node_scores"][1] > 1e-2)[0].tolist()
    assert want_keep == [0, 1, 3, 4, 6, 7]
    dev = _chain_on_device(chain)
    old = list(dev.parameters())                                     # (held, so that no new tensor can take an old one's place)
    keep, names = _timed(lambda: dev.prune_nodes(x.to(DEV)))
    assert "kagnn_kan_edge_moments" in names
    assert [k.tolist() for k in keep] == [want_keep]
    l0, l1 = dev.layers
    assert (l0.in_features, l0.out_features, l1.in_features, l1.out_features) == (4, 6, 6, 3)
    assert l0.base_weight.shape == (6, 4) and l0.spline_weight.shape == (6, 4, 8) and l0.spline_scaler.shape == (6, 4)
    assert l1.base_weight.shape == (3, 6) and l1.spline_weight.shape == (3, 6, 8) and l1.spline_scaler.shape == (3, 6) and l1.grid.shape == (6, 12)
    params = dict(dev.named_parameters())
    assert list(params) == [f"layers.{l}.{n}" for l in (0, 1) for n in ("base_weight", "spline_weight", "spline_scaler")]
    assert all(p.requires_grad and p.is_cuda for p in params.values()) and not any(p is q for p in params.values() for q in old)
    fresh = 0.8 * torch.randn(200, 4, generator=torch.Generator().manual_seed(77))
    got = dev(fresh.to(DEV))
    assert_close(got, pr.chain_forward64(list(chain.layers), fresh, zero_out={1: [2, 5]}), what="pruned chain vs the chain with zeroed edges")
    # the removed units carried 1e-4 of an ordinary unit's weight into sums of eight: at most 2 x 1e-4 of the output (3e-4 allowed)
    assert_close(got, pr.chain_forward64(list(chain.layers), fresh), 3e-4, what="pruned chain vs the untouched chain", elementwise=False)


DEAD_EDGES = [(0, 1, 2), (0, 3, 0), (1, 1, 3), (1, 0, 1)]


def test_prune_edges_switches_the_planted_dead_edges_off():
    chain, x = pr.planted_chain(0, widths=(3, 5, 2), dead_units=(), dead_edges=DEAD_EDGES)
    ref = pr.attribute64(list(chain.layers), x)
    assert all(pr.outside_band(e, 3e-2) for e in ref["edge_scores"])
    want = [np.argwhere(e < 3e-2).tolist() for e in ref["edge_scores"]]
    assert want == [[[1, 2], [3, 0]], [[0, 1], [1, 3]]]
    dev = _chain_on_device(chain)
    dev.layers[0].fix_symbolic(3, 0, "sin", params=(1.0, 0.0, 1e-6, 0.0))          # one dead edge is already fixed (and tiny): left alone
    ref = pr.attribute64(list(dev.layers), x)
    assert all(pr.outside_band(e, 3e-2) for e in ref["edge_scores"]) and ref["edge_scores"][0][3, 0] < 1e-2
    want[0].remove([3, 0])
    pruned = dev.prune_edges(x.to(DEV))
    assert [p.tolist() for p in pruned] == want
    assert dev.layers[0].fixed_edges() == {(1, 2): "0", (3, 0): "sin"}
    assert dev.layers[1].fixed_edges() == {(0, 1): "0", (1, 3): "0"}
    assert [p.tolist() for p in dev.prune_edges(x.to(DEV))] == [[], []]            # nothing left to prune
    y = dev(x.to(DEV))
    y.backward(torch.ones_like(y))
    for l, pairs in enumerate(want):
        layer = dev.layers[l]
        for o, i in pairs:
            for name in ("base_weight", "spline_weight", "spline_scaler"):
                g = getattr(layer, name).grad
                assert g is not None and not bool(g[o, i].any()), (l, o, i, name)
        assert bool(layer.base_weight.grad.any())
    assert_close(y, pr.chain_forward64(list(dev.layers), x), what="chain with pruned edges")


def test_five_adam_steps_after_prune():
    chain, x = pr.planted_chain(0, dead_edges=[(0, 1, 2)])
    dev = _chain_on_device(chain)
    xd = x.to(DEV)
    target = torch.randn(x.size(0), 3, generator=torch.Generator().manual_seed(5)).to(DEV)
    keep, edges = dev.prune(xd)
    assert [k.numel() for k in keep] == [6] and sum(e.size(0) for e in edges) >= 1
    opt = torch.optim.Adam(dev.parameters(), lr=1e-2)                # (a NEW optimizer: the Parameters are new)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = F.mse_loss(dev(xd), target)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


def test_keep_nodes_with_per_feature_knots_and_fixed_edges():
    chain, x = pr.per_feature_chain()
    want = pr.chain_forward64(list(chain.layers), x, zero_out={1: [1, 5]})
    dev = _chain_on_device(chain)
    wrong_grid = dev.layers[1].grid[:4].clone()
    dev.keep_nodes([[0, 2, 3, 4]])
    assert dev.layers[0].fixed_edges() == {(2, 0): "0"} and dev.layers[1].fixed_edges() == {(2, 3): "sin"}
    assert dev.layers[1]._knots().shape == (4, 12)
    assert_close(dev(x.to(DEV)), want, what="keep_nodes on per-feature knots")
    # mutation guard: the columns sliced, the grid rows not
    dev.layers[1].grid = wrong_grid
    dev.layers[1].refresh_knots()
    must_fail(dev(x.to(DEV)), want, what="keep_nodes that kept the first grid rows")


# ---------------------------------------------------------------------------------- models
def _kagin64(st, d, training):
    """KAGIN in fp64 from the oracle's pieces, BatchNorm by batch statistics (training) or by the running buffers (eval)"""
    layers = lambda prefix: [{q: st[f"{prefix}layers.{i}.{q}"] for q in ("base_weight", "spline_weight", "spline_scaler", "grid")}
                             for i in range(1 + max(int(k[len(prefix) + 7:].split(".")[0]) for k in st if k.startswith(prefix + "layers.")))]
    h = d.x.double()
    for l in range(2):
        eps = float(st[f"conv.{l}.eps"][0]) if f"conv.{l}.eps" in st else 0.0
        h = orc.gin_conv(h, d.edge_index, lambda t: orc.kan_forward(t, layers(f"conv.{l}.nn."), 3), eps)
        mu, var = (h.mean(0), h.var(0, unbiased=False)) if training else (st[f"bn.{l}.running_mean"], st[f"bn.{l}.running_var"])
        h = (h - mu) / torch.sqrt(var + 1e-5) * st[f"bn.{l}.weight"] + st[f"bn.{l}.bias"]
    return F.log_softmax(orc.kan_forward(orc.global_add_pool(h, d.batch, d.num_graphs), layers("kan."), 3), dim=1)


def _models():
    """name -> builder() -> (model on the device in training mode, its arguments, fp64 oracle forward(state, training), the chain
    that gets planted dead hidden units or None, the layer that gets planted dead edges)"""
    out = {}
    for conv in ("gin", "gcn"):
        for skip in (True, False):
            def build(conv=conv, skip=skip):
                torch.manual_seed(11)
                m = kagnn_amd.GKAN_Nodes(conv, 2, 12, 16, 5, skip=skip, grid_size=5, spline_order=3, hidden_layers=2, dropout=0.0)
                x, ei = _node_inputs()
                xc, eic = x.cpu(), ei.cpu()
                oracle = lambda st, training: orc.node_model_forward(xc.double(), eic, st, "kan", conv, 2, 3, skip=skip, training=training)
                return m.to(DEV).train(), (x, ei), oracle, ("convs.0.nn" if conv == "gin" else None), "lay_out"
            out[f"GKAN_Nodes-{conv}-skip{int(skip)}"] = build

    def kagin():
        torch.manual_seed(12)
        d = _graph_batch()
        dc = SimpleNamespace(**{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in vars(d).items()})
        return (kagnn_amd.KAGIN(2, 7, 16, 3, 2, 4, 3, 0.0).to(DEV).train(), (d,), (lambda st, training: _kagin64(st, dc, training)),
                "conv.0.nn", "kan.layers.1")
    out["KAGIN"] = kagin
    return out


MODELS = _models()
DEAD_UNITS = (3, 11)
MODEL_DEAD_EDGES = ((0, 1), (2, 5))
# a model has some 1500 edges whose scores are spread continuously down to ~1e-3; KAGIN's read-out chain, fed with pooled sums far below
# its grid (where silu is flat), has two dozen more between 1e-8 and 2.2e-5.  The edge threshold sits in the gap between the two
# groups in every model here (asserted below: no score within a factor 3 of it), the planted dead edges far below it
NODE_THRESHOLD, EDGE_THRESHOLD, DEAD_EDGE_SCALE = 1e-2, 1.5e-4, 1e-7


def _chain_names(model):
    inside = {id(l) for m in model.modules() if isinstance(m, kagnn_amd.KAN) for l in m.layers}
    return [n for n, m in model.named_modules() if isinstance(m, kagnn_amd.KAN) or (isinstance(m, kagnn_amd.KANLinear) and id(m) not in inside)]


def _layers_of(module):
    return list(module.layers) if isinstance(module, kagnn_amd.KAN) else [module]


def _state(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


@pytest.mark.parametrize("which", list(MODELS), ids=list(MODELS))
def test_attribute_over_a_model(which):
    model, args, _, _, _ = MODELS[which]()
    call = lambda mod: mod(*args)
    call(model)                                                     # (training mode: the fused routes run and cache what they cache)
    _, names_before = _timed(lambda: call(model))
    before = _state(model)
    model.eval()
    logits = call(model)
    model.train()
    flags = {n: m.training for n, m in model.named_modules()}
    found = kagnn_amd.attribute(model, *args, keep_inputs=True)
    assert not ops.layer_inputs_visible() and ops._edge_collectors() == []
    assert {n: m.training for n, m in model.named_modules()} == flags and all(flags.values())
    for k, v in model.state_dict().items():
        assert torch.equal(v.cpu(), before[k]), k                   # BatchNorm running buffers included
    modules = dict(model.named_modules())
    assert list(found) == _chain_names(model) and found
    for name, att in found.items():
        layers = _layers_of(modules[name])
        assert att.input.shape[1] == layers[0].in_features and len(att.edge_scores) == len(layers)
        again = modules[name].attribute(att.input) if isinstance(modules[name], kagnn_amd.KAN) else kagnn_amd.ekan._attribute_layers(layers, att.input)
        for field in ATTRIBUTE_FIELDS:
            for a, b in zip(getattr(att, field), getattr(again, field)):
                assert torch.equal(a, b), (name, field)
        assert bool((att.node_scores[-1] == 1).all())               # every chain's own outputs are scored 1
    model.eval()
    assert torch.equal(call(model), logits)
    model.train()
    _, names_after = _timed(lambda: call(model))
    assert names_after == names_before                              # the fused entry points are back in use
    print(f"{which}: fused entry points in use afterwards: {sorted(set(names_after) & set(FUSED_ENTRY_POINTS))}")


def _plant(model, chain_name, edge_layer):
    gen = torch.Generator().manual_seed(77)
    modules = dict(model.named_modules())
    with torch.no_grad():
        for m in model.modules():                                   # trained-like sizes: 0.3 randn, scaler 1 + 0.5 randn
            if isinstance(m, kagnn_amd.KANLinear):
                m.base_weight.copy_((0.3 * torch.randn(m.base_weight.shape, generator=gen)).to(DEV))
                m.spline_weight.copy_((0.3 * torch.randn(m.spline_weight.shape, generator=gen)).to(DEV))
                m.spline_scaler.copy_((1.0 + 0.5 * torch.randn(m.spline_scaler.shape, generator=gen)).to(DEV))
        if chain_name is not None:
            second = modules[chain_name].layers[1]
            for u in DEAD_UNITS:
                second.base_weight[:, u] *= 1e-4
                second.spline_scaler[:, u] *= 1e-4
        for o, i in MODEL_DEAD_EDGES:
            modules[edge_layer].base_weight[o, i] *= DEAD_EDGE_SCALE
            modules[edge_layer].spline_scaler[o, i] *= DEAD_EDGE_SCALE


def _expected_report(model, args):
    """the two passes of ``kagnn_amd.prune`` by hand on a copy, every decision taken by the fp64 restatement on the recorded inputs
    and asserted to lie outside the threshold's band"""
    twin = copy.deepcopy(model)
    modules = dict(twin.named_modules())
    keep, edges = {}, {}
    found = kagnn_amd.attribute(twin, *args, keep_inputs=True)
    for name, att in found.items():
        ref = pr.attribute64(_layers_of(modules[name]), att.input)
        interior = ref["node_scores"][1:-1]
        assert all(pr.outside_band(s, NODE_THRESHOLD) for s in interior), name
        keep[name] = [np.nonzero(s > NODE_THRESHOLD)[0].tolist() for s in interior]
        if isinstance(modules[name], kagnn_amd.KAN):
            modules[name].keep_nodes(keep[name])
    for m in twin.modules():
        m.__dict__.pop("_kagnn_model_call_template", None)
    ops._KNOTS_EQUAL.clear()
    found = kagnn_amd.attribute(twin, *args, keep_inputs=True)
    for name, att in found.items():
        ref = pr.attribute64(_layers_of(modules[name]), att.input)
        low = np.sort(np.concatenate([e.reshape(-1) for e in ref["edge_scores"]]))
        print(f"{name}: edge scores below 1e-2: {np.array2string(low[low < 1e-2], precision=2)}")
        assert all(pr.outside_band(e, EDGE_THRESHOLD) for e in ref["edge_scores"]), name
        edges[name] = [np.argwhere(e < EDGE_THRESHOLD).tolist() for e in ref["edge_scores"]]
    return keep, edges


def _embedded_state(model, fresh_state, report):
    """the pruned model's state zero-embedded into the ORIGINAL shapes ("0" edges: base weight and scaler zero), and per parameter
    name of the pruned model the (rows, cols) it occupies there and the mask of its switched-off entries"""
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    modules = dict(model.named_modules())
    where = {}
    for name, entry in report.chains.items():
        layers = _layers_of(modules[name])
        for l, layer in enumerate(layers):
            prefix = f"{name}.layers.{l}." if isinstance(modules[name], kagnn_amd.KAN) else f"{name}."
            rows = entry["keep"][l] if l < len(layers) - 1 else torch.arange(layer.out_features)
            cols = entry["keep"][l - 1] if l > 0 else torch.arange(layer.in_features)
            off = torch.zeros(layer.out_features, layer.in_features, dtype=torch.bool)
            pairs = torch.as_tensor(entry["edges"][l]).reshape(-1, 2)
            off[pairs[:, 0], pairs[:, 1]] = True
            where[prefix] = (rows, cols, off)
    st = {}
    for k, v in fresh_state.items():
        prefix, leaf = k.rsplit(".", 1)[0] + ".", k.rsplit(".", 1)[1]
        if prefix in where and leaf in ("base_weight", "spline_weight", "spline_scaler"):
            rows, cols, off = where[prefix]
            small = sd[k].double().clone()
            if leaf != "spline_weight":
                small[off] = 0.0
            full = torch.zeros(v.shape, dtype=torch.float64)
            full[rows[:, None], cols[None, :]] = small
            st[k] = full
        elif leaf == "grid":
            st[k] = v.double()
        else:
            st[k] = sd[k].double() if sd[k].is_floating_point() else sd[k]
    return st, where


@pytest.mark.parametrize("which", list(MODELS), ids=list(MODELS))
def test_prune_over_a_model(which):
    model, args, oracle, chain_name, edge_layer = MODELS[which]()
    call = lambda mod: mod(*args)
    _plant(model, chain_name, edge_layer)
    call(model)                                                     # the fused routes run once on the old shapes
    fresh_state = _state(model)
    want_keep, want_edges = _expected_report(model, args)
    widths = {n: [_layers_of(m)[0].in_features] + [l.out_features for l in _layers_of(m)] for n, m in model.named_modules() if n in want_keep}

    report = kagnn_amd.prune(model, *args, node_threshold=NODE_THRESHOLD, edge_threshold=EDGE_THRESHOLD)
    assert list(report.chains) == _chain_names(model) == list(want_keep)
    assert all(m.training for m in model.modules())
    for name, entry in report.chains.items():
        assert [k.tolist() for k in entry["keep"]] == want_keep[name], name
        assert [e.tolist() for e in entry["edges"]] == want_edges[name], name
        assert entry["widths_before"] == widths[name]
        after = [widths[name][0]] + [len(k) for k in want_keep[name]] + [widths[name][-1]]
        assert entry["widths_after"] == after == [_layers_of(dict(model.named_modules())[name])[0].in_features] + [l.out_features for l in _layers_of(dict(model.named_modules())[name])]
    if chain_name is not None:
        assert want_keep[chain_name] == [[u for u in range(16) if u not in DEAD_UNITS]]
    last = edge_layer if edge_layer in want_edges else edge_layer.rsplit(".layers.", 1)[0]
    planted = want_edges[last][-1]
    cols = want_keep[last][-1] if want_keep[last] else list(range(64))          # (the read-out chain's hidden units may have been re-indexed)
    assert all([o, cols.index(i)] in planted for o, i in MODEL_DEAD_EDGES), planted

    # the pruned model against the fp64 oracle of the ORIGINAL sizes on the zero-embedded state: eval logits and every gradient
    st, where = _embedded_state(model, fresh_state, report)
    leaves = {k: v.clone().requires_grad_(True) for k, v in st.items()
              if v.is_floating_point() and not k.endswith(("grid", "eps", "running_mean", "running_var"))}
    want = oracle({**st, **leaves}, False)
    upstream = torch.randn(want.shape, generator=torch.Generator().manual_seed(31), dtype=torch.float64)
    (want * upstream).sum().backward()
    model.eval()
    model.zero_grad(set_to_none=True)
    out = call(model)
    (out * upstream.float().to(DEV)).sum().backward()
    assert_close(out, want.detach(), 1e-4, what=f"{which}: eval logits after prune", elementwise=False)
    for name, p in model.named_parameters():
        if p.numel() == 0 or name.endswith(".eps"):
            continue                                                # (symbolic_affine of a layer whose fixed edges are all "0"; GIN's fixed eps)
        g = leaves[name].grad
        prefix = name.rsplit(".", 1)[0] + "."
        if prefix in where and name.rsplit(".", 1)[1] in ("base_weight", "spline_weight", "spline_scaler"):
            rows, cols, off = where[prefix]
            g = g[rows[:, None], cols[None, :]].clone()
            g[off] = 0.0                                            # switched-off entries get exactly zero gradient
            assert not bool(p.grad[off.to(DEV)].any()), name
        assert_close(p.grad, g, 1e-4, what=f"{which}: gradient of {name} after prune", elementwise=False)

    # fused against composed routes
    with kagnn_amd.collect_edge_l1(model):
        composed = call(model)
    assert_close(out, composed, 2e-5, what=f"{which}: fused routes vs composed routes after prune", elementwise=False)

    # a pruned checkpoint in a fresh model of the original sizes
    if chain_name is not None:
        with pytest.raises(RuntimeError, match="size mismatch"):
            MODELS[which]()[0].load_state_dict(model.state_dict())
    fresh = MODELS[which]()[0]
    kagnn_amd.apply_pruning(fresh, report)
    fresh.load_state_dict(model.state_dict())
    fresh.eval()
    assert torch.equal(call(fresh), out)


def test_zz_allowance_report():
    """which kernel cases needed the max(bound, 4 x E32) allowance of sqrt(m2 / N) (profiles/pruning.md states the answer)"""
    print("cases that needed the 4 x E32 allowance:", ALLOWANCE_USED or "none")
