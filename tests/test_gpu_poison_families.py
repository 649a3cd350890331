"""The heap-pattern and guard-band checks of tests/test_gpu_poison.py for the kernel families that file's case list predates:
MLP baselines (linear.hip), spline orders 5..16, per-edge activation norms (KAN and FastKAN), dense attention, grid refinement, the
edge-weight gradient, graph / node classification, graph regression with ``harness.Adam``, the device mini-batch loader, the graph
primitives outside a model, the ``kagnn::*`` library ops called eagerly, the overlapped layer backward and the read-out over parts.

One builder per family, ``build() -> (module or None, run)`` as there; ``run()`` returns EVERY device result of the path (a result
that is not returned is not checked) and, through ``_ran``, asserts from the entry-point timer that the library calls the case is
named for were made -- a case that silently took another route fails instead of testing that route.  ``FAMILIES`` maps each family
to its cases; tests/test_host_cpu.py checks without a GPU that none is empty."""
import copy
from types import SimpleNamespace

import pytest
import torch

import kagnn_amd
from kagnn_amd import harness, ops
from oracle import kan_oracle as orc
from test_gpu_poison import DEV, _GuardedEmpty, _guard_case, _heap_case, _poison, _under_every_pattern   # noqa: F401 (one copy of each)

pytestmark = pytest.mark.gpu


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=_gen(seed)) * scale).to(DEV)


def _ran(run, *entries, prefixes=()):
    """``run`` under an ``ops.EntryPointTimer``: every name of ``entries`` (and some name with each of ``prefixes``) must be among
    the library calls it made"""
    def timed():
        timer = ops.EntryPointTimer()
        ops.set_timer(timer)
        try:
            out = run()
        finally:
            ops.set_timer(None)
        called = {r[0] for r in timer.records}
        missing = [e for e in entries if e not in called] + [p + "*" for p in prefixes if not any(c.startswith(p) for c in called)]
        assert not missing, f"never called: {missing}; called: {sorted(called)}"
        return out
    return timed


def _leaf(t):
    return t.detach().clone().requires_grad_(True)


def _csr(g):
    return [g.rowptr, g.col, g.perm, g.rowptr_t, g.col_t, g.perm_t]


CASES = {}       # name -> (precision mode, build, floor of guarded buffers: 3 unless a raw op allocates fewer)
FAMILIES = {}    # family of the issue's table -> its case names


def _case(family, name, build, mode="split", floor=3):
    assert name not in CASES, name
    CASES[name] = (mode, build, floor)
    FAMILIES.setdefault(family, []).append(name)


# ---------------------------------------------------------------------------------------------------------------- MLP baselines
# linear.hip: the forward / input gradient pick their column tile by the output width (<= 16, 32, 48, 64, else 128), the weight
# gradient its row tile the same way and reduces ceil(N / 256) partial-sum slabs of [out, in + 1] from a workspace (linear_dw_plan:
# a slab is never shorter than 256 rows) -- 777 rows: four slabs, the last of 9 rows; 2049: nine, the last of ONE row; 3: one slab
def _linear(n, fin, fout, bias, relu):
    """returns y, gx, gW (and gb)"""
    def build():
        x, gy = _randn(n, fin, seed=1, scale=0.7), _randn(n, fout, seed=2)
        w0, b0 = _randn(fout, fin, seed=3, scale=0.3), _randn(fout, seed=4, scale=0.3)

        def run():
            xr, w, b = _leaf(x), _leaf(w0), (_leaf(b0) if bias else None)
            y = ops.linear(xr, w, b, relu=relu)
            y.backward(gy)
            return [y, xr.grad, w.grad] + ([b.grad] if bias else [])
        return None, _ran(run, "kagnn_linear_fwd", "kagnn_linear_bwd_input", "kagnn_linear_bwd_weight")
    return build


for _shape in [(777, 40, 7), (2049, 64, 64), (3, 5, 1), (515, 33, 130)]:
    for _bias, _relu in [(True, True), (False, False)]:
        _case("linear", "linear %dx%d->%d%s%s" % (*_shape, " bias" if _bias else "", " relu" if _relu else ""), _linear(*_shape, _bias, _relu))


# ---------------------------------------------------------------------------------------------------------------- orders 5..16
def _high_order(n, fin, fout, grid, order):
    """returns y, gx and the three parameter gradients; every precision request runs and must give the first one's bits"""
    def build():
        assert ops.high_order(order)
        torch.manual_seed(n)
        layer = kagnn_amd.KANLinear(fin, fout, grid_size=grid, spline_order=order).to(DEV)
        x, gy = _randn(n, fin, seed=1, scale=0.6), _randn(n, fout, seed=7)

        def run():
            first = None
            for mode in (ops.PREC_SPLIT, ops.PREC_HALF, ops.PREC_FP32):
                layer.precision = mode
                layer.zero_grad(set_to_none=True)
                xr = _leaf(x)
                y = layer(xr)
                y.backward(gy)
                got = [y, xr.grad] + [p.grad for p in layer.parameters()]
                if first is None:
                    first = got
                assert all(torch.equal(a, b) for a, b in zip(got, first)), f"precision request {mode} changes the bits at order {order}"
            return first
        return layer, _ran(run, "kagnn_kan_linear_fwd", "kagnn_kan_linear_bwd_input", "kagnn_kan_linear_bwd_weight")
    return build


_case("high order", "KANLinear 513x20->33 G4 order 5", _high_order(513, 20, 33, 4, 5))
_case("high order", "KANLinear 300x8->12 G3 order 16", _high_order(300, 8, 12, 3, 16))


# ---------------------------------------------------------------------------------------------------------------- edge norms
def _alone(fn, operands, gS):
    """the gradient of ``fn(*operands)`` for each differentiable operand ALONE (the want_* flags decide which buffers exist)"""
    out = []
    for k, t in enumerate(operands):
        if t is None:
            continue
        args = [_leaf(v) if i == k else v for i, v in enumerate(operands)]
        fn(*args).backward(gS)
        out.append(args[k].grad)
    return out


def _kan_edge(n, fin, fout):
    """returns S, the gradients of (x, base_weight, spline_weight, spline_scaler) requested together, then each requested alone, and
    the sampled curves phi[P, out, in] for shared and per-feature abscissae"""
    def build():
        torch.manual_seed(n)
        layer = kagnn_amd.KANLinear(fin, fout, grid_size=5, spline_order=3).to(DEV)
        x, gS = _randn(n, fin, seed=1, scale=0.6), _randn(fout, fin, seed=2)
        tail = (layer._knots(), 5, 3)
        pts, pts_f = torch.linspace(-1.3, 1.3, 37).to(DEV), _randn(37, fin, seed=3, scale=0.8)
        fn = lambda x_, bw, sw, sc: ops.kan_edge_abs_sum(x_, bw, sw, sc, *tail)

        def run():
            ws = [layer.base_weight.detach(), layer.spline_weight.detach(), layer.spline_scaler.detach()]
            every = [_leaf(x)] + [_leaf(w) for w in ws]
            S = fn(*every)
            S.backward(gS)
            curves = [ops.kan_edge_curves(p, *ws, *tail) for p in (pts, pts_f)]
            return [S] + [t.grad for t in every] + _alone(fn, [x] + ws, gS) + curves
        return layer, _ran(run, "kagnn_kan_edge_abs_sum", "kagnn_kan_edge_abs_sum_bwd", "kagnn_kan_edge_curves")
    return build


def _fastkan_edge(n, fin, fout, layernorm):
    """returns S, the gradients of (x, [ln weight, ln bias,] spline weight, base weight) together, each alone, and the curves with and
    without separate base abscissae"""
    def build():
        torch.manual_seed(n)
        layer = kagnn_amd.FastKANLayer(fin, fout, num_grids=8, use_layernorm=layernorm).to(DEV)
        if layernorm:
            with torch.no_grad():
                layer.layernorm.weight.uniform_(0.5, 1.5)
                layer.layernorm.bias.uniform_(-0.3, 0.3)
        x, gS = _randn(n, fin, seed=1, scale=1.2), _randn(fout, fin, seed=2)
        centers, den = layer.rbf.grid.detach(), float(layer.rbf.denominator)
        eps = float(layer.layernorm.eps) if layernorm else 1e-5
        pts, pts_f = torch.linspace(-2.0, 2.0, 37).to(DEV), _randn(37, fin, seed=3)
        fn = lambda x_, lw, lb, sw, bw: ops.fastkan_edge_abs_sum(x_, lw, lb, sw, bw, centers, den, eps)

        def run():
            ln = [layer.layernorm.weight.detach(), layer.layernorm.bias.detach()] if layernorm else [None, None]
            ws = ln + [layer.spline_linear.weight.detach(), layer.base_linear.weight.detach()]
            every = [_leaf(x)] + [None if w is None else _leaf(w) for w in ws]
            S = fn(*every)
            S.backward(gS)
            curves = [ops.fastkan_edge_curves(pts, ws[2], ws[3], centers, den), ops.fastkan_edge_curves(pts_f, ws[2], ws[3], centers, den, base_points=pts_f * 0.5)]
            return [S] + [t.grad for t in every if t is not None] + _alone(fn, [x] + ws, gS) + curves
        return layer, _ran(run, "kagnn_fastkan_edge_abs_sum", "kagnn_fastkan_edge_abs_sum_bwd", "kagnn_fastkan_edge_curves")
    return build


for _shape in [(1037, 33, 17), (4100, 64, 64)]:
    _case("edge norms", "KAN edge norms %dx%d->%d" % _shape, _kan_edge(*_shape))
    for _ln in (True, False):
        _case("edge norms", "FastKAN edge norms %dx%d->%d%s" % (*_shape, " layernorm" if _ln else ""), _fastkan_edge(*_shape, _ln))


# ---------------------------------------------------------------------------------------------------------------- dense attention
def _attention(B, Q, K, H, c, gate, bias):
    """returns o and the gradients of wq, wk, wv (and bias, gate)"""
    def build():
        hc = H * c
        ts = [_randn(B, Q, hc, seed=1), _randn(B, K, hc, seed=2), _randn(B, K, hc, seed=3)]
        bs, gt, go = _randn(B, Q, K, seed=4, scale=0.2), _randn(B, Q, hc, seed=5), _randn(B, Q, hc, seed=6)

        def run():
            wq, wk, wv = (_leaf(t) for t in ts)
            b, g = (_leaf(bs) if bias else None), (_leaf(gt) if gate else None)
            o = ops.dense_attention(wq, wk, wv, H, c ** -0.5, bias=b, gate=g)
            o.backward(go)
            return [o, wq.grad, wk.grad, wv.grad] + ([b.grad] if bias else []) + ([g.grad] if gate else [])
        return None, _ran(run, "kagnn_attention_fwd", "kagnn_attention_bwd")
    return build


for _shape in [(3, 37, 53, 2, 16), (2, 5, 7, 4, 20)]:
    for _gate in (True, False):
        for _b in (True, False):
            _case("attention", "attention B%d Q%d K%d H%d c%d%s%s" % (*_shape, " gate" if _gate else "", " bias" if _b else ""),
                  _attention(*_shape, _gate, _b))


# ---------------------------------------------------------------------------------------------------------------- grid refinement
def _grid_resize(g0, g1, window):
    """order 2, so 5 -> 11 and 8 -> 3 coefficients are grids of 3 -> 9 and 6 -> 1 intervals; 700 rows x 24 features.  Returns the
    refitted coefficients, the ``untouched`` counts and the dense bases of the rows on the old grid (kan_bsplines)"""
    def build():
        n, fin, fout, k = 700, 24, 10, 2
        x = _randn(n, fin, seed=1, scale=0.7)
        step = lambda g: torch.arange(-k, g + k + 1, dtype=torch.float32) * (2.0 / g) - 1.0
        go = (step(g0).expand(fin, -1) * torch.linspace(0.8, 1.3, fin).unsqueeze(1)).contiguous().to(DEV)
        gn = (step(g1).expand(fin, -1) * torch.linspace(0.7, 1.2, fin).unsqueeze(1)).contiguous().to(DEV)
        sw, sc = _randn(fout, fin, g0 + k, seed=2, scale=0.3), _randn(fout, fin, seed=3)
        win = torch.stack([gn[:, k], gn[:, -k - 1]], dim=1).contiguous() if window else None

        def run():
            fit, untouched = ops.kan_grid_resize(x, go, gn, sw, sc, g0, g1, k, window=win)
            return [fit, untouched, ops.kan_bsplines(x, go, g0, k)]
        return None, _ran(run, "kagnn_kan_grid_resize", "kagnn_kan_bsplines")
    return build


def _regrid(n, fi, fo, G, k, how):
    """``KANLinear.update_grid`` / ``refine(2 G, adaptive=True)`` on a fresh copy of the layer each run (shapes of
    tests/test_gpu_parity.py::test_update_grid_vs_oracle).  Returns the new grid and coefficients (and ``untouched``), then the
    output and every gradient of a step on the moved layer"""
    def build():
        torch.manual_seed(n)
        layer0 = kagnn_amd.KANLinear(fi, fo, grid_size=G, spline_order=k).to(DEV)
        x = ((torch.randn(n, fi, generator=_gen(n + 1)) * torch.linspace(0.3, 2.0, fi) + torch.linspace(-1, 1, fi))).to(DEV)
        gy = _randn(n, fo, seed=5)

        def run():
            layer = copy.deepcopy(layer0)
            extra = [layer.refine(x, 2 * G, adaptive=True)] if how == "refine" else []
            if how == "update":
                layer.update_grid(x)
            xr = _leaf(x)
            y = layer(xr)
            y.backward(gy)
            return [layer.grid, layer.spline_weight.detach()] + extra + [y, xr.grad] + [p.grad for p in layer.parameters()]
        return None, _ran(run, "kagnn_kan_grid_resize", "kagnn_kan_linear_fwd")
    return build


for _g0, _g1 in [(3, 9), (6, 1)]:
    for _w in (True, False):
        _case("grid refinement", "grid resize %d->%d coefficients%s" % (_g0 + 2, _g1 + 2, " window" if _w else ""), _grid_resize(_g0, _g1, _w))
_case("grid refinement", "update_grid 3001x70->5 G8", _regrid(3001, 70, 5, 8, 3, "update"))
_case("grid refinement", "refine adaptive 17x3->2 G3 order 2", _regrid(17, 3, 2, 3, 2, "refine"))


# ---------------------------------------------------------------------------------------------------------------- edge gradient
# aggregate_edge.hip: F % 4 == 0, F <= 256 and aligned rows take the lane-group kernels (F = 64: 16 lanes a row; 40: the same
# with lanes beyond F; 8: two lanes a row, eight edge slots), rows above hub_threshold go through the BY-DESTINATION hub segments
# (the graph as generated has its ~1 000-edge hub there; reversed, the hub is the row every other row gathers); anything else --
# here a column slice starting 4 bytes into a row -- takes the scalar kernel, which has no hub path
def _edge_grad(f, reverse, sliced=False):
    """returns the [E] gradient in original order (dropped self loops exactly 0) and the CSR arrays the run rebuilt"""
    def build():
        n, e = 20_000, 150_000
        ei = orc.powerlaw_graph(n, e, seed=8)
        if reverse:
            ei = ei.flip(0).contiguous()
        ei[:, :30] = torch.arange(30).repeat(2, 1)                   # explicit self loops
        ei = ei.to(DEV)
        wide = f + 8 if sliced else f
        xs, gs = _randn(n, wide, seed=1, scale=0.5), _randn(n, wide, seed=2, scale=0.5)
        x, gout = (xs[:, 1:f + 1], gs[:, 1:f + 1]) if sliced else (xs, gs)
        s_in, s_out = (0.5 + torch.rand(n, generator=_gen(3))).to(DEV), (0.5 + torch.rand(n, generator=_gen(4))).to(DEV)

        def run():
            g = ops.GraphIndex(ei, n)
            assert (g.num_hub_seg > 0) == (not reverse)
            gw = ops.aggregate_edge_grad(x, gout, g, in_scale=s_in, out_scale=s_out, skip_self_loops=True)
            assert not bool(gw[:30].any()), "a dropped self loop's slot is not 0"
            return [gw] + _csr(g)
        return None, _ran(run, "kagnn_aggregate_edge_grad")
    return build


for _f, _rev in [(64, False), (64, True), (40, False), (8, False), (8, True)]:
    _case("edge gradient", "edge gradient F%d%s" % (_f, " reversed" if _rev else " hub segments"), _edge_grad(_f, _rev))
_case("edge gradient", "edge gradient F40 column slice (scalar kernel)", _edge_grad(40, False, sliced=True))


# ---------------------------------------------------------------------------------------------------------------- graph-level loops
def _molecules(B=48, seed=21, classes=None):
    """48 graphs of 9..37 nodes, 2 n + 1 edges each (the batch of test_gpu_poison._graph_level as a flat dataset)"""
    gen = _gen(seed)
    sizes = torch.randint(9, 38, (B,), generator=gen)
    node_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)])
    src, dst = [], []
    for b in range(B):
        nb = int(sizes[b]); eb = 2 * nb + 1
        src.append(torch.randint(0, nb, (eb,), generator=gen) + node_ptr[b]); dst.append(torch.randint(0, nb, (eb,), generator=gen) + node_ptr[b])
    ei = torch.stack([torch.cat(src), torch.cat(dst)])
    n, e = int(node_ptr[-1]), ei.size(1)
    y = torch.randn(B, generator=gen) if classes is None else torch.randint(0, classes, (B,), generator=gen)
    return SimpleNamespace(x=torch.randint(0, 21, (n, 1), generator=gen), edge_index=ei, node_ptr=node_ptr,
                           edge_attr=torch.randint(0, 4, (e,), generator=gen), y=y, G=B)


def _restart(model, state):
    with torch.no_grad():
        for t, t0 in zip(model.state_dict().values(), state):
            t.copy_(t0)
    model.zero_grad(set_to_none=True)


def _graph_classification():
    """two epochs of the classification loop on a dataset built inside the run (its node features are ``degree_one_hot``'s): per
    batch nll_loss with a ClassificationMeter, backward, ``harness.Adam``.  Batches of 20: 20 + 20 + 8.  Returns the degree
    features, every batch loss, the meter's record after each epoch, the evaluation meter's record (reduction='sum', no gradient),
    the parameters and both Adam moments"""
    def build():
        d = _molecules(classes=3)
        torch.manual_seed(5)
        model = kagnn_amd.KAGIN(2, 36, 32, 3, 2, 4, 3, 0.0).to(DEV)
        state = [t.detach().clone() for t in model.state_dict().values()]

        def run():
            _restart(model, state)
            model.train()
            ds = kagnn_amd.DeviceGraphDataset(None, d.edge_index, d.node_ptr, y=d.y, device=DEV, degree_features=36)
            loader = kagnn_amd.DeviceBatchLoader(ds, 20, shuffle=True, generator=_gen(3))
            opt = harness.Adam(model.parameters(), lr=1e-2)
            meter, out = ops.ClassificationMeter(DEV), [ds.storage.x]
            for _ in range(2):
                meter.reset()
                for batch in loader:
                    opt.zero_grad()
                    loss = ops.nll_loss(model(batch), batch.y, accumulate=meter)
                    loss.backward()
                    opt.step()
                    out.append(loss.detach())
                out.append(meter.record.clone())
            model.eval()
            meter.reset()
            with torch.no_grad():
                for batch in kagnn_amd.DeviceBatchLoader(ds, 20):
                    out.append(ops.nll_loss(model(batch), batch.y, reduction="sum", accumulate=meter))
            ops.flush_graph_checks()
            return out + [meter.record] + [p.detach() for p in model.parameters()] + [opt._m, opt._v]
        return model, _ran(run, "kagnn_degree_one_hot", "kagnn_batch_assemble", "kagnn_nll_loss_fwd", "kagnn_nll_loss_bwd", "kagnn_adam_step")
    return build


def _graph_regression():
    """``harness.train_graph_regression`` for two epochs (metered l1_loss, RegressionStop, the best-weights copy_if, Adam) over
    three loaders of one 48-molecule dataset, batches of 20.  Returns the stopper's whole buffer (record and history), the
    weights it leaves and both Adam moments; then the plain l1_loss, its gradient (a ``torch.empty_like``) and the scaled,
    metered evaluation figure with its meter"""
    def build():
        d = _molecules()
        torch.manual_seed(5)
        m = kagnn_amd.KAGINRegression(1, 1, 2, 64, 2, 4, 3, 1, 0.0, True)
        m.atom_encoder = kagnn_amd.graph_models.AtomEncoder(64, [21])
        m.bond_encoder.bond_embedding_list = torch.nn.ModuleList([torch.nn.Embedding(4, 64)])
        m = m.to(DEV)
        state = [t.detach().clone() for t in m.state_dict().values()]
        pred, target, scale = _randn(37, 5, seed=1), _randn(37, 5, seed=2), (0.5 + torch.rand(5, generator=_gen(3))).to(DEV)
        seen = {}
        update = ops.RegressionStop.update

        def run():
            _restart(m, state)
            ds = kagnn_amd.DeviceGraphDataset(d.x, d.edge_index, d.node_ptr, edge_attr=d.edge_attr, y=d.y, device=DEV)
            loaders = [kagnn_amd.DeviceBatchLoader(ds, 20, shuffle=True, generator=_gen(3)), kagnn_amd.DeviceBatchLoader(ds[:30], 20),
                       kagnn_amd.DeviceBatchLoader(ds[25:], 20)]
            opt = harness.Adam(m.parameters(), lr=1e-2)
            ops.RegressionStop.update = lambda self, *a: (seen.__setitem__("stop", self), update(self, *a))[1]
            try:
                res = harness.train_graph_regression(m, *loaders, epochs=2, patience=5, poll_every=1, optimizer=opt, keep_best=True)
            finally:
                ops.RegressionStop.update = update
            assert res.epochs_run == 2
            p = _leaf(pred)
            loss = ops.l1_loss(p, target)
            loss.backward()
            meter = ops.RegressionMeter(5, DEV)
            with torch.no_grad():
                scaled = ops.l1_loss(pred, target, accumulate=meter, scale=scale)
            return [seen["stop"]._buf] + [t.detach() for t in m.state_dict().values()] + [opt._m, opt._v, loss.detach(), p.grad, scaled, meter.record]
        return m, _ran(run, "kagnn_batch_assemble", "kagnn_l1_loss_meter_fwd", "kagnn_l1_loss_bwd", "kagnn_l1_loss_fwd",
                       "kagnn_regression_epoch_update", "kagnn_copy_if", "kagnn_adam_step")
    return build


def _adam_alone():
    """``harness.Adam``: two steps from fixed gradients over tensors of 1, 7, 64 x 33 and 4099 elements, weight decay on.  Returns
    the parameters and both moment tensors"""
    def build():
        shapes = [(1,), (7,), (64, 33), (4099,)]
        p0 = [_randn(*s, seed=k) for k, s in enumerate(shapes)]
        grads = [[_randn(*s, seed=10 * step + k) for k, s in enumerate(shapes)] for step in (1, 2)]

        def run():
            params = [_leaf(p) for p in p0]
            opt = harness.Adam(params, lr=1e-2, weight_decay=1e-2)
            for gs in grads:
                for p, g in zip(params, gs):
                    p.grad = g.clone()
                opt.step()
            return [p.detach() for p in params] + [opt._m, opt._v]
        return None, _ran(run, "kagnn_adam_step")
    return build


_case("classification", "graph classification two epochs", _graph_classification())
_case("regression", "graph regression two epochs", _graph_regression())
_case("regression", "harness.Adam two steps", _adam_alone(), floor=1)        # the first moments (torch.zeros); the second are their zeros_like


# ---------------------------------------------------------------------------------------------------------------- node classification
# nodeclass.hip: 7 classes are 8 lanes a row, 32 rows a workgroup: 3001 rows are 94 workgroups (the last of 25 rows) whose partial
# records meet in a workspace; 25 rows are ONE workgroup that writes the records itself (no workspace)
def _node_classification():
    """``harness.train_node_classification`` for three epochs on 3001 nodes / 7 classes / 3 splits (node_eval through its
    workspace, EarlyStop, copy_if of the best weights).  Returns the history, the weights left, and -- from the primitives on
    fixed logits -- the split bytes, the records of 3001 and of 25 rows, and an EarlyStop's whole buffer and a copy_if target after
    an improving, a missing and an improving epoch"""
    def build():
        n, f, classes = 3001, 40, 7
        ei = orc.powerlaw_graph(n, 10 * n, seed=5).to(DEV)
        torch.manual_seed(11)
        model = kagnn_amd.GKAN_Nodes("gin", 2, f, 32, classes, skip=True, grid_size=5, spline_order=3, hidden_layers=2, dropout=0.0).to(DEV)
        state = [t.detach().clone() for t in model.state_dict().values()]
        x, y = _randn(n, f, seed=6, scale=0.4), torch.randint(0, classes, (n,), generator=_gen(8)).to(DEV)
        split = torch.randint(0, 4, (n,), generator=_gen(9)).to(DEV)                 # 3: in no split
        masks = [split == s for s in range(3)]
        logits = [_randn(n, classes, seed=20 + k, scale=s) for k, s in enumerate((1.0, 3.0, 0.2))]

        def run():
            _restart(model, state)
            res = harness.train_node_classification(model, x, ops.GraphIndex(ei, n), y, *masks, epochs=3, patience=5, poll_every=1)
            assert res.epochs_run == 3
            bits = ops.split_bits(*masks)
            stop = ops.EarlyStop(2, max_epochs=4, num_splits=3, device=DEV)
            live, saved, out = torch.zeros(1031, device=DEV), torch.full((1031,), -1.0, device=DEV), []
            for k, z in enumerate(logits):
                rec = ops.node_eval(z, y, bits, 3)
                stop.update(rec, 1)
                live.fill_(float(k + 1))
                ops.copy_if(stop.improved, [saved], [live])
                out += [rec, saved.clone()]
            small = ops.node_eval(logits[0][:25], y[:25], bits[:25].contiguous(), 3)
            ops.flush_graph_checks()
            return [res.history.to(DEV)] + [t.detach() for t in model.state_dict().values()] + [bits, small, stop._buf] + out
        return model, _ran(run, "kagnn_node_eval", "kagnn_early_stop_update", "kagnn_copy_if", "kagnn_adam_step")
    return build


_case("node classification", "node classification three epochs", _node_classification())


# ---------------------------------------------------------------------------------------------------------------- device datasets
def _batch_loader():
    """the dataset of tests/test_gpu_data.py::test_unaligned_storage_bases (60 QM9-shaped graphs, x / edge_attr / y starting 4 bytes
    into their allocations), two shuffled epochs in batches of 16 (16 + 16 + 16 + 12).  Returns every batch: x, edge_index,
    edge_attr, y, batch vector, pointers and the six arrays of the attached index"""
    def build():
        from test_gpu_data import _dataset, _qm9
        d = _qm9(G=60, seed=13)

        def shifted(t):
            buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
            v = buf[1:].view(t.shape)
            v.copy_(t)
            return v

        def run():
            ds = _dataset(d)
            st = ds.storage
            st.x, st.edge_attr, st.y = shifted(st.x), shifted(st.edge_attr), shifted(st.y)
            loader, out = kagnn_amd.DeviceBatchLoader(ds, 16, shuffle=True, generator=_gen(4)), []
            for _ in range(2):
                for b in loader:
                    assert b.graph_index is not None
                    out += [b.x, b.edge_index, b.edge_attr, b.y, b.batch, b.ptr] + _csr(b.graph_index)
            ops.flush_graph_checks()
            assert len(out) == 2 * 4 * 12
            return out
        return None, _ran(run, "kagnn_batch_assemble")
    return build


_case("device datasets", "DeviceBatchLoader two epochs ragged", _batch_loader())


# ---------------------------------------------------------------------------------------------------------------- graph primitives
def _small_graph(n, e, seed=3):
    return orc.powerlaw_graph(n, e, seed=seed).to(DEV)


def _gine():
    """returns out, gx, g_edge_attr and the rebuilt CSR arrays (1201 nodes, 9000 edges, F = 24: not a multiple of 16)"""
    def build():
        n, e, f = 1201, 9000, 24
        ei = _small_graph(n, e)
        x, ea, go = _randn(n, f, seed=1), _randn(e, f, seed=2), _randn(n, f, seed=3)

        def run():
            g = ops.GraphIndex(ei, n)
            xr, er = _leaf(x), _leaf(ea)
            out = ops.aggregate_gine(xr, er, g, 1.25)
            out.backward(go)
            return [out, xr.grad, er.grad] + _csr(g)
        return None, _ran(run, "kagnn_aggregate_gine", "kagnn_aggregate_gine_bwd")
    return build


def _pooling(mean):
    """segments that are empty, one row long, and that leave rows uncovered at both ends.  Returns the pooled rows and gx"""
    def build():
        n, f = 517, 33
        x, go = _randn(n, f, seed=1), _randn(7, f, seed=2)
        seg = torch.tensor([5, 5, 6, 40, 40, 300, 301, n - 3], dtype=torch.int32, device=DEV)

        def run():
            xr = _leaf(x)
            out = ops.segment_pool(xr, seg, mean=mean)
            out.backward(go)
            return [out, xr.grad]
        return None, _ran(run, "kagnn_segment_pool", "kagnn_segment_broadcast")
    return build


def _scaled_aggregation(f, dtype, hubs):
    """``aggregate_sum`` with in_scale, out_scale, bias, edge weights and dropped self loops; fp32 or bf16 gathered rows.  Returns out,
    gx, g_bias, g_edge_weight and the rebuilt CSR arrays"""
    def build():
        n, e = (20_000, 150_000) if hubs else (1201, 9000)
        ei = orc.powerlaw_graph(n, e, seed=8)
        ei[:, :30] = torch.arange(30).repeat(2, 1)
        ei = ei.to(DEV)
        x, go = _randn(n, f, seed=1, scale=0.5), _randn(n, f, seed=2, scale=0.5)
        s_in, s_out = (0.5 + torch.rand(n, generator=_gen(3))).to(DEV), (0.5 + torch.rand(n, generator=_gen(4))).to(DEV)
        b0, w0 = _randn(f, seed=5), (0.2 + torch.rand(e, generator=_gen(6))).to(DEV)

        def run():
            g = ops.GraphIndex(ei, n)
            assert (g.num_hub_seg > 0) == hubs
            xr, b, w = _leaf(x.to(dtype)), _leaf(b0), _leaf(w0)
            out = ops.aggregate_sum(xr, g, 1.5, edge_weight=w, in_scale=s_in, out_scale=s_out, bias=b, skip_self_loops=True)
            out.backward(go)
            return [out, xr.grad, b.grad, w.grad] + _csr(g)
        wanted = "kagnn_aggregate_sum_bf16" if dtype == torch.bfloat16 and ops._bf16_gather_width_ok(f) else "kagnn_aggregate_sum"
        return None, _ran(run, wanted, "kagnn_aggregate_edge_grad")
    return build


def _affine_aggregation():
    """``aggregate_sum_affine`` over hub rows (by destination, and transposed: no hub rows there).  Returns both outputs"""
    def build():
        n, e, f = 20_000, 150_000, 64
        ei = orc.powerlaw_graph(n, e, seed=8).to(DEV)
        x, aff = _randn(n, f, seed=1, scale=0.5), torch.stack([0.5 + torch.rand(f, generator=_gen(2)), torch.randn(f, generator=_gen(3))]).to(DEV)

        def run():
            g = ops.GraphIndex(ei, n)
            assert g.num_hub_seg > 0
            return [ops.aggregate_sum_affine(x, g, 1.5, aff), ops.aggregate_sum_affine(x, g, 0.0, aff, transposed=True)] + _csr(g)
        return None, _ran(run, "kagnn_aggregate_sum_affine")
    return build


_case("primitives", "GINE n1201 e9000 F24", _gine())
_case("primitives", "segment pool sum, empty and one-row segments", _pooling(False), floor=2)        # the pooled rows, gx
_case("primitives", "segment pool mean, empty and one-row segments", _pooling(True), floor=2)
_case("primitives", "scaled aggregation F40 bias", _scaled_aggregation(40, torch.float32, False))
_case("primitives", "scaled aggregation F64 bias hub rows", _scaled_aggregation(64, torch.float32, True))
_case("primitives", "bf16 rows F64 hub rows", _scaled_aggregation(64, torch.bfloat16, True))
assert ops._bf16_gather_width_ok(64) and not ops._bf16_gather_width_ok(65)
_case("primitives", "bf16 rows F65 (refused width: through fp32)", _scaled_aggregation(65, torch.bfloat16, False))
_case("primitives", "affine aggregation F64 hub rows", _affine_aggregation())


# ---------------------------------------------------------------------------------------------------------------- kagnn::* ops
# each op of kagnn_amd/library.py called eagerly, once, on the operands tests/test_gpu_compile.py hands to opcheck (129 x 33 -> 17
# layers, a 3000-node power-law graph with hub segments, F = 16).  ``floor``: the buffers the op really allocates
LIBRARY_OPS = {"aggregate_sum": (2, ("kagnn_aggregate_sum",)), "aggregate_edge_grad": (1, ("kagnn_aggregate_edge_grad",)),
               "kan_linear": (3, ("kagnn_kan_pack", "kagnn_kan_linear_fwd")), "kan_linear_bwd_input": (1, ("kagnn_kan_linear_bwd_input",)),
               "kan_linear_bwd_weight": (4, ("kagnn_kan_linear_bwd_weight",)), "fastkan_layer": (3, ("kagnn_fastkan_fwd",)),
               "fastkan_layer_bwd": (7, ("kagnn_fastkan_bwd",)), "batch_norm": (4, ("kagnn_batchnorm_fwd",)),
               "batch_norm_bwd": (4, ("kagnn_batchnorm_bwd",)), "segment_pool": (1, ("kagnn_segment_pool",)),
               "segment_broadcast": (1, ("kagnn_segment_broadcast",))}
_LIBRARY_INPUTS = {}


def _library_inputs():
    if _LIBRARY_INPUTS:
        return _LIBRARY_INPUTS
    from kagnn_amd import library      # noqa: F401 (registers the ops)
    n, fin, fout, G, k, ng, mode = 129, 33, 17, 4, 3, 8, ops.PREC_SPLIT
    torch.manual_seed(1)
    layer = kagnn_amd.KANLinear(fin, fout, grid_size=G, spline_order=k).to(DEV)
    x, gy = _randn(n, fin, seed=1, scale=0.6), _randn(n, fout, seed=2)
    bw, sw, sc, knots = layer.base_weight.detach(), layer.spline_weight.detach(), layer.spline_scaler.detach(), layer._knots()
    pack = torch.ops.kagnn.kan_linear(x, bw, sw, sc, knots, G, k, mode)[1]
    centers, den = torch.linspace(-2.0, 2.0, ng).to(DEV), 4.0 / (ng - 1)
    lw, lb = 1.0 + _randn(fin, seed=3, scale=0.3), _randn(fin, seed=4, scale=0.3)
    fsw, fbw, fbb = _randn(fout, fin * ng, seed=5, scale=0.1), _randn(fout, fin, seed=6, scale=0.3), _randn(fout, seed=7, scale=0.3)
    stats = torch.ops.kagnn.fastkan_layer(x, lw, lb, fsw, fbw, fbb, centers, den, 1e-5, mode)[1]
    gn, ge, f = 3000, 24000, 16
    small = ops._SMALL_CSR
    ops._SMALL_CSR = False             # the rocPRIM build: the only one that lists hub segments
    try:
        g = ops.GraphIndex(orc.powerlaw_graph(gn, ge).to(DEV), gn)
    finally:
        ops._SMALL_CSR = small
    assert g.num_hub_seg > 0
    ax, ago = _randn(gn, f, seed=8, scale=0.8), _randn(gn, f, seed=9, scale=0.8)
    aw = (0.2 + torch.rand(ge, generator=_gen(10))).to(DEV)[g.perm.long()].contiguous()
    s_in, s_out, ab = (0.5 + torch.rand(gn, generator=_gen(11))).to(DEV), (0.5 + torch.rand(gn, generator=_gen(12))).to(DEV), _randn(f, seed=13)
    bx, w1, b1 = _randn(n, fout, seed=14), 1.0 + _randn(fout, seed=15, scale=0.3), _randn(fout, seed=16, scale=0.3)
    rm, rv = torch.zeros(fout, device=DEV), torch.ones(fout, device=DEV)
    _, mean, rstd = torch.ops.kagnn.batch_norm(bx, w1, b1, rm, rv, True, 1e-5)
    ptr = torch.tensor([5, 5, 40, 100, n - 3], dtype=torch.int32, device=DEV)
    _LIBRARY_INPUTS.update({
        "aggregate_sum": (ax, g.rowptr, g.col, aw, s_in, s_out, ab, g.hub_seg, g.num_hub_seg, g.hub_threshold, 1.5, True),
        "aggregate_edge_grad": (ax, ago, g.rowptr, g.col, g.perm, s_in, s_out, g.hub_seg, g.num_hub_seg, g.hub_threshold, g.num_edges, True),
        "kan_linear": (x, bw, sw, sc, knots, G, k, mode),                     # -> (y, the input-gradient pack)
        "kan_linear_bwd_input": (x, gy, knots, pack, fout, G, k, mode),
        "kan_linear_bwd_weight": (x, gy, knots, sw, sc, G, k, mode, True),
        "fastkan_layer": (x, lw, lb, fsw, fbw, fbb, centers, den, 1e-5, mode),
        "fastkan_layer_bwd": (x, gy, lw, lb, fsw, fbw, centers, stats, den, 1e-5, mode),
        "batch_norm": (bx, w1, b1, rm, rv, True, 1e-5),
        "batch_norm_bwd": (bx, gy, w1, mean, rstd, True, True),
        "segment_pool": (x, ptr, True),
        "segment_broadcast": (_randn(4, fin, seed=17), ptr, n, True)})
    return _LIBRARY_INPUTS


def _library_op(name):
    """returns every output of ``torch.ops.kagnn.<name>`` -- for kan_linear that includes the uint8 pack it hands to its backward"""
    def build():
        args = _library_inputs()[name]

        def run():
            out = getattr(torch.ops.kagnn, name)(*args)
            return list(out) if isinstance(out, (tuple, list)) else [out]
        return None, _ran(run, *LIBRARY_OPS[name][1])
    return build


for _name, (_floor, _) in LIBRARY_OPS.items():
    _case("library ops", f"kagnn::{_name} eager", _library_op(_name), floor=_floor)


# ---------------------------------------------------------------------------------------------------------------- backward overlap
def _overlap(what):
    """the layer backward with its weight gradients beside the transposed aggregation (KAGNN_BWD_OVERLAP=1) on the 20 000-node
    graph REVERSED: its ~1 000-edge hub is then on the side the backward aggregates over (hub segments and their merge behind the
    co-run row kernel).  Returns the output, gx, every parameter gradient (and the running statistics)"""
    def build():
        import os
        n = 20_000
        ei = orc.powerlaw_graph(n, 150_000, seed=8).flip(0).contiguous().to(DEV)
        g = ops.GraphIndex(ei, n)
        assert g.num_hub_seg_t > 0
        if what == "layer":
            torch.manual_seed(642)
            net = kagnn_amd.GIKANLayer(64, 64, grid_size=5, spline_order=3, hidden_dim=64, nb_layers=2).to(DEV)
            gout = _randn(n, 64, seed=2, scale=0.5)
        else:
            torch.manual_seed(5)
            net = kagnn_amd.GKAN_Nodes("gin", 2, 64, 64, 40, skip=True, grid_size=5, spline_order=3, hidden_layers=2).to(DEV).train()
            gout = _randn(n, 40, seed=4, scale=0.5 / n)
        x = _randn(n, 64, seed=1, scale=0.5)

        def run():
            was = os.environ.get("KAGNN_BWD_OVERLAP")
            os.environ["KAGNN_BWD_OVERLAP"] = "1"
            try:
                xr = _leaf(x)
                y = net(xr, g)
                y.backward(gout)
            finally:
                if was is None:
                    del os.environ["KAGNN_BWD_OVERLAP"]
                else:
                    os.environ["KAGNN_BWD_OVERLAP"] = was
            return [y, xr.grad] + [p.grad for p in net.parameters()] + [b for b in net.buffers() if b.dtype.is_floating_point]
        return net, _ran(run, prefixes=("kagnn_gin_kan_layer_bwd_bn" if what == "model" else "kagnn_gin_kan_layer_bwd",))
    return build


_case("overlap", "overlapped backward GIKANLayer 64->64 reversed hubs", _overlap("layer"))
_case("overlap", "overlapped backward BatchNorm + skip node model reversed hubs", _overlap("model"))


# ---------------------------------------------------------------------------------------------------------------- read-out over parts
def _parts(n):
    """``KANLinear.forward_parts`` on [64 | 64 | 64] -> 40: a plain block and two ``AffineRows`` blocks whose ``NormSums`` carry the
    norm's mean / rstd.  From 128 row blocks of 256 on (kan_split_dx_stats_ok; 32 513 rows: the last block holds ONE row) their
    input gradients come from ``kagnn_kan_linear_bwd_input_affine_sums`` together with the two column sums, through a workspace of
    per-block partial sums; below (1037 rows) from ``kagnn_kan_linear_bwd_input_affine``, and no sums are parked.  Returns y, the
    three block gradients, the parameter gradients and the parked column sums"""
    def build():
        w, fout = 64, 40
        with_sums = -(-n // 256) >= 128
        torch.manual_seed(3)
        layer = kagnn_amd.KANLinear(3 * w, fout, grid_size=5, spline_order=3).to(DEV)
        blocks = [_randn(n, w, seed=k, scale=0.5) for k in (1, 2, 3)]
        affs = [torch.stack([0.5 + torch.rand(w, generator=_gen(10 + k)), 0.3 * torch.randn(w, generator=_gen(20 + k))]).to(DEV) for k in (1, 2)]
        stats = [(_randn(w, seed=30 + k, scale=0.2), (0.5 + torch.rand(w, generator=_gen(40 + k))).to(DEV)) for k in (1, 2)]
        gy = _randn(n, fout, seed=7)

        def run():
            leaves = [_leaf(b) for b in blocks]
            sums = []
            for mean, rstd in stats:
                ns = ops.NormSums()
                ns.mean, ns.rstd = mean, rstd
                sums.append(ns)
            y = layer.forward_parts([leaves[0], ops.AffineRows(leaves[1], affs[0], sums[0]), ops.AffineRows(leaves[2], affs[1], sums[1])])
            assert type(y.grad_fn).__name__ == "_KANLinearPartsFnBackward", type(y.grad_fn).__name__
            y.backward(gy)
            assert all((ns.sums is not None) == with_sums for ns in sums)
            return [y] + [t.grad for t in leaves] + [p.grad for p in layer.parameters()] + [ns.sums for ns in sums if with_sums]
        return layer, _ran(run, "kagnn_kan_linear_fwd_parts_affine", "kagnn_kan_linear_bwd_weight_affine",
                           "kagnn_kan_linear_bwd_input_affine_sums" if with_sums else "kagnn_kan_linear_bwd_input_affine")
    return build


_case("parts", "read-out over parts 32513x[64,64,64]->40 two affine blocks with sums", _parts(32513))
_case("parts", "read-out over parts 1037x[64,64,64]->40 two affine blocks", _parts(1037))


# ---------------------------------------------------------------------------------------------------------------- the two tests
@pytest.mark.parametrize("case", list(CASES))
def test_blind_to_the_heap(monkeypatch, case):
    _heap_case(monkeypatch, CASES, case)


@pytest.mark.parametrize("case", list(CASES))
def test_writes_stay_inside_their_buffers(monkeypatch, case):
    _guard_case(monkeypatch, CASES, case)
