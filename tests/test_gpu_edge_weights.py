"""Differentiable edge weights against fp64 on the CPU: ``kagnn_aggregate_edge_grad`` at kernel level, the gradient of
``ops.aggregate_sum`` with respect to ``edge_weight``, ``_NormalisedConv`` with weights that require a gradient, ``kagnn_amd.edge_mask``
over whole models and ``kagnn_amd.explain_edges``.

The reference is written here: ``index_add`` on ``x.double()`` plus autograd (``_ref_aggregate``); for the convolutions and models a
dense normalised adjacency or the oracle's message passing with the mask multiplied in (``masked_oracle``) around the oracle's layer
functions.  Kernel and autograd level: ``helpers.assert_close`` at its default, the fp32 bound of README contract row 2.  Convolutions
and whole models: 1e-4 of each tensor's own maximum (contract row 3).  An all-ones mask against the unmasked run: 2e-5, the
fused-versus-composed tolerance of tests/test_gpu_edge_activations.py.

Shapes: 300 nodes / 2000 edges with duplicate edges and self loops; 400 nodes with one 1613-edge destination hub (hub segments, the
last one ragged; built on the rocPRIM path, the small-graph CSR has no segments); N = 1; E = 0; models on 120 nodes / 500 edges.
"""
import itertools
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import kagnn_amd
from kagnn_amd import baselines as B
from kagnn_amd import models as M
from kagnn_amd import ops
from oracle import kan_oracle as orc
from helpers import assert_close, must_fail
import test_gpu_baselines as tb

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODEL_TOL = 1e-4
WIDTHS = [1, 3, 4, 8, 16, 20, 64, 128, 132, 256, 260]     # edge-parallel (LPR 1, 2, 4), LPR 8 .. 64 with and without idle lanes, generic
FUSED_ENTRY_POINTS = ("kagnn_gin_kan_layer_fwd", "kagnn_gin_kan_layer_fwd_affine")


# ---------------------------------------------------------------------------------- graphs and the fp64 reference
def _edges(seed, n, e, loops, dups=50):
    """``e`` edges: random non-loop edges, ``dups`` of them repeated, one self loop on each of ``loops`` distinct nodes; shuffled"""
    g = torch.Generator().manual_seed(seed)
    m = e - loops
    src = torch.randint(0, n, (m,), generator=g)
    dst = (src + 1 + torch.randint(0, n - 1, (m,), generator=g)) % n
    src[:dups], dst[:dups] = src[dups:2 * dups].clone(), dst[dups:2 * dups].clone()
    nodes = torch.randperm(n, generator=g)[:loops]
    ei = torch.stack([torch.cat([src, nodes]), torch.cat([dst, nodes])])
    return ei[:, torch.randperm(e, generator=g)].contiguous()


def _hub_edges(seed, n=400, hub=7, into_hub=1613, others=600):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (into_hub,), generator=g)
    src[5] = hub                                                        # the hub's own self loop
    rest = _edges(seed + 1, n, others, 20)
    ei = torch.cat([torch.stack([src, torch.full((into_hub,), hub)]), rest], 1)
    return ei[:, torch.randperm(ei.size(1), generator=g)].contiguous()


@pytest.fixture(scope="module")
def graphs():
    out = {}
    small = ops._SMALL_CSR
    ops._SMALL_CSR = False                       # the rocPRIM build: the only one that lists hub segments
    try:
        for name, ei, n in (("random", _edges(1, 300, 2000, 40), 300), ("hub", _hub_edges(2), 400)):
            out[name] = (ei, n, ops.GraphIndex(ei.to(DEV), n))
    finally:
        ops._SMALL_CSR = small
    assert out["random"][2].num_hub_seg == 0
    g = out["hub"][2]
    seg = g.hub_seg[:3 * g.num_hub_seg].view(-1, 3).cpu()
    lens = (seg[:, 2] - seg[:, 1]).tolist()
    assert g.num_hub_seg > 2 and bool((seg[:, 0] == 7).all()) and sum(lens) == int((out["hub"][0][1] == 7).sum()) >= 1613, seg
    assert len(set(lens)) > 1, lens                                    # a ragged last segment
    return out


def _ref_aggregate(x, ei, w=None, self_scale=0.0, in_scale=None, out_scale=None, skip=False, bias=None):
    """fp64: out[i] = out_scale[i] * (self_scale * s(i) x[i] + sum_{e: j -> i} w[e] s(j) x[j]) + bias, self loops dropped when ``skip``"""
    src, dst = ei[0], ei[1]
    n = x.size(0)
    s = torch.ones(n, dtype=torch.float64) if in_scale is None else in_scale.double().cpu()
    ww = torch.ones(ei.size(1), dtype=torch.float64) if w is None else w
    if skip:
        ww = ww * (src != dst)
    out = (self_scale * s.unsqueeze(1) * x).index_add(0, dst, (ww * s[src]).unsqueeze(1) * x[src])
    if out_scale is not None:
        out = out_scale.double().cpu().unsqueeze(1) * out
    return out if bias is None else out + bias


def _ref_edge_grad(x, gout, ei, in_scale=None, out_scale=None, skip=False):
    w = torch.ones(ei.size(1), dtype=torch.float64, requires_grad=True)
    _ref_aggregate(x.double().cpu(), ei, w, 0.0, in_scale, out_scale, skip).backward(gout.double().cpu())
    return w.grad if w.grad is not None else torch.zeros_like(w)


def _operands(n, f, seed):
    g = torch.Generator().manual_seed(seed)
    x, gout = 0.8 * torch.randn(n, f, generator=g), 0.8 * torch.randn(n, f, generator=g)
    s_in, s_out = 0.5 + torch.rand(n, generator=g), 0.5 + torch.rand(n, generator=g)
    return x.to(DEV), gout.to(DEV), s_in.to(DEV), s_out.to(DEV)


def _timed(fn):
    timer = ops.EntryPointTimer()
    ops.set_timer(timer)
    try:
        out = fn()
    finally:
        ops.set_timer(None)
    return out, [r[0] for r in timer.records]


# ---------------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize("f", WIDTHS)
def test_edge_grad_kernel_against_fp64(graphs, f):
    for name, (ei, n, g) in graphs.items():
        x, gout, s_in, s_out = _operands(n, f, 10 + f)
        loops = (ei[0] == ei[1]).to(DEV)
        assert bool(loops.any()) and not torch.equal(g.perm.cpu().long(), torch.arange(ei.size(1)))
        for scaled, skip in itertools.product((False, True), (False, True)):
            kw = dict(in_scale=s_in if scaled else None, out_scale=s_out if scaled else None, skip_self_loops=skip)
            got = ops.aggregate_edge_grad(x, gout, g, **kw)
            assert got.shape == (ei.size(1),) and got.dtype == torch.float32
            want = _ref_edge_grad(x, gout, ei, kw["in_scale"], kw["out_scale"], skip)
            assert_close(got, want, what=f"edge grad {name} F={f} scaled={scaled} skip={skip}")
            if skip:
                assert bool((got[loops] == 0).all()), "a dropped self loop must be exactly 0"
            else:
                assert bool((got[loops] != 0).all())
            assert torch.equal(got, ops.aggregate_edge_grad(x, gout, g, **kw)), "a second call must give the same bits"


def test_degenerate_graphs():
    one = torch.zeros(2, 3, dtype=torch.int64)                         # N = 1: three self loops
    g1 = ops.GraphIndex(one.to(DEV), 1)
    for f in (3, 4, 64):
        x, gout, s_in, s_out = _operands(1, f, f)
        got = ops.aggregate_edge_grad(x, gout, g1, s_in, s_out)
        assert_close(got, _ref_edge_grad(x, gout, one, s_in, s_out), what=f"N=1 F={f}")
        assert bool((ops.aggregate_edge_grad(x, gout, g1, s_in, s_out, skip_self_loops=True) == 0).all())
    none = torch.zeros(2, 0, dtype=torch.int64)                        # E = 0: nothing is launched, nothing is written
    g0 = ops.GraphIndex(none.to(DEV), 5)
    x, gout, s_in, s_out = _operands(5, 8, 3)
    assert ops.aggregate_edge_grad(x, gout, g0).shape == (0,)
    buf = torch.full((4,), -777.0, device=DEV)
    ops.aggregate_edge_grad(x, gout, g0, out=buf)
    assert bool((buf == -777.0).all())


def test_column_slices_and_leading_dimensions(graphs):
    ei, n, g = graphs["random"]
    f = 64
    big_x, big_g, s_in, s_out = _operands(n, f + 8, 77)
    for lo, width, what in ((4, f + 8, "aligned slice, ld 72: float4 rows"), (1, f + 8, "unaligned slice, ld 72: scalar rows")):
        x, gout = big_x[:, lo:lo + f], big_g[:, lo:lo + f]
        assert x.stride(0) == width and not x.is_contiguous()
        assert_close(ops.aggregate_edge_grad(x, gout, g, s_in, s_out), _ref_edge_grad(x, gout, ei, s_in, s_out), what=what)
    odd_x, odd_g = big_x[:, :f + 3].contiguous()[:, :f], big_g[:, :f + 3].contiguous()[:, :f]          # ld 67
    assert odd_x.stride(0) % 4 == 3
    assert_close(ops.aggregate_edge_grad(odd_x, odd_g, g, s_in, s_out), _ref_edge_grad(odd_x, odd_g, ei, s_in, s_out), what="ld % 4 != 0")
    # one operand strided, the other not
    assert_close(ops.aggregate_edge_grad(big_x[:, 4:4 + f], odd_g, g), _ref_edge_grad(big_x[:, 4:4 + f], odd_g, ei), what="mixed lds")


def test_original_edge_order_sentinel_and_mutation_guards(graphs):
    for name, (ei, n, g) in graphs.items():
        e = ei.size(1)
        x, gout, s_in, s_out = _operands(n, 20, 5)
        got = ops.aggregate_edge_grad(x, gout, g, s_in, s_out)
        want = _ref_edge_grad(x, gout, ei, s_in, s_out)
        assert_close(got, want, what=f"{name}: original order")
        # the gradient permutes with the edge list, bit for bit
        p = torch.randperm(e, generator=torch.Generator().manual_seed(9))
        small = ops._SMALL_CSR
        ops._SMALL_CSR = False
        try:
            g2 = ops.GraphIndex(ei[:, p].contiguous().to(DEV), n)
        finally:
            ops._SMALL_CSR = small
        assert torch.equal(ops.aggregate_edge_grad(x, gout, g2, s_in, s_out), got[p.to(DEV)])
        # entries beyond E of a longer buffer stay as they were
        buf = torch.full((e + 9,), -777.0, device=DEV)
        ret = ops.aggregate_edge_grad(x, gout, g, s_in, s_out, out=buf)
        assert ret.data_ptr() == buf.data_ptr() and torch.equal(buf[:e], got) and bool((buf[e:] == -777.0).all())
        # mutants: the values left in CSR order; out_scale dropped
        must_fail(got[g.perm.long()], want, what=f"{name}: gradient in CSR order")
        must_fail(ops.aggregate_edge_grad(x, gout, g, s_in, None), want, what=f"{name}: out_scale dropped")


@pytest.mark.parametrize("f", [3, 20, 64])
def test_nan_poisons_exactly_the_edges_that_touch_the_row(graphs, f):
    for name, (ei, n, g) in graphs.items():
        x, gout, s_in, s_out = _operands(n, f, 21)
        j0 = int(ei[0, 0])
        i0 = 7 if name == "hub" else int(ei[1, 1])
        xn = x.clone()
        xn[j0, f // 2] = float("nan")
        got = ops.aggregate_edge_grad(xn, gout, g, s_in, s_out)
        assert torch.equal(torch.isnan(got).cpu(), ei[0] == j0), f"{name}: NaN in x[{j0}]"
        gn = gout.clone()
        gn[i0, 0] = float("nan")
        got = ops.aggregate_edge_grad(x, gn, g, s_in, s_out)
        assert torch.equal(torch.isnan(got).cpu(), ei[1] == i0), f"{name}: NaN in gout[{i0}]"
        # ... and a dropped self loop is 0 even then
        got = ops.aggregate_edge_grad(xn, gn, g, s_in, s_out, skip_self_loops=True)
        loops = ei[0] == ei[1]
        assert bool((got.cpu()[loops] == 0).all())
        assert torch.equal(torch.isnan(got).cpu(), ((ei[0] == j0) | (ei[1] == i0)) & ~loops)


# ---------------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("f,skip", [(20, False), (64, True), (7, True)])
def test_aggregate_sum_differentiates_through_edge_weight(graphs, f, skip):
    for name, (ei, n, g) in graphs.items():
        e = ei.size(1)
        x0, gout, s_in, s_out = _operands(n, f, 31)
        gen = torch.Generator().manual_seed(32)
        w0, b0 = torch.rand(e, generator=gen), torch.randn(f, generator=gen)
        x, w, b = (t.clone().to(DEV).requires_grad_(True) for t in (x0.cpu(), w0, b0))
        out, names = _timed(lambda: ops.aggregate_sum(x, g, self_scale=1.5, edge_weight=w, in_scale=s_in, out_scale=s_out, bias=b, skip_self_loops=skip))
        out.backward(gout)
        assert w.grad is not None, "edge_weight.requires_grad: the aggregation must hand it a gradient"
        x64, w64, b64 = (t.detach().double().cpu().requires_grad_(True) for t in (x, w, b))
        want = _ref_aggregate(x64, ei, w64, 1.5, s_in, s_out, skip, b64)
        want.backward(gout.double().cpu())
        what = f"aggregate_sum {name} F={f} skip={skip}"
        assert_close(out, want, what=what + " out")
        assert_close(w.grad, w64.grad, what=what + " edge_weight.grad")
        assert_close(x.grad, x64.grad, what=what + " x.grad")
        assert_close(b.grad, b64.grad, what=what + " bias.grad")
        if skip:
            assert bool((w.grad.cpu()[ei[0] == ei[1]] == 0).all())
        must_fail(torch.zeros_like(w.grad), w64.grad, what=what + " edge_weight.grad zeroed")

        # weights that do not require a gradient: the same bits and the same launches as ever
        def run(weight):
            xr = x.detach().clone().requires_grad_(True)
            o = ops.aggregate_sum(xr, g, self_scale=1.5, edge_weight=weight, in_scale=s_in, out_scale=s_out, bias=b.detach(), skip_self_loops=skip)
            o.backward(gout)
            return o.detach(), xr.grad

        (o1, gx1), names1 = _timed(lambda: run(w.detach()))
        (o2, gx2), names2 = _timed(lambda: run(w.detach().clone()))
        assert torch.equal(o1, o2) and torch.equal(gx1, gx2) and torch.equal(o1, out.detach()) and torch.equal(gx1, x.grad)
        assert names1 == names2 and "kagnn_aggregate_edge_grad" not in names1, names1
        (o3, gx3), names3 = _timed(lambda: run(w.detach().clone().requires_grad_(True)))
        assert names3.count("kagnn_aggregate_edge_grad") == 1 and [k for k in names3 if k != "kagnn_aggregate_edge_grad"] == names1, names3
        assert torch.equal(o3, o1) and torch.equal(gx3, gx1)


def test_edge_weight_gradient_of_bf16_rows(graphs):
    """bf16 gather operands: the gradient is taken on the rows that were summed, the bf16 values in fp32"""
    ei, n, g = graphs["random"]
    x0, gout, s_in, s_out = _operands(n, 64, 41)
    xb = x0.to(torch.bfloat16)
    w = torch.rand(ei.size(1), generator=torch.Generator().manual_seed(42)).to(DEV).requires_grad_(True)
    out = ops.aggregate_sum(xb, g, self_scale=1.0, edge_weight=w, in_scale=s_in, out_scale=s_out)
    out.backward(gout)
    w64 = w.detach().double().cpu().requires_grad_(True)
    want = _ref_aggregate(xb.float().double().cpu(), ei, w64, 1.0, s_in, s_out)
    want.backward(gout.double().cpu())
    assert_close(out, want, what="bf16 rows: out")
    assert_close(w.grad, w64.grad, what="bf16 rows: edge_weight.grad")


# ---------------------------------------------------------------------------------- _NormalisedConv, weights that require grad
def _leaves64(module):
    return {k: p.detach().double().cpu().requires_grad_(p.requires_grad) for k, p in module.named_parameters()}


def _state64(module):
    return {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in module.state_dict().items()}


def _layer64(kind, P, prefix, spline_order=3):
    """the oracle's layer function on the fp64 tensors ``P[prefix + key]``"""
    if kind == "kan":
        return lambda h: orc.kan_linear_forward(h, P[prefix + "base_weight"], P[prefix + "spline_weight"], P.get(prefix + "spline_scaler"),
                                                P[prefix + "grid"], spline_order)
    sub = {k[len(prefix):]: v for k, v in P.items() if k.startswith(prefix)}
    return lambda h: orc.fastkan_forward(h, [sub])


@pytest.mark.parametrize("kind", ["kan", "fastkan"])
def test_gcn_conv_with_edge_weights_that_require_grad(kind):
    n, e, fin, fout = 200, 900, 9, 12
    ei = _edges(50, n, e, 30)                     # (at most one self loop per node: with two, which weight the loop keeps is unordered)
    torch.manual_seed(51)
    conv = kagnn_amd.KAGCNConv(fin, fout, 4, 3) if kind == "kan" else kagnn_amd.FASTKAGCNConv(fin, fout, 4)
    nn.init.normal_(conv.bias, std=0.5)
    gen = torch.Generator().manual_seed(52)
    x0, w0, gout = 0.8 * torch.randn(n, fin, generator=gen), 0.2 + torch.rand(e, generator=gen), torch.randn(n, fout, generator=gen)
    # fp64: dense normalised adjacency around the oracle's layer function
    P = _state64(conv)
    P.update(_leaves64(conv))
    x64, w64 = x0.double().requires_grad_(True), w0.double().requires_grad_(True)
    src, dst = ei[0], ei[1]
    keep = src != dst
    loop_w = torch.ones(n, dtype=torch.float64).index_put((src[~keep],), w64[~keep])
    ar = torch.arange(n)
    a_src, a_dst, wa = torch.cat([src[keep], ar]), torch.cat([dst[keep], ar]), torch.cat([w64[keep], loop_w])
    dis = torch.zeros(n, dtype=torch.float64).index_add(0, a_dst, wa).pow(-0.5)
    adj = torch.zeros(n, n, dtype=torch.float64).index_put((a_dst, a_src), dis[a_src] * wa * dis[a_dst], accumulate=True)
    want = adj @ _layer64(kind, P, "lin.")(x64) + P["bias"]
    want.backward(gout.double())

    conv = conv.to(DEV).train()
    x, w = x0.to(DEV).requires_grad_(True), w0.to(DEV).requires_grad_(True)
    got = conv(x, ei.to(DEV), w)
    got.backward(gout.to(DEV))
    what = f"{kind} GCN conv, differentiable weights: "
    assert_close(got, want, MODEL_TOL, what=what + "out")
    assert w.grad is not None
    assert_close(w.grad, w64.grad, MODEL_TOL, what=what + "edge_weight.grad")
    assert_close(x.grad, x64.grad, MODEL_TOL, what=what + "x.grad")
    for name, p in conv.named_parameters():
        if p.requires_grad:
            assert_close(p.grad, P[name].grad, MODEL_TOL, what=what + name)
    must_fail(torch.zeros_like(w.grad), w64.grad, MODEL_TOL, what=what + "edge_weight.grad zeroed")
    # the degrees are part of the gradient: the message term alone (weights treated as constants inside dis) is another vector
    with torch.no_grad():
        lin64 = _layer64(kind, P, "lin.")(x64)
        msg_only = torch.zeros(e, dtype=torch.float64)
        msg_only[keep] = (dis[src[keep]] * dis[dst[keep]]).detach() * (gout.double()[dst[keep]] * lin64[src[keep]]).sum(1)
    must_fail(msg_only, w64.grad, MODEL_TOL, what=what + "edge_weight.grad without the degree term")
    # weights that do not require a gradient keep the cached, non-differentiable form -- and agree with it
    plain = conv(x.detach(), ei.to(DEV), w.detach())
    assert_close(plain, want, MODEL_TOL, what=what + "cached form")


# ---------------------------------------------------------------------------------- masks over whole models
class masked_oracle:
    """inside the block ``oracle.gin_conv`` / ``oracle.gcn_conv`` multiply the message of original edge e by ``mask[e]``, the way
    torch_geometric's explain hook does: the GIN self term and GCN's added self loops unmasked, GCN's normalisation the unmasked
    graph's, self loops of the edge list (which GCN drops) untouched by the mask"""

    def __init__(self, mask):
        self.mask = mask

    def __enter__(self):
        self._orig = (orc.gin_conv, orc.gcn_conv)
        mask = self.mask

        def gin_conv(x, edge_index, nn_fn, eps=0.0):
            return nn_fn(orc.sum_aggregate(x, edge_index, edge_weight=mask.to(x.dtype)) + (1.0 + eps) * x)

        def gcn_conv(x, edge_index, lin_fn, bias):
            n = x.size(0)
            ei2, w2 = orc.gcn_norm(edge_index, n, x.dtype)
            keep = edge_index[0] != edge_index[1]
            out = orc.sum_aggregate(lin_fn(x), ei2, n, w2 * torch.cat([mask.to(x.dtype)[keep], torch.ones(n, dtype=x.dtype)]))
            return out if bias is None else out + bias

        orc.gin_conv, orc.gcn_conv = gin_conv, gcn_conv
        return self

    def __exit__(self, *exc):
        orc.gin_conv, orc.gcn_conv = self._orig
        return False


MN, ME, MF, MH, MC = 120, 500, 7, 8, 4


def _make_node_model(kind, conv_type, skip, seed):
    torch.manual_seed(seed)
    if kind == "kan":
        m = kagnn_amd.GKAN_Nodes(conv_type, 2, MF, MH, MC, skip=skip, grid_size=4, spline_order=3, hidden_layers=2)
    elif kind == "fastkan":
        m = kagnn_amd.GFASTKAN_Nodes(conv_type, 2, MF, MH, MC, skip=skip, grid_size=4, hidden_layers=2)
    else:
        m = B.GNN_Nodes(conv_type, 2, MF, MH, MC, skip=skip, hidden_layers=2)
    for name, p in m.named_parameters():
        if p.dim() == 1 and p.requires_grad:
            nn.init.normal_(p, std=0.5)              # biases and norm weights off their 0 / 1 start
    for bn in m.bns:                                 # eval mode must not be a no-op
        bn.running_mean.normal_(std=0.3)
        bn.running_var.uniform_(0.5, 1.5)
    return m


def _bn64(h, S, prefix, training):
    if training:
        return tb._bn64(h, S[prefix + "weight"], S[prefix + "bias"])
    return (h - S[prefix + "running_mean"]) / torch.sqrt(S[prefix + "running_var"] + 1e-5) * S[prefix + "weight"] + S[prefix + "bias"]


def _node_model64(kind, model, S, x, ei, conv_type, skip, training, kinks=None, dtype=torch.float64):
    """logits in ``dtype`` on the CPU from the state ``S``; call it inside ``masked_oracle`` for the masked model"""
    if kind in ("kan", "fastkan"):
        return orc.node_model_forward(x, ei, S, kind, conv_type, 2, 3, skip=skip, training=training)
    outs, h = [x], x
    for i, conv in enumerate(model.convs):
        h = _bn64(tb._conv64(S, f"convs.{i}.", conv, h, ei, kinks), S, f"bns.{i}.", training)
        outs.append(h)
    return (torch.cat(outs, 1) if skip else h) @ S["lay_out.weight"].t() + S["lay_out.bias"]


MASK_CASES = list(itertools.product(("kan", "fastkan", "mlp"), ("gin", "gcn"), (True, False), (True, False)))
MASK_SEEDS = {("mlp", "gin", True, False): 2}      # (kind, conv_type, skip, training) -> seed, where the default seed 0 misses the kink precondition


def _mask_case(kind, conv_type, skip, training):
    seed = MASK_SEEDS.get((kind, conv_type, skip, training), 0)
    model = _make_node_model(kind, conv_type, skip, 60 + seed)
    gen = torch.Generator().manual_seed(61 + seed)
    ei = _edges(62 + seed, MN, ME, 15)
    x, mask = torch.randn(MN, MF, generator=gen), torch.rand(ME, generator=gen)
    gout = torch.randn(MN, MC, generator=gen) / MN
    return model, ei, x, mask, gout


def _mask_reference(kind, model, ei, x, mask, gout, conv_type, skip, training):
    """fp64 logits of the masked model, d (logits * gout).sum() / d mask, and the ReLU inputs seen on the way (MLP baselines)"""
    S = _state64(model)
    m64 = mask.double().requires_grad_(True)
    kinks = []
    with masked_oracle(m64):
        want = _node_model64(kind, model, S, x.double(), ei, conv_type, skip, training, kinks)
    (want * gout.double()).sum().backward()
    return want.detach(), m64.grad, kinks


@pytest.mark.parametrize("kind,conv_type,skip,training", MASK_CASES,
                         ids=[f"{k}-{c}-{'skip' if s else 'noskip'}-{'train' if t else 'eval'}" for k, c, s, t in MASK_CASES])
def test_edge_mask_over_a_node_model(kind, conv_type, skip, training):
    model, ei, x, mask, gout = _mask_case(kind, conv_type, skip, training)
    want, want_grad, kinks = _mask_reference(kind, model, ei, x, mask, gout, conv_type, skip, training)
    tb._kinks_ok(kinks, f"{kind}.{conv_type}")                       # no fp64 pre-activation within 1e-5 of a ReLU kink
    model = model.to(DEV).train(training)
    xd, eid = x.to(DEV), ei.to(DEV)
    what = f"edge_mask {kind} {conv_type} skip={skip} training={training}: "
    plain, names_before = _timed(lambda: model(xd, eid))
    fused_before = [k for k in names_before if k in FUSED_ENTRY_POINTS]
    if kind == "kan" and conv_type == "gin":
        assert fused_before, names_before                             # the default route hides the aggregation
    with kagnn_amd.edge_mask(torch.ones(ME, device=DEV)):
        assert ops.aggregation_visible()
        ones, names_inside = _timed(lambda: model(xd, eid))
    assert not ops.aggregation_visible() and ops.edge_mask_of() is None
    assert not any(k in FUSED_ENTRY_POINTS for k in names_inside) and names_inside.count("kagnn_aggregate_sum") == 2, names_inside
    assert_close(ones, plain, 2e-5, what=what + "all-ones mask vs no mask", elementwise=False)
    md = mask.to(DEV).requires_grad_(True)
    with kagnn_amd.edge_mask(md):
        got = model(xd, eid)
    (got * gout.to(DEV)).sum().backward()
    assert_close(got, want, MODEL_TOL, what=what + "logits")
    assert md.grad is not None
    assert_close(md.grad, want_grad, MODEL_TOL, what=what + "mask.grad")
    must_fail(torch.zeros_like(md.grad), want_grad, MODEL_TOL, what=what + "mask.grad zeroed")
    if conv_type == "gcn":
        loops = ei[0] == ei[1]
        assert bool(loops.any()) and bool((md.grad.cpu()[loops] == 0).all()), "a self loop GCN drops: gradient exactly 0"
    # after the block the fused routes are back and give what they gave
    again, names_after = _timed(lambda: model(xd, eid))
    assert [k for k in names_after if k in FUSED_ENTRY_POINTS] == fused_before, (names_after, names_before)
    assert torch.equal(again, plain)
    with pytest.raises(ValueError, match="edges"):
        with kagnn_amd.edge_mask(torch.ones(ME + 1, device=DEV)):
            model(xd, eid)
    assert not ops.aggregation_visible()


def test_the_fused_norm_and_lazy_norm_routes_step_aside(monkeypatch):
    """GKAN_Nodes('gin') in training mode, wide enough for the one-node convolution + norm and the lazy-norm form between layers
    (``kagnn_gin_kan_layer_fwd_affine``): inside a block both take the per-operation form, afterwards they are back"""
    monkeypatch.setattr(M, "_SPLIT_READOUT_MIN_ROWS", 0)
    monkeypatch.setattr(M, "_SPLIT_READOUT_MIN_ROWS_ONE_LAUNCH", 0)
    n, e = 700, 5600
    torch.manual_seed(3)
    model = kagnn_amd.GKAN_Nodes("gin", 3, 64, 64, 40, skip=True, grid_size=5, spline_order=3, hidden_layers=2).to(DEV).train()
    ei = _edges(70, n, e, 25).to(DEV)
    x = (0.5 * torch.randn(n, 64, generator=torch.Generator().manual_seed(1))).to(DEV)
    plain, names_before = _timed(lambda: model(x, ei))
    assert names_before.count("kagnn_gin_kan_layer_fwd_affine") == 2, names_before          # the lazy-norm route is the default here
    with kagnn_amd.edge_mask(torch.ones(e, device=DEV)):
        ones, names_inside = _timed(lambda: model(x, ei))
    assert not any(k in FUSED_ENTRY_POINTS for k in names_inside) and names_inside.count("kagnn_aggregate_sum") == 3, names_inside
    assert "kagnn_aggregate_sum_affine" not in names_inside
    assert_close(ones, plain, 2e-5, what="lazy-norm model: all-ones mask vs no mask", elementwise=False)
    again, names_after = _timed(lambda: model(x, ei))
    assert [k for k in names_after if k in FUSED_ENTRY_POINTS] == [k for k in names_before if k in FUSED_ENTRY_POINTS]


def test_edge_mask_over_a_graph_level_model():
    """KAGIN is built on the same convolutions: the mask reaches them through ``conv_bn_dropout``; its gradient against central
    differences of the fp32 model itself would be noise, so: an all-ones mask reproduces the unmasked batch, a zero mask equals the
    model on a batch without edges"""
    import types
    n, e = 90, 360
    gen = torch.Generator().manual_seed(80)
    ei = _edges(81, n, e, 10)
    batch = torch.arange(n) // 30
    ei = ei[:, batch[ei[0]] == batch[ei[1]]].contiguous()                # three graphs, edges inside them
    e = ei.size(1)
    d = types.SimpleNamespace(x=torch.randn(n, 5, generator=gen).to(DEV), edge_index=ei.to(DEV), batch=batch.to(DEV), num_graphs=3)
    empty = types.SimpleNamespace(x=d.x, edge_index=ei[:, :0].contiguous().to(DEV), batch=d.batch, num_graphs=3)
    torch.manual_seed(82)
    model = kagnn_amd.KAGIN(2, 5, 8, 3, 2, 4, 3, 0.0).to(DEV).train()
    plain = model(d)
    with kagnn_amd.edge_mask(torch.ones(e, device=DEV)):
        ones = model(d)
    with kagnn_amd.edge_mask(torch.zeros(e, device=DEV)):
        zeros = model(d)
    assert_close(ones, plain, 1e-4, what="KAGIN: all-ones mask vs no mask", elementwise=False)      # (README: fused forms of the graph-level model)
    assert_close(zeros, model(empty), 1e-4, what="KAGIN: zero mask vs no edges", elementwise=False)
    must_fail(zeros, plain, 1e-4, what="KAGIN: zero mask vs all edges", elementwise=False)


# ---------------------------------------------------------------------------------- explain_edges
XN, XE, XF, XC = 60, 300, 6, 3


def _explainer_loop(forward, x, em, fm, target, node_idx, epochs, lr, adam):
    """the loop of ``explain_edges`` restated on CPU tensors of x's dtype: ``forward(h, mask)`` = the masked model's logits"""
    losses = []
    for step in range(1, epochs + 1):
        em.grad = fm.grad = None
        m, f = torch.sigmoid(em), torch.sigmoid(fm)
        logits = forward(x * f, m)
        lg, tg = (logits, target) if node_idx is None else (logits[node_idx].reshape(1, -1), target[node_idx].reshape(1))
        ent = lambda p: -p * torch.log(p + 1e-15) - (1.0 - p) * torch.log(1.0 - p + 1e-15)
        loss = F.cross_entropy(lg, tg) + 0.005 * m.sum() + 1.0 * ent(m).mean() + 1.0 * f.mean() + 0.1 * ent(f).mean()
        loss.backward()
        adam(step, lr)
        losses.append(loss.detach())
    return torch.sigmoid(em).detach(), torch.sigmoid(fm).detach().reshape(-1), torch.stack(losses)


@pytest.mark.parametrize("conv_type,node_idx", [("gin", None), ("gin", 17), ("gcn", None), ("gcn", 17)])
def test_explain_edges(conv_type, node_idx):
    epochs, lr = 5, 0.01
    torch.manual_seed(90)
    model = kagnn_amd.GKAN_Nodes(conv_type, 2, XF, 8, XC, skip=True, grid_size=4, spline_order=3, hidden_layers=2)
    for bn in model.bns:
        bn.running_mean.normal_(std=0.3)
        bn.running_var.uniform_(0.5, 1.5)
    ei = _edges(91, XN, XE, 8)
    x = torch.randn(XN, XF, generator=torch.Generator().manual_seed(92))
    model = model.to(DEV).train()
    model.bns[1].eval()
    flags = [m.training for m in model.modules()]
    before = {k: v.clone() for k, v in model.state_dict().items()}
    xd, eid = x.to(DEV), ei.to(DEV)
    run = lambda: kagnn_amd.explain_edges(model, xd, eid, node_idx=node_idx, epochs=epochs, lr=lr, generator=torch.Generator().manual_seed(5))
    a, b = run(), run()
    for key in ("edge_mask", "feature_mask", "losses"):
        assert a[key].device.type == "cuda" and torch.equal(a[key], b[key]), key          # same seed, same bits
    assert a["edge_mask"].shape == (XE,) and a["feature_mask"].shape == (XF,) and a["losses"].shape == (epochs,)
    assert bool(torch.isfinite(a["losses"]).all())
    assert [m.training for m in model.modules()] == flags
    after = model.state_dict()
    assert all(torch.equal(after[k], v) for k, v in before.items()) and all(p.grad is None for p in model.parameters())
    assert not ops.aggregation_visible()

    # the same loop in fp64 (Adam restated) and in fp32 with torch's own Adam, both on the CPU, from the same initial logits
    gen = torch.Generator().manual_seed(5)
    em0 = 1.0 + math.sqrt(2.0) * math.sqrt(2.0 / (2 * XN)) * torch.randn(XE, generator=gen)
    fm0 = 0.1 * torch.randn(1, XF, generator=gen)
    model.eval()
    with torch.no_grad():
        target = model(xd, eid).argmax(-1).cpu()
    model.train()
    res = {}
    for dtype in (torch.float64, torch.float32):
        S = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in _state64(model).items()}
        em, fm = em0.to(dtype).clone().requires_grad_(True), fm0.to(dtype).clone().requires_grad_(True)

        def forward(h, m):
            with masked_oracle(m):
                return orc.node_model_forward(h, ei, S, "kan", conv_type, 2, 3, skip=True, training=False)

        if dtype == torch.float64:
            mom = [[torch.zeros_like(p), torch.zeros_like(p)] for p in (em, fm)]

            def adam(step, lr, b1=0.9, b2=0.999, eps=1e-8):
                with torch.no_grad():
                    for p, (m1, m2) in zip((em, fm), mom):
                        m1.mul_(b1).add_(p.grad, alpha=1 - b1)
                        m2.mul_(b2).addcmul_(p.grad, p.grad, value=1 - b2)
                        p.sub_(lr * (m1 / (1 - b1 ** step)) / ((m2 / (1 - b2 ** step)).sqrt() + eps))
        else:
            opt = torch.optim.Adam([em, fm], lr=lr)
            adam = lambda step, lr: opt.step()
        res[dtype] = _explainer_loop(forward, x.to(dtype), em, fm, target, node_idx, epochs, lr, adam)
    e64, f64, l64 = res[torch.float64]
    e32, f32, _ = res[torch.float32]
    dev_e = float((e32.double() - e64).abs().max() / e64.abs().max())
    dev_f = float((f32.double() - f64).abs().max() / f64.abs().max())
    print(f"explain_edges {conv_type} node_idx={node_idx}: fp32 CPU restatement vs fp64: edge mask {dev_e:.3e}, feature mask {dev_f:.3e}; "
          f"device vs fp64: edge mask {float((a['edge_mask'].double().cpu() - e64).abs().max() / e64.abs().max()):.3e}, "
          f"feature mask {float((a['feature_mask'].double().cpu() - f64).abs().max() / f64.abs().max()):.3e}")
    assert_close(a["edge_mask"], e64, max(1e-4, 4 * dev_e), what=f"explain_edges {conv_type}: edge mask", elementwise=False)
    assert_close(a["feature_mask"], f64, max(1e-4, 4 * dev_f), what=f"explain_edges {conv_type}: feature mask", elementwise=False)
    assert_close(a["losses"], l64, max(1e-4, 4 * max(dev_e, dev_f)), what=f"explain_edges {conv_type}: losses", elementwise=False)
    # the masks moved: five Adam steps of 0.01 on the logits are far above the tolerance
    must_fail(torch.sigmoid(em0), e64, 1e-4, what="explain_edges: the initial edge mask", elementwise=False)
