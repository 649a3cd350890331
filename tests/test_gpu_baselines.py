"""The MLP baselines (kagnn_amd/baselines.py) against fp64 on the CPU.

The message passing of the reference comes from ``oracle.kan_oracle`` (``gin_conv``, ``gcn_conv``, ``gat_conv``, ``gine_conv``,
``global_add_pool``, ``global_mean_pool``: they take the transform as a callable); the transform is an fp64 copy of the module's own
parameters.  Convolutions are held to ``helpers.assert_close``'s default; whole models -- logits or predictions and EVERY parameter
gradient -- to 1e-4 of each tensor's own maximum, the whole-model rule of tests/test_gpu_models.py, with the same two noise floors
(``helpers.gat_att_noise`` for att_src / att_dst; a bias added right in front of a training-mode BatchNorm1d has an identically
zero gradient in exact arithmetic: 1e-4 of the largest gradient of its convolution, as ``helpers.prenorm_bias_noise`` reasons).

Kink precondition: every model test computes, on the fp64 side alone, the smallest |z| over all ReLU (and GAT leaky-ReLU)
inputs and asserts that it exceeds 1e-5 of the largest; the seeds below were picked on the CPU so that it does.

Shapes: 300 nodes (the last ten isolated), 1200 edges, widths <= 16; mini-batches of 6 graphs, one of them empty.
"""
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from kagnn_amd import baselines as B
from kagnn_amd import harness
from oracle import kan_oracle as orc
from helpers import assert_close, gat_att_noise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, E, FIN = 300, 1200, 11
MODEL_TOL = 1e-4
KINK = 1e-5


def _graph(seed):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, N - 10, (2, E), generator=g)              # nodes N-10 .. N-1 stay isolated
    x = torch.randn(N, FIN, generator=g)
    return x, ei


def _batch(seed, edge_width=None):
    """6 graphs in one disjoint union, graph 2 empty"""
    g = torch.Generator().manual_seed(seed)
    sizes = [60, 45, 0, 70, 55, 70]
    assert sum(sizes) == N
    srcs, dsts, batch, lo = [], [], [], 0
    for b, s in enumerate(sizes):
        if s:
            e = 4 * s
            srcs.append(lo + torch.randint(0, s, (e,), generator=g))
            dsts.append(lo + torch.randint(0, s, (e,), generator=g))
            batch.append(torch.full((s,), b, dtype=torch.int64))
        lo += s
    ei = torch.stack([torch.cat(srcs), torch.cat(dsts)])
    d = types.SimpleNamespace(x=torch.randn(N, FIN, generator=g), edge_index=ei, batch=torch.cat(batch), num_graphs=len(sizes))
    if edge_width:
        d.edge_attr = torch.randn(ei.size(1), edge_width, generator=g)
    d.y = torch.randint(0, 3, (len(sizes),), generator=g)
    return d


def _to(d, dev):
    return types.SimpleNamespace(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in vars(d).items()})


def _params64(module):
    return {k: p.detach().double().cpu().requires_grad_(True) for k, p in module.named_parameters()}


def _bn64(x, w, b, eps=1e-5):
    mean, var = x.mean(0), x.var(0, unbiased=False)
    return (x - mean) / torch.sqrt(var + eps) * w + b


def _seq64(P, prefix, seq, x, kinks):
    """an fp64 make_mlp chain: the structure (which blocks carry a ReLU / a BatchNorm1d) is the module's own, pinned by
    tests/test_baselines_host.py"""
    for i, block in enumerate(seq):
        z = x @ P[f"{prefix}{i}.0.weight"].t() + P[f"{prefix}{i}.0.bias"]
        if len(block) > 1:
            assert isinstance(block[1], nn.ReLU)
            kinks.append(z)
            x = F.relu(z)
        else:
            x = z
        if len(block) > 2:
            x = _bn64(x, P[f"{prefix}{i}.2.weight"], P[f"{prefix}{i}.2.bias"])
    return x


def _conv64(P, prefix, conv, x, ei, kinks, edge_attr=None):
    if isinstance(conv, B.GINEConv):
        kinks.append(x.index_select(0, ei[0]) + edge_attr)
        return orc.gine_conv(x, ei, edge_attr, lambda h: _seq64(P, prefix + "nn.", conv.nn, h, kinks))
    if isinstance(conv, B.GINConv):
        return orc.gin_conv(x, ei, lambda h: _seq64(P, prefix + "nn.", conv.nn, h, kinks))
    lin = lambda h: h @ P[prefix + "lin.weight"].t()
    if isinstance(conv, B.GCNConv):
        return orc.gcn_conv(x, ei, lin, P[prefix + "bias"])
    h = conv.heads
    xh = lin(x).view(x.size(0), h, -1)
    a_s = (xh * P[prefix + "att_src"].view(1, h, -1)).sum(-1)
    a_d = (xh * P[prefix + "att_dst"].view(1, h, -1)).sum(-1)
    keep = ei[0] != ei[1]
    ar = torch.arange(x.size(0))
    kinks.append(a_s[torch.cat([ei[0][keep], ar])] + a_d[torch.cat([ei[1][keep], ar])])      # the leaky ReLU's inputs
    ATT_SCALE.append(float(xh.detach().abs().max()) * max(1.0, float(kinks[-1].detach().abs().max())))   # helpers.gat_att_noise
    return orc.gat_conv(x, ei, lin, P[prefix + "att_src"], P[prefix + "att_dst"], P[prefix + "bias"], h)


ATT_SCALE = []


def _kinks_ok(kinks, what):
    if not kinks:
        return
    z = torch.cat([k.detach().reshape(-1) for k in kinks]).abs()
    assert float(z.min()) > KINK * float(z.max()), f"{what}: a pre-activation within {KINK} of the kink (pick another seed): {float(z.min())}, {float(z.max())}"


def _compare(model, got_out, P, want_out, gout, what, tol, n_nodes):
    att_scale = max(ATT_SCALE, default=1.0)
    del ATT_SCALE[:]
    (want_out * gout.double()).sum().backward()
    wants = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in P.items()}
    assert_close(got_out, want_out, tol, what=f"{what}.out")
    for name, p in model.named_parameters():
        assert p.grad is not None, name
        noise = 0.0
        if name.endswith("att_src") or name.endswith("att_dst"):
            noise = gat_att_noise(n_nodes, att_scale)
        elif name in getattr(model, "_prenorm_biases", ()):
            pre = name.split(".")[0] + "." + name.split(".")[1] + "."
            noise = 1e-4 * max(float(v.abs().max()) for k, v in wants.items() if k.startswith(pre))
        assert_close(p.grad, wants[name], tol, what=f"{what}.grad.{name}", noise=noise)


# ------------------------------------------------------------------ convolutions
CONV_SEEDS = {'gine': 5}      # kind -> seed, where the default seed 0 misses the kink precondition


@pytest.mark.parametrize("kind", ["gin", "gine", "gcn", "gat"])
def test_convolution_against_the_oracle(kind):
    seed = CONV_SEEDS.get(kind, 0)
    torch.manual_seed(11 + seed)
    x, ei = _graph(5 + seed)
    width = 16
    if kind == "gin":
        conv = B.GINConv(B.make_mlp_nodes(FIN, 16, width, 2))
    elif kind == "gine":
        conv = B.GINEConv(B.make_mlp(FIN, 16, width, 3, batch_norm=True))
    elif kind == "gcn":
        conv = B.GCNConv(FIN, width)
        nn.init.normal_(conv.bias)
    else:
        conv = B.GATConv(FIN, 8, 2)
        nn.init.normal_(conv.bias)
    ea = torch.randn(E, FIN, generator=torch.Generator().manual_seed(6)) if kind == "gine" else None
    P = _params64(conv)
    x64 = x.double().requires_grad_(True)
    kinks = []
    want = _conv64(P, "", conv, x64, ei, kinks, None if ea is None else ea.double())
    _kinks_ok(kinks, kind)
    gout = torch.randn(N, width, generator=torch.Generator().manual_seed(7))
    (want * gout.double()).sum().backward()
    _kinks_ok(kinks, kind)
    conv = conv.to(DEV).train()
    xd = x.to(DEV).requires_grad_(True)
    got = conv(xd, ei.to(DEV), ea.to(DEV)) if kind == "gine" else conv(xd, ei.to(DEV))
    got.backward(gout.to(DEV))
    assert_close(got, want, what=f"{kind}.y")
    assert_close(xd.grad, x64.grad, what=f"{kind}.gx")
    for name, p in conv.named_parameters():
        noise = gat_att_noise(N, max(ATT_SCALE, default=1.0)) if name in ("att_src", "att_dst") else 0.0
        assert_close(p.grad, P[name].grad, what=f"{kind}.grad.{name}", noise=noise)


# ------------------------------------------------------------------ node model
NODE_SEEDS = {('gin', True, 4): 4, ('gin', False, 4): 2}      # (conv_type, skip, hidden_layers) -> seed, where the default seed 0 misses the kink precondition


@pytest.mark.parametrize("hidden_layers", [1, 2, 4])
@pytest.mark.parametrize("skip", [True, False], ids=["skip", "noskip"])
@pytest.mark.parametrize("conv_type", ["gin", "gcn", "gat"])
def test_gnn_nodes_against_fp64(conv_type, skip, hidden_layers):
    seed = NODE_SEEDS.get((conv_type, skip, hidden_layers), 0)
    torch.manual_seed(100 + seed)
    x, ei = _graph(20 + seed)
    model = B.GNN_Nodes(conv_type, 2, FIN, 8, 5, skip=skip, hidden_layers=hidden_layers, dropout=0.0, heads=2)
    for p in model.parameters():
        if p.dim() == 1:
            nn.init.normal_(p, std=0.5)                  # biases and norm weights off their 0 / 1 start
    P = _params64(model)
    kinks, outs = [], [x.double()]
    h = outs[0]
    for i, conv in enumerate(model.convs):
        h = _bn64(_conv64(P, f"convs.{i}.", conv, h, ei, kinks), P[f"bns.{i}.weight"], P[f"bns.{i}.bias"])
        outs.append(h)
    want = (torch.cat(outs, 1) if skip else h) @ P["lay_out.weight"].t() + P["lay_out.bias"]
    _kinks_ok(kinks, f"GNN_Nodes.{conv_type}")
    # the biases added right in front of a BatchNorm1d: the conv bias of gcn / gat, the last Linear of a gin chain of >= 2 layers
    # (a one-layer chain ends in a ReLU, its bias gradient is not zero)
    if conv_type != "gin":
        model._prenorm_biases = [f"convs.{i}.bias" for i in range(2)]
    elif hidden_layers >= 2:
        model._prenorm_biases = [f"convs.{i}.nn.{hidden_layers - 1}.0.bias" for i in range(2)]
    gout = torch.randn(N, 5, generator=torch.Generator().manual_seed(3)) / N
    model = model.to(DEV).train()
    got = model(x.to(DEV), ei.to(DEV))
    got.backward(gout.to(DEV))
    _compare(model, got, P, want, gout, f"GNN_Nodes.{conv_type}.{skip}.{hidden_layers}", MODEL_TOL, N)


# ------------------------------------------------------------------ graph-level models
def _graph_model_reference(model, P, d, kinks):
    x = d.x.double()
    ea = None
    if hasattr(model, "atom_encoder"):
        x = x @ P["atom_encoder.weight"].t() + P["atom_encoder.bias"]
    if hasattr(model, "bond_encoder"):
        ea = d.edge_attr.double() @ P["bond_encoder.weight"].t() + P["bond_encoder.bias"]
    gin = isinstance(model, (B.GIN, B.GINRegression))
    for i, conv in enumerate(model.conv):
        x = _conv64(P, f"conv.{i}.", conv, x, d.edge_index, kinks, ea)
        if not gin:
            x = F.silu(x)
    mean = isinstance(model, B.GCN)
    pooled = (orc.global_mean_pool if mean else orc.global_add_pool)(x, d.batch, d.num_graphs)
    out = _seq64(P, "mlp." if gin else "readout.", model.mlp if gin else model.readout, pooled, kinks)
    return F.log_softmax(out, dim=1) if isinstance(model, (B.GIN, B.GCN, B.GAT)) else out


GRAPH_MODELS = {
    "GIN": lambda: B.GIN(2, FIN, 16, 3, 3, 0.0),
    "GCN": lambda: B.GCN(2, FIN, 16, 3, 0.0),
    "GAT": lambda: B.GAT(2, FIN, 8, 3, 0.0, 2),
    "GINRegression": lambda: B.GINRegression(FIN, 4, 2, 16, 2, 1, 0.0, False),
    "GCNRegression": lambda: B.GCNRegression(FIN, 2, 16, 1, 0.0, False),
}
GRAPH_SEEDS = {'GIN': 4, 'GINRegression': 8}     # name -> seed, where the default seed 0 misses the kink precondition


@pytest.mark.parametrize("name", list(GRAPH_MODELS))
def test_graph_model_against_fp64(name):
    seed = GRAPH_SEEDS.get(name, 0)
    torch.manual_seed(200 + seed)
    d = _batch(40 + seed, edge_width=4 if name == "GINRegression" else None)
    model = GRAPH_MODELS[name]()
    for p in model.parameters():
        if p.dim() == 1:
            nn.init.normal_(p, std=0.5)
    if hasattr(model, "mlp"):
        # add-pooled sums over up to 70 nodes feed the read-out: bring its first layer's pre-activations back to the scale of the
        # node-level ones (the kink precondition is relative to the LARGEST pre-activation of the model)
        with torch.no_grad():
            model.mlp[0][0].weight.mul_(1.0 / 16)
    P = _params64(model)
    kinks = []
    want = _graph_model_reference(model, P, d, kinks)
    _kinks_ok(kinks, name)
    gout = torch.randn(want.shape, generator=torch.Generator().manual_seed(4))
    model = model.to(DEV).train()
    got = model(_to(d, DEV))
    got.backward(gout.to(DEV))
    _compare(model, got, P, want, gout, name, MODEL_TOL, N)


# ------------------------------------------------------------------ the loops take the new modules
def test_one_epoch_of_the_node_classification_loop():
    torch.manual_seed(1)
    x, ei = _graph(2)
    y = torch.randint(0, 5, (N,))
    masks = [torch.rand(N) < 0.4 for _ in range(3)]
    model = B.GNN_Nodes("gin", 2, FIN, 8, 5).to(DEV)
    res = harness.train_node_classification(model, x.to(DEV), ei.to(DEV), y.to(DEV), *[m.to(DEV) for m in masks], epochs=1, lr=1e-2)
    assert res.epochs_run == 1
    for v in (res.train_acc, res.val_acc, res.val_loss, res.test_acc):
        assert v == v and abs(v) != float("inf"), res
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_one_epoch_of_the_graph_classification_loop():
    torch.manual_seed(2)
    loader = [_to(_batch(s), DEV) for s in (1, 2)]
    model = B.GIN(2, FIN, 16, 2, 3, 0.0).to(DEV)
    sec, losses = harness.train_graph_classification(model, loader, nb_epochs=1, lr=1e-3)
    assert len(losses) == 1 and losses[0] == losses[0] and abs(losses[0]) != float("inf") and sec > 0
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_make_any_model_builds_the_baseline():
    params = dict(architecture="mlp", conv_type="gcn", mp_layers=2, num_features=FIN, hidden_channels=8, num_classes=5, skip=True,
                  hidden_layers=2, dropout=0.0, grid_size=4, spline_order=3)
    m = harness.make_any_model(params)
    assert type(m) is B.GNN_Nodes and isinstance(m.lay_out, B.Linear)
    out = m.to(DEV)(*[t.to(DEV) for t in _graph(3)])
    assert out.shape == (N, 5) and bool(torch.isfinite(out).all())
    assert type(harness.make_any_model(dict(params, architecture="kan"))).__name__ == "GKAN_Nodes"
