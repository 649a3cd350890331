"""Which configurations the fused host routes accept, as a table, on the CPU: ``ops._chain_plan`` (the GIN / GINE one-call layer nodes),
``graph_ops._gine_stack_plan`` (the GINE stack node), ``graph_ops.kagin_regression_forward`` (the whole-model node),
``KAN._pack_chain`` and ``KANLinear.read_out_blocks_in_one_launch``.  Every one of them hands a layer's raw parameters to a library
call, so every one of them has to decline a layer that is no longer the plain reference layer.  No launch: the plans are host code,
and where a route would go on to the device the test stops it at the first device step (``_Reached``)."""
import pytest
import torch

import kagnn_amd
from kagnn_amd import graph_ops, ops
from kagnn_amd.graph_models import GINEKANLayer
from kagnn_amd.models import make_kan
from kagnn_amd.norm import BatchNorm1d

CPU = torch.device("cpu")


@pytest.fixture(autouse=True)
def _default_precision(monkeypatch):
    monkeypatch.delenv("KAGNN_PRECISION", raising=False)          # the default: split


def _fix(layer):
    layer.fix_symbolic(0, 0, "0")


def _unfix(layer):
    layer.unfix_symbolic(0, 0)


# ---------------------------------------------------------------------------------- ops._chain_plan
def _chain(widths=(4, 4, 4), **kw):
    torch.manual_seed(0)
    return kagnn_amd.KAN(list(widths), **kw)


def _fp32(chain, which):
    for i in which:
        chain.layers[i].precision = ops.PREC_FP32


def _scale_grid(layer):
    with torch.no_grad():
        layer.grid.mul_(2.0)
    layer.refresh_knots()


def _per_feature_knots(layer):
    with torch.no_grad():
        layer.grid[1, 2] += 0.01
    layer.refresh_knots()
    assert layer._knots().dim() == 2


def _no_scaler(chain, i):
    old = chain.layers[i]
    torch.manual_seed(1)
    chain.layers[i] = kagnn_amd.KANLinear(old.in_features, old.out_features, grid_size=old.grid_size, spline_order=old.spline_order,
                                          enable_standalone_scale_spline=False)


CHAIN_ROWS = {
    "plain": (dict(), None, True),
    "both-fp32": (dict(), lambda c: _fp32(c, (0, 1)), True),
    "G+K=16": (dict(grid_size=12, spline_order=4), None, True),
    "G+K=17": (dict(grid_size=13, spline_order=4), None, False),
    "mixed-precision": (dict(), lambda c: _fp32(c, (1,)), False),
    "one-grid-scaled": (dict(), lambda c: _scale_grid(c.layers[1]), False),
    "per-feature-knots": (dict(), lambda c: _per_feature_knots(c.layers[0]), False),
    "wider-than-7680": (dict(widths=(7684, 4)), None, False),
    "order-5": (dict(spline_order=5), None, False),
    "no-scaler": (dict(), lambda c: _no_scaler(c, 1), False),
    "fixed-edge-first": (dict(), lambda c: _fix(c.layers[0]), False),
    "fixed-edge-last": (dict(), lambda c: _fix(c.layers[1]), False),
}


@pytest.mark.parametrize("row", list(CHAIN_ROWS))
def test_chain_plan(row):
    kw, change, accepted = CHAIN_ROWS[row]
    chain = _chain(**kw)
    if change is not None:
        change(chain)
    plan = ops._chain_plan(list(chain.layers))
    assert (plan is not None) is accepted, row
    if accepted:
        mode, knots, params = plan
        want = ops.PREC_FP32 if row == "both-fp32" else ops.PREC_SPLIT
        assert mode == want and len(knots) == len(chain.layers) and all(k.dim() == 1 and torch.equal(k, knots[0]) for k in knots)
        flat = []
        for l in chain.layers:
            flat += [l.base_weight, l.spline_weight, l.spline_scaler]
        assert len(params) == len(flat) and all(a is b for a, b in zip(params, flat))


def test_chain_plan_accepts_again_after_unfix():
    chain = _chain()
    for i in (0, 1):
        _fix(chain.layers[i])
        assert ops._chain_plan(list(chain.layers)) is None
        _unfix(chain.layers[i])
        assert ops._chain_plan(list(chain.layers)) is not None


# ---------------------------------------------------------------------------------- graph_ops._gine_stack_plan
def _stack(nconv=2, H=16, nl=2, grid=4, order=3):
    torch.manual_seed(0)
    convs = [GINEKANLayer(make_kan(H, H, H, nl, grid, order)) for _ in range(nconv)]
    bns = [BatchNorm1d(H) for _ in range(nconv)]
    return convs, bns


def _stack_plan(convs, bns, H=16):
    return graph_ops._gine_stack_plan(graph_ops._ShapeOnly(10, H, CPU), convs, bns)


def _stack_no_scaler(convs, c, i):
    _no_scaler(convs[c].nn, i)


STACK_ROWS = {
    "plain": (dict(), None, True),
    "four-convs-H64": (dict(nconv=4, H=64), None, True),
    "eight-convs": (dict(nconv=8), None, True),
    "order-5": (dict(order=5), None, False),
    "order-2": (dict(order=2), None, False),
    "grid-6": (dict(grid=6), None, False),
    "H-65": (dict(H=65), None, False),
    "one-norm-eval": (dict(), lambda cv, bn: bn[1].eval(), False),
    "one-norm-not-affine": (dict(), lambda cv, bn: bn.__setitem__(0, BatchNorm1d(16, affine=False)), False),
    "one-norm-other-width": (dict(), lambda cv, bn: bn.__setitem__(1, BatchNorm1d(8)), False),
    "single-conv": (dict(nconv=1), None, False),
    "nine-convs": (dict(nconv=9), None, False),
    "one-grid-scaled": (dict(), lambda cv, bn: _scale_grid(cv[1].nn.layers[0]), False),
    "per-feature-knots": (dict(), lambda cv, bn: _per_feature_knots(cv[0].nn.layers[1]), False),
    "one-layer-fp32": (dict(), lambda cv, bn: _fp32(cv[1].nn, (1,)), False),
    "all-layers-fp32": (dict(), lambda cv, bn: [_fp32(c.nn, (0, 1)) for c in cv], False),
    "chains-of-other-lengths": (dict(), lambda cv, bn: cv.__setitem__(1, GINEKANLayer(make_kan(16, 16, 16, 3, 4, 3))), False),
    "chain-not-square": (dict(), lambda cv, bn: cv.__setitem__(1, GINEKANLayer(make_kan(16, 8, 16, 2, 4, 3))), False),
    "no-scaler": (dict(), lambda cv, bn: _stack_no_scaler(cv, 1, 0), False),
    "fixed-edge-conv0-layer0": (dict(), lambda cv, bn: _fix(cv[0].nn.layers[0]), False),
    "fixed-edge-conv0-layer1": (dict(), lambda cv, bn: _fix(cv[0].nn.layers[1]), False),
    "fixed-edge-conv1-layer0": (dict(), lambda cv, bn: _fix(cv[1].nn.layers[0]), False),
    "fixed-edge-conv1-layer1": (dict(), lambda cv, bn: _fix(cv[1].nn.layers[1]), False),
}


@pytest.mark.parametrize("row", list(STACK_ROWS))
def test_gine_stack_plan(row):
    kw, change, accepted = STACK_ROWS[row]
    convs, bns = _stack(**kw)
    if change is not None:
        change(convs, bns)
    plan = _stack_plan(convs, bns, kw.get("H", 16))
    assert (plan is not None) is accepted, row
    if accepted:
        first, nl, mode = plan
        assert first is convs[0].nn.layers[0] and nl == 2 and mode == ops.PREC_SPLIT


def test_gine_stack_plan_wants_fp32_device_rows_and_its_switches(monkeypatch):
    convs, bns = _stack()
    assert _stack_plan(convs, bns) is not None
    assert graph_ops._gine_stack_plan(torch.zeros(10, 16), convs, bns) is None                 # not on the device
    assert graph_ops._gine_stack_plan(graph_ops._ShapeOnly(1, 16, CPU), convs, bns) is None     # one row: no batch statistics
    for flag in ("_GINE_STACK_ABI", "_GINE_LAYER_ABI"):
        monkeypatch.setattr(graph_ops, flag, False)
        assert _stack_plan(convs, bns) is None
        monkeypatch.setattr(graph_ops, flag, True)
    assert _stack_plan(convs, bns) is not None


def test_gine_stack_plan_accepts_again_after_unfix():
    convs, bns = _stack()
    for c in (0, 1):
        for i in (0, 1):
            layer = convs[c].nn.layers[i]
            _fix(layer)
            assert _stack_plan(convs, bns) is None
            _unfix(layer)
            assert _stack_plan(convs, bns) is not None


# ---------------------------------------------------------------------------------- KAN._pack_chain, read_out_blocks_in_one_launch
def test_pack_chain_declines_a_fixed_edge_and_accepts_again(monkeypatch):
    chain = _chain()
    asked = []
    monkeypatch.setattr(ops, "kan_pack_chain", lambda layers, G, K, mode: (asked.append((layers, G, K, mode)), "packs")[1])
    x = torch.zeros(5, 4)
    assert chain._pack_chain(x) == "packs"
    layers, G, K, mode = asked.pop()
    assert (G, K, mode) == (5, 3, ops.PREC_SPLIT)
    assert all(got[j] is want for got, l in zip(layers, chain.layers) for j, want in enumerate((l.base_weight, l.spline_weight, l.spline_scaler)))
    for i in (0, 1):
        _fix(chain.layers[i])
        assert chain._pack_chain(x) is None and not asked
        _unfix(chain.layers[i])
        assert chain._pack_chain(x) == "packs" and asked.pop()
    _per_feature_knots(chain.layers[1])
    assert chain._pack_chain(x) is None and not asked
    other = _chain()
    _fp32(other, (0, 1))
    assert other._pack_chain(x) is None and not asked             # the packs are the split kernels'
    assert _chain(spline_order=5)._pack_chain(x) is None and not asked
    chain = _chain()
    _no_scaler(chain, 0)
    assert chain._pack_chain(x) == "packs" and asked.pop()[0][0][2] is None


def test_read_out_blocks_in_one_launch_declines_a_fixed_edge_and_accepts_again():
    torch.manual_seed(0)
    layer = kagnn_amd.KANLinear(192, 8, grid_size=4)
    widths = (64, 128)
    assert layer.read_out_blocks_in_one_launch(widths) is True
    _fix(layer)
    assert layer.read_out_blocks_in_one_launch(widths) is False
    _unfix(layer)
    assert layer.read_out_blocks_in_one_launch(widths) is True
    assert layer.read_out_blocks_in_one_launch((64, 64)) is False     # the blocks do not add up to in_features
    layer.precision = ops.PREC_FP32
    assert layer.read_out_blocks_in_one_launch(widths) is False
    layer.precision = None
    _per_feature_knots(layer)
    assert layer.read_out_blocks_in_one_launch(widths) is False
    assert kagnn_amd.KANLinear(192, 8, grid_size=4, spline_order=5).read_out_blocks_in_one_launch(widths) is False


# ---------------------------------------------------------------------------------- graph_ops.kagin_regression_forward
class _Reached(Exception):
    """every host-side condition of the whole-model node held: the next step is the batch's graph index, on the device"""


def _regression_model(monkeypatch, nconv=2, H=16):
    torch.manual_seed(0)
    model = kagnn_amd.KAGINRegression(1, 1, nconv, H, 2, 4, 3, 1, 0.0, True).train()
    model.atom_encoder = kagnn_amd.graph_models.AtomEncoder(H, [21])
    model.bond_encoder.bond_embedding_list = torch.nn.ModuleList([torch.nn.Embedding(4, H)])
    # the encoders' own condition (int64 features ON THE DEVICE) is not what is under test: hand their tables over as they would
    model.atom_encoder._fast_tables = lambda x: [t.weight for t in model.atom_encoder.atom_embedding_list]
    model.bond_encoder._fast_tables = lambda e: [t.weight for t in model.bond_encoder.bond_embedding_list]

    def reached(data, n):
        raise _Reached
    monkeypatch.setattr(graph_ops, "batch_graph_index", reached)
    from types import SimpleNamespace
    data = SimpleNamespace(x=torch.zeros(10, 1, dtype=torch.int64), edge_attr=torch.zeros(20, dtype=torch.int64),
                           edge_index=torch.zeros(2, 20, dtype=torch.int64), batch=torch.zeros(10, dtype=torch.int64), num_graphs=1)
    return model, data


def _accepted(model, data):
    try:
        out = graph_ops.kagin_regression_forward(model, data)
    except _Reached:
        return True
    assert out is None
    return False


@pytest.mark.parametrize("where", ["conv.0.nn.layers.0", "conv.1.nn.layers.0", "conv.1.nn.layers.1", "kan.layers.0", "kan.layers.1"])
def test_kagin_regression_forward_declines_a_fixed_edge(monkeypatch, where):
    model, data = _regression_model(monkeypatch)
    assert _accepted(model, data)
    layer = dict(model.named_modules())[where]
    _fix(layer)
    assert not _accepted(model, data)
    _unfix(layer)
    assert _accepted(model, data)


def test_kagin_regression_forward_other_refusals_and_what_the_read_out_may_differ_in(monkeypatch):
    model, data = _regression_model(monkeypatch)
    ro = model.kan.layers
    # per-layer precision, per-layer (uniform) knots and an absent scaler are the read-out's to have
    ro[0].precision = ops.PREC_FP32
    _scale_grid(ro[1])
    assert _accepted(model, data)
    _no_scaler(model.kan, 1)
    assert _accepted(model, data)
    _per_feature_knots(ro[0])
    assert not _accepted(model, data)
    model, data = _regression_model(monkeypatch)
    handle = model.conv[1].nn.layers[0].register_forward_hook(lambda *a: None)
    assert not _accepted(model, data)
    handle.remove()
    assert _accepted(model, data)
    model.eval()
    assert not _accepted(model, data)
    model.train()
    model.dropout.p = 0.5
    assert not _accepted(model, data)
    model.dropout.p = 0.0
    _scale_grid(model.conv[0].nn.layers[1])
    assert not _accepted(model, data)
    assert not _accepted(*_regression_model(monkeypatch, nconv=1))
    model, data = _regression_model(monkeypatch)
    model.kan = make_kan(16, 16, 1, 2, 4, 5)                       # a read-out at order 5
    assert not _accepted(model, data)
    monkeypatch.setattr(graph_ops, "_GINE_MODEL_NODE", False)
    assert not _accepted(*_regression_model(monkeypatch))
