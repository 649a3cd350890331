"""KAGNN_PREC_HALF -- the build-defined reduced-precision mode of BASELINE config 2 (the reference is fp32 only, ekan.py:154-162):
the split-precision kernels with ONE fp16 product per fp32 product.  Parity statement: the HIP path agrees with the oracle fed the
SAME once-rounded operands (tests/helpers.py: half_mode_oracle) -- 5e-5 in L2, 3e-4 in the max norm (isolated rounding-tie flips), and at least
5x closer than the unrounded oracle (observed: 20-60x); its distance from the unrounded fp64
oracle (~3e-4, fp16's 2^-11 per operand) is a property of the mode, bounded and reported here (gpurun_out/half_mode_errors.json)."""
# The mode is not one kernel: which of a layer's three GEMMs has a single-product instantiation is a routing table
# (tests/helpers.py: half_routing), and every case below writes down the class it expects of each tensor -- single-product tensors
# meet the statement above, three-product tensors the ordinary fp64 bound AND the bits of PREC_SPLIT (helpers.half_statement).
# tests/test_gpu_half_variants.py: one case per single-product instantiation, edge inputs, and the graph-level one-call paths.
import json
import os

import pytest
import torch

import kagnn_amd
from kagnn_amd import ops
from oracle import kan_oracle as orc
from helpers import (HALF_FLIP_TOL as FLIP_TOL, HALF_L2_TOL as L2_TOL, HALF_MODE_CEIL as MODE_CEIL, HALF_MODE_FLOOR as MODE_FLOOR,
                     HALF_REPORT as REPORT, check, half_classes, half_layer_oracles, half_mode_oracle, half_parity as _parity, half_routing,
                     half_statement, kanlinear_fwd_bwd, oracle_node_model_fwd_bwd, prenorm_bias_noise)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# L2_TOL / FLIP_TOL: the mode's two-norm parity statement, tests/helpers.py (half_parity); MODE_FLOOR / MODE_CEIL: a layer's distance
# from the UNROUNDED oracle (tests/helpers.py, beside half_statement)


def _rel(a, b):
    return float((a.detach().double().cpu() - b.double()).abs().max() / b.double().abs().max())


def _set_precision(module, mode):
    for m in module.modules():
        if hasattr(m, "precision"):
            m.precision = mode


# classes of (y, gx, weight gradients): S single-product, T three-product.  999x24x40: a narrow forward (<= 32 inputs) beside the
# single-product Q2 = 2 input gradient and the RS = 2 weight gradient; 1500x64x64 G=8: 11 coefficients, the two-window kernels
# throughout; 800x64x256: the wide (128-output) forward block, an input gradient over two accumulating 128-output blocks, and the
# single-product weight gradient over four 64-output chunks
KANLINEAR_CASES = [(4096, 64, 64, 5, "SSS"), (5000, 128, 64, 5, "SSS"), (3001, 64, 40, 5, "SSS"), (1037, 33, 17, 4, "SSS"), (777, 320, 40, 5, "SSS"),
                   (2000, 64, 32, 3, "SSS"), (999, 24, 40, 5, "TSS"), (1500, 64, 64, 8, "TTT"), (800, 64, 256, 5, "TTS")]


# (the ids these cases had while a ``covered`` flag stood where the classes stand now: True = single-product throughout)
@pytest.mark.parametrize("n,fi,fo,G,code", KANLINEAR_CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-{c[4] == 'SSS'}" for c in KANLINEAR_CASES])
def test_half_mode_kanlinear_vs_rounding_oracle(n, fi, fo, G, code):
    """one KANLinear, forward and all gradients, every tensor at the statement of the class the table gives it (and the table is the
    routing the host code implements: helpers.half_routing)."""
    assert tuple(c == "S" for c in code) == half_routing(fi, fo, G, 3), (code, half_routing(fi, fo, G, 3))
    gen = torch.Generator().manual_seed(n + fi)
    p = orc.init_kan_linear(fi, fo, G, 3, gen)
    x = torch.randn(n, fi, generator=gen) * 0.8
    x[::7, 0] = 3.0                                        # outside the spline support
    gy = torch.randn(n, fo, generator=gen) * torch.logspace(-3, 2, n).unsqueeze(1)      # row scales over five decades
    got = kanlinear_fwd_bwd(p, x, gy, G, 3, ops.PREC_HALF)
    split = kanlinear_fwd_bwd(p, x, gy, G, 3, ops.PREC_SPLIT) if "T" in code else None
    plain, rounded = half_layer_oracles(x, gy, p, 3, code)
    # gx: the rows' scales span five decades and each row is rounded at its own scale -> compared row-normalised (half_statement)
    half_statement(got, plain, rounded, half_classes(code), f"half.kanlinear({n},{fi},{fo},G={G})", split)


def test_half_mode_is_a_switch_not_a_fallback():
    """the mode keeps every fused path of the split mode (same packs, same entry points), is selected per layer or by
    KAGNN_PRECISION=half, and HALF results differ from SPLIT results (the single-product kernels really ran)."""
    n, e, f = 20000, 160000, 64
    ei = orc.powerlaw_graph(n, e, seed=2).to(DEV)
    g = ops.GraphIndex(ei, n)
    x = (torch.randn(n, f, generator=torch.Generator().manual_seed(1)) * 0.3).to(DEV)
    gy = torch.randn(n, f, generator=torch.Generator().manual_seed(2)).to(DEV)
    torch.manual_seed(3)
    conv = kagnn_amd.GIKANLayer(f, f, grid_size=5, spline_order=3, hidden_dim=f, nb_layers=2).to(DEV)
    out = {}
    for mode in (ops.PREC_SPLIT, ops.PREC_HALF):
        _set_precision(conv, mode)
        conv.zero_grad()
        xr = x.clone().requires_grad_(True)
        timer = ops.EntryPointTimer()
        ops.set_timer(timer)
        try:
            y = conv(xr, g)
            y.backward(gy)
        finally:
            ops.set_timer(None)
        names = {r[0] for r in timer.records}
        assert "kagnn_gin_kan_layer_fwd" in names and ({"kagnn_gin_kan_layer_bwd", "kagnn_gin_kan_layer_bwd_add"} & names), names
        out[mode] = (y.detach().clone(), xr.grad.clone(), [p.grad.clone() for p in conv.parameters()])
    d = _rel(out[ops.PREC_HALF][0], out[ops.PREC_SPLIT][0].cpu())
    assert MODE_FLOOR <= d <= MODE_CEIL, d
    assert ops.default_precision() in (ops.PREC_SPLIT, ops.PREC_FP32, ops.PREC_HALF)
    os.environ["KAGNN_PRECISION"], keep = "half", os.environ.get("KAGNN_PRECISION")
    try:
        assert ops.default_precision() == ops.PREC_HALF
        _set_precision(conv, None)
        assert torch.equal(conv(x, g), out[ops.PREC_HALF][0])           # the environment switch selects the same kernels
    finally:
        if keep is None:
            del os.environ["KAGNN_PRECISION"]
        else:
            os.environ["KAGNN_PRECISION"] = keep


def test_half_mode_gin_layer_one_call_path_vs_rounding_oracle():
    """GIKANLayer(64 -> 64, two KANLinears) through kagnn_gin_kan_layer_fwd / _bwd with mode = KAGNN_PREC_HALF on a power-law graph
    with hubs: y, gx and every parameter gradient against the rounding oracle (the aggregation is exact fp32 in either)."""
    n, e, f = 30011, 300000, 64
    ei = orc.powerlaw_graph(n, e, seed=5)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(n, f, generator=gen) * 0.25
    gy = torch.randn(n, f, generator=gen)
    layers = [orc.init_kan_linear(f, f, 5, 3, gen) for _ in range(2)]
    conv = kagnn_amd.GIKANLayer(f, f, grid_size=5, spline_order=3, hidden_dim=f, nb_layers=2)
    for l, p in zip(conv.nn.layers, layers):
        l.load_state_dict(p)
    conv = conv.to(DEV)
    _set_precision(conv, ops.PREC_HALF)
    xr = x.to(DEV).requires_grad_(True)
    y = conv(xr, ei.to(DEV))
    y.backward(gy.to(DEV))
    y64, gx64, g64 = orc.kan_gin_layer_fwd_bwd(x.double(), ei, [{k: v.double() for k, v in p.items()} for p in layers], 3, gy.double())
    with half_mode_oracle():
        yr, gxr, gr = orc.kan_gin_layer_fwd_bwd(x.double(), ei, [{k: v.double() for k, v in p.items()} for p in layers], 3, gy.double())
    # two chained layers: a rounding flip in layer 0 (an fp32 basis value on the other side of an fp16 tie than its fp64 twin:
    # ~2e-4 of the values) moves one input of layer 1 by 2^-11 of a term -- 2e-4 instead of the single-layer 1e-4
    # (two chained layers: a flip in layer 0 moves an input of layer 1 -- twice the single-layer bounds)
    _parity(y, yr, y64, "half.gin_layer.y", 2 * L2_TOL, 2 * FLIP_TOL)
    _parity(xr.grad, gxr, gx64, "half.gin_layer.gx", 2 * L2_TOL, 2 * FLIP_TOL)
    for li, l in enumerate(conv.nn.layers):
        for k in ("base_weight", "spline_weight", "spline_scaler"):
            _parity(getattr(l, k).grad, gr[li][k], g64[li][k], f"half.gin_layer.L{li}.{k}", 2 * L2_TOL, 2 * FLIP_TOL)
    REPORT["half.gin_layer(30011,64)"] = {"y": _rel(y, y64), "gx": _rel(xr.grad, gx64),
                                          **{f"L{li}.{k}": _rel(getattr(l, k).grad, g64[li][k]) for li, l in enumerate(conv.nn.layers)
                                             for k in ("base_weight", "spline_weight", "spline_scaler")}}
    for k, v in REPORT["half.gin_layer(30011,64)"].items():
        check(v <= 2 * MODE_CEIL, f"half.gin_layer.{k}: distance from the unrounded oracle", v)


@pytest.mark.parametrize("act", ["fp32", "bf16"])
def test_half_mode_config2_model_vs_rounding_oracle(act, monkeypatch):
    """BASELINE config 2 as a mode: GKAN_Nodes('gin', 3, 128 -> 64, 40 classes) on a 30 000-node power-law graph with
    KAGNN_PRECISION=half (and, ``act == 'bf16'``, bf16 gather operands on top: the two build-defined modes together) -- logits,
    d/dx and every parameter gradient against the oracle that rounds where the mode(s) round; distances from the unrounded
    oracle reported.  Tolerances: three conv layers + BatchNorm amplify a layer-level flip (see the layer test) by the norm's
    1 / std and compound over depth; what is asserted is what the bf16 mode's rounding-oracle comparison is held to."""
    from helpers import bf16_gather_oracle
    from contextlib import ExitStack
    monkeypatch.setenv("KAGNN_ACT", act)
    n, e = 30_000, 210_000
    ei = orc.powerlaw_graph(n, e, seed=21)
    x = torch.randn(n, 128, generator=torch.Generator().manual_seed(22)) * 0.5
    gout = torch.randn(n, 40, generator=torch.Generator().manual_seed(23)) / n
    torch.manual_seed(1)
    model = kagnn_amd.GKAN_Nodes("gin", 3, 128, 64, 40, skip=True, grid_size=5, spline_order=3, hidden_layers=2)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    plain = oracle_node_model_fwd_bwd(x, ei, state, gout, "kan", "gin", 3, 3, 8192, torch.float64)
    with ExitStack() as st:
        st.enter_context(half_mode_oracle())
        if act == "bf16":
            st.enter_context(bf16_gather_oracle())
        rounded = oracle_node_model_fwd_bwd(x, ei, state, gout, "kan", "gin", 3, 3, 8192, torch.float64)
    _set_precision(model, ops.PREC_HALF)
    model = model.to(DEV).train()
    xd = x.to(DEV).requires_grad_(True)
    timer = ops.EntryPointTimer()
    ops.set_timer(timer)
    try:
        out = model(xd, ei.to(DEV))
        out.backward(gout.to(DEV))
    finally:
        ops.set_timer(None)
    names = [r[0] for r in timer.records]
    assert sum(1 for r in names if r in ("kagnn_gin_kan_layer_bwd_bn", "kagnn_gin_kan_layer_bwd_bn_sums")) == 3, names   # the default fused path
    tol = {"logits": 1e-3, "gx": 8e-3, "params": 8e-3}
    errs_r = {"logits": _rel(out, rounded[0]), "gx": _rel(xd.grad, rounded[1]), "params": 0.0}
    errs_p = {"logits": _rel(out, plain[0]), "gx": _rel(xd.grad, plain[1]), "params": 0.0, "per_param": {}}
    for name, p in model.named_parameters():
        if not p.requires_grad or prenorm_bias_noise(name, plain[2]) > 0.0:
            continue
        errs_r["params"] = max(errs_r["params"], _rel(p.grad, rounded[2][name]))
        errs_p["per_param"][name] = _rel(p.grad, plain[2][name])
        errs_p["params"] = max(errs_p["params"], errs_p["per_param"][name])
    REPORT[f"half.config2_model(act={act})"] = {"vs_rounding_oracle": errs_r, "vs_unrounded_oracle": errs_p, "tolerance_vs_rounding_oracle": tol}
    for k in tol:
        check(errs_r[k] <= tol[k], f"half config-2 model (act={act}) vs the rounding oracle: {k}", errs_r)
    check(errs_p["logits"] <= (1e-2 if act == "bf16" else 5e-3), f"half config-2 model (act={act}) vs the unrounded oracle: logits", errs_p)


def test_zz_half_mode_report():
    """(last in this file) the distances collected above -> gpurun_out/half_mode_errors.json; profiles/ holds the judged copy"""
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "half_mode_errors.json"), "w") as fh:
        json.dump(REPORT, fh, indent=1)
    assert REPORT
