"""Shared helpers of the parity tests: tolerances, state loading, oracle drivers.

Tolerances.  BASELINE.json's contract is "within 1e-4 fp32" (``CONTRACT``).  The tests pin an order of magnitude
tighter: ``TOL`` = 2e-5 relative to the tensor's OWN magnitude ``max|reference|`` for every element -- about 10x the
error both precision modes actually show on the layer-level cases (``profiles/r02_parity_errors.json``), so a regression
of the fp16 hi/lo split path (a dropped product, a wrong scale exponent: >= 2^-11) cannot hide behind the contract
figure.  Round 5: the scale used to be ``max(1, max|reference|)``, which made the bound ABSOLUTE for
small tensors -- with a mean-type loss gradient (``gout / n``) the arxiv-shaped model tests accepted all-zero input
gradients.  The scale is now the reference tensor's own maximum, floored only by an explicit ``noise`` estimate the
caller passes and justifies (the rounding noise of a cancelling fp32 sum: ``eps32 x sum|terms|``); an all-zero reference
without a noise estimate must be matched exactly.  ``tests/test_gpu_models.py`` holds the mutation guards (zeroed and
1e-3-perturbed gradients MUST fail).  On top of the max-norm bound every element at or above ``REL_FLOOR`` x scale must
agree to ``CONTRACT`` RELATIVE to its own magnitude.  Tests that need more room (errors compounded through BatchNorm /
several layers / Adam) pass an explicit ``tol`` and say why.

``KAGNN_TEST_SOFT=1`` (a survey aid, never the driver's mode): violations are recorded in ``SOFT_FAILURES`` and written to
``gpurun_out/parity_soft_failures.json`` instead of raised, so ONE run of the suite lists every check a rule change moves.
"""
import json
import os

import numpy as np
import torch

from oracle import kan_oracle as orc

CONTRACT = 1e-4   # BASELINE.json north_star: "within 1e-4 fp32"
TOL = 2e-5        # what the tests hold both precision modes to (max-norm, relative to max(1, max|reference|))
REL_FLOOR = 0.1   # elements >= REL_FLOOR * scale are also checked relative to their own magnitude (CONTRACT)
KAN_KEYS = ("base_weight", "spline_weight", "spline_scaler", "grid")
FK_KEYS = ("layernorm.weight", "layernorm.bias", "rbf.grid", "spline_linear.weight",
           "base_linear.weight", "base_linear.bias")

ERROR_LOG = []    # (what, observed error / scale, tolerance): dumped by conftest.py at session end


def T(a, device=None):
    t = torch.from_numpy(np.asarray(a))
    return t if device is None else t.to(device)


SOFT = os.environ.get("KAGNN_TEST_SOFT", "0") == "1"
SOFT_FAILURES = []


def _fail(what, msg, **info):
    if SOFT:
        SOFT_FAILURES.append(dict(what=what, msg=msg, **info))
        return
    raise AssertionError(msg)


def check(cond, what, info=None):
    """a plain assertion that KAGNN_TEST_SOFT=1 records instead of raising (for checks that do not go through assert_close)"""
    if not cond:
        _fail(what, f"{what}: {info}", info=repr(info))


def assert_close(got, want, tol=TOL, what="", elementwise=True, noise=0.0):
    """max-norm: ``max|got - want| <= tol * max|want| + noise``; element-wise: see the module docstring.  ``noise`` is an ABSOLUTE
    error the caller accepts on top because the reference itself carries it (state where it comes from at the call site: the
    rounding noise of a cancelling fp32 sum, ``eps32 x sum|terms|``); the default is none."""
    got = got.detach().double().cpu()
    want = T(want).double() if not torch.is_tensor(want) else want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.equal(torch.isnan(got), torch.isnan(want)), f"{what}: NaN pattern differs"
    if not want.numel():
        return 0.0
    g, w = torch.nan_to_num(got), torch.nan_to_num(want)
    own = float(w.abs().max())
    noise = float(noise)
    diff = (g - w).abs()
    err = float(diff.max())
    bound = tol * own + noise
    if bound == 0.0:                       # an identically zero reference and no noise estimate: exact match
        ERROR_LOG.append((what, 0.0 if err == 0.0 else float("inf"), tol))
        if err != 0.0:
            _fail(what, f"{what}: reference is identically zero, got max |value| {err:.3e}", err=err, scale=0.0, tol=tol)
        return 0.0
    ERROR_LOG.append((what, err / (bound / tol), tol))
    if err > bound:
        _fail(what, f"{what}: max abs err {err:.3e} > {tol:.0e} * {own:.3g} + {noise:.3g}", err=err, scale=own, noise=noise, tol=tol,
              old_rule_ok=bool(err <= tol * max(1.0, own)))
    big = w.abs() >= REL_FLOOR * own
    if elementwise and own > 0.0 and bool(big.any()):
        rel = float(((diff[big] - noise).clamp(min=0.0) / w.abs()[big]).max())
        if rel > max(CONTRACT, 5 * tol):
            _fail(what, f"{what}: element-wise relative error {rel:.3e} on a large element", rel=rel, scale=own, tol=tol)
    return err / (bound / tol)


def prenorm_bias_noise(name, wants):
    """Noise floor for the gradient of a bias that is added RIGHT IN FRONT of a training-mode BatchNorm1d: the GCN / GAT conv bias
    ``convs.i.bias`` and the base bias of the LAST FastKAN layer of a GIN conv (``convs.i.nn.layers.L.base_linear.bias``).  The batch
    mean is subtracted, so the gradient is identically zero in exact arithmetic; what fp32 holds (here AND in the reference-made
    fixtures) is the rounding noise of a cancelling sum over the nodes, sum_n g[n, c].  The terms are those of the sibling weight
    gradients sum_n g[n, c] * act[n, i] (|act| <= ~1), whose worst-case accumulation error is eps32 * sum|g| ~ eps32 * sqrt(n)
    relative to their own size: 1e-4 of the largest gradient of the same conv covers n up to ~1e6 rows.  ``wants``: {name: reference
    gradient} of the whole model.  0.0 for every other parameter (round 5: needed since assert_close no longer floors its scale at 1)."""
    parts = name.split(".")
    if len(parts) < 3 or parts[0] != "convs" or parts[-1] != "bias":
        return 0.0
    if len(parts) > 3:
        if not name.endswith(".base_linear.bias"):
            return 0.0
        layers = [int(k.split(".")[4]) for k in wants if k.startswith(f"convs.{parts[1]}.nn.layers.")]
        if not layers or int(parts[4]) != max(layers):
            return 0.0
    pre = f"convs.{parts[1]}."
    peak = max(float(np.abs(np.asarray(v.detach().cpu() if torch.is_tensor(v) else v)).max()) for k, v in wants.items() if k.startswith(pre))
    return 1e-4 * peak


def gat_att_noise(n, scale=1.0):
    """Noise floor for the gradients of the GAT attention vectors ``att_src`` / ``att_dst``: sums over all ``n`` nodes of
    (logit gradient) x (features).  Where a node has one incoming edge its softmax is the constant 1 and the exact term is 0
    (and with every logit of a row on one side of the leaky ReLU's kink its whole att_dst term is), so what fp32 adds up is
    rounding noise that grows like sqrt(n): 2e-5 x max(1, 0.05 sqrt(n)) at unit-scale operands (n = 20 000, e = 0: 5e-5).
    ``scale``: the operands' magnitude relative to that unit scale -- max|xh| x max(1, max|logit|), since the fp32 rounding of
    a logit perturbs every softmax weight of its row by eps32 x |logit|.  Only for att_src / att_dst."""
    return 2e-5 * max(1.0, 0.05 * float(n) ** 0.5) * max(1.0, float(scale))


def must_fail(got, want, tol=TOL, what="", **kw):
    """mutation guard: the SAME assertion the test just passed has to reject this ``got`` (with the old
    ``max(1, .)`` scale an all-zero input gradient passed the arxiv-shaped model tests)"""
    if SOFT:
        before = len(SOFT_FAILURES)
        assert_close(got, want, tol, what=what + " [mutant]", **kw)
        caught = len(SOFT_FAILURES) > before
        del SOFT_FAILURES[before:]
    else:
        try:
            assert_close(got, want, tol, what=what + " [mutant]", **kw)
            caught = False
        except AssertionError:
            caught = True
    while ERROR_LOG and ERROR_LOG[-1][0].endswith("[mutant]"):
        ERROR_LOG.pop()
    assert caught, f"{what}: the check accepted a mutated tensor -- it cannot fail"


def dump_soft_failures(path):
    if not SOFT:
        return
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(SOFT_FAILURES, f, indent=1)


def dump_error_log(path):
    if not ERROR_LOG:
        return
    worst = {}
    for what, err, tol in ERROR_LOG:
        key = what
        if key not in worst or err > worst[key][0]:
            worst[key] = (err, tol)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"n_checks": len(ERROR_LOG), "scale_rule": "max|reference| of the tensor itself, floored only by an explicit noise estimate",
                   "max_ratio_to_tol": max(e / t for _, e, t in ERROR_LOG if t > 0),
                   "worst_per_label": {k: {"err": v[0], "tol": v[1]} for k, v in sorted(worst.items(), key=lambda kv: -kv[1][0])[:200]}},
                  f, indent=1)


def load_kanlinear(layer, z, prefix, device):
    sd = {k: T(z[f"{prefix}{k}"]) for k in KAN_KEYS}
    layer.load_state_dict(sd)
    return layer.to(device)


def oracle_kan_linear_fwd_bwd(x, gy, p, k, dtype=torch.float64, chunk=None):
    """fp64 'truth' through the oracle (same algorithm as the reference, wider arithmetic).  ``chunk``: rows per pass (the rows of
    a KANLinear are independent and the parameter gradients add up over them in ``dtype``) -- for row counts whose dense basis
    tensors would not fit at once."""
    x = x.detach().cpu().to(dtype)
    gy = gy.detach().cpu().to(dtype)
    ps = {n: (v.detach().cpu().to(dtype).requires_grad_(True) if n != "grid" else v.detach().cpu().to(dtype))
          for n, v in p.items()}
    ys, gxs = [], []
    step = x.size(0) if not chunk else int(chunk)
    for lo in range(0, max(x.size(0), 1), max(step, 1)):
        xc = x[lo:lo + step].clone().requires_grad_(True)
        y = orc.kan_linear_forward(xc, ps["base_weight"], ps["spline_weight"], ps["spline_scaler"], ps["grid"], k)
        y.backward(gy[lo:lo + step])
        ys.append(y.detach())
        gxs.append(xc.grad)
    return torch.cat(ys), torch.cat(gxs), {n: ps[n].grad for n in ("base_weight", "spline_weight", "spline_scaler")}


def oracle_node_model_fwd_bwd(x, edge_index, state, gout, arch, conv_type, mp_layers, spline_order=3, chunk=None,
                              dtype=torch.float64):
    """logits, d/dx and every parameter gradient of a GKAN_Nodes / GFASTKAN_Nodes model through the oracle
    (``oracle.node_model_forward``) in ``dtype``; ``gout`` is the upstream gradient of the logits."""
    frozen = ("grid", "rbf.grid", "eps", "running_mean", "running_var", "num_batches_tracked")
    st, leaves = {}, {}
    for k, v in state.items():
        v = v.detach().cpu()
        if v.is_floating_point():
            v = v.to(dtype)
        if k.endswith(frozen):
            st[k] = v
        else:
            leaves[k] = v.clone().requires_grad_(True)
            st[k] = leaves[k]
    xr = x.detach().cpu().to(dtype).requires_grad_(True)
    ei = edge_index
    if isinstance(ei, torch.Tensor) and ei.is_sparse:
        ei = ei.cpu().to(dtype)
    out = orc.node_model_forward(xr, ei, st, arch, conv_type, mp_layers, spline_order, chunk=chunk)
    out.backward(gout.detach().cpu().to(dtype))
    return out.detach(), xr.grad, {k: v.grad for k, v in leaves.items()}


# ---------------------------------------------------------------------------------- the bf16 gather mode, restated
class _RoundRowsBf16(torch.autograd.Function):
    """what KAGNN_ACT=bf16 does to a matrix the aggregation gathers on the way FORWARD: one round-to-nearest-even to bf16
    (the gradient passes through unchanged: the HIP path hands the transposed aggregation's output straight to x.grad)"""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundGradBf16(torch.autograd.Function):
    """... and on the way BACK: d loss / d h0, the matrix the transposed aggregation gathers, is stored as bf16"""

    @staticmethod
    def forward(ctx, h):
        return h.view_as(h)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


class bf16_gather_oracle:
    """context manager: inside it ``oracle.gin_conv`` rounds the two gathered matrices of every KAN-GIN convolution to bf16
    exactly where the build-defined KAGNN_ACT=bf16 mode does -- everything else stays fp64.  The HIP
    path must agree with THIS oracle at (nearly) the fp32 tolerance: that is the parity statement for the mode; its distance
    from the unrounded oracle is a property of the mode, reported separately.  ``gathered_grad``: the backward's rounding on
    its own, for checkers that restate the transposed aggregation themselves (the forward's rounded rows are then the
    device's own aggregate)."""

    @staticmethod
    def gathered_grad(g):
        return g.to(torch.bfloat16).to(g.dtype)

    def __enter__(self):
        self._orig = orc.gin_conv

        def gin_conv(x, edge_index, nn_fn, eps=0.0):
            xr = _RoundRowsBf16.apply(x)
            return nn_fn(_RoundGradBf16.apply(orc.sum_aggregate(xr, edge_index) + (1.0 + eps) * xr))
        orc.gin_conv = gin_conv
        return self

    def __exit__(self, *exc):
        orc.gin_conv = self._orig
        return False


# ---------------------------------------------------------------------------------- KAGNN_PREC_HALF, restated (round 5)
def round11(t):
    """round to nearest even at 11 significant bits -- fp16's precision without its range.  The device rounds every operand of the
    mode after an exact power-of-two scaling into fp16's normal range (bases x 2^10, W x 2^-e, gy per row / per wave), and a
    floating-point rounding commutes with power-of-two scaling; operands that fall below fp16's normal range are < 2^-24 of their
    scale group's maximum (absolute error < 2^-35 of it)."""
    m, e = torch.frexp(t)
    return torch.ldexp(torch.round(m * 2048.0) / 2048.0, e)


def half_routing(fin, fout, G, k):
    """(round_fwd, round_dx, round_dw): which of a KANLinear's three GEMMs KAGNN_PREC_HALF runs as ONE fp16 product per fp32 product.
    Everything else runs the split mode's three-product kernel on the same pack (host.h: ModeScope rewrites the mode to SPLIT and
    raises a flag that only the launchers below look at).  Restated from the host code, once:
      forward            kan_sparse_fwd.hip: launch_sparse (``!SH && !NARROW && OT != 4``), launch_sparse_parts -- cubic, <= 8
                         coefficients (SH), more than 32 inputs (NARROW), and the 64-wide output block: sp_out_blk takes the
                         128-wide one (OT = 4) when ``out % 128 == 0`` (KAGNN_FWD_WIDE, on by default)
      input gradient     kan_split_bwd.hip: launch_dx_pp (``K == 3 && !GEN && Q2 <= 2``) -- cubic, <= 8 coefficients (GEN: more, or an
                         accumulating output block beyond the first 128) and <= 64 outputs (split_common.h: dx_q2)
      weight gradients   kan_split_bwd.hip: kan_split_dw_any (``half = g_half_products && K == 3 && !sh``) -- cubic, <= 8
                         coefficients, any width (9..16 coefficients leave earlier through kan_dw_w2_ok; the shared-expansion kernel
                         is switched off while the flag is up)
    More than 16 coefficients run as a sum of layers over coefficient groups of <= 16 (ops.kan_linear, ``coefficient_groups`` below)
    and every group is routed on its own: groups of 9..16 coefficients run three products, but 17 coefficients split 9 + 8 and the
    second group is a cubic 8-coefficient layer -- single-product.  This function is asked per group (``half_mode_oracle`` splits)."""
    lean = k == 3 and G + k <= 8
    return (lean and fin > 32 and fout % 128 != 0, lean and fout <= 64, lean)


def coefficient_groups(n_coef):
    """[(first coefficient, count)]: how ops.kan_linear cuts a layer of more than 16 coefficients into consecutive groups of <= 16 under
    the split-like modes (one group otherwise)"""
    groups = -(-n_coef // 16)
    size, extra = divmod(n_coef, groups)
    out, c0 = [], 0
    for g in range(groups):
        cg = size + (1 if g < extra else 0)
        out.append((c0, cg))
        c0 += cg
    return out


class _HalfKanLinear(torch.autograd.Function):
    """what KAGNN_PREC_HALF computes for one KANLinear, in fp64: every GEMM of the layer that ``flags`` = (forward, input gradient,
    weight gradient) marks as single-product, on operands that were evaluated exactly and rounded ONCE -- bases, SiLU, the scaled
    spline weight (formed in fp32 like the pack kernel forms it), the base weight, gy.  The basis DERIVATIVES and SiLU' of the input
    gradient, the chain rule through spline_scaler and all accumulation stay exact; a GEMM whose flag is down is the plain fp64
    one.  This is not the gradient of the rounded forward; it is the mode's definition."""

    @staticmethod
    def forward(ctx, x, base_weight, spline_weight, spline_scaler, knots, spline_order, flags=(True, True, True)):
        ctx.save_for_backward(x, base_weight, spline_weight, spline_scaler, knots)
        ctx.k, ctx.flags = spline_order, flags
        n, out = x.size(0), base_weight.size(0)
        if not flags[0]:
            return orc_kan_linear_forward(x, base_weight, spline_weight, spline_scaler, knots, spline_order)
        wcat = spline_weight if spline_scaler is None else (spline_weight.float() * spline_scaler.float().unsqueeze(-1)).to(x.dtype)
        br = round11(orc.bspline_bases(x, knots, spline_order))
        return (torch.nn.functional.linear(round11(torch.nn.functional.silu(x)), round11(base_weight))
                + torch.nn.functional.linear(br.view(n, -1), round11(wcat).view(out, -1)))

    @staticmethod
    def backward(ctx, gy):
        x, bw, sw, sc, knots = ctx.saved_tensors
        k = ctx.k
        _, rdx, rdw = ctx.flags
        n, out = x.size(0), bw.size(0)
        # input gradient: D[n, f, c] = sum_o gyr[n, o] Wr[o, f, c], contracted with the exact basis derivatives; base branch likewise
        if rdx:
            wcat = sw if sc is None else (sw.float() * sc.float().unsqueeze(-1)).to(x.dtype)
            ga, wa, ba = round11(gy), round11(wcat), round11(bw)
        else:
            ga, wa, ba = gy, (sw if sc is None else sw * sc.unsqueeze(-1)).detach(), bw.detach()   # (constants of the graphs built below)
        d = (ga @ wa.view(out, -1)).view(n, x.size(1), -1)
        with torch.enable_grad():
            xx = x.detach().requires_grad_(True)
            (orc.bspline_bases(xx, knots, k) * d).sum().backward()
            gx = xx.grad
            xs = x.detach().requires_grad_(True)
            (torch.nn.functional.silu(xs) * (ga @ ba)).sum().backward()
            gx = gx + xs.grad
        # weight gradient
        r = round11 if rdw else (lambda t: t)
        gb = r(gy)
        br = r(orc.bspline_bases(x, knots, k))
        gcat = (gb.t() @ br.view(n, -1)).view(out, x.size(1), -1)
        g_bw = gb.t() @ r(torch.nn.functional.silu(x))
        if sc is None:
            return gx, g_bw, gcat, None, None, None, None
        return gx, g_bw, gcat * sc.unsqueeze(-1), (gcat * sw).sum(-1), None, None, None


orc_kan_linear_forward = orc.kan_linear_forward      # the plain layer, whatever a context manager below has put in its place


class half_mode_oracle:
    """context manager: inside it ``oracle.kan_linear_forward`` is the restatement of KAGNN_PREC_HALF above (every KANLinear of every
    chain / conv / model the oracle evaluates).  ``route``: (in, out, G, k) -> which of the layer's three GEMMs are rounded; the
    default is the device's routing (``half_routing``), so the three-product GEMMs of a mixed layer stay plain fp64 and chains,
    convolutions and models get the right expectation per layer.  The HIP path must agree with THIS oracle at the fp32 contract
    (parity proper); its distance from the unrounded oracle is a property of the mode, reported separately (README: numerical
    contract)."""

    def __init__(self, route=half_routing):
        self.route = route

    def __enter__(self):
        self._orig = orc.kan_linear_forward
        route = self.route

        def kan_linear_forward(x, bw, sw, sc, knots, k):
            y = None
            for g, (c0, cg) in enumerate(coefficient_groups(sw.size(2))):
                flags = tuple(bool(f) for f in route(x.size(1), bw.size(0), cg - k, k))
                # a uniform B-spline basis function depends on its own k + 2 knots only: the group's layer on its slice of the knots; the
                # SiLU branch rides with the first group (a zero base weight elsewhere: it rounds to zero and its gradient is dropped)
                part = _HalfKanLinear.apply(x, bw if g == 0 else torch.zeros_like(bw).detach(), sw[:, :, c0:c0 + cg], sc,
                                            knots[:, c0:c0 + cg + k + 1], k, flags)
                y = part if y is None else y + part
            return y
        orc.kan_linear_forward = kan_linear_forward
        return self

    def __exit__(self, *exc):
        orc.kan_linear_forward = self._orig
        return False


# Parity of KAGNN_PREC_HALF (against the oracle fed the SAME once-rounded operands) is stated in two norms.  L2: the HIP path differs
# from that oracle only where the device's fp32 evaluation of an operand (bases by the closed cubic form, SiLU through v_exp / v_rcp:
# ~1e-7 from the oracle's fp64) lands on the other side of an fp16 rounding boundary -- ~2e-4 of the operands, each moving one term by
# 2^-11 of itself: SPARSE errors, <= HALF_L2_TOL of the tensor's norm, at least 5x below the mode's own (dense) distance from the
# unrounded oracle.  Max norm: one flipped term is up to ~1e-4 of max|y| at these widths (observed 0.5..1.0e-4), so the bound is
# HALF_FLIP_TOL = 3e-4 -- a dropped operand, a wrong scale exponent or a missing product is >= 2^-11 dense, i.e. fails the L2 bound.
HALF_L2_TOL, HALF_FLIP_TOL = 5e-5, 3e-4


def l2_rel(a, b):
    return float((a.detach().double().cpu() - b.double()).norm() / b.double().norm())


def half_parity(got, rounded, plain, what, l2_tol=HALF_L2_TOL, flip_tol=HALF_FLIP_TOL):
    """the two-norm parity statement of KAGNN_PREC_HALF above; returns (L2 vs rounding oracle, L2 vs unrounded oracle).
    ``plain=None``: no unrounded oracle at hand -- the 5x separation is not checked."""
    assert_close(got, rounded, flip_tol, what=what + " vs rounding oracle", elementwise=False)
    lr = l2_rel(got, rounded)
    check(lr <= l2_tol, what + ": L2 distance from the rounding oracle", lr)
    if plain is None:
        return lr, None
    lp = l2_rel(got, plain)
    check(5.0 * lr <= lp, what + ": the rounding oracle must explain the result at least 5x better than the unrounded one", (lr, lp))
    return lr, lp


# A layer's distance from the UNROUNDED oracle, relative to the tensor's maximum: above the three-product kernels' 1e-6 by construction
# (the floor proves that the single-product instantiation ran), below ~6 x 2^-11 (operand roundings add up over two operands and the
# two branches)
HALF_MODE_FLOOR, HALF_MODE_CEIL = 3e-5, 3e-3
SINGLE, THREE = "single-product", "three-product"
KAN_GRADS = ("base_weight", "spline_weight", "spline_scaler")
HALF_REPORT = {}     # case -> tensor -> class and distances; tests/test_gpu_half.py: test_zz_half_mode_report writes it out


def half_classes(code):
    """'STS' -> the class of y, gx and the three weight gradients of one KANLinear case (S: single-product, T: three-product), as the
    case tables of tests/test_gpu_half*.py write it down"""
    c = {"S": SINGLE, "T": THREE}
    return {"y": c[code[0]], "gx": c[code[1]], **{k: c[code[2]] for k in KAN_GRADS}}


def half_layer_oracles(x, gy, p, k, code, chunk=None):
    """(plain, rounded): y, gx and the weight gradients of one KANLinear from the unrounded fp64 oracle and from the rounding oracle
    that rounds exactly the GEMMs ``code`` marks single-product"""
    flags = tuple(ch == "S" for ch in code)
    y, gx, g = oracle_kan_linear_fwd_bwd(x, gy, p, k, chunk=chunk)
    with half_mode_oracle(lambda *a: flags):
        yr, gxr, gr = oracle_kan_linear_fwd_bwd(x, gy, p, k, chunk=chunk)
    return {"y": y, "gx": gx, **g}, {"y": yr, "gx": gxr, **gr}


def kanlinear_on_device(p, G, k, mode, device="cuda:0"):
    """a ``kagnn_amd.KANLinear`` with state ``p`` on the device, at precision ``mode``"""
    import kagnn_amd
    fo, fi = p["base_weight"].shape
    layer = kagnn_amd.KANLinear(fi, fo, grid_size=G, spline_order=k)
    layer.load_state_dict(p)
    layer = layer.to(device)
    layer.precision = mode
    return layer


def kanlinear_fwd_bwd(p, x, gy, G, k, mode, device="cuda:0"):
    """y, gx and the three weight gradients of that layer on the device under precision ``mode``"""
    layer = kanlinear_on_device(p, G, k, mode, device)
    xd = x.to(device).requires_grad_(True)
    y = layer(xd)
    y.backward(gy.to(device))
    return {"y": y.detach(), "gx": xd.grad, **{k_: getattr(layer, k_).grad for k_ in KAN_GRADS}}


def max_rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max())


def half_statement(got, plain, rounded, classes, tag, split=None, l2_tol=HALF_L2_TOL, flip_tol=HALF_FLIP_TOL, rows=("gx",), floor=True,
                   tol=TOL):
    """The statement of KAGNN_PREC_HALF per output tensor.  ``classes[name]`` says which it is:
    SINGLE -- ``half_parity`` against the rounding oracle (two norms and the 5x separation) and, with ``floor``, a max-norm distance
              from the unrounded oracle in [HALF_MODE_FLOOR, HALF_MODE_CEIL]: the single-product kernel ran, and nothing worse;
    THREE  -- the ordinary layer bound against the unrounded oracle and the very bits of ``split[name]``, the same operands under
              PREC_SPLIT: it is the same kernel reading the same pack.
    ``floor``: True / False, or the names of the tensors the floor is asked of.
    ``rows``: tensors compared row-normalised (each row by the rounding oracle's maximum of that row) -- gx wherever the rows of gy
    span decades, since every row is rounded at its own scale.  Distances go to HALF_REPORT[tag]."""
    rep = HALF_REPORT.setdefault(tag, {})
    for name, g in got.items():
        g, r, p = (t.detach().double().cpu() for t in (g, rounded[name], plain[name]))
        if name in rows:
            rs = r.abs().amax(1, keepdim=True).clamp(min=1e-300)
            g, r, p = g / rs, r / rs, p / rs
        what = f"{tag}.{name}" + (" (per row)" if name in rows else "")
        # the distance from the unrounded oracle is relative to the tensor's maximum, as HALF_MODE_FLOOR / _CEIL are defined (a row whose
        # own maximum is a cancelling sum is further away on its own scale: recorded for the row-normalised tensors, not bounded)
        rep[name] = {"class": classes[name], "max_norm_vs_unrounded": max_rel(got[name], plain[name]), "max_norm_vs_rounding_oracle": max_rel(g, r),
                     "l2_vs_rounding_oracle": l2_rel(g, r), "l2_vs_unrounded": l2_rel(g, p)}
        if name in rows:
            rep[name]["max_norm_vs_unrounded (per row)"] = max_rel(g, p)
        if classes[name] == SINGLE:
            half_parity(g, r, p, what, l2_tol, flip_tol)
            d = rep[name]["max_norm_vs_unrounded"]
            if floor is True or (floor and name in floor):
                check(HALF_MODE_FLOOR <= d <= HALF_MODE_CEIL, what + ": distance from the unrounded oracle", d)
        else:
            assert classes[name] == THREE, classes[name]
            assert_close(got[name], plain[name], tol, what=f"{tag}.{name} (three-product) vs the unrounded oracle")
            check(split is not None and torch.equal(got[name], split[name]), f"{tag}.{name}: the bits of PREC_SPLIT on the same operands",
                  None if split is None else float((got[name] - split[name]).abs().max()))
    return rep


# ---------------------------------------------------------------------------------- feature-sharded FastKAN layer, restated
# The local halves of the feature-sharded FastKAN layer (kagnn_amd.ops.fastkan_row_moments ... fastkan_shard_bwd_finish) with torch
# ops in fp64: the stand-ins the gloo tests inject as ``local_ops`` (tests/test_sharded_gloo.py: what is under test there is the
# exchange algebra around them) and the per-rank reference of tests/test_gpu_fastkan_shards.py.  Results come back in x's dtype.
def fk_row_moments(x):
    xd = x.double()
    mean = xd.mean(1)
    return torch.stack([mean, ((xd - mean[:, None]) ** 2).sum(1)], 1).to(x.dtype)


def fk_merge_moments(gathered, width, eps):
    g = gathered.double()
    mean, m2 = g[0, :, 0].clone(), g[0, :, 1].clone()
    for p in range(1, g.size(0)):                       # Chan's update, rank order
        na, nb = float(p * width), float(width)
        d = g[p, :, 0] - mean
        mean = mean + d * (nb / (na + nb))
        m2 = m2 + g[p, :, 1] + d * d * (na * nb / (na + nb))
    return torch.stack([mean, torch.rsqrt(m2 / (g.size(0) * width) + eps)], 1).to(gathered.dtype)


def fk_partial(z, x, sw, bw, bb, centers, den):
    phi = orc.rbf_bases(z, centers.double(), den)
    y = torch.nn.functional.linear(phi.view(z.size(0), -1), sw.double())
    if bw is not None:
        y = y + torch.nn.functional.linear(torch.nn.functional.silu(x), bw.double(), None if bb is None else bb.double())
    return y


def fk_shard_fwd(x, stats, ln_w, ln_b, sw, bw, bb, centers, den, mode=None):
    xd = x.double()
    with torch.no_grad():
        z = xd if ln_w is None else (xd - stats[:, :1].double()) * stats[:, 1:].double() * ln_w.double() + ln_b.double()
        return fk_partial(z, xd, sw, bw, bb, centers, den).to(x.dtype)


def fk_shard_bwd(x, gy, stats, ln_w, ln_b, sw, bw, centers, den, mode=None, want_bias=False):
    xd = x.detach().double()
    zhat = None if ln_w is None else (xd - stats[:, :1].double()) * stats[:, 1:].double()
    with torch.enable_grad():
        xb = xd.clone().requires_grad_(True)                     # the base branch's (and, without LayerNorm, the RBF's) input
        z = xb if ln_w is None else (zhat * ln_w.detach().double() + ln_b.detach().double()).requires_grad_(True)
        swd = sw.detach().double().requires_grad_(True)
        bwd = None if bw is None else bw.detach().double().requires_grad_(True)
        bbd = torch.zeros(sw.size(0), dtype=torch.float64, requires_grad=True) if (want_bias and bw is not None) else None
        y = fk_partial(z, xb, swd, bwd, bbd, centers, den)
        y.backward(gy.double())
    gxb = torch.zeros_like(xd) if xb.grad is None else xb.grad      # (LayerNorm without base branch: x enters through z alone)
    st = dict(gx=gxb, gz=None if ln_w is None else z.grad, zhat=zhat, rstd=None if ln_w is None else stats[:, 1:].double(),
              lw=ln_w, dtype=x.dtype)
    sums = None
    if ln_w is not None:
        h = z.grad * ln_w.detach().double()
        sums = torch.stack([h.sum(1), (h * zhat).sum(1)], 1).to(x.dtype)
    f = x.dtype
    return st, sums, swd.grad.to(f), None if bwd is None else bwd.grad.to(f), None if bbd is None else bbd.grad.to(f)


def fk_shard_bwd_finish(st, sums, width_total):
    f = st["dtype"]
    if st["lw"] is None:
        return st["gx"].to(f), None, None
    h = st["gz"] * st["lw"].detach().double()
    s = sums.double() / width_total
    gx = st["gx"] + st["rstd"] * (h - s[:, :1] - st["zhat"] * s[:, 1:])
    return gx.to(f), (st["gz"] * st["zhat"]).sum(0).to(f), st["gz"].sum(0).to(f)
