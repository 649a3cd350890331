"""KAGNN_PREC_HALF, kernel by kernel (tests/test_gpu_half.py holds the mode's statement and its layer / model cases).

The mode is a routing table, not one kernel (tests/helpers.py: half_routing).  Here: one case per single-product instantiation at
the smallest shape that selects it, each tensor at the statement of the class its case writes down (helpers.half_statement:
single-product -> the rounding oracle in two norms, 5x closer than the unrounded one, and a floor that proves the kernel ran;
three-product -> the ordinary fp64 bound and the bits of PREC_SPLIT); the moments epilogue, the column-block read-out and the
folded-norm (affine) variants; edge inputs -- the exact-fp32 SiLU fallback inside a single-product kernel, rows of gy forty decades
apart, non-finite rows, 1 / 31 / 257 rows, the persistent grids' second pass, strided column views; what the switch must leave
alone; and the graph-level one-call paths.  Every distance goes to the mode's report file with its case's class
(tests/test_gpu_half.py: test_zz_half_mode_report, which the last test here runs again)."""
import pytest
import torch

import kagnn_amd
from kagnn_amd import graph_ops, ops
from kagnn_amd.norm import BatchNorm1d
from oracle import kan_oracle as orc
from helpers import (HALF_FLIP_TOL as FLIP_TOL, HALF_L2_TOL as L2_TOL, HALF_MODE_CEIL as MODE_CEIL, HALF_MODE_FLOOR as MODE_FLOOR,
                     HALF_REPORT as REPORT, KAN_GRADS, SINGLE, THREE, T, assert_close, bf16_gather_oracle, check, half_classes,
                     half_layer_oracles, half_mode_oracle, half_parity, half_routing, half_statement, l2_rel, max_rel,
                     kanlinear_fwd_bwd, kanlinear_on_device, oracle_kan_linear_fwd_bwd)
from test_gpu_epilogue import _check_moments      # the bounds of test_forward_moments_equal_the_statistics_of_the_output

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G, K = 5, 3                 # every case here unless it says otherwise: 8 coefficients, cubic
CHUNK = 8200                # rows per pass of the fp64 oracles at N = 32 800 / 65 537


def _inputs(n, fi, fo, grid=G, k=K, dense_gy=False, seed=None):
    """the operands of test_half_mode_kanlinear_vs_rounding_oracle: x = 0.8 * randn with a column outside the support, gy with row
    scales over five decades (``dense_gy``: unit rows)"""
    gen = torch.Generator().manual_seed(n + fi if seed is None else seed)
    p = orc.init_kan_linear(fi, fo, grid, k, gen)
    x = torch.randn(n, fi, generator=gen) * 0.8
    x[::7, 0] = 3.0
    gy = torch.randn(n, fo, generator=gen)
    if not dense_gy:
        gy = gy * torch.logspace(-3, 2, n).unsqueeze(1)
    return p, x, gy


_CASES = {}


def _case(n, fi, fo, code, dense_gy=False):
    """operands and both fp64 oracles of one KANLinear case, computed once per (shape, classes) and shared by the tests that use them
    (the 32 800-row oracles take seconds); nobody writes to what this returns"""
    key = (n, fi, fo, code, dense_gy)
    if key not in _CASES:
        p, x, gy = _inputs(n, fi, fo, dense_gy=dense_gy)
        plain, rounded = half_layer_oracles(x, gy, p, K, code, chunk=CHUNK if n > 20000 else None)
        _CASES[key] = (p, x, gy, plain, rounded)
    return _CASES[key]


def _dev_layer(p, grid=G, k=K, mode=ops.PREC_HALF):
    return kanlinear_on_device(p, grid, k, mode, DEV)


def _weights(layer):
    return layer.base_weight.detach().contiguous(), layer.spline_weight.detach().contiguous(), layer.spline_scaler.detach().contiguous()


def _packs(layer, mode):
    """(forward pack, input-gradient pack) of the layer's current weights: kagnn_kan_pack, as ops._kan_fwd_raw calls it"""
    bw, sw, sc = _weights(layer)
    fo, fi = bw.shape
    fb, db = ops._sizes("kagnn_kan_pack_bytes", fi, fo, layer.grid_size, layer.spline_order, mode, outputs=2)
    pf, pd = ops._ws(fb, bw.device), ops._ws(db, bw.device)
    ops._call("kagnn_kan_pack", ops._ptr(bw), ops._ptr(sw), ops._ptr(sc), fi, fo, layer.grid_size, layer.spline_order, mode,
              ops._ptr(pf), ops._ptr(pd), ops._stream())
    return pf, pd


# ====================================================================== 2. one case per single-product instantiation
# (n, in, out, classes of y / gx / weight gradients, the instantiations the case selects).  Read from kan_sparse_fwd.hip
# (kan_sparse_fwd, launch_sparse, sp_split_plan), kan_split_bwd.hip (launch_dx_pp, split_dw_plan, kan_split_dw_any):
LAYER_CASES = [
    # ---- forward: kan_sparse_fwd_kernel<OT, false, false, false, -1, false, true>
    (257, 33, 17, "SSS", "fwd a: OT = 1 (17 outputs), one chunk; dx Q2 = 1; dW RS = 1, NTO = 2"),
    (257, 64, 33, "SSS", "fwd b: OT = 2 (33 outputs), one chunk; dW NTO = 3"),
    (300, 65, 100, "STS", "fwd c: second chunk one feature wide, output blocks 64 + 36, the launch split over the two chunks + "
                          "sparse_sum_splits_kernel; gx at 100 outputs is Q2 = 4: three-product; dW over two output chunks"),
    (32800, 80, 64, "SSS", "fwd d / dx d: cdiv(N, 256) = 129 >= 128 -> one split: two chunks streamed through the LDS double buffer "
                           "in one launch; dx: five feature tiles x 36 KB exceed the 160 KB budget with one split -> weights not resident"),
    (300, 64, 128, "TTS", "fwd e: the wide 128-output block (OT = 4) has no single-product form, nor has dx at Q2 = 4; dW over two chunks"),
    # ---- input gradient: kan_split_dx_kernel<3, Q2, false, 1, false, false, false, false, true>
    (257, 24, 17, "TSS", "dx a: Q2 = 1 on a narrow input (two feature tiles, the second one half empty); narrow forward: three-product"),
    (257, 64, 64, "SSS", "dx b: Q2 = 2, resident weights"),
    (300, 320, 40, "SSS", "dx c: 20 feature tiles split over blockIdx.y (2 row blocks -> 20 splits); fwd: five chunks split over the launch"),
    (300, 64, 100, "STS", "dx e: 100 outputs -> Q2 = 4: three-product"),
    # ---- weight gradients: kan_split_dw_kernel<3, false, RS, NTO, false, true>
    (4097, 8, 64, "TSS", "dW a: RS = 4 (<= 16 inputs); 4097 rows: dW f, a last row block of one row for four sub-ranges"),
    (95, 16, 40, "TSS", "dW a / f: RS = 4, 95 rows do not fill the sub-ranges' 32-row chunks"),
    (1000, 24, 40, "TSS", "dW b: RS = 2 (17..32 inputs)"),
    (33, 32, 17, "TSS", "dW b / f: RS = 2, 33 rows: the second sub-range holds one row"),
    (20001, 16, 40, "TSS", "dW f: RS = 4, 96 rows per workgroup -> sub-ranges of 32 / 32 / 32 / 0 rows; the last workgroup holds 33 rows: 32 + 1"),
    (20001, 24, 40, "TSS", "dW f: RS = 2, the same rows -> sub-ranges of 64 / 32 rows; the last workgroup: 33 + 0"),
    (300, 64, 16, "SSS", "dW c: NTO = 1; fwd OT = 1; dx Q2 = 1"),
    (300, 64, 32, "SSS", "dW c: NTO = 2"),
    (300, 64, 48, "SSS", "dW c: NTO = 3"),
    (300, 64, 64, "SSS", "dW c: NTO = 4, one output chunk"),
    (800, 64, 256, "TTS", "dW d: four 64-output chunks, one workgroup per chunk in ONE launch (grid.y = FG * OC) in place of the shared-expansion kernel"),
    (777, 72, 192, "STS", "dW d: three output chunks x two feature groups; fwd: 192 outputs are three 64-wide blocks: single-product"),
]


@pytest.mark.parametrize("n,fi,fo,code,what", LAYER_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}-{c[3]}" for c in LAYER_CASES])
def test_half_single_product_instantiations_vs_rounding_oracle(n, fi, fo, code, what):
    assert tuple(c == "S" for c in code) == half_routing(fi, fo, G, K), (code, half_routing(fi, fo, G, K))
    p, x, gy, plain, rounded = _case(n, fi, fo, code)
    got = kanlinear_fwd_bwd(p, x, gy, G, K, ops.PREC_HALF)
    split = kanlinear_fwd_bwd(p, x, gy, G, K, ops.PREC_SPLIT) if "T" in code else None
    rep = half_statement(got, plain, rounded, half_classes(code), f"half.instantiation({n},{fi},{fo})", split)
    rep["selects"] = what


@pytest.mark.parametrize("n,fi,fo", [(3001, 64, 40), (300, 33, 17)])
def test_half_forward_moments_epilogue(n, fi, fo):
    """kan_sparse_fwd_kernel<OT, false, true, false, -1, false, true> (MOM): the same y to the bit as the plain single-product forward,
    column moments that are the statistics of that y, and that y at the rounding oracle"""
    p, x, gy, plain, rounded = _case(n, fi, fo, "SSS")
    layer = _dev_layer(p)
    xd = x.to(DEV)
    assert ops._sizes("kagnn_kan_fwd_workspace_bytes", n, fi, fo, G, K, ops.PREC_HALF) == 0      # one chunk: the epilogue form, not the stand-alone pass
    y, _, mom = ops._kan_fwd_raw(xd, *_weights(layer), layer._knots(), G, K, ops.PREC_HALF, moments=True)
    with torch.no_grad():
        assert torch.equal(y, layer(xd)), "the moments variant must write the same y"
    _check_moments(y, mom, f"half moments ({n},{fi},{fo})")
    half_statement({"y": y}, plain, rounded, {"y": SINGLE}, f"half.moments({n},{fi},{fo})")


@pytest.mark.parametrize("widths,fo,n", [([64, 64], 40, 777), ([128, 64], 17, 777)])
def test_half_parts_read_out(widths, fo, n):
    """kan_sparse_fwd_kernel<OT, false, false, false, -1, true, true> (launch_sparse_parts<OT, true>: OT = 2 at 40 outputs, 1 at 17), plain and
    with per-block affines: the bits of the single-product forward of the concatenation (the affine blocks: of the rows written
    out with the kernel's own fused multiply-add.  Split mode's test_read_out_over_folded_norm_blocks_equals_the_materialised_blocks
    claims 4e-6 against rows written out by torch.addcmul; under half a last-bit difference of a row can cross an fp16 rounding
    tie -- 4.2e-5 measured -- so the rows are formed the kernel's way and the claim is the bits), and both forwards at the rounding oracle"""
    fi = sum(widths)
    p, x, gy, plain, rounded = _case(n, fi, fo, "SSS")
    layer = _dev_layer(p)
    xd = x.to(DEV)
    parts, f0 = [], 0
    for w in widths:
        parts.append(xd[:, f0:f0 + w].contiguous())
        f0 += w
    assert ops._parts_one_launch(parts, fo, G, K, ops.PREC_HALF)
    timer = ops.EntryPointTimer()
    ops.set_timer(timer)
    try:
        with torch.no_grad():
            y = layer.forward_parts(parts)
            whole = layer(xd)
            # the same rows as folded norms: block i is (raw_i, affine_i) with raw_i * scale_i + shift_i = parts[i] up to fp32 rounding
            gen = torch.Generator().manual_seed(fi)
            affs = [torch.stack([torch.rand(w, generator=gen) * 0.5 + 0.5, torch.randn(w, generator=gen) * 0.3]).to(DEV) for w in widths]
            raws = [(t - a[1]) / a[0] for t, a in zip(parts, affs)]
            # the rows written out as the kernel forms them, fmaf(x, scale, shift) (kan_sparse_fwd.hip: load8) -- in fp64 the product is
            # exact and the sum is rounded once more to fp32: the fused multiply-add's bits, but for a double rounding (the fp64 sum
            # exactly half way between two fp32 values: ~2^-29 per element).  The bit-equality below therefore holds for THESE seeded
            # operands -- none of their 150 000 elements meets that double rounding and then an fp16 tie; other operands might
            rows = [(r.double() * a[0].double() + a[1].double()).float() for r, a in zip(raws, affs)]
            ya = layer.forward_parts([ops.AffineRows(r, a) for r, a in zip(raws, affs)])
            ym = layer(torch.cat(rows, dim=1))
    finally:
        ops.set_timer(None)
    names = [r[0] for r in timer.records]
    assert names.count("kagnn_kan_linear_fwd_parts_affine") == 2, names
    assert torch.equal(y, whole), "parts forward under half: not the bits of the forward of the concatenation"
    assert torch.equal(ya, ym), ("parts-affine forward under half: not the bits of the forward of the rows written out", float((ya - ym).abs().max()))
    tag = f"half.parts({widths}->{fo})"
    half_statement({"y": whole}, plain, rounded, {"y": SINGLE}, tag)
    # the affine form against the rounding oracle of ITS rows (exact affine in fp64, then the layer)
    h64 = torch.cat(rows, dim=1).double().cpu()
    pl, ro = half_layer_oracles(h64, gy, p, K, "SSS")
    half_statement({"y": ya}, pl, ro, {"y": SINGLE}, tag + ".affine")


# ---------------------------------------------------------------------------------------------------------- input gradient f / g
def _affine_case(n, fi, fo, seed):
    """a layer whose input exists as (raw rows, per-column scale and shift): operands, the affine, and both oracles of the layer on
    h = scale * raw + shift in fp64 (the gradient is with respect to h: ops.AffineRows' convention)"""
    p, raw, gy = _inputs(n, fi, fo, seed=seed)
    gen = torch.Generator().manual_seed(seed + 1)
    raw = raw * 2.0 + 1.0
    aff = torch.stack([torch.rand(fi, generator=gen) * 0.3 + 0.35, torch.randn(fi, generator=gen) * 0.2 - 0.5])
    h64 = raw.double() * aff[0].double() + aff[1].double()
    plain, rounded = half_layer_oracles(h64, gy, p, K, "SSS", chunk=CHUNK if n > 20000 else None)
    return p, raw, gy, aff, plain, rounded


@pytest.mark.parametrize("n,fi,fo", [(777, 64, 40), (300, 64, 64), (300, 64, 17)])
def test_half_input_and_weight_gradients_of_a_folded_norm(n, fi, fo):
    """dx f: kan_split_dx_kernel<3, Q2, false, 1, false, false, true (XAFF), false, true> through kagnn_kan_linear_bwd_input_affine (Q2 = 2 at 40
    and 64 outputs, 1 at 17); dW e: kan_split_dw_kernel<3, false, 1, NTO, true (XAFF), true> through kagnn_kan_linear_bwd_weight_affine (NTO = 3 at
    40 outputs, 4 at 64, 2 at 17)
    -- against the rounding oracle on the affine rows formed exactly"""
    p, raw, gy, aff, plain, rounded = _affine_case(n, fi, fo, seed=n + fo)
    layer = _dev_layer(p)
    bw, sw, sc = _weights(layer)
    _, pd = _packs(layer, ops.PREC_HALF)
    rd, gd, ad = raw.to(DEV), gy.to(DEV), aff.to(DEV).contiguous()
    gx = ops._kan_bwd_input_raw(rd, gd, layer._knots(), pd, fi, fo, G, K, ops.PREC_HALF, x_affine=ad)
    gbw, gsw, gsc = ops._kan_bwd_weight_raw(rd, gd, layer._knots(), sw, sc, fi, fo, G, K, ops.PREC_HALF, True, x_affine=ad)
    got = {"gx": gx, "base_weight": gbw, "spline_weight": gsw, "spline_scaler": gsc}
    cls = half_classes("SSS")
    half_statement(got, plain, rounded, {k: cls[k] for k in got}, f"half.affine({n},{fi},{fo})")


def test_half_input_gradient_with_column_sums():
    """dx g: kan_split_dx_kernel<3, 2, false, 1, false, false, true, true (XST), true> through kagnn_kan_linear_bwd_input_affine_sums at
    (32 800, 64, 40) -- the sums need >= 128 row blocks and <= 64 inputs: gx at the rounding oracle, and the two column sums (sum gx,
    sum gx * xhat) at the sums of that oracle's gx (dominated by the rows at the top of gy's five decades)"""
    n, fi, fo = 32800, 64, 40
    p, raw, gy, aff, plain, rounded = _affine_case(n, fi, fo, seed=5)
    layer = _dev_layer(p)
    _, pd = _packs(layer, ops.PREC_HALF)
    gen = torch.Generator().manual_seed(6)
    ns = ops.NormSums()
    mean, rstd = torch.randn(fi, generator=gen) * 0.2 + 1.0, torch.rand(fi, generator=gen) + 0.5
    ns.mean, ns.rstd = mean.to(DEV), rstd.to(DEV)
    assert ops._lib.load().kagnn_kan_bwd_input_sums_ok(n, fi, fo, G, K, ops.PREC_HALF) == 1
    gx, sums = ops._kan_bwd_input_sums_raw(raw.to(DEV), gy.to(DEV), layer._knots(), pd, fi, fo, G, K, ops.PREC_HALF, aff.to(DEV).contiguous(), ns)
    xhat = (raw.double() - mean.double()) * rstd.double()
    want = {"gx": (plain["gx"], rounded["gx"])}
    want["sums"] = tuple(torch.stack([g.sum(0), (g * xhat).sum(0)]) for g in want["gx"])
    half_statement({"gx": gx, "sums": sums}, {k: v[0] for k, v in want.items()}, {k: v[1] for k, v in want.items()},
                   {"gx": SINGLE, "sums": SINGLE}, f"half.affine_sums({n},{fi},{fo})", floor=("gx",))
    # the same kernel without the sums writes the same gradient rows
    gx2 = ops._kan_bwd_input_raw(raw.to(DEV), gy.to(DEV), layer._knots(), pd, fi, fo, G, K, ops.PREC_HALF, x_affine=aff.to(DEV).contiguous())
    assert torch.equal(gx, gx2)


# ---------------------------------------------------------------------------------------------------------- input gradient h / i
_BN_GRAPH = {}


def _bn_layer_oracles(x, ei, layers, bn_w, bn_b, gz):
    """bn(GIKANLayer(x)) with training statistics (biased variance, eps 1e-5), forward and backward in fp64 through
    ``orc.gin_conv`` / ``orc.kan_forward``, so the context managers of helpers.py round where the modes round; the norm and its
    backward are exact"""
    xr = x.double().requires_grad_(True)
    ps = [{k: (v.double().requires_grad_(True) if k != "grid" else v.double()) for k, v in p.items()} for p in layers]
    w, b = bn_w.double().requires_grad_(True), bn_b.double().requires_grad_(True)
    h = orc.gin_conv(xr, ei, lambda t: orc.kan_forward(t, ps, K))
    mean, var = h.mean(0), h.var(0, unbiased=False)
    z = (h - mean) / torch.sqrt(var + 1e-5) * w + b
    z.backward(gz.double())
    out = {"z": z.detach(), "gx": xr.grad, "bn.weight": w.grad, "bn.bias": b.grad}
    for li, q in enumerate(ps):
        for k in KAN_GRADS:
            out[f"L{li}.{k}"] = q[k].grad
    return out


# gx under KAGNN_ACT=bf16 (case i).  Before the bf16 store the first layer's gradient rows agree with the rounding oracle's as every
# two-layer chain does: 2 * L2_TOL in L2.  An element at relative distance d from the oracle's value lands on the other side of a
# bf16 rounding boundary with probability d / s, s = 2^-8 the (largest) relative spacing of bf16, and then differs by one spacing:
# expected squared error d * s per element, so  L2 <= sqrt(2 * L2_TOL * 2^-8) + 2 * L2_TOL = 7.3e-4  (the transposed aggregation adds
# rows with independent errors: relative L2 unchanged).  Max norm: isolated flips of one bf16 spacing of one gathered element; the
# worst element observed against the rounding oracle is 8.9e-4 of max|gx| (one flipped element of a hub row), x 1.5 for the
# box-to-box spread of the v_exp / v_rcp ties that decide which elements flip.
GX16_L2_TOL = (2 * L2_TOL * 2.0 ** -8) ** 0.5 + 2 * L2_TOL
GX16_FLIP_TOL = 1.5 * 8.9e-4


@pytest.mark.parametrize("act,fo", [("fp32", 64), ("bf16", 64), ("fp32", 32)])       # (GX16 is the FIRST layer's kernel, 64 -> 64 in every case: one bf16 case selects it)
def test_half_fused_norm_layer_on_a_powerlaw_graph(act, fo, monkeypatch):
    """dx h: kan_split_dx_kernel<3, Q2, false, 0, false, true (BNB), false, false, true> (Q2 = 2 at 64 outputs, 1 at 32: kan_split_dx_bn) --
    GIKANLayer(64 -> 64 -> ``fo``, two KANLinears) + BatchNorm1d as the fused node (kagnn_gin_kan_layer_bwd_bn): the norm's backward is
    applied to the rows the last layer's input-gradient kernel loads, then they are rounded once.  dx i (``act == 'bf16'``): the
    first layer's gradient rows leave as bf16 (GX16, kan_split_dx_kernel<3, 2, false, 1, true, false, false, false, true>) for the transposed
    aggregation, bf16_gather_oracle stacked on the half oracle.
    Statement: two chained layers, so the doubled bounds of test_half_mode_gin_layer_one_call_path_vs_rounding_oracle for every
    tensor, bf16 or not -- except gx under bf16 (GX16_L2_TOL / GX16_FLIP_TOL above).  The "unrounded" oracle of the 5x separation and
    of the floor / ceiling is the one WITHOUT the half mode's roundings: under bf16 it keeps the bf16 roundings, so the separation
    shows the single-product kernels and not the bf16 store.  And, as split mode's test_conv_and_norm_as_one_tape_node_give_the_two_
    nodes_bits states it: the fused node gives the bits of the convolution node followed by the norm node, under PREC_HALF too."""
    import copy
    from kagnn_amd import models as M
    monkeypatch.setenv("KAGNN_ACT", act)
    n, e, f = 5000, 60000, 64
    ei = orc.powerlaw_graph(n, e, seed=9)
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(n, f, generator=gen) * 0.25
    gz = torch.randn(n, fo, generator=gen)
    layers = [orc.init_kan_linear(f, f, G, K, gen), orc.init_kan_linear(f, fo, G, K, gen)]
    bn_w, bn_b = torch.rand(fo, generator=gen) + 0.5, torch.randn(fo, generator=gen) * 0.2
    if act == "bf16":
        with bf16_gather_oracle():
            plain = _bn_layer_oracles(x, ei, layers, bn_w, bn_b, gz)
        with half_mode_oracle(), bf16_gather_oracle():
            rounded = _bn_layer_oracles(x, ei, layers, bn_w, bn_b, gz)
    else:
        plain = _bn_layer_oracles(x, ei, layers, bn_w, bn_b, gz)
        with half_mode_oracle():
            rounded = _bn_layer_oracles(x, ei, layers, bn_w, bn_b, gz)
    conv0 = kagnn_amd.GIKANLayer(f, fo, grid_size=G, spline_order=K, hidden_dim=f, nb_layers=2)
    for l, p in zip(conv0.nn.layers, layers):
        l.load_state_dict(p)
        l.precision = ops.PREC_HALF
    bn0 = BatchNorm1d(fo)
    with torch.no_grad():
        bn0.weight.copy_(bn_w)
        bn0.bias.copy_(bn_b)
    conv0, bn0 = conv0.to(DEV).train(), bn0.to(DEV).train()
    g = ops.GraphIndex(ei.to(DEV), n)
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(M, "_FUSED_NORM_BACKWARD", fused)
        conv, bn = copy.deepcopy(conv0), copy.deepcopy(bn0)
        xd = x.to(DEV).requires_grad_(True)
        timer = ops.EntryPointTimer()
        ops.set_timer(timer)
        try:
            z = M.conv_bn_dropout(conv, bn, torch.nn.Dropout(0.0), xd, g)
            assert type(z.grad_fn).__name__ == ("_GinKanBnLayerFnBackward" if fused else "_BatchNormFnBackward")
            z.backward(gz.to(DEV))
        finally:
            ops.set_timer(None)
        names = [r[0] for r in timer.records]
        assert ("kagnn_gin_kan_layer_bwd_bn" in names) == fused, names
        out = {"z": z.detach(), "gx": xd.grad.float(), "bn.weight": bn.weight.grad, "bn.bias": bn.bias.grad,
               "running_mean": bn.running_mean.clone(), "running_var": bn.running_var.clone()}
        for li, l in enumerate(conv.nn.layers):
            for k in KAN_GRADS:
                out[f"L{li}.{k}"] = getattr(l, k).grad
        res[fused] = out
    got = {k: v for k, v in res[True].items() if not k.startswith("running")}
    tag = f"half.fused_norm_layer(act={act},64->64->{fo})"
    rep = REPORT.setdefault(tag, {})
    for k, t in got.items():
        rep[k] = {"class": "no KAN operand (either oracle)" if k == "bn.bias" else SINGLE,
                  "max_norm_vs_unrounded": max_rel(t, plain[k]), "max_norm_vs_rounding_oracle": max_rel(t, rounded[k]),
                  "l2_vs_rounding_oracle": l2_rel(t, rounded[k]), "l2_vs_unrounded": l2_rel(t, plain[k])}
    print(tag, {k: {q: float("%.3g" % w) for q, w in v.items() if q != "class"} for k, v in rep.items()})
    for k, t in got.items():
        if k == "bn.bias":              # the column sums of gz: no KAN operand in it, the same number from either oracle
            assert_close(t, plain[k], what=f"{tag}.{k}")
            continue
        if act == "bf16" and k == "gx":
            half_parity(t, rounded[k], plain[k], f"{tag}.{k}", GX16_L2_TOL, GX16_FLIP_TOL)
        else:
            half_parity(t, rounded[k], plain[k], f"{tag}.{k}", 2 * L2_TOL, 2 * FLIP_TOL)
        d = rep[k]["max_norm_vs_unrounded"]
        check(MODE_FLOOR <= d <= 2 * MODE_CEIL, f"{tag}.{k}: distance from the oracle without the half mode's roundings", rep[k])
    for k in res[True]:
        a_, b_ = res[True][k], res[False][k]
        assert torch.equal(a_, b_), f"{tag}.{k}: fused node vs convolution node + norm node: max |diff| {float((a_ - b_).abs().max()):.3e}"


# ====================================================================== 3. edge inputs
def test_half_extreme_ranges():
    """the shape of test_kanlinear_extreme_ranges_vs_oracle under half: (4099, 64, 64), base weights x 37, spline weights x 1e-3.
    The huge activations (1e4 x a row, 3e5, -2e4, and one value either side of the forward's fallback threshold: |silu| * 16 against
    60 000, kan_sparse_fwd.hip: silu_prep) sit in rows 1024..1055 -- ONE wave group of the forward (row0 = tile * 256 + wave * 32,
    kan_sparse_fwd_kernel) and of the input gradient (gy_ro = (wave * 32 + li) rows, kan_split_dx_kernel), and ONE chunk of the weight
    gradient (split_dw_plan: 4099 rows over 256 workgroups -> 32 rows each, rbeg = blockIdx.x * 32, kan_split_dw_kernel).  The fallback
    is wave-uniform and exact fp32, so those 32 rows lie between the two oracles; every other row is rounded once."""
    n, fi, fo = 4099, 64, 64
    gen = torch.Generator().manual_seed(77)
    p = orc.init_kan_linear(fi, fo, G, K, gen)
    p["base_weight"] = p["base_weight"] * 37.0
    p["spline_weight"] = p["spline_weight"] * 1e-3
    x = torch.randn(n, fi, generator=gen) * 0.7
    b0, b1 = 1024, 1056
    x[b0 + 1] *= 1e4; x[b0 + 5, :8] = 3e5; x[b0 + 9] = -2e4
    x[b0 + 13, 3] = 3751.0; x[b0 + 17, 5] = 3749.0          # silu(x) * 16 = 60 016 / 59 984: above / below the threshold
    gy = torch.randn(n, fo, generator=gen)
    scale = torch.ones(n, 1)
    scale[:500] = 1e-18; scale[500:900] = 1e-6; scale[2500:2600] = 1e9; scale[4090:] = 1e19
    gy = gy * scale
    plain, rounded = half_layer_oracles(x, gy, p, K, "SSS")
    got = kanlinear_fwd_bwd(p, x, gy, G, K, ops.PREC_HALF)
    keep = torch.ones(n, dtype=torch.bool)
    keep[b0:b1] = False
    assert int((~keep).sum()) <= 32
    tag = "half.extreme_ranges"
    sel = lambda d, rows: {k: d[k].detach().cpu()[rows] for k in ("y", "gx")}
    # rows outside the block: a rounding commutes with the per-row power of two, so rows at 1e-18 .. 1e19 stay on the rounding oracle
    half_statement(sel(got, keep), sel(plain, keep), sel(rounded, keep), {"y": SINGLE, "gx": SINGLE}, tag, floor=False)
    rep = REPORT[tag]
    for k in ("y", "gx"):
        g, w = got[k].detach().double().cpu()[b0:b1], plain[k][b0:b1]
        assert torch.equal(torch.isnan(g), torch.isnan(w)), k
        d = ((g - w).abs().amax(1) / w.abs().amax(1).clamp(min=1e-300))
        rep[k + " rows of the fallback block"] = {"class": "between the oracles", "max_norm_vs_unrounded (per row)": float(d.max())}
        check(float(d.max()) <= MODE_CEIL, f"{tag}.{k}: the fallback block's rows against the unrounded oracle", d.tolist())
    for k in KAN_GRADS:
        d = max_rel(got[k], plain[k])
        rep[k] = {"class": "between the oracles", "max_norm_vs_unrounded": d, "max_norm_vs_rounding_oracle": max_rel(got[k], rounded[k])}
        assert_close(got[k], plain[k], MODE_CEIL, what=f"{tag}.{k}", elementwise=False)


def test_half_non_finite_rows():
    """one NaN, one +Inf and one -Inf entry in three rows of a (1037, 64, 64) layer: the NaN masks of y, gx and the weight gradients
    are the fp64 oracle's; every finite entry of y and gx is at the single-product statement, the finite weight gradients within
    MODE_CEIL of the unrounded oracle (the chunk that holds the non-finite values takes the exact-fp32 path)"""
    n, fi, fo = 1037, 64, 64
    p, x, gy = _inputs(n, fi, fo, dense_gy=True, seed=31)
    # (rows 200..202: ONE 32-row wave group, 192..223 -- a non-finite SiLU value sends its whole group down the forward's exact-fp32
    # base branch, kan_sparse_fwd.hip: silu_prep, so the group's finite rows are rounded in fewer places than the oracle rounds)
    x[200, 0] = float("inf"); x[201, 1] = float("nan"); x[202, 2] = float("-inf")
    plain, rounded = half_layer_oracles(x, gy, p, K, "SSS")
    got = {k: v.detach().double().cpu() for k, v in kanlinear_fwd_bwd(p, x, gy, G, K, ops.PREC_HALF).items()}
    tag = "half.non_finite_rows"
    masks = {}
    for k in got:
        masks[k] = (int(torch.isnan(got[k]).sum()), int(torch.isnan(plain[k]).sum()), int(torch.isinf(got[k]).sum()), int(torch.isinf(plain[k]).sum()))
    print(tag, "NaN / Inf counts (device NaN, oracle NaN, device Inf, oracle Inf):", masks)
    REPORT.setdefault(tag, {})["nan_inf_counts"] = {k: list(v) for k, v in masks.items()}
    for k in got:
        assert torch.equal(torch.isnan(got[k]), torch.isnan(plain[k])), f"{tag}.{k}: NaN pattern differs {masks[k]}"
        assert torch.equal(torch.isnan(rounded[k]), torch.isnan(plain[k])), k
    fin = lambda d, keys: {k: torch.where(torch.isfinite(plain[k]), d[k], torch.zeros_like(d[k])) for k in keys}
    half_statement(fin(got, ("y", "gx")), fin(plain, ("y", "gx")), fin(rounded, ("y", "gx")), {"y": SINGLE, "gx": SINGLE}, tag, rows=())
    for k in KAN_GRADS:
        ok = torch.isfinite(plain[k])
        assert torch.equal(torch.isfinite(got[k]), ok), f"{tag}.{k}: Inf pattern differs {masks[k]}"
        assert_close(fin(got, (k,))[k], fin(plain, (k,))[k], MODE_CEIL, what=f"{tag}.{k}", elementwise=False)


@pytest.mark.parametrize("n", [1, 31, 257])
def test_half_few_rows(n):
    """1 / 31 / 257 rows at (N, 64, 64): less than one wave group, one short of it, one row into a second workgroup tile"""
    p, x, gy, plain, rounded = _case(n, 64, 64, "SSS", dense_gy=True)
    got = kanlinear_fwd_bwd(p, x, gy, G, K, ops.PREC_HALF)
    half_statement(got, plain, rounded, half_classes("SSS"), f"half.rows({n},64,64)", rows=())


def test_half_second_pass_of_the_persistent_grids():
    """N = 65 537 at (N, 64, 40), dense gy: the first tile of a second pass of the forward's and the input gradient's 256 persistent
    workgroups (test_second_pass_of_the_persistent_grids_vs_oracle for the other modes)"""
    n, fi, fo = 65537, 64, 40
    p, x, gy, plain, rounded = _case(n, fi, fo, "SSS", dense_gy=True)
    got = kanlinear_fwd_bwd(p, x, gy, G, K, ops.PREC_HALF)
    half_statement(got, plain, rounded, half_classes("SSS"), f"half.second_pass({n},{fi},{fo})", rows=())
    # rows are independent across the pass boundary: the slice alone gives the same bits (the instantiation does not depend on N)
    layer = _dev_layer(p)
    with torch.no_grad():
        assert torch.equal(layer(x[65280:65537].to(DEV)), got["y"][65280:65537])


@pytest.mark.parametrize("off", [4, 3])
def test_half_on_column_slices(off):
    """x, gy and both outputs as column slices at offset 4 (16-byte aligned rows) and 3 (not) of wider buffers, through the C entry
    points with their own leading dimensions: the bits of the contiguous copies, and not a byte outside the slices"""
    n, fi, fo = 777, 64, 48
    p, x, gy = _inputs(n, fi, fo, seed=21 + off)
    layer = _dev_layer(p)
    bw, sw, sc = _weights(layer)
    knots, mode = layer._knots(), ops.PREC_HALF
    pf, pd = _packs(layer, mode)
    pad = 8

    def run(strided):
        def place(t, fill):
            if not strided:
                return t.to(DEV).contiguous(), None
            buf = torch.full((n, t.size(1) + pad), fill, device=DEV)
            buf[:, off:off + t.size(1)] = t.to(DEV)
            return buf[:, off:off + t.size(1)], buf
        xv, _ = place(x, 0.25)
        gv, _ = place(gy, -0.5)
        yv, ybuf = place(torch.zeros(n, fo), 7.0)
        gxv, gxbuf = place(torch.zeros(n, fi), -9.0)
        wb = ops._sizes("kagnn_kan_fwd_workspace_bytes", n, fi, fo, G, K, mode)
        ws = ops._ws(wb, xv.device) if wb else None
        ops._call("kagnn_kan_linear_fwd", ops._ptr(xv), ops._ld(xv), n, ops._ptr(knots), fi, fo, G, K, mode, ops._ptr(pf), ops._ptr(yv),
                  ops._ld(yv), ops._ptr(ws), wb, ops._stream())
        ops._call("kagnn_kan_linear_bwd_input", ops._ptr(xv), ops._ld(xv), ops._ptr(gv), ops._ld(gv), n, ops._ptr(knots), fi, fo, G, K, mode,
                  ops._ptr(pd), ops._ptr(gxv), ops._ld(gxv), ops._lib.DTYPE_F32, ops._stream())
        gw = ops._kan_bwd_weight_raw(xv, gv, knots, sw, sc, fi, fo, G, K, mode, True)
        return yv, gxv, gw, ybuf, gxbuf
    yc, gxc, gwc, _, _ = run(False)
    ys, gxs, gws, ybuf, gxbuf = run(True)
    assert ys.stride(0) == fo + pad and gxs.stride(0) == fi + pad
    assert torch.equal(ys, yc) and torch.equal(gxs, gxc)
    for a, b, k in zip(gws, gwc, KAN_GRADS):
        assert torch.equal(a, b), k
    for buf, w, fill in ((ybuf, fo, 7.0), (gxbuf, fi, -9.0)):
        outside = torch.cat([buf[:, :off], buf[:, off + w:]], dim=1)
        assert bool((outside == fill).all()), "written outside the slice"
    plain, rounded = half_layer_oracles(x, gy, p, K, "SSS")
    got = {"y": ys, "gx": gxs, **dict(zip(KAN_GRADS, gws))}
    half_statement(got, plain, rounded, half_classes("SSS"), f"half.column_slices(offset {off})")


# ====================================================================== 4. what the switch must leave alone
@pytest.mark.parametrize("n,fi,fo,grid,k", [(300, 40, 24, 4, 4), (257, 33, 40, 8, 1), (400, 40, 160, 3, 2), (300, 64, 64, 13, 3), (257, 40, 70, 20, 3)],
                         ids=lambda v: str(v))
def test_half_leaves_the_other_kanlinear_kernels_alone(n, fi, fo, grid, k):
    """other orders, 9..16 coefficients (13 + 3: the two-window kernels) and more than 16 (20 + 3: two coefficient groups of 12 and
    11): no single-product instantiation -- the bits of PREC_SPLIT, at the ordinary fp64 bound"""
    assert half_routing(fi, fo, grid, k) == (False, False, False)
    gen = torch.Generator().manual_seed(n + fi + grid)
    p = orc.init_kan_linear(fi, fo, grid, k, gen)
    x = torch.randn(n, fi, generator=gen) * 0.7
    gy = torch.randn(n, fo, generator=gen)
    got = kanlinear_fwd_bwd(p, x, gy, grid, k, ops.PREC_HALF)
    split = kanlinear_fwd_bwd(p, x, gy, grid, k, ops.PREC_SPLIT)
    y64, gx64, g64 = oracle_kan_linear_fwd_bwd(x, gy, p, k)
    plain = {"y": y64, "gx": gx64, **g64}
    half_statement(got, plain, plain, half_classes("TTT"), f"half.untouched.kanlinear({n},{fi},{fo},G={grid},k={k})", split, rows=())


@pytest.mark.parametrize("use_ln", [True, False], ids=["layernorm", "plain"])
@pytest.mark.parametrize("n,fi,fo,ng", [(300, 64, 64, 8), (129, 40, 160, 5)])
def test_half_leaves_the_fastkan_kernels_alone(n, fi, fo, ng, use_ln):
    """the RBF kernels have no single-product form: FastKANLayer under PREC_HALF is PREC_SPLIT to the bit, at the fp64 bound"""
    torch.manual_seed(n + ng)
    layer = kagnn_amd.FastKANLayer(fi, fo, num_grids=ng, use_base_update=True, use_layernorm=use_ln)
    if use_ln:
        layer.layernorm.weight.data.uniform_(0.5, 1.5)
        layer.layernorm.bias.data.uniform_(-0.3, 0.3)
    x = torch.randn(n, fi) * 1.3 + 0.2
    gy = torch.randn(n, fo)
    p64 = {k: v.detach().double() for k, v in layer.state_dict().items()}
    w64 = {k: v.clone().requires_grad_(True) for k, v in p64.items() if k != "rbf.grid"}
    x64 = x.double().requires_grad_(True)
    y64 = orc.fastkan_layer_forward(x64, w64.get("layernorm.weight"), w64.get("layernorm.bias"), p64["rbf.grid"], layer.rbf.denominator,
                                    w64["spline_linear.weight"], w64.get("base_linear.weight"), w64.get("base_linear.bias"))
    y64.backward(gy.double())
    layer = layer.to(DEV)
    res = {}
    for mode in (ops.PREC_HALF, ops.PREC_SPLIT):
        layer.precision = mode
        layer.zero_grad()
        xd = x.to(DEV).requires_grad_(True)
        y = layer(xd)
        y.backward(gy.to(DEV))
        res[mode] = {"y": y.detach(), "gx": xd.grad, **{k: q.grad.clone() for k, q in layer.named_parameters() if q.requires_grad}}
    plain = {"y": y64.detach(), "gx": x64.grad, **{k: v.grad for k, v in w64.items()}}
    assert set(res[ops.PREC_HALF]) == set(plain)
    half_statement(res[ops.PREC_HALF], plain, plain, {k: THREE for k in plain}, f"half.untouched.fastkan({n},{fi},{fo},{ng},ln={use_ln})",
                   res[ops.PREC_SPLIT], rows=())


def test_half_at_17_coefficients_is_one_group_of_each_kind():
    """(300, 64, 64, G = 14, k = 3): ops.kan_linear cuts 17 coefficients into groups of 9 and 8.  The first group (with the SiLU branch)
    runs the two-window three-product kernels; the second is a cubic 8-coefficient layer on 64 inputs and 64 outputs: every kernel
    of it single-product.  So: g_base_weight and g_spline_weight[..., :9] are PREC_SPLIT's bits at the fp64 bound;
    g_spline_weight[..., 9:] and g_spline_scaler (the sum over both groups) meet the single-product statement; y and gx are sums of a
    three-product and a once-rounded part -- held to the routed oracle at the mode's two norms and the 5x separation (not the floor:
    the rounded group moves y by 1e-5 of its maximum only), and they are NOT PREC_SPLIT's bits.  Spline weights x 30, so that the second
    group is not lost beside the SiLU branch."""
    n, fi, fo, grid = 300, 64, 64, 14
    gen = torch.Generator().manual_seed(n + fi + grid)
    p = orc.init_kan_linear(fi, fo, grid, K, gen)
    p["spline_weight"] = p["spline_weight"] * 30.0
    x = torch.randn(n, fi, generator=gen) * 0.8
    gy = torch.randn(n, fo, generator=gen)
    got = kanlinear_fwd_bwd(p, x, gy, grid, K, ops.PREC_HALF)
    split = kanlinear_fwd_bwd(p, x, gy, grid, K, ops.PREC_SPLIT)
    y64, gx64, g64 = oracle_kan_linear_fwd_bwd(x, gy, p, K)
    plain = {"y": y64, "gx": gx64, **g64}
    with half_mode_oracle():                                     # (routes each coefficient group on its own: helpers.coefficient_groups)
        yr, gxr, gr = oracle_kan_linear_fwd_bwd(x, gy, p, K)
    rounded = {"y": yr, "gx": gxr, **gr}
    cut = lambda d: {**{k: v for k, v in d.items() if k != "spline_weight"}, "spline_weight[:9]": d["spline_weight"][..., :9],
                     "spline_weight[9:]": d["spline_weight"][..., 9:]}
    got, split, plain, rounded = (cut(d) for d in (got, split, plain, rounded))
    tag = f"half.17_coefficients({n},{fi},{fo},G={grid})"
    classes = {"base_weight": THREE, "spline_weight[:9]": THREE, "spline_weight[9:]": SINGLE, "spline_scaler": SINGLE}
    half_statement({k: got[k] for k in classes}, plain, rounded, classes, tag, split, rows=())
    for k in ("y", "gx"):
        lr, _ = half_parity(got[k], rounded[k], plain[k], f"{tag}.{k}")
        REPORT[tag][k] = {"class": "sum of a three-product and a single-product group", "l2_vs_rounding_oracle": lr,
                          "l2_vs_unrounded": l2_rel(got[k], plain[k]), "max_norm_vs_rounding_oracle": max_rel(got[k], rounded[k]),
                          "max_norm_vs_unrounded": max_rel(got[k], plain[k])}
        assert not torch.equal(got[k], split[k]), k


def test_half_at_spline_order_8_is_the_exact_fp32_path():
    """orders above 4 run the exact-fp32 kernels whatever precision was asked for (ops.kan_linear): the PREC_FP32 bits"""
    n, fi, fo, grid, k = 200, 20, 24, 3, 8
    gen = torch.Generator().manual_seed(8)
    p = orc.init_kan_linear(fi, fo, grid, k, gen)
    x = torch.randn(n, fi, generator=gen) * 0.7
    gy = torch.randn(n, fo, generator=gen)
    a = kanlinear_fwd_bwd(p, x, gy, grid, k, ops.PREC_HALF)
    b = kanlinear_fwd_bwd(p, x, gy, grid, k, ops.PREC_FP32)
    for key in a:
        assert torch.equal(a[key], b[key]), key


# ====================================================================== 5. the graph-level one-call paths
def test_half_graph_level_one_call_paths(golden, monkeypatch):
    """KAGINRegression on the ZINC-shaped fixture batch (256 graphs / 5 932 nodes / 12 670 edges, hidden 32, grid 4) with every layer at
    PREC_HALF: the whole-model call (kagnn_kagin_model_fwd / _bwd), the one-node model, the stack call (kagnn_gine_kan_stack_fwd / _bwd)
    and the per-convolution nodes give the same bits everywhere -- the claim test_gine_one_library_call_each_way_matches_the_composition
    makes for split mode (the per-OPERATION composition takes its batch statistics from another pass and is not bit-equal there
    either).  Hidden width 32: narrow three-product forwards beside single-product gradients, which the routed oracle knows.
    Predictions against ``orc.graph_regression_forward`` under that oracle at the logits bound of the config-2 model test (1e-3);
    gradients at model depth are recorded against both oracles, and the rounding oracle must explain each of them better.
    (Every forward of this fixture's model is narrow, so the one-call paths' single-product FORWARD, the batched read-out packs
    included, is not reached here; the layer-level one-call path at 64 features is test_half_mode_gin_layer_one_call_path_vs_rounding_oracle.)"""
    z = golden("g8b_zinc_batch")

    class Data:
        pass
    d = Data()
    d.x, d.edge_index, d.batch = T(z["x"], DEV), T(z["edge_index"], DEV), T(z["batch"], DEV)
    d.edge_attr, d.num_graphs = T(z["edge_attr"], DEV), 256
    y = T(z["kan.y"], DEV)
    m = kagnn_amd.KAGINRegression(1, 1, 3, 32, 2, 4, 3, 1, 0.0, True)
    m.atom_encoder = kagnn_amd.graph_models.AtomEncoder(32, [21])
    m.bond_encoder.bond_embedding_list = torch.nn.ModuleList([torch.nn.Embedding(4, 32)])
    pre = "kan.state."
    state = {k[len(pre):]: T(z[k], DEV) for k in z.files if k.startswith(pre)}
    for mod in m.modules():
        if hasattr(mod, "precision"):
            mod.precision = ops.PREC_HALF
    res = {}
    for how in ("call", "model", "stack", "layer", "ops"):
        monkeypatch.setattr(graph_ops, "_GINE_MODEL_CALL", how == "call")
        monkeypatch.setattr(graph_ops, "_GINE_MODEL_NODE", how in ("call", "model"))
        monkeypatch.setattr(graph_ops, "_GINE_STACK_ABI", how in ("call", "model", "stack"))
        monkeypatch.setattr(graph_ops, "_GINE_LAYER_ABI", how != "ops")
        m.load_state_dict(state, strict=True)
        m = m.to(DEV).train()
        m.zero_grad()
        timer = ops.EntryPointTimer()
        ops.set_timer(timer)
        try:
            pred = m(d)
            loss = torch.nn.L1Loss()(pred.squeeze(), y)
            loss.backward()
        finally:
            ops.set_timer(None)
        res[how] = (pred.detach().clone(), float(loss), {k: q.grad.clone() for k, q in m.named_parameters() if q.grad is not None},
                    [r[0] for r in timer.records])
    assert res["call"][3].count("kagnn_kagin_model_fwd") == 1 and res["call"][3].count("kagnn_kagin_model_bwd") == 1, res["call"][3]
    assert res["stack"][3].count("kagnn_gine_kan_stack_fwd") == 1 and res["stack"][3].count("kagnn_gine_kan_stack_bwd") == 1, res["stack"][3]
    assert res["layer"][3].count("kagnn_gine_kan_layer_fwd") == 3 and res["layer"][3].count("kagnn_gine_kan_layer_bwd") == 3, res["layer"][3]
    for how in ("call", "model", "stack"):
        assert torch.equal(res[how][0], res["layer"][0]) and res[how][1] == res["layer"][1], how
        assert set(res[how][2]) == set(res["layer"][2])
        for k, gref in res["layer"][2].items():
            assert torch.equal(res[how][2][k], gref), (how, k)
    # the per-OPERATION composition (aggregate_gine -> pack -> KANLinear x 2 -> BatchNorm, each its own library call) under PREC_HALF.
    # Its batch statistics come from the statistics pass instead of the forward kernel's epilogue, so it is not bit-equal in any
    # mode.  Predictions and loss: every forward here is three-product, so the bounds the split-mode test
    # (test_gine_one_library_call_each_way_matches_the_composition) holds them to.  Gradients: a last-bit difference of a norm's
    # output puts single-product operands on the other side of an fp16 tie, and at model depth one flip is ~3e-4 of a gradient
    # (3.5e-4 measured between the two routes; split mode's 1e-4 between them cannot hold) -- like every gradient at model depth
    # they get no number of their own: recorded below against both oracles, and the rounding oracle must explain them better
    on = res["ops"][3]
    assert "kagnn_aggregate_gine" in on and "kagnn_gine_kan_layer_fwd" not in on, on
    assert_close(res["layer"][0], res["ops"][0], 2e-5, what="half gine one-call pred vs the per-operation composition")
    assert abs(res["layer"][1] - res["ops"][1]) <= 1e-6
    assert set(res["ops"][2]) == set(res["layer"][2])
    # the mode ran: not the bits of PREC_SPLIT (on the one-call route again)
    for flag in ("_GINE_MODEL_CALL", "_GINE_MODEL_NODE", "_GINE_STACK_ABI", "_GINE_LAYER_ABI"):
        monkeypatch.setattr(graph_ops, flag, True)
    for mod in m.modules():
        if hasattr(mod, "precision"):
            mod.precision = ops.PREC_SPLIT
    m.load_state_dict(state, strict=True)
    m = m.to(DEV).train()
    m.zero_grad()
    pred_s = m(d)
    torch.nn.L1Loss()(pred_s.squeeze(), y).backward()
    # (every KANLinear here has 32 or fewer inputs: narrow forwards, three-product -- the predictions are PREC_SPLIT's to the bit, and
    # the mode shows in the gradients alone)
    assert torch.equal(pred_s.detach(), res["call"][0])
    assert any(not torch.equal(q.grad, res["call"][2][k]) for k, q in m.named_parameters() if q.grad is not None)

    def oracle():
        st = {k[len(pre):]: (T(z[k]).double().requires_grad_(True) if z[k].dtype.kind == "f" else T(z[k])) for k in z.files if k.startswith(pre)}
        p64 = orc.graph_regression_forward(T(z["x"]), T(z["edge_index"]), T(z["edge_attr"]), T(z["batch"]), 256, st, "kan", 3)
        (p64.squeeze() - T(z["kan.y"]).double()).abs().mean().backward()
        return p64.detach(), {k: v.grad for k, v in st.items() if torch.is_tensor(v) and v.requires_grad and v.grad is not None}
    pred64, g64 = oracle()
    with half_mode_oracle():
        predr, gr = oracle()
    tag = "half.graph_level_one_call"
    rep = REPORT.setdefault(tag, {})
    pred = res["call"][0]
    rep["pred"] = {"class": THREE + " (every forward of this model is narrow)", "max_norm_vs_rounding_oracle": max_rel(pred, predr),
                   "max_norm_vs_unrounded": max_rel(pred, pred64), "l2_vs_rounding_oracle": l2_rel(pred, predr), "l2_vs_unrounded": l2_rel(pred, pred64)}
    check(rep["pred"]["max_norm_vs_rounding_oracle"] <= 1e-3, f"{tag}: predictions vs the rounding oracle", rep["pred"])
    gmax = max(float(v.abs().max()) for v in g64.values())
    for route, grads in (("one call", res["call"][2]), ("per operation", res["ops"][2])):
        dr = dp = 0.0
        for k, g in grads.items():
            if k not in g64 or float(g64[k].abs().max()) <= 1e-12 * gmax:        # (a bias in front of a training-mode BatchNorm: identically zero)
                continue
            e = {"class": SINGLE + " gradients at model depth: recorded, not bounded", "max_norm_vs_rounding_oracle": max_rel(g, gr[k]),
                 "max_norm_vs_unrounded": max_rel(g, g64[k]), "l2_vs_rounding_oracle": l2_rel(g, gr[k]), "l2_vs_unrounded": l2_rel(g, g64[k])}
            if route == "per operation":
                e["max_norm_vs_the_one_call_path"] = max_rel(g, res["call"][2][k])
            rep[f"grad.{k} ({route})"] = e
            check(e["l2_vs_rounding_oracle"] < e["l2_vs_unrounded"], f"{tag}: grad.{k} ({route}): the rounding oracle must explain it better than the unrounded one", e)
            dr += e["l2_vs_rounding_oracle"] ** 2
            dp += e["l2_vs_unrounded"] ** 2
        rep[f"gradients ({route}), root sum of squared L2 distances"] = {"vs_rounding_oracle": dr ** 0.5, "vs_unrounded": dp ** 0.5}
        check(dr < dp, f"{tag} ({route}): the rounding oracle must explain the gradients better than the unrounded one", (dr ** 0.5, dp ** 0.5))


def test_zz_half_mode_report():
    """(last of the half-mode tests) the report file once more, now with every case above beside those of tests/test_gpu_half.py"""
    import test_gpu_half
    test_gpu_half.test_zz_half_mode_report()
