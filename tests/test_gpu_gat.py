"""The GAT attention aggregation (``csrc/gat.hip`` behind ``ops.gat_aggregate``) and its callers against the fp64 restatement
of torch_geometric's GATConv (``oracle.gat_conv``, ``oracle.node_model_forward(conv_type="gat")``).

gat.hip picks between several kernels per call: the packed-heads ``*_rows`` kernels or the per-(row, head) wave kernels, the
hub kernels for long rows, the attention-vector gradient ``gat_att_grad_partial<KC>`` by width (or a torch contraction beyond
1024 columns).  ``gat_kernels`` restates that choice; ``KERNEL_CASES`` is parametrised so that every kernel and variant runs
(``tests/test_host_cpu.py::test_gat_kernel_cases_reach_every_gat_kernel_and_variant`` checks it without a GPU), and every case
compares the output and the gradients of xh, att_src, att_dst and bias with fp64."""
import os
import re
import subprocess
import sys

import pytest
import torch

import kagnn_amd
from kagnn_amd import ekan, ops
from oracle import kan_oracle as orc
from helpers import assert_close, gat_att_noise, must_fail, oracle_node_model_fwd_bwd, prenorm_bias_noise
from test_gpu_models import _cora_like, _set_precision

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = [ops.PREC_FP32, ops.PREC_SPLIT]
MODE_IDS = ["fp32", "split"]

# ------------------------------------------------------------------ the dispatch of gat.hip, restated
PACKED_C = (4, 8, 16, 32, 64)      # gat.hip:521 (gat_packed_ok)
PACKED_MAX_HC = 128                # gat.hip:523 (64 * kPk)
MAX_C = 128                        # gat.hip:19 kGatMaxK = 8 -> 16 * 8 channels per head; :539 / :560 refuse more
ATT_GRAD_MAX_HC = 1024             # gat.hip:664 and ops._GatFn.backward: a torch contraction beyond
SMALL_CSR_MAX = 65536              # csr.hip:69-71 csr_small_ok: the one-launch CSR build makes no hub segments
SRC_HUB = 1500                     # out-edges of one source, all walked by one lane group of gat_bwd_src* (no hub variant)


def _cdiv(a, b):
    return -(-a // b)


def gat_kernels(H, C, n, e, max_in, max_out=0, csr="small", ld_ok=True, bias_aligned=True):
    """what one forward + backward of ``ops.gat_aggregate`` runs, as gat.hip and ops.py choose it: kernel names as rocprofv3
    lists them plus the variants that matter (channel chunks of the per-head kernels, hub rows, layout refusals).
    ``max_in`` / ``max_out``: the longest neighbour list of a destination / source; ``csr``: 'small' (the one-launch build,
    taken when csr_small_ok holds and ops._SMALL_CSR is on) or 'rocprim'; ``ld_ok``: every row stride a multiple of 4 floats
    and every matrix 16-byte aligned; ``bias_aligned``: the bias 16-byte aligned."""
    if C > MAX_C:
        return {"refused"}
    hc = H * C
    ks = {"gat_logits"}
    shape_ok = C in PACKED_C and hc <= PACKED_MAX_HC
    packed = shape_ok and ld_ok and bias_aligned                 # gat.hip:519-524, :541, :563-565
    if packed:
        ks |= {"gat_fwd_rows", "gat_bwd_dst_rows", "gat_bwd_src_rows"}
    else:
        ks |= {"gat_fwd", "gat_bwd_dst", "gat_bwd_src", f"wave chunks {_cdiv(C, 16)}"}
        if shape_ok:
            ks.add("packed refused by layout")
    small = csr == "small" and 1 <= e <= SMALL_CSR_MAX and 1 <= n <= SMALL_CSR_MAX
    if max_in > ops.HUB_THRESHOLD and not small:                 # csr.hip:41 hub segments; gat.hip:540, :546, :573
        ks |= {"gat_fwd_hub", "gat_bwd_dst hub", f"hub chunks {_cdiv(C, 16)}", "packed + hub" if packed else "wave + hub"}
    elif max_in > ops.HUB_THRESHOLD:
        ks.add("long row in the row kernels")
    if max_out >= SRC_HUB:
        ks.add("source hub")
    if hc > ATT_GRAD_MAX_HC:
        ks.add("att grad torch fallback")
    else:
        kc = _cdiv(hc, 64)                                         # gat.hip:670-672
        ks |= {f"gat_att_grad_partial<{next(k for k in (1, 2, 4, 8, 16) if kc <= k)}>", "gat_att_grad_finish"}
    return ks


# ------------------------------------------------------------------ kernel-level cases
def _case(name, H, C, n, e, seed, **kw):
    return dict(name=name, H=H, C=C, n=n, e=e, seed=seed, dst_hub=kw.get("dst_hub", 0), src_hub=kw.get("src_hub", 0),
                csr=kw.get("csr", "small"), layout=kw.get("layout", "plain"), logits=kw.get("logits", "unit"))


KERNEL_CASES = [
    # packed heads (C in {4, 8, 16, 32, 64}, H * C <= 128)
    _case("packed H1C4", 1, 4, 300, 2000, 1),
    _case("packed H2C64", 2, 64, 500, 4000, 2),
    _case("packed H4C32 hub", 4, 32, 3000, 30000, 3, dst_hub=1000, csr="rocprim"),
    _case("packed H1C64 hub", 1, 64, 2000, 20000, 4, dst_hub=600, csr="rocprim"),
    _case("packed H4C8 source hub", 4, 8, 3000, 20000, 5, src_hub=1600),
    _case("packed H2C16 long row", 2, 16, 1500, 10000, 6, dst_hub=700),
    # per-(row, head) wave kernels
    _case("wave H3C2", 3, 2, 400, 3000, 7),
    _case("wave H4C17", 4, 17, 600, 5000, 8),
    _case("wave H2C33 hub", 2, 33, 2500, 25000, 9, dst_hub=700, csr="rocprim"),
    _case("wave H1C100", 1, 100, 500, 4000, 10),
    _case("wave H1C128 hub", 1, 128, 2000, 20000, 11, dst_hub=1000, csr="rocprim"),
    _case("wave H4C64 source hub", 4, 64, 2500, 12000, 12, src_hub=1600),
    _case("wave H4C128", 4, 128, 800, 6000, 13),
    _case("wave H8C128 hub", 8, 128, 1200, 9000, 14, dst_hub=400, csr="rocprim"),
    _case("fallback H9C128", 9, 128, 300, 2000, 15),
    # the packed path refused by layout alone
    _case("layout xh ld%4!=0 H2C32", 2, 32, 700, 6000, 16, layout="ld"),
    _case("layout bias misaligned H2C32 hub", 2, 32, 2000, 20000, 17, dst_hub=500, csr="rocprim", layout="bias"),
    # graph edges (self loops, duplicates and isolated nodes are in every case with enough edges)
    _case("N1 E0", 2, 8, 1, 0, 18),
    _case("N5 E0 wave", 1, 20, 5, 0, 19),
    _case("N2 E1", 2, 16, 2, 1, 20),
    # softmax numerics
    _case("logits ~90 packed", 2, 16, 1500, 12000, 21, logits="big"),
    _case("logits ~90 wave hub", 2, 20, 2000, 20000, 22, dst_hub=800, csr="rocprim", logits="big"),
    _case("rising logits hub", 2, 24, 1400, 8000, 23, csr="rocprim", logits="rising"),
    _case("rising logits long row packed", 2, 16, 1400, 8000, 24, logits="rising"),
    _case("rising logits long row wave", 2, 24, 1400, 8000, 25, logits="rising"),
]
RISING = 1100          # neighbours of the rising-logit row


def gat_graph(case):
    """edge_index [2, E] on the host: random edges among the first 95 % of the nodes (the rest isolated), explicit self loops,
    duplicate edges, then the case's destination hub (node 7), source hub (node 3) or rising-logit row (node 0, sources
    1..RISING in this order, so its CSR neighbour list is in that order too)"""
    n, e = case["n"], case["e"]
    if e == 0:
        return torch.zeros(2, 0, dtype=torch.long)
    g = torch.Generator().manual_seed(case["seed"])
    m = max(1, n - n // 20)
    lo = 1 if case["logits"] == "rising" else 0                   # no random edge into the rising row
    src = torch.randint(0, m, (e,), generator=g)
    dst = torch.randint(lo, max(lo + 1, m), (e,), generator=g) % m
    k = min(20, e // 4)
    src[:k] = dst[:k] = (torch.arange(k) + lo) % m                  # explicit self loops (removed, one re-added per node)
    d = min(20, e // 8)
    if d:
        src[k:k + d], dst[k:k + d] = src[k + d:k + 2 * d].clone(), dst[k + d:k + 2 * d].clone()   # duplicates
    off = k + 2 * d
    if case["dst_hub"]:
        dst[off:off + case["dst_hub"]] = 7 % m
        off += case["dst_hub"]
    if case["src_hub"]:
        src[off:off + case["src_hub"]] = 3 % m
    if case["logits"] == "rising":
        src[e - RISING:], dst[e - RISING:] = torch.arange(1, RISING + 1), 0
    return torch.stack([src, dst])


def case_kernels(case):
    ei = gat_graph(case)
    n = case["n"]
    deg_in = torch.bincount(ei[1], minlength=n)
    deg_out = torch.bincount(ei[0], minlength=n)
    return gat_kernels(case["H"], case["C"], n, ei.size(1), int(deg_in.max()), int(deg_out.max()), case["csr"],
                       ld_ok=case["layout"] != "ld", bias_aligned=case["layout"] != "bias")


def _inputs(case):
    """fp32 host tensors xh [n, H*C], att_src / att_dst [1, H, C], bias [H*C], upstream gradient"""
    n, H, C = case["n"], case["H"], case["C"]
    g = torch.Generator().manual_seed(100 + case["seed"])
    xh = torch.randn(n, H * C, generator=g) * 0.7
    a_s = torch.randn(1, H, C, generator=g) * 0.5
    a_d = torch.randn(1, H, C, generator=g) * 0.5
    b = torch.randn(H * C, generator=g) * 0.1
    gy = torch.randn(n, H * C, generator=g)
    x3 = xh.view(n, H, C)
    if case["logits"] == "big":
        # every destination logit ~85 (one channel of value 85 under att_dst = 1): e_ij up to ~95, past log(FLT_MAX) = 88.7
        x3[:, :, 0] = 85.0
        a_d[0, :, 0] = 1.0
        a_s[0, :, 0] = 0.05
    elif case["logits"] == "rising":
        # a_s of sources 1..RISING strictly increasing (-2 .. 2, both sides of the leaky ReLU's kink), node 0's own below them
        rows = torch.arange(0, RISING + 1)
        tgt = torch.cat([torch.tensor([-3.0], dtype=torch.float64), torch.linspace(-2.0, 2.0, RISING, dtype=torch.float64)])
        for h in range(H):
            a = a_s[0, h].double()
            cur = x3[rows, h].double() @ a
            x3[rows, h] = (x3[rows, h].double() + ((tgt - cur) / (a @ a)).unsqueeze(1) * a).float()
    return xh, a_s, a_d, b, gy


def _reference(case, ei, xh, a_s, a_d, b, gy):
    leaves = [t.double().requires_grad_(True) for t in (xh, a_s, a_d, b)]
    want = orc.gat_conv(leaves[0], ei, lambda t: t, leaves[1], leaves[2], leaves[3], case["H"])
    want.backward(gy.double())
    return want.detach(), [t.grad for t in leaves]


def _device_inputs(case, xh, a_s, a_d, b):
    hc = xh.size(1)
    if case["layout"] == "ld":               # a column slice of a wider matrix: row stride H*C + 1 floats
        wide = torch.zeros(xh.size(0), hc + 1, device=DEV)
        wide[:, :hc] = xh.to(DEV)
        xd = wide[:, :hc].detach().requires_grad_(True)
        assert xd.stride(0) % 4 != 0
    else:
        xd = xh.to(DEV).requires_grad_(True)
    if case["layout"] == "bias":             # the bias 4 bytes past a 16-byte boundary
        buf = torch.zeros(hc + 1, device=DEV)
        buf[1:] = b.to(DEV)
        bd = buf[1:].detach().requires_grad_(True)
        assert bd.data_ptr() % 16 == 4
    else:
        bd = b.to(DEV).requires_grad_(True)
    return [xd, a_s.to(DEV).requires_grad_(True), a_d.to(DEV).requires_grad_(True), bd]


def _run_device(case, ei, xh, a_s, a_d, b, gy, monkeypatch):
    if case["csr"] == "rocprim":
        monkeypatch.setattr(ops, "_SMALL_CSR", False)
    gi = ops.GraphIndex(ei.to(DEV), case["n"])
    dl = _device_inputs(case, xh, a_s, a_d, b)
    got = ops.gat_aggregate(dl[0], dl[1], dl[2], dl[3], gi, case["H"], case["C"])
    got.backward(gy.to(DEV))
    torch.cuda.synchronize()
    return gi, got.detach(), [t.grad for t in dl]


@pytest.mark.parametrize("case", KERNEL_CASES, ids=[c["name"] for c in KERNEL_CASES])
def test_gat_aggregate_vs_fp64(case, monkeypatch):
    ei = gat_graph(case)
    xh, a_s, a_d, b, gy = _inputs(case)
    want, gw = _reference(case, ei, xh, a_s, a_d, b, gy)
    gi, got, gg = _run_device(case, ei, xh, a_s, a_d, b, gy, monkeypatch)
    assert (gi.num_hub_seg > 0) == ("gat_fwd_hub" in case_kernels(case)), gi.num_hub_seg
    n = case["n"]
    scale = 1.0
    if case["logits"] != "unit":
        x3 = xh.double().view(n, case["H"], -1)
        ls, ld_ = (x3 * a_s.double()).sum(-1), (x3 * a_d.double()).sum(-1)
        keep = ei[0] != ei[1]
        if case["logits"] == "big":
            e = torch.nn.functional.leaky_relu(ls[ei[0][keep]] + ld_[ei[1][keep]], 0.2)
            assert float(e.max()) > 88.8, float(e.max())         # exp(e) without the running maximum overflows fp32
            scale = float(xh.abs().max()) * float(e.abs().max())
        else:
            row = ls[ei[0][(ei[1] == 0) & keep]]                   # node 0's neighbours in CSR order (stable by destination)
            assert row.size(0) == RISING and bool((row[1:] > row[:-1]).all()) and bool((row[0] > ls[0]).all())
    tag = f"gat[{case['name']}]"
    assert_close(got, want, what=tag + ".out")
    for nme, a, w in zip(("xh", "att_src", "att_dst", "bias"), gg, gw):
        noise = gat_att_noise(n, scale) if nme.startswith("att_") else 0.0
        assert_close(a, w, what=f"{tag}.g_{nme}", noise=noise)


@pytest.mark.parametrize("name", ["packed H4C32 hub", "wave H2C33 hub", "wave H8C128 hub"])
def test_gat_aggregate_is_bit_reproducible_with_hub_rows(name, monkeypatch):
    """the hub kernels merge their 16 lane groups' softmax states, and the attention-vector gradient its per-workgroup partial
    sums, in a fixed order: two runs on freshly built indices give the same bits"""
    case = next(c for c in KERNEL_CASES if c["name"] == name)
    ei = gat_graph(case)
    xh, a_s, a_d, b, gy = _inputs(case)
    runs = []
    for _ in range(2):
        gi, got, gg = _run_device(case, ei, xh, a_s, a_d, b, gy, monkeypatch)
        assert gi.num_hub_seg > 0
        runs.append([got] + gg)
    for k, (p, q) in enumerate(zip(*runs)):
        assert torch.equal(p, q), (name, k, float((p - q).abs().max()))


def test_gat_refuses_more_than_128_channels_per_head():
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]], device=DEV)
    gi = ops.GraphIndex(ei, 3)
    for heads, c in ((1, 129), (2, 200)):
        xh = torch.randn(3, heads * c, device=DEV)
        a = torch.randn(1, heads, c, device=DEV)
        with pytest.raises(RuntimeError, match="more than 128 channels per head"):
            ops.gat_aggregate(xh, a, a, None, gi, heads, c)


# ------------------------------------------------------------------ convolutions
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("arch,k", [("kan", 1), ("kan", 2), ("kan", 3), ("fastkan", 2), ("fastkan", 32)],
                         ids=["kan-order1", "kan-order2", "kan-order3", "fastkan-grid2", "fastkan-grid32"])
def test_gat_conv_vs_fp64(arch, k, mode):
    """KAGATConv (spline orders 1..3) and FASTKAGATConv (2 and 32 grids, the ends of the reference's search range) against the
    fp64 GATConv, every gradient, both precision modes; packed heads for KAN (4 x 16), wave kernels for FastKAN (3 x 20)"""
    n, fi = 900, 24
    case = _case(f"conv {arch}", 4 if arch == "kan" else 3, 16 if arch == "kan" else 20, n, 8000, 40 + k, dst_hub=300)
    ei = gat_graph(case)
    heads, c = case["H"], case["C"]
    torch.manual_seed(50 + k)
    if arch == "kan":
        conv = kagnn_amd.KAGATConv(fi, c, heads, grid_size=5, spline_order=k)
    else:
        conv = kagnn_amd.FASTKAGATConv(fi, c, heads, grid_size=k)
    conv.bias.data.uniform_(-0.2, 0.2)
    _set_precision(conv, mode)
    x = torch.randn(n, fi, generator=torch.Generator().manual_seed(k)) * 0.6
    gy = torch.randn(n, heads * c, generator=torch.Generator().manual_seed(k + 1))
    p64 = {nm: v.detach().double().requires_grad_(v.requires_grad) for nm, v in conv.lin.named_parameters()}
    p64.update({nm: v.detach().double() for nm, v in conv.lin.named_buffers()})
    if arch == "kan":
        lin = lambda t: orc.kan_linear_forward(t, p64["base_weight"], p64["spline_weight"], p64["spline_scaler"], p64["grid"], k)
    else:
        lin = lambda t: orc.fastkan_forward(t, [p64])
    a_s, a_d, b = (conv.att_src.detach().double().requires_grad_(True), conv.att_dst.detach().double().requires_grad_(True),
                   conv.bias.detach().double().requires_grad_(True))
    x64 = x.double().requires_grad_(True)
    y64 = orc.gat_conv(x64, ei, lin, a_s, a_d, b, heads)
    y64.backward(gy.double())
    conv = conv.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    y = conv(xd, ei.to(DEV))
    y.backward(gy.to(DEV))
    tag = f"gat_conv.{arch}{k}.{MODE_IDS[mode]}"
    assert_close(y, y64, what=tag + ".y")
    assert_close(xd.grad, x64.grad, what=tag + ".gx")
    assert_close(conv.att_src.grad, a_s.grad, what=tag + ".g_att_src", noise=gat_att_noise(n))
    assert_close(conv.att_dst.grad, a_d.grad, what=tag + ".g_att_dst", noise=gat_att_noise(n))
    assert_close(conv.bias.grad, b.grad, what=tag + ".g_bias")
    for nm, p in conv.lin.named_parameters():
        if p.requires_grad:
            assert_close(p.grad, p64[nm].grad, what=f"{tag}.g_lin.{nm}")


# ------------------------------------------------------------------ node models
def _model_tols(want32, want64):
    """per-tensor (tol, noise) of the node-model checks: 1e-4 of the tensor's own maximum, or twice the reference's OWN fp32
    error where that is larger (README: relaxation 1's rule).  Attention models sum cancelling gradients over all rows (the
    softmax weights of a row sum to one, so the alpha-weighted part of the lin's base-bias gradient cancels exactly): at Cora's
    shape the fp32 oracle is 3.7e-4 off there.  A conv bias in front of the norm has a zero gradient: its bound is absolute,
    the larger of ``prenorm_bias_noise`` and twice the fp32 oracle's own absolute error."""
    out = {}
    for k, w in want64.items():
        err32 = float((want32[k].double() - w).abs().max())
        noise = prenorm_bias_noise(k, {q: v for q, v in want64.items() if q not in ("logits", "gx")})
        if noise:
            out[k] = (1e-4, max(noise, 2.0 * err32))
        else:
            out[k] = (max(1e-4, 2.0 * err32 / max(float(w.abs().max()), 1e-300)), 0.0)
    return out


def _oracles(model, arch, x, ei, gout, chunk):
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    w64, gx64, g64 = oracle_node_model_fwd_bwd(x, ei, state, gout, arch, "gat", 2, 3, chunk)
    w32, gx32, g32 = oracle_node_model_fwd_bwd(x, ei, state, gout, arch, "gat", 2, 3, chunk, dtype=torch.float32)
    tols = _model_tols(dict(g32, logits=w32, gx=gx32), dict(g64, logits=w64, gx=gx64))
    return state, (w64, gx64, g64), tols


def _check_gat_model(model, out, gx, want, tols, label):
    w, gxw, gw = want
    assert_close(out, w, tols["logits"][0], what=f"{label}.logits")
    assert_close(gx, gxw, tols["gx"][0], what=f"{label}.gx")
    for name, p in model.named_parameters():
        if p.requires_grad:
            assert_close(p.grad, gw[name], tols[name][0], what=f"{label}.grad.{name}", noise=tols[name][1])


def _att_src_guards(model, gw, tols, label):
    """the att_src checks above must be able to fail: a zeroed gradient always, a 1e-3-perturbed one where the bound is tighter"""
    bites = 0
    for i, conv in enumerate(model.convs):
        nm = f"convs.{i}.att_src"
        must_fail(torch.zeros_like(conv.att_src.grad), gw[nm], tols[nm][0], what=f"{label}.grad.{nm}")
        if tols[nm][0] <= 5e-4:
            must_fail(conv.att_src.grad * (1.0 + 1e-3), gw[nm], tols[nm][0], what=f"{label}.grad.{nm}")
            bites += 1
    assert bites, {k: v for k, v in tols.items() if k.endswith("att_src")}


def _run_gat_model(model, state, x, ei):
    model.load_state_dict(state)
    model = model.to(DEV).train()
    model.zero_grad(set_to_none=True)
    xd = x.to(DEV).requires_grad_(True)
    return model, xd


@pytest.mark.parametrize("arch,hidden", [("kan", 8), ("fastkan", 20), ("kan", 64), ("fastkan", 128)],
                         ids=["kan-4x8-packed", "fastkan-4x20-wave", "kan-4x64-KC4", "fastkan-4x128-KC8"])
def test_cora_shaped_gat_node_model_vs_oracle(arch, hidden):
    """GKAN_Nodes / GFASTKAN_Nodes('gat', 2 layers, 4 heads, skip) at Cora's shape against oracle.node_model_forward in fp64:
    logits, d/dx and every parameter gradient at 1e-4 of each tensor's own maximum (or twice the fp32 oracle's own error, see
    _model_tols; the conv bias in front of the norm: its noise floor).  Between them the four widths run the packed and the
    wave kernels and the attention-vector gradient at KC 1, 2, 4 and 8.  Mutation guards on att_src."""
    ei, x = _cora_like(seed=hidden)
    torch.manual_seed(30 + hidden)
    if arch == "kan":
        model = kagnn_amd.GKAN_Nodes("gat", 2, 1433, hidden, 7, skip=True, grid_size=5, spline_order=3, heads=4)
    else:
        model = kagnn_amd.GFASTKAN_Nodes("gat", 2, 1433, hidden, 7, skip=True, grid_size=4, heads=4)
    for conv in model.convs:
        conv.bias.data.uniform_(-0.2, 0.2)
    gout = torch.randn(2708, 7, generator=torch.Generator().manual_seed(hidden + 1))
    state, want, tols = _oracles(model, arch, x, ei, gout, 512)
    model, xd = _run_gat_model(model, state, x, ei)
    out = model(xd, ei.to(DEV))
    out.backward(gout.to(DEV))
    label = f"cora.gat.{arch}{hidden}"
    _check_gat_model(model, out, xd.grad, want, tols, label)
    _att_src_guards(model, want[2], tols, label)


BIG_N, BIG_E = 125_000, 125_000


@pytest.fixture(scope="module")
def big_gat_model_case():
    """a >= 120k-row GKAN_Nodes('gat'): the split read-out over [x | h1 | h2] with ops.SkipGradient objects that a GAT
    convolution never consumes, hub rows on the rocPRIM-built index; its fp64 (and fp32) oracle once for this module
    (row-chunked with checkpointing, like the arxiv-shaped tests)"""
    ei = orc.powerlaw_graph(BIG_N, BIG_E, seed=17)
    x = torch.randn(BIG_N, 128, generator=torch.Generator().manual_seed(18)) * 0.5
    torch.manual_seed(19)
    model = kagnn_amd.GKAN_Nodes("gat", 2, 128, 32, 40, skip=True, grid_size=5, spline_order=3, heads=2)
    for conv in model.convs:
        conv.bias.data.uniform_(-0.2, 0.2)
    gout = torch.randn(BIG_N, 40, generator=torch.Generator().manual_seed(20)) / BIG_N     # a mean-type loss gradient
    state, want, tols = _oracles(model, "kan", x, ei, gout, 8192)
    return model, state, x, ei, gout, want, tols


def _big_gat_model_run(case, monkeypatch):
    model, state, x, ei, gout, want, tols = case
    model, xd = _run_gat_model(model, state, x, ei)
    seen = []
    real = ekan.KANLinear.forward_parts
    monkeypatch.setattr(ekan.KANLinear, "forward_parts", lambda self, p, s=None: seen.append(s) or real(self, p, s))
    out = model(xd, ei.to(DEV))
    out.backward(gout.to(DEV))
    # the split read-out ran, with a SkipGradient per convolution input
    assert len(seen) == 1 and seen[0] is not None and all(s is not None for s in seen[0][:-1]), seen
    return model, out, xd.grad, want, tols


def test_big_gat_node_model_split_read_out_vs_oracle(big_gat_model_case, monkeypatch):
    model, out, gx, want, tols = _big_gat_model_run(big_gat_model_case, monkeypatch)
    _check_gat_model(model, out, gx, want, tols, "big.gat")


def test_big_gat_node_model_checks_reject_a_wrong_att_src_gradient(big_gat_model_case, monkeypatch):
    model, _out, _gx, want, tols = _big_gat_model_run(big_gat_model_case, monkeypatch)
    for i, conv in enumerate(model.convs):
        nm = f"convs.{i}.att_src"
        assert_close(conv.att_src.grad, want[2][nm], tols[nm][0], what=f"big.gat.grad.{nm}")
    _att_src_guards(model, want[2], tols, "big.gat")


# ------------------------------------------------------------------ the randomised graph fuzzer
def test_fuzz_graph_sum_and_gat_vs_oracle():
    """tools/fuzz_graph.py inside the suite: 40 random graphs (1..20 000 nodes, no edges to 20 per node, hubs on both sides, self
    loops, duplicates) through the sum aggregation and the GAT aggregation (up to 9 x 128 columns), forward and backward,
    against fp64"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_graph.py"), "40", "0"], cwd=root, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "failures: 0" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    assert len(re.findall(r"^ok +case \d+: gat ", r.stdout, re.M)) >= 8, r.stdout[-2000:]
