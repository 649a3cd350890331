"""``ops.dense_attention`` (csrc/attention.hip) against the formula written in fp64 torch here, and
``AttentionWithFastKANTransform`` against the reference's own fp64 results (tests/golden/g15_attention.npz).

Kernel level.  o and the gradients of wq, wk, wv, bias and gate are held to ``helpers.assert_close``'s default bound (2e-5 of the
reference tensor's own maximum plus the 1e-4 element-wise rule) with no relaxation: the kernels are ordered fp32 fma chains.  The
one allowance the file knows is for g_wq / g_wk where ``dA - D`` cancels: ``max(fp32 bound, 4 x E32)`` with E32 the error of torch's
own fp32 CPU autograd of the same formula on the same inputs against fp64 (the README's rule for g_gamma / g_beta).  It is applied
only after the plain bound has failed and every use is printed (``-s``).  Observed on MI355X (library version 271): no case needed
it; worst fraction of the plain bound 0.66 (g_wq, rising logits without a bias: the gradient is a cancelling sum over keys of norm
~25), 0.21 with a bias, 0.09 at logits of +-50, at most 0.06 on the eight shapes (profiles/attention.md).  Module level: at most 0.07 of
the bound, and 0.12 / 0.18 / 0.50 of the noise floor for ``linear_k.base_linear.bias.grad``.

The bias enters AFTER the softmax, so ``D = sum_k p dA`` is not ``<d_o, o>``; ``test_shortcut_for_D_is_visible`` evaluates the
fp64 formulas with that shortcut and asserts that the biased cases reject the result.

Module level.  Output, parameter and input gradients at 1e-4 of each tensor's own maximum (the whole-model bound: the five FastKAN
layers run in the default split mode) or, where larger, twice the fixture's own fp32-vs-fp64 error.  The gradient of
``linear_k.base_linear.bias`` is identically zero (a constant added to every wk row shifts all logits of a query equally); it is held
to a noise floor of 4 x the magnitude of the fixture's fp32 value, which is pure rounding noise.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import kagnn_amd
from kagnn_amd import _lib, ops
from helpers import TOL, assert_close, must_fail

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.5

# (B, Q, K, H, c): one element; two blocks of nothing; ragged c, K past four tiles; c = 32 with Q, K one past a tile; c = 128 and
# B > 1; c = 64 with three query blocks and K past eight tiles; one query; one key
SHAPES = [(1, 1, 1, 1, 1), (2, 5, 7, 2, 4), (2, 31, 129, 3, 5), (1, 33, 65, 4, 32), (3, 64, 64, 1, 128), (1, 130, 257, 4, 64),
          (1, 1, 300, 2, 16), (1, 300, 1, 2, 16)]
NEEDED_E32 = []          # (what, 4 x E32 / plain bound) of every check that took the allowance


# ------------------------------------------------------------------------------------------------ the fp64 formula
def _operands(shape, seed=0, amp=0.8, kind="randn"):
    B, Q, K, H, c = shape
    g = torch.Generator().manual_seed(1000 * seed + B + 3 * Q + 7 * K + 11 * H + 13 * c)
    wq = torch.randn(B, Q, H * c, generator=g) * amp
    wk = torch.randn(B, K, H * c, generator=g) * amp
    if kind == "rising":      # logits that rise along k within every row: each chunk of 16 keys rescales the accumulator
        wq = wq.abs() + 0.1
        wk = (torch.arange(K).float().view(1, K, 1) + 1.0) * (12.0 / K) * (0.5 + torch.rand(B, 1, H * c, generator=g)) / amp
    return dict(wq=wq, wk=wk, wv=torch.randn(B, K, H * c, generator=g) * 0.8, bias=torch.randn(B, Q, K, generator=g) * 0.3,
                gate=torch.randn(B, Q, H * c, generator=g), gout=torch.randn(B, Q, H * c, generator=g))


def _formula(t, H, scale, bias, gate, dtype=torch.float64):
    """autograd of the formula of the issue in ``dtype`` on the CPU: (o, {gradients})"""
    names = ["wq", "wk", "wv"] + (["bias"] if bias else []) + (["gate"] if gate else [])
    x = {n: t[n].to(dtype).requires_grad_(True) for n in names}
    B, Q, hc = x["wq"].shape
    K = x["wk"].size(1)
    q4, k4, v4 = (x[n].view(B, -1, H, hc // H) for n in ("wq", "wk", "wv"))
    p = (torch.einsum("bqhc,bkhc->bqkh", q4, k4) * scale).softmax(2) if K else torch.zeros(B, Q, 0, H, dtype=dtype)
    a = p + x["bias"][..., None] if bias else p
    o = torch.einsum("bqkh,bkhc->bqhc", a, v4).reshape(B, Q, hc)
    if gate:
        o = torch.sigmoid(x["gate"]) * o
    o.backward(t["gout"].to(dtype))
    return o.detach(), {n: x[n].grad for n in names}


def _manual(t, H, scale, bias, gate, shortcut):
    """the backward formulas of the issue in fp64, with D from p itself or (``shortcut``) as <d_o, o>"""
    d = {n: v.double() for n, v in t.items()}
    B, Q, hc = d["wq"].shape
    c = hc // H
    q4, k4, v4 = (d[n].view(B, -1, H, c) for n in ("wq", "wk", "wv"))
    p = (torch.einsum("bqhc,bkhc->bqkh", q4, k4) * scale).softmax(2)
    a = p + d["bias"][..., None] if bias else p
    o = torch.einsum("bqkh,bkhc->bqhc", a, v4)
    sig = torch.sigmoid(d["gate"]).view(B, Q, H, c) if gate else 1.0
    d_o = d["gout"].view(B, Q, H, c) * sig
    dA = torch.einsum("bqhc,bkhc->bqkh", d_o, v4)
    D = (d_o * o).sum(-1) if shortcut else (p * dA).sum(2)
    dS = p * (dA - D[:, :, None, :])
    out = {"wq": scale * torch.einsum("bqkh,bkhc->bqhc", dS, k4).reshape(B, Q, hc),
           "wk": scale * torch.einsum("bqkh,bqhc->bkhc", dS, q4).reshape(B, -1, hc),
           "wv": torch.einsum("bqkh,bqhc->bkhc", a, d_o).reshape(B, -1, hc)}
    if bias:
        out["bias"] = dA.sum(-1)
    if gate:
        out["gate"] = (d["gout"].view(B, Q, H, c) * o * sig * (1 - sig)).reshape(B, Q, hc)
    return out


@functools.lru_cache(maxsize=None)
def _reference(shape, bias, gate, seed=0, amp=0.8, kind="randn"):
    t = _operands(shape, seed, amp, kind)
    o, grads = _formula(t, shape[3], shape[4] ** -0.5, bias, gate)
    return t, o, grads


def _device_run(t, H, scale, bias, gate, views=None):
    views = views or {}
    names = ["wq", "wk", "wv"] + (["bias"] if bias else []) + (["gate"] if gate else [])
    x = {n: (views[n] if n in views else t[n].to(DEV)).requires_grad_(True) for n in names}
    o = ops.dense_attention(x["wq"], x["wk"], x["wv"], H, scale, x.get("bias"), x.get("gate"))
    o.backward(t["gout"].to(DEV))
    return o.detach(), {n: x[n].grad for n in names}


def _check_grad(got, want, what, name, e32):
    """the plain bound; for g_wq / g_wk only, after it failed: max(fp32 bound, 4 x E32)"""
    try:
        return assert_close(got, want, what=what)
    except AssertionError:
        if name not in ("wq", "wk"):
            raise
    err32 = float((e32()[name].double() - want).abs().max())
    bound = TOL * float(want.abs().max())
    NEEDED_E32.append((what, 4 * err32 / bound))
    print(f"ALLOWANCE {what}: 4 x E32 = {4 * err32:.3e}, plain bound {bound:.3e}")
    return assert_close(got, want, what=what + " [4 x E32]", elementwise=False, noise=max(0.0, 4 * err32 - bound))


def _compare(shape, bias, gate, seed=0, amp=0.8, kind="randn", views=None, tag=""):
    t, o64, g64 = _reference(shape, bias, gate, seed, amp, kind)
    H, scale = shape[3], shape[4] ** -0.5
    o, g = _device_run(t, H, scale, bias, gate, views(t) if views else None)
    what = f"attention{tag} {shape} bias={bias} gate={gate}"
    worst = assert_close(o, o64, what=what + " o") / TOL
    e32 = functools.lru_cache(maxsize=None)(lambda: _formula(t, H, scale, bias, gate, torch.float32)[1])
    for n in g64:
        worst = max(worst, _check_grad(g[n], g64[n], f"{what} g_{n}", n, e32) / TOL)
    print(f"FRACTION {what}: worst fraction of the bound {worst:.3f}")
    return t, o, g, o64, g64


# ------------------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("gate", [False, True], ids=["nogate", "gate"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_matches_fp64(shape, bias, gate):
    t, o, g, o64, g64 = _compare(shape, bias, gate)
    if shape[2] == 1:           # one key: the softmax is the constant 1
        assert torch.count_nonzero(g["wq"]) == 0 and torch.count_nonzero(g["wk"]) == 0
        assert torch.count_nonzero(g64["wq"]) == 0 and torch.count_nonzero(g64["wk"]) == 0


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
def test_large_logits(bias):
    """operands of 3.5 randn at c = 64: logits reach about +-50, every row is close to one-hot"""
    shape = (2, 70, 150, 2, 64)
    t, _, _ = _reference(shape, bias, True, 3, 3.5)
    s = torch.einsum("bqhc,bkhc->bqkh", t["wq"].double().view(2, 70, 2, 64), t["wk"].double().view(2, 150, 2, 64)) * 64 ** -0.5
    assert float(s.max()) > 40 and float(s.min()) < -40, (float(s.min()), float(s.max()))
    _compare(shape, bias, True, 3, 3.5, tag=" large logits")


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
def test_rising_logits_rescale_every_chunk(bias):
    shape = (1, 40, 200, 2, 8)
    t, _, _ = _reference(shape, bias, False, 4, 0.8, "rising")
    s = torch.einsum("bqhc,bkhc->bqkh", t["wq"].double().view(1, 40, 2, 8), t["wk"].double().view(1, 200, 2, 8)) * 8 ** -0.5
    assert bool((s[:, :, 1:] > s[:, :, :-1]).all()), "the logits do not rise along k"
    assert float(s.max()) > 10
    _compare(shape, bias, False, 4, 0.8, "rising", tag=" rising logits")


def test_bias_with_batch_stride_zero():
    """an ``expand``ed bias is read in place (batch stride 0); autograd sums its dense gradient over the batch"""
    shape = (3, 33, 65, 2, 8)
    t = dict(_operands(shape, 5))
    t["bias"] = t["bias"][:1].expand(3, 33, 65)
    o64, g64 = _formula(t, 2, 8 ** -0.5, True, True)
    leaf = t["bias"][:1].clone().to(DEV).requires_grad_(True)
    view = leaf.expand(3, 33, 65)
    assert view.stride(0) == 0
    x = {n: t[n].to(DEV).requires_grad_(True) for n in ("wq", "wk", "wv", "gate")}
    o = ops.dense_attention(x["wq"], x["wk"], x["wv"], 2, 8 ** -0.5, view, x["gate"])
    o.backward(t["gout"].to(DEV))
    assert_close(o, o64, what="stride-0 bias o")
    for n in x:
        assert_close(x[n].grad, g64[n], what=f"stride-0 bias g_{n}")
    assert_close(leaf.grad, g64["bias"].sum(0, keepdim=True), what="stride-0 bias g_bias")


def test_operands_as_column_slices():
    """wq, wk, wv, gate as column slices of wider matrices (row stride > H * c, one column in: off a 16-byte boundary), passed
    without a copy"""
    def views(t):
        out = {}
        for n in ("wq", "wk", "wv", "gate"):
            wide = torch.full((t[n].size(0), t[n].size(1), t[n].size(2) + 7), 7.0, device=DEV)
            wide[:, :, 1:1 + t[n].size(2)] = t[n].to(DEV)
            out[n] = wide[:, :, 1:1 + t[n].size(2)].detach()
            assert ops._att_rows(out[n], n)[0].data_ptr() == out[n].data_ptr()           # no copy
        return out
    for shape in ((2, 33, 65, 2, 8), (2, 31, 40, 3, 5)):
        _compare(shape, True, True, 6, views=views, tag=" column slices")
    # an aligned slice of a wider matrix (16-byte loads, row stride 4 more than the width)
    def aligned(t):
        out = {}
        for n in ("wq", "wk", "wv", "gate"):
            wide = torch.full((t[n].size(0), t[n].size(1), t[n].size(2) + 4), 7.0, device=DEV)
            wide[:, :, 4:] = t[n].to(DEV)
            out[n] = wide[:, :, 4:].detach()
        return out
    _compare((2, 33, 65, 2, 8), True, True, 6, views=aligned, tag=" aligned column slices")


def test_o_into_a_wider_buffer_leaves_the_padding():
    B, Q, K, H, c = 2, 33, 65, 3, 5
    t = _operands((B, Q, K, H, c), 7)
    hc = H * c
    d = {n: t[n].to(DEV).contiguous() for n in ("wq", "wk", "wv", "bias", "gate")}
    ld = hc + 6
    buf = torch.full((B * Q + 2, ld), SENTINEL, device=DEV)
    ou = torch.full((B * Q + 2, ld), SENTINEL, device=DEV)
    stats = torch.empty(2, B, Q, H, device=DEV)
    o_view, ou_view = buf[1:1 + B * Q, 3:3 + hc], ou[1:1 + B * Q, 3:3 + hc]
    P = lambda x: ctypes.c_void_p(x.data_ptr())
    _lib.call("kagnn_attention_fwd", P(d["wq"]), hc, P(d["wk"]), hc, P(d["wv"]), hc, P(d["bias"]), Q * K, K, P(d["gate"]), hc, B, Q, K, H, c,
              c ** -0.5, P(o_view), ld, P(ou_view), ld, P(stats), None)
    torch.cuda.synchronize()
    want = ops.dense_attention(d["wq"], d["wk"], d["wv"], H, c ** -0.5, d["bias"], d["gate"])
    assert torch.equal(o_view.reshape(B, Q, hc), want)
    o64, _ = _formula(t, H, c ** -0.5, True, True)
    assert_close(o_view.reshape(B, Q, hc), o64, what="o in a wider buffer")
    assert_close(ou_view.reshape(B, Q, hc) * torch.sigmoid(d["gate"]), o64, what="ungated o in a wider buffer")
    for b_ in (buf, ou):
        pad = torch.ones_like(b_, dtype=torch.bool)
        pad[1:1 + B * Q, 3:3 + hc] = False
        assert bool((b_[pad] == SENTINEL).all()), "the kernel wrote outside [rows, H * c]"
    # the statistics: the row maximum of the logits and the log of the sum
    s = torch.einsum("bqhc,bkhc->bqkh", t["wq"].double().view(B, Q, H, c), t["wk"].double().view(B, K, H, c)) * c ** -0.5
    assert_close(stats[0], s.amax(2), what="stats: maximum")
    assert_close(stats[0] + stats[1], torch.logsumexp(s, 2), what="stats: maximum + log-sum")


def test_second_call_gives_the_same_bits():
    for shape, bias, gate in (((2, 130, 257, 2, 16), True, True), ((2, 31, 129, 3, 5), False, False)):
        t, _, _ = _reference(shape, bias, gate, 8)
        runs = [_device_run(t, shape[3], shape[4] ** -0.5, bias, gate) for _ in range(2)]
        assert torch.equal(runs[0][0], runs[1][0])
        assert set(runs[0][1]) == {"wq", "wk", "wv"} | ({"bias"} if bias else set()) | ({"gate"} if gate else set())
        for n in runs[0][1]:
            assert torch.equal(runs[0][1][n], runs[1][1][n]), n


@pytest.mark.parametrize("shape", [(0, 5, 7, 2, 4), (2, 0, 7, 2, 4), (2, 5, 0, 2, 4)], ids=["B0", "Q0", "K0"])
def test_empty_dimensions(shape):
    B, Q, K, H, c = shape
    t = _operands(shape, 9)
    o, g = _device_run(t, H, c ** -0.5, True, True)
    torch.cuda.synchronize()
    assert o.shape == (B, Q, H * c) and torch.count_nonzero(o) == 0           # K == 0: an empty sum
    for n, r in (("wq", Q), ("wk", K), ("wv", K), ("gate", Q)):
        assert g[n].shape == (B, r, H * c) and torch.count_nonzero(g[n]) == 0, n
    assert g["bias"].shape == (B, Q, K)


def test_nan_rows_poison_what_they_reach_and_nothing_else():
    shape = (3, 40, 70, 2, 8)
    t = dict(_operands(shape, 10))
    clean, _ = _device_run(t, 2, 8 ** -0.5, True, True)
    bad = dict(t)
    bad["wq"] = t["wq"].clone()
    bad["wq"][1, 17] = float("nan")
    o, _ = _device_run(bad, 2, 8 ** -0.5, True, True)
    nan_rows = torch.isnan(o).any(-1)
    assert bool(torch.isnan(o[1, 17]).all()) and int(nan_rows.sum()) == 1
    assert torch.equal(o[~nan_rows], clean[~nan_rows])
    bad = dict(t)
    bad["wk"] = t["wk"].clone()
    bad["wk"][2, 33] = float("nan")
    o, _ = _device_run(bad, 2, 8 ** -0.5, True, True)
    assert bool(torch.isnan(o[2]).all())
    assert torch.equal(o[:2], clean[:2])


def test_mutants_are_rejected():
    shape = (2, 31, 129, 3, 5)
    t, o, g, o64, g64 = _compare(shape, True, True)
    moved = o.clone()
    moved[1, 7] += 1e-3 * float(o64.abs().max())
    must_fail(moved, o64, what="o with one row moved by 1e-3")
    must_fail(torch.zeros_like(g["bias"]), g64["bias"], what="zeroed g_bias")


@pytest.mark.parametrize("gate", [False, True], ids=["nogate", "gate"])
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[2] > 1], ids=lambda s: "x".join(map(str, s)))
def test_shortcut_for_D_is_visible(shape, gate):
    """the fp64 formulas with D = <d_o, o> must FAIL the bound of the biased cases (and the formulas with D from p must equal autograd)"""
    t, _, g64 = _reference(shape, True, gate)
    right = _manual(t, shape[3], shape[4] ** -0.5, True, gate, shortcut=False)
    for n in g64:
        assert float((right[n] - g64[n]).abs().max()) <= 1e-12 * max(1.0, float(g64[n].abs().max())), n
    wrong = _manual(t, shape[3], shape[4] ** -0.5, True, gate, shortcut=True)
    must_fail(wrong["wq"], g64["wq"], what=f"shortcut D g_wq {shape}")
    must_fail(wrong["wk"], g64["wk"], what=f"shortcut D g_wk {shape}")
    # without a bias the shortcut is exact
    t, _, g64 = _reference(shape, False, gate)
    same = _manual(t, shape[3], shape[4] ** -0.5, False, gate, shortcut=True)
    for n in ("wq", "wk"):
        assert float((same[n] - g64[n]).abs().max()) <= 1e-12 * max(1.0, float(g64[n].abs().max())), n


def test_nothing_of_size_QK_is_allocated():
    B, Q, K, H, c = 1, 2048, 2048, 8, 16
    g = torch.Generator().manual_seed(11)
    x = [(torch.randn(B, r, H * c, generator=g) * 0.8).to(DEV).requires_grad_(True) for r in (Q, K, K)]
    gout = torch.randn(B, Q, H * c, generator=g).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    o = ops.dense_attention(x[0], x[1], x[2], H, c ** -0.5)
    o.backward(gout)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    assert rise < Q * K * H * 4 // 2, f"forward + backward raised the peak by {rise / 2 ** 20:.1f} MiB"
    # spot check of the big shape against fp64 on one head's first rows
    q4, k4, v4 = (t.detach().double().cpu().view(r, H, c) for t, r in zip(x, (Q, K, K)))
    p = (torch.einsum("qc,kc->qk", q4[:64, 3], k4[:, 3]) * c ** -0.5).softmax(1)
    assert_close(o[0, :64, 3 * c:4 * c], p @ v4[:, 3], what="o at 2048 x 2048")


# ------------------------------------------------------------------------------------------------ module level
@functools.lru_cache(maxsize=None)
def _golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "g15_attention.npz"))
    return z, json.loads(str(z["meta"]))


def _module(case, z):
    m = kagnn_amd.AttentionWithFastKANTransform(*case["dims"], gating=case["gating"])
    m.load_state_dict({n: torch.from_numpy(z[f"{case['name']}/state/{n}"]) for n in case["state_keys"]})
    return m.to(DEV)


def _module_run(m, case, z):
    ins = {n: torch.from_numpy(z[f"{case['name']}/{n}"]).to(DEV).requires_grad_(True) for n in ("q", "k", "v", "bias")
           if f"{case['name']}/{n}" in z.files}
    for p in m.parameters():
        p.grad = None
    out = m(ins["q"], ins["k"], ins["v"], ins.get("bias"))
    out.backward(torch.from_numpy(z[f"{case['name']}/gout"]).to(DEV))
    grads = {"in." + n: t.grad for n, t in ins.items()}
    grads.update({n: p.grad for n, p in m.named_parameters() if p.requires_grad})
    return out.detach(), grads, ins


@pytest.mark.parametrize("index", [0, 1, 2], ids=["c0", "c1", "c2"])
def test_module_matches_the_reference_fp64(index):
    z, meta = _golden()
    case = meta["cases"][index]
    name = case["name"]
    m = _module(case, z)
    out, grads, _ = _module_run(m, case, z)

    def hold(got, key32, key64, what, floor=0.0):
        w32, w64 = torch.from_numpy(z[key32]).double(), torch.from_numpy(z[key64])
        own = float(w64.abs().max())
        ref_err = float((w32 - w64).abs().max())            # the reference's own fp32 against its fp64
        bound = max(1e-4 * own, 2 * ref_err, floor)
        err = float((got.detach().double().cpu() - w64).abs().max())
        print(f"MODULE {what}: err {err:.3e}, bound {bound:.3e} (1e-4 x {own:.3g}; 2 x fp32-vs-fp64 {2 * ref_err:.3e}), fraction {err / bound:.3f}")
        assert_close(got, w64, tol=1e-4, what=what, elementwise=False, noise=bound - 1e-4 * own)

    hold(out, f"{name}/out32", f"{name}/out64", f"module {name} out")
    assert sorted(grads) == sorted(case["grad_keys"])
    for n in case["grad_keys"]:
        floor = 0.0
        if n == "linear_k.base_linear.bias":               # identically zero in exact arithmetic: pure rounding noise in fp32
            assert float(np.abs(z[f"{name}/g64/{n}"]).max()) < 1e-12
            floor = 4 * float(np.abs(z[f"{name}/g32/{n}"]).max())
        hold(grads[n], f"{name}/g32/{n}", f"{name}/g64/{n}", f"module {name} g[{n}]", floor)


def test_module_composition_precision_and_collection():
    z, meta = _golden()
    case = meta["cases"][0]                                 # gating and a bias, no leading dimension
    m = _module(case, z)
    out, grads, ins = _module_run(m, case, z)
    q, k, v, bias = (ins[n].detach() for n in ("q", "k", "v", "bias"))
    with torch.no_grad():
        # by hand: the five layers around one ops.dense_attention call, bit for bit
        o = ops.dense_attention(m.linear_q(q)[None], m.linear_k(k)[None], m.linear_v(v)[None], m.num_heads, m.norm, bias[None],
                                m.linear_g(q)[None])
        assert torch.equal(m.linear_o(o[0]), out)
        # exact fp32 on the five layers: within 2e-5 of the default (split) mode
        for layer in (m.linear_q, m.linear_k, m.linear_v, m.linear_o, m.linear_g):
            layer.precision = ops.PREC_FP32
        exact = m(q, k, v, bias)
        for layer in (m.linear_q, m.linear_k, m.linear_v, m.linear_o, m.linear_g):
            layer.precision = None
        assert_close(out, exact, tol=2e-5, what="module: split against fp32 layers", elementwise=False)
        with kagnn_amd.collect_edge_l1(m) as stats:
            again = m(q, k, v, bias)
        assert torch.equal(again, out)
        assert sorted(stats) == ["linear_g", "linear_k", "linear_o", "linear_q", "linear_v"]
        for n, s in stats.items():
            layer = getattr(m, n)
            assert s.shape == (layer.output_dim, layer.input_dim) and bool((s >= 0).all()) and float(s.sum()) > 0
