#!/usr/bin/env python3
"""Forward + backward of `AttentionWithFastKANTransform` (five FastKANLayers around one `ops.dense_attention` call, csrc/attention.hip)
beside the same five layers with the core written in torch ops the way the reference writes it: the broadcast products
`[B, Q, K, H, c]` (twice) and the attention tensor `[B, Q, K, H]` materialised, autograd through them.

    python tools/attention_step.py [--batch 8] [--queries 1024] [--keys 1024] [--heads 8] [--head-dim 32] [--dim 64] [--no-bias]
                                   [--no-gate] [--json out.json]

Both variants share one module (the same parameters), the same seeded inputs and upstream gradient; their outputs and input
gradients are compared first (1e-4 of the maximum: the layers run in the default split mode on both sides).  Timing: device
events around a window of back-to-back steps, each window at least `--window` seconds (0.2) long, `--windows` (3) windows per variant,
the variants ALTERNATING window by window in one process; reported: median and range of the per-step time.  Memory: the rise of
`torch.cuda.max_memory_allocated` over one step above what is allocated before it (parameters and inputs).  When the torch-op side
does not fit, the batch is halved until it does and both sides run at that batch.  The core's operation count is
4 B Q K H c flop forward (two products; 6 with a bias: bias wv is a third) and 10 B Q K H c backward with the recomputed logits (14 with
a bias: D takes a pass of its own).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kagnn_amd                                   # noqa: E402
from kagnn_amd import ops                          # noqa: E402


def torch_core(wq, wk, wv, num_heads, scale, bias, gate):
    """the core as broadcast products in torch ops: everything of size Q x K is materialised and kept for the backward"""
    B, Q, _ = wq.shape
    K = wk.size(1)
    att = ((wq * scale).view(B, Q, 1, num_heads, -1) * wk.view(B, 1, K, num_heads, -1)).sum(-1).softmax(2)
    if bias is not None:
        att = att + bias.unsqueeze(-1)
    o = (att.unsqueeze(-1) * wv.view(B, 1, K, num_heads, -1)).sum(2).reshape(B, Q, -1)
    return o if gate is None else torch.sigmoid(gate) * o


def module_forward(m, q, k, v, bias, core):
    g = None if m.linear_g is None else m.linear_g(q)
    return m.linear_o(core(m.linear_q(q), m.linear_k(k), m.linear_v(v), m.num_heads, m.norm, bias, g))


def window(fn, min_seconds):
    """per-call milliseconds over one window of at least `min_seconds` of device time"""
    calls = 1
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= 1e3 * min_seconds:
            return ms / calls
        calls = max(calls + 1, int(calls * 1.2e3 * min_seconds / max(ms, 1e-3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--keys", type=int, default=1024)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--head-dim", type=int, default=32)
    ap.add_argument("--dim", type=int, default=64, help="q_dim = k_dim = v_dim")
    ap.add_argument("--no-bias", action="store_true")
    ap.add_argument("--no-gate", action="store_true")
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    m = kagnn_amd.AttentionWithFastKANTransform(args.dim, args.dim, args.dim, args.head_dim, args.heads, gating=not args.no_gate).to(dev)
    with torch.no_grad():                                     # logits of order 1 rather than the init scale's few hundredths
        m.linear_q.spline_linear.weight.mul_(6.0)
        m.linear_k.spline_linear.weight.mul_(6.0)
    Q, K, H, c = args.queries, args.keys, args.heads, args.head_dim
    B = args.batch
    while True:
        q = (0.8 * torch.randn(B, Q, args.dim, device=dev)).requires_grad_(True)
        k = (0.8 * torch.randn(B, K, args.dim, device=dev)).requires_grad_(True)
        v = (0.8 * torch.randn(B, K, args.dim, device=dev)).requires_grad_(True)
        bias = None if args.no_bias else (0.3 * torch.randn(B, Q, K, device=dev)).requires_grad_(True)
        gout = torch.randn(B, Q, args.dim, device=dev)
        leaves = [t for t in (q, k, v, bias) if t is not None]

        def step(core):
            for t in leaves:
                t.grad = None
            m.zero_grad(set_to_none=True)
            out = module_forward(m, q, k, v, bias, core)
            out.backward(gout)
            return out

        def measure_memory(core):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            out = step(core).detach()
            torch.cuda.synchronize()
            return out, [t.grad.clone() for t in leaves], torch.cuda.max_memory_allocated() - before

        fused_out, fused_grads, fused_mem = measure_memory(ops.dense_attention)
        assert torch.equal(fused_out, m(q, k, v, bias).detach())          # the module's own forward is this composition
        try:
            torch_out, torch_grads, torch_mem = measure_memory(torch_core)
            break
        except torch.OutOfMemoryError:
            if B == 1:
                raise
            del q, k, v, bias, gout, leaves
            B //= 2
            print(f"the torch-op side does not fit: batch -> {B}", flush=True)

    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    diffs = {"out": rel(fused_out, torch_out)}
    for name, a, b in zip(("g_q", "g_k", "g_v", "g_bias"), fused_grads, torch_grads):
        diffs[name] = rel(a, b)
    assert max(diffs.values()) < 1e-4, diffs

    times = {"fused": [], "torch_ops": []}
    for _ in range(args.windows):
        times["fused"].append(window(lambda: step(ops.dense_attention), args.window))
        times["torch_ops"].append(window(lambda: step(torch_core), args.window))
    flop = (20 if bias is not None else 14) * B * Q * K * H * c
    res = dict(shape=dict(B=B, Q=Q, K=K, H=H, c=c, dim=args.dim, bias=bias is not None, gate=not args.no_gate),
               device=torch.cuda.get_device_name(0), library_version=kagnn_amd._lib.load().kagnn_version(),
               agreement_relative_to_max=diffs, core_gflop_fwd_bwd=flop / 1e9, product_tensor_gb=B * Q * K * H * c * 4 / 1e9)
    for name, ts in times.items():
        res[name] = dict(step_ms_median=statistics.median(ts), step_ms_min=min(ts), step_ms_max=max(ts),
                         peak_memory_rise_mb=(fused_mem if name == "fused" else torch_mem) / 2 ** 20)
    res["fused"]["core_tflops_at_median"] = flop / res["fused"]["step_ms_median"] / 1e9
    print(json.dumps(res, indent=1))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
