#!/usr/bin/env python3
"""What a layer's symbolic fit costs: `ops.symbolic_fit` (csrc/symbolic.hip) on the edge functions of one KANLinear -- by default
N 1024 rows, 64 -> 64, all 19 functions, grid_number 101, 3 iterations -- beside the same search written in torch ops (the
`[N, Gn, Gn]` tensor per edge and function that the kernels never build) for ONE function on a 4 x 4 layer, scaled up by the number of
edges and functions.

    python tools/symbolic_fit_step.py [--rows 1024] [--width 64] [--grid-number 101] [--iterations 3] [--functions sin,x^2]
                                      [--repeats 3] [--no-torch] [--iterations-split] [--json out.json]

Timing: host wall clock around one synchronised call, `--repeats` calls after one warm-up call; median and range.  `--iterations-split`
also times `iterations=1` (preparation + the shared MFMA pass + the read-out), whose difference to the full call is the zoom pass; the
per-kernel split itself comes from `rocprofv3 --kernel-trace --stats -- python tools/symbolic_fit_step.py --no-torch --repeats 1` in a
run of its own.  The shared pass's multiply-adds are 2 * Gn^2 * N * in * out * F flop; its share of the fp32-MFMA rate is printed from
the `iterations=1` time (an upper bound on the pass's own time, so a lower bound on the rate)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kagnn_amd                                   # noqa: E402
from kagnn_amd import ops                          # noqa: E402
from kagnn_amd.symbolic import SYMBOLIC_LIB        # noqa: E402

MFMA_FP32_TFLOPS = 157.3                           # v_mfma_f32_32x32x2_f32 peak of the MI355X


def torch_search(x, phi, name, gn, iterations, a_range=(-10.0, 10.0), b_range=(-10.0, 10.0)):
    """the same search in torch ops, edge by edge: the [N, Gn, Gn] tensor of u, two-pass sums, arg-max, per-axis zoom"""
    fn = SYMBOLIC_LIB[name][1]
    n, fout, fin = phi.shape
    best = torch.zeros(fout, fin, device=x.device)
    for o in range(fout):
        for i in range(fin):
            y = phi[:, o, i]
            dy = y - y.mean()
            syy = (dy * dy).sum()
            ra, rb = a_range, b_range
            for _ in range(iterations):
                a = torch.linspace(ra[0], ra[1], gn, device=x.device, dtype=torch.float64).float()
                b = torch.linspace(rb[0], rb[1], gn, device=x.device, dtype=torch.float64).float()
                u = fn(a[None, :, None] * x[:, i, None, None] + b[None, None, :])          # [N, Gn, Gn]
                du = u - u.mean(0, keepdim=True)
                suu, suy = (du * du).sum(0), (du * dy[:, None, None]).sum(0)
                bad = ~torch.isfinite(u).all(0) | (suu / n <= torch.clamp(1e-5 * (u * u).mean(0), min=1e-24))
                r2 = torch.nan_to_num(torch.where(bad, torch.zeros((), device=x.device), suy * suy / (suu * syy)), nan=0.0, posinf=0.0)
                w = int(r2.reshape(-1).argmax())
                ka, kb = w // gn, w % gn
                edge = lambda v, k: (float(v[max(k - 1, 0) if k < gn - 1 else gn - 2]), float(v[min(k + 1, gn - 1) if k > 0 else 1]))
                ra, rb = edge(a, ka), edge(b, kb)
            best[o, i] = r2.reshape(-1)[w]
    return best


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def stats(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--grid-number", type=int, default=101)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--functions", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--iterations-split", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev, w, gn, its = "cuda:0", args.width, args.grid_number, args.iterations
    names = tuple(SYMBOLIC_LIB) if args.functions is None else tuple(args.functions.split(","))
    torch.manual_seed(0)
    layer = kagnn_amd.KANLinear(w, w, grid_size=5, spline_order=3).to(dev)
    with torch.no_grad():
        layer.base_weight.copy_(0.3 * torch.randn(w, w))
        layer.spline_weight.copy_(0.3 * torch.randn(w, w, 8))
    x = 2 * torch.rand(args.rows, w, device=dev) - 1
    phi = layer.edge_curves(x)
    out = {"device": torch.cuda.get_device_name(0), "library_version": kagnn_amd._lib.load().kagnn_version(), "rows": args.rows, "width": w,
           "functions": len(names), "grid_number": gn, "iterations": its}
    full = lambda: ops.symbolic_fit(x, phi, names, grid_number=gn, iterations=its)
    fit, _ = timed(full)
    out["symbolic_fit_ms"] = stats([timed(full)[1] for _ in range(args.repeats)])
    out["edges_with_r2_above_0.99"] = int((fit.r2.max(0).values > 0.99).sum())
    if args.iterations_split:
        first = lambda: ops.symbolic_fit(x, phi, names, grid_number=gn, iterations=1)
        timed(first)
        out["iterations_1_ms"] = stats([timed(first)[1] for _ in range(args.repeats)])
        flop = 2.0 * gn * gn * args.rows * w * w * len(names)
        out["shared_pass_flop"] = flop
        out["shared_pass_tflops_lower_bound"] = flop / (out["iterations_1_ms"]["median"] * 1e-3) / 1e12
        out["shared_pass_share_of_mfma_fp32_peak"] = out["shared_pass_tflops_lower_bound"] / MFMA_FP32_TFLOPS
    if not args.no_torch:
        small = kagnn_amd.KANLinear(4, 4, grid_size=5, spline_order=3).to(dev)
        xs = x[:, :4].contiguous()
        ps = small.edge_curves(xs)
        one = names[len(names) // 2]
        composed = lambda: torch_search(xs, ps, one, gn, its)
        got, _ = timed(composed)
        ts = [timed(composed)[1] for _ in range(args.repeats)]
        ref = ops.symbolic_fit(xs, ps, (one,), grid_number=gn, iterations=its).r2[0]
        out["torch_ops_4x4_one_function_ms"] = stats(ts)
        out["torch_ops_function"] = one
        out["torch_ops_max_r2_difference"] = float((got - ref).abs().max())
        out["torch_ops_scaled_to_this_layer_s"] = statistics.median(ts) * 1e-3 * (w * w / 16.0) * len(names)
        out["speedup_over_torch_ops"] = out["torch_ops_scaled_to_this_layer_s"] / (out["symbolic_fit_ms"]["median"] * 1e-3)
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
