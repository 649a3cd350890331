#!/usr/bin/env python3
"""What the attribution statistics cost: `KANLinear.edge_stats` (`ops.kan_edge_moments`, csrc/kan_edge.hip: mean and centred sum of
squares of every edge function) beside `KANLinear.edge_l1` (`ops.kan_edge_abs_sum`: the same expansion with one accumulator per
output instead of two) at a KAN-GNN layer's shape (64 -> 64, grid 5, order 3, N = 2^20 rows), and a whole `KAN.prune` of a small
chain for scale.

    python tools/prune_step.py [--rows 1048576] [--width 64] [--grid 5] [--order 3] [--json out.json]

Timing: device events around a window of back-to-back calls, each window at least `--window` seconds (0.2) long, five windows per
variant, the variants ALTERNATING window by window in one process; reported per variant: median and range (min .. max) of the
per-call time.  The moments are first compared with a two-pass fp64 evaluation on a strided subset of the rows (2e-5 of the
maximum)."""
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
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--grid", type=int, default=5)
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prune_step.py measures on the GPU: no device found")
    dev = "cuda:0"
    torch.manual_seed(0)
    layer = kagnn_amd.KANLinear(args.width, args.width, grid_size=args.grid, spline_order=args.order).to(dev)
    with torch.no_grad():
        layer.base_weight.normal_(0, 0.3); layer.spline_weight.normal_(0, 0.3); layer.spline_scaler.normal_(1, 0.5)
    x = 0.8 * torch.randn(args.rows, args.width, device=dev)

    sub = x[::max(1, args.rows // 4096)]
    phi = layer.edge_curves(sub).double()
    got = layer.edge_stats(sub, unbiased=False)
    err_mean = float((got.mean - phi.mean(0)).abs().max() / phi.mean(0).abs().max())
    err_std = float((got.std - phi.std(0, unbiased=False)).abs().max() / phi.std(0, unbiased=False).max())
    if not max(err_mean, err_std) <= 2e-5:
        raise SystemExit(f"edge_stats and the two-pass evaluation disagree: mean {err_mean:.3e}, std {err_std:.3e} of the maximum")

    def edge_l1():
        with torch.no_grad():
            layer.edge_l1(x)

    variants = {"edge_l1": edge_l1, "edge_stats": lambda: layer.edge_stats(x)}
    for fn in variants.values():        # warm-up: code objects, workspaces
        fn(); fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.windows):
        for name, fn in variants.items():
            times[name].append(window(fn, args.window))

    chain = kagnn_amd.KAN([args.width, args.width, args.width], grid_size=args.grid, spline_order=args.order).to(dev)
    rows = x[:1 << 16]
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    keep, edges = chain.prune(rows)
    b.record()
    b.synchronize()

    out = {"device": torch.cuda.get_device_name(0), "library_version": kagnn_amd._lib.load().kagnn_version(),
           "rows": args.rows, "width": args.width, "grid": args.grid, "order": args.order, "window_s": args.window,
           "windows": args.windows, "mean_max_rel": err_mean, "std_max_rel": err_std,
           "ms": {name: {"median": statistics.median(t), "min": min(t), "max": max(t)} for name, t in times.items()},
           "chain_prune": {"rows": rows.size(0), "ms_first_call": a.elapsed_time(b), "kept": [int(k.numel()) for k in keep],
                           "edges_off": [int(e.size(0)) for e in edges]}}
    out["edge_stats_over_edge_l1"] = out["ms"]["edge_stats"]["median"] / out["ms"]["edge_l1"]["median"]
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
