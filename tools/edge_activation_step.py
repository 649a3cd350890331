#!/usr/bin/env python3
"""What the per-edge activation statistics cost: `ops.kan_edge_abs_sum` forward and backward (csrc/kan_edge.hip) at a KAN-GNN layer's
shape (64 -> 64, grid 5, order 3, N = 2^20 rows), beside the only way to get the same [out, in] matrix from the ops the package had
before: `ops.kan_bsplines` + `einsum` on the device, in row chunks small enough for the [rows, out, in] intermediate (forward only;
autograd through that composition would keep every chunk's intermediate alive).

    python tools/edge_activation_step.py [--rows 1048576] [--width 64] [--grid 5] [--order 3] [--chunk 16384] [--json out.json]
    python tools/edge_activation_step.py --fastkan [--rows 1048576] [--width 64] [--num-grids 8] [--json out.json]

`--fastkan`: the FastKAN twin (csrc/fastkan_edge.hip) on a `FastKANLayer(width, width, num_grids)` with its LayerNorm and base branch:
`edge_l1` and its backward (all five gradients) beside the same layer's own forward and backward, same rows, same process.

Timing: device events around a window of back-to-back calls, each window at least `--window` seconds (0.2) long, five windows per
variant, the variants ALTERNATING window by window in one process; reported per variant: median and range (min .. max) of the
per-call time.  The two forward variants are compared on the same seeded inputs first (2e-5 of the maximum).  The algorithmic
operation count of the fused forward is N * in * out * (2 (k + 2) + 1) flop; that of the backward twice that plus the dense
C + 1 wide products of the parameter kernel."""
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


def composed_abs_sum(x, layer, chunk):
    """sum_n |phi| from the dense bases: [chunk, in, C] bases, [chunk, out, in] activations per chunk"""
    w = layer.scaled_spline_weight.detach()
    bw = layer.base_weight.detach()
    total = torch.zeros_like(bw)
    for r0 in range(0, x.size(0), chunk):
        rows = x[r0:r0 + chunk]
        bases = ops.kan_bsplines(rows, layer.grid, layer.grid_size, layer.spline_order)
        phi = torch.einsum("nic,oic->noi", bases, w)
        phi.addcmul_(torch.nn.functional.silu(rows).unsqueeze(1), bw.unsqueeze(0))
        total += phi.abs_().sum(0)
    return total


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


def main_fastkan(args):
    dev = "cuda:0"
    torch.manual_seed(0)
    layer = kagnn_amd.FastKANLayer(args.width, args.width, num_grids=args.num_grids).to(dev)
    with torch.no_grad():
        layer.spline_linear.weight.normal_(0, 0.3); layer.base_linear.weight.normal_(0, 0.3)
        layer.layernorm.weight.normal_(1, 0.3); layer.layernorm.bias.normal_(0, 0.2)
    x = (0.8 * torch.randn(args.rows, args.width, device=dev)).requires_grad_(True)
    gS = torch.randn(args.width, args.width, device=dev)
    gy = torch.randn(args.rows, args.width, device=dev)

    def layer_step():
        layer(x).backward(gy)

    def edge_step():
        layer.edge_l1(x).backward(gS)

    def edge_forward():
        with torch.no_grad():
            layer.edge_l1(x)

    def layer_forward():
        with torch.no_grad():
            layer(x)

    variants = {"layer_forward": layer_forward, "layer_forward_backward": layer_step, "edge_l1_forward": edge_forward,
                "edge_l1_forward_backward": edge_step}
    for fn in variants.values():
        fn(); fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.windows):
        for name, fn in variants.items():
            times[name].append(window(fn, args.window))
    out = {"device": torch.cuda.get_device_name(0), "library_version": kagnn_amd._lib.load().kagnn_version(), "layer": "FastKANLayer",
           "rows": args.rows, "width": args.width, "num_grids": args.num_grids, "window_s": args.window, "windows": args.windows,
           "ms": {name: {"median": statistics.median(t), "min": min(t), "max": max(t)} for name, t in times.items()}}
    out["edge_over_layer_forward_backward"] = out["ms"]["edge_l1_forward_backward"]["median"] / out["ms"]["layer_forward_backward"]["median"]
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fastkan", action="store_true")
    ap.add_argument("--num-grids", type=int, default=8)
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--grid", type=int, default=5)
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=16384)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edge_activation_step.py measures on the GPU: no device found")
    if args.fastkan:
        return main_fastkan(args)
    dev = "cuda:0"
    torch.manual_seed(0)
    layer = kagnn_amd.KANLinear(args.width, args.width, grid_size=args.grid, spline_order=args.order).to(dev)
    with torch.no_grad():
        layer.base_weight.normal_(0, 0.3); layer.spline_weight.normal_(0, 0.3); layer.spline_scaler.normal_(1, 0.5)
    x = 0.8 * torch.randn(args.rows, args.width, device=dev)
    gS = torch.randn(args.width, args.width, device=dev)
    bw, sw, sc = layer.base_weight.detach(), layer.spline_weight.detach(), layer.spline_scaler.detach()
    kn, pf = layer._knots(), 0
    dims = (pf, args.width, args.width, args.grid, args.order)

    fused = ops._kan_edge_abs_sum_raw(x, bw, sw, sc, kn, *dims)
    composed = composed_abs_sum(x, layer, args.chunk)
    err = float((fused - composed).abs().max() / composed.abs().max())
    if not err <= 2e-5:
        raise SystemExit(f"the fused abs sum and the composition disagree: {err:.3e} of the maximum")

    variants = {
        "fused_forward": lambda: ops._kan_edge_abs_sum_raw(x, bw, sw, sc, kn, *dims),
        "fused_backward_params": lambda: ops._kan_edge_abs_sum_bwd_raw(x, bw, sw, sc, kn, *dims, gS, True, True, True, False),
        "fused_backward_input": lambda: ops._kan_edge_abs_sum_bwd_raw(x, bw, sw, sc, kn, *dims, gS, False, False, False, True),
        "fused_backward": lambda: ops._kan_edge_abs_sum_bwd_raw(x, bw, sw, sc, kn, *dims, gS, True, True, True, True),
        "composed_forward": lambda: composed_abs_sum(x, layer, args.chunk),
    }
    for fn in variants.values():        # warm-up: code objects, workspaces of every shape
        fn(); fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.windows):
        for name, fn in variants.items():
            times[name].append(window(fn, args.window))
    pairs = args.rows * args.width * args.width
    flop_fwd = pairs * (2 * (args.order + 2) + 1)
    out = {"device": torch.cuda.get_device_name(0), "library_version": kagnn_amd._lib.load().kagnn_version(),
           "rows": args.rows, "width": args.width, "grid": args.grid, "order": args.order, "chunk": args.chunk,
           "window_s": args.window, "windows": args.windows, "fused_vs_composed_max_rel": err,
           "fused_forward_gflop": flop_fwd / 1e9, "ms": {}}
    for name, t in times.items():
        out["ms"][name] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
    out["composed_over_fused_forward"] = out["ms"]["composed_forward"]["median"] / out["ms"]["fused_forward"]["median"]
    out["fused_forward_tflops"] = flop_fwd / (out["ms"]["fused_forward"]["median"] * 1e-3) / 1e12
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
