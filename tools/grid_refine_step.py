#!/usr/bin/env python3
"""What a grid refinement costs: `ops.kan_grid_resize` (csrc/kan_grid.hip) at a KAN-GNN layer's shape (64 -> 64, order 3, N = 2^20 rows)
for 5 -> 10 and 8 -> 40, beside the same normal equations composed from the package's other calls (`composed_resize`): dense bases
from `ops.kan_bsplines` 8192 rows at a time, fp64 `einsum` Gram matrices on the device, a minimum-norm `lstsq` on the host -- run
on the same inputs with the two grid sizes.

    python tools/grid_refine_step.py [--rows 1048576] [--width 64] [--order 3] [--pairs 5:10,8:40] [--json out.json]

Timing: host wall clock around one synchronised call (the composed route ends in a host solve, so device events would not see all
of it), `--repeats` (5) calls per variant after one warm-up call each, the variants alternating; reported per variant: median and
range.  Both routes fit the unscaled coefficients on uniform rows in [-0.99, 0.99] (every row inside the range: the window changes
nothing) and are compared first, at 5e-5 of the maximum."""
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


def composed_resize(x, grid_old, grid_new, sw, g0, g1, k, chunk=8192):
    """the comparison route: [chunk, in, C] dense bases, fp64 einsum Gram matrices, host solve"""
    fin = x.size(1)
    a = torch.zeros((fin, g1 + k, g1 + k), dtype=torch.float64, device=x.device)
    b = torch.zeros((fin, g1 + k, g0 + k), dtype=torch.float64, device=x.device)
    for r0 in range(0, x.size(0), chunk):
        rows = x[r0:r0 + chunk].contiguous()
        a_new = ops.kan_bsplines(rows, grid_new, g1, k).double()
        a_old = ops.kan_bsplines(rows, grid_old, g0, k).double()
        a += torch.einsum("nfc,nfd->fcd", a_new, a_new)
        b += torch.einsum("nfc,nfd->fcd", a_new, a_old)
    rhs = torch.einsum("fcd,ofd->fco", b, sw.double())
    sol = torch.linalg.lstsq(a.cpu(), rhs.cpu(), driver="gelsd").solution
    return sol.permute(2, 0, 1).to(dtype=torch.float32, device=x.device).contiguous()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--pairs", default="5:10,8:40")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev, k, w = "cuda:0", args.order, args.width
    torch.manual_seed(0)
    x = torch.rand(args.rows, w, device=dev) * 1.98 - 0.99
    out = {"device": torch.cuda.get_device_name(0), "library_version": kagnn_amd._lib.load().kagnn_version(), "rows": args.rows, "width": w,
           "order": k, "pairs": []}
    for pair in args.pairs.split(","):
        g0, g1 = (int(v) for v in pair.split(":"))
        old = kagnn_amd.KANLinear(w, w, grid_size=g0, spline_order=k).to(dev)
        grid_new = kagnn_amd.KANLinear(w, w, grid_size=g1, spline_order=k).grid.to(dev)
        sw = 0.3 * torch.randn(w, w, g0 + k, device=dev)
        window = torch.stack([grid_new[:, k], grid_new[:, -k - 1]], dim=1).contiguous()
        fused = lambda: ops.kan_grid_resize(x, old.grid, grid_new, sw, None, g0, g1, k, window)[0]
        composed = lambda: composed_resize(x, old.grid, grid_new, sw, g0, g1, k)
        (got, _), (want, _) = timed(fused), timed(composed)                 # warm-up and parity
        err = float((got - want).abs().max() / want.abs().max())
        assert err <= 5e-5, err
        times = {"kan_grid_resize": [], "composed": []}
        for _ in range(args.repeats):
            times["kan_grid_resize"].append(timed(fused)[1])
            times["composed"].append(timed(composed)[1])
        entry = {"grid_size": [g0, g1], "coefficients": g1 + k, "max_difference_over_max": err}
        for name, t in times.items():
            entry[name + "_ms"] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
        entry["speedup"] = entry["composed_ms"]["median"] / entry["kan_grid_resize_ms"]["median"]
        out["pairs"].append(entry)
        print(json.dumps(entry))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
