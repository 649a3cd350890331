#!/usr/bin/env python3
"""What fixed symbolic edges cost: forward + backward of `ops.symbolic_edges` (csrc/symbolic_edges.hip) and of a KANLinear with fixed
edges -- by default N = 1M rows at 64 -> 64 with 1 %, 10 % and 100 % of the edges fixed (random pairs, the 19 functions in turn) --
beside a torch-ops composition of the same formula: one masked dense `[rows, out, in]` evaluation per function present,

    t = A * x[:, None, :] + B,    y = sum_f where(mask_f, C * f(where(mask_f, t, 2.5)) + D, 0).sum(-1),

A, B, C, D dense [out, in], scattered from affine [E, 4] (f sees 2.5, an argument inside every function's domain, wherever the
edge is not its own: neither the values nor the gradients pick up a NaN from another function's edge).  At 1M rows one such tensor is 16 GiB and
autograd keeps several per function, so the composition walks the rows in chunks of `--torch-chunk` (default 32768) and adds the
parameter gradients; the kernel route takes all rows in one call.

    python tools/symbolic_edges_step.py [--rows 1000000] [--width 64] [--densities 0.01,0.1,1.0] [--repeats 3] [--torch-chunk 32768]
                                        [--no-torch] [--no-kinks] [--json out.json]

`max_rel_diff_to_torch` (y, gx, g_affine; each relative to the tensor's maximum) compares two fp32 evaluations.  The kernels form the
argument as `fmaf(a, x, b)`, torch as a product and a sum, so for a few of the ~1e8 arguments of `sgn` / `abs` edges at full density
the two land on different sides of 0 and one term of y moves by `2c`: `--no-kinks` puts `sin` / `cos` in their place and shows the
agreement without those flips.

Timing: host wall clock around one synchronised forward + backward, `--repeats` runs after one warm-up run; the median.  Memory:
the allocator's peak above what was allocated before the run (inputs and parameters excluded)."""
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

POSITIVE = (4, 5, 6, 7, 9)                         # 1/x, 1/x^2, sqrt, 1/sqrt(x), log: a in [0.3, 1], b in [2, 3]


def make_edges(width, density, gen, kinks=True):
    e = max(1, int(round(density * width * width)))
    pairs = sorted(torch.randperm(width * width, generator=gen)[:e].tolist())
    triples = [(p // width, p % width, k % 19) for k, p in enumerate(pairs)]
    if not kinks:                                  # abs -> sin, sgn -> cos
        triples = [(o, i, {10: 11, 15: 12}.get(f, f)) for o, i, f in triples]
    aff = torch.empty(e, 4)
    for k, (_, _, f) in enumerate(triples):
        u = torch.rand(4, generator=gen)
        if f in POSITIVE:
            aff[k] = torch.stack([0.3 + 0.7 * u[0], 2.0 + u[1], 0.3 + u[2], u[3] - 0.5])
        elif f == 13:                              # tan
            aff[k] = torch.stack([0.3 + 0.3 * u[0], u[1] - 0.5, 0.3 + u[2], u[3] - 0.5])
        else:
            aff[k] = torch.stack([3.0 * u[0] - 1.5, 3.0 * u[1] - 1.5, 0.3 + u[2], u[3] - 0.5])
    return triples, aff


def torch_composition(x, gy, triples, affine, width, chunk):
    """forward + backward of the formula in torch ops, rows in chunks; returns (y, gx, g_affine)"""
    dev = x.device
    idx = torch.tensor(triples, device=dev)
    o, i, f = idx[:, 0], idx[:, 1], idx[:, 2]
    fns = [v[1] for v in SYMBOLIC_LIB.values()]
    present = sorted(set(f.tolist()))
    masks = {k: torch.zeros(width, width, device=dev).index_put((o[f == k], i[f == k]), torch.ones((), device=dev)).bool() for k in present}
    safe, zero = torch.full((), 2.5, device=dev), torch.zeros((), device=dev)
    g_aff = torch.zeros_like(affine)
    ys, gxs = [], []
    for r in range(0, x.size(0), chunk):
        xc = x[r:r + chunk].detach().requires_grad_(True)
        aff = affine.detach().requires_grad_(True)
        dense = lambda col, fill: torch.full((width, width), fill, device=dev).index_put((o, i), aff[:, col])
        A, B, C, D = dense(0, 0.0), dense(1, 2.5), dense(2, 0.0), dense(3, 0.0)
        t = A * xc[:, None, :] + B
        y = sum(torch.where(masks[k], C * fns[k](torch.where(masks[k], t, safe)) + D, zero).sum(-1) for k in present)
        y.backward(gy[r:r + chunk])
        ys.append(y.detach()); gxs.append(xc.grad)
        g_aff += aff.grad
    return torch.cat(ys), torch.cat(gxs), g_aff


def measure(fn, repeats):
    fn()                                           # warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
        del out
    return statistics.median(times), torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--densities", default="0.01,0.1,1.0")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--torch-chunk", type=int, default=32768)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-kinks", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("symbolic_edges_step.py measures on the GPU: no device visible")
    dev, w, n = "cuda:0", args.width, args.rows
    gen = torch.Generator().manual_seed(0)
    x = (2.0 * torch.rand(n, w, generator=gen) - 1.0).to(dev)
    gy = torch.randn(n, w, generator=gen).to(dev)
    report = {"rows": n, "width": w, "torch_chunk": args.torch_chunk, "densities": {}}
    for density in (float(v) for v in args.densities.split(",")):
        triples, aff = make_edges(w, density, gen, kinks=not args.no_kinks)
        edges = ops.SymbolicEdges.from_sorted(triples, w, w, dev)
        aff = aff.to(dev)

        def op_step():
            xr, ar = x.detach().requires_grad_(True), aff.detach().requires_grad_(True)
            y = ops.symbolic_edges(xr, edges, ar, w)
            y.backward(gy)
            return y.detach(), xr.grad, ar.grad

        torch.manual_seed(0)
        layer = kagnn_amd.KANLinear(w, w).to(dev)
        plain_ms, plain_peak = measure(lambda: layer(x.detach().requires_grad_(True)).backward(gy), args.repeats)
        layer._set_fixed({(o, i): (ops.SYMBOLIC_FUNCTIONS[f], aff[k]) for k, (o, i, f) in enumerate(triples)})

        def layer_step():
            layer.zero_grad(set_to_none=True)
            layer(x.detach().requires_grad_(True)).backward(gy)

        row = {"edges": len(triples)}
        row["kernel_ms"], row["kernel_peak_bytes"] = measure(op_step, args.repeats)
        row["layer_fixed_ms"], row["layer_fixed_peak_bytes"] = measure(layer_step, args.repeats)
        row["layer_plain_ms"], row["layer_plain_peak_bytes"] = plain_ms, plain_peak
        if not args.no_torch:
            step = lambda: torch_composition(x, gy, triples, aff, w, args.torch_chunk)
            row["torch_ms"], row["torch_peak_bytes"] = measure(step, args.repeats)
            got, want = op_step(), step()
            row["max_rel_diff_to_torch"] = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(got, want)]
            row["speedup_over_torch"] = row["torch_ms"] / row["kernel_ms"]
        report["densities"][str(density)] = row
        print(json.dumps({str(density): row}), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
