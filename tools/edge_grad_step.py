#!/usr/bin/env python3
"""What the edge-weight gradient costs: `ops.aggregate_edge_grad` (csrc/aggregate_edge.hip) at the headline graph (N = 1M nodes,
E = 10M edges of `oracle.powerlaw_graph`, F = 64) beside the forward aggregation `kagnn_aggregate_sum` with edge weights on the same
graph -- the two calls a step with differentiable edge weights adds to each other.

    python tools/edge_grad_step.py [--nodes 1000000] [--edges 10000000] [--widths 64] [--repeats 20] [--json out.json]

Timing: device events around each call on the launch stream, `--repeats` calls per variant after three warm-up calls each, the
variants alternating; reported per variant: median and range, and the algorithmic bytes of the gradient, `E (4 F + 12) + 4 N F`
(per edge one gathered row of x, col, perm and the stored value; gout once per row), over the median time.  The forward moves the
same rows plus the edge weights and writes `4 N F`: the same count serves as its yardstick.  A correctness check against fp64 on a
sample of the edges comes first."""
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
from oracle import kan_oracle as orc               # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=10_000_000)
    ap.add_argument("--widths", default="64")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edge_grad_step.py measures on the GPU; none is visible")
    dev, n, e = "cuda:0", args.nodes, args.edges
    ei = orc.powerlaw_graph(n, e, seed=0)
    g = ops.GraphIndex(ei.to(dev), n)
    deg = torch.bincount(ei[1], minlength=n)
    out = {"device": torch.cuda.get_device_name(0), "library_version": kagnn_amd._lib.load().kagnn_version(), "nodes": n, "edges": e,
           "max_in_degree": int(deg.max()), "hub_segments": g.num_hub_seg, "hub_threshold": g.hub_threshold, "widths": []}
    gen = torch.Generator().manual_seed(1)
    w = torch.rand(e, generator=gen).to(dev)
    w_csr = w[g.perm.long()].contiguous()
    dis = g.gcn_dis
    for f in (int(v) for v in args.widths.split(",")):
        x, gout = (0.8 * torch.randn(n, f, generator=gen)).to(dev), (0.8 * torch.randn(n, f, generator=gen)).to(dev)
        grad = lambda: ops.aggregate_edge_grad(x, gout, g, dis, dis, True)
        fwd = lambda: ops._aggregate_raw(x, g, False, 1.0, w_csr, dis, dis, None, True)
        got = grad()
        pick = torch.randint(0, e, (20000,), generator=gen)
        src, dst = ei[0, pick], ei[1, pick]
        d64 = dis.double().cpu()
        want = d64[dst] * d64[src] * (gout.cpu().double()[dst] * x.cpu().double()[src]).sum(1) * (src != dst)
        err = float((got.cpu().double()[pick] - want).abs().max() / want.abs().max())
        assert err <= 2e-5, err
        assert torch.equal(got, grad()), "the gradient must be bit-reproducible"
        for _ in range(3):
            grad(), fwd()
        times = {"aggregate_edge_grad": [], "aggregate_sum": []}
        for _ in range(args.repeats):
            times["aggregate_edge_grad"].append(event_ms(grad))
            times["aggregate_sum"].append(event_ms(fwd))
        nbytes = e * (4 * f + 12) + 4 * n * f
        entry = {"F": f, "algorithmic_bytes": nbytes, "max_error_over_max_on_20000_edges": err}
        for name, t in times.items():
            med = statistics.median(t)
            entry[name + "_ms"] = {"median": med, "min": min(t), "max": max(t)}
            entry[name + "_TB_per_s"] = nbytes / (med * 1e-3) / 1e12
        entry["edge_grad_over_forward"] = entry["aggregate_edge_grad_ms"]["median"] / entry["aggregate_sum_ms"]["median"]
        out["widths"].append(entry)
        print(json.dumps(entry))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
