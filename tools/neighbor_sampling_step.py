#!/usr/bin/env python3
"""What a neighbour-sampled mini-batch costs: `ops.sample_neighbors` (csrc/subgraph.hip: mark, count, one read-back, fill) at the
headline graph (N = 1M nodes, E = 10M edges of `oracle.powerlaw_graph`, the recipe of bench.py), its two halves on their own, the
training step of `GKAN_Nodes('gin', 3, ...)` that the batch feeds, and `ops.k_hop_subgraph` at the same seeds and depth beside them.

    python tools/neighbor_sampling_step.py [--nodes 1000000] [--edges 10000000] [--seeds 1024] [--fanouts 10,10,10]
                                           [--hub-edges 120000] [--repeats 20] [--json out.json]

Timing: wall clock around each call, ended by a device synchronise; `--repeats` calls per form after three warm-up calls each, the
forms alternating in one process; reported per form: median, minimum and maximum in ms.  `mark` is `kagnn_neighbor_sample_mark` alone
(three memsets, the seed kernel, one level kernel per fan-out), `extract` is count, the read of the two counts, and fill on the
mark call's output.  The training step is `{zero_grad, forward on the batch, cross entropy on the seed rows, backward, Adam}` --
`harness._training_step`, the one `train_node_classification_sampled` takes -- on ONE batch sampled ahead of the timed calls.

The long-row path: the power-law graph's largest row has some 10k edges, so `--hub-edges` (>= 100 000) more edges into node 0 are
appended to the edge list, the graph indexed again, and the mark call timed with node 0 as the only seed at fan-out 10 (radix select
over the whole row) and at fan-out -1 (the whole row, no key), beside a seed of ordinary degree.  Figures are reported, not gated."""
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
from kagnn_amd import harness, ops                 # noqa: E402
from oracle import kan_oracle as orc               # noqa: E402


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def alternate(forms, repeats):
    for fn in forms.values():
        for _ in range(3):
            fn()
    times = {k: [] for k in forms}
    for _ in range(repeats):
        for k, fn in forms.items():
            times[k].append(wall_ms(fn))
    return {k: stats(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=10_000_000)
    ap.add_argument("--seeds", type=int, default=1024)
    ap.add_argument("--fanouts", default="10,10,10")
    ap.add_argument("--hub-edges", type=int, default=120_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--features", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--classes", type=int, default=40)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("neighbor_sampling_step.py measures on the GPU; none is visible")
    if args.repeats < 20:
        raise SystemExit("at least 20 timed calls per form")
    dev, n, e = "cuda:0", args.nodes, args.edges
    fan = [int(v) for v in args.fanouts.split(",")]
    ei = orc.powerlaw_graph(n, e, seed=0).to(dev)
    g = ops.graph_index(ei, n)
    gen = torch.Generator().manual_seed(1)
    seeds = torch.randperm(n, generator=gen)[:args.seeds].to(dev)
    out = {"device": torch.cuda.get_device_name(0), "library_version": kagnn_amd._lib.load().kagnn_version(), "nodes": n, "edges": e,
           "seeds": args.seeds, "fanouts": fan, "repeats": args.repeats}

    # ---- the sampler, its halves, and the full receptive field beside it
    sub = ops.sample_neighbors(seeds, fan, g, seed=7)
    full = ops.k_hop_subgraph(seeds, len(fan), g)
    marked = ops._mark_sampled(seeds, fan, g, 7)

    def extract():
        hop, keep, rec = marked
        return ops._subgraph_extract("sample_neighbors", hop, rec, g, seeds, True, keep)
    t = alternate({"sample_neighbors": lambda: ops.sample_neighbors(seeds, fan, g, seed=7),
                   "mark": lambda: ops._mark_sampled(seeds, fan, g, 7), "extract": extract,
                   "k_hop_subgraph": lambda: ops.k_hop_subgraph(seeds, len(fan), g)}, args.repeats)
    out["sampler"] = {"n_sub": sub.num_nodes, "e_sub": sub.num_edges, "k_hop_n_sub": full.num_nodes, "k_hop_e_sub": full.num_edges,
                      "sample_neighbors_ms": t["sample_neighbors"], "mark_ms": t["mark"], "extract_ms": t["extract"],
                      "k_hop_subgraph_ms": t["k_hop_subgraph"]}
    print(json.dumps(out["sampler"]), flush=True)

    # ---- one training step on the batch
    torch.manual_seed(0)
    model = kagnn_amd.GKAN_Nodes("gin", len(fan), args.features, args.hidden, args.classes, grid_size=5, spline_order=3).to(dev).train()
    x = (0.5 * torch.randn(n, args.features, generator=gen)).to(dev)
    y = torch.randint(0, args.classes, (n,), generator=gen).to(dev)
    xb, yb = x[sub.nodes], y[seeds]
    step = harness._training_step(harness.Adam(model.parameters(), lr=1e-3))

    def loss_of():
        return ops.softmax_cross_entropy(model(xb, sub.index)[sub.mapping], yb)

    def sample_and_gather():                       # what the loader does per batch
        s = ops.sample_neighbors(seeds, fan, g, seed=7)
        return x[s.nodes], y[seeds]
    with harness._autograd_threads(False):
        t = alternate({"step": lambda: step(loss_of), "sample_and_gather": sample_and_gather}, args.repeats)
    share = t["sample_and_gather"]["median"] / t["step"]["median"]
    out["training_step"] = {"model": f"GKAN_Nodes('gin', {len(fan)}, {args.features} -> {args.hidden} -> {args.classes}, grid 5)",
                            "rows": sub.num_nodes, "edges": sub.num_edges, "step_ms": t["step"], "sample_and_gather_ms": t["sample_and_gather"],
                            "sampler_over_step": share, "sampler_exceeds_a_quarter_of_the_step": share > 0.25}
    print(json.dumps(out["training_step"]), flush=True)

    # ---- the long-row path: a hub of >= 100k edges in the frontier
    if args.hub_edges > 0:
        hub_src = torch.randint(0, n, (args.hub_edges,), generator=gen).to(dev)
        ei_hub = torch.cat([ei, torch.stack([hub_src, torch.zeros_like(hub_src)])], 1).contiguous()
        gh = ops.GraphIndex(ei_hub, n)
        deg = int(gh.rowptr[1] - gh.rowptr[0])
        hub, plain = torch.zeros(1, dtype=torch.int64, device=dev), seeds[:1]
        plain_deg = int((gh.rowptr[plain + 1] - gh.rowptr[plain])[0])
        t = alternate({"hub_k10": lambda: ops._mark_sampled(hub, [10], gh, 7), "hub_all": lambda: ops._mark_sampled(hub, [-1], gh, 7),
                       "hub_k_half": lambda: ops._mark_sampled(hub, [deg // 2], gh, 7),
                       "plain_k10": lambda: ops._mark_sampled(plain, [10], gh, 7)}, args.repeats)
        kept = int(ops._mark_sampled(hub, [10], gh, 7)[1].sum())
        out["hub"] = {"hub_in_degree": deg, "plain_in_degree": plain_deg, "edges": gh.num_edges, "kept_at_fanout_10": kept,
                      "mark_hub_fanout_10_ms": t["hub_k10"], "mark_hub_fanout_half_ms": t["hub_k_half"], "mark_hub_all_ms": t["hub_all"],
                      "mark_plain_fanout_10_ms": t["plain_k10"],
                      "long_row_cost_ms": t["hub_k10"]["median"] - t["plain_k10"]["median"]}
        print(json.dumps(out["hub"]), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
