#!/usr/bin/env python3
"""What a k-hop subgraph costs: `ops.k_hop_subgraph` (csrc/subgraph.hip: mark, count, one read-back, fill -- no sort) beside the torch
composition a caller had to write before it, at the headline graph (N = 1M nodes, E = 10M edges of `oracle.powerlaw_graph`, the
recipe of bench.py), and what that does to one epoch of `explain_edges` on `GKAN_Nodes('gin', 3, ...)`.

    python tools/subgraph_step.py [--nodes 1000000] [--edges 10000000] [--seeds 1,16,256] [--hops 2,3] [--repeats 20] [--json out.json]

The torch composition is torch_geometric's `k_hop_subgraph(..., relabel_nodes=True)` written in torch ops on the device (a boolean
pass over all E edges and a masked select -- a host synchronisation -- per hop, `unique`, the relabelling gathers) followed by
`GraphIndex(sub_edge_index, n_sub)`, the sort-based build of the index the convolutions need.  Both forms return the same subgraph
(checked first, field by field and index array by index array).  Timing: wall clock around each call, ended by a device
synchronise, `--repeats` calls per form after three warm-up calls each, the two forms alternating in one process; reported: median,
minimum and maximum of each -- the spread of the composition is the only margin of the comparison.  The explainer rows time
`explain_edges(epochs=1, target=given)` with `num_hops` (extraction included, every call) and without."""
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
from oracle import kan_oracle as orc               # noqa: E402


def torch_k_hop_subgraph(node_idx, num_hops, edge_index, num_nodes):
    """torch_geometric.utils.k_hop_subgraph (2.5.3, flow='source_to_target', relabel_nodes=True) in torch ops, then the index"""
    row, col = edge_index[0], edge_index[1]
    node_mask = torch.empty(num_nodes, dtype=torch.bool, device=row.device)
    edge_mask = torch.empty(row.size(0), dtype=torch.bool, device=row.device)
    subsets = [node_idx]
    for _ in range(num_hops):
        node_mask.fill_(False)
        node_mask[subsets[-1]] = True
        torch.index_select(node_mask, 0, col, out=edge_mask)
        subsets.append(row[edge_mask])
    subset, inv = torch.cat(subsets).unique(return_inverse=True)
    inv = inv[:node_idx.numel()]
    node_mask.fill_(False)
    node_mask[subset] = True
    edge_mask = node_mask[row] & node_mask[col]
    sub_ei = edge_index[:, edge_mask]
    relabel = torch.full((num_nodes,), -1, dtype=torch.int64, device=row.device)
    relabel[subset] = torch.arange(subset.numel(), device=row.device)
    sub_ei = relabel[sub_ei].contiguous()
    return subset, sub_ei, inv, edge_mask, ops.GraphIndex(sub_ei, int(subset.numel()))


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
    ap.add_argument("--seeds", default="1,16,256")
    ap.add_argument("--hops", default="2,3")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--features", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--classes", type=int, default=40)
    ap.add_argument("--no-explainer", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("subgraph_step.py measures on the GPU; none is visible")
    if args.repeats < 20:
        raise SystemExit("at least 20 timed calls per form")
    dev, n, e = "cuda:0", args.nodes, args.edges
    ei = orc.powerlaw_graph(n, e, seed=0).to(dev)
    g = ops.graph_index(ei, n)
    out = {"device": torch.cuda.get_device_name(0), "library_version": kagnn_amd._lib.load().kagnn_version(), "nodes": n, "edges": e,
           "repeats": args.repeats, "extraction": [], "explainer": []}
    gen = torch.Generator().manual_seed(1)
    for ns in (int(v) for v in args.seeds.split(",")):
        seeds = torch.randperm(n, generator=gen)[:ns].to(dev)
        for hops in (int(v) for v in args.hops.split(",")):
            sub = ops.k_hop_subgraph(seeds, hops, g)
            subset, sub_ei, inv, edge_mask, want = torch_k_hop_subgraph(seeds, hops, ei, n)
            same = (torch.equal(sub.nodes, subset) and torch.equal(sub.edge_index, sub_ei) and torch.equal(sub.mapping, inv)
                    and torch.equal(sub.edge_ids, edge_mask.nonzero().flatten())
                    and all(torch.equal(a, b) for a, b in zip(sub.index.side(False)[:3] + sub.index.side(True)[:3],
                                                              want.side(False)[:3] + want.side(True)[:3])))
            assert same, (ns, hops)
            t = alternate({"k_hop_subgraph": lambda: ops.k_hop_subgraph(seeds, hops, g),
                           "torch_composition": lambda: torch_k_hop_subgraph(seeds, hops, ei, n)}, args.repeats)
            entry = {"seeds": ns, "hops": hops, "n_sub": sub.num_nodes, "e_sub": sub.num_edges, "identical": same,
                     "k_hop_subgraph_ms": t["k_hop_subgraph"], "torch_composition_ms": t["torch_composition"],
                     "composition_spread_ms": t["torch_composition"]["max"] - t["torch_composition"]["min"],
                     "composition_over_k_hop": t["torch_composition"]["median"] / t["k_hop_subgraph"]["median"]}
            entry["not_slower"] = entry["k_hop_subgraph_ms"]["median"] <= entry["torch_composition_ms"]["median"]
            out["extraction"].append(entry)
            print(json.dumps(entry), flush=True)
    if not args.no_explainer:
        torch.manual_seed(0)
        model = kagnn_amd.GKAN_Nodes("gin", 3, args.features, args.hidden, args.classes, grid_size=5, spline_order=3).to(dev).eval()
        x = (0.5 * torch.randn(n, args.features, generator=gen)).to(dev)
        with torch.no_grad():
            target = model(x, ei).argmax(-1)
        node = int(torch.randperm(n, generator=gen)[0])
        for hops in (int(v) for v in args.hops.split(",")):
            run = lambda h: kagnn_amd.explain_edges(model, x, ei, node_idx=node, target=target, epochs=1, num_hops=h,
                                                    generator=torch.Generator().manual_seed(2))
            sub = ops.k_hop_subgraph(node, hops, g)
            t = alternate({"local": lambda: run(hops), "whole_graph": lambda: run(None)}, args.repeats)
            entry = {"explain_edges_epoch": True, "hops": hops, "receptive_hops": kagnn_amd.receptive_hops(model), "n_sub": sub.num_nodes,
                     "e_sub": sub.num_edges, "local_ms": t["local"], "whole_graph_ms": t["whole_graph"],
                     "whole_over_local": t["whole_graph"]["median"] / t["local"]["median"]}
            out["explainer"].append(entry)
            print(json.dumps(entry), flush=True)
    print(json.dumps({"library_version": out["library_version"], "device": out["device"], "nodes": n, "edges": e,
                      "extraction_not_slower_everywhere": all(r["not_slower"] for r in out["extraction"])}), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
