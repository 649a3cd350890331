#!/usr/bin/env python3
"""What one epoch of `harness.train_link_prediction` costs, beside the same epoch written with torch ops only.

    python tools/link_prediction_step.py [--shapes cora,arxiv] [--repeats 5] [--json out.json]

Shapes: `cora` = 2 708 nodes, 10 556 edges; `arxiv` = 169 343 nodes, about 1.17M edges -- random undirected graphs of those sizes
(both directions listed), 128 random features, `LinkPredictor(GKAN_Nodes('gcn', 2, 128, 64, 64))`, a 5 % / 10 % split.

The device loop: `train_link_prediction(epochs=K)` is timed at two epoch counts, K and 3K (wall clock ended by a device synchronise,
the two alternating, `--repeats` times after one warm-up each), and the epoch is (T(3K) - T(K)) / 2K -- the set-up (indexing the
graphs and the fixed pair lists, the evaluation negatives) is in both and drops out.  The per-kernel split is the library's stage
timer (`ops.LibraryStageTimer`) around a further run of K epochs, in a run of its own.

The baseline: the same epoch with torch ops only, the SAME encoder, optimiser and pair counts -- `torch.randint` candidates filtered
with `torch.isin` against the key vector (rejected slots get weight 0, as EMPTY slots do), gathered-row dot products, a weighted
`F.binary_cross_entropy_with_logits`, backward, `harness.Adam`; then the eval-mode forward, the validation loss and a
`torch.sort`-based AUC (rank sum of the positives), all left on the device.  Timed the same way, from the same starting weights.
The stage timer's run includes the set-up and the final test evaluation once (their stages are divided by K like the rest).
Figures are reported, not gated."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kagnn_amd                                   # noqa: E402
from kagnn_amd import data, harness, ops           # noqa: E402

SHAPES = {"cora": (2708, 10556, 10), "arxiv": (169343, 1166243, 3)}       # nodes, directed edges, K


def undirected_graph(n, e_directed, seed):
    gen = torch.Generator().manual_seed(seed)
    m = e_directed // 2
    u, v = torch.randint(0, n, (m,), generator=gen), torch.randint(0, n, (m,), generator=gen)
    keep = u != v
    lo, hi = torch.minimum(u, v)[keep], torch.maximum(u, v)[keep]
    code = torch.unique(lo * n + hi)
    lo, hi = code // n, code % n
    return torch.cat([torch.stack([lo, hi]), torch.stack([hi, lo])], dim=1).contiguous()


def wall_s(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def per_epoch_ms(run, k, repeats):
    """(T(3k) - T(k)) / 2k over alternating runs, in ms: median, minimum and maximum of the `repeats` differences"""
    run(k), run(3 * k)
    diffs = []
    for _ in range(repeats):
        a, b = wall_s(lambda: run(k)), wall_s(lambda: run(3 * k))
        diffs.append((b - a) / (2 * k) * 1e3)
    return {"median": statistics.median(diffs), "min": min(diffs), "max": max(diffs)}


def torch_ops_loop(model, x, split, epochs, lr, seed):
    """the baseline: no kagnn op outside the encoder and the optimiser"""
    n, dev = split.num_nodes, x.device
    g = ops.graph_index(split.train_edge_index, n)
    keys = torch.unique(split.train_edge_index[0] * n + split.train_edge_index[1])
    pos, p = split.train_pos, split.train_pos.size(1)
    val_pairs = torch.cat([split.val_pos, split.val_neg], dim=1)
    y_val = torch.cat([torch.ones(split.val_pos.size(1), device=dev), torch.zeros(split.val_neg.size(1), device=dev)])
    w_val = torch.cat([torch.ones(split.val_pos.size(1), device=dev), split.val_neg_valid.float()])
    y_train = torch.cat([torch.ones(p, device=dev), torch.zeros(p, device=dev)])
    gen = torch.Generator(device=dev).manual_seed(seed)
    optimizer = harness.Adam(model.parameters(), lr=lr)
    history = torch.zeros((epochs, 2), device=dev)

    def dots(z, pairs):
        return (z.index_select(0, pairs[0]) * z.index_select(0, pairs[1])).sum(-1)
    for epoch in range(epochs):
        neg = torch.randint(0, n, (2, p), generator=gen, device=dev)
        valid = (neg[0] != neg[1]) & ~torch.isin(neg[0] * n + neg[1], keys, assume_unique=False)
        model.train()
        optimizer.zero_grad(set_to_none=True)
        z = model.encode(x, g)
        scores = torch.cat([dots(z, pos), dots(z, neg)])
        w = torch.cat([torch.ones(p, device=dev), valid.float()])
        loss = F.binary_cross_entropy_with_logits(scores, y_train, weight=w, reduction="sum") / w.sum().clamp(min=1.0)
        loss.backward()
        optimizer.step()
        model.eval()
        with torch.no_grad():
            s = dots(model.encode(x, g), val_pairs)
            history[epoch, 0] = F.binary_cross_entropy_with_logits(s, y_val, weight=w_val, reduction="sum") / w_val.sum().clamp(min=1.0)
            order = torch.sort(s).indices
            rank = torch.empty_like(s)
            rank[order] = torch.arange(1, s.numel() + 1, device=dev, dtype=s.dtype)
            n_pos, n_neg = y_val.sum(), (1.0 - y_val).sum()
            history[epoch, 1] = ((rank * y_val).sum() - n_pos * (n_pos + 1) / 2) / (n_pos * n_neg)
    return history


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cora,arxiv")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--features", type=int, default=128)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("link_prediction_step.py measures on the GPU; none is visible")
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "library_version": kagnn_amd._lib.load().kagnn_version(), "repeats": args.repeats,
           "shapes": {}}
    for name in args.shapes.split(","):
        n, e, k = SHAPES[name]
        ei = undirected_graph(n, e, 1).to(dev)
        x = (0.5 * torch.randn(n, args.features, generator=torch.Generator().manual_seed(2))).to(dev)
        split = data.random_link_split(ei, n, 0.05, 0.1, generator=torch.Generator().manual_seed(3)).with_negatives(4)
        torch.manual_seed(5)
        start = kagnn_amd.LinkPredictor(kagnn_amd.GKAN_Nodes("gcn", 2, args.features, args.hidden, args.hidden)).to(dev)
        state = {key: v.clone() for key, v in start.state_dict().items()}

        def device_loop(epochs):
            start.load_state_dict(state)
            return harness.train_link_prediction(start, x, split, epochs=epochs, lr=0.01, patience=epochs + 1, poll_every=epochs + 1, seed=4)

        def baseline(epochs):
            start.load_state_dict(state)
            return torch_ops_loop(start, x, split, epochs, 0.01, 4)
        with harness._autograd_threads(False):
            res = {"nodes": n, "edges": int(ei.size(1)), "train_positives": int(split.train_pos.size(1)),
                   "val_pairs": int(split.val_pos.size(1) + split.val_neg.size(1)), "epochs_k": k,
                   "small_csr_path_for_the_negatives": bool(kagnn_amd._lib.load().kagnn_csr_small_ok(int(split.train_pos.size(1)), n)),
                   "device_loop_epoch_ms": per_epoch_ms(device_loop, k, args.repeats),
                   "torch_ops_epoch_ms": per_epoch_ms(baseline, k, args.repeats)}
            with ops.LibraryStageTimer():
                device_loop(k)
                torch.cuda.synchronize()
                stages = ops.LibraryStageTimer.collect(capacity=128)
            res["stage_ms_per_epoch"] = {s: round(v["total_ms"] / k, 4) for s, v in sorted(stages.items(), key=lambda kv: -kv[1]["total_ms"])}
            res["stage_launches_per_epoch"] = {s: v["launches"] / k for s, v in stages.items()}
            last = device_loop(k)
            res["val_auc_after_k_epochs"] = ops.link_rank_figures(last.rank_history[-1])["auc"]
            res["baseline_val_auc_after_k_epochs"] = float(baseline(k)[-1, 1])
        res["device_over_torch_ops"] = res["device_loop_epoch_ms"]["median"] / res["torch_ops_epoch_ms"]["median"]
        out["shapes"][name] = res
        print(json.dumps({name: res}), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
