#!/usr/bin/env python3
"""What the graph-classification loops cost per step: `harness.train_graph_classification` / `evaluate_graph_classification` (one
`ops.nll_loss` launch per batch that feeds a device record, ONE read-back per epoch) against the loops of the reference's script
written out (`graph_classification/graph_classification_utils.py:45-72`: `F.nll_loss`, `loss.item()` per batch; `reduction='sum'` and
`.item()` per batch; `max(1)[1].eq(y).sum().item()` per batch), timed in ONE process on one box, the variants ALTERNATING, on a
TU-shaped synthetic dataset (graphs of 1-600 nodes, 2 n edges, float x [N, 7], two classes: the shapes of
tests/test_gpu_data.py::test_tu_shaped_epochs_equal_the_restatement) fed by the same `DeviceBatchLoader` and the same KAGIN.

Everything except the loop form is held equal: both train loops step `kagnn_amd.harness.Adam` and run autograd on the calling
thread (what `train_graph_classification` does), so the difference is the loss launch(es) and the read-back per batch.  The script
needs TWO passes over a loader for loss and accuracy (`val` and `test`), the native evaluation one; the passes are reported apart.

    python tools/classification_step.py [--graphs 1000] [--batch 32] [--epochs 3] [--repeats 5] [--json out.json]

Per variant: the median over the repeats and their spread (max - min).  The requirement is stated in profiles/classification_loop.md."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kagnn_amd                                   # noqa: E402
from kagnn_amd import harness, ops                 # noqa: E402


def dataset(graphs, dev, seed=2):
    g = torch.Generator().manual_seed(seed)
    sizes = torch.randint(1, 601, (graphs,), generator=g)
    esizes = 2 * sizes
    node_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)])
    n, e = int(node_ptr[-1]), int(esizes.sum())
    lo, span = torch.repeat_interleave(node_ptr[:-1], esizes), torch.repeat_interleave(sizes, esizes)
    ei = torch.stack([lo + (torch.rand(e, generator=g) * span).long().clamp(max=span - 1),
                      lo + (torch.rand(e, generator=g) * span).long().clamp(max=span - 1)])
    return kagnn_amd.DeviceGraphDataset(torch.randn(n, 7, generator=g), ei, node_ptr, y=torch.randint(0, 2, (graphs,), generator=g), device=dev)


def script_train(model, loader, optimizer, epochs):
    """the reference's `train`, `epochs` times; seconds per step"""
    mt_was = torch.autograd.is_multithreading_enabled()
    torch.autograd.set_multithreading_enabled(False)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(epochs):
            model.train()
            loss_all = 0
            for data in loader:
                data = data.to("cuda")
                loss = F.nll_loss(model(data), data.y)
                optimizer.zero_grad()
                loss.backward()
                loss_all += data.num_graphs * loss.item()
                optimizer.step()
            ops.flush_graph_checks()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (epochs * len(loader))
    finally:
        torch.autograd.set_multithreading_enabled(mt_was)


def script_val(model, loader):
    model.eval()
    loss_all = 0
    with torch.no_grad():
        for data in loader:
            data = data.to("cuda")
            loss_all += F.nll_loss(model(data), data.y, reduction='sum').item()
    return loss_all / len(loader.dataset)


def script_test(model, loader):
    model.eval()
    correct = 0
    with torch.no_grad():
        for data in loader:
            data = data.to("cuda")
            pred = model(data).max(1)[1]
            correct += pred.eq(data.y).sum().item()
    return correct / len(loader.dataset)


def per_batch(fn, loader, passes):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(passes):
        out = fn()
    ops.flush_graph_checks()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (passes * len(loader)), out


def figures(ms):
    s = sorted(ms)
    return {"median_ms": s[len(s) // 2], "spread_ms": s[-1] - s[0], "repeats_ms": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ds = dataset(args.graphs, dev)
    cut = args.graphs * 9 // 10
    train_ds, val_ds = ds[:cut], ds[cut:]

    def train_loader():
        return kagnn_amd.DeviceBatchLoader(train_ds, args.batch, shuffle=True, generator=torch.Generator().manual_seed(1))
    val_loader = kagnn_amd.DeviceBatchLoader(val_ds, args.batch)
    torch.manual_seed(0)
    native = kagnn_amd.KAGIN(2, 7, 32, 2, 2, 4, 3, 0.0).to(dev)
    import copy
    script = copy.deepcopy(native)
    native_opt, script_opt = harness.Adam(native.parameters(), lr=1e-3), harness.Adam(script.parameters(), lr=1e-3)
    # warm-up: every shape of the timed windows once, both forms
    harness.train_graph_classification(native, train_loader(), nb_epochs=1, optimizer=native_opt)
    script_train(script, train_loader(), script_opt, 1)
    harness.evaluate_graph_classification(native, val_loader), script_val(script, val_loader), script_test(script, val_loader)
    ms = {k: [] for k in ("native_train_step", "script_train_step", "native_eval_batch", "script_val_batch", "script_test_batch")}
    checks = {}
    passes = max(1, 3 * args.epochs)
    for _ in range(args.repeats):                      # alternating: a drift of the box hits every variant alike
        ms["native_train_step"].append(harness.train_graph_classification(native, train_loader(), nb_epochs=args.epochs,
                                                                          optimizer=native_opt)[0] * 1e3)
        ms["script_train_step"].append(script_train(script, train_loader(), script_opt, args.epochs) * 1e3)
        t, checks["native_eval"] = per_batch(lambda: harness.evaluate_graph_classification(native, val_loader), val_loader, passes)
        ms["native_eval_batch"].append(t * 1e3)
        t, checks["script_val"] = per_batch(lambda: script_val(native, val_loader), val_loader, passes)
        ms["script_val_batch"].append(t * 1e3)
        t, checks["script_test"] = per_batch(lambda: script_test(native, val_loader), val_loader, passes)
        ms["script_test_batch"].append(t * 1e3)
    out = {"device": torch.cuda.get_device_name(0), "library_version": kagnn_amd._lib.load().kagnn_version(), "graphs": args.graphs,
           "batch": args.batch, "train_steps_per_epoch": len(train_loader()), "eval_batches": len(val_loader), "epochs": args.epochs,
           "repeats": args.repeats, "eval_passes_per_repeat": passes, **{k: figures(v) for k, v in ms.items()},
           "same_model_figures": {"native (nll, accuracy)": checks["native_eval"], "script val": checks["script_val"],
                                  "script test": checks["script_test"]}}
    tr, ev = out["native_train_step"], out["native_eval_batch"]
    out["requirement"] = {
        "train: native - script (ms)": tr["median_ms"] - out["script_train_step"]["median_ms"],
        "train: spread allowed (ms)": max(tr["spread_ms"], out["script_train_step"]["spread_ms"]),
        "eval: native - script val pass (ms)": ev["median_ms"] - out["script_val_batch"]["median_ms"],
        "eval: spread allowed (ms)": max(ev["spread_ms"], out["script_val_batch"]["spread_ms"]),
    }
    r = out["requirement"]
    r["train met"] = r["train: native - script (ms)"] <= r["train: spread allowed (ms)"]
    r["eval met"] = r["eval: native - script val pass (ms)"] <= r["eval: spread allowed (ms)"]
    print(json.dumps(out, indent=1))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
