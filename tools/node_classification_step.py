"""Milliseconds per epoch of the node-classification experiment (``harness.train_node_classification``) against the same loop built
from what the package offered before it: ``ops.softmax_cross_entropy`` for the training loss, then -- as the reference's
``train_total`` does -- boolean-mask indexing and torch's CrossEntropyLoss for the validation loss, the three ``int(correct.sum())``
accuracies (every ``--rate-print`` epochs), the host comparison of the early stopper and in-memory ``state_dict`` clones on improvement.

Two workloads: a Cora-shaped random graph (2708 nodes, 10556 edges, 1433 features, 7 classes) and an ogbn-arxiv-shaped one (169343
nodes, 1166243 edges, 128 features, 40 classes), ``GKAN_Nodes('gcn', 2, ..., 64)``.  Patience is larger than the epoch count, so
every variant runs the same number of epochs; each is warmed up, then timed ``--repeats`` times, alternating the variants; median and
min..max are reported.  One JSON line per workload on stdout; ``--out`` also writes them to a file.

    python tools/node_classification_step.py --epochs 64 --repeats 5 --out results/node_classification_step.json
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kagnn_amd                                                    # noqa: E402
from kagnn_amd import harness, ops                                  # noqa: E402

SHAPES = {"cora": (2708, 10556, 1433, 7), "arxiv": (169343, 1166243, 128, 40)}


def workload(name, device):
    n, e, f, c = SHAPES[name]
    g = torch.Generator().manual_seed(0)
    x = torch.randn(n, f, generator=g)
    ei = torch.randint(0, n, (2, e), generator=g)
    y = torch.randint(0, c, (n,), generator=g)
    perm = torch.randperm(n, generator=g)
    masks = torch.zeros(3, n, dtype=torch.bool)
    a, b = int(0.5 * n), int(0.7 * n)
    masks[0, perm[:a]], masks[1, perm[a:b]], masks[2, perm[b:]] = True, True, True
    model = kagnn_amd.GKAN_Nodes("gcn", 2, f, 64, c)
    return model.to(device), x.to(device), ei.to(device), y.to(device), masks.to(device)


def node_eval_launches(n, c):
    """kagnn_node_eval: one launch while one workgroup (256 lanes, a power-of-two group of lanes >= c per row, at most 64) covers the
    rows, else the per-workgroup partials and the launch that sums them"""
    w = 1
    while w < min(c, 64):
        w *= 2
    return 1 if n <= 256 // w else 2


def script_form(model, x, ei, y, train_mask, val_mask, test_mask, epochs, lr, patience, rate_print):
    """the reference's loop on the facilities the package had before the device loop"""
    saved = {k: v.detach().clone() for k, v in model.state_dict().items()}
    lowest, misses = float("inf"), 0
    opt = harness.Adam(model.parameters(), lr=lr)
    criterion = torch.nn.CrossEntropyLoss()
    g = ops.graph_index(ei, x.size(0))
    model.train()
    for epoch in range(epochs):
        opt.zero_grad()
        loss = ops.softmax_cross_entropy(model(x, g), y, train_mask)
        loss.backward()
        opt.step()
        with torch.no_grad():
            out = model(x, g)
            val_loss = criterion(out[val_mask], y[val_mask])
            if not (epoch + 1) % rate_print:
                pred = out.argmax(dim=1)
                for m in (train_mask, val_mask, test_mask):
                    _acc = int((pred[m] == y[m]).sum()) / int(m.sum())
        if val_loss < lowest:
            lowest, misses = val_loss, 0
            saved = {k: v.detach().clone() for k, v in model.state_dict().items()}
        elif val_loss >= lowest:
            misses += 1
            if misses >= patience:
                break
    model.load_state_dict(saved)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rate-print", type=int, default=10)
    ap.add_argument("--shapes", default="cora,arxiv")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/node_classification_step.py times the MI355X path: no GPU found")
    device, lines = "cuda:0", []
    for name in args.shapes.split(","):
        model0, x, ei, y, masks = workload(name, device)
        tr, va, te = masks
        kw = dict(epochs=args.epochs, lr=1e-3, patience=args.epochs + 1)

        def device_loop(poll):
            return lambda m: harness.train_node_classification(m, x, ei, y, tr, va, te, poll_every=poll, **kw)
        variants = {"device poll_every=16": device_loop(16), "device poll_every=1": device_loop(1),
                    "script form": lambda m: script_form(m, x, ei, y, tr, va, te, rate_print=args.rate_print, **kw)}
        times = {k: [] for k in variants}
        for rep in range(args.repeats + 1):                        # (repeat 0 warms every variant up and is dropped)
            for k, run in variants.items():
                m = copy.deepcopy(model0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(m)
                torch.cuda.synchronize()
                if rep:
                    times[k].append(1e3 * (time.perf_counter() - t0) / args.epochs)
        tensors = len(model0.state_dict())
        line = {"workload": name, "shape": dict(zip(("nodes", "edges", "features", "classes"), SHAPES[name])), "epochs": args.epochs,
                "repeats": args.repeats, "state_dict_tensors": tensors,
                "bookkeeping_launches_per_epoch": {"node_eval": node_eval_launches(*SHAPES[name][::3]), "early_stop_update": 1,
                                                   "copy_if": -(-tensors // 32)},
                "ms_per_epoch": {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                                 for k, v in times.items()}}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
