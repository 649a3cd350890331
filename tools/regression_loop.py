#!/usr/bin/env python3
"""What one epoch of the graph-regression experiment costs: `harness.train_graph_regression` (a metered `ops.l1_loss` launch per
batch, one `kagnn_regression_epoch_update` per epoch, the record polled every `--poll` epochs) against the composition the package
offered before it -- per epoch `train_graph_batches(nb_epochs=1)` plus two `evaluate_graph_batches` (validation, test), the stopper
on the host -- timed in ONE process on one box, the two forms ALTERNATING, on the same loaders and copies of the same model.

Two shapes: `--shape zinc` (256-graph batches of molecules of 18-28 atoms, 2 n + 4 bonds, integer features, bench.py's config-4
model: KAGINRegression(4 GINE convolutions, hidden 64, embedding encoders); 10 training, 2 validation and 2 test batches) and
`--shape test` (the 40-graph loaders of tests/test_gpu_graph_regression.py: batches of 16, 3 + 2 + 2 batches, linear encoders).

    python tools/regression_loop.py --shape zinc [--epochs 8] [--repeats 5] [--json out.json]          # ms per epoch
    python tools/regression_loop.py --shape zinc --count [--epochs 4]                                   # launches and read-backs

`--count` is a run of its own (a profiler slows the host): kernel launches per epoch from torch.profiler's device events, and what
reaches the host per epoch (`item / tolist / cpu / numpy / float() / int() / bool()` on device tensors, and explicit stream, event
and device waits), counted by wrappers.  The figures are reported in profiles/graph_regression_loop.md; none is a gate."""
from __future__ import annotations

import argparse
import copy
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kagnn_amd                                   # noqa: E402
from kagnn_amd import harness, ops                 # noqa: E402


def dataset(shape, graphs, dev, seed=1):
    g = torch.Generator().manual_seed(seed)
    zinc = shape == "zinc"
    sizes = torch.randint(18, 29, (graphs,), generator=g) if zinc else torch.randint(3, 10, (graphs,), generator=g)
    esizes = 2 * sizes + 4 if zinc else 2 * sizes
    node_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)])
    n, e = int(node_ptr[-1]), int(esizes.sum())
    lo, span = torch.repeat_interleave(node_ptr[:-1], esizes), torch.repeat_interleave(sizes, esizes)
    ei = torch.stack([lo + (torch.rand(e, generator=g) * span).long().clamp(max=span - 1) for _ in range(2)])
    if zinc:
        x, ea = torch.randint(0, 21, (n, 1), generator=g), torch.randint(0, 4, (e,), generator=g)
    else:
        x, ea = torch.randn(n, 21, generator=g), torch.randn(e, 4, generator=g)
    return kagnn_amd.DeviceGraphDataset(x, ei, node_ptr, edge_attr=ea, y=torch.randn(graphs, generator=g), device=dev)


def model(shape, dev):
    torch.manual_seed(0)
    if shape == "zinc":
        m = kagnn_amd.KAGINRegression(1, 1, 4, 64, 2, 4, 3, 1, 0.0, True)
        m.atom_encoder = kagnn_amd.graph_models.AtomEncoder(64, [21])
        m.bond_encoder.bond_embedding_list = torch.nn.ModuleList([torch.nn.Embedding(4, 64)])
        return m.to(dev)
    return kagnn_amd.KAGINRegression(21, 4, 2, 32, 2, 4, 3, 1, 0.0).to(dev)


def composed(m, opt, loaders, epochs, patience=10 ** 6):
    """the experiment from the parts there were: three host waits and two read-backs per epoch, the rules on the host"""
    tr, va, te = loaders
    best, lowest, counter, test = float("inf"), float("inf"), 0, float("nan")
    for _ in range(epochs):
        harness.train_graph_batches(m, tr, nb_epochs=1, optimizer=opt)
        val = harness.evaluate_graph_batches(m, va)
        every = harness.evaluate_graph_batches(m, te)                  # (every epoch, as the native loop: the same device work)
        if best >= val:
            best, test = val, every
        if val < lowest:
            lowest, counter = val, 0
        elif val >= lowest:
            counter += 1
            if counter >= patience:
                break
    return best, test


def native(m, opt, loaders, epochs, poll):
    r = harness.train_graph_regression(m, *loaders, epochs=epochs, patience=10 ** 6, poll_every=poll, optimizer=opt)
    return r.best_val_loss, r.test_loss


class HostTraffic:
    """counts what brings a device value to the host, and explicit waits, while installed"""
    NAMES = ("item", "tolist", "cpu", "numpy", "__float__", "__int__", "__bool__", "__index__")

    def __enter__(self):
        self.reads, self.waits, self._undo = 0, 0, []
        outer = self

        def wrap(owner, name, kind, when):
            real = getattr(owner, name)

            def counted(*a, **kw):
                if when is None or when(a[0]):
                    setattr(outer, kind, getattr(outer, kind) + 1)
                return real(*a, **kw)
            setattr(owner, name, counted)
            self._undo.append((owner, name, real))
        for name in self.NAMES:
            wrap(torch.Tensor, name, "reads", lambda t: t.is_cuda)
        real_to = torch.Tensor.to

        def to(t, *a, **kw):
            out = real_to(t, *a, **kw)
            outer.reads += bool(t.is_cuda and not out.is_cuda)
            return out
        torch.Tensor.to = to
        self._undo.append((torch.Tensor, "to", real_to))
        wrap(torch.cuda, "synchronize", "waits", None)
        wrap(torch.cuda.Event, "synchronize", "waits", None)
        wrap(torch.cuda.Stream, "synchronize", "waits", None)
        return self

    def __exit__(self, *exc):
        for owner, name, real in reversed(self._undo):
            setattr(owner, name, real)
        return False


def count(fn, epochs):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with HostTraffic() as host:
        fn()
        torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    kernels = copies = 0
    for ev in prof.events():
        if str(getattr(ev, "device_type", "")).endswith("CUDA"):
            if any(k in ev.name for k in ("Memcpy", "Memset", "memcpy", "memset")):
                copies += 1
            else:
                kernels += 1
    return {"kernel_launches_per_epoch": kernels / epochs, "device_copies_and_fills_per_epoch": copies / epochs,
            "host_read_backs_per_epoch": host.reads / epochs, "host_waits_per_epoch": (host.waits - 1) / epochs}


def figures(ms):
    s = sorted(ms)
    return {"median_ms": s[len(s) // 2], "spread_ms": s[-1] - s[0], "repeats_ms": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("zinc", "test"), default="zinc")
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--poll", type=int, default=8)
    ap.add_argument("--count", action="store_true")
    ap.add_argument("--json")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.shape == "zinc":
        ds, batch = dataset("zinc", 2560 + 512 + 512, dev), 256
        views = (ds[:2560], ds[2560:3072], ds[3072:])
    else:
        ds, batch = dataset("test", 40, dev), 16
        views = (ds, ds[list(range(5, 30))], ds[20:40])
    loaders = (kagnn_amd.DeviceBatchLoader(views[0], batch, shuffle=True, generator=torch.Generator().manual_seed(1)),
               kagnn_amd.DeviceBatchLoader(views[1], batch), kagnn_amd.DeviceBatchLoader(views[2], batch))
    m_native = model(args.shape, dev)
    m_composed = copy.deepcopy(m_native)
    o_native, o_composed = harness.Adam(m_native.parameters(), lr=1e-3), harness.Adam(m_composed.parameters(), lr=1e-3)
    run_native = lambda: native(m_native, o_native, loaders, args.epochs, args.poll)            # noqa: E731
    run_composed = lambda: composed(m_composed, o_composed, loaders, args.epochs)               # noqa: E731
    run_native(), run_composed()                       # warm-up: every shape of the timed windows once, both forms
    out = {"device": torch.cuda.get_device_name(0), "library_version": kagnn_amd._lib.load().kagnn_version(), "shape": args.shape,
           "batch": batch, "batches_per_epoch": [len(l) for l in loaders], "epochs": args.epochs, "poll_every": args.poll}
    if args.count:
        out["native"], out["composed"] = count(run_native, args.epochs), count(run_composed, args.epochs)
    else:
        ms = {"native": [], "composed": []}
        for _ in range(args.repeats):                  # alternating: a drift of the box hits both forms alike
            for name, fn in (("native", run_native), ("composed", run_composed)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3 / args.epochs)
        out["repeats"] = args.repeats
        out["native_ms_per_epoch"], out["composed_ms_per_epoch"] = figures(ms["native"]), figures(ms["composed"])
    print(json.dumps(out, indent=1))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
