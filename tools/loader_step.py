#!/usr/bin/env python3
"""What feeding the ZINC-shaped training step costs: four ways to hand `harness.train_graph_batches` its mini-batches, timed in ONE
process on one box with the bench's protocol for this step (median of 3 repeats of 10 epochs, bench.py::graph_level_step_figures'
model recipe) on a 10 000-graph ZINC-shaped synthetic dataset, 256 graphs per batch:

  (a) 8 premade batches reused every epoch        -- the path before kagnn_amd.data existed; the baseline
  (b) DeviceBatchLoader, shuffle=True             -- a fresh batch per step from one kagnn_batch_assemble launch, its CSR index included
  (c) the same with the assembled index withheld  -- the model rebuilds the CSR per batch: isolates what the CSR slices buy
  (d) host collation per step + five .to(device)  -- what a user had to write without the loader, same shuffled order

    python tools/loader_step.py [--epochs 10] [--only b] [--json out.json]

`--only b` runs one variant alone (for a kernel trace of it).  The requirement on (b) is stated in profiles/loader_step.md."""
from __future__ import annotations

import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kagnn_amd                                   # noqa: E402
from kagnn_amd import harness                      # noqa: E402

B, H, G = 256, 64, 10_000


def dataset_arrays(seed=0):
    g = torch.Generator().manual_seed(seed)
    sizes = torch.randint(18, 29, (G,), generator=g)
    esizes = 2 * sizes + 4
    node_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)])
    edge_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(esizes, 0)])
    n, e = int(node_ptr[-1]), int(edge_ptr[-1])
    lo, span = torch.repeat_interleave(node_ptr[:-1], esizes), torch.repeat_interleave(sizes, esizes)
    ei = torch.stack([lo + (torch.rand(e, generator=g) * span).long().clamp(max=span - 1),
                      lo + (torch.rand(e, generator=g) * span).long().clamp(max=span - 1)])
    return SimpleNamespace(x=torch.randint(0, 21, (n, 1), generator=g), edge_index=ei, edge_attr=torch.randint(0, 4, (e,), generator=g),
                           y=torch.randn(G, generator=g), node_ptr=node_ptr, edge_ptr=edge_ptr)


def collate(d, ids):
    """the plain torch restatement of torch_geometric's Batch.from_data_list (host tensors)"""
    ids = ids.tolist()
    sizes = torch.tensor([int(d.node_ptr[g + 1] - d.node_ptr[g]) for g in ids])
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)])
    return SimpleNamespace(
        x=torch.cat([d.x[d.node_ptr[g]:d.node_ptr[g + 1]] for g in ids]),
        edge_index=torch.cat([d.edge_index[:, d.edge_ptr[g]:d.edge_ptr[g + 1]] - d.node_ptr[g] + ptr[k] for k, g in enumerate(ids)], dim=1),
        edge_attr=torch.cat([d.edge_attr[d.edge_ptr[g]:d.edge_ptr[g + 1]] for g in ids]),
        y=torch.cat([d.y[g:g + 1] for g in ids]), batch=torch.repeat_interleave(torch.arange(len(ids)), sizes), ptr=ptr, num_graphs=len(ids))


def to_device(b, dev):
    return SimpleNamespace(x=b.x.to(dev), edge_index=b.edge_index.to(dev), edge_attr=b.edge_attr.to(dev), y=b.y.to(dev), batch=b.batch.to(dev),
                           ptr=b.ptr.to(dev), num_graphs=b.num_graphs)


class HostCollation:
    """(d): a shuffled epoch collated on the host, batch by batch, and copied over -- re-iterable, with len()"""

    def __init__(self, d, dev, steps, generator):
        self.d, self.dev, self.steps, self.generator = d, dev, steps, generator

    def __len__(self):
        return self.steps

    def __iter__(self):
        order = torch.randperm(G, generator=self.generator)
        for k in range(self.steps):
            yield to_device(collate(self.d, order[k * B:(k + 1) * B]), self.dev)


class FirstBatches:
    """the first `steps` batches of every epoch of a loader (so that all four variants time the same number of steps per epoch)"""

    def __init__(self, loader, steps):
        self.loader, self.steps = loader, steps

    def __len__(self):
        return self.steps

    def __iter__(self):
        yield from self.loader.batches_of(self.loader.order()[:self.steps * B])


def model(dev):
    torch.manual_seed(0)
    m = kagnn_amd.KAGINRegression(1, 1, 4, H, 2, 4, 3, 1, 0.0, True)
    m.atom_encoder = kagnn_amd.graph_models.AtomEncoder(H, [21])
    m.bond_encoder.bond_embedding_list = torch.nn.ModuleList([torch.nn.Embedding(4, H)])
    return m.to(dev)


def timed(batches, dev, epochs):
    m = model(dev)
    reps = [harness.train_graph_batches(m, batches, nb_epochs=epochs, warmup=1)[0] * 1e3 for _ in range(3)]
    return {"ms_per_step": sorted(reps)[1], "repeats_ms_per_step": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--steps", type=int, default=8, help="steps per epoch (the bench's premade list has 8 batches)")
    ap.add_argument("--only", choices="abcd")
    ap.add_argument("--json")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    d = dataset_arrays()
    ds = kagnn_amd.DeviceGraphDataset(d.x, d.edge_index, d.node_ptr, edge_attr=d.edge_attr, y=d.y, device=dev)
    variants = {
        "a": lambda: [to_device(collate(d, torch.arange(k * B, (k + 1) * B)), dev) for k in range(args.steps)],
        "b": lambda: FirstBatches(kagnn_amd.DeviceBatchLoader(ds, B, shuffle=True, generator=torch.Generator().manual_seed(1)), args.steps),
        "c": lambda: FirstBatches(kagnn_amd.DeviceBatchLoader(ds, B, shuffle=True, generator=torch.Generator().manual_seed(1),
                                                              attach_graph_index=False), args.steps),
        "d": lambda: HostCollation(d, dev, args.steps, torch.Generator().manual_seed(1)),
    }
    out = {"device": torch.cuda.get_device_name(0), "library_version": kagnn_amd._lib.load().kagnn_version(), "graphs": G, "batch": B,
           "epochs": args.epochs, "steps_per_epoch": args.steps}
    for name, make in variants.items():
        if args.only in (None, name):
            out[name] = timed(make(), dev, args.epochs)
            print(name, json.dumps(out[name]), flush=True)
    if "a" in out and "b" in out:
        spread = max(out["a"]["repeats_ms_per_step"]) - min(out["a"]["repeats_ms_per_step"])
        out["requirement"] = {"b_minus_a_ms": out["b"]["ms_per_step"] - out["a"]["ms_per_step"], "spread_of_a_ms": spread,
                              "met": out["b"]["ms_per_step"] <= out["a"]["ms_per_step"] + spread}
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
