"""The MLP rows beside the KAN rows: ``node_classification_clean/time_model.py:84-106``'s table on synthetic Cora- and
ogbn-arxiv-shaped inputs, and the dense layer under the MLP rows against torch's own.

Models (``--step models-cora`` / ``models-arxiv``): ``GNN_Nodes`` at hidden 4 / 64 / 256 / 1024, ``GKAN_Nodes`` at 16 / 32 / 64 / 128 x
grid 1 / 8 x order 1 / 4, ``GFASTKAN_Nodes`` at 16 / 64 / 256 / 512 x grid 2 / 9; gcn, and gin with 2 and 4 hidden layers -- the script's
loops and widths -- each through ``harness.time_model`` (seconds per epoch, the script's column).  The inputs are random graphs of the
datasets' sizes (2708 nodes / 10556 edges / 1433 features / 7 classes, 2 layers; 169343 / 1166243 / 128 / 40, 3 layers) given as a
plain ``edge_index``.  ``--widths short`` keeps the first and third width of every family.

Dense layer (``--step linear``): per (N, in, out) that these models run, forward + backward of ``ops.linear(x, W, b, relu=True)``
against ``F.relu(F.linear(x, W, b))`` on the same tensors.  Every shape is warmed up first; then the two alternate inside this one
process, each repetition bracketed by device events; the median of ``--repeats`` is reported, with the ratio ours / torch and, where
ours is slower, the bound that applies -- bytes over 6.3 TB/s or flops over 157 TF (fp32 matrix rate), whichever is larger -- and
the share of it the kernels reach.

Without ``--step`` the tool is a driver: it starts one child process per step under that step's own time limit and stops at the
first step that fails or runs out of time, so nothing is started on a device after a fault.

    python tools/mlp_vs_kan_step.py --out results/mlp_vs_kan_step.md
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = [("linear", 240), ("models-cora", 300), ("models-arxiv", 420)]          # (name, time limit in seconds)
SHAPES = {"cora": (2708, 10556, 1433, 7, 2), "arxiv": (169343, 1166243, 128, 40, 3)}
LINEAR_SHAPES = [(2708, 1433, 4), (2708, 1433, 64), (2708, 1433, 1024), (2708, 64, 64), (2708, 1024, 1024), (2708, 1561, 7),
                 (169343, 128, 4), (169343, 128, 64), (169343, 128, 256), (169343, 64, 64), (169343, 256, 256), (169343, 1024, 1024),
                 (169343, 320, 40)]
HBM_BYTES_PER_S, FP32_MFMA_FLOPS = 6.3e12, 157e12


def linear_bounds(n, fin, fout):
    """lower bounds of forward + both gradients: every operand read or written once per kernel; 3 products of 2 n in out flops"""
    fwd = n * fin + fout * fin + fout + n * fout
    dx = 2 * n * fout + fout * fin + n * fin                  # gy, y (mask), W -> gx
    dw = n * fin + 2 * n * fout + fout * fin + fout           # x, gy, y -> gW, gb
    return 4.0 * (fwd + dx + dw) / HBM_BYTES_PER_S, 6.0 * n * fin * fout / FP32_MFMA_FLOPS


def step_linear(args, emit):
    import torch
    import torch.nn.functional as F
    from kagnn_amd import ops
    dev = "cuda:0"
    forms = {"ours": lambda x, w, b: ops.linear(x, w, b, relu=True), "torch": lambda x, w, b: F.relu(F.linear(x, w, b))}
    cases = []
    for n, fin, fout in LINEAR_SHAPES:
        g = torch.Generator().manual_seed(n + fin + fout)
        x = torch.randn(n, fin, generator=g).to(dev).requires_grad_(True)
        w = (torch.randn(fout, fin, generator=g) / fin ** 0.5).to(dev).requires_grad_(True)
        b = torch.randn(fout, generator=g).to(dev).requires_grad_(True)
        gy = torch.randn(n, fout, generator=g).to(dev)
        cases.append((x, w, b, gy))

    def once(form, case):
        x, w, b, gy = case
        x.grad = w.grad = b.grad = None
        forms[form](x, w, b).backward(gy)

    for case in cases:                                        # warm-up of every shape, both forms
        for form in forms:
            for _ in range(3):
                once(form, case)
    torch.cuda.synchronize()
    emit("| N | in | out | ours ms | torch ms | ours / torch | bound (where slower) | share of the bound |")
    emit("|---|---|---|---|---|---|---|---|")
    for (n, fin, fout), case in zip(LINEAR_SHAPES, cases):
        times = {f: [] for f in forms}
        for _ in range(args.repeats):
            for form in forms:                                # the two alternate
                a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                once(form, case)
                z.record()
                z.synchronize()
                times[form].append(a.elapsed_time(z))
        ours, ref = statistics.median(times["ours"]), statistics.median(times["torch"])
        bound, share = "", ""
        if ours > ref:
            tb, tf = linear_bounds(n, fin, fout)
            bound = f"bytes / 6.3 TB/s = {tb * 1e3:.4f} ms" if tb >= tf else f"flops / 157 TF = {tf * 1e3:.4f} ms"
            share = f"{100.0 * max(tb, tf) * 1e3 / ours:.1f} %"
        emit(f"| {n} | {fin} | {fout} | {ours:.4f} | {ref:.4f} | {ours / ref:.2f} | {bound} | {share} |")


def step_models(name, args, emit):
    import torch
    import kagnn_amd
    from kagnn_amd import harness
    dev = "cuda:0"
    n, e, f, c, layers = SHAPES[name]
    g = torch.Generator().manual_seed(0)
    x = torch.randn(n, f, generator=g).to(dev)
    ei = torch.randint(0, n, (2, e), generator=g).to(dev)
    y = torch.randint(0, c, (n,), generator=g).to(dev)
    mask = (torch.rand(n, generator=g) < 0.5).to(dev)
    pick = (lambda ws: ws) if args.widths == "full" else (lambda ws: ws[::2])
    emit(f"| model ({name}) | conv | hidden | hidden layers | grid | order | parameters | s / epoch |")
    emit("|---|---|---|---|---|---|---|---|")

    def row(label, model, conv, hidden, hl, grid, order):
        model = model.to(dev)
        t, _ = harness.time_model(model, x, ei, y, mask, nb_epochs=args.epochs, warmup=2)
        emit(f"| {label} | {conv} | {hidden} | {hl or 'NA'} | {grid} | {order} | {harness.count_params(model)} | {t:.6f} |")

    for conv in ("gcn", "gin"):
        hiddens = [2, 4] if conv == "gin" else [0]
        for h in pick([4, 64, 256, 1024]):
            for hl in hiddens:
                row("GNN_Nodes", kagnn_amd.GNN_Nodes(conv, layers, f, h, c, skip=True, hidden_layers=hl, dropout=0), conv, h, hl, "NA", "NA")
        for h in pick([16, 32, 64, 128]):
            for hl in hiddens:
                for grid in (1, 8):
                    for order in (1, 4):
                        row("GKAN_Nodes", kagnn_amd.GKAN_Nodes(conv, layers, f, h, c, skip=True, hidden_layers=hl, grid_size=grid,
                                                               spline_order=order, dropout=0), conv, h, hl, grid, order)
        for h in pick([16, 64, 256, 512]):
            for hl in hiddens:
                for grid in (2, 9):
                    row("GFASTKAN_Nodes", kagnn_amd.GFASTKAN_Nodes(conv, layers, f, h, c, skip=True, hidden_layers=hl, grid_size=grid,
                                                                   dropout=0), conv, h, hl, grid - 1, "NA")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=[s for s, _ in STEPS])
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--widths", choices=["full", "short"], default="full")
    ap.add_argument("--out", help="also append the tables to this file")
    args = ap.parse_args()
    if args.step is None:
        if args.out and os.path.exists(args.out):
            os.remove(args.out)
        for name, limit in STEPS:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--repeats", str(args.repeats), "--epochs", str(args.epochs),
                   "--widths", args.widths] + (["--out", args.out] if args.out else [])
            try:
                rc = subprocess.run(cmd, timeout=limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print(f"step {name} ended with status {rc}: stopping here", file=sys.stderr, flush=True)
                return rc
        return 0

    def emit(line):
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    emit(f"\n### {args.step}\n")
    if args.step == "linear":
        step_linear(args, emit)
    else:
        step_models(args.step.split("-")[1], args, emit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
