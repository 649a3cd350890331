"""The graph-classification workflow on the device (reference ``graph_classification/graph_classification_utils.py``): the ``Degree``
node features (``kagnn_degree_one_hot``), ``F.nll_loss`` with the epoch's meter (``kagnn_nll_loss_fwd`` / ``_bwd``,
``ops.ClassificationMeter``) and the train / val / test loops of ``kagnn_amd.harness`` -- each against the plain torch statement of
what the reference's script does, written out here.  Bounds: one-hot rows, accuracy counts and the script-form trajectories are exact
(nothing rounds); sums of fp32 addends accumulated in fp64 are held to 1e-12 relative; figures rounded once to fp32 to one fp32
ulp; parameter gradients to the 2e-4 that ``test_gpu_parity.py::test_graph_classification_models_golden`` holds the same models to."""
import copy
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kagnn_amd
from kagnn_amd import _lib, data, harness, ops
from oracle import kan_oracle as orc
from helpers import assert_close, must_fail
from test_gpu_data import _graphs, _tu, collate
from test_gpu_poison import _GuardedEmpty

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LIMIT = _lib.BATCH_MAX_GRAPHS


# ------------------------------------------------------------------------------------------------ Degree
def _degree_restated(edge_index, n, k):
    return F.one_hot(torch.clip(torch.bincount(edge_index[0], minlength=n), 0, k - 1), k).float()


def _degree_graph():
    """directed: node 0 -> 35 others (out-degree exactly 35), node 40 -> 36 others, node 100 -> 200 others (with repeats of an edge
    counted as edges), a cycle 300 -> 301 -> 302 -> 300, a sink (node 1: in-degree 3, out-degree 0) and isolated nodes (303 .. 319)"""
    src = [0] * 35 + [40] * 36 + [100] * 200 + [300, 301, 302]
    dst = list(range(1, 36)) + list(range(41, 77)) + [1] + list(range(101, 300)) + [301, 302, 300]
    ei = torch.tensor([src, dst], dtype=torch.int64)
    n = 320
    out_deg, in_deg = torch.bincount(ei[0], minlength=n), torch.bincount(ei[1], minlength=n)
    assert int(out_deg[0]) == 35 and int(out_deg[40]) == 36 and int(out_deg[100]) == 200 and int(out_deg[310]) == 0 == int(in_deg[310])
    assert not torch.equal(out_deg, in_deg)                        # picking the by-destination CSR gives another answer
    return ei[:, torch.randperm(ei.size(1), generator=torch.Generator().manual_seed(3))], n


@pytest.mark.parametrize("k", [36, 5])
def test_degree_one_hot_equals_the_restatement(k):
    ei, n = _degree_graph()
    want = _degree_restated(ei, n, k)
    assert not torch.equal(want, _degree_restated(ei.flip(0), n, k))
    eid = ei.to(DEV)
    got = ops.degree_one_hot(eid, n, k)
    assert got.dtype == torch.float32 and got.shape == (n, k) and torch.equal(got.cpu(), want)
    assert torch.equal(ops.degree_one_hot(ops.GraphIndex(eid, n), n, k).cpu(), want)
    # no edges: every row has its 1 in column 0
    none = ops.degree_one_hot(eid[:, :0], 7, k)
    assert torch.equal(none.cpu(), _degree_restated(ei[:, :0], 7, k)) and float(none[:, 0].sum()) == 7.0
    # a row stride larger than the row, from an unaligned base: the columns between the rows are not touched
    buf = torch.full((n * (k + 3) + 1,), -7.0, device=DEV)
    x = buf[1:].view(n, k + 3)
    gi = ops.GraphIndex(eid, n)
    ops._call("kagnn_degree_one_hot", ops._ptr(gi.rowptr_t), n, k, ops._ptr(x), k + 3, ops._stream())
    assert torch.equal(x[:, :k].cpu(), want) and bool((x[:, k:] == -7.0).all()) and float(buf[0]) == -7.0
    if k == 36:
        assert torch.equal(ops.degree_one_hot(eid, n).cpu(), want)             # the reference's 36 is the default


def _unlabeled(seed=6, G=45):
    sizes = torch.randint(1, 40, (G,), generator=torch.Generator().manual_seed(seed))
    return _graphs(seed, sizes, lambda n, k: 3 * n + (k % 5), lambda N, g: None, None, lambda G_, g: torch.randint(0, 3, (G_,), generator=g))


@pytest.mark.parametrize("k", [36, 5])
def test_degree_featured_dataset_yields_the_restatement(k):
    d = _unlabeled()
    ds = kagnn_amd.DeviceGraphDataset(None, d.edge_index, d.node_ptr, y=d.y, device=DEV, degree_features=k)
    assert ds.num_node_features == k and ds.num_features == k and ds.num_classes == 3
    d.x = _degree_restated(d.edge_index, int(d.node_ptr[-1]), k)            # graphs are disjoint: per-graph degrees = the dataset's
    assert torch.equal(ds.storage.x.cpu(), d.x)
    loader = kagnn_amd.DeviceBatchLoader(ds[torch.arange(d.G - 1, -1, -1)], 7)
    ids = torch.arange(d.G - 1, -1, -1)
    for b_i, b in enumerate(loader):
        ref = collate(d.x, d.edge_index, d.node_ptr, d.edge_ptr, ids[7 * b_i:7 * b_i + 7], None, d.y)
        assert b.x.dtype == torch.float32 and torch.equal(b.x.cpu(), ref["x"]) and torch.equal(b.y.cpu(), ref["y"])
        # ... which is the transform applied to each graph of the batch on its own
        assert torch.equal(b.x.cpu(), _degree_restated(ref["edge_index"], b.num_nodes, k))
    ops.flush_graph_checks()
    graphs = [SimpleNamespace(num_nodes=int(d.node_ptr[g + 1] - d.node_ptr[g]), x=None, y=d.y[g:g + 1],
                              edge_index=d.edge_index[:, d.edge_ptr[g]:d.edge_ptr[g + 1]] - d.node_ptr[g]) for g in range(d.G)]
    ds2 = kagnn_amd.DeviceGraphDataset.from_graphs(graphs, device=DEV, degree_features=k)
    assert len(ds2) == d.G and ds2.num_node_features == k and torch.equal(ds2.storage.x, ds.storage.x)
    # a dataset without a single edge
    ds0 = kagnn_amd.DeviceGraphDataset(None, torch.zeros(2, 0, dtype=torch.int64), [0, 3, 4, 9], y=torch.tensor([0, 1, 0]), device=DEV,
                                       degree_features=k)
    (b0,) = list(kagnn_amd.DeviceBatchLoader(ds0, 3))
    assert b0.x.shape == (9, k) and torch.equal(b0.x.cpu(), F.one_hot(torch.zeros(9, dtype=torch.int64), k).float())
    with pytest.raises(ValueError):
        kagnn_amd.DeviceGraphDataset(None, d.edge_index, d.node_ptr, device=DEV)
    with pytest.raises(ValueError):
        kagnn_amd.DeviceGraphDataset(d.x, d.edge_index, d.node_ptr, device=DEV, degree_features=k)


# ------------------------------------------------------------------------------------------------ nll_loss forward
def _logp(b, c, seed, ld_extra=0):
    g = torch.Generator().manual_seed(seed)
    z = torch.log_softmax(torch.randn(b, c + ld_extra, generator=g) * 2.0, 1)
    y = torch.randint(0, c, (b,), generator=g)
    return z, y


def _ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def _check_forward(z_host, y_host, z_dev, what):
    b = z_host.size(0)
    want = float((-z_host.double()[torch.arange(b), y_host]).sum())
    meter = ops.ClassificationMeter(DEV)
    yd = y_host.to(DEV)
    mean = ops.nll_loss(z_dev, yd, accumulate=meter)
    total = ops.nll_loss(z_dev, yd, reduction="sum")
    nll_sum, correct, graphs = meter.read()
    print(f"{what}: nll_sum {nll_sum!r} want {want!r} mean {float(mean)!r} sum {float(total)!r}")
    assert graphs == b and mean.shape == () and total.shape == () and mean.dtype == torch.float32
    assert abs(nll_sum - want) <= 1e-12 * abs(want), (what, nll_sum, want)
    assert float(total) == float(np.float32(nll_sum)), (what, "loss_sum is the fp64 sum rounded once")
    assert abs(float(total) - want) <= _ulp32(want), what
    if b:
        assert float(mean) == float(np.float32(nll_sum / b)), (what, "loss_mean is sum / B rounded once")
        assert abs(float(mean) - want / b) <= _ulp32(want / b), what
    assert correct == int((z_host.argmax(1) == y_host).sum()), what
    return meter


@pytest.mark.parametrize("c", [2, 3, 6, 64, 65, 300])
@pytest.mark.parametrize("b", [1, 2, 255, 256, LIMIT, LIMIT + 37])
def test_nll_loss_forward_against_fp64(b, c):
    z, y = _logp(b, c, seed=b * 1000 + c)
    _check_forward(z, y, z.to(DEV), f"B={b} C={c}")


@pytest.mark.parametrize("b,c", [(1, 2), (255, 3), (256, 6), (LIMIT + 37, 65)])
def test_nll_loss_forward_on_a_column_slice(b, c):
    wide, y = _logp(b, c, seed=b + c, ld_extra=5)
    zd = wide.to(DEV)[:, 2:2 + c]
    assert zd.stride(0) == c + 5
    _check_forward(wide[:, 2:2 + c], y, zd, f"slice B={b} C={c}")
    ops.flush_graph_checks()


def test_nll_loss_of_no_rows():
    meter = ops.ClassificationMeter(DEV)
    z, y = torch.empty(0, 4, device=DEV), torch.empty(0, dtype=torch.int64, device=DEV)
    mean, total = ops.nll_loss(z, y, accumulate=meter), ops.nll_loss(z, y, reduction="sum")
    assert bool(torch.isnan(mean)) and float(total) == 0.0
    assert meter.read() == (0.0, 0, 0)
    ops.flush_graph_checks()


# ------------------------------------------------------------------------------------------------ accuracy and the meter
@pytest.mark.parametrize("c", [2, 6, 65, 300])
def test_correct_counts_the_arg_max(c):
    b = 1000
    g = torch.Generator().manual_seed(c)
    z = torch.log_softmax(torch.randn(b, c, generator=g), 1)
    assert all(int((z[r] == z[r].max()).sum()) == 1 for r in range(b))          # no ties
    y = torch.where(torch.rand(b, generator=g) < 0.5, z.argmax(1), torch.randint(0, c, (b,), generator=g))
    meter = ops.ClassificationMeter(DEV)
    ops.nll_loss(z.to(DEV), y.to(DEV), accumulate=meter)
    want = int((z.argmax(1) == y).sum())
    assert 0 < want < b and meter.read()[1:] == (want, b)


def _correct_of(rows, labels):
    meter = ops.ClassificationMeter(DEV)
    ops.nll_loss(torch.tensor(rows, dtype=torch.float32, device=DEV), torch.tensor(labels, device=DEV), reduction="sum", accumulate=meter)
    return meter.read()[1]


def test_ties_go_to_the_lowest_index_and_nan_rows_are_wrong():
    tie = [-1.0, -1.0, -3.0]
    assert _correct_of([tie], [0]) == 1 and _correct_of([tie], [1]) == 0 and _correct_of([tie, tie, tie], [0, 1, 0]) == 2
    assert _correct_of([[-3.0, -1.0, -1.0]], [1]) == 1 and _correct_of([[-3.0, -1.0, -1.0]], [2]) == 0
    wide = torch.full((4, 300), -9.0)
    wide[0, 3] = wide[0, 200] = -0.5           # two lanes of the row's group
    wide[1, 5] = wide[1, 69] = -0.5            # the same lane, 64 columns apart
    wide[2, 299] = -0.5                        # the last column alone
    wide[3, :] = float("-inf")                 # all equal: index 0
    for labels, want in (([3, 5, 299, 0], 4), ([200, 69, 299, 0], 2), ([3, 69, 0, 1], 1)):
        assert _correct_of(wide.tolist(), labels) == want, labels
    nan = float("nan")
    assert _correct_of([[-0.1, -5.0, nan]], [0]) == 0 and _correct_of([[-0.1, nan, -5.0], [-0.1, -4.0, -5.0]], [0, 0]) == 1
    big = torch.full((2, 300), -9.0)
    big[:, 7] = -0.1
    big[0, 250] = nan
    assert _correct_of(big.tolist(), [7, 7]) == 1
    ops.flush_graph_checks()


def test_the_meter_accumulates_over_batches_and_resets():
    meter = ops.ClassificationMeter(DEV)
    want_sum, want_correct, want_graphs = 0.0, 0, 0
    for k, b in enumerate([1, 64, 3, 255, 256, LIMIT, 37]):
        z, y = _logp(b, 6, seed=70 + k)
        y = torch.where(torch.arange(b) % 3 == 0, z.argmax(1), y)
        ops.nll_loss(z.to(DEV), y.to(DEV), reduction="sum" if k % 2 else "mean", accumulate=meter)
        want_sum += float((-z.double()[torch.arange(b), y]).sum())
        want_correct += int((z.argmax(1) == y).sum())
        want_graphs += b
    nll_sum, correct, graphs = meter.read()
    print(f"meter over 7 batches: nll_sum {nll_sum!r} want {want_sum!r}")
    assert isinstance(correct, int) and isinstance(graphs, int) and isinstance(nll_sum, float)
    assert (correct, graphs) == (want_correct, want_graphs) and abs(nll_sum - want_sum) <= 1e-12 * abs(want_sum)
    meter.reset()
    assert meter.read() == (0.0, 0, 0)
    ops.flush_graph_checks()


# ------------------------------------------------------------------------------------------------ nll_loss backward
@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("b,c", [(255, 6), (1, 2), (LIMIT + 37, 65)])
def test_nll_loss_backward(reduction, b, c):
    z, y = _logp(b, c, seed=b + 7 * c)
    up = 0.37
    zd = z.to(DEV).requires_grad_(True)
    (ops.nll_loss(zd, y.to(DEV), reduction=reduction) * up).backward()
    g = zd.grad.cpu()
    on = F.one_hot(y, c).bool()
    assert g.shape == (b, c) and bool((g[~on] == 0.0).all())                # EXACTLY zero off the label
    z64 = z.double().requires_grad_(True)
    (F.nll_loss(z64, y, reduction=reduction) * up).backward()
    want = z64.grad[on]
    assert_close(g[on], want, what=f"nll_loss backward {reduction} B={b} C={c}")
    # mutation guard: rows + 1 in the divisor has to fail the same assertion
    must_fail(g[on] * (b / (b + 1.0)), want, what=f"nll_loss backward {reduction} B={b} C={c}")
    # the default root gradient (1) too
    zd.grad = None
    ops.nll_loss(zd, y.to(DEV), reduction=reduction).backward()
    assert_close(zd.grad.cpu()[on], want / up, what=f"nll_loss backward {reduction}, unit upstream")
    ops.flush_graph_checks()


# ------------------------------------------------------------------------------------------------ bad labels
@pytest.mark.parametrize("bad", ["C", "-1"])
def test_a_label_outside_the_classes_is_reported_not_executed(monkeypatch, bad):
    c, b = 5, 40
    ops.flush_graph_checks()
    z, _ = _logp(b, c, seed=11)
    wrong = (z.argmax(1) + 1) % c                                   # every row's label is NOT its arg-max ...
    y = wrong.clone()
    y[17] = c if bad == "C" else -1                                 # ... and row 17's is outside [0, C)
    meter = ops.ClassificationMeter(DEV)
    ops.nll_loss(z.to(DEV), z.argmax(1).to(DEV), accumulate=meter)  # a good batch first: 40 correct
    before = meter.read()
    assert before[1:] == (b, b)
    guarded = _GuardedEmpty()
    monkeypatch.setattr(torch, "empty", guarded)
    zd = z.to(DEV).requires_grad_(True)
    loss = ops.nll_loss(zd, y.to(DEV), accumulate=meter)
    total = ops.nll_loss(zd, y.to(DEV), reduction="sum")
    (loss + total).backward()
    assert guarded.check("nll_loss with a bad label") >= 4          # both losses and both gradient blocks sit between intact bands
    monkeypatch.undo()
    assert bool(torch.isnan(loss)) and bool(torch.isnan(total))
    after = meter.read()
    assert after[1] == before[1] and after[2] == 2 * b              # `correct` unchanged
    g = zd.grad.cpu()
    assert bool((g[17] == 0.0).all()) and bool(torch.isfinite(g).all())
    assert bool((g[torch.arange(b) != 17].sum(1) < 0).all())        # the other rows still got their gradient
    with pytest.raises(RuntimeError, match="kagnn_nll_loss_fwd"):
        ops.flush_graph_checks()
    ops.flush_graph_checks()                                        # reported once; the flag starts clean again
    ok = ops.nll_loss(z.to(DEV), wrong.to(DEV))
    ops.flush_graph_checks()
    assert bool(torch.isfinite(ok))


# ------------------------------------------------------------------------------------------------ the loops
def _tu_dataset(G=100, seed=51):
    d = _tu(G=G, seed=seed)
    return d, kagnn_amd.DeviceGraphDataset(d.x, d.edge_index, d.node_ptr, y=d.y, device=DEV)


def _model(name):
    torch.manual_seed(5)
    if name == "KAGIN":
        return kagnn_amd.KAGIN(2, 7, 32, 2, 2, 4, 3, 0.0)
    return kagnn_amd.KAGCN(2, 7, 32, 2, 4, 3, 0.0)


def _reference_train(model, loader, optimizer, device):
    """graph_classification_utils.py:45-55"""
    model.train()
    loss_all = 0
    for batch in loader:
        batch = batch.to(device)
        loss = F.nll_loss(model(batch), batch.y)
        optimizer.zero_grad()
        loss.backward()
        loss_all += batch.num_graphs * loss.item()
        optimizer.step()
    return loss_all / len(loader.dataset)


def _reference_val(model, loader, device):
    """:57-63"""
    model.eval()
    loss_all = 0
    for batch in loader:
        batch = batch.to(device)
        loss_all += F.nll_loss(model(batch), batch.y, reduction='sum').item()
    return loss_all / len(loader.dataset)


def _reference_test(model, loader, device):
    """:65-72"""
    model.eval()
    correct = 0
    for batch in loader:
        batch = batch.to(device)
        pred = model(batch).max(1)[1]
        correct += pred.eq(batch.y).sum().item()
    return correct / len(loader.dataset)


def _loader(ds, seed=3, batch_size=32):
    return kagnn_amd.DeviceBatchLoader(ds, batch_size, shuffle=True, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("name", ["KAGIN", "KAGCN"])
def test_training_with_the_scripts_loss_and_optimiser_is_the_script_bit_for_bit(name):
    _d, ds = _tu_dataset()
    ma = _model(name).to(DEV)
    mb = copy.deepcopy(ma)
    _t, losses = harness.train_graph_classification(ma, _loader(ds), nb_epochs=2, loss_fn=F.nll_loss,
                                                    optimizer=torch.optim.Adam(ma.parameters(), lr=1e-3, fused=True))
    opt, loader_b = torch.optim.Adam(mb.parameters(), lr=1e-3, fused=True), _loader(ds)
    want = [_reference_train(mb, loader_b, opt, DEV) for _ in range(2)]
    ops.flush_graph_checks()
    for (pname, pa), pb in zip(ma.named_parameters(), mb.parameters()):
        assert torch.equal(pa, pb), pname
    for ba, bb in zip(ma.buffers(), mb.buffers()):
        assert torch.equal(ba, bb)
    print(f"{name}: epoch losses {losses} script {want}")
    assert len(losses) == 2 and all(abs(a - w) <= 1e-6 * abs(w) for a, w in zip(losses, want)) and ma.training


def _oracle_state(model):
    frozen = ("grid", "rbf.grid", "eps", "running_mean", "running_var", "num_batches_tracked")
    return {k: (v.detach().cpu().double().requires_grad_(True) if v.is_floating_point() and not k.endswith(frozen)
                else v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in model.state_dict().items()}


@pytest.mark.parametrize("name,family", [("KAGIN", "gin"), ("KAGCN", "gcn")])
def test_first_step_gradients_of_the_native_loss_against_the_fp64_oracle(name, family):
    """the default loop (``ops.nll_loss`` + ``harness.Adam``): after one step on one batch every ``p.grad`` is the gradient at the
    INITIAL parameters; truth = ``oracle.kan_oracle.graph_classification_forward`` (the one fixture G13 is checked with) + ``F.nll_loss``
    in fp64; bound = the 2e-4 of ``test_gpu_parity.py::test_graph_classification_models_golden`` for parameter gradients"""
    sizes = torch.randint(5, 60, (48,), generator=torch.Generator().manual_seed(8))
    d = _graphs(8, sizes, lambda n, k: 2 * n, lambda N, g: torch.randn(N, 7, generator=g), None,
                lambda G_, g: torch.randint(0, 2, (G_,), generator=g))
    ds = kagnn_amd.DeviceGraphDataset(d.x, d.edge_index, d.node_ptr, y=d.y, device=DEV)
    (batch,) = list(kagnn_amd.DeviceBatchLoader(ds, 48))
    m = _model(name)
    st = _oracle_state(m)
    m = m.to(DEV)
    _t, (loss,) = harness.train_graph_classification(m, [batch], nb_epochs=1)
    out64 = orc.graph_classification_forward(d.x.double(), d.edge_index, torch.repeat_interleave(torch.arange(48), sizes), 48, st, "kan",
                                             family, 2)
    loss64 = F.nll_loss(out64, d.y)
    loss64.backward()
    print(f"{name}: loss {loss!r} fp64 {float(loss64)!r}")
    assert_close(torch.tensor(loss), loss64.detach(), 5e-5, what=f"{name} native training loss")
    checked = 0
    for pname, p in m.named_parameters():
        if not p.requires_grad:
            continue
        assert p.grad is not None and st[pname].grad is not None, pname
        assert_close(p.grad, st[pname].grad, 2e-4, what=f"{name} first-step grad {pname}")
        checked += 1
    assert checked >= 8
    first = next(n for n, p in m.named_parameters() if p.requires_grad)
    must_fail(torch.zeros_like(st[first].grad), st[first].grad, 2e-4, what=f"{name} first-step grad {first}")


def test_evaluation_equals_val_and_test_of_the_script_on_read_splits_views(tmp_path):
    d, ds = _tu_dataset(G=120, seed=52)
    perm = torch.randperm(120, generator=torch.Generator().manual_seed(1)).tolist()
    folds = [{"test": perm[:33], "model_selection": [{"train": perm[33:100], "validation": perm[100:]}]},
             {"test": perm[5:6], "model_selection": [{"train": perm[:5], "validation": perm[6:40]}]}]
    path = tmp_path / "TU_splits.json"
    path.write_text(json.dumps(folds))
    splits = data.read_splits(str(path))
    m = _model("KAGIN").to(DEV)
    train, val, test = splits[0]
    harness.train_graph_classification(m, _loader(ds[train], batch_size=16), nb_epochs=2)
    for idx, what in ((val, "validation: 16 + 4"), (test, "test: 16 + 16 + 1"), (splits[1][2], "one graph"), (splits[1][1], "34 graphs")):
        view = ds[idx]
        assert len(view) == idx.numel()
        loader = kagnn_amd.DeviceBatchLoader(view, 16)
        nll, acc = harness.evaluate_graph_classification(m, loader)
        assert not m.training
        want_nll, want_acc = _reference_val(m, loader, DEV), _reference_test(m, loader, DEV)
        print(f"{what}: nll {nll!r} script {want_nll!r}; accuracy {acc!r} script {want_acc!r}")
        assert acc == want_acc and abs(nll - want_nll) <= 1e-6 * abs(want_nll), what
    assert len(kagnn_amd.DeviceBatchLoader(ds[test], 16)) == 3 and test.numel() % 16 == 1


# ------------------------------------------------------------------------------------------------ read-backs
class _ReadBacks:
    """counts what brings a DEVICE tensor's value to the host -- ``item / tolist / cpu / numpy / to(cpu) / float() / int() /
    bool()`` -- and every explicit wait (``torch.cuda.synchronize``, ``Event.synchronize``), tagged with the phase the loop is in"""

    def __init__(self, monkeypatch):
        self.phase, self.reads, self.waits = "outside", [], []
        for name in ("item", "tolist", "cpu", "numpy", "__float__", "__int__", "__bool__", "__index__"):
            self._wrap(monkeypatch, name)
        real_to = torch.Tensor.to

        def to(t, *a, **kw):
            out = real_to(t, *a, **kw)
            if t.is_cuda and not out.is_cuda:
                self.reads.append((self.phase, "to"))
            return out
        monkeypatch.setattr(torch.Tensor, "to", to)
        real_sync, real_ev = torch.cuda.synchronize, torch.cuda.Event.synchronize

        def sync(*a, **kw):
            self.waits.append((self.phase, "synchronize"))
            return real_sync(*a, **kw)

        def ev_sync(ev):
            self.waits.append((self.phase, "Event.synchronize"))
            return real_ev(ev)
        monkeypatch.setattr(torch.cuda, "synchronize", sync)
        monkeypatch.setattr(torch.cuda.Event, "synchronize", ev_sync)

    def _wrap(self, monkeypatch, name):
        real = getattr(torch.Tensor, name)

        def counted(t, *a, **kw):
            if t.is_cuda:
                self.reads.append((self.phase, name))
            return real(t, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, counted)

    def loop(self, loader):
        """``loader`` with the phase set to 'loop' from the first batch until the iterator is exhausted"""
        outer = self

        class Tagged:
            dataset = loader.dataset

            def __len__(self):
                return len(loader)

            def __iter__(self):
                outer.phase = "loop"
                try:
                    yield from loader
                finally:
                    outer.phase = "after"
        return Tagged()

    def during(self, phase):
        return [r for r in self.reads if r[0] == phase], [w for w in self.waits if w[0] == phase]


def test_no_read_back_inside_the_loops(monkeypatch):
    _d, ds = _tu_dataset(G=100, seed=53)
    m = _model("KAGIN").to(DEV)
    harness.train_graph_classification(m, _loader(ds), nb_epochs=1)           # (first use: packs, allocator)
    torch.cuda.synchronize()
    # teeth: the script's own loop reads once per batch, and the counter sees it
    rb = _ReadBacks(monkeypatch)
    script = copy.deepcopy(m)
    _reference_train(script, rb.loop(_loader(ds)), torch.optim.Adam(script.parameters(), fused=True), DEV)
    assert [r[1] for r in rb.during("loop")[0]].count("item") == 4            # 100 graphs / 32: four batches, four .item()
    monkeypatch.undo()

    rb = _ReadBacks(monkeypatch)
    harness.train_graph_classification(m, rb.loop(_loader(ds)), nb_epochs=1)
    reads, waits = rb.during("loop")
    assert reads == [] and waits == [], (reads, waits)
    assert [r[1] for r in rb.during("after")[0]] == ["cpu"]                   # the meter, once per epoch
    monkeypatch.undo()

    rb = _ReadBacks(monkeypatch)
    harness.evaluate_graph_classification(m, rb.loop(kagnn_amd.DeviceBatchLoader(ds, 32)))
    reads, waits = rb.during("loop")
    assert reads == [] and waits == [], (reads, waits)
    assert [r[1] for r in rb.during("after")[0]] == ["cpu"]
    monkeypatch.undo()


# ------------------------------------------------------------------------------------------------ reproducibility
def test_two_runs_from_the_same_state_give_the_same_bits():
    _d, ds = _tu_dataset(G=100, seed=54)
    m0 = _model("KAGIN").to(DEV)
    runs = []
    for _ in range(2):
        m = copy.deepcopy(m0)
        _t, losses = harness.train_graph_classification(m, _loader(ds), nb_epochs=2)
        meter = ops.ClassificationMeter(DEV)
        m.eval()
        with torch.no_grad():
            for b in kagnn_amd.DeviceBatchLoader(ds, 32):
                ops.nll_loss(m(b), b.y, reduction="sum", accumulate=meter)
        ops.flush_graph_checks()
        runs.append((losses, [p.detach().clone() for p in m.parameters()] + [b.detach().clone() for b in m.buffers()], meter.read(),
                     harness.evaluate_graph_classification(m, kagnn_amd.DeviceBatchLoader(ds, 32))))
    (la, pa, ma_, ea), (lb, pb, mb_, eb) = runs
    assert la == lb and all(l == l for l in la) and ma_ == mb_ and ea == eb and ma_[2] == 100
    assert all(torch.equal(a, b) for a, b in zip(pa, pb))
    assert ea == (ma_[0] / 100, ma_[1] / 100)
