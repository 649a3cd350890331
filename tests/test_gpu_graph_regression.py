"""The graph-regression experiment on the device (reference ``graph_regression/optuna_zinc.py:38-92``, ``optuna_qm9.py:38-96``:
``train_model_with_parameters``; ``graph_regression/utils.py``: ``EarlyStopper``): ``kagnn_l1_loss_meter_fwd``,
``kagnn_regression_epoch_update`` and the loop of ``kagnn_amd.harness`` built on them -- each against the plain statement of what the
scripts do, written out here.

Bounds.  The meter's terms are the bits of torch's fp32 elementwise results (every operation rounded on its own), so a column sum is
held to 1e-12 relative of those terms added in fp64 -- two fp64 summation orders over at most 1025 terms differ by at most
``rows x 2^-53`` = 1.2e-13.  ``loss_mean`` is that fp64 mean rounded once: 1.2e-7 relative (one fp32 ulp).  The stopper's record, the
history, accumulation, the gradient and the script-form parameter trajectory are exact.  The script's epoch figures are fp32 means
per batch weighted on the host (ZINC) or fp32 column sums (QM9) against fp64 sums here: 1e-6 relative."""
import copy
import math

import numpy as np
import pytest
import torch

import kagnn_amd
from kagnn_amd import harness, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAXT = 32


# ------------------------------------------------------------------------------------------------ the meter
def _operands(rows, targets, seed, extra=0):
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn(rows, targets + extra, generator=g) * 2.0
    t = torch.randn(rows, targets, generator=g)
    s = torch.rand(targets, generator=g) * 3.0 + 0.1
    return buf, buf[:, :targets], t, s


def _terms(p, t, s=None):
    """the fp32 terms as torch's CPU elementwise kernels round them"""
    return (p - t).abs() if s is None else (t * s - p * s).abs() / s


def _launch(buf, targets, t, s=None, meter=None):
    pd = buf.to(DEV)[:, :targets]
    assert buf.size(1) == targets or (pd.stride(0) == buf.size(1) and (pd.size(0) == 1 or not pd.is_contiguous()))
    meter = ops.RegressionMeter(targets, DEV) if meter is None else meter
    loss = ops.l1_loss(pd, t.to(DEV), accumulate=meter, scale=None if s is None else s.to(DEV))
    return loss, meter


@pytest.mark.parametrize("rows", [1, 255, 256, 257, 1025])
@pytest.mark.parametrize("targets", [1, 12, 32])
def test_meter_against_torch_terms_summed_in_fp64(targets, rows):
    for extra in (0, 5):                                                 # contiguous, and a column slice of a wider buffer (ldp > targets)
        buf, p, t, s = _operands(rows, targets, 100 * targets + rows, extra)
        for scale in (None, s):
            terms = _terms(p, t, scale)
            assert terms.dtype == torch.float32
            want = terms.double().sum(0)
            want_mean = float(terms.double().sum()) / (rows * targets)
            loss, meter = _launch(buf, targets, t, scale)
            got, graphs = meter.read()
            rel = ((got - want).abs() / want.abs()).max().item()
            lrel = abs(float(loss) - want_mean) / abs(want_mean)
            print(f"T={targets} rows={rows} extra={extra} scale={scale is not None}: abs_sum rel {rel:.3e}, loss_mean rel {lrel:.3e}")
            assert got.dtype == torch.float64 and got.shape == (targets,) and graphs == rows
            assert rel <= 1e-12
            assert loss.shape == () and loss.dtype == torch.float32 and lrel <= 1.2e-7
            assert int(meter.record[1]) == targets
            # the [B] form of one target is the [B, 1] form
            if targets == 1 and extra == 0:
                meter1 = ops.RegressionMeter(1, DEV)
                loss1 = ops.l1_loss(p[:, 0].to(DEV), t[:, 0].to(DEV), accumulate=meter1, scale=None if scale is None else scale.to(DEV))
                assert torch.equal(loss1, loss) and torch.equal(meter1.record, meter.record)
    # without a meter (a scale alone) the mean is the same number
    only = ops.l1_loss(p.to(DEV), t.to(DEV), scale=s.to(DEV))
    assert torch.equal(only, _launch(p.contiguous(), targets, t, s)[0])


def test_meter_accumulates_over_launches_resets_and_repeats_its_bits():
    targets = 12
    meter = ops.RegressionMeter(targets, DEV)
    parts, rows_seen = [], 0
    for k, rows in enumerate((256, 256, 73)):
        buf, p, t, s = _operands(rows, targets, 7 + k)
        _launch(buf, targets, t, s, meter)
        alone = _launch(buf, targets, t, s)[1]
        again = _launch(buf, targets, t, s)[1]
        assert torch.equal(alone.record, again.record)                   # the same bits on a second run
        parts.append(alone.read()[0])
        rows_seen += rows
    got, graphs = meter.read()
    want = (parts[0] + parts[1]) + parts[2]                              # the launches add in stream order
    assert graphs == rows_seen == 585 and torch.equal(got, want)
    meter.reset()
    assert meter.read()[1] == 0 and not meter.read()[0].any() and int(meter.record[1]) == targets


def test_meter_with_no_rows_gives_nan_and_leaves_the_record():
    for targets in (1, 12):
        buf, p, t, s = _operands(9, targets, 3)
        _loss, meter = _launch(buf, targets, t)
        before = meter.record.clone()
        empty = torch.empty(0, targets, device=DEV)
        for scale in (None, s.to(DEV)):
            loss = ops.l1_loss(empty, empty.clone(), accumulate=meter, scale=scale)
            assert math.isnan(float(loss)) and torch.equal(meter.record, before)
    loss = ops.l1_loss(torch.empty(0, device=DEV), torch.empty(0, device=DEV), accumulate=ops.RegressionMeter(1, DEV))
    assert math.isnan(float(loss))


def test_a_nan_prediction_poisons_its_own_target_only():
    targets, rows = 12, 300
    buf, p, t, s = _operands(rows, targets, 21)
    buf[137, 5] = float("nan")
    for scale in (None, s):
        loss, meter = _launch(buf, targets, t, scale)
        got, graphs = meter.read()
        want = _terms(p, t, scale).double().sum(0)
        keep = [c for c in range(targets) if c != 5]
        assert math.isnan(float(loss)) and math.isnan(float(got[5])) and graphs == rows
        assert ((got[keep] - want[keep]).abs() <= 1e-12 * want[keep].abs()).all()


def test_more_than_32_targets_and_other_misuse_are_refused():
    p, t = torch.randn(4, 33, device=DEV), torch.randn(4, 33, device=DEV)
    with pytest.raises(ValueError, match="1..32"):
        ops.l1_loss(p, t, scale=torch.ones(33, device=DEV))
    out = torch.empty(1, device=DEV)
    with pytest.raises(RuntimeError, match="targets must be 1..KAGNN_REGRESSION_MAX_TARGETS"):
        ops._call("kagnn_l1_loss_meter_fwd", ops._ptr(p), 33, ops._ptr(t), 33, 4, 33, None, ops._ptr(out), None, ops._stream())
    with pytest.raises(ValueError, match="1..32"):
        ops.RegressionMeter(33, DEV)
    with pytest.raises(ValueError, match="made for 12 targets"):
        ops.l1_loss(p[:, :3], t[:, :3], accumulate=ops.RegressionMeter(12, DEV))
    with pytest.raises(ValueError, match="requires a gradient"):
        ops.l1_loss(p[:, :3].clone().requires_grad_(), t[:, :3], scale=torch.ones(3, device=DEV))
    with pytest.raises(ValueError, match="same shape"):
        ops.l1_loss(p[:, 0], t[:, :1], accumulate=ops.RegressionMeter(1, DEV))
    ops.l1_loss(p[:, :32], t[:, :32], accumulate=ops.RegressionMeter(32, DEV))       # 32 is served


@pytest.mark.parametrize("shape", [(257,), (257, 1), (40, 12), (1025, 32)])
def test_gradient_through_the_metered_loss_is_the_plain_losss_bit_for_bit(shape):
    g = torch.Generator().manual_seed(5)
    p0, t = torch.randn(*shape, generator=g).to(DEV), torch.randn(*shape, generator=g).to(DEV)
    t[3] = p0[3]                                                         # an exact zero difference: sign(0) = 0 on both paths
    up = torch.tensor(0.37, device=DEV)
    grads = []
    for metered in (False, True):
        p = p0.clone().requires_grad_()
        targets = 1 if len(shape) == 1 else shape[1]
        loss = ops.l1_loss(p, t, accumulate=ops.RegressionMeter(targets, DEV)) if metered else ops.l1_loss(p, t)
        loss.backward(up)
        grads.append(p.grad)
    assert grads[1].shape == p0.shape and torch.equal(grads[0], grads[1]) and bool(grads[0].any())
    if len(shape) == 2:                                                  # a strided prediction: the gradient lands in its columns
        wide = torch.randn(shape[0], shape[1] + 3, generator=g).to(DEV).requires_grad_()
        ops.l1_loss(wide[:, :shape[1]], t, accumulate=ops.RegressionMeter(shape[1], DEV)).backward()
        flat = wide.detach()[:, :shape[1]].contiguous().requires_grad_()
        ops.l1_loss(flat, t).backward()
        assert torch.equal(wide.grad[:, :shape[1]], flat.grad) and not wide.grad[:, shape[1]:].any()


# ------------------------------------------------------------------------------------------------ the epoch update
class _Rule:
    """the scripts' two rules (optuna_zinc.py:75-86, utils.py:8-16), restated on fp32 figures; plus the counters the record keeps"""

    def __init__(self, patience, min_delta, max_epochs):
        self.patience, self.min_delta, self.max_epochs = patience, np.float32(min_delta), max_epochs
        self.min = self.best_val = np.float32(np.inf)
        self.test_at_best = np.float32(np.nan)
        self.counter, self.epochs, self.best_epoch, self.test_epoch, self.improved, self.stopped = 0, 0, -1, -1, 0, 0

    def inert(self):
        return bool(self.stopped or self.epochs >= self.max_epochs)

    def update(self, val, test):
        self.improved = 0
        if self.inert():
            return
        val, test = np.float32(val), np.float32(test)
        if self.best_val >= val:
            self.best_val, self.test_at_best, self.test_epoch = val, test, self.epochs
        if val < self.min:
            self.min, self.counter, self.best_epoch, self.improved = val, 0, self.epochs, 1
        elif val >= np.float32(self.min + self.min_delta):
            self.counter += 1
            if self.counter >= self.patience:
                self.stopped = 1
        self.epochs += 1

    def record(self):
        return (float(self.min), float(self.min_delta), float(self.best_val), float(self.test_at_best), self.patience, self.counter,
                self.epochs, self.best_epoch, self.test_epoch, bool(self.improved), bool(self.stopped))


def _same(a, b):
    return len(a) == len(b) and all((isinstance(x, float) and isinstance(y, float) and math.isnan(x) and math.isnan(y)) or x == y
                                    for x, y in zip(a, b))


def _fill(meter, abs_sum, graphs):
    """write chosen sums into a meter from the host"""
    host = torch.zeros(2 + MAXT, dtype=torch.int64)
    host[0], host[1] = graphs, meter.num_targets
    host[2:2 + len(abs_sum)] = torch.tensor(abs_sum, dtype=torch.float64).view(torch.int64)
    meter.record.copy_(host)


def _figure(abs_sum, n):
    """the split's figure as the header states it: abs_sum[t] / n in fp64, added in index order, over T, rounded once to fp32"""
    acc = 0.0
    for v in abs_sum:
        acc += (v / n) if n else float("nan")
    return np.float32(acc / len(abs_sum))


def _is_zero(meter):
    host = meter.record.cpu()
    return int(host[0]) == 0 and int(host[1]) == meter.num_targets and not host[2:].any()


N_SPLIT = (7, 4, 9)                                                      # the three divisors; 4 makes `4 v / 4` exactly v
NAN = float("nan")
# name: (patience, min_delta, max_epochs, [(val figure, test figure), ...]) -- figures exactly representable in fp32
UPDATE_CASES = {
    "strictly falling": (3, 0.0, 16, [(1.0, 5.0), (0.875, 4.0), (0.75, 3.0), (0.625, 2.0), (0.5, 1.0)]),
    "a tie takes the test figure again and counts as a miss": (2, 0.0, 16, [(1.0, 5.0), (1.0, 4.0), (0.5, 3.0), (0.5, 2.0), (0.5, 1.0), (0.25, 0.5)]),
    "min_delta 0.25": (2, 0.25, 16, [(1.0, 1.0), (1.125, 2.0), (1.2421875, 3.0), (1.25, 4.0), (0.875, 5.0), (1.0, 6.0), (1.125, 7.0), (2.0, 8.0), (0.125, 9.0)]),
    "a NaN changes nothing": (2, 0.0, 16, [(1.0, 1.0), (NAN, 2.0), (1.5, 3.0), (NAN, NAN), (0.5, 4.0), (0.75, 5.0), (NAN, 6.0), (0.75, 7.0), (0.125, 8.0)]),
    "a NaN first": (1, 0.0, 16, [(NAN, 2.0), (NAN, 3.0), (2.0, 4.0), (2.0, 5.0), (1.0, 6.0)]),
    "patience 1": (1, 0.0, 16, [(0.5, 1.0), (0.25, 2.0), (0.25, 3.0), (0.125, 4.0)]),
    "longer than max_epochs": (50, 0.0, 4, [(1.0, 1.0), (0.875, 2.0), (1.0, 3.0), (0.75, 4.0), (0.5, 5.0), (0.25, 6.0)]),
}


@pytest.mark.parametrize("name", list(UPDATE_CASES))
@pytest.mark.parametrize("with_test", [True, False], ids=["test meter", "test_meter=NULL"])
def test_epoch_update_equals_the_restated_rules(name, with_test):
    patience, delta, max_epochs, seq = UPDATE_CASES[name]
    stop = ops.RegressionStop(patience, delta, max_epochs=max_epochs, num_targets=1, device=DEV)
    ref = _Rule(patience, delta, max_epochs)
    meters = [ops.RegressionMeter(1, DEV) for _ in range(3)]
    first = stop.read()
    assert _same(tuple(first[:11]), ref.record()) and first.history.shape == (0, 3, 1) and first.history.dtype == torch.float64
    rows, frozen = [], None
    for e, (v, w) in enumerate(seq):
        sums = ([float(e + 1)], [NAN if math.isnan(v) else 4.0 * v], [NAN if math.isnan(w) else 9.0 * w])
        for m, a, n in zip(meters, sums, N_SPLIT):
            _fill(m, a, n)
        inert = ref.inert()
        if inert and frozen is None:
            frozen = stop._buf.clone()
        stop.update(meters[0], meters[1], meters[2] if with_test else None, N_SPLIT)
        w_seen = w if with_test else v
        assert math.isnan(v) or float(_figure(sums[1], 4)) == v           # the figures are the chosen values exactly
        ref.update(v, w_seen)
        if not inert:
            rows.append([sums[0][0] / 7, sums[1][0] / 4, sums[2][0] / 9 if with_test else sums[1][0] / 4])
        got = stop.read()
        assert _same(tuple(got[:11]), ref.record()), (name, e, got[:11], ref.record())
        assert int(stop.improved) == ref.improved
        assert _is_zero(meters[0]) and _is_zero(meters[1]) and (_is_zero(meters[2]) or not with_test)
        hist = got.history[:, :, 0]
        want = torch.tensor(rows, dtype=torch.float64).reshape(-1, 3)
        assert hist.shape == want.shape and torch.equal(hist.nan_to_num(nan=-1.0), want.nan_to_num(nan=-1.0))    # (a NaN is a NaN)
        if inert:                                                        # nothing but `improved` (cleared) may differ
            now = stop._buf.clone()
            words = [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11]
            assert torch.equal(now[6:], frozen[6:]) and torch.equal(now[:6].view(torch.int32)[words], frozen[:6].view(torch.int32)[words])
            assert int(now[:6].view(torch.int32)[9]) == 0
    assert frozen is not None or name == "strictly falling", name       # every other sequence goes inert and is fed further values
    if name.startswith("a tie"):
        # epoch 1 ties epoch 0: the test figure and test_epoch moved, best_epoch and improved did not, and the tie was a miss
        assert ref.stopped and ref.epochs == 5 and ref.best_epoch == 2 and ref.test_epoch == 4
        assert float(ref.test_at_best) == (1.0 if with_test else 0.5)
    if name == "min_delta 0.25":
        assert ref.stopped and ref.epochs == 8 and ref.best_epoch == 4   # values inside [min, min + delta) counted neither way
    if name == "longer than max_epochs":
        assert ref.epochs == 4 and not ref.stopped
    # a raw call without a history leaves the rules unchanged
    st = torch.tensor([0x7F800000, 0, 0x7F800000, 0x7FC00000, 1, 0, 0, -1, -1, 0, 0, 0], dtype=torch.int32, device=DEV)
    _fill(meters[1], [2.0], 4)
    _fill(meters[2], [18.0], 9)
    ops._call("kagnn_regression_epoch_update", ops._ptr(meters[0].record), ops._ptr(meters[1].record), ops._ptr(meters[2].record),
              7, 4, 9, ops._ptr(st), None, 4, ops._stream())
    half, two = int(np.float32(0.5).view(np.int32)), int(np.float32(2.0).view(np.int32))
    assert st.tolist() == [half, 0, half, two, 1, 0, 1, 0, 0, 1, 0, 0]


def test_epoch_update_with_twelve_targets_takes_the_mean_of_the_per_target_means():
    T = 12
    g = torch.Generator().manual_seed(9)
    stop = ops.RegressionStop(2, 0.0, max_epochs=8, num_targets=T, device=DEV)
    ref = _Rule(2, 0.0, 8)
    meters = [ops.RegressionMeter(T, DEV) for _ in range(3)]
    n = (40, 25, 20)
    rows = []
    for e in range(7):
        sums = [(torch.rand(T, generator=g, dtype=torch.float64) * (50.0 if e != 2 else 20.0)).tolist() for _ in range(3)]
        if e == 3:
            sums[1][7] = NAN                                             # one poisoned target: the split's figure is NaN
        for m, a, k in zip(meters, sums, n):
            _fill(m, a, k * 16)
        inert = ref.inert()
        stop.update(meters[0], meters[1], meters[2], n)
        ref.update(_figure(sums[1], n[1]), _figure(sums[2], n[2]))
        if not inert:
            rows.append([[v / k for v in a] for a, k in zip(sums, n)])
        got = stop.read()
        assert _same(tuple(got[:11]), ref.record()), (e, got[:11], ref.record())
        assert all(_is_zero(m) for m in meters)
        want = torch.tensor(rows, dtype=torch.float64)
        assert got.history.shape == (len(rows), 3, T) and torch.equal(got.history.nan_to_num(nan=-1.0), want.nan_to_num(nan=-1.0))
        # columns at and beyond the targets are written as zeros
        assert not stop.history[:len(rows), :, T:].any()
    assert ref.best_epoch == 2 and ref.stopped and ref.epochs == 6 and len(rows) == 6 and ref.test_epoch == 2
    with pytest.raises(ValueError):
        stop.update(meters[0], meters[1], object(), n)


# ------------------------------------------------------------------------------------------------ the loop
G, BATCH, EPOCHS, LR = 40, 16, 4, 1e-2


def _dataset(kind, targets, seed=31):
    """40 random graphs of 3 to 9 nodes, 2 n edges each; KAGIN: 21 node and 4 edge features, KAGCN: 6 node features"""
    g = torch.Generator().manual_seed(seed)
    sizes = torch.randint(3, 10, (G,), generator=g)
    node_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)])
    esizes = 2 * sizes
    lo, span = torch.repeat_interleave(node_ptr[:-1], esizes), torch.repeat_interleave(sizes, esizes)
    E, N = int(esizes.sum()), int(node_ptr[-1])
    ei = torch.stack([lo + (torch.rand(E, generator=g) * span).long().clamp(max=span - 1) for _ in range(2)])
    x = torch.randn(N, 21 if kind == "KAGIN" else 6, generator=g)
    ea = torch.randn(E, 4, generator=g) if kind == "KAGIN" else None
    y = torch.randn(G, generator=g) if targets == 1 else torch.randn(G, targets, generator=g) * 3.0 + 1.0
    return kagnn_amd.DeviceGraphDataset(x, ei, node_ptr, edge_attr=ea, y=y, device=DEV), y


_PRISTINE = {}


def _model(kind, targets, seed=5):
    """a copy of ONE initial model per (kind, targets): KANLinear's initial spline weights come from a least-squares solve on the host
    that does not return the same bits twice for the same seed, so equal starting points are copies, never rebuilds"""
    if (kind, targets) not in _PRISTINE:
        torch.manual_seed(seed)
        if kind == "KAGIN":
            _PRISTINE[kind, targets] = kagnn_amd.KAGINRegression(21, 4, 2, 32, 2, 4, 3, targets, 0.0)
        else:
            _PRISTINE[kind, targets] = kagnn_amd.KAGCNRegression(6, 2, 8, 4, 3, targets, 0.0)
    return copy.deepcopy(_PRISTINE[kind, targets]).to(DEV)


def _loaders(ds):
    """train: all 40 graphs (16 + 16 + 8); val: 25 (16 + 9); test: 20 (16 + 4); unshuffled"""
    return tuple(kagnn_amd.DeviceBatchLoader(view, BATCH) for view in (ds, ds[list(range(5, 30))], ds[20:40]))


def _setup(kind, targets):
    ds, y = _dataset(kind, targets)
    std = None
    if targets > 1:                                                      # the QM9 script's preparation and its de-standardised figure
        ds, mean, std = ds.standardize_targets()
        assert mean.shape == std.shape == (1, targets) and std.is_cuda
    return ds, std


def _script(model, loaders, epochs, lr, patience, std, figures):
    """train_model_with_parameters (optuna_zinc.py:38-92 for std=None, optuna_qm9.py:38-96 otherwise), with its per-batch .item();
    ``figures`` also gets every epoch's test figure (taken outside the script's rule: an eval pass changes no state)"""
    train_loader, val_loader, test_loader = loaders
    optimizer = torch.optim.Adam(model.parameters(), lr=lr, fused=True)
    loss_function = torch.nn.L1Loss()
    best_val_loss, counter, lowest = float("inf"), 0, float("inf")
    test_loss = float("nan")

    def evaluate(loader):
        if std is None:
            total = 0
            for data in loader:
                total += loss_function(model(data).squeeze(), data.y).item() * data.num_graphs
            return total / len(loader.dataset)
        total = torch.zeros([1, std.size(1)]).to(DEV)
        for data in loader:
            total += ((data.y * std - model(data) * std).abs() / std).sum(dim=0)
        return (total / len(loader.dataset)).mean().item()

    ran = 0
    for epoch in range(1, epochs + 1):
        model.train()
        train_loss = 0
        for data in train_loader:
            optimizer.zero_grad()
            out = model(data).squeeze() if std is None else model(data)
            loss = loss_function(out, data.y)
            loss.backward()
            train_loss += loss.item() * data.num_graphs
            optimizer.step()
        train_loss = train_loss / len(train_loader.dataset)
        model.eval()
        val_loss = evaluate(val_loader)
        every_test = evaluate(test_loader)
        if best_val_loss >= val_loss:
            best_val_loss = val_loss
            test_loss = evaluate(test_loader)
        figures.append((train_loss, val_loss, every_test))
        ran = epoch
        if val_loss < lowest:                                            # EarlyStopper.early_stop
            lowest, counter = val_loss, 0
        elif val_loss >= lowest:
            counter += 1
            if counter >= patience:
                break
    ops.flush_graph_checks()
    return test_loss, best_val_loss, ran


def _same_state(a, b, what=""):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), f"{what}: {k}"


def _close(a, b, tol=1e-6):
    return abs(a - b) <= tol * abs(b)


@pytest.mark.parametrize("targets", [1, 12])
@pytest.mark.parametrize("kind", ["KAGIN", "KAGCN"])
def test_the_loop_with_the_scripts_loss_and_optimiser_is_the_script_bit_for_bit(kind, targets):
    ds, std = _setup(kind, targets)
    ma = _model(kind, targets)
    mb = copy.deepcopy(ma)
    figures = []
    want_test, want_best, ran = _script(mb, _loaders(ds), EPOCHS, LR, EPOCHS, std, figures)
    got = harness.train_graph_regression(ma, *_loaders(ds), epochs=EPOCHS, lr=LR, patience=EPOCHS, poll_every=1, loss_fn=torch.nn.L1Loss(),
                                         optimizer=torch.optim.Adam(ma.parameters(), lr=LR, fused=True), target_scale=std)
    print(f"{kind} T={targets}: script {figures} test {want_test} best {want_best}; device {got[:9]}")
    _same_state(ma, mb, f"{kind} T={targets}")
    assert ran == EPOCHS == got.epochs_run and not got.stopped and not ma.training
    assert len(got.train_losses) == len(got.val_losses) == len(got.test_losses) == EPOCHS and got.per_target.shape == (EPOCHS, 3, targets)
    for e, (tr, va, te) in enumerate(figures):
        assert _close(got.train_losses[e], tr) and _close(got.val_losses[e], va) and _close(got.test_losses[e], te), (e, tr, va, te)
    # the script's decisions hang on the order of validation figures: wherever two of them are compared they differ by far more
    # than the 1e-6 by which the two ways of taking a figure may differ, so the device took the same decisions
    vals = [f[1] for f in figures]
    assert all(abs(a - b) > 1e-5 * abs(b) for i, a in enumerate(vals) for b in vals[:i])
    assert _close(got.best_val_loss, want_best) and _close(got.test_loss, want_test)
    assert got.test_epoch == got.best_epoch == min(range(EPOCHS), key=vals.__getitem__)
    assert got.best_val_loss == got.val_losses[got.best_epoch] and got.test_loss == got.test_losses[got.test_epoch]


def _run(kind, targets, poll_every, **kw):
    ds, std = _setup(kind, targets)
    m = _model(kind, targets)
    res = harness.train_graph_regression(m, *_loaders(ds), poll_every=poll_every, target_scale=std, **kw)
    return m, res, ds, std


def _same_result(a, b):
    return _same(tuple(a[:6]), tuple(b[:6])) and a[6:9] == b[6:9] and torch.equal(a.per_target.nan_to_num(nan=-1.0), b.per_target.nan_to_num(nan=-1.0))


def test_polling_does_not_change_the_result():
    # (keep_best: the epochs a lazy poll runs after the stop train the live weights; the snapshot is what must not depend on them)
    for kw in (dict(epochs=5, lr=LR, patience=100), dict(epochs=12, lr=0.3, patience=2), dict(epochs=12, lr=0.0, patience=2)):
        (m1, r1, ds, std), (m3, r3, _, _) = [_run("KAGCN", 12, p, keep_best=True, **kw) for p in (1, 3)]
        print(f"{kw}: {r1[:9]}")
        _same_state(m1, m3, str(kw))
        assert _same_result(r1, r3), (r1[:9], r3[:9])
        assert r1.stopped or r1.epochs_run == kw["epochs"]
        if kw["lr"] == 0.0:
            assert r1.stopped and r1.epochs_run == 3                      # the poll at epoch 3 sees it; with poll_every=1 too


def test_evaluation_agrees_with_the_historys_last_row_and_validation_stands_in_for_a_missing_test_loader():
    kw = dict(epochs=3, lr=LR, patience=100)
    m1, r1, ds, std = _run("KAGCN", 12, 2, **kw)
    assert r1.epochs_run == 3 and not r1.stopped
    # the history's last row is an evaluation of the weights the loop leaves behind (the training figure is taken WHILE training)
    for s, loader in enumerate(_loaders(ds)):
        if s:
            mean, per_target = harness.evaluate_graph_regression(m1, loader, target_scale=std)
            assert torch.equal(per_target, r1.per_target[-1, s]) and mean == (r1.val_losses, r1.test_losses)[s - 1][-1]
    plain_mean, plain = harness.evaluate_graph_regression(m1, _loaders(ds)[1])
    # the unscaled figure is the same quantity rounded differently: |y s - p s| / s carries the roundings of y s and p s, each 2^-24 of
    # a standardised target (a few units at most) against errors of order one -- 1e-5 relative covers it with room
    assert plain.shape == (12,) and abs(plain_mean - r1.val_losses[-1]) <= 1e-5 * r1.val_losses[-1]
    tr, va, _te = _loaders(ds)
    r = harness.train_graph_regression(_model("KAGCN", 12), tr, va, None, target_scale=std, **kw)
    assert r.val_losses == r1.val_losses and r.test_losses == r.val_losses and r.test_loss == r.best_val_loss == r1.best_val_loss


def test_lists_of_premade_batches_serve_as_loaders():
    kw = dict(epochs=2, lr=LR, patience=100)
    m1, r1, ds, std = _run("KAGCN", 12, 1, **kw)
    lists = [list(loader) for loader in _loaders(ds)]                   # (unshuffled: the same batches every epoch)
    ops.flush_graph_checks()
    m2 = _model("KAGCN", 12)
    r2 = harness.train_graph_regression(m2, *lists, poll_every=1, target_scale=std, **kw)
    _same_state(m1, m2, "lists")
    assert _same_result(r1, r2) and r2.epochs_run == 2                   # the divisors are the graphs the lists hold: 40 / 25 / 20
    mean, per_target = harness.evaluate_graph_regression(m2, lists[1], target_scale=std)
    assert mean == r2.val_losses[-1] and torch.equal(per_target, r2.per_target[-1, 1])


def test_the_training_pass_is_train_graph_batches_step_bit_for_bit():
    """default loss, default harness.Adam: the experiment's training pass and ``train_graph_batches`` take the same step, so the same
    batches leave the same weights (the metered loss gives the plain loss's gradient bits; the evaluation passes between the epochs
    run in ``eval()`` mode and the model has no dropout, so they change no state)"""
    ds, _ = _setup("KAGCN", 1)
    lists = [list(loader) for loader in _loaders(ds)]                   # (unshuffled: 16 + 16 + 8, the same batches every epoch)
    ops.flush_graph_checks()
    ma = _model("KAGCN", 1)
    mb = copy.deepcopy(ma)
    res = harness.train_graph_regression(ma, *lists, epochs=2, lr=LR, patience=100, poll_every=1)
    harness.train_graph_batches(mb, lists[0], nb_epochs=2, warmup=0, lr=LR)
    assert res.epochs_run == 2 and not res.stopped
    _same_state(ma, mb, "train_graph_regression against train_graph_batches")


class _Stub(torch.nn.Module):
    """one parameter; with lr = 0 every epoch repeats the first one's figures exactly"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.full((1,), 0.25))

    def forward(self, data):
        return self.w * torch.ones(data.y.size(0), device=data.y.device)


@pytest.mark.parametrize("poll_every", [1, 8])
def test_with_lr_zero_every_epoch_ties_and_the_stop_comes_after_patience_misses(poll_every):
    ds, _ = _setup("KAGCN", 1)
    patience = 3
    res = harness.train_graph_regression(_Stub().to(DEV), *_loaders(ds), epochs=20, lr=0.0, patience=patience, poll_every=poll_every)
    print(res[:9])
    assert res.stopped and res.epochs_run == patience + 1 and res.best_epoch == 0 and res.test_epoch == res.epochs_run - 1
    assert len(set(res.val_losses)) == 1 and res.best_val_loss == res.val_losses[0] and res.test_loss == res.test_losses[0]
    assert res.per_target.shape == (patience + 1, 3, 1)


def test_keep_best_restores_the_best_epochs_weights():
    kw = dict(epochs=8, lr=0.3, patience=100)
    ds, std = _setup("KAGIN", 1)
    start = _model("KAGIN", 1)
    m = copy.deepcopy(start)
    res = harness.train_graph_regression(m, *_loaders(ds), poll_every=3, keep_best=True, **kw)
    print(res[:9])
    assert res.epochs_run == 8 and 0 <= res.best_epoch < 8
    # a rerun that ends with epoch best_epoch: its last weights are the snapshot's
    again = copy.deepcopy(start)
    r2 = harness.train_graph_regression(again, *_loaders(ds), poll_every=1, **{**kw, "epochs": res.best_epoch + 1})
    _same_state(m, again, "keep_best")
    assert r2.val_losses == res.val_losses[:res.best_epoch + 1] and r2.best_epoch == res.best_epoch
    # and without keep_best the loop leaves the last epoch's weights, which differ unless the last epoch was the best one
    last = copy.deepcopy(start)
    r3 = harness.train_graph_regression(last, *_loaders(ds), poll_every=3, **kw)
    assert _same_result(r3, res)
    differs = any(not torch.equal(a, b) for a, b in zip(last.state_dict().values(), m.state_dict().values()))
    assert differs == (res.best_epoch != res.epochs_run - 1)
    # teeth that hang on no KAN: one parameter walking towards the targets' median in Adam steps of ~1 overshoots it -- on these
    # targets the validation figure of epoch 1 (0.58) is 3 % below every later one (torch's Adam on the CPU: 0.82 0.58 0.90 0.67 0.60)
    ds1, _ = _setup("KAGCN", 1)
    kw = dict(epochs=5, lr=1.0, patience=100)
    kept, plain = _Stub().to(DEV), _Stub().to(DEV)
    res = harness.train_graph_regression(kept, *_loaders(ds1), poll_every=4, keep_best=True, **kw)
    harness.train_graph_regression(plain, *_loaders(ds1), poll_every=1, **{**kw, "epochs": res.best_epoch + 1})
    print(res[:9], float(kept.w.detach()), float(plain.w.detach()))
    assert res.epochs_run == 5 and res.best_epoch < 4 and torch.equal(kept.w, plain.w)
    harness.train_graph_regression(plain, *_loaders(ds1), poll_every=1, **{**kw, "epochs": 5})
    assert not torch.equal(kept.w, plain.w)


# ------------------------------------------------------------------------------------------------ read-backs
class _Reads:
    """this file's counter of what brings a device value to the host (``item / tolist / cpu / numpy / to(cpu) / float() / int() /
    bool()``) and of explicit waits, tagged 'poll' inside ``RegressionStop.read``, 'flush' inside ``flush_graph_checks`` (the epoch's
    one wait on its deferred checks) and 'loop' elsewhere"""

    def __init__(self, monkeypatch):
        self.phase, self.log, self.polls, self.flushes = "loop", [], 0, 0
        outer = self
        for name in ("item", "tolist", "cpu", "numpy", "__float__", "__int__", "__bool__", "__index__"):
            self._count(monkeypatch, torch.Tensor, name, lambda t: t.is_cuda)
        real_to = torch.Tensor.to

        def to(t, *a, **kw):
            out = real_to(t, *a, **kw)
            if t.is_cuda and not out.is_cuda:
                outer.log.append((outer.phase, "to"))
            return out
        monkeypatch.setattr(torch.Tensor, "to", to)
        self._count(monkeypatch, torch.cuda, "synchronize", None)
        self._count(monkeypatch, torch.cuda.Event, "synchronize", lambda ev: True, "Event.synchronize")
        self._count(monkeypatch, torch.cuda.Stream, "synchronize", lambda st: True, "Stream.synchronize")
        real_read, real_flush = ops.RegressionStop.read, ops.flush_graph_checks

        def read(stop, *a, **kw):
            was, outer.phase = outer.phase, "poll"
            outer.polls += 1
            try:
                return real_read(stop, *a, **kw)
            finally:
                outer.phase = was

        def flush(*a, **kw):
            was, outer.phase = outer.phase, "flush"
            outer.flushes += 1
            try:
                return real_flush(*a, **kw)
            finally:
                outer.phase = was
        monkeypatch.setattr(ops.RegressionStop, "read", read)
        monkeypatch.setattr(ops, "flush_graph_checks", flush)

    def _count(self, monkeypatch, owner, name, when, label=None):
        real, outer = getattr(owner, name), self

        def counted(*a, **kw):
            if when is None or when(a[0]):
                outer.log.append((outer.phase, label or name))
            return real(*a, **kw)
        monkeypatch.setattr(owner, name, counted)

    def during(self, phase):
        return [what for p, what in self.log if p == phase]


def test_no_read_back_between_the_polls(monkeypatch):
    ds, std = _setup("KAGIN", 12)
    _run("KAGIN", 12, 16, epochs=2, lr=LR, patience=100)                 # (first use: packs, allocator)
    torch.cuda.synchronize()
    # teeth: the script's loop reads once per batch, and the counter sees it
    rd = _Reads(monkeypatch)
    _script(_model("KAGIN", 12), _loaders(ds), 2, LR, 100, std, [])
    assert len(rd.during("loop")) >= 2 * 3
    monkeypatch.undo()
    for poll_every, polls in ((4, 2), (1, 10), (64, 0)):
        m = _model("KAGIN", 12)
        with torch.no_grad():
            m(next(iter(_loaders(ds)[0])))                               # (a fresh model's first forward checks its knot grids once)
        ops.flush_graph_checks()
        rd = _Reads(monkeypatch)
        res = harness.train_graph_regression(m, *_loaders(ds), epochs=10, lr=LR, patience=100, poll_every=poll_every, target_scale=std,
                                             keep_best=True)
        monkeypatch.undo()
        assert res.epochs_run == 10
        assert rd.during("loop") == [], rd.during("loop")                # nothing between the polls
        assert rd.polls == polls + 1 and rd.during("poll") == ["cpu"] * (polls + 1)      # one read-back per poll, one at the end
        assert rd.flushes == 10 + 1 and set(rd.during("flush")) <= {"Event.synchronize"}   # the epoch's one wait; never a read-back


def test_standardize_targets_is_the_scripts_preparation():
    ds, y = _dataset("KAGCN", 12)
    for columns, pick in ((None, slice(None)), (slice(0, 5), slice(0, 5)), ([1, 7], [1, 7])):
        new, mean, std = ds[3:33].standardize_targets(columns)
        yc = y[:, pick]
        wm, ws = yc.mean(dim=0, keepdim=True), yc.std(dim=0, keepdim=True)    # over the WHOLE dataset, as the script does before it splits
        # (fp32 sums of 40 values on two devices: n x 2^-24 = 2.4e-6)
        assert torch.allclose(mean.cpu(), wm, rtol=1e-5, atol=1e-6) and torch.allclose(std.cpu(), ws, rtol=1e-5, atol=0)
        assert torch.allclose(new.storage.y.cpu(), (yc - wm) / ws, rtol=1e-5, atol=1e-5) and len(new) == 30
        assert new.storage.x is ds.storage.x and ds.storage.y.shape == (G, 12)      # shared arrays; the source is untouched
        batch = next(iter(kagnn_amd.DeviceBatchLoader(new, 4)))
        assert torch.equal(batch.y, new.storage.y[3:7])
    one, mean, std = _dataset("KAGCN", 1)[0].standardize_targets()
    assert one.storage.y.shape == (G, 1) and mean.shape == (1, 1)
