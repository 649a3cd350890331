"""The node-classification experiment on the device (reference ``node_classification_clean/utils.py``: ``train_total``, ``all_splits``,
``EarlyStopper``): ``kagnn_node_eval``, ``kagnn_early_stop_update``, ``kagnn_copy_if`` and the loops of ``kagnn_amd.harness`` built on
them -- each against the plain statement of what the reference's script does, written out here.

Bounds.  Row counts, correct counts, the stopper's record, the predicated copies and the script-form trajectories are exact (nothing
rounds differently).  A cross-entropy SUM is held to ``max(4 x E32, 1e-6 x |fp64 value|)``, where E32 is the error of torch's own fp32
``F.cross_entropy`` on the CPU against the fp64 value for the same fp32 logits (the factor 4 covers the different exp / log
implementations).  Parameter gradients of the native training loss against the script's: the layer contract of ``helpers.assert_close``.
The worst observed fraction of the cross-entropy bound is recorded in ``profiles/node_classification_loop.md``."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kagnn_amd
from kagnn_amd import harness, ops
from helpers import assert_close, must_fail, prenorm_bias_noise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -0x0123456789ABCDEF


# ------------------------------------------------------------------------------------------------ node_eval against fp64
def _case(n, c, seed, extra=0, empty_split=None):
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn(n, c + extra, generator=g) * 3.0
    z = buf[:, :c]
    y = torch.randint(0, c, (n,), generator=g)
    # three overlapping splits, each row in each with probability 0.536: (1 - 0.536)^3 = 10 % of the rows in none
    masks = [torch.rand(n, generator=g) < 0.536 for _ in range(3)]
    if empty_split is not None:
        masks[empty_split] = torch.zeros(n, dtype=torch.bool)
    return buf, z, y, masks


def _xent_bound(z, y, m):
    """(fp64 sum, the bound on |figure - fp64 sum|) over the rows ``m``"""
    if not bool(m.any()):
        return 0.0, 0.0
    want = float(F.cross_entropy(z.double()[m], y[m], reduction="sum"))
    e32 = abs(float(F.cross_entropy(z[m], y[m], reduction="sum")) - want)
    return want, max(4.0 * e32, 1e-6 * abs(want))


def _records(rec):
    host = rec.cpu()
    return host[:, 0].view(torch.float64).tolist(), host[:, 1].tolist(), host[:, 2].tolist()


WORST = {"fraction": 0.0}


def _check_eval(buf, z, y, masks, what):
    zd = buf.to(DEV)[:, :z.size(1)]
    assert zd.stride(0) == buf.size(1) and (z.size(0) == 1 or zd.is_contiguous() == (buf.size(1) == z.size(1)))
    rec = ops.node_eval(zd, y.to(DEV), ops.split_bits(*masks).to(DEV), len(masks))
    assert rec.dtype == torch.int64 and rec.shape == (len(masks), 3) and rec.is_cuda
    xent, correct, rows = _records(rec)
    pred = z.argmax(1)
    for s, m in enumerate(masks):
        assert rows[s] == int(m.sum()) and correct[s] == int((pred[m] == y[m]).sum()), (what, s)
        want, bound = _xent_bound(z, y, m)
        err = abs(xent[s] - want)
        frac = err / bound if bound > 0.0 else (0.0 if err == 0.0 else math.inf)
        WORST["fraction"] = max(WORST["fraction"], frac)
        print(f"{what} split {s}: rows {rows[s]} xent_sum {xent[s]!r} fp64 {want!r} err {err:.3e} bound {bound:.3e} fraction {frac:.3f}")
        assert err <= bound, (what, s, xent[s], want, bound)
    ops.flush_graph_checks()
    return rec


SHAPES = [(1, 2), (63, 5), (64, 7), (65, 7), (1000, 40), (1000, 47), (257, 1), (300, 130), (70001, 7)]


@pytest.mark.parametrize("extra", [0, 3], ids=["ld=C", "ld=C+3"])
@pytest.mark.parametrize("n,c", SHAPES)
def test_node_eval_against_fp64(n, c, extra):
    buf, z, y, masks = _case(n, c, 100 + n + c, extra)
    none = ~(masks[0] | masks[1] | masks[2])
    if n >= 1000:
        assert 0.05 < float(none.float().mean()) < 0.15 and bool((masks[0] & masks[1]).any())
    _check_eval(buf, z, y, masks, f"N={n} C={c} ld={c + extra}")
    print(f"worst fraction of the bound so far: {WORST['fraction']:.4f}")


def test_node_eval_with_an_empty_split_and_with_no_rows():
    buf, z, y, masks = _case(500, 6, 7, 0, empty_split=1)
    rec = _check_eval(buf, z, y, masks, "empty split")
    xent, correct, rows = _records(rec)
    assert (xent[1], correct[1], rows[1]) == (0.0, 0, 0) and rows[0] > 0 and rows[2] > 0
    # N = 0: every record is zero
    out = torch.full((3, 3), SENTINEL, dtype=torch.int64, device=DEV)
    ops.node_eval(torch.empty(0, 4, device=DEV), torch.empty(0, dtype=torch.int64, device=DEV), torch.empty(0, dtype=torch.uint8, device=DEV), 3, out=out)
    assert _records(out) == ([0.0] * 3, [0] * 3, [0] * 3)
    # a single split
    one = ops.node_eval(z.to(DEV), y.to(DEV), ops.split_bits(masks[0]).to(DEV), 1)
    assert torch.equal(one.cpu(), rec.cpu()[:1])


# ------------------------------------------------------------------------------------------------ node_eval edge behaviour
def _eval1(z, y, bits, s=1):
    xent, correct, rows = _records(ops.node_eval(z.to(DEV), torch.tensor(y).to(DEV), torch.tensor(bits, dtype=torch.uint8).to(DEV), s))
    return xent, correct, rows


def test_node_eval_ties_go_to_the_lowest_index():
    z = torch.tensor([[1.0, 5.0, 5.0, 2.0]] * 2)
    assert _eval1(z, [1, 2], [1, 1])[1] == [1]                       # only the row labelled 1 is correct
    assert _eval1(z, [2, 2], [1, 1])[1] == [0]
    # 130 classes: 64 lanes share a row -- a tie inside one lane (columns 3 and 67), across lanes (3 and 70), across both (67 and 70)
    for a, b in ((3, 67), (3, 70), (67, 70), (0, 129), (64, 128)):
        row = torch.zeros(130)
        row[a] = row[b] = 9.0
        wide = torch.stack([row, row])
        assert _eval1(wide, [a, b], [1, 1])[1] == [1], (a, b)
        assert _eval1(wide, [b, b], [1, 1])[1] == [0], (a, b)
    ops.flush_graph_checks()


def test_node_eval_nan_row_is_wrong_and_poisons_only_its_own_splits():
    buf, z, y, masks = _case(200, 5, 11)
    r = int(torch.nonzero(masks[0] & ~masks[1] & ~masks[2])[0])
    z[r, 2] = float("nan")
    y[r] = int(torch.nan_to_num(z[r], nan=-1e30).argmax())           # the label IS the largest finite entry: still never correct
    xent, correct, rows = _records(ops.node_eval(z.to(DEV), y.to(DEV), ops.split_bits(*masks).to(DEV), 3))
    assert math.isnan(xent[0]) and not math.isnan(xent[1]) and not math.isnan(xent[2])
    keep = torch.ones(200, dtype=torch.bool)
    keep[r] = False
    pred = z.argmax(1)
    for s, m in enumerate(masks):
        assert rows[s] == int(m.sum()) and correct[s] == int((pred[m & keep] == y[m & keep]).sum())
    for s in (1, 2):
        want, bound = _xent_bound(z, y, masks[s])
        assert abs(xent[s] - want) <= bound
    ops.flush_graph_checks()                                          # a NaN logit is not a bad label: nothing raised


@pytest.mark.parametrize("bad", [-1, "C"])
def test_node_eval_bad_label_raises_at_flush_and_writes_nothing_else(bad):
    buf, z, y, masks = _case(300, 7, 12)
    r = int(torch.nonzero(masks[1] & ~masks[0] & ~masks[2])[0])
    y[r] = 7 if bad == "C" else -1
    guarded = torch.full((5, 3), SENTINEL, dtype=torch.int64, device=DEV)
    rec = ops.node_eval(z.to(DEV), y.to(DEV), ops.split_bits(*masks).to(DEV), 3, out=guarded[1:4])
    assert rec.data_ptr() == guarded[1:4].data_ptr()
    with pytest.raises(RuntimeError, match="kagnn_node_eval"):
        ops.flush_graph_checks()
    ops.flush_graph_checks()                                          # reported once, the flag is cleared
    assert bool((guarded[0] == SENTINEL).all()) and bool((guarded[4] == SENTINEL).all())
    xent, correct, rows = _records(rec)
    assert math.isnan(xent[1]) and not math.isnan(xent[0]) and not math.isnan(xent[2])
    keep = torch.ones(300, dtype=torch.bool)
    keep[r] = False
    pred = z.argmax(1)
    for s, m in enumerate(masks):
        assert rows[s] == int(m.sum()) and correct[s] == int((pred[m & keep] == y[m & keep]).sum())
    # a bad label in a row of NO split is never looked at
    y2 = y.clone()
    y2[r] = 0
    none = int(torch.nonzero(~(masks[0] | masks[1] | masks[2]))[0])
    y2[none] = 1 << 40
    ops.node_eval(z.to(DEV), y2.to(DEV), ops.split_bits(*masks).to(DEV), 3)
    ops.flush_graph_checks()


def test_node_eval_split_count_and_high_bits():
    buf, z, y, masks = _case(400, 9, 13)
    zd, yd, bits = z.to(DEV), y.to(DEV), ops.split_bits(*masks).to(DEV)
    with pytest.raises(ValueError, match="num_splits"):
        ops.node_eval(zd, yd, bits, 9)
    with pytest.raises(ValueError, match="num_splits"):
        ops.node_eval(zd, yd, bits, 0)
    rec9 = torch.empty(9, 3, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="num_splits"):              # ... and by the library itself
        ops._call("kagnn_node_eval", ops._ptr(zd), 9, 400, 9, ops._ptr(yd), ops._ptr(bits), 9, ops._ptr(rec9), ops._ptr(torch.zeros(2, dtype=torch.int32, device=DEV)),
                  None, 0, ops._stream())
    with pytest.raises(ValueError, match="1 to 8"):
        ops.split_bits(*([masks[0]] * 9))
    want = ops.node_eval(zd, yd, bits, 3)
    high = bits | 0xF8                                                   # every row, also those of no split, has bits 3..7 set
    got = ops.node_eval(zd, yd, high, 3)
    assert torch.equal(got, want)
    # all eight splits at once: splits 3..7 are every row
    full = ops.node_eval(zd, yd, high, 8)
    assert torch.equal(full[:3], want) and full[3:, 2].tolist() == [400] * 5 and len({tuple(r) for r in full[3:].tolist()}) == 1
    every = _xent_bound(z, y, torch.ones(400, dtype=torch.bool))
    assert abs(float(full[3:4, 0].view(torch.float64)[0]) - every[0]) <= every[1]
    ops.flush_graph_checks()


def test_node_eval_two_runs_give_the_same_bits():
    buf, z, y, masks = _case(70001, 7, 14)
    zd, yd, bits = z.to(DEV), y.to(DEV), ops.split_bits(*masks).to(DEV)
    a = ops.node_eval(zd, yd, bits, 3).clone()
    torch.empty(1 << 20, device=DEV).fill_(3.0)                          # (another workspace block in between)
    b = ops.node_eval(zd, yd, bits, 3)
    assert torch.equal(a, b)
    ops.flush_graph_checks()


# ------------------------------------------------------------------------------------------------ EarlyStop
class _Stopper:
    """the reference's rule, restated on fp32 values; plus the counters the device record keeps"""

    def __init__(self, patience, min_delta, max_epochs):
        self.patience, self.min_delta, self.max_epochs = patience, np.float32(min_delta), max_epochs
        self.min, self.counter, self.epochs, self.best, self.improved, self.stopped = np.float32(np.inf), 0, 0, -1, 0, 0
        self.history = []

    def update(self, v):
        if self.stopped or self.epochs >= self.max_epochs:
            self.improved = 0
            return
        v = np.float32(v)
        self.history.append(v)
        self.improved = 0
        if v < self.min:
            self.min, self.counter, self.best, self.improved = v, 0, self.epochs, 1
        elif v >= np.float32(self.min + self.min_delta):
            self.counter += 1
            if self.counter >= self.patience:
                self.stopped = 1
        self.epochs += 1

    def record(self):
        return (float(self.min), float(self.min_delta), self.patience, self.counter, self.epochs, self.best, bool(self.improved), bool(self.stopped))


def _val_records(v, epoch):
    """records whose validation mean is exactly the fp32 value ``v``: xent_sum = 4 v over 4 rows (NaN: 0 / 0 rows)"""
    rec = torch.zeros(3, 3, dtype=torch.int64)
    rec[:, 0] = torch.tensor([float(epoch), 0.0 if np.isnan(v) else 4.0 * float(np.float32(v)), -1.5], dtype=torch.float64).view(torch.int64)
    rec[:, 1] = torch.tensor([epoch, 2, 3])
    rec[:, 2] = torch.tensor([7, 0 if np.isnan(v) else 4, 9])
    return rec


EARLY_CASES = {
    "strictly decreasing": (3, 0.0, 16, [1.0, 0.9, 0.8, 0.7, 0.6, 0.5]),
    "equal consecutive values are misses": (3, 0.0, 16, [1.0, 1.0, 1.0, 0.5, 0.5, 0.5, 0.5, 0.4]),
    "a NaN in the middle changes nothing": (2, 0.0, 16, [1.0, 1.1, float("nan"), float("nan"), 0.9, 1.0, float("nan"), 1.0, 0.1]),
    "patience 1": (1, 0.0, 16, [0.5, 0.4, 0.4, 0.3]),
    "min_delta 0.05": (2, 0.05, 16, [1.0, 1.01, 1.04, 1.049, 1.05, 0.99, 1.03, 1.039, 1.04, 1.2, 0.1]),
    "longer than max_epochs": (50, 0.0, 5, [1.0, 0.9, 1.0, 0.8, 0.7, 0.6, 0.5, 0.4]),
    "infinite losses": (2, 0.0, 16, [float("inf"), float("inf"), 1.0, float("inf"), 2.0, 0.5]),
}


@pytest.mark.parametrize("name", list(EARLY_CASES))
def test_early_stop_update_equals_the_restated_rule(name):
    patience, delta, max_epochs, values = EARLY_CASES[name]
    dev = ops.EarlyStop(patience, delta, max_epochs=max_epochs, num_splits=3, device=DEV)
    ref = _Stopper(patience, delta, max_epochs)
    first = dev.read()
    assert first[:8] == ref.record() and first.history.shape == (0, 3, 3)
    fed, frozen = [], None
    for e, v in enumerate(values):
        rec = _val_records(v, e)
        inert = ref.stopped or ref.epochs >= max_epochs
        if inert and frozen is None:
            frozen = dev._buf.clone()
        dev.update(rec.to(DEV), 1)
        ref.update(v)
        if not inert:
            fed.append(rec)
        got = dev.read()
        assert got[:8] == ref.record(), (name, e, got[:8], ref.record())
        assert int(dev.improved) == ref.improved
        assert torch.equal(got.history, torch.stack(fed)) if fed else got.history.numel() == 0
        if inert:                                                        # after the stop: nothing but `improved` (cleared) may differ
            now = dev._buf.clone()
            assert torch.equal(now[4:], frozen[4:]) and torch.equal(now[:4].view(torch.int32)[[0, 1, 2, 3, 4, 5, 7]], frozen[:4].view(torch.int32)[[0, 1, 2, 3, 4, 5, 7]])
            assert int(now[:4].view(torch.int32)[6]) == 0
    if name == "longer than max_epochs":
        assert ref.epochs == 5 and not ref.stopped and frozen is not None
    elif name not in ("strictly decreasing",):
        assert ref.stopped and frozen is not None, name                 # every other sequence stops and is then fed further values
    if name == "min_delta 0.05":
        assert ref.epochs == 10 and ref.best == 5                       # values inside [min, min + delta) counted neither way
    # the history of a nullable history pointer: a raw call without one leaves the record's rule unchanged
    st = torch.tensor([0x7F800000, 0, 1, 0, 0, -1, 0, 0], dtype=torch.int32, device=DEV)
    ops._call("kagnn_early_stop_update", ops._ptr(_val_records(0.5, 0).to(DEV)), 3, 1, ops._ptr(st), None, 4, ops._stream())
    assert st.tolist() == [int(np.float32(0.5).view(np.int32)), 0, 1, 0, 1, 0, 1, 0]


def test_early_stop_refuses_bad_arguments():
    dev = ops.EarlyStop(3, device=DEV)
    with pytest.raises(ValueError):
        dev.update(torch.zeros(3, 3, dtype=torch.int64, device=DEV), 3)
    with pytest.raises(ValueError):
        dev.update(torch.zeros(2, 3, dtype=torch.int64, device=DEV), 1)
    with pytest.raises(RuntimeError, match="bad split"):
        ops._call("kagnn_early_stop_update", ops._ptr(torch.zeros(3, 3, dtype=torch.int64, device=DEV)), 3, 3, ops._ptr(dev.state), None, 4, ops._stream())


# ------------------------------------------------------------------------------------------------ copy_if
def _copy_case(seed=5):
    """40 (dtype, byte size, offset) slots inside guarded byte buffers: 4 bytes, an int64 scalar, 12 bytes, 4 * 1000 + 4 bytes and a
    4-byte aligned but not 16-byte aligned view (offset 20) -- the allocator's blocks are at least 16-byte aligned"""
    g = torch.Generator().manual_seed(seed)
    kinds = [(torch.float32, 4, 16), (torch.int64, 8, 16), (torch.float32, 12, 16), (torch.float32, 4004, 16), (torch.float32, 4004, 20),
             (torch.int64, 8, 24), (torch.float32, 36, 20), (torch.int32, 64, 16)]
    slots = []
    for k in range(40):
        dtype, nbytes, off = kinds[k % len(kinds)]
        raw_d = torch.randint(0, 256, (off + nbytes + 32,), dtype=torch.uint8, generator=g).to(DEV)
        raw_s = torch.randint(0, 256, (off + nbytes + 32,), dtype=torch.uint8, generator=g).to(DEV)
        assert raw_d.data_ptr() % 16 == 0 and raw_s.data_ptr() % 16 == 0
        d, s = raw_d[off:off + nbytes].view(dtype), raw_s[off:off + nbytes].view(dtype)
        if dtype == torch.int64 and nbytes == 8:
            d, s = d[0], s[0]                                            # a 0-dim counter, as num_batches_tracked
        slots.append((raw_d, raw_s, d, s, off, nbytes))
    return slots


@pytest.mark.parametrize("flag", [1, 0, -5])
def test_copy_if_copies_every_byte_or_none(flag):
    slots = _copy_case()
    before = [raw_d.clone() for raw_d, *_ in slots]
    sources = [raw_s.clone() for _, raw_s, *_ in slots]
    word = torch.tensor([flag], dtype=torch.int32, device=DEV)
    ops.copy_if(word, [s[2] for s in slots], [s[3] for s in slots])
    ops.copy_if(word, [s[2] for s in slots], [s[3] for s in slots])      # (the cached tables)
    assert any(s[2].data_ptr() % 16 for s in slots) and len(slots) == 40
    for (raw_d, raw_s, d, s, off, nbytes), was, src in zip(slots, before, sources):
        assert torch.equal(raw_s, src)
        if flag:
            assert torch.equal(raw_d[off:off + nbytes], raw_s[off:off + nbytes]), (off, nbytes)
        else:
            assert torch.equal(raw_d[off:off + nbytes], was[off:off + nbytes]), (off, nbytes)
        assert torch.equal(raw_d[:off], was[:off]) and torch.equal(raw_d[off + nbytes:], was[off + nbytes:]), (off, nbytes)


def test_copy_if_refuses_what_it_cannot_copy():
    word = torch.ones(1, dtype=torch.int32, device=DEV)
    a, b = torch.zeros(6, device=DEV), torch.zeros(6, device=DEV)
    with pytest.raises(ValueError):
        ops.copy_if(word, [a], [b, b])
    with pytest.raises(ValueError):
        ops.copy_if(word, [a.view(2, 3).t()], [b.view(2, 3).t()])
    with pytest.raises(ValueError):
        ops.copy_if(word, [torch.zeros(3, dtype=torch.uint8, device=DEV)], [torch.zeros(3, dtype=torch.uint8, device=DEV)])
    with pytest.raises(TypeError):
        ops.copy_if(word.float(), [a], [b])
    ops.copy_if(word, [], [])


# ------------------------------------------------------------------------------------------------ the loop
N, E, FEAT, CLASSES, EPOCHS, PATIENCE, LR = 300, 1500, 16, 3, 40, 5, 0.03
_GRAPH = {}


def _graph():
    if not _GRAPH:
        g = torch.Generator().manual_seed(21)
        x = torch.randn(N, FEAT, generator=g)
        ei = torch.randint(0, N, (2, E), generator=g)
        y = torch.randint(0, CLASSES, (N,), generator=g)
        perm = torch.randperm(N, generator=g)
        masks = torch.zeros(3, 3, N, dtype=torch.bool)                     # [mask row, {train, val, test}, N]
        for r in range(3):
            p = perm.roll(37 * r)
            masks[r, 0, p[:120]] = True
            masks[r, 1, p[120:200]] = True
            masks[r, 2, p[180:290]] = True                                 # test overlaps val; 10 nodes in no split
        _GRAPH.update(x=x.to(DEV), ei=ei.to(DEV), y=y.to(DEV), masks=masks.to(DEV))
    return _GRAPH["x"], _GRAPH["ei"], _GRAPH["y"], _GRAPH["masks"]


_PRISTINE = {}


def _model(kind, dropout, seed=3):
    """a copy of ONE initial model per (kind, dropout): KANLinear's initial spline weights come from a least-squares solve on the host
    that does not return the same bits twice for the same seed, so equal starting points are copies, never rebuilds"""
    if (kind, dropout) not in _PRISTINE:
        torch.manual_seed(seed)
        if kind == "kan-gin":
            _PRISTINE[kind, dropout] = kagnn_amd.GKAN_Nodes("gin", 2, FEAT, 16, CLASSES, dropout=dropout)
        else:
            _PRISTINE[kind, dropout] = kagnn_amd.GFASTKAN_Nodes("gcn", 2, FEAT, 16, CLASSES, dropout=dropout)
    return copy.deepcopy(_PRISTINE[kind, dropout]).to(DEV)


def _acc(out, y, mask):
    pred = out.argmax(dim=1)
    return int((pred[mask] == y[mask]).sum()) / int(mask.sum())


def _script(model, x, ei, y, train_mask, val_mask, test_mask, epochs, lr, patience, loss_of=None, trace=None):
    """the reference's loop in this file's words: boolean indexing, torch's CrossEntropyLoss and Adam, a host stopper, state_dict clones"""
    saved = {k: v.detach().clone() for k, v in model.state_dict().items()}
    if test_mask is None:
        test_mask = val_mask
    lowest, misses, best, ran, stopped = float("inf"), 0, -1, 0, False
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    criterion = torch.nn.CrossEntropyLoss()
    model.train()
    out = None
    for epoch in range(epochs):
        opt.zero_grad()
        out = model(x, ei)
        loss = criterion(out[train_mask], y[train_mask]) if loss_of is None else loss_of(out, y, train_mask)
        loss.backward()
        opt.step()
        with torch.no_grad():
            out = model(x, ei)
            val_loss = criterion(out[val_mask], y[val_mask])
        ran += 1
        if trace is not None:
            trace.append((float(val_loss), float(lowest)))
        if val_loss < lowest:
            lowest, misses, best = val_loss, 0, epoch
            saved = {k: v.detach().clone() for k, v in model.state_dict().items()}
        elif val_loss >= lowest + 0:
            misses += 1
            if misses >= patience:
                stopped = True
                break
    model.load_state_dict(saved)
    return dict(train_acc=_acc(out, y, train_mask), val_acc=_acc(out, y, val_mask), test_acc=_acc(out, y, test_mask),
                val_loss=float(criterion(out[val_mask], y[val_mask])), out=out, epochs_run=ran, best_epoch=best, stopped=stopped)


def _same_state(a, b, what=""):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), f"{what}: {k}"


FIELDS = ("train_acc", "val_acc", "val_loss", "test_acc", "epochs_run", "best_epoch", "stopped")


def _fields(res):
    return tuple(getattr(res, k) for k in FIELDS)


@pytest.mark.parametrize("dropout", [0.0, 0.3])
@pytest.mark.parametrize("kind", ["kan-gin", "fastkan-gcn"])
def test_the_loop_with_the_scripts_loss_and_optimiser_is_the_script_bit_for_bit(kind, dropout):
    x, ei, y, masks = _graph()
    tr, va, te = masks[0]
    ma = _model(kind, dropout)
    mb = copy.deepcopy(ma)
    trace = []
    torch.manual_seed(77)
    want = _script(mb, x, ei, y, tr, va, te, EPOCHS, LR, PATIENCE, trace=trace)
    # precondition, from the restated loop alone: wherever the decision depends on the order of two losses they differ by more than
    # 1e-5 relative -- far above the rounding by which the two ways of taking the mean may differ
    for e, (v, lowest) in enumerate(trace):
        assert math.isinf(lowest) or abs(v - lowest) > 1e-5 * abs(lowest), (e, v, lowest)
    torch.manual_seed(77)
    got = harness.train_node_classification(ma, x, ei, y, tr, va, te, epochs=EPOCHS, lr=LR, patience=PATIENCE, poll_every=1,
                                            optimizer=torch.optim.Adam(ma.parameters(), lr=LR), loss_fn=torch.nn.CrossEntropyLoss())
    print(f"{kind} dropout {dropout}: script {[(k, want[k]) for k in FIELDS]} device {got}")
    _same_state(ma, mb, f"{kind} dropout {dropout}")
    assert (got.best_epoch, got.epochs_run, got.stopped) == (want["best_epoch"], want["epochs_run"], want["stopped"])
    assert (got.train_acc, got.val_acc, got.test_acc) == (want["train_acc"], want["val_acc"], want["test_acc"])
    out = want["out"].cpu()
    ref = float(F.cross_entropy(out.double()[va.cpu()], y.cpu()[va.cpu()]))
    e32 = abs(float(F.cross_entropy(out[va.cpu()], y.cpu()[va.cpu()])) - ref)
    assert abs(got.val_loss - ref) <= max(4.0 * e32, 1e-6 * abs(ref)), (got.val_loss, ref, e32)
    assert got.history.shape == (got.epochs_run, 3, 3) and ma.training
    assert 0 <= got.best_epoch < got.epochs_run <= EPOCHS
    if dropout == 0.0:
        assert got.stopped and got.epochs_run < EPOCHS                   # (the case the polling test stops early on)


@pytest.mark.parametrize("kind", ["kan-gin", "fastkan-gcn"])
def test_first_step_gradients_of_the_native_loss_against_the_scripts(kind):
    x, ei, y, masks = _graph()
    tr, va, te = masks[0]
    ma = _model(kind, 0.0)
    mb = copy.deepcopy(ma)
    harness.train_node_classification(ma, x, ei, y, tr, va, te, epochs=1, lr=LR, patience=PATIENCE)
    mb.train()
    F.cross_entropy(mb(x, ei)[tr], y[tr]).backward()
    wants = {k: p.grad for k, p in mb.named_parameters() if p.grad is not None}
    checked = 0
    for name, p in ma.named_parameters():
        if not p.requires_grad:
            continue
        assert p.grad is not None and name in wants, name
        assert_close(p.grad, wants[name], what=f"{kind} first-step grad {name}", noise=prenorm_bias_noise(name, wants))
        checked += 1
    assert checked >= 6
    first = next(n for n, p in ma.named_parameters() if p.requires_grad)
    must_fail(torch.zeros_like(wants[first]), wants[first], what=f"{kind} first-step grad {first}")


def _run(kind, poll_every, **kw):
    x, ei, y, masks = _graph()
    tr, va, te = masks[0]
    m = _model(kind, 0.0)
    torch.manual_seed(78)
    res = harness.train_node_classification(m, x, ei, y, tr, va, te, poll_every=poll_every, **kw)
    return m, res


def test_polling_does_not_change_the_result():
    x, ei, y, masks = _graph()
    start = _model("kan-gin", 0.0)
    cases = {"stops early": dict(epochs=EPOCHS, lr=LR, patience=PATIENCE),
             "never stops": dict(epochs=12, lr=LR, patience=100),
             "never improves after the first epoch": dict(epochs=20, lr=0.0, patience=3)}
    for what, kw in cases.items():
        runs = [_run("kan-gin", p, **kw) for p in (1, 7, 64)]
        for m, res in runs[1:]:
            _same_state(m, runs[0][0], what)
            assert _fields(res) == _fields(runs[0][1]) and torch.equal(res.history, runs[0][1].history), what
        m, res = runs[0]
        print(f"{what}: {res}")
        if what == "stops early":
            assert res.stopped and res.epochs_run < EPOCHS and res.epochs_run == res.best_epoch + 1 + PATIENCE
            for mode in ("last", "best"):                                # the figures are those of the history's row
                r2 = _run("kan-gin", 7, metrics_at=mode, **kw)[1]
                at = r2.epochs_run - 1 if mode == "last" else r2.best_epoch
                xent, correct, rows = (r2.history[at, :, 0].view(torch.float64).tolist(), r2.history[at, :, 1].tolist(), r2.history[at, :, 2].tolist())
                assert (r2.train_acc, r2.val_acc, r2.test_acc) == tuple(c / r for c, r in zip(correct, rows))
                assert r2.val_loss == float(np.float32(xent[1] / rows[1])) and rows == [120, 80, 110]
        elif what == "never stops":
            assert not res.stopped and res.epochs_run == 12
        else:
            # lr = 0: the loss of epoch 0 is the only improvement, every later epoch repeats it exactly and counts as a miss
            assert res.stopped and res.best_epoch == 0 and res.epochs_run == 4
            for (k, p), (_, p0) in zip(m.named_parameters(), start.named_parameters()):
                assert torch.equal(p, p0), k                                 # the initial weights ...
            assert all(int(bn.num_batches_tracked) == 2 for bn in m.bns)     # ... and the running statistics as saved after epoch 0


# ------------------------------------------------------------------------------------------------ read-backs
class _Reads:
    """this file's counter of what brings a device value to the host (``item / tolist / cpu / numpy / to(cpu) / float() / int() /
    bool()``) and of explicit waits, tagged 'poll' inside ``EarlyStop.read`` and 'loop' elsewhere until ``flush_graph_checks``"""

    def __init__(self, monkeypatch):
        self.phase, self.log, self.polls = "loop", [], 0
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
        real_read, real_flush = ops.EarlyStop.read, ops.flush_graph_checks

        def read(stop, *a, **kw):
            was, outer.phase = outer.phase, "poll" if outer.phase == "loop" else outer.phase
            outer.polls += outer.phase == "poll"
            try:
                return real_read(stop, *a, **kw)
            finally:
                outer.phase = was

        def flush(*a, **kw):
            outer.phase = "after"
            return real_flush(*a, **kw)
        monkeypatch.setattr(ops.EarlyStop, "read", read)
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


def test_no_read_back_inside_the_loop(monkeypatch):
    x, ei, y, masks = _graph()
    tr, va, te = masks[0]
    _run("kan-gin", 16, epochs=2, lr=LR, patience=100)                   # (first use: packs, allocator, the graph index)
    torch.cuda.synchronize()
    # teeth: the script's loop reads at least once per epoch, and the counter sees it
    rd = _Reads(monkeypatch)
    _script(_model("kan-gin", 0.0), x, ei, y, tr, va, te, 6, LR, 100)
    assert len(rd.during("loop")) >= 6
    monkeypatch.undo()
    for poll_every, polls in ((4, 5), (1, 20), (64, 0)):
        m = _model("kan-gin", 0.0)
        with torch.no_grad():
            m(x, ei)                                                     # (a fresh model's first forward checks its knot grids once)
        rd = _Reads(monkeypatch)
        res = harness.train_node_classification(m, x, ei, y, tr, va, te, epochs=20, lr=LR, patience=100, poll_every=poll_every)
        monkeypatch.undo()
        assert res.epochs_run == 20
        assert rd.during("loop") == [], rd.during("loop")                # nothing between the polls
        assert rd.polls == polls and rd.during("poll") == ["cpu"] * polls   # exactly one read-back per poll
        assert rd.during("after").count("cpu") == 1                      # the record and the history, once, at the end


# ------------------------------------------------------------------------------------------------ all_splits, test_mask=None
# (the FastKAN architecture: its initialisation is reproducible from the seed, the KAN one's least-squares solve is not -- see _model)
PARAMS = dict(architecture="fastkan", conv_type="gcn", mp_layers=2, num_features=FEAT, hidden_channels=16, num_classes=CLASSES, skip=True,
              hidden_layers=2, dropout=0.0, grid_size=4, spline_order=3, epochs=15, lr=LR, patience=4)


def test_node_classification_splits_equals_separate_runs():
    x, ei, y, masks = _graph()
    torch.manual_seed(5)
    models, train_accs, val_accs, val_losses, test_accs = harness.node_classification_splits(PARAMS, x, ei, y, masks[:, 0], masks[:, 1], masks[:, 2])
    assert len(models) == 3 == len(train_accs) == len(val_accs) == len(val_losses) == len(test_accs)
    torch.manual_seed(5)
    figures = set()
    for r in range(3):
        m = harness.make_model(PARAMS).to(DEV)
        res = harness.train_node_classification(m, x, ei, y, masks[r, 0], masks[r, 1], masks[r, 2], epochs=15, lr=LR, patience=4)
        _same_state(models[r], m, f"split {r}")
        assert (train_accs[r], val_accs[r], val_losses[r], test_accs[r]) == (res.train_acc, res.val_acc, res.val_loss, res.test_acc)
        figures.add((res.train_acc, res.val_acc, res.val_loss, res.test_acc))
    assert len(figures) == 3                                             # three different splits, three different models
    assert not torch.equal(models[0].lay_out.base_linear.weight, models[1].lay_out.base_linear.weight)


def test_without_a_test_mask_the_validation_figures_are_reported():
    x, ei, y, masks = _graph()
    tr, va, te = masks[0]
    res = harness.train_node_classification(_model("kan-gin", 0.0), x, ei, y, tr, va, None, epochs=8, lr=LR, patience=100)
    assert res.test_acc == res.val_acc and torch.equal(res.history[:, 2], res.history[:, 1]) and res.history[0, 1, 2] == 80
    other = harness.train_node_classification(_model("kan-gin", 0.0), x, ei, y, tr, va, te, epochs=8, lr=LR, patience=100)
    assert other.val_acc == res.val_acc and other.val_loss == res.val_loss and other.history[0, 2, 2] == 110
    # an empty split: NaN figures, and a validation loss that is never below the minimum
    empty = torch.zeros_like(va)
    res = harness.train_node_classification(_model("kan-gin", 0.0), x, ei, y, tr, empty, te, epochs=6, lr=LR, patience=100)
    assert math.isnan(res.val_acc) and math.isnan(res.val_loss) and res.best_epoch == -1 and res.epochs_run == 6 and not res.stopped
