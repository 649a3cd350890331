"""Link prediction on the device (csrc/linkpred.hip and the Python layer around it): edge keys and the uniform negative sampler,
the dot-product decoder ``ops.pair_scores``, ``ops.bce_with_logits`` with its meter row, ``ops.link_rank`` and the loop
``harness.train_link_prediction``.

Integers are compared bit for bit with the restatements of tests/test_link_prediction_host.py (``negative_sample_reference``,
``edge_keys_reference``, ``rank_reference``).  Floats: pair scores and their gradient, and the BCE gradient, against fp64 at the
default bound of ``helpers.assert_close``; the BCE loss SUM within ``max(4 x E32, 1e-6 relative)`` of fp64, E32 being the error of
torch's own fp32 ``F.binary_cross_entropy_with_logits(reduction='sum')`` on the CPU (``node_eval``'s rule).  The loop is compared,
bit for bit, with the same loop written out here from the public pieces."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kagnn_amd
from kagnn_amd import data, harness, ops
from helpers import assert_close, must_fail
from test_gpu_node_classification import _Reads
from test_gpu_poison import _guard_case, _heap_case
from test_link_prediction_host import (GRAPHS, distinct_edges, edge_keys_reference, negative_sample_reference, rank_reference, roc_auc,
                                       roc_auc_by_sorting)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x0123456789ABCDEF                              # (both words of the seed in use)
NUMS = (1, 63, 64, 65, 1000)


# ---------------------------------------------------------------------------------------------------------------- sampler
def _sampler_graphs():
    rng = np.random.RandomState(8)
    out = {name: (distinct_edges(n, e, 11), n) for name, (n, e, _) in GRAPHS.items()}
    path = np.arange(9, dtype=np.int64)
    out["path"] = (np.concatenate([np.stack([path, path + 1]), np.stack([path + 1, path])], axis=1), 10)
    dup = rng.randint(0, 20, size=(2, 150)).astype(np.int64)
    dup[:, 100:] = dup[:, :50]                                             # duplicates; self loops come with the draw
    dup[:, 140:] = np.arange(10, dtype=np.int64)[None, :]                  # and ten self loops for certain
    out["duplicates and self loops"] = (dup, 20)
    out["70001 nodes"] = (np.stack([rng.randint(0, 70001, 200), rng.randint(0, 70001, 200)]).astype(np.int64), 70001)
    out["one node"] = (np.zeros((2, 3), dtype=np.int64), 1)
    out["no edges"] = (np.zeros((2, 0), dtype=np.int64), 50)
    out["first and last key"] = (np.array([[0, 3, 1], [1, 2, 2]], dtype=np.int64), 4)      # keys 1 and 14: the ends of the search
    return out


SAMPLER_GRAPHS = _sampler_graphs()


@pytest.mark.parametrize("name", list(SAMPLER_GRAPHS))
def test_negative_sample_equals_the_restatement_bit_for_bit(name):
    ei, n = SAMPLER_GRAPHS[name]
    keys_ref = edge_keys_reference(ei, n)
    keys = ops.edge_keys(torch.from_numpy(ei).to(DEV), n)
    assert keys.dtype == torch.int64 and np.array_equal(keys.cpu().numpy(), keys_ref), name
    if name == "70001 nodes":
        assert int(keys_ref.max()) > 1 << 32
    edges = set(keys_ref.tolist())
    for num in NUMS:
        for attempts in (1, 8):
            for seed in (SEED, 5):
                pairs, valid = ops.negative_sample(num, keys, n, seed, attempts)
                want_pairs, want_valid = negative_sample_reference(num, keys_ref, n, seed, attempts)
                what = f"{name}: num {num}, attempts {attempts}, seed {seed:#x}"
                assert pairs.dtype == torch.int64 and pairs.shape == (2, num) and valid.dtype == torch.uint8 and valid.shape == (num,)
                assert np.array_equal(pairs.cpu().numpy(), want_pairs) and np.array_equal(valid.cpu().numpy(), want_valid), what
                p, v = pairs.cpu().numpy(), valid.cpu().numpy() != 0
                assert bool((p[0, v] != p[1, v]).all()) and not edges & set((p[0, v] * n + p[1, v]).tolist()), what
                assert not p[:, ~v].any(), what
    first, again = ops.negative_sample(1000, keys, n, SEED, 8), ops.negative_sample(1000, keys, n, SEED, 8)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])           # two calls, the same bits
    if name == "one node":
        assert not bool(first[1].any())                                  # u == v every time: every slot is EMPTY
    if name == "7 nodes 30 edges":
        assert 0 < int(first[1].sum()) < 1000                            # the graph that leaves slots empty


@pytest.mark.parametrize("e", [1, 255, 256, 257, 5000])
def test_edge_keys_equal_torch_unique(e):
    n = 300
    gen = torch.Generator().manual_seed(e)
    ei = torch.randint(0, n, (2, e), generator=gen)
    if e > 100:
        ei[:, e // 2:e // 2 + 40] = ei[:, :40]                             # duplicates
    dev = ei.to(DEV)
    want = torch.unique(ei[0] * n + ei[1])
    assert torch.equal(ops.edge_keys(dev, n).cpu(), want)
    g = ops.GraphIndex(dev, n)
    keys = g.edge_keys
    assert torch.equal(keys.cpu(), want) and g.edge_keys is keys             # built once, kept
    pairs, valid = ops.negative_sample(500, g, n, 3)
    ref = negative_sample_reference(500, want.numpy(), n, 3)
    assert np.array_equal(pairs.cpu().numpy(), ref[0]) and np.array_equal(valid.cpu().numpy(), ref[1])
    with pytest.raises(RuntimeError, match="carries no edge list"):
        ops.GraphIndex.from_arrays(g.rowptr, g.col, g.perm, g.rowptr_t, g.col_t, g.perm_t, n, e).edge_keys


def _integer_ops_case():
    """the sampler, the key build and the ranking on fresh buffers: the heap-pattern and guard-band case of this family"""
    ei, n = SAMPLER_GRAPHS["40 nodes 300 edges"]
    dev = torch.from_numpy(ei).to(DEV)
    gen = torch.Generator().manual_seed(3)
    s = (torch.randn(4099, generator=gen) * 2).round().to(DEV)              # ties
    y = (torch.rand(4099, generator=gen) < 0.3).to(torch.uint8).to(DEV)
    w = (torch.rand(4099, generator=gen) < 0.9).to(torch.uint8).to(DEV)

    def run():
        keys = ops.edge_keys(dev, n)
        out = [keys]
        for num in (65, 1000):
            out += list(ops.negative_sample(num, keys, n, SEED, 8))
        out.append(ops.link_rank(s, y, w, ks=(5, 50, 500)))
        rec = torch.zeros(3, dtype=torch.int64, device=DEV)
        out.append(ops.bce_with_logits(s, y, w, accumulate=rec).reshape(1))
        out.append(rec)
        big = ops.bce_with_logits(s.repeat(3), y.repeat(3), w.repeat(3), accumulate=rec)      # (above 4096 rows: the two-stage path)
        return out + [big.reshape(1), rec.clone()]
    return None, run


INTEGER_CASES = {"link prediction integer ops": ("split", _integer_ops_case, 8)}


def test_the_integer_ops_are_blind_to_the_heap(monkeypatch):
    _heap_case(monkeypatch, INTEGER_CASES, "link prediction integer ops")


def test_the_integer_ops_write_inside_their_buffers(monkeypatch):
    _guard_case(monkeypatch, INTEGER_CASES, "link prediction integer ops")


# ---------------------------------------------------------------------------------------------------------------- pair scores
WIDTHS = (1, 3, 4, 16, 64, 100, 256, 260)


def _pair_sets():
    gen = torch.Generator().manual_seed(21)
    plain = torch.randint(0, 300, (2, 2000), generator=gen)
    plain[:, 1900:] = plain[:, :100]                                       # duplicate pairs
    plain[1, 1800:1850] = plain[0, 1800:1850]                              # self pairs
    hub = torch.randint(0, 300, (2, 2600), generator=gen)
    hub[1, :1613] = 7                                                      # node 7 is the destination of 1613 pairs: hub segments
    hub[0, 2000:2300] = 11                                                 # and node 11 the source of 300
    return {"2000 pairs": plain, "1613-pair node": hub}


PAIR_SETS = _pair_sets()


def _scores64(z, pairs, gs):
    z64 = z.detach().double().cpu().requires_grad_(True)
    s = (z64.index_select(0, pairs[0]) * z64.index_select(0, pairs[1])).sum(1)
    (s * gs.double().cpu()).sum().backward()
    return s.detach(), z64.grad


@pytest.mark.parametrize("small", [True, False], ids=["small-graph build", "rocPRIM build"])
@pytest.mark.parametrize("name", list(PAIR_SETS))
def test_pair_scores_and_their_gradient_against_fp64(monkeypatch, name, small):
    monkeypatch.setattr(ops, "_SMALL_CSR", small)
    pairs = PAIR_SETS[name]
    p = pairs.size(1)
    dev_pairs = pairs.to(DEV)
    index = ops.pair_index(dev_pairs, 300)
    assert (index.num_hub_seg > 0) == (name == "1613-pair node" and not small)
    gen = torch.Generator().manual_seed(22)
    for d in WIDTHS:
        z = torch.randn(300, d, generator=gen).to(DEV).requires_grad_(True)
        gs = torch.randn(p, generator=gen).to(DEV)
        want_s, want_g = _scores64(z, pairs, gs)
        for given in (dev_pairs, index):
            z.grad = None
            s = ops.pair_scores(z, given)
            assert s.dtype == torch.float32 and s.shape == (p,)
            s.backward(gs)
            assert_close(s, want_s, what=f"{name} d={d} scores")
            assert_close(z.grad, want_g, what=f"{name} d={d} z.grad")
        first = (s.detach().clone(), z.grad.clone())
        z.grad = None
        s = ops.pair_scores(z, index)
        s.backward(gs)
        assert torch.equal(s, first[0]) and torch.equal(z.grad, first[1]), f"{name} d={d}: two calls differ"
    must_fail(torch.zeros_like(want_g), want_g, what=f"{name} z.grad")


def test_pair_scores_of_a_strided_z_of_no_pairs_and_the_refusals():
    gen = torch.Generator().manual_seed(23)
    pairs = PAIR_SETS["2000 pairs"]
    wide = torch.randn(300, 40, generator=gen).to(DEV)
    for lo, hi in ((0, 16), (3, 20), (8, 40)):
        z = wide[:, lo:hi].detach().requires_grad_(True)                   # (a leaf that is a strided view)
        assert not z.is_contiguous()
        gs = torch.randn(2000, generator=gen).to(DEV)
        want_s, want_g = _scores64(z, pairs, gs)
        s = ops.pair_scores(z, pairs.to(DEV))
        s.backward(gs)
        assert_close(s, want_s, what=f"strided z[{lo}:{hi}] scores")
        assert_close(z.grad, want_g, what=f"strided z[{lo}:{hi}] grad")
    z = torch.randn(300, 8, generator=gen).to(DEV).requires_grad_(True)
    s = ops.pair_scores(z, torch.zeros((2, 0), dtype=torch.int64, device=DEV))
    assert s.shape == (0,) and s.dtype == torch.float32
    s.sum().backward()
    assert z.grad.shape == z.shape and not bool(z.grad.any())
    with pytest.raises(ValueError, match="describes 300 nodes"):
        ops.pair_scores(z[:200], ops.pair_index(pairs.to(DEV), 300))
    model = kagnn_amd.LinkPredictor(torch.nn.Identity())
    assert torch.equal(model.decode(z, pairs.to(DEV)), ops.pair_scores(z, pairs.to(DEV)))


def test_dropping_either_backward_aggregation_is_caught(monkeypatch):
    pairs = PAIR_SETS["2000 pairs"]
    gen = torch.Generator().manual_seed(24)
    z = torch.randn(300, 16, generator=gen).to(DEV).requires_grad_(True)
    gs = torch.randn(2000, generator=gen).to(DEV)
    _, want_g = _scores64(z, pairs, gs)
    index = ops.pair_index(pairs.to(DEV), 300)
    real = ops._aggregate_csr
    for drop in ("by destination", "by source"):
        def mutant(x, *a, addend=None, **kw):
            if drop == "by destination" and addend is None:
                return torch.zeros_like(x)                                  # the first aggregation contributes nothing
            if drop == "by source" and addend is not None:
                return addend.clone()                                       # the second adds nothing to the first
            return real(x, *a, addend=addend, **kw)
        monkeypatch.setattr(ops, "_aggregate_csr", mutant)
        z.grad = None
        ops.pair_scores(z, index).backward(gs)
        monkeypatch.undo()
        must_fail(z.grad, want_g, what=f"z.grad without the aggregation {drop}")
    z.grad = None
    ops.pair_scores(z, index).backward(gs)
    assert_close(z.grad, want_g, what="z.grad, both aggregations")


# ---------------------------------------------------------------------------------------------------------------- BCE
def _bce_case(p, seed):
    gen = torch.Generator().manual_seed(seed)
    s = 3.0 * torch.randn(p, generator=gen)
    special = torch.tensor([50.0, -50.0, 100.0, -100.0, 0.0])
    s[:min(p, 5)] = special[:min(p, 5)]
    if p > 10:
        s[5:10] = special                                                  # (each special value with both labels, very likely)
    y = (torch.rand(p, generator=gen) < 0.5).to(torch.uint8)
    w = (torch.rand(p, generator=gen) < 0.8).to(torch.uint8)
    return s, y, w


def _bce_reference(s, y, w):
    keep = w != 0
    s64, y64 = s.double()[keep], y.double()[keep]
    total = float(F.binary_cross_entropy_with_logits(s64, y64, reduction="sum")) if keep.any() else 0.0
    e32 = abs(float(F.binary_cross_entropy_with_logits(s[keep], y[keep].float(), reduction="sum")) - total) if keep.any() else 0.0
    correct = int(((s[keep] > 0) == (y[keep] != 0)).sum())
    return total, e32, correct, int(keep.sum())


@pytest.mark.parametrize("p", [1, 257, 4096, 4097, 70001])
def test_bce_with_logits_loss_counts_and_gradient(p):
    s, y, w = _bce_case(p, p)
    for weight in (None, w):
        wt = torch.ones_like(y) if weight is None else weight
        if p == 1:
            wt = torch.ones_like(y)
        total, e32, correct, rows = _bce_reference(s, y, wt)
        sd = s.to(DEV).requires_grad_(True)
        rec = torch.full((1, 3), -1, dtype=torch.int64, device=DEV)
        loss = ops.bce_with_logits(sd, y.to(DEV), None if weight is None else wt.to(DEV), accumulate=rec)
        loss.backward()
        host = rec.cpu()[0]
        got_sum = float(host[:1].view(torch.float64)[0])
        print(f"P={p} weighted={weight is not None}: sum {got_sum!r} fp64 {total!r} E32 {e32:.3e} err {abs(got_sum - total):.3e}")
        assert abs(got_sum - total) <= max(4.0 * e32, 1e-6 * abs(total)), (got_sum, total, e32)
        assert (int(host[1]), int(host[2])) == (correct, rows)
        assert float(loss.detach()) == float(np.float32(got_sum / max(rows, 1)))     # the mean, rounded once
        s64 = s.double().requires_grad_(True)
        keep = wt != 0
        (F.binary_cross_entropy_with_logits(s64[keep], y.double()[keep], reduction="sum") / max(rows, 1)).backward()
        assert_close(sd.grad, s64.grad, what=f"BCE gradient P={p}")
        assert not bool(sd.grad.cpu()[~keep].any())
        # without the meter: the same loss, bit for bit
        assert torch.equal(ops.bce_with_logits(sd.detach(), y.to(DEV), None if weight is None else wt.to(DEV)), loss.detach())
    if p > 1:                                                              # (one row at +50: the gradient itself is below 1e-21)
        must_fail(torch.zeros_like(s64.grad), s64.grad, what="BCE gradient")


def test_bce_weight_zero_rows_change_nothing_and_the_degenerate_cases():
    s, y, w = _bce_case(5000, 9)
    keep = w != 0
    rec_a, rec_b = torch.zeros(3, dtype=torch.int64, device=DEV), torch.zeros(3, dtype=torch.int64, device=DEV)
    a = ops.bce_with_logits(s.to(DEV), y.to(DEV), w.to(DEV), accumulate=rec_a)
    other = s.clone()
    other[~keep] = torch.tensor([float("nan"), float("inf"), -1e30, 7.0]).repeat(int((~keep).sum()) // 4 + 1)[:int((~keep).sum())]
    flipped = y.clone()
    flipped[~keep] ^= 1
    b = ops.bce_with_logits(other.to(DEV), flipped.to(DEV), w.to(DEV), accumulate=rec_b)
    assert torch.equal(a, b) and torch.equal(rec_a, rec_b)                  # whatever a weight-0 row holds
    # every weight 0: loss 0, gradient 0, an empty record
    sd = other.to(DEV).requires_grad_(True)
    rec = torch.full((3,), -1, dtype=torch.int64, device=DEV)
    loss = ops.bce_with_logits(sd, y.to(DEV), torch.zeros_like(w).to(DEV), accumulate=rec)
    loss.backward()
    assert float(loss.detach()) == 0.0 and not bool(sd.grad.any()) and rec.tolist() == [0, 0, 0]
    # a NaN score of weight 1: the sum is NaN, the counts are those of the rule (s > 0) == y, the other gradients are untouched
    bad = s.clone()
    at = int(keep.nonzero()[3])
    bad[at] = float("nan")
    sd = bad.to(DEV).requires_grad_(True)
    loss = ops.bce_with_logits(sd, y.to(DEV), w.to(DEV), accumulate=rec)
    loss.backward()
    host = rec.cpu()
    assert np.isnan(float(loss.detach())) and np.isnan(float(host[:1].view(torch.float64)[0]))
    assert (int(host[1]), int(host[2])) == (int(((bad[keep] > 0) == (y[keep] != 0)).sum()), int(keep.sum()))
    good = s.to(DEV).requires_grad_(True)
    ops.bce_with_logits(good, y.to(DEV), w.to(DEV)).backward()
    grad, ref = sd.grad.cpu(), good.grad.cpu()
    assert np.isnan(float(grad[at])) and torch.equal(torch.cat([grad[:at], grad[at + 1:]]), torch.cat([ref[:at], ref[at + 1:]]))


def test_the_bce_record_drives_the_early_stopper():
    """the stopper's rule on the host, fed the fp64 means of the same five score vectors (far apart: no decision is borderline)"""
    s, y, w = _bce_case(300, 4)
    stop = ops.EarlyStop(2, 0.0, max_epochs=6, num_splits=1, device=DEV)
    rec = torch.zeros((1, 3), dtype=torch.int64, device=DEV)
    lowest, misses, best, ran, stopped = float("inf"), 0, -1, 0, False
    for scale in (1.0, 0.5, 0.1, 2.0, 3.0, 4.0):
        ops.bce_with_logits((s * scale).to(DEV), y.to(DEV), w.to(DEV), accumulate=rec)
        stop.update(rec, 0)
        total, _, _, rows = _bce_reference(s * scale, y, w)
        if not stopped:
            ran += 1
            if total / rows < lowest:
                lowest, misses, best = total / rows, 0, ran - 1
            else:
                misses += 1
                stopped = misses >= 2
    st = stop.read()
    assert (st.epochs, st.best_epoch, st.stopped) == (ran, best, stopped) and stopped and ran < 6
    assert st.history.shape == (ran, 1, 3) and bool((st.history[:, 0, 2] == int((w != 0).sum())).all())


# ---------------------------------------------------------------------------------------------------------------- ranking
def _rank_cases():
    rng = np.random.RandomState(31)
    cases = {}
    for p in (1, 2, 255, 256, 257, 4099):
        cases[f"random P={p}"] = (rng.randn(p).astype(np.float32), (rng.rand(p) < 0.4), None)
    p = 4099
    y = rng.rand(p) < 0.4
    cases["8 levels"] = (rng.randint(0, 8, p).astype(np.float32) - 3.0, y, None)
    cases["all equal"] = (np.full(p, 1.25, dtype=np.float32), y, None)
    one_pos = np.zeros(p, dtype=bool); one_pos[17] = True
    cases["one positive"] = (rng.randn(p).astype(np.float32), one_pos, None)
    cases["one negative"] = (rng.randn(p).astype(np.float32), ~one_pos, None)
    cases["only positives"] = (rng.randn(300).astype(np.float32), np.ones(300, dtype=bool), None)
    zeros = np.where(rng.rand(p) < 0.5, 0.0, -0.0).astype(np.float32)
    zeros[::7] = rng.randn(zeros[::7].size).astype(np.float32) * 1e-3
    cases["zeros of both signs"] = (zeros, y, None)
    inf = rng.randn(p).astype(np.float32)
    inf[::5], inf[1::11] = np.inf, -np.inf
    cases["infinities"] = (inf, y, None)
    nan = rng.randint(-4, 4, p).astype(np.float32)
    nan[::9] = np.nan
    cases["NaN rows"] = (nan, y, rng.rand(p) < 0.9)
    cases["weight-0 rows"] = (rng.randint(-4, 4, p).astype(np.float32), y, rng.rand(p) < 0.5)
    cases["k above n_neg"] = (rng.randn(60).astype(np.float32), rng.rand(60) < 0.7, None)
    return cases


RANK_CASES = _rank_cases()


@pytest.mark.parametrize("name", list(RANK_CASES))
def test_link_rank_equals_the_quadratic_definition(name):
    s, y, w = RANK_CASES[name]
    sd, yd = torch.from_numpy(s).to(DEV), torch.from_numpy(y.astype(np.uint8)).to(DEV)
    wd = None if w is None else torch.from_numpy(w.astype(np.uint8)).to(DEV)
    for ks in ((20, 50, 100), (1, 2, 3), (5,), ()):
        want = rank_reference(s, y, w, ks)
        got = ops.link_rank(sd, yd, wd, ks=ks)
        assert got.dtype == torch.int64 and got.shape == (8,)
        assert got.cpu().tolist() == want.tolist(), (name, ks, got.cpu().tolist(), want.tolist())
        assert torch.equal(ops.link_rank(sd, yd, wd, ks=ks), got)
    out = torch.full((3, 8), -7, dtype=torch.int64, device=DEV)
    assert ops.link_rank(sd, yd, wd, out=out[1]).data_ptr() == out[1].data_ptr()
    assert out[1].cpu().tolist() == rank_reference(s, y, w).tolist() and bool((out[0] == -7).all()) and bool((out[2] == -7).all())
    if name == "zeros of both signs":
        # a key transform that separates -0.0 from +0.0 must fail here: the same scores with every zero made positive give the same record
        assert int(((s == 0) & np.signbit(s) & y).sum()) > 100 and int(((s == 0) & ~np.signbit(s) & ~y).sum()) > 100
        separated = rank_reference(np.where((s == 0) & np.signbit(s), np.float32(-1e-30), s), y, w)
        assert separated[0] != rank_reference(s, y, w)[0]
    if name == "k above n_neg":
        fig = ops.link_rank_figures(ops.link_rank(sd, yd, wd, ks=(100,)), ks=(100,))
        assert fig["hits"][100] == 1.0 and fig["n_neg"] < 100
    if name == "only positives":
        assert np.isnan(ops.link_rank_figures(got)["auc"])


def test_link_rank_at_70001_rows_against_the_sort_based_auc():
    rng = np.random.RandomState(32)
    s = rng.permutation(70001).astype(np.float32) * 0.25 - 9000.0         # tie-free, exactly representable
    y = rng.rand(70001) < 0.45
    got = ops.link_rank(torch.from_numpy(s).to(DEV), torch.from_numpy(y.astype(np.uint8)).to(DEV)).cpu()
    n_pos, n_neg = int(y.sum()), int((~y).sum())
    two_u = round(roc_auc_by_sorting(s, y) * 2 * n_pos * n_neg)
    assert abs(roc_auc_by_sorting(s, y) * 2 * n_pos * n_neg - two_u) < 1e-3 and two_u % 2 == 0       # no ties: 2U is even
    assert got.tolist()[:4] == [two_u, n_pos, n_neg, 0]
    order = np.sort(s[~y])
    assert got.tolist()[4:7] == [int((s[y] > order[-k]).sum()) for k in (20, 50, 100)]
    assert abs(roc_auc(got.numpy()) - roc_auc_by_sorting(s, y)) <= 1e-12
    assert torch.equal(ops.link_rank(torch.from_numpy(s).to(DEV), torch.from_numpy(y.astype(np.uint8)).to(DEV)).cpu(), got)


# ---------------------------------------------------------------------------------------------------------------- the loop
LN, LF, LR, KS = 80, 12, 0.01, (5, 10, 20)
_LOOP = {}


def _loop_graph():
    """80 nodes in two communities of 40, about 400 undirected edges (dense inside, sparse across), features that tell them apart"""
    if "graph" not in _LOOP:
        rng = np.random.RandomState(41)
        u, v = np.triu_indices(LN, 1)
        same = (u < 40) == (v < 40)
        take = rng.rand(u.size) < np.where(same, 0.24, 0.012)
        und = np.stack([u[take], v[take]]).astype(np.int64)
        ei = torch.from_numpy(np.concatenate([und, und[::-1]], axis=1)).contiguous()
        x = torch.randn(LN, LF, generator=torch.Generator().manual_seed(42)) * 0.5
        x[:40, 0] += 1.0
        x[40:, 1] += 1.0
        split = data.random_link_split(ei.to(DEV), LN, 0.1, 0.2, generator=torch.Generator().manual_seed(43))
        _LOOP["graph"] = (x.to(DEV), ei.to(DEV), split.with_negatives(7))
    return _LOOP["graph"]


def _encoder(kind):
    if ("model", kind) not in _LOOP:
        torch.manual_seed(44)
        if kind == "kan-gcn":
            enc = kagnn_amd.GKAN_Nodes("gcn", 2, LF, 16, 16)
        elif kind == "fastkan-gin":
            enc = kagnn_amd.GFASTKAN_Nodes("gin", 2, LF, 16, 16)
        else:
            enc = kagnn_amd.GNN_Nodes("gcn", 2, LF, 16, 16)
        _LOOP["model", kind] = kagnn_amd.LinkPredictor(enc)
    return copy.deepcopy(_LOOP["model", kind]).to(DEV)


def _written_out(model, x, split, epochs, patience, seed, neg_log=None):
    """``train_link_prediction`` from the public pieces, one statement per step of its docstring"""
    n = split.num_nodes
    u8 = dict(dtype=torch.uint8, device=DEV)
    g = ops.graph_index(split.train_edge_index, n)
    keys = ops.edge_keys(split.train_edge_index, n)
    p_train = split.train_pos.size(1)
    pos = ops.GraphIndex(split.train_pos, n)
    y_train = torch.cat([torch.ones(p_train, **u8), torch.zeros(p_train, **u8)])
    val = ops.GraphIndex(torch.cat([split.val_pos, split.val_neg], dim=1).contiguous(), n)
    y_val = torch.cat([torch.ones(split.val_pos.size(1), **u8), torch.zeros(split.val_neg.size(1), **u8)])
    w_val = torch.cat([torch.ones(split.val_pos.size(1), **u8), split.val_neg_valid])
    optimizer = harness.Adam(model.parameters(), lr=LR)
    best = harness._BestWeights(model, "test")
    stop = ops.EarlyStop(patience, 0.0, max_epochs=epochs, num_splits=1, device=DEV)
    record = torch.zeros((1, 3), dtype=torch.int64, device=DEV)
    ranks = torch.zeros((epochs, 8), dtype=torch.int64, device=DEV)
    step = harness._training_step(optimizer)

    def loss_of(neg, valid):
        z = model.encode(x, g)
        scores = torch.cat([ops.pair_scores(z, pos), ops.pair_scores(z, neg)])
        return ops.bce_with_logits(scores, y_train, torch.cat([torch.ones(p_train, **u8), valid]))
    for epoch in range(epochs):
        neg, valid = ops.negative_sample(p_train, keys, n, seed + 16 * (epoch + 1))
        if neg_log is not None:
            neg_log.append((neg.cpu().numpy(), valid.cpu().numpy()))
        model.train()
        step(loss_of, neg, valid)
        model.eval()
        with torch.no_grad():
            scores = ops.pair_scores(model.encode(x, g), val)
        ops.bce_with_logits(scores, y_val, w_val, accumulate=record)
        ops.link_rank(scores, y_val, w_val, KS, out=ranks[epoch])
        stop.update(record, 0)
        ops.copy_if(stop.improved, best.saved, best.live)
        if stop.read(history=False).stopped:
            break
    st = stop.read()
    best.restore()
    model.train()
    return st, ranks[:st.epochs].cpu()


def _same_state(a, b, what):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), f"{what}: {k}"


def _untrained_auc(model, x, split):
    n = split.num_nodes
    model.eval()
    with torch.no_grad():
        scores = model(x, split.train_edge_index, torch.cat([split.val_pos, split.val_neg], dim=1).contiguous())
    y = torch.cat([torch.ones(split.val_pos.size(1)), torch.zeros(split.val_neg.size(1))]).to(torch.uint8).to(DEV)
    model.train()
    return ops.link_rank_figures(ops.link_rank(scores, y, torch.cat([torch.ones_like(split.val_neg_valid), split.val_neg_valid])))["auc"], n


def _three_ways(epochs, patience, seed, log=None):
    """the device loop polled every 16 epochs, the loop written out above, the device loop polled every epoch: one result"""
    x, ei, split = _loop_graph()
    ma, mb, mc = _encoder("kan-gcn"), _encoder("kan-gcn"), _encoder("kan-gcn")
    got = harness.train_link_prediction(ma, x, split, epochs=epochs, lr=LR, patience=patience, poll_every=16, seed=seed, ks=KS)
    st, ranks = _written_out(mb, x, split, epochs, patience, seed, log)
    print(f"epochs {epochs}, patience {patience}: {got}")
    _same_state(ma, mb, "loop against the written-out loop")
    assert (got.epochs_run, got.best_epoch, got.stopped) == (st.epochs, st.best_epoch, st.stopped)
    assert torch.equal(got.history, st.history) and torch.equal(got.rank_history, ranks)
    assert got.history.shape == (got.epochs_run, 1, 3) and got.rank_history.shape == (got.epochs_run, 8) and ma.training
    one = harness.train_link_prediction(mc, x, split, epochs=epochs, lr=LR, patience=patience, poll_every=1, seed=seed, ks=KS)
    _same_state(ma, mc, "poll_every 16 against 1")
    assert (one.epochs_run, one.best_epoch, one.stopped) == (got.epochs_run, got.best_epoch, got.stopped)
    assert torch.equal(one.history, got.history) and torch.equal(one.rank_history, got.rank_history)
    assert (one.val_loss, one.val_auc, one.test_loss, one.test_auc, one.test_hits) == (got.val_loss, got.val_auc, got.test_loss, got.test_auc, got.test_hits)
    return got


def test_the_loop_with_a_short_patience_is_the_loop_written_out_whatever_the_polling():
    got = _three_ways(25, 2, 5)
    assert 0 <= got.best_epoch < got.epochs_run <= 25 and (got.stopped or got.epochs_run == 25)
    if got.stopped:
        assert got.epochs_run == got.best_epoch + 1 + 2


def test_the_loop_is_the_loop_written_out_whatever_the_polling():
    x, ei, split = _loop_graph()
    assert 330 <= ei.size(1) // 2 <= 470 and split.val_neg.shape == split.val_pos.shape
    epochs, seed = 60, 3
    before, _ = _untrained_auc(_encoder("kan-gcn"), x, split)
    log = []
    got = _three_ways(epochs, 100, seed, log)
    print(f"untrained validation AUC {before:.4f}")
    assert got.epochs_run == epochs and not got.stopped
    # every epoch's training negatives are the restatement's at the documented seed, and no slot is empty: with 80 nodes and ~640
    # training edges the share of empty slots at 8 attempts is (1 - free / N^2)^8 < 1e-6
    keys = edge_keys_reference(split.train_edge_index.cpu().numpy(), LN)
    free = LN * LN - LN - keys.size
    assert (1.0 - free / (LN * LN)) ** 8 < 1e-6
    p_train = split.train_pos.size(1)
    for epoch, (neg, valid) in enumerate(log):
        want = negative_sample_reference(p_train, keys, LN, seed + 16 * (epoch + 1), 8)
        assert np.array_equal(neg, want[0]) and np.array_equal(valid, want[1]) and bool(valid.all()), epoch
    # the figures are the best epoch's, the test split's are finite, and training helped (a sanity check, not a tuned threshold)
    fig = ops.link_rank_figures(got.rank_history[got.best_epoch], KS)
    assert got.val_auc == fig["auc"] and got.val_hits == fig["hits"] and got.val_loss == harness._split_figures(got.history[got.best_epoch, 0])[0]
    assert 0.0 <= got.test_auc <= 1.0 and np.isfinite(got.test_loss) and set(got.test_hits) == set(KS)
    after = ops.link_rank_figures(got.rank_history[epochs - 1], KS)["auc"]
    print(f"validation AUC after {epochs} epochs {after:.4f}")
    assert after > before, (before, after)


@pytest.mark.parametrize("kind", ["fastkan-gin", "mlp-gcn"])
def test_three_epochs_of_the_other_encoders_against_the_written_out_loop(kind):
    x, ei, split = _loop_graph()
    ma, mb = _encoder(kind), _encoder(kind)
    got = harness.train_link_prediction(ma, x, split, epochs=3, lr=LR, patience=100, seed=11, ks=KS)
    st, ranks = _written_out(mb, x, split, 3, 100, 11)
    _same_state(ma, mb, kind)
    assert got.epochs_run == 3 == st.epochs and got.best_epoch == st.best_epoch and not got.stopped
    assert torch.equal(got.history, st.history) and torch.equal(got.rank_history, ranks)


def test_no_read_back_between_polls(monkeypatch):
    x, ei, split = _loop_graph()
    harness.train_link_prediction(_encoder("kan-gcn"), x, split, epochs=2, lr=LR, patience=100, ks=KS)      # (first use: packs, indexes)
    torch.cuda.synchronize()
    for poll_every, polls in ((4, 3), (1, 12), (64, 0)):
        m = _encoder("kan-gcn")
        with torch.no_grad():
            m.encode(x, split.train_edge_index)                             # (a fresh model's first forward checks its knot grids once)
        torch.cuda.synchronize()
        reads = []
        real = ops.negative_sample

        def sampled(*a, **kw):                                              # the phase 'loop' begins with the first epoch's negatives
            if not reads:
                reads.append(_Reads(monkeypatch))
            return real(*a, **kw)
        monkeypatch.setattr(ops, "negative_sample", sampled)
        res = harness.train_link_prediction(m, x, split, epochs=12, lr=LR, patience=100, poll_every=poll_every, ks=KS)
        monkeypatch.undo()
        rd = reads[0]
        assert res.epochs_run == 12
        assert rd.during("loop") == [], rd.during("loop")                   # nothing between the polls
        assert rd.polls == polls and rd.during("poll") == ["cpu"] * polls   # exactly one read-back per poll
