"""Link prediction, host side (no GPU): the restatements that tests/test_gpu_link_prediction.py holds the kernels to, what the
restated sampler does as a uniform sampler, ``random_link_split`` on CPU tensors, the refusals that come before any launch, and the
new entry points' place in the C ABI.

``negative_sample_reference`` is the rule of include/kagnn_hip.h (``kagnn_negative_sample``) in numpy: slot ``p``, attempt ``t``,
counter ``c = p T + t``, ``u = (key32(seed, 2c) N) >> 32``, ``v = (key32(seed, 2c + 1) N) >> 32``, the first attempt with ``u != v``
that is no edge.  Three graphs of E distinct directed non-self edges, seeds 0, 1 and 12345678901234567: every free pair must appear,
every count within 5 binomial standard deviations of ``filled / free`` (the bound of tests/test_gpu_neighbor_sampling.py), and the
share of EMPTY slots within 5 standard deviations of ``(1 - free / N^2)^T`` -- 5.2e-5 for (12, 30), 4.2e-6 for (40, 300) and 0.106
for (7, 30), the graph that exists to produce empty slots.  ``rank_reference`` is the O(P^2) definition of ``2U`` and hits@k in int64."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import kagnn_amd
from kagnn_amd import _lib, data, harness, ops
from test_neighbor_sampling_host import key32
from test_subgraph_host import _NoLaunch, _cpu_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"kagnn_edge_keys_workspace_bytes": 2, "kagnn_edge_keys_build": 9, "kagnn_negative_sample": 9, "kagnn_bce_logits_fwd": 10,
         "kagnn_bce_logits_bwd": 8, "kagnn_link_rank_workspace_bytes": 2, "kagnn_link_rank": 10}
SEEDS = (0, 1, 12345678901234567)
# (N, E, slots): the three graphs of the uniformity check
GRAPHS = {"12 nodes 30 edges": (12, 30, 400_000), "40 nodes 300 edges": (40, 300, 2_000_000), "7 nodes 30 edges": (7, 30, 200_000)}


# ---------------------------------------------------------------------------------------------------------------- the restatements
def edge_keys_reference(edge_index, num_nodes):
    """ascending, duplicate-free ``src * N + dst`` of an int64 ``[2, E]`` array (numpy or CPU tensor)"""
    ei = np.asarray(edge_index, dtype=np.int64)
    return np.unique(ei[0] * np.int64(num_nodes) + ei[1])


def negative_sample_reference(num, keys, num_nodes, seed, attempts=8):
    """``(pairs int64 [2, num], valid uint8 [num])`` of ``kagnn_negative_sample`` for the sorted key array ``keys``"""
    keys = np.asarray(keys, dtype=np.int64)
    n = int(num_nodes)
    pairs, valid = np.zeros((2, num), dtype=np.int64), np.zeros(num, dtype=np.uint8)
    if n == 0:
        return pairs, valid
    todo = np.arange(num, dtype=np.int64)
    for t in range(attempts):
        if todo.size == 0:
            break
        c = todo * attempts + t
        u = ((key32(seed, 2 * c).astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
        v = ((key32(seed, 2 * c + 1).astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
        q = u * n + v
        edge = np.zeros(q.size, dtype=bool)
        if keys.size:
            at = np.searchsorted(keys, q)
            edge = (at < keys.size) & (keys[np.minimum(at, keys.size - 1)] == q)
        ok = (u != v) & ~edge
        pairs[0, todo[ok]], pairs[1, todo[ok]], valid[todo[ok]] = u[ok], v[ok], 1
        todo = todo[~ok]
    return pairs, valid


def rank_reference(scores, labels, weight=None, ks=(20, 50, 100)):
    """the int64 ``[8]`` record of ``kagnn_link_rank`` by the definition: every positive against every negative"""
    s = np.asarray(scores, dtype=np.float32)
    y = np.asarray(labels) != 0
    w = np.ones(s.size, dtype=bool) if weight is None else np.asarray(weight) != 0
    nan = np.isnan(s)
    pos, neg = s[w & ~nan & y], s[w & ~nan & ~y]
    two_u = 0
    for lo in range(0, pos.size, 1024):
        block = pos[lo:lo + 1024, None]
        two_u += 2 * int((block > neg[None, :]).sum(dtype=np.int64)) + int((block == neg[None, :]).sum(dtype=np.int64))
    hits = [0, 0, 0]
    for j, k in enumerate(ks):
        hits[j] = int(pos.size) if neg.size < k else int((pos > np.sort(neg)[neg.size - k]).sum())
    return np.array([two_u, pos.size, neg.size, int((w & nan).sum()), *hits, 0], dtype=np.int64)


def roc_auc(record):
    r = [int(v) for v in np.asarray(record).reshape(-1)]
    return r[0] / (2 * r[1] * r[2])


def roc_auc_by_sorting(scores, labels):
    """ROC-AUC in fp64 from mid-ranks: (sum of the positives' ranks - n_pos (n_pos + 1) / 2) / (n_pos n_neg)"""
    s = np.asarray(scores, dtype=np.float64) + 0.0                       # (-0.0 + 0.0 = +0.0)
    y = np.asarray(labels) != 0
    _, inverse, counts = np.unique(s, return_inverse=True, return_counts=True)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    rank = (first + (counts + 1) / 2.0)[inverse]                         # 1-based mid-rank
    n_pos, n_neg = int(y.sum()), int((~y).sum())
    return (rank[y].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg)


def distinct_edges(num_nodes, num_edges, seed):
    """``num_edges`` distinct directed non-self edges of ``num_nodes`` nodes, int64 ``[2, E]`` numpy, in random order"""
    n = num_nodes
    u, v = np.divmod(np.arange(n * n, dtype=np.int64), n)
    keep = np.nonzero(u != v)[0]
    pick = np.random.RandomState(seed).permutation(keep)[:num_edges]
    return np.stack([u[pick], v[pick]])


# ---------------------------------------------------------------------------------------------------------------- the sampler's statistics
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("graph", list(GRAPHS))
def test_the_restated_sampler_is_uniform_over_the_free_pairs_and_leaves_the_predicted_share_empty(graph, seed):
    n, e, slots = GRAPHS[graph]
    keys = edge_keys_reference(distinct_edges(n, e, 11), n)
    assert keys.size == e
    pairs, valid = negative_sample_reference(slots, keys, n, seed, 8)
    filled = valid != 0
    assert not pairs[:, ~filled].any()                                   # an EMPTY slot is the pair (0, 0)
    code = pairs[0, filled] * n + pairs[1, filled]
    counts = np.bincount(code, minlength=n * n)
    u, v = np.divmod(np.arange(n * n), n)
    free = (u != v) & ~np.isin(np.arange(n * n), keys)
    nfree, nfilled = int(free.sum()), int(filled.sum())
    assert nfree == n * n - n - e
    assert not counts[~free].any() and bool((counts[free] > 0).all())    # no edge, no self pair; every free pair appears
    p = 1.0 / nfree
    worst = float(np.abs(counts[free] - nfilled * p).max() / np.sqrt(nfilled * p * (1 - p)))
    q = (1.0 - nfree / (n * n)) ** 8
    empty = 1.0 - nfilled / slots
    dev = abs(empty - q) / np.sqrt(q * (1 - q) / slots)
    print(f"{graph} seed {seed}: worst pair {worst:.2f} sd; empty share {empty:.3e} against {q:.3e} ({dev:.2f} sd)")
    assert worst <= 5.0
    assert dev <= 5.0


def test_the_reference_takes_the_first_valid_attempt_and_is_a_pure_function():
    n = 9
    keys = edge_keys_reference(distinct_edges(n, 40, 3), n)
    a = negative_sample_reference(500, keys, n, 77, 8)
    b = negative_sample_reference(500, keys, n, 77, 8)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    one = negative_sample_reference(500, keys, n, 77, 1)
    took_first = one[1] != 0
    assert took_first.any() and not took_first.all()
    # with T = 1 slot p reads the counters 2p, 2p + 1; with T = 8 the counters 16p, 16p + 1: spelled out for three slots
    for p in (0, 7, 499):
        for T, got in ((1, one), (8, a)):
            want = None
            for t in range(T):
                c = p * T + t
                u, v = (int(key32(77, [2 * c])[0]) * n) >> 32, (int(key32(77, [2 * c + 1])[0]) * n) >> 32
                if u != v and u * n + v not in set(keys.tolist()):
                    want = (u, v)
                    break
            assert (int(got[0][0, p]), int(got[0][1, p]), int(got[1][p])) == ((*want, 1) if want else (0, 0, 0)), (p, T)
    assert not negative_sample_reference(64, np.zeros(0, dtype=np.int64), 1, 5, 8)[1].any()      # N = 1: u == v always
    assert negative_sample_reference(64, np.zeros(0, dtype=np.int64), 50, 5, 8)[1].mean() > 0.9  # E = 0: only self pairs fail


# ---------------------------------------------------------------------------------------------------------------- the ranking
def test_the_quadratic_auc_agrees_with_the_sort_based_one():
    rng = np.random.RandomState(4)
    for what, s in (("random", rng.randn(3001).astype(np.float32)), ("8 levels", rng.randint(0, 8, 3001).astype(np.float32)),
                    ("zeros of both signs", np.where(rng.rand(3001) < 0.5, 0.0, -0.0).astype(np.float32) * (rng.rand(3001) < 0.7))):
        y = (rng.rand(s.size) < 0.4).astype(np.uint8)
        rec = rank_reference(s, y)
        assert rec[1] + rec[2] == s.size and rec[3] == 0
        assert abs(roc_auc(rec) - roc_auc_by_sorting(s, y)) <= 1e-12, what
    rec = rank_reference(np.array([3.0, 2.0, 2.0, 1.0, np.nan, 5.0], dtype=np.float32), [1, 0, 1, 0, 1, 0], [1, 1, 1, 1, 1, 0], ks=(1, 2, 3))
    # positives 3, 2 against negatives 2, 1 (NaN row counted, weight-0 row gone): 3 > both (4), 2 == 2 (1), 2 > 1 (2)
    assert rec.tolist() == [7, 2, 2, 1, 1, 2, 2, 0]


# ---------------------------------------------------------------------------------------------------------------- random_link_split
def _undirected(n, m, seed):
    und = distinct_edges(n, 2 * m, seed)
    und = und[:, und[0] < und[1]][:, :m]
    ei = torch.from_numpy(np.concatenate([und, und[::-1]], axis=1))
    return ei[:, torch.randperm(ei.size(1), generator=torch.Generator().manual_seed(seed))].contiguous()


def _codes(pairs, n):
    return set((pairs[0] * n + pairs[1]).tolist())


def test_random_link_split_on_cpu_tensors():
    n = 60
    ei = _undirected(n, 400, 5)
    e_rep = ei.size(1) // 2
    sp = data.random_link_split(ei, n, 0.05, 0.1, generator=torch.Generator().manual_seed(9))
    assert isinstance(sp, kagnn_amd.LinkSplit) and sp.num_nodes == n and sp.val_neg is None
    nv, nt = int(0.05 * e_rep), int(0.1 * e_rep)
    assert (sp.val_pos.size(1), sp.test_pos.size(1), sp.train_pos.size(1)) == (nv, nt, e_rep - nv - nt)
    parts = [_codes(p, n) for p in (sp.train_pos, sp.val_pos, sp.test_pos)]
    rep = _codes(ei[:, ei[0] < ei[1]], n)
    assert sum(len(p) for p in parts) == e_rep == len(rep) and set().union(*parts) == rep         # a partition of the representatives
    for p in (sp.train_pos, sp.val_pos, sp.test_pos):
        assert bool((p[0] < p[1]).all())
    train_graph = _codes(sp.train_edge_index, n)
    assert train_graph == parts[0] | _codes(sp.train_pos.flip(0), n) and sp.val_edge_index is sp.train_edge_index
    for p in (sp.val_pos, sp.test_pos):                                  # nothing a later split is scored on, nor its reverse
        assert not (_codes(p, n) | _codes(p.flip(0), n)) & train_graph
    assert _codes(sp.test_edge_index, n) == train_graph | parts[1] | _codes(sp.val_pos.flip(0), n)
    assert not (_codes(sp.test_pos, n) | _codes(sp.test_pos.flip(0), n)) & _codes(sp.test_edge_index, n)
    again = data.random_link_split(ei, n, 0.05, 0.1, generator=torch.Generator().manual_seed(9))
    other = data.random_link_split(ei, n, 0.05, 0.1, generator=torch.Generator().manual_seed(10))
    for k in ("train_pos", "val_pos", "test_pos", "train_edge_index", "test_edge_index"):
        assert torch.equal(getattr(sp, k), getattr(again, k)), k
    assert not torch.equal(sp.val_pos, other.val_pos)


def test_random_link_split_of_a_directed_graph():
    n = 30
    ei = torch.from_numpy(distinct_edges(n, 200, 2))
    sp = data.random_link_split(ei, n, 0.1, 0.2, is_undirected=False, generator=torch.Generator().manual_seed(1))
    assert (sp.val_pos.size(1), sp.test_pos.size(1), sp.train_pos.size(1)) == (20, 40, 140)
    parts = [_codes(p, n) for p in (sp.train_pos, sp.val_pos, sp.test_pos)]
    assert sum(len(p) for p in parts) == 200 and set().union(*parts) == _codes(ei, n)
    assert _codes(sp.train_edge_index, n) == parts[0] and _codes(sp.test_edge_index, n) == parts[0] | parts[1]
    assert sp.train_edge_index.size(1) == 140 and sp.test_edge_index.size(1) == 160
    with pytest.raises(ValueError, match="ratios"):
        data.random_link_split(ei, n, 0.6, 0.5)
    with pytest.raises(ValueError, match="int64"):
        data.random_link_split(ei.float(), n)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_come_before_any_launch():
    keys = torch.arange(5, dtype=torch.int64)
    z, pairs = torch.randn(6, 4), torch.randint(0, 6, (2, 9))
    s, y = torch.randn(9), torch.ones(9, dtype=torch.uint8)
    g = _cpu_graph(6, 9)
    with _NoLaunch():
        for bad in (0, 33, -1):
            with pytest.raises(ValueError, match="attempts"):
                ops.negative_sample(10, keys, 6, 0, attempts=bad)
        with pytest.raises(ValueError, match="below 2\\^32"):
            ops.negative_sample(1 << 28, keys, 6, 0, attempts=8)          # 2 * 2^28 * 8 = 2^32
        with pytest.raises(ValueError, match="below 2\\^32"):
            ops.negative_sample(1 << 31, keys, 6, 0, attempts=1)
        with pytest.raises(ValueError, match="num_nodes"):
            ops.negative_sample(10, keys, 1 << 31, 0)
        for bad in (1.5, "0", True, None):
            with pytest.raises(ValueError, match="seed"):
                ops.negative_sample(10, keys, 6, bad)
        with pytest.raises(TypeError, match="key vector"):
            ops.negative_sample(10, keys.int(), 6, 0)
        with pytest.raises(ValueError, match="at most 3"):
            ops.link_rank(s, y, ks=(1, 2, 3, 4))
        with pytest.raises(ValueError, match="at most 3"):
            ops.link_rank(s, y, ks=(0,))
        for fn in (ops.bce_with_logits, ops.link_rank):
            with pytest.raises(ValueError, match="entries for 9 scores"):
                fn(s, y[:8])
            with pytest.raises(ValueError, match="entries for 9 scores"):
                fn(s, y, torch.ones(10, dtype=torch.uint8))
            with pytest.raises(TypeError, match="uint8"):
                fn(s, y.long())
            with pytest.raises(TypeError, match="fp32"):
                fn(s.double(), y)
        with pytest.raises(ValueError, match="accumulate"):
            ops.bce_with_logits(s, y, accumulate=torch.zeros(4, dtype=torch.int64))
        with pytest.raises(ValueError, match="int64"):
            ops.pair_scores(z, pairs.int())
        with pytest.raises(ValueError, match="int64"):
            ops.edge_keys(pairs.float(), 6)
        # everything in order: refused like every other op on the CPU, still without a call
        for call in (lambda: ops.negative_sample(10, keys, 6, -3), lambda: ops.negative_sample(10, g, 6, 0),
                     lambda: ops.edge_keys(pairs, 6), lambda: ops.pair_scores(z, pairs), lambda: ops.pair_scores(z, g),
                     lambda: ops.bce_with_logits(s, y), lambda: ops.bce_with_logits(s, y, y), lambda: ops.link_rank(s, y),
                     lambda: ops.link_rank(s, y, y, ks=(5,))):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()
        model = kagnn_amd.LinkPredictor(kagnn_amd.GKAN_Nodes("gcn", 2, 4, 8, 8))
        split = data.random_link_split(_undirected(6, 9, 1), 6, generator=torch.Generator().manual_seed(0))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            harness.train_link_prediction(model, torch.randn(6, 4), split, epochs=1)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            split.with_negatives(0)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model(torch.randn(6, 4), split.train_edge_index, split.train_pos)


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_the_seven_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    assert lib.kagnn_version() >= 278
    header = open(os.path.join(ROOT, "include", "kagnn_hip.h")).read()
    assert re.search(r"#define\s+KAGNN_NEGATIVE_MAX_ATTEMPTS\s+32\b", header) and _lib.NEGATIVE_MAX_ATTEMPTS == 32
    assert re.search(r"#define\s+KAGNN_BCE_WORKSPACE_BYTES\s+6144\b", header) and _lib.BCE_WORKSPACE_BYTES == 6144
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, nargs in NAMES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name) and name in _lib.EXPORTED and len(_lib._SIGNATURES[name][1]) == nargs, name
    for name in ("edge_keys", "negative_sample", "pair_scores", "pair_index", "bce_with_logits", "link_rank", "link_rank_figures"):
        assert callable(getattr(ops, name)), name
    assert kagnn_amd.random_link_split is data.random_link_split and kagnn_amd.LinkSplit is data.LinkSplit
    assert callable(harness.train_link_prediction) and isinstance(kagnn_amd.LinkPredictor(torch.nn.Identity()), torch.nn.Module)
    from kagnn_amd import _build
    assert "linkpred.hip" in _build.SOURCES


def test_argument_checks_need_no_gpu():
    lib = _lib.load()
    out = ctypes.c_size_t(0)
    sizes = []
    for p in (0, 1, 4099, 70001, 1 << 20):
        assert lib.kagnn_link_rank_workspace_bytes(p, ctypes.byref(out)) == 0
        assert out.value >= 2 * 4 * p + 2 * (p + 1) + 4 * (p + 1)        # two key arrays, two label arrays, the scan
        sizes.append(out.value)
        assert lib.kagnn_edge_keys_workspace_bytes(p, ctypes.byref(out)) == 0 and out.value >= 16 * p
    assert sizes == sorted(sizes)
    assert lib.kagnn_link_rank_workspace_bytes(-1, ctypes.byref(out)) != 0 and lib.kagnn_link_rank_workspace_bytes(5, None) != 0
    assert lib.kagnn_edge_keys_workspace_bytes(1 << 31, ctypes.byref(out)) != 0
    neg = lib.kagnn_negative_sample
    for attempts in (0, 33, -4):
        assert neg(None, 0, 10, 5, 0, attempts, None, None, None) != 0 and b"attempts must be 1..32" in lib.kagnn_last_error()
    assert neg(None, 0, 10, 1 << 28, 0, 8, None, None, None) != 0 and b"below 2^32" in lib.kagnn_last_error()
    assert neg(None, 0, 1 << 31, 5, 0, 8, None, None, None) != 0 and b"num_nodes" in lib.kagnn_last_error()
    assert neg(None, 0, 10, 5, 0, 8, None, None, None) != 0 and b"null array" in lib.kagnn_last_error()
    assert neg(None, 0, 0, 5, 0, 8, None, None, None) == 0 and neg(None, 0, 10, 0, 0, 8, None, None, None) == 0      # nothing to launch
    ks = (ctypes.c_int32 * 4)(20, 50, 100, 200)
    rank = lib.kagnn_link_rank
    assert rank(None, None, None, 5, ks, 4, None, None, 0, None) != 0 and b"at most 3" in lib.kagnn_last_error()
    assert rank(None, None, None, 5, (ctypes.c_int32 * 1)(0), 1, None, None, 0, None) != 0 and b"a k below 1" in lib.kagnn_last_error()
    assert rank(None, None, None, 5, ks, 3, None, None, 0, None) != 0 and b"null array" in lib.kagnn_last_error()
    assert lib.kagnn_bce_logits_fwd(None, None, None, 5, None, None, None, None, 0, None) != 0 and b"kagnn_bce_logits_fwd" in lib.kagnn_last_error()
    assert lib.kagnn_bce_logits_bwd(None, None, None, 5, None, None, None, None) != 0
    assert lib.kagnn_edge_keys_build(None, None, 5, 0, None, None, None, 0, None) != 0 and b"edges without nodes" in lib.kagnn_last_error()
