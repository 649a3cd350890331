"""Neighbour sampling, host side (no GPU): the three entry points' place in the C ABI and their argument checks, what
``ops.sample_neighbors`` refuses before anything is launched, the arithmetic of ``kagnn_amd.NeighborLoader`` (per-batch sampling seed,
epoch order), and the CPU restatement of the sampler that tests/test_gpu_neighbor_sampling.py holds the kernels to -- ``key32`` and
"the k smallest pairs (key32, e) of a row" of include/kagnn_hip.h, restated in numpy's uint32 arithmetic.

The restatement itself is held to what a uniform k-subset without replacement does (``test_the_key_function_draws_uniform_...``):
four rows -- edge ids 100..119 and 0..19 at k = 5, ids 200..269 at k = 10 (seeds 0..3999), ids 0..1612 at k = 64 (seeds 0..1999).
Bounds, in binomial standard deviations of a frequency over T seeds, sqrt(p (1 - p) / T): every edge's inclusion frequency within
5 of k / deg (5.5 for the 1613-edge row: the maximum of 1613 deviates), every pair's joint frequency within 5 of
k (k - 1) / (deg (deg - 1)) (the three short rows), the mean overlap of consecutive seeds' selections within 5 % of k^2 / deg.
Measured for the function as it stands (the test prints them): marginal 1.5 / 1.8 / 2.6 / 3.7 deviations, pairwise 3.4 / 2.4 / 4.2,
overlaps 1.253 / 1.227 / 1.413 / 2.494 against 1.250 / 1.250 / 1.429 / 2.539.  Re-check them when the function changes."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import kagnn_amd
from kagnn_amd import _lib, data, harness, ops
from test_subgraph_host import _NoLaunch, _cpu_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"kagnn_neighbor_sample_mark": 14, "kagnn_edge_subgraph_count": 14, "kagnn_edge_subgraph_fill": 23}
GOLDEN = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------------------------- the restatement
def mix32(x):
    """``mix32`` of csrc/common.h on a numpy uint32 array (arithmetic mod 2^32)"""
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def key32(seed, e):
    """the sampling key of original edge id ``e`` (array) under the 64-bit ``seed``: include/kagnn_hip.h"""
    seed = int(seed) & M64
    lo, hi = np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32)
    with np.errstate(over="ignore"):
        h1 = mix32(np.array([lo], dtype=np.uint32) + np.uint32(0x9E3779B9))
        h2 = mix32(np.array([hi], dtype=np.uint32) ^ h1 ^ np.uint32(0x85EBCA6B))
        return mix32(mix32(np.asarray(e, dtype=np.int64).astype(np.uint32) ^ h1) + h2)


def k_smallest(seed, edge_ids, k):
    """the edge ids a row holding ``edge_ids`` keeps at fan-out ``k`` (-1: all): the ``k`` smallest pairs ``(key32, e)``, ascending in e"""
    e = np.asarray(edge_ids, dtype=np.int64)
    if k < 0 or k >= e.size:
        return np.sort(e)
    order = np.lexsort((e, key32(seed, e)))              # (last key is the primary one)
    return np.sort(e[order[:k]])


def sample_reference(edge_index, num_nodes, seeds, fanouts, seed):
    """the sampler restated on the CPU: a level BFS along the in-edges in which every node expands once, at the level it is first
    reached, and keeps ``k_smallest`` of its in-edges.  Returns ``(hop int32 [N], keep bool [E])`` as torch tensors"""
    src, dst = edge_index[0].numpy(), edge_index[1].numpy()
    order = np.argsort(dst, kind="stable")
    starts = np.searchsorted(dst[order], np.arange(num_nodes + 1))
    hop = np.full(num_nodes, -1, dtype=np.int32)
    keep = np.zeros(src.size, dtype=bool)
    hop[np.asarray(seeds, dtype=np.int64)] = 0
    for d, k in enumerate(fanouts):
        reached = []
        for i in np.nonzero(hop == d)[0]:
            row = order[starts[i]:starts[i + 1]]
            if k == 0 or row.size == 0:
                continue
            took = k_smallest(seed, row, k)
            keep[took] = True
            reached.append(src[took])
        if reached:
            new = np.concatenate(reached)
            new = new[hop[new] < 0]
            hop[new] = d + 1
    return torch.from_numpy(hop), torch.from_numpy(keep)


def test_key32_in_plain_python_integers():
    """the numpy form against the formula written out with Python ints, and two values pinned for good"""
    def m(x):
        x &= 0xFFFFFFFF
        x ^= x >> 16
        x = x * 0x7FEB352D & 0xFFFFFFFF
        x ^= x >> 15
        x = x * 0x846CA68B & 0xFFFFFFFF
        return x ^ x >> 16

    def key(seed, e):
        lo, hi = seed & 0xFFFFFFFF, seed >> 32 & 0xFFFFFFFF
        h1 = m(lo + 0x9E3779B9)
        h2 = m(hi ^ h1 ^ 0x85EBCA6B)
        return m(m(e & 0xFFFFFFFF ^ h1) + h2)
    es = [0, 1, 2, 63, 64, 1612, 123456789, 2**31 - 2]
    for seed in (0, 1, 2**32, 2**32 + 1, GOLDEN, M64):
        assert key32(seed, es).tolist() == [key(seed, e) for e in es], seed
    assert [hex(int(v)) for v in key32(0, [0, 1])] == ['0x333a3c44', '0x68ccc634'] and hex(int(key32(GOLDEN, [1612])[0])) == '0xd6d05646'
    assert key32(0, [0])[0] != key32(1, [0])[0] and key32(0, [0])[0] != key32(2**32, [0])[0]
    # what f(e ^ seed) would do and this form must not: seed s at edge e and seed s ^ 1 at edge e ^ 1 share no key
    a, b = key32(6, np.arange(64)), key32(7, np.arange(64) ^ 1)
    assert int((a == b).sum()) == 0


def test_k_smallest_breaks_ties_by_edge_id_and_takes_whole_rows():
    ids = np.array([9, 4, 7, 1])
    assert k_smallest(3, ids, -1).tolist() == [1, 4, 7, 9] and k_smallest(3, ids, 4).tolist() == [1, 4, 7, 9]
    assert k_smallest(3, ids, 9).tolist() == [1, 4, 7, 9] and k_smallest(3, ids, 0).tolist() == []
    keys = key32(3, ids)
    assert k_smallest(3, ids, 1).tolist() == [int(ids[np.argmin(keys)])]
    for k in (1, 2, 3):
        got = k_smallest(3, ids, k)
        assert got.size == k and set(got.tolist()) == set(ids[np.argsort(keys)[:k]].tolist())


ROWS = [(np.arange(100, 120), 5, 4000, 5.0, True), (np.arange(0, 20), 5, 4000, 5.0, True), (np.arange(200, 270), 10, 4000, 5.0, True),
        (np.arange(0, 1613), 64, 2000, 5.5, False)]


@pytest.mark.parametrize("row", range(len(ROWS)), ids=["20 edges at 100", "20 edges at 0", "70 edges", "1613 edges"])
def test_the_key_function_draws_uniform_pairwise_uniform_subsets_independent_between_consecutive_seeds(row):
    ids, k, T, bound, pairs = ROWS[row]
    deg = ids.size
    M = np.zeros((T, deg), dtype=np.float32)
    for s in range(T):
        M[s, np.searchsorted(ids, k_smallest(s, ids, k))] = 1.0
    assert bool((M.sum(1) == k).all())
    p = k / deg
    worst = float(np.abs(M.mean(0) - p).max() / np.sqrt(p * (1 - p) / T))
    print(f"row {row}: marginal {worst:.2f} deviations (bound {bound})")
    assert worst <= bound
    if pairs:
        p2 = k * (k - 1) / (deg * (deg - 1))
        joint = (M.T @ M) / T
        off = ~np.eye(deg, dtype=bool)
        worst2 = float(np.abs(joint[off] - p2).max() / np.sqrt(p2 * (1 - p2) / T))
        print(f"row {row}: pairwise {worst2:.2f} deviations (bound 5)")
        assert worst2 <= 5.0
    overlap = float((M[1:] * M[:-1]).sum(1).mean())
    print(f"row {row}: overlap of consecutive seeds {overlap:.3f} against {k * k / deg:.3f}")
    assert abs(overlap - k * k / deg) <= 0.05 * k * k / deg


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_the_three_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    assert lib.kagnn_version() >= 277
    header = open(os.path.join(ROOT, "include", "kagnn_hip.h")).read()
    assert re.search(r"#define\s+KAGNN_SAMPLE_MAX_LEVELS\s+16\b", header) and _lib.SAMPLE_MAX_LEVELS == 16
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, nargs in NAMES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name) and name in _lib.EXPORTED and len(_lib._SIGNATURES[name][1]) == nargs, name
    assert callable(ops.sample_neighbors) and kagnn_amd.NeighborLoader is data.NeighborLoader and kagnn_amd.NodeBatch is data.NodeBatch
    assert callable(harness.train_node_classification_sampled)


def test_argument_checks_need_no_gpu():
    lib = _lib.load()
    mark, count, fill = lib.kagnn_neighbor_sample_mark, lib.kagnn_edge_subgraph_count, lib.kagnn_edge_subgraph_fill
    fan = (ctypes.c_int32 * 17)(*([3] * 17))
    assert mark(None, None, None, -1, 0, None, 0, fan, 1, 0, None, None, None, None) != 0
    assert mark(None, None, None, 0, 5, None, 0, fan, 1, 0, None, None, None, None) != 0 and b"edges without nodes" in lib.kagnn_last_error()
    for levels in (0, 17, -1):
        assert mark(None, None, None, 10, 5, None, 0, fan, levels, 0, None, None, None, None) != 0
        assert b"num_levels" in lib.kagnn_last_error()
    assert mark(None, None, None, 10, 5, None, 0, None, 1, 0, None, None, None, None) != 0 and b"num_levels" in lib.kagnn_last_error()
    bad = (ctypes.c_int32 * 2)(3, -2)
    assert mark(None, None, None, 10, 5, None, 0, bad, 2, 0, None, None, None, None) != 0 and b"fanout" in lib.kagnn_last_error()
    assert mark(None, None, None, 10, 5, None, 0, fan, 2, 0, None, None, None, None) != 0 and b"null array" in lib.kagnn_last_error()
    assert count(None, None, None, None, None, None, None, None, -1, 0, None, 0, None, None) != 0
    assert count(None, None, None, None, None, None, None, None, 0, 5, None, 0, None, None) != 0 and b"edges without nodes" in lib.kagnn_last_error()
    assert count(None, None, None, None, None, None, None, None, 10, 5, None, 0, None, None) != 0 and b"null array" in lib.kagnn_last_error()
    assert b"kagnn_edge_subgraph_count" in lib.kagnn_last_error()
    nulls = [None] * 9
    assert fill(None, 0, None, None, None, None, None, None, None, -1, 0, 0, 0, *nulls, None) != 0
    assert fill(None, 0, None, None, None, None, None, None, None, 10, 5, 11, 0, *nulls, None) != 0 and b"n_sub" in lib.kagnn_last_error()
    assert fill(None, 0, None, None, None, None, None, None, None, 10, 5, 3, 6, *nulls, None) != 0 and b"n_sub" in lib.kagnn_last_error()
    assert fill(None, 0, None, None, None, None, None, None, None, 10, 5, 3, 2, *nulls, None) != 0 and b"null array" in lib.kagnn_last_error()
    assert b"kagnn_edge_subgraph_fill" in lib.kagnn_last_error()


def test_refusals_come_before_any_launch():
    g = _cpu_graph(5, 7)
    one = torch.tensor([1])
    with _NoLaunch():
        for bad in ([], [1] * 17, None, 3, torch.ones(2, 2, dtype=torch.int64)):
            with pytest.raises(ValueError, match="1 to 16"):
                ops.sample_neighbors(one, bad, g)
        for bad in ([-2], [3, -5], [1.5], [2, "3"], [True], [None], [1 << 31]):
            with pytest.raises(ValueError, match="fan-out"):
                ops.sample_neighbors(one, bad, g)
        for bad in (1.5, "0", True, None):
            with pytest.raises(ValueError, match="seed"):
                ops.sample_neighbors(one, [2], g, seed=bad)
        with pytest.raises(ValueError, match="mask"):
            ops.sample_neighbors(torch.ones(5, dtype=torch.bool), [2], g)
        for ids in (torch.tensor([1.0]), torch.tensor([1], dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int64)):
            with pytest.raises(ValueError, match="int64"):
                ops.sample_neighbors(ids, [2], g)
        with pytest.raises(TypeError, match="GraphIndex"):
            ops.sample_neighbors([1], [2], torch.zeros(2, 3, dtype=torch.int64))
        # everything in order: refused like every other op on the CPU, still without a call
        for fan in ([2], [-1, 0, 5], (3, 3), torch.tensor([4, 4]), [2.0]):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                ops.sample_neighbors(one, fan, g, seed=-7)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.sample_neighbors([], [2], g)


# ---------------------------------------------------------------------------------------------------------------- the loader
def test_the_loader_refuses_bad_arguments_before_any_launch():
    g = _cpu_graph(5, 7)
    with _NoLaunch():
        with pytest.raises(ValueError, match="batch_size"):
            kagnn_amd.NeighborLoader(g, torch.arange(5), [2], 0)
        with pytest.raises(ValueError, match="1 to 16"):
            kagnn_amd.NeighborLoader(g, torch.arange(5), [], 2)
        with pytest.raises(ValueError, match="fan-out"):
            kagnn_amd.NeighborLoader(g, torch.arange(5), [-3], 2)
        with pytest.raises(ValueError, match="seed"):
            kagnn_amd.NeighborLoader(g, torch.arange(5), [2], 2, seed=0.5)
        with pytest.raises(TypeError, match="GraphIndex"):
            kagnn_amd.NeighborLoader(torch.zeros(2, 3, dtype=torch.int64), torch.arange(5), [2], 2)
        with pytest.raises(ValueError, match=r"shape \[5\]"):
            kagnn_amd.NeighborLoader(g, torch.ones(4, dtype=torch.bool), [2], 2)
        with pytest.raises(ValueError, match="int64"):
            kagnn_amd.NeighborLoader(g, torch.tensor([0.5]), [2], 2)
        with pytest.raises(ValueError, match="x must have"):
            kagnn_amd.NeighborLoader(g, torch.arange(5), [2], 2, x=torch.zeros(4, 3))
        with pytest.raises(ValueError, match="y must have"):
            kagnn_amd.NeighborLoader(g, torch.arange(5), [2], 2, y=torch.zeros(6))


def test_the_per_batch_seed_formula_and_the_epoch_order():
    g = _cpu_graph(50, 7)
    ids = torch.arange(3, 40)                             # 37 input nodes
    mask = torch.zeros(50, dtype=torch.bool)
    mask[ids] = True
    for given in (ids, mask):
        for drop_last, nb in ((False, 4), (True, 3)):
            loader = kagnn_amd.NeighborLoader(g, given, [3, 2], 10, drop_last=drop_last, seed=12345)
            assert len(loader) == nb and loader.fanouts == [3, 2] and torch.equal(loader.input_nodes, ids)
            seen = set()
            for t in range(3):
                for b in range(nb):
                    s = loader.sampling_seed(t, b)
                    assert s == (12345 + GOLDEN * (1 + t * nb + b)) % (1 << 64) and s not in seen
                    seen.add(s)
    assert kagnn_amd.NeighborLoader(g, ids, [1], 10, seed=-1).sampling_seed(0, 0) == (GOLDEN - 1) % (1 << 64)
    assert kagnn_amd.NeighborLoader(g, ids, [1], 10, seed=M64).sampling_seed(2, 3) == (M64 + GOLDEN * 12) % (1 << 64)
    # the order of an epoch is epoch_order's, epoch after epoch, and the epoch counter advances with every order drawn
    a = kagnn_amd.NeighborLoader(g, ids, [1], 10, shuffle=True, generator=torch.Generator().manual_seed(5))
    gen = torch.Generator().manual_seed(5)
    for t in range(3):
        assert a.epoch == t
        assert torch.equal(a.order(), ids[data.epoch_order(37, True, gen)])
    assert a.epoch == 3
    b = kagnn_amd.NeighborLoader(g, ids, [1], 10)
    assert torch.equal(b.order(), ids) and torch.equal(b.order(), ids) and b.epoch == 2
    # on the CPU the first batch is refused like every other op
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        next(iter(b))


def test_the_sampled_training_loop_refuses_cpu_tensors_before_any_launch():
    model = kagnn_amd.GKAN_Nodes("gin", 2, 4, 8, 3)
    x, ei, y = torch.randn(6, 4), torch.randint(0, 6, (2, 9)), torch.randint(0, 3, (6,))
    m = torch.ones(6, dtype=torch.bool)
    with _NoLaunch():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            harness.train_node_classification_sampled(model, x, ei, y, m, m, fanouts=[2, 2], epochs=1)
        with pytest.raises(ValueError, match="fanouts"):
            harness.train_node_classification_sampled(model, x, ei, y, m, m, epochs=1)
