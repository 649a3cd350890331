"""Neighbour sampling on the device (``ops.sample_neighbors``: csrc/subgraph.hip), its loader (``kagnn_amd.NeighborLoader``) and the
sampled training loop (``harness.train_node_classification_sampled``).

Everything the sampler returns is an integer and is compared bit for bit.  The reference is ``sample_reference`` of
tests/test_neighbor_sampling_host.py -- a level BFS on the CPU that takes, per expanded row, the k smallest ``(key32, e)`` -- so the
kernels' three row paths (whole row, one key per lane, radix select) are held to one statement; rows of 63 / 64 / 65 entries and
the 1613-edge hub of graph (b) sit on both sides of every threshold between them.  The six index arrays are held to
``GraphIndex(sub.edge_index, sub.num_nodes)`` on both build paths.  Models: with every fan-out -1 and ``receptive_hops(model)`` levels the
logits at the seeds are the full graph's (fp64 oracle of tests/test_gpu_subgraph.py, 1e-4 of the tensor's maximum, eval mode).  The
training loop is compared, bit for bit, with the same loop written out here from the public pieces."""
import ctypes

import pytest
import torch

import kagnn_amd
from kagnn_amd import _lib, harness, ops
from helpers import assert_close, must_fail
from test_gpu_poison import _guard_case, _heap_case
from test_gpu_subgraph import DEV, MF, MODEL_TOL, _arrays, _bfs, _fields, _gen, _logits64, _model, _parent, _undirected_path
from test_neighbor_sampling_host import GOLDEN, sample_reference

pytestmark = pytest.mark.gpu
SEED = 0x0123456789ABCDEF                              # (both words of the seed in use)
FANOUTS = ([5], [3, 2], [0, 4], [-1, 1], [2, 2, 2])
SMALL = ["a", "b hub", "c source hub", "d path"]
SEED_SETS = {"a": ([11], [3, 11, 42, 250, 11, 0, 299], [7]), "b hub": ([3], [3, 11, 42, 250, 11, 0, 299], [7]),
             "c source hub": ([3], [3, 11, 42, 250, 11, 0, 299], [7]), "d path": ([9], [9, 0, 5, 3, 9, 1, 8], [7])}


def _expected(hop, keep, ei, n):
    nodes = (hop >= 0).nonzero().flatten()
    rel = torch.full((n,), -1, dtype=torch.int64)
    rel[nodes] = torch.arange(nodes.numel())
    return nodes, rel[ei[:, keep]], keep.nonzero().flatten(), rel


def _check(sub, ei, n, seeds, fanouts, seed, what):
    """``sub`` against the CPU restatement: nodes, hops, edge_ids, edge_index, mapping; the shape of the index"""
    hop, keep = sample_reference(ei, n, seeds, fanouts, seed)
    nodes, sei, eids, rel = _expected(hop, keep, ei, n)
    assert (sub.num_nodes, sub.num_edges) == (nodes.numel(), eids.numel()), what
    assert sub.nodes.dtype == sub.edge_ids.dtype == sub.edge_index.dtype == sub.mapping.dtype == torch.int64 and sub.hops.dtype == torch.int32
    assert torch.equal(sub.nodes.cpu(), nodes), what
    assert torch.equal(sub.hops.cpu(), hop[nodes]), what
    assert torch.equal(sub.edge_ids.cpu(), eids), what
    assert sub.edge_index.shape == (2, eids.numel()) and torch.equal(sub.edge_index.cpu(), sei), what
    assert torch.equal(sub.mapping.cpu(), rel[torch.as_tensor(seeds, dtype=torch.int64)]), what
    idx = sub.index
    assert (idx.num_nodes, idx.num_edges, idx.num_hub_seg, idx.num_hub_seg_t) == (sub.num_nodes, sub.num_edges, 0, 0)
    assert [t.numel() for t in _arrays(idx)] == [sub.num_nodes + 1, sub.num_edges, sub.num_edges] * 2
    assert all(t.dtype == torch.int32 for t in _arrays(idx))
    return hop, keep


def _same_index_as_a_build(sub, monkeypatch, what):
    for small in (True, False):
        monkeypatch.setattr(ops, "_SMALL_CSR", small)
        want = ops.GraphIndex(sub.edge_index.contiguous(), sub.num_nodes)
        for k, (a, b) in enumerate(zip(_arrays(sub.index), _arrays(want))):
            assert torch.equal(a, b), f"{what}: index array {k} differs from a build (small path {small})"
    monkeypatch.undo()


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", SMALL)
def test_sample_neighbors_equals_the_cpu_restatement(name):
    ei, _, n, g = _parent(name)
    case = 0
    for seeds in SEED_SETS[name]:
        for fan in FANOUTS:
            case += 1
            seed = (SEED + case * GOLDEN) % (1 << 64)
            sub = ops.sample_neighbors(torch.tensor(seeds, device=DEV), fan, g, seed=seed)
            _check(sub, ei, n, seeds, fan, seed, f"{name}: seeds {seeds}, fanouts {fan}")


def test_the_hub_row_at_every_fan_out_around_the_wave_and_the_row_length():
    """the 1613-edge row of node 7 (26 chunks) takes the radix path for k < deg, the whole-row path from k = deg on"""
    ei, _, n, g = _parent("b hub")
    deg = int(g.rowptr[8] - g.rowptr[7])
    assert deg >= 1613
    sizes = {}
    for k in sorted({1, 63, 64, 65, 1000, 1612, 1613, 2000, deg - 1, deg, deg + 1}):
        sub = ops.sample_neighbors([7], [k], g, seed=SEED + k)
        _, keep = _check(sub, ei, n, [7], [k], SEED + k, f"hub row, k = {k}")
        sizes[k] = sub.num_edges
        assert sub.num_edges == min(k, deg) and bool((ei[1, keep] == 7).all())
    assert sizes[1] == 1 and sizes[2000] == deg


def _rows_graph():
    """200 nodes; the in-degrees of nodes 0 .. 5 are exactly 64, 65, 63, 6, 1 and 128, their edges scattered among 500 others that
    end at nodes 10 .. 199"""
    gen = _gen(11)
    degs = [64, 65, 63, 6, 1, 128]
    dst = torch.cat([torch.full((d,), i) for i, d in enumerate(degs)] + [torch.randint(10, 200, (500,), generator=gen)])
    src = torch.randint(0, 200, (dst.numel(),), generator=gen)
    both = torch.stack([src, dst])
    return both[:, torch.randperm(dst.numel(), generator=gen)].contiguous(), 200, degs


def test_rows_of_exactly_64_and_65_entries_and_fan_outs_at_and_next_to_the_degree():
    ei, n, degs = _rows_graph()
    g = ops.GraphIndex(ei.to(DEV), n)
    assert (g.rowptr[1:7] - g.rowptr[:6]).tolist() == degs
    for node, deg in enumerate(degs):
        for k in sorted({1, 5, 6, 62, 63, 64, 65, 127, deg - 1, deg, deg + 1} - {0}):
            sub = ops.sample_neighbors([node], [k], g, seed=SEED ^ k)
            _check(sub, ei, n, [node], [k], SEED ^ k, f"a row of {deg} entries, k = {k}")
            assert sub.num_edges == min(k, deg)
    # all six rows in one wave, two levels
    sub = ops.sample_neighbors([0, 1, 2, 3, 4, 5], [63, 2], g, seed=5)
    _check(sub, ei, n, [0, 1, 2, 3, 4, 5], [63, 2], 5, "six rows, two levels")


def test_one_node_no_edges_and_empty_seeds():
    for name, seeds in (("f one node", [0]), ("f no edges", [4, 0, 2]), ("f isolated seed", [0, 4, 0])):
        ei, _, n, g = _parent(name)
        for fan in ([3], [-1, 2]):
            _check(ops.sample_neighbors(seeds, fan, g, seed=1), ei, n, seeds, fan, 1, name)
    g = _parent("a")[3]
    for empty in ([], torch.empty(0, dtype=torch.int64, device=DEV)):
        sub = ops.sample_neighbors(empty, [3, 3], g)
        assert (sub.num_nodes, sub.num_edges) == (0, 0) and sub.nodes.numel() == 0 and sub.edge_index.shape == (2, 0)
        assert sub.mapping.numel() == 0 and sub.hops.numel() == 0 and sub.index.rowptr.tolist() == [0] and sub.index.rowptr_t.tolist() == [0]
    a, b, c = ops.sample_neighbors(11, [3, 3], g), ops.sample_neighbors([11], [3, 3], g), ops.sample_neighbors(torch.tensor(11, device=DEV), (3, 3), g)
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(_fields(a), _fields(b), _fields(c)))


# ---------------------------------------------------------------------------------------------------------------- invariants
@pytest.mark.parametrize("name", ["b hub", "c source hub", "e large"])
def test_every_expanded_row_keeps_its_fan_out_and_every_kept_edge_is_inside(name):
    ei, ei_dev, n, g = _parent(name)
    fan = [3, 70, 2]
    seeds = torch.tensor([3, 7, 42, 7], device=DEV)
    sub = ops.sample_neighbors(seeds, fan, g, seed=SEED)
    hop = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    hop[sub.nodes] = sub.hops.long()
    keep = torch.zeros(ei.size(1), dtype=torch.bool, device=DEV)
    keep[sub.edge_ids] = True
    src, dst = ei_dev
    deg = torch.bincount(dst, minlength=n)
    kept_in = torch.bincount(dst[keep], minlength=n)
    want = torch.zeros(n, dtype=torch.int64, device=DEV)
    for d, k in enumerate(fan):
        want = torch.where(hop == d, torch.clamp(deg, max=k), want)
    assert torch.equal(kept_in, want)
    assert bool((hop[src[keep]] >= 0).all()) and bool((hop[dst[keep]] >= 0).all())
    is_source = torch.zeros(n, dtype=torch.bool, device=DEV)
    is_source[src[keep]] = True
    assert bool(is_source[hop > 0].all()) and set(sub.nodes[sub.hops == 0].tolist()) == {3, 7, 42}
    # a source sits at most one level beyond the row that took it
    assert bool((hop[src[keep]] <= hop[dst[keep]] + 1).all())
    assert torch.equal(sub.edge_index, torch.stack([torch.searchsorted(sub.nodes, src[sub.edge_ids]), torch.searchsorted(sub.nodes, dst[sub.edge_ids])]))


@pytest.mark.parametrize("name", ["a", "b hub", "c source hub", "d path"])
def test_all_neighbours_at_every_level_is_the_k_hop_subgraph_less_its_outermost_rows(name):
    ei, ei_dev, n, g = _parent(name)
    for levels in (1, 2, 3):
        for seeds in SEED_SETS[name][:2]:
            sub = ops.sample_neighbors(seeds, [-1] * levels, g, seed=levels)
            full = ops.k_hop_subgraph(seeds, levels, g)
            assert torch.equal(sub.nodes, full.nodes) and torch.equal(sub.hops, full.hops) and torch.equal(sub.mapping, full.mapping)
            inner = full.hops[full.edge_index[1]] < levels
            assert torch.equal(sub.edge_ids, full.edge_ids[inner]) and torch.equal(sub.edge_index, full.edge_index[:, inner])
            assert torch.equal(sub.hops.cpu(), _bfs(torch.tensor(seeds), levels, ei, n)[sub.nodes.cpu()])


@pytest.mark.parametrize("name", ["b hub", "c source hub"])
def test_the_index_holds_the_bits_of_a_build_on_both_paths(name, monkeypatch):
    g = _parent(name)[3]
    for seeds, fan in (([3, 11, 42], [5]), ([3, 11, 42], [-1, 1]), ([7, 3], [2, 2, 2]), ([7], [1000]), ([7, 250], [64, 3]), ([7], [-1, -1])):
        sub = ops.sample_neighbors(seeds, fan, g, seed=SEED)
        assert sub.num_edges > 0
        _same_index_as_a_build(sub, monkeypatch, f"{name}: seeds {seeds}, fanouts {fan}")


# ---------------------------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("name", ["b hub", "c source hub", "e large"])
def test_a_second_call_returns_the_same_bits(name):
    g = _parent(name)[3]
    first = _fields(ops.sample_neighbors([3, 7, 42], [100, 5, 5], g, seed=SEED))
    junk = torch.full((1 << 20,), -7, dtype=torch.int32, device=DEV)      # (the allocator hands the next call other memory)
    second = _fields(ops.sample_neighbors([3, 7, 42], [100, 5, 5], g, seed=SEED))
    del junk
    assert len(first) == len(second) == 11 and all(torch.equal(a, b) for a, b in zip(first, second))


def test_the_result_depends_on_the_seed_set_and_the_sampling_seed_only():
    ei, _, n, g = _parent("b hub")
    seeds = [3, 11, 42, 250, 7, 0, 299]
    base = ops.sample_neighbors(seeds, [40, 3], g, seed=SEED)
    gen = _gen(3)
    for _ in range(3):
        order = torch.randperm(len(seeds), generator=gen)
        again = torch.tensor(seeds)[torch.cat([order, order[:3]])]
        sub = ops.sample_neighbors(again.to(DEV), [40, 3], g, seed=SEED)
        assert all(torch.equal(getattr(sub, f), getattr(base, f)) for f in ("nodes", "edge_index", "edge_ids", "hops"))
        assert all(torch.equal(a, b) for a, b in zip(_arrays(sub.index), _arrays(base.index)))
        assert torch.equal(sub.nodes[sub.mapping].cpu(), again)
    # another sampling seed, another selection from the hub's row -- in either word of the seed
    hub = ops.sample_neighbors([7], [64], g, seed=SEED)
    for other in (SEED + 1, SEED ^ (1 << 32), SEED ^ (1 << 63)):
        moved = ops.sample_neighbors([7], [64], g, seed=other)
        assert moved.num_edges == 64 and not torch.equal(moved.edge_ids, hub.edge_ids)
        assert len(set(moved.edge_ids.tolist()) & set(hub.edge_ids.tolist())) < 24        # (expected overlap 64^2 / 1613 = 2.5)
    # a seed is taken mod 2^64
    assert torch.equal(ops.sample_neighbors([7], [64], g, seed=SEED - (1 << 64)).edge_ids, hub.edge_ids)


def test_edges_are_selected_by_their_id_not_by_their_place_in_the_row():
    """a permuted edge list: the edges of every destination trade their sources among themselves, so every row holds the ids it
    held and its entries stand where they stood -- with other sources.  The rows select the same ids; what they reach follows the
    permutation.  And a relabelling of the NODES (rows move to other lanes and waves) selects the same edge ids outright"""
    ei, _, n, g = _parent("b hub")
    gen = _gen(4)
    src = ei[0].clone()
    for i in (7, 3, 42):
        ids = (ei[1] == i).nonzero().flatten()
        src[ids] = ei[0][ids[torch.randperm(ids.numel(), generator=gen)]]
    traded = torch.stack([src, ei[1]]).contiguous()
    g2 = ops.GraphIndex(traded.to(DEV), n)
    for k in (5, 64, 200):
        a, b = ops.sample_neighbors([7, 3, 42], [k], g, seed=SEED), ops.sample_neighbors([7, 3, 42], [k], g2, seed=SEED)
        assert torch.equal(a.edge_ids, b.edge_ids)
        assert torch.equal(b.nodes.cpu(), torch.unique(torch.cat([torch.tensor([7, 3, 42]), traded[0][b.edge_ids.cpu()]])))
    relabel = torch.randperm(n, generator=gen)
    g3 = ops.GraphIndex(relabel[ei].contiguous().to(DEV), n)
    for fan in ([5], [64, 2], [3, 3, 3]):
        a = ops.sample_neighbors([7, 3, 42], fan, g, seed=SEED)
        b = ops.sample_neighbors(relabel[torch.tensor([7, 3, 42])].to(DEV), fan, g3, seed=SEED)
        assert torch.equal(a.edge_ids, b.edge_ids) and torch.equal(torch.sort(relabel[a.nodes.cpu()]).values, b.nodes.cpu())


# ---------------------------------------------------------------------------------------------------------------- bounds
SENTINEL = -1234567
_ptr = ops._ptr


def test_an_out_of_range_seed_raises_and_the_mark_call_stays_inside_its_buffers():
    ei, _, n, g = _parent("b hub")
    e = g.num_edges
    for bad in ([3, n], [-1, 3], [3, 1 << 40], [n]):
        with pytest.raises(ValueError, match="outside"):
            ops.sample_neighbors(bad, [3, 3], g)
    pad = 64
    hop = torch.full((pad + n + pad,), SENTINEL, dtype=torch.int32, device=DEV)
    keep = torch.full((pad + e + pad,), 0x5A, dtype=torch.uint8, device=DEV)
    flags = torch.full((pad + 1 + pad,), SENTINEL, dtype=torch.int32, device=DEV)
    fan = (ctypes.c_int32 * 2)(1000, 3)

    def mark(seeds):
        seeds = torch.tensor(seeds, device=DEV)
        _lib.call("kagnn_neighbor_sample_mark", _ptr(g.rowptr), _ptr(g.col), _ptr(g.perm), n, e, _ptr(seeds), seeds.numel(), fan, 2, SEED,
                  _ptr(hop[pad:]), _ptr(keep[pad:]), _ptr(flags[pad:]), ops._stream())
    mark([n, 3, -5, 7, 1 << 33, 11])
    assert int(flags[pad]) == 1 and bool((flags[:pad] == SENTINEL).all()) and bool((flags[pad + 1:] == SENTINEL).all())
    assert bool((hop[:pad] == SENTINEL).all()) and bool((hop[pad + n:] == SENTINEL).all())
    assert bool((keep[:pad] == 0x5A).all()) and bool((keep[pad + e:] == 0x5A).all())
    want_hop, want_keep = sample_reference(ei, n, [3, 7, 11], [1000, 3], SEED)
    assert torch.equal(hop[pad:pad + n].cpu(), want_hop) and torch.equal(keep[pad:pad + e].cpu().bool(), want_keep)
    assert bool((keep[pad:pad + e] <= 1).all())
    mark([3, 7, 11])
    assert int(flags[pad]) == 0


@pytest.mark.parametrize("name", ["b hub", "c source hub"])
def test_outputs_inside_larger_sentinel_filled_buffers_keep_their_tails(name):
    """the three calls of the C ABI by hand, every output of the fill call a slice of a larger buffer"""
    _, _, n, g = _parent(name)
    e = g.num_edges
    want = ops.sample_neighbors([3, 7, 42], [1000, 3], g, seed=SEED)
    ns, es = want.num_nodes, want.num_edges
    seeds = torch.tensor([3, 7, 42], device=DEV)
    hop = torch.empty(n, dtype=torch.int32, device=DEV)
    keep = torch.empty(e, dtype=torch.uint8, device=DEV)
    rec = torch.full((8,), SENTINEL, dtype=torch.int32, device=DEV)
    size = ops._sizes("kagnn_subgraph_workspace_bytes", n, e)
    ws = torch.full((size + 4096,), 0x5A, dtype=torch.uint8, device=DEV)
    parent = [_ptr(t) for t in _arrays(g)]
    fan = (ctypes.c_int32 * 2)(1000, 3)
    _lib.call("kagnn_neighbor_sample_mark", *parent[:3], n, e, _ptr(seeds), 3, fan, 2, SEED, _ptr(hop), _ptr(keep), _ptr(rec[2:]), ops._stream())
    _lib.call("kagnn_edge_subgraph_count", _ptr(hop), _ptr(keep), *parent, n, e, _ptr(ws), size, _ptr(rec), ops._stream())
    assert rec.tolist() == [ns, es, 0] + [SENTINEL] * 5
    assert bool((ws[size:] == 0x5A).all()), "the count call wrote past its workspace"
    pad = 100
    i64 = lambda k: torch.full((k + pad,), SENTINEL, dtype=torch.int64, device=DEV)
    i32 = lambda k: torch.full((k + pad,), SENTINEL, dtype=torch.int32, device=DEV)
    nodes, eids, sei = i64(ns), i64(es), i64(2 * es)
    six = [i32(ns + 1), i32(es), i32(es), i32(ns + 1), i32(es), i32(es)]
    _lib.call("kagnn_edge_subgraph_fill", _ptr(ws), size, _ptr(keep), *parent, n, e, ns, es, _ptr(nodes), _ptr(eids), _ptr(sei),
              *[_ptr(t) for t in six], ops._stream())
    for t, k, ref in [(nodes, ns, want.nodes), (eids, es, want.edge_ids), (sei, 2 * es, want.edge_index.reshape(-1))] + \
                     [(t, r.numel(), r) for t, r in zip(six, _arrays(want.index))]:
        assert torch.equal(t[:k], ref) and bool((t[k:] == SENTINEL).all())
    assert bool((ws[size:] == 0x5A).all())
    # figures that are NOT the count call's (one node and one edge short): refused or harmless, never a write past them
    short = [i64(ns - 1), i64(es - 1), i64(2 * (es - 1))] + [i32(ns), i32(es - 1), i32(es - 1), i32(ns), i32(es - 1), i32(es - 1)]
    _lib.call("kagnn_edge_subgraph_fill", _ptr(ws), size, _ptr(keep), *parent, n, e, ns - 1, es - 1, *[_ptr(t) for t in short], ops._stream())
    for t, k in zip(short, [ns - 1, es - 1, 2 * (es - 1), ns, es - 1, es - 1, ns, es - 1, es - 1]):
        assert bool((t[k:] == SENTINEL).all())
    # an edge selection that breaks the contract (every edge "kept", few nodes selected): the edges with an endpoint outside are
    # dropped from the rows and nothing leaves the outputs
    keep.fill_(1)
    _lib.call("kagnn_edge_subgraph_count", _ptr(hop), _ptr(keep), *parent, n, e, _ptr(ws), size, _ptr(rec), ops._stream())
    ns2, es2 = rec[:2].tolist()
    induced = ops.induced_subgraph(want.nodes, g)
    assert (ns2, es2) == (induced.num_nodes, induced.num_edges)
    outs = [i64(ns2), i64(es2), i64(2 * es2), i32(ns2 + 1), i32(es2), i32(es2), i32(ns2 + 1), i32(es2), i32(es2)]
    _lib.call("kagnn_edge_subgraph_fill", _ptr(ws), size, _ptr(keep), *parent, n, e, ns2, es2, *[_ptr(t) for t in outs], ops._stream())
    for t, k in zip(outs, [ns2, es2, 2 * es2, ns2 + 1, es2, es2, ns2 + 1, es2, es2]):
        assert bool((t[k:] == SENTINEL).all())
    assert torch.equal(outs[0][:ns2], induced.nodes) and torch.equal(outs[3][:ns2 + 1], induced.index.rowptr)
    assert torch.equal(outs[4][:es2], induced.index.col) and torch.equal(outs[7][:es2], induced.index.col_t)


def _sample_and_aggregate(name, fan):
    """the poison / guard-band case form of tests/test_gpu_poison.py: every device result of ``sample_neighbors`` and one aggregation
    on its index"""
    def build():
        _, _, n, g = _parent(name)
        x = torch.randn(n, 24, generator=_gen(3)).to(DEV)

        def run():
            sub = ops.sample_neighbors([3, 7, 42], fan, g, seed=SEED)
            assert 0 < sub.num_edges
            xs = x[sub.nodes]
            return _fields(sub) + [ops._aggregate_raw(xs, sub.index, t, 1.0, None, None, None, None, False) for t in (False, True)]
        return None, run
    return build


CASES = {"sample_neighbors hub graph [1000, 3] + aggregation": ("split", _sample_and_aggregate("b hub", [1000, 3])),
         "sample_neighbors hub graph [40, -1] + aggregation": ("split", _sample_and_aggregate("b hub", [40, -1])),
         "sample_neighbors 70001 nodes [5, 5, 5] + aggregation": ("split", _sample_and_aggregate("e large", [5, 5, 5]))}


@pytest.mark.parametrize("case", list(CASES))
def test_blind_to_the_heap(monkeypatch, case):
    _heap_case(monkeypatch, CASES, case)


@pytest.mark.parametrize("case", list(CASES))
def test_writes_stay_inside_their_buffers(monkeypatch, case):
    _guard_case(monkeypatch, CASES, case)


# ---------------------------------------------------------------------------------------------------------------- models
@pytest.mark.parametrize("kind", ["gin", "gcn"])
@pytest.mark.parametrize("arch", ["kan", "fastkan", "mlp"])
def test_logits_at_the_seeds_with_every_neighbour_kept_equal_the_full_graph(arch, kind):
    ei, _, n, g = _parent("b hub")
    x = torch.randn(n, MF, generator=_gen(7)) * 0.5
    model = _model(arch, kind, True)
    hops = kagnn_amd.receptive_hops(model)
    assert hops == (3 if kind == "gcn" else 2)
    seeds = torch.tensor([3, 11, 42])
    want = _logits64(model, arch, kind, True, x, ei)[seeds]
    model = model.to(DEV)
    sub = ops.sample_neighbors(seeds.to(DEV), [-1] * hops, g, seed=SEED)
    with torch.no_grad():
        got = model(x.to(DEV)[sub.nodes], sub.index)[sub.mapping]
    assert not model.training and 3 < sub.num_nodes < n // 2
    assert_close(got, want, MODEL_TOL, what=f"sampled.{arch}.{kind}.logits")


@pytest.mark.parametrize("kind", ["gcn", "gin"])
def test_one_level_too_few_is_caught(kind):
    """mutation guard on the undirected path 0 - 1 - ... - 13, as in tests/test_gpu_subgraph.py: one level short of
    ``receptive_hops(model)`` must FAIL the check the full depth passes"""
    n = 14
    ei = _undirected_path(n)
    x = torch.randn(n, MF, generator=_gen(8))
    model = _model("kan", kind, True, seed=1)
    seeds = torch.tensor([6])
    want = _logits64(model, "kan", kind, True, x, ei)[seeds]
    model = model.to(DEV)
    g = ops.GraphIndex(ei.to(DEV), n)
    right = kagnn_amd.receptive_hops(model)

    def logits(levels):
        sub = ops.sample_neighbors(seeds.to(DEV), [-1] * levels, g)
        with torch.no_grad():
            return model(x.to(DEV)[sub.nodes], sub.index)[sub.mapping], sub
    got, sub = logits(right)
    assert sub.nodes.tolist() == list(range(6 - right, 7 + right))
    assert_close(got, want, MODEL_TOL, what=f"sampled.path.{kind}.logits")
    short, sub = logits(right - 1)
    assert sub.num_nodes == 2 * (right - 1) + 1
    must_fail(short, want, MODEL_TOL, what=f"sampled.path.{kind}.logits at {right - 1} levels")


# ---------------------------------------------------------------------------------------------------------------- the loader
def _loader_inputs():
    _, ei_dev, n, g = _parent("a")
    gen = _gen(12)
    x = torch.randn(n, 5, generator=gen).to(DEV)
    y = torch.randint(0, 4, (n,), generator=gen).to(DEV)
    ids = torch.randperm(n, generator=gen)[:37].sort().values
    return ei_dev, n, g, x, y, ids


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("drop_last", [False, True])
def test_one_epoch_of_the_loader_partitions_the_input_nodes(shuffle, drop_last):
    ei_dev, n, g, x, y, ids = _loader_inputs()
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    mask[ids.to(DEV)] = True
    for given, graph in ((ids, g), (mask, (ei_dev, n)), (ids.to(DEV), g)):
        loader = kagnn_amd.NeighborLoader(graph, given, [3, 2], 10, shuffle=shuffle, drop_last=drop_last, generator=_gen(5), seed=77, x=x, y=y)
        order = ids[kagnn_amd.data.epoch_order(37, shuffle, _gen(5))]
        batches = list(loader)
        assert len(batches) == len(loader) == (3 if drop_last else 4) and loader.epoch == 1
        seen = torch.cat([b.seeds for b in batches]).cpu()
        assert torch.equal(seen, order[:30] if drop_last else order)
        assert [b.num_seeds for b in batches] == ([10, 10, 10] if drop_last else [10, 10, 10, 7])
        for i, b in enumerate(batches):
            assert isinstance(b, kagnn_amd.NodeBatch) and isinstance(b.index, ops.GraphIndex)
            assert torch.equal(b.x, x[b.nodes]) and torch.equal(b.y, y[b.seeds]) and torch.equal(b.nodes[b.seed_rows], b.seeds)
            assert b.seeds.dtype == b.seed_rows.dtype == torch.int64 and b.seeds.device == x.device
            want = ops.sample_neighbors(b.seeds, [3, 2], g, seed=loader.sampling_seed(0, i))
            assert loader.sampling_seed(0, i) == (77 + GOLDEN * (1 + i)) % (1 << 64)
            assert (b.num_nodes, b.num_edges) == (want.num_nodes, want.num_edges)
            got = [b.nodes, b.edge_index, b.edge_ids, b.seed_rows, b.hops, *_arrays(b.index)]
            assert all(torch.equal(p, q) for p, q in zip(got, _fields(want)))
    bare = next(iter(kagnn_amd.NeighborLoader(g, ids, [3, 2], 10)))
    assert bare.x is None and bare.y is None


def test_two_loaders_built_alike_agree_and_epochs_differ():
    _, n, g, x, y, ids = _loader_inputs()
    make = lambda: kagnn_amd.NeighborLoader(g, ids, [3, 2], 10, shuffle=False, seed=77, x=x, y=y)
    a, b = make(), make()
    epochs = []
    for t in range(2):
        ba, bb = list(a), list(b)
        for p, q in zip(ba, bb):
            for f in ("nodes", "edge_index", "edge_ids", "hops", "seed_rows", "seeds", "x", "y"):
                assert torch.equal(getattr(p, f), getattr(q, f)), f
            assert all(torch.equal(u, v) for u, v in zip(_arrays(p.index), _arrays(q.index)))
        epochs.append(ba)
    assert a.epoch == b.epoch == 2
    # the same seeds in both epochs (no shuffle), other sampling seeds: other neighbourhoods
    assert all(torch.equal(p.seeds, q.seeds) for p, q in zip(*epochs))
    assert any(not torch.equal(p.edge_ids, q.edge_ids) for p, q in zip(*epochs))
    assert a.sampling_seed(1, 0) == (77 + GOLDEN * 5) % (1 << 64)
    want = ops.sample_neighbors(epochs[1][2].seeds, [3, 2], g, seed=a.sampling_seed(1, 2))
    assert torch.equal(epochs[1][2].edge_ids, want.edge_ids)
    # with shuffle, two loaders with generators seeded alike agree too
    c = kagnn_amd.NeighborLoader(g, ids, [3, 2], 10, shuffle=True, generator=_gen(9), seed=1)
    d = kagnn_amd.NeighborLoader(g, ids, [3, 2], 10, shuffle=True, generator=_gen(9), seed=1)
    for _ in range(2):
        for p, q in zip(c, d):
            assert torch.equal(p.seeds, q.seeds) and torch.equal(p.edge_ids, q.edge_ids) and torch.equal(p.nodes, q.nodes)


# ---------------------------------------------------------------------------------------------------------------- the training loop
TN, TC, TF = 600, 3, 8
_TRAIN = {}


def _planted():
    """600 nodes in 3 classes; 3000 edges, four in five inside a class; features = a class direction plus noise"""
    if "data" not in _TRAIN:
        gen = _gen(20)
        y = torch.randint(0, TC, (TN,), generator=gen)
        src = torch.randint(0, TN, (3000,), generator=gen)
        same = torch.rand(3000, generator=gen) < 0.8
        cand = torch.randint(0, TN, (3000, 8), generator=gen)
        hit = (y[cand] == y[src][:, None]) == same[:, None]
        dst = cand[torch.arange(3000), hit.float().argmax(1)]
        ei = torch.stack([torch.cat([src, dst]), torch.cat([dst, src])]).contiguous()
        x = torch.randn(TC, TF, generator=gen)[y] * 0.7 + torch.randn(TN, TF, generator=gen)
        split = torch.rand(TN, generator=gen)
        masks = [split < 0.5, (split >= 0.5) & (split < 0.75), split >= 0.75]
        _TRAIN["data"] = [t.to(DEV) for t in (x, ei, y, *masks)]
    return _TRAIN["data"]


def _fresh_model():
    """the same starting weights every time: KANLinear's initial spline coefficients come from a least-squares solve on the CPU whose
    last bits vary from one construction to the next, so the first construction's state is kept and loaded"""
    torch.manual_seed(31)
    model = kagnn_amd.GKAN_Nodes("gin", 2, TF, 8, TC, grid_size=4, spline_order=3, hidden_layers=2)
    if "init" not in _TRAIN:
        _TRAIN["init"] = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.load_state_dict(_TRAIN["init"])
    return model.to(DEV)


def _trained(seed=5, poll_every=16):
    key = (seed, poll_every)
    if key not in _TRAIN:
        x, ei, y, tr, va, te = _planted()
        model = _fresh_model()
        res = harness.train_node_classification_sampled(model, x, ei, y, tr, va, te, fanouts=[5, 5], batch_size=64, seed=seed, epochs=3, lr=1e-2,
                                                        poll_every=poll_every)
        _TRAIN[key] = ({k: v.detach().clone() for k, v in model.state_dict().items()}, res)
    return _TRAIN[key]


def _same(a, b):
    return a[1].best_epoch == b[1].best_epoch and a[1].epochs_run == b[1].epochs_run and torch.equal(a[1].history, b[1].history) and \
        all(torch.equal(v, b[0][k]) for k, v in a[0].items())


def test_the_sampled_training_loop_is_the_loop_written_out():
    x, ei, y, tr, va, te = _planted()
    got_state, got = _trained()
    assert got.epochs_run == 3 and not got.stopped and got.history.shape == (3, 3, 3)
    model = _fresh_model()
    g = ops.graph_index(ei, TN)
    loader = kagnn_amd.NeighborLoader(g, tr, [5, 5], 64, shuffle=True, generator=torch.Generator().manual_seed(5), seed=5, x=x, y=y)
    assert len(loader) == (int(tr.sum()) + 63) // 64 >= 4
    optimizer = harness.Adam(model.parameters(), lr=1e-2)
    best = harness._BestWeights(model, "test")
    stop = ops.EarlyStop(100, 0.0, max_epochs=3, num_splits=3, device=x.device)
    bits = ops.split_bits(tr, va, te)
    records = torch.empty((3, 3), dtype=torch.int64, device=x.device)
    step = harness._training_step(optimizer)

    def loss_of(batch):
        return ops.softmax_cross_entropy(model(batch.x, batch.index)[batch.seed_rows], batch.y)
    for _ in range(3):
        model.train()
        for batch in loader:
            step(loss_of, batch)
        model.eval()
        with torch.no_grad():
            out = model(x, g)
        ops.node_eval(out, y, bits, 3, out=records)
        stop.update(records, 1)
        ops.copy_if(stop.improved, best.saved, best.live)
    st = stop.read()
    best.restore()
    assert st.epochs == got.epochs_run and st.best_epoch == got.best_epoch and torch.equal(st.history, got.history)
    for k, v in model.state_dict().items():
        assert torch.equal(v, got_state[k]), k
    # the figures are the last counted epoch's
    val_loss, val_acc = harness._split_figures(got.history[2, 1])
    assert got.val_loss == val_loss and got.val_acc == val_acc and 0.0 <= got.test_acc <= 1.0 and val_loss == val_loss


def test_the_sampled_training_loop_repeats_itself_and_follows_its_seed():
    base = _trained()
    again = _TRAIN.pop((5, 16))
    assert _same(_trained(), again)
    assert _same(_trained(poll_every=1), base)
    other = _trained(seed=6)
    assert not all(torch.equal(v, other[0][k]) for k, v in base[0].items())
