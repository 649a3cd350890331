"""k-hop and induced subgraphs on the device (``ops.k_hop_subgraph``, ``ops.induced_subgraph``: csrc/subgraph.hip), what a model
computes on them (``kagnn_amd.receptive_hops``) and the local form of ``kagnn_amd.explain_edges`` (``num_hops=``).

Integer results have no tolerance.  Node sets, hop distances, ``edge_ids``, the relabelled edge list and ``mapping`` are held to a
boolean-mask BFS in torch ops on the CPU -- the algorithm of torch_geometric's ``k_hop_subgraph`` (``flow='source_to_target'``,
``relabel_nodes=True``), restated in ``_bfs``; the six index arrays to ``GraphIndex(sub.edge_index, sub.num_nodes)`` on the device, bit
for bit, with ``ops._SMALL_CSR`` both True and False.  Models: logits at the seeds from the subgraph at ``receptive_hops(model)``
against fp64 on the FULL graph, to 1e-4 of the tensor's own maximum (the whole-model rule of tests/test_gpu_models.py).  The fp64
side is ``oracle.node_model_forward(training=False)`` for the KAN / FastKAN models -- ``helpers.oracle_node_model_fwd_bwd`` wraps
that function in training mode only, and the subgraph statement holds in eval mode only (the batch statistics of a subgraph are
another function) -- and the fp64 convolutions of tests/test_gpu_baselines.py for the MLP models."""
import pytest
import torch

import kagnn_amd
from kagnn_amd import _lib, ops
from kagnn_amd import baselines as B
from oracle import kan_oracle as orc
from helpers import assert_close, must_fail
from test_gpu_baselines import ATT_SCALE, _conv64, _params64
from test_gpu_poison import _guard_case, _heap_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODEL_TOL = 1e-4


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------- graphs
def _graph_a():
    """300 nodes / 900 edges: 870 random, 20 of them repeated, 10 self loops"""
    g = _gen(0)
    ei = torch.randint(0, 300, (2, 900), generator=g)
    ei[:, 870:890] = ei[:, 100:120]
    ei[1, 890:900] = ei[0, 890:900]
    return ei, 300


def _graph_b():
    """(a) plus a 1613-edge destination hub at node 7, its edges scattered through the list: the parent's row has hub segments and
    the ordered compaction of that row runs 26 chunks"""
    ei, n = _graph_a()
    g = _gen(1)
    hub = torch.stack([torch.randint(0, n, (1613,), generator=g), torch.full((1613,), 7)])
    both = torch.cat([ei, hub], 1)
    return both[:, torch.randperm(both.size(1), generator=g)].contiguous(), n


def _graph_c():
    ei, n = _graph_b()
    return ei.flip(0).contiguous(), n


def _graph_d():
    return torch.stack([torch.arange(0, 9), torch.arange(1, 10)]), 10


def _graph_e():
    g = _gen(2)
    return torch.randint(0, 70001, (2, 400_000), generator=g), 70001


GRAPHS = {"a": _graph_a, "b hub": _graph_b, "c source hub": _graph_c, "d path": _graph_d, "e large": _graph_e,
          "f one node": lambda: (torch.zeros(2, 0, dtype=torch.int64), 1), "f no edges": lambda: (torch.zeros(2, 0, dtype=torch.int64), 5),
          "f isolated seed": lambda: (torch.tensor([[1, 2, 3, 1], [2, 3, 1, 3]]), 5)}
SEEDS = {"a": [3, 11, 42], "b hub": [3, 7, 42], "c source hub": [3, 7, 42], "d path": [9, 0, 5], "e large": [5, 40_000, 70_000],
         "f one node": [0], "f no edges": [4, 0, 2], "f isolated seed": [0, 4, 0]}
_PARENTS = {}


def _parent(name):
    """(edge_index on the CPU, on the device, N, GraphIndex): one per graph and session, never modified.  The two hub graphs are
    indexed by the sort-based build whatever their size, so that the parent's hub row comes with hub segments"""
    if name not in _PARENTS:
        ei, n = GRAPHS[name]()
        dev = ei.to(DEV)
        small = ops._SMALL_CSR
        ops._SMALL_CSR = small and "hub" not in name
        try:
            _PARENTS[name] = (ei, dev, n, ops.GraphIndex(dev, n))
        finally:
            ops._SMALL_CSR = small
    return _PARENTS[name]


# ---------------------------------------------------------------------------------------------------------------- references
def _bfs(seeds, k, ei, n):
    """torch_geometric's k_hop_subgraph restated (CPU): hop[i] = least number of hops from i to a seed along edge direction"""
    src, dst = ei
    hop = torch.full((n,), -1, dtype=torch.int32)
    hop[seeds] = 0
    for d in range(k):
        front = hop == d
        new = torch.zeros(n, dtype=torch.bool)
        new[src[front[dst]]] = True
        hop[new & (hop < 0)] = d + 1
    return hop


def _expected(sel, ei, n):
    """(nodes, relabelled edge list, edge ids, relabel) of the subgraph induced by the bool mask ``sel``"""
    nodes = sel.nonzero().flatten()
    keep = sel[ei[0]] & sel[ei[1]]
    rel = torch.full((n,), -1, dtype=torch.int64)
    rel[nodes] = torch.arange(nodes.numel())
    return nodes, rel[ei[:, keep]], keep.nonzero().flatten(), rel


def _arrays(g):
    return [g.rowptr, g.col, g.perm, g.rowptr_t, g.col_t, g.perm_t]


def _check(sub, name, sel, seeds, hop, monkeypatch, what):
    ei, _, n, _ = _parent(name)
    nodes, sei, eids, rel = _expected(sel, ei, n)
    assert (sub.num_nodes, sub.num_edges) == (nodes.numel(), eids.numel()), what
    assert sub.nodes.dtype == sub.edge_ids.dtype == sub.edge_index.dtype == torch.int64
    assert torch.equal(sub.nodes.cpu(), nodes), what
    assert torch.equal(sub.edge_ids.cpu(), eids), what
    assert sub.edge_index.shape == (2, eids.numel()) and torch.equal(sub.edge_index.cpu(), sei), what
    if seeds is None:
        assert sub.mapping is None
    else:
        assert sub.mapping.dtype == torch.int64 and torch.equal(sub.mapping.cpu(), rel[seeds]), what
    if hop is None:
        assert sub.hops is None
    else:
        assert sub.hops.dtype == torch.int32 and torch.equal(sub.hops.cpu(), hop[nodes]), what
    idx = sub.index
    assert (idx.num_nodes, idx.num_edges, idx.num_hub_seg, idx.num_hub_seg_t) == (sub.num_nodes, sub.num_edges, 0, 0)
    assert all(t.dtype == torch.int32 for t in _arrays(idx))
    assert [t.numel() for t in _arrays(idx)] == [sub.num_nodes + 1, sub.num_edges, sub.num_edges] * 2
    if sub.num_nodes == 0:
        assert int(idx.rowptr[0]) == 0 and int(idx.rowptr_t[0]) == 0
        return
    for small in (True, False):
        monkeypatch.setattr(ops, "_SMALL_CSR", small)
        want = ops.GraphIndex(sub.edge_index.contiguous(), sub.num_nodes)
        for k, (a, b) in enumerate(zip(_arrays(idx), _arrays(want))):
            assert torch.equal(a, b), f"{what}: index array {k} differs from a build (small path {small})"
    monkeypatch.undo()


def _seed_sets(name):
    n = _parent(name)[2]
    s = SEEDS[name]
    return {"one": s[:1], "three": s, "duplicated": [s[0], s[-1], s[0]], "all": list(range(n))}


# ---------------------------------------------------------------------------------------------------------------- k hops
@pytest.mark.parametrize("name", list(GRAPHS))
def test_k_hop_subgraph_equals_the_bfs_and_a_rebuild(name, monkeypatch):
    ei, _, n, g = _parent(name)
    sizes = []
    for hops in (0, 1, 2, 3, 12):                        # 12: past the diameter of the path graph (d)
        for label, seeds in _seed_sets(name).items():
            if name == "e large" and label == "all" and hops not in (0, 3):
                continue                                # (the whole 400k-edge graph: first and last level only)
            st = torch.tensor(seeds, dtype=torch.int64)
            sub = ops.k_hop_subgraph(st.to(DEV), hops, g)
            hop = _bfs(st, hops, ei, n)
            _check(sub, name, hop >= 0, st, hop, monkeypatch, f"{name}: {label} seeds, {hops} hops")
            if label == "three":
                sizes.append(sub.num_nodes)
    if name == "a":
        assert sizes[0] == 3 and sizes[0] < sizes[1] < sizes[2] < sizes[3] < n, sizes      # a strict subset that grows with every hop
    if name == "e large":
        assert 3 < sizes[3] < n // 10, sizes


def test_reachability_follows_the_edge_direction():
    """the path 0 -> 1 -> ... -> 9: node 9 is reached from 9 - k .. 9 within k hops, node 0 from nobody but itself"""
    g = _parent("d path")[3]
    for k in range(0, 12):
        sub = ops.k_hop_subgraph(9, k, g)
        assert sub.nodes.tolist() == list(range(max(9 - k, 0), 10)) and sub.hops.tolist() == list(range(min(k, 9), -1, -1))
        assert sub.edge_ids.tolist() == list(range(max(9 - k, 0), 9)) and sub.mapping.tolist() == [sub.num_nodes - 1]
        sub = ops.k_hop_subgraph([0], k, g)
        assert sub.nodes.tolist() == [0] and sub.num_edges == 0 and sub.mapping.tolist() == [0]


def test_seeds_as_int_list_and_tensor_and_empty_seeds():
    ei, _, n, g = _parent("a")
    a, b, c = ops.k_hop_subgraph(11, 2, g), ops.k_hop_subgraph([11], 2, g), ops.k_hop_subgraph(torch.tensor(11, device=DEV), 2, g)
    for f in ("nodes", "edge_index", "edge_ids", "mapping", "hops"):
        assert torch.equal(getattr(a, f), getattr(b, f)) and torch.equal(getattr(a, f), getattr(c, f)), f
    for empty in ([], torch.empty(0, dtype=torch.int64, device=DEV)):
        sub = ops.k_hop_subgraph(empty, 3, g)
        assert (sub.num_nodes, sub.num_edges) == (0, 0) and sub.nodes.numel() == 0 and sub.edge_index.shape == (2, 0)
        assert sub.mapping.numel() == 0 and sub.hops.numel() == 0 and sub.index.rowptr.tolist() == [0] and sub.index.rowptr_t.tolist() == [0]
        sub = ops.induced_subgraph(empty, g)
        assert (sub.num_nodes, sub.num_edges) == (0, 0) and sub.hops is None


# ---------------------------------------------------------------------------------------------------------------- induced
@pytest.mark.parametrize("name", list(GRAPHS))
def test_induced_subgraph_equals_the_mask_and_a_rebuild(name, monkeypatch):
    ei, ei_dev, n, g = _parent(name)
    pick = torch.rand(n, generator=_gen(5)) < 0.4
    pick[SEEDS[name][0]] = True
    if name in ("b hub", "c source hub"):
        pick[7] = True                                   # the hub's row survives in part: kept and dropped entries in every chunk
    ids = pick.nonzero().flatten()
    shuffled = ids[torch.randperm(ids.numel(), generator=_gen(6))]
    cases = {"ids": ids, "shuffled ids with duplicates": torch.cat([shuffled, shuffled[:3], shuffled[-1:]]), "mask": pick,
             "all ids": torch.arange(n), "all mask": torch.ones(n, dtype=torch.bool), "no ids": torch.empty(0, dtype=torch.int64),
             "no mask": torch.zeros(n, dtype=torch.bool)}
    for label, arg in cases.items():
        sub = ops.induced_subgraph(arg.to(DEV), g)
        if arg.dtype == torch.bool:
            sel, seeds = arg, None
        else:
            sel, seeds = torch.zeros(n, dtype=torch.bool), arg
            sel[arg] = True
        _check(sub, name, sel, seeds, None, monkeypatch, f"{name}: induced, {label}")
        if label.startswith("all"):                      # the subgraph of all nodes IS the parent
            assert torch.equal(sub.edge_index, ei_dev) and torch.equal(sub.nodes.cpu(), torch.arange(n))
            assert torch.equal(sub.edge_ids.cpu(), torch.arange(ei.size(1)))
            for k, (a, b) in enumerate(zip(_arrays(sub.index), _arrays(g))):
                assert torch.equal(a, b), f"{name}: array {k} of the subgraph of all nodes differs from the parent's"
    if name == "b hub":
        row = g.rowptr[7:9].tolist()
        assert row[1] - row[0] >= 1613 and g.num_hub_seg > 0 and (row[1] - row[0] + 63) // 64 == 26


def _fields(sub):
    return [t for t in (sub.nodes, sub.edge_index, sub.edge_ids, sub.mapping, sub.hops, *_arrays(sub.index)) if t is not None]


@pytest.mark.parametrize("name", ["b hub", "c source hub", "e large"])
def test_a_second_call_returns_the_same_bits(name):
    g = _parent(name)[3]
    first = _fields(ops.k_hop_subgraph(SEEDS[name], 2, g))
    junk = torch.full((1 << 20,), -7, dtype=torch.int32, device=DEV)      # (the allocator hands the next call other memory)
    second = _fields(ops.k_hop_subgraph(SEEDS[name], 2, g))
    del junk
    assert len(first) == len(second) == 11 and all(torch.equal(a, b) for a, b in zip(first, second))


# ---------------------------------------------------------------------------------------------------------------- bounds
SENTINEL = -1234567


def _ptr(t):
    return ops._ptr(t)


def test_an_out_of_range_seed_raises_and_nothing_is_written_past_the_buffers():
    ei, _, n, g = _parent("b hub")
    for bad in ([3, n], [-1, 3], [3, 1 << 40], [n]):
        with pytest.raises(ValueError, match="outside"):
            ops.k_hop_subgraph(bad, 2, g)
        with pytest.raises(ValueError, match="outside"):
            ops.induced_subgraph(torch.tensor(bad, device=DEV), g)
    # the mark call itself: the bad seeds are skipped and flagged, the good ones marked, the bytes around hop and flags untouched
    pad = 64
    hop = torch.full((pad + n + pad,), SENTINEL, dtype=torch.int32, device=DEV)
    flags = torch.full((pad + 1 + pad,), SENTINEL, dtype=torch.int32, device=DEV)
    seeds = torch.tensor([n, 3, -5, 42, 1 << 33, 11], device=DEV)
    _lib.call("kagnn_k_hop_mark", _ptr(g.rowptr), _ptr(g.col), n, _ptr(seeds), seeds.numel(), 2, _ptr(hop[pad:]), _ptr(flags[pad:]), ops._stream())
    assert int(flags[pad]) == 1 and bool((flags[:pad] == SENTINEL).all()) and bool((flags[pad + 1:] == SENTINEL).all())
    assert bool((hop[:pad] == SENTINEL).all()) and bool((hop[pad + n:] == SENTINEL).all())
    assert torch.equal(hop[pad:pad + n].cpu(), _bfs(torch.tensor([3, 42, 11]), 2, ei, n))
    seeds = torch.tensor([3, 42, 11], device=DEV)
    _lib.call("kagnn_k_hop_mark", _ptr(g.rowptr), _ptr(g.col), n, _ptr(seeds), seeds.numel(), 2, _ptr(hop[pad:]), _ptr(flags[pad:]), ops._stream())
    assert int(flags[pad]) == 0


@pytest.mark.parametrize("name", ["b hub", "c source hub", "e large"])
def test_outputs_inside_larger_sentinel_filled_buffers_keep_their_tails(name):
    """the three calls of the C ABI by hand, every output of the fill call a slice of a larger buffer"""
    ei, _, n, g = _parent(name)
    e = g.num_edges
    want = ops.k_hop_subgraph(SEEDS[name], 2, g)
    ns, es = want.num_nodes, want.num_edges
    seeds = torch.tensor(SEEDS[name], device=DEV)
    hop = torch.empty(n, dtype=torch.int32, device=DEV)
    rec = torch.full((8,), SENTINEL, dtype=torch.int32, device=DEV)
    size = ops._sizes("kagnn_subgraph_workspace_bytes", n, e)
    ws = torch.full((size + 4096,), 0x5A, dtype=torch.uint8, device=DEV)
    parent = [_ptr(t) for t in _arrays(g)]
    _lib.call("kagnn_k_hop_mark", parent[0], parent[1], n, _ptr(seeds), 3, 2, _ptr(hop), _ptr(rec[2:]), ops._stream())
    _lib.call("kagnn_subgraph_count", _ptr(hop), *parent, n, e, _ptr(ws), size, _ptr(rec), ops._stream())
    assert rec.tolist() == [ns, es, 0] + [SENTINEL] * 5
    assert bool((ws[size:] == 0x5A).all()), "the count call wrote past its workspace"
    pad = 100
    i64 = lambda k: torch.full((k + pad,), SENTINEL, dtype=torch.int64, device=DEV)
    i32 = lambda k: torch.full((k + pad,), SENTINEL, dtype=torch.int32, device=DEV)
    nodes, eids, sei = i64(ns), i64(es), i64(2 * es)
    six = [i32(ns + 1), i32(es), i32(es), i32(ns + 1), i32(es), i32(es)]
    _lib.call("kagnn_subgraph_fill", _ptr(ws), size, *parent, n, e, ns, es, _ptr(nodes), _ptr(eids), _ptr(sei), *[_ptr(t) for t in six], ops._stream())
    for t, k, ref in [(nodes, ns, want.nodes), (eids, es, want.edge_ids), (sei, 2 * es, want.edge_index.reshape(-1))] + \
                     [(t, r.numel(), r) for t, r in zip(six, _arrays(want.index))]:
        assert torch.equal(t[:k], ref) and bool((t[k:] == SENTINEL).all())
    assert bool((ws[size:] == 0x5A).all())
    # figures that are NOT the count call's (one node and one edge short): refused or harmless, never a write past them
    short = [i64(ns - 1), i64(es - 1), i64(2 * (es - 1))] + [i32(ns), i32(es - 1), i32(es - 1), i32(ns), i32(es - 1), i32(es - 1)]
    _lib.call("kagnn_subgraph_fill", _ptr(ws), size, *parent, n, e, ns - 1, es - 1, *[_ptr(t) for t in short], ops._stream())
    for t, k in zip(short, [ns - 1, es - 1, 2 * (es - 1), ns, es - 1, es - 1, ns, es - 1, es - 1]):
        assert bool((t[k:] == SENTINEL).all())


def _extract_and_aggregate(name, hops):
    """the poison / guard-band case form of tests/test_gpu_poison.py: every device result of ``k_hop_subgraph`` and one aggregation on
    its index"""
    def build():
        _, _, n, g = _parent(name)
        x = torch.randn(n, 24, generator=_gen(3)).to(DEV)

        def run():
            sub = ops.k_hop_subgraph(SEEDS[name], hops, g)
            assert 0 < sub.num_edges
            xs = x[sub.nodes]
            return _fields(sub) + [ops._aggregate_raw(xs, sub.index, t, 1.0, None, None, None, None, False) for t in (False, True)]
        return None, run
    return build


CASES = {"k_hop_subgraph hub graph 2 hops + aggregation": ("split", _extract_and_aggregate("b hub", 2)),
         "k_hop_subgraph 70001 nodes 3 hops + aggregation": ("split", _extract_and_aggregate("e large", 3))}


@pytest.mark.parametrize("case", list(CASES))
def test_blind_to_the_heap(monkeypatch, case):
    _heap_case(monkeypatch, CASES, case)


@pytest.mark.parametrize("case", list(CASES))
def test_writes_stay_inside_their_buffers(monkeypatch, case):
    _guard_case(monkeypatch, CASES, case)


# ---------------------------------------------------------------------------------------------------------------- models
MF, MH, MC = 9, 8, 5


def _model(arch, kind, skip, seed=0):
    torch.manual_seed(40 + seed)
    if arch == "kan":
        m = kagnn_amd.GKAN_Nodes(kind, 2, MF, MH, MC, skip=skip, grid_size=4, spline_order=3, hidden_layers=2, heads=2)
    elif arch == "fastkan":
        m = kagnn_amd.GFASTKAN_Nodes(kind, 2, MF, MH, MC, skip=skip, grid_size=4, hidden_layers=2, heads=2)
    else:
        m = B.GNN_Nodes(kind, 2, MF, MH, MC, skip=skip, hidden_layers=2, heads=2)
    gen = _gen(50 + seed)
    for bn in m.bns:                                   # eval mode normalises with the running statistics: off their 0 / 1 start
        bn.running_mean.copy_(0.3 * torch.randn(bn.running_mean.shape, generator=gen))
        bn.running_var.copy_(0.5 + torch.rand(bn.running_var.shape, generator=gen))
    return m.eval()


def _logits64(model, arch, kind, skip, x, ei):
    """eval-mode logits of the whole graph in fp64 on the CPU"""
    if arch in ("kan", "fastkan"):
        st = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in model.state_dict().items()}
        return orc.node_model_forward(x.double(), ei, st, arch, kind, 2, 3, skip=skip, training=False).detach()
    P = {k: v.detach() for k, v in _params64(model).items()}
    outs = [x.double()]
    h = outs[0]
    for i, (conv, bn) in enumerate(zip(model.convs, model.bns)):
        h = _conv64(P, f"convs.{i}.", conv, h, ei, [])
        h = (h - bn.running_mean.double().cpu()) / torch.sqrt(bn.running_var.double().cpu() + bn.eps) * P[f"bns.{i}.weight"] + P[f"bns.{i}.bias"]
        outs.append(h)
    del ATT_SCALE[:]                                   # (_conv64's note for the gradient checks of its own file: not used here)
    return (torch.cat(outs, 1) if skip else h) @ P["lay_out.weight"].t() + P["lay_out.bias"]


def _logits_on_subgraph(model, x_dev, g, seeds, hops):
    sub = ops.k_hop_subgraph(seeds, hops, g)
    with torch.no_grad():
        return model(x_dev[sub.nodes], sub.index)[sub.mapping], sub


@pytest.mark.parametrize("skip", [True, False], ids=["skip", "noskip"])
@pytest.mark.parametrize("kind", ["gin", "gcn", "gat"])
@pytest.mark.parametrize("arch", ["kan", "fastkan", "mlp"])
def test_logits_at_the_seeds_from_the_receptive_field_equal_the_full_graph(arch, kind, skip):
    ei, _, n, g = _parent("b hub")
    x = torch.randn(n, MF, generator=_gen(7)) * 0.5
    model = _model(arch, kind, skip)
    hops = kagnn_amd.receptive_hops(model)
    assert hops == (3 if kind == "gcn" else 2)
    seeds = torch.tensor([3, 11, 42])                  # (their receptive field is a strict subset: 26 nodes at 2 hops, 70 at 3)
    want = _logits64(model, arch, kind, skip, x, ei)[seeds]
    model = model.to(DEV)
    got, sub = _logits_on_subgraph(model, x.to(DEV), g, seeds.to(DEV), hops)
    assert not model.training and 3 < sub.num_nodes < n // 2
    assert_close(got, want, MODEL_TOL, what=f"subgraph.{arch}.{kind}.{'skip' if skip else 'noskip'}.logits")


def _undirected_path(n):
    a = torch.arange(n - 1)
    return torch.stack([torch.cat([a, a + 1]), torch.cat([a + 1, a])]).contiguous()


@pytest.mark.parametrize("kind", ["gcn", "gin"])
def test_one_hop_too_few_is_caught(kind):
    """mutation guard on the undirected path 0 - 1 - ... - 13: a 2-layer gcn model on 2 hops (the leaf of the subgraph has degree 2
    where the full graph gives it 3) and a 2-layer gin model on 1 hop must FAIL the check they pass at receptive_hops"""
    n = 14
    ei = _undirected_path(n)
    x = torch.randn(n, MF, generator=_gen(8))
    model = _model("kan", kind, True, seed=1)
    seeds = torch.tensor([6])
    want = _logits64(model, "kan", kind, True, x, ei)[seeds]
    model = model.to(DEV)
    g = ops.GraphIndex(ei.to(DEV), n)
    right = kagnn_amd.receptive_hops(model)
    assert right == (3 if kind == "gcn" else 2)
    got, sub = _logits_on_subgraph(model, x.to(DEV), g, seeds.to(DEV), right)
    assert sub.nodes.tolist() == list(range(6 - right, 7 + right))
    assert_close(got, want, MODEL_TOL, what=f"subgraph.path.{kind}.logits")
    short, sub = _logits_on_subgraph(model, x.to(DEV), g, seeds.to(DEV), right - 1)
    assert sub.num_nodes == 2 * (right - 1) + 1
    must_fail(short, want, MODEL_TOL, what=f"subgraph.path.{kind}.logits at {right - 1} hops")


# ---------------------------------------------------------------------------------------------------------------- explain_edges
def _snapshot(model):
    return ({k: v.detach().clone() for k, v in model.state_dict().items()}, [m.training for m in model.modules()],
            [None if p.grad is None else p.grad.clone() for p in model.parameters()])


@pytest.mark.parametrize("kind", ["gin", "gcn"])
def test_local_explanation_is_the_explanation_of_the_subgraph(kind):
    ei, ei_dev, n, g = _parent("a")
    x = torch.randn(n, MF, generator=_gen(9)) * 0.5
    model = _model("kan", kind, True, seed=2)
    node = 11
    full64 = _logits64(model, "kan", kind, True, x, ei)[node]
    top = full64.topk(2).values
    assert float(top[0] - top[1]) > 1e-3, "precondition: the fp64 logit margin at the node (pick another seed)"
    model = model.to(DEV).train()
    model.bns[0].eval()
    xd = x.to(DEV)
    before = _snapshot(model)
    hops = kagnn_amd.receptive_hops(model)
    sub = ops.k_hop_subgraph(node, hops, g)
    assert 1 < sub.num_nodes < n and 0 < sub.num_edges < ei.size(1)
    kw = dict(epochs=6, lr=0.05)
    got = kagnn_amd.explain_edges(model, xd, ei_dev, node_idx=node, num_hops=hops, generator=_gen(21), **kw)
    hand = kagnn_amd.explain_edges(model, xd[sub.nodes], sub.edge_index, node_idx=sub.mapping, generator=_gen(21), **kw)
    assert got["edge_mask"].shape == (ei.size(1),) and torch.equal(got["nodes"], sub.nodes) and torch.equal(got["edge_ids"], sub.edge_ids)
    assert torch.equal(got["edge_mask"][sub.edge_ids], hand["edge_mask"]) and float(hand["edge_mask"].min()) > 0.0
    off = torch.ones(ei.size(1), dtype=torch.bool, device=DEV)
    off[sub.edge_ids] = False
    assert bool((got["edge_mask"][off] == 0).all())
    assert torch.equal(got["feature_mask"], hand["feature_mask"]) and torch.equal(got["losses"], hand["losses"])
    assert got["losses"].numel() == 6 and float(got["losses"][-1]) < float(got["losses"][0])
    # "auto" is receptive_hops(model)
    auto = kagnn_amd.explain_edges(model, xd, ei_dev, node_idx=node, num_hops="auto", generator=_gen(21), **kw)
    assert all(torch.equal(auto[k], got[k]) for k in ("edge_mask", "feature_mask", "losses", "nodes", "edge_ids"))
    # the default target is the full graph's prediction at the node; a target of length N is gathered at sub.nodes
    model.eval()
    with torch.no_grad():
        full_target = model(xd, ei_dev).argmax(-1)
        sub_target = model(xd[sub.nodes], sub.index).argmax(-1)
    assert int(full_target[node]) == int(full64.argmax()) == int(sub_target[sub.mapping])
    model.train()
    model.bns[0].eval()
    given = kagnn_amd.explain_edges(model, xd, ei_dev, node_idx=node, num_hops=hops, target=full_target, generator=_gen(21), **kw)
    assert all(torch.equal(given[k], got[k]) for k in ("edge_mask", "feature_mask", "losses"))
    other = (full_target + 1) % MC
    moved = kagnn_amd.explain_edges(model, xd, ei_dev, node_idx=node, num_hops=hops, target=other, generator=_gen(21), **kw)
    assert not torch.equal(moved["losses"], got["losses"])
    # nothing of the model has changed
    after = _snapshot(model)
    assert all(torch.equal(after[0][k], v) for k, v in before[0].items()) and after[1] == before[1]
    assert all(p is None for p in after[2])
    with pytest.raises(ValueError, match="node_idx"):
        kagnn_amd.explain_edges(model, xd, ei_dev, num_hops=2)
