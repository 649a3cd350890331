"""kagnn_amd.data on the device: the one-launch mini-batch assembly (``kagnn_batch_assemble``) against a plain torch restatement of
torch_geometric's collation, bit for bit -- nothing here rounds, so every comparison is ``torch.equal``.

``collate`` is the yardstick (the same function as in tests/test_data_cpu.py): ``torch.cat`` of per-graph slices, ``edge_index`` +
node offset, ``repeat_interleave`` for ``batch``, ``cumsum`` for ``ptr`` -- the definition of ``Batch.from_data_list`` for these
attributes ("parity unpinned": torch_geometric itself is not installed where this project is tested)."""
import copy
from types import SimpleNamespace

import pytest
import torch

import kagnn_amd
from kagnn_amd import _lib, data, harness, ops
from test_gpu_poison import _GuardedEmpty, _under_every_pattern

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def collate(x, edge_index, node_ptr, edge_ptr, ids, edge_attr=None, y=None):
    ids = [int(g) for g in ids]
    sizes = torch.tensor([int(node_ptr[g + 1] - node_ptr[g]) for g in ids], dtype=torch.int64)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)])
    out = {"x": torch.cat([x[node_ptr[g]:node_ptr[g + 1]] for g in ids]),
           "edge_index": torch.cat([edge_index[:, edge_ptr[g]:edge_ptr[g + 1]] - node_ptr[g] + ptr[k] for k, g in enumerate(ids)], dim=1),
           "batch": torch.repeat_interleave(torch.arange(len(ids)), sizes), "ptr": ptr}
    if edge_attr is not None:
        out["edge_attr"] = torch.cat([edge_attr[edge_ptr[g]:edge_ptr[g + 1]] for g in ids])
    if y is not None:
        out["y"] = torch.cat([y[g:g + 1] for g in ids])
    return out


def _graphs(seed, sizes, edges_of, x_of, edge_attr_of=None, y_of=None):
    """flat CPU arrays of a synthetic dataset: ``edges_of(n, g)`` edges per graph with random endpoints inside the graph"""
    g = torch.Generator().manual_seed(seed)
    sizes = torch.as_tensor(sizes, dtype=torch.int64)
    esizes = torch.tensor([edges_of(int(n), k) if int(n) else 0 for k, n in enumerate(sizes)], dtype=torch.int64)
    node_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)])
    edge_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(esizes, 0)])
    N, E, G = int(node_ptr[-1]), int(edge_ptr[-1]), sizes.numel()
    lo, span = torch.repeat_interleave(node_ptr[:-1], esizes), torch.repeat_interleave(sizes, esizes)
    ei = torch.stack([lo + (torch.rand(E, generator=g) * span).long().clamp(max=span - 1) if E else lo,
                      lo + (torch.rand(E, generator=g) * span).long().clamp(max=span - 1) if E else lo])
    return SimpleNamespace(x=x_of(N, g), edge_index=ei, node_ptr=node_ptr, edge_ptr=edge_ptr,
                           edge_attr=None if edge_attr_of is None else edge_attr_of(E, g), y=None if y_of is None else y_of(G, g), G=G)


def _zinc(G=2000, seed=1):
    sizes = torch.randint(18, 29, (G,), generator=torch.Generator().manual_seed(seed))
    return _graphs(seed, sizes, lambda n, k: 2 * n + 4, lambda N, g: torch.randint(0, 21, (N, 1), generator=g),
                   lambda E, g: torch.randint(0, 4, (E,), generator=g), lambda G_, g: torch.randn(G_, generator=g))


def _tu(G=300, seed=2):
    sizes = torch.randint(1, 601, (G,), generator=torch.Generator().manual_seed(seed))
    return _graphs(seed, sizes, lambda n, k: 2 * n, lambda N, g: torch.randn(N, 7, generator=g), None,
                   lambda G_, g: torch.randint(0, 2, (G_,), generator=g))


def _qm9(G=500, seed=3):
    sizes = torch.randint(3, 30, (G,), generator=torch.Generator().manual_seed(seed))
    return _graphs(seed, sizes, lambda n, k: 2 * n - 2, lambda N, g: torch.randn(N, 11, generator=g),
                   lambda E, g: torch.randn(E, 3, generator=g), lambda G_, g: torch.randn(G_, 12, generator=g))


def _edge_cases(seed=4):
    """graphs without edges, single-node graphs (with and without a self loop), an empty graph, rows of 12 bytes (x [N, 3] float32:
    the 4-byte path)"""
    sizes = [5, 1, 1, 7, 0, 3, 12, 1, 2, 9, 4, 1]
    edges = [8, 0, 1, 0, 0, 5, 30, 2, 0, 9, 0, 0]
    return _graphs(seed, sizes, lambda n, k: edges[k], lambda N, g: torch.randn(N, 3, generator=g),
                   lambda E, g: torch.randn(E, generator=g), lambda G_, g: torch.randn(G_, generator=g))


def _dataset(d, **kw):
    return kagnn_amd.DeviceGraphDataset(d.x, d.edge_index, d.node_ptr, edge_attr=d.edge_attr, y=d.y, device=DEV, **kw)


def _check_batch(d, b, ids, what):
    ref = collate(d.x, d.edge_index, d.node_ptr, d.edge_ptr, ids, d.edge_attr, d.y)
    assert b.num_graphs == len(ids) and b.num_nodes == ref["x"].size(0) and b.num_edges == ref["edge_index"].size(1), what
    for name, want in ref.items():
        got = getattr(b, name)
        assert got.dtype == want.dtype and got.shape == want.shape and got.device == torch.device(DEV), (what, name, got.shape, want.shape)
        assert torch.equal(got.cpu(), want), (what, name)
    if d.edge_attr is None:
        assert b.edge_attr is None
    # (2) the assembled index against the existing build from the batch's own edge_index -- or absent, exactly when that build
    # would not have taken the small-graph path
    n, e = b.num_nodes, b.num_edges
    if _lib.load().kagnn_csr_small_ok(e, n):
        gi = b.graph_index
        assert isinstance(gi, ops.GraphIndex) and gi._flags is None and gi.num_hub_seg == 0 and gi.num_hub_seg_t == 0, what
        old = ops.GraphIndex(b.edge_index, n)
        for name in ("rowptr", "col", "perm", "rowptr_t", "col_t", "perm_t"):
            assert getattr(gi, name).dtype == torch.int32 and torch.equal(getattr(gi, name), getattr(old, name)), (what, name)
    else:
        assert b.graph_index is None, what
    return ref


def _two_epochs(d, ds, batch_size, what, positions=None, **kw):
    gen, mirror = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
    loader = kagnn_amd.DeviceBatchLoader(ds, batch_size, shuffle=True, generator=gen, **kw)
    seen = 0
    for epoch in range(2):
        order = torch.randperm(len(ds), generator=mirror)          # what torch's RandomSampler draws for this generator ...
        torch.randperm(len(ds), generator=mirror)                  # ... and its unused second draw at the end of the epoch
        if positions is not None:
            order = positions[order]
        batches = list(loader)
        assert len(batches) == len(loader)
        for k, b in enumerate(batches):
            _check_batch(d, b, order[k * batch_size:(k + 1) * batch_size], f"{what} epoch {epoch} batch {k}")
            seen += b.num_graphs
    ops.flush_graph_checks()
    return seen


# ------------------------------------------------------------------------------------------------ (1) + (2)
def test_zinc_shaped_epochs_equal_the_restatement():
    d = _zinc()
    assert _two_epochs(d, _dataset(d), 256, "zinc") == 2 * d.G              # 7 full batches and a last short one per epoch


def test_tu_shaped_epochs_equal_the_restatement():
    """float32 x [N, 7] (28-byte rows: the 4-byte path), no edge_attr, int64 y; at 64 graphs of 1-600 nodes a batch has ~19k nodes /
    ~38k edges; at 256 it is past 65 536 edges, so no index is attached"""
    d = _tu()
    ds = _dataset(d)
    assert ds.num_classes == 2 and ds.num_features == 7 and ds.num_edge_features == 0
    _two_epochs(d, ds, 64, "tu/64")
    _two_epochs(d, ds, 256, "tu/256", drop_last=True)
    big = next(iter(kagnn_amd.DeviceBatchLoader(ds, 256)))
    assert big.num_edges > 65536 and big.graph_index is None


def test_qm9_shaped_epochs_equal_the_restatement():
    d = _qm9()
    ds = _dataset(d, edge_ptr=d.edge_ptr)
    assert ds.num_edge_features == 3 and ds.num_node_features == 11
    _two_epochs(d, ds, 128, "qm9")


@pytest.mark.parametrize("batch_size", [1, 5, 12])
def test_edge_case_graphs_and_batch_sizes(batch_size):
    d = _edge_cases()
    _two_epochs(d, _dataset(d), batch_size, f"edge cases / {batch_size}")


def test_a_batch_without_edges_has_no_index_and_the_model_still_runs():
    d = _edge_cases()
    ds = _dataset(d)[[1, 3, 8, 10]]                                # four graphs without a single edge
    (b,) = list(kagnn_amd.DeviceBatchLoader(ds, 4))
    _check_batch(d, b, [1, 3, 8, 10], "no edges")
    assert b.num_edges == 0 and b.graph_index is None
    torch.manual_seed(0)
    m = kagnn_amd.KAGIN(2, 3, 16, 2, 2, 4, 3, 0.0).to(DEV)
    out = m(b)
    assert out.shape == (4, 2) and bool(torch.isfinite(out).all())
    # ... and past 65 536 edges (the TU-shaped dataset at 256 graphs per batch): the model indexes edge_index itself, as today
    t = _tu()
    big = next(iter(kagnn_amd.DeviceBatchLoader(_dataset(t), 256)))
    assert big.graph_index is None
    m7 = kagnn_amd.KAGIN(2, 7, 16, 2, 2, 4, 3, 0.0).to(DEV)
    out = m7(big)
    ops.flush_graph_checks()
    assert out.shape == (256, 2) and bool(torch.isfinite(out).all())


def test_batch_of_one_and_batch_at_the_limit():
    B = _lib.BATCH_MAX_GRAPHS
    sizes = torch.randint(1, 6, (B + 50,), generator=torch.Generator().manual_seed(5))
    d = _graphs(5, sizes, lambda n, k: n + (k % 3), lambda N, g: torch.randn(N, 4, generator=g), None, lambda G_, g: torch.randn(G_, generator=g))
    ds = _dataset(d)
    order = torch.randperm(d.G, generator=torch.Generator().manual_seed(9))
    loader = kagnn_amd.DeviceBatchLoader(ds, B)
    big, rest = list(loader.batches_of(order))
    _check_batch(d, big, order[:B], "B at the limit")
    _check_batch(d, rest, order[B:], "the short batch after it")
    (one,) = list(kagnn_amd.DeviceBatchLoader(ds[[17]], 1))
    _check_batch(d, one, [17], "B = 1")
    assert one.to(DEV) is one and one.to("cuda") is one
    with pytest.raises(RuntimeError):
        one.to("cpu")
    ops.flush_graph_checks()


def test_subset_views_and_repeated_ids():
    d = _zinc(G=400, seed=11)
    ds = _dataset(d)
    positions = torch.randperm(400, generator=torch.Generator().manual_seed(2))[:150]
    sub = ds[positions]
    assert len(sub) == 150 and sub.storage is ds.storage
    _two_epochs(d, sub, 64, "subset", positions=positions)
    subsub = sub[10:60:3]
    _two_epochs(d, subsub, 8, "subset of a subset", positions=positions[10:60:3])
    ids = torch.tensor([5, 5, 5, 399, 0, 5, 0, 399, 399, 7])
    batches = list(kagnn_amd.DeviceBatchLoader(ds, 4).batches_of(ids))
    for k, b in enumerate(batches):
        _check_batch(d, b, ids[4 * k:4 * k + 4], f"repeated ids, batch {k}")
    ops.flush_graph_checks()


def test_unaligned_storage_bases():
    """x / edge_attr / y whose storage starts 4 bytes into an allocation: the 16- and 8-byte paths are not available"""
    d = _qm9(G=60, seed=13)
    ds = _dataset(d)
    st = ds.storage

    def shifted(t):
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 8 == 4
        return v
    st.x, st.edge_attr, st.y = shifted(st.x), shifted(st.edge_attr), shifted(st.y)
    _two_epochs(d, ds, 16, "unaligned bases")
    # and aligned bases with 16-byte rows (x [N, 4] float32) / 8-byte rows (int64 targets): the wide paths
    d4 = _graphs(14, [3, 9, 1, 6, 2], lambda n, k: 2 * n, lambda N, g: torch.randn(N, 4, generator=g),
                 lambda E, g: torch.randint(0, 9, (E, 2), generator=g), lambda G_, g: torch.randint(0, 5, (G_,), generator=g))
    _two_epochs(d4, _dataset(d4), 3, "16-byte rows")


def test_from_graphs_builds_the_same_dataset():
    d = _zinc(G=40, seed=17)
    graphs = [SimpleNamespace(x=d.x[d.node_ptr[g]:d.node_ptr[g + 1]], edge_index=d.edge_index[:, d.edge_ptr[g]:d.edge_ptr[g + 1]] - d.node_ptr[g],
                              edge_attr=d.edge_attr[d.edge_ptr[g]:d.edge_ptr[g + 1]], y=d.y[g:g + 1]) for g in range(d.G)]
    ds = kagnn_amd.DeviceGraphDataset.from_graphs(graphs, device=DEV)
    assert len(ds) == 40
    _two_epochs(d, ds, 16, "from_graphs")
    with pytest.raises(ValueError, match="two different graphs"):
        bad = d.edge_index.clone()
        bad[1, 0] = d.node_ptr[5]
        kagnn_amd.DeviceGraphDataset(d.x, bad, d.node_ptr, device=DEV)


# ------------------------------------------------------------------------------------------------ (3) the models
def _restated(d, ids):
    ref = collate(d.x, d.edge_index, d.node_ptr, d.edge_ptr, ids, d.edge_attr, d.y)
    return SimpleNamespace(num_graphs=len(ids), **{k: v.to(DEV) for k, v in ref.items()})


def _config4_model():
    torch.manual_seed(0)
    m = kagnn_amd.KAGINRegression(1, 1, 4, 64, 2, 4, 3, 1, 0.0, True)
    m.atom_encoder = kagnn_amd.graph_models.AtomEncoder(64, [21])
    m.bond_encoder.bond_embedding_list = torch.nn.ModuleList([torch.nn.Embedding(4, 64)])
    return m.to(DEV)


def _out_and_grads(m, batch, loss):
    m.zero_grad(set_to_none=True)
    out = m(batch)
    loss(out, batch).backward()
    return [out.detach().clone()] + [p.grad.detach().clone() for p in m.parameters() if p.grad is not None]


class _Counter:
    def __init__(self, monkeypatch):
        self.calls, real = 0, ops.graph_index

        def counted(*a, **kw):
            self.calls += 1
            return real(*a, **kw)
        monkeypatch.setattr(ops, "graph_index", counted)


def test_models_give_the_same_bits_on_a_loader_batch_and_on_the_restatement(monkeypatch):
    count = _Counter(monkeypatch)
    d = _zinc(G=600, seed=21)
    b = next(iter(kagnn_amd.DeviceBatchLoader(_dataset(d), 256)))
    m = _config4_model().train()
    l1 = lambda out, bt: ops.l1_loss(out.squeeze(), bt.y.squeeze())
    got = _out_and_grads(m, b, l1)
    assert count.calls == 0                                        # the loader's batch brought its index along
    want = _out_and_grads(m, _restated(d, range(256)), l1)
    assert count.calls == 1
    assert len(got) == len(want) > 10 and all(torch.equal(a, c) for a, c in zip(got, want))

    t = _tu(G=120, seed=22)
    bt = next(iter(kagnn_amd.DeviceBatchLoader(_dataset(t), 48)))
    torch.manual_seed(1)
    clf = kagnn_amd.KAGIN(3, 7, 32, 2, 2, 4, 3, 0.0).to(DEV).train()
    nll = lambda out, bt_: torch.nn.functional.nll_loss(out, bt_.y)
    count.calls = 0
    got = _out_and_grads(clf, bt, nll)
    assert count.calls == 0 and bt.graph_index is not None
    want = _out_and_grads(clf, _restated(t, range(48)), nll)
    assert count.calls == 1 and all(torch.equal(a, c) for a, c in zip(got, want))
    ops.flush_graph_checks()


def test_training_over_the_loader_equals_training_over_restated_batches(monkeypatch):
    d = _zinc(G=700, seed=23)
    loader = kagnn_amd.DeviceBatchLoader(_dataset(d), 256)          # shuffle=False: 256 + 256 + 188 graphs, in dataset order
    restated = [_restated(d, range(s, min(s + 256, 700))) for s in range(0, 700, 256)]
    ma = _config4_model()
    mb = copy.deepcopy(ma)             # (a copy, not a second construction: KANLinear's initial least-squares fit differs in the last bits from call to call)
    count = _Counter(monkeypatch)
    _t, losses_a = harness.train_graph_batches(ma, loader, nb_epochs=2)
    assert count.calls == 0                                        # never a per-batch CSR build on the loader path
    _t, losses_b = harness.train_graph_batches(mb, restated, nb_epochs=2)
    assert count.calls == 2 * 3
    assert losses_a == losses_b and all(l == l for l in losses_a)
    for (name, pa), pb in zip(ma.named_parameters(), mb.parameters()):
        assert torch.equal(pa, pb), name
    for ba, bb in zip(ma.buffers(), mb.buffers()):
        assert torch.equal(ba, bb)
    ea, eb = harness.evaluate_graph_batches(ma, loader), harness.evaluate_graph_batches(mb, restated)
    assert ea == eb and ea == ea and not ma.training


# ------------------------------------------------------------------------------------------------ (4) bad input
def _guarded_batches(monkeypatch, loader, ids):
    guarded = _GuardedEmpty()
    monkeypatch.setattr(torch, "empty", guarded)
    out = list(loader.batches_of(ids))
    n = guarded.check("kagnn_batch_assemble")
    monkeypatch.undo()
    assert n >= 6
    return out


def test_a_graph_id_outside_the_dataset_is_reported_not_executed(monkeypatch):
    d = _zinc(G=50, seed=31)
    loader = kagnn_amd.DeviceBatchLoader(_dataset(d), 8)
    ops.flush_graph_checks()
    for bad in (50, 10 ** 12, -1):
        ids = torch.tensor([3, 4, bad, 7, 1, 0, 2, 9, 11, 12])
        _guarded_batches(monkeypatch, loader, ids)                 # no write outside the outputs ...
        with pytest.raises(RuntimeError, match="kagnn_batch_assemble"):
            ops.flush_graph_checks()                               # ... and the flag arrives with the deferred checks
    good = _guarded_batches(monkeypatch, loader, torch.arange(10))
    ops.flush_graph_checks()
    _check_batch(d, good[1], [8, 9], "after the bad ones")


@pytest.mark.parametrize("dn,de", [(3, 0), (-3, 0), (0, 5), (0, -5), (40, -9)])
def test_wrong_totals_are_reported_not_executed(monkeypatch, dn, de):
    d = _zinc(G=50, seed=32)
    loader = kagnn_amd.DeviceBatchLoader(_dataset(d), 8)
    ops.flush_graph_checks()
    real = data.batch_plan

    def wrong(*a, **kw):
        starts, sizes, nodes, edges = real(*a, **kw)
        return starts, sizes, [n + dn for n in nodes], [e + de for e in edges]
    monkeypatch.setattr(data, "batch_plan", wrong)
    guarded = _GuardedEmpty()
    monkeypatch.setattr(torch, "empty", guarded)
    batches = list(loader.batches_of(torch.arange(16)))
    m = kagnn_amd.KAGIN(2, 1, 16, 2, 2, 4, 3, 0.0).to(DEV)
    for b in batches:                                              # every index written is inside the batch: the kernels that consume it
        b.x = b.x.float()                                          # before the flags are read stay inside their buffers too
        m(b)
    assert guarded.check("wrong totals") >= 6
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match="kagnn_batch_assemble"):
        ops.flush_graph_checks()


# ------------------------------------------------------------------------------------------------ (5) poison independence
def test_the_assembled_batch_does_not_depend_on_the_heap():
    d = _edge_cases()
    ds = _dataset(d)
    z = _zinc(G=300, seed=41)
    dz = _dataset(z)

    def run():
        out = []
        for loader in (kagnn_amd.DeviceBatchLoader(ds, 5), kagnn_amd.DeviceBatchLoader(dz, 256)):
            for b in loader:
                out += [b.x, b.edge_index, b.edge_attr, b.y, b.batch, b.ptr]
                if b.graph_index is not None:
                    gi = b.graph_index
                    out += [gi.rowptr, gi.col, gi.perm, gi.rowptr_t, gi.col_t, gi.perm_t]
        ops.flush_graph_checks()
        return out
    _under_every_pattern(None, run, "kagnn_batch_assemble")
