"""The graph-level primitives under every fused call -- neighbour aggregation (``kagnn_aggregate_sum``, ``_add``, ``_bf16``), the
GINE message, segment pooling / broadcast and the embedding tables -- against a plain fp64 restatement (``oracle/kan_oracle.py``),
one case per kernel instantiation and per edge of the dispatch in ``csrc/aggregate.hip`` / ``csrc/aggregate_bf16.hip``.

The aggregation tests share ONE hand-built graph (``boundary_graph``) whose in-degrees sit on the boundaries the kernels branch on:
the unroll-by-4 and edge-slot tails, ``HUB_THRESHOLD`` -1 / +0 / +1, and hubs of more than 4, 8, 16, 32 and 64 segments (the
round-robin loop of the merge kernels takes a second trip once a row has more segments than ``256 / LPR`` lane groups).  Explicit
edge weights, distinct in / out scales, a bias, explicit self loops (also inside hub rows) and duplicate edges are part of every
width's case.  Tolerances are the neighbouring tests': ``helpers.TOL`` for fp32, 2e-6 for the bf16 gather with fp32 sums, one bf16
rounding for bf16 output, 1e-5 (max norm) for embedding-table gradients."""
import functools
import os
import re

import pytest
import torch

import kagnn_amd
from kagnn_amd import graph_ops, library, ops
from oracle import kan_oracle as orc
from helpers import CONTRACT, TOL, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS32 = float(torch.finfo(torch.float32).eps)
NUM_NODES = 3000
ISOLATED = 8                      # the last nodes: no edge in either direction


# ------------------------------------------------------------------ 1. the boundary graph
def hub_segment_length(threshold):
    """the segment length ``csr_hub_kernel`` cuts hub rows into, read from csr.hip (today ``max(T / 4, 64)``)"""
    with open(os.path.join(os.path.dirname(kagnn_amd.__file__), "csrc", "csr.hip")) as f:
        m = re.search(r"const int L = max\(T / (\d+), (\d+)\);", f.read())
    assert m, "csr.hip no longer states the hub segment length in the form this test reads"
    return max(threshold // int(m.group(1)), int(m.group(2)))


def prescribed_degrees():
    """(in-degrees pinned by the test, of which hubs): unroll-by-4 tails of the row kernels; the edge-slot tails of
    agg_rows_ep_kernel (EP = 16, 8, 4 slots: degree mod 2 EP decides whether the ``if (e < t)`` tail runs); the hub threshold;
    hubs of 5, 10, 18, 34 and 66 segments -- one an exact multiple of the segment length, one that plus 1"""
    T = ops.HUB_THRESHOLD
    L = hub_segment_length(T)
    tails = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17]
    slots = [11, 12, 13, 23, 24, 25, 31, 32, 33, 47, 48, 49, 63, 64, 65]
    hubs = [5 * L, 9 * L + 1, 17 * L + 37, 33 * L + 11, 65 * L + 3]
    return sorted(set(d for d in tails + slots + [T - 1, T] if d <= T)) + [T + 1] + hubs, [T + 1] + hubs


def boundary_graph(seed=20):
    """-> (edge_index [2, E] int64 on the host, {node: pinned in-degree}, the node whose reversed edges make it a hub of the
    transposed structure).  Sources are drawn with replacement (duplicate edges: a 2000-edge row over 3000 nodes repeats many);
    explicit self loops sit in the middle of some rows, hub rows included; the pinned degree-0 node is a source only; the last
    ``ISOLATED`` nodes have no edge at all; the edge list is shuffled, so ``perm`` and ``perm_t`` are far from the identity."""
    gen = torch.Generator().manual_seed(seed)
    degs, hubs = prescribed_degrees()
    n = NUM_NODES
    live = n - ISOLATED
    place = torch.randperm(live, generator=gen)[:len(degs)].tolist()
    special = dict(zip(place, degs))
    filler = torch.tensor([i for i in range(live) if i not in special])
    deg = torch.randint(0, 9, (n,), generator=gen)
    deg[live:] = 0
    for node, d in special.items():
        deg[node] = d
    T = ops.HUB_THRESHOLD
    L = hub_segment_length(T)
    with_loop = {3, 8, T, T + 1, 5 * L, 33 * L + 11}
    reversed_hub = next(node for node, d in special.items() if d == 33 * L + 11)
    source_only = next(node for node, d in special.items() if d == 0)
    src, dst = [], []
    for i in range(live):
        d = int(deg[i])
        if d == 0:
            continue
        if i == reversed_hub:            # (its sources gain an in-edge below: fillers only, the pinned degrees stay exact)
            s = filler[torch.randint(0, filler.numel(), (d,), generator=gen)]
        else:
            s = torch.randint(0, live, (d,), generator=gen)
        if i in special and special[i] in with_loop:
            s[d // 2] = i
            if i == reversed_hub:
                s[1] = i                 # (a second, duplicate loop)
        if i in special and special[i] == 9 * L + 1:
            s[0] = source_only
        src.append(s)
        dst.append(torch.full((d,), i, dtype=torch.int64))
    src, dst = torch.cat(src), torch.cat(dst)
    back = (dst == reversed_hub) & (src != reversed_hub)
    src, dst = torch.cat([src, dst[back]]), torch.cat([dst, src[back]])
    order = torch.randperm(src.numel(), generator=gen)
    return torch.stack([src[order], dst[order]]).contiguous(), special, reversed_hub


@functools.lru_cache(maxsize=None)
def _boundary():
    ei, special, reversed_hub = boundary_graph()
    small = ops._SMALL_CSR
    ops._SMALL_CSR = False              # (the one-launch CSR build of small graphs makes no hub segments)
    try:
        g = ops.GraphIndex(ei.to(DEV), NUM_NODES)
    finally:
        ops._SMALL_CSR = small
    return ei, g, special, reversed_hub


def _hub_rows(ei, transposed=False):
    return torch.bincount(ei[0 if transposed else 1], minlength=NUM_NODES) > ops.HUB_THRESHOLD


def test_boundary_graph_holds_every_degree_class_and_both_structures_have_hubs():
    ei, g, special, reversed_hub = _boundary()
    T = ops.HUB_THRESHOLD
    L = hub_segment_length(T)
    assert 2500 <= NUM_NODES <= 5000 and ei.size(1) <= 65536
    indeg = torch.bincount(ei[1], minlength=NUM_NODES)
    outdeg = torch.bincount(ei[0], minlength=NUM_NODES)
    for node, d in special.items():
        assert int(indeg[node]) == d, (node, d, int(indeg[node]))
    assert {T - 1, T, T + 1} <= set(special.values())
    assert int(((indeg == 0) & (outdeg > 0)).sum()) >= 3 and int(((indeg == 0) & (outdeg == 0)).sum()) >= ISOLATED
    loops = ei[0] == ei[1]
    assert int(loops.sum()) >= 6 and bool((indeg[ei[1][loops]] > T).any()) and int(outdeg[reversed_hub]) > 32 * L
    pairs = ei[0] * NUM_NODES + ei[1]
    assert pairs.unique().numel() < pairs.numel()                  # duplicate edges
    assert g.num_hub_seg > 0 and g.num_hub_seg_t > 0
    for seg, nseg, degs in ((g.hub_seg, g.num_hub_seg, indeg), (g.hub_seg_t, g.num_hub_seg_t, outdeg)):
        seg = seg[:3 * nseg].view(-1, 3).cpu().long()
        count = torch.bincount(seg[:, 0], minlength=NUM_NODES)
        assert torch.equal(count, torch.where(degs > T, (degs + L - 1) // L, torch.zeros_like(degs)))
        assert int(count.max()) > 32 and int((seg[:, 2] - seg[:, 1]).max()) == L
    seg = g.hub_seg[:3 * g.num_hub_seg].view(-1, 3).cpu().long()
    last = {int(r): int(t - s) for r, s, t in seg.tolist()}                     # (segments are listed in edge order: the last one of each row stays)
    assert {L, 1} <= set(last.values()), last                                    # an exact multiple of the segment length, and that + 1
    per_row = sorted(set(((indeg[indeg > T] + L - 1) // L).tolist()))
    assert [any(lo < c <= hi for c in per_row) for lo, hi in ((4, 8), (8, 16), (16, 32), (32, 64), (64, 128))] == [True] * 5, per_row
    assert torch.equal(g.rowptr.cpu().long(), torch.cat([torch.zeros(1, dtype=torch.int64), indeg.cumsum(0)]))


# ------------------------------------------------------------------ the aggregation, restated in fp64
def ref_aggregate(x, ei, w, self_scale, in_s, out_s, bias, skip):
    """out_i = out_s[i] * (self_scale * in_s[i] * x_i + sum_{e: j -> i} w_e * in_s[j] * x_j) + bias; ``skip`` drops the loops"""
    src, dst = ei[0], ei[1]
    we = torch.ones(src.numel(), dtype=torch.float64) if w is None else w.double()
    if in_s is not None:
        we = we * in_s.double()[src]
    if skip:
        we = we * (src != dst).double()
    sw = torch.full((x.size(0), 1), float(self_scale), dtype=torch.float64)
    if in_s is not None:
        sw = sw * in_s.double().view(-1, 1)
    out = orc.sum_aggregate(x, ei, x.size(0), we) + sw * x
    if out_s is not None:
        out = out_s.double().view(-1, 1) * out
    return out if bias is None else out + bias.double()


def _ref(x, ei, form):
    self_scale, w, in_s, out_s, bias, skip = form
    return ref_aggregate(x, ei, w, self_scale, in_s, out_s, bias, skip)


def abs_terms(x, ei, form):
    """sum of the magnitudes of the terms of every output element (the scale of an fp32 sum's rounding noise)"""
    self_scale, w, in_s, out_s, bias, skip = form
    a = lambda t: None if t is None else t.abs()
    return ref_aggregate(x.abs(), ei, a(w), abs(self_scale), a(in_s), a(out_s), a(bias), skip)


def close_by_class(got, want, hubs, tol, what):
    """ordinary rows and hub rows each against their OWN magnitude: a hub row is tens of times larger than a row of three edges,
    whose error one max norm over the whole matrix would hide"""
    got = got.detach().double().cpu()
    assert_close(got[~hubs], want[~hubs], tol, what=what + ", rows")
    assert_close(got[hubs], want[hubs], tol, what=what + ", hub rows")


def _forms(n, f, e, gen):
    """the five forms of the issue: name -> (self_scale, edge weights, in_scale, out_scale, bias, skip_self_loops)"""
    w = torch.rand(e, generator=gen) + 0.1
    in_s, out_s = torch.rand(n, generator=gen) + 0.5, torch.rand(n, generator=gen) + 0.5       # (distinct: a swapped scale shows)
    bias = torch.randn(f, generator=gen)
    return {"a": (1.5, None, None, None, None, False), "b": (1.0, w, None, None, None, False),
            "c": (1.25, w, in_s, out_s, bias, False), "d": (1.25, w, in_s, out_s, bias, True)}


def _dev(t):
    return None if t is None else t.to(DEV)


def _raw(x, g, transposed, form, out_dtype=torch.float32, addend=None):
    """ops._aggregate_raw wants the weights in the order of the structure it walks: ``perm`` forward, ``perm_t`` transposed"""
    self_scale, w, in_s, out_s, bias, skip = form
    if w is not None:
        w = w.to(DEV)[(g.perm_t if transposed else g.perm).long()].contiguous()
    return ops._aggregate_raw(x, g, transposed, self_scale, w, _dev(in_s), _dev(out_s), _dev(bias), skip, out_dtype=out_dtype, addend=addend)


# ------------------------------------------------------------------ 2. fp32 aggregation
# aggregate_sum (aggregate.hip): vec4_ok -- F % 4 == 0, F <= 256, rows 16-byte aligned with a leading dimension % 4 == 0 -- else
# agg_rows_generic_kernel (no hub kernels).  Within vec4: F <= 4 / 8 / 16 -> agg_rows_ep_kernel<1 / 2 / 4> (EP = 16 / 8 / 4 edge
# slots), F <= 32 / 64 / 128 / 256 -> agg_rows_v4_kernel<8 / 16 / 32 / 64>; hub rows -> agg_hub_v4_kernel<LPR> and
# agg_hub_merge_kernel<LPR> with the same LPR (G = 256 / LPR lane groups: 256, 128, 64, 32, 16, 8, 4).
FP32_CASES = [(4, False), (8, False), (12, False), (16, False),      # EP 16, 8, 4, 4 (12: the last column group of LPR = 4 idle)
              (20, False), (32, False),                              # LPR 8
              (36, False), (64, False),                              # LPR 16
              (68, False), (128, False),                             # LPR 32
              (132, False), (256, False),                            # LPR 64
              (7, False), (260, False), (300, False),                # generic: unaligned width, wider than 256 (two column blocks)
              (64, True)]                                            # generic at F = 64: a column slice, leading dimension 67


@pytest.mark.parametrize("f,sliced", FP32_CASES, ids=[f"F{f}{'-sliced' if s else ''}" for f, s in FP32_CASES])
def test_fp32_aggregation_matches_fp64_in_every_form_and_direction(f, sliced):
    ei, g, _, _ = _boundary()
    n, e = NUM_NODES, ei.size(1)
    gen = torch.Generator().manual_seed(100 + f + sliced)
    if sliced:
        wide = torch.randn(n, f + 3, generator=gen)
        x, xd = wide[:, 1:f + 1], wide.to(DEV)[:, 1:f + 1]                      # (ld = F + 3, rows 4 bytes off a 16-byte boundary)
        assert xd.stride(0) % 4 != 0 and xd.data_ptr() % 16 != 0
    else:
        x = torch.randn(n, f, generator=gen)
        xd = x.to(DEV)
    x64 = x.double()
    gout = torch.randn(n, f, generator=gen)
    add = torch.randn(n, f + 4, generator=gen).to(DEV)[:, :f]                  # (a strided addend)
    forms = _forms(n, f, e, gen)
    timer = ops.EntryPointTimer()
    ops.set_timer(timer)
    try:
        for name, form in forms.items():
            self_scale, w, in_s, out_s, bias, skip = form
            for transposed in (False, True):
                edges = ei.flip(0) if transposed else ei
                want = _ref(x64, edges, form)
                got = _raw(xd, g, transposed, form)
                close_by_class(got, want, _hub_rows(ei, transposed), TOL, f"fp32 aggregation ({name}) {'transposed' if transposed else 'forward'}")
                assert torch.equal(got, _raw(xd, g, transposed, form))             # hub rows are reproducible run to run
                if name == "c":                                                     # form (e): the addend rides in the epilogue
                    assert torch.equal(_raw(xd, g, transposed, form, addend=add), got + add)
            # through autograd: ops.aggregate_sum permutes the weights itself (perm forward, perm_t backward) and swaps the scales
            xr = x64.clone().requires_grad_(True)
            br = None if bias is None else bias.double().requires_grad_(True)
            ref = ref_aggregate(xr, ei, w, self_scale, in_s, out_s, br, skip)
            ref.backward(gout.double())
            xg = xd.detach().requires_grad_(True)
            bg = None if bias is None else bias.to(DEV).requires_grad_(True)
            out = ops.aggregate_sum(xg, g, self_scale, _dev(w), _dev(in_s), _dev(out_s), bg, skip)
            out.backward(gout.to(DEV))
            close_by_class(out, ref.detach(), _hub_rows(ei), TOL, f"fp32 aggregate_sum ({name}) output")
            close_by_class(xg.grad, xr.grad, _hub_rows(ei, True), TOL, f"fp32 aggregate_sum ({name}) x.grad")
            if bias is not None:
                assert_close(bg.grad, br.grad, TOL, what=f"fp32 aggregate_sum ({name}) bias.grad", noise=EPS32 * float(gout.abs().sum(0).max()))
            xg2 = xd.detach().requires_grad_(True)
            ops.aggregate_sum(xg2, g, self_scale, _dev(w), _dev(in_s), _dev(out_s), _dev(bias), skip).backward(gout.to(DEV))
            assert torch.equal(xg2.grad, xg.grad)
    finally:
        ops.set_timer(None)
    names = {r[0] for r in timer.records}
    assert {"kagnn_aggregate_sum", "kagnn_aggregate_sum_add"} <= names and "kagnn_aggregate_sum_bf16" not in names, names


# ------------------------------------------------------------------ 3. bf16 gather
# aggregate_sum_bf16 (aggregate_bf16.hip run16): F % 8 == 0, F <= 512, 8 columns per lane; F <= 8 / 16 / 32 / 64 / 128 / 256 ->
# agg16_rows_kernel / agg16_hub_kernel / agg16_hub_merge_kernel<1 / 2 / 4 / 8 / 16 / 32>, wider (264..512) -> <64>.
BF16_WIDTHS = [8, 16, 24, 32, 40, 64, 72, 128, 136, 256, 264, 384, 512]


def one_bf16_rounding(got16, want, noise, what):
    """a bf16 result is the fp32 sum rounded once: 2^-8 of the value itself, on top of the fp32 sum's own rounding noise
    ``eps32 * sum|terms|`` (computed in fp64 from the inputs of that element) where the terms cancel"""
    assert got16.dtype == torch.bfloat16
    err = (got16.double().cpu() - want).abs()
    bound = want.abs() * 2.0 ** -8 + noise
    worst = float((err / bound.clamp_min(1e-300)).max())
    assert worst <= 1.0, f"{what}: {worst:.3f} of one bf16 rounding"


@pytest.mark.parametrize("f", BF16_WIDTHS)
def test_bf16_gather_matches_fp64_on_the_rounded_rows(f):
    ei, g, _, _ = _boundary()
    n, e = NUM_NODES, ei.size(1)
    gen = torch.Generator().manual_seed(200 + f)
    xb = torch.randn(n, f, generator=gen).to(torch.bfloat16)
    x64, xd = xb.double(), xb.to(DEV)
    forms = _forms(n, f, e, gen)
    timer = ops.EntryPointTimer()
    ops.set_timer(timer)
    try:
        for name, form in forms.items():
            for transposed in ((False, True) if name in "ad" else (False,)):
                edges = ei.flip(0) if transposed else ei
                where = f"({name}) {'transposed' if transposed else 'forward'}"
                want = _ref(x64, edges, form)
                got = _raw(xd, g, transposed, form)
                assert got.dtype == torch.float32
                close_by_class(got, want, _hub_rows(ei, transposed), 2e-6, f"bf16 gather, fp32 sums {where}")
                assert torch.equal(got, _raw(xd, g, transposed, form))
                if name in "ad":
                    noise = EPS32 * abs_terms(x64, edges, form)
                    got16 = _raw(xd, g, transposed, form, out_dtype=torch.bfloat16)
                    one_bf16_rounding(got16, want, noise, f"bf16 gather, bf16 output {where} F={f}")
                    assert torch.equal(got16, _raw(xd, g, transposed, form, out_dtype=torch.bfloat16))
    finally:
        ops.set_timer(None)
    names = {r[0] for r in timer.records}
    assert "kagnn_aggregate_sum_bf16" in names and not names & {"kagnn_aggregate_sum", "kagnn_aggregate_sum_add"}, names


def test_bf16_rows_wider_than_512_take_the_fp32_kernels_and_still_match():
    ei, g, _, _ = _boundary()
    f = 520
    assert not ops._bf16_gather_width_ok(f) and ops._bf16_gather_width_ok(512)
    gen = torch.Generator().manual_seed(520)
    xb = torch.randn(NUM_NODES, f, generator=gen).to(torch.bfloat16)
    forms = _forms(NUM_NODES, f, ei.size(1), gen)
    timer = ops.EntryPointTimer()
    ops.set_timer(timer)
    try:
        for name in "ad":
            want = _ref(xb.double(), ei, forms[name])
            got = _raw(xb.to(DEV), g, False, forms[name])
            close_by_class(got, want, _hub_rows(ei), 2e-6, f"bf16 rows through the fp32 kernels ({name})")
            got16 = _raw(xb.to(DEV), g, False, forms[name], out_dtype=torch.bfloat16)
            noise = EPS32 * abs_terms(xb.double(), ei, forms[name])
            one_bf16_rounding(got16, want, noise, f"bf16 rows through the fp32 kernels, bf16 output ({name})")
    finally:
        ops.set_timer(None)
    names = {r[0] for r in timer.records}
    assert "kagnn_aggregate_sum" in names and "kagnn_aggregate_sum_bf16" not in names, names


# ------------------------------------------------------------------ a hub of more segments than ANY kernel has lane groups
@functools.lru_cache(maxsize=None)
def _deep_hub():
    """one row of 257 full segments + 5 edges (258 segments) among 600 nodes: the merge kernels' round-robin loop takes a second trip even with
    G = 256 lane groups (LPR = 1: fp32 F <= 4, bf16 F <= 8) -- the boundary graph stops at 66 segments"""
    L = hub_segment_length(ops.HUB_THRESHOLD)
    gen = torch.Generator().manual_seed(7)
    n, hub = 600, 311
    d = 257 * L + 5
    src = torch.cat([torch.randint(0, n, (d,), generator=gen), torch.randint(0, n, (1500,), generator=gen)])
    dst = torch.cat([torch.full((d,), hub), torch.randint(0, n, (1500,), generator=gen)])
    src[d // 3] = hub
    ei = torch.stack([src, dst])[:, torch.randperm(src.numel(), generator=gen)].contiguous()
    small = ops._SMALL_CSR
    ops._SMALL_CSR = False
    try:
        g = ops.GraphIndex(ei.to(DEV), n)
    finally:
        ops._SMALL_CSR = small
    return ei, g, n


@pytest.mark.parametrize("f", [4, 8, 16, 32])
def test_hub_of_more_segments_than_lane_groups_at_the_narrow_widths(f):
    ei, g, n = _deep_hub()
    seg = g.hub_seg[:3 * g.num_hub_seg].view(-1, 3).cpu().long()
    assert int(torch.bincount(seg[:, 0]).max()) > 256
    hubs = torch.bincount(ei[1], minlength=n) > ops.HUB_THRESHOLD
    gen = torch.Generator().manual_seed(300 + f)
    forms = _forms(n, f, ei.size(1), gen)
    x = torch.randn(n, f, generator=gen)
    xb = x.to(torch.bfloat16)
    for name in "ad":
        form = forms[name]
        got = _raw(x.to(DEV), g, False, form)
        want = _ref(x.double(), ei, form)
        for rows, which in ((~hubs, "rows"), (hubs, "hub rows")):
            assert_close(got[rows.to(DEV)], want[rows], TOL, what=f"fp32 aggregation, 258-segment hub ({name}), {which}")
        assert torch.equal(got, _raw(x.to(DEV), g, False, form))
        if f % 8 == 0:
            got = _raw(xb.to(DEV), g, False, form)
            want = _ref(xb.double(), ei, form)
            for rows, which in ((~hubs, "rows"), (hubs, "hub rows")):
                assert_close(got[rows.to(DEV)], want[rows], 2e-6, what=f"bf16 gather, 258-segment hub ({name}), {which}")
            assert torch.equal(got, _raw(xb.to(DEV), g, False, form))


# ------------------------------------------------------------------ 4. the GINE message
@functools.lru_cache(maxsize=None)
def _components():
    """about 40 disjoint small components, as a mini-batch of molecules is: sizes 1..30 (single nodes without an edge among them),
    random edges inside each component, duplicates and loops included; indexed by the one-launch CSR build"""
    gen = torch.Generator().manual_seed(11)
    sizes = torch.cat([torch.tensor([1, 1, 2, 30]), torch.randint(1, 31, (36,), generator=gen)])
    off = torch.cumsum(sizes, 0) - sizes
    src, dst = [], []
    for b in range(sizes.numel()):
        k = int(sizes[b])
        if k == 1:
            continue
        src.append(torch.randint(0, k, (2 * k,), generator=gen) + off[b])
        dst.append(torch.randint(0, k, (2 * k,), generator=gen) + off[b])
    ei = torch.stack([torch.cat(src), torch.cat(dst)]).contiguous()
    n = int(sizes.sum())
    g = ops.GraphIndex(ei.to(DEV), n)
    assert g.num_hub_seg == 0
    return ei, g, n


def _gine_inputs(ei, n, f, gen):
    """x, edge_attr with no x_j + e_ij within 1e-6 of zero: the ReLU mask is then the same in fp32 and in fp64 (a condition on
    the inputs, asserted on the fp64 side -- not a tolerance)"""
    x = torch.randn(n, f, generator=gen)
    ea = torch.randn(ei.size(1), f, generator=gen)
    near = (x[ei[0]] + ea).abs() < 1e-3
    ea = torch.where(near, ea + 0.25, ea)
    assert float((x.double()[ei[0]] + ea.double()).abs().min()) >= 1e-6
    return x, ea


def _sliced(t, yes, gen):
    """the same values as a column slice of a wider device matrix (row stride F + 3, first element off the allocation's start)"""
    if not yes:
        return t.to(DEV)
    wide = torch.randn(t.size(0), t.size(1) + 3, generator=gen)
    wide[:, 2:2 + t.size(1)] = t
    return wide.to(DEV)[:, 2:2 + t.size(1)]


GINE_WIDTHS = [1, 7, 16, 63, 64, 65, 130, 200]     # gine_*_kernel: a wave per row, lane = column; F > 64: the second trip of `f += 64`


@pytest.mark.parametrize("graph", ["boundary", "components"])
@pytest.mark.parametrize("f", GINE_WIDTHS)
def test_gine_message_forward_and_both_gradients_match_fp64(graph, f):
    if graph == "boundary":
        ei, g, _, _ = _boundary()
        n = NUM_NODES
    else:
        ei, g, n = _components()
    k = GINE_WIDTHS.index(f)
    sliced, self_scale = k % 2 == (graph == "boundary"), (1.0, 1.3)[(k // 2 + (graph == "boundary")) % 2]
    gen = torch.Generator().manual_seed(400 + f)
    x, ea = _gine_inputs(ei, n, f, gen)
    gout = torch.randn(n, f, generator=gen)
    xr, er = x.double().requires_grad_(True), ea.double().requires_grad_(True)
    ref = orc.gine_conv(xr, ei, er, lambda t: t, eps=self_scale - 1.0)
    ref.backward(gout.double())
    xd = _sliced(x, sliced, gen).detach().requires_grad_(True)
    ed = _sliced(ea, sliced, gen).detach().requires_grad_(True)
    gd = _sliced(gout, sliced, gen)
    assert (xd.stride(0) != f) == sliced and (gd.stride(0) != f) == sliced
    out = ops.aggregate_gine(xd, ed, g, self_scale)
    out.backward(gd)
    assert_close(out, ref.detach(), what=f"GINE message ({graph})")
    assert_close(xd.grad, xr.grad, what=f"GINE message x.grad ({graph})")
    assert_close(ed.grad, er.grad, what=f"GINE message edge_attr.grad ({graph})")
    isolated = (torch.bincount(ei[0], minlength=n) + torch.bincount(ei[1], minlength=n)) == 0
    assert bool(isolated.any())
    assert torch.equal(out.detach().cpu()[isolated], (torch.tensor(self_scale) * x)[isolated])
    # needs_input_grad[1] == False: no edge-attribute gradient is written (gea == nullptr), the same x.grad
    x2 = xd.detach().requires_grad_(True)
    e2 = ed.detach()
    ops.aggregate_gine(x2, e2, g, self_scale).backward(gd)
    assert e2.grad is None and torch.equal(x2.grad, xd.grad)


STACK_SEED, STACK_MARGIN = 6, 1e-4     # (the seed is chosen so that no pre-activation of either convolution is within 1e-4 of zero)


def _bn64(h, weight, bias, eps):
    mean, var = h.mean(0), h.var(0, unbiased=False)
    return (h - mean) / torch.sqrt(var + eps) * weight + bias


def test_gine_stack_adds_the_edge_attribute_gradients_of_its_convolutions():
    """``gea_accumulate``: inside kagnn_gine_kan_stack_bwd the second convolution to run its backward ADDS its edge-attribute
    gradient onto the first one's.  Two convolutions (GINE message -> 2-layer KAN -> training-mode BatchNorm1d) at hidden 16
    against the fp64 oracle of the same stack, whose autograd sums the two.  The KAN chains run in the split-precision mode and a
    batch norm follows each: ``helpers.CONTRACT`` (1e-4, the bound the graph-regression model tests hold these gradients to), max
    norm -- one convolution's share missing is an error of the order of the gradient itself.  Both convolutions' pre-activations
    stay clear of zero in fp64 (asserted), so the ReLU masks agree."""
    ei, g, n = _components()
    H, nl, nconv = 16, 2, 2
    gen = torch.Generator().manual_seed(15)
    x = torch.randn(n, H, generator=gen) * 0.5
    ea = torch.randn(ei.size(1), H, generator=gen) * 0.5
    ea = torch.where((x[ei[0]] + ea).abs() < 1e-3, ea + 0.25, ea)
    wgt = torch.randn(n, H, generator=gen)
    torch.manual_seed(STACK_SEED)
    convs = torch.nn.ModuleList(kagnn_amd.graph_models.GINEKANLayer(kagnn_amd.models.make_kan(H, H, H, nl, 4, 3)) for _ in range(nconv))
    bns = torch.nn.ModuleList(kagnn_amd.BatchNorm1d(H) for _ in range(nconv))
    for bn in bns:
        bn.weight.data.uniform_(0.5, 1.5); bn.bias.data.uniform_(-0.5, 0.5)
    # fp64
    xr, er = x.double().requires_grad_(True), ea.double().requires_grad_(True)
    h, margin = xr, float("inf")
    for conv, bn in zip(convs, bns):
        layers = [{k: v.detach().double() for k, v in l.state_dict().items()} for l in conv.nn.layers]
        margin = min(margin, float((h.detach()[ei[0]] + er.detach()).abs().min()))
        h = _bn64(orc.gine_conv(h, ei, er, lambda t: orc.kan_forward(t, layers, 3)), bn.weight.detach().double(), bn.bias.detach().double(), bn.eps)
    assert margin >= STACK_MARGIN, margin
    (h * wgt.double()).sum().backward()
    # device
    convs, bns = convs.to(DEV).train(), bns.to(DEV).train()
    xd, ed = x.to(DEV).requires_grad_(True), ea.to(DEV).requires_grad_(True)
    timer = ops.EntryPointTimer()
    ops.set_timer(timer)
    try:
        out = graph_ops.gine_kan_stack(xd, ed, g, list(convs), list(bns))
        assert out is not None
        (out * wgt.to(DEV)).sum().backward()
    finally:
        ops.set_timer(None)
    names = [r[0] for r in timer.records]
    assert names.count("kagnn_gine_kan_stack_bwd") == 1 and "kagnn_aggregate_gine_bwd" not in names, names
    assert_close(out, h.detach(), CONTRACT, what="GINE stack output", elementwise=False)
    assert_close(ed.grad, er.grad, CONTRACT, what="GINE stack edge_attr.grad (two convolutions accumulate)", elementwise=False)
    assert_close(xd.grad, xr.grad, CONTRACT, what="GINE stack x.grad", elementwise=False)


# ------------------------------------------------------------------ 5. pooling
POOL_FIXED = [0, 1, 0, 5, 64, 65, 1, 0]


def _segment_sizes(b):
    """B segments: the fixed sizes (empty, single-row, one wave's trip of 64 and one more) followed by random ones; fewer than
    eight segments take a window of the fixed ones"""
    gen = torch.Generator().manual_seed(b)
    seq = POOL_FIXED + torch.randint(0, 40, (64,), generator=gen).tolist()
    return torch.tensor(seq[:b] if b >= len(POOL_FIXED) else POOL_FIXED[3:3 + b])


def _poison(n, f):
    """leave NaNs in the block the allocator hands out next for an [n, f] fp32 matrix: an uninitialised row shows"""
    junk = torch.full((n, f), float("nan"), device=DEV)
    del junk


@pytest.mark.parametrize("b", [1, 3, 4, 5, 37])
def test_segment_pool_and_its_broadcast_match_fp64(b):
    sizes = _segment_sizes(b)
    n = int(sizes.sum())
    seg = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).to(torch.int32).to(DEV)
    batch = torch.repeat_interleave(torch.arange(b), sizes)
    empty = sizes == 0
    for k, f in enumerate([1, 16, 63, 64, 65, 200]):
        gen = torch.Generator().manual_seed(500 + f)
        x, gout = torch.randn(n, f, generator=gen), torch.randn(b, f, generator=gen)
        for mean in (False, True):
            xr = x.double().requires_grad_(True)
            ref = (orc.global_mean_pool if mean else orc.global_add_pool)(xr, batch, b)
            ref.backward(gout.double())
            xd = _sliced(x, k % 2 == 1, gen).detach().requires_grad_(True)
            gd = _sliced(gout, k % 2 == 1, gen)
            _poison(n, f)
            out = ops.segment_pool(xd, seg, mean)
            out.backward(gd)
            what = f"segment pool ({'mean' if mean else 'sum'})"
            assert_close(out, ref.detach(), what=what)
            assert_close(xd.grad, xr.grad, what=what + " x.grad")
            assert not bool(out.detach().cpu()[empty].any())                 # an empty segment: a zero row (mean: 0 / max(0, 1))


@pytest.mark.parametrize("how", ["autograd", "library-op"])
def test_rows_outside_every_segment_get_a_zero_gradient(how):
    """a ``seg_ptr`` that starts after row 0 and stops short of the last row: the pooled values do not depend on those rows, so
    their gradient is exactly zero -- also through ``kagnn::segment_pool``, the op the torch.compile path traces"""
    sizes = _segment_sizes(37)
    head, tail = 3, 5
    n = head + int(sizes.sum()) + tail
    seg = (torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]) + head).to(torch.int32).to(DEV)
    batch = torch.repeat_interleave(torch.arange(37), sizes)
    pool = ops.segment_pool if how == "autograd" else library.segment_pool
    for f in (16, 65):
        gen = torch.Generator().manual_seed(600 + f)
        x, gout = torch.randn(n, f, generator=gen), torch.randn(37, f, generator=gen)
        for mean in (False, True):
            xr = x.double()[head:n - tail].requires_grad_(True)
            ref = (orc.global_mean_pool if mean else orc.global_add_pool)(xr, batch, 37)
            ref.backward(gout.double())
            xd = x.to(DEV).requires_grad_(True)
            _poison(n, f)
            out = pool(xd, seg, mean)
            out.backward(gout.to(DEV))
            assert_close(out, ref.detach(), what=f"segment pool, partial cover ({how})")
            grad = xd.grad.cpu()
            assert_close(grad[head:n - tail], xr.grad, what=f"segment pool, partial cover ({how}) x.grad")
            assert torch.equal(grad[:head], torch.zeros(head, f)) and torch.equal(grad[n - tail:], torch.zeros(tail, f))
    # no segment at all: nothing depends on any row
    xd = torch.randn(4, 8).to(DEV).requires_grad_(True)
    _poison(4, 8)
    out = pool(xd, torch.zeros(1, dtype=torch.int32, device=DEV), False)
    assert out.shape == (0, 8)
    out.sum().backward()
    assert torch.equal(xd.grad.cpu(), torch.zeros(4, 8))


# ------------------------------------------------------------------ 6. embedding tables
# embedding_bwd (aggregate.hip): an LDS table of V x 64 floats per wave; 4 waves per workgroup while 4 tables fit 64 KiB
# (V <= 64), 2 while 2 fit 128 KiB (V <= 256), else 1 (V <= 512: 128 KiB of LDS); more rows are refused.  A workgroup covers
# 128 index rows (32 / 64 / 128 per wave), fetched 16 at a time.
EDGE_SHAPES = [(1, 1), (17, 64), (129, 70), (300, 130), (127, 64), (128, 70), (16, 1), (15, 130)]        # (N, F)
EMBEDDING_CASES = {1: [(15, 64), (128, 70), (300, 130)], 64: EDGE_SHAPES, 65: EDGE_SHAPES, 256: EDGE_SHAPES, 257: EDGE_SHAPES,
                   512: [(17, 64), (129, 70), (300, 130), (1, 1)]}


@pytest.mark.parametrize("v", sorted(EMBEDDING_CASES))
def test_embedding_table_forward_and_gradient_match_fp64(v):
    for n, f in EMBEDDING_CASES[v]:
        gen = torch.Generator().manual_seed(700 + 10 * n + f)
        table = torch.randn(v, f, generator=gen)
        idx = torch.randint(0, v, (n, 1), generator=gen)
        if n >= v:
            idx[:v, 0] = torch.randperm(v, generator=gen)            # (every table row is hit, the first and the last one included)
        gout = torch.randn(n, f, generator=gen)
        cases = [(idx, torch.ones(n, dtype=torch.bool))]
        if n >= 15:                                                    # out of range on either side: NaN rows forward, skipped backward
            bad = idx.clone()
            bad[n // 2, 0], bad[n - 1, 0] = -1, v
            cases.append((bad, (bad[:, 0] >= 0) & (bad[:, 0] < v)))
        for ix, ok in cases:
            td = table.to(DEV).requires_grad_(True)
            out = graph_ops.embedding_sum(ix.to(DEV), [td])
            want = table[ix[:, 0].clamp(0, v - 1)]
            want[~ok] = float("nan")
            got = out.detach().cpu()
            assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got[ok], want[ok]), (v, n, f)
            out.backward(gout.to(DEV))
            ref = torch.zeros(v, f, dtype=torch.float64).index_add_(0, ix[ok, 0], gout.double()[ok])
            assert_close(td.grad, ref, 1e-5, what="embedding table gradient" + ("" if bool(ok.all()) else ", indices out of range skipped"),
                         elementwise=False)
            again = graph_ops._embedding_sum_bwd_raw(ix.to(DEV), gout.to(DEV), [(v, f)])[0]
            assert torch.equal(again, td.grad), (v, n, f)                # bit-reproducible


def test_embedding_tables_of_more_than_512_rows_are_refused():
    idx = torch.zeros(4, 1, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="at most 512 rows"):
        graph_ops._embedding_sum_bwd_raw(idx, torch.ones(4, 8, device=DEV), [(513, 8)])
    assert graph_ops._embedding_sum_bwd_raw(idx, torch.ones(4, 8, device=DEV), [(512, 8)])[0].shape == (512, 8)
