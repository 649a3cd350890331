"""The local half of the feature-sharded FastKAN layer against fp64, one rank at a time.

``ops.fastkan_row_moments`` / ``fastkan_merge_moments`` / ``fastkan_shard_fwd`` / ``fastkan_shard_bwd`` (both halves) /
``fastkan_shard_bwd_finish`` are what ``kagnn_amd.sharded.ShardedFastKANLayer`` runs between its collectives.  Here the P ranks are a
Python loop over the column blocks ``[p*w, (p+1)*w)`` of one ``[N, P*w]`` input in ONE process: every rank's moments are stacked by
hand (the all-gather), every rank's row sums are added by hand in rank order, in fp32 on the device (the all-reduce).  No process
group, no collective.

The reference is the fp64 oracle of the UNSHARDED layer (``oracle.fastkan_layer_forward`` + autograd): a rank's gradients are the
column slices of the full ones; its partial ``y`` and its ``row_sums`` come from the fp64 restatement of the shard calls in
``helpers`` (``fk_shard_fwd`` / ``fk_shard_bwd``) on the fp64 statistics of the full row.  Every rank is compared on its own -- a sum
over the ranks can hide one rank's error behind the others' magnitude -- with ``helpers.assert_close`` at the default ``TOL``,
element-wise check on.  The one ``noise=`` term is on ``row_sums`` (see ``_compare``)."""
import functools
from types import SimpleNamespace

import pytest
import torch

import kagnn_amd
from kagnn_amd import ops
from oracle import kan_oracle as orc
from helpers import TOL, assert_close, fk_shard_bwd, fk_shard_bwd_finish, fk_shard_fwd, must_fail

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = [ops.PREC_FP32, ops.PREC_SPLIT]
MODE_IDS = ["fp32", "split"]
LN_EPS = 1e-5
EPS32 = float(torch.finfo(torch.float32).eps)
OUTPUTS = ("y", "row_sums", "gx", "g_ln_w", "g_ln_b", "g_spline", "g_base_w", "g_base_b")


def _ratio(got, want):
    """max-norm error in units of the rule's bound ``TOL * max|want|`` (> 1: the rule rejects ``got``)"""
    want = want.double().cpu()
    return float((got.detach().double().cpu() - want).abs().max() / (TOL * want.abs().max()))


# ================================================================================== (a) the LayerNorm exchange
FAMILIES = {"unit": (1.3, 0.2), "offset50": (0.5, 50.0)}      # x = a * randn + b; offset50: |mean| = 100 std, what Chan's merge is for


def _rows(family, n, width, seed):
    a, b = FAMILIES[family]
    return torch.randn(n, width, generator=torch.Generator().manual_seed(seed)) * a + b


def _stats64(x):
    xd = x.double()
    mean = xd.mean(1)
    return mean, torch.rsqrt(((xd - mean[:, None]) ** 2).mean(1) + LN_EPS)


def _device_stats(xd, P, w):
    gathered = torch.stack([ops.fastkan_row_moments(xd[:, p * w:(p + 1) * w].contiguous()) for p in range(P)])
    return gathered, ops.fastkan_merge_moments(gathered, w, LN_EPS)


@pytest.mark.parametrize("family,w", [(f, w) for f in FAMILIES for w in (1, 3, 4, 20, 64, 100) if f == "unit" or w >= 4])
def test_merged_row_statistics_vs_fp64(family, w, capsys):
    """``row_moments`` per rank, then ``merge_moments``: (mean, 1 / sqrt(biased variance + eps)) over all P * w columns against fp64.
    N = 1 and 17: partial 16-row groups of the moments kernel, a partial 256-thread block of the merge.  The offset family holds the
    kernels to what they are built for (|mean| >> std); it starts at w = 4: below that an exact fp32 evaluation of the same
    formulas already reaches 1.5e-5 in single elements, too close to the 2e-5 bound to tell a defect from rounding.  Its two controls -- a rank's LOCAL statistics, and the merge of (sum x, sum x^2) the kernel comment rejects --
    must miss the fp64 statistics under the same rule."""
    for P in (1, 2, 3, 8):
        for n in (1000, 1, 17):
            x = _rows(family, n, P * w, seed=1000 * P + w + n)
            mean64, rstd64 = _stats64(x)
            xd = x.to(DEV)
            gathered, stats = _device_stats(xd, P, w)
            assert stats.shape == (n, 2) and gathered.shape == (P, n, 2)
            assert_close(stats[:, 0], mean64, what=f"stats {family}: mean")
            assert_close(stats[:, 1], rstd64, what=f"stats {family}: rstd")
            if P == 1:              # one rank: its own (mean, rsqrt(M2 / w + eps))
                assert torch.equal(stats[:, 0], gathered[0, :, 0])
                assert_close(stats[:, 1], torch.rsqrt(gathered[0, :, 1].double() / w + LN_EPS), what=f"stats {family}: rstd of one rank's M2")
            if family == "offset50" and P > 1 and n == 1000:
                local = torch.rsqrt(gathered[0, :, 1] / w + LN_EPS)
                must_fail(local, rstd64, what=f"stats {family} w={w} P={P}: rank 0's local rstd")
                must_fail(gathered[0, :, 0], mean64, what=f"stats {family} w={w} P={P}: rank 0's local mean")
                s1 = torch.zeros(n, device=DEV)
                s2 = torch.zeros(n, device=DEV)
                for p in range(P):  # (sum x, sum x^2) per rank, added in rank order: fp32 torch ops
                    xs = xd[:, p * w:(p + 1) * w]
                    s1 += xs.sum(1)
                    s2 += (xs * xs).sum(1)
                m = s1 / (P * w)
                naive = torch.rsqrt(s2 / (P * w) - m * m + LN_EPS)
                must_fail(naive, rstd64, what=f"stats {family} w={w} P={P}: rstd from summed (sum x, sum x^2)")
                with capsys.disabled():
                    print(f"\nMARGIN stats {family} w={w} P={P}: local rstd {_ratio(local, rstd64):.3g} x bound, "
                          f"sum-of-squares rstd {_ratio(naive, rstd64):.3g} x bound, merged rstd {_ratio(stats[:, 1], rstd64):.3g} x bound")


@pytest.mark.parametrize("family", list(FAMILIES))
def test_row_moments_of_a_strided_column_view(family):
    """a shard passed as ``x_full[:, lo:hi]`` with an odd ``lo`` (row stride = the full width, unaligned start): the same bits as its
    contiguous copy"""
    for n in (1000, 17, 1):
        xd = _rows(family, n, 131, seed=n).to(DEV)
        for lo, w in ((1, 1), (1, 3), (3, 4), (5, 20), (33, 64), (31, 100)):
            view = xd[:, lo:lo + w]
            assert n == 1 or not view.is_contiguous()
            assert torch.equal(ops.fastkan_row_moments(view), ops.fastkan_row_moments(view.contiguous())), (n, lo, w)


# ================================================================================== (b) the layer halves
#        (N, in_total, P, out, centres, layernorm, base)
CASES = [(257, 64, 2, 64, 8, True, True),       # one-chunk split layer: a rank must not take the statistics from its own columns
         (129, 64, 8, 40, 8, True, True),       # width 8, the P = 8 headline shard; ragged out
         (300, 256, 2, 256, 8, True, True),     # width 128, out > 128: multi-chunk split; two launches over ot0 in fp32
         (333, 96, 3, 33, 5, True, False),      # LayerNorm without base branch: what gx holds before the finish adds into it
         (500, 130, 2, 24, 8, False, True),     # no LayerNorm (stats / row_sums None, the finish returns gx, None, None); odd width 65
         (150, 66, 2, 200, 3, True, True),      # odd width 33; seven 32-wide output tiles
         (200, 60, 3, 72, 17, True, True),      # 17 centres: split mode must land on the exact-fp32 kernels, finish included
         (1, 16, 4, 16, 4, True, True),         # one row, width 4
         (2100, 64, 2, 64, 8, True, True)]      # more rows than one dW row slab / one group of LayerNorm-backward blocks
ONE_CHUNK, WIDTH_128, ODD_33, CENTRES_17 = CASES[0], CASES[2], CASES[5], CASES[6]
WIDE_BUFFER = (64, 32, 2, 16, 8, True, True)    # its shards are column views of an [N, 7700] buffer (row stride > 7680 floats)


def _tag(shape):
    n, fi, P, fo, ng, use_ln, use_base = shape
    return f"{n}x{fi}_P{P}_out{fo}_G{ng}{'' if use_ln else '_noLN'}{'' if use_base else '_nobase'}"


@functools.lru_cache(maxsize=None)
def _case(shape):
    """the layer, its inputs and every fp64 reference of one case -- computed once, shared by the tests and modes, left unchanged"""
    n, fi, P, fo, ng, use_ln, use_base = shape
    assert fi % P == 0
    w = fi // P
    torch.manual_seed(sum(int(v) for v in shape))
    layer = kagnn_amd.FastKANLayer(fi, fo, num_grids=ng, use_base_update=use_base, use_layernorm=use_ln)
    with torch.no_grad():
        if use_ln:
            layer.layernorm.weight.uniform_(0.5, 1.5)
            layer.layernorm.bias.uniform_(-0.3, 0.3)
        if use_base:
            layer.base_linear.bias.uniform_(-0.5, 0.5)
    x = torch.randn(n, fi) * 1.3 + 0.2
    gy = torch.randn(n, fo)
    den = float(layer.rbf.denominator)
    p64 = {k: v.detach().double() for k, v in layer.state_dict().items()}
    w64 = {k: v.clone().requires_grad_(True) for k, v in p64.items() if k != "rbf.grid"}
    x64 = x.double().requires_grad_(True)
    y64 = orc.fastkan_layer_forward(x64, w64.get("layernorm.weight"), w64.get("layernorm.bias"), p64["rbf.grid"], den,
                                    w64["spline_linear.weight"], w64.get("base_linear.weight"), w64.get("base_linear.bias"), LN_EPS)
    y64.backward(gy.double())
    g_sw_full = w64["spline_linear.weight"].grad.view(fo, fi, ng)
    stats64 = torch.stack(_stats64(x), 1) if use_ln else None

    c = SimpleNamespace(shape=shape, n=n, fi=fi, P=P, w=w, fo=fo, ng=ng, use_ln=use_ln, use_base=use_base, den=den,
                        x=x, gy=gy, centers=p64["rbf.grid"].float(), stats64=stats64, ranks=[], dev=None)
    sums_total, states = None, []
    for p in range(P):
        cols = slice(p * w, (p + 1) * w)
        r = SimpleNamespace(cols=cols)
        r.lw = p64["layernorm.weight"][cols].float() if use_ln else None
        r.lb = p64["layernorm.bias"][cols].float() if use_ln else None
        r.sw = p64["spline_linear.weight"].view(fo, fi, ng)[:, cols, :].reshape(fo, w * ng).float()
        r.bw = p64["base_linear.weight"][:, cols].float().contiguous() if use_base else None
        r.bb = p64["base_linear.bias"].float() if (use_base and p == 0) else None          # the bias enters the summed partials once
        xs = x[:, cols].double()
        args = (stats64, None if r.lw is None else r.lw.double(), None if r.lb is None else r.lb.double(), r.sw.double(),
                None if r.bw is None else r.bw.double())
        want = {"y": fk_shard_fwd(xs, *args, None if r.bb is None else r.bb.double(), c.centers.double(), den)}
        st, sums, _, _, _ = fk_shard_bwd(xs, gy.double(), *args, c.centers.double(), den)
        states.append(st)
        want["row_sums"] = sums
        r.noise = (0.0, 0.0)
        if use_ln:
            h = st["gz"] * st["lw"]
            r.noise = (EPS32 * float(h.abs().sum(1).max()), EPS32 * float((h * st["zhat"]).abs().sum(1).max()))
            sums_total = sums.clone() if sums_total is None else sums_total + sums
        want["gx"] = x64.grad[:, cols]
        want["g_ln_w"] = w64["layernorm.weight"].grad[cols] if use_ln else None
        want["g_ln_b"] = w64["layernorm.bias"].grad[cols] if use_ln else None
        want["g_spline"] = g_sw_full[:, cols, :].reshape(fo, w * ng)
        want["g_base_w"] = w64["base_linear.weight"].grad[:, cols] if use_base else None
        want["g_base_b"] = w64["base_linear.bias"].grad if (use_base and p == 0) else None
        r.want = want
        c.ranks.append(r)
    # the two references must be one statement: the restated partials add up to the oracle's layer, the restated finish gives its gx
    assert float((sum(r.want["y"] for r in c.ranks) - y64.detach()).abs().max()) <= 1e-11 * float(y64.detach().abs().max())
    for r, st in zip(c.ranks, states):
        gx = fk_shard_bwd_finish(st, sums_total, fi)[0]
        assert float((gx - r.want["gx"]).abs().max()) <= 1e-11 * float(x64.grad.abs().max())
    return c


def _on_device(c):
    if c.dev is None:
        mv = lambda t: None if t is None else t.to(DEV)
        c.dev = SimpleNamespace(x=c.x.to(DEV), gy=c.gy.to(DEV), centers=c.centers.to(DEV),
                                ranks=[SimpleNamespace(lw=mv(r.lw), lb=mv(r.lb), sw=mv(r.sw), bw=mv(r.bw), bb=mv(r.bb)) for r in c.ranks])
    return c.dev


def _run(c, mode, part="both", x_src=None, strided=False, rows=None):
    """forward, backward and finish of every emulated rank -> one dict of the eight outputs per rank (+ ``mode``: what the state
    carries into the finish).  ``x_src``: the [N, in_total] rows to cut the shards from (default: the contiguous input);
    ``strided``: hand the column VIEWS to the calls, not contiguous copies; ``rows``: only rows [r0, r1) of x / stats / gy."""
    d = _on_device(c)
    x_full = d.x if x_src is None else x_src
    gy = d.gy
    stats = _device_stats(d.x, c.P, c.w)[1] if c.use_ln else None
    if rows is not None:
        x_full, gy, stats = x_full[rows[0]:rows[1]], gy[rows[0]:rows[1]], None if stats is None else stats[rows[0]:rows[1]]
    outs, states, total = [], [], None
    for p, r in enumerate(d.ranks):
        xs = x_full[:, p * c.w:(p + 1) * c.w]
        if not strided:
            xs = xs.contiguous()
        args = (stats, r.lw, r.lb, r.sw, r.bw)
        y = ops.fastkan_shard_fwd(xs, *args, r.bb, d.centers, c.den, mode)
        want_bias = c.use_base and p == 0
        if part == "both":
            st, sums, gsw, gbw, gbb = ops.fastkan_shard_bwd(xs, gy, *args, d.centers, c.den, mode, want_bias=want_bias)
        else:
            st, sums = ops.fastkan_shard_bwd_halves(xs, gy, *args, d.centers, c.den, mode, part="input")
            gsw, gbw, gbb = ops.fastkan_shard_bwd_halves(xs, gy, *args, d.centers, c.den, mode, part="weight", state=st, want_bias=want_bias)
        if p > 0:
            assert gbb is None
        if sums is not None:
            total = sums.clone() if total is None else total + sums          # the all-reduce: rank order, fp32, on the device
        states.append(st)
        outs.append({"y": y, "row_sums": sums, "g_spline": gsw, "g_base_w": gbw, "g_base_b": gbb, "mode": st.mode})
    for st, o in zip(states, outs):
        o["gx"], o["g_ln_w"], o["g_ln_b"] = ops.fastkan_shard_bwd_finish(st, total, c.fi)
    torch.cuda.synchronize()
    return outs


def _compare(c, outs, what, keys=OUTPUTS):
    for p, (r, o) in enumerate(zip(c.ranks, outs)):
        for k in keys:
            want, got = r.want[k], o[k]
            if want is None:
                assert got is None, (what, p, k)
                continue
            assert got is not None, (what, p, k)
            try:
                if k == "row_sums":
                    # the one noise term of this file.  row_sums[:, 0] = sum_f gz*gamma is a CANCELLING fp32 sum (its terms have both
                    # signs; the sum can be orders below them), row_sums[:, 1] = sum_f gz*gamma*zhat likewise: fp32 carries the
                    # rounding noise eps32 * sum_f |terms| of the worst row, taken from the fp64 reference
                    assert_close(got[:, 0], want[:, 0], what=f"{what}: row_sums[0]", noise=r.noise[0])
                    assert_close(got[:, 1], want[:, 1], what=f"{what}: row_sums[1]", noise=r.noise[1])
                else:
                    assert_close(got, want, what=f"{what}: {k}")
            except AssertionError as e:
                raise AssertionError(f"rank {p} of {c.P}: {e}") from None


def _same_bits(a, b, what, keys=OUTPUTS):
    assert len(a) == len(b)
    for p, (oa, ob) in enumerate(zip(a, b)):
        for k in keys:
            assert (oa[k] is None) == (ob[k] is None), (what, p, k)
            if oa[k] is not None:
                assert torch.equal(oa[k], ob[k]), f"{what}: rank {p}: {k} differs (max {float((oa[k] - ob[k]).abs().max()):.3e})"


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", CASES, ids=_tag)
def test_shard_halves_vs_fp64(shape, mode):
    c = _case(shape)
    outs = _run(c, mode)
    forced = c.ng > 16                         # more than 16 centres: the exact-fp32 kernels, and the state says so to the finish
    assert all(o["mode"] == (ops.PREC_FP32 if forced else mode) for o in outs)
    if not c.use_ln:
        assert all(o["row_sums"] is None and o["g_ln_w"] is None and o["g_ln_b"] is None for o in outs)
    _compare(c, outs, f"shard {_tag(shape)} {MODE_IDS[MODES.index(mode)]}")


def test_seventeen_centres_in_split_mode_are_the_exact_fp32_kernels():
    c = _case(CENTRES_17)
    _same_bits(_run(c, ops.PREC_SPLIT), _run(c, ops.PREC_FP32), "17 centres, split vs fp32")


def test_a_row_stride_past_7680_floats_in_split_mode_is_the_exact_fp32_kernels():
    """the shards are column views of an [N, 7700] buffer: the split kernels' 32-bit windows do not take that stride, the call falls
    back to the exact-fp32 kernels -- same bits as asking for them, and the fp64 result"""
    c = _case(WIDE_BUFFER)
    buf = torch.zeros(c.n, 7700, device=DEV)
    src = buf[:, 5:5 + c.fi]
    src.copy_(_on_device(c).x)
    assert src.stride(0) == 7700
    split = _run(c, ops.PREC_SPLIT, x_src=src, strided=True)
    exact = _run(c, ops.PREC_FP32, x_src=src, strided=True)
    assert all(o["mode"] == ops.PREC_FP32 for o in split)
    _same_bits(split, exact, "wide buffer, split vs fp32")
    _compare(c, split, f"shard {_tag(WIDE_BUFFER)} ld7700 split")
    assert all(o["mode"] == ops.PREC_SPLIT for o in _run(c, ops.PREC_SPLIT))       # (the contiguous shard stays on the split kernels)


# ================================================================================== (c) bit-level properties
BIT_CASES = [ONE_CHUNK, WIDTH_128, ODD_33]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", BIT_CASES, ids=_tag)
def test_the_two_halves_are_the_one_call_and_repeat_bit_for_bit(shape, mode):
    """``part="input"`` then ``part="weight", state=st`` (the all-reduce of the row sums runs between them in the product) gives the
    bits of ``part="both"``, and a second identical call gives the bits of the first (fixed-order reductions, no atomics)"""
    c = _case(shape)
    both = _run(c, mode)
    _same_bits(_run(c, mode, part="halves"), both, "input + weight vs both")
    _same_bits(_run(c, mode), both, "second call")


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", BIT_CASES, ids=_tag)
def test_a_strided_column_view_is_its_contiguous_copy_bit_for_bit(shape, mode):
    """the shard as ``x_full[:, lo:hi]``: row stride in_total and, at width 33, a start that is not 16-byte aligned"""
    c = _case(shape)
    d = _on_device(c)
    assert c.P == 1 or not d.x[:, c.w:2 * c.w].is_contiguous()
    _same_bits(_run(c, mode, strided=True), _run(c, mode), "column view vs contiguous copy")


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", BIT_CASES, ids=_tag)
def test_row_chunks_are_rows_of_the_one_call(shape, mode):
    """what ``_ShardedFastKANFn`` does: the calls on rows [r0, r1) of x, stats and gy, three ragged chunks.  Forward rows, gx rows
    and row_sums rows are the one call's bits; the weight and LayerNorm gradients, summed over the chunks, are the fp64 ones"""
    c = _case(shape)
    whole = _run(c, mode)
    a, b = c.n // 3 + 1, (2 * c.n) // 3 + 5
    chunks = [_run(c, mode, rows=rows) for rows in ((0, a), (a, b), (b, c.n))]
    summed = []
    for p in range(c.P):
        o = {k: torch.cat([ch[p][k] for ch in chunks]) for k in ("y", "row_sums", "gx")}
        for k in ("g_ln_w", "g_ln_b", "g_spline", "g_base_w", "g_base_b"):
            o[k] = None if chunks[0][p][k] is None else chunks[0][p][k] + chunks[1][p][k] + chunks[2][p][k]
        summed.append(o)
    _same_bits(summed, whole, "row chunks vs one call", keys=("y", "row_sums", "gx"))
    _compare(c, summed, f"shard {_tag(shape)} {MODE_IDS[MODES.index(mode)]} 3 row chunks", keys=("g_ln_w", "g_ln_b", "g_spline", "g_base_w", "g_base_b"))


# ================================================================================== (d) a rank without rows
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("use_ln", [True, False], ids=["LN", "noLN"])
def test_no_rows(use_ln, mode):
    """N = 0 (a rank whose row chunk is empty): empty row outputs, and every weight gradient an empty sum -- zeros,
    whatever the allocator hands out (the outputs' blocks are filled with NaN and freed first)"""
    w, P, fo, ng = 16, 2, 24, 8
    torch.manual_seed(3)
    x = torch.empty(0, w, device=DEV)
    gy = torch.empty(0, fo, device=DEV)
    lw, lb = (torch.rand(w, device=DEV) + 0.5, torch.rand(w, device=DEV)) if use_ln else (None, None)
    sw, bw, bb = torch.randn(fo, w * ng, device=DEV), torch.randn(fo, w, device=DEV), torch.randn(fo, device=DEV)
    centers = torch.linspace(-2, 2, ng, device=DEV)
    stats = None
    if use_ln:
        mom = ops.fastkan_row_moments(x)
        assert mom.shape == (0, 2)
        stats = ops.fastkan_merge_moments(torch.stack([mom] * P), w, LN_EPS)
        assert stats.shape == (0, 2)
    assert ops.fastkan_shard_fwd(x, stats, lw, lb, sw, bw, bb, centers, 0.5, mode).shape == (0, fo)
    for part in ("both", "halves"):
        for shape in ((fo, w * ng), (fo, w), (fo,), (w,), (w,)):
            torch.full(shape, float("nan"), device=DEV)                      # (freed at once: the next torch.empty of that size lands on it)
        if part == "both":
            st, sums, gsw, gbw, gbb = ops.fastkan_shard_bwd(x, gy, stats, lw, lb, sw, bw, centers, 0.5, mode, want_bias=True)
        else:
            st, sums = ops.fastkan_shard_bwd_halves(x, gy, stats, lw, lb, sw, bw, centers, 0.5, mode, part="input")
            gsw, gbw, gbb = ops.fastkan_shard_bwd_halves(x, gy, stats, lw, lb, sw, bw, centers, 0.5, mode, part="weight", state=st, want_bias=True)
        gx, glw, glb = ops.fastkan_shard_bwd_finish(st, sums, P * w)
        torch.cuda.synchronize()
        assert gx.shape == (0, w)
        assert gsw.shape == (fo, w * ng) and gbw.shape == (fo, w) and gbb.shape == (fo,)
        assert not bool(gsw.any()) and not bool(gbw.any()) and not bool(gbb.any())
        if use_ln:
            assert sums.shape == (0, 2) and glw.shape == (w,) and glb.shape == (w,)
            assert not bool(glw.any()) and not bool(glb.any())
        else:
            assert sums is None and glw is None and glb is None
