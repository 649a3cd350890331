"""The launch arithmetic of the co-run aggregation in the fused layer's backward (aggregate.hip: aggregate_sum with an AggCorun;
fused_calls.hip: layer_bwd_impl).  The transposed aggregation's row groups -- 16 rows each at 16 lanes per row, the grid rounded up
to whole eighths -- go through agg_rows_v4_corun_kernel as a head beside the deferred weight gradients and, unless the head's share
reaches 100 per cent, a tail behind the join; the hub kernels follow.  Whatever the split, every row is computed once and as the plain
row kernel computes it, so ``gx`` and every parameter gradient of the public fused backward equal the serial order's
(KAGNN_BWD_OVERLAP=0) bit for bit:

* both entry points: ``kagnn_gin_kan_layer_bwd`` and ``kagnn_gin_kan_layer_bwd_add`` with a ``gx`` addend;
* 64 -> 64 -> 64, grid 5, order 3, split mode, F = 64: both layers' weight gradients are deferred, the head's share is 100 per cent
  and the rows go in ONE launch; and the one-layer chain 64 -> 64, whose single deferred weight gradient leaves the two-launch path
  (the node models' case).  Row counts 1, 15, 127, 128 (one row group per XCD slot or fewer: a head that rounds down to zero row
  groups), 129 (a head of exactly eight row groups, a tail whose eighth is all but one round-up), 300, 2 049 and 20 000 (both
  launches with rows, a last eighth that is partly round-up);
* both orientations of the power-law recipe -- reversed, the hub rows sit on the side the backward aggregates over, so the hub
  kernels run behind the co-run launches -- and a graph whose last node has no edge at all;
* one case repeats the step twenty times and wants twenty equal results (a missing join shows as a row read in flight).
"""
import functools

import pytest
import torch

import kagnn_amd
from kagnn_amd import ops
from oracle import kan_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SWITCH = "KAGNN_BWD_OVERLAP"
ROW_COUNTS = [1, 15, 127, 128, 129, 300, 2_049, 20_000]
CASES = [(n, kind) for n in ROW_COUNTS for kind in ("forward", "reversed")] + [(129, "isolated"), (2_049, "isolated")]


def _edges(n):
    return 150_000 if n == 20_000 else 8 * n


@functools.lru_cache(maxsize=None)
def _graph(n, kind):
    if kind == "isolated":                     # the recipe on the first n - 1 nodes: node n - 1 has no edge in either direction
        ei = orc.powerlaw_graph(n - 1, _edges(n), seed=8)
    else:
        ei = orc.powerlaw_graph(n, _edges(n), seed=8)
        if kind == "reversed":
            ei = ei.flip(0).contiguous()
    return ops.GraphIndex(ei.to(DEV), n)


@functools.lru_cache(maxsize=None)
def _rows(n, seed):
    return (torch.randn(n, 64, generator=torch.Generator().manual_seed(seed)) * 0.5).to(DEV)


@functools.lru_cache(maxsize=None)
def _conv(nb_layers=2):
    torch.manual_seed(640 + nb_layers)
    return kagnn_amd.GIKANLayer(64, 64, grid_size=5, spline_order=3, hidden_dim=64, nb_layers=nb_layers).to(DEV)


class _Park(torch.autograd.Function):
    """identity whose backward hands ``addend`` to the convolution below it outside the tape, as the skip-concat read-out does"""

    @staticmethod
    def forward(ctx, y, skip, addend):
        ctx.skip, ctx.addend = skip, addend
        return y.view_as(y)

    @staticmethod
    def backward(ctx, g):
        ctx.skip.park(ctx.addend)
        return g, None, None


def _plain_entry_point(monkeypatch, seen):
    """route the node's ``kagnn_gin_kan_layer_bwd_add`` call with a null addend to ``kagnn_gin_kan_layer_bwd`` (the same arguments
    without the addend and its leading dimension)"""
    call = ops._call

    def routed(name, *args):
        if name == "kagnn_gin_kan_layer_bwd_add":
            assert args[23] is None and args[24] == 0, "this form carries no addend"
            seen.append("kagnn_gin_kan_layer_bwd")
            return call("kagnn_gin_kan_layer_bwd", *args[:23], *args[25:])
        return call(name, *args)

    monkeypatch.setattr(ops, "_call", routed)


def _step(conv, graph, x, gy, addend):
    """one forward + backward of the convolution through the fused node -> [x.grad, every parameter gradient]"""
    conv.zero_grad(set_to_none=True)
    xr = x.clone().requires_grad_(True)
    if addend is None:
        y = ops.gin_kan_layer(xr, graph, 1.0, conv.nn)
    else:
        skip = ops.SkipGradient()
        y = ops.gin_kan_layer(xr, graph, 1.0, conv.nn, skip_gradient=skip)
        assert skip.consumer
        y = _Park.apply(y, skip, addend)
    assert y is not None
    y.backward(gy)
    return [xr.grad.clone()] + [p.grad.clone() for p in conv.parameters()]


def _assert_same(got, want, conv, what):
    names = ["x.grad"] + [k for k, _ in conv.named_parameters()]
    assert len(got) == len(want) == len(names)
    for a, b, k in zip(got, want, names):
        assert torch.equal(a, b), f"{what}: {k} differs (max abs diff {float((a - b).abs().max()):.3e})"


@pytest.mark.parametrize("nb_layers", [2, 1])
@pytest.mark.parametrize("form", ["bwd", "bwd_add"])
@pytest.mark.parametrize("n,kind", CASES)
def test_fused_backward_overlap_on_equals_off_bitwise(n, kind, form, nb_layers, monkeypatch):
    graph = _graph(n, kind)
    if n == 20_000:            # the top node's edges are hub rows of the side they sit on: the transposed one when reversed
        assert (graph.num_hub_seg_t > 0) == (kind == "reversed")
    x, gy = _rows(n, 1), _rows(n, 2)
    addend = _rows(n, 3) if form == "bwd_add" else None
    seen = []
    if form == "bwd":
        _plain_entry_point(monkeypatch, seen)
    conv = _conv(nb_layers)
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv(SWITCH, flag)
        res[flag] = _step(conv, graph, x, gy, addend)
    assert form != "bwd" or seen == ["kagnn_gin_kan_layer_bwd"] * 2
    _assert_same(res["1"], res["0"], conv, f"n={n} {kind} {form} L={nb_layers}")
    assert all(bool(torch.isfinite(t).all()) for t in res["1"])
    if addend is not None:     # the addend arrived: without it gx is another matrix
        assert not torch.equal(res["1"][0], _step(conv, graph, x, gy, None)[0])


def test_twenty_steps_are_all_equal(monkeypatch):
    monkeypatch.setenv(SWITCH, "1")
    n = 20_000
    graph = _graph(n, "reversed")
    x, gy, addend = _rows(n, 1), _rows(n, 2), _rows(n, 3)
    conv = _conv()
    first = _step(conv, graph, x, gy, addend)
    for k in range(1, 20):
        _assert_same(_step(conv, graph, x, gy, addend), first, conv, f"step {k}")
