"""The fused layer's backward with its weight gradients on a side stream beside the transposed aggregation (KAGNN_BWD_OVERLAP,
default on; fused_calls.hip: layer_bwd_impl).  The same kernels run on the same operands and reduce the same slabs in the same order,
and the aggregation's rows -- now two launches of the co-run row kernel, a capped head beside the weight gradients and a tail behind the
join -- are computed row by row as before, so every output is the serial order's (KAGNN_BWD_OVERLAP=0) bit for bit:

* x.grad and every parameter gradient, overlap on against off: chains of 1, 2 and 3 layers, a graph with more than one row tile
  and a row count that is no multiple of the tile, the same graph with its edges reversed (the hub rows -- about 1 000 edges on the
  top node -- are then on the side the BACKWARD aggregates over: hub segments and their merge run behind the co-run row kernel), a
  graph with fewer row tiles than CUs, a 40-feature input (the co-run row kernel on rows that do not fill their 16 lanes), and the
  node model with BatchNorm and skip (the _bwd_bn / _bwd_bn_sums entry points);
* the join: twenty steps in one process, the backward on the calling thread and on autograd's worker thread, each equal to the first
  (a consumer that did not wait for the side stream reads a weight gradient or a workspace in flight);
* a captured step stays serial: capture succeeds and the replay equals the eager step.
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


@functools.lru_cache(maxsize=None)
def _graph(n, e, reverse=False):
    ei = orc.powerlaw_graph(n, e, seed=8)
    if reverse:
        ei = ei.flip(0).contiguous()
    return ops.GraphIndex(ei.to(DEV), n)


@functools.lru_cache(maxsize=None)
def _rows(n, f, seed):
    return (torch.randn(n, f, generator=torch.Generator().manual_seed(seed)) * 0.5).to(DEV)


def _conv(fin, nb_layers):
    torch.manual_seed(10 * fin + nb_layers)
    return kagnn_amd.GIKANLayer(fin, 64, grid_size=5, spline_order=3, hidden_dim=64, nb_layers=nb_layers).to(DEV)


def _layer_step(conv, x, graph, gy):
    """one forward + backward of the convolution -> [x.grad, every parameter gradient]"""
    conv.zero_grad(set_to_none=True)
    xr = x.clone().requires_grad_(True)
    conv(xr, graph).backward(gy)
    return [xr.grad.clone()] + [p.grad.clone() for p in conv.parameters()]


def _names(module):
    return ["x.grad"] + [k for k, _ in module.named_parameters()]


def _assert_same(got, want, names, what):
    assert len(got) == len(want) == len(names)
    for a, b, k in zip(got, want, names):
        assert torch.equal(a, b), f"{what}: {k} differs (max abs diff {float((a - b).abs().max()):.3e})"


@pytest.mark.parametrize("nb_layers", [1, 2, 3])
@pytest.mark.parametrize("n,e,reverse,fin", [(20_000, 150_000, False, 64), (20_000, 150_000, True, 64), (300, 2_000, False, 64),
                                             (20_000, 150_000, True, 40)])
def test_layer_backward_overlap_on_equals_off_bitwise(n, e, reverse, fin, nb_layers, monkeypatch):
    graph = _graph(n, e, reverse)
    if n == 20_000:
        # the top node's ~1 000 edges are hub rows of the side they sit on: the transposed one when the edges are reversed
        assert (graph.num_hub_seg_t > 0) == reverse and (graph.num_hub_seg > 0) == (not reverse)
    x, gy = _rows(n, fin, 1), _rows(n, 64, 2)
    conv = _conv(fin, nb_layers)
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv(SWITCH, flag)
        res[flag] = _layer_step(conv, x, graph, gy)
    _assert_same(res["1"], res["0"], _names(conv), f"n={n} reverse={reverse} fin={fin} L={nb_layers}")
    assert all(bool(torch.isfinite(t).all()) for t in res["1"])
    assert float(res["1"][0].abs().max()) > 0 and float(res["1"][2].abs().max()) > 0


@pytest.mark.parametrize("reverse", [False, True])
def test_node_model_with_batchnorm_and_skip_overlap_on_equals_off_bitwise(reverse, monkeypatch):
    n = 20_000
    graph = _graph(n, 150_000, reverse)
    x = _rows(n, 64, 3)
    gout = _rows(n, 40, 4) / n
    torch.manual_seed(5)
    model = kagnn_amd.GKAN_Nodes("gin", 2, 64, 64, 40, skip=True, grid_size=5, spline_order=3, hidden_layers=2).to(DEV).train()
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv(SWITCH, flag)
        timer = ops.EntryPointTimer()
        ops.set_timer(timer)
        try:
            model.zero_grad(set_to_none=True)
            xr = x.clone().requires_grad_(True)
            model(xr, graph).backward(gout)
        finally:
            ops.set_timer(None)
        called = {r[0] for r in timer.records}
        assert any(k.startswith("kagnn_gin_kan_layer_bwd_bn") for k in called), sorted(called)
        res[flag] = [xr.grad.clone()] + [p.grad.clone() for p in model.parameters()]
    _assert_same(res["1"], res["0"], _names(model), f"GKAN_Nodes reverse={reverse}")


@pytest.mark.parametrize("worker_thread", [False, True])
def test_twenty_overlapped_steps_are_all_equal(worker_thread, monkeypatch):
    monkeypatch.setenv(SWITCH, "1")
    n = 20_000
    graph = _graph(n, 150_000, True)
    x, gy = _rows(n, 64, 1), _rows(n, 64, 2)
    conv = _conv(64, 2)
    was = torch.autograd.is_multithreading_enabled()
    torch.autograd.set_multithreading_enabled(worker_thread)      # False: every node's backward runs on the calling thread
    try:
        first = _layer_step(conv, x, graph, gy)
        for k in range(1, 20):
            _assert_same(_layer_step(conv, x, graph, gy), first, _names(conv), f"step {k} (worker thread: {worker_thread})")
    finally:
        torch.autograd.set_multithreading_enabled(was)


def test_captured_step_replays_the_eager_result(monkeypatch):
    monkeypatch.setenv(SWITCH, "1")
    n = 300
    graph = _graph(n, 2_000)
    x, gy = _rows(n, 64, 1), _rows(n, 64, 2)
    conv = _conv(64, 2)
    eager = _layer_step(conv, x, graph, gy)
    xs = x.clone().requires_grad_(True)

    def step():
        conv.zero_grad(set_to_none=True)
        xs.grad = None
        conv(xs, graph).backward(gy)
        return [xs.grad] + [p.grad for p in conv.parameters()]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                    # warm-up off the default stream, as graph capture requires
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    captured = torch.cuda.CUDAGraph()
    with torch.cuda.graph(captured):
        static = step()
    for t in static:
        t.zero_()
    captured.replay()
    torch.cuda.synchronize()
    _assert_same([t.clone() for t in static], eager, _names(conv), "replay of the captured step")
