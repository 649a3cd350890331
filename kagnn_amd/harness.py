"""Timing harness: the working counterpart of the reference's ``node_classification_clean/time_model.py``.

``time_model`` reproduces the reference loop :35-48 -- Adam(lr=1e-3), 20 x {zero_grad, forward, softmax,
CrossEntropyLoss on the masked nodes, backward, step} -- including its softmax-before-CE quirk, and fixes
what makes the original unusable as a benchmark: it warms up, synchronises the device
around the timed region, and forwards ``grid_size`` to the model.  Returns seconds per epoch.

``graphed=True`` captures one whole epoch (forward, loss, backward, Adam) into a HIP graph after the
warm-up and replays it: full-batch node classification has static shapes, and on Cora-sized graphs the
epoch is launch-bound (~150 kernels of a few microseconds each), so replaying removes the host from the
loop.  The arithmetic is the same kernels in the same order; the masked rows are selected through a
precomputed index instead of boolean indexing (which would synchronise inside the capture).
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import time
from typing import NamedTuple

import numpy as np
import torch


def _time_model_graphed(model, x, edge_index, y, mask, nb_epochs: int, warmup: int):
    from . import ops
    try:
        optimizer = torch.optim.Adam(model.parameters(), lr=0.001, capturable=True, fused=True)
    except (TypeError, RuntimeError):
        optimizer = torch.optim.Adam(model.parameters(), lr=0.001, capturable=True)
    if mask.dtype != torch.bool:
        mask = torch.zeros(x.size(0), dtype=torch.bool, device=x.device).index_fill_(0, mask, True)
    if isinstance(edge_index, ops.GraphIndex) or (isinstance(edge_index, torch.Tensor) and edge_index.is_sparse):
        graph_index = edge_index           # sparse adjacency (gcn timing branch): the convs index it, cached
    else:
        graph_index = ops.graph_index(edge_index, x.size(0))

    def epoch():
        optimizer.zero_grad(set_to_none=True)
        loss = ops.softmax_cross_entropy(model(x, graph_index), y, mask, pre_softmax=True)
        loss.backward()
        optimizer.step()
        return loss

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                    # warm-up off the default stream, as graph capture requires
        for _ in range(max(warmup, 3)):
            epoch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_loss = epoch()
    losses = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(nb_epochs):
        graph.replay()
        losses.append(static_loss.detach().clone())
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / nb_epochs
    return float(np.round(dt, 6)), [float(l) for l in losses]


@contextlib.contextmanager
def _autograd_threads(enabled: bool):
    """Run the backward passes inside on autograd's per-device worker threads (``True``) or on the calling thread (``False``).
    The backward of a ~1 ms step is ~80 kernel launches from ~10 library calls: handing every tape node to the engine's worker
    thread costs more than running it (host issue time of the ZINC-shaped step on the round-6 boxes: 1.41-1.50 ms per step with
    the engine's threads, 0.85-0.90 ms on the calling thread -- tools/host_profile_cfg4.py, profiles/r06_experiments.md).  One
    device, one stream: nothing runs concurrently in that backward anyway.  The timed loops pass ``KAGNN_CFG4_MT == "1"``, the
    switch that keeps the engine's threads for the A/B; the experiment loops always pass ``False``."""
    was = torch.autograd.is_multithreading_enabled()
    torch.autograd.set_multithreading_enabled(enabled)
    try:
        yield
    finally:
        torch.autograd.set_multithreading_enabled(was)


def time_model(model, x, edge_index, y, mask, nb_epochs: int = 20, warmup: int = 2, graphed: bool = False):
    if graphed:
        return _time_model_graphed(model, x, edge_index, y, mask, nb_epochs, warmup)
    from . import ops
    # (the reference's optimiser, time_model.py:36; on the device its update runs as ONE fused launch over all parameter tensors
    # instead of ~10 multi-tensor launches: same update rule)
    try:
        optimizer = torch.optim.Adam(model.parameters(), lr=0.001, fused=bool(x.is_cuda) and os.environ.get("KAGNN_FUSED_ADAM", "1") != "0")
    except (TypeError, RuntimeError):
        optimizer = torch.optim.Adam(model.parameters(), lr=0.001)
    losses = []

    def epoch():
        optimizer.zero_grad()
        out = model(x, edge_index)
        # the reference applies softmax before CrossEntropyLoss (:43-44): softmax, masked gather, log_softmax and the
        # mean are one kernel each way (kagnn_softmax_xent_*)
        loss = ops.softmax_cross_entropy(out, y, mask, pre_softmax=True)
        loss.backward()
        optimizer.step()
        return loss

    with _autograd_threads(os.environ.get("KAGNN_CFG4_MT", "0") == "1"):     # (round 6: on small graphs an epoch is such a ~1 ms step)
        for _ in range(warmup):
            epoch()
        if x.is_cuda:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(nb_epochs):
            losses.append(epoch())
        if x.is_cuda:
            torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / nb_epochs
    return float(np.round(dt, 6)), [float(l.detach()) for l in losses]


class Adam:
    """``torch.optim.Adam(params, lr, betas, eps, weight_decay)`` (no amsgrad) for fp32 device parameters as ONE library call per
    step (``kagnn_adam_step``: one launch per 64 tensors) -- the optimiser of the reference's graph-regression scripts
    (``graph_regression/optuna_zinc.py:49,62``).  Same update rule in fp32; what it removes is torch.optim's per-step Python (state
    dictionaries, tensor grouping, step counters kept as tensors: 0.2-0.3 ms of host time per step, fused or not -- a quarter of a
    256-molecule mini-batch's step).  ``step()`` / ``zero_grad()`` / ``state_dict()``-free by design: a training-loop helper, not a
    torch.optim subclass (schedulers and checkpoints want the real one: pass it to ``train_graph_batches(optimizer=...)``).
    As in torch.optim.Adam the step count of the bias correction is PER PARAMETER TENSOR and advances only when that tensor has a
    gradient (a global counter gave a tensor that skips steps another correction than the reference's optimiser);
    ``amsgrad`` / ``maximize`` are not implemented and rejected."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, amsgrad: bool = False,
                 maximize: bool = False):
        if amsgrad or maximize:
            raise NotImplementedError("kagnn_amd.harness.Adam implements torch.optim.Adam's default rule only (no amsgrad / maximize); "
                                      "pass a torch.optim.Adam to train_graph_batches(optimizer=...) for those")
        self.params = [p for p in params if p.requires_grad]
        if not self.params or any((not p.is_cuda) or p.dtype != torch.float32 or not p.is_contiguous() for p in self.params):
            raise TypeError("kagnn_amd.harness.Adam takes contiguous fp32 parameters on the GPU (there is no CPU path)")
        if len({p.device for p in self.params}) != 1:
            raise ValueError("kagnn_amd.harness.Adam: all parameters on one device")
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.steps = 0                                               # steps taken by the optimiser
        self._tensor_steps = None                                    # per-tensor counts; None while every tensor has taken every step
        total = sum(p.numel() for p in self.params)
        self._m = torch.zeros(total, dtype=torch.float32, device=self.params[0].device)
        self._v = torch.zeros_like(self._m)
        off, moff = 0, []
        for p in self.params:
            moff.append(off); off += p.numel()
        n = len(self.params)
        self._VP, self._I64 = ctypes.c_void_p * n, ctypes.c_int64 * n
        self._m_ptr = [self._m.data_ptr() + 4 * o for o in moff]
        self._v_ptr = [self._v.data_ptr() + 4 * o for o in moff]
        self._numel = [p.numel() for p in self.params]
        self._p_ptr = [p.data_ptr() for p in self.params]            # (parameters are updated in place: their storage stays)
        self._p_tab, self._m_tab, self._v_tab = self._VP(*self._p_ptr), self._VP(*self._m_ptr), self._VP(*self._v_ptr)
        self._n_tab = self._I64(*self._numel)

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            if set_to_none or p.grad is None:
                p.grad = None
            else:
                p.grad.zero_()

    @torch.no_grad()
    def step(self):
        self.steps += 1
        f32 = torch.float32
        ptrs = [p.data_ptr() for p in self.params]
        if ptrs != self._p_ptr:                                       # a parameter's storage was replaced (p.data = ...): follow it
            self._p_ptr, self._p_tab = ptrs, self._VP(*ptrs)
        gs = [p.grad for p in self.params]
        keep = None                                                   # the indices of the tensors that step; None: all
        if not all(g is not None and g.dtype is f32 and g.is_contiguous() for g in gs):     # rare: a subset, or gradients to convert
            # (`None in gs` would compare every TENSOR with None through torch's dispatcher: 10 us each)
            keep = [k for k, g in enumerate(gs) if g is not None]
            if not keep:
                self.steps -= 1                                       # (no gradient anywhere: not a step, as in torch.optim.Adam)
                return
            if len(keep) < len(gs) and self._tensor_steps is None:    # first time a tensor sits a step out: counts diverge from here
                self._tensor_steps = [self.steps - 1] * len(gs)
            gs = [g if g is None or (g.dtype is f32 and g.is_contiguous()) else g.to(f32).contiguous() for g in gs]
        if self._tensor_steps is None:
            return self._launch(keep, gs, self.steps)
        groups = {}
        for k in range(len(gs)) if keep is None else keep:
            self._tensor_steps[k] += 1
            groups.setdefault(self._tensor_steps[k], []).append(k)
        for t, ks in groups.items():                                  # one library call per distinct step count (normally one)
            self._launch(ks, gs, t)

    def _launch(self, ks, gs, t: int):
        """one ``kagnn_adam_step`` at step count ``t`` over the tensors with the indices ``ks`` (None: all) and the gradients
        ``gs[k]``; for all of them, the pointer tables cached at construction and one fresh table of gradient pointers"""
        from . import ops
        n = len(gs if ks is None else ks)
        if n == len(gs):
            tables = (self._p_tab, self._VP(*[g.data_ptr() for g in gs]), self._m_tab, self._v_tab, self._n_tab)
        else:
            VP, I64 = ctypes.c_void_p * n, ctypes.c_int64 * n
            tables = (VP(*[self._p_ptr[k] for k in ks]), VP(*[gs[k].data_ptr() for k in ks]), VP(*[self._m_ptr[k] for k in ks]),
                      VP(*[self._v_ptr[k] for k in ks]), I64(*[self._numel[k] for k in ks]))
        with ops._device_of(self.params[0]):
            ops._call("kagnn_adam_step", n, *tables, self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, t,
                      ops._stream())


class GradientReplicas:
    """Data-parallel replicas of a mini-batch training loop ("replicas only ... a gradient all-reduce of <= a few
    MB" -- BASELINE config 4: every rank trains the same model on its own mini-batches; the reference loop is
    ``graph_regression/optuna_zinc.py:56-66`` on one device).  ONE flat all-reduce per step, between ``backward()`` and
    ``optimizer.step()``: the ranks' gradients are concatenated into one buffer, summed (RCCL), and ``p.grad`` of every parameter
    becomes a view of the result.  The 1/P of the mean over the global batch is folded into the upstream gradient of the loss
    (``scale()``), so the all-reduce is a plain sum and no extra pass touches the gradients.  Parameters are broadcast from
    rank 0 at construction; equal updates keep them equal (the optimiser state is replicated, not communicated)."""

    def __init__(self, params, group=None):
        import torch.distributed as dist
        self.group = group
        self.world = dist.get_world_size(group)
        self.params = [p for p in params if p.requires_grad]
        for p in self.params:
            dist.broadcast(p.data, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        self._flat = None
        self._scale = None

    def scale(self, like: torch.Tensor) -> torch.Tensor:
        """the upstream gradient ``1 / world`` of this rank's loss (``loss.backward(replicas.scale(loss))``)"""
        if self._scale is None or self._scale.device != like.device or self._scale.dtype != like.dtype:
            self._scale = torch.full((), 1.0 / self.world, dtype=like.dtype, device=like.device)
        return self._scale

    def sync(self) -> None:
        """sum the gradients of this step over the ranks: one ``torch.cat``, one all-reduce, views back"""
        import torch.distributed as dist
        live = [p for p in self.params if p.grad is not None]
        if not live:
            return
        flat = torch.cat([p.grad.reshape(-1) for p in live])
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.group)
        off = 0
        for p in live:
            n = p.numel()
            p.grad = flat[off:off + n].view_as(p)
            off += n


def train_graph_batches(model, batches, nb_epochs: int = 1, warmup: int = 0, lr: float = 1e-3, optimizer=None, group=None,
                        loss_fn=None):
    """The mini-batch training loop of the reference's graph-regression scripts (``graph_regression/optuna_zinc.py:56-66``: Adam,
    L1 loss, ``{zero_grad, loss(model(data).squeeze(), data.y), backward, step}`` per batch) over ``batches`` -- objects with
    ``x, edge_index, edge_attr, batch, y`` (``num_graphs`` / ``ptr`` when the loader supplies them) already on the device: a list
    of premade batches, or any re-iterable with ``len()`` such as ``kagnn_amd.data.DeviceBatchLoader``, which assembles a fresh
    (reshuffled) batch per step on the device and hands the model its CSR index with it.
    Returns ``(seconds per step, mean training loss per epoch)``.  Differences from the script, none of them in the mathematics:
    * the optimiser is ``kagnn_amd.harness.Adam`` unless one is passed (torch.optim.Adam's rule in fp32 as one library call;
      torch's own kernels round differently -- its fused one mixes double arithmetic -- so trajectories agree to rounding, not
      to the bit; with ``optimizer=torch.optim.Adam(..., fused=True)`` the loop IS the script's, bit for bit);
    * the loss is ``ops.l1_loss`` (the same mean absolute error, the same gradient bits; its forward sum runs in another order);
    * the running loss is accumulated ON THE DEVICE and read once per epoch -- the script's ``loss.item()`` per batch drains the
      stream every step, which on a step of ~1 ms of device work is the difference between the host running ahead of the GPU
      and waiting for it.
    ``group`` (a torch.distributed process group, or ``True`` for the default one): data-parallel REPLICAS -- ``batches`` are this
    rank's own; every step ends in ONE flat gradient all-reduce (``GradientReplicas``), i.e. the step of the script on the
    P-times larger batch that the ranks' batches form together (except that BatchNorm statistics stay per replica, as in
    torch's DistributedDataParallel).  The returned loss is this rank's."""
    replicas = None
    if group is not None:
        replicas = GradientReplicas(model.parameters(), None if group is True else group)
    from . import ops as ops_mod
    if loss_fn is None:
        loss_fn = ops_mod.l1_loss      # = torch.nn.L1Loss() (mean |p - t|), one launch each way instead of six
    losses, weights = [], []

    def begin():
        losses.clear()
        weights.clear()

    def batch_loss(data):
        return loss_fn(model(data).squeeze(), data.y.squeeze())

    def end():             # (still no read-back: the caller converts after the final synchronisation)
        return _weighted_mean(losses, weights) if losses else torch.zeros(())

    dt, means = _train_minibatches(model, batches, nb_epochs, warmup, lr, optimizer, replicas, begin, batch_loss,
                                   lambda loss, data: (losses.append(loss), weights.append(_graphs_in(data))), end)
    return dt, [float(m) for m in means]


def _graphs_in(data) -> float:
    return float(int(getattr(data, "num_graphs", 0) or data.y.size(0)))


def _weighted_mean(losses, weights) -> torch.Tensor:
    """the mean of the per-batch device losses weighted by graphs per batch: three small launches per EPOCH, no read-back"""
    w = torch.tensor(weights, dtype=losses[0].dtype).to(losses[0].device, non_blocking=True)
    return (torch.stack(losses) * w).sum() / max(sum(weights), 1.0)


def _training_step(optimizer, replicas=None):
    """the training step every loop here takes: ``step(loss_of, *args)`` does ``{zero_grad(set_to_none=True), loss = loss_of(*args),
    backward, [the replicas' gradient all-reduce], optimizer.step()}`` and returns the loss.  The root gradient of the backward is
    cached (the implicit one would be a ``torch.ones_like``: one fill launch per step) and made again only when the loss changes
    device, dtype or shape; with replicas it is their ``scale()``."""
    root = None

    def step(loss_of, *args):
        nonlocal root
        optimizer.zero_grad(set_to_none=True)
        loss = loss_of(*args)
        if replicas is None:
            if root is None or root.device != loss.device or root.dtype != loss.dtype or root.shape != loss.shape:
                root = torch.ones(loss.shape, dtype=loss.dtype, device=loss.device)
            loss.backward(root)
        else:
            loss.backward(replicas.scale(loss))
            replicas.sync()
        optimizer.step()
        return loss
    return step


def _train_minibatches(model, batches, nb_epochs, warmup, lr, optimizer, replicas, begin, batch_loss, record, end):
    """the skeleton the mini-batch training loops share (``train_graph_batches``, ``train_graph_classification``): per epoch
    ``begin()``, then per batch ``{zero_grad, loss = batch_loss(data), backward, step, record(loss.detach(), data)}``, then the
    epoch's deferred graph checks and ``end()`` -- the epoch's figure.  Returns ``(seconds per step, [end() of every timed epoch])``."""
    if optimizer is None:
        optimizer = Adam(model.parameters(), lr=lr)            # torch.optim.Adam's rule, one library call per step
    from . import ops as ops_mod
    model.train()
    on_gpu = any(p.is_cuda for p in model.parameters())
    step = _training_step(optimizer, replicas)

    def epoch():
        begin()
        for data in batches:
            record(step(batch_loss, data).detach(), data)      # (kept on the device: no kernel and no read-back per step)
        if on_gpu:
            ops_mod.flush_graph_checks()       # the epoch's deferred node-id range checks (incl. the LAST batch's): one wait per epoch
        return end()

    with _autograd_threads(os.environ.get("KAGNN_CFG4_MT", "0") == "1"):     # (=1: the engine's worker threads, for A/B)
        for _ in range(warmup):
            epoch()
        if on_gpu:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        means = [epoch() for _ in range(nb_epochs)]
        if on_gpu:
            torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / max(1, nb_epochs * len(batches))
    return float(dt), means


def evaluate_graph_batches(model, batches, loss_fn=None) -> float:
    """The evaluation loop of the same scripts (``graph_regression/optuna_zinc.py:68-73``: ``model.eval()``, no gradients,
    ``total += loss(model(data).squeeze(), data.y).item() * data.num_graphs``, divided by the number of graphs): the mean loss per
    graph over ``batches`` (as for ``train_graph_batches``).  The per-batch losses stay on the device and are read back ONCE; the
    deferred graph checks of the loop are flushed before that.  Leaves the model in evaluation mode, as the scripts do."""
    from . import ops as ops_mod
    if loss_fn is None:
        loss_fn = ops_mod.l1_loss
    model.eval()
    losses, weights = [], []
    with torch.no_grad():
        for data in batches:
            losses.append(loss_fn(model(data).squeeze(), data.y.squeeze()).detach())
            weights.append(_graphs_in(data))
    if any(p.is_cuda for p in model.parameters()):
        ops_mod.flush_graph_checks()
    return float(_weighted_mean(losses, weights)) if losses else 0.0


def _dataset_size(loader, seen=None) -> int:
    """``len(loader.dataset)``, the divisor of the reference's loops; for a plain list of batches, the graphs it holds (``seen``,
    where a pass over them has counted these already)"""
    ds = getattr(loader, "dataset", None)
    if ds is not None:
        return len(ds)
    return int(sum(_graphs_in(d) for d in loader)) if seen is None else seen


def train_graph_classification(model, loader, nb_epochs: int = 1, warmup: int = 0, lr: float = 1e-3, optimizer=None, loss_fn=None):
    """The training loop of the reference's graph-classification scripts (``graph_classification/graph_classification_utils.py:45-55``:
    ``loss = F.nll_loss(model(data), data.y)``, ``{zero_grad, backward, step}`` per batch, ``loss_all += data.num_graphs *
    loss.item()``, ``loss_all / len(loader.dataset)``) over ``loader`` -- a ``kagnn_amd.data.DeviceBatchLoader``, or any
    re-iterable of batch objects with ``len()``.  The skeleton is ``train_graph_batches``' (autograd on the calling thread, a
    cached root gradient, ``kagnn_amd.harness.Adam`` unless an optimiser is passed, the deferred graph checks once per epoch).
    Returns ``(seconds per step, [mean training loss per epoch])``.  The loss is ``ops.nll_loss`` with a ``ClassificationMeter``: one
    launch per batch that also adds the batch's loss sum to a device record, which is read ONCE per epoch -- the script's
    ``loss.item()`` per batch drains the stream every step.  With ``loss_fn=torch.nn.functional.nll_loss`` and
    ``optimizer=torch.optim.Adam(..., fused=True)`` the parameter trajectory is the script's, bit for bit (the epoch's loss is then
    ``sum(num_graphs * loss)`` over the batch losses kept on the device, summed in fp64, still one read per epoch)."""
    from . import ops as ops_mod
    meter = None
    if loss_fn is None:
        meter = ops_mod.ClassificationMeter(next(model.parameters()).device)
    losses, weights = [], []

    def begin():
        losses.clear()
        weights.clear()
        if meter is not None:
            meter.reset()

    def batch_loss(data):
        if meter is not None:
            return ops_mod.nll_loss(model(data), data.y, accumulate=meter)
        return loss_fn(model(data), data.y)

    def record(loss, data):
        if meter is None:
            losses.append(loss)
            weights.append(_graphs_in(data))

    def end():
        if meter is not None:
            nll_sum, _correct, graphs = meter.read()
            return nll_sum / max(_dataset_size(loader, graphs), 1)
        if not losses:
            return 0.0
        w = torch.tensor(weights, dtype=torch.float64).to(losses[0].device, non_blocking=True)
        return float((torch.stack(losses).double() * w).sum()) / max(_dataset_size(loader, int(sum(weights))), 1)

    return _train_minibatches(model, loader, nb_epochs, warmup, lr, optimizer, None, begin, batch_loss, record, end)


def evaluate_graph_classification(model, loader):
    """``val`` and ``test`` of the same scripts (``graph_classification_utils.py:57-72``: ``model.eval()``, ``loss_all +=
    F.nll_loss(model(data), data.y, reduction='sum').item()`` and ``correct += model(data).max(1)[1].eq(data.y).sum().item()``,
    both over ``len(loader.dataset)``) in ONE pass: ``(mean nll per graph, accuracy)``.  One ``ops.nll_loss(..., reduction='sum',
    accumulate=meter)`` launch per batch, under ``no_grad``; the deferred graph checks are flushed and the meter is read back ONCE,
    at the end.  Leaves the model in evaluation mode, as the scripts do."""
    from . import ops as ops_mod
    model.eval()
    meter = ops_mod.ClassificationMeter(next(model.parameters()).device)
    with torch.no_grad():
        for data in loader:
            ops_mod.nll_loss(model(data), data.y, reduction="sum", accumulate=meter)
    ops_mod.flush_graph_checks()
    nll_sum, correct, graphs = meter.read()
    n = max(_dataset_size(loader, graphs), 1)
    return nll_sum / n, correct / n


class _BestWeights:
    """the best-weights copy of the two early-stopping experiments: the live ``state_dict`` entries of ``model`` and clones of them
    (``saved``: the starting weights, until ``_run_until_stopped`` copies an improved epoch's over them); ``restore()`` loads the
    clones back.  ``who``: the calling function, for the error message."""

    def __init__(self, model, who: str):
        self.live = list(model.state_dict().values())
        if any(not t.is_contiguous() for t in self.live):
            raise ValueError(f"{who}: every state_dict entry must be contiguous (the snapshot copies them as bytes)")
        self.saved = [t.detach().clone() for t in self.live]

    def restore(self) -> None:
        with torch.no_grad():
            for t, saved in zip(self.live, self.saved):
                t.copy_(saved)


def _run_until_stopped(one_epoch, epochs: int, poll_every: int, stop, best=None) -> None:
    """the polled loop of the two early-stopping experiments: up to ``epochs`` times ``one_epoch()`` (which ends in ``stop.update``),
    then ``ops.copy_if(stop.improved, ...)`` into ``best``, a ``_BestWeights``, when there is one; the host reads the stopper's
    record every ``poll_every`` epochs and leaves at the first poll that sees the stop.  The backward passes run on the calling thread."""
    from . import ops as ops_mod
    with _autograd_threads(False):
        for epoch in range(epochs):
            one_epoch()
            if best is not None:
                ops_mod.copy_if(stop.improved, best.saved, best.live)
            if (epoch + 1) % poll_every == 0 and stop.read(history=False).stopped:
                break


class GraphRegressionResult(NamedTuple):
    """what ``train_graph_regression`` returns.  ``best_val_loss`` / ``test_loss``: what the reference's
    ``train_model_with_parameters`` returns -- the lowest validation figure (ties included) and the test figure of the last epoch
    that reached it (``test_epoch``; without a test loader: that validation figure).  ``epochs_run`` / ``best_epoch`` / ``stopped``
    as the device record counted them (``best_epoch``: the last STRICT improvement, the epoch ``keep_best`` restores).
    ``train_losses`` / ``val_losses`` / ``test_losses``: one figure per counted epoch, rounded once to fp32 as the device compared
    them; ``per_target``: the per-target mean absolute errors behind them, a CPU float64 ``[epochs_run, 3, T]`` tensor (splits in
    the order train, val, test)"""
    best_val_loss: float
    test_loss: float
    epochs_run: int
    best_epoch: int
    test_epoch: int
    stopped: bool
    train_losses: list
    val_losses: list
    test_losses: list
    per_target: torch.Tensor


def _regression_targets(loader) -> int:
    """the number of regression targets of a loader's graphs: 1 for ``y [G]``, T for ``y [G, T]``"""
    ds = getattr(loader, "dataset", None)
    y = ds.storage.y if ds is not None and hasattr(ds, "storage") else None
    if y is None and isinstance(loader, (list, tuple)) and loader:
        y = loader[0].y
    if y is None:
        raise TypeError("graph regression needs a kagnn_amd.data.DeviceBatchLoader over a dataset with targets, or a list of batches")
    return 1 if y.dim() == 1 else int(y.size(1))


def _regression_output(model, data):
    """``model(data)`` shaped like ``data.y``: ``[B, 1]`` against ``[B]`` loses its last axis (the scripts' ``.squeeze()``, which would
    also drop the batch axis of a one-graph batch)"""
    out = model(data)
    if out.dim() == 2 and out.size(1) == 1 and data.y.dim() == 1:
        out = out.squeeze(-1)
    return out


def _figures(per_target: torch.Tensor) -> list:
    """a split's figure per epoch from its ``[epochs, T]`` per-target means, as ``kagnn_regression_epoch_update`` takes it: added in
    index order in fp64, divided by T, rounded once to fp32"""
    out = []
    for row in per_target.tolist():
        acc = 0.0
        for v in row:
            acc += v
        out.append(float(np.float32(acc / len(row))) if row else float("nan"))
    return out


def train_graph_regression(model, train_loader, val_loader, test_loader=None, epochs: int = 1000, lr: float = 1e-3, patience: int = 20,
                           min_delta: float = 0.0, poll_every: int = 8, optimizer=None, loss_fn=None, target_scale=None,
                           keep_best: bool = False) -> GraphRegressionResult:
    """The graph-regression experiment of the reference (``graph_regression/optuna_zinc.py:38-92`` and ``optuna_qm9.py:38-96``,
    ``train_model_with_parameters``): per epoch a training pass with the L1 loss and Adam, a validation pass in ``eval()`` mode, the
    test pass whenever ``best_val_loss >= val_loss``, and ``EarlyStopper(patience)``; it returns the test figure at the best
    validation figure.  Here an epoch never reads anything back:
    * the training pass is ``train_graph_batches``' step (autograd on the calling thread, a cached root gradient,
      ``kagnn_amd.harness.Adam`` unless an optimiser is passed) with ``ops.l1_loss(pred, data.y, accumulate=train_meter)``: the
      launch that makes the loss also adds the batch's per-target absolute errors to a device record;
    * the validation and the test pass run under ``no_grad`` in ``eval()`` mode into meters of their own, with ``target_scale`` (the
      targets' standard deviation, fp32 ``[T]`` or ``[1, T]``) as ``scale`` -- the QM9 script's ``(y * std - pred * std).abs() / std``;
      ``None`` is the ZINC script's plain L1 figure.  THE TEST PASS RUNS EVERY EPOCH: skipping it on a miss would need the
      comparison's outcome on the host, i.e. a read-back per epoch.  The figure reported is still the one of the epochs where the
      script would have computed it (the device record takes it exactly when ``best_val >= val``);
    * ``ops.RegressionStop.update`` -- one tiny launch -- turns the three meters into the epoch's figures, applies both of the
      script's rules, files the figures in the history and zeroes the meters; with ``keep_best=True`` an ``ops.copy_if(improved,
      snapshot, live)`` over every ``state_dict`` entry follows and the snapshot (the weights of ``best_epoch``; the starting weights
      if no epoch counted) is loaded back at the end -- the scripts keep the last weights, which is the default here.
    The deferred graph checks are flushed once per epoch (one wait on the epoch's queue; the composition of
    ``train_graph_batches`` and two ``evaluate_graph_batches`` waits three times and reads two figures back).  The host reads the
    48-byte record every ``poll_every`` epochs and once, with the history, at the end; it leaves the loop at the first poll that
    sees the stop, and epochs run after the stop change neither the record nor the history nor the snapshot (they do train the
    live weights).  ``poll_every=1`` is the script's one synchronisation per epoch.
    ``loss_fn`` (e.g. ``torch.nn.L1Loss()``): that function drives the backward and the meter is fed by a second, ``no_grad``
    metered call on the same prediction; with it and ``optimizer=torch.optim.Adam(..., fused=True)`` the parameter trajectory is
    the script's, bit for bit.  The loaders: ``kagnn_amd.data.DeviceBatchLoader``s (divisor: ``len(loader.dataset)``) or lists of
    premade batches.  ``test_loader=None``: the validation figures stand in (the script then returns ``best_val_loss``).  Leaves
    the model in evaluation mode, as the scripts do."""
    from . import ops as ops_mod
    epochs, poll_every = int(epochs), max(1, int(poll_every))
    params = list(model.parameters())
    ops_mod._need_cuda(*params, target_scale)
    if not params:
        raise ValueError("train_graph_regression: the model has no parameters")
    dev = params[0].device
    targets = _regression_targets(train_loader)
    sizes = (_dataset_size(train_loader), _dataset_size(val_loader), _dataset_size(val_loader if test_loader is None else test_loader))
    scale = None
    if target_scale is not None:
        scale = target_scale.detach().to(torch.float32).reshape(-1).contiguous()
        if scale.numel() != targets:
            raise ValueError(f"train_graph_regression: target_scale has {scale.numel()} entries for {targets} targets")
    if optimizer is None:
        optimizer = Adam(params, lr=lr)
    meters = [ops_mod.RegressionMeter(targets, dev) for _ in range(2 if test_loader is None else 3)]
    train_meter, val_meter, test_meter = meters[0], meters[1], (None if test_loader is None else meters[2])
    stop = ops_mod.RegressionStop(patience, min_delta, max_epochs=epochs, num_targets=targets, device=dev)
    best = _BestWeights(model, "train_graph_regression") if keep_best else None
    step = _training_step(optimizer)

    def train_loss(data):
        pred = _regression_output(model, data)
        if loss_fn is None:
            return ops_mod.l1_loss(pred, data.y, accumulate=train_meter)
        loss = loss_fn(pred, data.y)
        with torch.no_grad():
            ops_mod.l1_loss(pred.detach(), data.y, accumulate=train_meter)
        return loss

    def one_epoch():
        model.train()
        for data in train_loader:
            step(train_loss, data)
        model.eval()
        with torch.no_grad():
            for loader, meter in ((val_loader, val_meter), (test_loader, test_meter)):
                if loader is not None:
                    for data in loader:
                        ops_mod.l1_loss(_regression_output(model, data), data.y, accumulate=meter, scale=scale)
        stop.update(train_meter, val_meter, test_meter, sizes)
        ops_mod.flush_graph_checks()           # the epoch's deferred checks (three loaders' batches): one wait per epoch

    _run_until_stopped(one_epoch, epochs, poll_every, stop, best)
    ops_mod.flush_graph_checks()
    st = stop.read()
    if keep_best:
        best.restore()
    model.eval()
    hist = st.history
    return GraphRegressionResult(best_val_loss=st.best_val, test_loss=st.test_at_best, epochs_run=st.epochs, best_epoch=st.best_epoch,
                                 test_epoch=st.test_epoch, stopped=st.stopped, train_losses=_figures(hist[:, 0]),
                                 val_losses=_figures(hist[:, 1]), test_losses=_figures(hist[:, 2]), per_target=hist)


def evaluate_graph_regression(model, loader, target_scale=None):
    """One evaluation pass of the same scripts (``optuna_zinc.py:68-73``, ``optuna_qm9.py:68-75``: ``model.eval()``, no gradients, the
    absolute errors summed per target over the batches, divided by ``len(loader.dataset)``, averaged over the targets):
    ``(mean, per-target MAE)`` -- the figure rounded once to fp32 as ``train_graph_regression`` reports it, and a CPU float64
    ``[T]`` tensor.  ``target_scale`` as there.  One metered ``ops.l1_loss`` launch per batch; the deferred graph checks are flushed
    and the meter is read back ONCE, at the end.  Leaves the model in evaluation mode."""
    from . import ops as ops_mod
    params = list(model.parameters())
    ops_mod._need_cuda(*params, target_scale)
    targets = _regression_targets(loader)
    scale = None if target_scale is None else target_scale.detach().to(torch.float32).reshape(-1).contiguous()
    meter = ops_mod.RegressionMeter(targets, params[0].device)
    model.eval()
    with torch.no_grad():
        for data in loader:
            ops_mod.l1_loss(_regression_output(model, data), data.y, accumulate=meter, scale=scale)
    ops_mod.flush_graph_checks()
    abs_sum, graphs = meter.read()
    per_target = abs_sum / float(_dataset_size(loader, graphs))
    return _figures(per_target[None])[0], per_target


class NodeClassificationResult:
    """what ``train_node_classification`` returns: the figures the reference's ``train_total`` returns (``train_acc``, ``val_acc``,
    ``val_loss``, ``test_acc``; NaN for an empty split), ``epochs_run`` / ``best_epoch`` / ``stopped`` as the device record counted
    them, and ``history`` -- the ``ops.node_eval`` records of every counted epoch, a CPU int64 ``[epochs_run, 3, 3]`` tensor
    (``history[e, s]`` = split ``s`` in {train, val, test}: xent_sum as the bits of a double, correct, rows)"""
    __slots__ = ("train_acc", "val_acc", "val_loss", "test_acc", "epochs_run", "best_epoch", "stopped", "history")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])

    def __repr__(self):
        return "NodeClassificationResult(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in self.__slots__[:-1]) + ")"


def _split_figures(row: torch.Tensor):
    """(mean loss rounded once to fp32, accuracy) of one ``[3]`` history entry; an empty split: NaN, NaN"""
    xent, correct, rows = float(row[:1].view(torch.float64)[0]), int(row[1]), int(row[2])
    if rows == 0:
        return float("nan"), float("nan")
    return float(np.float32(xent / rows)), correct / rows


def train_node_classification(model, x, edge_index, y, train_mask, val_mask, test_mask=None, epochs: int = 1000, lr: float = 1e-2,
                              patience: int = 100, min_delta: float = 0.0, poll_every: int = 16, optimizer=None, loss_fn=None,
                              metrics_at: str = "last", _bits=None):
    """The node-classification experiment of the reference (``node_classification_clean/utils.py:162-193``, ``train_total`` with its
    ``EarlyStopper``): per epoch a training step on the ``train_mask`` rows, a second forward under ``no_grad`` STILL IN TRAIN MODE
    (batch statistics, running statistics updated again, dropout drawn again -- the script never switches to ``eval()`` here), the
    validation loss and the three accuracies of that output, the early stopper, the weights saved on every improvement and loaded
    back at the end.  Everything after the second forward stays on the device: ``ops.node_eval`` (one pass for the three splits),
    ``ops.EarlyStop.update`` and ``ops.copy_if(improved, snapshot, live)`` over every entry of the ``state_dict`` -- three launches
    and two more per 32 tensors.  The host reads the 32-byte record every ``poll_every`` epochs and once, with the history, at
    the end; it leaves the loop at the first poll that sees the stop.  Epochs run after the stop change neither the snapshot nor
    the history (they do train the live weights, which the snapshot then replaces, and they advance the RNG).
    ``poll_every=1`` is the script's one synchronisation per epoch.  The training loss is ``ops.softmax_cross_entropy(out, y,
    train_mask)`` and the optimiser ``kagnn_amd.harness.Adam`` unless given; with ``loss_fn=torch.nn.CrossEntropyLoss()`` (applied
    to ``out[train_mask], y[train_mask]``) and ``optimizer=torch.optim.Adam(...)`` the parameter trajectory is the script's, bit
    for bit.  ``test_mask=None``: the validation mask.  ``metrics_at``: ``"last"`` -- the figures of the last counted epoch's
    output, as the script returns them (NOT those of the reloaded weights) -- or ``"best"``, the best epoch's.  ``edge_index``:
    int64 ``[2, E]`` or an ``ops.GraphIndex``; the index is built once."""
    from . import ops as ops_mod
    if metrics_at not in ("last", "best"):
        raise ValueError(f"train_node_classification: metrics_at must be 'last' or 'best', got {metrics_at!r}")
    epochs, poll_every = int(epochs), max(1, int(poll_every))
    ops_mod._need_cuda(x, y, train_mask, val_mask, test_mask, *model.parameters())
    if test_mask is None:
        test_mask = val_mask
    g = edge_index if isinstance(edge_index, ops_mod.GraphIndex) or edge_index.is_sparse else ops_mod.graph_index(edge_index, x.size(0))
    bits = ops_mod.split_bits(train_mask, val_mask, test_mask, out=_bits)
    if optimizer is None:
        optimizer = Adam(model.parameters(), lr=lr)
    best = _BestWeights(model, "train_node_classification")       # the script saves the starting weights before the first epoch
    stop = ops_mod.EarlyStop(patience, min_delta, max_epochs=epochs, num_splits=3, device=x.device)
    records = torch.empty((3, 3), dtype=torch.int64, device=x.device)
    step = _training_step(optimizer)
    model.train()

    def train_loss():
        out = model(x, g)
        return ops_mod.softmax_cross_entropy(out, y, train_mask) if loss_fn is None else loss_fn(out[train_mask], y[train_mask])

    def one_epoch():
        step(train_loss)
        with torch.no_grad():
            out = model(x, g)
        ops_mod.node_eval(out, y, bits, 3, out=records)
        stop.update(records, 1)

    _run_until_stopped(one_epoch, epochs, poll_every, stop, best)
    ops_mod.flush_graph_checks(x.device)
    st = stop.read()
    best.restore()
    at = st.epochs - 1 if metrics_at == "last" else st.best_epoch
    nan = float("nan")
    (_, train_acc), (val_loss, val_acc), (_, test_acc) = [_split_figures(st.history[at, s]) for s in range(3)] if at >= 0 else [(nan, nan)] * 3
    return NodeClassificationResult(train_acc=train_acc, val_acc=val_acc, val_loss=val_loss, test_acc=test_acc, epochs_run=st.epochs,
                                    best_epoch=st.best_epoch, stopped=st.stopped, history=st.history)


def train_node_classification_sampled(model, x, edge_index, y, train_mask, val_mask, test_mask=None, fanouts=None, batch_size: int = 1024,
                                      seed: int = 0, epochs: int = 1000, lr: float = 1e-2, patience: int = 100, min_delta: float = 0.0,
                                      poll_every: int = 16, optimizer=None, loss_fn=None):
    """``train_node_classification`` with neighbour-sampled mini-batches (GraphSAGE training; no counterpart in the reference, whose
    node-level scripts are full batch).  Per epoch every batch of a ``kagnn_amd.NeighborLoader`` over the ``train_mask`` ids
    (``fanouts``, ``batch_size``, ``seed``; reshuffled per epoch from a ``torch.Generator`` seeded with ``seed``, so that one
    ``seed`` fixes both the order and the sampling) takes one training step on its sampled subgraph, ``model(batch.x, batch.index)``, with the
    loss on ``out[batch.seed_rows]`` against ``batch.y`` (``ops.softmax_cross_entropy`` unless ``loss_fn`` is given).  Then ONE
    full-graph forward under ``no_grad`` in EVAL mode (running statistics, no dropout: a sampled batch's statistics say nothing about
    the full graph's) and the device bookkeeping of ``train_node_classification``, unchanged: ``ops.node_eval`` over the three
    splits, ``ops.EarlyStop.update``, the predicated best-weights copy, a poll of the 32-byte record every ``poll_every`` epochs.
    The per-batch read of the two subgraph counts (``ops.sample_neighbors``) is the loop's only synchronisation between polls.
    Returns a ``NodeClassificationResult`` with the figures of the last counted epoch; the best weights are loaded back and the
    model is left in training mode.  ``fanouts`` is required (one entry per hop, ``kagnn_amd.receptive_hops(model)`` of them for
    the model's full depth)."""
    from . import ops as ops_mod
    from .data import NeighborLoader
    if fanouts is None:
        raise ValueError("train_node_classification_sampled: fanouts is required (one fan-out per hop, -1 for all neighbours)")
    fan = ops_mod._fanouts("train_node_classification_sampled", fanouts)
    epochs, poll_every = int(epochs), max(1, int(poll_every))
    ops_mod._need_cuda(x, y, train_mask, val_mask, test_mask, *model.parameters())
    if test_mask is None:
        test_mask = val_mask
    g = edge_index if isinstance(edge_index, ops_mod.GraphIndex) else ops_mod.graph_index(edge_index, x.size(0))
    bits = ops_mod.split_bits(train_mask, val_mask, test_mask)
    generator = torch.Generator().manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF)
    loader = NeighborLoader(g, train_mask, fan, batch_size, shuffle=True, generator=generator, seed=seed, x=x, y=y)
    if optimizer is None:
        optimizer = Adam(model.parameters(), lr=lr)
    best = _BestWeights(model, "train_node_classification_sampled")
    stop = ops_mod.EarlyStop(patience, min_delta, max_epochs=epochs, num_splits=3, device=x.device)
    records = torch.empty((3, 3), dtype=torch.int64, device=x.device)
    step = _training_step(optimizer)

    def batch_loss(batch):
        out = model(batch.x, batch.index)[batch.seed_rows]
        return ops_mod.softmax_cross_entropy(out, batch.y) if loss_fn is None else loss_fn(out, batch.y)

    def one_epoch():
        model.train()
        for batch in loader:
            step(batch_loss, batch)
        model.eval()
        with torch.no_grad():
            out = model(x, g)
        ops_mod.node_eval(out, y, bits, 3, out=records)
        stop.update(records, 1)

    _run_until_stopped(one_epoch, epochs, poll_every, stop, best)
    model.train()
    ops_mod.flush_graph_checks(x.device)
    st = stop.read()
    best.restore()
    at = st.epochs - 1
    nan = float("nan")
    (_, train_acc), (val_loss, val_acc), (_, test_acc) = [_split_figures(st.history[at, s]) for s in range(3)] if at >= 0 else [(nan, nan)] * 3
    return NodeClassificationResult(train_acc=train_acc, val_acc=val_acc, val_loss=val_loss, test_acc=test_acc, epochs_run=st.epochs,
                                    best_epoch=st.best_epoch, stopped=st.stopped, history=st.history)


class LinkPredictionResult:
    """what ``train_link_prediction`` returns.  ``val_*``: the figures of the BEST epoch (the weights that were loaded back),
    ``test_*``: those weights on the test split, evaluated once -- ``loss`` (mean BCE rounded once to fp32), ``acc`` (rows with
    ``(score > 0) == label``), ``auc`` (ROC-AUC), ``hits`` (``{k: share of positives above the k-th negative}``); NaN where a
    split is empty.  ``epochs_run`` / ``best_epoch`` / ``stopped`` as the device record counted them.  ``history``: the validation
    ``ops.bce_with_logits`` records of the counted epochs, a CPU int64 ``[epochs_run, 1, 3]`` tensor (loss sum as the bits of a
    double, correct, rows); ``rank_history``: their ``ops.link_rank`` records, CPU int64 ``[epochs_run, 8]``."""
    __slots__ = ("val_loss", "val_acc", "val_auc", "val_hits", "test_loss", "test_acc", "test_auc", "test_hits", "epochs_run",
                 "best_epoch", "stopped", "history", "rank_history")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])

    def __repr__(self):
        return "LinkPredictionResult(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in self.__slots__[:-2]) + ")"


def _link_figures(record: torch.Tensor, rank: torch.Tensor, ks):
    """(loss, accuracy, auc, hits) of one BCE record ``[3]`` and one rank record ``[8]`` on the host"""
    from . import ops as ops_mod
    loss, acc = _split_figures(record)
    fig = ops_mod.link_rank_figures(rank, ks)
    return loss, acc, fig["auc"], fig["hits"]


def train_link_prediction(model, x, split, epochs: int = 200, lr: float = 0.01, patience: int = 50, min_delta: float = 0.0,
                          poll_every: int = 16, neg_ratio: float = 1.0, seed: int = 0, optimizer=None, ks=(20, 50, 100)):
    """Link prediction by torch_geometric's standard recipe, device-resident like the other experiments here: ``model`` is a
    ``kagnn_amd.LinkPredictor``, ``x`` the node features, ``split`` a ``data.LinkSplit`` (``random_link_split``; evaluation
    negatives are attached with ``split.with_negatives(seed, neg_ratio)`` when it has none).  Per epoch ``e`` = 0, 1, ...:

    1. training negatives: ``ops.negative_sample(round(neg_ratio * P_train), keys of the training graph, N, seed + 16 * (e + 1))``
       -- THE SEED RULE; the evaluation negatives use ``seed + 1`` and ``seed + 2``, so no two draws share a seed for any number
       of epochs -- with ``attempts = 8``;
    2. one training step in train mode: ``z = model.encode(x, training graph)``, scores ``cat(decode(z, positives), decode(z,
       negatives))``, labels 1 / 0, weights 1 for the positives and ``valid`` for the negatives (an EMPTY slot weighs nothing),
       loss ``ops.bce_with_logits``, ``harness.Adam(lr)`` unless ``optimizer`` is given;
    3. an eval-mode ``no_grad`` forward on the validation split's graph, its positives and fixed negatives scored in one list;
    4. ``ops.bce_with_logits(accumulate=record)`` and ``ops.link_rank(out=rank_history[e])`` on those scores;
    5. ``ops.EarlyStop.update(record, 0)`` on the validation loss;
    6. ``ops.copy_if(improved, snapshot, live)`` over the ``state_dict``.

    Nothing is read back between polls (every ``poll_every`` epochs, 32 bytes): the positives and the evaluation pairs are
    indexed once, the negatives' pair index is built per epoch without synchronising as long as it has at most 65 536 pairs
    (``ops.pair_scores``).  Epochs run after the stop change neither the snapshot nor the counted histories.  At the end the best
    weights are loaded back, the test split is evaluated once on its own graph (training plus validation edges), and the model is
    left in training mode.  Returns a ``LinkPredictionResult``."""
    from . import ops as ops_mod
    epochs, poll_every = int(epochs), max(1, int(poll_every))
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError(f"train_link_prediction: seed must be an int, got {seed!r}")
    ks = [int(k) for k in ks]
    if len(ks) > ops_mod.LINK_RANK_MAX_KS or any(k < 1 for k in ks):
        raise ValueError(f"train_link_prediction: ks holds at most {ops_mod.LINK_RANK_MAX_KS} values >= 1, got {ks}")
    ops_mod._need_cuda(x, split.edge_index, split.train_edge_index, split.train_pos, *model.parameters())
    if split.val_neg is None:
        split = split.with_negatives(seed, neg_ratio)
    n, dev = split.num_nodes, x.device
    u8 = dict(dtype=torch.uint8, device=dev)
    g_train = ops_mod.graph_index(split.train_edge_index, n)
    g_val = g_train if split.val_edge_index is split.train_edge_index else ops_mod.graph_index(split.val_edge_index, n)
    train_keys = g_train.edge_keys
    p_train = int(split.train_pos.size(1))
    num_neg = round(neg_ratio * p_train)
    pos_index = ops_mod.GraphIndex(split.train_pos, n) if p_train else split.train_pos
    y_train = torch.cat([torch.ones(p_train, **u8), torch.zeros(num_neg, **u8)])
    w_pos = torch.ones(p_train, **u8)

    def eval_set(pos, neg, neg_valid):
        pairs = torch.cat([pos, neg], dim=1).contiguous()
        index = ops_mod.GraphIndex(pairs, n) if pairs.size(1) else pairs
        y = torch.cat([torch.ones(pos.size(1), **u8), torch.zeros(neg.size(1), **u8)])
        return index, y, torch.cat([torch.ones(pos.size(1), **u8), neg_valid])
    val_index, y_val, w_val = eval_set(split.val_pos, split.val_neg, split.val_neg_valid)
    if optimizer is None:
        optimizer = Adam(model.parameters(), lr=lr)
    best = _BestWeights(model, "train_link_prediction")
    stop = ops_mod.EarlyStop(patience, min_delta, max_epochs=epochs, num_splits=1, device=dev)
    record = torch.zeros((1, 3), dtype=torch.int64, device=dev)
    rank_history = torch.zeros((max(epochs, 1), 8), dtype=torch.int64, device=dev)
    step = _training_step(optimizer)
    epoch = 0

    def train_loss(neg, valid):
        z = model.encode(x, g_train)
        scores = torch.cat([model.decode(z, pos_index), model.decode(z, neg)])
        return ops_mod.bce_with_logits(scores, y_train, torch.cat([w_pos, valid]))

    def one_epoch():
        nonlocal epoch
        neg, valid = ops_mod.negative_sample(num_neg, train_keys, n, seed + 16 * (epoch + 1))
        model.train()
        step(train_loss, neg, valid)
        model.eval()
        with torch.no_grad():
            scores = model.decode(model.encode(x, g_val), val_index)
        ops_mod.bce_with_logits(scores, y_val, w_val, accumulate=record)
        ops_mod.link_rank(scores, y_val, w_val, ks, out=rank_history[epoch])
        stop.update(record, 0)
        epoch += 1

    _run_until_stopped(one_epoch, epochs, poll_every, stop, best)
    ops_mod.flush_graph_checks(dev)
    st = stop.read()
    ranks = rank_history[:st.epochs].cpu()
    best.restore()
    nan = float("nan")
    val = _link_figures(st.history[st.best_epoch, 0], ranks[st.best_epoch], ks) if st.best_epoch >= 0 else (nan, nan, nan, {k: nan for k in ks})
    test_index, y_test, w_test = eval_set(split.test_pos, split.test_neg, split.test_neg_valid)
    model.eval()
    with torch.no_grad():
        scores = model.decode(model.encode(x, ops_mod.graph_index(split.test_edge_index, n)), test_index)
    test_record = torch.zeros(3, dtype=torch.int64, device=dev)
    ops_mod.bce_with_logits(scores, y_test, w_test, accumulate=test_record)
    test = _link_figures(test_record.cpu(), ops_mod.link_rank(scores, y_test, w_test, ks).cpu(), ks)
    model.train()
    return LinkPredictionResult(val_loss=val[0], val_acc=val[1], val_auc=val[2], val_hits=val[3], test_loss=test[0], test_acc=test[1],
                                test_auc=test[2], test_hits=test[3], epochs_run=st.epochs, best_epoch=st.best_epoch, stopped=st.stopped,
                                history=st.history, rank_history=ranks)


def node_classification_splits(params: dict, x, edge_index, y, train_masks, val_masks, test_masks, **train_kw):
    """``all_splits`` of the reference (``node_classification_clean/utils.py:195-211``): a fresh ``make_model(params)`` trained by
    ``train_node_classification`` for every row of the ``[splits, N]`` mask tensors, with ``epochs``, ``lr`` and ``patience`` taken
    from ``params`` as the script does (``train_kw`` overrides them and passes anything else on).  Returns ``(models, train_accs,
    val_accs, val_losses, test_accs)`` -- lists with one entry per split.  The graph index and the split-bits byte buffer are built
    once and reused by every split."""
    from . import ops as ops_mod
    ops_mod._need_cuda(x, y, train_masks, val_masks, test_masks)
    g = edge_index if isinstance(edge_index, ops_mod.GraphIndex) or edge_index.is_sparse else ops_mod.graph_index(edge_index, x.size(0))
    bits = torch.empty(x.size(0), dtype=torch.uint8, device=x.device)
    kw = {k: params[k] for k in ("epochs", "lr", "patience") if k in params}
    kw.update(train_kw)
    models, train_accs, val_accs, val_losses, test_accs = [], [], [], [], []
    for s in range(train_masks.size(0)):
        model = make_model(params).to(x.device)
        res = train_node_classification(model, x, g, y, train_masks[s], val_masks[s], None if test_masks is None else test_masks[s],
                                        _bits=bits, **kw)
        models.append(model)
        train_accs.append(res.train_acc)
        val_accs.append(res.val_acc)
        val_losses.append(res.val_loss)
        test_accs.append(res.test_acc)
    return models, train_accs, val_accs, val_losses, test_accs


def count_params(model) -> int:
    return int(sum(p.numel() for p in model.parameters()))


def make_model(params: dict):
    """``utils.make_model`` of the reference (``node_classification_clean/utils.py:88-123``) for the KAN / FastKAN
    architectures: the same ``params`` dictionary builds the same model classes.  The MLP baselines
    (``architecture == 'mlp'``) are stock torch_geometric models and outside this package."""
    from .models import GFASTKAN_Nodes, GKAN_Nodes
    common = dict(_model_kwargs(params), grid_size=params["grid_size"])
    if params["architecture"] == "kan":
        return GKAN_Nodes(spline_order=params["spline_order"], **common)
    if params["architecture"] == "fastkan":
        return GFASTKAN_Nodes(**common)
    raise ValueError("kagnn_amd.harness.make_model builds the 'kan' and 'fastkan' architectures")


def _model_kwargs(params: dict) -> dict:
    """the keyword arguments every node-model class takes, from the reference's ``params`` dictionary"""
    return dict(conv_type=params["conv_type"], mp_layers=params["mp_layers"], num_features=params["num_features"],
                hidden_channels=params["hidden_channels"], num_classes=params["num_classes"], skip=params["skip"],
                hidden_layers=params["hidden_layers"], dropout=params["dropout"], heads=params.get("heads", 4))


def make_any_model(params: dict):
    """``utils.make_model`` of the reference (``node_classification_clean/utils.py:88-123``) for every architecture: ``'mlp'`` builds
    this package's ``baselines.GNN_Nodes`` from the same ``params`` dictionary, everything else goes to ``make_model``."""
    if params["architecture"] == "mlp":
        from .baselines import GNN_Nodes
        return GNN_Nodes(**_model_kwargs(params))
    return make_model(params)
