"""Which edges does a prediction rest on: edge masks for whole models and GNNExplainer on top of them.

``edge_mask`` is torch_geometric's explain hook restated for this package's convolutions -- inside the block every GIN / GCN
flavoured convolution multiplies the message of ORIGINAL edge ``e`` by ``mask[e]`` -- and ``explain_edges`` is GNNExplainer
(Ying et al. 2019; torch_geometric 2.5.3 ``explain.algorithm.GNNExplainer`` with its default coefficients) for the full-batch
node models.  The gradient of the mask comes from ``kagnn_aggregate_edge_grad`` (``ops.aggregate_edge_grad``) through the tape
node of ``ops.aggregate_sum``.
"""
from __future__ import annotations

import contextlib
import math
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops

_EPS = 1e-15


@contextlib.contextmanager
def edge_mask(mask: torch.Tensor):
    """``with edge_mask(mask): out = model(x, edge_index)``: every ``_SumAggregateConv`` / ``_NormalisedConv`` under the forwards
    inside the block (the KAN, FastKAN and MLP-baseline GIN / GCN convolutions, hence ``GKAN_Nodes``, ``GFASTKAN_Nodes``,
    ``GNN_Nodes`` and the graph-level models built on those convolutions) multiplies the message of ORIGINAL edge ``e`` by
    ``mask[e]``.  ``mask``: ``[E]`` float32 on the model's device; it may require a gradient, which then arrives through
    ``kagnn_aggregate_edge_grad``.  torch_geometric's semantics: the self term of GIN and the self loops GCN adds are NOT masked;
    GCN's normalisation is that of the unmasked graph (the mask enters beside ``deg^-1/2`` as an edge weight); self loops in the
    edge list, which GCN drops, get weight and gradient 0.  A convolution whose graph has another number of edges raises
    ``ValueError``; the attention and GINE convolutions, a sparse adjacency and an explicit ``edge_weight`` argument raise
    ``NotImplementedError``.

    While the block is open the routes that hide the aggregation step (the fused convolution node with or without its norm, the
    lazy-norm form between layers) take their per-operation form (``ops.aggregation_visible``); outside it nothing changes.  The
    block belongs to the thread that opened it; an inner block replaces the outer mask until it closes."""
    if not isinstance(mask, torch.Tensor) or mask.dim() != 1 or mask.dtype != torch.float32:
        raise ValueError("edge_mask: the mask must be a float32 tensor of shape [num_edges]")
    before = ops.edge_mask_of()
    ops._set_edge_mask(mask)
    try:
        yield mask
    finally:
        ops._set_edge_mask(before)


def _entropy(m: torch.Tensor) -> torch.Tensor:
    return -m * torch.log(m + _EPS) - (1.0 - m) * torch.log(1.0 - m + _EPS)


def explainer_loss(logits, target, edge_m, feat_m, node_idx=None, edge_size=0.005, edge_ent=1.0, feat_size=1.0, feat_ent=0.1):
    """GNNExplainer's objective: cross-entropy of ``logits`` against ``target`` (on row ``node_idx``, or on all rows) plus
    ``edge_size * sum(m) + edge_ent * mean(H(m))`` of the edge mask and ``feat_size * mean(f) + feat_ent * mean(H(f))`` of the
    feature mask (``None``: no feature terms); ``H(m) = -m log(m + 1e-15) - (1 - m) log(1 - m + 1e-15)``."""
    if node_idx is None:
        loss = F.cross_entropy(logits, target)
    else:
        loss = F.cross_entropy(logits[node_idx].reshape(-1, logits.size(-1)), target[node_idx].reshape(-1))
    loss = loss + edge_size * edge_m.sum() + edge_ent * _entropy(edge_m).mean()
    if feat_m is not None:
        loss = loss + feat_size * feat_m.mean() + feat_ent * _entropy(feat_m).mean()
    return loss


def receptive_hops(model: nn.Module) -> int:
    """How many hops of in-neighbourhood a node's prediction under ``model`` rests on: the number of message-passing convolutions
    under it (GIN, GCN, GAT and GINE flavoured: KAN, FastKAN and MLP baselines), plus ONE if any of them is GCN-normalised -- a
    node ``L`` hops out enters with ``deg^-1/2``, and its degree counts in-neighbours ``L + 1`` hops out, which a subgraph of
    ``L`` hops truncates.  The ``num_hops`` at which ``ops.k_hop_subgraph`` keeps the prediction at the seeds what it is on the full
    graph (eval mode).  ``ValueError`` for a model without convolutions."""
    from .graph_models import GINEKANLayer
    from .models import _AttentionConv, _NormalisedConv, _SumAggregateConv
    convs = [m for m in model.modules() if isinstance(m, (_SumAggregateConv, _NormalisedConv, _AttentionConv, GINEKANLayer))]
    if not convs:
        raise ValueError("receptive_hops: the model holds no message-passing convolution")
    return len(convs) + (1 if any(isinstance(m, _NormalisedConv) for m in convs) else 0)


def explain_edges(model: nn.Module, x: torch.Tensor, edge_index: torch.Tensor, *, node_idx=None, target: Optional[torch.Tensor] = None,
                  epochs: int = 100, lr: float = 0.01, edge_size: float = 0.005, edge_ent: float = 1.0, feat_size: float = 1.0,
                  feat_ent: float = 0.1, feature_mask: bool = True, generator: Optional[torch.Generator] = None, num_hops=None) -> dict:
    """GNNExplainer for a full-batch node model ``model(x, edge_index) -> [N, classes]``: learns a soft edge mask (and a soft feature
    mask shared by all nodes) under which the model keeps predicting ``target`` -- by default its own argmax prediction on the
    unmasked graph -- for node ``node_idx`` (``None``: for every node), while the masks are pushed towards few, decided entries.

    Edge logits start as ``1 + std * randn(E)``, ``std = sqrt(2) * sqrt(2 / (2 N))``, feature logits ``[1, F]`` as ``0.1 * randn``,
    both drawn from ``generator``.  Each epoch runs ``model(x * sigmoid(fm), edge_index)`` under ``edge_mask(sigmoid(em))``, takes
    ``explainer_loss`` and one ``torch.optim.Adam(lr)`` step on the two logit tensors.  The model runs in eval mode (the
    ``training`` flags are restored) and only the logits receive gradients: no parameter, buffer or ``.grad`` of the model
    changes.  Every kernel on the way is deterministic, so two calls with equally seeded generators return the same bits.

    Returns ``{"edge_mask": sigmoid(em) [E], "feature_mask": sigmoid(fm) [F] or None, "losses": [epochs]}`` on the device; the one
    host read, at the end, is the check that every loss was finite (``FloatingPointError`` otherwise).

    ``num_hops`` (an int, or ``"auto"`` = ``receptive_hops(model)``; needs ``node_idx``, ``ValueError`` otherwise): explain the node
    LOCALLY.  ``sub = ops.k_hop_subgraph(node_idx, num_hops, ops.graph_index(edge_index, N))`` is extracted on the device and the
    same loop runs on ``(x[sub.nodes], sub.index)`` with ``node_idx = sub.mapping``: the standard deviation of the edge logits
    uses the subgraph's node count, ``randn`` draws ``sub.num_edges`` values from ``generator``, the default target is the model's
    argmax on the subgraph, a ``target`` of length N is gathered at ``sub.nodes``.  With ``num_hops >= receptive_hops(model)`` the
    logits at ``node_idx`` are those of the full graph IN EVAL MODE, which is the mode this function runs the model in; the
    training-mode BatchNorm of a subgraph normalises with the subgraph's statistics and is a different function.  The result gains
    ``"nodes"`` and ``"edge_ids"`` (``sub.nodes``, ``sub.edge_ids``) and its ``"edge_mask"`` is scattered back to length E: exactly 0
    on every edge outside the subgraph.  ``None`` (the default) explains on the whole graph."""
    sub = None
    if num_hops is not None:
        if node_idx is None:
            raise ValueError("explain_edges: num_hops explains one node's neighbourhood and needs node_idx")
        hops = receptive_hops(model) if isinstance(num_hops, str) and num_hops == "auto" else num_hops
        if isinstance(hops, (str, bool)) or int(hops) != hops or hops < 0:
            raise ValueError(f"explain_edges: num_hops must be None, 'auto' or a non-negative integer, got {num_hops!r}")
        num_edges_full = edge_index.size(1)
        seeds = node_idx.to(x.device) if isinstance(node_idx, torch.Tensor) else node_idx
        sub = ops.k_hop_subgraph(seeds, int(hops), ops.graph_index(edge_index, x.size(0)))
        if target is not None and target.size(0) == x.size(0):
            target = target[sub.nodes]
        x, edge_index, node_idx = x[sub.nodes], sub.index, sub.mapping
    n, f = x.shape
    e = edge_index.size(1) if sub is None else sub.num_edges
    dev = x.device

    def randn(*shape):
        where = dev if generator is None else generator.device
        return torch.randn(*shape, generator=generator, device=where, dtype=torch.float32).to(dev)

    flags = [(m, m.training) for m in model.modules()]
    model.eval()
    try:
        xd = x.detach()
        if target is None:
            with torch.no_grad():
                target = model(xd, edge_index).argmax(dim=-1)
        em = (1.0 + math.sqrt(2.0) * math.sqrt(2.0 / (2 * n)) * randn(e)).requires_grad_(True)
        fm = (0.1 * randn(1, f)).requires_grad_(True) if feature_mask else None
        leaves = [em] if fm is None else [em, fm]
        opt = torch.optim.Adam(leaves, lr=lr)
        losses = []
        for _ in range(int(epochs)):
            edge_m = torch.sigmoid(em)
            feat_m = None if fm is None else torch.sigmoid(fm)
            with edge_mask(edge_m):
                logits = model(xd if feat_m is None else xd * feat_m, edge_index)
            loss = explainer_loss(logits, target, edge_m, feat_m, node_idx, edge_size, edge_ent, feat_size, feat_ent)
            for leaf, grad in zip(leaves, torch.autograd.grad(loss, leaves)):     # (not .backward(): the model's .grad stay as they are)
                leaf.grad = grad
            opt.step()
            losses.append(loss.detach())
        losses = torch.stack(losses) if losses else torch.empty(0, dtype=torch.float32, device=dev)
    finally:
        for m, flag in flags:
            m.training = flag
    if not bool(torch.isfinite(losses).all()):
        raise FloatingPointError("explain_edges: the loss became non-finite")
    out = {"edge_mask": torch.sigmoid(em).detach(), "feature_mask": None if fm is None else torch.sigmoid(fm).detach().reshape(-1),
           "losses": losses}
    if sub is not None:
        out["edge_mask"] = torch.zeros(num_edges_full, dtype=torch.float32, device=dev).index_copy_(0, sub.edge_ids, out["edge_mask"])
        out["nodes"], out["edge_ids"] = sub.nodes, sub.edge_ids
    return out
