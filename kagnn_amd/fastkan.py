"""FastKAN layers with the reference's module surface, computed by libkagnn_hip.so.

Drop-in for ``node_classification_clean/fastkan.py`` of the reference (``SplineLinear`` :22-28,
``RadialBasisFunction`` :30-47, ``FastKANLayer`` :49-85, ``FastKAN`` :118-145): same constructor
signatures and the same state_dict keys (``layernorm.weight, layernorm.bias, rbf.grid,
spline_linear.weight, base_linear.weight, base_linear.bias``).  ``FastKANLayer.forward`` is one
call to ``kagnn_fastkan_fwd`` -- LayerNorm statistics, the Gaussian RBF expansion and both linear
maps are fused in the kernel.  ``plot_curve`` (:87-115) is one column of ``edge_curves``; on the same kernels
(``csrc/fastkan_edge.hip``) sit ``edge_l1`` and the KAN regulariser ``regularization_loss(x)``, which the reference has for
efficient-KAN layers only.  ``AttentionWithFastKANTransform`` (:148-202) is five ``FastKANLayer`` projections around ONE call
to ``ops.dense_attention`` (``csrc/attention.hip``): the reference's broadcast products ``[*, Q, K, H, c]`` and its attention
tensor ``[*, Q, K, H]`` never exist.

Attribution: the module surface restated here (class names, constructor signatures, attribute names, parameter layout and the
trunc-normal / linspace initialisation of ``SplineLinear`` / ``RadialBasisFunction`` / ``FastKANLayer`` / ``FastKAN`` /
``AttentionWithFastKANTransform``) follows the reference's ``node_classification_clean/fastkan.py``, which is
    Copyright 2024 Li, Ziyao -- Licensed under the Apache License, Version 2.0
    (http://www.apache.org/licenses/LICENSE-2.0); distributed there on an "AS IS" BASIS, WITHOUT WARRANTIES OR
    CONDITIONS OF ANY KIND.
The state_dict / constructor contract is what forces the shared lines; the forward and backward
are this package's HIP kernels.
"""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops


class SplineLinear(nn.Linear):
    """Bias-free linear map over the (in major, grid minor) RBF columns; trunc-normal init."""

    def __init__(self, in_features: int, out_features: int, init_scale: float = 0.1, **kw) -> None:
        self.init_scale = init_scale
        super().__init__(in_features, out_features, bias=False, **kw)

    def reset_parameters(self) -> None:
        nn.init.trunc_normal_(self.weight, mean=0, std=self.init_scale)


class RadialBasisFunction(nn.Module):
    """Holder of the RBF centres (``grid``, a frozen Parameter as in the reference so it shows up
    in ``parameters()`` / ``state_dict()``) and the common width ``denominator``."""

    def __init__(self, grid_min: float = -2., grid_max: float = 2., num_grids: int = 8,
                 denominator: float = None):
        super().__init__()
        self.grid_min, self.grid_max, self.num_grids = grid_min, grid_max, num_grids
        self.grid = nn.Parameter(torch.linspace(grid_min, grid_max, num_grids), requires_grad=False)
        self.denominator = denominator or (grid_max - grid_min) / (num_grids - 1)


class FastKANLayer(nn.Module):
    def __init__(self, input_dim: int, output_dim: int, grid_min: float = -2., grid_max: float = 2.,
                 num_grids: int = 8, use_base_update: bool = True, use_layernorm: bool = True,
                 base_activation=F.silu, spline_weight_init_scale: float = 0.1) -> None:
        super().__init__()
        if use_base_update and base_activation is not F.silu:
            raise NotImplementedError("the fused kernel implements the SiLU base branch only")
        self.input_dim, self.output_dim = input_dim, output_dim
        self.layernorm = None
        if use_layernorm:
            assert input_dim > 1, "Do not use layernorms on 1D inputs. Set `use_layernorm=False`."
            self.layernorm = nn.LayerNorm(input_dim)
        self.rbf = RadialBasisFunction(grid_min, grid_max, num_grids)
        self.spline_linear = SplineLinear(input_dim * num_grids, output_dim, spline_weight_init_scale)
        self.use_base_update = use_base_update
        self.precision = None                     # None -> ops.default_precision()
        if use_base_update:
            self.base_activation = base_activation
            self.base_linear = nn.Linear(input_dim, output_dim)

    def forward(self, x, use_layernorm=True):
        if ops.layer_inputs_visible():
            _collect(self, x, use_layernorm)
        return self._forward(x, use_layernorm)

    def _forward(self, x, use_layernorm=True):
        """the layer itself, without the statistics of a ``collect_edge_l1`` block (the chain walks of ``FastKAN.edge_l1`` /
        ``FastKAN.regularization_loss`` are not the model's forward)"""
        lead = x.shape[:-1]
        x2 = x.reshape(-1, x.shape[-1])
        ln = self.layernorm if (self.layernorm is not None and use_layernorm) else None
        y = ops.fastkan_layer(
            x2,
            None if ln is None else ln.weight, None if ln is None else ln.bias,
            self.spline_linear.weight,
            self.base_linear.weight if self.use_base_update else None,
            self.base_linear.bias if self.use_base_update else None,
            self.rbf.grid, self.rbf.denominator, 1e-5 if ln is None else ln.eps, self.precision)
        return y.reshape(*lead, self.output_dim)

    # ------------------------------------------------------------------ the edge functions phi_{o,i}
    #   phi_{o,i}(n) = sum_g spline_linear.weight[o, i*G+g] rbf_g(u[n,i]) + base_linear.weight[o,i] silu(x[n,i]),  u = layernorm(x) or x;
    #   forward(x)[n,o] = sum_i phi_{o,i}(n) + base_linear.bias[o]
    def _edge_weights(self):
        return self.spline_linear.weight, (self.base_linear.weight if self.use_base_update else None)

    def edge_l1(self, x: torch.Tensor, use_layernorm: bool = True) -> torch.Tensor:
        """``[out, in]``: the mean magnitude ``mean_n |phi_{o,i}(n)|`` of every edge's activation over the rows of ``x`` -- what the
        KAN paper's regulariser is defined on, and what tells which inputs / edges a trained layer uses.  One fused kernel
        (``ops.fastkan_edge_abs_sum``): no [N, out, in] tensor.  Differentiable."""
        x2 = x.reshape(-1, x.shape[-1])
        assert x2.size(1) == self.input_dim
        ln = self.layernorm if (self.layernorm is not None and use_layernorm) else None
        sw, bw = self._edge_weights()
        S = ops.fastkan_edge_abs_sum(x2, None if ln is None else ln.weight, None if ln is None else ln.bias, sw, bw,
                                     self.rbf.grid, self.rbf.denominator, 1e-5 if ln is None else ln.eps)
        return S / max(x2.size(0), 1)

    @torch.no_grad()
    def edge_curves(self, points: torch.Tensor, base_points: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``[P, out, in]``: every edge function sampled at ``points`` (``[P]``, shared by all inputs, or ``[P, in]``): the RBFs'
        argument, i.e. the value after the layernorm.  ``base_points``: other abscissae for the base branch, which sees the
        row before the layernorm (``None``: ``points``)."""
        sw, bw = self._edge_weights()
        return ops.fastkan_edge_curves(points, sw, bw, self.rbf.grid, self.rbf.denominator, base_points)

    def suggest_symbolic(self, x: torch.Tensor, functions=None, topk: int = 3, max_rows: int = 4096, use_layernorm: bool = True,
                         **search):
        """``KANLinear.suggest_symbolic`` for this layer, on ``edge_curves``.  With a LayerNorm the FIT VARIABLE is the normalised
        input ``u = layernorm(x)``, as in ``edge_curves``: ``phi_{o,i} ~ c f(a u_i + b) + d``, the base branch evaluated at the row
        before the norm.  ``SymbolicSuggestion.x`` holds ``u``."""
        from .symbolic import suggest_fastkan
        return suggest_fastkan(self, x, functions, topk, max_rows, use_layernorm, **search)

    @torch.no_grad()
    def plot_curve(self, input_index: int, output_index: int, num_pts: int = 1000, num_extrapolate_bins: int = 2):
        """The reference's ``plot_curve`` (fastkan.py:87-115): ``(x, y)`` with ``x = linspace(grid_min - N_e h, grid_max + N_e h,
        num_pts)`` and ``y`` the spline branch of edge ``(output_index, input_index)`` there -- that column of ``edge_curves``
        without the base branch, evaluated for this one edge.  Both on the layer's device."""
        ng, h = self.rbf.num_grids, self.rbf.denominator
        assert input_index < self.input_dim
        assert output_index < self.output_dim
        w = self.spline_linear.weight[output_index:output_index + 1, input_index * ng:(input_index + 1) * ng]
        x = torch.linspace(self.rbf.grid_min - num_extrapolate_bins * h, self.rbf.grid_max + num_extrapolate_bins * h, num_pts,
                           dtype=w.dtype, device=w.device)
        y = ops.fastkan_edge_curves(x, w, None, self.rbf.grid, h)
        return x, y.reshape(-1)

    def regularization_loss(self, x: torch.Tensor, regularize_activation=1.0, regularize_entropy=1.0):
        """The KAN paper's L1 + entropy regulariser on the edge activations of the layer's input ``x``: the formula of
        ``KANLinear.regularization_loss(x=)`` with ``mag = edge_l1(x)``.  (``x`` is required: the reference has no weight
        stand-in for FastKAN.)  Like that formula, an all-zero ``mag`` (zero weights, no rows) gives 0 / 0 = NaN for the loss and
        its gradients."""
        mag = self.edge_l1(x)
        total = mag.sum()
        share = mag / total
        return regularize_activation * total - regularize_entropy * torch.sum(share * share.log())


class FastKAN(nn.Module):
    def __init__(self, layers_hidden: List[int], grid_min: float = -2., grid_max: float = 2.,
                 num_grids: int = 8, use_base_update: bool = True, base_activation=F.silu,
                 spline_weight_init_scale: float = 0.1) -> None:
        super().__init__()
        self.layers = nn.ModuleList(
            FastKANLayer(a, b, grid_min=grid_min, grid_max=grid_max, num_grids=num_grids,
                         use_base_update=use_base_update, base_activation=base_activation,
                         spline_weight_init_scale=spline_weight_init_scale)
            for a, b in zip(layers_hidden[:-1], layers_hidden[1:]))

    def forward(self, x):
        for layer in self.layers:
            x = layer(x)
        return x

    def regularization_loss(self, x: torch.Tensor, regularize_activation=1.0, regularize_entropy=1.0):
        """``x``: the chain's input -- every layer is regularised on the activations of ITS input (the chain is walked)"""
        total = 0.0
        for i, layer in enumerate(self.layers):
            total = total + layer.regularization_loss(x, regularize_activation, regularize_entropy)
            if i + 1 < len(self.layers):
                x = layer._forward(x)             # (not a forward of the model: a collect_edge_l1 block does not record it)
        return total

    def edge_l1(self, x: torch.Tensor) -> List[torch.Tensor]:
        """``FastKANLayer.edge_l1`` of every layer on its own input, ``x`` being the chain's"""
        out = []
        for i, layer in enumerate(self.layers):
            out.append(layer.edge_l1(x))
            if i + 1 < len(self.layers):
                x = layer._forward(x)
        return out

    def suggest_symbolic(self, x: torch.Tensor, **kw) -> list:
        """``FastKANLayer.suggest_symbolic`` of every layer on its own input, ``x`` being the chain's"""
        from .symbolic import suggest_chain
        return suggest_chain(self, x, **kw)


class AttentionWithFastKANTransform(nn.Module):
    """Multi-head attention whose five linear maps are ``FastKANLayer``s and whose additive ``bias`` enters AFTER the softmax
    (the reference's formula, fastkan.py:182-198).  ``q [*, Q, q_dim]``, ``k [*, K, k_dim]``, ``v [*, K, v_dim]``, ``bias``
    broadcastable to ``[*, Q, K]`` -> ``[*, Q, q_dim]``.  With ``gating`` the heads' output is multiplied by
    ``sigmoid(linear_g(q))`` (the gate sees the raw ``q``) before ``linear_o``."""

    def __init__(self, q_dim: int, k_dim: int, v_dim: int, head_dim: int, num_heads: int, gating: bool = True):
        super().__init__()
        self.num_heads = num_heads
        total_dim = head_dim * self.num_heads
        self.gating = gating
        self.linear_q = FastKANLayer(q_dim, total_dim)
        self.linear_k = FastKANLayer(k_dim, total_dim)
        self.linear_v = FastKANLayer(v_dim, total_dim)
        self.linear_o = FastKANLayer(total_dim, q_dim)
        self.linear_g = None
        if self.gating:
            self.linear_g = FastKANLayer(q_dim, total_dim)
        self.norm = head_dim ** -0.5

    def forward(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, bias: torch.Tensor = None) -> torch.Tensor:
        wq, wk, wv = self.linear_q(q), self.linear_k(k), self.linear_v(v)
        g = None if self.linear_g is None else self.linear_g(q)
        nq, nk = q.shape[-2], k.shape[-2]
        lead = torch.broadcast_shapes(q.shape[:-2], k.shape[:-2], v.shape[:-2])
        # equal leading dimensions: views.  Anything else that broadcasts is expanded and materialised here, after the projections
        # (autograd sums the copies back)
        rows = lambda t: t.expand(*lead, *t.shape[-2:]).reshape(-1, *t.shape[-2:])
        if bias is not None:
            bias = bias.expand(*lead, nq, nk).reshape(-1, nq, nk)        # (one leading dimension: still the stride-0 view)
        o = ops.dense_attention(rows(wq), rows(wk), rows(wv), self.num_heads, self.norm, bias, None if g is None else rows(g))
        return self.linear_o(o.reshape(*lead, nq, o.shape[-1]))


def _collect(layer: FastKANLayer, x: torch.Tensor, use_layernorm: bool) -> None:
    """inside ``kagnn_amd.collect_edge_l1`` blocks of this thread: ``edge_l1`` of the input ``forward`` sees, with its ``use_layernorm``"""
    for entry in ops._edge_collectors():
        name = entry[0].get(id(layer))
        if name is None:
            continue
        if len(entry) > 2:
            entry[2](name, layer, x, use_layernorm)       # a kagnn_amd.suggest_symbolic walk: it wants the input, not the statistics
        else:
            entry[1][name] = layer.edge_l1(x if x.dtype == torch.float32 else x.float(), use_layernorm)
