"""efficient-KAN layers with the reference's module surface, computed by libkagnn_hip.so.

Drop-in for ``node_classification_clean/ekan.py`` (``KANLinear`` :7-233, ``KAN`` :236-281 of
the reference): same constructor signatures, same parameter / buffer names and shapes
(``base_weight, spline_weight, spline_scaler, grid``), so ``state_dict()`` round-trips with the
reference.  ``forward`` does not run torch ops: it calls ``kagnn_kan_linear_fwd`` (and the two
backward entry points through autograd) -- see ``kagnn_amd.ops``.

Only parameter *initialisation* runs host-side torch code (a one-off least-squares fit, like the
reference's ``reset_parameters`` :57-77); it is not on the hot path.
"""
from __future__ import annotations

import contextlib
import math
import os
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional, Sequence

import torch
from torch import nn

from . import ops


_FIXED_CHUNK_ELEMENTS = 1 << 22      # [rows, fixed edges] values per chunk when a layer's fixed symbolic edges are evaluated in torch ops
_PACK_CHAIN = True      # all layers of a chain packed in one launch (a module attribute for the bitwise A/B tests, no longer an environment switch)


class EdgeStats(NamedTuple):
    """``KANLinear.edge_stats``: mean and standard deviation of every edge function over the rows, both ``[out, in]``"""
    mean: torch.Tensor
    std: torch.Tensor


@dataclass
class Attribution:
    """``KAN.attribute``: per layer ``edge_std [out_l, in_l]`` (the edge functions' standard deviation on the layer's input),
    ``out_std [out_l]`` (the layer outputs' standard deviation), ``edge_scores [out_l, in_l]``; ``node_scores``: one vector per width,
    ``L + 1`` of them, the first being the chain's input features.  ``input``: the chain's input when the caller asked to keep it."""
    edge_std: List[torch.Tensor]
    out_std: List[torch.Tensor]
    edge_scores: List[torch.Tensor]
    node_scores: List[torch.Tensor]
    input: Optional[torch.Tensor] = None

    @property
    def input_scores(self) -> torch.Tensor:
        return self.node_scores[0]


@dataclass
class PruneReport:
    """``kagnn_amd.prune``: per chain name ``{"keep": [index tensor per interior width], "edges": [pruned (o, i) rows per layer],
    "widths_before": [...], "widths_after": [...]}`` -- host data; ``apply_pruning`` replays it on a fresh model"""
    chains: Dict[str, dict] = field(default_factory=dict)


def _init_bases(points: torch.Tensor, knots: torch.Tensor, order: int) -> torch.Tensor:
    """Dense B-spline collocation matrix for the init-time fit only (G+1 sample points).
    points [M, in], knots [in, G+2k+1] -> [M, in, G+k]."""
    p = points.unsqueeze(-1)
    b = ((p >= knots[:, :-1]) & (p < knots[:, 1:])).to(points.dtype)
    for d in range(1, order + 1):
        left = (p - knots[:, : -(d + 1)]) / (knots[:, d:-1] - knots[:, : -(d + 1)])
        right = (knots[:, d + 1:] - p) / (knots[:, d + 1:] - knots[:, 1:-d])
        b = left * b[..., :-1] + right * b[..., 1:]
    return b


class KANLinear(nn.Module):
    """``y = silu(x) @ base_weight.T + B(x) @ (spline_weight * spline_scaler[..., None]).T``

    ``B(x)`` are the ``grid_size + spline_order`` uniform B-spline bases per input feature; they
    are evaluated in registers inside the HIP kernel and never stored.

    ``fix_symbolic`` replaces single edges by ``c f(a x + b) + d`` (INTEGRATION.md "Fixed symbolic edges"); a layer that never fixed
    an edge has the reference's state and routes.
    """
    _symbolic = None        # (also for a module unpickled from before the attribute existed)

    def __init__(self, in_features, out_features, grid_size=5, spline_order=3, scale_noise=0.1,
                 scale_base=1.0, scale_spline=1.0, enable_standalone_scale_spline=True,
                 base_activation=torch.nn.SiLU, grid_eps=0.02, grid_range=[-1, 1]):
        super().__init__()
        if base_activation is not torch.nn.SiLU:
            raise NotImplementedError("the fused kernel implements the SiLU base branch only "
                                      "(the only activation KAGNN uses)")
        if not 1 <= spline_order <= ops.MAX_SPLINE_ORDER:
            raise NotImplementedError(f"spline_order must be in 1..{ops.MAX_SPLINE_ORDER}")
        if ops.high_order(spline_order) and grid_size + 2 * spline_order + 1 > ops.HIGH_ORDER_MAX_KNOTS:
            raise NotImplementedError(f"grid_size + 2 * spline_order + 1 must be <= {ops.HIGH_ORDER_MAX_KNOTS} at spline_order above 4 "
                                      f"(got {grid_size + 2 * spline_order + 1})")
        self.in_features = in_features
        self.out_features = out_features
        self.grid_size = grid_size
        self.spline_order = spline_order
        self.scale_noise = scale_noise
        self.scale_base = scale_base
        self.scale_spline = scale_spline
        self.enable_standalone_scale_spline = enable_standalone_scale_spline
        self.base_activation = base_activation()
        self.grid_eps = grid_eps
        self.precision: Optional[int] = None      # None -> ops.default_precision()

        step = (grid_range[1] - grid_range[0]) / grid_size
        row = torch.arange(-spline_order, grid_size + spline_order + 1) * step + grid_range[0]
        self.register_buffer("grid", row.expand(in_features, -1).contiguous())

        coeffs = grid_size + spline_order
        self.base_weight = nn.Parameter(torch.empty(out_features, in_features))
        self.spline_weight = nn.Parameter(torch.empty(out_features, in_features, coeffs))
        if enable_standalone_scale_spline:
            self.spline_scaler = nn.Parameter(torch.empty(out_features, in_features))
        self._knots_key = None
        self._knots_row = None
        self._symbolic: Optional[ops.SymbolicEdges] = None     # the list of fixed symbolic edges (fix_symbolic); None: the reference's layer
        self.reset_parameters()
        self.refresh_knots()

    # ------------------------------------------------------------------ init (host side)
    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.base_weight, a=math.sqrt(5) * self.scale_base)
        with torch.no_grad():
            k = self.spline_order
            noise = (torch.rand(self.grid_size + 1, self.in_features, self.out_features) - 0.5)
            noise = noise * self.scale_noise / self.grid_size
            fit = self.curve2coeff(self.grid.T[k:-k], noise)
            if not self.enable_standalone_scale_spline:
                fit = fit * self.scale_spline
            self.spline_weight.copy_(fit)
            if self.enable_standalone_scale_spline:
                nn.init.kaiming_uniform_(self.spline_scaler, a=math.sqrt(5) * self.scale_spline)

    def curve2coeff(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """Least-squares spline coefficients through samples ``y[M,in,out]`` at ``x[M,in]``."""
        assert x.dim() == 2 and x.size(1) == self.in_features
        assert y.size() == (x.size(0), self.in_features, self.out_features)
        lhs = _init_bases(x, self.grid, self.spline_order).permute(1, 0, 2)   # [in, M, C]
        sol = torch.linalg.lstsq(lhs, y.permute(1, 0, 2)).solution            # [in, C, out]
        return sol.permute(2, 0, 1).contiguous()

    @property
    def scaled_spline_weight(self):
        if self.enable_standalone_scale_spline:
            return self.spline_weight * self.spline_scaler.unsqueeze(-1)
        return self.spline_weight

    # ------------------------------------------------------------------ hot path
    def _knots(self) -> torch.Tensor:
        if torch.compiler.is_compiling():
            # dynamo cannot trace the data_ptr-keyed cache below or its host-side uniformity check: traced code reads what
            # ``refresh_knots`` left.  Every eager site that writes the grid (the constructor, update_grid, refine, state loading,
            # a move to another device or dtype) calls it, so no eager forward is needed first; only a direct write to
            # ``layer.grid`` must be followed by ``layer.refresh_knots()``
            row = self._knots_row
            if row is None or row.device != self.grid.device or row.size(-1) != self.grid.size(1):
                raise RuntimeError("KANLinear under torch.compile: the knots cache does not belong to this grid; call "
                                   "layer.refresh_knots() (or run the layer once eagerly) after writing to layer.grid")
            return row
        g = self.grid
        key = (g.data_ptr(), g._version, g.device)          # (the device object itself: str() of it was 1.5 us x 13 calls per graph-level step)
        if key != self._knots_key:
            self._knots_row = self._knots_of(g)
            self._knots_key = key
        return self._knots_row

    @staticmethod
    def _knots_of(g: torch.Tensor) -> torch.Tensor:
        """what the kernels take for the grid buffer ``g``: its first row when all rows are that one uniform row, else the whole
        buffer (per-feature knot rows), fp32"""
        row = g[0].detach().to(torch.float32)
        steps = row[1:] - row[:-1]
        h = float(steps.mean())
        same = bool((g == row).all()) and bool(((steps - h).abs() <= 1e-4 * abs(h)).all()) and h > 0
        if same:
            return row.contiguous().clone()
        # adaptive grid (update_grid was called): the whole buffer, per-feature knot rows
        if not bool((g[:, 1:] > g[:, :-1]).all()):
            raise ValueError("KANLinear.grid rows must be strictly increasing")
        return g.detach().to(torch.float32).contiguous().clone()

    def refresh_knots(self) -> None:
        """Bring the knots cache in line with ``self.grid`` now (host code: it reads the grid).  Eager forwards do this on their
        own; a compiled forward cannot, so every method of the layer that writes the grid ends with this call.  A grid whose rows
        are not strictly increasing leaves the cache empty: the next forward raises, as it always did."""
        self._knots_key = self._knots_row = None
        g = self.grid
        if g.is_meta or torch.compiler.is_compiling():
            return
        try:
            self._knots_row = self._knots_of(g)
        except ValueError:
            return
        self._knots_key = (g.data_ptr(), g._version, g.device)

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)          # .to() / .cuda() / .float(): the cache is a plain attribute and does not move
        self.refresh_knots()
        if self._symbolic is not None and self._symbolic.device != self.symbolic_index.device:
            self._symbolic = ops.SymbolicEdges.from_sorted(self._symbolic.triples, self.in_features, self.out_features,
                                                           self.symbolic_index.device)
        return out

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        index = state_dict.get(prefix + "symbolic_index")
        if index is None:
            self._drop_symbolic_state()                    # the checkpoint's layer has no fixed edge
        else:                                              # make room for the checkpoint's list, whatever this layer holds
            dev = self.base_weight.device
            self._drop_symbolic_state()
            self.symbolic_affine = nn.Parameter(torch.zeros((index.size(0), 4), dtype=torch.float32, device=dev))
            self.register_buffer("symbolic_index", torch.zeros((index.size(0), 3), dtype=torch.int32, device=dev))
            self.register_buffer("symbolic_keep", torch.ones((self.out_features, self.in_features), dtype=torch.float32, device=dev))
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)     # a checkpoint's grid may hold per-feature rows
        if index is not None:
            self._symbolic = ops.SymbolicEdges.from_sorted(self.symbolic_index.cpu().tolist(), self.in_features, self.out_features,
                                                           self.symbolic_index.device)
        self.refresh_knots()

    def forward(self, x: torch.Tensor, _packed=None) -> torch.Tensor:
        assert x.dim() == 2 and x.size(1) == self.in_features
        if ops.layer_inputs_visible():
            walk = ops._refine_walk()
            if walk is not None:
                walk.visit(self, x)                # a refine_grids walk: the layer moves to the finer grid BEFORE it evaluates x
                _packed = None
            _collect(self, x)
        return self._forward(x, _packed)

    def _forward(self, x: torch.Tensor, _packed=None) -> torch.Tensor:
        """the layer itself, without the statistics of a ``collect_edge_l1`` block (the chain walks of ``KAN.edge_l1`` /
        ``KAN.regularization_loss(x=)`` are not the model's forward)"""
        if self._symbolic is not None:
            return self._forward_fixed(x)
        return ops.kan_linear(x, self.base_weight, self.spline_weight, self._scaler(), self._knots(),
                              self.grid_size, self.spline_order, self.precision, _packed)

    def _scaler(self):
        return self.spline_scaler if self.enable_standalone_scale_spline else None

    def _plain_knots(self):
        """What every host path that hands this layer's raw parameters to a library call asks (the one-call layer / stack / model
        nodes, the chain pack, the one-launch read-out): is the forward exactly ``ops.kan_linear`` on them over ONE uniform knot
        vector at orders 1..4?  That vector, else ``None`` (fixed symbolic edges, orders above 4, per-feature knot rows).  A feature
        that changes what a layer computes adds its condition HERE."""
        if self._symbolic is not None or self.spline_order > ops.FUSED_MAX_SPLINE_ORDER:      # (ops.high_order, without the call)
            return None
        knots = self._knots()
        return knots if knots.dim() == 1 else None

    def _refuse_fixed_edges(self, what: str) -> None:
        if self._symbolic is not None:       # for a caller that keeps copies or slices of the raw parameters: they could not tell
            raise NotImplementedError(f"a KANLinear with fixed symbolic edges cannot be {what} (unfix_symbolic first)")

    def _fast_operands(self):
        """``(base_weight, spline_weight, spline_scaler or None, knots)`` of a layer ``_plain_knots`` accepts, else ``None``"""
        knots = self._plain_knots()
        return None if knots is None else (self.base_weight, self.spline_weight, self._scaler(), knots)

    def _kept_operands(self):
        """``(base_weight, spline_weight, spline_scaler)`` with the fixed edges switched off: small torch ops on ``symbolic_keep``, so the
        fixed edges' entries get exactly zero gradient"""
        keep, scaler = self.symbolic_keep, self._scaler()
        if scaler is not None:
            return self.base_weight * keep, self.spline_weight, scaler * keep
        return self.base_weight * keep, self.spline_weight * keep.unsqueeze(-1), None

    def _forward_fixed(self, x: torch.Tensor) -> torch.Tensor:
        """the layer with fixed symbolic edges: ``ops.kan_linear`` on the kept spline edges, then ``ops.symbolic_edges`` adds the
        formulas to its output (any spline order: the symbolic kernel does not see the spline)"""
        if torch.compiler.is_compiling():
            raise NotImplementedError("a KANLinear with fixed symbolic edges is not supported under torch.compile (unfix_symbolic first)")
        bw, sw, sc = self._kept_operands()
        y = ops.kan_linear(x, bw, sw, sc, self._knots(), self.grid_size, self.spline_order, self.precision)
        return ops.symbolic_edges(x, self._symbolic, self.symbolic_affine, self.out_features, y=y)

    def read_out_blocks_in_one_launch(self, widths) -> bool:
        """would ``forward_parts`` over fp32 blocks of these widths run as one forward launch (``kagnn_kan_fwd_parts_ok``)?"""
        mode = self.precision if self.precision is not None else ops.default_precision()
        return (self._plain_knots() is not None and ops.split_like(mode) and sum(widths) == self.in_features
                and ops.parts_one_launch_widths_ok(tuple(int(w) for w in widths), self.out_features, self.grid_size, self.spline_order, mode))

    def forward_parts(self, parts, skip_gradients=None) -> torch.Tensor:
        """``forward(torch.cat(parts, dim=1))`` without the concatenation (``ops.kan_linear_parts``)."""
        fast = None if ops.layer_inputs_visible() else self._fast_operands()
        if fast is None:
            # not the plain layer (_plain_knots): keep it simple; a collect_edge_l1 block: forward() must see the input
            return self.forward(ops.concat_columns([t.materialise() if isinstance(t, ops.AffineRows) else t for t in parts]))
        return ops.kan_linear_parts(parts, *fast, self.grid_size, self.spline_order, self.precision, skip_gradients)

    # ------------------------------------------------------------------ not on the KAGNN path
    def b_splines(self, x: torch.Tensor) -> torch.Tensor:
        """Dense bases ``[N, in, G+k]`` on this layer's grid (``ekan.py:79-112``); the forward never builds it."""
        assert x.dim() == 2 and x.size(1) == self.in_features
        return ops.kan_bsplines(x, self.grid, self.grid_size, self.spline_order)

    @torch.no_grad()
    def update_grid(self, x: torch.Tensor, margin=0.01):
        """Move the knots to the batch's per-feature quantiles (blended with a uniform grid by ``grid_eps``) and
        refit the coefficients so the layer's curves are kept, ``ekan.py:164-211``.  The knot arithmetic is a
        handful of [G+1, in] torch ops in the reference's order; the refit is one device call,
        ``ops.kan_grid_refit``, at every ``grid_size + spline_order`` the layer accepts (up to 46) -- no [N, in, out]
        intermediate.  The layer then runs on per-feature knots."""
        assert x.dim() == 2 and x.size(1) == self.in_features
        if ops.high_order(self.spline_order):
            # a decision, not an omission: the reference's own refit (fp64 least squares) breaks down from order 12 -- fitted
            # coefficients of 1e7..1e10, a function residual above the function at (G, k) = (16, 16) and (2, 16), and its fp64 solve
            # and the normal equations disagreeing by 100 % -- so there is nothing to hold a device refit to
            raise NotImplementedError("update_grid is not implemented at spline_order above 4: the least-squares refit of the "
                                      "coefficients is ill-conditioned at these orders (the reference's own fp64 refit loses the "
                                      "function from order 12). A layer whose grid buffer already holds per-feature knot rows runs.")
        g, k = self.grid_size, self.spline_order
        new_grid = self._quantile_knots(x, g, margin)
        fitted = ops.kan_grid_refit(x, self.grid, new_grid, self.spline_weight, self._scaler(), g, k)
        self.grid.copy_(new_grid)
        self.spline_weight.data.copy_(fitted)
        self.refresh_knots()

    def _quantile_knots(self, x: torch.Tensor, g: int, margin: float) -> torch.Tensor:
        """``update_grid``'s knot rule (``ekan.py:180-205``) for ``g`` intervals: ``[in, g+2k+1]``"""
        n, k, dev = x.size(0), self.spline_order, x.device
        ranked = torch.sort(x, dim=0).values
        quantiles = ranked[torch.linspace(0, n - 1, g + 1, dtype=torch.int64, device=dev)]       # [G+1, in]
        step = (ranked[-1] - ranked[0] + 2 * margin) / g
        even = torch.arange(g + 1, dtype=torch.float32, device=dev).unsqueeze(1) * step + ranked[0] - margin
        inner = self.grid_eps * even + (1 - self.grid_eps) * quantiles
        below = inner[:1] - step * torch.arange(k, 0, -1, device=dev).unsqueeze(1)
        above = inner[-1:] + step * torch.arange(1, k + 1, device=dev).unsqueeze(1)
        return torch.cat([below, inner, above], dim=0).T.contiguous()

    @torch.no_grad()
    def refine(self, x: torch.Tensor, grid_size: int, adaptive: bool = False, grid_range=None, margin=0.01) -> torch.Tensor:
        """Grid extension (KAN paper, section 2.4): move the layer onto a grid of ``grid_size`` intervals -- finer, or coarser -- and
        refit the coefficients on the rows of ``x`` (the layer's own input) so that its curves are kept; one device call,
        ``ops.kan_grid_resize``, up to 46 coefficients.  Returns ``untouched [in]``: per input feature, the new bases no row reached.

        ``adaptive=False``: every feature's new knot row is uniform over its current inner range ``[grid[f, k], grid[f, -k-1]]`` (or
        ``grid_range``), extended by ``k`` steps either side as the constructor does; a layer on one shared uniform row stays on one
        (and so on the split / sparse kernels).  Only rows inside the new inner range take part in the fit: beyond it the finer
        space cannot represent the old curve, and the misfit of such rows would leak into the range (6e-2 of the function for
        0.8 randn inputs on [-1, 1], against 4e-8 with the window).  ``adaptive=True``: ``update_grid``'s quantile knots (``grid_eps``,
        ``margin``) at the new size, every row taking part.

        The UNSCALED coefficients are fitted and ``spline_scaler`` is kept: the scaling is linear per edge, so the layer's function
        is kept (``update_grid`` folds the scaler into the fit and keeps it too, as the reference does; that is not copied here).
        ``grid`` and ``spline_weight`` become NEW tensors of the new shapes: an optimizer built on the old Parameter must be rebuilt."""
        assert x.dim() == 2 and x.size(1) == self.in_features
        k, g_new = self.spline_order, int(grid_size)
        if ops.high_order(k):
            raise NotImplementedError("refine is not implemented at spline_order above 4: like update_grid's, the least-squares refit "
                                      "of the coefficients is ill-conditioned at these orders (the reference's own fp64 refit loses "
                                      "the function from order 12)")
        if g_new < 1 or g_new + 2 * k + 1 > ops.MAX_KNOTS:
            raise ValueError(f"refine: grid_size must be >= 1 with grid_size + 2 * spline_order + 1 <= {ops.MAX_KNOTS} "
                             f"(got {grid_size} at spline_order {k})")
        ops._need_cuda(x, self.grid, self.spline_weight)
        dev = x.device
        if adaptive:
            new_grid, window = self._quantile_knots(x, g_new, margin), None
        else:
            steps = torch.arange(-k, g_new + k + 1)
            if grid_range is not None or self._knots().dim() == 1:        # one shared uniform row, built as the constructor builds it
                lo, hi = (float(self.grid[0, k]), float(self.grid[0, -k - 1])) if grid_range is None else (float(grid_range[0]), float(grid_range[1]))
                if not hi > lo:
                    raise ValueError("refine: grid_range must be increasing")
                row = steps * ((hi - lo) / g_new) + lo
                new_grid = row.to(device=dev, dtype=torch.float32).expand(self.in_features, -1).contiguous()
            else:                                                           # per-feature rows: each over its own inner range
                lo, hi = self.grid[:, k].float(), self.grid[:, -k - 1].float()
                new_grid = (lo.unsqueeze(1) + steps.to(dev).float().unsqueeze(0) * ((hi - lo) / g_new).unsqueeze(1)).contiguous()
            window = torch.stack([new_grid[:, k], new_grid[:, -k - 1]], dim=1).contiguous()
        fitted, untouched = ops.kan_grid_resize(x, self.grid, new_grid, self.spline_weight, None, self.grid_size, g_new, k, window)
        old = self.spline_weight
        self.grid = new_grid.to(self.grid.dtype)
        self.spline_weight = nn.Parameter(fitted.to(old.dtype), requires_grad=old.requires_grad)
        self.grid_size = g_new
        self.refresh_knots()
        return untouched

    # ------------------------------------------------------------------ the edge functions phi_{o,i}
    def _edge_args(self):
        return self.base_weight, self.spline_weight, self._scaler(), self._knots(), self.grid_size, self.spline_order

    def edge_l1(self, x: torch.Tensor) -> torch.Tensor:
        """``[out, in]``: the mean magnitude ``mean_n |phi_{o,i}(x[n,i])|`` of every edge's activation over the rows of ``x`` --
        what the KAN paper's regulariser is defined on, and what tells which inputs / edges a trained layer uses.  One fused
        kernel (``ops.kan_edge_abs_sum``): no [N, out, in] tensor.  Differentiable.  Spline orders 1..4."""
        assert x.dim() == 2 and x.size(1) == self.in_features
        if self._symbolic is not None:
            # the layer as it now is: the kept spline edges, and mean |c f(a x + b) + d| of the fixed ones ("0": nothing)
            from .symbolic import fixed_edge_values
            rows = max(x.size(0), 1)
            mag = ops.kan_edge_abs_sum(x, *self._kept_operands(), *self._edge_args()[3:]) / rows
            idx = self.symbolic_index.long()
            if idx.size(0) == 0 or x.size(0) == 0:
                return mag
            step = max(1, _FIXED_CHUNK_ELEMENTS // idx.size(0))
            total = sum(fixed_edge_values(x[r:r + step], self._symbolic.triples, self.symbolic_affine).abs().sum(0)
                        for r in range(0, x.size(0), step))
            return mag.index_put((idx[:, 0], idx[:, 1]), total / rows)
        return ops.kan_edge_abs_sum(x, *self._edge_args()) / max(x.size(0), 1)

    @torch.no_grad()
    def edge_curves(self, points: torch.Tensor) -> torch.Tensor:
        """``[P, out, in]``: every edge function sampled at ``points`` (``[P]``, shared by all inputs, or ``[P, in]``) -- the
        reference's ``plot_curve`` (``fastkan.py``) for all edges at once.  Fixed symbolic edges show their formula (``"0"``: 0)."""
        if self._symbolic is not None:
            from .symbolic import fixed_edge_values
            phi = ops.kan_edge_curves(points, *self._kept_operands(), *self._edge_args()[3:])
            idx = self.symbolic_index.long()
            if idx.size(0):
                pts = points.to(phi.dtype)
                pts = pts.reshape(-1, 1).expand(-1, self.in_features) if pts.dim() == 1 else pts
                phi[:, idx[:, 0], idx[:, 1]] = fixed_edge_values(pts, self._symbolic.triples, self.symbolic_affine.detach())
            return phi
        return ops.kan_edge_curves(points, *self._edge_args())

    @torch.no_grad()
    def edge_stats(self, x: torch.Tensor, unbiased: bool = True) -> EdgeStats:
        """``EdgeStats(mean, std)``, both ``[out, in]``: mean and standard deviation of ``phi_{o,i}(x[n,i])`` over the rows of ``x`` -- the
        centred scale of every edge that attribution scores are built on (pykan's ``edge_actscale``).  ``std = sqrt(m2 / (N - 1))`` as
        ``torch.std`` (``unbiased=False``: ``/ N``); one row gives NaN under ``unbiased=True``, as torch does.  One fused kernel
        (``ops.kan_edge_moments``): no [N, out, in] tensor.  A layer with fixed symbolic edges is described as it now is: the fixed
        functions' own moments, ``"0"`` edges exactly 0.  Not differentiable.  Spline orders 1..4."""
        assert x.dim() == 2 and x.size(1) == self.in_features
        x = x.detach() if x.dtype == torch.float32 else x.detach().float()
        n = x.size(0)
        if self._symbolic is None:
            mean, m2 = ops.kan_edge_moments(x, *self._edge_args())
        else:
            from .symbolic import fixed_edge_values
            mean, m2 = ops.kan_edge_moments(x, *self._kept_operands(), *self._edge_args()[3:])
            idx = self.symbolic_index.long()
            if idx.size(0) and n:
                step = max(1, _FIXED_CHUNK_ELEMENTS // idx.size(0))
                count, f_mean, f_m2 = 0, 0.0, 0.0
                for r in range(0, n, step):           # one evaluation per row chunk, the chunks merged pairwise in fp64
                    v = fixed_edge_values(x[r:r + step], self._symbolic.triples, self.symbolic_affine.detach()).double()
                    c_mean = v.mean(0)
                    delta = c_mean - f_mean
                    total = count + v.size(0)
                    f_m2 = f_m2 + (v - c_mean).square().sum(0) + delta * delta * (count * v.size(0) / total)
                    f_mean = f_mean + delta * (v.size(0) / total)
                    count = total
                mean = mean.index_put((idx[:, 0], idx[:, 1]), f_mean.float())
                m2 = m2.index_put((idx[:, 0], idx[:, 1]), f_m2.float())
        return EdgeStats(mean, (m2 / (n - 1 if unbiased else n)).sqrt())

    @torch.no_grad()
    def _keep(self, rows: Optional[torch.Tensor], cols: Optional[torch.Tensor]) -> None:
        """keep these outputs (``rows``) / inputs (``cols``), sorted int64 CPU index tensors or None: NEW Parameters and grid buffer of
        the smaller shapes; fixed edges on a removed row or column are dropped, the rest re-indexed"""
        fixed = self._fixed_state()
        dev = self.base_weight.device
        names = ("base_weight", "spline_weight") + (("spline_scaler",) if self.enable_standalone_scale_spline else ())
        for name in names:
            old = getattr(self, name)
            v = old.detach()
            if rows is not None:
                v = v.index_select(0, rows.to(dev))
            if cols is not None:
                v = v.index_select(1, cols.to(dev))
            setattr(self, name, nn.Parameter(v.contiguous(), requires_grad=old.requires_grad))
        if cols is not None:
            self.grid = self.grid.index_select(0, cols.to(dev)).contiguous()       # (it may hold per-feature knot rows)
        row_of = {int(o): j for j, o in enumerate(range(self.out_features) if rows is None else rows.tolist())}
        col_of = {int(i): j for j, i in enumerate(range(self.in_features) if cols is None else cols.tolist())}
        self.out_features, self.in_features = len(row_of), len(col_of)
        self._set_fixed({(row_of[o], col_of[i]): v for (o, i), v in fixed.items() if o in row_of and i in col_of})
        self.refresh_knots()

    def _switch_off(self, pairs) -> None:
        """``fix_symbolic(o, i, "0")`` for every ``(o, i)`` of ``pairs`` at once: one new symbolic state"""
        fixed = self._fixed_state()
        for o, i in pairs:
            fixed.setdefault(self._check_edge(o, i), ("0", None))
        self._set_fixed(fixed)

    # ------------------------------------------------------------------ fixed symbolic edges (pykan's fix_symbolic)
    def _drop_symbolic_state(self) -> None:
        self._symbolic = None
        self._parameters.pop("symbolic_affine", None)
        self._buffers.pop("symbolic_index", None)
        self._buffers.pop("symbolic_keep", None)
        self._non_persistent_buffers_set.discard("symbolic_index")
        self._non_persistent_buffers_set.discard("symbolic_keep")

    def fixed_edges(self) -> Dict[tuple, str]:
        """``{(o, i): name}`` of the fixed edges, sorted by ``(o, i)``; ``name`` is a function of ``SYMBOLIC_LIB`` or ``"0"`` (switched off)"""
        if self._symbolic is None:
            return {}
        out = {(o, i): ops.SYMBOLIC_FUNCTIONS[f] for o, i, f in self._symbolic.triples}
        for o, i in (self.symbolic_keep == 0).nonzero().cpu().tolist():
            out.setdefault((o, i), "0")
        return dict(sorted(out.items()))

    def _set_fixed(self, fixed: Dict[tuple, tuple]) -> None:
        """install ``{(o, i): (name, affine row or None)}`` as the layer's fixed edges: NEW ``symbolic_affine`` Parameter and buffers, one
        validated ``ops.SymbolicEdges``; empty: the symbolic state is removed and the layer is the reference's again"""
        dev = self.base_weight.device
        self._drop_symbolic_state()
        if not fixed:
            return
        live = sorted((o, i, ops.SYMBOLIC_FUNCTIONS.index(name)) for (o, i), (name, _) in fixed.items() if name != "0")
        edges = ops.SymbolicEdges.from_sorted(live, self.in_features, self.out_features, dev)
        rows = [fixed[(o, i)][1].detach().to(device=dev, dtype=torch.float32).reshape(4) for o, i, _ in live]
        affine = torch.stack(rows) if rows else torch.zeros((0, 4), dtype=torch.float32, device=dev)
        keep = torch.ones((self.out_features, self.in_features), dtype=torch.float32, device=dev)
        at = torch.tensor(sorted(fixed), dtype=torch.int64, device=dev).reshape(-1, 2)
        keep[at[:, 0], at[:, 1]] = 0.0
        self.symbolic_affine = nn.Parameter(affine.contiguous(), requires_grad=self.base_weight.requires_grad)
        self.register_buffer("symbolic_index", edges.index)
        self.register_buffer("symbolic_keep", keep)
        self._symbolic = edges

    def _fixed_state(self) -> Dict[tuple, tuple]:
        if self._symbolic is None:
            return {}
        rows = {(o, i): self.symbolic_affine[e] for e, (o, i, _) in enumerate(self._symbolic.triples)}
        return {k: (name, rows.get(k)) for k, name in self.fixed_edges().items()}

    def _check_edge(self, o, i) -> tuple:
        o, i = int(o), int(i)
        if not (0 <= o < self.out_features and 0 <= i < self.in_features):
            raise IndexError(f"edge ({o}, {i}) is outside a layer of {self.out_features} x {self.in_features}")
        return o, i

    def fix_symbolic(self, o: int, i: int, name: str, params=None, x: Optional[torch.Tensor] = None, max_rows: int = 4096, **search):
        """Replace edge ``(o, i)`` by ``c f(a x + b) + d`` in the forward (pykan's ``fix_symbolic``): ``name`` is a function of
        ``SYMBOLIC_LIB``, or ``"0"``, which switches the edge off with no symbolic term.  ``params = (a, b, c, d)`` is given, or fitted
        on the rows ``x [N, in]`` (the layer's own input): ``ops.symbolic_fit`` of that one function on ``edge_curves`` with
        ``suggest_symbolic``'s row rule (``max_rows``) and ``**search`` -- bit for bit the parameters ``suggest_symbolic`` reports for
        that function.  Returns the fit's ``r2``, or ``None`` when nothing was fitted.

        The four numbers are trainable (``symbolic_affine [E, 4]``, one row per fixed function edge in ``(o, i)`` order); the edge's
        spline parameters stay where they are, get exactly zero gradient while it is fixed, and are back with ``unfix_symbolic``.
        Every change of the list makes ``symbolic_affine`` a NEW Parameter: rebuild the optimizer, as after ``refine``.  The plain
        functions: ``sqrt`` / ``log`` outside their domain and ``1/x`` at 0 give what IEEE gives (pykan's singularity-protected
        variants are not provided)."""
        from .symbolic import SYMBOLIC_LIB, _rows32, strided_rows
        o, i = self._check_edge(o, i)
        if name != "0" and name not in SYMBOLIC_LIB:
            raise ValueError(f"fix_symbolic: unknown function {name!r}; the library is {', '.join(SYMBOLIC_LIB)} and \"0\"")
        r2, row = None, None
        if name != "0":
            if params is not None:
                row = torch.as_tensor(params, dtype=torch.float32).reshape(-1)
                if row.numel() != 4:
                    raise ValueError("fix_symbolic: params must be (a, b, c, d)")
            elif x is not None:
                with torch.no_grad():
                    rows = strided_rows(_rows32(x, self.in_features), max_rows)
                    fit = ops.symbolic_fit(rows, self.edge_curves(rows), (name,), **search)
                row, r2 = fit.params[0, o, i].clone(), float(fit.r2[0, o, i])
            else:
                raise ValueError("fix_symbolic: give params=(a, b, c, d), or the rows x to fit them on")
        fixed = self._fixed_state()
        fixed[(o, i)] = (name, row)
        self._set_fixed(fixed)
        return r2

    def unfix_symbolic(self, o: int, i: int) -> None:
        """edge ``(o, i)`` is a spline again, with the coefficients it had; the last edge unfixed removes the symbolic state"""
        o, i = self._check_edge(o, i)
        fixed = self._fixed_state()
        if (o, i) not in fixed:
            raise KeyError(f"edge ({o}, {i}) is not fixed")
        del fixed[(o, i)]
        self._set_fixed(fixed)

    def symbolic_formula(self, o: int, digits: int = 4) -> str:
        """output ``o`` as text, ``0.73*sin(3.1*x0 + 0.4) - 0.2 + ...`` over the inputs ``x0, x1, ...``; defined when all of ``o``'s
        incoming edges are fixed"""
        from .symbolic import format_edge
        o, _ = self._check_edge(o, 0)
        fixed = self._fixed_state()
        missing = [i for i in range(self.in_features) if (o, i) not in fixed]
        if missing:
            raise ValueError(f"symbolic_formula: output {o} still has spline edges from inputs {missing}")
        text = ""
        for i in range(self.in_features):
            name, row = fixed[(o, i)]
            if name == "0":
                continue
            term = format_edge(name, *(float(v) for v in row.tolist()), digits=digits, var=f"x{i}")
            text = term if not text else (f"{text} - {term[1:]}" if term.startswith("-") else f"{text} + {term}")
        return text or "0"

    def suggest_symbolic(self, x: torch.Tensor, functions=None, topk: int = 3, max_rows: int = 4096, **search):
        """Which elementary function is every edge ``phi_{o,i}``: a ``SymbolicSuggestion`` (``kagnn_amd/symbolic.py``) with the
        ``topk`` best ``c f(a x + b) + d`` per edge, ranked by ``r2`` (ties: the lower library id), for the ``functions`` of
        ``SYMBOLIC_LIB`` (default: all 19).  ``x [N, in]`` is the layer's own input; of more than ``max_rows`` rows the evenly strided
        subset ``x[::ceil(N / max_rows)]`` is used.  ``edge_curves`` on those rows, then ``ops.symbolic_fit`` (``**search``:
        ``a_range``, ``b_range``, ``grid_number``, ``iterations``).  Spline orders 1..4.  Nothing of the layer changes."""
        from .symbolic import suggest_kanlinear
        return suggest_kanlinear(self, x, functions, topk, max_rows, **search)

    def regularization_loss(self, regularize_activation=1.0, regularize_entropy=1.0, x: Optional[torch.Tensor] = None):
        """``x=None``: efficient-KAN's stand-in on ``|spline_weight|`` (``ekan.py:213-233``).  With the layer's input ``x``: the
        KAN paper's L1 + entropy regulariser on the edge activations, ``mag = edge_l1(x)`` in the same formula."""
        mag = self.spline_weight.abs().mean(-1) if x is None else self.edge_l1(x)
        total = mag.sum()
        share = mag / total
        return regularize_activation * total - regularize_entropy * torch.sum(share * share.log())


class KAN(nn.Module):
    """A bare chain of KANLinear layers (no activation or norm in between), ``ekan.py:236-281``."""

    def __init__(self, layers_hidden: Sequence[int], grid_size=5, spline_order=3, scale_noise=0.1,
                 scale_base=1.0, scale_spline=1.0, base_activation=torch.nn.SiLU, grid_eps=0.02,
                 grid_range=[-1, 1]):
        super().__init__()
        self.grid_size = grid_size
        self.spline_order = spline_order
        self.layers = nn.ModuleList(
            KANLinear(a, b, grid_size=grid_size, spline_order=spline_order, scale_noise=scale_noise,
                      scale_base=scale_base, scale_spline=scale_spline, base_activation=base_activation,
                      grid_eps=grid_eps, grid_range=grid_range)
            for a, b in zip(layers_hidden[:-1], layers_hidden[1:]))

    def forward(self, x: torch.Tensor, update_grid=False) -> torch.Tensor:
        packs = None
        if _PACK_CHAIN and not update_grid and x.is_cuda and len(self.layers) > 1 and not torch.compiler.is_compiling():
            packs = self._pack_chain(x)
        for i, layer in enumerate(self.layers):
            if update_grid:
                layer.update_grid(x)
            x = layer(x) if packs is None else layer(x, _packed=packs[i])
        return x

    @torch.no_grad()
    def refine(self, x: torch.Tensor, grid_size: int, adaptive: bool = False, grid_range=None, margin=0.01) -> List[torch.Tensor]:
        """``KANLinear.refine`` of every layer on its own input (``x`` is the chain's): each layer is refined, then evaluated
        refined for the next one.  Returns the layers' ``untouched`` counts."""
        out = []
        for i, layer in enumerate(self.layers):
            out.append(layer.refine(x, grid_size, adaptive=adaptive, grid_range=grid_range, margin=margin))
            if i + 1 < len(self.layers):
                x = layer._forward(x)
        self.grid_size = int(grid_size)
        return out

    def _pack_chain(self, x):
        """all layers' weight packs in one launch when the chain runs on the sparse-forward / split kernels"""
        first = self.layers[0]
        mode = first.precision if first.precision is not None else ops.default_precision()
        if ops.layer_inputs_visible() or not ops.split_like(mode) or x.size(0) == 0 or not ops._fits32(x, 1):
            return None
        fast = [l._fast_operands() for l in self.layers]
        if any(f is None or l.precision != first.precision for f, l in zip(fast, self.layers)):
            return None
        return ops.kan_pack_chain([f[:3] for f in fast], self.grid_size, self.spline_order, mode)

    def regularization_loss(self, regularize_activation=1.0, regularize_entropy=1.0, x: Optional[torch.Tensor] = None):
        """``x``: the chain's input -- every layer is then regularised on the activations of ITS input (the chain is walked)"""
        if x is None:
            return sum(l.regularization_loss(regularize_activation, regularize_entropy) for l in self.layers)
        total = 0.0
        for i, layer in enumerate(self.layers):
            total = total + layer.regularization_loss(regularize_activation, regularize_entropy, x=x)
            if i + 1 < len(self.layers):
                x = layer._forward(x)             # (not a forward of the model: a collect_edge_l1 block does not record it)
        return total

    def edge_l1(self, x: torch.Tensor) -> List[torch.Tensor]:
        """``KANLinear.edge_l1`` of every layer on its own input, ``x`` being the chain's"""
        out = []
        for i, layer in enumerate(self.layers):
            out.append(layer.edge_l1(x))
            if i + 1 < len(self.layers):
                x = layer._forward(x)
        return out

    def suggest_symbolic(self, x: torch.Tensor, **kw) -> list:
        """``KANLinear.suggest_symbolic`` of every layer on its own input, ``x`` being the chain's"""
        from .symbolic import suggest_chain
        return suggest_chain(self, x, **kw)

    # ------------------------------------------------------------------ attribution and pruning (pykan's attribute / prune)
    def attribute(self, x: torch.Tensor, out_scores=None) -> Attribution:
        """Which inputs, hidden units and edges the chain uses on the rows ``x`` (pykan's ``attribute``, without multiplication nodes).
        One eval-style walk under ``no_grad``, every layer on its own input: ``E_l = layer_l.edge_stats(x_l).std`` and ``s_l``, the
        column standard deviation of ``layer_l(x_l)``; then from ``node_scores[L] = out_scores`` (default: ones) backwards
        ``edge_scores[l][o,i] = E_l[o,i] node_scores[l+1][o] / (s_l[o] + 1e-4)``, ``node_scores[l][i] = sum_o edge_scores[l][o,i]``.
        Everything stays on the device.  Spline orders 1..4."""
        return _attribute_layers(list(self.layers), x, out_scores)

    @torch.no_grad()
    def keep_nodes(self, keep) -> None:
        """Shrink the chain's INTERIOR widths: ``keep[l]`` holds the sorted indices of the units of width ``l + 1`` that stay (one
        entry per interior width; the chain's input and output widths never change, so it keeps fitting its neighbours).  Layer ``l``
        keeps those rows of its parameters, layer ``l + 1`` those columns and those rows of its grid buffer; ``in_features`` /
        ``out_features`` follow; fixed symbolic edges on a removed unit are dropped, the others re-indexed.  Every touched layer gets
        NEW Parameters: rebuild the optimizer, as after ``refine``.  An empty keep list raises ``ValueError``."""
        layers = list(self.layers)
        if len(keep) != len(layers) - 1:
            raise ValueError(f"keep_nodes: one index list per interior width, {len(layers) - 1} of them (got {len(keep)})")
        lists = []
        for l, k in enumerate(keep):
            k = torch.as_tensor(k, dtype=torch.int64).reshape(-1).cpu()
            width = layers[l].out_features
            if k.numel() == 0:
                raise ValueError(f"keep_nodes: nothing is kept of interior width {l + 1}")
            if int(k[0]) < 0 or int(k[-1]) >= width or bool((k[1:] <= k[:-1]).any()):
                raise ValueError(f"keep_nodes: keep[{l}] must be sorted, without repeats, within [0, {width})")
            lists.append(k)
        for l, k in enumerate(lists):
            if k.numel() == layers[l].out_features:
                continue
            layers[l]._keep(k, None)
            layers[l + 1]._keep(None, k)
        ops._KNOTS_EQUAL.clear()

    def prune_nodes(self, x: torch.Tensor, threshold: float = 1e-2) -> List[torch.Tensor]:
        """``attribute(x)``, then ``keep_nodes`` of the interior units whose score exceeds ``threshold`` (of a width where none does:
        the one of highest score).  Returns the keep lists (int64, on the host).  New Parameters: rebuild the optimizer."""
        keep = _keep_lists(self.attribute(x), threshold)
        self.keep_nodes(keep)
        return keep

    def prune_edges(self, x: torch.Tensor, threshold: float = 3e-2) -> List[torch.Tensor]:
        """``attribute(x)``, then every spline edge with ``edge_scores[l][o,i] < threshold`` is switched off as
        ``fix_symbolic(o, i, "0")`` does (its parameters stay and get exactly zero gradient); already fixed edges are left alone.
        Returns the pruned ``(o, i)`` rows per layer (int64 ``[P_l, 2]``, on the host).  New ``symbolic_affine`` Parameters: rebuild
        the optimizer."""
        return _switch_off_edges(list(self.layers), self.attribute(x), threshold)

    def prune(self, x: torch.Tensor, node_threshold: float = 1e-2, edge_threshold: float = 3e-2):
        """``prune_nodes``, then ``prune_edges`` on a fresh attribution of the shrunk chain (pykan's ``prune``): ``(keep lists,
        pruned edges)``"""
        keep = self.prune_nodes(x, node_threshold)
        return keep, self.prune_edges(x, edge_threshold)


@torch.no_grad()
def _attribute_layers(layers, x: torch.Tensor, out_scores=None) -> Attribution:
    for layer in layers:
        if ops.high_order(layer.spline_order):
            raise NotImplementedError(f"attribute: spline_order must be in 1..{ops.FUSED_MAX_SPLINE_ORDER} (got {layer.spline_order}); "
                                      "the per-edge activation kernels do not cover the orders above")
    x = x.detach() if x.dtype == torch.float32 else x.detach().float()
    edge_std, out_std = [], []
    for layer in layers:
        edge_std.append(layer.edge_stats(x).std)
        x = layer._forward(x)                     # (not a forward of the model: nothing records it)
        out_std.append(torch.var_mean(x, dim=0)[0].sqrt())
    score = torch.ones_like(out_std[-1]) if out_scores is None else \
        torch.as_tensor(out_scores, dtype=torch.float32, device=x.device).reshape(out_std[-1].shape)
    node, edge = [score], []
    for e, s in zip(reversed(edge_std), reversed(out_std)):
        edge.insert(0, e * (node[0] / (s + 1e-4)).unsqueeze(1))
        node.insert(0, edge[0].sum(0))
    return Attribution(edge_std, out_std, edge, node)


def _keep_lists(att: Attribution, threshold: float) -> List[torch.Tensor]:
    """per interior width the units with ``node_scores > threshold`` (none: the best one); one read-back of the masks"""
    masks = []
    for score in att.node_scores[1:-1]:
        m = score > threshold
        best = torch.zeros_like(m).index_fill_(0, score.nan_to_num(nan=-math.inf).argmax().reshape(1), True)
        masks.append(torch.where(m.any(), m, best))
    if not masks:
        return []
    host = torch.cat(masks).cpu()
    return [m.nonzero().reshape(-1) for m in host.split([m.numel() for m in masks])]


def _switch_off_edges(layers, att: Attribution, threshold: float) -> List[torch.Tensor]:
    masks = []
    for layer, score in zip(layers, att.edge_scores):
        m = score < threshold
        masks.append((m if layer._symbolic is None else m & (layer.symbolic_keep != 0)).reshape(-1))
    host = torch.cat(masks).cpu()                          # one read-back
    out = []
    for layer, m in zip(layers, host.split([m.numel() for m in masks])):
        pairs = m.reshape(layer.out_features, layer.in_features).nonzero()
        if pairs.size(0):
            layer._switch_off(pairs.tolist())
        out.append(pairs)
    return out


def _collect(layer: KANLinear, x: torch.Tensor) -> None:
    for entry in ops._edge_collectors():
        name = entry[0].get(id(layer))
        if name is None:
            continue
        if len(entry) > 2:
            entry[2](name, layer, x)              # a kagnn_amd.suggest_symbolic walk: it wants the input, not the statistics
        else:
            entry[1][name] = layer.edge_l1(x if x.dtype == torch.float32 else x.float())


@contextlib.contextmanager
def collect_edge_l1(model: nn.Module):
    """``with collect_edge_l1(model) as stats: out = model(...)`` fills ``stats`` with ``{qualified module name: edge_l1 [out, in]}``
    for every ``KANLinear`` of spline order <= 4 and every ``FastKANLayer`` under ``model``, taken on the input each layer sees during the forwards inside
    the block (a layer called again overwrites its entry).  The statistics are differentiable: add a regulariser built from them
    to the loss.  While a block is active the fused layer / stack / model routes, which never expose a layer's input, take their
    composed per-layer form (``ops.layer_inputs_visible``); outside it nothing changes.

    EVERY ``KANLinear.forward`` / ``FastKANLayer.forward`` inside the block records -- also under ``torch.no_grad()`` or in eval mode -- and the latest call
    wins, so run inside the block only the forward whose statistics are wanted.  The chain walks of ``KAN.edge_l1`` and
    ``KAN.regularization_loss(x=)`` do not record.  The block belongs to the thread that opened it: forwards on other threads
    (data-parallel replicas, a loader thread) keep their fused routes and are not recorded."""
    from .fastkan import FastKANLayer             # (FastKAN chains run composed as they are: FastKANLayer.forward records)
    names = {id(m): n for n, m in model.named_modules()
             if (isinstance(m, KANLinear) and not ops.high_order(m.spline_order)) or isinstance(m, FastKANLayer)}
    entry = (names, {})
    active = ops._edge_collectors()
    active.append(entry)
    try:
        yield entry[1]
    finally:
        active.remove(entry)


class _RefineWalk:
    """the state of one ``refine_grids`` call: which layers to refine, how, and what happened"""

    def __init__(self, names, grid_size, adaptive, keep_inputs):
        self.names, self.grid_size, self.adaptive, self.keep_inputs = names, int(grid_size), adaptive, keep_inputs
        self.report: Dict[str, dict] = {}

    def visit(self, layer: KANLinear, x: torch.Tensor) -> None:
        name = self.names.get(id(layer))
        if name is None or name in self.report:           # not under the model, or already refined on its first input
            return
        rows = x.detach() if x.dtype == torch.float32 else x.detach().float()
        old = layer.grid_size
        untouched = layer.refine(rows, self.grid_size, adaptive=self.adaptive)
        entry = {"grid_size": (old, self.grid_size), "rows": rows.size(0), "untouched": untouched}
        if self.keep_inputs:
            entry["input"] = rows.clone()
        self.report[name] = entry


def refine_grids(model: nn.Module, grid_size: int, *args, adaptive: bool = False, keep_inputs: bool = False, **kwargs) -> dict:
    """Grid extension for a whole model: ONE forward ``model(*args, **kwargs)`` under ``no_grad`` in eval mode (no dropout, no
    running statistics move; the ``training`` flags are restored), during which every ``KANLinear`` of spline order <= 4 under
    ``model`` is refined to ``grid_size`` (``KANLinear.refine``) on the first input it sees, BEFORE it evaluates that input -- so
    every layer downstream is fitted on what the refined layers upstream produce, as in ``KAN.forward(update_grid=True)``.  As
    inside a ``collect_edge_l1`` block, the fused layer / stack / model routes take their composed per-layer form for this one
    forward (``ops.layer_inputs_visible``).  Wrapper modules that mirror ``grid_size`` (``KAN``) follow their layers.

    Returns ``{module name: {"grid_size": (old, new), "rows": N, "untouched": int32 [in], "input": x if keep_inputs}}`` plus
    ``"skipped"``: the names of the ``KANLinear`` layers of order 5..16 and of the ``FastKANLayer`` s, which are left as they are (and
    of layers the forward never reached).  ``grid`` and ``spline_weight`` of every refined layer are NEW tensors: build a new optimizer."""
    from .fastkan import FastKANLayer
    if ops._refine_walk() is not None:
        raise RuntimeError("refine_grids is already running on this thread")
    names, skipped = {}, []
    for n, m in model.named_modules():
        if isinstance(m, KANLinear) and not ops.high_order(m.spline_order):
            names[id(m)] = n
        elif isinstance(m, (KANLinear, FastKANLayer)):
            skipped.append(n)
    k_max = max((m.spline_order for m in model.modules() if id(m) in names), default=1)
    if int(grid_size) < 1 or int(grid_size) + 2 * k_max + 1 > ops.MAX_KNOTS:
        raise ValueError(f"refine_grids: grid_size must be >= 1 with grid_size + 2 * spline_order + 1 <= {ops.MAX_KNOTS} (got {grid_size})")
    walk = _RefineWalk(names, grid_size, adaptive, keep_inputs)
    flags = [(m, m.training) for m in model.modules()]
    model.eval()
    ops._set_refine_walk(walk)
    try:
        with torch.no_grad():
            model(*args, **kwargs)
    finally:
        ops._set_refine_walk(None)
        for m, flag in flags:
            m.training = flag
        # everything derived from the old shapes or parameters: the knot comparisons and the graph-level model call's template
        ops._KNOTS_EQUAL.clear()
        for m in model.modules():
            m.__dict__.pop("_kagnn_model_call_template", None)
    for n, m in model.named_modules():                    # wrappers that mirror their layers' grid_size
        if isinstance(m, (KANLinear, FastKANLayer)) or not isinstance(getattr(m, "grid_size", None), int):
            continue
        below = [walk.report.get(names.get(id(l))) for l in m.modules() if isinstance(l, KANLinear)]
        if below and all(e is not None for e in below):
            m.grid_size = int(grid_size)
    report = dict(walk.report)
    report["skipped"] = skipped + [n for n in names.values() if n not in walk.report]
    return report


def _chains(model: nn.Module):
    """``[(name, the KAN or None, layers)]`` in ``named_modules()`` order: every ``KAN`` under ``model``, and every ``KANLinear`` outside any
    ``KAN`` as a chain of one"""
    inside = {id(l) for m in model.modules() if isinstance(m, KAN) for l in m.layers}
    out = []
    for n, m in model.named_modules():
        if isinstance(m, KAN):
            out.append((n, m, list(m.layers)))
        elif isinstance(m, KANLinear) and id(m) not in inside:
            out.append((n, None, [m]))
    return out


def _forget_shapes(model: nn.Module) -> None:
    # everything derived from the old shapes or parameters (as after refine_grids)
    ops._KNOTS_EQUAL.clear()
    for m in model.modules():
        m.__dict__.pop("_kagnn_model_call_template", None)


def attribute(model: nn.Module, *args, keep_inputs: bool = False, **kwargs) -> Dict[str, Attribution]:
    """Attribution scores for a whole model: ONE forward ``model(*args, **kwargs)`` under ``no_grad`` in eval mode (no dropout, no
    running statistics move; the ``training`` flags are restored) inside a visible-inputs block (``ops.layer_inputs_visible``: the
    fused layer / stack / model routes take their composed per-layer form for this one forward and are back afterwards), during
    which every chain records the input it sees (the latest call wins).  Then ``{chain name: chain.attribute(that input)}`` for every
    ``ekan.KAN`` under ``model``; a ``KANLinear`` outside any ``KAN`` counts as a chain of one.  Every chain's own outputs are scored 1:
    attribution does NOT cross an aggregation, a BatchNorm or any other module between two chains -- the scores say what each chain
    uses of ITS input, not what the model uses of the graph's features.  ``keep_inputs``: every ``Attribution.input`` holds the
    recorded input.  Spline orders 1..4."""
    chains = _chains(model)
    first = {id(layers[0]): n for n, _, layers in chains}
    seen: Dict[str, torch.Tensor] = {}

    def visit(name, layer, x, *_):
        seen[name] = x.detach()

    entry = (first, {}, visit)
    flags = [(m, m.training) for m in model.modules()]
    model.eval()
    active = ops._edge_collectors()
    active.append(entry)
    try:
        with torch.no_grad():
            model(*args, **kwargs)
    finally:
        active.remove(entry)
        for m, flag in flags:
            m.training = flag
    out = {}
    for name, _, layers in chains:
        if name in seen:
            out[name] = _attribute_layers(layers, seen[name])
            if keep_inputs:
                out[name].input = seen[name]
    return out


def prune(model: nn.Module, *args, node_threshold: float = 1e-2, edge_threshold: float = 3e-2, **kwargs) -> PruneReport:
    """Prune every chain of a model (``KAN.prune`` chain by chain, on the inputs the chains see in the model): one
    ``attribute(model, ...)`` pass decides the hidden units of every ``KAN`` (``KAN.keep_nodes``), a second pass on the shrunk model
    decides the edges (switched off as ``fix_symbolic(o, i, "0")``).  Chains' outer widths never change.  Returns a ``PruneReport``;
    the touched layers have NEW Parameters: rebuild the optimizer.  A checkpoint of the pruned model loads into a fresh model of the
    original sizes after ``apply_pruning(fresh, report)``."""
    report = PruneReport()
    chains = _chains(model)
    found = attribute(model, *args, **kwargs)
    for name, chain, layers in chains:
        if name not in found:
            continue
        before = [layers[0].in_features] + [l.out_features for l in layers]
        keep = _keep_lists(found[name], node_threshold)
        if chain is not None:
            chain.keep_nodes(keep)
        report.chains[name] = {"keep": keep, "edges": [], "widths_before": before,
                               "widths_after": [layers[0].in_features] + [l.out_features for l in layers]}
    _forget_shapes(model)
    found = attribute(model, *args, **kwargs)
    for name, _, layers in chains:
        if name in found:
            report.chains[name]["edges"] = _switch_off_edges(layers, found[name], edge_threshold)
    _forget_shapes(model)
    return report


def apply_pruning(model: nn.Module, report: PruneReport) -> None:
    """Replay a ``PruneReport`` on a fresh model of the ORIGINAL sizes: the keep lists and the ``"0"`` edges, so that
    ``model.load_state_dict(pruned.state_dict())`` then succeeds (``load_state_dict`` itself is unchanged)."""
    chains = {n: (chain, layers) for n, chain, layers in _chains(model)}
    for name, entry in report.chains.items():
        if name not in chains:
            raise KeyError(f"apply_pruning: the model has no chain {name!r}")
        chain, layers = chains[name]
        if chain is not None:
            chain.keep_nodes(entry["keep"])
        for layer, pairs in zip(layers, entry["edges"]):
            if len(pairs):
                layer._switch_off(torch.as_tensor(pairs).reshape(-1, 2).tolist())
    _forget_shapes(model)
