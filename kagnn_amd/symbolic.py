"""Symbolic fits of KAN edge functions: which elementary function is ``phi_{o,i}``, with what affine parameters, how well.

pykan's ``suggest_symbolic`` / ``fit_params`` for every edge of a layer at once: ``ops.symbolic_fit`` (``csrc/symbolic.hip``) searches
``(a, b)`` of ``phi(x) ~ c f(a x + b) + d`` on a zoomed grid for every function of ``SYMBOLIC_LIB`` and every edge; the layers'
``suggest_symbolic`` methods sample their edge functions on the rows they are given (``edge_curves``) and rank the functions per
edge; ``suggest_symbolic(model, ...)`` does so for every eligible layer of a model on the input it sees in one forward.

Acting on a fit: ``KANLinear.fix_symbolic`` puts a formula into the layer's forward (``ops.symbolic_edges``,
``csrc/symbolic_edges.hip``) with its four numbers trainable, ``"0"`` switches a dead edge off, ``auto_symbolic`` does both for a
whole model from one ``suggest_symbolic`` walk, ``KANLinear.symbolic_formula`` reads an output off as text.

Not here: fixed edges in a ``FastKANLayer``, in the sharded / RCCL layers or under ``torch.compile`` (a layer with fixed edges raises
there), pruning whole nodes (which changes shapes), pykan's singularity-protected functions (the library is the plain one: ``sqrt``
/ ``log`` outside their domain and ``1/x`` at 0 give what IEEE gives), sympy expressions, gradients through the fit.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch
import torch.nn.functional as F

from . import ops

# name -> (library id, the same definition in torch ops, format string of the formula: {} is the argument)
SYMBOLIC_LIB = {
    "x": (0, lambda t: t, "({})"),
    "x^2": (1, lambda t: t * t, "({})**2"),
    "x^3": (2, lambda t: t * t * t, "({})**3"),
    "x^4": (3, lambda t: (t * t) * (t * t), "({})**4"),
    "1/x": (4, lambda t: 1.0 / t, "1/({})"),
    "1/x^2": (5, lambda t: 1.0 / (t * t), "1/({})**2"),
    "sqrt": (6, torch.sqrt, "sqrt({})"),
    "1/sqrt(x)": (7, lambda t: 1.0 / torch.sqrt(t), "1/sqrt({})"),
    "exp": (8, torch.exp, "exp({})"),
    "log": (9, torch.log, "log({})"),
    "abs": (10, torch.abs, "abs({})"),
    "sin": (11, torch.sin, "sin({})"),
    "cos": (12, torch.cos, "cos({})"),
    "tan": (13, torch.tan, "tan({})"),
    "tanh": (14, torch.tanh, "tanh({})"),
    "sgn": (15, torch.sign, "sign({})"),
    "arctan": (16, torch.atan, "arctan({})"),
    "gaussian": (17, lambda t: torch.exp(-(t * t)), "exp(-({})**2)"),
    "silu": (18, lambda t: t / (1.0 + torch.exp(-t)), "silu({})"),
}
assert tuple(SYMBOLIC_LIB) == ops.SYMBOLIC_FUNCTIONS and all(v[0] == k for k, v in enumerate(SYMBOLIC_LIB.values()))


def format_edge(name: str, a: float, b: float, c: float, d: float, digits: int = 4, var: str = "x") -> str:
    """``c*f(a*var + b) + d`` as text (``SymbolicSuggestion.formula``, ``KANLinear.symbolic_formula``)"""
    num = lambda v: f"{abs(v):.{int(digits)}g}"
    sign = lambda v: "-" if (v < 0 or (v == 0 and str(v).startswith("-"))) else "+"
    arg = f"{'-' if sign(a) == '-' else ''}{num(a)}*{var} {sign(b)} {num(b)}"
    body = SYMBOLIC_LIB[name][2].format(arg)
    return f"{'-' if sign(c) == '-' else ''}{num(c)}*{body} {sign(d)} {num(d)}"


def fixed_edge_values(x: torch.Tensor, triples, affine: torch.Tensor) -> torch.Tensor:
    """``[N, E]``: ``c f(a x[:, i] + b) + d`` of the fixed edges ``triples = (o, i, function id)`` in torch ops -- the views of a layer
    with fixed edges (``edge_l1``, ``edge_curves``) and the tests' restatement; the forward itself runs ``ops.symbolic_edges``"""
    cols = torch.tensor([i for _, i, _ in triples], dtype=torch.int64, device=x.device)
    t = affine[:, 0] * x.index_select(1, cols) + affine[:, 1]
    fn_of = [v[1] for v in SYMBOLIC_LIB.values()]
    out = torch.zeros_like(t)
    for fid in sorted({f for _, _, f in triples}):
        at = torch.tensor([e for e, (_, _, f) in enumerate(triples) if f == fid], dtype=torch.int64, device=x.device)
        out = out.index_copy(1, at, fn_of[fid](t.index_select(1, at)))
    return affine[:, 2] * out + affine[:, 3]


class SymbolicSuggestion:
    """The ``topk`` best functions of every edge of one layer, ranked by ``r2`` (ties: the lower library id first).

    ``names[rank][o][i]``; ``params [topk, out, in, 4]`` = ``(a, b, c, d)`` of ``phi_{o,i}(x) ~ c f(a x + b) + d``; ``r2 [topk, out, in]``;
    ``edge_l1 [out, in]``: the layer's mean ``|phi_{o,i}|`` on the same rows (an edge with a negligible one is dead, whatever its
    fit); ``x [rows, in]``: the rows that were fitted, in the fit variable (for a ``FastKANLayer`` with a LayerNorm: the normalised
    input); ``fit``: the ``ops.SymbolicFit`` of all functions; ``input``: the layer's own input when asked for (``keep_inputs``)."""

    def __init__(self, fit: ops.SymbolicFit, topk: int, x: torch.Tensor, edge_l1: Optional[torch.Tensor] = None):
        ids = [SYMBOLIC_LIB[n][0] for n in fit.functions]
        by_id = sorted(range(len(ids)), key=lambda j: ids[j])                # dimension 0 in library order: a stable sort then
        order = torch.tensor(by_id, dtype=torch.int64, device=fit.r2.device)   # breaks ties towards the lower id
        fns = [fit.functions[j] for j in by_id]
        r2, params = fit.r2.index_select(0, order), fit.params.index_select(0, order)
        k = max(1, min(int(topk), len(fns)))
        ranked, at = torch.sort(r2, dim=0, descending=True, stable=True)
        at = at[:k]
        self.r2 = ranked[:k].contiguous()
        self.params = torch.gather(params, 0, at.unsqueeze(-1).expand(-1, -1, -1, 4)).contiguous()
        self.names: List[List[List[str]]] = [[[fns[j] for j in row] for row in plane] for plane in at.cpu().tolist()]
        self.edge_l1, self.x, self.fit, self.input = edge_l1, x, fit, None

    def formula(self, o: int, i: int, rank: int = 0, digits: int = 4) -> str:
        """``c*f(a*x + b) + d`` of edge ``(o, i)`` as text, e.g. ``0.731*sin(3.1*x + 0.4) - 0.2``: numbers with ``digits`` significant
        digits (9 reproduces the fp32 parameters exactly).  The function names are numpy's, plus ``silu(t) = t / (1 + exp(-t))``."""
        a, b, c, d = (float(v) for v in self.params[rank, o, i].tolist())
        return format_edge(self.names[rank][o][i], a, b, c, d, digits=digits)

    @torch.no_grad()
    def curves(self, points: torch.Tensor, rank: int = 0) -> torch.Tensor:
        """``[P, out, in]``: the rank's formulas at ``points`` (``[P]``, shared by all inputs, or ``[P, in]``), in torch ops on the
        parameters' device -- to plot against the layer's ``edge_curves(points)``."""
        p = self.params[rank]                                                  # [out, in, 4]
        pts = points.to(device=p.device, dtype=p.dtype)
        pts = pts.reshape(-1, 1, 1) if pts.dim() == 1 else pts.unsqueeze(1)    # [P, 1, 1 or in]
        t = p[..., 0] * pts + p[..., 1]
        out = torch.empty_like(t)
        names = self.names[rank]
        for name, (_, fn, _) in SYMBOLIC_LIB.items():
            mask = torch.tensor([[n == name for n in row] for row in names], device=p.device)
            if bool(mask.any()):
                out = torch.where(mask, fn(t), out)
        return p[..., 2] * out + p[..., 3]

    def __repr__(self):
        return f"SymbolicSuggestion(topk={len(self.names)}, out={self.r2.size(1)}, in={self.r2.size(2)}, rows={self.x.size(0)})"


def strided_rows(x: torch.Tensor, max_rows: int) -> torch.Tensor:
    """the rows a fit uses: all of ``x [N, in]`` when ``N <= max_rows``, else the evenly strided subset ``x[::ceil(N / max_rows)]``"""
    n = x.size(0)
    if max_rows is None or n <= int(max_rows):
        return x
    if int(max_rows) < 1:
        raise ValueError("max_rows must be at least 1")
    return x[::-(-n // int(max_rows))]


def _rows32(x: torch.Tensor, width: int) -> torch.Tensor:
    x = x.detach().reshape(-1, x.shape[-1])
    assert x.size(1) == width
    return x if x.dtype == torch.float32 else x.float()


@torch.no_grad()
def suggest_kanlinear(layer, x, functions=None, topk=3, max_rows=4096, **search) -> SymbolicSuggestion:
    """``KANLinear.suggest_symbolic``"""
    if ops.high_order(layer.spline_order):
        raise NotImplementedError("suggest_symbolic covers spline orders 1..4, the range of edge_curves")
    rows = strided_rows(_rows32(x, layer.in_features), max_rows)
    phi = layer.edge_curves(rows)
    fit = ops.symbolic_fit(rows, phi, functions, **search)
    return SymbolicSuggestion(fit, topk, rows, layer.edge_l1(rows).detach())


@torch.no_grad()
def suggest_fastkan(layer, x, functions=None, topk=3, max_rows=4096, use_layernorm=True, **search) -> SymbolicSuggestion:
    """``FastKANLayer.suggest_symbolic``"""
    rows = strided_rows(_rows32(x, layer.input_dim), max_rows)
    ln = layer.layernorm if (layer.layernorm is not None and use_layernorm) else None
    u = rows if ln is None else F.layer_norm(rows, (layer.input_dim,), ln.weight, ln.bias, ln.eps)
    phi = layer.edge_curves(u, None if ln is None else rows.contiguous())
    fit = ops.symbolic_fit(u, phi, functions, **search)
    return SymbolicSuggestion(fit, topk, u, layer.edge_l1(rows, use_layernorm).detach())


@torch.no_grad()
def suggest_chain(chain, x, **kw) -> List[SymbolicSuggestion]:
    """``KAN.suggest_symbolic`` / ``FastKAN.suggest_symbolic``: every layer on its own input, ``x`` being the chain's"""
    out = []
    for i, layer in enumerate(chain.layers):
        out.append(layer.suggest_symbolic(x, **kw))
        if i + 1 < len(chain.layers):
            x = layer._forward(x)
    return out


def suggest_symbolic(model: torch.nn.Module, *args, functions: Optional[Sequence[str]] = None, topk: int = 3, max_rows: int = 4096,
                     search: Optional[dict] = None, keep_inputs: bool = False, **kwargs) -> Dict[str, SymbolicSuggestion]:
    """Symbolic fits for a whole model: ONE forward ``model(*args, **kwargs)`` under ``no_grad`` in eval mode (the ``training`` flags
    are restored), during which every ``KANLinear`` of spline order <= 4 and every ``FastKANLayer`` under ``model`` records the input
    it sees (the latest call wins, as in a ``collect_edge_l1`` block -- it is that mechanism: the fused layer / stack / model
    routes take their composed per-layer form for this one forward, ``ops.layer_inputs_visible``, and are back afterwards).  Each
    layer is then fitted on that input: ``{qualified module name: layer.suggest_symbolic(input, functions, topk, max_rows,
    **search)}`` (``search``: ``a_range``, ``b_range``, ``grid_number``, ``iterations``).  Nothing of the model is modified.
    ``keep_inputs``: every suggestion's ``.input`` holds the recorded input."""
    from .ekan import KANLinear
    from .fastkan import FastKANLayer
    names = {id(m): n for n, m in model.named_modules()
             if (isinstance(m, KANLinear) and not ops.high_order(m.spline_order)) or isinstance(m, FastKANLayer)}
    seen: Dict[str, tuple] = {}

    def visit(name, layer, x, *use_layernorm):
        seen[name] = (layer, x.detach(), use_layernorm)

    entry = (names, {}, visit)
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
    for name in (n for n in names.values() if n in seen):                        # (named_modules order)
        layer, x, use_layernorm = seen[name]
        kw = dict(search or {})
        if use_layernorm:
            kw["use_layernorm"] = use_layernorm[0]
        out[name] = layer.suggest_symbolic(x, functions=functions, topk=topk, max_rows=max_rows, **kw)
        if keep_inputs:
            out[name].input = x
    return out


def auto_symbolic(model: torch.nn.Module, *args, r2_threshold: float, dead_threshold: float, functions: Optional[Sequence[str]] = None,
                  max_rows: int = 4096, search: Optional[dict] = None, **kwargs) -> Dict[str, list]:
    """Fix what a model's fits allow (pykan's ``auto_symbolic``): ONE ``suggest_symbolic(model, *args, functions=..., topk=1, ...)``
    walk, then per eligible ``KANLinear`` (spline order <= 4) and per edge that is still a spline: ``edge_l1 < dead_threshold`` -> fixed
    to ``"0"``; else the rank-0 function when its ``r2 >= r2_threshold``, with the suggestion's parameters (no second fit); else left
    as it is.  Returns ``{layer name: [(o, i, name, r2)]}`` of what was fixed (``r2`` of a ``"0"`` edge: ``None``).  Both thresholds are
    the caller's to choose.  Every touched layer gets a NEW ``symbolic_affine`` Parameter: rebuild the optimizer."""
    from .ekan import KANLinear
    found = suggest_symbolic(model, *args, functions=functions, topk=1, max_rows=max_rows, search=search, **kwargs)
    layers = dict(model.named_modules())
    report: Dict[str, list] = {}
    for name, sug in found.items():
        layer = layers[name]
        if not isinstance(layer, KANLinear):
            continue
        l1, r2, params = sug.edge_l1.cpu(), sug.r2[0].cpu(), sug.params[0].cpu()
        fixed = layer._fixed_state()
        done = []
        for o in range(layer.out_features):
            for i in range(layer.in_features):
                if (o, i) in fixed:
                    continue
                if float(l1[o, i]) < dead_threshold:
                    fixed[(o, i)] = ("0", None)
                    done.append((o, i, "0", None))
                elif float(r2[o, i]) >= r2_threshold:
                    fn = sug.names[0][o][i]
                    fixed[(o, i)] = (fn, params[o, i].clone())
                    done.append((o, i, fn, float(r2[o, i])))
        if done:
            layer._set_fixed(fixed)
        report[name] = done
    return report
