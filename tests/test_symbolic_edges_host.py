"""Fixed symbolic edges, what runs without a GPU: the derivative table of ``kagnn_symbolic_edges_bwd`` against fp64 autograd of
``SYMBOLIC_LIB``'s lambdas, the workspace and plan queries, the validation of an edge list (``ops.SymbolicEdges`` ->
``kagnn_symbolic_edges_plan``), the bookkeeping of ``KANLinear.fix_symbolic`` / ``unfix_symbolic`` / ``"0"`` / a state_dict round trip,
the formula text, and the presence of the new symbols in the header and the library."""
import os
import re

import pytest
import torch

import kagnn_amd
from kagnn_amd import _lib, ops
from kagnn_amd.symbolic import SYMBOLIC_LIB, format_edge
from test_subgraph_host import _NoLaunch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"kagnn_symbolic_edges_plan_bytes": 4, "kagnn_symbolic_edges_plan": 6, "kagnn_symbolic_edges_bwd_workspace_bytes": 3,
         "kagnn_symbolic_edges_fwd": 13, "kagnn_symbolic_edges_bwd": 16}

# the derivative table of include/kagnn_hip.h (kagnn_symbolic_edges_fwd), restated
sig = lambda t: 1.0 / (1.0 + torch.exp(-t))
DERIVATIVE = {
    "x": lambda t: torch.ones_like(t), "x^2": lambda t: 2 * t, "x^3": lambda t: 3 * t ** 2, "x^4": lambda t: 4 * t ** 3,
    "1/x": lambda t: -1 / t ** 2, "1/x^2": lambda t: -2 / t ** 3, "sqrt": lambda t: 0.5 / torch.sqrt(t),
    "1/sqrt(x)": lambda t: -0.5 / (t * torch.sqrt(t)), "exp": torch.exp, "log": lambda t: 1 / t, "abs": torch.sign,
    "sin": torch.cos, "cos": lambda t: -torch.sin(t), "tan": lambda t: 1 + torch.tan(t) ** 2, "tanh": lambda t: 1 - torch.tanh(t) ** 2,
    "sgn": lambda t: torch.zeros_like(t), "arctan": lambda t: 1 / (1 + t ** 2), "gaussian": lambda t: -2 * t * torch.exp(-t ** 2),
    "silu": lambda t: sig(t) * (1 + t * (1 - sig(t))),
}
POSITIVE = ("1/x", "1/x^2", "sqrt", "1/sqrt(x)", "log")


def test_the_derivative_table_is_autograd_of_the_library():
    assert tuple(DERIVATIVE) == tuple(SYMBOLIC_LIB)
    gen = torch.Generator().manual_seed(3)
    for name, (_, fn, _) in SYMBOLIC_LIB.items():
        t = torch.rand(200, generator=gen, dtype=torch.float64) * 2.8 + 0.1            # away from the kinks at 0
        if name not in POSITIVE:
            t = torch.cat([t, -t])
        if name == "tan":
            t = t[(t.abs() - 1.5708).abs() > 0.1]
        t.requires_grad_(True)
        (auto,) = torch.autograd.grad(fn(t).sum(), t)
        want = DERIVATIVE[name](t.detach())
        assert torch.allclose(auto, want, rtol=1e-12, atol=1e-13), name


def test_the_new_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    assert lib.kagnn_version() >= 280
    header = open(os.path.join(ROOT, "include", "kagnn_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, nargs in NAMES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, plain)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name) and name in _lib.EXPORTED and len(_lib._SIGNATURES[name][1]) == nargs, name
    for word in ("fmaf(c, f(t), d)", "singularity-protected", "plan_host"):
        assert word in header, word
    from kagnn_amd import _build
    assert "symbolic_edges.hip" in _build.SOURCES
    assert os.path.exists(os.path.join(ROOT, "kagnn_amd", "csrc", "symbolic_fn.h"))
    src = open(os.path.join(ROOT, "kagnn_amd", "csrc", "symbolic.hip")).read()
    assert '#include "symbolic_fn.h"' in src and "float sym_fn(" not in src
    assert callable(ops.symbolic_edges) and callable(kagnn_amd.auto_symbolic)
    for method in ("fix_symbolic", "unfix_symbolic", "fixed_edges", "symbolic_formula"):
        assert callable(getattr(kagnn_amd.KANLinear, method))


def test_the_size_queries_need_no_gpu():
    small = ops.symbolic_edges_workspace_bytes(1000, 8)
    assert small >= 4 * 4 * 8 * 4                             # 1000 rows: four slabs of 256 rows
    assert ops.symbolic_edges_workspace_bytes(1000, 16) > small
    # all 4096 edges of a 64 x 64 layer on 200 000 rows: far below an [N, E] tensor
    assert ops.symbolic_edges_workspace_bytes(200_000, 4096) < 200_000 * 4096 * 4 // 16
    assert ops.symbolic_edges_workspace_bytes(0, 0) >= 0
    for bad in ((-1, 4), (10, -1)):
        with pytest.raises(RuntimeError, match="argument check failed"):
            ops.symbolic_edges_workspace_bytes(*bad)
    assert ops._sizes("kagnn_symbolic_edges_plan_bytes", 3, 3, 2) == 4 * 32
    for bad in ((7, 3, 2), (-1, 3, 2), (0, 0, 2), (0, 3, 0)):
        with pytest.raises(RuntimeError, match="argument check failed"):
            ops._sizes("kagnn_symbolic_edges_plan_bytes", *bad)


def test_an_edge_list_is_sorted_validated_and_planned():
    e = ops.SymbolicEdges([(1, 0, "sin"), (0, 2, "x^2"), (0, 1, "silu")], 3, 2, "cpu")
    assert e.triples == ((0, 1, 18), (0, 2, 1), (1, 0, 11)) and len(e) == 3
    assert e.index.tolist() == [list(t) for t in e.triples] and e.index.dtype == torch.int32
    plan = e.plan_host.tolist()
    assert plan[1:4] == [3, 3, 2] and plan[8:11] == [0, 2, 3]                      # header; optr
    assert plan[12:24] == [0, 1, 18, 0, 0, 2, 1, 0, 1, 0, 11, 0]                   # records
    assert plan[24:28] == [0, 1, 2, 3] and plan[28:31] == [2, 0, 1]                # iptr; the edges by input
    assert torch.equal(e.plan.cpu(), e.plan_host)
    empty = ops.SymbolicEdges([], 3, 2, "cpu")
    assert len(empty) == 0 and empty.index.shape == (0, 3)
    full = ops.SymbolicEdges([(o, i, "x") for o in range(2) for i in range(3)], 3, 2, "cpu")
    assert len(full) == 6
    refusals = [([(0, 1, 3), (0, 0, 2)], "not sorted"), ([(1, 0, 3), (0, 2, 2)], "not sorted"), ([(0, 1, 3), (0, 1, 2)], "repeats"),
                ([(0, 1, 19)], "unknown function id"), ([(0, 1, -1)], "unknown function id"), ([(2, 0, 1)], "outside"),
                ([(0, 3, 1)], "outside"), ([(0, -1, 1)], "outside"), ([(-1, 0, 1)], "outside")]
    for bad, why in refusals:
        with pytest.raises(ValueError, match=why):
            ops.SymbolicEdges.from_sorted(bad, 3, 2, "cpu")
    with pytest.raises(ValueError, match="repeats"):
        ops.SymbolicEdges([(0, 1, "sin"), (0, 1, "cos")], 3, 2, "cpu")
    with pytest.raises(ValueError, match="unknown function"):
        ops.SymbolicEdges([(0, 1, "sinh")], 3, 2, "cpu")
    for fin, fout in ((0, 2), (3, 0), (-1, 2)):
        with pytest.raises(ValueError, match=">= 1"):
            ops.SymbolicEdges([], fin, fout, "cpu")


def test_symbolic_edges_refuses_before_any_launch():
    e = ops.SymbolicEdges([(0, 1, "sin")], 3, 2, "cpu")
    x, aff = torch.zeros(5, 3), torch.zeros(1, 4)
    with _NoLaunch():
        with pytest.raises(TypeError, match="SymbolicEdges"):
            ops.symbolic_edges(x, [(0, 1, 11)], aff, 2)
        with pytest.raises(ValueError, match="2 outputs"):
            ops.symbolic_edges(x, e, aff, 3)
        with pytest.raises(ValueError, match=r"\[N, 3\]"):
            ops.symbolic_edges(torch.zeros(5, 4), e, aff, 2)
        with pytest.raises(ValueError, match=r"\[1, 4\]"):
            ops.symbolic_edges(x, e, torch.zeros(2, 4), 2)
        with pytest.raises(ValueError, match=r"y must be \[5, 2\]"):
            ops.symbolic_edges(x, e, aff, 2, y=torch.zeros(5, 3))
        with pytest.raises(TypeError, match="fp32"):
            ops.symbolic_edges(x.double(), e, aff, 2)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.symbolic_edges(x, e, aff, 2)


def test_a_layer_that_never_fixed_an_edge_is_the_reference_layer():
    torch.manual_seed(0)
    layer = kagnn_amd.KANLinear(3, 2)
    assert list(layer.state_dict()) == ["base_weight", "spline_weight", "spline_scaler", "grid"]
    assert [n for n, _ in layer.named_parameters()] == ["base_weight", "spline_weight", "spline_scaler"]
    assert layer.fixed_edges() == {} and layer._symbolic is None
    with pytest.raises(KeyError, match="not fixed"):
        layer.unfix_symbolic(0, 0)
    assert list(layer.state_dict()) == ["base_weight", "spline_weight", "spline_scaler", "grid"]


def test_fix_unfix_zero_and_a_state_dict_round_trip():
    torch.manual_seed(0)
    layer = kagnn_amd.KANLinear(3, 2)
    plain = {k: v.clone() for k, v in layer.state_dict().items()}
    assert layer.fix_symbolic(1, 0, "sin", params=(3.1, 0.4, 0.73, -0.2)) is None
    first = layer.symbolic_affine
    layer.fix_symbolic(1, 1, "0")
    layer.fix_symbolic(0, 2, "x^2", params=torch.tensor([1.0, 0.0, -2.0, 0.5]))
    assert layer.fixed_edges() == {(0, 2): "x^2", (1, 0): "sin", (1, 1): "0"}
    assert layer.symbolic_affine is not first                                      # a new Parameter with every change of the list
    assert isinstance(layer.symbolic_affine, torch.nn.Parameter) and layer.symbolic_affine.requires_grad
    assert layer.symbolic_affine.tolist() == [[1.0, 0.0, -2.0, 0.5], [pytest.approx(3.1), pytest.approx(0.4), pytest.approx(0.73), pytest.approx(-0.2)]]
    assert layer.symbolic_index.tolist() == [[0, 2, 1], [1, 0, 11]] and layer.symbolic_index.dtype == torch.int32
    assert layer.symbolic_keep.tolist() == [[1.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    assert set(layer.state_dict()) == set(plain) | {"symbolic_affine", "symbolic_index", "symbolic_keep"}
    for k, v in plain.items():                                                     # the spline parameters stay where they are
        assert torch.equal(layer.state_dict()[k], v)
    # fixing a fixed edge again replaces it and keeps the others' numbers
    layer.fix_symbolic(1, 0, "cos", params=(1, 2, 3, 4))
    assert layer.fixed_edges()[(1, 0)] == "cos" and layer.symbolic_affine.tolist() == [[1.0, 0.0, -2.0, 0.5], [1.0, 2.0, 3.0, 4.0]]

    other = kagnn_amd.KANLinear(3, 2)
    other.load_state_dict(layer.state_dict())
    assert other.fixed_edges() == layer.fixed_edges() and other._symbolic.triples == layer._symbolic.triples
    for k, v in layer.state_dict().items():
        assert torch.equal(other.state_dict()[k], v), k
    # a checkpoint without fixed edges brings a layer with fixed edges back to the reference's state
    other.load_state_dict(plain)
    assert other.fixed_edges() == {} and set(other.state_dict()) == set(plain)

    layer.unfix_symbolic(1, 1)
    assert layer.fixed_edges() == {(0, 2): "x^2", (1, 0): "cos"} and layer.symbolic_keep.tolist() == [[1.0, 1.0, 0.0], [0.0, 1.0, 1.0]]
    layer.unfix_symbolic(0, 2)
    layer.unfix_symbolic(1, 0)
    assert layer._symbolic is None and list(layer.state_dict()) == list(plain)
    assert [n for n, _ in layer.named_parameters()] == ["base_weight", "spline_weight", "spline_scaler"]
    for k, v in plain.items():
        assert torch.equal(layer.state_dict()[k], v)
    # only "0" edges: an empty list, still a state
    layer.fix_symbolic(0, 0, "0")
    assert layer.symbolic_affine.shape == (0, 4) and layer.symbolic_index.shape == (0, 3) and layer.fixed_edges() == {(0, 0): "0"}
    other.load_state_dict(layer.state_dict())
    assert other.fixed_edges() == {(0, 0): "0"}

    for bad in ((2, 0), (0, 3), (-1, 0)):
        with pytest.raises(IndexError):
            layer.fix_symbolic(*bad, "sin", params=(1, 0, 1, 0))
    with pytest.raises(ValueError, match="unknown function"):
        layer.fix_symbolic(0, 1, "sinh", params=(1, 0, 1, 0))
    with pytest.raises(ValueError, match=r"\(a, b, c, d\)"):
        layer.fix_symbolic(0, 1, "sin", params=(1, 0, 1))
    with pytest.raises(ValueError, match="rows x"):
        layer.fix_symbolic(0, 1, "sin")
    with pytest.raises(RuntimeError, match="no CPU fallback"):                     # a fit needs the device
        layer.fix_symbolic(0, 1, "sin", x=torch.randn(5, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):                     # and so does a forward
        layer(torch.randn(5, 3))


def test_fused_routes_step_aside_for_a_layer_with_fixed_edges():
    torch.manual_seed(0)
    chain = kagnn_amd.KAN([4, 4, 4])
    assert ops._chain_plan(list(chain.layers)) is not None
    chain.layers[1].fix_symbolic(0, 0, "0")
    assert ops._chain_plan(list(chain.layers)) is None
    assert chain.layers[1].read_out_blocks_in_one_launch((2, 2)) is False
    chain.layers[1].unfix_symbolic(0, 0)
    assert ops._chain_plan(list(chain.layers)) is not None
    from kagnn_amd.sharded import ShardedKANLinear
    layer = kagnn_amd.KANLinear(4, 4)
    ShardedKANLinear(layer, 0, 2)
    layer.fix_symbolic(1, 1, "x", params=(1, 0, 1, 0))
    with pytest.raises(NotImplementedError, match="fixed symbolic edges"):
        ShardedKANLinear(layer, 0, 2)


def test_formula_text():
    assert format_edge("sin", 3.1, 0.4, 0.731, -0.2) == "0.731*sin(3.1*x + 0.4) - 0.2"
    assert format_edge("x^2", -1.5, -0.25, -2.0, 0.0, var="x3") == "-2*(-1.5*x3 - 0.25)**2 + 0"
    torch.manual_seed(0)
    layer = kagnn_amd.KANLinear(3, 2)
    layer.fix_symbolic(1, 0, "sin", params=(3.1, 0.4, 0.73, -0.2))
    layer.fix_symbolic(1, 1, "0")
    with pytest.raises(ValueError, match=r"inputs \[2\]"):
        layer.symbolic_formula(1)
    layer.fix_symbolic(1, 2, "exp", params=(1.0, 0.0, -2.0, 0.5))
    assert layer.symbolic_formula(1) == "0.73*sin(3.1*x0 + 0.4) - 0.2 - 2*exp(1*x2 + 0) + 0.5"
    assert layer.symbolic_formula(1, digits=2) == "0.73*sin(3.1*x0 + 0.4) - 0.2 - 2*exp(1*x2 + 0) + 0.5"
    with pytest.raises(ValueError, match="still has spline edges"):
        layer.symbolic_formula(0)
    for i in range(3):
        layer.fix_symbolic(0, i, "0")
    assert layer.symbolic_formula(0) == "0"
    # the suggestion's text is built from the same pieces
    assert kagnn_amd.SymbolicSuggestion.formula.__code__.co_names.count("format_edge") == 1
