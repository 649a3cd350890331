"""CPU-side checks of the MLP baselines (kagnn_amd/baselines.py): state_dict keys against written-out lists, the ``make_mlp``
quirks, constructor signatures against the reference's sources, the refusal of CPU tensors, ``run_reference --baselines`` and the
register budget of the dense-layer kernels.  No GPU, no compute call."""
import ast
import importlib.util
import inspect
import os
import shutil
import sys

import pytest
import torch
import torch.nn as nn

import kagnn_amd
from kagnn_amd import baselines as B
from kagnn_amd import _lib, harness, ops, run_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("KAGNN_REFERENCE", "/root/reference")

BN = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]


def _keys(m):
    return list(m.state_dict())


def test_state_dict_keys_node_model():
    want = []
    for i in range(2):
        want += [f"convs.{i}.eps", f"convs.{i}.nn.0.0.weight", f"convs.{i}.nn.0.0.bias", f"convs.{i}.nn.1.0.weight", f"convs.{i}.nn.1.0.bias"]
    want += [f"bns.{i}.{k}" for i in range(2) for k in BN] + ["lay_out.weight", "lay_out.bias"]
    m = B.GNN_Nodes("gin", 2, 10, 8, 3)
    assert sorted(_keys(m)) == sorted(want)
    assert m.lay_out.in_features == 10 + 2 * 8 and type(m.lay_out) is B.Linear
    assert B.GNN_Nodes("gin", 2, 10, 8, 3, skip=False).lay_out.in_features == 8
    m = B.GNN_Nodes("gcn", 1, 10, 8, 3)
    assert sorted(_keys(m)) == sorted(["convs.0.bias", "convs.0.lin.weight"] + [f"bns.0.{k}" for k in BN] + ["lay_out.weight", "lay_out.bias"])
    m = B.GNN_Nodes("gat", 2, 10, 8, 3, heads=3)
    assert sorted(_keys(m)) == sorted([f"convs.{i}.{k}" for i in range(2) for k in ("att_src", "att_dst", "bias", "lin.weight")]
                                      + [f"bns.{i}.{k}" for i in range(2) for k in BN] + ["lay_out.weight", "lay_out.bias"])
    assert m.convs[1].lin.weight.shape == (24, 24) and m.convs[0].att_src.shape == (1, 3, 8) and m.bns[0].num_features == 24
    assert m.lay_out.in_features == 10 + 2 * 24
    assert B.GNN_Nodes("gcn", 2, 10, 8, 3, heads=3).bns[0].num_features == 8          # heads is forced to 1 unless gat
    with pytest.raises(ValueError, match="unknown conv_type"):
        B.GNN_Nodes("sage", 1, 4, 4, 2)


def test_state_dict_keys_graph_models():
    m = B.GIN(2, 5, 8, 3, 4, 0.0)
    want = []
    for i in range(2):
        want += [f"conv.{i}.eps"]
        for j in range(2):
            want += [f"conv.{i}.nn.{j}.0.weight", f"conv.{i}.nn.{j}.0.bias"] + [f"conv.{i}.nn.{j}.2.{k}" for k in BN]
        want += [f"conv.{i}.nn.2.0.weight", f"conv.{i}.nn.2.0.bias"]
    want += [f"mlp.{j}.0.{k}" for j in range(3) for k in ("weight", "bias")]
    assert sorted(_keys(m)) == sorted(want)
    assert "conv.0.nn.0.2.running_var" in want and "mlp.1.0.bias" in want
    assert m.conv[0].nn[0][0].weight.shape == (8, 5) and m.mlp[2][0].weight.shape == (4, 8)
    assert type(m.conv[0].nn[0][2]) is kagnn_amd.BatchNorm1d
    assert sorted(_keys(B.GCN(2, 5, 8, 4, 0.0))) == sorted(["conv.0.bias", "conv.0.lin.weight", "conv.1.bias", "conv.1.lin.weight",
                                                            "readout.0.0.weight", "readout.0.0.bias"])
    m = B.GAT(2, 5, 8, 4, 0.0, 2)
    assert sorted(_keys(m)) == sorted([f"conv.{i}.{k}" for i in range(2) for k in ("att_src", "att_dst", "bias", "lin.weight")]
                                      + ["readout.0.0.weight", "readout.0.0.bias"])
    assert m.conv[1].lin.weight.shape == (16, 16) and m.readout[0][0].weight.shape == (4, 16)
    m = B.GINRegression(5, 3, 1, 8, 2, 1, 0.0, False)
    assert sorted(_keys(m)) == sorted(["atom_encoder.weight", "atom_encoder.bias", "bond_encoder.weight", "bond_encoder.bias", "conv.0.eps",
                                       "conv.0.nn.0.0.weight", "conv.0.nn.0.0.bias"] + [f"conv.0.nn.0.2.{k}" for k in BN]
                                      + ["conv.0.nn.1.0.weight", "conv.0.nn.1.0.bias", "mlp.0.0.weight", "mlp.0.0.bias", "mlp.1.0.weight", "mlp.1.0.bias"])
    m = B.GINRegression(5, 3, 1, 8, 2, 1, 0.0, True)
    assert "atom_encoder.atom_embedding_list.0.weight" in _keys(m) and "bond_encoder.bond_embedding_list.2.weight" in _keys(m)
    m = B.GCNRegression(5, 2, 8, 1, 0.0, False)
    assert sorted(_keys(m)) == sorted(["atom_encoder.weight", "atom_encoder.bias", "conv.0.bias", "conv.0.lin.weight", "conv.1.bias",
                                       "conv.1.lin.weight", "readout.0.0.weight", "readout.0.0.bias"])


def test_a_stock_torch_state_dict_loads():
    """the reference's make_mlp, restated with stock modules, saves a state_dict this package's chain loads (and the other way)"""
    stock = nn.Sequential(nn.Sequential(nn.Linear(5, 8), nn.ReLU(), nn.BatchNorm1d(8)), nn.Sequential(nn.Linear(8, 8), nn.ReLU(), nn.BatchNorm1d(8)),
                          nn.Sequential(nn.Linear(8, 3, nn.ReLU())))
    ours = B.make_mlp(5, 8, 3, 3, batch_norm=True)
    ours.load_state_dict(stock.state_dict())
    stock.load_state_dict(ours.state_dict())
    assert list(ours.state_dict()) == list(stock.state_dict())


def test_make_mlp_quirks():
    for flavour in (lambda h: B.make_mlp_nodes(5, 8, 3, h), lambda h: B.make_mlp(5, 8, 3, h, batch_norm=True),
                    lambda h: B.make_mlp(5, 8, 3, h, batch_norm=False)):
        for h in (2, 3, 4):
            chain = flavour(h)
            assert len(chain) == h
            last = chain[-1]
            assert len(last) == 1 and type(last[0]) is B.Linear and last[0].bias is not None       # a bias, and NO ReLU
            assert last[0].weight.shape == (3, 8)
            for block in chain[:-1]:
                assert type(block) is B.LinearReLU and type(block[0]) is B.Linear and type(block[1]) is nn.ReLU
        one = flavour(1)
        assert len(one) == 1 and len(one[0]) == 2 and type(one[0][1]) is nn.ReLU and one[0][0].weight.shape == (3, 5)   # Linear -> ReLU
    assert all(len(b) == 3 and type(b[2]) is kagnn_amd.BatchNorm1d for b in B.make_mlp(5, 8, 3, 3, batch_norm=True)[:-1])
    assert all(len(b) == 2 for b in B.make_mlp(5, 8, 3, 3, batch_norm=False)[:-1])
    assert all(len(b) == 2 for b in B.make_mlp_nodes(5, 8, 3, 3)[:-1])
    assert list(inspect.signature(B.make_mlp_nodes).parameters) == ["num_features", "hidden_dim", "out_dim", "hidden_layers"]
    sig = inspect.signature(B.make_mlp)
    assert list(sig.parameters) == ["num_features", "hidden_dim", "out_dim", "hidden_layers", "batch_norm"] and sig.parameters["batch_norm"].default is True


def test_linear_keeps_the_stock_surface_and_initialisation():
    torch.manual_seed(3)
    a = B.Linear(7, 4)
    torch.manual_seed(3)
    b = nn.Linear(7, 4)
    assert torch.equal(a.weight, b.weight) and torch.equal(a.bias, b.bias)
    assert list(inspect.signature(B.Linear.__init__).parameters) == list(inspect.signature(nn.Linear.__init__).parameters)
    conv = B.GCNConv(6, 4)
    assert conv.lin.bias is None and float(conv.lin.weight.detach().abs().max()) <= (6.0 / (6 + 4)) ** 0.5 and not bool(conv.bias.any())   # glorot, zero bias
    conv = B.GATConv(6, 4, 3)
    assert conv.lin.bias is None and conv.lin.weight.shape == (12, 6) and float(conv.lin.weight.detach().abs().max()) <= (6.0 / (6 + 12)) ** 0.5


def test_linear_relu_block_falls_back_to_the_plain_sequential(monkeypatch):
    calls = []
    monkeypatch.setattr(ops, "linear", lambda x, w, b=None, relu=False: (calls.append(relu), torch.relu(x @ w.t() + b) if relu else x @ w.t() + b)[1])
    x = torch.randn(6, 5)
    block = B.LinearReLU(B.Linear(5, 4), nn.ReLU())
    want = torch.relu(x @ block[0].weight.t() + block[0].bias)
    assert torch.equal(block(x), want) and calls == [True]                  # ONE fused call
    del calls[:]
    seen = []
    handle = block[0].register_forward_hook(lambda m, i, o: seen.append(o))
    assert torch.equal(block(x), want) and calls == [False] and len(seen) == 1 and float(seen[0].detach().min()) < 0     # the hook sees the pre-activation
    handle.remove()
    del calls[:]
    block[1] = nn.Tanh()
    assert torch.equal(block(x), torch.tanh(x @ block[0].weight.t() + block[0].bias)) and calls == [False]


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.linear(torch.randn(4, 3), torch.randn(2, 3), torch.randn(2), relu=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        B.Linear(3, 2)(torch.randn(4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        B.make_mlp(3, 4, 2, 2)(torch.randn(4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        B.GNN_Nodes("gin", 1, 3, 4, 2)(torch.randn(4, 3), torch.zeros(2, 0, dtype=torch.int64))


def test_entry_points_validate_their_arguments_before_any_device_call():
    import ctypes
    lib = _lib.load()
    assert lib.kagnn_version() >= 267
    n = ctypes.c_size_t(0)
    assert lib.kagnn_linear_bwd_weight_workspace_bytes(70001, 16, 16, ctypes.byref(n)) == 0
    assert n.value % (16 * 17 * 4) == 0 and n.value // (16 * 17 * 4) >= 2            # slabs * out * (in + 1) floats
    assert lib.kagnn_linear_bwd_weight_workspace_bytes(10, 0, 16, ctypes.byref(n)) != 0
    assert lib.kagnn_linear_bwd_weight_workspace_bytes(10, 4, 4, None) != 0
    assert lib.kagnn_linear_fwd(None, 3, 10, 64, None, None, 8, 0, None, 8, None) != 0      # ldx < in
    assert b"bad shape" in lib.kagnn_last_error()
    assert lib.kagnn_linear_fwd(None, 64, 10, 64, None, None, 8, 2, None, 8, None) != 0     # relu not 0 / 1
    assert lib.kagnn_linear_fwd(None, 64, 10, 64, None, None, 8, 1, None, 8, None) != 0     # null arrays
    assert b"null array" in lib.kagnn_last_error()
    assert lib.kagnn_linear_fwd(None, 64, 0, 64, None, None, 8, 1, None, 8, None) == 0      # no rows: nothing to do
    assert lib.kagnn_linear_bwd_input(None, 4, None, 0, 10, 8, None, 64, None, 64, None) != 0          # ldgy < out
    assert lib.kagnn_linear_bwd_input(None, 8, None, 0, 10, 8, None, 64, None, 64, None) != 0          # null arrays
    assert lib.kagnn_linear_bwd_input(None, 8, None, 0, 0, 8, None, 64, None, 64, None) == 0
    assert lib.kagnn_linear_bwd_weight(None, 64, None, 8, None, 0, 10, 64, 8, None, None, None, 0, None) != 0   # null gW


def test_make_any_model():
    params = dict(architecture="mlp", conv_type="gin", mp_layers=2, num_features=6, hidden_channels=8, num_classes=3, skip=False,
                  hidden_layers=3, dropout=0.5, grid_size=4, spline_order=3)
    m = harness.make_any_model(params)
    assert type(m) is B.GNN_Nodes and len(m.convs[0].nn) == 3 and m.lay_out.in_features == 8 and m.dropout.p == 0.5
    assert type(harness.make_any_model(dict(params, architecture="kan"))) is kagnn_amd.GKAN_Nodes
    with pytest.raises(ValueError):
        harness.make_model(params)                       # the older factory still refuses 'mlp'


REFERENCE_CLASSES = [
    ("node_classification_clean/models.py", "GNN_Nodes", B.GNN_Nodes),
    ("graph_classification/models.py", "GIN", B.GIN), ("graph_classification/models.py", "GCN", B.GCN),
    ("graph_classification/models.py", "GAT", B.GAT),
    ("graph_regression/models.py", "GIN", B.GINRegression), ("graph_regression/models.py", "GCN", B.GCNRegression),
]


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference tree is not on this machine")
@pytest.mark.parametrize("path,name,cls", REFERENCE_CLASSES, ids=[f"{p.split('/')[0]}.{n}" for p, n, _ in REFERENCE_CLASSES])
def test_constructor_parameters_match_the_reference_sources(path, name, cls):
    """the reference cannot be imported without torch_geometric: its models.py is read with ast"""
    tree = ast.parse(open(os.path.join(REFERENCE, path)).read())
    node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == name)
    init = next(n for n in node.body if isinstance(n, ast.FunctionDef) and n.name == "__init__")
    ref_names = [a.arg for a in init.args.args][1:]
    ref_defaults = [ast.literal_eval(d) for d in init.args.defaults]
    sig = inspect.signature(cls.__init__)
    assert list(sig.parameters)[1:] == ref_names
    ours = [p.default for p in sig.parameters.values() if p.default is not inspect.Parameter.empty]
    assert ours == ref_defaults


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference tree is not on this machine")
@pytest.mark.parametrize("path,fn", [("node_classification_clean/models.py", B.make_mlp_nodes), ("graph_classification/models.py", B.make_mlp),
                                     ("graph_regression/models.py", B.make_mlp)], ids=["node", "graph_classification", "graph_regression"])
def test_make_mlp_parameters_match_the_reference_sources(path, fn):
    tree = ast.parse(open(os.path.join(REFERENCE, path)).read())
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "make_mlp")
    assert list(inspect.signature(fn).parameters) == [a.arg for a in node.args.args]


def test_run_reference_installs_the_package_baselines(tmp_path):
    saved = {k: sys.modules.get(k) for k in ("ekan", "fastkan", "models")}
    try:
        mod = run_reference.install("node", str(tmp_path))
        with pytest.raises(ImportError, match="torch_geometric baselines"):       # the default: the explaining stand-in
            mod.GNN_Nodes("gin", 1, 3, 4, 2)
        mod = run_reference.install("node", str(tmp_path), baselines="package")
        assert mod.GNN_Nodes is B.GNN_Nodes and mod.GKAN_Nodes is kagnn_amd.GKAN_Nodes and sys.modules["models"] is mod
        mod = run_reference.install("graph_classification", None, baselines="package")
        assert (mod.GIN, mod.GCN, mod.GAT) == (B.GIN, B.GCN, B.GAT) and mod.KAGIN is kagnn_amd.KAGIN
        mod = run_reference.install("graph_regression", None, baselines="package")
        assert (mod.GIN, mod.GCN) == (B.GINRegression, B.GCNRegression) and mod.KAGIN is kagnn_amd.KAGINRegression
        mod = run_reference.install("graph_regression", None)
        with pytest.raises(ImportError):
            mod.GIN(5, 3, 1, 8, 2, 1, 0.0, False)
        with pytest.raises(ValueError, match="baselines"):
            run_reference.install("node", None, baselines="torch")
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_dense_layer_kernels_use_no_scratch():
    objdir = os.path.join(ROOT, "kagnn_amd", "lib", "obj")
    if not os.path.isdir(objdir) or not shutil.which("c++filt") or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no build objects / LLVM tools on this machine (the library was shipped prebuilt)")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = [k for k in kr.collect(objdir) if k["tu"] == "linear"]
    names = [k["demangled"] for k in rows]
    assert sum("linear_gemm_kernel<" in n for n in names) >= 12 and any("linear_dw_reduce_kernel" in n for n in names), names
    # both MFMA shapes are instantiated: 32x32x2 and 16x16x4
    assert any("linear_gemm_kernel<32," in n for n in names) and any("linear_gemm_kernel<16," in n for n in names)
    for k in rows:
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k
        assert k.get("group_segment_fixed_size", 0) % 16 == 0, k           # LDS carve-outs keep 16-byte alignment
    covered = {r[0] for r in kr.hot_path_report(rows)}
    assert set(names) <= covered, "the spill gate of tools/kernel_resources.py does not cover every dense-layer kernel"
