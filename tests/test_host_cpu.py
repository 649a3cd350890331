"""CPU-side checks (no GPU, no compute calls): the C-ABI library loads and exports every symbol that
include/kagnn_hip.h declares; the module surface mirrors the reference's names, constructor
signatures and state_dict keys; the product refuses CPU tensors instead of falling back."""
import inspect
import os
import re
import sys

import pytest
import torch

import kagnn_amd
from kagnn_amd import _lib, rccl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the two C-ABI libraries: header, ctypes host module, minimum number of entry points
ABIS = [("kagnn_hip.h", _lib, 20), ("kagnn_rccl.h", rccl, 8)]


def _declared_symbols(header="kagnn_hip.h"):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(kagnn_[a-z0-9_]+)\s*\(", src)))


@pytest.mark.parametrize("header,mod,least", ABIS, ids=[a[0] for a in ABIS])
def test_library_exports_every_declared_symbol(header, mod, least):
    if not os.path.exists(mod.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = mod.load()
    declared = _declared_symbols(header)
    assert len(declared) >= least
    for name in declared:
        assert hasattr(lib, name), f"{name} is declared in include/{header} but not exported"
    assert sorted(mod.EXPORTED) == declared, "ctypes signature table and header disagree"
    assert (lib.kagnn_version() if mod is _lib else lib.kagnn_rccl_version()) >= 100


@pytest.mark.parametrize("header,mod,least", ABIS, ids=[a[0] for a in ABIS])
def test_ctypes_signatures_match_the_header_prototypes(header, mod, least):
    """every prototype of include/kagnn_hip.h (kagnn_rccl.h) against the ctypes table of kagnn_amd/_lib.py (rccl.py): number of
    parameters, and per parameter pointer / 64-bit integer / 32-bit integer / float / size_t -- a drifted signature would
    otherwise only show up as garbage arguments on the GPU box"""
    import ctypes
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = dict(re.findall(r"\b(kagnn_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S))

    def kind_c(param):
        param = " ".join(param.split())
        if "*" in param:
            return "ptr"
        if re.search(r"\b(int64_t|uint64_t)\b", param):
            return "i64"
        if re.search(r"\bsize_t\b", param):
            return "size"
        if re.search(r"\bfloat\b", param):
            return "f32"
        if re.search(r"\b(int32_t|int)\b", param):
            return "i32"
        raise AssertionError(f"unclassified C parameter: {param}")

    def kind_py(t):
        if t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
            return "ptr"
        return {ctypes.c_int64: "i64", ctypes.c_uint64: "i64", ctypes.c_size_t: "size", ctypes.c_float: "f32",
                ctypes.c_int32: "i32"}[t]

    sizes = {"i64": 8, "size": ctypes.sizeof(ctypes.c_size_t), "ptr": ctypes.sizeof(ctypes.c_void_p)}
    checked = 0
    for name, (_res, argtypes) in mod._SIGNATURES.items():
        params = protos[name].strip()
        c_kinds = [] if params in ("", "void") else [kind_c(q) for q in params.split(",")]
        py_kinds = [kind_py(t) for t in argtypes]
        assert len(c_kinds) == len(py_kinds), f"{name}: header has {len(c_kinds)} parameters, ctypes table {len(py_kinds)}"
        for i, (a, b) in enumerate(zip(c_kinds, py_kinds)):
            assert a == b or sizes.get(a, 4) == sizes.get(b, 4) and {a, b} <= {"i64", "size"}, f"{name}: parameter {i}: header {a}, ctypes {b}"
        checked += 1
    assert checked == len(protos) >= least


def test_state_dict_surface_matches_reference_names():
    m = kagnn_amd.GKAN_Nodes("gin", 2, 10, 8, 3, grid_size=5, spline_order=3)
    keys = set(m.state_dict())
    for k in ("convs.0.eps", "convs.0.nn.layers.0.base_weight", "convs.0.nn.layers.1.spline_scaler",
              "convs.1.nn.layers.0.grid", "bns.0.running_mean", "lay_out.spline_weight"):
        assert k in keys, k
    assert m.lay_out.in_features == 10 + 2 * 8
    m = kagnn_amd.GKAN_Nodes("gcn", 2, 10, 8, 3)
    keys = set(m.state_dict())
    for k in ("convs.0.bias", "convs.0.lin.base_weight", "convs.1.lin.grid"):
        assert k in keys, k
    assert m.convs[0].lin.grid_size == 4                      # the reference's default grid_size=4
    f = kagnn_amd.GFASTKAN_Nodes("gin", 3, 6, 4, 2)
    keys = set(f.state_dict())
    for k in ("convs.0.nn.layers.0.layernorm.weight", "convs.0.nn.layers.0.rbf.grid",
              "convs.2.nn.layers.1.spline_linear.weight", "lay_out.base_linear.bias"):
        assert k in keys, k
    assert not f.convs[0].nn.layers[0].rbf.grid.requires_grad
    with pytest.raises(ValueError, match="unknown conv_type"):
        kagnn_amd.GKAN_Nodes("sage", 1, 4, 4, 2)


def test_constructor_signatures_match_reference():
    sig = inspect.signature(kagnn_amd.KANLinear.__init__)
    assert list(sig.parameters)[1:] == ["in_features", "out_features", "grid_size", "spline_order", "scale_noise",
                                        "scale_base", "scale_spline", "enable_standalone_scale_spline",
                                        "base_activation", "grid_eps", "grid_range"]
    assert sig.parameters["grid_size"].default == 5 and sig.parameters["spline_order"].default == 3
    sig = inspect.signature(kagnn_amd.GIKANLayer.__init__)
    assert list(sig.parameters)[1:] == ["in_feat", "out_feat", "grid_size", "spline_order", "hidden_dim", "nb_layers"]
    assert sig.parameters["hidden_dim"].default == 16
    sig = inspect.signature(kagnn_amd.FastKANLayer.__init__)
    assert list(sig.parameters)[1:] == ["input_dim", "output_dim", "grid_min", "grid_max", "num_grids",
                                        "use_base_update", "use_layernorm", "base_activation",
                                        "spline_weight_init_scale"]


def _reference_state(z, prefix):
    return {k: torch.from_numpy(z[f"{prefix}.{k}"]) for k in z[f"{prefix}.keys"]}


def test_reference_state_dict_loads(golden):
    """a state_dict produced by the reference's own KAN / FastKAN (tests/golden/g14_reference_surface.npz) loads into ours
    unchanged, and ours gives back the same keys, shapes and values (so the reference loads it in turn)."""
    z = golden("g14_reference_surface")
    ref = _reference_state(z, "kan")
    ours = kagnn_amd.KAN([6, 5, 4], grid_size=4, spline_order=2)
    ours.load_state_dict(ref)
    back = ours.state_dict()
    assert list(back) == list(ref)
    for k, v in ref.items():
        assert torch.equal(back[k], v), k
    rf = _reference_state(z, "fastkan")
    of = kagnn_amd.FastKAN([6, 5, 4], num_grids=3)
    of.load_state_dict(rf)
    assert [n for n, _ in of.named_parameters()] == list(z["fastkan.param_names"])


def test_init_distributions_match_reference(golden):
    """same init *distributions* (not RNG streams): compare moments of many draws (the reference's KANLinear(64, 64) drawn
    under seed 1, stored in g14_reference_surface)."""
    z = golden("g14_reference_surface")
    a = _reference_state(z, "init")
    torch.manual_seed(2)
    b = kagnn_amd.KANLinear(64, 64)
    for name in ("base_weight", "spline_weight", "spline_scaler"):
        x, y = a[name], getattr(b, name).detach()
        assert abs(float(x.std()) - float(y.std())) < 0.1 * float(x.std()), name
        assert abs(float(x.mean()) - float(y.mean())) < 0.05 * float(x.std()) + 1e-4, name
    assert torch.equal(a["grid"], b.grid)


def test_cpu_tensors_are_refused_not_emulated():
    layer = kagnn_amd.KANLinear(4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer(torch.randn(2, 4))
    fk = kagnn_amd.FastKANLayer(4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fk(torch.randn(2, 4))
    conv = kagnn_amd.GIKANLayer(4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv(torch.randn(5, 4), torch.zeros(2, 3, dtype=torch.long))


def test_make_model_mirrors_the_reference_factory():
    from kagnn_amd.harness import count_params, make_model
    base = dict(conv_type="gin", mp_layers=2, num_features=10, hidden_channels=8, num_classes=3, skip=True,
                hidden_layers=2, dropout=0.0, grid_size=4, spline_order=3, heads=2)
    kan = make_model(dict(base, architecture="kan"))
    fk = make_model(dict(base, architecture="fastkan", conv_type="gat"))
    assert type(kan).__name__ == "GKAN_Nodes" and type(fk).__name__ == "GFASTKAN_Nodes"
    assert count_params(kan) > 0 and fk.lay_out.input_dim == 10 + 2 * 8 * 2
    import pytest as _pt
    with _pt.raises(ValueError):
        make_model(dict(base, architecture="mlp"))


def test_ogb_encoders_surface():
    import torch
    import kagnn_amd
    a, b = kagnn_amd.AtomEncoder(6), kagnn_amd.BondEncoder(6)
    assert [e.num_embeddings for e in a.atom_embedding_list] == [119, 5, 12, 12, 10, 6, 6, 2, 2]
    assert [e.num_embeddings for e in b.bond_embedding_list] == [5, 6, 2]
    assert a(torch.zeros(3, 9, dtype=torch.long)).shape == (3, 6) and b(torch.ones(4, 3, dtype=torch.long)).shape == (4, 6)
    m = kagnn_amd.KAGINRegression(9, 3, 2, 8, 2, 4, 3, 1, 0.0, ogb_encoders=True)
    assert "atom_encoder.atom_embedding_list.0.weight" in m.state_dict() and "bond_encoder.bond_embedding_list.2.weight" in m.state_dict()


def test_size_queries_and_argument_checks_need_no_gpu():
    """the *_bytes queries are host arithmetic and bad arguments are refused before any HIP call: both work here"""
    from ctypes import byref, c_size_t
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    a, b = c_size_t(0), c_size_t(0)
    for mode in (_lib.PREC_FP32, _lib.PREC_SPLIT, _lib.PREC_FP32_GRID):
        assert lib.kagnn_kan_pack_bytes(64, 64, 5, 3, mode, byref(a), byref(b)) == 0 and a.value > 0 and b.value > 0
    assert lib.kagnn_kan_bwd_weight_workspace_bytes(1_000_000, 64, 64, 5, 3, _lib.PREC_SPLIT, byref(a)) == 0
    assert 0 < a.value < (1 << 30)                                   # per-workgroup slabs, not per-row storage
    assert lib.kagnn_kan_fwd_workspace_bytes(1_000_000, 64, 64, 5, 3, _lib.PREC_SPLIT, byref(a)) == 0 and a.value == 0
    assert lib.kagnn_kan_fwd_workspace_bytes(2708, 1433, 32, 5, 3, _lib.PREC_SPLIT, byref(a)) == 0 and a.value > 0   # split-K
    assert lib.kagnn_softmax_xent_workspace_bytes(1000, byref(a)) == 0 and a.value > 0
    assert lib.kagnn_kan_grid_refit_workspace_bytes(1000, 8, 5, 3, byref(a)) == 0 and a.value > 0
    assert lib.kagnn_gat_att_grad_workspace_bytes(1000, 4, 16, byref(a)) == 0 and a.value > 0
    assert lib.kagnn_batchnorm_workspace_bytes(1000, 64, byref(a)) == 0 and a.value > 0
    # refused with a message, no crash, no device needed
    assert lib.kagnn_kan_pack_bytes(64, 64, 5, 7, _lib.PREC_SPLIT, byref(a), byref(b)) != 0          # spline order 7
    assert b"spline_order" in lib.kagnn_last_error()
    assert lib.kagnn_kan_pack_bytes(64, 64, 5, 3, 9, byref(a), byref(b)) != 0                         # unknown mode
    assert lib.kagnn_kan_pack_bytes(0, 64, 5, 3, _lib.PREC_SPLIT, byref(a), byref(b)) != 0
    assert lib.kagnn_kan_linear_fwd(None, 3, 10, None, 64, 64, 5, 3, _lib.PREC_SPLIT, None, None, 64, None, 0, None) != 0   # ldx < in
    assert b"argument check failed" in lib.kagnn_last_error()
    assert lib.kagnn_softmax_xent_fwd(None, 4, 10, 40, None, None, 1, None, None, None, None, 0, None) != 0            # ld < classes
    assert lib.kagnn_kan_grid_refit_workspace_bytes(0, 8, 5, 3, byref(a)) != 0                                         # no rows
    # round 3: the read-out over column blocks, the layer backward with the norm inside
    import ctypes
    w4 = (ctypes.c_int32 * 4)(64, 64, 64, 64)
    assert lib.kagnn_kan_fwd_parts_ok(w4, 4, 256, 40, 5, 3, _lib.PREC_SPLIT) == 1
    assert lib.kagnn_kan_fwd_parts_ok(w4, 4, 256, 40, 5, 3, _lib.PREC_FP32) == 0
    assert lib.kagnn_kan_fwd_parts_ok((ctypes.c_int32 * 2)(128, 40), 2, 168, 40, 5, 3, _lib.PREC_SPLIT) == 0          # 40 is not whole chunks
    assert lib.kagnn_kan_fwd_parts_ok((ctypes.c_int32 * 9)(*([64] * 9)), 9, 576, 40, 5, 3, _lib.PREC_SPLIT) == 0        # > 8 chunks
    assert lib.kagnn_gin_kan_layer_bwd_bn_workspace_bytes(1_000_000, 64, byref(a)) == 0 and a.value > 0
    assert lib.kagnn_gin_kan_layer_bwd_bn_workspace_bytes(10, 0, byref(a)) != 0
    assert lib.kagnn_aggregate_sum_add(None, 4, None, 8, None, None, None, 10, 8, 1.0, None, None, None, 0, None, 0, 0, None, 0, None, 0,
                                       None) != 0                                                                    # null arrays / ldx < F


def test_rccl_library_size_query_and_argument_checks_need_no_gpu():
    """libkagnn_rccl.so (include/kagnn_rccl.h): the workspace query is host arithmetic on top of libkagnn_hip's own queries and
    bad arguments are refused before any HIP / RCCL call"""
    from ctypes import byref, c_size_t
    lib = rccl.load()
    f, b = c_size_t(0), c_size_t(0)
    n, out = 1_000_000, 64
    assert lib.kagnn_sharded_kan_linear_workspace_bytes(n, 8, out, 5, 3, _lib.PREC_SPLIT, 8, 4, byref(f), byref(b)) == 0
    mat = n * out * 4
    assert 2 * mat <= f.value < 2 * mat + (1 << 20)                  # partial sums + rank-major blocks (tall input: no kernel scratch)
    assert 2 * mat < b.value < 2 * mat + (1 << 30)                   # gathered blocks + gathered gradient + weight-gradient slabs
    assert lib.kagnn_sharded_kan_linear_workspace_bytes(n, 8, 60, 5, 3, _lib.PREC_SPLIT, 8, 4, byref(f), byref(b)) != 0     # 60 % 8
    assert b"divisible" in lib.kagnn_rccl_last_error()
    assert lib.kagnn_sharded_kan_linear_workspace_bytes(n, 8, out, 5, 3, _lib.PREC_SPLIT, 8, 0, byref(f), byref(b)) != 0    # 0 chunks
    assert lib.kagnn_sharded_kan_linear_workspace_bytes(n, 8, out, 5, 7, _lib.PREC_SPLIT, 8, 1, byref(f), byref(b)) != 0    # order 7
    assert b"spline_order" in lib.kagnn_rccl_last_error()           # (libkagnn_hip's message is carried through)
    assert lib.kagnn_sharded_kan_linear_fwd(None, 8, 10, None, 8, out, 5, 3, _lib.PREC_SPLIT, None, None, None, 8, 0, 1, None, 0,
                                            None, None) != 0         # no communicator
    assert b"comm is NULL" in lib.kagnn_rccl_last_error()
    assert lib.kagnn_rccl_comm_init(None, 2, 0, None) != 0
    assert lib.kagnn_rccl_comm_destroy(None) == 0
    with pytest.raises(ValueError):
        rccl.Communicator(b"short", 1, 0, torch.device("cpu"))


def test_hot_path_kernels_do_not_spill_registers():
    """Round 2's slow kernels (column-moments forward, config 3's weight gradient, the headline weight gradient) were all
    visible in the compiler's own metadata: spilled VGPRs / scratch bytes per lane.  tools/kernel_resources.py reads that
    metadata from the objects _build leaves in kagnn_amd/lib/obj; an instantiation on a measured path that spills fails here."""
    import importlib.util
    import shutil
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    objdir = os.path.join(root, "kagnn_amd", "lib", "obj")
    if not os.path.isdir(objdir) or not shutil.which("c++filt") or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no build objects / LLVM tools on this machine (the library was shipped prebuilt)")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = kr.collect(objdir)
    report = kr.hot_path_report(rows)
    names = [r[0] for r in report]
    # the gate really covers the kernels bench.py times (a renamed kernel must not silently drop out of it)
    for must in ("kan_sparse_fwd_kernel<2,false,false,false,-1,false,false>", "kan_sparse_fwd_kernel<2,false,true,false,-1,false,false>",
                 "kan_sparse_fwd_kernel<2,false,false,true,8,false,false>", "kan_sparse_fwd_kernel<2,false,false,false,-1,true,false>",
                 "kan_split_dw_kernel<3,false,1,4,false,false>", "kan_split_dx_kernel<3,2,false,1,false,false,false,false,false>",
                 "kan_split_dx_kernel<3,2,false,0,false,true,false,false,false>", "kan_split_dw_w2_kernel<3,1>",
                 "kan_split_dx_w2_kernel<4,3>", "kan_split_dw_kernel<0,false,1,4,false,false>", "agg_rows_v4_kernel<16,false>",
                     "agg_rows_v4_kernel<16,true>", "agg_hub_merge_kernel<16,true>",      # (with the column statistics of the result: the norm backward fold)
                 # round 4: the wide-layer weight gradient and the read-out kernels that apply a folded BatchNorm1d to their rows
                 "kan_split_dw_shared_kernel<0,4>", "kan_split_dw_kernel<3,false,1,3,true,false>", "kan_split_dx_kernel<3,2,false,1,false,false,true,false,false>",
                     "kan_split_dx_kernel<3,2,false,1,false,false,true,true,false>",      # (+ the column statistics of the stored gradient rows)
                 # round 5: the single-product (KAGNN_PREC_HALF) instantiations of the config-2 model's kernels
                 "kan_sparse_fwd_kernel<2,false,false,false,-1,false,true>", "kan_sparse_fwd_kernel<2,false,true,false,-1,false,true>",
                 "kan_sparse_fwd_kernel<2,false,false,false,-1,true,true>", "kan_split_dw_kernel<3,false,1,4,false,true>",
                 "kan_split_dw_kernel<3,false,1,3,true,true>", "kan_split_dx_kernel<3,2,false,1,false,false,false,false,true>",
                 "kan_split_dx_kernel<3,2,false,0,false,true,false,false,true>", "kan_split_dx_kernel<3,2,false,1,true,false,false,false,true>",
                 "kan_split_dx_kernel<3,2,false,1,false,false,true,true,true>",
                 # round 5: the 128-output forward of config 3's layers (two waves per SIMD, one accumulator set)
                 "kan_sparse_fwd_kernel<4,true,false,false,-1,false,false>", "kan_sparse_fwd_kernel<4,true,true,false,-1,false,false>",
                 "kan_sparse_fwd_kernel<4,false,false,false,-1,false,false>"):
        assert must in names, f"{must} is not covered by the spill gate: {sorted(names)[:5]}..."
    bad = [r for r in report if r[1] > r[3] or r[2] > r[4]]
    assert not bad, "hot-path kernels spill registers: " + "; ".join(f"{r[0]}: {r[1]} VGPRs / {r[2]} B" for r in bad)
    # one wave per SIMD is the floor: nothing may need more than the 512-entry file
    assert all(k["vgpr_count"] <= 512 for k in rows)


def test_gat_kernel_cases_reach_every_gat_kernel_and_variant():
    """tests/test_gpu_gat.py restates how csrc/gat.hip and ops._GatFn choose their kernels (``gat_kernels``) and parametrises its
    kernel-level cases so that each of them runs.  Without a GPU: the restated thresholds are still the ones in the sources, and
    the case list still reaches every kernel, every KC instantiation of gat_att_grad_partial, the torch fallback, the hub kernels
    behind both row paths, a long row inside the row kernels, a source hub, the last channel chunk and the layout refusal of the
    packed path -- moving a threshold fails here instead of thinning the coverage."""
    import test_gpu_gat as tg
    from kagnn_amd import ops
    gat = open(os.path.join(ROOT, "kagnn_amd", "csrc", "gat.hip")).read()
    csr = open(os.path.join(ROOT, "kagnn_amd", "csrc", "csr.hip")).read()
    for snippet in ("constexpr int kGatMaxK = 8;", "constexpr int kPk = 2;", "C == 4 || C == 8 || C == 16 || C == 32 || C == 64",
                    "H * C <= 64 * kPk", "if (C > 16 * kGatMaxK)", "if (H * C > 1024)",
                    "if (kc <= 1) L(1); else if (kc <= 2) L(2); else if (kc <= 4) L(4); else if (kc <= 8) L(8); else L(16);"):
        assert snippet in gat, f"gat.hip no longer holds {snippet!r}: update gat_kernels in tests/test_gpu_gat.py"
    for snippet in ("constexpr int kSmallMax = 1 << 16;", "E >= 1 && E <= kSmallMax && N >= 1 && N <= kSmallMax",
                    "if (t - s <= T) return;"):
        assert snippet in csr, f"csr.hip no longer holds {snippet!r}: update gat_kernels in tests/test_gpu_gat.py"
    assert "heads * channels <= 1024" in inspect.getsource(ops._GatFn.backward)
    assert (tg.PACKED_C, tg.PACKED_MAX_HC, tg.MAX_C, tg.ATT_GRAD_MAX_HC, tg.SMALL_CSR_MAX) == ((4, 8, 16, 32, 64), 128, 128, 1024, 1 << 16)
    reached = set().union(*(tg.case_kernels(c) for c in tg.KERNEL_CASES))
    need = {"gat_logits", "gat_fwd_rows", "gat_bwd_dst_rows", "gat_bwd_src_rows", "gat_fwd", "gat_bwd_dst", "gat_bwd_src",
            "gat_fwd_hub", "gat_bwd_dst hub", "packed + hub", "wave + hub", "long row in the row kernels", "source hub",
            "packed refused by layout", "wave chunks 8", "hub chunks 8", "att grad torch fallback", "gat_att_grad_finish"}
    need |= {f"gat_att_grad_partial<{k}>" for k in (1, 2, 4, 8, 16)}
    assert not need - reached, sorted(need - reached)
    assert tg.gat_kernels(1, 129, 10, 10, 1) == {"refused"}


def test_every_newer_kernel_family_has_a_heap_and_a_guard_case():
    """tests/test_gpu_poison_families.py registers one builder or more per kernel family that tests/test_gpu_poison.py's own case
    list predates; both of its tests run over the whole table, so a registered case IS a heap case and a guard case.  Without a GPU:
    no family has lost its cases, every case belongs to a family, the source each family is named for is still there, the eleven
    kagnn::* ops are all called, and a lowered guarded-buffer floor is stated only by cases that run raw ops."""
    import test_gpu_poison as tp
    import test_gpu_poison_families as tf
    sources = {"linear": ["linear.hip"], "high order": ["kan_high_order.hip"], "edge norms": ["kan_edge.hip", "fastkan_edge.hip"],
               "attention": ["attention.hip"], "grid refinement": ["kan_grid.hip"], "edge gradient": ["aggregate_edge.hip"],
               "classification": ["classify.hip"], "node classification": ["nodeclass.hip"], "regression": ["regress.hip", "loss.hip"],
               "device datasets": ["batch.hip", "csr.hip"], "primitives": ["aggregate.hip", "aggregate_bf16.hip"],
               "library ops": ["api.hip"], "overlap": ["fused_calls.hip"], "parts": ["kan_split_bwd.hip"]}
    assert set(tf.FAMILIES) == set(sources), sorted(set(tf.FAMILIES) ^ set(sources))
    for family, files in sources.items():
        assert tf.FAMILIES[family], f"no heap / guard case is left for the family '{family}'"
        for name in files:
            assert os.path.exists(os.path.join(ROOT, "kagnn_amd", "csrc", name)), name
    listed = [c for cases in tf.FAMILIES.values() for c in cases]
    assert sorted(listed) == sorted(tf.CASES) and not set(tf.CASES) & set(tp.CASES)
    assert len(tf.FAMILIES["edge norms"]) >= 4 and len(tf.FAMILIES["attention"]) >= 4 and len(tf.FAMILIES["linear"]) >= 6
    from kagnn_amd import library
    ops_registered = sorted(n for n in tf.LIBRARY_OPS if hasattr(library, n))
    assert ops_registered == sorted(tf.LIBRARY_OPS) and len(ops_registered) == 11
    assert [f"kagnn::{n} eager" for n in tf.LIBRARY_OPS] == tf.FAMILIES["library ops"]
    for name, (mode, build, floor) in tf.CASES.items():
        assert mode in ("split", "half", "fp32") and callable(build)
        raw = name in tf.FAMILIES["library ops"] or name.startswith(("segment pool", "harness.Adam"))
        assert floor == 3 or (raw and 1 <= floor), (name, floor)
    for fn in (tf.test_blind_to_the_heap, tf.test_writes_stay_inside_their_buffers):
        (mark,) = [m for m in fn.pytestmark if m.name == "parametrize"]
        assert list(mark.args[1]) == list(tf.CASES)


def test_assert_close_scales_by_the_reference_itself_and_can_fail():
    """tests/helpers.assert_close (round 5): the bound is relative to max|reference| of the tensor, so small
    tensors are held to the same RELATIVE accuracy as large ones; zeros and 1e-3 perturbations are rejected whatever the
    magnitude; an all-zero reference must be matched exactly unless the caller supplies a noise estimate."""
    import helpers
    if helpers.SOFT:
        pytest.skip("KAGNN_TEST_SOFT=1 records instead of raising")
    g = torch.Generator().manual_seed(0)
    for mag in (1e-6, 1e-3, 1.0, 1e4):
        w = torch.randn(100, 7, generator=g, dtype=torch.float64) * mag
        helpers.assert_close(w * (1 + 1e-6), w, 2e-5, what="tiny perturbation")
        helpers.must_fail(torch.zeros_like(w), w, 2e-5, what=f"zeros at magnitude {mag}")
        helpers.must_fail(w * (1 + 1e-3), w, 1e-4, what=f"1e-3 perturbation at magnitude {mag}")
        helpers.assert_close(w + 1e-3 * mag, w, 2e-5, what="inside an explicit noise floor", noise=100 * mag, elementwise=False)
    z = torch.zeros(5)
    helpers.assert_close(z, z, what="exact zeros")
    helpers.must_fail(z + 1e-30, z, what="zero reference, no noise estimate")
    helpers.assert_close(z + 1e-9, z, 1e-4, what="zero reference with a noise estimate", noise=1e-4)


def test_half_mode_statement_can_fail_and_the_routing_table_is_the_documented_one():
    """tests/helpers.half_statement, with the oracles alone: (a) a tensor that was never rounded -- the unrounded oracle's own, i.e. what
    a three-product kernel would deliver where a single-product one is expected -- fails the floor; (b) the rounding oracle with ONE
    GEMM left unrounded (the weight gradient's) fails the L2 bound or the 5x separation for every weight gradient at (1000, 24, 40),
    while its y and gx pass; (c) the routing table of helpers.half_routing at the shapes the GPU cases are built around."""
    import helpers
    from oracle import kan_oracle as orc
    if helpers.SOFT:
        pytest.skip("KAGNN_TEST_SOFT=1 records instead of raising")
    n, fi, fo, G, k = 1000, 24, 40, 5, 3
    assert helpers.half_routing(fi, fo, G, k) == (False, True, True)
    gen = torch.Generator().manual_seed(n + fi)
    p = orc.init_kan_linear(fi, fo, G, k, gen)
    x = torch.randn(n, fi, generator=gen) * 0.8
    gy = torch.randn(n, fo, generator=gen) * torch.logspace(-3, 2, n).unsqueeze(1)
    plain, rounded = helpers.half_layer_oracles(x, gy, p, k, "TSS")
    cls = helpers.half_classes("TSS")
    try:
        assert torch.equal(rounded["y"], plain["y"])                     # the narrow forward is three-product: left alone
        helpers.half_statement({"gx": rounded["gx"]}, plain, rounded, cls, "teeth")       # the right answer passes, floor included
        for name in ("gx",) + helpers.KAN_GRADS:
            # (a) never rounded, judged by a rounding oracle that agrees with it: only the floor can object
            with pytest.raises(AssertionError, match="distance from the unrounded oracle"):
                helpers.half_statement({name: plain[name]}, plain, plain, cls, "teeth")
            with pytest.raises(AssertionError):                           # ... and against the real rounding oracle it fails parity too
                helpers.half_statement({name: plain[name]}, plain, rounded, cls, "teeth")
        # a GEMM whose flag is down is the plain oracle's, and leaves the other two as they are
        none = helpers.half_layer_oracles(x, gy, p, k, "TTT")[1]
        for name in plain:
            helpers.assert_close(none[name], plain[name], 1e-12, what="unflagged oracle " + name)
        assert all(torch.equal(rounded[name], helpers.half_layer_oracles(x, gy, p, k, "SSS")[1][name]) for name in ("gx",) + helpers.KAN_GRADS)
        # (b) one operand left unrounded
        _, mutant = helpers.half_layer_oracles(x, gy, p, k, "TST")
        helpers.half_statement({"gx": mutant["gx"]}, plain, rounded, cls, "teeth")
        for name in helpers.KAN_GRADS:
            helpers.assert_close(mutant[name], plain[name], 1e-12, what="weight gradients beside a rounded input gradient: " + name)
        _, beside = helpers.half_layer_oracles(x, gy, p, k, "TTS")
        for name in helpers.KAN_GRADS:                      # ... and rounded weight gradients beside an unrounded input gradient
            assert torch.equal(beside[name], rounded[name]), name
        for name in helpers.KAN_GRADS:
            with pytest.raises(AssertionError):
                helpers.half_statement({name: mutant[name]}, plain, rounded, cls, "teeth")
            # ... by the L2 bound AND the separation, not only by the max norm (which objects first, at 3.4e-4 against 3e-4)
            lr, lp = helpers.l2_rel(mutant[name], rounded[name]), helpers.l2_rel(mutant[name], plain[name])
            assert lr > 4 * helpers.HALF_L2_TOL and 5.0 * lr > lp, (name, lr, lp)
            with pytest.raises(AssertionError, match="L2 distance from the rounding oracle"):
                helpers.half_parity(mutant[name], rounded[name], plain[name], "teeth", flip_tol=1.0)
        # a three-product tensor that is not the bits of PREC_SPLIT, or that misses the fp64 bound
        with pytest.raises(AssertionError, match="the bits of PREC_SPLIT"):
            helpers.half_statement({"y": plain["y"]}, plain, rounded, cls, "teeth", split={"y": plain["y"] * (1 + 1e-7)})
        with pytest.raises(AssertionError, match="three-product"):
            helpers.half_statement({"y": plain["y"] * (1 + 1e-4)}, plain, rounded, cls, "teeth", split={"y": plain["y"] * (1 + 1e-4)})
    finally:
        helpers.HALF_REPORT.pop("teeth", None)
    # (c) (in, out, G, k) -> single-product (forward, input gradient, weight gradients)
    for shape, want in {(64, 64, 5, 3): (True, True, True), (33, 17, 4, 3): (True, True, True), (32, 64, 5, 3): (False, True, True),
                        (64, 128, 5, 3): (False, False, True), (64, 100, 5, 3): (True, False, True), (72, 192, 5, 3): (True, False, True),
                        (64, 256, 5, 3): (False, False, True), (64, 65, 5, 3): (True, False, True), (64, 64, 6, 3): (False, False, False),
                        (64, 64, 5, 2): (False, False, False), (40, 70, 20, 3): (False, False, False)}.items():
        assert helpers.half_routing(*shape) == want, (shape, helpers.half_routing(*shape), want)


def test_norm_sums_side_channel_drops_sums_when_the_parked_gradient_was_accumulated_into_in_place():
    """ops.NormSums: the parked column sums describe the gradient tensor AS IT WAS when the next layer's aggregation
    wrote it.  Identity of storage is not enough -- an engine that accumulates a second consumer's gradient into the same tensor
    in place keeps data_ptr / shape / stride and changes the contents; the version counter tells.  A second consumer's gradient
    arriving BEFORE the park (the parked tensor already carries it: sums valid) and AFTER it (stale sums: dropped)."""
    from kagnn_amd import ops
    sums = torch.ones(2, 4)
    g = torch.zeros(8, 4)
    g.add_(1.0)                                   # another consumer's gradient, accumulated BEFORE the aggregation parked its sums
    ns = ops.NormSums()
    ns.park(sums, g)
    assert ns.take(g) is sums                     # untouched since the park: the sums describe it
    assert ns.take(g) is None                     # (taken once)
    ns.park(sums, g)
    g.add_(1.0)                                   # ... and AFTER: same storage, new contents
    assert ns.take(g) is None
    ns.park(sums, g)
    assert ns.take(g.clone()) is None             # a new tensor (what autograd's out-of-place accumulation produces)
    ns.park(sums, g)
    assert ns.take(g.view(8, 4)) is sums          # an alias of the unmodified tensor is still that gradient


def _run_standin(tmp_path):
    import json
    import subprocess
    out = tmp_path / "report.json"
    script = os.path.join(ROOT, "tests", "standin", "time_model_standin.py")
    r = subprocess.run([sys.executable, "-m", "kagnn_amd.run_reference", script, str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(out.read_text())


def test_run_reference_resolves_the_scripts_own_import_lines(tmp_path):
    """`python -m kagnn_amd.run_reference <script>`: a script carrying time_model.py:13-15's exact import lines (`from utils import *`,
    `from models import GNN_Nodes, GKAN_Nodes, GFASTKAN_Nodes`) runs unedited -- `models` / `ekan` / `fastkan` resolve to this
    package, `utils` to the script's own directory, GNN_Nodes to a class that explains itself when torch_geometric is absent; without
    a GPU every forward is refused loudly (no CPU path)."""
    rep = _run_standin(tmp_path)
    assert set(rep["classes"]) == {"GKAN_Nodes/gcn", "GKAN_Nodes/gin", "GFASTKAN_Nodes/gcn", "GFASTKAN_Nodes/gin"}
    for k, v in rep["classes"].items():
        assert v["module"] == "kagnn_amd.models" and v["params"] > 0, (k, v)
        if rep["device"] == "cpu":
            assert "no CPU fallback" in v["error"], v
    try:
        import torch_geometric  # noqa: F401
    except ImportError:
        assert rep["GNN_Nodes"].startswith("ImportError") and "torch_geometric" in rep["GNN_Nodes"]


def test_kagin_model_struct_mirror_matches_the_header():
    """kagnn_kagin_model_t (include/kagnn_hip.h) against its ctypes mirror kagnn_amd._lib.KaginModel: same size as the built library's
    struct, and the same field names in the same order (every field is 8 bytes wide or a float array at the end, so name order + size
    pin the layout)"""
    import ctypes
    src = open(os.path.join(ROOT, "include", "kagnn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    body = re.search(r"typedef struct kagnn_kagin_model \{(.*?)\} kagnn_kagin_model_t;", src, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        # "const float* a[N]" / "int64_t a, b, c" / "const int32_t* rowptr" / "float* x[N]"
        first, *rest = [p.strip() for p in decl.split(",")]
        names.append(re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*(\[[^\]]*\])?$", first).group(1))
        names += [re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*(\[[^\]]*\])?$", p).group(1) for p in rest]
    mirror = [f[0] for f in _lib.KaginModel._fields_]
    assert names == mirror, [(a, b) for a, b in zip(names, mirror) if a != b][:5]
    lib = _lib.load()
    assert lib.kagnn_kagin_model_struct_bytes() == ctypes.sizeof(_lib.KaginModel)
    # size query on an out-of-range description: an error code and a message, not a crash
    m = _lib.KaginModel()
    outs = [ctypes.c_size_t(0) for _ in range(4)]
    assert lib.kagnn_kagin_model_sizes(ctypes.byref(m), *[ctypes.byref(o) for o in outs]) != 0
    assert b"kagnn_kagin_model" in lib.kagnn_last_error()


def test_bench_dump_outputs_samples_the_same_rows_within_the_budget(tmp_path):
    """bench.py --dump-outputs over the budget: every per-node array keeps the same seeded rows (the same ones on every run),
    arrays without a row per node are written whole, everything as float32 within DUMP_BUDGET_BYTES."""
    import numpy as np
    import bench
    n, f = 300_000, 64
    g = torch.Generator().manual_seed(5)
    arrays = {"y": torch.randn(n, f, generator=g), "x_grad": torch.randn(n, f, generator=g).bfloat16(),
              "grad.w": torch.randn(64, 64, 8, generator=g), "loss": torch.tensor(1.5)}
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), arrays, n)
    got = {p.stem: np.load(p) for p in (tmp_path / "a").glob("*.npy")}
    assert set(got) == set(arrays) and all(a.dtype == np.float32 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_BUDGET_BYTES
    keep = got["y"].shape[0]
    assert 0 < keep < n and got["x_grad"].shape == (keep, f)
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(0))[:keep].sort().values
    assert np.array_equal(got["y"], arrays["y"][rows].numpy())
    assert np.array_equal(got["x_grad"], arrays["x_grad"][rows].float().numpy())
    assert np.array_equal(got["grad.w"], arrays["grad.w"].numpy()) and got["loss"] == np.float32(1.5)
    for name, a in got.items():
        assert np.array_equal(a, np.load(tmp_path / "b" / f"{name}.npy")), name


def test_knots_cache_follows_every_host_write_of_the_grid():
    """the knots a compiled KANLinear evaluates on (``_knots_row``: dynamo cannot trace the check behind it) are refreshed by the
    constructor, state loading and every move of the module -- no eager forward needed; a direct write needs ``refresh_knots()``"""
    import copy
    layer = kagnn_amd.KANLinear(5, 3, grid_size=4)
    assert layer._knots_row.dim() == 1 and torch.equal(layer._knots_row, layer.grid[0])
    uniform = layer.grid.clone()
    state = copy.deepcopy(layer.state_dict())
    state["grid"] = state["grid"] + 0.01 * torch.arange(5.0).unsqueeze(1)          # per-feature rows, each still increasing
    layer.load_state_dict(state)
    assert layer._knots_row.shape == (5, 11) and torch.equal(layer._knots_row, state["grid"])
    layer.double()                                                                 # (a move: the cache is a plain attribute)
    assert layer._knots_row.dtype == torch.float32 and torch.equal(layer._knots_row, state["grid"])
    assert layer._knots_key == (layer.grid.data_ptr(), layer.grid._version, layer.grid.device)
    layer.float()
    with torch.no_grad():
        layer.grid.copy_(uniform)                                                  # a direct write: the cache is stale until refreshed
    assert layer._knots_row.dim() == 2
    layer.refresh_knots()
    assert layer._knots_row.dim() == 1 and torch.equal(layer._knots_row, uniform[0])
    with torch.no_grad():
        layer.grid[:, 3] = layer.grid[:, 2]                                        # not strictly increasing: no cache, the forward raises
    layer.refresh_knots()
    assert layer._knots_row is None and layer._knots_key is None
    with pytest.raises(ValueError, match="strictly increasing"):
        layer._knots()
    clone = copy.deepcopy(kagnn_amd.KANLinear(5, 3, grid_size=4))
    assert torch.equal(clone._knots_row, clone.grid[0])
