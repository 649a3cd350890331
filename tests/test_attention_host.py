"""Host side of the dense attention entry points (csrc/attention.hip) and of ``AttentionWithFastKANTransform``: ABI surface, the
workspace query, argument checks, the reference's constructor / parameter surface (tests/golden/g15_attention.npz, made by
tests/golden/make_golden_attention.py from the reference class), what the Python surface refuses, the ``fastkan`` alias of
``run_reference`` and the spill gate -- all without a GPU."""
import ctypes
import importlib.util
import inspect
import json
import os
import re
import shutil
import sys

import numpy as np
import pytest
import torch

import kagnn_amd
from kagnn_amd import _build, _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("kagnn_attention_fwd", "kagnn_attention_bwd_workspace_bytes", "kagnn_attention_bwd")
KAGNN_ERR_ARG, KAGNN_ERR_UNSUPPORTED = -1, -3
GOLDEN = os.path.join(ROOT, "tests", "golden", "g15_attention.npz")


def _lib_or_build():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return z, json.loads(str(z["meta"]))


def test_version_and_symbols():
    lib = _lib_or_build()
    assert lib.kagnn_version() >= 271
    header = open(os.path.join(ROOT, "include", "kagnn_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED and hasattr(lib, name), name
    assert "attention.hip" in _build.SOURCES


def test_workspace_query():
    lib = _lib_or_build()
    fn = lib.kagnn_attention_bwd_workspace_bytes
    n = ctypes.c_size_t(0)
    for gate in (0, 1):
        last = 0
        for q in (0, 1, 63, 1024, 1 << 16):                                  # monotone in Q
            assert fn(2, q, 1024, 8, 16, gate, ctypes.byref(n)) == 0
            assert n.value >= last, (q, gate)
            last = n.value
        last = 0
        for k in (0, 1, 63, 1024, 1 << 16, 1 << 22):                          # monotone in K, and bounded in it:
            assert fn(2, 1024, k, 8, 16, gate, ctypes.byref(n)) == 0
            assert n.value >= last, (k, gate)
            last = n.value
            # D [B, Q, H] and, with a gate, d_o [B, Q, H * c]: no term in Q * K * H (that would be 2 * 1024 * k * 8 * 4 bytes)
            assert n.value <= 2 * 1024 * 8 * (1 + 16 * gate) * 4 + 64, (k, gate, n.value)
    assert fn(1, 8, 8, 2, 4, 0, None) == KAGNN_ERR_ARG
    assert fn(-1, 8, 8, 2, 4, 0, ctypes.byref(n)) == KAGNN_ERR_ARG
    assert fn(1, -1, 8, 2, 4, 0, ctypes.byref(n)) == KAGNN_ERR_ARG
    assert fn(1, 8, 1 << 31, 2, 4, 0, ctypes.byref(n)) == KAGNN_ERR_ARG
    assert fn(1, 8, 8, 0, 4, 0, ctypes.byref(n)) == KAGNN_ERR_ARG
    for c in (0, 129, -3):
        assert fn(1, 8, 8, 2, c, 0, ctypes.byref(n)) == KAGNN_ERR_UNSUPPORTED
        assert b"head_dim" in lib.kagnn_last_error() and b"1..128" in lib.kagnn_last_error()
    for c in (1, 5, 128):
        assert fn(1, 8, 8, 2, c, 1, ctypes.byref(n)) == 0


def test_argument_checks_need_no_device():
    lib = _lib_or_build()
    one = ctypes.c_void_p(16)       # never dereferenced: every call below fails its checks first
    big = 1 << 24

    def f(wq=one, ldq=8, wk=one, ldk=8, wv=one, ldv=8, bias=None, bbs=0, brs=0, gate=None, ldg=0, B=2, Q=5, K=7, H=2, c=4, o=one, ldo=8,
          ou=None, ldou=0, stats=None):
        return lib.kagnn_attention_fwd(wq, ldq, wk, ldk, wv, ldv, bias, bbs, brs, gate, ldg, B, Q, K, H, c, 0.5, o, ldo, ou, ldou, stats, None)

    def b(go=one, ldgo=8, wq=one, ldq=8, wk=one, ldk=8, wv=one, ldv=8, bias=None, bbs=0, brs=0, gate=None, ldg=0, ou=one, ldou=8, stats=one,
          B=2, Q=5, K=7, H=2, c=4, gq=one, ldgq=8, gk=one, ldgk=8, gv=one, ldgv=8, gb=None, gbbs=0, gbrs=0, gg=None, ldgg=0, ws=one,
          nbytes=big):
        return lib.kagnn_attention_bwd(go, ldgo, wq, ldq, wk, ldk, wv, ldv, bias, bbs, brs, gate, ldg, ou, ldou, stats, B, Q, K, H, c, 0.5,
                                       gq, ldgq, gk, ldgk, gv, ldgv, gb, gbbs, gbrs, gg, ldgg, ws, nbytes, None)

    for c in (0, 129, -1):
        assert f(c=c) == KAGNN_ERR_UNSUPPORTED and b(c=c) == KAGNN_ERR_UNSUPPORTED
        assert b"head_dim" in lib.kagnn_last_error()
    for kw in (dict(B=-1), dict(Q=-1), dict(K=-1), dict(H=0), dict(Q=1 << 31)):
        assert f(**kw) == KAGNN_ERR_ARG and b(**kw) == KAGNN_ERR_ARG, kw
    for kw in (dict(ldq=7), dict(ldk=7), dict(ldv=7), dict(ldo=7), dict(gate=one, ldg=7), dict(ou=one, ldou=7, stats=one),
               dict(ou=one, ldou=8),                        # the ungated o without the statistics
               dict(bias=one, bbs=-1), dict(bias=one, brs=-7),
               dict(wq=None), dict(wk=None), dict(wv=None), dict(o=None)):
        assert f(**kw) == KAGNN_ERR_ARG, kw
    assert f(B=0, wq=None, wk=None, wv=None, o=None) == 0          # nothing to do: no launch, no pointer needed
    assert f(Q=0, wq=None, wk=None, wv=None, o=None) == 0
    for kw in (dict(ldgo=7), dict(ldq=7), dict(ldk=7), dict(ldv=7), dict(ldou=7), dict(ldgq=7), dict(ldgk=7), dict(ldgv=7),
               dict(gate=one, ldg=8, gg=one, ldgg=7), dict(gate=one, ldg=8),             # a gate without its gradient
               dict(gg=one, ldgg=8),                                                     # a gate gradient without a gate
               dict(bias=one, bbs=-1), dict(bias=one, bbs=35, brs=7, gb=one, gbbs=35, gbrs=6),       # g_bias rows overlap
               dict(bias=one, bbs=0, brs=7, gb=one, gbbs=0, gbrs=7),                     # g_bias is dense: no broadcast on the write side
               dict(go=None), dict(wq=None), dict(wk=None), dict(wv=None), dict(ou=None), dict(stats=None),
               dict(gq=None), dict(gk=None), dict(gv=None), dict(ws=None), dict(ws=ctypes.c_void_p(20)), dict(nbytes=16)):
        assert b(**kw) == KAGNN_ERR_ARG, kw
    assert b(nbytes=16) == KAGNN_ERR_ARG and b"workspace too small" in lib.kagnn_last_error()
    assert b(B=0, go=None, wq=None, wk=None, wv=None, ou=None, stats=None, gq=None, gk=None, gv=None, ws=None, nbytes=0) == 0


def test_constructor_and_parameters_match_the_reference(golden):
    z, meta = golden
    assert str(inspect.signature(kagnn_amd.AttentionWithFastKANTransform.__init__, eval_str=True)) == meta["signature"]
    assert kagnn_amd.fastkan.AttentionWithFastKANTransform is kagnn_amd.AttentionWithFastKANTransform
    for case in meta["cases"]:
        m = kagnn_amd.AttentionWithFastKANTransform(*case["dims"], gating=case["gating"])
        assert {n: list(p.shape) for n, p in m.named_parameters()} == case["param_shapes"]
        assert list(case["param_shapes"]) == [n for n, _ in m.named_parameters()]          # the same order
        assert m.norm == case["dims"][3] ** -0.5 and m.num_heads == case["dims"][4] and m.gating == case["gating"]
        assert (m.linear_g is None) == (not case["gating"])


def test_state_dict_round_trip(golden):
    z, meta = golden
    for case in meta["cases"]:
        m = kagnn_amd.AttentionWithFastKANTransform(*case["dims"], gating=case["gating"])
        state = {n: torch.from_numpy(z[f"{case['name']}/state/{n}"]) for n in case["state_keys"]}
        m.load_state_dict(state, strict=True)
        back = m.state_dict()
        assert list(back) == case["state_keys"]
        for n in state:
            assert torch.equal(back[n], state[n]), n


def test_dimensions_of_one_raise_the_reference_assertion():
    for dims in ((1, 4, 3, 4, 2), (6, 1, 3, 4, 2), (6, 4, 1, 4, 2), (6, 4, 3, 1, 1)):
        with pytest.raises(AssertionError, match="Do not use layernorms on 1D inputs"):
            kagnn_amd.AttentionWithFastKANTransform(*dims)
    kagnn_amd.AttentionWithFastKANTransform(6, 4, 3, 1, 2)          # head_dim 1 is fine while num_heads * head_dim > 1


def test_python_surface_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.dense_attention(torch.zeros(1, 5, 8), torch.zeros(1, 7, 8), torch.zeros(1, 7, 8), 2, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.dense_attention(torch.zeros(1, 5, 8), torch.zeros(1, 7, 8), torch.zeros(1, 7, 8), 2, 0.5, bias=torch.zeros(1, 5, 7),
                            gate=torch.zeros(1, 5, 8))
    m = kagnn_amd.AttentionWithFastKANTransform(6, 4, 3, 4, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(5, 6), torch.zeros(7, 4), torch.zeros(7, 3))


def test_name_resolves_through_run_reference():
    from kagnn_amd import run_reference
    saved = {n: sys.modules.get(n) for n in ("ekan", "fastkan", "models")}
    try:
        run_reference.install("node")
        assert sys.modules["fastkan"].AttentionWithFastKANTransform is kagnn_amd.AttentionWithFastKANTransform
        ns = {}
        exec("from fastkan import AttentionWithFastKANTransform as A", ns)
        assert ns["A"] is kagnn_amd.AttentionWithFastKANTransform
    finally:
        for n, mod in saved.items():
            if mod is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = mod


def test_attention_kernels_do_not_spill():
    objdir = os.path.join(ROOT, "kagnn_amd", "lib", "obj")
    if not os.path.isdir(objdir) or not shutil.which("c++filt") or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no build objects / LLVM tools on this machine (the library was shipped prebuilt)")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = [k for k in kr.collect(objdir) if k["tu"] == "attention"]
    names = sorted(k["demangled"] for k in rows)
    # {forward, dQ, dK/dV} x head_dim <= 32 / 64 / 128 x {no bias, bias}, and the gate pre-pass of the backward
    want = sorted(["attention_%s_kernel<%d,%s>" % (which, nch, bias) for which in ("fwd", "bwd_q", "bwd_kv") for nch in (2, 4, 8)
                   for bias in ("false", "true")] + ["attention_gate_bwd_kernel"])
    assert [n.replace("kagnn::", "") for n in names] == want, names
    bad = [k for k in rows if k["vgpr_spill_count"] or k["private_segment_fixed_size"]]
    assert not bad, [(k["name"], k["vgpr_spill_count"], k["private_segment_fixed_size"]) for k in bad]
    covered = {r[0] for r in kr.hot_path_report(rows)}
    assert set(names) <= covered, "the spill gate of tools/kernel_resources.py does not cover every attention kernel"
