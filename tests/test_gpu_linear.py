"""``ops.linear`` (csrc/linear.hip: y = act(x W^T + b) and its two gradients, exact fp32 MFMA) against fp64 torch on the CPU.

Every case runs with the bias on and off and the fused ReLU on and off, and checks y, gx, gW and gb at ``helpers.assert_close``'s
default bound (2e-5 of the reference tensor's own maximum plus the 1e-4 element-wise rule): an exact fp32 fma chain sits near
1e-7 * sum|a b|, so no relaxation.

ReLU mask.  The kernel contract is ``m = (y > 0)`` on the SAVED device output (torch's threshold_backward), so the fp64 reference of
gx / gW / gb is built with that mask; the test additionally asserts that the mask equals ``(z64 > 0)`` on every element with
``|z64| > 1e-5 max|z64|`` -- the mask cannot be arbitrary, and no compared value is left out.

Strides and memory.  x and gy are column slices of wider matrices (ld > width; x starts one column in, i.e. off a 16-byte
boundary, for every other case); y and gx are written through the raw entry points into views of wider buffers whose padding
columns hold a sentinel that must be bit-unchanged afterwards.
"""
import ctypes

import pytest
import torch

from kagnn_amd import _lib, ops
from helpers import assert_close, must_fail

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(1, 1, 1), (1, 5, 3),                         # single row, K below one MFMA step
          (31, 7, 1), (33, 2, 40),                      # odd K, rows just short of / just past one tile, out = 40
          (64, 64, 64), (129, 33, 65), (257, 128, 40),  # exact tiles, and one past in every dimension
          (300, 1433, 16),                              # Cora's first layer: long K, narrow out
          (500, 1024, 16), (1000, 16, 1024),            # time_model's widest hidden size on either side
          (70001, 16, 16)]                              # many row blocks, more than one dW slab
SENTINEL = -12345.5


def _case(n, fin, fout, seed, offset):
    """operands as column slices of wider matrices; fp32 values, fp64 copies on the CPU"""
    g = torch.Generator().manual_seed(seed)
    xw = torch.randn(n, fin + 5, generator=g)
    gyw = torch.randn(n, fout + 3, generator=g)
    w = torch.randn(fout, fin, generator=g) / max(1.0, fin ** 0.5)
    b = torch.randn(fout, generator=g)
    return xw, gyw, w, b, offset


def _run(n, fin, fout, bias, relu, seed=0):
    xw, gyw, w, b, off = _case(n, fin, fout, seed, (n + fin) % 2)
    xd = xw.to(DEV)[:, off:off + fin].requires_grad_(True)          # a view: ld = fin + 5
    gyd = gyw.to(DEV)[:, 1:1 + fout]
    wd = w.to(DEV).requires_grad_(True)
    bd = b.to(DEV).requires_grad_(True) if bias else None
    assert n <= 1 or xd.stride(0) > fin
    y = ops.linear(xd, wd, bd, relu=relu)
    y.backward(gyd)
    # fp64 reference
    x64, w64, gy64 = xw[:, off:off + fin].double(), w.double(), gyw[:, 1:1 + fout].double()
    z64 = x64 @ w64.t() + (b.double() if bias else 0.0)
    y64 = z64.clamp(min=0.0) if relu else z64
    yc = y.detach().cpu()
    if relu:
        m = yc > 0
        if n:
            sure = z64.abs() > 1e-5 * float(z64.abs().max())
            assert torch.equal(m[sure], (z64 > 0)[sure]), "the ReLU mask differs from (z > 0) away from the kink"
        g64 = gy64 * m.double()
    else:
        g64 = gy64
    want = {"y": y64, "gx": g64 @ w64, "gW": g64.t() @ x64, "gb": g64.sum(0)}
    got = {"y": y, "gx": xd.grad, "gW": wd.grad, "gb": bd.grad if bias else None}
    return got, want


@pytest.mark.parametrize("relu", [False, True], ids=["id", "relu"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_linear_against_fp64(shape, bias, relu):
    n, fin, fout = shape
    got, want = _run(n, fin, fout, bias, relu)
    tag = f"linear[{n},{fin},{fout},bias={bias},relu={relu}]"
    for k in ("y", "gx", "gW") + (("gb",) if bias else ()):
        assert got[k] is not None, k
        assert_close(got[k], want[k], what=f"{tag}.{k}")


def test_more_than_one_weight_gradient_slab():
    n, fin, fout = 70001, 16, 16
    nbytes = ops._sizes("kagnn_linear_bwd_weight_workspace_bytes", n, fin, fout)
    assert nbytes % (fout * (fin + 1) * 4) == 0
    assert nbytes // (fout * (fin + 1) * 4) >= 2            # slabs * out * (in + 1) floats (include/kagnn_hip.h)


def test_weight_gradient_is_bit_reproducible():
    n, fin, fout = 70001, 16, 16
    a, _ = _run(n, fin, fout, True, True, seed=3)
    b, _ = _run(n, fin, fout, True, True, seed=3)
    assert torch.equal(a["gW"], b["gW"]) and torch.equal(a["gb"], b["gb"])
    assert torch.equal(a["y"], b["y"]) and torch.equal(a["gx"], b["gx"])


def test_empty_input():
    x = torch.empty(0, 7, device=DEV, requires_grad=True)
    w = torch.randn(3, 7, device=DEV, requires_grad=True)
    b = torch.randn(3, device=DEV, requires_grad=True)
    launches = []
    real = ops._lib.call
    ops._lib.call = lambda name, *a: (launches.append(name), real(name, *a))[1]
    try:
        y = ops.linear(x, w, b, relu=True)
        y.sum().backward()
    finally:
        ops._lib.call = real
    assert y.shape == (0, 3) and x.grad.shape == (0, 7)
    assert not [k for k in launches if k.startswith("kagnn_linear_") and not k.endswith("_bytes")], launches
    assert torch.equal(w.grad, torch.zeros_like(w)) and torch.equal(b.grad, torch.zeros_like(b))


def _raw(name, *args):
    _lib.call(name, *args)


@pytest.mark.parametrize("shape", [(33, 2, 40), (129, 33, 65), (257, 128, 40), (31, 7, 1)], ids=lambda s: "x".join(map(str, s)))
def test_padding_columns_are_never_written(shape):
    """y and gx as column slices of sentinel-filled buffers, through the C entry points"""
    n, fin, fout = shape
    xw, gyw, w, b, off = _case(n, fin, fout, 1, 1)
    xd, gyd = xw.to(DEV)[:, off:off + fin], gyw.to(DEV)[:, 1:1 + fout]
    wd, bd = w.to(DEV), b.to(DEV)
    ybuf = torch.full((n, fout + 7), SENTINEL, device=DEV)
    gxbuf = torch.full((n, fin + 6), SENTINEL, device=DEV)
    yv, gxv = ybuf[:, 3:3 + fout], gxbuf[:, 2:2 + fin]
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ops._stream()
    _raw("kagnn_linear_fwd", P(xd), xd.stride(0), n, fin, P(wd), P(bd), fout, 1, P(yv), ybuf.stride(0), st)
    _raw("kagnn_linear_bwd_input", P(gyd), gyd.stride(0), P(yv), ybuf.stride(0), n, fout, P(wd), fin, P(gxv), gxbuf.stride(0), st)
    torch.cuda.synchronize()
    x64, w64, gy64 = xd.double().cpu(), w.double(), gyd.double().cpu()
    y64 = (x64 @ w64.t() + b.double()).clamp(min=0.0)
    assert_close(yv, y64, what="strided y")
    assert_close(gxv, (gy64 * (yv.cpu() > 0).double()) @ w64, what="strided gx")
    for buf, lo, width in ((ybuf, 3, fout), (gxbuf, 2, fin)):
        pad = torch.cat([buf[:, :lo], buf[:, lo + width:]], dim=1)
        assert torch.equal(pad, torch.full_like(pad, SENTINEL)), "a padding column was written"


def test_mutation_guards():
    n, fin, fout = 129, 33, 65
    got, want = _run(n, fin, fout, True, True)
    must_fail(torch.zeros_like(got["gb"]), want["gb"], what="gb zeroed")
    y = got["y"].detach().clone()
    y[n // 2] += 1e-3 * float(want["y"].abs().max())
    must_fail(y, want["y"], what="y moved by 1e-3 of its maximum in one row")


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.linear(torch.randn(4, 3), torch.randn(2, 3))
