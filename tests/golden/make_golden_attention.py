#!/usr/bin/env python3
"""Generate tests/golden/g15_attention.npz by IMPORTING the reference's ``AttentionWithFastKANTransform``.

Run in the build container only (``/root/reference`` present):

    python tests/golden/make_golden_attention.py

The reference class (``node_classification_clean/fastkan.py``) is imported read-only and driven on three seeded cases, once in
fp32 and once with the module and its inputs in ``.double()``.  Stored: the constructor's signature as text, the parameter names
and shapes, and per case the state_dict, the inputs, the upstream gradient, the output and every gradient of both runs (data
only -- no reference source travels).  The spline weights of ``linear_q`` / ``linear_k`` are scaled up: at the default init scale
of 0.1 the logits differ by a few hundredths, the softmax is nearly flat and a flat softmax tests little.
"""
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/node_classification_clean"
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

import fastkan as ref_fastkan    # noqa: E402  (reference, read-only)

torch.set_num_threads(1)  # deterministic reduction order in the fixture

LOGIT_GAIN = 6.0          # factor on the linear_q / linear_k spline weights

# (name, leading dims, (q_dim, k_dim, v_dim, head_dim, num_heads), Q, K, gating, bias shape or None)
CASES = [
    ("c0", (), (6, 4, 3, 4, 2), 5, 7, True, (5, 7)),
    ("c1", (2,), (5, 4, 3, 4, 4), 33, 65, False, (1, 33, 65)),       # a bias shared by the batch: the gradient is summed over it
    ("c2", (2, 3), (6, 4, 3, 4, 2), 5, 7, True, None),
]


def npy(t):
    return t.detach().cpu().numpy()


def run(module, q, k, v, bias, gout, dtype):
    module = module.to(dtype)
    ins = {n: t.detach().to(dtype).requires_grad_(True) for n, t in (("q", q), ("k", k), ("v", v), ("bias", bias)) if t is not None}
    for p in module.parameters():
        p.grad = None
    out = module(ins["q"], ins["k"], ins["v"], ins.get("bias"))
    out.backward(gout.to(dtype))
    grads = {"in." + n: t.grad for n, t in ins.items()}
    grads.update({n: p.grad for n, p in module.named_parameters() if p.requires_grad})
    return out, grads


def main():
    arrays = {}
    meta = {"signature": str(inspect.signature(ref_fastkan.AttentionWithFastKANTransform.__init__)), "logit_gain": LOGIT_GAIN, "cases": []}
    for i, (name, lead, dims, nq, nk, gating, bias_shape) in enumerate(CASES):
        torch.manual_seed(1500 + i)
        gen = torch.Generator().manual_seed(2500 + i)
        m = ref_fastkan.AttentionWithFastKANTransform(*dims, gating=gating)
        with torch.no_grad():
            m.linear_q.spline_linear.weight.mul_(LOGIT_GAIN)
            m.linear_k.spline_linear.weight.mul_(LOGIT_GAIN)
            for p in m.parameters():                                  # biases and layernorm affine away from their 0 / 1 init
                if p.requires_grad and p.dim() == 1:
                    p.add_(0.1 * torch.randn(p.shape, generator=gen))
        q = torch.randn(*lead, nq, dims[0], generator=gen) * 0.8
        k = torch.randn(*lead, nk, dims[1], generator=gen) * 0.8
        v = torch.randn(*lead, nk, dims[2], generator=gen) * 0.8
        bias = None if bias_shape is None else torch.randn(*bias_shape, generator=gen) * 0.3
        gout = torch.randn(*lead, nq, dims[0], generator=gen)
        state = {n: t.clone() for n, t in m.state_dict().items()}
        out32, g32 = run(m, q, k, v, bias, gout, torch.float32)
        out64, g64 = run(m, q, k, v, bias, gout, torch.float64)
        with torch.no_grad():                                         # how far from flat the softmax is (printed, not stored)
            md = m.double()
            wq = md.linear_q(q.double()).view(*lead, nq, dims[4], -1) * md.norm
            wk = md.linear_k(k.double()).view(*lead, nk, dims[4], -1)
            s = torch.einsum("...qhc,...khc->...qkh", wq, wk)
            pmax = s.softmax(-2).amax(-2)
        print(f"{name}: logits in [{float(s.min()):.2f}, {float(s.max()):.2f}], largest softmax weight of a row: mean {float(pmax.mean()):.3f} "
              f"(flat would be {1 / nk:.3f}); out fp32 vs fp64 {float((out32.detach().double() - out64.detach()).abs().max() / out64.detach().abs().max()):.2e}")
        meta["cases"].append(dict(name=name, lead=list(lead), dims=list(dims), Q=nq, K=nk, gating=gating, has_bias=bias is not None,
                                  state_keys=list(state), param_shapes={n: list(p.shape) for n, p in m.named_parameters()},
                                  grad_keys=list(g64)))
        for n, t in state.items():
            arrays[f"{name}/state/{n}"] = npy(t)
        for n, t in (("q", q), ("k", k), ("v", v), ("bias", bias), ("gout", gout)):
            if t is not None:
                arrays[f"{name}/{n}"] = npy(t)
        arrays[f"{name}/out32"], arrays[f"{name}/out64"] = npy(out32), npy(out64)
        for n in g64:
            arrays[f"{name}/g32/{n}"], arrays[f"{name}/g64/{n}"] = npy(g32[n]), npy(g64[n])
    arrays["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "g15_attention.npz")
    np.savez_compressed(path, **arrays)
    print(f"g15_attention.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
