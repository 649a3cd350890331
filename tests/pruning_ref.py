"""fp64 restatements shared by tests/test_pruning_host.py and tests/test_gpu_pruning.py: the edge functions of a ``KANLinear`` (fixed
symbolic edges included) from ``oracle.kan_oracle.bspline_bases``, their moments, and pykan's attribution rule in numpy."""
import copy

import numpy as np
import torch
import torch.nn.functional as F

from kagnn_amd.symbolic import SYMBOLIC_LIB
from oracle import kan_oracle as orc


def phi_of(x, knots, k, bw, sw, sc, dtype=torch.float64):
    """phi[n, o, i] in ``dtype``; ``bw`` / ``sc`` may be None; ``knots`` [in, G+2k+1]"""
    x = x.to(dtype)
    w = sw.to(dtype) if sc is None else sw.to(dtype) * sc.to(dtype).unsqueeze(-1)
    phi = torch.einsum("nic,oic->noi", orc.bspline_bases(x, knots.to(dtype), k), w)
    if bw is not None:
        phi = phi + F.silu(x)[:, None, :] * bw.to(dtype)
    return phi


def moments64(phi):
    """mean [o, i] and centred sum of squares [o, i] of phi [n, o, i], two passes in fp64"""
    phi = phi.double()
    mean = phi.mean(0)
    return mean, (phi - mean).square().sum(0)


def layer_phi64(layer, x):
    """phi[n, o, i] of a ``kagnn_amd.KANLinear`` as it now is, in fp64 on the CPU: "0" edges are 0, fixed function edges their formula"""
    layer = copy.deepcopy(layer).cpu()
    x = x.detach().cpu().double()
    sc = layer.spline_scaler.detach() if layer.enable_standalone_scale_spline else None
    phi = phi_of(x, layer.grid, layer.spline_order, layer.base_weight.detach(), layer.spline_weight.detach(), sc)
    for (o, i), (name, row) in layer._fixed_state().items():
        if name == "0":
            phi[:, o, i] = 0.0
        else:
            a, b, c, d = (float(v) for v in row.detach().double())
            phi[:, o, i] = c * SYMBOLIC_LIB[name][1](a * x[:, i] + b) + d
    return phi


def chain_forward64(layers, x, zero_out=None):
    """the chain in fp64; ``zero_out``: {l: units of width l (the inputs of layer l) whose OUTGOING edges are zeroed}"""
    h = x.detach().cpu().double()
    for l, layer in enumerate(layers):
        phi = layer_phi64(layer, h)
        if zero_out and l in zero_out:
            phi[:, :, list(zero_out[l])] = 0.0
        h = phi.sum(2)
    return h


def attribute64(layers, x, out_scores=None, normalise=True):
    """pykan's rule restated in numpy on fp64 statistics -> dict of lists, as ``Attribution``'s fields"""
    h = x.detach().cpu().double()
    edge_std, out_std = [], []
    for layer in layers:
        phi = layer_phi64(layer, h)
        edge_std.append(phi.std(0, unbiased=True).numpy())
        h = phi.sum(2)
        out_std.append(h.std(0, unbiased=True).numpy())
    L = len(layers)
    node = [None] * (L + 1)
    edge = [None] * L
    node[L] = np.ones(out_std[-1].shape) if out_scores is None else np.asarray(out_scores, dtype=np.float64)
    for l in range(L - 1, -1, -1):
        scale = (out_std[l] + 1e-4) if normalise else np.ones_like(out_std[l])
        edge[l] = edge_std[l] * (node[l + 1] / scale)[:, None]
        node[l] = edge[l].sum(0)
    return {"edge_std": edge_std, "out_std": out_std, "edge_scores": edge, "node_scores": node}


def offset_case(n=70001, fin=4, fout=4, G=5, k=3, seed=0):
    """check 2 of the issue: bw = 0, sw = 5 + 0.01 randn, x uniform in [-0.99, 0.99]: phi ~ 5 +- 0.01"""
    gen = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, fin, generator=gen) * 2 - 1) * 0.99
    sw = 5.0 + 0.01 * torch.randn(fout, fin, G + k, generator=gen)
    return x, torch.zeros(fout, fin), sw, orc.make_knots(fin, G, k)


def offset_reference(x, bw, sw, knots, k=3, chunk=8192):
    """(mean64, sqrt(m2/N) in fp64 by two passes, the same by ONE pass in fp32: sum phi^2 - (sum phi)^2 / N, E32: error of a TWO-pass
    fp32 evaluation)"""
    n = x.size(0)
    pieces = [phi_of(x[r:r + chunk], knots, k, bw, sw, None) for r in range(0, n, chunk)]
    mean = sum(p.sum(0) for p in pieces) / n
    m2 = sum((p - mean).square().sum(0) for p in pieces)
    p32 = [phi_of(x[r:r + chunk], knots, k, bw, sw, None, torch.float32) for r in range(0, n, chunk)]
    s1 = sum(p.sum(0) for p in p32)
    s2 = sum(p.square().sum(0) for p in p32)
    naive = ((s2 - s1 * s1 / n).clamp(min=0) / n).sqrt()
    mean32 = s1 / n
    two_pass = (sum((p - mean32).square().sum(0) for p in p32) / n).sqrt()
    want = (m2 / n).sqrt()
    return mean, want, naive, float((two_pass.double() - want).abs().max())


def random_chain(widths, seed, grid_size=5, spline_order=3):
    """a ``kagnn_amd.KAN`` on the CPU with the edge tests' operand scales: bw, sw ~ 0.3 randn, sc ~ 1 + 0.5 randn"""
    import kagnn_amd
    gen = torch.Generator().manual_seed(seed)
    chain = kagnn_amd.KAN(list(widths), grid_size=grid_size, spline_order=spline_order)
    with torch.no_grad():
        for layer in chain.layers:
            layer.base_weight.copy_(0.3 * torch.randn(layer.base_weight.shape, generator=gen))
            layer.spline_weight.copy_(0.3 * torch.randn(layer.spline_weight.shape, generator=gen))
            layer.spline_scaler.copy_(1.0 + 0.5 * torch.randn(layer.spline_scaler.shape, generator=gen))
    return chain, gen


def planted_chain(seed, widths=(4, 8, 3), dead_units=(2, 5), dead_edges=(), rows=400):
    """a chain with PLANTED dead parts: the outgoing ``base_weight`` / ``spline_scaler`` columns of the hidden units ``dead_units`` (of
    width 1) and the entries ``dead_edges = [(layer, o, i)]`` are scaled by 1e-4.  -> chain (CPU), rows x"""
    chain, gen = random_chain(widths, seed)
    with torch.no_grad():
        for u in dead_units:
            chain.layers[1].base_weight[:, u] *= 1e-4
            chain.layers[1].spline_scaler[:, u] *= 1e-4
        for l, o, i in dead_edges:
            chain.layers[l].base_weight[o, i] *= 1e-4
            chain.layers[l].spline_scaler[o, i] *= 1e-4
    return chain, 0.8 * torch.randn(rows, widths[0], generator=gen)


def outside_band(scores, threshold):
    """the margin condition: no score within a factor 3 of the threshold, so that rounding cannot flip a decision"""
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    return bool(np.all((s < threshold / 3) | (s > 3 * threshold)))


def per_feature_chain(seed=3):
    """[4, 6, 3]; the second layer on jittered per-feature knots, with one fixed function edge on a kept column, one on a removed
    column, and a "0" edge on a removed row of the first layer"""
    chain, gen = random_chain((4, 6, 3), seed)
    l1 = chain.layers[1]
    with torch.no_grad():
        l1.grid.add_((2.0 / 5) * 0.3 * (torch.rand(l1.grid.shape, generator=gen) - 0.5))
    l1.refresh_knots()
    l1.fix_symbolic(2, 4, "sin", params=(1.3, 0.2, 0.7, -0.1))
    l1.fix_symbolic(0, 1, "tanh", params=(0.9, -0.3, 1.1, 0.2))
    chain.layers[0].fix_symbolic(1, 2, "0")
    chain.layers[0].fix_symbolic(3, 0, "0")
    return chain, 0.8 * torch.randn(64, 4, generator=gen)
