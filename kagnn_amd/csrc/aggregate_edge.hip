// Gradient of the neighbour aggregation (aggregate.hip) with respect to its EDGE WEIGHTS: a sampled dense-dense product over the
// edges.  For the by-destination CSR the forward is
//   out[i] = out_scale[i] * (self_scale * s(i) * x[i] + sum_{e in row i} w[e] * s(col[e]) * x[col[e]]) + bias
// so for CSR position e of row i, j = col[e]:
//   d loss / d w[e] = out_scale[i] * s(j) * <gout[i, :F], x[j, :F]>
// which is what torch_geometric differentiates through `edge_weight` (GNNExplainer's edge mask, learned edge weights).  HBM-bound
// like the forward and shaped like it: a destination row is owned by a group of LPR lanes that keep one float4 of gout[i] each in
// registers (the row is read once), walk the row's neighbour list with four independent 16-byte gathers of x[j] in flight and
// reduce each edge's dot product across the group with a butterfly (a fixed order: bit-reproducible).  Every edge is written
// exactly once -- `perm` is a permutation -- so there are no atomics and no merge pass: rows above `hub_threshold` edges go through
// the forward's hub segments {row, e0, e1}, one workgroup each, and are skipped by the row kernel.
#include "common.h"
#include "host.h"

namespace kagnn {

namespace {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float dot4(const float4& a, const float4& b) {
    return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)));
}

// sum over the LPR lanes of a group (aligned, LPR a power of two): every lane of the group ends with the same bits.  All lanes
// of a group run the same trip counts, so a lane only ever reads lanes that are active with it
template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

// CSR position e of row `row` (j = col[e]) receives its value; a dropped self loop is exactly 0 whatever the operands hold
__device__ __forceinline__ void put(const EdgeGradArgs& a, int e, int j, long row, float os, float d) {
    float v = os * (a.in_scale ? a.in_scale[j] : 1.0f) * d;
    if (a.skip_self && j == (int)row) v = 0.0f;
    a.out[a.perm ? a.perm[e] : e] = v;
}

// edges e, e + stride, ... < e_end of one row for a lane group: g = this lane's four columns of gout[row], cc its
// column offset into x; a lane beyond F (`on` false) loads inside the row and contributes an exact 0, whatever it loaded;
// lead = the lane that stores
template <int LPR>
__device__ __forceinline__ void walk(const EdgeGradArgs& a, long row, const float4& g, float os, int e, int e_end, int stride, int cc,
                                     bool on, bool lead) {
    for (; e + 3 * stride < e_end; e += 4 * stride) {       // four gathers of a lane group in flight
        const int j0 = a.col[e], j1 = a.col[e + stride], j2 = a.col[e + 2 * stride], j3 = a.col[e + 3 * stride];
        const float4 v0 = ld4(a.x + (long)j0 * a.ldx + cc);
        const float4 v1 = ld4(a.x + (long)j1 * a.ldx + cc);
        const float4 v2 = ld4(a.x + (long)j2 * a.ldx + cc);
        const float4 v3 = ld4(a.x + (long)j3 * a.ldx + cc);
        const float d0 = group_sum<LPR>(on ? dot4(g, v0) : 0.0f), d1 = group_sum<LPR>(on ? dot4(g, v1) : 0.0f);
        const float d2 = group_sum<LPR>(on ? dot4(g, v2) : 0.0f), d3 = group_sum<LPR>(on ? dot4(g, v3) : 0.0f);
        if (lead) {
            put(a, e, j0, row, os, d0);
            put(a, e + stride, j1, row, os, d1);
            put(a, e + 2 * stride, j2, row, os, d2);
            put(a, e + 3 * stride, j3, row, os, d3);
        }
    }
    for (; e < e_end; e += stride) {
        const int j = a.col[e];
        const float4 v = ld4(a.x + (long)j * a.ldx + cc);
        const float d = group_sum<LPR>(on ? dot4(g, v) : 0.0f);
        if (lead) put(a, e, j, row, os, d);
    }
}

// LPR lanes hold a row of F <= 4 * LPR columns.  A row owns R = max(LPR, 16) lanes: at F <= 16 the R / LPR lane groups of a row are
// edge slots (slot k walks edges s + k, s + k + EP, ...), as in agg_rows_ep_kernel, so short rows do not idle a wave
template <int LPR>
__global__ __launch_bounds__(256) void edge_grad_rows_kernel(EdgeGradArgs a) {
    constexpr int R = LPR < 16 ? 16 : LPR, EP = R / LPR;
    const long row = (blockIdx.x * 256L + threadIdx.x) / R;
    if (row >= a.N) return;                                   // (uniform over the row's lanes)
    const int s = a.rowptr[row], t = a.rowptr[row + 1];
    if (t - s > a.hub_threshold) return;                      // edge_grad_hub_kernel's
    const int lr = threadIdx.x % R, cg = lr % LPR, eg = lr / LPR, c4 = cg * 4;
    const bool on = c4 < a.F;
    const int cc = on ? c4 : 0;
    const float4 g = ld4(a.gout + row * a.ldg + cc);
    walk<LPR>(a, row, g, a.out_scale ? a.out_scale[row] : 1.0f, s + eg, t, EP, cc, on, cg == 0);
}

// one workgroup per hub segment {row, e0, e1}: its 256 / LPR lane groups take the segment's edges round-robin
template <int LPR>
__global__ __launch_bounds__(256) void edge_grad_hub_kernel(EdgeGradArgs a, const int* __restrict__ seg) {
    const int row = seg[3 * blockIdx.x], e0 = seg[3 * blockIdx.x + 1], e1 = seg[3 * blockIdx.x + 2];
    constexpr int G = 256 / LPR;
    const int grp = threadIdx.x / LPR, cg = threadIdx.x % LPR, c4 = cg * 4;
    const bool on = c4 < a.F;
    const int cc = on ? c4 : 0;
    const float4 g = ld4(a.gout + (long)row * a.ldg + cc);
    walk<LPR>(a, row, g, a.out_scale ? a.out_scale[row] : 1.0f, e0 + grp, e1, G, cc, on, cg == 0);
}

// any F / any alignment: a wave per row, lane = column (mod 64), edges walked in order, the 64 partial dots meet in a butterfly
__global__ __launch_bounds__(256) void edge_grad_generic_kernel(EdgeGradArgs a) {
    const long row = blockIdx.x * 4L + (threadIdx.x >> 6);
    if (row >= a.N) return;                                   // (wave-uniform)
    const int lane = threadIdx.x & 63;
    const int s = a.rowptr[row], t = a.rowptr[row + 1];
    const float os = a.out_scale ? a.out_scale[row] : 1.0f;
    const float* gr = a.gout + row * a.ldg;
    for (int e = s; e < t; ++e) {
        const int j = a.col[e];
        const float* xr = a.x + (long)j * a.ldx;
        float d = 0.0f;
        for (int f = lane; f < a.F; f += 64) d = fmaf(gr[f], xr[f], d);
        d = group_sum<64>(d);
        if (lane == 0) put(a, e, j, row, os, d);
    }
}

bool vec4_ok(const EdgeGradArgs& a) {
    auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    return a.F % 4 == 0 && a.F <= 256 && a.ldx % 4 == 0 && a.ldg % 4 == 0 && al(a.x) && al(a.gout);
}

}  // namespace

int aggregate_edge_grad(const EdgeGradArgs& a, const int* hub_seg, long num_hub_seg, hipStream_t st) {
    if (a.N == 0 || a.E == 0) return KAGNN_OK;
    EdgeGradArgs b = a;
    if (!vec4_ok(a)) {
        b.hub_threshold = 0x7fffffff;
        edge_grad_generic_kernel<<<cdiv(a.N, 4), 256, 0, st>>>(b);
        KAGNN_LAUNCH_CHECK();
        return KAGNN_OK;
    }
    if (num_hub_seg <= 0 || hub_seg == nullptr) b.hub_threshold = 0x7fffffff;
#define ROWS(LPR)                                                                                         \
    {                                                                                                     \
        edge_grad_rows_kernel<LPR><<<cdiv(a.N * (LPR < 16 ? 16 : LPR), 256), 256, 0, st>>>(b);            \
        KAGNN_LAUNCH_CHECK();                                                                             \
        if (b.hub_threshold != 0x7fffffff) {                                                              \
            edge_grad_hub_kernel<LPR><<<(unsigned)num_hub_seg, 256, 0, st>>>(b, hub_seg);                 \
            KAGNN_LAUNCH_CHECK();                                                                         \
        }                                                                                                 \
    }
    if (a.F <= 4) ROWS(1) else if (a.F <= 8) ROWS(2) else if (a.F <= 16) ROWS(4) else if (a.F <= 32) ROWS(8)
    else if (a.F <= 64) ROWS(16) else if (a.F <= 128) ROWS(32) else ROWS(64)
#undef ROWS
    return KAGNN_OK;
}

}  // namespace kagnn
