// Per-edge activations of a FastKANLayer: the edge functions
//   phi_{o,i}(n) = sum_g spline_weight[o, i*G+g] exp(-((u[n,i] - c_g) / h)^2) + base_weight[o,i] silu(x[n,i]),
//   u = LayerNorm(x) (a layer with one) or x,
// that the layer's forward only ever sums over i (base_linear.bias is per output and no part of phi).  Three results, as for a
// KANLinear (kan_edge.hip), none of which stores phi over the rows:
//   abs sum   S[o,i] = sum_n |phi_{o,i}(n)|
//   its backward under an upstream gS[out,in]: both weight gradients, gx and -- through the layer's own LayerNorm backward
//             (fastkan.hip) -- the two LayerNorm parameter gradients; sign(0) = 0
//   curves    phi[p,o,i] at sample points for the spline branch and, optionally, other points for the base branch
// Exact fp32 in every precision mode (the layer's `mode` does not reach this file); rbf_val is the layer kernels' own, so the
// layer's output is sum_i phi + bias to rounding.  Every num_grids the layer takes (1..kMaxKnots).
//
// Row kernels (abs sum, gx, curves): a workgroup of four waves owns four consecutive features, one per wave; lane = row.  Unlike
// a B-spline, an RBF row is dense over the centres: the G values (and silu) of a (row, feature) are evaluated once into registers
// and reused over the tile's 64 outputs, whose weight rows [w_0 .. w_{GC-1} | bw | gS | 0 0] lie in LDS -- every lane of a wave reads
// the same address (a broadcast, no bank conflicts), 16 bytes at a time.  GC = the centre count rounded up to the kernel's bound
// (zero weights and zero basis values beyond G).  The abs sum keeps one accumulator per output and reduces across lanes once per
// row slab; the slab partials are added in index order (edge_common.h).
//
// Parameter gradients: lane = output with its G+1 weights and accumulators in registers, the rows' dense rows
// [rbf_0 .. rbf_{G-1} | silu] staged 64 at a time through LDS, as in kan_edge_param_kernel; 49 columns at 48 centres.
//
// The kernels live in namespace fastkan_edge so that their symbol names stay apart from the kan_edge_* kernels', which the
// resource gate of that file counts by name.  No atomics anywhere: the same inputs give the same bits.
#include "edge_common.h"
#include "host.h"

namespace kagnn {
namespace fastkan_edge {

enum { EDGE_SUM = 0, EDGE_GX = 1, EDGE_CURVES = 2 };
constexpr int kMaxNQ = 13;                 // widest parameter-gradient kernel: NQ * 4 = 52 dense columns
static_assert(kMaxNQ * 4 >= kMaxKnots + 1, "the widest parameter kernel must hold every centre and the base column");

struct Args {
    const float* x; long ldx; int xcs;       // spline argument (before LayerNorm) of (n, f) at x[n*ldx + f*xcs]   (xcs 0: shared points)
    const float* xb; long ldxb; int xbcs;    // base argument; NULL: the same as x
    long N;
    const float* stats; const float* lnw; const float* lnb;     // LayerNorm: row (mean, rstd) [N, 2], gamma, beta; stats NULL: none
    const float* centers; int ng; float inv_den;
    int in, out;
    const float* sw; const float* bw;        // [out, in*ng] / [out, in]; either may be NULL (that branch is absent)
    long rows_per_slab;
    float* partial;                          // abs sum [slab][out][in]; parameter gradients [slab][in][ng+1][out]
    const float* gS; long ldgS;
    float* gu;                               // gx kernel with LayerNorm: d / du [N, in] (contiguous); gx then holds the base part
    float* gx; long ldgx;
    float* phi;                              // curves [N][out][in]
};

__device__ __forceinline__ float ln_apply(const Args& a, long n, int f, float x) {
    if (!a.stats) return x;                  // (uniform)
    return fmaf((x - a.stats[2 * n]) * a.stats[2 * n + 1], a.lnw[f], a.lnb[f]);      // the layer kernels' own expression
}

template <int GC, int MODE>
__global__ __launch_bounds__(kEdgeThreads) void rows_kernel(Args a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int RS = GC + 4;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* s_w = smem;                                          // [4][64][RS]
    float* s_c = smem + kEdgeFT * kEdgeOB * RS;                 // [GC]
    const int f0 = blockIdx.y * kEdgeFT, f = f0 + wave;
    const bool fok = f < a.in;
    for (int g = threadIdx.x; g < GC; g += kEdgeThreads) s_c[g] = g < a.ng ? a.centers[g] : 0.0f;
    const long n0 = (long)blockIdx.x * a.rows_per_slab, n1 = min(a.N, n0 + a.rows_per_slab);
    const int nob = cdiv(a.out, kEdgeOB);
    const int ob_begin = MODE == EDGE_GX ? 0 : (int)blockIdx.z, ob_end = MODE == EDGE_GX ? nob : ob_begin + 1;
    const float* wrow = s_w + wave * kEdgeOB * RS;
    const float* xb = a.xb ? a.xb : a.x;
    const long ldxb = a.xb ? a.ldxb : a.ldx;
    const int xbcs = a.xb ? a.xbcs : a.xcs;
    const float k2 = -2.0f * a.inv_den * a.inv_den;

    for (int ob = ob_begin; ob < ob_end; ++ob) {
        const int o0 = ob * kEdgeOB, oc = min(kEdgeOB, a.out - o0);
        __syncthreads();                                        // the previous tile's readers are done (first pass: the centres)
        for (int idx = threadIdx.x; idx < kEdgeFT * kEdgeOB * RS; idx += kEdgeThreads) {
            const int j = idx % RS, t = idx / RS, o = t % kEdgeOB, w = t / kEdgeOB;
            const int ff = f0 + w;
            float v = 0.0f;
            if (ff < a.in && o < oc) {
                const long e = (long)(o0 + o) * a.in + ff;
                if (j < a.ng) v = a.sw ? a.sw[e * a.ng + j] : 0.0f;
                else if (j == GC) v = a.bw ? a.bw[e] : 0.0f;
                else if (j == GC + 1) v = MODE == EDGE_GX ? a.gS[(long)(o0 + o) * a.ldgS + ff] : 0.0f;
            }
            s_w[idx] = v;
        }
        __syncthreads();
        if (!fok) continue;

        float acc[MODE == EDGE_SUM ? kEdgeOB : 1];
        if constexpr (MODE == EDGE_SUM) {
#pragma unroll
            for (int o = 0; o < kEdgeOB; ++o) acc[o] = 0.0f;
        }
        for (long n = n0 + lane; n < n1; n += 64) {
            // an absent branch reads nothing: its zero weights must not meet an Inf of the other branch's argument
            const float xs = a.sw ? a.x[n * a.ldx + (long)f * a.xcs] : 0.0f;
            const float xv = a.bw ? xb[n * ldxb + (long)f * xbcs] : 0.0f;
            const float u = ln_apply(a, n, f, xs);
            float r[GC], dr[MODE == EDGE_GX ? GC : 1];
#pragma unroll
            for (int g = 0; g < GC; ++g) {
                const bool live = g < a.ng;
                const float v = rbf_val(u, s_c[g], a.inv_den);
                r[g] = live ? v : 0.0f;
                if constexpr (MODE == EDGE_GX) dr[g] = live ? v * (k2 * (u - s_c[g])) : 0.0f;
            }
            const float sl = siluf(xv);
            const float sg = MODE == EDGE_GX ? silu_gradf(xv) : 0.0f;
            if constexpr (MODE == EDGE_CURVES) {                // a store per output, nothing accumulated: a plain loop
                float* dst = a.phi + (n * a.out + o0) * a.in + f;
#pragma unroll 2
                for (int o = 0; o < oc; ++o) {
                    const float* q = wrow + o * RS;
                    float phi = q[GC] * sl;
#pragma unroll
                    for (int g = 0; g < GC; ++g) phi = __builtin_fmaf(q[g], r[g], phi);
                    dst[(long)o * a.in] = phi;
                }
            } else if constexpr (MODE == EDGE_GX) {
                float gu = 0.0f, gb = 0.0f;
#pragma unroll 2
                for (int o = 0; o < oc; ++o) {
                    const float* q = wrow + o * RS;
                    const float b = q[GC];
                    float phi = b * sl, d = 0.0f;
#pragma unroll
                    for (int g = 0; g < GC; ++g) {
                        phi = __builtin_fmaf(q[g], r[g], phi);
                        d = __builtin_fmaf(q[g], dr[g], d);
                    }
                    const float s = q[GC + 1] * edge_sign(phi);
                    gu = __builtin_fmaf(s, d, gu);
                    gb = __builtin_fmaf(s, b * sg, gb);
                }
                // (the same thread wrote both for the previous tile)
                float* p = a.gx + n * a.ldgx + f;
                if (a.gu) {
                    float* pu = a.gu + n * (long)a.in + f;
                    *pu = ob == 0 ? gu : *pu + gu;
                    *p = ob == 0 ? gb : *p + gb;
                } else {
                    *p = ob == 0 ? gu + gb : *p + (gu + gb);
                }
            } else {
#pragma unroll
                for (int og = 0; og < kEdgeOB; og += 16) {
                    if (og < oc) {                              // (workgroup-uniform)
#pragma unroll
                        for (int oo = 0; oo < 16; ++oo) {
                            const int o = og + oo;
                            const float* q = wrow + o * RS;
                            float phi = q[GC] * sl;
#pragma unroll
                            for (int g = 0; g < GC; ++g) phi = __builtin_fmaf(q[g], r[g], phi);
                            acc[o] += fabsf(phi);
                        }
                    }
                }
            }
        }
        if constexpr (MODE == EDGE_SUM) {
            float mine = 0.0f;
#pragma unroll
            for (int o = 0; o < kEdgeOB; ++o) {
                float v = acc[o];
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
                mine = lane == o ? v : mine;
            }
            if (lane < oc) a.partial[((long)blockIdx.x * a.out + o0 + lane) * a.in + f] = mine;
        }
    }
}

// T[o,f,c] = sum_n sign(phi_{o,f}(n)) D[n,f,c],  D = [rbf_0 .. rbf_{G-1} | silu]: one slab of it.  NQ * 4 >= G + 1.
template <int NQ>
__global__ __launch_bounds__(kEdgeThreads) void param_kernel(Args a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int CP = NQ * 4;
    if (a.ng + 1 > CP) return;                                  // (the launcher picks NQ; never write past a lane's columns)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float4* s_d = reinterpret_cast<float4*>(smem);              // [4][64][NQ]
    float* s_c = smem + kEdgeFT * 64 * CP;                      // [CP]
    const int f0 = blockIdx.y * kEdgeFT, f = f0 + wave;
    const bool fok = f < a.in;
    for (int g = threadIdx.x; g < CP; g += kEdgeThreads) s_c[g] = g < a.ng ? a.centers[g] : 0.0f;
    const int o = blockIdx.z * kEdgeOB + lane;
    const bool ok = fok && o < a.out;
    float w[CP], acc[CP];
#pragma unroll
    for (int c = 0; c < CP; ++c) { w[c] = 0.0f; acc[c] = 0.0f; }
    if (ok) {
        const long e = (long)o * a.in + f;
#pragma unroll
        for (int c = 0; c < CP; ++c) {
            if (c < a.ng) w[c] = a.sw[e * a.ng + c];
            else if (c == a.ng) w[c] = a.bw ? a.bw[e] : 0.0f;
        }
    }
    __syncthreads();                                            // the centres
    const long n0 = (long)blockIdx.x * a.rows_per_slab, n1 = min(a.N, n0 + a.rows_per_slab);
    float4* mine = s_d + (wave * 64 + lane) * NQ;
    for (long base = n0; base < n1; base += 64) {               // (workgroup-uniform trip count)
        if (base != n0) __syncthreads();                        // the previous rows' readers are done
        const long n = base + lane;
        if (fok && n < n1) {
            const float xv = a.x[n * a.ldx + f];
            const float u = ln_apply(a, n, f, xv);
            const float sl = a.bw ? siluf(xv) : 0.0f;         // (no base branch: its zero weight must not meet silu(Inf))
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int g = 4 * q + j;
                    const float rv = rbf_val(u, s_c[g], a.inv_den);
                    v[j] = g < a.ng ? rv : (g == a.ng ? sl : 0.0f);
                }
                mine[q] = make_float4(v[0], v[1], v[2], v[3]);
            }
        } else {
#pragma unroll
            for (int q = 0; q < NQ; ++q) mine[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __syncthreads();
        if (ok) {
            const int cnt = (int)min(64L, n1 - base);
            const float4* d = s_d + wave * 64 * NQ;
            for (int r = 0; r < cnt; ++r, d += NQ) {
                float dv[CP];
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const float4 t = d[q];
                    dv[4 * q] = t.x; dv[4 * q + 1] = t.y; dv[4 * q + 2] = t.z; dv[4 * q + 3] = t.w;
                }
                float phi = 0.0f;
#pragma unroll
                for (int c = 0; c < CP; ++c) phi = __builtin_fmaf(w[c], dv[c], phi);
                const float s = edge_sign(phi);
#pragma unroll
                for (int c = 0; c < CP; ++c) acc[c] = __builtin_fmaf(s, dv[c], acc[c]);
            }
        }
    }
    if (ok) {
        float* p = a.partial + (((long)blockIdx.x * a.in + f) * (a.ng + 1)) * a.out + o;
#pragma unroll
        for (int c = 0; c < CP; ++c)
            if (c <= a.ng) p[(long)c * a.out] = acc[c];
    }
}

}  // namespace fastkan_edge

using fastkan_edge::Args;

static size_t fke_al256(size_t b) { return (b + 255) & ~(size_t)255; }

// the centre bound of the row kernels: 4, 8, 16, 32 or kMaxKnots
static int fke_gc(int ng) { return ng <= 4 ? 4 : ng <= 8 ? 8 : ng <= 16 ? 16 : ng <= 32 ? 32 : kMaxKnots; }

template <int MODE>
static int fke_launch_rows(const Args& a, dim3 grid, hipStream_t st) {
    const int GC = fke_gc(a.ng);
    const size_t lds = ((size_t)kEdgeFT * kEdgeOB * (GC + 4) + GC) * sizeof(float);
    switch (GC) {
        case 4: fastkan_edge::rows_kernel<4, MODE><<<grid, kEdgeThreads, lds, st>>>(a); break;
        case 8: fastkan_edge::rows_kernel<8, MODE><<<grid, kEdgeThreads, lds, st>>>(a); break;
        case 16: fastkan_edge::rows_kernel<16, MODE><<<grid, kEdgeThreads, lds, st>>>(a); break;
        case 32: fastkan_edge::rows_kernel<32, MODE><<<grid, kEdgeThreads, lds, st>>>(a); break;
        default: fastkan_edge::rows_kernel<kMaxKnots, MODE><<<grid, kEdgeThreads, lds, st>>>(a); break;
    }
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

template <int NQ>
static int fke_launch_param(const Args& a, dim3 grid, hipStream_t st) {
    const size_t lds = ((size_t)kEdgeFT * 64 * NQ * 4 + NQ * 4) * sizeof(float);
    fastkan_edge::param_kernel<NQ><<<grid, kEdgeThreads, lds, st>>>(a);
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

static Args fke_args(const float* x, long ldx, long N, int in, int out, int ng, const float* centers, float den, const float* sw,
                     const float* bw) {
    Args a{};
    a.x = x; a.ldx = ldx; a.xcs = 1; a.N = N; a.centers = centers; a.ng = ng; a.inv_den = 1.0f / den; a.in = in; a.out = out;
    a.sw = sw; a.bw = bw;
    return a;
}

// ---- workspaces: [slab partials | row statistics [N, 2] | d / du [N, in] | LayerNorm partial rows], the last three with LayerNorm only
size_t fastkan_edge_abs_sum_ws_bytes(long N, int in, int out, bool layernorm) {
    long S, r;
    edge_plan(N, edge_tiles(in, out), 2048, &S, &r);
    return fke_al256((size_t)S * out * in * sizeof(float)) + (layernorm ? fke_al256((size_t)N * 2 * sizeof(float)) : 0);
}

static size_t fke_bwd_partial_bytes(long N, int in, int out, int ng) {
    long S, r;
    edge_plan(N, edge_tiles(in, out), 2048, &S, &r);
    return fke_al256((size_t)S * in * (ng + 1) * out * sizeof(float));
}

size_t fastkan_edge_abs_sum_bwd_ws_bytes(long N, int in, int out, int ng, bool layernorm) {
    size_t b = fke_bwd_partial_bytes(N, in, out, ng);
    if (layernorm) b += fke_al256((size_t)N * 2 * sizeof(float)) + fke_al256((size_t)N * in * sizeof(float)) + fastkan_ln_bwd_ws_bytes(N, in);
    return b;
}

int fastkan_edge_abs_sum(const float* x, long ldx, long N, int in, int out, int ng, const float* centers, float den, const float* lnw,
                         const float* lnb, float eps, const float* sw, const float* bw, float* S_, long ldS, void* ws, size_t ws_bytes,
                         hipStream_t st) {
    static const char fn[] = "fastkan_edge_abs_sum";
    if (ws_bytes < fastkan_edge_abs_sum_ws_bytes(N, in, out, lnw != nullptr)) return fail(KAGNN_ERR_ARG, "%s: workspace too small", fn);
    long S, r;
    edge_plan(N, edge_tiles(in, out), 2048, &S, &r);
    if (!edge_grid_ok(S, cdiv(in, kEdgeFT), cdiv(out, kEdgeOB))) return fail(KAGNN_ERR_UNSUPPORTED, "%s: shape too large for one launch", fn);
    Args a = fke_args(x, ldx, N, in, out, ng, centers, den, sw, bw);
    a.rows_per_slab = r; a.partial = (float*)ws;
    if (lnw) {
        float* stats = (float*)((char*)ws + fke_al256((size_t)S * out * in * sizeof(float)));
        int rc = launch_stats(x, ldx, N, in, eps, stats, st);
        if (rc) return rc;
        a.stats = stats; a.lnw = lnw; a.lnb = lnb;
    }
    int rc = fke_launch_rows<fastkan_edge::EDGE_SUM>(a, dim3((unsigned)S, cdiv(in, kEdgeFT), cdiv(out, kEdgeOB)), st);
    if (rc) return rc;
    return edge_sum_reduce((const float*)ws, S, in, out, S_, ldS, st);
}

int fastkan_edge_abs_sum_bwd(const float* x, long ldx, long N, int in, int out, int ng, const float* centers, float den, const float*
                             lnw, const float* lnb, float eps, const float* sw, const float* bw, const float* gS, long ldgS, float*
                             g_sw, float* g_bw, float* gx, long ldgx, float* g_lnw, float* g_lnb, void* ws, size_t ws_bytes,
                             hipStream_t st) {
    static const char fn[] = "fastkan_edge_abs_sum_bwd";
    if (ws_bytes < fastkan_edge_abs_sum_bwd_ws_bytes(N, in, out, ng, lnw != nullptr)) return fail(KAGNN_ERR_ARG, "%s: workspace too small", fn);
    char* q = (char*)ws;
    float* partial = (float*)q; q += fke_bwd_partial_bytes(N, in, out, ng);
    Args a = fke_args(x, ldx, N, in, out, ng, centers, den, sw, bw);
    a.gS = gS; a.ldgS = ldgS;
    float *gu = nullptr, *lnpart = nullptr;
    if (lnw) {
        float* stats = (float*)q; q += fke_al256((size_t)N * 2 * sizeof(float));
        gu = (float*)q; q += fke_al256((size_t)N * in * sizeof(float));
        lnpart = (float*)q;
        int rc = launch_stats(x, ldx, N, in, eps, stats, st);
        if (rc) return rc;
        a.stats = stats; a.lnw = lnw; a.lnb = lnb;
    }
    if (g_sw || g_bw) {
        long S, r;
        edge_plan(N, edge_tiles(in, out), 2048, &S, &r);
        a.rows_per_slab = r; a.partial = partial;
        if (!edge_grid_ok(S, cdiv(in, kEdgeFT), cdiv(out, kEdgeOB))) return fail(KAGNN_ERR_UNSUPPORTED, "%s: shape too large for one launch", fn);
        const dim3 grid((unsigned)S, cdiv(in, kEdgeFT), cdiv(out, kEdgeOB));
        // G + 1 dense columns per lane, NQ * 4 of them: the widest instantiation takes the 49 columns of kMaxKnots centres
        const int cols = ng + 1;
        if (fastkan_edge::kMaxNQ * 4 < cols) return fail(KAGNN_ERR_UNSUPPORTED, "%s: more than 48 centres + base column", fn);
        int rc = cols <= 12 ? fke_launch_param<3>(a, grid, st) : cols <= 20 ? fke_launch_param<5>(a, grid, st)
               : cols <= 36 ? fke_launch_param<9>(a, grid, st) : fke_launch_param<fastkan_edge::kMaxNQ>(a, grid, st);
        if (rc) return rc;
        rc = edge_param_reduce(partial, S, in, out, ng, gS, ldgS, sw, nullptr, g_bw, g_sw, nullptr, st);
        if (rc) return rc;
    }
    if (gx) {
        long S, r;
        edge_plan(N, cdiv(in, kEdgeFT), 4096, &S, &r);
        a.rows_per_slab = r; a.partial = nullptr; a.gx = gx; a.ldgx = ldgx; a.gu = gu;
        if (!edge_grid_ok(S, cdiv(in, kEdgeFT), 1)) return fail(KAGNN_ERR_UNSUPPORTED, "%s: shape too large for one launch", fn);
        int rc = fke_launch_rows<fastkan_edge::EDGE_GX>(a, dim3((unsigned)S, cdiv(in, kEdgeFT), 1), st);
        if (rc) return rc;
        if (lnw) {                                   // gx holds the base part; the spline part goes back through the normalisation
            rc = fastkan_ln_bwd(x, ldx, gu, N, in, lnw, lnb, eps, a.stats, gx, ldgx, g_lnw, g_lnb, lnpart, st);
            if (rc) return rc;
        }
    }
    return KAGNN_OK;
}

int fastkan_edge_curves(const float* t, long ldt, const float* tb, long ldtb, long P, int in, int out, int ng, const float* centers,
                        float den, const float* sw, const float* bw, float* phi, hipStream_t st) {
    long S, r;
    edge_plan(P, edge_tiles(in, out), 2048, &S, &r);
    Args a = fke_args(t, ldt == 0 ? 1 : ldt, P, in, out, ng, centers, den, t ? sw : nullptr, bw);
    a.xcs = ldt == 0 ? 0 : 1;
    a.xb = tb; a.ldxb = ldtb == 0 ? 1 : ldtb; a.xbcs = ldtb == 0 ? 0 : 1;
    a.rows_per_slab = r; a.phi = phi;
    if (!edge_grid_ok(S, cdiv(in, kEdgeFT), cdiv(out, kEdgeOB))) return fail(KAGNN_ERR_UNSUPPORTED, "%s: shape too large for one launch", "fastkan_edge_curves");
    return fke_launch_rows<fastkan_edge::EDGE_CURVES>(a, dim3((unsigned)S, cdiv(in, kEdgeFT), cdiv(out, kEdgeOB)), st);
}

}  // namespace kagnn
