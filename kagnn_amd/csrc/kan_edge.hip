// Per-edge activations of a KANLinear: the edge functions
//   phi_{o,i}(t) = base_weight[o,i] silu(t) + spline_scaler[o,i] sum_c spline_weight[o,i,c] B_c(t)
// that the layer's forward only ever sums over i.  Three results, none of which stores phi over the rows:
//   abs sum   S[o,i] = sum_n |phi_{o,i}(x[n,i])|                       (the magnitude the KAN regulariser is defined on)
//   its backward: the three parameter gradients and gx under an upstream gS[out,in], with sign(0) = 0
//   curves    phi[p,o,i] at sample points t[p] or t[p,i]               (the reference's plot_curve, fastkan.py)
//   moments   mean[o,i] and the centred sum of squares m2[o,i] of phi_{o,i}(x[n,i]) over the rows   (attribution's edge scale)
// Exact fp32 in every precision mode (the `mode` of the layer entry points does not reach this file), spline orders 1..4,
// the shared uniform knot row or per-feature knot rows, any in / out / grid the layer kernels take.
//
// Row kernels (abs sum, gx, curves): a workgroup of four waves owns four consecutive features, one per wave; lane = row.
// The weights of the tile's 64 outputs lie in LDS as rows [bw | gS | K zeros | C scaled coefficients | K zeros]: a lane in
// knot span m reads the K+1 consecutive words at m of output o's row -- lanes in one span read one address (a broadcast), lanes
// in different spans read different consecutive banks -- and the zero padding stands for the bases left and right of the
// coefficient range.  K+2 FMAs per (row, feature, output).  The abs sum keeps one accumulator per output in registers and
// reduces across lanes once per row slab; the slab partials [slab][out][in] are added in index order by a second kernel.
// The moments keep two accumulators per output, sum d and sum d^2 of d = phi - p, where the pivot p[o,i] = phi_{o,i}(x[0,i]) is
// the same in every slab (each workgroup evaluates it into its rows' slot 1, the gx kernel's gS): sum phi^2 - (sum phi)^2 / N in fp32 would
// lose an edge that sits on an offset.  The second kernel adds the slabs in fp64 and forms mean = p + Sd/N, m2 = Sd2 - Sd^2/N.
//
// Parameter gradients: sum_n sign(phi) B_c(x) is a product over the rows, so the roles turn round: lane = output with its
// C+1 weights and C+1 accumulators in registers (statically indexed), and the rows' dense basis rows [B_0..B_{C-1} | silu]
// are staged 64 at a time through LDS (lane = row evaluates them, every lane then reads them back as broadcasts).  Slab
// partials [slab][in][C+1][out] are added in index order by a second kernel that also applies gS, the scaler and forms the
// scaler's gradient  g_sc = gS sum_c w_c T_c.
//
// No atomics anywhere: the same inputs give the same bits.
#include "edge_common.h"
#include "host.h"

namespace kagnn {

// (workgroup shape, edge_sign, edge_plan and the declarations of the two slab reductions: edge_common.h, shared with fastkan_edge.hip)
constexpr int kEdgeMaxNQ = 12;         // widest parameter-gradient kernel: NQ * 4 = 48 dense columns
// check_kan_dims: G + 2K + 1 <= kMaxKnots, so C = G + K <= kMaxKnots - 1 - K, largest at K = 1
static_assert(kEdgeMaxNQ * 4 >= (kMaxKnots - 2) + 1, "the widest parameter kernel must hold C + 1 columns at the knot limit");

enum { EDGE_SUM = 0, EDGE_GX = 1, EDGE_CURVES = 2 };
// outputs per pass over a slab's rows in the moments kernel, 2 * kEdgeMomOT accumulators per lane: two passes over a 64-output tile.
// One pass of 64 fits without scratch but leaves one wave per SIMD; two passes evaluate the bases twice and keep the abs sum's
// occupancy, which is the faster trade (both measured: profiles/pruning.md)
constexpr int kEdgeMomOT = 32;

struct EdgeArgs {
    const float* x; long ldx; int xcs;      // element (n, f) at x[n*ldx + f*xcs]   (xcs 0: the curves' shared sample points)
    long N;
    const float* knots; int nknots;
    int in, out, C;
    const float* bw; const float* sw; const float* sc;
    long rows_per_slab;
    float* partial;                         // abs sum [slab][out][in]; parameter gradients [slab][in][C+1][out];
                                            // moments [slab][2][out][in], then the pivots [out][in]
    const float* gS; long ldgS;
    float* gx; long ldgx;
    float* phi;                             // curves [N][out][in]
};

// span m and the K+1 local bases (and derivatives) of x; bases whose index m-K+r lies outside [0, C) do not exist
template <int K, bool PF, bool DERIV>
__device__ __forceinline__ int edge_basis(float x, const float* kn /* LDS: this feature's knot row */, const SplineGeom& g, int C,
                                          float (&N)[K + 1], float (&dN)[K + 1]) {
    int m;
    if constexpr (PF) m = bspline_generic<K, DERIV>(x, kn, g.nknots, N, dN);
    else m = bspline_local<K, DERIV>(x, kn, g, N, dN);
#pragma unroll
    for (int r = 0; r <= K; ++r) {
        const int j = m - K + r;
        const bool ok = j >= 0 && j < C;
        N[r] = ok ? N[r] : 0.0f;
        if (DERIV) dN[r] = ok ? dN[r] : 0.0f;
    }
    return m;
}

// the knot rows a workgroup needs, into LDS: the four features' own rows [4][nknots] (PF), else the one shared row
template <bool PF>
__device__ __forceinline__ void edge_stage_knots(const EdgeArgs& a, int f0, float* s_kn) {
    for (int idx = threadIdx.x; idx < (PF ? kEdgeFT : 1) * a.nknots; idx += kEdgeThreads) {
        const int w = idx / a.nknots, j = idx - w * a.nknots;
        s_kn[idx] = PF ? a.knots[(long)min(f0 + w, a.in - 1) * a.nknots + j] : a.knots[j];
    }
}

// the weight rows [4][64][RS] of the output tile [o0, o0 + oc) for the four features from f0, into LDS:
// [bw | slot 1 | K zeros | C scaled coefficients | K zeros], slot 1 = gS[o, f] (NULL: 0); rows beyond the tile or the layer are zero
template <int K>
__device__ __forceinline__ void edge_stage_weights(const EdgeArgs& a, int f0, int o0, int oc, const float* gS, float* s_w) {
    const int RS = a.C + 2 * K + 2;
    for (int idx = threadIdx.x; idx < kEdgeFT * kEdgeOB * RS; idx += kEdgeThreads) {
        const int j = idx % RS, t = idx / RS, o = t % kEdgeOB, w = t / kEdgeOB;
        const int ff = f0 + w;
        float v = 0.0f;
        if (ff < a.in && o < oc) {
            const long e = (long)(o0 + o) * a.in + ff;
            if (j == 0) v = a.bw ? a.bw[e] : 0.0f;
            else if (j == 1) v = gS ? gS[(long)(o0 + o) * a.ldgS + ff] : 0.0f;
            else {
                const int c = j - 2 - K;
                if (c >= 0 && c < a.C) {
                    v = a.sw[e * a.C + c];
                    if (a.sc) v *= a.sc[e];
                }
            }
        }
        s_w[idx] = v;
    }
}

template <int K, bool PF, int MODE>
__global__ __launch_bounds__(kEdgeThreads) void kan_edge_rows_kernel(EdgeArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int RS = a.C + 2 * K + 2;
    float* s_w = smem;                                          // [4][64][RS]
    float* s_kn = smem + kEdgeFT * kEdgeOB * RS;                // PF: [4][nknots], else [nknots]
    const int f0 = blockIdx.y * kEdgeFT, f = f0 + wave;
    const bool fok = f < a.in;
    edge_stage_knots<PF>(a, f0, s_kn);
    const long n0 = (long)blockIdx.x * a.rows_per_slab, n1 = min(a.N, n0 + a.rows_per_slab);
    const int nob = cdiv(a.out, kEdgeOB);
    const int ob_begin = MODE == EDGE_GX ? 0 : (int)blockIdx.z, ob_end = MODE == EDGE_GX ? nob : ob_begin + 1;
    const float* kn = s_kn + (PF ? wave * a.nknots : 0);
    const float* wrow = s_w + wave * kEdgeOB * RS;

    for (int ob = ob_begin; ob < ob_end; ++ob) {
        const int o0 = ob * kEdgeOB, oc = min(kEdgeOB, a.out - o0);
        __syncthreads();                                        // the previous tile's readers are done
        edge_stage_weights<K>(a, f0, o0, oc, MODE == EDGE_GX ? a.gS : nullptr, s_w);
        __syncthreads();
        if (!fok) continue;
        SplineGeom g;
        if constexpr (PF) { g.nknots = a.nknots; g.g0 = 0.0f; g.inv_h = 0.0f; }
        else g = geom_from_knots(kn, a.nknots);

        float acc[kEdgeOB];
        if constexpr (MODE == EDGE_SUM) {
#pragma unroll
            for (int o = 0; o < kEdgeOB; ++o) acc[o] = 0.0f;
        }
        for (long n = n0 + lane; n < n1; n += 64) {
            const float x = a.x[n * a.ldx + (long)f * a.xcs];
            float N[K + 1], dN[K + 1];
            const int m = edge_basis<K, PF, MODE == EDGE_GX>(x, kn, g, a.C, N, dN);
            const float sl = siluf(x);
            const float sg = MODE == EDGE_GX ? silu_gradf(x) : 0.0f;
            const float* wp = wrow + 2 + m;
            float gsum = 0.0f;
            if constexpr (MODE == EDGE_CURVES) {                // a store per output, nothing accumulated: a plain loop
                float* dst = a.phi + (n * a.out + o0) * a.in + f;
#pragma unroll 2
                for (int o = 0; o < oc; ++o) {
                    const float* q = wp + o * RS;
                    float phi = wrow[o * RS] * sl;
#pragma unroll
                    for (int r = 0; r <= K; ++r) phi = __builtin_fmaf(q[r], N[r], phi);
                    dst[(long)o * a.in] = phi;
                }
            } else {
#pragma unroll
            for (int og = 0; og < kEdgeOB; og += 16) {
                if (og < oc) {                                  // (workgroup-uniform)
#pragma unroll
                    for (int oo = 0; oo < 16; ++oo) {
                        const int o = og + oo;
                        const float* q = wp + o * RS;
                        const float b = wrow[o * RS];
                        float phi = b * sl;
#pragma unroll
                        for (int r = 0; r <= K; ++r) phi = __builtin_fmaf(q[r], N[r], phi);
                        if constexpr (MODE == EDGE_SUM) acc[o] += fabsf(phi);
                        if constexpr (MODE == EDGE_GX) {
                            float d = b * sg;
#pragma unroll
                            for (int r = 0; r <= K; ++r) d = __builtin_fmaf(q[r], dN[r], d);
                            gsum = __builtin_fmaf(wrow[o * RS + 1] * edge_sign(phi), d, gsum);
                        }
                    }
                }
            }
            }
            if constexpr (MODE == EDGE_GX) {
                float* p = a.gx + n * a.ldgx + f;
                *p = ob == 0 ? gsum : *p + gsum;                // (the same thread wrote it for the previous tile)
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

// S[o*ldS + f] = sum_s partial[s][o][f], slabs in index order
__global__ void kan_edge_sum_reduce_kernel(const float* __restrict__ partial, long S, int in, int out, float* __restrict__ dst,
                                           long ld) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const long per = (long)out * in;
    if (i >= per) return;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    long s = 0;
    for (; s + 4 <= S; s += 4) {
        a0 += partial[(s + 0) * per + i];
        a1 += partial[(s + 1) * per + i];
        a2 += partial[(s + 2) * per + i];
        a3 += partial[(s + 3) * per + i];
    }
    for (; s < S; ++s) a0 += partial[s * per + i];
    dst[(i / in) * ld + (i % in)] = (a0 + a1) + (a2 + a3);
}

// The moments' row kernel: the abs sum's grid, LDS weight rows (slot 1 holds the pivot instead of gS) and lane = row, wave = feature;
// one slab of  sum d, sum d^2,  d = phi - p.  A non-finite x poisons its column: both partials of the slab are NaN.
template <int K, bool PF>
__global__ __launch_bounds__(kEdgeThreads) void kan_phi_moments_kernel(EdgeArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int RS = a.C + 2 * K + 2;
    float* s_w = smem;                                          // [4][64][RS]
    float* s_kn = smem + kEdgeFT * kEdgeOB * RS;                // PF: [4][nknots], else [nknots]
    const int f0 = blockIdx.y * kEdgeFT, f = f0 + wave;
    const bool fok = f < a.in;
    edge_stage_knots<PF>(a, f0, s_kn);
    const long n0 = (long)blockIdx.x * a.rows_per_slab, n1 = min(a.N, n0 + a.rows_per_slab);
    const int o0 = blockIdx.z * kEdgeOB, oc = min(kEdgeOB, a.out - o0);
    edge_stage_weights<K>(a, f0, o0, oc, nullptr, s_w);         // (slot 1: 0 for now, then the pivot)
    __syncthreads();
    const float* kn = s_kn + (PF ? wave * a.nknots : 0);
    float* wrow = s_w + wave * kEdgeOB * RS;
    SplineGeom g;
    if constexpr (PF) { g.nknots = a.nknots; g.g0 = 0.0f; g.inv_h = 0.0f; }
    else g = geom_from_knots(kn, a.nknots);
    {                                                           // lane = output: the pivot phi_{o,f}(x[0,f]), in the loop's arithmetic
        const float x = a.x[min(f, a.in - 1)];
        float N[K + 1], dN[K + 1];
        const int m = edge_basis<K, PF, false>(x, kn, g, a.C, N, dN);
        const float* q = wrow + lane * RS + 2 + m;
        float phi = wrow[lane * RS] * siluf(x);
#pragma unroll
        for (int r = 0; r <= K; ++r) phi = __builtin_fmaf(q[r], N[r], phi);
        wrow[lane * RS + 1] = phi;
    }
    __syncthreads();
    if (!fok) return;
    const long per = (long)a.out * a.in;
    float* dst = a.partial + (long)blockIdx.x * 2 * per + (long)(o0 + lane) * a.in + f;
    for (int h = 0; h < oc; h += kEdgeMomOT) {
        float sd[kEdgeMomOT], sq[kEdgeMomOT];
#pragma unroll
        for (int o = 0; o < kEdgeMomOT; ++o) { sd[o] = 0.0f; sq[o] = 0.0f; }
        bool bad = false;
        for (long n = n0 + lane; n < n1; n += 64) {
            const float x = a.x[n * a.ldx + f];
            bad |= !(fabsf(x) <= 3.402823466e38f);
            float N[K + 1], dN[K + 1];
            const int m = edge_basis<K, PF, false>(x, kn, g, a.C, N, dN);
            const float sl = siluf(x);
            const float* wp = wrow + h * RS + 2 + m;
#pragma unroll
            for (int og = 0; og < kEdgeMomOT; og += 16) {
                if (h + og < oc) {                              // (workgroup-uniform)
#pragma unroll
                    for (int oo = 0; oo < 16; ++oo) {
                        const int o = og + oo;
                        const float* q = wp + o * RS;
                        float phi = wrow[(h + o) * RS] * sl;
#pragma unroll
                        for (int r = 0; r <= K; ++r) phi = __builtin_fmaf(q[r], N[r], phi);
                        const float d = phi - wrow[(h + o) * RS + 1];     // (the pivot row itself: exactly 0)
                        sd[o] += d;
                        sq[o] = __builtin_fmaf(d, d, sq[o]);
                    }
                }
            }
        }
        bad = __any(bad);
        float m1 = 0.0f, m2 = 0.0f;
#pragma unroll
        for (int o = 0; o < kEdgeMomOT; ++o) {
            float v = sd[o], w = sq[o];
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) { v += __shfl_xor(v, d, 64); w += __shfl_xor(w, d, 64); }
            m1 = lane - h == o ? v : m1;
            m2 = lane - h == o ? w : m2;
        }
        if (lane >= h && lane < min(oc, h + kEdgeMomOT)) {
            dst[0] = bad ? __builtin_nanf("") : m1;
            dst[per] = bad ? __builtin_nanf("") : m2;
        }
    }
    if (blockIdx.x == 0 && lane < oc) a.partial[(long)gridDim.x * 2 * per + (long)(o0 + lane) * a.in + f] = wrow[lane * RS + 1];
}

// partial[s][2][o][f] = slab s's (sum d, sum d^2) about the pivot p[o][f] that follows the last slab; slabs in index order, fp64:
//   mean = p + Sd / N,   m2 = Sd2 - Sd^2 / N   (never below 0; NaN stays NaN)
__global__ void kan_phi_moments_reduce_kernel(const float* __restrict__ partial, long S, long N, int in, int out,
                                               float* __restrict__ mean, long ld_mean, float* __restrict__ m2, long ld_m2) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const long per = (long)out * in;
    if (i >= per) return;
    double sd = 0.0, sq = 0.0;
    for (long s = 0; s < S; ++s) {
        sd += (double)partial[(2 * s) * per + i];
        sq += (double)partial[(2 * s + 1) * per + i];
    }
    const double p = (double)partial[2 * S * per + i];
    const double v = sq - sd * sd / (double)N;
    if (mean) mean[(i / in) * ld_mean + (i % in)] = (float)(p + sd / (double)N);
    if (m2) m2[(i / in) * ld_m2 + (i % in)] = (float)(v < 0.0 ? 0.0 : v);
}

// T[o,f,c] = sum_n sign(phi_{o,f}(x[n,f])) D[n,f,c],  D = [B_0 .. B_{C-1} | silu]: one slab of it.  NQ * 4 >= C + 1.
template <int K, bool PF, int NQ>
__global__ __launch_bounds__(kEdgeThreads) void kan_edge_param_kernel(EdgeArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int CP = NQ * 4;
    if (a.C + 1 > CP) return;                                   // (the launcher picks NQ; never write past a lane's columns)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float4* s_d = reinterpret_cast<float4*>(smem);              // [4][64][NQ]
    float* s_kn = smem + kEdgeFT * 64 * CP;
    const int f0 = blockIdx.y * kEdgeFT, f = f0 + wave;
    const bool fok = f < a.in;
    edge_stage_knots<PF>(a, f0, s_kn);
    const float* kn = s_kn + (PF ? wave * a.nknots : 0);
    const int o = blockIdx.z * kEdgeOB + lane;
    const bool ok = fok && o < a.out;
    float w[CP], acc[CP];
#pragma unroll
    for (int c = 0; c < CP; ++c) { w[c] = 0.0f; acc[c] = 0.0f; }
    if (ok) {
        const long e = (long)o * a.in + f;
        const float scale = a.sc ? a.sc[e] : 1.0f;
#pragma unroll
        for (int c = 0; c < CP; ++c) {
            if (c < a.C) w[c] = a.sw[e * a.C + c] * scale;
            else if (c == a.C) w[c] = a.bw ? a.bw[e] : 0.0f;
        }
    }
    __syncthreads();                                            // the knots
    SplineGeom g;
    if constexpr (PF) { g.nknots = a.nknots; g.g0 = 0.0f; g.inv_h = 0.0f; }
    else g = geom_from_knots(kn, a.nknots);
    const long n0 = (long)blockIdx.x * a.rows_per_slab, n1 = min(a.N, n0 + a.rows_per_slab);
    float4* mine = s_d + (wave * 64 + lane) * NQ;
    for (long base = n0; base < n1; base += 64) {               // (workgroup-uniform trip count)
        if (base != n0) __syncthreads();                        // the previous rows' readers are done
        const long n = base + lane;
#pragma unroll
        for (int q = 0; q < NQ; ++q) mine[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (fok && n < n1) {
            const float x = a.x[n * a.ldx + f];
            float N[K + 1], dN[K + 1];
            const int m = edge_basis<K, PF, false>(x, kn, g, a.C, N, dN);
            float* dr = reinterpret_cast<float*>(mine);
#pragma unroll
            for (int r = 0; r <= K; ++r) {
                const int j = m - K + r;
                if (j >= 0 && j < a.C) dr[j] = N[r];
            }
            dr[a.C] = siluf(x);
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
        float* p = a.partial + (((long)blockIdx.x * a.in + f) * (a.C + 1)) * a.out + o;
#pragma unroll
        for (int c = 0; c < CP; ++c)
            if (c <= a.C) p[(long)c * a.out] = acc[c];
    }
}

// thread = (f, o), o fastest: adds the slabs in index order, then
//   g_bw = gS T_C,   g_sw[c] = gS scaler T_c,   g_sc = gS sum_c sw_c T_c
__global__ void kan_edge_param_reduce_kernel(const float* __restrict__ partial, long S, int in, int out, int C,
                                             const float* __restrict__ gS, long ldgS, const float* __restrict__ sw,
                                             const float* __restrict__ sc, float* __restrict__ g_bw, float* __restrict__ g_sw,
                                             float* __restrict__ g_sc) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= (long)in * out) return;
    const int f = (int)(i / out), o = (int)(i % out);
    const long e = (long)o * in + f;
    const float g = gS[(long)o * ldgS + f];
    const float scale = sc ? sc[e] : 1.0f;
    const long per = (long)in * (C + 1) * out;
    const float* p = partial + ((long)f * (C + 1)) * out + o;
    float dot = 0.0f;
    for (int c = 0; c <= C; ++c) {
        float t = 0.0f;
        for (long s = 0; s < S; ++s) t += p[s * per + (long)c * out];
        if (c < C) {
            if (g_sw) g_sw[e * C + c] = g * scale * t;
            dot = __builtin_fmaf(sw[e * C + c], t, dot);
        } else if (g_bw) {
            g_bw[e] = g * t;
        }
    }
    if (g_sc) g_sc[e] = g * dot;
}

int edge_sum_reduce(const float* partial, long slabs, int in, int out, float* dst, long ld, hipStream_t st) {
    kan_edge_sum_reduce_kernel<<<cdiv((long)out * in, 256), 256, 0, st>>>(partial, slabs, in, out, dst, ld);
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

int edge_param_reduce(const float* partial, long slabs, int in, int out, int C, const float* gS, long ldgS, const float* sw,
                      const float* sc, float* g_bw, float* g_sw, float* g_sc, hipStream_t st) {
    kan_edge_param_reduce_kernel<<<cdiv((long)out * in, 256), 256, 0, st>>>(partial, slabs, in, out, C, gS, ldgS, sw, sc, g_bw, g_sw, g_sc);
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

static size_t edge_rows_lds_bytes(int nknots, int C, int K, bool pf) {
    return ((size_t)kEdgeFT * kEdgeOB * (C + 2 * K + 2) + (size_t)(pf ? kEdgeFT : 1) * nknots) * sizeof(float);
}

template <int MODE>
static int edge_launch_rows(const EdgeArgs& a, int K, bool pf, dim3 grid, hipStream_t st) {
    const size_t lds = edge_rows_lds_bytes(a.nknots, a.C, K, pf);
#define KAGNN_EDGE_ROWS(KK)                                                                                  \
    case KK:                                                                                                 \
        if (pf) kan_edge_rows_kernel<KK, true, MODE><<<grid, kEdgeThreads, lds, st>>>(a);                     \
        else kan_edge_rows_kernel<KK, false, MODE><<<grid, kEdgeThreads, lds, st>>>(a);                       \
        break;
    switch (K) {
        KAGNN_EDGE_ROWS(1) KAGNN_EDGE_ROWS(2) KAGNN_EDGE_ROWS(3) KAGNN_EDGE_ROWS(4)
        default: return fail(KAGNN_ERR_UNSUPPORTED, "%s: spline_order must be 1..4", "kan_edge");
    }
#undef KAGNN_EDGE_ROWS
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

template <int NQ>
static int edge_launch_param(const EdgeArgs& a, int K, bool pf, dim3 grid, hipStream_t st) {
    const size_t lds = ((size_t)kEdgeFT * 64 * NQ * 4 + (size_t)(pf ? kEdgeFT : 1) * a.nknots) * sizeof(float);
#define KAGNN_EDGE_PARAM(KK)                                                                                 \
    case KK:                                                                                                 \
        if (pf) kan_edge_param_kernel<KK, true, NQ><<<grid, kEdgeThreads, lds, st>>>(a);                      \
        else kan_edge_param_kernel<KK, false, NQ><<<grid, kEdgeThreads, lds, st>>>(a);                        \
        break;
    switch (K) {
        KAGNN_EDGE_PARAM(1) KAGNN_EDGE_PARAM(2) KAGNN_EDGE_PARAM(3) KAGNN_EDGE_PARAM(4)
        default: return fail(KAGNN_ERR_UNSUPPORTED, "%s: spline_order must be 1..4", "kan_edge");
    }
#undef KAGNN_EDGE_PARAM
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

size_t kan_edge_abs_sum_ws_bytes(long N, int in, int out) {
    long S, r;
    edge_plan(N, edge_tiles(in, out), 2048, &S, &r);
    return (size_t)S * out * in * sizeof(float);
}

size_t kan_edge_moments_ws_bytes(long N, int in, int out) {
    long S, r;
    edge_plan(N, edge_tiles(in, out), 2048, &S, &r);
    return (size_t)(2 * S + 1) * out * in * sizeof(float);
}

size_t kan_edge_abs_sum_bwd_ws_bytes(long N, int in, int out, int C) {
    long S, r;
    edge_plan(N, edge_tiles(in, out), 2048, &S, &r);
    return (size_t)S * in * (C + 1) * out * sizeof(float);
}

int kan_edge_abs_sum(const float* x, long ldx, long N, const float* knots, bool pf, int in, int out, int G, int K, const float* bw,
                     const float* sw, const float* sc, float* S_, long ldS, float* ws, size_t ws_bytes, hipStream_t st) {
    if (ws_bytes < kan_edge_abs_sum_ws_bytes(N, in, out)) return fail(KAGNN_ERR_ARG, "%s: workspace too small", "kan_edge_abs_sum");
    long S, r;
    edge_plan(N, edge_tiles(in, out), 2048, &S, &r);
    EdgeArgs a{};
    a.x = x; a.ldx = ldx; a.xcs = 1; a.N = N; a.knots = knots; a.nknots = G + 2 * K + 1; a.in = in; a.out = out; a.C = G + K;
    a.bw = bw; a.sw = sw; a.sc = sc; a.rows_per_slab = r; a.partial = ws;
    if (!edge_grid_ok(S, cdiv(in, kEdgeFT), cdiv(out, kEdgeOB))) return fail(KAGNN_ERR_UNSUPPORTED, "%s: shape too large for one launch", "kan_edge_abs_sum");
    int rc = edge_launch_rows<EDGE_SUM>(a, K, pf, dim3((unsigned)S, cdiv(in, kEdgeFT), cdiv(out, kEdgeOB)), st);
    if (rc) return rc;
    return edge_sum_reduce(ws, S, in, out, S_, ldS, st);
}

int kan_edge_moments(const float* x, long ldx, long N, const float* knots, bool pf, int in, int out, int G, int K, const float* bw,
                     const float* sw, const float* sc, float* mean, long ld_mean, float* m2, long ld_m2, float* ws, size_t ws_bytes,
                     hipStream_t st) {
    if (ws_bytes < kan_edge_moments_ws_bytes(N, in, out)) return fail(KAGNN_ERR_ARG, "%s: workspace too small", "kan_edge_moments");
    long S, r;
    edge_plan(N, edge_tiles(in, out), 2048, &S, &r);
    EdgeArgs a{};
    a.x = x; a.ldx = ldx; a.xcs = 1; a.N = N; a.knots = knots; a.nknots = G + 2 * K + 1; a.in = in; a.out = out; a.C = G + K;
    a.bw = bw; a.sw = sw; a.sc = sc; a.rows_per_slab = r; a.partial = ws;
    if (!edge_grid_ok(S, cdiv(in, kEdgeFT), cdiv(out, kEdgeOB))) return fail(KAGNN_ERR_UNSUPPORTED, "%s: shape too large for one launch", "kan_edge_moments");
    const dim3 grid((unsigned)S, cdiv(in, kEdgeFT), cdiv(out, kEdgeOB));
    const size_t lds = edge_rows_lds_bytes(a.nknots, a.C, K, pf);
#define KAGNN_PHI_MOMENTS(KK)                                                                                \
    case KK:                                                                                                 \
        if (pf) kan_phi_moments_kernel<KK, true><<<grid, kEdgeThreads, lds, st>>>(a);                         \
        else kan_phi_moments_kernel<KK, false><<<grid, kEdgeThreads, lds, st>>>(a);                           \
        break;
    switch (K) {
        KAGNN_PHI_MOMENTS(1) KAGNN_PHI_MOMENTS(2) KAGNN_PHI_MOMENTS(3) KAGNN_PHI_MOMENTS(4)
        default: return fail(KAGNN_ERR_UNSUPPORTED, "%s: spline_order must be 1..4", "kan_edge");
    }
#undef KAGNN_PHI_MOMENTS
    KAGNN_LAUNCH_CHECK();
    kan_phi_moments_reduce_kernel<<<cdiv((long)out * in, 256), 256, 0, st>>>(ws, S, N, in, out, mean, ld_mean, m2, ld_m2);
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

int kan_edge_abs_sum_bwd(const float* x, long ldx, long N, const float* knots, bool pf, int in, int out, int G, int K,
                         const float* bw, const float* sw, const float* sc, const float* gS, long ldgS, float* g_bw, float* g_sw,
                         float* g_sc, float* gx, long ldgx, float* ws, size_t ws_bytes, hipStream_t st) {
    const int C = G + K;
    EdgeArgs a{};
    a.x = x; a.ldx = ldx; a.xcs = 1; a.N = N; a.knots = knots; a.nknots = G + 2 * K + 1; a.in = in; a.out = out; a.C = C;
    a.bw = bw; a.sw = sw; a.sc = sc; a.gS = gS; a.ldgS = ldgS;
    if (g_bw || g_sw || g_sc) {
        if (ws_bytes < kan_edge_abs_sum_bwd_ws_bytes(N, in, out, C)) return fail(KAGNN_ERR_ARG, "%s: workspace too small", "kan_edge_abs_sum_bwd");
        long S, r;
        edge_plan(N, edge_tiles(in, out), 2048, &S, &r);
        a.rows_per_slab = r; a.partial = ws;
        if (!edge_grid_ok(S, cdiv(in, kEdgeFT), cdiv(out, kEdgeOB))) return fail(KAGNN_ERR_UNSUPPORTED, "%s: shape too large for one launch", "kan_edge_abs_sum_bwd");
        const dim3 grid((unsigned)S, cdiv(in, kEdgeFT), cdiv(out, kEdgeOB));
        // the parameter kernel holds C + 1 dense columns per lane, NQ * 4 of them: the widest instantiation takes every C that
        // check_kan_dims lets through (G + 2K + 1 <= 48 knots: C + 1 <= 47 at K = 1)
        const int NQ = C + 1 <= 12 ? 3 : C + 1 <= 20 ? 5 : C + 1 <= 40 ? 10 : kEdgeMaxNQ;
        if (NQ * 4 < C + 1) return fail(KAGNN_ERR_UNSUPPORTED, "%s: more than 47 coefficients + base column", "kan_edge_abs_sum_bwd");
        int rc = NQ == 3 ? edge_launch_param<3>(a, K, pf, grid, st) : NQ == 5 ? edge_launch_param<5>(a, K, pf, grid, st)
               : NQ == 10 ? edge_launch_param<10>(a, K, pf, grid, st) : edge_launch_param<kEdgeMaxNQ>(a, K, pf, grid, st);
        if (rc) return rc;
        rc = edge_param_reduce(ws, S, in, out, C, gS, ldgS, sw, sc, g_bw, g_sw, g_sc, st);
        if (rc) return rc;
    }
    if (gx) {
        long S, r;
        edge_plan(N, cdiv(in, kEdgeFT), 4096, &S, &r);
        a.rows_per_slab = r; a.gx = gx; a.ldgx = ldgx;
        if (!edge_grid_ok(S, cdiv(in, kEdgeFT), 1)) return fail(KAGNN_ERR_UNSUPPORTED, "%s: shape too large for one launch", "kan_edge_abs_sum_bwd");
        int rc = edge_launch_rows<EDGE_GX>(a, K, pf, dim3((unsigned)S, cdiv(in, kEdgeFT), 1), st);
        if (rc) return rc;
    }
    return KAGNN_OK;
}

int kan_edge_curves(const float* t, long ldt, long P, const float* knots, bool pf, int in, int out, int G, int K, const float* bw,
                    const float* sw, const float* sc, float* phi, hipStream_t st) {
    long S, r;
    edge_plan(P, edge_tiles(in, out), 2048, &S, &r);
    EdgeArgs a{};
    a.x = t; a.ldx = ldt == 0 ? 1 : ldt; a.xcs = ldt == 0 ? 0 : 1; a.N = P; a.knots = knots; a.nknots = G + 2 * K + 1;
    a.in = in; a.out = out; a.C = G + K; a.bw = bw; a.sw = sw; a.sc = sc; a.rows_per_slab = r; a.phi = phi;
    if (!edge_grid_ok(S, cdiv(in, kEdgeFT), cdiv(out, kEdgeOB))) return fail(KAGNN_ERR_UNSUPPORTED, "%s: shape too large for one launch", "kan_edge_curves");
    return edge_launch_rows<EDGE_CURVES>(a, K, pf, dim3((unsigned)S, cdiv(in, kEdgeFT), cdiv(out, kEdgeOB)), st);
}

}  // namespace kagnn
