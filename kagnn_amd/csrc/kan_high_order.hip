// efficient-KAN layer at spline orders 5..16, exact-fp32 (KAGNN_PREC_FP32 / KAGNN_PREC_FP32_GRID): the arithmetic of
// kan_fp32.hip -- v_mfma_f32_32x32x2_f32, one product per coefficient plus the SiLU branch, results an ordered fp32 fma
// chain -- with the order a KERNEL ARGUMENT.  Twelve orders times the variant axes would be ~170 instantiations, so the
// kernels are templated on an order BOUND (KB = 8 or 16) and every loop over the order is unrolled to the bound under
// wave-uniform predicates (`p <= K`): all private arrays keep compile-time indices (nothing goes to scratch).
//
// Reference behaviour replaced: node_classification_clean/ekan.py:79-112 (b_splines, a plain Cox-de Boor loop with no order
// limit), :146-162 (scaled_spline_weight, forward) and their autograd backward; graph_classification/time_model.py:117-133
// sweeps spline_order up to 16.
//
// Two things differ from the low orders:
//  * the coefficient operand.  pick_basis<K> is a chain of K+1 selects per coefficient, C*(K+1) VALU operations per scalar
//    (544 at G = K = 16) against C+1 MFMAs.  Here the K+1 local values go into a zeroed, wave-private LDS row of C+1 floats
//    per lane ([c][lane]: conflict-free), slot C holding silu(x); the coefficient loop reads a = row[c].  After the loop the
//    K+1 slots are zeroed again.  (Forward and weight gradient, where every coefficient feeds an MFMA; the input gradient's
//    epilogue touches 8 or 9 coefficients per pass and keeps the select chain, which measured faster there.)
//  * the input gradient.  Its epilogue evaluates the basis derivative of the 16 scalars a lane owns in a 32x32 tile; unrolled
//    16 times at order 16 that is ~250 KB of code.  The loop over the 16 values stays ROLLED: each trip works on element 0 of
//    the accumulators and then rotates them one place (compile-time indices only), so the evaluation is emitted once.
//
// The fp32 weight packs (kan_pack_f32_kernel, generic in C), the slab reduction and the unpack of kan_fp32.hip are reused.
#include "common.h"
#include "host.h"

namespace kagnn {

constexpr int kHoMaxKnots = 64;      // G + 2K + 1 <= 64 (G = K = 16 needs 49; kMaxKnots sizes the low-order kernels' LDS and stays)
// Accumulators held at once.  Every pass over a coefficient group evaluates the bases again, and at these orders the evaluation
// (~K^2/2 fma pairs per scalar) outweighs the group's MFMAs, so both gradients run ONE wave per SIMD (512 registers) with large
// groups (the accumulators of a wave live in its 256 AGPRs, the evaluation in the other 256 registers).
constexpr int ho_dx_group(int KB) { return KB <= 8 ? 9 : 8; }     // (9 at KB = 16 spilled up to 10 registers on per-feature knots)
constexpr int kHoDwGroup = 11;
constexpr int kHoDwAhead = 4;

// ------------------------------------------------------------------ local bases, order K <= KB at run time
// Same contract as bspline_local / bspline_generic (common.h): returns the span m; N[r] = B_{m-K+r,K}(x) for r = 0..K (0 beyond
// K), dN the derivative.  The recursion runs in place from r = p down to 0, so no copy of the previous order is needed; the
// derivative is formed from the order K-1 values right before the last step.
template <int KB, bool DERIV>
__device__ __forceinline__ int ho_bspline_local(float x, const float* __restrict__ knots /* LDS */, const SplineGeom& g, int K,
                                                float (&N)[KB + 1], float (&dN)[KB + 1]) {
    const int last = g.nknots - 2;
    const float t = (x - g.g0) * g.inv_h;
    const float tc = fminf(fmaxf(t, 0.0f), (float)last);      // NaN -> 0
    int m = (int)tc;
    float tl = knots[m], tr = knots[m + 1];
    if (x >= tr && m < last) {
        ++m; tl = tr; tr = knots[m + 1];
    } else if (x < tl && m > 0) {
        --m; tr = tl; tl = knots[m];
    }
    const bool inside = (x >= tl) && (x < tr);
    const float u = (x - tl) * g.inv_h;
    float n[KB + 1];
    n[0] = 1.0f;
#pragma unroll
    for (int r = 1; r <= KB; ++r) n[r] = 0.0f;
#pragma unroll
    for (int r = 0; r <= KB; ++r) dN[r] = 0.0f;
#pragma unroll
    for (int p = 1; p <= KB; ++p) {
        if (p <= K) {                                           // wave-uniform
            if (DERIV && p == K) {
#pragma unroll
                for (int r = 0; r <= p; ++r) {
                    const float lo = (r >= 1) ? n[r - 1] : 0.0f;
                    const float hi = (r <= p - 1) ? n[r] : 0.0f;
                    dN[r] = (lo - hi) * g.inv_h;
                }
            }
            const float ip = 1.0f / (float)p;
#pragma unroll
            for (int r = p; r >= 0; --r) {
                const float a = (r >= 1) ? (u + (float)(p - r)) * ip * n[r - 1] : 0.0f;
                const float b = (r <= p - 1) ? ((float)(r + 1) - u) * ip * n[r] : 0.0f;
                n[r] = a + b;
            }
        }
    }
    const bool finite = fabsf(x) <= 3.4028234e38f;
    const float nanv = __builtin_nanf("");
#pragma unroll
    for (int r = 0; r <= KB; ++r) {
        N[r] = finite ? (inside ? n[r] : 0.0f) : nanv;
        if (DERIV) dN[r] = finite ? (inside ? dN[r] : 0.0f) : nanv;
    }
    return m;
}

// per-feature, non-uniform knot row t.  w[q] = t[m - KB + q]: placed relative to the BOUND so that t_j for j = m-p+r is
// w[KB-p+r], a compile-time index at every order.  All 2KB+2 entries are loaded whatever the order: stores to w[] under a
// predicate made the compiler keep the 18 floats of KB = 8 as one 32-register tuple and spill it whole at every store.
// Clamped indices feed bases j < 0 or j >= G+K only, which are never selected.
template <int KB, bool DERIV>
__device__ __forceinline__ int ho_bspline_generic(float x, const float* __restrict__ t, int nknots, int K,
                                                  float (&N)[KB + 1], float (&dN)[KB + 1]) {
    int cnt = 0;
    for (int j = 0; j < nknots; ++j) cnt += (x >= t[j]) ? 1 : 0;
    const bool inside = cnt >= 1 && cnt < nknots;
    const int m = min(max(cnt - 1, 0), nknots - 2);
    float w[2 * KB + 2];
#pragma unroll
    for (int q = 0; q < 2 * KB + 2; ++q) w[q] = t[min(max(m - KB + q, 0), nknots - 1)];
    float n[KB + 1];
    n[0] = 1.0f;
#pragma unroll
    for (int r = 1; r <= KB; ++r) n[r] = 0.0f;
#pragma unroll
    for (int r = 0; r <= KB; ++r) dN[r] = 0.0f;
#pragma unroll
    for (int p = 1; p <= KB; ++p) {
        if (p <= K) {
            if (DERIV && p == K) {
#pragma unroll
                for (int r = 0; r <= p; ++r) {
                    const int q0 = KB - p + r;
                    const float lo = (r >= 1) ? n[r - 1] / (w[q0 + p] - w[q0]) : 0.0f;
                    const float hi = (r <= p - 1) ? n[r] / (w[q0 + p + 1] - w[q0 + 1]) : 0.0f;
                    dN[r] = (float)p * (lo - hi);
                }
            }
#pragma unroll
            for (int r = p; r >= 0; --r) {
                const int q0 = KB - p + r;                      // w[q0] = t_j for j = m-p+r
                const float a = (r >= 1) ? (x - w[q0]) / (w[q0 + p] - w[q0]) * n[r - 1] : 0.0f;
                const float b = (r <= p - 1) ? (w[q0 + p + 1] - x) / (w[q0 + p + 1] - w[q0 + 1]) * n[r] : 0.0f;
                n[r] = a + b;
            }
        }
    }
    const bool finite = fabsf(x) <= 3.4028234e38f;
    const float nanv = __builtin_nanf("");
#pragma unroll
    for (int r = 0; r <= KB; ++r) {
        N[r] = finite ? (inside ? n[r] : 0.0f) : nanv;
        if (DERIV) dN[r] = finite ? (inside ? dN[r] : 0.0f) : nanv;
    }
    return m;
}

template <int KB, bool DERIV, bool PF>
__device__ __forceinline__ int ho_eval_basis(float x, const float* s_knots, const SplineGeom& g, const float* __restrict__ knots_g,
                                             int f, int K, float (&N)[KB + 1], float (&dN)[KB + 1]) {
    if constexpr (PF) return ho_bspline_generic<KB, DERIV>(x, knots_g + (long)f * g.nknots, g.nknots, K, N, dN);
    else return ho_bspline_local<KB, DERIV>(x, s_knots, g, K, N, dN);
}

// value of basis index c given the local set: the select chain of pick_basis with the order at run time (N[r] = 0 for r > K).
// The input gradient's epilogue uses it on the 8 or 9 coefficients of a pass, where it measured 1 to 5 % faster than the row.
template <int KB>
__device__ __forceinline__ float ho_pick_basis(const float (&N)[KB + 1], int m, int K, int c) {
    const int d = c - (m - K);
    float a = 0.0f;
#pragma unroll
    for (int r = 0; r <= KB; ++r) a = (d == r) ? N[r] : a;
    return a;
}

// the dense row: row points at this lane's column of the wave's [C+1][64] LDS block
template <int KB>
__device__ __forceinline__ void ho_row_put(float* row, const float (&N)[KB + 1], int m, int K, int C) {
#pragma unroll
    for (int r = 0; r <= KB; ++r) {
        const int c = m - K + r;
        if (r <= K && c >= 0 && c < C) row[c * 64] = N[r];
    }
}
__device__ __forceinline__ void ho_row_clear(float* row, int m, int K, int C, int KB) {
    for (int r = 0; r <= KB; ++r) {
        const int c = m - K + r;
        if (r <= K && c >= 0 && c < C) row[c * 64] = 0.0f;
    }
}

// ------------------------------------------------------------------ forward
// dynamic LDS: knots [kHoMaxKnots] | 4 waves x [C+1][64] dense rows
template <int KB, int OT, bool PF>
__global__ __launch_bounds__(256) void kan_ho_fwd_kernel(
    const float* __restrict__ x, long ldx, long N, int in, int C, int K, const float* __restrict__ knots_g,
    int nknots, const float* __restrict__ pack, int ot0, int OT_total, float* __restrict__ y, long ldy, int out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* s_knots = smem;
    if (threadIdx.x < nknots) s_knots[threadIdx.x] = knots_g[threadIdx.x];
    __syncthreads();
    const SplineGeom geom = geom_from_knots(s_knots, nknots);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long row0 = ((long)blockIdx.x * 4 + wave) * 32;
    if (row0 >= N) return;
    const int r = lane & 31, kh = lane >> 5;
    const long row = row0 + r;
    const bool rv = row < N;
    const int P = (in + 1) / 2, CT = C + 1;
    const float* xr = x + (rv ? row : 0) * ldx;
    float* brow = smem + kHoMaxKnots + (long)wave * CT * 64 + lane;
    for (int c = 0; c < CT; ++c) brow[c * 64] = 0.0f;

    f32x16 acc[OT];
#pragma unroll
    for (int t = 0; t < OT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;

    for (int p = 0; p < P; ++p) {
        const int f = p + kh * P;
        const bool fv = rv && f < in;
        const float xv = xr[min(f, in - 1)];
        float Nv[KB + 1], dummy[KB + 1];
        const int m = ho_eval_basis<KB, false, PF>(xv, s_knots, geom, knots_g, min(f, in - 1), K, Nv, dummy);
        float sl = siluf(xv);
        if (!fv) {
            sl = 0.0f;
#pragma unroll
            for (int i = 0; i <= KB; ++i) Nv[i] = 0.0f;
        }
        ho_row_put<KB>(brow, Nv, m, K, C);
        brow[C * 64] = sl;
        const float* wp = pack + ((long)p * CT * OT_total + ot0) * 64 + lane;
        for (int c = 0; c < CT; ++c) {
            const float a = brow[c * 64];
#pragma unroll
            for (int t = 0; t < OT; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wp[((long)c * OT_total + t) * 64], acc[t], 0, 0, 0);
        }
        ho_row_clear(brow, m, K, C, KB);
    }
#pragma unroll
    for (int t = 0; t < OT; ++t) {
        const int col = 32 * (ot0 + t) + r;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const long rr = row0 + mfma32_row(i, kh);
            if (rr < N && col < out) y[rr * ldy + col] = acc[t][i];
        }
    }
}

// ------------------------------------------------------------------ input gradient
// As kan_dx_f32_kernel: D_c[n][f] = sum_o gy[n][o] Wcat[o][f][c], ho_dx_group(KB) coefficients per pass, the W fragments of a pass
// staged in LDS when they fit (STAGE); gx[n][f] = sum_c D_c dB_c/dx + D_C silu'.  The epilogue over the lane's 16 values is a
// rolled loop that rotates x, the accumulators and the running sums by one element per trip.
// The 8 or 9 derivative coefficients of a pass are SELECTED (ho_pick_basis): here the chain beat the dense row.
// dynamic LDS: knots [kHoMaxKnots] | nw gy tiles [32][2Q+1] | STAGE: [ho_dx_group(KB)][Q][64]
template <int KB, bool PF, bool STAGE>
__global__ __launch_bounds__(256) void kan_ho_dx_kernel(
    const float* __restrict__ x, long ldx, const float* __restrict__ gy, long ldgy, long N, int in, int out, int C, int K,
    const float* __restrict__ knots_g, int nknots, const float* __restrict__ pack, int OT_total,
    float* __restrict__ gx, long ldgx) {
    constexpr int kHoDxGroup = ho_dx_group(KB);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* s_knots = smem;
    const int Q = 16 * OT_total, outP = 2 * Q, ldt = outP + 1;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    float* s_gy = smem + kHoMaxKnots + (long)wave * 32 * ldt;
    float* s_w = smem + kHoMaxKnots + (long)nw * 32 * ldt;
    if (threadIdx.x < nknots) s_knots[threadIdx.x] = knots_g[threadIdx.x];
    const long row0 = ((long)blockIdx.x * nw + wave) * 32;
    for (int i = lane; i < 32 * outP; i += 64) {
        const int rr = i / outP, o = i - rr * outP;
        const long row = row0 + rr;
        const float gv = gy[min(row, N - 1) * ldgy + min(o, out - 1)];
        s_gy[rr * ldt + o] = (row < N && o < out) ? gv : 0.0f;
    }
    __syncthreads();
    if (!STAGE && row0 >= N) return;             // STAGE: every wave keeps walking (barriers below); rows >= N are never stored
    const SplineGeom geom = geom_from_knots(s_knots, nknots);
    const int r = lane & 31, kh = lane >> 5;
    const int CT = C + 1, FT = cdiv(in, 32);
    const float* arow = s_gy + r * ldt + kh * Q;

    for (int ft = 0; ft < FT; ++ft) {
        const int f = 32 * ft + r, fc = min(f, in - 1);
        float xq[16], gacc[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const long rr = min(row0 + mfma32_row(i, kh), N - 1);
            xq[i] = x[rr * ldx + fc];
            gacc[i] = 0.0f;
        }
        for (int c0 = 0; c0 < CT; c0 += kHoDxGroup) {
            f32x16 D[kHoDxGroup];
#pragma unroll
            for (int j = 0; j < kHoDxGroup; ++j)
#pragma unroll
                for (int i = 0; i < 16; ++i) D[j][i] = 0.0f;
            const float* gsrc = pack + ((long)ft * CT + c0) * Q * 64;
            if (STAGE) {
                const int n4 = min(kHoDxGroup, CT - c0) * Q * 16;
                __syncthreads();
                for (int i = threadIdx.x; i < n4; i += blockDim.x)
                    reinterpret_cast<float4*>(s_w)[i] = reinterpret_cast<const float4*>(gsrc)[i];
                __syncthreads();
            }
            const float* wp = (STAGE ? s_w : gsrc) + lane;
            for (int q = 0; q < Q; ++q) {
                const float a = arow[q];
#pragma unroll
                for (int j = 0; j < kHoDxGroup; ++j)
                    if (c0 + j < CT)
                        D[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wp[((long)j * Q + q) * 64], D[j], 0, 0, 0);
            }
#pragma unroll 1
            for (int i = 0; i < 16; ++i) {
                const float xv = xq[0];
                float Nv[KB + 1], dN[KB + 1];
                const int m = ho_eval_basis<KB, true, PF>(xv, s_knots, geom, knots_g, fc, K, Nv, dN);
                const float sg = silu_gradf(xv);
                float s = 0.0f;
#pragma unroll
                for (int j = 0; j < kHoDxGroup; ++j) {
                    const int c = c0 + j;
                    if (c < CT) s = fmaf(D[j][0], (c == C) ? sg : ho_pick_basis<KB>(dN, m, K, c), s);
                }
                const float g0 = gacc[0] + s;
#pragma unroll
                for (int k = 0; k < 15; ++k) {
                    xq[k] = xq[k + 1];
                    gacc[k] = gacc[k + 1];
#pragma unroll
                    for (int j = 0; j < kHoDxGroup; ++j) D[j][k] = D[j][k + 1];
                }
                xq[15] = xv;
                gacc[15] = g0;
            }
        }
        if (f < in) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const long rr = row0 + mfma32_row(i, kh);
                if (rr < N) gx[rr * ldgx + f] = gacc[i];
            }
        }
    }
}

// ------------------------------------------------------------------ weight gradient
// As kan_dw_f32_kernel (grid = (NBx, FT*OT), one partial slab per wave, kan_dw_reduce sums them in a fixed order: no atomics),
// the A operand read from the dense row.  dynamic LDS: knots [kHoMaxKnots] | 4 waves x [C+1][64]
template <int KB, bool PF>
__global__ __launch_bounds__(256) void kan_ho_dw_kernel(
    const float* __restrict__ x, long ldx, const float* __restrict__ gy, long ldgy, long N, int in, int out, int C, int K,
    const float* __restrict__ knots_g, int nknots, int OT, long rows_per_wave, float* __restrict__ slab) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* s_knots = smem;
    if (threadIdx.x < nknots) s_knots[threadIdx.x] = knots_g[threadIdx.x];
    __syncthreads();
    const SplineGeom geom = geom_from_knots(s_knots, nknots);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 31, kh = lane >> 5;
    const int ft = blockIdx.y / OT, ot = blockIdx.y % OT;
    const int FT = gridDim.y / OT;
    const long s = (long)blockIdx.x * 4 + wave;
    const long rbeg = s * rows_per_wave;
    const long rend = min(N, rbeg + rows_per_wave);
    const int CT = C + 1;
    const int f = 32 * ft + r, o = 32 * ot + r;
    const bool fv = f < in;                               // (o >= out: a copy of column out-1 lands in the slab's padding, which the unpack never reads)
    const long inP = 32L * FT, outP = 32L * OT;
    float* brow = smem + kHoMaxKnots + (long)wave * CT * 64 + lane;
    for (int c = 0; c < CT; ++c) brow[c * 64] = 0.0f;

    for (int c0 = 0; c0 < CT; c0 += kHoDwGroup) {
        f32x16 D[kHoDwGroup];
#pragma unroll
        for (int j = 0; j < kHoDwGroup; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) D[j][i] = 0.0f;
        for (long n0 = rbeg; n0 < rend; n0 += 2 * kHoDwAhead) {
            float xs[kHoDwAhead], bs[kHoDwAhead];
#pragma unroll
            for (int u = 0; u < kHoDwAhead; ++u) {
                const long nc = min(n0 + 2 * u + kh, N - 1);
                xs[u] = x[nc * ldx + min(f, in - 1)];
                bs[u] = gy[nc * ldgy + min(o, out - 1)];
            }
#pragma unroll 1
            for (int u = 0; u < kHoDwAhead; ++u) {
                const bool nv = n0 + 2 * u + kh < rend;
                const float xv = xs[0], b = bs[0];
                float Nv[KB + 1], dummy[KB + 1];
                const int m = ho_eval_basis<KB, false, PF>(xv, s_knots, geom, knots_g, min(f, in - 1), K, Nv, dummy);
                float sl = siluf(xv);
                if (!(nv && fv)) {
                    sl = 0.0f;
#pragma unroll
                    for (int i = 0; i <= KB; ++i) Nv[i] = 0.0f;
                }
                ho_row_put<KB>(brow, Nv, m, K, C);
                brow[C * 64] = sl;
#pragma unroll
                for (int j = 0; j < kHoDwGroup; ++j) {
                    const int c = c0 + j;
                    if (c < CT) D[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(brow[c * 64], b, D[j], 0, 0, 0);
                }
                ho_row_clear(brow, m, K, C, KB);
#pragma unroll
                for (int k = 0; k < kHoDwAhead - 1; ++k) { xs[k] = xs[k + 1]; bs[k] = bs[k + 1]; }
            }
        }
#pragma unroll
        for (int j = 0; j < kHoDwGroup; ++j) {
            const int c = c0 + j;
            if (c < CT) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int fl = 32 * ft + mfma32_row(i, kh);
                    slab[((s * CT + c) * inP + fl) * outP + o] = D[j][i];
                }
            }
        }
    }
}

// ------------------------------------------------------------------ dense bases (b_splines, ekan.py:79-112)
// One thread per scalar: the row of C values is zeroed and the K+1 local ones stored over it (global memory takes a run-time
// index).  A non-finite x gives NaN in every basis, as the reference's recursion does (0 * inf / NaN at order 1).
template <int KB>
__global__ void kan_ho_bsplines_kernel(const float* __restrict__ x, long ldx, long N, int in, int C, int K,
                                       const float* __restrict__ grid, int nknots, float* __restrict__ bases) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= N * in) return;
    const long n = i / in; const int f = (int)(i - n * in);
    const float xv = x[n * ldx + f];
    float Nv[KB + 1], dummy[KB + 1];
    const int m = ho_bspline_generic<KB, false>(xv, grid + (long)f * nknots, nknots, K, Nv, dummy);
    float* b = bases + i * C;
    const bool finite = fabsf(xv) <= 3.4028234e38f;
    const float fill = finite ? 0.0f : __builtin_nanf("");
    for (int c = 0; c < C; ++c) b[c] = fill;
    if (!finite) return;
#pragma unroll
    for (int r = 0; r <= KB; ++r) {
        const int c = m - K + r;
        if (r <= K && c >= 0 && c < C) b[c] = Nv[r];
    }
}

// ------------------------------------------------------------------ host launchers
static size_t ho_row_lds(int C) { return (kHoMaxKnots + (size_t)4 * (C + 1) * 64) * sizeof(float); }

template <int KB, bool PF>
static int ho_fwd_dispatch(const float* x, long ldx, long N, int in, int out, int C, int K, const float* knots, int g,
                           const float* pack, float* y, long ldy, hipStream_t st) {
    const int OTt = cdiv(out, 32);
    const size_t lds = ho_row_lds(C);
    dim3 grid(cdiv(N, 128));
    for (int ot0 = 0; ot0 < OTt; ot0 += 4) {
        const int n = min(4, OTt - ot0);
#define L(OTN) kan_ho_fwd_kernel<KB, OTN, PF><<<grid, 256, lds, st>>>(x, ldx, N, in, C, K, knots, g, pack, ot0, OTt, y, ldy, out)
        if (n == 1) L(1); else if (n == 2) L(2); else if (n == 3) L(3); else L(4);
#undef L
        KAGNN_LAUNCH_CHECK();
    }
    return KAGNN_OK;
}

static int ho_check(const char* fn, int G, int K) {
    if (K <= kMaxOrder || K > KAGNN_MAX_SPLINE_ORDER) return fail(KAGNN_ERR_UNSUPPORTED, "%s: spline_order must be 5..16 here", fn);
    if (G < 1 || G + 2 * K + 1 > kHoMaxKnots) return fail(KAGNN_ERR_UNSUPPORTED, "%s: grid_size + 2 * spline_order + 1 must be <= 64", fn);
    return KAGNN_OK;
}

int kan_ho_fwd(const float* x, long ldx, long N, const float* knots, int in, int out, int G, int K, const float* pack,
               float* y, long ldy, bool pf, hipStream_t st) {
    int rc = ho_check("kan_ho_fwd", G, K);
    if (rc) return rc;
    const int g = G + 2 * K + 1, C = G + K;
    if (K <= 8) return pf ? ho_fwd_dispatch<8, true>(x, ldx, N, in, out, C, K, knots, g, pack, y, ldy, st)
                          : ho_fwd_dispatch<8, false>(x, ldx, N, in, out, C, K, knots, g, pack, y, ldy, st);
    return pf ? ho_fwd_dispatch<16, true>(x, ldx, N, in, out, C, K, knots, g, pack, y, ldy, st)
              : ho_fwd_dispatch<16, false>(x, ldx, N, in, out, C, K, knots, g, pack, y, ldy, st);
}

int kan_ho_dx(const float* x, long ldx, const float* gy, long ldgy, long N, const float* knots, int in, int out, int G, int K,
              const float* pack, float* gx, long ldgx, bool pf, hipStream_t st) {
    int rc = ho_check("kan_ho_dx", G, K);
    if (rc) return rc;
    const int g = G + 2 * K + 1, C = G + K, OTt = cdiv(out, 32);
    // waves per workgroup: 4 (one per SIMD) with the W tile staged in LDS when both fit, else as many as the gy tiles leave room for
    const size_t wtile = (size_t)ho_dx_group(K <= 8 ? 8 : 16) * 16 * OTt * 64 * sizeof(float);
    auto gy_bytes = [&](int w) { return (kHoMaxKnots + (size_t)w * 32 * (32 * OTt + 1)) * sizeof(float); };
    int W = 4;
    while (W > 1 && gy_bytes(W) + wtile > 160 * 1024) W >>= 1;
    const bool stage = gy_bytes(W) + wtile <= 160 * 1024 && W >= 2;
    if (!stage) { W = 4; while (W > 1 && gy_bytes(W) > 160 * 1024) W >>= 1; }
    const size_t lds = gy_bytes(W) + (stage ? wtile : 0);
    if (lds > 160 * 1024) return fail(KAGNN_ERR_UNSUPPORTED, "%s: out_features too large for the fp32 dx kernel", "kan_ho_dx");
    dim3 grid(cdiv(N, 32 * W));
#define L3(KB, PF, ST)                                                                           \
    {                                                                                             \
        if (lds > 64 * 1024)                                                                      \
            KAGNN_HIP(hipFuncSetAttribute((const void*)kan_ho_dx_kernel<KB, PF, ST>,              \
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
        kan_ho_dx_kernel<KB, PF, ST><<<grid, 64 * W, lds, st>>>(x, ldx, gy, ldgy, N, in, out, C, K, knots, g, pack, OTt, gx, ldgx); \
    }
#define L2(KB, PF) { if (stage) L3(KB, PF, true) else L3(KB, PF, false) }
#define L1(KB) { if (pf) L2(KB, true) else L2(KB, false) }
    if (K <= 8) L1(8) else L1(16)
#undef L3
#undef L2
#undef L1
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

int kan_ho_dw(const float* x, long ldx, const float* gy, long ldgy, long N, const float* knots, int in, int out, int G, int K,
              const float* sw, const float* sc, float* g_bw, float* g_sw, float* g_sc, float* ws, size_t ws_bytes, bool pf,
              hipStream_t st) {
    int rc = ho_check("kan_ho_dw", G, K);
    if (rc) return rc;
    const int g = G + 2 * K + 1, C = G + K, FT = cdiv(in, 32), OT = cdiv(out, 32);
    if (ws_bytes < kan_f32_dw_ws_bytes(N, in, out, C)) return fail(KAGNN_ERR_ARG, "%s: workspace too small", "kan_ho_dw");
    if (N == 0) {                                         // no rows: zero gradients, no launch
        KAGNN_HIP(hipMemsetAsync(g_sw, 0, (size_t)out * in * C * sizeof(float), st));
        if (g_bw) KAGNN_HIP(hipMemsetAsync(g_bw, 0, (size_t)out * in * sizeof(float), st));
        if (g_sc) KAGNN_HIP(hipMemsetAsync(g_sc, 0, (size_t)out * in * sizeof(float), st));
        return KAGNN_OK;
    }
    int nb; long rpw;
    dw_plan(N, in, out, &nb, &rpw);
    const long NS = (long)nb * 4;
    const long per = (long)(C + 1) * 32 * FT * 32 * OT;
    float* gcat = ws;
    float* slab = ws + per;
    const size_t lds = ho_row_lds(C);
    dim3 grid(nb, FT * OT);
#define L(KB, PF) kan_ho_dw_kernel<KB, PF><<<grid, 256, lds, st>>>(x, ldx, gy, ldgy, N, in, out, C, K, knots, g, OT, rpw, slab)
    if (K <= 8) { if (pf) L(8, true); else L(8, false); }
    else { if (pf) L(16, true); else L(16, false); }
#undef L
    KAGNN_LAUNCH_CHECK();
    rc = kan_dw_reduce(slab, NS, per, gcat, st);
    if (rc) return rc;
    return kan_dw_unpack(gcat, in, out, C, 32L * FT, 32L * OT, sw, sc, g_bw, g_sw, g_sc, st);
}

int kan_ho_bsplines(const float* x, long ldx, long N, const float* grid, int in, int G, int K, float* bases, hipStream_t st) {
    int rc = ho_check("kan_ho_bsplines", G, K);
    if (rc) return rc;
    const int nk = G + 2 * K + 1, C = G + K;
    if (N * in == 0) return KAGNN_OK;
    const int blocks = cdiv(N * in, 256);
    if (K <= 8) kan_ho_bsplines_kernel<8><<<blocks, 256, 0, st>>>(x, ldx, N, in, C, K, grid, nk, bases);
    else kan_ho_bsplines_kernel<16><<<blocks, 256, 0, st>>>(x, ldx, N, in, C, K, grid, nk, bases);
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

}  // namespace kagnn
