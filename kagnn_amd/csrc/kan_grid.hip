// Adaptive grids of the efficient-KAN layer: what KANLinear.update_grid (node_classification_clean/ekan.py:164-211)
// and the dense b_splines (:79-112) need on the device.  KAGNN itself never calls update_grid,
// so this is the widening row, built for correctness and bounded memory rather than tuned.
//
// The reference refits the coefficients after moving the knots by materialising the old layer's per-feature
// outputs [N, in, out] and running a batched least-squares solve over A = bases_new(x) [in, N, C]
// (curve2coeff, ekan.py:114-144).  Here nothing of size N*in*C or N*in*out exists: with A_o = bases_old(x),
//   A^T (A_o W) = (A^T A_o) W ,
// so the normal equations of feature f need only two Gram matrices, which one streaming pass over x accumulates in fp64 on
// v_mfma_f64_16x16x4_f64 (deterministic: per-wave partials, summed in a fixed order); a second small kernel solves
// G1 S = G2 W per feature by a banded fp64 Cholesky.  There is ONE refit, between knot sets of TWO sizes (the same size for
// update_grid; grid extension of the KAN paper moves a coarse grid's curves onto a finer one, or back):
//   G1 = A_new^T A_new [Cn x Cn],  G2 = A_new^T A_old [Cn x Co],  Cn = G_new + k, Co = G_old + k, both <= kMaxKnots - 2 = 46,
// tiled over 16-blocks (at most three each way).  G1 is banded with half-width k <= 4 < 16, so only its diagonal blocks and the
// first sub-diagonal ones are accumulated (2 nb - 1 of them, the lower triangle); G2 has no such structure when the two grids span
// different ranges and is accumulated whole.  `window` [in, 2] restricts feature f's fit to the rows with lo <= x < hi: rows in the
// knot extension, where the finer space cannot represent the old curve, otherwise leak their misfit into the range.
#include "common.h"
#include "host.h"

namespace kagnn {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------ dense bases (b_splines, ekan.py:79-112)
template <int K>
__global__ void kan_bsplines_kernel(const float* __restrict__ x, long ldx, long N, int in, int C,
                                    const float* __restrict__ grid, int nknots, float* __restrict__ bases) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= N * in) return;
    const long n = i / in; const int f = (int)(i - n * in);
    float Nv[K + 1], dummy[K + 1];
    const int m = bspline_generic<K, false>(x[n * ldx + f], grid + (long)f * nknots, nknots, Nv, dummy);
    float* b = bases + i * C;
    for (int c = 0; c < C; ++c) b[c] = pick_basis<K>(Nv, m, c);
}

int kan_bsplines(const float* x, long ldx, long N, const float* grid, int in, int G, int K, float* bases,
                 hipStream_t st) {
    const int nk = G + 2 * K + 1, C = G + K;
    if (N * in == 0) return KAGNN_OK;
    const int blocks = cdiv(N * in, 256);
#define L(KK) kan_bsplines_kernel<KK><<<blocks, 256, 0, st>>>(x, ldx, N, in, C, grid, nk, bases)
    switch (K) {
        case 1: L(1); break;
        case 2: L(2); break;
        case 3: L(3); break;
        case 4: L(4); break;
        default: return fail(KAGNN_ERR_UNSUPPORTED, "%s: spline_order must be 1..4", "kan_bsplines");
    }
#undef L
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

// ------------------------------------------------------------------ the refit: Gram matrices, reduction, per-feature solve
constexpr int kResizeMaxNb = 3;                                   // ceil(46 / 16)
constexpr int kResizeMaxBlocks = 2 * kResizeMaxNb - 1 + kResizeMaxNb * kResizeMaxNb;      // 5 of G1 + 9 of G2
constexpr int kResizeMaxC = kMaxKnots - 2;                        // G + k at k = 1
__host__ __device__ inline int resize_nb(int C) { return (C + 15) >> 4; }
__host__ __device__ inline int resize_blocks(int Cn, int Co) { return 2 * resize_nb(Cn) - 1 + resize_nb(Cn) * resize_nb(Co); }

// workgroup (chunk, f): its four waves take the chunk's rows in interleaved groups of 64, 4 rows per MFMA (k-lane l>>4 <-> row),
// lane l feeds basis 16 b + (l & 15) of block b.  The waves' partials are added in LDS in wave order, then slab[f][chunk][block][16][16] is written:
// blocks 2 bi - (bi - bj) of G1 (bi - bj in {0, 1}), then n1 + bi * nbo + bj of G2.
template <int K>
__global__ __launch_bounds__(256) void kan_grid_resize_gram_kernel(
    const float* __restrict__ x, long ldx, long N, int Cn, int Co, const float* __restrict__ grid_old, int nko,
    const float* __restrict__ grid_new, int nkn, const float* __restrict__ window, long rows_per_wg, double* __restrict__ slab) {
    __shared__ float s_tn[kMaxKnots], s_to[kMaxKnots];
    __shared__ double s_red[kResizeMaxBlocks * 256];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f = blockIdx.y, i = lane & 15, k = lane >> 4;
    const int nbn = resize_nb(Cn), nbo = resize_nb(Co), n1 = 2 * nbn - 1, nblk = n1 + nbn * nbo;
    if (threadIdx.x < nkn) s_tn[threadIdx.x] = grid_new[(long)f * nkn + threadIdx.x];
    if (threadIdx.x >= 64 && threadIdx.x - 64 < nko) s_to[threadIdx.x - 64] = grid_old[(long)f * nko + threadIdx.x - 64];
    __syncthreads();
    const bool windowed = window != nullptr;
    const float wlo = windowed ? window[2 * f] : 0.0f, whi = windowed ? window[2 * f + 1] : 0.0f;
    const long rbeg = (long)blockIdx.x * rows_per_wg, rend = min(N, rbeg + rows_per_wg);
    f64x4 g1[2 * kResizeMaxNb - 1], g2[kResizeMaxNb * kResizeMaxNb];
#pragma unroll
    for (int b = 0; b < 2 * kResizeMaxNb - 1; ++b) g1[b] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int b = 0; b < kResizeMaxNb * kResizeMaxNb; ++b) g2[b] = f64x4{0.0, 0.0, 0.0, 0.0};
    // a wave takes 64 rows at a time: lane l evaluates row n0 + l ONCE (two knot searches, two Cox-de Boor recursions), then the
    // 16 MFMA steps of 4 rows each fetch their row's span index and k + 1 values from the lane that holds them
    for (long n0 = rbeg + 64 * wave; n0 < rend; n0 += 256) {
        const long n = n0 + lane;
        const float xv = x[min(n, N - 1) * ldx + f];
        float Nn[K + 1], No[K + 1], dummy[K + 1];
        const int mn = bspline_generic<K, false>(xv, s_tn, nkn, Nn, dummy);
        const int mo = bspline_generic<K, false>(xv, s_to, nko, No, dummy);
        const bool live = n < rend && (!windowed || (xv >= wlo && xv < whi));
#pragma unroll
        for (int r = 0; r <= K; ++r) { Nn[r] = live ? Nn[r] : 0.0f; No[r] = live ? No[r] : 0.0f; }
        const int steps = (int)min(16L, (rend - n0 + 3) >> 2);
        for (int s = 0; s < steps; ++s) {
            const int src = 4 * s + k;
            const int smn = __shfl(mn, src), smo = __shfl(mo, src);
            float rn[K + 1], ro[K + 1];
#pragma unroll
            for (int r = 0; r <= K; ++r) { rn[r] = __shfl(Nn[r], src); ro[r] = __shfl(No[r], src); }
            double an[kResizeMaxNb], ao[kResizeMaxNb];
#pragma unroll
            for (int b = 0; b < kResizeMaxNb; ++b) {
                const int c = 16 * b + i;
                an[b] = c < Cn ? (double)pick_basis<K>(rn, smn, c) : 0.0;
                ao[b] = c < Co ? (double)pick_basis<K>(ro, smo, c) : 0.0;
            }
#pragma unroll
            for (int bi = 0; bi < kResizeMaxNb; ++bi) {
                if (bi < nbn) {
                    g1[2 * bi] = __builtin_amdgcn_mfma_f64_16x16x4f64(an[bi], an[bi], g1[2 * bi], 0, 0, 0);
                    if (bi > 0) g1[2 * bi - 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(an[bi], an[bi > 0 ? bi - 1 : 0], g1[2 * bi - 1], 0, 0, 0);
#pragma unroll
                    for (int bj = 0; bj < kResizeMaxNb; ++bj)
                        if (bj < nbo) g2[bi * kResizeMaxNb + bj] = __builtin_amdgcn_mfma_f64_16x16x4f64(an[bi], ao[bj], g2[bi * kResizeMaxNb + bj], 0, 0, 0);
                }
            }
        }
    }
    // C/D of the f64 form: col = lane & 15, row = (lane >> 4) + 4 * reg.  One wave at a time, in wave order: the same bits every run
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int bi = 0; bi < kResizeMaxNb; ++bi) {
                if (bi < nbn) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int e = (k + 4 * r) * 16 + i;
                        double* d = s_red + (2 * bi) * 256 + e;
                        *d = w == 0 ? g1[2 * bi][r] : *d + g1[2 * bi][r];
                        if (bi > 0) {
                            double* s = s_red + (2 * bi - 1) * 256 + e;
                            *s = w == 0 ? g1[bi > 0 ? 2 * bi - 1 : 0][r] : *s + g1[bi > 0 ? 2 * bi - 1 : 0][r];
                        }
#pragma unroll
                        for (int bj = 0; bj < kResizeMaxNb; ++bj) {
                            if (bj < nbo) {
                                double* q = s_red + (n1 + bi * nbo + bj) * 256 + e;
                                *q = w == 0 ? g2[bi * kResizeMaxNb + bj][r] : *q + g2[bi * kResizeMaxNb + bj][r];
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
    double* o = slab + ((long)f * gridDim.x + blockIdx.x) * nblk * 256;
    for (int e = threadIdx.x; e < nblk * 256; e += 256) o[e] = s_red[e];
}

// gram[f][block][16][16] = sum_s slab[f][s][block][..] in slab order
__global__ __launch_bounds__(256) void kan_grid_resize_reduce_kernel(const double* __restrict__ slab, long S, int nblk,
                                                                     double* __restrict__ gram) {
    const int f = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const double* p = slab + ((long)f * S * nblk + b) * 256 + t;
    double a = 0.0;
    for (long s = 0; s < S; ++s) a += p[s * nblk * 256];
    gram[((long)f * nblk + b) * 256 + t] = a;
}

// per-feature solve G1 S = G2 W in LDS.  G1 is banded (half-width K) and its Cholesky factor keeps the band, so the factorisation
// and both substitutions touch K entries per row.  A pivot at or below 1e-13 of the largest diagonal entry is dead: coefficient 0.
// Where every dead pivot belongs to a basis no participating row reached (a zero diagonal entry) that is the minimum-norm answer,
// and `untouched` counts them.  A dead pivot of a basis that WAS reached means rows too few to tell neighbouring bases apart (one
// row: rank 1); dropping that basis would keep the fitted function but not give the minimum-norm coefficients a least-squares
// solve returns, so such a feature is factorised again with a ridge of 1e-10 of the largest diagonal entry on the reached bases.
constexpr int kResizeOutChunk = 32;
__global__ __launch_bounds__(256) void kan_grid_resize_solve_kernel(const double* __restrict__ gram, int in, int out, int Cn, int Co,
                                                                    int K, const float* __restrict__ sw,
                                                                    const float* __restrict__ sc, float* __restrict__ new_sw,
                                                                    int* __restrict__ untouched) {
    __shared__ double L[kResizeMaxC][kResizeMaxC + 1];
    __shared__ double X[kResizeMaxC][kResizeMaxC + 1];
    __shared__ double W[kResizeMaxC][kResizeOutChunk + 1];
    __shared__ double Y[kResizeMaxC][kResizeOutChunk + 1];
    __shared__ double diag[kResizeMaxC];
    __shared__ int dead[kResizeMaxC];
    const int f = blockIdx.x, t = threadIdx.x;
    const int nbn = resize_nb(Cn), nbo = resize_nb(Co), n1 = 2 * nbn - 1, nblk = n1 + nbn * nbo;
    const double* g = gram + (long)f * nblk * 256;
    for (int e = t; e < Cn * Cn; e += blockDim.x) {              // both triangles from the stored lower blocks
        const int r = e / Cn, c = e - r * Cn;
        const int hi = max(r, c), lo = min(r, c), bi = hi >> 4, bj = lo >> 4;
        L[r][c] = bi - bj <= 1 ? g[(2 * bi - (bi - bj)) * 256 + (hi & 15) * 16 + (lo & 15)] : 0.0;
    }
    for (int e = t; e < Cn * Co; e += blockDim.x) {
        const int r = e / Co, c = e - r * Co;
        X[r][c] = g[(n1 + (r >> 4) * nbo + (c >> 4)) * 256 + (r & 15) * 16 + (c & 15)];
    }
    __syncthreads();
    if (t == 0) {                                         // banded Cholesky, in place in the lower triangle
        double dmax = 0.0;
        for (int j = 0; j < Cn; ++j) { diag[j] = L[j][j]; dmax = fmax(dmax, L[j][j]); }
        const double tiny = dmax * 1e-13;
        for (int pass = 0; pass < 2; ++pass) {
            bool again = false;
            for (int j = 0; j < Cn; ++j) {
                double d = L[j][j];
                for (int q = max(0, j - K); q < j; ++q) d -= L[j][q] * L[j][q];
                const bool ok = pass == 0 ? d > tiny : (diag[j] > 0.0 && d > 0.0);
                dead[j] = ok ? 0 : 1;
                again = again || (!ok && diag[j] > 0.0);
                const double piv = ok ? sqrt(d) : 1.0;
                L[j][j] = piv;
                const int rmax = min(Cn - 1, j + K);
                for (int r = j + 1; r <= rmax; ++r) {
                    double v = L[r][j];
                    for (int q = max(0, r - K); q < j; ++q) v -= L[r][q] * L[j][q];
                    L[r][j] = ok ? v / piv : 0.0;
                }
            }
            if (pass == 1 || !again) break;
            for (int j = 0; j < Cn; ++j) {                // the upper triangle still holds G1
                L[j][j] = diag[j] > 0.0 ? diag[j] + dmax * 1e-10 : 0.0;
                for (int r = j + 1; r < Cn; ++r) L[r][j] = L[j][r];
            }
        }
        if (untouched) {
            int cnt = 0;
            for (int j = 0; j < Cn; ++j) cnt += dead[j];
            untouched[f] = cnt;
        }
    }
    __syncthreads();
    for (int o0 = 0; o0 < out; o0 += kResizeOutChunk) {
        const int no = min(kResizeOutChunk, out - o0);
        for (int e = t; e < no * Co; e += blockDim.x) {       // W[c][o] = spline_weight[o][f][c] * scaler[o][f]
            const int oo = e / Co, c = e - oo * Co;
            const long of = (long)(o0 + oo) * in + f;
            W[c][oo] = (double)sw[of * Co + c] * (sc ? (double)sc[of] : 1.0);
        }
        __syncthreads();
        for (int e = t; e < Cn * no; e += blockDim.x) {       // rhs = G2 W
            const int r = e / no, oo = e - r * no;
            double v = 0.0;
            for (int c = 0; c < Co; ++c) v += X[r][c] * W[c][oo];
            Y[r][oo] = v;
        }
        __syncthreads();
        if (t < no) {
            for (int r = 0; r < Cn; ++r) {                    // forward substitution
                double v = Y[r][t];
                for (int q = max(0, r - K); q < r; ++q) v -= L[r][q] * Y[q][t];
                Y[r][t] = dead[r] ? 0.0 : v / L[r][r];
            }
            for (int r = Cn - 1; r >= 0; --r) {               // back substitution with L^T
                double v = Y[r][t];
                const int qmax = min(Cn - 1, r + K);
                for (int q = r + 1; q <= qmax; ++q) v -= L[q][r] * Y[q][t];
                Y[r][t] = dead[r] ? 0.0 : v / L[r][r];
            }
        }
        __syncthreads();
        for (int e = t; e < no * Cn; e += blockDim.x) {
            const int oo = e / Cn, c = e - oo * Cn;
            new_sw[((long)(o0 + oo) * in + f) * Cn + c] = (float)Y[c][oo];
        }
        __syncthreads();
    }
}

static void resize_plan(long N, int in, int* nbx, long* rows_per_wg) {
    long nb = max(1L, min((long)cdiv(N, 4096), (long)max(1, 1024 / in)));
    long r = (N + nb - 1) / nb;
    r = max(256L, (r + 255) & ~255L);
    *nbx = (int)max(1L, (long)cdiv(N, r));
    *rows_per_wg = r;
}

size_t kan_grid_resize_ws_bytes(long N, int in, int Cn, int Co) {
    int nb; long rpw;
    resize_plan(N, in, &nb, &rpw);
    return ((size_t)in * nb + (size_t)in) * resize_blocks(Cn, Co) * 256 * sizeof(double);
}

int kan_grid_resize(const float* x, long ldx, long N, const float* grid_old, const float* grid_new, const float* window, int in,
                    int out, int G_old, int G_new, int K, const float* sw, const float* sc, float* new_sw, int* untouched, void* ws,
                    size_t ws_bytes, hipStream_t st) {
    const int Cn = G_new + K, Co = G_old + K, nkn = G_new + 2 * K + 1, nko = G_old + 2 * K + 1;
    if (Cn > kResizeMaxC || Co > kResizeMaxC) return fail(KAGNN_ERR_UNSUPPORTED, "%s: grid_size + spline_order must be <= 46", "kan_grid_resize");
    if (ws_bytes < kan_grid_resize_ws_bytes(N, in, Cn, Co)) return fail(KAGNN_ERR_ARG, "%s: workspace too small", "kan_grid_resize");
    int nb; long rpw;
    resize_plan(N, in, &nb, &rpw);
    const int nblk = resize_blocks(Cn, Co);
    double* gram = (double*)ws;
    double* slab = gram + (size_t)in * nblk * 256;
    dim3 grid(nb, in);
#define L(KK) kan_grid_resize_gram_kernel<KK><<<grid, 256, 0, st>>>(x, ldx, N, Cn, Co, grid_old, nko, grid_new, nkn, window, rpw, slab)
    switch (K) {
        case 1: L(1); break;
        case 2: L(2); break;
        case 3: L(3); break;
        case 4: L(4); break;
        default: return fail(KAGNN_ERR_UNSUPPORTED, "%s: spline_order must be 1..4", "kan_grid_resize");
    }
#undef L
    KAGNN_LAUNCH_CHECK();
    kan_grid_resize_reduce_kernel<<<dim3(in, nblk), 256, 0, st>>>(slab, (long)nb, nblk, gram);
    KAGNN_LAUNCH_CHECK();
    kan_grid_resize_solve_kernel<<<in, 256, 0, st>>>(gram, in, out, Cn, Co, K, sw, sc, new_sw, untouched);
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

}  // namespace kagnn
