// Symbolic fits of edge functions: for every edge phi_{o,i} sampled on N rows and every function f of a fixed library, the
// affine parameters (a, b, c, d) of  phi(t) ~ c f(a t + b) + d  and the fit's R^2 -- pykan's `suggest_symbolic` / `fit_params`
// (a brute-force grid over (a, b), zoomed `iterations` times), for all edges of a layer at once.  include/kagnn_hip.h
// (kagnn_symbolic_fit) holds the normative rule; this file is three kernels:
//
//   sym_prep_kernel     per edge: ybar (two passes), S_yy, the residual sum of the centred column, the edge's flag
//                       (clean / constant / poisoned by a non-finite x or phi), and the centred column Yc[i][o][n] in the
//                       workspace, n contiguous and zero-padded to a multiple of 8 rows; per feature the column xT[i][n].
//   sym_shared_kernel   iteration 1.  Every output of feature i searches the same (a, b) grid, so u = f(a x_i + b) depends on
//                       (i, f, a, b, n) only and  S_uy[(a,b), o] = sum_n u Yc_i[n, o]  is a GEMM  [Gn^2 x N] x [N x out]  per (i, f).
//                       A wave owns 32 candidates at a time: each lane evaluates u for (candidate lane & 31, rows of its half)
//                       ONCE in registers and feeds it as the A operand of v_mfma_f32_32x32x2_f32 against the centred columns
//                       of up to 64 outputs (B operand, 16-byte loads of 4 consecutive rows; the k order is permuted the same way
//                       for A and B, which a sum over k does not see).  The transcendental runs on the VALU, its `out`
//                       multiply-adds on the matrix pipe.  sum u and sum u^2 are per candidate, shared by all outputs.
//   sym_zoom_kernel     one workgroup per (f, o, i): reduces iteration 1's per-slot maxima, then runs iterations 2.. in the same
//                       launch -- per-edge ranges, so nothing is shared but the two columns, staged in LDS; each lane carries
//                       4 candidates with three accumulators each over the rows -- derives the next ranges in the kernel, and
//                       at the end evaluates the winner once more, in fp64, for (c, d).
//
// Sums.  u enters every sum as w = u - s, s being the candidate's own u at row 0: c, S_uu and S_uy do not see a shift, and the
// products w * Yc stay at the size of u's variation rather than of its mean (the degeneracy threshold lies at a relative
// variance of 1e-5).  sum w and sum w^2 are accumulated in fp64 (two fp64 operations beside a transcendental), so
// S_uu = sum w^2 - (sum w)^2 / N does not cancel; sum w Yc is fp32 (the MFMA in the shared pass, fmaf in the zoom pass) and is
// corrected by (sum w)(sum Yc) / N for the rounding residue of the centring.  A non-finite u makes w and then sum w^2
// non-finite, which is how it is seen: there is no per-element test.  No atomics: every reduction has a fixed order, and
// ties go to the lowest flat candidate index.
//
// Nothing of size N x Gn^2 exists; the workspace (symbolic_ws_bytes) is xT, Yc, 4 floats per edge and 32 (score, index) pairs per
// (f, o, i).  The optional tables / ranges / winners outputs are written by the same kernels.
#include "common.h"
#include "host.h"
#include "symbolic_fn.h"

#include <cfloat>

namespace kagnn {

constexpr int kSymSlots = 32;                 // candidate-tile slots of the shared pass per (f, i): 8 workgroups of 4 waves
constexpr int kSymThreads = 256;
constexpr int kSymC = 4;                      // candidates per lane and batch in the zoom pass
constexpr int kSymChunk = 1024;               // rows staged in LDS at a time in the zoom pass

struct SymEdge {                              // per edge (i * out + o), 16 bytes
    float ybar, syy, rsum, flag;              // flag: 0 clean, 1 constant column (all scores 0), 2 poisoned (and c, d = NaN)
};

struct SymBest {
    float score;
    int idx;
};

static inline long sym_np(long N) { return (N + 7) / 8 * 8; }

size_t symbolic_ws_bytes(long N, int in, int out, int F) {
    const size_t np = (size_t)sym_np(N);
    return sizeof(float) * np * in + sizeof(float) * np * in * out + sizeof(SymEdge) * (size_t)in * out +
           sizeof(SymBest) * (size_t)F * in * out * kSymSlots + 64;
}

// (sym_fn<FID> and its fp64 twin sym_fn_d<FID>: symbolic_fn.h, shared with symbolic_edges.hip)

// candidate k of an axis: (float)(lo + k (hi - lo) / (Gn - 1)), in fp64 as the header states it
__device__ __forceinline__ float sym_axis(float lo, float hi, int k, int Gn) {
    return (float)((double)lo + (double)k * ((double)hi - (double)lo) / (double)(Gn - 1));
}

// the rule's score from a candidate's sums over w = u - s (sw, sww in fp64) and its fp32 sum w Yc
struct SymCand {
    float suu;            // S_uu as fp32, 0 when the candidate is degenerate
    float sw;             // sum w as fp32
    int ok;
};

__device__ __forceinline__ SymCand sym_candidate(double sw, double sww, float s, long N) {
    SymCand c;
    const double n = (double)N;
    const double suu = sww - sw * sw / n;
    const double ubar = (double)s + sw / n;
    const double var = suu / n, mean2 = var + ubar * ubar;
    const double thr = fmax(1e-5 * mean2, 1e-24);
    // (non-finite sums compare false; sum u^2 beyond the fp32 range counts as a non-finite sum)
    c.ok = (sww <= (double)FLT_MAX) && (fabs(sw) <= (double)FLT_MAX) && (n * mean2 <= (double)FLT_MAX) && (var > thr);
    c.suu = c.ok ? (float)suu : 0.0f;
    c.sw = c.ok ? (float)sw : 0.0f;
    return c;
}

__device__ __forceinline__ float sym_score(const SymCand& c, float swy, const SymEdge& e, float inv_n) {
    if (!c.ok || e.flag != 0.0f) return 0.0f;
    const float suy = swy - c.sw * e.rsum * inv_n;
    const float r2 = (suy / c.suu) * (suy / e.syy);
    return (r2 >= 0.0f && r2 <= FLT_MAX) ? r2 : 0.0f;
}

// ------------------------------------------------------------------------------------------------------------ preparation
// 64 consecutive edges (phi's own order e = o * in + i: coalesced) x 4 row groups per workgroup.
__global__ __launch_bounds__(kSymThreads) void sym_prep_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ phi,
                                                               long N, long Np, int in, int out, float* __restrict__ xT,
                                                               float* __restrict__ Yc, SymEdge* __restrict__ edges) {
    __shared__ float red[4][64];
    __shared__ float red2[4][64];
    __shared__ int redf[4][64];
    const int el = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const long ne = (long)in * out;
    const long e = (long)blockIdx.x * 64 + el;
    const bool live = e < ne;
    const int o = live ? (int)(e / in) : 0, i = live ? (int)(e % in) : 0;
    const float* col = phi + (live ? e : 0);

    float sum = 0.0f;
    int bad = 0;
    if (live)
        for (long n = rg; n < N; n += 4) {
            const float y = col[n * ne], xv = x[n * ldx + i];
            bad |= !(fabsf(y) <= FLT_MAX) || !(fabsf(xv) <= FLT_MAX);
            sum += y;
        }
    red[rg][el] = sum;
    redf[rg][el] = bad;
    __syncthreads();
    const float ybar = ((red[0][el] + red[1][el]) + (red[2][el] + red[3][el])) / (float)N;
    bad = redf[0][el] | redf[1][el] | redf[2][el] | redf[3][el];
    __syncthreads();

    float sd = 0.0f, sdd = 0.0f;
    if (live && !bad)
        for (long n = rg; n < N; n += 4) {
            const float d = col[n * ne] - ybar;
            sd += d;
            sdd = fmaf(d, d, sdd);
        }
    red[rg][el] = sd;
    red2[rg][el] = sdd;
    __syncthreads();
    sd = (red[0][el] + red[1][el]) + (red[2][el] + red[3][el]);
    sdd = (red2[0][el] + red2[1][el]) + (red2[2][el] + red2[3][el]);
    const float inv_n = 1.0f / (float)N;
    const float syy = sdd - sd * sd * inv_n;
    const float var = syy * inv_n, mean2 = var + ybar * ybar;
    int flag = 0;
    if (bad) flag = 2;
    else if (!(syy <= FLT_MAX) || !(var > fmaxf(1e-5f * mean2, 1e-24f))) flag = 1;
    if (!live) return;
    if (rg == 0) {
        SymEdge se;
        se.ybar = ybar; se.syy = syy; se.rsum = sd; se.flag = (float)flag;
        edges[(long)i * out + o] = se;
    }
    float* yc = Yc + ((long)i * out + o) * Np;
    for (long n = rg; n < Np; n += 4) yc[n] = (n < N && flag == 0) ? col[n * ne] - ybar : 0.0f;
    if (o == 0) {
        float* xc = xT + (long)i * Np;
        for (long n = rg; n < Np; n += 4) xc[n] = n < N ? x[n * ldx + i] : 0.0f;
    }
}

// ------------------------------------------------------------------------------------------------------------ iteration 1
// TODO: the B fragments are 16-byte loads from 32 different Yc rows per step, served by L1 / L2; staging a row chunk of the
// feature's centred columns in LDS once per workgroup, and more than 8 workgroups per feature, should lift the 42 % of the fp32-MFMA
// rate measured (profiles/symbolic_fit.md).  Left: this pass is 3.5 % of a three-iteration call, the zoom pass is the rest.
// grid (kSymSlots / 4, in); four waves, wave w of block bx is slot bx * 4 + w and owns the candidate tiles slot, slot + 32, ...
// NT: 32-wide output tiles evaluated against one evaluation of u (1 or 2); outputs beyond NT * 32 take another round.
template <int FID, int NT>
__global__ __launch_bounds__(kSymThreads) void sym_shared_kernel(const float* __restrict__ xT, const float* __restrict__ Yc,
                                                                 const SymEdge* __restrict__ edges, long N, long Np, int in, int out,
                                                                 int Gn, float alo, float ahi, float blo, float bhi,
                                                                 SymBest* __restrict__ part, float* __restrict__ table) {
    typedef float accv __attribute__((ext_vector_type(16)));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, kh = lane >> 5;
    const int slot = blockIdx.x * 4 + wave;
    const int i = blockIdx.y;
    const int ncand = Gn * Gn, ntiles = (ncand + 31) / 32;
    const float inv_n = 1.0f / (float)N;
    const float* xc = xT + (long)i * Np;
    const float x0 = xc[0];

    for (int o0 = 0; o0 < out; o0 += NT * 32) {
        const float* yc[NT];
        SymEdge se[NT];
        bool ovalid[NT];
        float best[NT];
        int bidx[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int o = o0 + t * 32 + r;
            ovalid[t] = o < out;
            const long e = (long)i * out + (ovalid[t] ? o : 0);
            yc[t] = Yc + e * Np;
            se[t] = edges[e];
            best[t] = -1.0f;
            bidx[t] = 0x7fffffff;
        }
        for (int tile = slot; tile < ntiles; tile += kSymSlots) {
            const int cand = tile * 32 + r;
            const int cc = cand < ncand ? cand : ncand - 1;
            const float a = sym_axis(alo, ahi, cc / Gn, Gn), b = sym_axis(blo, bhi, cc % Gn, Gn);
            const float s = sym_fn<FID>(fmaf(a, x0, b));
            double sw = 0.0, sww = 0.0;
            accv acc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int j = 0; j < 16; ++j) acc[t][j] = 0.0f;
            for (long base = 0; base < Np; base += 8) {
                const long n0 = base + kh * 4;                       // this half-wave's four rows of the step
                const float4 xv = *reinterpret_cast<const float4*>(xc + n0);
                float4 yv[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    yv[t] = ovalid[t] ? *reinterpret_cast<const float4*>(yc[t] + n0) : make_float4(0.f, 0.f, 0.f, 0.f);
                const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float w = sym_fn<FID>(fmaf(a, xs[j], b)) - s;
                    if (n0 + j >= N) w = 0.0f;                       // the zero padding of the columns is no row
                    const double wd = (double)w;
                    sw += wd;
                    sww = fma(wd, wd, sww);
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const float yj = j == 0 ? yv[t].x : j == 1 ? yv[t].y : j == 2 ? yv[t].z : yv[t].w;
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(w, yj, acc[t], 0, 0, 0);
                    }
                }
            }
            // the two halves of the rows: lanes r and r + 32 hold the same candidate
            sw += __shfl_xor(sw, 32);
            sww += __shfl_xor(sww, 32);
            const SymCand c = sym_candidate(sw, sww, s, N);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int m = mfma32_row(j, kh);                      // this accumulator register's candidate within the tile
                SymCand cm;
                cm.suu = __shfl(c.suu, m);
                cm.sw = __shfl(c.sw, m);
                cm.ok = __shfl(c.ok, m);
                const int cj = tile * 32 + m;
                if (cj >= ncand) continue;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    if (!ovalid[t]) continue;
                    const float r2 = sym_score(cm, acc[t][j], se[t], inv_n);
                    if (table) table[((long)(o0 + t * 32 + r) * in + i) * ncand + cj] = r2;
                    if (r2 > best[t]) { best[t] = r2; bidx[t] = cj; }            // (ascending cj per lane: first maximum kept)
                }
            }
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float ob = __shfl_xor(best[t], 32);
            const int oi = __shfl_xor(bidx[t], 32);
            if (ob > best[t] || (ob == best[t] && oi < bidx[t])) { best[t] = ob; bidx[t] = oi; }
            if (kh == 0 && ovalid[t]) {
                SymBest sb;
                sb.score = best[t]; sb.idx = bidx[t];
                part[((long)(o0 + t * 32 + r) * in + i) * kSymSlots + slot] = sb;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ iterations 2..
__device__ __forceinline__ void sym_better(float& s, int& i, float s2, int i2) {
    if (s2 > s || (s2 == s && i2 < i)) { s = s2; i = i2; }
}

// grid (out * in): block e = o * in + i (the outputs' own order).  part: this function's [out][in][kSymSlots].
// table / ranges / winners (optional): this function's slice of iteration 0, `it_stride*` elements between iterations.
template <int FID>
__global__ __launch_bounds__(kSymThreads) void sym_zoom_kernel(const float* __restrict__ xT, const float* __restrict__ Yc,
                                                               const SymEdge* __restrict__ edges, long N, long Np, int in, int out,
                                                               int Gn, int iterations, float alo, float ahi, float blo, float bhi,
                                                               const SymBest* __restrict__ part, float* __restrict__ params,
                                                               float* __restrict__ r2_out, float* __restrict__ table, long it_table,
                                                               float* __restrict__ ranges, long it_ranges, int* __restrict__ winners,
                                                               long it_winners) {
    __shared__ float2 sxy[kSymChunk];
    __shared__ float sav[128], sbv[128];
    __shared__ float rs[kSymThreads];
    __shared__ int ri[kSymThreads];
    __shared__ double rd[3][kSymThreads];
    const int tid = threadIdx.x;
    const long eo = blockIdx.x;                               // o * in + i
    const int o = (int)(eo / in), i = (int)(eo % in);
    const SymEdge se = edges[(long)i * out + o];
    const float* xc = xT + (long)i * Np;
    const float* yc = Yc + ((long)i * out + o) * Np;
    const int ncand = Gn * Gn;
    const float inv_n = 1.0f / (float)N;
    const float x0 = xc[0];
    const bool dead = se.flag != 0.0f;

    // iteration 1's winner: the slots' maxima in slot order
    float wscore = -1.0f;
    int widx = 0x7fffffff;
    for (int sl = 0; sl < kSymSlots; ++sl) {
        const SymBest sb = part[eo * kSymSlots + sl];
        sym_better(wscore, widx, sb.score, sb.idx);
    }
    float r_alo = alo, r_ahi = ahi, r_blo = blo, r_bhi = bhi;
    if (tid == 0) {
        if (ranges) { float* p = ranges + eo * 4; p[0] = r_alo; p[1] = r_ahi; p[2] = r_blo; p[3] = r_bhi; }
        if (winners) winners[eo] = widx;
    }

    for (int it = 1; it < iterations; ++it) {
        // the next ranges, per axis: an interior winner k gives [v_{k-1}, v_{k+1}], the ends [v_0, v_1] and [v_{Gn-2}, v_{Gn-1}]
        {
            const int ka = widx / Gn, kb = widx % Gn;
            const int la = ka == 0 ? 0 : (ka == Gn - 1 ? Gn - 2 : ka - 1), ha = ka == 0 ? 1 : (ka == Gn - 1 ? Gn - 1 : ka + 1);
            const int lb = kb == 0 ? 0 : (kb == Gn - 1 ? Gn - 2 : kb - 1), hb = kb == 0 ? 1 : (kb == Gn - 1 ? Gn - 1 : kb + 1);
            const float n_alo = sym_axis(r_alo, r_ahi, la, Gn), n_ahi = sym_axis(r_alo, r_ahi, ha, Gn);
            const float n_blo = sym_axis(r_blo, r_bhi, lb, Gn), n_bhi = sym_axis(r_blo, r_bhi, hb, Gn);
            r_alo = n_alo; r_ahi = n_ahi; r_blo = n_blo; r_bhi = n_bhi;
        }
        __syncthreads();                                      // the previous iteration's readers of sav / sbv / rs / ri are done
        if (tid < Gn) { sav[tid] = sym_axis(r_alo, r_ahi, tid, Gn); sbv[tid] = sym_axis(r_blo, r_bhi, tid, Gn); }
        if (tid == 0 && ranges) { float* p = ranges + it * it_ranges + eo * 4; p[0] = r_alo; p[1] = r_ahi; p[2] = r_blo; p[3] = r_bhi; }
        __syncthreads();
        float* tab = table ? table + it * it_table + eo * ncand : nullptr;
        float best = -1.0f;
        int bidx = 0x7fffffff;
        for (int c0 = 0; c0 < ncand; c0 += kSymThreads * kSymC) {
            float a[kSymC], b[kSymC], s[kSymC], swy[kSymC];
            double sw[kSymC], sww[kSymC];
#pragma unroll
            for (int j = 0; j < kSymC; ++j) {
                const int c = c0 + j * kSymThreads + tid;
                const int cc = c < ncand ? c : ncand - 1;
                a[j] = sav[cc / Gn]; b[j] = sbv[cc % Gn];
                s[j] = sym_fn<FID>(fmaf(a[j], x0, b[j]));
                swy[j] = 0.0f; sw[j] = 0.0; sww[j] = 0.0;
            }
            if (!dead) {
                for (long nb = 0; nb < N; nb += kSymChunk) {
                    const int rows = (int)min((long)kSymChunk, N - nb);
                    __syncthreads();                          // the previous chunk's readers are done
                    for (int n = tid; n < rows; n += kSymThreads) sxy[n] = make_float2(xc[nb + n], yc[nb + n]);
                    __syncthreads();
                    for (int n = 0; n < rows; ++n) {
                        const float2 xy = sxy[n];
#pragma unroll
                        for (int j = 0; j < kSymC; ++j) {
                            const float w = sym_fn<FID>(fmaf(a[j], xy.x, b[j])) - s[j];
                            const double wd = (double)w;
                            sw[j] += wd;
                            sww[j] = fma(wd, wd, sww[j]);
                            swy[j] = fmaf(w, xy.y, swy[j]);
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < kSymC; ++j) {
                const int c = c0 + j * kSymThreads + tid;
                if (c >= ncand) continue;
                float r2 = 0.0f;
                if (!dead) r2 = sym_score(sym_candidate(sw[j], sww[j], s[j], N), swy[j], se, inv_n);
                if (tab) tab[c] = r2;
                if (r2 > best) { best = r2; bidx = c; }       // (ascending c per lane: first maximum kept)
            }
        }
        rs[tid] = best; ri[tid] = bidx;
        __syncthreads();
        for (int step = kSymThreads / 2; step > 0; step >>= 1) {
            if (tid < step) {
                float s1 = rs[tid];
                int i1 = ri[tid];
                sym_better(s1, i1, rs[tid + step], ri[tid + step]);
                rs[tid] = s1; ri[tid] = i1;
            }
            __syncthreads();
        }
        wscore = rs[0]; widx = ri[0];
        if (tid == 0 && winners) winners[it * it_winners + eo] = widx;
    }

    // the result: the last iteration's winner, evaluated once more over the rows for c and d (fp64 sums, fixed order)
    const float a = sym_axis(r_alo, r_ahi, widx / Gn, Gn), b = sym_axis(r_blo, r_bhi, widx % Gn, Gn);
    // (the mean of the column in fp64: the prep kernel's fp32 mean plus the residue of its centring, as S_uy is corrected for it)
    const double ybar = (double)se.ybar + (double)se.rsum / (double)N;
    float cpar = 0.0f, dpar = (float)ybar;
    if (wscore > 0.0f) {                                      // (block-uniform)
        // (t in fp32 as everywhere; f, the shift and the sums in fp64)
        const double s = sym_fn_d<FID>((double)fmaf(a, x0, b));
        double sw = 0.0, sww = 0.0, swy = 0.0;
        for (long n = tid; n < N; n += kSymThreads) {
            const double wd = sym_fn_d<FID>((double)fmaf(a, xc[n], b)) - s;
            sw += wd;
            sww = fma(wd, wd, sww);
            swy = fma(wd, (double)yc[n], swy);
        }
        __syncthreads();
        rd[0][tid] = sw; rd[1][tid] = sww; rd[2][tid] = swy;
        __syncthreads();
        for (int step = kSymThreads / 2; step > 0; step >>= 1) {
            if (tid < step) {
                rd[0][tid] += rd[0][tid + step]; rd[1][tid] += rd[1][tid + step]; rd[2][tid] += rd[2][tid + step];
            }
            __syncthreads();
        }
        const double n = (double)N;
        sw = rd[0][0]; sww = rd[1][0]; swy = rd[2][0];
        const double suu = sww - sw * sw / n, suy = swy - sw * (double)se.rsum / n;
        const double cd = suy / suu;
        cpar = (float)cd;
        dpar = (float)(ybar - cd * (s + sw / n));
    }
    if (tid == 0) {
        if (se.flag == 2.0f) cpar = dpar = __builtin_nanf("");
        float* p = params + eo * 4;
        p[0] = a; p[1] = b; p[2] = cpar; p[3] = dpar;
        r2_out[eo] = wscore > 0.0f ? wscore : 0.0f;
    }
}

// ------------------------------------------------------------------------------------------------------------ host
struct SymArgs {
    const float *xT, *Yc;
    const SymEdge* edges;
    long N, Np;
    int in, out, Gn, iterations;
    float alo, ahi, blo, bhi;
    SymBest* part;
    float *params, *r2, *table;
    long it_table;
    float* ranges;
    long it_ranges;
    int* winners;
    long it_winners;
};

template <int FID>
static void sym_launch_one(const SymArgs& g, hipStream_t st) {
    dim3 grid(kSymSlots / 4, (unsigned)g.in);
    if (g.out <= 32)
        sym_shared_kernel<FID, 1><<<grid, kSymThreads, 0, st>>>(g.xT, g.Yc, g.edges, g.N, g.Np, g.in, g.out, g.Gn, g.alo, g.ahi, g.blo,
                                                                g.bhi, g.part, g.table);
    else
        sym_shared_kernel<FID, 2><<<grid, kSymThreads, 0, st>>>(g.xT, g.Yc, g.edges, g.N, g.Np, g.in, g.out, g.Gn, g.alo, g.ahi, g.blo,
                                                                g.bhi, g.part, g.table);
    sym_zoom_kernel<FID><<<(unsigned)((long)g.in * g.out), kSymThreads, 0, st>>>(
        g.xT, g.Yc, g.edges, g.N, g.Np, g.in, g.out, g.Gn, g.iterations, g.alo, g.ahi, g.blo, g.bhi, g.part, g.params, g.r2, g.table,
        g.it_table, g.ranges, g.it_ranges, g.winners, g.it_winners);
}

template <int... IDS>
static void sym_dispatch(int fid, const SymArgs& g, hipStream_t st, std::integer_sequence<int, IDS...>) {
    ((fid == IDS ? sym_launch_one<IDS>(g, st) : (void)0), ...);
}

int symbolic_fit(const float* x, long ldx, const float* phi, long N, int in, int out, const int* functions, int F, float alo,
                 float ahi, float blo, float bhi, int Gn, int iterations, float* params, float* r2, float* tables, float* ranges,
                 int* winners, void* ws, size_t ws_bytes, hipStream_t st) {
    if (ws_bytes < symbolic_ws_bytes(N, in, out, F)) return fail(KAGNN_ERR_ARG, "%s: workspace too small", "symbolic_fit");
    const long ne = (long)in * out, Np = sym_np(N), ncand = (long)Gn * Gn;
    if (in > 65535 || ne > 0x7fffffffL / kSymSlots || ne * ncand > 0x7fffffffffL)
        return fail(KAGNN_ERR_UNSUPPORTED, "%s: shape too large for one launch", "symbolic_fit");
    char* p = static_cast<char*>(ws);
    p += (16 - ((uintptr_t)p & 15)) & 15;                    // (the 64 spare bytes of the size cover this)
    float* xT = reinterpret_cast<float*>(p);
    float* Yc = xT + Np * in;
    SymEdge* edges = reinterpret_cast<SymEdge*>(Yc + Np * ne);
    SymBest* part = reinterpret_cast<SymBest*>(edges + ne);
    sym_prep_kernel<<<(unsigned)((ne + 63) / 64), kSymThreads, 0, st>>>(x, ldx, phi, N, Np, in, out, xT, Yc, edges);
    KAGNN_LAUNCH_CHECK();
    for (int f = 0; f < F; ++f) {
        SymArgs g{xT, Yc, edges, N, Np, in, out, Gn, iterations, alo, ahi, blo, bhi, part + (long)f * ne * kSymSlots,
                  params + (long)f * ne * 4, r2 + (long)f * ne,
                  tables ? tables + (long)f * ne * ncand : nullptr, (long)F * ne * ncand,
                  ranges ? ranges + (long)f * ne * 4 : nullptr, (long)F * ne * 4,
                  winners ? winners + (long)f * ne : nullptr, (long)F * ne};
        sym_dispatch(functions[f], g, st, std::make_integer_sequence<int, KAGNN_SYMBOLIC_NUM_FUNCTIONS>{});
        KAGNN_LAUNCH_CHECK();
    }
    return KAGNN_OK;
}

}  // namespace kagnn
