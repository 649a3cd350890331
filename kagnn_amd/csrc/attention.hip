// Dense multi-head attention with the bias added AFTER the softmax, and its backward, exact fp32.
//
// Reference behaviour replaced: the core of AttentionWithFastKANTransform.forward (node_classification_clean/fastkan.py:182-198)
// between the projections and linear_o, and the autograd backward of those broadcast products:
//   s[q,k,h] = scale * <wq[q,h,:], wk[k,h,:]>      p = softmax over k of s      a = p + bias[q,k]   (the same bias for every head)
//   o[q,h,:] = sum_k a[q,k,h] wv[k,h,:]            o *= sigmoid(gate[q,h,:])    (with a gate)
// The reference materialises [*, Q, K, H, c] twice and [*, Q, K, H] once; nothing of size Q*K exists here except g_bias, which
// is a result.
//
// Every product runs on the VALU as an ordered fp32 fma chain.  There is no split- or reduced-precision form: KAGNN_PRECISION
// does not reach these kernels.  No atomics: every sum has one owner and a fixed order, the same inputs give the same bits.
//
// One thread layout serves the three kernels.  A workgroup of 256 threads owns 64 rows of one (batch, head) -- queries in the
// forward and in the dQ kernel, keys in the dK/dV kernel -- one row per QUAD of lanes.  Lane t of a quad holds the 16-byte
// chunks t, t+4, t+8, .. of the row's c channels (NCH chunks: c <= 32, 64, 128 -> NCH = 2, 4, 8; channels past c are zeros),
// so a quad reads 64 contiguous bytes of a global or an LDS row at a time.  The other side is walked in tiles of 32 rows
// staged in LDS (zero outside [rows, c]); every lane of a wave reads the same LDS row (a broadcast).  A logit is the lane's
// partial dot product over its chunks, summed over the quad by an xor butterfly, which leaves the same bits in its four
// lanes; the forward, the dQ and the dK/dV kernel form the logit in the same order, so the backward's p is the forward's.
//
// Forward: an online softmax over chunks of 16 keys: running maximum m and sum l, the accumulator is rescaled by exp(m - m')
// whenever the maximum rises.  o = acc / l + bacc with bacc = sum_k bias[q,k] wv[k] kept apart (it is not rescaled).  With
// `stats` the kernel also leaves the ungated o and the row statistics m and log l.
//
// Backward (d_o: the gradient of the UNGATED o; p = exp((s - m) - log l) recomputed):
//   dA[q,k,h] = <d_o[q,h,:], wv[k,h,:]>      g_wv[k] = sum_q a d_o[q]      g_bias[q,k] = sum_h dA   (= d_o[b] wv[b]^T: linear.hip)
//   D[q,h] = sum_k p dA                       dS = p (dA - D)
//   g_wq[q] = scale sum_k dS wk[k]            g_wk[k] = scale sum_q dS wq[q]
// The usual shortcut D = <d_o, o> is WRONG with a bias: <d_o, o> = D + sum_k bias dA.  With a bias the dQ kernel walks K twice
// (D first, from p itself, divided by sum_k p); without one it takes the shortcut, which is then exact.  D goes to the workspace for the dK/dV
// kernel.  With a gate a pre-pass leaves d_o = g_out * sig in the workspace and writes g_gate = g_out * o_ungated * sig (1 - sig).
#include "common.h"
#include "host.h"

namespace kagnn {

constexpr int kAttThreads = 256;
constexpr int kAttRows = 64;       // rows a workgroup owns (one per quad)
constexpr int kAttTile = 32;       // rows of the walked side per LDS tile
constexpr int kAttChunk = 16;      // logits held in registers at a time

struct AttMat {            // [B*rows, H*c] rows: element (b, row, h, ch) at p[(b*rows + row)*ld + h*c + ch]
    const float* p;
    long ld;
    int vec;               // 16-byte accesses allowed: p 16-byte aligned, ld % 4 == 0, c % 4 == 0
};
struct AttOut {
    float* p;
    long ld;
    int vec;
};

struct AttArgs {
    AttMat wq, wk, wv, gate, oung, dout;     // dout: d_o (backward)
    const float* bias; long bias_bs, bias_rs;
    long Q, K;
    int H, c;
    long tiles;                              // row tiles of the owned side per (batch, head)
    float scale;
    AttOut o, oung_w, gq, gk, gv;
    float* stats_w;                          // forward: [2][B*Q*H] (m, log l) or nullptr
    const float* stats;                      // backward
    float* Dw;                               // dQ kernel: D[B*Q*H] out
    const float* D;                          // dK/dV kernel
    long BQH;
};

template <int NCH>
__device__ __forceinline__ void att_load_row(float (&r)[4 * NCH], const AttMat& m, long row, int h, int c, int t, bool valid, float mul) {
    const float* p = m.p + row * m.ld + (long)h * c;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int col = 4 * (t + 4 * i);
        if (valid && m.vec && col < c) {
            const float4 v = *reinterpret_cast<const float4*>(p + col);
            r[4 * i + 0] = v.x * mul; r[4 * i + 1] = v.y * mul; r[4 * i + 2] = v.z * mul; r[4 * i + 3] = v.w * mul;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) r[4 * i + e] = (valid && col + e < c) ? p[col + e] * mul : 0.0f;
        }
    }
}

template <int NCH>
__device__ __forceinline__ void att_store_row(const float (&r)[4 * NCH], const AttOut& m, long row, int h, int c, int t, bool valid) {
    if (!valid) return;
    float* p = m.p + row * m.ld + (long)h * c;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int col = 4 * (t + 4 * i);
        if (m.vec && col < c) {
            *reinterpret_cast<float4*>(p + col) = make_float4(r[4 * i + 0], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (col + e < c) p[col + e] = r[4 * i + e];
        }
    }
}

// rows [row0, row0 + 32) of batch-local row range [0, rows) -> s[j][16 * NCH], times mul; zeros outside [rows, c]
template <int NCH>
__device__ __forceinline__ void att_stage(float* s, const AttMat& m, long base_row, long row0, long rows, int h, int c, float mul) {
    constexpr int CQ = 4 * NCH;                    // float4 items per row
    constexpr int ITEMS = kAttTile * CQ;
#pragma unroll
    for (int u = 0; u < ITEMS / kAttThreads; ++u) {
        const int idx = threadIdx.x + u * kAttThreads;
        const int j = idx / CQ, col = 4 * (idx % CQ);
        const long row = row0 + j;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < rows && col < c) {
            const float* p = m.p + (base_row + row) * m.ld + (long)h * c + col;
            if (m.vec) {
                v = *reinterpret_cast<const float4*>(p);
            } else {
                v.x = p[0];
                if (col + 1 < c) v.y = p[1];
                if (col + 2 < c) v.z = p[2];
                if (col + 3 < c) v.w = p[3];
            }
            v.x *= mul; v.y *= mul; v.z *= mul; v.w *= mul;
        }
        *reinterpret_cast<float4*>(s + j * (16 * NCH) + col) = v;
    }
}

// sum over the four lanes of a quad, the same bits in all four: (a + b) + (c + d) up to the order inside each pair.  DPP quad
// permutes: __shfl_xor compiles to ds_bpermute here, two LDS operations per logit beside the 2 * NCH reads it is made of
__device__ __forceinline__ float att_quad_sum(float a) {
    a += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(a), 0xB1, 0xf, 0xf, true));    // quad_perm [1,0,3,2]
    a += __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(a), 0x4E, 0xf, 0xf, true));    // quad_perm [2,3,0,1]
    return a;
}

// the lane's partial <r, s row j> over its chunks, summed over the quad (the same bits in the four lanes)
template <int NCH>
__device__ __forceinline__ float att_dot(const float (&r)[4 * NCH], const float* srow, int t) {
    float a = 0.0f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const float4 v = *reinterpret_cast<const float4*>(srow + 4 * (t + 4 * i));
        a = fmaf(r[4 * i + 0], v.x, a); a = fmaf(r[4 * i + 1], v.y, a);
        a = fmaf(r[4 * i + 2], v.z, a); a = fmaf(r[4 * i + 3], v.w, a);
    }
    return att_quad_sum(a);
}

template <int NCH>
__device__ __forceinline__ void att_axpy(float (&acc)[4 * NCH], float w, const float* srow, int t) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const float4 v = *reinterpret_cast<const float4*>(srow + 4 * (t + 4 * i));
        acc[4 * i + 0] = fmaf(w, v.x, acc[4 * i + 0]); acc[4 * i + 1] = fmaf(w, v.y, acc[4 * i + 1]);
        acc[4 * i + 2] = fmaf(w, v.z, acc[4 * i + 2]); acc[4 * i + 3] = fmaf(w, v.w, acc[4 * i + 3]);
    }
}

__device__ __forceinline__ void att_block(const AttArgs& a, long& b, int& h, long& tile) {
    const long id = blockIdx.x;
    tile = id % a.tiles;
    const long bh = id / a.tiles;
    h = (int)(bh % a.H);
    b = bh / a.H;
}

// ---------------------------------------------------------------- forward
template <int NCH, bool BIAS>
__global__ __launch_bounds__(kAttThreads) void attention_fwd_kernel(AttArgs a) {
    constexpr int CP = 4 * NCH, LD = 4 * CP;
    __shared__ __attribute__((aligned(16))) float sK[kAttTile * LD];
    __shared__ __attribute__((aligned(16))) float sV[kAttTile * LD];
    long b, tile; int h;
    att_block(a, b, h, tile);
    const int t = threadIdx.x & 3;
    const long q = tile * kAttRows + (threadIdx.x >> 2);
    const bool valid = q < a.Q;
    const long qrow = b * a.Q + q;

    float qr[CP], acc[CP], bacc[CP];
    att_load_row<NCH>(qr, a.wq, qrow, h, a.c, t, valid, a.scale);
#pragma unroll
    for (int i = 0; i < CP; ++i) { acc[i] = 0.0f; bacc[i] = 0.0f; }
    float m = -INFINITY, l = 0.0f;
    // (a lane past Q reads row 0 of its batch, which exists, and drops the value)
    const float* brow = BIAS ? a.bias + b * a.bias_bs + (valid ? q : 0) * a.bias_rs : nullptr;

    for (long k0 = 0; k0 < a.K; k0 += kAttTile) {
        __syncthreads();                                   // the previous tile's readers are done
        att_stage<NCH>(sK, a.wk, b * a.K, k0, a.K, h, a.c, 1.0f);
        att_stage<NCH>(sV, a.wv, b * a.K, k0, a.K, h, a.c, 1.0f);
        __syncthreads();
#pragma unroll 1
        for (int j0 = 0; j0 < kAttTile; j0 += kAttChunk) {
            if (k0 + j0 >= a.K) break;                     // (block-uniform)
            float s[kAttChunk], bj[kAttChunk];
            float mt = -INFINITY;
            if (BIAS) {                                    // unconditional loads at a clamped index (branches here made the compiler spill)
#pragma unroll
                for (int j = 0; j < kAttChunk; ++j) {
                    const long kk = k0 + j0 + j;
                    const float v = brow[min(kk, a.K - 1)];
                    bj[j] = (valid && kk < a.K) ? v : 0.0f;
                }
            }
#pragma unroll
            for (int j = 0; j < kAttChunk; ++j) {
                const float d = att_dot<NCH>(qr, sK + (j0 + j) * LD, t);
                s[j] = k0 + j0 + j < a.K ? d : -INFINITY;
                mt = fmaxf(mt, s[j]);
            }
            if (mt > m) {                                  // the maximum rises: rescale what has been summed (exp(-inf) = 0 the first time)
                const float r = expf(m - mt);
                l *= r;
#pragma unroll
                for (int i = 0; i < CP; ++i) acc[i] *= r;
                m = mt;
            }
#pragma unroll
            for (int j = 0; j < kAttChunk; ++j) {
                const float p = expf(s[j] - m);
                l += p;
                att_axpy<NCH>(acc, p, sV + (j0 + j) * LD, t);
                if (BIAS) att_axpy<NCH>(bacc, bj[j], sV + (j0 + j) * LD, t);
            }
        }
    }

    const float inv = a.K > 0 ? 1.0f / l : 0.0f;
#pragma unroll
    for (int i = 0; i < CP; ++i) acc[i] = BIAS ? fmaf(acc[i], inv, bacc[i]) : acc[i] * inv;
    if (a.stats_w) {
        if (a.oung_w.p) att_store_row<NCH>(acc, a.oung_w, qrow, h, a.c, t, valid);
        if (valid && t == 0) {
            const long i = qrow * a.H + h;
            a.stats_w[i] = m;
            a.stats_w[a.BQH + i] = logf(l);
        }
    }
    if (a.gate.p) {
        att_load_row<NCH>(bacc, a.gate, qrow, h, a.c, t, valid, 1.0f);
#pragma unroll
        for (int i = 0; i < CP; ++i) acc[i] *= 1.0f / (1.0f + expf(-bacc[i]));
    }
    att_store_row<NCH>(acc, a.o, qrow, h, a.c, t, valid);
}

// ---------------------------------------------------------------- backward pre-pass (gate): d_o = g_out sig, g_gate = g_out o_ungated sig (1 - sig)
__global__ void attention_gate_bwd_kernel(const float* __restrict__ gout, long ldgo, const float* __restrict__ gate, long ldg,
                                          const float* __restrict__ oung, long ldou, long rows, int hc, float* __restrict__ d_o,
                                          float* __restrict__ g_gate, long ldgg) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= rows * hc) return;
    const long r = i / hc;
    const int j = (int)(i % hc);
    const float g = gout[r * ldgo + j];
    const float sig = 1.0f / (1.0f + expf(-gate[r * ldg + j]));
    d_o[i] = g * sig;
    g_gate[r * ldgg + j] = g * oung[r * ldou + j] * sig * (1.0f - sig);
}

// ---------------------------------------------------------------- backward, query side: D and g_wq
template <int NCH, bool BIAS>
__global__ __launch_bounds__(kAttThreads) void attention_bwd_q_kernel(AttArgs a) {
    constexpr int CP = 4 * NCH, LD = 4 * CP;
    __shared__ __attribute__((aligned(16))) float sK[kAttTile * LD];
    __shared__ __attribute__((aligned(16))) float sV[kAttTile * LD];
    long b, tile; int h;
    att_block(a, b, h, tile);
    const int t = threadIdx.x & 3;
    const long q = tile * kAttRows + (threadIdx.x >> 2);
    const bool valid = q < a.Q;
    const long qrow = b * a.Q + q;

    float qr[CP], dor[CP], gq[CP];
    att_load_row<NCH>(qr, a.wq, qrow, h, a.c, t, valid, a.scale);
    att_load_row<NCH>(dor, a.dout, qrow, h, a.c, t, valid, 1.0f);
    // p = exp((s - m) - log l): s - m is exact near the maximum and log l is small, so sum_k p stays within a few ulp of 1 also
    // where the logits are large (m + log l would be rounded at the magnitude of m)
    float m = 0.0f, logl = 0.0f;
    if (valid) { m = a.stats[qrow * a.H + h]; logl = a.stats[a.BQH + qrow * a.H + h]; }
    float D = 0.0f, P = 0.0f;
    if (!BIAS) {                                           // no bias: o = sum_k p wv[k], so <d_o, o> = sum_k p dA
        att_load_row<NCH>(gq, a.oung, qrow, h, a.c, t, valid, 1.0f);
#pragma unroll
        for (int i = 0; i < CP; ++i) D = fmaf(dor[i], gq[i], D);
        D = att_quad_sum(D);
    }
#pragma unroll
    for (int i = 0; i < CP; ++i) gq[i] = 0.0f;

    for (int pass = BIAS ? 0 : 1; pass < 2; ++pass) {
        for (long k0 = 0; k0 < a.K; k0 += kAttTile) {
            __syncthreads();
            att_stage<NCH>(sK, a.wk, b * a.K, k0, a.K, h, a.c, 1.0f);
            att_stage<NCH>(sV, a.wv, b * a.K, k0, a.K, h, a.c, 1.0f);
            __syncthreads();
#pragma unroll 1
            for (int j0 = 0; j0 < kAttTile; j0 += kAttChunk) {
                if (k0 + j0 >= a.K) break;
#pragma unroll
                for (int j = 0; j < kAttChunk; ++j) {
                    const float d = att_dot<NCH>(qr, sK + (j0 + j) * LD, t);
                    const float s = k0 + j0 + j < a.K ? d : -INFINITY;
                    const float dA = att_dot<NCH>(dor, sV + (j0 + j) * LD, t);
                    const float p = expf((s - m) - logl);
                    if (pass == 0) { D = fmaf(p, dA, D); P += p; }
                    else att_axpy<NCH>(gq, p * (dA - D), sK + (j0 + j) * LD, t);
                }
            }
        }
        // D is the p-weighted MEAN of dA: dividing by sum_k p (1 up to rounding) makes sum_k dS vanish as it does in exact
        // arithmetic; without it the rounding of sum_k p is multiplied by D sum_k p wk, which need not be small where g_wq is
        if (pass == 0 && a.K > 0) D /= P;
    }
    if (valid && t == 0) a.Dw[qrow * a.H + h] = D;
#pragma unroll
    for (int i = 0; i < CP; ++i) gq[i] *= a.scale;
    att_store_row<NCH>(gq, a.gq, qrow, h, a.c, t, valid);
}

// ---------------------------------------------------------------- backward, key side: g_wk and g_wv
template <int NCH, bool BIAS>
__global__ __launch_bounds__(kAttThreads) void attention_bwd_kv_kernel(AttArgs a) {
    constexpr int CP = 4 * NCH, LD = 4 * CP;
    __shared__ __attribute__((aligned(16))) float sQ[kAttTile * LD];     // scale * wq rows
    __shared__ __attribute__((aligned(16))) float sG[kAttTile * LD];     // d_o rows
    __shared__ float sM[kAttTile], sL[kAttTile], sD[kAttTile];
    long b, tile; int h;
    att_block(a, b, h, tile);
    const int t = threadIdx.x & 3;
    const long k = tile * kAttRows + (threadIdx.x >> 2);
    const bool valid = k < a.K;
    const long krow = b * a.K + k;

    float kr[CP], vr[CP], gk[CP], gv[CP];
    att_load_row<NCH>(kr, a.wk, krow, h, a.c, t, valid, 1.0f);
    att_load_row<NCH>(vr, a.wv, krow, h, a.c, t, valid, 1.0f);
#pragma unroll
    for (int i = 0; i < CP; ++i) { gk[i] = 0.0f; gv[i] = 0.0f; }
    const float* bcol = (BIAS && valid) ? a.bias + b * a.bias_bs + k : nullptr;

    for (long q0 = 0; q0 < a.Q; q0 += kAttTile) {
        __syncthreads();
        att_stage<NCH>(sQ, a.wq, b * a.Q, q0, a.Q, h, a.c, a.scale);
        att_stage<NCH>(sG, a.dout, b * a.Q, q0, a.Q, h, a.c, 1.0f);
        if (threadIdx.x < kAttTile) {
            const long q = q0 + threadIdx.x;
            const long i = (b * a.Q + q) * a.H + h;
            sM[threadIdx.x] = q < a.Q ? a.stats[i] : 0.0f;                  // (rows past Q are not walked)
            sL[threadIdx.x] = q < a.Q ? a.stats[a.BQH + i] : 0.0f;
            sD[threadIdx.x] = q < a.Q ? a.D[i] : 0.0f;
        }
        __syncthreads();
        const int nj = (int)min((long)kAttTile, a.Q - q0);
#pragma unroll 1
        for (int j = 0; j < nj; ++j) {
            const float s = att_dot<NCH>(kr, sQ + j * LD, t);
            const float dA = att_dot<NCH>(vr, sG + j * LD, t);
            const float p = expf((s - sM[j]) - sL[j]);
            float w = p;
            if (BIAS) w += bcol ? bcol[(q0 + j) * a.bias_rs] : 0.0f;
            att_axpy<NCH>(gv, w, sG + j * LD, t);
            att_axpy<NCH>(gk, p * (dA - sD[j]), sQ + j * LD, t);
        }
    }
    att_store_row<NCH>(gk, a.gk, krow, h, a.c, t, valid);
    att_store_row<NCH>(gv, a.gv, krow, h, a.c, t, valid);
}

// ---------------------------------------------------------------- host
static inline int att_vec(const void* p, long ld, int c) { return p == nullptr || ((((uintptr_t)p) & 15) == 0 && (ld & 3) == 0 && (c & 3) == 0); }
static inline AttMat att_mat(const float* p, long ld, int c) { return AttMat{p, ld, att_vec(p, ld, c)}; }
static inline AttOut att_out(float* p, long ld, int c) { return AttOut{p, ld, att_vec(p, ld, c)}; }

enum { ATT_FWD = 0, ATT_BWD_Q = 1, ATT_BWD_KV = 2 };

template <int NCH, bool BIAS>
static void att_launch_one(int which, const AttArgs& a, unsigned grid, hipStream_t st) {
    if (which == ATT_FWD) attention_fwd_kernel<NCH, BIAS><<<grid, kAttThreads, 0, st>>>(a);
    else if (which == ATT_BWD_Q) attention_bwd_q_kernel<NCH, BIAS><<<grid, kAttThreads, 0, st>>>(a);
    else attention_bwd_kv_kernel<NCH, BIAS><<<grid, kAttThreads, 0, st>>>(a);
}

// rows: the owned side's rows per (batch, head)
static int att_launch(int which, AttArgs a, long B, long rows, hipStream_t st) {
    a.tiles = (rows + kAttRows - 1) / kAttRows;
    const long blocks = a.tiles * a.H * B;
    if (blocks <= 0) return KAGNN_OK;
    if (blocks > 0x7fffffffL || a.tiles * a.H > 0x7fffffffL) return fail(KAGNN_ERR_UNSUPPORTED, "%s: shape too large for one launch", "attention");
    const unsigned grid = (unsigned)blocks;
    const bool bias = a.bias != nullptr;
    if (a.c <= 32) { if (bias) att_launch_one<2, true>(which, a, grid, st); else att_launch_one<2, false>(which, a, grid, st); }
    else if (a.c <= 64) { if (bias) att_launch_one<4, true>(which, a, grid, st); else att_launch_one<4, false>(which, a, grid, st); }
    else { if (bias) att_launch_one<8, true>(which, a, grid, st); else att_launch_one<8, false>(which, a, grid, st); }
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

int attention_fwd(const float* wq, long ldq, const float* wk, long ldk, const float* wv, long ldv, const float* bias, long bias_bs,
                  long bias_rs, const float* gate, long ldg, long B, long Q, long K, int H, int c, float scale, float* o, long ldo,
                  float* o_ungated, long ldou, float* stats, hipStream_t st) {
    AttArgs a{};
    a.wq = att_mat(wq, ldq, c); a.wk = att_mat(wk, ldk, c); a.wv = att_mat(wv, ldv, c); a.gate = att_mat(gate, ldg, c);
    a.bias = K > 0 ? bias : nullptr; a.bias_bs = bias_bs; a.bias_rs = bias_rs;
    a.Q = Q; a.K = K; a.H = H; a.c = c; a.scale = scale;
    a.o = att_out(o, ldo, c); a.oung_w = att_out(o_ungated, ldou, c);
    a.stats_w = stats; a.BQH = B * Q * H;
    return att_launch(ATT_FWD, a, B, Q, st);
}

static inline size_t att_align(size_t n) { return (n + 15) & ~(size_t)15; }

// D [B*Q*H] floats, then (with a gate) d_o [B*Q, H*c] floats; nothing proportional to Q*K
size_t attention_bwd_ws_bytes(long B, long Q, long K, int H, int c, int has_gate) {
    (void)K;
    size_t n = att_align((size_t)B * Q * H * sizeof(float));
    if (has_gate) n += att_align((size_t)B * Q * H * c * sizeof(float));
    return n;
}

int attention_bwd(const float* g_out, long ldgo, const float* wq, long ldq, const float* wk, long ldk, const float* wv, long ldv,
                  const float* bias, long bias_bs, long bias_rs, const float* gate, long ldg, const float* o_ungated, long ldou,
                  const float* stats, long B, long Q, long K, int H, int c, float scale, float* g_wq, long ldgq, float* g_wk,
                  long ldgk, float* g_wv, long ldgv, float* g_bias, long gb_bs, long gb_rs, float* g_gate, long ldgg, float* ws,
                  size_t ws_bytes, hipStream_t st) {
    if (ws_bytes < attention_bwd_ws_bytes(B, Q, K, H, c, gate != nullptr)) return fail(KAGNN_ERR_ARG, "%s: workspace too small", "attention_bwd");
    const long hc = (long)H * c;
    float* D = ws;
    const float* d_o = g_out;
    long ldd = ldgo;
    if (gate && B * Q > 0) {
        float* buf = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + att_align((size_t)B * Q * H * sizeof(float)));
        const long n = B * Q * hc;
        const long blocks = (n + 255) / 256;
        if (blocks > 0x7fffffffL) return fail(KAGNN_ERR_UNSUPPORTED, "%s: shape too large for one launch", "attention_bwd");
        attention_gate_bwd_kernel<<<(unsigned)blocks, 256, 0, st>>>(g_out, ldgo, gate, ldg, o_ungated, ldou, B * Q, (int)hc, buf, g_gate, ldgg);
        KAGNN_LAUNCH_CHECK();
        d_o = buf;
        ldd = hc;
    }
    AttArgs a{};
    a.wq = att_mat(wq, ldq, c); a.wk = att_mat(wk, ldk, c); a.wv = att_mat(wv, ldv, c);
    a.oung = att_mat(o_ungated, ldou, c); a.dout = att_mat(d_o, ldd, c);
    a.bias = bias; a.bias_bs = bias_bs; a.bias_rs = bias_rs;
    a.Q = Q; a.K = K; a.H = H; a.c = c; a.scale = scale;
    a.gq = att_out(g_wq, ldgq, c); a.gk = att_out(g_wk, ldgk, c); a.gv = att_out(g_wv, ldgv, c);
    a.stats = stats; a.Dw = D; a.D = D; a.BQH = B * Q * H;
    if (K == 0) a.bias = nullptr;
    int rc = att_launch(ATT_BWD_Q, a, B, Q, st);
    if (rc) return rc;
    if (Q == 0) a.bias = nullptr;
    rc = att_launch(ATT_BWD_KV, a, B, K, st);
    if (rc) return rc;
    if (g_bias && Q > 0 && K > 0) {
        if (hc > 0x7fffffffL) return fail(KAGNN_ERR_UNSUPPORTED, "%s: num_heads * head_dim too large", "attention_bwd");
        for (long b = 0; b < B; ++b) {                 // g_bias[b] = d_o[b] (Q x Hc) wv[b]^T (Hc x K): the heads summed in channel order
            rc = linear_abt(d_o + b * Q * ldd, ldd, Q, (int)hc, wv + b * K * ldv, ldv, K, g_bias + b * gb_bs, gb_rs, st);
            if (rc) return rc;
        }
    }
    return KAGNN_OK;
}

}  // namespace kagnn
