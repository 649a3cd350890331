// Dense layer of the MLP baselines: y = act(x W^T + b) and its two gradients, exact fp32.
//
// Every product runs on the fp32-input matrix instructions (v_mfma_f32_32x32x2_f32, and v_mfma_f32_16x16x4_f32 where one
// side of the product is at most 16 or 33..48 wide), whose result is bit-for-bit an ordered fp32 fma chain.  There is no
// split- or reduced-precision form of these kernels: KAGNN_PRECISION / the `mode` argument of the KAN entry points does not
// reach them, they are exact fp32 in every mode.
//
// Reference behaviour replaced: torch.nn.Linear (+ torch.nn.ReLU) inside the reference's make_mlp chains
// (node_classification_clean/models.py, graph_classification/models.py, graph_regression/models.py) and the `lin` of
// torch_geometric's GCNConv / GATConv, with the autograd backward of those (addmm, threshold_backward).
//
// One LDS-staged tile GEMM  C[M,Nc] = A[M,K] * B[K,Nc]  serves the three products.  A workgroup of four waves owns a
// BM x BN tile of C and walks K in steps of 16: the A and B tiles of a step are fetched with 16-byte loads into registers
// (the next step's loads are in flight under this step's MFMAs), written to LDS k-major ( s[k][row], two buffers: one barrier
// per step ), and every wave reads its fragments from there.  How an operand lies in memory only decides how its tile is fetched:
//   KC (k contiguous)  element (row, k) at p[row*ld + k]   x in the forward, W in the forward, gy in the input gradient
//   KM (k major)       element (row, k) at p[k*ld + row]   W in the input gradient, gy and x in the weight gradient
// A 16-byte load is used where the four elements lie inside the operand and the address is 16-byte aligned (base pointer
// and leading dimension both allow it: a wave-uniform flag from the host); everything else -- edges, odd leading
// dimensions, column slices that start off a 16-byte boundary -- goes element by element with its own bounds check, and
// what lies outside [rows, K] enters the product as 0.  Nothing outside an operand is read, nothing outside [rows, width]
// of a result is written.
//
// LDS rows are BM + 4 (BN + 4) floats: a multiple of 4 (16-byte stores stay aligned) that is 4 mod 16, which makes the
// transposed stores of a KC tile (lanes 4c..4c+3 of a row quad go to rows 4c+i) and the fragment reads (the k-lanes of an MFMA
// read rows 8 apart for 32x32x2, 4 apart for 16x16x4) hit distinct banks.  The k index inside a step is permuted the
// same way for A and B (k-lane q reads k = q*steps + i at MFMA i), which a sum over k does not see.
//
// ReLU backward: m = (y > 0) on the SAVED output (torch's threshold_backward: zero gradient at y == 0); the mask is applied
// to gy while its tile is fetched, so gy (.) m never exists in memory.
//
// Weight gradient: the sum runs over the N rows.  N is cut into slabs of `rows_per_slab` rows (a multiple of 16, at least
// 256), blockIdx.z owns one slab and writes its partial [out][in(+1)] product to the workspace; linear_dw_reduce_kernel adds the
// slabs in index order.  No atomics anywhere: the same inputs give the same bits.  The bias gradient is column `in` of the
// same product: x is read as [x | 1].
#include "common.h"
#include "host.h"

namespace kagnn {

constexpr int kBK = 16;                       // K step of the tile loop
constexpr int kThreads = 256;                 // four waves

struct LinOperand {
    const float* p;        // element (row, k): KC p[row*ld + k], KM p[k*ld + row]
    long ld;
    const float* mask;     // same layout with ldm, or nullptr: the element counts where mask > 0
    long ldm;
    long rows;             // valid rows (the M or the Nc of the product)
    long ones_row;         // KM only: this row is all ones (the bias column of [x | 1]); -1: none
    int vec;               // 16-byte loads allowed (alignment of p, ld, mask, ldm)
};

enum { KC = 0, KM = 1 };

__device__ __forceinline__ float lin_elem(const LinOperand& o, int kind, long row, long k, long kend) {
    if (k >= kend) return 0.0f;
    if (kind == KM && row == o.ones_row) return 1.0f;
    if (row >= o.rows) return 0.0f;
    const long i = kind == KC ? row * o.ld + k : k * o.ld + row;
    float v = o.p[i];
    if (o.mask) {
        const long j = kind == KC ? row * o.ldm + k : k * o.ldm + row;
        v = o.mask[j] > 0.0f ? v : 0.0f;
    }
    return v;
}

// The tile [R rows][16 k] of one operand, R*16/256 floats per thread held in float4 registers between fetch and LDS store.
//   KC: item = (row = idx / 4, k quad = idx % 4)      KM: item = (k = idx / (R/4), row quad = idx % (R/4))
template <int KIND, int R>
struct LinTile {
    static constexpr int kItems = R * 4;                                   // float4 items of the tile
    static constexpr int kPer = (kItems + kThreads - 1) / kThreads;        // per thread
    float4 v[kPer];

    __device__ __forceinline__ void fetch(const LinOperand& o, long row0, long k0, long kend) {
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const int idx = threadIdx.x + u * kThreads;
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            if (kItems % kThreads == 0 || idx < kItems) {
                if (KIND == KC) {
                    const long row = row0 + (idx >> 2), k = k0 + 4 * (idx & 3);
                    if (o.vec && row < o.rows && k + 3 < kend) {
                        t = *reinterpret_cast<const float4*>(o.p + row * o.ld + k);
                        if (o.mask) {
                            const float4 m = *reinterpret_cast<const float4*>(o.mask + row * o.ldm + k);
                            t.x = m.x > 0.f ? t.x : 0.f; t.y = m.y > 0.f ? t.y : 0.f;
                            t.z = m.z > 0.f ? t.z : 0.f; t.w = m.w > 0.f ? t.w : 0.f;
                        }
                    } else {
                        t.x = lin_elem(o, KC, row, k + 0, kend); t.y = lin_elem(o, KC, row, k + 1, kend);
                        t.z = lin_elem(o, KC, row, k + 2, kend); t.w = lin_elem(o, KC, row, k + 3, kend);
                    }
                } else {
                    const long k = k0 + idx / (R / 4), row = row0 + 4 * (idx % (R / 4));
                    if (o.vec && k < kend && row + 3 < o.rows) {
                        t = *reinterpret_cast<const float4*>(o.p + k * o.ld + row);
                        if (o.mask) {
                            const float4 m = *reinterpret_cast<const float4*>(o.mask + k * o.ldm + row);
                            t.x = m.x > 0.f ? t.x : 0.f; t.y = m.y > 0.f ? t.y : 0.f;
                            t.z = m.z > 0.f ? t.z : 0.f; t.w = m.w > 0.f ? t.w : 0.f;
                        }
                    } else {
                        t.x = lin_elem(o, KM, row + 0, k, kend); t.y = lin_elem(o, KM, row + 1, k, kend);
                        t.z = lin_elem(o, KM, row + 2, k, kend); t.w = lin_elem(o, KM, row + 3, k, kend);
                    }
                }
            }
            v[u] = t;
        }
    }

    // s[k][row], row stride LD = R + 4
    __device__ __forceinline__ void store(float* s) const {
        constexpr int LD = R + 4;
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const int idx = threadIdx.x + u * kThreads;
            if (kItems % kThreads == 0 || idx < kItems) {
                if (KIND == KC) {
                    const int row = idx >> 2, k = 4 * (idx & 3);
                    s[(k + 0) * LD + row] = v[u].x; s[(k + 1) * LD + row] = v[u].y;
                    s[(k + 2) * LD + row] = v[u].z; s[(k + 3) * LD + row] = v[u].w;
                } else {
                    const int k = idx / (R / 4), row = 4 * (idx % (R / 4));
                    *reinterpret_cast<float4*>(s + k * LD + row) = v[u];
                }
            }
        }
    }
};

struct LinEpilogue {
    float* c;              // C[row*ldc + col] (one slab of it, for the weight gradient)
    long ldc;
    long slab_stride;      // floats between the partial products of consecutive K slabs (0: no slabs)
    const float* bias;     // per column, or nullptr
    int relu;
};

// T: the MFMA tile (32: 32x32x2, 16: 16x16x4).  The four waves form a WM x WN arrangement, each wave owns MT x NT MFMA tiles:
// BM = WM*MT*T rows, BN = WN*NT*T columns.  grid = (row tiles, column tiles, K slabs).
template <int T, int WM, int WN, int MT, int NT, int KA, int KB>
__global__ __launch_bounds__(kThreads) void linear_gemm_kernel(LinOperand A, LinOperand B, long K, long k_per_slab,
                                                               long M, long Nc, LinEpilogue e) {
    static_assert(WM * WN == 4, "four waves");
    constexpr int BM = WM * MT * T, BN = WN * NT * T, LDA = BM + 4, LDB = BN + 4;
    constexpr int KL = T == 32 ? 2 : 4;            // k-lanes of one MFMA
    constexpr int STEPS = kBK / KL;                // MFMAs per K step and accumulator
    constexpr int AR = T == 32 ? 16 : 4;           // accumulator registers per tile
    __shared__ __attribute__((aligned(16))) float sA[2][kBK * LDA];    // two buffers: the next step is stored while this one is read
    __shared__ __attribute__((aligned(16))) float sB[2][kBK * LDB];

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wm = wave / WN, wn = wave % WN;
    const int r = lane & (T - 1), q = lane / T;
    const long row0 = (long)blockIdx.x * BM, col0 = (long)blockIdx.y * BN;
    const long kbeg = (long)blockIdx.z * k_per_slab, kend = min(K, kbeg + k_per_slab);

    typedef float accv __attribute__((ext_vector_type(AR)));
    accv acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int i = 0; i < AR; ++i) acc[m][n][i] = 0.0f;

    LinTile<KA, BM> ta;
    LinTile<KB, BN> tb;
    if (kbeg < kend) {
        ta.fetch(A, row0, kbeg, kend);
        tb.fetch(B, col0, kbeg, kend);
        ta.store(sA[0]);
        tb.store(sB[0]);
    }
    __syncthreads();
    int cur = 0;
    for (long k0 = kbeg; k0 < kend; k0 += kBK, cur ^= 1) {
        const bool more = k0 + kBK < kend;                  // (block-uniform)
        if (more) { ta.fetch(A, row0, k0 + kBK, kend); tb.fetch(B, col0, k0 + kBK, kend); }
        const float* pa = sA[cur] + (q * STEPS) * LDA + wm * MT * T + r;
        const float* pb = sB[cur] + (q * STEPS) * LDB + wn * NT * T + r;
#pragma unroll
        for (int i = 0; i < STEPS; ++i) {
            float a[MT], b[NT];
#pragma unroll
            for (int m = 0; m < MT; ++m) a[m] = pa[i * LDA + m * T];
#pragma unroll
            for (int n = 0; n < NT; ++n) b[n] = pb[i * LDB + n * T];
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    if constexpr (T == 32) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], b[n], acc[m][n], 0, 0, 0);
                    else acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], b[n], acc[m][n], 0, 0, 0);
                }
        }
        // the other buffer's last readers passed the barrier that ended the previous step
        if (more) { ta.store(sA[cur ^ 1]); tb.store(sB[cur ^ 1]); }
        __syncthreads();
    }

    float* c = e.c + (long)blockIdx.z * e.slab_stride;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const long col = col0 + (wn * NT + n) * T + r;
        if (col >= Nc) continue;
        const float bv = e.bias ? e.bias[col] : 0.0f;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
#pragma unroll
            for (int i = 0; i < AR; ++i) {
                const long row = row0 + (wm * MT + m) * T + (T == 32 ? mfma32_row(i, q) : 4 * q + i);
                if (row < M) {
                    float v = acc[m][n][i] + bv;
                    if (e.relu) v = v > 0.0f ? v : 0.0f;
                    c[row * e.ldc + col] = v;
                }
            }
        }
    }
}

// gW[o][f] = sum_s slab[s][o][f], gb[o] = sum_s slab[s][o][in]  (f < in; slabs added in index order)
__global__ void linear_dw_reduce_kernel(const float* __restrict__ slab, long S, int in, int out, int cols,
                                        float* __restrict__ gW, float* __restrict__ gb) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const long per = (long)out * cols;
    if (i >= per) return;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    long s = 0;
    for (; s + 4 <= S; s += 4) {
        a0 += slab[(s + 0) * per + i];
        a1 += slab[(s + 1) * per + i];
        a2 += slab[(s + 2) * per + i];
        a3 += slab[(s + 3) * per + i];
    }
    for (; s < S; ++s) a0 += slab[s * per + i];
    const float v = (a0 + a1) + (a2 + a3);
    const int o = (int)(i / cols), f = (int)(i % cols);
    if (f < in) gW[(long)o * in + f] = v;
    else gb[o] = v;
}

static inline int vec_ok(const float* p, long ld) { return p == nullptr || (((uintptr_t)p & 15) == 0 && (ld & 3) == 0); }

template <int T, int WM, int WN, int MT, int NT, int KA, int KB>
static int launch_gemm(const LinOperand& A, const LinOperand& B, long K, long k_per_slab, long slabs, long M, long Nc,
                const LinEpilogue& e, hipStream_t st) {
    constexpr int BM = WM * MT * T, BN = WN * NT * T;
    const long gx = (M + BM - 1) / BM, gy = (Nc + BN - 1) / BN;
    if (gx > 0x7fffffffL || gy > 65535 || slabs > 65535) return fail(KAGNN_ERR_UNSUPPORTED, "%s: shape too large for one launch", "linear");
    dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)slabs);
    linear_gemm_kernel<T, WM, WN, MT, NT, KA, KB><<<grid, kThreads, 0, st>>>(A, B, K, k_per_slab, M, Nc, e);
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

// rows x Nc product with the rows on the long side (forward, input gradient): 128 rows per workgroup, the column tile by Nc
template <int KB>
static int launch_tall(const LinOperand& A, const LinOperand& B, long K, long M, long Nc, const LinEpilogue& e, hipStream_t st) {
    if (Nc <= 16) return launch_gemm<16, 4, 1, 2, 1, KC, KB>(A, B, K, K, 1, M, Nc, e, st);
    if (Nc <= 32) return launch_gemm<32, 4, 1, 1, 1, KC, KB>(A, B, K, K, 1, M, Nc, e, st);
    if (Nc <= 48) return launch_gemm<16, 4, 1, 2, 3, KC, KB>(A, B, K, K, 1, M, Nc, e, st);
    if (Nc <= 64) return launch_gemm<32, 4, 1, 1, 2, KC, KB>(A, B, K, K, 1, M, Nc, e, st);
    return launch_gemm<32, 2, 2, 2, 2, KC, KB>(A, B, K, K, 1, M, Nc, e, st);      // 128 x 128: every fragment read feeds two MFMAs
}

int linear_fwd(const float* x, long ldx, long N, int in, const float* W, const float* bias, int out, int relu,
               float* y, long ldy, hipStream_t st) {
    const LinOperand A{x, ldx, nullptr, 0, N, -1, vec_ok(x, ldx)};
    const LinOperand B{W, in, nullptr, 0, out, -1, vec_ok(W, in)};
    const LinEpilogue e{y, ldy, 0, bias, relu};
    return launch_tall<KC>(A, B, in, N, out, e, st);
}

int linear_abt(const float* a, long lda, long M, int K, const float* b, long ldb, long Nc, float* c, long ldc, hipStream_t st) {
    const LinOperand A{a, lda, nullptr, 0, M, -1, vec_ok(a, lda)};
    const LinOperand B{b, ldb, nullptr, 0, Nc, -1, vec_ok(b, ldb)};
    const LinEpilogue e{c, ldc, 0, nullptr, 0};
    return launch_tall<KC>(A, B, K, M, Nc, e, st);
}

int linear_dx(const float* gy, long ldgy, const float* y, long ldy, long N, int out, const float* W, int in,
              float* gx, long ldgx, hipStream_t st) {
    const LinOperand A{gy, ldgy, y, ldy, N, -1, vec_ok(gy, ldgy) && vec_ok(y, ldy)};
    const LinOperand B{W, in, nullptr, 0, in, -1, vec_ok(W, in)};
    const LinEpilogue e{gx, ldgx, 0, nullptr, 0};
    return launch_tall<KM>(A, B, out, N, in, e, st);
}

// rows (outputs) of the weight gradient's workgroup tile; 128 columns (inputs) in every form
static int linear_dw_tile_rows(int out) { return out <= 16 ? 16 : out <= 32 ? 32 : out <= 64 ? 64 : 128; }

// slabs of the weight gradient: about 512 workgroups in all, a slab never shorter than 256 rows
void linear_dw_plan(long N, int in, int out, long* slabs, long* rows_per_slab) {
    const long tiles = (long)cdiv(in + 1, 128) * cdiv(out, linear_dw_tile_rows(out));
    const long want = max(1L, 512 / tiles);
    long r = (N + want - 1) / want;
    r = max(256L, (r + kBK - 1) / kBK * kBK);
    *rows_per_slab = r;
    *slabs = max(1L, (N + r - 1) / r);
}

size_t linear_dw_ws_bytes(long N, int in, int out) {
    long S, r;
    linear_dw_plan(N, in, out, &S, &r);
    return (size_t)S * out * (in + 1) * sizeof(float);
}

int linear_dw(const float* x, long ldx, const float* gy, long ldgy, const float* y, long ldy, long N, int in, int out,
              float* gW, float* gb, float* ws, size_t ws_bytes, hipStream_t st) {
    if (ws_bytes < linear_dw_ws_bytes(N, in, out)) return fail(KAGNN_ERR_ARG, "%s: workspace too small", "linear_dw");
    long S, r;
    linear_dw_plan(N, in, out, &S, &r);
    const int cols = in + (gb ? 1 : 0);
    const LinOperand A{gy, ldgy, y, ldy, out, -1, vec_ok(gy, ldgy) && vec_ok(y, ldy)};
    const LinOperand B{x, ldx, nullptr, 0, in, gb ? (long)in : -1L, vec_ok(x, ldx)};
    const LinEpilogue e{ws, cols, (long)out * cols, nullptr, 0};
    const int tr = linear_dw_tile_rows(out);
    int rc = tr == 16 ? launch_gemm<16, 1, 4, 1, 2, KM, KM>(A, B, N, r, S, out, cols, e, st)
           : tr == 32 ? launch_gemm<32, 1, 4, 1, 1, KM, KM>(A, B, N, r, S, out, cols, e, st)
           : tr == 64 ? launch_gemm<32, 1, 4, 2, 1, KM, KM>(A, B, N, r, S, out, cols, e, st)
                      : launch_gemm<32, 2, 2, 2, 2, KM, KM>(A, B, N, r, S, out, cols, e, st);
    if (rc) return rc;
    const long per = (long)out * cols;
    linear_dw_reduce_kernel<<<cdiv(per, 256), 256, 0, st>>>(ws, S, in, out, cols, gW, gb);
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

}  // namespace kagnn
