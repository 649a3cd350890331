// What the reference's graph-classification scripts wrap around their models (graph_classification/graph_classification_utils.py):
// the `Degree` node-feature transform of the unlabeled TU datasets (:31-36), and the loss / accuracy bookkeeping of its train, val
// and test loops (:45-72: F.nll_loss per batch, `reduction='sum'` for validation, `max(1)[1].eq(y).sum()` for the accuracy), each of
// which ends in an `.item()` per batch.  Here the loss of a mini-batch is ONE launch that also keeps the epoch's running figures
// in a 24-byte device record, so a loop reads back once per epoch.
#include "common.h"
#include "host.h"

namespace kagnn {

// ------------------------------------------------------------------ x = one_hot(clip(degree(edge_index[0]), 0, K - 1), K).float()
// deg(v) = rowptr[v + 1] - rowptr[v] of the CSR grouped by SOURCE (torch_geometric.utils.degree(edge_index[0]) counts sources);
// rowptr == nullptr: a dataset without edges, every degree is 0.  Every element of every row is written (no memset before, no
// atomics).  VEC: ldx == K and a 16-byte aligned base -- the [N, K] block is one flat array, four elements per thread and one
// 16-byte store; else one element per thread, consecutive threads on consecutive columns of a row.
template <bool VEC>
__global__ __launch_bounds__(256) void degree_one_hot_kernel(const int* __restrict__ rowptr, long N, int K, float* __restrict__ x,
                                                             long ldx) {
    const long total = N * K;
    if (VEC) {
        const long i0 = (blockIdx.x * 256L + threadIdx.x) * 4;
        if (i0 >= total) return;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long e = min(i0 + j, total - 1), r = e / K;
            const int c = (int)(e - r * K);
            const int d = rowptr ? min(rowptr[r + 1] - rowptr[r], K - 1) : 0;
            v[j] = c == d ? 1.0f : 0.0f;
        }
        if (i0 + 3 < total) {
            *reinterpret_cast<f32x4*>(x + i0) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
            for (int j = 0; i0 + j < total; ++j) x[i0 + j] = v[j];
        }
    } else {
        const long e = blockIdx.x * 256L + threadIdx.x;
        if (e >= total) return;
        const long r = e / K;
        const int c = (int)(e - r * K);
        const int d = rowptr ? min(rowptr[r + 1] - rowptr[r], K - 1) : 0;
        x[r * ldx + c] = c == d ? 1.0f : 0.0f;
    }
}

int degree_one_hot(const int* rowptr, long N, int K, float* x, long ldx, hipStream_t st) {
    if (N == 0) return KAGNN_OK;
    const long total = N * K;
    if (ldx == K && ((uintptr_t)x & 15) == 0) {
        degree_one_hot_kernel<true><<<cdiv(total, 1024), 256, 0, st>>>(rowptr, N, K, x, ldx);
    } else {
        degree_one_hot_kernel<false><<<cdiv(total, 256), 256, 0, st>>>(rowptr, N, K, x, ldx);
    }
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

// ------------------------------------------------------------------ F.nll_loss(logp, y) of a mini-batch, both reductions at once,
// plus the number of rows whose arg-max is the label.  ONE workgroup of 1024 threads (a mini-batch is at most
// KAGNN_BATCH_MAX_GRAPHS rows; more rows just loop).  W = the power of two >= classes, capped at 64, lanes share a row: each scans
// its columns l, l + W, ... for the row's maximum (first index wins inside a lane), the W candidates fold by xor shuffles with
// ties to the LOWER index, and a NaN anywhere in the row marks it as never correct.  The first lane of the group reads
// -logp[r, y[r]] and adds it IN DOUBLE (the addends are fp32 values, so the only rounding of the sum is fp64's); the 1024 partial
// sums fold pairwise through LDS in a fixed order.  Thread 0 writes sum / rows and sum, each rounded once to fp32, and -- when
// there is a record -- adds to {double nll_sum; int64 correct; int64 graphs} with plain loads and stores: launches on one stream
// are ordered, so the record needs no atomics and is deterministic.  A label outside [0, classes): both losses (and nll_sum) are
// NaN, *flag is set (never cleared here), the row counts as wrong.
struct ClassifyRecord { double nll_sum; long long correct; long long graphs; };

__global__ __launch_bounds__(1024) void nll_loss_fwd_kernel(const float* __restrict__ logp, long ld, long rows, int C,
                                                            const long* __restrict__ y, float* __restrict__ loss_mean,
                                                            float* __restrict__ loss_sum, ClassifyRecord* __restrict__ rec,
                                                            int* __restrict__ flag, int W, int want_correct) {
    __shared__ double s_a[1024];
    __shared__ int s_c[1024], s_bad[1024];
    const int l = threadIdx.x & (W - 1), g = threadIdx.x / W, G = 1024 / W;
    double a = 0.0;
    int correct = 0, bad = 0;
    for (long base = 0; base < rows; base += G) {              // (uniform trip count: every lane takes part in the shuffles)
        const long row = base + g, r = min(row, rows - 1);
        const float* zr = logp + r * ld;
        const long yv = y[r];
        const bool label_ok = yv >= 0 && yv < C;
        if (want_correct) {
            float best = -INFINITY;
            int idx = 0x7fffffff, nan = 0;
            for (int c = l; c < C; c += W) {
                const float v = zr[c];
                nan |= v != v;
                if (idx == 0x7fffffff || v > best) { best = v; idx = c; }
            }
            for (int o = W >> 1; o >= 1; o >>= 1) {
                const float ob = __shfl_xor(best, o);
                const int oi = __shfl_xor(idx, o);
                nan |= __shfl_xor(nan, o);
                if (oi != 0x7fffffff && (idx == 0x7fffffff || ob > best || (ob == best && oi < idx))) { best = ob; idx = oi; }
            }
            if (l == 0 && row < rows && label_ok && !nan && (long)idx == yv) ++correct;
        }
        if (l == 0 && row < rows) {
            if (label_ok) a -= (double)zr[yv];
            else bad = 1;
        }
    }
    s_a[threadIdx.x] = a; s_c[threadIdx.x] = correct; s_bad[threadIdx.x] = bad;
    __syncthreads();
    for (int w = 512; w >= 1; w >>= 1) {                        // fixed tree => deterministic
        if ((int)threadIdx.x < w) {
            s_a[threadIdx.x] += s_a[threadIdx.x + w];
            s_c[threadIdx.x] += s_c[threadIdx.x + w];
            s_bad[threadIdx.x] |= s_bad[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double sum = s_bad[0] ? (double)__builtin_nanf("") : s_a[0];
        if (loss_mean) loss_mean[0] = (float)(sum / (double)rows);        // no rows: 0 / 0 = NaN, as torch's mean
        if (loss_sum) loss_sum[0] = (float)sum;
        if (s_bad[0] && flag) flag[0] = 1;
        if (rec) {
            rec->nll_sum = rec->nll_sum + sum;
            rec->correct = rec->correct + s_c[0];
            rec->graphs = rec->graphs + rows;
        }
    }
}

int nll_loss_fwd(const float* logp, long ld, long rows, int C, const long* y, float* loss_mean, float* loss_sum, void* accum,
                 int* flag, hipStream_t st) {
    int W = 1;
    while (W < C && W < 64) W <<= 1;
    nll_loss_fwd_kernel<<<1, 1024, 0, st>>>(logp, ld, rows, C, y, loss_mean, loss_sum, (ClassifyRecord*)accum, flag, W,
                                            accum != nullptr);
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

// backward: g_logp[r, c] = -(g_loss / rows) (mean) or -g_loss (sum) at c == y[r], exactly 0 elsewhere; the whole [rows, classes]
// block in one launch (rows with a label outside [0, classes) are all zero)
__global__ __launch_bounds__(256) void nll_loss_bwd_kernel(const long* __restrict__ y, long rows, int C,
                                                           const float* __restrict__ g_loss, int mean, float* __restrict__ g_logp,
                                                           long ldg) {
    const long e = blockIdx.x * 256L + threadIdx.x;
    if (e >= rows * C) return;
    const long r = e / C;
    const int c = (int)(e - r * C);
    const float g = mean ? g_loss[0] / (float)rows : g_loss[0];
    g_logp[r * ldg + c] = (long)c == y[r] ? -g : 0.0f;
}

int nll_loss_bwd(const long* y, long rows, int C, const float* g_loss, int reduction, float* g_logp, long ldg, hipStream_t st) {
    if (rows == 0) return KAGNN_OK;
    nll_loss_bwd_kernel<<<cdiv(rows * C, 256), 256, 0, st>>>(y, rows, C, g_loss, reduction == KAGNN_REDUCTION_MEAN, g_logp, ldg);
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

}  // namespace kagnn
