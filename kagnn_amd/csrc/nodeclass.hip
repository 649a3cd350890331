// What the reference's node-classification experiment does after the logits (node_classification_clean/utils.py: train_total,
// EarlyStopper).  Per epoch the script takes a CrossEntropyLoss over the validation mask, on print epochs three arg-max accuracies
// through boolean indexing (a read-back each), compares `val_loss < min` on the host and saves a whole state_dict on every
// improvement.  Here the same figures are ONE pass over the [N, C] logits for all splits at once (kagnn_node_eval), the stopper is
// a 32-byte device record updated by one tiny launch (kagnn_early_stop_update), and the best-weights save is a copy predicated on
// a device word (kagnn_copy_if) -- a loop built from them never has to read anything back.
#include "common.h"
#include "host.h"

namespace kagnn {

struct NodeEvalRecord { double xent_sum; long long correct; long long rows; };
constexpr int kNodeEvalMaxSplits = 8;
constexpr int kNodeEvalMaxBlocks = 1024;

// ------------------------------------------------------------------ per split: sum of logsumexp(z) - z[y], correct arg-max rows, rows
// W = the power of two >= C (capped at 64) lanes share a row, 256 / W rows per workgroup and trip: a wave's loads cover 64 / W
// consecutive rows of W (<= C rounded up) consecutive floats.  The group first reads the row's byte of split bits; a row in no
// split (of the first S) issues no other load -- the loads are predicated, not branched around, so every lane takes part in the
// shuffles.  Row term in fp32, max-subtracted; arg-max as kagnn_nll_loss_fwd (first index inside a lane, ties to the LOWER index
// across lanes, a NaN anywhere: never correct -- and the row term is NaN).  Lane 0 of the group adds the term IN DOUBLE to each of
// the row's splits; the 256 per-thread sums fold through LDS in a fixed tree, and the workgroup writes S records: to `out`
// directly when the grid is one workgroup, else to its slot of the workspace, which node_eval_finish_kernel sums in index order.
// A label outside [0, C): the term is NaN, the row counts as wrong, *flag is set (never cleared here); z[.., y] is not read.
template <int W>
__global__ __launch_bounds__(256) void node_eval_kernel(const float* __restrict__ z, long ld, long N, int C,
                                                        const long* __restrict__ y, const unsigned char* __restrict__ bits, int S,
                                                        NodeEvalRecord* __restrict__ out, int* __restrict__ flag) {
    constexpr int G = 256 / W;
    __shared__ double s_a[256];
    __shared__ int s_c[256], s_r[256];
    const int l = threadIdx.x & (W - 1), g = threadIdx.x / W;
    const unsigned smask = (1u << S) - 1u;
    double acc[kNodeEvalMaxSplits];
    int correct[kNodeEvalMaxSplits], rows[kNodeEvalMaxSplits];
#pragma unroll
    for (int s = 0; s < kNodeEvalMaxSplits; ++s) { acc[s] = 0.0; correct[s] = 0; rows[s] = 0; }
    for (long base = (long)blockIdx.x * G; base < N; base += (long)gridDim.x * G) {      // (uniform trip count per workgroup)
        const long row = base + g, r = min(row, N - 1);
        const unsigned b = row < N ? (bits[r] & smask) : 0u;
        const bool on = b != 0u;
        const float* zr = z + r * ld;
        const long yv = on ? y[r] : 0;
        const bool label_ok = yv >= 0 && yv < C;
        float best = (on && l < C) ? zr[l] : -INFINITY;
        const float v0 = best;
        int idx = l < C ? l : 0x7fffffff, nan = best != best;
        for (int c = l + W; c < C; c += W) {
            const float v = on ? zr[c] : -INFINITY;
            nan |= v != v;
            if (v > best) { best = v; idx = c; }
        }
#pragma unroll
        for (int o = W >> 1; o >= 1; o >>= 1) {
            const float ob = __shfl_xor(best, o);
            const int oi = __shfl_xor(idx, o);
            nan |= __shfl_xor(nan, o);
            if (oi != 0x7fffffff && (idx == 0x7fffffff || ob > best || (ob == best && oi < idx))) { best = ob; idx = oi; }
        }
        float e = l < C ? expf(v0 - best) : 0.0f;                                        // best = the row's maximum
        for (int c = l + W; c < C; c += W) e += expf((on ? zr[c] : -INFINITY) - best);
#pragma unroll
        for (int o = W >> 1; o >= 1; o >>= 1) e += __shfl_xor(e, o);
        if (l == 0 && on) {
            const float zy = zr[label_ok ? yv : 0];
            float term = (best - zy) + logf(e);
            if (!label_ok || nan) term = __builtin_nanf("");
            if (!label_ok) flag[0] = 1;
            const int ok = label_ok && !nan && (long)idx == yv;
#pragma unroll
            for (int s = 0; s < kNodeEvalMaxSplits; ++s) {
                if ((b >> s) & 1u) { acc[s] += (double)term; correct[s] += ok; rows[s] += 1; }
            }
        }
    }
    NodeEvalRecord* dst = out + (long)blockIdx.x * S;
#pragma unroll
    for (int s = 0; s < kNodeEvalMaxSplits; ++s) {
        if (s >= S) break;
        __syncthreads();
        s_a[threadIdx.x] = acc[s]; s_c[threadIdx.x] = correct[s]; s_r[threadIdx.x] = rows[s];
        __syncthreads();
        for (int w = 128; w >= 1; w >>= 1) {                    // fixed tree => deterministic
            if ((int)threadIdx.x < w) {
                s_a[threadIdx.x] += s_a[threadIdx.x + w];
                s_c[threadIdx.x] += s_c[threadIdx.x + w];
                s_r[threadIdx.x] += s_r[threadIdx.x + w];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) { dst[s].xent_sum = s_a[0]; dst[s].correct = s_c[0]; dst[s].rows = s_r[0]; }
    }
}

// one workgroup: thread t adds the partials of workgroups t, t + 256, ... in that order, then the fixed tree
__global__ __launch_bounds__(256) void node_eval_finish_kernel(const NodeEvalRecord* __restrict__ partial, int nb, int S,
                                                               NodeEvalRecord* __restrict__ out) {
    __shared__ double s_a[256];
    __shared__ long long s_c[256], s_r[256];
    for (int s = 0; s < S; ++s) {
        double a = 0.0;
        long long c = 0, r = 0;
        for (int b = threadIdx.x; b < nb; b += 256) {
            const NodeEvalRecord p = partial[(long)b * S + s];
            a += p.xent_sum; c += p.correct; r += p.rows;
        }
        __syncthreads();
        s_a[threadIdx.x] = a; s_c[threadIdx.x] = c; s_r[threadIdx.x] = r;
        __syncthreads();
        for (int w = 128; w >= 1; w >>= 1) {
            if ((int)threadIdx.x < w) {
                s_a[threadIdx.x] += s_a[threadIdx.x + w];
                s_c[threadIdx.x] += s_c[threadIdx.x + w];
                s_r[threadIdx.x] += s_r[threadIdx.x + w];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) { out[s].xent_sum = s_a[0]; out[s].correct = s_c[0]; out[s].rows = s_r[0]; }
    }
}

static int node_eval_width(int C) {
    int W = 1;
    while (W < C && W < 64) W <<= 1;
    return W;
}

// workgroups of the first stage: one per 256 / W rows, at most kNodeEvalMaxBlocks (more rows: more trips)
static int node_eval_blocks(long N, int C) {
    const long per = 256 / node_eval_width(C);
    return (int)max(1L, min((long)kNodeEvalMaxBlocks, (N + per - 1) / per));
}

size_t node_eval_ws_bytes(long N, int C, int S) {
    const int nb = node_eval_blocks(N, C);
    return nb > 1 ? (size_t)nb * S * sizeof(NodeEvalRecord) : 0;
}

int node_eval(const float* z, long ld, long N, int C, const long* y, const unsigned char* bits, int S, void* records, int* flag,
              void* ws, size_t ws_bytes, hipStream_t st) {
    const int nb = node_eval_blocks(N, C);
    if (nb > 1 && (ws == nullptr || ws_bytes < node_eval_ws_bytes(N, C, S) || ((uintptr_t)ws & 7) != 0))
        return fail(KAGNN_ERR_ARG, "%s: the workspace is missing, smaller than kagnn_node_eval_workspace_bytes says or not 8-byte aligned",
                    "kagnn_node_eval");
    NodeEvalRecord* first = nb > 1 ? (NodeEvalRecord*)ws : (NodeEvalRecord*)records;
    switch (node_eval_width(C)) {
#define KAGNN_NODE_EVAL(W_) case W_: node_eval_kernel<W_><<<nb, 256, 0, st>>>(z, ld, N, C, y, bits, S, first, flag); break;
        KAGNN_NODE_EVAL(1) KAGNN_NODE_EVAL(2) KAGNN_NODE_EVAL(4) KAGNN_NODE_EVAL(8) KAGNN_NODE_EVAL(16) KAGNN_NODE_EVAL(32)
        default: node_eval_kernel<64><<<nb, 256, 0, st>>>(z, ld, N, C, y, bits, S, first, flag); break;
#undef KAGNN_NODE_EVAL
    }
    KAGNN_LAUNCH_CHECK();
    if (nb > 1) {
        node_eval_finish_kernel<<<1, 256, 0, st>>>(first, nb, S, (NodeEvalRecord*)records);
        KAGNN_LAUNCH_CHECK();
    }
    return KAGNN_OK;
}

// ------------------------------------------------------------------ EarlyStopper(patience, min_delta) as a device record
// One workgroup of 64.  Every thread reads `stopped` and `epochs` BEFORE the barrier; after it the threads copy this epoch's eval
// records into history[epochs] (8-byte words) while thread 0 applies the reference's rule to the validation split's mean, rounded
// once to fp32, with fp32 comparisons (the script compares fp32 tensors):
//   v < min: min = v, counter = 0, improved;  else v >= min + min_delta: ++counter, stopped once counter >= patience;
//   anything else (v inside [min, min + min_delta), or NaN -- rows == 0 gives 0 / 0): nothing.
// Stopped, or max_epochs epochs counted: improved = 0 and nothing else is written.
struct EarlyStopState { float min_loss, min_delta; int patience, counter, epochs, best_epoch, improved, stopped; };

__global__ __launch_bounds__(64) void early_stop_update_kernel(const NodeEvalRecord* __restrict__ rec, int S, int val_split,
                                                               EarlyStopState* __restrict__ st, NodeEvalRecord* __restrict__ history,
                                                               int max_epochs) {
    const int stopped = st->stopped, epochs = st->epochs;
    __syncthreads();
    if (stopped || epochs >= max_epochs) {
        if (threadIdx.x == 0) st->improved = 0;
        return;
    }
    if (history) {
        const long long* src = reinterpret_cast<const long long*>(rec);
        long long* dst = reinterpret_cast<long long*>(history + (long)epochs * S);
        for (int i = threadIdx.x; i < 3 * S; i += 64) dst[i] = src[i];
    }
    if (threadIdx.x == 0) {
        const NodeEvalRecord r = rec[val_split];
        const float v = (float)(r.xent_sum / (double)r.rows);
        const float lo = st->min_loss;
        int improved = 0;
        if (v < lo) {
            st->min_loss = v; st->counter = 0; st->best_epoch = epochs;
            improved = 1;
        } else if (v >= lo + st->min_delta) {
            const int c = st->counter + 1;
            st->counter = c;
            if (c >= st->patience) st->stopped = 1;
        }
        st->improved = improved;
        st->epochs = epochs + 1;
    }
}

int early_stop_update(const void* records, int S, int val_split, void* state, void* history, int max_epochs, hipStream_t st) {
    early_stop_update_kernel<<<1, 64, 0, st>>>((const NodeEvalRecord*)records, S, val_split, (EarlyStopState*)state,
                                               (NodeEvalRecord*)history, max_epochs);
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

// ------------------------------------------------------------------ dst[k] = src[k] for every tensor k, if *flag != 0
// The best-weights snapshot: parameters AND buffers as bytes (running statistics, num_batches_tracked, grids), 32 tensors per
// launch through pointer tables in the kernel arguments (as kagnn_adam_step).  A tensor whose two pointers are 16-byte aligned
// moves as 16-byte vectors with a tail of 4-byte words; any other as 4-byte words.  *flag == 0: no store at all.
constexpr int kCopyBatch = 32;
struct CopyBatch { void* dst[kCopyBatch]; const void* src[kCopyBatch]; long bytes[kCopyBatch]; };

__global__ __launch_bounds__(256) void copy_if_kernel(const int* __restrict__ flag, const CopyBatch b) {
    if (flag[0] == 0) return;
    const int k = blockIdx.y;
    const long words = b.bytes[k] >> 2;
    const long t = blockIdx.x * 256L + threadIdx.x, stride = (long)gridDim.x * 256;
    long done = 0;
    if ((((uintptr_t)b.dst[k] | (uintptr_t)b.src[k]) & 15) == 0) {
        const u32x4* __restrict__ s = static_cast<const u32x4*>(b.src[k]);
        u32x4* __restrict__ d = static_cast<u32x4*>(b.dst[k]);
        const long vecs = words >> 2;
        for (long i = t; i < vecs; i += stride) d[i] = s[i];
        done = vecs << 2;
    }
    const unsigned* __restrict__ s = static_cast<const unsigned*>(b.src[k]);
    unsigned* __restrict__ d = static_cast<unsigned*>(b.dst[k]);
    for (long i = done + t; i < words; i += stride) d[i] = s[i];
}

int copy_if(const int* flag, int count, void* const* dst, const void* const* src, const long* bytes, hipStream_t st) {
    for (int k0 = 0; k0 < count; k0 += kCopyBatch) {
        CopyBatch b{};
        const int nb = min(kCopyBatch, count - k0);
        long bmax = 0;
        for (int k = 0; k < nb; ++k) {
            b.dst[k] = dst[k0 + k]; b.src[k] = src[k0 + k]; b.bytes[k] = bytes[k0 + k];
            bmax = max(bmax, b.bytes[k]);
        }
        const unsigned gx = (unsigned)max(1L, min((long)cdiv(bmax, 256L * 16 * 4), 256L));
        copy_if_kernel<<<dim3(gx, (unsigned)nb), 256, 0, st>>>(flag, b);
        KAGNN_LAUNCH_CHECK();
    }
    return KAGNN_OK;
}

}  // namespace kagnn
