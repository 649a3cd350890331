// Link prediction around an encoder (kagnn_edge_keys_build, kagnn_negative_sample, kagnn_bce_logits_fwd / _bwd, kagnn_link_rank:
// include/kagnn_hip.h).  torch_geometric's recipe -- negative_sampling, a dot-product decoder, BCEWithLogitsLoss, ROC-AUC -- has its
// float part in the library already: the pair score <z[u], z[v]> is kagnn_aggregate_edge_grad over the pair list and its gradient
// two weighted aggregations.  What is here is the integer and statistical rest:
//   edge keys      the edge set as the ascending, duplicate-free 64-bit keys src * N + dst (rocPRIM radix sort + unique), built once
//                  per graph; membership is a binary search;
//   negatives      slot p draws up to T pairs from the counter-based key32 (common.h) and keeps the first that is neither a self
//                  pair nor an edge: a fixed-size output, no compaction, no read-back, a pure function of (seed, keys, N, T);
//   binary loss    the weighted mean of max(s, 0) - s y + log1p(exp(-|s|)) with fp64 partial sums in a fixed order, and in the same
//                  call the meter row of kagnn_node_eval's format (loss sum, rows with (s > 0) == y, rows);
//   ranking        2U of the Mann-Whitney statistic (ROC-AUC = 2U / (2 n_pos n_neg)) and hits@k, exact in int64: scores become
//                  order-preserving 32-bit keys (-0.0 = +0.0, NaN and weight-0 rows behind everything), one radix sort with the
//                  label as value, an exclusive scan of the negatives, and per positive two binary searches for its tie group.
// No float atomics anywhere; the integer sums of the ranking are atomic adds, whose order does not matter.
#include "common.h"
#include "host.h"
#include <rocprim/rocprim.hpp>

namespace kagnn {

constexpr int kLpThreads = 256;

static size_t lp_align(size_t x) { return (x + 255) & ~(size_t)255; }
// Temporary storage of a rocPRIM sort / scan / unique over n items of item_bytes, bounded on the host (the size queries need a
// device; the *_workspace_bytes entry points do not): the second buffer of an out-of-place radix sort is n items, the look-back
// state of the single-pass primitives a few bytes per BLOCK of some thousand items.  Twice the items plus 8 bytes per item plus
// 1 MiB; every primitive checks rocPRIM's real figure against what it was given before it runs.
static size_t lp_temp_bound(long n, size_t item_bytes) { return lp_align(2 * (size_t)n * item_bytes + 8 * (size_t)n + ((size_t)1 << 20)); }

static int lp_temp_check(const char* fn, size_t need, size_t have) {
    if (need > have) return fail(KAGNN_ERR_UNSUPPORTED, "%s: rocPRIM needs %ld bytes of temporary storage, the workspace holds %ld", fn, (long)need, (long)have);
    return KAGNN_OK;
}

// ------------------------------------------------------------------------------------------------- edge keys
// ids outside [0, N) are clamped to 0 (GraphIndex has validated the same edge list; nothing here reads through an id)
__global__ void lp_edge_key_kernel(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, long E, long N,
                                   unsigned long long* __restrict__ key) {
    const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (e >= E) return;
    int64_t u = src[e], v = dst[e];
    u = (u < 0 || u >= N) ? 0 : u;
    v = (v < 0 || v >= N) ? 0 : v;
    key[e] = (unsigned long long)u * (unsigned long long)N + (unsigned long long)v;
}

struct EdgeKeysWorkspace { unsigned long long* raw; unsigned long long* sorted; void* tmp; size_t tmp_bytes; size_t total; };

static void edge_keys_workspace(long E, void* ws, EdgeKeysWorkspace* w) {
    char* p = static_cast<char*>(ws);
    const size_t kb = lp_align((size_t)E * 8);
    w->raw = reinterpret_cast<unsigned long long*>(p); p += kb;
    w->sorted = reinterpret_cast<unsigned long long*>(p); p += kb;
    w->tmp = p;
    w->tmp_bytes = lp_temp_bound(E, 8);
    w->total = 2 * kb + w->tmp_bytes + 256;
}

size_t edge_keys_ws_bytes(long E) {
    EdgeKeysWorkspace w;
    edge_keys_workspace(E, nullptr, &w);
    return w.total;
}

static int lp_key_bits(long N) {                                   // keys < N * N
    int b = 1;
    while (b < 62 && (1ULL << b) < (unsigned long long)N * (unsigned long long)N) ++b;
    return b;
}

int edge_keys_build(const int64_t* src, const int64_t* dst, long E, long N, int64_t* keys, int64_t* num_keys, void* ws, size_t ws_bytes,
                    hipStream_t st) {
    static const char fn[] = "kagnn_edge_keys_build";
    KAGNN_HIP(hipMemsetAsync(num_keys, 0, sizeof(int64_t), st));
    if (E == 0) return KAGNN_OK;
    EdgeKeysWorkspace w;
    edge_keys_workspace(E, ws, &w);
    if (ws_bytes < w.total) return fail(KAGNN_ERR_ARG, "%s: workspace too small", fn);
    lp_edge_key_kernel<<<cdiv(E, kLpThreads), kLpThreads, 0, st>>>(src, dst, E, N, w.raw);
    KAGNN_LAUNCH_CHECK();
    const int bits = lp_key_bits(N);
    size_t need = 0;
    KAGNN_HIP(rocprim::radix_sort_keys(nullptr, need, (const unsigned long long*)w.raw, w.sorted, (size_t)E, 0, bits, st, false));
    { int rc = lp_temp_check(fn, need, w.tmp_bytes); if (rc) return rc; }
    KAGNN_HIP(rocprim::radix_sort_keys(w.tmp, need, (const unsigned long long*)w.raw, w.sorted, (size_t)E, 0, bits, st, false));
    unsigned long long* out = reinterpret_cast<unsigned long long*>(keys);
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(num_keys);
    need = 0;
    KAGNN_HIP(rocprim::unique(nullptr, need, (const unsigned long long*)w.sorted, out, cnt, (size_t)E,
                              rocprim::equal_to<unsigned long long>(), st, false));
    { int rc = lp_temp_check(fn, need, w.tmp_bytes); if (rc) return rc; }
    KAGNN_HIP(rocprim::unique(w.tmp, need, (const unsigned long long*)w.sorted, out, cnt, (size_t)E,
                              rocprim::equal_to<unsigned long long>(), st, false));
    return KAGNN_OK;
}

// ------------------------------------------------------------------------------------------------- negative sampling
__device__ __forceinline__ bool lp_is_key(const unsigned long long* __restrict__ keys, long K, unsigned long long q) {
    long lo = 0, hi = K;                                           // first position whose key is >= q
    while (lo < hi) {
        const long mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < q) lo = mid + 1; else hi = mid;
    }
    return lo < K && keys[lo] == q;
}

// One thread per slot.  Attempt t of slot p reads the counters 2c, 2c + 1 with c = p T + t (2 num T < 2^32: api.hip); a draw is
// the high word of key32 * N, so it lies in [0, N).  The slot keeps its FIRST valid attempt; none: the pair (0, 0) and valid = 0.
__global__ __launch_bounds__(kLpThreads) void lp_negative_sample_kernel(const unsigned long long* __restrict__ keys, long K,
                                                                        unsigned long long N, long num, int T, unsigned seed_lo,
                                                                        unsigned seed_hi, int64_t* __restrict__ pairs,
                                                                        unsigned char* __restrict__ valid) {
    const long p = blockIdx.x * (long)kLpThreads + threadIdx.x;
    if (p >= num) return;
    const SampleSeed sd = sample_seed(seed_lo, seed_hi);
    unsigned long long u = 0, v = 0;
    unsigned char ok = 0;
    for (int t = 0; t < T; ++t) {
        const unsigned c = (unsigned)p * (unsigned)T + (unsigned)t;
        const unsigned long long a = ((unsigned long long)sample_key32(sd, (int)(2u * c)) * N) >> 32;
        const unsigned long long b = ((unsigned long long)sample_key32(sd, (int)(2u * c + 1u)) * N) >> 32;
        if (a == b || lp_is_key(keys, K, a * N + b)) continue;
        u = a; v = b; ok = 1;
        break;
    }
    pairs[p] = (int64_t)u;
    pairs[num + p] = (int64_t)v;
    valid[p] = ok;
}

int negative_sample(const int64_t* keys, long K, long N, long num, unsigned long long seed, int T, int64_t* pairs, unsigned char* valid,
                    hipStream_t st) {
    if (num == 0 || N == 0) return KAGNN_OK;
    lp_negative_sample_kernel<<<cdiv(num, kLpThreads), kLpThreads, 0, st>>>(reinterpret_cast<const unsigned long long*>(keys), K,
                                                                            (unsigned long long)N, num, T, (unsigned)seed,
                                                                            (unsigned)(seed >> 32), pairs, valid);
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

// ------------------------------------------------------------------------------------------------- binary cross entropy on logits
struct BceRecord { double sum; long long correct; long long rows; };      // (kagnn_node_eval's record: early_stop_update reads it)
constexpr int kBceMaxBlocks = KAGNN_BCE_WORKSPACE_BYTES / (int)sizeof(BceRecord);
constexpr long kBceRowsPerBlock = 4096;
static_assert(kBceMaxBlocks == 256, "the finishing kernel folds one partial per thread");

// the fixed tree over the 256 per-thread figures; the result in element 0 after the last barrier
__device__ __forceinline__ void bce_fold(double* s_a, long long* s_c, long long* s_r) {
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) {
            s_a[threadIdx.x] += s_a[threadIdx.x + w];
            s_c[threadIdx.x] += s_c[threadIdx.x + w];
            s_r[threadIdx.x] += s_r[threadIdx.x + w];
        }
        __syncthreads();
    }
}

// loss[0] = sum / max(rows, 1) rounded once to fp32, divisor[0] = max(rows, 1) for the backward, the meter row when asked for
__device__ __forceinline__ void bce_finish(double sum, long long correct, long long rows, float* loss, long long* divisor,
                                           BceRecord* record) {
    const long long d = rows > 0 ? rows : 1;
    loss[0] = (float)(sum / (double)d);
    divisor[0] = d;
    if (record) { record->sum = sum; record->correct = correct; record->rows = rows; }
}

// Workgroup b owns the rows [b per_block, (b + 1) per_block); a thread adds its rows (stride 256) in ascending order, in double;
// the term itself is fp32: max(s, 0) - s y + log1p(exp(-|s|)) (NaN for a NaN score).  FINAL (one workgroup): the results at once.
template <bool FINAL>
__global__ __launch_bounds__(kLpThreads) void bce_fwd_kernel(const float* __restrict__ s, const unsigned char* __restrict__ y,
                                                             const unsigned char* __restrict__ w, long P, long per_block,
                                                             BceRecord* __restrict__ partial, float* __restrict__ loss,
                                                             long long* __restrict__ divisor, BceRecord* __restrict__ record) {
    __shared__ double s_a[kLpThreads];
    __shared__ long long s_c[kLpThreads], s_r[kLpThreads];
    const long begin = blockIdx.x * per_block, end = min(P, begin + per_block);
    double a = 0.0;
    long long c = 0, r = 0;
    for (long i = begin + threadIdx.x; i < end; i += kLpThreads) {
        if (w && w[i] == 0) continue;
        const float sv = s[i];
        const bool yv = y[i] != 0;
        const float term = fmaxf(sv, 0.0f) - sv * (yv ? 1.0f : 0.0f) + log1pf(expf(-fabsf(sv)));
        a += (double)term;
        c += ((sv > 0.0f) == yv) ? 1 : 0;
        r += 1;
    }
    s_a[threadIdx.x] = a; s_c[threadIdx.x] = c; s_r[threadIdx.x] = r;
    bce_fold(s_a, s_c, s_r);
    if (threadIdx.x == 0) {
        if (FINAL) bce_finish(s_a[0], s_c[0], s_r[0], loss, divisor, record);
        else { partial[blockIdx.x].sum = s_a[0]; partial[blockIdx.x].correct = s_c[0]; partial[blockIdx.x].rows = s_r[0]; }
    }
}

// one workgroup: thread t holds the partial of workgroup t (nb <= 256), then the same tree
__global__ __launch_bounds__(kLpThreads) void bce_finish_kernel(const BceRecord* __restrict__ partial, int nb, float* __restrict__ loss,
                                                                long long* __restrict__ divisor, BceRecord* __restrict__ record) {
    __shared__ double s_a[kLpThreads];
    __shared__ long long s_c[kLpThreads], s_r[kLpThreads];
    const bool on = (int)threadIdx.x < nb;
    s_a[threadIdx.x] = on ? partial[threadIdx.x].sum : 0.0;
    s_c[threadIdx.x] = on ? partial[threadIdx.x].correct : 0;
    s_r[threadIdx.x] = on ? partial[threadIdx.x].rows : 0;
    bce_fold(s_a, s_c, s_r);
    if (threadIdx.x == 0) bce_finish(s_a[0], s_c[0], s_r[0], loss, divisor, record);
}

static int bce_blocks(long P) { return (int)max(1L, min((long)kBceMaxBlocks, (P + kBceRowsPerBlock - 1) / kBceRowsPerBlock)); }

int bce_logits_fwd(const float* s, const unsigned char* y, const unsigned char* w, long P, float* loss, int64_t* divisor, void* record,
                   void* ws, size_t ws_bytes, hipStream_t st) {
    const int nb = bce_blocks(P);
    long long* div = reinterpret_cast<long long*>(divisor);
    if (nb == 1) {
        bce_fwd_kernel<true><<<1, kLpThreads, 0, st>>>(s, y, w, P, P, nullptr, loss, div, (BceRecord*)record);
        KAGNN_LAUNCH_CHECK();
        return KAGNN_OK;
    }
    if (ws == nullptr || ws_bytes < (size_t)KAGNN_BCE_WORKSPACE_BYTES || ((uintptr_t)ws & 7) != 0)
        return fail(KAGNN_ERR_ARG, "%s: above 4096 rows the workspace must hold KAGNN_BCE_WORKSPACE_BYTES, 8-byte aligned", "kagnn_bce_logits_fwd");
    const long per_block = (P + nb - 1) / nb;
    bce_fwd_kernel<false><<<nb, kLpThreads, 0, st>>>(s, y, w, P, per_block, (BceRecord*)ws, nullptr, nullptr, nullptr);
    KAGNN_LAUNCH_CHECK();
    bce_finish_kernel<<<1, kLpThreads, 0, st>>>((const BceRecord*)ws, nb, loss, div, (BceRecord*)record);
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

// g[p] = (sigmoid(s) - y) * g_loss / divisor on rows of weight 1, exactly 0 on the others (whatever their score)
__global__ __launch_bounds__(kLpThreads) void bce_bwd_kernel(const float* __restrict__ s, const unsigned char* __restrict__ y,
                                                             const unsigned char* __restrict__ w, long P,
                                                             const long long* __restrict__ divisor, const float* __restrict__ g_loss,
                                                             float* __restrict__ g) {
    const long i = blockIdx.x * (long)kLpThreads + threadIdx.x;
    if (i >= P) return;
    float out = 0.0f;
    if (!w || w[i] != 0) {
        const float scale = g_loss[0] / (float)divisor[0];
        const float sv = s[i];
        const float e = expf(-fabsf(sv));                          // in (0, 1]: no overflow on either side
        const float sig = sv >= 0.0f ? 1.0f / (1.0f + e) : e / (1.0f + e);
        out = (sig - (y[i] != 0 ? 1.0f : 0.0f)) * scale;           // (a NaN score: NaN)
    }
    g[i] = out;
}

int bce_logits_bwd(const float* s, const unsigned char* y, const unsigned char* w, long P, const int64_t* divisor, const float* g_loss,
                   float* g, hipStream_t st) {
    if (P == 0) return KAGNN_OK;
    bce_bwd_kernel<<<cdiv(P, kLpThreads), kLpThreads, 0, st>>>(s, y, w, P, reinterpret_cast<const long long*>(divisor), g_loss, g);
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

// ------------------------------------------------------------------------------------------------- ranking metrics
constexpr unsigned kRankOut = 0xffffffffu;                         // key of a row that takes no part (above the key of +Inf)
enum : unsigned char { kRankNeg = 0, kRankPos = 1, kRankNone = 2 };

// The key orders like the score: sign bit flipped for non-negative values, all bits for negative ones; both zeros are +0.0.  The
// largest key of a number is +Inf's, 0xff800000.  Rows of weight 0 and NaN rows get kRankOut / kRankNone; the NaN rows of weight 1
// are counted into record[3] (one integer atomic per wave that holds any).
__global__ __launch_bounds__(kLpThreads) void rank_key_kernel(const float* __restrict__ s, const unsigned char* __restrict__ y,
                                                              const unsigned char* __restrict__ w, long P, unsigned* __restrict__ key,
                                                              unsigned char* __restrict__ val, unsigned char* __restrict__ val_sorted,
                                                              unsigned long long* __restrict__ record) {
    const long i = blockIdx.x * (long)kLpThreads + threadIdx.x;
    if (i == 0) val_sorted[P] = kRankNone;                         // (the scan's closing element; the sort writes [0, P))
    bool nan = false;
    if (i < P) {
        unsigned k = kRankOut;
        unsigned char v = kRankNone;
        if (!w || w[i] != 0) {
            unsigned b = __float_as_uint(s[i]);
            if ((b & 0x7fffffffu) > 0x7f800000u) nan = true;
            else {
                if ((b & 0x7fffffffu) == 0u) b = 0u;
                k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
                v = y[i] != 0 ? kRankPos : kRankNeg;
            }
        }
        key[i] = k;
        val[i] = v;
    }
    const unsigned long long nans = __ballot(nan);
    if (nans != 0ull && (threadIdx.x & 63) == 0) atomicAdd(record + 3, (unsigned long long)__popcll(nans));
}

struct RankIsNeg {
    __host__ __device__ int operator()(unsigned char v) const { return v == kRankNeg ? 1 : 0; }
};
using RankNegIter = rocprim::transform_iterator<const unsigned char*, RankIsNeg, int>;

struct RankKs { int k[3]; };

// One thread per sorted position; a positive finds its tie group [lo, hi) by two binary searches and adds
//   2 negscan[lo] + (negscan[hi] - negscan[lo])                                  to 2U,
//   1 to hits[j] if fewer than k_j negatives score at least as high: n_neg - negscan[lo] < k_j.
// The workgroup folds its five int64 figures through LDS and adds them to the record with integer atomics.
__global__ __launch_bounds__(kLpThreads) void rank_reduce_kernel(const unsigned* __restrict__ key, const unsigned char* __restrict__ val,
                                                                 const int* __restrict__ negscan, long P, RankKs ks,
                                                                 unsigned long long* __restrict__ record) {
    __shared__ long long s_v[5][kLpThreads];
    const long q = blockIdx.x * (long)kLpThreads + threadIdx.x;
    const long long n_neg = negscan[P];
    long long f[5] = {0, 0, 0, 0, 0};
    if (q < P && val[q] == kRankPos) {
        const unsigned k = key[q];
        long lo = 0, hi = P;                                       // first position with key >= k
        while (lo < hi) {
            const long mid = lo + ((hi - lo) >> 1);
            if (key[mid] < k) lo = mid + 1; else hi = mid;
        }
        const long first = lo;
        hi = P;                                                    // first position with key > k (from `first` on)
        while (lo < hi) {
            const long mid = lo + ((hi - lo) >> 1);
            if (key[mid] <= k) lo = mid + 1; else hi = mid;
        }
        const long long below = negscan[first], tied = negscan[lo] - negscan[first];
        f[0] = 2 * below + tied;
        f[1] = 1;
#pragma unroll
        for (int j = 0; j < 3; ++j) f[2 + j] = (ks.k[j] > 0 && n_neg - below < (long long)ks.k[j]) ? 1 : 0;
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) s_v[j][threadIdx.x] = f[j];
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int j = 0; j < 5; ++j) s_v[j][threadIdx.x] += s_v[j][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (s_v[0][0]) atomicAdd(record + 0, (unsigned long long)s_v[0][0]);
        if (s_v[1][0]) atomicAdd(record + 1, (unsigned long long)s_v[1][0]);
#pragma unroll
        for (int j = 0; j < 3; ++j) if (s_v[2 + j][0]) atomicAdd(record + 4 + j, (unsigned long long)s_v[2 + j][0]);
        if (blockIdx.x == 0) record[2] = (unsigned long long)n_neg;          // (zeroed ahead of the launches; no other writer)
    }
}

struct RankWorkspace {
    unsigned* key; unsigned* key_sorted;       // [P]
    unsigned char* val;                        // [P]
    unsigned char* val_sorted;                 // [P + 1]
    int* negscan;                              // [P + 1]
    void* tmp; size_t tmp_bytes; size_t total;
};

static void rank_workspace(long P, void* ws, RankWorkspace* w) {
    char* p = static_cast<char*>(ws);
    const size_t kb = lp_align((size_t)P * 4), vb = lp_align((size_t)P + 1), sb = lp_align((size_t)(P + 1) * 4);
    w->key = reinterpret_cast<unsigned*>(p); p += kb;
    w->key_sorted = reinterpret_cast<unsigned*>(p); p += kb;
    w->val = reinterpret_cast<unsigned char*>(p); p += vb;
    w->val_sorted = reinterpret_cast<unsigned char*>(p); p += vb;
    w->negscan = reinterpret_cast<int*>(p); p += sb;
    w->tmp = p;
    w->tmp_bytes = lp_temp_bound(P + 1, 5);
    w->total = 2 * kb + 2 * vb + sb + w->tmp_bytes + 256;
}

size_t link_rank_ws_bytes(long P) {
    RankWorkspace w;
    rank_workspace(P, nullptr, &w);
    return w.total;
}

int link_rank(const float* s, const unsigned char* y, const unsigned char* wgt, long P, const int* ks_host, int num_ks, int64_t* record,
              void* ws, size_t ws_bytes, hipStream_t st) {
    static const char fn[] = "kagnn_link_rank";
    KAGNN_HIP(hipMemsetAsync(record, 0, 8 * sizeof(int64_t), st));
    if (P == 0) return KAGNN_OK;
    RankWorkspace w;
    rank_workspace(P, ws, &w);
    if (ws == nullptr || ws_bytes < w.total) return fail(KAGNN_ERR_ARG, "%s: workspace too small", fn);
    unsigned long long* rec = reinterpret_cast<unsigned long long*>(record);
    const int blocks = cdiv(P, kLpThreads);
    rank_key_kernel<<<blocks, kLpThreads, 0, st>>>(s, y, wgt, P, w.key, w.val, w.val_sorted, rec);
    KAGNN_LAUNCH_CHECK();
    size_t need = 0;
    KAGNN_HIP(rocprim::radix_sort_pairs(nullptr, need, (const unsigned*)w.key, w.key_sorted, (const unsigned char*)w.val, w.val_sorted,
                                        (size_t)P, 0, 32, st, false));
    { int rc = lp_temp_check(fn, need, w.tmp_bytes); if (rc) return rc; }
    KAGNN_HIP(rocprim::radix_sort_pairs(w.tmp, need, (const unsigned*)w.key, w.key_sorted, (const unsigned char*)w.val, w.val_sorted,
                                        (size_t)P, 0, 32, st, false));
    need = 0;
    RankNegIter negs(w.val_sorted, RankIsNeg());
    KAGNN_HIP(rocprim::exclusive_scan(nullptr, need, negs, w.negscan, 0, (size_t)(P + 1), rocprim::plus<int>(), st, false));
    { int rc = lp_temp_check(fn, need, w.tmp_bytes); if (rc) return rc; }
    KAGNN_HIP(rocprim::exclusive_scan(w.tmp, need, negs, w.negscan, 0, (size_t)(P + 1), rocprim::plus<int>(), st, false));
    RankKs ks{{0, 0, 0}};
    for (int j = 0; j < num_ks && j < 3; ++j) ks.k[j] = ks_host[j];
    rank_reduce_kernel<<<blocks, kLpThreads, 0, st>>>(w.key_sorted, w.val_sorted, w.negscan, P, ks, rec);
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

}  // namespace kagnn
