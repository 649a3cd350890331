// k-hop neighbourhoods and induced subgraphs of an indexed graph, on the device (kagnn_k_hop_mark, kagnn_subgraph_count,
// kagnn_subgraph_fill: include/kagnn_hip.h).  Replaces torch_geometric.utils.k_hop_subgraph / subgraph (a boolean pass over all E
// edges and a nonzero per hop) AND the sort-based index build of the result: the parent's by-destination CSR is the adjacency a
// backward BFS walks, and both CSR structures of an induced subgraph are the parent's rows with entries dropped, in unchanged
// order -- `perm` comes from a stable sort, so the restriction of a parent row already is in the order a rebuild would produce.
// No sort, no float, no atomic read-modify-write: every result is a pure function of the inputs.
//
// Work distribution of the three row kernels: one thread per parent node decides whether its row takes part (frontier / selected);
// the wave then walks each participating row of its 64 nodes with all 64 lanes, so a 100k-edge hub costs 1.6k coalesced steps,
// not 100k serial ones, and rows that do not take part (nearly all of them: a receptive field is a sliver of the graph) cost one
// load.  Order inside a row is kept by a ballot per 64-entry chunk and a running offset carried across the chunks.
#include "common.h"
#include "host.h"
#include <rocprim/rocprim.hpp>

namespace kagnn {

constexpr int kSubThreads = 256;

__device__ __forceinline__ int ld_relaxed(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_relaxed(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int lanes_below(unsigned long long mask, int lane) { return __popcll(mask & ((1ull << lane) - 1ull)); }

// hop was filled with -1 ahead of this launch.  Every writer of hop[v] stores 0 and every writer of flags[0] stores 1.
__global__ void khop_seed_kernel(const int64_t* __restrict__ seeds, long S, long N, int* hop, int* flags) {
    const long s = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int64_t v = seeds[s];
    if (v < 0 || v >= N) st_relaxed(flags, 1);
    else st_relaxed(hop + v, 0);
}

// Level d: rows whose hop is d (final before this launch) mark their still unreached in-neighbours d + 1.  Entries are only ever
// changed from -1 to d + 1 here, so concurrent writers store the same value and a stale -1 read only repeats the store.
__global__ __launch_bounds__(kSubThreads) void khop_level_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, long N, int d,
                                                                 int* hop) {
    const long i = blockIdx.x * (long)kSubThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool front = i < N && ld_relaxed(hop + i) == d;
    int s = 0, t = 0;
    if (front) { s = rowptr[i]; t = rowptr[i + 1]; }
    unsigned long long rows = __ballot(front);
    while (rows) {
        const int src = __ffsll((long long)rows) - 1;
        rows &= rows - 1;
        const int rs = __shfl(s, src), rt = __shfl(t, src);
#pragma unroll 4
        for (int p = rs + lane; p < rt; p += 64) {
            const int j = col[p];
            if ((unsigned)j < (unsigned long)N && ld_relaxed(hop + j) == -1) st_relaxed(hop + j, d + 1);
        }
    }
}

// cnt[i] = number of entries of row i whose other endpoint is selected (0 for a row that is not selected itself; cnt[N] = 0, the
// closing entry of the scan).  KEEP (the by-destination side): keep[perm[p]] = 1 for every such entry -- the kept edges in ORIGINAL
// edge order; keep was zeroed ahead of the launch and perm is a permutation, so every byte has one writer.
template <bool KEEP>
__global__ __launch_bounds__(kSubThreads) void sub_count_rows_kernel(const int* __restrict__ hop, const int* __restrict__ rowptr,
                                                                     const int* __restrict__ col, const int* __restrict__ perm, long N,
                                                                     long E, int* __restrict__ cnt, unsigned char* __restrict__ keep) {
    const long i = blockIdx.x * (long)kSubThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool sel = i < N && hop[i] >= 0;
    int s = 0, t = 0, mine = 0;
    if (sel) { s = rowptr[i]; t = rowptr[i + 1]; }
    unsigned long long rows = __ballot(sel);
    while (rows) {
        const int src = __ffsll((long long)rows) - 1;
        rows &= rows - 1;
        const int rs = __shfl(s, src), rt = __shfl(t, src);
        int c = 0;
#pragma unroll 4
        for (int p = rs + lane; p < rt; p += 64) {
            const int j = col[p];
            const bool k = (unsigned)j < (unsigned long)N && hop[j] >= 0;
            c += k ? 1 : 0;
            if (KEEP && k) {
                const int e = perm[p];
                if ((unsigned)e < (unsigned long)E) keep[e] = 1;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
        mine = lane == src ? c : mine;
    }
    if (i <= N) cnt[i] = mine;
}

// relabel[i] = rank of node i among the selected nodes, -1 outside the selection; counts[0..1] = n_sub, e_sub
__global__ void sub_finish_count_kernel(const int* __restrict__ hop, const int* __restrict__ nscan, const int* __restrict__ rp_d, long N,
                                        int* __restrict__ relabel, int* __restrict__ counts) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i < N) relabel[i] = hop[i] >= 0 ? nscan[i] : -1;
    if (i == N - 1) { counts[0] = nscan[i] + (hop[i] >= 0 ? 1 : 0); counts[1] = rp_d[N]; }
}

// One side of the subgraph's index from the same side of the parent's: row i of the parent becomes row relabel[i], starting at
// rp[i] (the scanned counts), its kept entries in the parent's order.  BY_DST also writes what is indexed by node or by original
// edge: nodes, edge_ids and the relabelled edge list (row i is the DESTINATION of its entries, col the source).  Every store is
// guarded by the caller's n_sub / e_sub: with figures that are not the count call's nothing leaves the outputs.
template <bool BY_DST>
__global__ __launch_bounds__(kSubThreads) void sub_fill_kernel(const int* __restrict__ relabel, const int* __restrict__ rp,
                                                               const int* __restrict__ edge_rank, const int* __restrict__ rowptr,
                                                               const int* __restrict__ col, const int* __restrict__ perm, long N, long E,
                                                               int n_sub, int e_sub, int* __restrict__ rowptr_o, int* __restrict__ col_o,
                                                               int* __restrict__ perm_o, int64_t* __restrict__ nodes,
                                                               int64_t* __restrict__ edge_ids, int64_t* __restrict__ ei) {
    const long i = blockIdx.x * (long)kSubThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int r = i < N ? relabel[i] : -1;
    const bool sel = r >= 0 && r < n_sub;
    int s = 0, t = 0, base = 0;
    if (i == 0) rowptr_o[n_sub] = e_sub;
    if (sel) {
        s = rowptr[i]; t = rowptr[i + 1];
        base = rp[i];
        rowptr_o[r] = min(base, e_sub);
        if (BY_DST) nodes[r] = i;
    }
    unsigned long long rows = __ballot(sel);
    while (rows) {
        const int src = __ffsll((long long)rows) - 1;
        rows &= rows - 1;
        const int rs = __shfl(s, src), rt = __shfl(t, src), rr = __shfl(r, src);
        int run = __shfl(base, src);
        for (int p0 = rs; p0 < rt; p0 += 64) {                     // (wave-uniform trip count: every lane takes part in the ballot)
            const int p = p0 + lane;
            int cj = -1;
            if (p < rt) {
                const int j = col[p];
                cj = (unsigned)j < (unsigned long)N ? relabel[j] : -1;
            }
            const bool k = cj >= 0;
            const unsigned long long kept = __ballot(k);
            if (k) {
                const int pos = run + lanes_below(kept, lane);
                const int e = perm[p];
                const int er = (unsigned)e < (unsigned long)E ? edge_rank[e] : -1;
                if (pos < e_sub) { col_o[pos] = cj; perm_o[pos] = er; }
                if (BY_DST && er >= 0 && er < e_sub) {
                    edge_ids[er] = e;
                    ei[er] = cj;
                    ei[(long)e_sub + er] = rr;
                }
            }
            run += __popcll(kept);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
struct SelectedAsInt {
    __host__ __device__ int operator()(int h) const { return h >= 0 ? 1 : 0; }
};
struct ByteAsInt {
    __host__ __device__ int operator()(unsigned char b) const { return (int)b; }
};
using SelIter = rocprim::transform_iterator<const int*, SelectedAsInt, int>;
using ByteIter = rocprim::transform_iterator<const unsigned char*, ByteAsInt, int>;

// The workspace is sized on the host without asking rocPRIM (the size query below needs a device; kagnn_subgraph_workspace_bytes does
// not): a decoupled look-back scan keeps a few bytes of state per BLOCK of several thousand elements, sub_scan_temp_bound allows a
// quarter byte per ELEMENT plus 64 KiB, and every scan checks rocPRIM's real figure against what it was given before it runs.
static size_t sub_align(size_t x) { return (x + 255) & ~(size_t)255; }
static size_t sub_scan_temp_bound(long n) { return sub_align((size_t)n / 4 + ((size_t)64 << 10)); }

template <class In>
static int sub_scan(void* tmp, size_t tmp_bytes, In in, int* out, long n, hipStream_t st) {
    if (n <= 0) return KAGNN_OK;
    size_t need = 0;
    KAGNN_HIP(rocprim::exclusive_scan(nullptr, need, in, out, 0, (size_t)n, rocprim::plus<int>(), st, false));
    if (need > tmp_bytes) return fail(KAGNN_ERR_UNSUPPORTED, "%s: the scan needs %ld bytes of temporary storage, the workspace holds %ld", "kagnn_subgraph_count", (long)need, (long)tmp_bytes);
    KAGNN_HIP(rocprim::exclusive_scan(tmp, need, in, out, 0, (size_t)n, rocprim::plus<int>(), st, false));
    return KAGNN_OK;
}

// the workspace: relabel FIRST (a binding gathers a seed's position in `nodes` from it), then the scan outputs the fill call reads
struct SubWorkspace {
    int* relabel;            // [N]
    int* nscan;              // [N]      exclusive scan of (hop >= 0)
    int* edge_rank;          // [E]      exclusive scan of keep: the rank of a kept edge among kept edges, original edge order
    int* rp_d; int* rp_s;    // [N + 1]  exclusive scans of the row counts: where parent row i starts in the subgraph (both sides)
    int* cnt_d; int* cnt_s;  // [N + 1]
    unsigned char* keep;     // [E]
    void* tmp; size_t tmp_bytes;
    size_t total;
};

static void sub_workspace(long N, long E, void* ws, SubWorkspace* w) {
    char* p = static_cast<char*>(ws);
    const size_t nb = sub_align((size_t)(N + 1) * 4), eb = sub_align((size_t)E * 4);
    w->relabel = reinterpret_cast<int*>(p); p += nb;
    w->nscan = reinterpret_cast<int*>(p); p += nb;
    w->edge_rank = reinterpret_cast<int*>(p); p += eb;
    w->rp_d = reinterpret_cast<int*>(p); p += nb;
    w->rp_s = reinterpret_cast<int*>(p); p += nb;
    w->cnt_d = reinterpret_cast<int*>(p); p += nb;
    w->cnt_s = reinterpret_cast<int*>(p); p += nb;
    w->keep = reinterpret_cast<unsigned char*>(p); p += sub_align((size_t)E);
    w->tmp = p;
    w->tmp_bytes = sub_scan_temp_bound(N + 1 > E ? N + 1 : E);
    w->total = (size_t)(p - static_cast<char*>(ws)) + w->tmp_bytes + 256;
}

int subgraph_workspace_bytes(long N, long E, size_t* bytes) {
    SubWorkspace w;
    sub_workspace(N, E, nullptr, &w);
    *bytes = w.total;
    return KAGNN_OK;
}

int k_hop_mark(const int* rowptr, const int* col, long N, const int64_t* seeds, long S, int num_hops, int* hop, int* flags, hipStream_t st) {
    KAGNN_HIP(hipMemsetAsync(flags, 0, sizeof(int), st));
    if (N > 0) KAGNN_HIP(hipMemsetAsync(hop, 0xff, (size_t)N * 4, st));        // -1
    if (S == 0) return KAGNN_OK;
    khop_seed_kernel<<<cdiv(S, 256), 256, 0, st>>>(seeds, S, N, hop, flags);    // (N == 0: every seed is out of range)
    KAGNN_LAUNCH_CHECK();
    if (N == 0) return KAGNN_OK;
    for (int d = 0; d < num_hops; ++d) {
        khop_level_kernel<<<cdiv(N, kSubThreads), kSubThreads, 0, st>>>(rowptr, col, N, d, hop);
        KAGNN_LAUNCH_CHECK();
    }
    return KAGNN_OK;
}

int subgraph_count(const int* hop, const int* rowptr, const int* col, const int* perm, const int* rowptr_t, const int* col_t, long N, long E,
                   void* ws, size_t ws_bytes, int* counts, hipStream_t st) {
    SubWorkspace w;
    sub_workspace(N, E, ws, &w);
    if (ws_bytes < w.total) return fail(KAGNN_ERR_ARG, "%s: workspace too small", "kagnn_subgraph_count");
    if (N == 0) {
        KAGNN_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int), st));
        return KAGNN_OK;
    }
    const size_t tb = w.tmp_bytes;
    { int rc = sub_scan(w.tmp, tb, SelIter(hop, SelectedAsInt()), w.nscan, N, st); if (rc) return rc; }
    if (E > 0) KAGNN_HIP(hipMemsetAsync(w.keep, 0, (size_t)E, st));
    const int blocks = cdiv(N + 1, kSubThreads);
    sub_count_rows_kernel<true><<<blocks, kSubThreads, 0, st>>>(hop, rowptr, col, perm, N, E, w.cnt_d, w.keep);
    KAGNN_LAUNCH_CHECK();
    sub_count_rows_kernel<false><<<blocks, kSubThreads, 0, st>>>(hop, rowptr_t, col_t, nullptr, N, E, w.cnt_s, nullptr);
    KAGNN_LAUNCH_CHECK();
    { int rc = sub_scan(w.tmp, tb, (const int*)w.cnt_d, w.rp_d, N + 1, st); if (rc) return rc; }
    { int rc = sub_scan(w.tmp, tb, (const int*)w.cnt_s, w.rp_s, N + 1, st); if (rc) return rc; }
    { int rc = sub_scan(w.tmp, tb, ByteIter(w.keep, ByteAsInt()), w.edge_rank, E, st); if (rc) return rc; }
    sub_finish_count_kernel<<<cdiv(N, 256), 256, 0, st>>>(hop, w.nscan, w.rp_d, N, w.relabel, counts);
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

int subgraph_fill(const void* ws, size_t ws_bytes, const int* rowptr, const int* col, const int* perm, const int* rowptr_t, const int* col_t,
                  const int* perm_t, long N, long E, long n_sub, long e_sub, int64_t* nodes, int64_t* edge_ids, int64_t* ei, int* rowptr_o,
                  int* col_o, int* perm_o, int* rowptr_to, int* col_to, int* perm_to, hipStream_t st) {
    SubWorkspace w;
    sub_workspace(N, E, const_cast<void*>(ws), &w);
    if (ws_bytes < w.total) return fail(KAGNN_ERR_ARG, "%s: workspace too small", "kagnn_subgraph_fill");
    if (N == 0 || n_sub == 0) {                                    // (no selected row: only the closing row pointers)
        KAGNN_HIP(hipMemsetAsync(rowptr_o, 0, sizeof(int), st));
        KAGNN_HIP(hipMemsetAsync(rowptr_to, 0, sizeof(int), st));
        return KAGNN_OK;
    }
    const int blocks = cdiv(N, kSubThreads);
    sub_fill_kernel<true><<<blocks, kSubThreads, 0, st>>>(w.relabel, w.rp_d, w.edge_rank, rowptr, col, perm, N, E, (int)n_sub, (int)e_sub,
                                                         rowptr_o, col_o, perm_o, nodes, edge_ids, ei);
    KAGNN_LAUNCH_CHECK();
    sub_fill_kernel<false><<<blocks, kSubThreads, 0, st>>>(w.relabel, w.rp_s, w.edge_rank, rowptr_t, col_t, perm_t, N, E, (int)n_sub,
                                                          (int)e_sub, rowptr_to, col_to, perm_to, nullptr, nullptr, nullptr);
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

}  // namespace kagnn
