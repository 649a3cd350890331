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
//
// Fan-out-limited neighbour sampling (kagnn_neighbor_sample_mark, kagnn_edge_subgraph_count, kagnn_edge_subgraph_fill) is the same
// BFS with every expanded row keeping the k in-edges of smallest (key32(seed, edge id), edge id) instead of all of them, and the
// same extraction with "the edge was kept by the sampler" in place of "both endpoints are selected" (the EDGE flag of the two row
// kernels).  The keys are a counter-based hash of the ORIGINAL edge id: which edges a row keeps is a pure function of (seed, graph),
// whatever the order of the seeds, the launch geometry or the lane that sees an entry.
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

// ------------------------------------------------------------------------------------------------- neighbour sampling
// (key32 of the ABI -- sample_seed, sample_key32 -- lives in common.h: linkpred.hip draws its negatives from the same function)

// entry p of an expanding row is selected: its edge is kept, its source joins level d + 1 if nobody reached it before
__device__ __forceinline__ void sample_take(const int* __restrict__ col, int p, int e, long N, long E, int d, int* hop,
                                            unsigned char* __restrict__ keep) {
    if ((unsigned)e < (unsigned long)E) keep[e] = 1;
    const int j = col[p];
    if ((unsigned)j < (unsigned long)N && ld_relaxed(hop + j) == -1) st_relaxed(hop + j, d + 1);
}

// Level d of the sampled BFS: rows whose hop is d (final before this launch) select min(deg, k) of their in-edges -- the k entries of
// smallest (key32, edge id) -- set keep[] for them and mark their still unreached sources d + 1.  Same store discipline as
// khop_level_kernel: hop entries only go from -1 to d + 1, keep bytes only from 0 to 1, so concurrent writers agree.
//   k >= deg:   the whole row, no key computed.
//   deg <= 64:  one key per lane, rank by comparison against every other lane's pair (v_readlane), keep rank < k.
//   longer:     radix select on the key, most significant byte first -- a 256-bin histogram per wave in LDS (integer counts: the
//               order of the adds does not matter), four passes over the row narrow (prefix, need) down to the k-th smallest key T
//               and the number of entries equal to T still to take; a fifth pass keeps key < T and, by an ordered ballot with a
//               running count, the first `need` entries with key == T -- the row stands in ascending edge id, so those are the
//               lowest edge ids.  Nothing of a row is staged: a row of any length works at any k.
__global__ __launch_bounds__(kSubThreads) void sample_level_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                   const int* __restrict__ perm, long N, long E, int d, int k,
                                                                   unsigned seed_lo, unsigned seed_hi, int* hop,
                                                                   unsigned char* __restrict__ keep) {
    __shared__ unsigned s_hist[kSubThreads / 64][256];
    const long i = blockIdx.x * (long)kSubThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    unsigned* hist = s_hist[threadIdx.x >> 6];
    const SampleSeed sd = sample_seed(seed_lo, seed_hi);
    const bool front = i < N && ld_relaxed(hop + i) == d;
    int s = 0, t = 0;
    if (front) { s = rowptr[i]; t = rowptr[i + 1]; }
    unsigned long long rows = k > 0 ? __ballot(front) : 0ull;
    while (rows) {
        const int src = __ffsll((long long)rows) - 1;
        rows &= rows - 1;
        const int rs = __shfl(s, src), rt = __shfl(t, src);
        const int deg = rt - rs;
        if (deg <= 0) continue;
        if (k >= deg) {
#pragma unroll 4
            for (int p = rs + lane; p < rt; p += 64) sample_take(col, p, perm[p], N, E, d, hop, keep);
        } else if (deg <= 64) {
            const int p = rs + lane;
            const bool valid = p < rt;
            const int e = valid ? perm[p] : 0;
            const unsigned key = sample_key32(sd, e);
            int rank = 0;
            for (int l = 0; l < deg; ++l) {                          // (l is wave-uniform: a scalar lane select)
                const unsigned kl = (unsigned)__builtin_amdgcn_readlane((int)key, l);
                const int el = __builtin_amdgcn_readlane(e, l);
                rank += (kl < key || (kl == key && el < e)) ? 1 : 0;
            }
            if (valid && rank < k) sample_take(col, p, e, N, E, d, hop, keep);
        } else {
            unsigned prefix = 0;                                     // the bytes of T settled so far, in place
            int need = k;                                            // 1 <= need <= number of entries whose key matches prefix
            for (int shift = 24; shift >= 0; shift -= 8) {
#pragma unroll
                for (int b = 0; b < 4; ++b) hist[lane * 4 + b] = 0;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const unsigned above = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
                for (int p = rs + lane; p < rt; p += 64) {
                    const unsigned key = sample_key32(sd, perm[p]);
                    if ((key & above) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                int b4[4], sum = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) { b4[b] = (int)hist[lane * 4 + b]; sum += b4[b]; }
                int incl = sum;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int up = __shfl_up(incl, o);
                    incl += lane >= o ? up : 0;
                }
                const int excl = incl - sum;
                const bool mine = excl < need && need <= incl;       // exactly one lane: the counts sum to >= need
                int digit = 0, left = 0;
                if (mine) {
                    int run = excl;
                    bool done = false;
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        if (!done && need <= run + b4[b]) { digit = lane * 4 + b; left = need - run; done = true; }
                        run += b4[b];
                    }
                }
                const unsigned long long who = __ballot(mine);
                const int from = who ? __ffsll((long long)who) - 1 : 0;
                digit = __shfl(digit, from);
                need = __shfl(left, from);
                prefix |= (unsigned)digit << shift;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // (the bins are read before the next pass clears them)
                __builtin_amdgcn_wave_barrier();
            }
            int ties = 0;                                            // entries with key == prefix taken so far, in row order
            for (int p0 = rs; p0 < rt; p0 += 64) {                   // (wave-uniform trip count: every lane takes part in the ballot)
                const int p = p0 + lane;
                int e = 0;
                unsigned key = 0xffffffffu;
                bool tie = false;
                if (p < rt) { e = perm[p]; key = sample_key32(sd, e); tie = key == prefix; }
                const unsigned long long tied = __ballot(tie);
                const bool take = p < rt && (key < prefix || (tie && ties + lanes_below(tied, lane) < need));
                if (take) sample_take(col, p, e, N, E, d, hop, keep);
                ties += __popcll(tied);
            }
        }
    }
}

// cnt[i] = number of entries of row i whose other endpoint is selected (0 for a row that is not selected itself; cnt[N] = 0, the
// closing entry of the scan).  KEEP (the by-destination side): keep[perm[p]] = 1 for every such entry -- the kept edges in ORIGINAL
// edge order; keep was zeroed ahead of the launch and perm is a permutation, so every byte has one writer.
// EDGE (the subgraph of an edge selection): an entry counts only if given[perm[p]] is set as well -- the caller's edge selection, by
// original edge id; nothing is written to keep.
template <bool KEEP, bool EDGE>
__global__ __launch_bounds__(kSubThreads) void sub_count_rows_kernel(const int* __restrict__ hop, const int* __restrict__ rowptr,
                                                                     const int* __restrict__ col, const int* __restrict__ perm, long N,
                                                                     long E, int* __restrict__ cnt, unsigned char* __restrict__ keep,
                                                                     const unsigned char* __restrict__ given) {
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
            bool k = (unsigned)j < (unsigned long)N && hop[j] >= 0;
            if (EDGE) {
                const int e = perm[p];
                k = k && (unsigned)e < (unsigned long)E && given[e] != 0;
            }
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
// EDGE: an entry is kept only if given[perm[p]] is set as well (the count kernel's rule).
template <bool BY_DST, bool EDGE>
__global__ __launch_bounds__(kSubThreads) void sub_fill_kernel(const int* __restrict__ relabel, const int* __restrict__ rp,
                                                               const int* __restrict__ edge_rank, const int* __restrict__ rowptr,
                                                               const int* __restrict__ col, const int* __restrict__ perm, long N, long E,
                                                               int n_sub, int e_sub, int* __restrict__ rowptr_o, int* __restrict__ col_o,
                                                               int* __restrict__ perm_o, int64_t* __restrict__ nodes,
                                                               int64_t* __restrict__ edge_ids, int64_t* __restrict__ ei,
                                                               const unsigned char* __restrict__ given) {
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
                if (EDGE) {
                    const int e = perm[p];
                    cj = (unsigned)e < (unsigned long)E && given[e] != 0 ? cj : -1;
                }
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
struct SetByteAsInt {                                               // (a caller's edge selection: any non-zero byte)
    __host__ __device__ int operator()(unsigned char b) const { return b != 0 ? 1 : 0; }
};
using ByteIter = rocprim::transform_iterator<const unsigned char*, ByteAsInt, int>;
using SetIter = rocprim::transform_iterator<const unsigned char*, SetByteAsInt, int>;

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

// level d of the sampled BFS takes min(deg, fanout[d]) in-edges per frontier row; a negative fan-out is "all"
int neighbor_sample_mark(const int* rowptr, const int* col, const int* perm, long N, long E, const int64_t* seeds, long S, const int* fanout,
                         int num_levels, unsigned long long seed, int* hop, unsigned char* keep, int* flags, hipStream_t st) {
    KAGNN_HIP(hipMemsetAsync(flags, 0, sizeof(int), st));
    if (N > 0) KAGNN_HIP(hipMemsetAsync(hop, 0xff, (size_t)N * 4, st));        // -1
    if (E > 0) KAGNN_HIP(hipMemsetAsync(keep, 0, (size_t)E, st));
    if (S == 0) return KAGNN_OK;
    khop_seed_kernel<<<cdiv(S, 256), 256, 0, st>>>(seeds, S, N, hop, flags);    // (N == 0: every seed is out of range)
    KAGNN_LAUNCH_CHECK();
    if (N == 0 || E == 0) return KAGNN_OK;                                      // (no edge: nothing to select, nobody to reach)
    for (int d = 0; d < num_levels; ++d) {
        const int k = fanout[d] < 0 ? 0x7fffffff : fanout[d];
        sample_level_kernel<<<cdiv(N, kSubThreads), kSubThreads, 0, st>>>(rowptr, col, perm, N, E, d, k, (unsigned)seed,
                                                                          (unsigned)(seed >> 32), hop, keep);
        KAGNN_LAUNCH_CHECK();
    }
    return KAGNN_OK;
}

// given == nullptr: the induced subgraph of the node selection (kagnn_subgraph_count); else the subgraph of the edge selection `given`
// (kagnn_edge_subgraph_count), which is read in place -- the workspace's own keep bytes stay unused
static int sub_count(const char* fn, const int* hop, const unsigned char* given, const int* rowptr, const int* col, const int* perm,
                     const int* rowptr_t, const int* col_t, const int* perm_t, long N, long E, void* ws, size_t ws_bytes, int* counts,
                     hipStream_t st) {
    SubWorkspace w;
    sub_workspace(N, E, ws, &w);
    if (ws_bytes < w.total) return fail(KAGNN_ERR_ARG, "%s: workspace too small", fn);
    if (N == 0) {
        KAGNN_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int), st));
        return KAGNN_OK;
    }
    const size_t tb = w.tmp_bytes;
    { int rc = sub_scan(w.tmp, tb, SelIter(hop, SelectedAsInt()), w.nscan, N, st); if (rc) return rc; }
    const int blocks = cdiv(N + 1, kSubThreads);
    if (given) {
        sub_count_rows_kernel<false, true><<<blocks, kSubThreads, 0, st>>>(hop, rowptr, col, perm, N, E, w.cnt_d, nullptr, given);
        KAGNN_LAUNCH_CHECK();
        sub_count_rows_kernel<false, true><<<blocks, kSubThreads, 0, st>>>(hop, rowptr_t, col_t, perm_t, N, E, w.cnt_s, nullptr, given);
        KAGNN_LAUNCH_CHECK();
    } else {
        if (E > 0) KAGNN_HIP(hipMemsetAsync(w.keep, 0, (size_t)E, st));
        sub_count_rows_kernel<true, false><<<blocks, kSubThreads, 0, st>>>(hop, rowptr, col, perm, N, E, w.cnt_d, w.keep, nullptr);
        KAGNN_LAUNCH_CHECK();
        sub_count_rows_kernel<false, false><<<blocks, kSubThreads, 0, st>>>(hop, rowptr_t, col_t, nullptr, N, E, w.cnt_s, nullptr, nullptr);
        KAGNN_LAUNCH_CHECK();
    }
    { int rc = sub_scan(w.tmp, tb, (const int*)w.cnt_d, w.rp_d, N + 1, st); if (rc) return rc; }
    { int rc = sub_scan(w.tmp, tb, (const int*)w.cnt_s, w.rp_s, N + 1, st); if (rc) return rc; }
    if (given) { int rc = sub_scan(w.tmp, tb, SetIter(given, SetByteAsInt()), w.edge_rank, E, st); if (rc) return rc; }
    else { int rc = sub_scan(w.tmp, tb, ByteIter(w.keep, ByteAsInt()), w.edge_rank, E, st); if (rc) return rc; }
    sub_finish_count_kernel<<<cdiv(N, 256), 256, 0, st>>>(hop, w.nscan, w.rp_d, N, w.relabel, counts);
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

static int sub_fill(const char* fn, const void* ws, size_t ws_bytes, const unsigned char* given, const int* rowptr, const int* col,
                    const int* perm, const int* rowptr_t, const int* col_t, const int* perm_t, long N, long E, long n_sub, long e_sub,
                    int64_t* nodes, int64_t* edge_ids, int64_t* ei, int* rowptr_o, int* col_o, int* perm_o, int* rowptr_to, int* col_to,
                    int* perm_to, hipStream_t st) {
    SubWorkspace w;
    sub_workspace(N, E, const_cast<void*>(ws), &w);
    if (ws_bytes < w.total) return fail(KAGNN_ERR_ARG, "%s: workspace too small", fn);
    if (N == 0 || n_sub == 0) {                                    // (no selected row: only the closing row pointers)
        KAGNN_HIP(hipMemsetAsync(rowptr_o, 0, sizeof(int), st));
        KAGNN_HIP(hipMemsetAsync(rowptr_to, 0, sizeof(int), st));
        return KAGNN_OK;
    }
    const int blocks = cdiv(N, kSubThreads);
    const int ns = (int)n_sub, es = (int)e_sub;
    if (given) {
        sub_fill_kernel<true, true><<<blocks, kSubThreads, 0, st>>>(w.relabel, w.rp_d, w.edge_rank, rowptr, col, perm, N, E, ns, es, rowptr_o,
                                                                   col_o, perm_o, nodes, edge_ids, ei, given);
        KAGNN_LAUNCH_CHECK();
        sub_fill_kernel<false, true><<<blocks, kSubThreads, 0, st>>>(w.relabel, w.rp_s, w.edge_rank, rowptr_t, col_t, perm_t, N, E, ns, es,
                                                                    rowptr_to, col_to, perm_to, nullptr, nullptr, nullptr, given);
        KAGNN_LAUNCH_CHECK();
        return KAGNN_OK;
    }
    sub_fill_kernel<true, false><<<blocks, kSubThreads, 0, st>>>(w.relabel, w.rp_d, w.edge_rank, rowptr, col, perm, N, E, ns, es, rowptr_o,
                                                                col_o, perm_o, nodes, edge_ids, ei, nullptr);
    KAGNN_LAUNCH_CHECK();
    sub_fill_kernel<false, false><<<blocks, kSubThreads, 0, st>>>(w.relabel, w.rp_s, w.edge_rank, rowptr_t, col_t, perm_t, N, E, ns, es,
                                                                 rowptr_to, col_to, perm_to, nullptr, nullptr, nullptr, nullptr);
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

int subgraph_count(const int* hop, const int* rowptr, const int* col, const int* perm, const int* rowptr_t, const int* col_t, long N, long E,
                   void* ws, size_t ws_bytes, int* counts, hipStream_t st) {
    return sub_count("kagnn_subgraph_count", hop, nullptr, rowptr, col, perm, rowptr_t, col_t, nullptr, N, E, ws, ws_bytes, counts, st);
}

int subgraph_fill(const void* ws, size_t ws_bytes, const int* rowptr, const int* col, const int* perm, const int* rowptr_t, const int* col_t,
                  const int* perm_t, long N, long E, long n_sub, long e_sub, int64_t* nodes, int64_t* edge_ids, int64_t* ei, int* rowptr_o,
                  int* col_o, int* perm_o, int* rowptr_to, int* col_to, int* perm_to, hipStream_t st) {
    return sub_fill("kagnn_subgraph_fill", ws, ws_bytes, nullptr, rowptr, col, perm, rowptr_t, col_t, perm_t, N, E, n_sub, e_sub, nodes,
                    edge_ids, ei, rowptr_o, col_o, perm_o, rowptr_to, col_to, perm_to, st);
}

int edge_subgraph_count(const int* hop, const unsigned char* keep, const int* rowptr, const int* col, const int* perm, const int* rowptr_t,
                        const int* col_t, const int* perm_t, long N, long E, void* ws, size_t ws_bytes, int* counts, hipStream_t st) {
    return sub_count("kagnn_edge_subgraph_count", hop, keep, rowptr, col, perm, rowptr_t, col_t, perm_t, N, E, ws, ws_bytes, counts, st);
}

int edge_subgraph_fill(const void* ws, size_t ws_bytes, const unsigned char* keep, const int* rowptr, const int* col, const int* perm,
                       const int* rowptr_t, const int* col_t, const int* perm_t, long N, long E, long n_sub, long e_sub, int64_t* nodes,
                       int64_t* edge_ids, int64_t* ei, int* rowptr_o, int* col_o, int* perm_o, int* rowptr_to, int* col_to, int* perm_to,
                       hipStream_t st) {
    return sub_fill("kagnn_edge_subgraph_fill", ws, ws_bytes, keep, rowptr, col, perm, rowptr_t, col_t, perm_t, N, E, n_sub, e_sub, nodes,
                    edge_ids, ei, rowptr_o, col_o, perm_o, rowptr_to, col_to, perm_to, st);
}

}  // namespace kagnn
