// Mini-batch assembly from a device-resident dataset of disjoint graphs (kagnn_batch_assemble, include/kagnn_hip.h).
// Replaces, per training step, torch_geometric's host-side collation + `data.to(device)` (reference
// graph_regression/optuna_zinc.py:59-66, graph_classification/graph_classification_utils.py:109-128) AND the per-batch CSR
// build: the dataset is collated once as one giant batch in dataset order and indexed once; a mini-batch -- x, edge_index,
// edge_attr, y, batch, ptr and both CSR structures -- is per-graph slices of those arrays, concatenated in batch order with the
// node / edge offsets rebased.  The graphs are disjoint and their nodes contiguous, so a stable sort by destination (source)
// never moves an edge across a graph boundary: the slices of the dataset's (rowptr, col, perm) ARE the batch's, element for
// element.  No sort, one launch, no dependency between workgroups.
#include "common.h"
#include "host.h"

namespace kagnn {

constexpr int kBatchThreads = 256;
constexpr int kBatchMaxBlocks = 2048;

struct BatchArgs {
    const int64_t* node_ptr; const int64_t* edge_ptr; const int64_t* ids;
    long G; int B; int N; int E;                       // dataset graphs; graphs / nodes / edges of the batch (the host's figures)
    const unsigned char* x_all; const unsigned char* ea_all; const unsigned char* y_all;
    unsigned char* x; unsigned char* ea; unsigned char* y;
    int x_unit, ea_unit, y_unit;                       // bytes per access: 16 / 8 / 4 (what row size and both bases allow)
    long x_upr, ea_upr, y_upr;                         // units per row
    const int64_t* src_all; const int64_t* dst_all;
    const int* R; const int* C; const int* P; const int* Rt; const int* Ct; const int* Pt;
    int64_t* ei; int64_t* batch; int64_t* ptr;
    int* rowptr; int* col; int* perm; int* rowptr_t; int* col_t; int* perm_t;       // all six or none
    int* flags;
    long s_x, s_node, s_edge, s_ea, s_y, s_ptr;        // sizes of the six sections of the flat work list
};

__device__ __forceinline__ void copy_unit(unsigned char* dst, const unsigned char* src, int unit, long d, long s) {
    if (unit == 16) reinterpret_cast<u32x4*>(dst)[d] = reinterpret_cast<const u32x4*>(src)[s];
    else if (unit == 8) reinterpret_cast<u32x2*>(dst)[d] = reinterpret_cast<const u32x2*>(src)[s];
    else reinterpret_cast<unsigned*>(dst)[d] = reinterpret_cast<const unsigned*>(src)[s];
}

// the graph slot k of item i: off[k] <= i < off[k + 1] (empty graphs have off[k] == off[k + 1] and are never chosen);
// -1 when i >= off[B], i.e. the scanned total is short of the host's figure (flagged; nothing is written for such an item)
__device__ __forceinline__ int find_slot(const int* __restrict__ off, int B, int i) {
    if (i >= off[B]) return -1;
    int lo = 0, hi = B - 1;                            // first k with off[k + 1] > i
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (off[mid + 1] > i) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// Every workgroup scans the batch's B node and edge counts itself (LDS; nothing passes between workgroups), then takes its
// share of ONE flat work list:  [x units | node items | edge items | edge_attr units | y units | ptr items].
// LDS (dynamic): s_no[B + 1], s_eo[B + 1] = the batch's exclusive node / edge offsets, s_ns[B], s_es[B] = where graph ids[k]
// starts in the dataset.  int32 throughout: the dataset's N and E fit (the library's index type), the batch's offsets are
// clamped at 2^31 - 1 (a sum beyond the host's figure is a flagged mismatch, and clamped offsets stay monotone, so no item
// resolves to a row outside its graph).
__global__ __launch_bounds__(kBatchThreads) void batch_assemble_kernel(const BatchArgs a) {
    constexpr int T = kBatchThreads;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_batch[];
    __shared__ long long s_part[2][T / 64];
    const int B = a.B, tid = threadIdx.x;
    int* s_no = reinterpret_cast<int*>(smem_batch);
    int* s_eo = s_no + (B + 1);
    int* s_ns = s_eo + (B + 1);
    int* s_es = s_ns + B;

    const int c = (B + T - 1) / T;                     // slots per thread, contiguous
    const int k0 = min(tid * c, B), k1 = min(k0 + c, B);
    long long nsum = 0, esum = 0;
    int bad = 0;
    for (int k = k0; k < k1; ++k) {
        int64_t g = a.ids[k];
        const bool ok = g >= 0 && g < a.G;
        bad |= ok ? 0 : 1;
        g = ok ? g : 0;
        const int64_t n0 = a.node_ptr[g], n1 = a.node_ptr[g + 1], e0 = a.edge_ptr[g], e1 = a.edge_ptr[g + 1];
        s_ns[k] = (int)n0; s_es[k] = (int)e0;
        s_no[k] = (int)min(nsum, 2147483647LL); s_eo[k] = (int)min(esum, 2147483647LL);     // (thread-local; the base is added below)
        nsum += ok ? n1 - n0 : 0; esum += ok ? e1 - e0 : 0;
    }
    long long ni = nsum, ei = esum;                    // inclusive scan of the thread sums: per wave by shuffles, the waves through LDS
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long vn = __shfl_up(ni, o), ve = __shfl_up(ei, o);
        if ((tid & 63) >= o) { ni += vn; ei += ve; }
    }
    if ((tid & 63) == 63) { s_part[0][tid >> 6] = ni; s_part[1][tid >> 6] = ei; }
    __syncthreads();
    long long nb = ni - nsum, eb = ei - esum, ntot = 0, etot = 0;
#pragma unroll
    for (int w = 0; w < T / 64; ++w) {
        if (w < (tid >> 6)) { nb += s_part[0][w]; eb += s_part[1][w]; }
        ntot += s_part[0][w]; etot += s_part[1][w];
    }
    for (int k = k0; k < k1; ++k) {
        s_no[k] = (int)min(nb + s_no[k], 2147483647LL);
        s_eo[k] = (int)min(eb + s_eo[k], 2147483647LL);
    }
    if (tid == 0) { s_no[B] = (int)min(ntot, 2147483647LL); s_eo[B] = (int)min(etot, 2147483647LL); }
    const int any_bad = __syncthreads_or(bad);         // (also the barrier that publishes the offsets)
    if (blockIdx.x == 0 && tid == 0) {                 // every workgroup reaches the same verdict: one of them reports it
        a.flags[0] = any_bad ? 1 : 0;
        a.flags[1] = (ntot != (long long)a.N || etot != (long long)a.E) ? 1 : 0;
    }

    const long b_node = a.s_x, b_edge = b_node + a.s_node, b_ea = b_edge + a.s_edge, b_y = b_ea + a.s_ea, b_ptr = b_y + a.s_y;
    const long total = b_ptr + a.s_ptr;
    // With a flagged input (an id outside [0, G), totals that differ from the host's figures) every index written below is still
    // INSIDE the batch -- values are clamped to N - 1 / E - 1 / E, items past the scanned totals get fillers -- so neither this
    // kernel nor the model kernels that run before the host looks at the flags can touch memory outside their buffers.  On a
    // valid input no clamp ever binds.
    const int Nm1 = max(a.N - 1, 0), Em1 = max(a.E - 1, 0);
    for (long w = blockIdx.x * (long)T + tid; w < total; w += (long)gridDim.x * T) {
        if (w < b_node) {                                                   // x: unit u of row i
            const int i = (int)(w / a.x_upr);
            const int k = find_slot(s_no, B, i);
            if (k >= 0) copy_unit(a.x, a.x_all, a.x_unit, w, w + (long)(s_ns[k] - s_no[k]) * a.x_upr);
        } else if (w < b_edge) {                                            // node i (i == N: the closing row pointer)
            const int i = (int)(w - b_node);
            if (i == a.N) {
                if (a.rowptr) { a.rowptr[i] = a.E; a.rowptr_t[i] = a.E; }
                continue;
            }
            const int k = find_slot(s_no, B, i);
            a.batch[i] = k >= 0 ? k : B - 1;
            if (a.rowptr) {
                int r = min(s_eo[B], a.E), rt = r;                          // (a row past the scanned total: empty, behind the last real one)
                if (k >= 0) {
                    const long j = (long)i + (s_ns[k] - s_no[k]);
                    const int de = s_eo[k] - s_es[k];
                    r = min(a.R[j] + de, a.E); rt = min(a.Rt[j] + de, a.E);
                }
                a.rowptr[i] = r; a.rowptr_t[i] = rt;
            }
        } else if (w < b_ea) {                                              // edge e
            const int e = (int)(w - b_edge);
            const int k = find_slot(s_eo, B, e);
            int64_t s = 0, d = 0;
            int cv = 0, pv = e, ctv = 0, ptv = e;                           // (an edge past the scanned total: a self loop of node 0)
            if (k >= 0) {
                const long j = (long)e + (s_es[k] - s_eo[k]);
                const int dn = s_no[k] - s_ns[k], de = s_eo[k] - s_es[k];
                s = min(a.src_all[j] + dn, (int64_t)Nm1); d = min(a.dst_all[j] + dn, (int64_t)Nm1);
                if (a.rowptr) {
                    cv = min(a.C[j] + dn, Nm1); pv = min(a.P[j] + de, Em1);
                    ctv = min(a.Ct[j] + dn, Nm1); ptv = min(a.Pt[j] + de, Em1);
                }
            }
            a.ei[e] = s; a.ei[(long)a.E + e] = d;
            if (a.rowptr) { a.col[e] = cv; a.perm[e] = pv; a.col_t[e] = ctv; a.perm_t[e] = ptv; }
        } else if (w < b_y) {                                               // edge_attr: unit u of row e
            const long u = w - b_ea;
            const int e = (int)(u / a.ea_upr);
            const int k = find_slot(s_eo, B, e);
            if (k >= 0) copy_unit(a.ea, a.ea_all, a.ea_unit, u, u + (long)(s_es[k] - s_eo[k]) * a.ea_upr);
        } else if (w < b_ptr) {                                             // y: unit u of graph slot k
            const long u = w - b_y;
            const int k = (int)(u / a.y_upr);
            const int64_t g = a.ids[k];
            if (g >= 0 && g < a.G) copy_unit(a.y, a.y_all, a.y_unit, u, u + (g - k) * a.y_upr);
        } else {                                                            // ptr[k], k = 0 .. B
            const int k = (int)(w - b_ptr);
            a.ptr[k] = min(s_no[k], a.N);
        }
    }
}

static int unit_of(const void* p, const void* q, long row_bytes) {
    const uintptr_t m = (uintptr_t)p | (uintptr_t)q | (uintptr_t)row_bytes;
    return (m & 15) == 0 ? 16 : (m & 7) == 0 ? 8 : 4;
}

int batch_assemble(const kagnn_batch_assemble_t* p, hipStream_t st) {
    BatchArgs a;
    a.node_ptr = p->node_ptr; a.edge_ptr = p->edge_ptr; a.ids = p->ids;
    a.G = (long)p->num_graphs_total; a.B = (int)p->num_graphs; a.N = (int)p->num_nodes; a.E = (int)p->num_edges;
    a.x_all = static_cast<const unsigned char*>(p->x_all); a.x = static_cast<unsigned char*>(p->x);
    a.ea_all = static_cast<const unsigned char*>(p->edge_attr_all); a.ea = static_cast<unsigned char*>(p->edge_attr);
    a.y_all = static_cast<const unsigned char*>(p->y_all); a.y = static_cast<unsigned char*>(p->y);
    a.x_unit = unit_of(a.x_all, a.x, p->x_row_bytes); a.x_upr = p->x_row_bytes / a.x_unit;
    a.ea_unit = a.ea ? unit_of(a.ea_all, a.ea, p->edge_attr_row_bytes) : 4; a.ea_upr = a.ea ? p->edge_attr_row_bytes / a.ea_unit : 1;
    a.y_unit = a.y ? unit_of(a.y_all, a.y, p->y_row_bytes) : 4; a.y_upr = a.y ? p->y_row_bytes / a.y_unit : 1;
    a.src_all = p->src_all; a.dst_all = p->dst_all;
    a.R = p->rowptr_all; a.C = p->col_all; a.P = p->perm_all; a.Rt = p->rowptr_t_all; a.Ct = p->col_t_all; a.Pt = p->perm_t_all;
    a.ei = p->edge_index; a.batch = p->batch; a.ptr = p->ptr;
    a.rowptr = p->rowptr; a.col = p->col; a.perm = p->perm; a.rowptr_t = p->rowptr_t; a.col_t = p->col_t; a.perm_t = p->perm_t;
    a.flags = p->flags;
    a.s_x = (long)a.N * a.x_upr; a.s_node = (long)a.N + 1; a.s_edge = a.E;
    a.s_ea = a.ea ? (long)a.E * a.ea_upr : 0; a.s_y = a.y ? (long)a.B * a.y_upr : 0; a.s_ptr = (long)a.B + 1;
    const long total = a.s_x + a.s_node + a.s_edge + a.s_ea + a.s_y + a.s_ptr;
    const int blocks = (int)min((total + kBatchThreads - 1) / kBatchThreads, (long)kBatchMaxBlocks);
    const size_t lds = (size_t)(4 * a.B + 2) * sizeof(int);
    if (lds > 48 * 1024) {
        static unsigned long long configured = 0;          // (per device: common.h)
        if (auto first_use_ = first_use_on_this_device(configured))
            KAGNN_HIP(hipFuncSetAttribute((const void*)batch_assemble_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)((4 * KAGNN_BATCH_MAX_GRAPHS + 2) * sizeof(int))));
    }
    batch_assemble_kernel<<<blocks, kBatchThreads, lds, st>>>(a);
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

}  // namespace kagnn

using namespace kagnn;

#pragma GCC visibility push(default)
extern "C" {

int kagnn_batch_assemble_struct_bytes(void) { return (int)sizeof(kagnn_batch_assemble_t); }

int kagnn_batch_assemble(const kagnn_batch_assemble_t* a, void* stream) {
    KAGNN_CHECK_ARG(a != nullptr, "the argument struct is null");
    if (a->struct_bytes != (int64_t)sizeof(kagnn_batch_assemble_t))
        return fail(KAGNN_ERR_ARG, "%s: struct_bytes is %ld, this library's kagnn_batch_assemble_t has %ld (header mismatch)", __func__,
                    (long)a->struct_bytes, (long)sizeof(kagnn_batch_assemble_t));
    if (a->num_graphs > KAGNN_BATCH_MAX_GRAPHS)
        return fail(KAGNN_ERR_UNSUPPORTED, "%s: %ld graphs in one batch; the limit is KAGNN_BATCH_MAX_GRAPHS = %ld", __func__,
                    (long)a->num_graphs, (long)KAGNN_BATCH_MAX_GRAPHS);
    KAGNN_CHECK_ARG(a->num_graphs >= 1 && a->num_graphs_total >= 1, "no graphs");
    KAGNN_CHECK_ARG(a->num_nodes >= 0 && a->num_edges >= 0 && a->num_nodes < 2147483647LL && a->num_edges < 2147483647LL,
                    "num_nodes and num_edges must fit int32");
    KAGNN_CHECK_ARG(a->num_edges == 0 || a->num_nodes > 0, "edges without nodes");
    KAGNN_CHECK_ARG(a->node_ptr && a->edge_ptr && a->ids && (a->num_nodes == 0 || a->batch) && a->ptr && a->flags, "null array");
    KAGNN_CHECK_ARG(a->x_row_bytes >= 4 && a->x_row_bytes % 4 == 0 && a->edge_attr_row_bytes % 4 == 0 && a->y_row_bytes % 4 == 0 &&
                    a->edge_attr_row_bytes >= 0 && a->y_row_bytes >= 0, "row sizes must be multiples of 4 bytes");
    KAGNN_CHECK_ARG(a->x_all && (a->num_nodes == 0 || a->x), "x is null");
    KAGNN_CHECK_ARG(a->num_edges == 0 || (a->src_all && a->dst_all && a->edge_index), "null edge arrays");
    KAGNN_CHECK_ARG((a->edge_attr_all != nullptr) == (a->edge_attr_row_bytes > 0) && (a->y_all != nullptr) == (a->y_row_bytes > 0),
                    "an optional array and its row size must be given together");
    KAGNN_CHECK_ARG(!a->edge_attr_all || a->num_edges == 0 || a->edge_attr, "edge_attr output is null");
    KAGNN_CHECK_ARG(!a->y_all || a->y, "y output is null");
    const bool csr_in = a->rowptr_all && a->col_all && a->perm_all && a->rowptr_t_all && a->col_t_all && a->perm_t_all;
    const bool csr_any = a->rowptr || a->col || a->perm || a->rowptr_t || a->col_t || a->perm_t;
    const bool csr_out = a->rowptr && a->rowptr_t && (a->num_edges == 0 || (a->col && a->perm && a->col_t && a->perm_t));
    KAGNN_CHECK_ARG(!csr_any || (csr_in && csr_out), "the CSR arrays are optional as a group: all six of the dataset and all six outputs, or no output");
    const uintptr_t align = (uintptr_t)a->x_all | (uintptr_t)a->x | (uintptr_t)a->edge_attr_all | (uintptr_t)a->edge_attr |
                            (uintptr_t)a->y_all | (uintptr_t)a->y;
    KAGNN_CHECK_ARG((align & 3) == 0, "x / edge_attr / y must be 4-byte aligned");
    return batch_assemble(a, as_stream(stream));
}

}
#pragma GCC visibility pop
