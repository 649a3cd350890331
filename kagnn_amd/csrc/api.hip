// extern "C" surface of libkagnn_hip.so (declared in include/kagnn_hip.h): argument validation
// and dispatch only -- the kernels live in the sibling .hip files, the host orchestration of the fused layer, stack and model
// calls in fused_calls.hip.
#include "host.h"
#include <mutex>
#include <string>
#include <vector>

namespace kagnn {
thread_local char g_err[512] = "";
thread_local bool g_half_products = false;      // KAGNN_PREC_HALF for the duration of an entry-point call (split_common.h)

// ---------------------------------------------------------------- stage timer (host.h: StageScope)
namespace {
struct StageRecord { const char* name; hipEvent_t a, b; int dev; };
constexpr int kStageMaxDevices = 64;
struct StageTimer {
    std::mutex mu;
    bool on = false;
    std::string only;                       // empty: every stage
    std::vector<StageRecord> rec;
    // events of earlier sessions, reused -- PER DEVICE: an event belongs to the device that was current when it was created, and
    // recording it on another device's stream fails (the ignored error used to show up as 0 ms timings: ADVICE r04)
    std::vector<hipEvent_t> pool[kStageMaxDevices];
} g_stage;
thread_local int g_stage_depth = 0;         // nested entry points (fwd_moments -> fwd): only the outermost is a stage
constexpr size_t kStageMaxRecords = 1u << 16;
}  // namespace

StageScope::StageScope(const char* nm, void* stream) : st(as_stream(stream)), name(nm) {
    const bool outer = g_stage_depth++ == 0;
    if (!outer || !g_stage.on) return;              // (unlocked read of a flag that only bench.py toggles, between steps)
    std::lock_guard<std::mutex> lk(g_stage.mu);
    if (!g_stage.on || (!g_stage.only.empty() && g_stage.only != nm) || g_stage.rec.size() >= kStageMaxRecords) return;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kStageMaxDevices) return;
    std::vector<hipEvent_t>& pool = g_stage.pool[dev];
    hipEvent_t ev[2] = {nullptr, nullptr};
    for (int i = 0; i < 2; ++i) {
        if (!pool.empty()) { ev[i] = pool.back(); pool.pop_back(); }
        else if (hipEventCreate(&ev[i]) != hipSuccess) {
            (void)hipGetLastError();
            if (i == 1) pool.push_back(ev[0]);      // a partial failure must not leak the first event
            return;
        }
    }
    (void)hipEventRecord(ev[0], st);
    b = ev[1];
    g_stage.rec.push_back(StageRecord{nm, ev[0], ev[1], dev});
}
StageScope::~StageScope() {
    --g_stage_depth;
    if (b) (void)hipEventRecord(b, st);
}

// the body of kagnn_kan_linear_bwd_weight_affine (x_affine: as kagnn_kan_linear_bwd_input_affine -- the weight gradient of a layer
// whose input is a folded BatchNorm1d output), plus the deferral record of a stack call (host.h)
int kan_linear_bwd_weight(const float* x, int64_t ldx, const float* x_affine, const float* gy, int64_t ldgy, int64_t N, const float* knots,
                          int32_t in, int32_t out, int32_t G, int32_t K, int32_t mode, const float* sw, const float* sc, float* g_bw,
                          float* g_sw, float* g_sc, void* ws, size_t ws_bytes, void* stream, DwDefer* defer) {
    static const char fn[] = "kagnn_kan_linear_bwd_weight_affine";
    ModeScope mode_scope_(mode);
    KAGNN_STAGE_AS("kagnn_kan_linear_bwd_weight", stream);
    int rc = check_kan_dims_wide(fn, in, out, G, K, mode);
    if (rc) return rc;
    KAGNN_CHECK_ARG_AS(fn, N >= 0 && ldx >= in && ldgy >= out, "bad shape");
    KAGNN_CHECK_ARG_AS(fn, knots && sw && g_sw && ws, "null array");          // g_base_weight NULL: not wanted
    KAGNN_CHECK_ARG_AS(fn, N == 0 || (x && gy), "null array");
    KAGNN_CHECK_ARG_AS(fn, (sc == nullptr) == (g_sc == nullptr), "spline_scaler and its gradient must both be given or both be null");
    if (use_split_dw(in, out, G, K, mode)) {
        if (!(fits32(N, ldx) && fits32(N, ldgy))) return fail(KAGNN_ERR_UNSUPPORTED, "%s: leading dimension > 7680 floats; call with KAGNN_PREC_FP32", fn);
        return kan_split_dw(x, ldx, gy, ldgy, N, knots, in, out, G, K, sw, sc, g_bw, g_sw, g_sc, (float*)ws, ws_bytes, as_stream(stream), x_affine, defer);
    }
    if (x_affine) return fail(KAGNN_ERR_UNSUPPORTED, "%s: an input affine is applied by the split-precision kernels only", fn);
    if (high_order(K))
        return kan_ho_dw(x, ldx, gy, ldgy, N, knots, in, out, G, K, sw, sc, g_bw, g_sw, g_sc, (float*)ws, ws_bytes, mode == KAGNN_PREC_FP32_GRID, as_stream(stream));
    return kan_f32_dw(x, ldx, gy, ldgy, N, knots, in, out, G, K, sw, sc, g_bw, g_sw, g_sc, (float*)ws, ws_bytes, mode == KAGNN_PREC_FP32_GRID, as_stream(stream));
}
}  // namespace kagnn

using namespace kagnn;


#pragma GCC visibility push(default)
extern "C" {

int kagnn_version(void) { return 281; }
const char* kagnn_last_error(void) { return g_err; }

int kagnn_stage_timer_enable(const char* only) {
    std::lock_guard<std::mutex> lk(g_stage.mu);
    g_stage.only = only ? only : "";
    g_stage.on = true;
    return KAGNN_OK;
}

int kagnn_stage_timer_disable(void) {
    std::lock_guard<std::mutex> lk(g_stage.mu);
    g_stage.on = false;
    return KAGNN_OK;
}

// Aggregates the records taken so far by stage name (waits for their events), hands the events back to the pool and clears
// the records.  names: caller's array of `capacity` char[64] slots; returns the number of distinct stages through *n_stages.
int kagnn_stage_timer_collect(char* names, int64_t* launches, double* total_ms, int32_t capacity, int32_t* n_stages) {
    KAGNN_CHECK_ARG(names && launches && total_ms && n_stages && capacity >= 1, "null output");
    std::lock_guard<std::mutex> lk(g_stage.mu);
    int n = 0;
    for (const StageRecord& r : g_stage.rec) {
        float ms = 0.0f;
        if (hipEventSynchronize(r.b) != hipSuccess || hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) {
            (void)hipGetLastError();
            ms = 0.0f;
        }
        g_stage.pool[r.dev].push_back(r.a);             // (before any `continue`: a record beyond `capacity` used to leak its events)
        g_stage.pool[r.dev].push_back(r.b);
        int k = 0;
        while (k < n && strncmp(names + 64 * k, r.name, 63) != 0) ++k;
        if (k == n) {
            if (n == capacity) continue;
            strncpy(names + 64 * n, r.name, 63);
            names[64 * n + 63] = 0;
            launches[n] = 0; total_ms[n] = 0.0;
            ++n;
        }
        launches[k] += 1;
        total_ms[k] += ms;
    }
    g_stage.rec.clear();
    *n_stages = n;
    return KAGNN_OK;
}

int kagnn_csr_workspace_bytes(int64_t E, int64_t N, size_t* bytes) {
    KAGNN_CHECK_ARG(bytes != nullptr && E >= 0 && N >= 0, "null output or negative size");
    KAGNN_CHECK_ARG(E < 2147483647LL && N < 2147483647LL, "N and E must fit int32");
    return csr_workspace_bytes(E, N, bytes);
}

int kagnn_csr_build(const int64_t* key, const int64_t* val, int64_t E, int64_t N, int32_t* rowptr,
                    int32_t* col, int32_t* perm, int32_t hub_threshold, int32_t* hub_seg,
                    int64_t hub_seg_capacity, int64_t* num_hub_seg_host, void* ws, size_t ws_bytes,
                    void* stream) {
    KAGNN_CHECK_ARG(E >= 0 && N >= 0 && E < 2147483647LL && N < 2147483647LL, "N and E must fit int32");
    KAGNN_CHECK_ARG(rowptr != nullptr, "rowptr is null");
    KAGNN_CHECK_ARG(E == 0 || (key && val && col && perm && ws), "null array");
    return csr_build(key, val, E, N, rowptr, col, perm, hub_threshold, hub_seg, hub_seg_capacity,
                     num_hub_seg_host, ws, ws_bytes, as_stream(stream));
}

int kagnn_csr_small_ok(int64_t E, int64_t N) { return csr_small_ok(E, N) ? 1 : 0; }

int kagnn_csr_small_workspace_bytes(int64_t E, size_t* bytes) {
    KAGNN_CHECK_ARG(bytes != nullptr && E >= 0, "null output or negative size");
    *bytes = csr_small_workspace_bytes(E);
    return KAGNN_OK;
}

int kagnn_csr_build_small(const int64_t* src, const int64_t* dst, int64_t E, int64_t N, int32_t* rowptr, int32_t* col, int32_t* perm,
                          int32_t* rowptr_t, int32_t* col_t, int32_t* perm_t, int32_t* flags, void* ws, size_t ws_bytes, void* stream) {
    KAGNN_CHECK_ARG(src && dst && rowptr && col && perm && rowptr_t && col_t && perm_t && flags && ws, "null array");
    return csr_build_small(src, dst, E, N, rowptr, col, perm, rowptr_t, col_t, perm_t, flags, ws, ws_bytes, as_stream(stream));
}

int kagnn_subgraph_workspace_bytes(int64_t N, int64_t E, size_t* bytes) {
    KAGNN_CHECK_ARG(bytes != nullptr && E >= 0 && N >= 0, "null output or negative size");
    KAGNN_CHECK_ARG(E < 2147483647LL && N < 2147483647LL, "N and E must fit int32");
    return subgraph_workspace_bytes(N, E, bytes);
}

int kagnn_k_hop_mark(const int32_t* rowptr, const int32_t* col, int64_t N, const int64_t* seeds, int64_t num_seeds, int32_t num_hops,
                     int32_t* hop, int32_t* flags, void* stream) {
    KAGNN_CHECK_ARG(N >= 0 && N < 2147483647LL && num_seeds >= 0 && num_seeds < 2147483647LL, "num_nodes and num_seeds must fit int32");
    KAGNN_CHECK_ARG(num_hops >= 0, "num_hops is negative");
    KAGNN_CHECK_ARG(flags != nullptr && (N == 0 || hop) && (num_seeds == 0 || seeds), "null array");
    KAGNN_CHECK_ARG(N == 0 || num_seeds == 0 || num_hops == 0 || rowptr, "null CSR array");      // (col: NULL for a graph without edges)
    return k_hop_mark(rowptr, col, N, seeds, num_seeds, num_hops, hop, flags, as_stream(stream));
}

int kagnn_subgraph_count(const int32_t* hop, const int32_t* rowptr, const int32_t* col, const int32_t* perm, const int32_t* rowptr_t,
                         const int32_t* col_t, const int32_t* perm_t, int64_t N, int64_t E, void* ws, size_t ws_bytes, int32_t* counts,
                         void* stream) {
    (void)perm_t;                                              // (the kept edges in original order come from the by-destination side)
    KAGNN_CHECK_ARG(N >= 0 && E >= 0 && E < 2147483647LL && N < 2147483647LL, "N and E must fit int32");
    KAGNN_CHECK_ARG(E == 0 || N > 0, "edges without nodes");
    KAGNN_CHECK_ARG(counts != nullptr && ws != nullptr, "null array");
    KAGNN_CHECK_ARG(N == 0 || (hop && rowptr && rowptr_t), "null array");
    KAGNN_CHECK_ARG(E == 0 || (col && perm && col_t), "null CSR array");
    return subgraph_count(hop, rowptr, col, perm, rowptr_t, col_t, N, E, ws, ws_bytes, counts, as_stream(stream));
}

int kagnn_subgraph_fill(const void* ws, size_t ws_bytes, const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                        const int32_t* rowptr_t, const int32_t* col_t, const int32_t* perm_t, int64_t N, int64_t E, int64_t n_sub,
                        int64_t e_sub, int64_t* nodes, int64_t* edge_ids, int64_t* edge_index_sub, int32_t* rowptr_sub, int32_t* col_sub,
                        int32_t* perm_sub, int32_t* rowptr_t_sub, int32_t* col_t_sub, int32_t* perm_t_sub, void* stream) {
    KAGNN_CHECK_ARG(N >= 0 && E >= 0 && E < 2147483647LL && N < 2147483647LL, "N and E must fit int32");
    KAGNN_CHECK_ARG(n_sub >= 0 && n_sub <= N && e_sub >= 0 && e_sub <= E && (e_sub == 0 || n_sub > 0), "n_sub / e_sub outside the parent's sizes");
    KAGNN_CHECK_ARG(ws != nullptr && rowptr_sub && rowptr_t_sub, "null array");
    KAGNN_CHECK_ARG(n_sub == 0 || (rowptr && rowptr_t && nodes), "null array");
    KAGNN_CHECK_ARG(n_sub == 0 || E == 0 || (col && perm && col_t && perm_t), "null CSR array");
    KAGNN_CHECK_ARG(e_sub == 0 || (edge_ids && edge_index_sub && col_sub && perm_sub && col_t_sub && perm_t_sub), "null output");
    return subgraph_fill(ws, ws_bytes, rowptr, col, perm, rowptr_t, col_t, perm_t, N, E, n_sub, e_sub, nodes, edge_ids, edge_index_sub,
                         rowptr_sub, col_sub, perm_sub, rowptr_t_sub, col_t_sub, perm_t_sub, as_stream(stream));
}

int kagnn_neighbor_sample_mark(const int32_t* rowptr, const int32_t* col, const int32_t* perm, int64_t N, int64_t E, const int64_t* seeds,
                               int64_t num_seeds, const int32_t* fanout_host, int32_t num_levels, uint64_t seed, int32_t* hop, uint8_t* keep,
                               int32_t* flags, void* stream) {
    KAGNN_CHECK_ARG(N >= 0 && N < 2147483647LL && E >= 0 && E < 2147483647LL && num_seeds >= 0 && num_seeds < 2147483647LL,
                    "num_nodes, num_edges and num_seeds must fit int32");
    KAGNN_CHECK_ARG(E == 0 || N > 0, "edges without nodes");
    KAGNN_CHECK_ARG(num_levels >= 1 && num_levels <= KAGNN_SAMPLE_MAX_LEVELS && fanout_host, "num_levels outside 1..16, or no fan-outs");
    for (int d = 0; d < num_levels; ++d) KAGNN_CHECK_ARG(fanout_host[d] >= -1, "a fanout below -1");
    KAGNN_CHECK_ARG(flags != nullptr && (N == 0 || hop) && (E == 0 || keep) && (num_seeds == 0 || seeds), "null array");
    KAGNN_CHECK_ARG(E == 0 || num_seeds == 0 || (rowptr && col && perm), "null CSR array");
    return neighbor_sample_mark(rowptr, col, perm, N, E, seeds, num_seeds, fanout_host, num_levels, seed, hop, keep, flags, as_stream(stream));
}

int kagnn_edge_subgraph_count(const int32_t* hop, const uint8_t* keep, const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                              const int32_t* rowptr_t, const int32_t* col_t, const int32_t* perm_t, int64_t N, int64_t E, void* ws,
                              size_t ws_bytes, int32_t* counts, void* stream) {
    KAGNN_CHECK_ARG(N >= 0 && E >= 0 && E < 2147483647LL && N < 2147483647LL, "N and E must fit int32");
    KAGNN_CHECK_ARG(E == 0 || N > 0, "edges without nodes");
    KAGNN_CHECK_ARG(counts != nullptr && ws != nullptr, "null array");
    KAGNN_CHECK_ARG(N == 0 || (hop && rowptr && rowptr_t), "null array");
    KAGNN_CHECK_ARG(E == 0 || (keep && col && perm && col_t && perm_t), "null CSR array");
    // (keep may be NULL at E == 0, where both forms of the subgraph agree)
    return edge_subgraph_count(hop, keep, rowptr, col, perm, rowptr_t, col_t, perm_t, N, E, ws, ws_bytes, counts,
                               as_stream(stream));
}

int kagnn_edge_subgraph_fill(const void* ws, size_t ws_bytes, const uint8_t* keep, const int32_t* rowptr, const int32_t* col,
                             const int32_t* perm, const int32_t* rowptr_t, const int32_t* col_t, const int32_t* perm_t, int64_t N, int64_t E,
                             int64_t n_sub, int64_t e_sub, int64_t* nodes, int64_t* edge_ids, int64_t* edge_index_sub, int32_t* rowptr_sub,
                             int32_t* col_sub, int32_t* perm_sub, int32_t* rowptr_t_sub, int32_t* col_t_sub, int32_t* perm_t_sub,
                             void* stream) {
    KAGNN_CHECK_ARG(N >= 0 && E >= 0 && E < 2147483647LL && N < 2147483647LL, "N and E must fit int32");
    KAGNN_CHECK_ARG(n_sub >= 0 && n_sub <= N && e_sub >= 0 && e_sub <= E && (e_sub == 0 || n_sub > 0), "n_sub / e_sub outside the parent's sizes");
    KAGNN_CHECK_ARG(ws != nullptr && rowptr_sub && rowptr_t_sub, "null array");
    KAGNN_CHECK_ARG(n_sub == 0 || (rowptr && rowptr_t && nodes), "null array");
    KAGNN_CHECK_ARG(n_sub == 0 || E == 0 || (keep && col && perm && col_t && perm_t), "null CSR array");
    KAGNN_CHECK_ARG(e_sub == 0 || (edge_ids && edge_index_sub && col_sub && perm_sub && col_t_sub && perm_t_sub), "null output");
    return edge_subgraph_fill(ws, ws_bytes, keep, rowptr, col, perm, rowptr_t, col_t, perm_t, N, E, n_sub, e_sub, nodes,
                              edge_ids, edge_index_sub, rowptr_sub, col_sub, perm_sub, rowptr_t_sub, col_t_sub, perm_t_sub,
                              as_stream(stream));
}

// link prediction around an encoder (linkpred.hip)
int kagnn_edge_keys_workspace_bytes(int64_t E, size_t* bytes) {
    KAGNN_CHECK_ARG(bytes != nullptr && E >= 0 && E < 2147483647LL, "null output, or num_edges outside [0, 2^31)");
    *bytes = edge_keys_ws_bytes(E);
    return KAGNN_OK;
}

int kagnn_edge_keys_build(const int64_t* src, const int64_t* dst, int64_t E, int64_t N, int64_t* keys, int64_t* num_keys, void* ws,
                          size_t ws_bytes, void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(E >= 0 && E < 2147483647LL && N >= 0 && N < 2147483648LL, "num_edges and num_nodes must lie below 2^31");
    KAGNN_CHECK_ARG(E == 0 || N > 0, "edges without nodes");
    KAGNN_CHECK_ARG(num_keys != nullptr && (E == 0 || (src && dst && keys && ws)), "null array");
    return edge_keys_build(src, dst, E, N, keys, num_keys, ws, ws_bytes, as_stream(stream));
}

int kagnn_negative_sample(const int64_t* keys, int64_t num_keys, int64_t N, int64_t num, uint64_t seed, int32_t attempts, int64_t* pairs,
                          uint8_t* valid, void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(attempts >= 1 && attempts <= KAGNN_NEGATIVE_MAX_ATTEMPTS, "attempts must be 1..32");
    KAGNN_CHECK_ARG(num >= 0 && num < (1LL << 32) && 2 * num * (int64_t)attempts < (1LL << 32), "2 * num * attempts must lie below 2^32");
    KAGNN_CHECK_ARG(N >= 0 && N < 2147483648LL && num_keys >= 0, "num_nodes must lie in [0, 2^31), num_keys >= 0");
    if (num == 0 || N == 0) return KAGNN_OK;
    KAGNN_CHECK_ARG(pairs && valid && (num_keys == 0 || keys), "null array");
    return negative_sample(keys, num_keys, N, num, seed, attempts, pairs, valid, as_stream(stream));
}

int kagnn_bce_logits_fwd(const float* scores, const uint8_t* labels, const uint8_t* weight, int64_t P, float* loss, int64_t* divisor,
                         void* record, void* ws, size_t ws_bytes, void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(P >= 0 && loss && divisor && (P == 0 || (scores && labels)), "null array or negative size");
    KAGNN_CHECK_ARG((((uintptr_t)record | (uintptr_t)divisor) & 7) == 0, "the record and the divisor must be 8-byte aligned");
    return bce_logits_fwd(scores, labels, weight, P, loss, divisor, record, ws, ws_bytes, as_stream(stream));
}

int kagnn_bce_logits_bwd(const float* scores, const uint8_t* labels, const uint8_t* weight, int64_t P, const int64_t* divisor,
                         const float* g_loss, float* g_scores, void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(P >= 0 && (P == 0 || (scores && labels && divisor && g_loss && g_scores)), "null array or negative size");
    return bce_logits_bwd(scores, labels, weight, P, divisor, g_loss, g_scores, as_stream(stream));
}

int kagnn_link_rank_workspace_bytes(int64_t P, size_t* bytes) {
    KAGNN_CHECK_ARG(bytes != nullptr && P >= 0 && P < 2147483647LL, "null output, or num_rows outside [0, 2^31 - 1)");
    *bytes = link_rank_ws_bytes(P);
    return KAGNN_OK;
}

int kagnn_link_rank(const float* scores, const uint8_t* labels, const uint8_t* weight, int64_t P, const int32_t* ks_host, int32_t num_ks,
                    int64_t* record, void* ws, size_t ws_bytes, void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(P >= 0 && P < 2147483647LL, "num_rows outside [0, 2^31 - 1)");
    KAGNN_CHECK_ARG(num_ks >= 0 && num_ks <= 3 && (num_ks == 0 || ks_host), "at most 3 values of k, in a host array");
    for (int j = 0; j < num_ks; ++j) KAGNN_CHECK_ARG(ks_host[j] >= 1, "a k below 1");
    KAGNN_CHECK_ARG(record && ((uintptr_t)record & 7) == 0 && (P == 0 || (scores && labels)), "null array or misaligned record");
    return link_rank(scores, labels, weight, P, ks_host, num_ks, record, ws, ws_bytes, as_stream(stream));
}

int kagnn_gcn_deg_inv_sqrt(const int32_t* rowptr, const int32_t* col, int64_t N, float* dis, void* stream) {
    KAGNN_CHECK_ARG(N >= 0 && rowptr && dis, "null array");
    return gcn_deg_inv_sqrt(rowptr, col, N, dis, as_stream(stream));
}

int kagnn_aggregate_sum_add(const float* x, int64_t ldx, float* out, int64_t ldo, const int32_t* rowptr,
                            const int32_t* col, const float* edge_weight, int64_t N, int32_t F,
                            float self_scale, const float* in_scale, const float* out_scale,
                            const float* bias, int32_t skip_self_loops, const int32_t* hub_seg,
                            int64_t num_hub_seg, int32_t hub_threshold, const float* addend, int64_t ld_addend,
                            void* workspace, size_t workspace_bytes, void* stream) {
    KAGNN_STAGE_AS("kagnn_aggregate_sum", stream);
    KAGNN_CHECK_ARG(N >= 0 && F >= 1, "bad shape");
    KAGNN_CHECK_ARG(N == 0 || (x && out && rowptr), "null array");
    KAGNN_CHECK_ARG(ldx >= F && ldo >= F && (!addend || ld_addend >= F), "leading dimension smaller than num_feat");
    KAGNN_CHECK_ARG(x != out, "in-place aggregation is not supported");
    AggArgs a{x, ldx, out, ldo, rowptr, col, edge_weight, N, F, self_scale, in_scale, out_scale, bias,
              skip_self_loops, hub_threshold > 0 ? hub_threshold : 0x7fffffff, addend, ld_addend};
    return aggregate_sum(a, hub_seg, num_hub_seg, static_cast<float*>(workspace), workspace_bytes, as_stream(stream));
}

int kagnn_aggregate_sum(const float* x, int64_t ldx, float* out, int64_t ldo, const int32_t* rowptr,
                        const int32_t* col, const float* edge_weight, int64_t N, int32_t F,
                        float self_scale, const float* in_scale, const float* out_scale,
                        const float* bias, int32_t skip_self_loops, const int32_t* hub_seg,
                        int64_t num_hub_seg, int32_t hub_threshold, void* workspace, size_t workspace_bytes,
                        void* stream) {
    return kagnn_aggregate_sum_add(x, ldx, out, ldo, rowptr, col, edge_weight, N, F, self_scale, in_scale, out_scale, bias,
                                   skip_self_loops, hub_seg, num_hub_seg, hub_threshold, nullptr, 0, workspace, workspace_bytes, stream);
}

// GIN-form aggregation of a matrix that exists only as  col_scale[c] * x[.][c] + col_shift[c]  -- the output of a training-mode
// BatchNorm1d whose normalising pass is folded into the aggregation that gathers it (reference node_classification_clean/
// models.py:198-200, `x = self.bns[i](self.convs[i](x, edge_index))` feeding the next GINConv):
//   out_i = col_scale * (self_scale * x_i + sum_{j->i} x_j) + (self_scale + deg_i) * col_shift   [+ addend_i]
// Unit edge weights (no edge_weight / in_scale / out_scale / bias / skip_self_loops).  col_scale / col_shift: F floats each.
int kagnn_aggregate_sum_affine(const float* x, int64_t ldx, float* out, int64_t ldo, const int32_t* rowptr, const int32_t* col,
                               int64_t N, int32_t F, float self_scale, const float* col_scale, const float* col_shift,
                               const int32_t* hub_seg, int64_t num_hub_seg, int32_t hub_threshold, const float* addend,
                               int64_t ld_addend, void* workspace, size_t workspace_bytes, void* stream) {
    KAGNN_STAGE_AS("kagnn_aggregate_sum", stream);
    KAGNN_CHECK_ARG(N >= 0 && F >= 1, "bad shape");
    KAGNN_CHECK_ARG(N == 0 || (x && out && rowptr), "null array");
    KAGNN_CHECK_ARG(ldx >= F && ldo >= F && (!addend || ld_addend >= F), "leading dimension smaller than num_feat");
    KAGNN_CHECK_ARG(x != out, "in-place aggregation is not supported");
    KAGNN_CHECK_ARG((col_scale == nullptr) == (col_shift == nullptr), "col_scale and col_shift must both be given or both be null");
    AggArgs a{x, ldx, out, ldo, rowptr, col, nullptr, N, F, self_scale, nullptr, nullptr, nullptr,
              0, hub_threshold > 0 ? hub_threshold : 0x7fffffff, addend, ld_addend};
    a.col_scale = col_scale; a.col_shift = col_shift;
    return aggregate_sum(a, hub_seg, num_hub_seg, static_cast<float*>(workspace), workspace_bytes, as_stream(stream));
}

// d loss / d edge_weight of kagnn_aggregate_sum (aggregate_edge.hip): one value per CSR position, written to ORIGINAL edge order
// through `perm` (NULL: CSR order).  fp32 only.
int kagnn_aggregate_edge_grad(const float* x, int64_t ldx, const float* gout, int64_t ldg, const int32_t* rowptr, const int32_t* col,
                              const int32_t* perm, int64_t N, int64_t E, int32_t F, const float* in_scale, const float* out_scale,
                              int32_t skip_self_loops, const int32_t* hub_seg, int64_t num_hub_seg, int32_t hub_threshold,
                              float* g_edge_weight, void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(N >= 0 && E >= 0 && F >= 1 && N < 2147483647LL && E < 2147483647LL && num_hub_seg >= 0, "bad shape");
    KAGNN_CHECK_ARG(ldx >= F && ldg >= F, "leading dimension smaller than num_feat");
    if (N == 0 || E == 0) return KAGNN_OK;
    KAGNN_CHECK_ARG(x && gout && rowptr && col && g_edge_weight, "null array");
    KAGNN_CHECK_ARG(num_hub_seg == 0 || hub_seg, "hub segments counted but not given");
    EdgeGradArgs a{x, ldx, gout, ldg, rowptr, col, perm, N, E, F, in_scale, out_scale, skip_self_loops,
                   hub_threshold > 0 ? hub_threshold : 0x7fffffff, g_edge_weight};
    return aggregate_edge_grad(a, hub_seg, num_hub_seg, as_stream(stream));
}

int kagnn_aggregate_sum_bf16(const void* x, int64_t ldx, void* out, int64_t ldo, int32_t out_dtype, const int32_t* rowptr,
                             const int32_t* col, const float* edge_weight, int64_t N, int32_t F, float self_scale,
                             const float* in_scale, const float* out_scale, const float* bias, int32_t skip_self_loops,
                             const int32_t* hub_seg, int64_t num_hub_seg, int32_t hub_threshold, void* workspace,
                             size_t workspace_bytes, void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(N >= 0 && F >= 1, "bad shape");
    KAGNN_CHECK_ARG(N == 0 || (x && out && rowptr), "null array");
    KAGNN_CHECK_ARG(ldx >= F && ldo >= F, "leading dimension smaller than num_feat");
    KAGNN_CHECK_ARG(out_dtype == KAGNN_DTYPE_F32 || out_dtype == KAGNN_DTYPE_BF16, "out_dtype must be KAGNN_DTYPE_F32 or KAGNN_DTYPE_BF16");
    KAGNN_CHECK_ARG(x != out, "in-place aggregation is not supported");
    if (!aggregate_bf16_ok(x, ldx, out, ldo, out_dtype == KAGNN_DTYPE_BF16, F, bias))
        return fail(KAGNN_ERR_UNSUPPORTED, "%s: bf16 rows need num_feat % 8 == 0 (<= 512) and 16-byte aligned rows", __func__);
    return aggregate_sum_bf16(x, ldx, out, ldo, out_dtype == KAGNN_DTYPE_BF16, rowptr, col, edge_weight, N, F, self_scale, in_scale,
                              out_scale, bias, skip_self_loops, hub_seg, num_hub_seg, hub_threshold,
                              static_cast<float*>(workspace), workspace_bytes, as_stream(stream));
}

int kagnn_rows_to_bf16(const float* x, int64_t ldx, void* y, int64_t ldy, int64_t N, int32_t F, void* stream) {
    KAGNN_CHECK_ARG(N >= 0 && F >= 1 && ldx >= F && ldy >= F, "bad shape");
    KAGNN_CHECK_ARG(N == 0 || (x && y), "null array");
    return rows_to_bf16(x, ldx, y, ldy, N, F, as_stream(stream));
}

int kagnn_aggregate_workspace_bytes(int64_t num_hub_seg, int32_t F, size_t* bytes_host) {
    KAGNN_CHECK_ARG(num_hub_seg >= 0 && F >= 1 && bytes_host, "bad argument");
    *bytes_host = aggregate_bf16_ws_bytes(num_hub_seg, F);       // (F rounded up to 8: covers the fp32 form's round-up to 4)
    return KAGNN_OK;
}

int kagnn_aggregate_gine(const float* x, int64_t ldx, const float* ea, int64_t lde, float* out,
                         int64_t ldo, const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                         int64_t N, int32_t F, float self_scale, void* stream) {
    KAGNN_CHECK_ARG(N >= 0 && F >= 1, "bad shape");
    KAGNN_CHECK_ARG(N == 0 || (x && out && rowptr), "null array");
    return gine_fwd(x, ldx, ea, lde, out, ldo, rowptr, col, perm, N, F, self_scale, as_stream(stream));
}

int kagnn_aggregate_gine_bwd(const float* x, int64_t ldx, const float* ea, int64_t lde,
                             const float* gout, int64_t ldg, float* gx, int64_t ldgx, float* gea,
                             int64_t ldge, const int32_t* rowptr_t, const int32_t* col_t,
                             const int32_t* perm_t, int64_t N, int32_t F, float self_scale, void* stream) {
    KAGNN_CHECK_ARG(N >= 0 && F >= 1, "bad shape");
    KAGNN_CHECK_ARG(N == 0 || (x && gout && gx && rowptr_t), "null array");
    return gine_bwd(x, ldx, ea, lde, gout, ldg, gx, ldgx, gea, ldge, rowptr_t, col_t, perm_t, N, F,
                    self_scale, as_stream(stream));
}

int kagnn_segment_pool(const float* x, int64_t ldx, float* out, int64_t ldo, const int32_t* seg,
                       int64_t B, int32_t F, int32_t mean, void* stream) {
    KAGNN_CHECK_ARG(B >= 0 && F >= 1 && (B == 0 || (x && out && seg)), "bad argument");
    return segment_pool(x, ldx, out, ldo, seg, B, F, mean, as_stream(stream));
}

int kagnn_segment_broadcast(const float* g, int64_t ldg, float* gx, int64_t ldgx, const int32_t* seg,
                            int64_t B, int32_t F, int32_t mean, void* stream) {
    KAGNN_CHECK_ARG(B >= 0 && F >= 1 && (B == 0 || (g && gx && seg)), "bad argument");
    return segment_bcast(g, ldg, gx, ldgx, seg, B, F, mean, as_stream(stream));
}

// ---------------------------------------------------------------- efficient-KAN
int kagnn_embedding_fwd(const int64_t* index, int64_t index_stride, int64_t N, const float* table, int32_t V, int32_t F, float* out,
                        int64_t ldo, int32_t accumulate, void* stream) {
    KAGNN_CHECK_ARG(N >= 0 && V >= 1 && F >= 1 && index_stride >= 1 && ldo >= F, "bad shape");
    KAGNN_CHECK_ARG(N == 0 || (index && table && out), "null array");
    return embedding_fwd(index, index_stride, N, table, V, F, out, ldo, accumulate, as_stream(stream));
}

int kagnn_embedding_bwd_workspace_bytes(int64_t N, int32_t V, int32_t F, size_t* bytes) {
    KAGNN_CHECK_ARG(N >= 0 && V >= 1 && F >= 1 && bytes, "bad argument");
    *bytes = embedding_bwd_ws_bytes(N, V, F);
    return KAGNN_OK;
}

int kagnn_embedding_bwd(const int64_t* index, int64_t index_stride, int64_t N, const float* g, int64_t ldg, int32_t V, int32_t F,
                        float* g_table, void* workspace, size_t workspace_bytes, void* stream) {
    KAGNN_CHECK_ARG(N >= 0 && V >= 1 && F >= 1 && index_stride >= 1 && ldg >= F && g_table && workspace, "bad shape");
    KAGNN_CHECK_ARG(N == 0 || (index && g), "null array");
    return embedding_bwd(index, index_stride, N, g, ldg, V, F, g_table, static_cast<float*>(workspace), workspace_bytes, as_stream(stream));
}

int kagnn_kan_pack_bytes(int32_t in, int32_t out, int32_t G, int32_t K, int32_t mode,
                         size_t* fwd_bytes, size_t* dx_bytes) {
    ModeScope mode_scope_(mode);
    int rc = check_kan_dims_wide(__func__, in, out, G, K, mode);
    if (rc) return rc;
    KAGNN_CHECK_ARG(fwd_bytes && dx_bytes, "null output");
    *fwd_bytes = use_sparse_fwd(in, out, G, K, mode) ? kan_sparse_pack_fwd_bytes(in, out, G + K)
               : use_split_fwd(in, out, G, K, mode) ? kan_split_pack_fwd_bytes(in, out, G + K) : kan_f32_pack_fwd_bytes(in, out, G + K);
    *dx_bytes = use_split_dx(in, out, G, K, mode) ? kan_split_pack_dx_bytes(in, out, G + K, K) : kan_f32_pack_dx_bytes(in, out, G + K);
    return KAGNN_OK;
}

int kagnn_kan_pack(const float* bw, const float* sw, const float* sc, int32_t in, int32_t out,
                   int32_t G, int32_t K, int32_t mode, void* pack_fwd, void* pack_dx, void* stream) {
    ModeScope mode_scope_(mode);
    KAGNN_STAGE(stream);
    int rc = check_kan_dims_wide(__func__, in, out, G, K, mode);
    if (rc) return rc;
    KAGNN_CHECK_ARG(sw && pack_fwd && pack_dx, "null array");          // base_weight NULL = no SiLU branch
    const bool sf = use_split_fwd(in, out, G, K, mode), sd = use_split_dx(in, out, G, K, mode);
    // each workgroup derives the power-of-two weight scale itself; the hot case takes ONE launch for both layouts
    if (sd && use_sparse_fwd(in, out, G, K, mode) && kan_fused_pack_ok(in, out, G + K))
        return kan_fused_pack(bw, sw, sc, in, out, G + K, pack_fwd, pack_dx, as_stream(stream));
    if (sf) {
        rc = use_sparse_fwd(in, out, G, K, mode) ? kan_sparse_pack_fwd(bw, sw, sc, in, out, G + K, pack_fwd, as_stream(stream))
                                                 : kan_split_pack_fwd_noscale(bw, sw, sc, in, out, G + K, pack_fwd, as_stream(stream));
        if (rc) return rc;
    }
    if (sd) { rc = kan_split_pack_dx_noscale(bw, sw, sc, in, out, G + K, K, pack_dx, as_stream(stream)); if (rc) return rc; }
    if (!sf || !sd)
        return kan_f32_pack(bw, sw, sc, in, out, G + K, sf ? nullptr : (float*)pack_fwd, sd ? nullptr : (float*)pack_dx, as_stream(stream));
    return KAGNN_OK;
}

int kagnn_kan_pack_batch(int32_t n_layers, const float* const* bw, const float* const* sw, const float* const* sc,
                         const int32_t* in, const int32_t* out, int32_t G, int32_t K, int32_t mode,
                         void* const* pack_fwd, void* const* pack_dx, void* stream) {
    ModeScope mode_scope_(mode);
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(n_layers >= 1 && bw && sw && in && out && pack_fwd && pack_dx, "null array");
    for (int l = 0; l < n_layers; ++l) {
        int rc = check_kan_dims(__func__, in[l], out[l], G, K, mode);
        if (rc) return rc;
        KAGNN_CHECK_ARG(sw[l] && pack_fwd[l] && pack_dx[l], "null array");
        if (!(use_split_dx(in[l], out[l], G, K, mode) && use_sparse_fwd(in[l], out[l], G, K, mode)))
            return fail(KAGNN_ERR_UNSUPPORTED, "%s: only layers on the sparse-forward / split path batch their packs", __func__);
    }
    return kan_fused_pack_batch(n_layers, bw, sw, sc, in, out, G + K, pack_fwd, pack_dx, as_stream(stream));
}

int kagnn_kan_fwd_workspace_bytes(int64_t N, int32_t in, int32_t out, int32_t G, int32_t K, int32_t mode,
                                  size_t* bytes) {
    ModeScope mode_scope_(mode);
    int rc = check_kan_dims_wide(__func__, in, out, G, K, mode);
    if (rc) return rc;
    KAGNN_CHECK_ARG(bytes && N >= 0, "bad argument");
    *bytes = use_sparse_fwd(in, out, G, K, mode) ? kan_sparse_fwd_ws_bytes(N, in, out, G + K)
           : use_split_fwd(in, out, G, K, mode) ? kan_split_fwd_ws_bytes(N, in, out, G + K) : 0;
    return KAGNN_OK;
}

int kagnn_kan_linear_fwd(const float* x, int64_t ldx, int64_t N, const float* knots, int32_t in,
                         int32_t out, int32_t G, int32_t K, int32_t mode, const void* pack_fwd,
                         float* y, int64_t ldy, void* ws, size_t ws_bytes, void* stream) {
    ModeScope mode_scope_(mode);
    KAGNN_STAGE(stream);
    int rc = check_kan_dims_wide(__func__, in, out, G, K, mode);
    if (rc) return rc;
    KAGNN_CHECK_ARG(N >= 0 && ldx >= in && ldy >= out, "bad shape");
    if (N == 0) return KAGNN_OK;
    KAGNN_CHECK_ARG(x && knots && pack_fwd && y, "null array");
    if (use_split_fwd(in, out, G, K, mode)) {
        if (!(fits32(N, ldx) && fits32(N, ldy))) return fail(KAGNN_ERR_UNSUPPORTED, "%s: leading dimension > 7680 floats; call with KAGNN_PREC_FP32", __func__);
        if (use_sparse_fwd(in, out, G, K, mode))
            return kan_sparse_fwd(x, ldx, N, knots, in, out, G, K, pack_fwd, y, ldy, ws, ws_bytes, nullptr, nullptr, as_stream(stream));
        return kan_split_fwd(x, ldx, N, knots, in, out, G, K, pack_fwd, y, ldy, ws, ws_bytes, as_stream(stream));
    }
    if (high_order(K))
        return kan_ho_fwd(x, ldx, N, knots, in, out, G, K, (const float*)pack_fwd, y, ldy, mode == KAGNN_PREC_FP32_GRID, as_stream(stream));
    return kan_f32_fwd(x, ldx, N, knots, in, out, G, K, (const float*)pack_fwd, y, ldy, mode == KAGNN_PREC_FP32_GRID, as_stream(stream));
}

// forward on an input given as column blocks [x_0 | x_1 | ...] that live in different buffers: the
// skip-concat read-out of the node models (reference node_classification_clean/models.py:202 `torch.cat(l, dim=1)` feeding
// `lay_out`) without building the concatenation, one launch, one write of y.  pack_fwd is the pack of the WHOLE layer.
int kagnn_kan_fwd_parts_ok(const int32_t* part_widths, int32_t num_parts, int32_t in, int32_t out, int32_t G, int32_t K, int32_t mode) {
    ModeScope mode_scope_(mode);
    if (!part_widths || check_kan_dims(__func__, in, out, G, K, mode)) return 0;
    return use_sparse_fwd(in, out, G, K, mode) && kan_sparse_fwd_parts_ok(part_widths, num_parts, in, out, G, K) ? 1 : 0;
}

int kagnn_kan_linear_fwd_parts(const float* const* x_parts, const int32_t* part_widths, const int64_t* part_ld, int32_t num_parts,
                               int64_t N, const float* knots, int32_t in, int32_t out, int32_t G, int32_t K, int32_t mode,
                               const void* pack_fwd, float* y, int64_t ldy, void* ws, size_t ws_bytes, void* stream) {
    ModeScope mode_scope_(mode);
    return kagnn_kan_linear_fwd_parts_affine(x_parts, part_widths, part_ld, nullptr, num_parts, N, knots, in, out, G, K, mode, pack_fwd, y, ldy,
                                             ws, ws_bytes, stream);
}

// part_affine (NULL, or per block NULL / 2 * width floats: the block's column scales, then its column shifts): the block is
// read as  scale * x + shift  -- a BatchNorm1d output that was never written (the skip read-out of the node models over
// normalised layer outputs, reference node_classification_clean/models.py:198-203).
int kagnn_kan_linear_fwd_parts_affine(const float* const* x_parts, const int32_t* part_widths, const int64_t* part_ld,
                                      const float* const* part_affine, int32_t num_parts,
                                      int64_t N, const float* knots, int32_t in, int32_t out, int32_t G, int32_t K, int32_t mode,
                                      const void* pack_fwd, float* y, int64_t ldy, void* ws, size_t ws_bytes, void* stream) {
    ModeScope mode_scope_(mode);
    KAGNN_STAGE_AS("kagnn_kan_linear_fwd_parts", stream);
    int rc = check_kan_dims(__func__, in, out, G, K, mode);
    if (rc) return rc;
    KAGNN_CHECK_ARG(x_parts && part_widths && part_ld && num_parts >= 1, "null block table");
    KAGNN_CHECK_ARG(N >= 0 && ldy >= out, "bad shape");
    if (!kagnn_kan_fwd_parts_ok(part_widths, num_parts, in, out, G, K, mode))
        return fail(KAGNN_ERR_UNSUPPORTED, "%s: blocks not covered (kagnn_kan_fwd_parts_ok): concatenate and call kagnn_kan_linear_fwd", __func__);
    if (N == 0) return KAGNN_OK;
    KAGNN_CHECK_ARG(knots && pack_fwd && y, "null array");
    if (!fits32(N, ldy)) return fail(KAGNN_ERR_UNSUPPORTED, "%s: leading dimension > 7680 floats", __func__);
    static_assert(sizeof(long) == sizeof(int64_t), "LP64");
    return kan_sparse_fwd_parts(x_parts, part_widths, reinterpret_cast<const long*>(part_ld), num_parts, N, knots, in, out, G, K, pack_fwd, y, ldy, ws, ws_bytes, as_stream(stream), part_affine);
}

// forward + column moments of its output (the statistics of the BatchNorm1d that follows a convolution)
static bool fused_moments(int64_t N, int32_t in, int32_t out, int32_t G, int32_t K, int32_t mode) {
    return use_split_fwd(in, out, G, K, mode) && use_sparse_fwd(in, out, G, K, mode) && kan_sparse_fwd_moments_ok(N, in, out, G, K);
}

int kagnn_kan_fwd_moments_workspace_bytes(int64_t N, int32_t in, int32_t out, int32_t G, int32_t K, int32_t mode,
                                          size_t* bytes) {
    ModeScope mode_scope_(mode);
    size_t b = 0;
    int rc = check_kan_dims(__func__, in, out, G, K, mode);
    if (rc) return rc;
    rc = kagnn_kan_fwd_workspace_bytes(N, in, out, G, K, mode, &b);
    if (rc) return rc;
    const size_t m = fused_moments(N, in, out, G, K, mode) ? kan_sparse_fwd_moments_ws_bytes(N, out) : bn_ws_bytes(N, out);
    *bytes = b > m ? b : m;
    return KAGNN_OK;
}

int kagnn_kan_linear_fwd_moments(const float* x, int64_t ldx, int64_t N, const float* knots, int32_t in,
                                 int32_t out, int32_t G, int32_t K, int32_t mode, const void* pack_fwd,
                                 float* y, int64_t ldy, float* col_mean, float* col_m2, void* ws, size_t ws_bytes,
                                 void* stream) {
    ModeScope mode_scope_(mode);
    KAGNN_STAGE(stream);
    int rc = check_kan_dims(__func__, in, out, G, K, mode);
    if (rc) return rc;
    KAGNN_CHECK_ARG(N >= 1 && ldx >= in && ldy >= out, "bad shape (column moments need at least one row)");
    KAGNN_CHECK_ARG(x && knots && pack_fwd && y && col_mean && col_m2, "null array");
    size_t need = 0;
    rc = kagnn_kan_fwd_moments_workspace_bytes(N, in, out, G, K, mode, &need);
    if (rc) return rc;
    KAGNN_CHECK_ARG(need == 0 || (ws && ws_bytes >= need), "workspace too small (kagnn_kan_fwd_moments_workspace_bytes)");
    if (fused_moments(N, in, out, G, K, mode)) {
        if (!(fits32(N, ldx) && fits32(N, ldy))) return fail(KAGNN_ERR_UNSUPPORTED, "%s: leading dimension > 7680 floats; call with KAGNN_PREC_FP32", __func__);
        return kan_sparse_fwd(x, ldx, N, knots, in, out, G, K, pack_fwd, y, ldy, ws, ws_bytes, col_mean, col_m2, as_stream(stream));
    }
    rc = kagnn_kan_linear_fwd(x, ldx, N, knots, in, out, G, K, mode, pack_fwd, y, ldy, ws, ws_bytes, stream);
    if (rc) return rc;
    return col_moments(y, ldy, N, out, col_mean, col_m2, ws, ws_bytes, as_stream(stream));
}

int kagnn_kan_linear_bwd_input(const float* x, int64_t ldx, const float* gy, int64_t ldgy, int64_t N,
                               const float* knots, int32_t in, int32_t out, int32_t G, int32_t K,
                               int32_t mode, const void* pack_dx, void* gx, int64_t ldgx, int32_t gx_dtype, void* stream) {
    ModeScope mode_scope_(mode);
    return kagnn_kan_linear_bwd_input_affine(x, ldx, nullptr, gy, ldgy, N, knots, in, out, G, K, mode, pack_dx, gx, ldgx, gx_dtype, stream);
}

// x_affine (NULL, or 2 * in floats: column scales, then column shifts): the layer input is  scale * x + shift  -- a BatchNorm1d
// output that was never written; gx is the gradient with respect to THAT input (the norm's own backward takes it from there).
// Covered: split precision, cubic layers of <= 8 coefficients and <= 64 outputs (the read-out of the node models).
int kagnn_kan_linear_bwd_input_affine(const float* x, int64_t ldx, const float* x_affine, const float* gy, int64_t ldgy, int64_t N,
                                      const float* knots, int32_t in, int32_t out, int32_t G, int32_t K,
                                      int32_t mode, const void* pack_dx, void* gx, int64_t ldgx, int32_t gx_dtype, void* stream) {
    ModeScope mode_scope_(mode);
    KAGNN_STAGE_AS("kagnn_kan_linear_bwd_input", stream);
    int rc = check_kan_dims_wide(__func__, in, out, G, K, mode);
    if (rc) return rc;
    KAGNN_CHECK_ARG(N >= 0 && ldx >= in && ldgy >= out && ldgx >= in, "bad shape");
    KAGNN_CHECK_ARG(gx_dtype == KAGNN_DTYPE_F32 || gx_dtype == KAGNN_DTYPE_BF16, "gx_dtype must be KAGNN_DTYPE_F32 or KAGNN_DTYPE_BF16");
    if (N == 0) return KAGNN_OK;
    KAGNN_CHECK_ARG(x && gy && knots && pack_dx && gx, "null array");
    if (use_split_dx(in, out, G, K, mode)) {
        if (!(fits32(N, ldx) && fits32(N, ldgy) && fits32(N, ldgx))) return fail(KAGNN_ERR_UNSUPPORTED, "%s: leading dimension > 7680 floats; call with KAGNN_PREC_FP32", __func__);
        return kan_split_dx(x, ldx, gy, ldgy, N, knots, in, out, G, K, pack_dx, static_cast<float*>(gx), ldgx, as_stream(stream),
                            gx_dtype == KAGNN_DTYPE_BF16, x_affine);
    }
    if (x_affine) return fail(KAGNN_ERR_UNSUPPORTED, "%s: an input affine is applied by the split-precision kernels only", __func__);
    if (gx_dtype != KAGNN_DTYPE_F32) return fail(KAGNN_ERR_UNSUPPORTED, "%s: bf16 gradient rows are produced by the split-precision kernels only", __func__);
    float* gxf = static_cast<float*>(gx);
    if (high_order(K))
        return kan_ho_dx(x, ldx, gy, ldgy, N, knots, in, out, G, K, (const float*)pack_dx, gxf, ldgx, mode == KAGNN_PREC_FP32_GRID, as_stream(stream));
    return kan_f32_dx(x, ldx, gy, ldgy, N, knots, in, out, G, K, (const float*)pack_dx, gxf, ldgx, mode == KAGNN_PREC_FP32_GRID, as_stream(stream));
}

// kagnn_kan_linear_bwd_input_affine that ALSO leaves the two column sums the backward of the folded BatchNorm1d starts from:
// sums[0][in] = sum_n gx, sums[1][in] = sum_n gx * xhat, xhat = (x - bn_mean) * bn_rstd on the raw rows (x = the norm's input).
// The read-out's gradient of the LAST convolution's output in the node models (reference node_classification_clean/models.py:198-203):
// that norm's incoming gradient is exactly this gx, so its statistics pass over (gx, x) goes away.  Covered (kagnn_kan_bwd_input_sums_ok):
// split precision, cubic layers of <= 8 coefficients, <= 64 inputs (a multiple of 4) and outputs, >= 32768 rows.
int kagnn_kan_bwd_input_sums_ok(int64_t N, int32_t in, int32_t out, int32_t G, int32_t K, int32_t mode) {
    ModeScope mode_scope_(mode);
    return mode == KAGNN_PREC_SPLIT && use_split_dx(in, out, G, K, mode) && kan_split_dx_stats_ok(N, in, out, G, K) ? 1 : 0;
}
int kagnn_kan_bwd_input_sums_workspace_bytes(int64_t N, int32_t in, size_t* bytes) {
    KAGNN_CHECK_ARG(N >= 0 && in >= 1 && bytes, "bad argument");
    *bytes = ((size_t)kan_split_dx_stats_blocks(N) + 1) * 2 * in * sizeof(float);
    return KAGNN_OK;
}
int kagnn_kan_linear_bwd_input_affine_sums(const float* x, int64_t ldx, const float* x_affine, const float* bn_mean, const float* bn_rstd,
                                           const float* gy, int64_t ldgy, int64_t N, const float* knots, int32_t in, int32_t out,
                                           int32_t G, int32_t K, int32_t mode, const void* pack_dx, float* gx, int64_t ldgx,
                                           float* sums, void* workspace, size_t workspace_bytes, void* stream) {
    ModeScope mode_scope_(mode);
    int rc = check_kan_dims(__func__, in, out, G, K, mode);
    if (rc) return rc;
    KAGNN_CHECK_ARG(N >= 1 && ldx >= in && ldgy >= out && ldgx >= in, "bad shape");
    KAGNN_CHECK_ARG(x && x_affine && bn_mean && bn_rstd && gy && knots && pack_dx && gx && sums && workspace, "null array");
    if (!kagnn_kan_bwd_input_sums_ok(N, in, out, G, K, mode)) return fail(KAGNN_ERR_UNSUPPORTED, "%s: shape not covered (kagnn_kan_bwd_input_sums_ok)", __func__);
    if (!(fits32(N, ldx) && fits32(N, ldgy) && fits32(N, ldgx))) return fail(KAGNN_ERR_UNSUPPORTED, "%s: leading dimension > 7680 floats", __func__);
    const int B = kan_split_dx_stats_blocks(N);
    KAGNN_CHECK_ARG(workspace_bytes >= ((size_t)B + 1) * 2 * in * sizeof(float), "workspace too small (kagnn_kan_bwd_input_sums_workspace_bytes)");
    float* partial = static_cast<float*>(workspace);
    {
        KAGNN_STAGE_AS("kagnn_kan_linear_bwd_input", stream);
        rc = kan_split_dx_stats(x, ldx, gy, ldgy, N, knots, in, out, G, K, pack_dx, gx, ldgx, as_stream(stream), x_affine, bn_mean, bn_rstd, partial);
        if (rc) return rc;
    }
    KAGNN_STAGE_AS("kagnn_batchnorm_bwd statistics fold", stream);
    return bn_finish_partials(partial, B, in, sums, as_stream(stream));
}

int kagnn_kan_bwd_weight_workspace_bytes(int64_t N, int32_t in, int32_t out, int32_t G, int32_t K,
                                         int32_t mode, size_t* bytes) {
    ModeScope mode_scope_(mode);
    int rc = check_kan_dims_wide(__func__, in, out, G, K, mode);
    if (rc) return rc;
    KAGNN_CHECK_ARG(bytes && N >= 0, "bad argument");
    *bytes = use_split_dw(in, out, G, K, mode) ? kan_split_dw_ws_bytes(N, in, out, G + K, K)
                                                                   : kan_f32_dw_ws_bytes(N, in, out, G + K);
    return KAGNN_OK;
}

int kagnn_kan_linear_bwd_weight(const float* x, int64_t ldx, const float* gy, int64_t ldgy, int64_t N,
                                const float* knots, int32_t in, int32_t out, int32_t G, int32_t K,
                                int32_t mode, const float* sw, const float* sc, float* g_bw,
                                float* g_sw, float* g_sc, void* ws, size_t ws_bytes, void* stream) {
    return kan_linear_bwd_weight(x, ldx, nullptr, gy, ldgy, N, knots, in, out, G, K, mode, sw, sc, g_bw, g_sw, g_sc, ws, ws_bytes, stream, nullptr);
}

// x_affine: as kagnn_kan_linear_bwd_input_affine (the weight gradient of a layer whose input is a folded BatchNorm1d output)
int kagnn_kan_linear_bwd_weight_affine(const float* x, int64_t ldx, const float* x_affine, const float* gy, int64_t ldgy, int64_t N,
                                       const float* knots, int32_t in, int32_t out, int32_t G, int32_t K,
                                       int32_t mode, const float* sw, const float* sc, float* g_bw,
                                       float* g_sw, float* g_sc, void* ws, size_t ws_bytes, void* stream) {
    return kan_linear_bwd_weight(x, ldx, x_affine, gy, ldgy, N, knots, in, out, G, K, mode, sw, sc, g_bw, g_sw, g_sc, ws, ws_bytes, stream, nullptr);
}

// ---------------------------------------------------------------- FastKAN
static int check_fk(const char* fn, int in, int out, int ng, int mode) {
    if (in < 1 || out < 1) return fail(KAGNN_ERR_ARG, "%s: input_dim/output_dim must be >= 1", fn);
    if (ng < 1 || ng > kMaxKnots) return fail(KAGNN_ERR_UNSUPPORTED, "%s: num_grids out of range", fn);
    if (mode != KAGNN_PREC_FP32 && mode != KAGNN_PREC_SPLIT) return fail(KAGNN_ERR_ARG, "%s: unknown precision mode", fn);
    return KAGNN_OK;
}

// ---------------------------------------------------------------- adaptive grids (update_grid)
int kagnn_kan_bsplines(const float* x, int64_t ldx, int64_t N, const float* grid, int32_t in, int32_t G,
                       int32_t K, float* bases, void* stream) {
    int rc = check_kan_dims_wide(__func__, in, 1, G, K, KAGNN_PREC_FP32_GRID);
    if (rc) return rc;
    KAGNN_CHECK_ARG(N >= 0 && ldx >= in, "bad shape");
    KAGNN_CHECK_ARG(N == 0 || (x && grid && bases), "null array");
    if (high_order(K)) return kan_ho_bsplines(x, ldx, N, grid, in, G, K, bases, as_stream(stream));
    return kan_bsplines(x, ldx, N, grid, in, G, K, bases, as_stream(stream));
}

int kagnn_kan_grid_refit_workspace_bytes(int64_t N, int32_t in, int32_t G, int32_t K, size_t* bytes) {
    int rc = check_kan_dims(__func__, in, 1, G, K, KAGNN_PREC_FP32_GRID);
    if (rc) return rc;
    KAGNN_CHECK_ARG(bytes != nullptr && N >= 1, "null output or no rows");
    *bytes = kan_grid_resize_ws_bytes(N, in, G + K, G + K);
    return KAGNN_OK;
}

int kagnn_kan_grid_refit(const float* x, int64_t ldx, int64_t N, const float* grid_old, const float* grid_new,
                         int32_t in, int32_t out, int32_t G, int32_t K, const float* sw, const float* sc,
                         float* new_sw, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_kan_dims(__func__, in, out, G, K, KAGNN_PREC_FP32_GRID);
    if (rc) return rc;
    KAGNN_CHECK_ARG(N >= 1 && ldx >= in, "bad shape");
    KAGNN_CHECK_ARG(x && grid_old && grid_new && sw && new_sw && ws, "null array");
    KAGNN_CHECK_ARG(sw != new_sw, "the refit is not in place");
    return kan_grid_resize(x, ldx, N, grid_old, grid_new, nullptr, in, out, G, G, K, sw, sc, new_sw, nullptr, ws, ws_bytes,
                           as_stream(stream));
}

// grid resize: the refit between grids of two sizes (grid extension), up to kMaxKnots knots on either side; the two calls above
// are this one with equal sizes, every row taking part
int kagnn_kan_grid_resize_workspace_bytes(int64_t N, int32_t in, int32_t G_old, int32_t G_new, int32_t K, size_t* bytes) {
    int rc = check_kan_dims(__func__, in, 1, G_old, K, KAGNN_PREC_FP32_GRID);
    if (!rc) rc = check_kan_dims(__func__, in, 1, G_new, K, KAGNN_PREC_FP32_GRID);
    if (rc) return rc;
    KAGNN_CHECK_ARG(bytes != nullptr && N >= 1, "null output or no rows");
    *bytes = kan_grid_resize_ws_bytes(N, in, G_new + K, G_old + K);
    return KAGNN_OK;
}

int kagnn_kan_grid_resize(const float* x, int64_t ldx, int64_t N, const float* grid_old, const float* grid_new, const float* window,
                          int32_t in, int32_t out, int32_t G_old, int32_t G_new, int32_t K, const float* sw, const float* sc,
                          float* new_sw, int32_t* untouched, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_kan_dims(__func__, in, out, G_old, K, KAGNN_PREC_FP32_GRID);
    if (!rc) rc = check_kan_dims(__func__, in, out, G_new, K, KAGNN_PREC_FP32_GRID);
    if (rc) return rc;
    KAGNN_CHECK_ARG(N >= 1 && ldx >= in, "bad shape");
    KAGNN_CHECK_ARG(x && grid_old && grid_new && sw && new_sw && ws, "null array");
    KAGNN_CHECK_ARG(sw != new_sw, "the refit is not in place");
    return kan_grid_resize(x, ldx, N, grid_old, grid_new, window, in, out, G_old, G_new, K, sw, sc, new_sw, untouched, ws, ws_bytes,
                           as_stream(stream));
}

int kagnn_fastkan_fwd_workspace_bytes(int64_t N, int32_t in, int32_t out, int32_t ng, int32_t mode, size_t* bytes) {
    ModeScope mode_scope_(mode);
    int rc = check_fk(__func__, in, out, ng, mode);
    if (rc) return rc;
    KAGNN_CHECK_ARG(bytes && N >= 0, "bad argument");
    *bytes = fastkan_fwd_ws_bytes(N, in, out, ng, mode);
    return KAGNN_OK;
}

int kagnn_fastkan_fwd(const float* x, int64_t ldx, int64_t N, int32_t in, int32_t out, int32_t ng,
                      const float* centers, float denominator, const float* ln_w, const float* ln_b,
                      float ln_eps, const float* spline_w, const float* base_w, const float* base_b,
                      float* y, int64_t ldy, float* row_stats, int32_t mode, void* ws, size_t ws_bytes, void* stream) {
    ModeScope mode_scope_(mode);
    KAGNN_STAGE(stream);
    int rc = check_fk(__func__, in, out, ng, mode);
    if (rc) return rc;
    KAGNN_CHECK_ARG(N >= 0 && ldx >= in && ldy >= out, "bad shape");
    if (N == 0) return KAGNN_OK;
    KAGNN_CHECK_ARG(x && centers && spline_w && y && ws, "null array");
    KAGNN_CHECK_ARG(denominator != 0.0f, "denominator is zero");
    KAGNN_CHECK_ARG((ln_w == nullptr) == (ln_b == nullptr), "layernorm weight and bias must both be given or both be null");
    if (mode == KAGNN_PREC_SPLIT && !(fits32(N, ldx) && fits32(N, ldy)))
        return fail(KAGNN_ERR_UNSUPPORTED, "%s: leading dimension > 7680 floats; call with KAGNN_PREC_FP32", __func__);
    return fastkan_fwd(x, ldx, N, in, out, ng, centers, denominator, ln_w, ln_b, ln_eps, spline_w, base_w,
                       base_b, y, ldy, row_stats, ws, ws_bytes, mode, as_stream(stream));
}

int kagnn_fastkan_fwd_stats_in_kernel(int64_t N, int32_t in, int32_t out, int32_t ng, int32_t mode) {
    ModeScope mode_scope_(mode);
    if (check_fk(__func__, in, out, ng, mode)) return 0;
    return fastkan_fwd_stats_in_kernel(N, in, out, ng, mode) ? 1 : 0;
}

int kagnn_fastkan_bwd_workspace_bytes(int64_t N, int32_t in, int32_t out, int32_t ng, int32_t mode, size_t* bytes) {
    ModeScope mode_scope_(mode);
    int rc = check_fk(__func__, in, out, ng, mode);
    if (rc) return rc;
    KAGNN_CHECK_ARG(bytes && N >= 0, "bad argument");
    *bytes = fastkan_bwd_ws_bytes(N, in, out, ng, mode);
    return KAGNN_OK;
}

int kagnn_fastkan_bwd(const float* x, int64_t ldx, const float* gy, int64_t ldgy, int64_t N, int32_t in,
                      int32_t out, int32_t ng, const float* centers, float denominator,
                      const float* ln_w, const float* ln_b, float ln_eps, const float* spline_w,
                      const float* base_w, const float* row_stats, float* gx, int64_t ldgx,
                      float* g_ln_w, float* g_ln_b, float* g_spline_w, float* g_base_w,
                      float* g_base_b, int32_t mode, void* ws, size_t ws_bytes, void* stream) {
    ModeScope mode_scope_(mode);
    KAGNN_STAGE(stream);
    int rc = check_fk(__func__, in, out, ng, mode);
    if (rc) return rc;
    KAGNN_CHECK_ARG(N >= 0 && ldx >= in && ldgy >= out && ldgx >= in, "bad shape");
    KAGNN_CHECK_ARG(centers && spline_w && g_spline_w && ws, "null array");
    KAGNN_CHECK_ARG(N == 0 || (x && gy && gx), "null array");
    KAGNN_CHECK_ARG(ln_w == nullptr || (ln_b && row_stats && g_ln_w && g_ln_b), "layernorm needs bias, row_stats and both gradient outputs");
    KAGNN_CHECK_ARG(base_w == nullptr || (g_base_w && g_base_b), "base branch needs both gradient outputs");
    if (mode == KAGNN_PREC_SPLIT && !(fits32(N, ldx) && fits32(N, ldgy) && fits32(N, ldgx)))
        return fail(KAGNN_ERR_UNSUPPORTED, "%s: leading dimension > 7680 floats; call with KAGNN_PREC_FP32", __func__);
    return fastkan_bwd(x, ldx, gy, ldgy, N, in, out, ng, centers, denominator, ln_w, ln_b, ln_eps, spline_w,
                       base_w, row_stats, gx, ldgx, g_ln_w, g_ln_b, g_spline_w, g_base_w, g_base_b, ws,
                       ws_bytes, mode, as_stream(stream));
}

// ---------------------------------------------------------------- per-edge activations of a FastKANLayer (fastkan_edge.hip)
// exact fp32 in every precision mode (no `mode` argument); every num_grids the layer takes; fixed-order slab reductions (no atomics)

int kagnn_fastkan_edge_abs_sum_workspace_bytes(int64_t N, int32_t in, int32_t out, int32_t ng, int32_t layernorm, size_t* bytes) {
    int rc = check_fk(__func__, in, out, ng, KAGNN_PREC_FP32);
    if (rc) return rc;
    KAGNN_CHECK_ARG(bytes != nullptr && N >= 0, "null output or negative row count");
    *bytes = fastkan_edge_abs_sum_ws_bytes(N, in, out, layernorm != 0);
    return KAGNN_OK;
}

int kagnn_fastkan_edge_abs_sum(const float* x, int64_t ldx, int64_t N, int32_t in, int32_t out, int32_t ng, const float* centers,
                               float denominator, const float* ln_w, const float* ln_b, float ln_eps, const float* spline_w,
                               const float* base_w, float* S, int64_t ldS, void* ws, size_t ws_bytes, void* stream) {
    KAGNN_STAGE(stream);
    int rc = check_fk(__func__, in, out, ng, KAGNN_PREC_FP32);
    if (rc) return rc;
    KAGNN_CHECK_ARG(N >= 0 && ldx >= in && ldS >= in, "bad shape");
    KAGNN_CHECK_ARG(S != nullptr, "null array");
    KAGNN_CHECK_ARG((ln_w == nullptr) == (ln_b == nullptr), "layernorm weight and bias must both be given or both be null");
    if (N == 0) {                                   // an empty sum: zeros, no kernel
        KAGNN_HIP(hipMemset2DAsync(S, (size_t)ldS * sizeof(float), 0, (size_t)in * sizeof(float), (size_t)out, as_stream(stream)));
        return KAGNN_OK;
    }
    KAGNN_CHECK_ARG(x && centers && spline_w && ws, "null array");          // base_weight NULL: the layer has no base branch
    KAGNN_CHECK_ARG(denominator != 0.0f, "denominator is zero");
    return fastkan_edge_abs_sum(x, ldx, N, in, out, ng, centers, denominator, ln_w, ln_b, ln_eps, spline_w, base_w, S, ldS, ws,
                                ws_bytes, as_stream(stream));
}

int kagnn_fastkan_edge_abs_sum_bwd_workspace_bytes(int64_t N, int32_t in, int32_t out, int32_t ng, int32_t layernorm, size_t* bytes) {
    int rc = check_fk(__func__, in, out, ng, KAGNN_PREC_FP32);
    if (rc) return rc;
    KAGNN_CHECK_ARG(bytes != nullptr && N >= 0, "null output or negative row count");
    *bytes = fastkan_edge_abs_sum_bwd_ws_bytes(N, in, out, ng, layernorm != 0);
    return KAGNN_OK;
}

int kagnn_fastkan_edge_abs_sum_bwd(const float* x, int64_t ldx, int64_t N, int32_t in, int32_t out, int32_t ng, const float* centers,
                                   float denominator, const float* ln_w, const float* ln_b, float ln_eps, const float* spline_w,
                                   const float* base_w, const float* gS, int64_t ldgS, float* g_spline_w, float* g_base_w, float* gx,
                                   int64_t ldgx, float* g_ln_w, float* g_ln_b, void* ws, size_t ws_bytes, void* stream) {
    KAGNN_STAGE(stream);
    int rc = check_fk(__func__, in, out, ng, KAGNN_PREC_FP32);
    if (rc) return rc;
    KAGNN_CHECK_ARG(N >= 0 && ldx >= in && ldgS >= in && (!gx || ldgx >= in), "bad shape");
    KAGNN_CHECK_ARG((ln_w == nullptr) == (ln_b == nullptr), "layernorm weight and bias must both be given or both be null");
    KAGNN_CHECK_ARG(!g_base_w || base_w, "a base_weight gradient needs base_weight");
    KAGNN_CHECK_ARG((g_ln_w == nullptr) == (g_ln_b == nullptr) && (!g_ln_w || ln_w), "the layernorm gradients come as a pair and need layernorm");
    if (N == 0) {                                   // empty sums: zeros, no kernel (gx has no rows)
        const size_t e = (size_t)in * out * sizeof(float);
        if (g_base_w) KAGNN_HIP(hipMemsetAsync(g_base_w, 0, e, as_stream(stream)));
        if (g_spline_w) KAGNN_HIP(hipMemsetAsync(g_spline_w, 0, e * ng, as_stream(stream)));
        if (g_ln_w) KAGNN_HIP(hipMemsetAsync(g_ln_w, 0, (size_t)in * sizeof(float), as_stream(stream)));
        if (g_ln_b) KAGNN_HIP(hipMemsetAsync(g_ln_b, 0, (size_t)in * sizeof(float), as_stream(stream)));
        return KAGNN_OK;
    }
    KAGNN_CHECK_ARG(x && centers && spline_w && gS, "null array");
    KAGNN_CHECK_ARG(!ln_w || (gx == nullptr) == (g_ln_w == nullptr), "with layernorm, gx and the layernorm gradients come from one pass: all three or none");
    KAGNN_CHECK_ARG(denominator != 0.0f, "denominator is zero");
    KAGNN_CHECK_ARG(ws != nullptr, "the workspace is missing");
    return fastkan_edge_abs_sum_bwd(x, ldx, N, in, out, ng, centers, denominator, ln_w, ln_b, ln_eps, spline_w, base_w, gS, ldgS,
                                    g_spline_w, g_base_w, gx, ldgx, g_ln_w, g_ln_b, ws, ws_bytes, as_stream(stream));
}

int kagnn_fastkan_edge_curves(const float* t, int64_t ldt, const float* t_base, int64_t ldt_base, int64_t P, int32_t in, int32_t out,
                              int32_t ng, const float* centers, float denominator, const float* spline_w, const float* base_w,
                              float* phi, void* stream) {
    KAGNN_STAGE(stream);
    int rc = check_fk(__func__, in, out, ng, KAGNN_PREC_FP32);
    if (rc) return rc;
    KAGNN_CHECK_ARG(P >= 0 && (ldt == 0 || ldt >= in) && (ldt_base == 0 || ldt_base >= in), "bad shape");
    KAGNN_CHECK_ARG(spline_w || base_w, "neither branch is given");
    KAGNN_CHECK_ARG(phi != nullptr || P == 0, "null array");
    if (P == 0) return KAGNN_OK;
    KAGNN_CHECK_ARG(centers && (!spline_w || t) && (!base_w || t || t_base), "null array");
    KAGNN_CHECK_ARG(denominator != 0.0f, "denominator is zero");
    return fastkan_edge_curves(spline_w ? t : nullptr, ldt, base_w ? (t_base ? t_base : t) : nullptr, t_base ? ldt_base : ldt, P, in, out,
                               ng, centers, denominator, spline_w, base_w, phi, as_stream(stream));
}

// ---------------------------------------------------------------- feature-sharded FastKAN layer
int kagnn_fastkan_row_moments(const float* x, int64_t ldx, int64_t N, int32_t in, float* moments, void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(N >= 0 && in >= 1 && ldx >= in, "bad shape");
    KAGNN_CHECK_ARG(N == 0 || (x && moments), "null array");
    return fastkan_row_moments(x, ldx, N, in, moments, as_stream(stream));
}

int kagnn_fastkan_merge_moments(const float* gathered, int32_t P, int64_t N, int32_t in, float ln_eps, float* row_stats,
                                void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(N >= 0 && in >= 1 && P >= 1, "bad shape");
    KAGNN_CHECK_ARG(N == 0 || (gathered && row_stats), "null array");
    return fastkan_merge_moments(gathered, P, N, in, ln_eps, row_stats, as_stream(stream));
}

int kagnn_fastkan_shard_fwd(const float* x, int64_t ldx, int64_t N, int32_t in, int32_t out, int32_t ng,
                            const float* centers, float denominator, const float* ln_w, const float* ln_b,
                            const float* row_stats, const float* spline_w, const float* base_w, const float* base_b,
                            float* y, int64_t ldy, int32_t mode, void* ws, size_t ws_bytes, void* stream) {
    ModeScope mode_scope_(mode);
    KAGNN_STAGE(stream);
    int rc = check_fk(__func__, in, out, ng, mode);
    if (rc) return rc;
    KAGNN_CHECK_ARG(N >= 0 && ldx >= in && ldy >= out, "bad shape");
    if (N == 0) return KAGNN_OK;
    KAGNN_CHECK_ARG(x && centers && spline_w && y && ws, "null array");
    KAGNN_CHECK_ARG(denominator != 0.0f, "denominator is zero");
    KAGNN_CHECK_ARG((ln_w == nullptr) == (ln_b == nullptr), "layernorm weight and bias must both be given or both be null");
    KAGNN_CHECK_ARG(ln_w == nullptr || row_stats, "layernorm on a column shard needs the merged row statistics");
    if (mode == KAGNN_PREC_SPLIT && !(fits32(N, ldx) && fits32(N, ldy)))
        return fail(KAGNN_ERR_UNSUPPORTED, "%s: leading dimension > 7680 floats; call with KAGNN_PREC_FP32", __func__);
    return fastkan_fwd(x, ldx, N, in, out, ng, centers, denominator, ln_w, ln_b, 0.0f, spline_w, base_w, base_b, y, ldy,
                       const_cast<float*>(row_stats), ws, ws_bytes, mode, as_stream(stream), ln_w != nullptr);
}

int kagnn_fastkan_shard_bwd(const float* x, int64_t ldx, const float* gy, int64_t ldgy, int64_t N, int32_t in,
                            int32_t out, int32_t ng, const float* centers, float denominator,
                            const float* ln_w, const float* ln_b, const float* spline_w,
                            const float* base_w, const float* row_stats, float* gx, int64_t ldgx,
                            float* row_sums, float* g_spline_w, float* g_base_w,
                            float* g_base_b, int32_t parts, int32_t mode, void* ws, size_t ws_bytes, void* stream) {
    ModeScope mode_scope_(mode);
    KAGNN_STAGE(stream);
    int rc = check_fk(__func__, in, out, ng, mode);
    if (rc) return rc;
    KAGNN_CHECK_ARG(N >= 0 && ldx >= in && ldgy >= out && ldgx >= in, "bad shape");
    KAGNN_CHECK_ARG(parts >= 1 && parts <= 3, "parts: 1 = input-gradient half, 2 = weight-gradient half, 3 = both");
    KAGNN_CHECK_ARG(centers && spline_w && ws, "null array");
    KAGNN_CHECK_ARG(N == 0 || (x && gy), "null array");
    KAGNN_CHECK_ARG(!(parts & 1) || N == 0 || gx, "null array");
    KAGNN_CHECK_ARG(!(parts & 1) || ln_w == nullptr || N == 0 || row_sums, "layernorm needs row_sums");
    KAGNN_CHECK_ARG(!(parts & 2) || (g_spline_w && (base_w == nullptr || g_base_w)), "the weight-gradient half needs its outputs");
    KAGNN_CHECK_ARG(ln_w == nullptr || (ln_b && (N == 0 || row_stats)), "layernorm needs bias and row_stats");   // (no rows: no statistics)
    if (mode == KAGNN_PREC_SPLIT && !(fits32(N, ldx) && fits32(N, ldgy) && fits32(N, ldgx)))
        return fail(KAGNN_ERR_UNSUPPORTED, "%s: leading dimension > 7680 floats; call with KAGNN_PREC_FP32", __func__);
    return fastkan_bwd(x, ldx, gy, ldgy, N, in, out, ng, centers, denominator, ln_w, ln_b, 0.0f, spline_w,
                       base_w, row_stats, gx, ldgx, nullptr, nullptr, g_spline_w, g_base_w, g_base_b, ws,
                       ws_bytes, mode, as_stream(stream), parts == 3 ? 1 : parts == 1 ? 3 : 4, row_sums, 0);
}

int kagnn_fastkan_shard_bwd_finish(const float* x, int64_t ldx, int64_t N, int32_t in, int32_t in_total, int32_t out,
                                   int32_t ng, const float* ln_w, const float* ln_b, const float* row_stats,
                                   const float* row_sums, float* gx, int64_t ldgx, float* g_ln_w, float* g_ln_b,
                                   int32_t mode, void* ws, size_t ws_bytes, void* stream) {
    ModeScope mode_scope_(mode);
    KAGNN_STAGE(stream);
    int rc = check_fk(__func__, in, out, ng, mode);
    if (rc) return rc;
    KAGNN_CHECK_ARG(N >= 0 && ldx >= in && ldgx >= in && in_total >= in, "bad shape");
    KAGNN_CHECK_ARG(ln_w && ln_b && g_ln_w && g_ln_b && ws, "null array");
    KAGNN_CHECK_ARG(N == 0 || (x && gx && row_stats && row_sums), "null array");
    return fastkan_bwd(x, ldx, nullptr, out, N, in, out, ng, nullptr, 1.0f, ln_w, ln_b, 0.0f, nullptr,
                       nullptr, row_stats, gx, ldgx, g_ln_w, g_ln_b, nullptr, nullptr, nullptr, ws,
                       ws_bytes, mode, as_stream(stream), 2, const_cast<float*>(row_sums), in_total);
}

// ---------------------------------------------------------------- BatchNorm1d
int kagnn_batchnorm_workspace_bytes(int64_t N, int32_t F, size_t* bytes) {
    KAGNN_CHECK_ARG(bytes && N >= 0 && F >= 1, "bad argument");
    *bytes = bn_ws_bytes(N, F);
    return KAGNN_OK;
}

int kagnn_batchnorm_fwd(const float* x, int64_t ldx, int64_t N, int32_t F, const float* weight, const float* bias,
                        float* running_mean, float* running_var, float momentum, float eps, int32_t training,
                        const float* col_mean, const float* col_m2, float dropout_p, uint64_t dropout_seed,
                        float* y, int64_t ldy, float* save_mean, float* save_rstd, void* ws, size_t ws_bytes,
                        void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(N >= 0 && F >= 1 && ldx >= F && ldy >= F, "bad shape");
    if (N == 0) return KAGNN_OK;
    KAGNN_CHECK_ARG(x && y && save_mean && save_rstd && ws, "null array");
    KAGNN_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr), "running_mean and running_var must both be given or both be null");
    KAGNN_CHECK_ARG(training || running_mean, "eval mode needs the running statistics");
    KAGNN_CHECK_ARG((col_mean == nullptr) == (col_m2 == nullptr), "col_mean and col_m2 must both be given or both be null");
    KAGNN_CHECK_ARG(dropout_p >= 0.0f && dropout_p <= 1.0f, "dropout_p outside [0, 1]");
    return bn_fwd(x, ldx, N, F, weight, bias, running_mean, running_var, momentum, eps, training, col_mean, col_m2, dropout_p,
                  dropout_seed, y, ldy, save_mean, save_rstd, ws, ws_bytes, as_stream(stream));
}

// The statistics half of a training-mode BatchNorm1d forward whose normalising pass is folded into the kernels that read its
// output (round 4; reference node_classification_clean/models.py:198-200): from the column moments (mean, M2) the producing
// kernel left behind -> save_mean, save_rstd (for the backward), the running statistics update, and the per-column affine
//   affine[0][c] = gamma[c] * rstd[c],   affine[1][c] = beta[c] - mean[c] * affine[0][c]
// that kagnn_aggregate_sum_affine / kagnn_gin_kan_layer_fwd_affine / kagnn_kan_linear_*_affine apply to the rows they load.
int kagnn_batchnorm_stats_affine(const float* col_mean, const float* col_m2, int64_t N, int32_t F, const float* gamma, const float* beta,
                                 float* running_mean, float* running_var, float momentum, float eps, float* save_mean,
                                 float* save_rstd, float* affine, void* stream) {
    KAGNN_CHECK_ARG(N >= 1 && F >= 1 && col_mean && col_m2 && save_mean && save_rstd && affine, "bad argument");
    KAGNN_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr), "running_mean and running_var must both be given or both be null");
    return bn_stats_affine(col_mean, col_m2, N, F, gamma, beta, running_mean, running_var, momentum, eps, save_mean, save_rstd, affine,
                           as_stream(stream));
}

int kagnn_batchnorm_bwd(const float* x, int64_t ldx, const float* gy, int64_t ldgy, int64_t N, int32_t F,
                        const float* weight, const float* save_mean, const float* save_rstd, int32_t training,
                        float dropout_p, uint64_t dropout_seed,
                        float* gx, int64_t ldgx, float* g_weight, float* g_bias, void* ws, size_t ws_bytes,
                        void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(N >= 0 && F >= 1 && ldx >= F && ldgy >= F && (gx == nullptr || ldgx >= F), "bad shape");
    if (N == 0) return KAGNN_OK;
    KAGNN_CHECK_ARG(x && gy && save_mean && save_rstd && ws, "null array");
    KAGNN_CHECK_ARG(dropout_p >= 0.0f && dropout_p <= 1.0f, "dropout_p outside [0, 1]");
    return bn_bwd(x, ldx, gy, ldgy, N, F, weight, save_mean, save_rstd, training, dropout_p, dropout_seed, gx, ldgx, g_weight,
                  g_bias, ws, ws_bytes, as_stream(stream));
}

// ---------------------------------------------------------------- GAT attention aggregation
int kagnn_gat_logits(const float* xh, int64_t ldx, int64_t N, int32_t H, int32_t C, const float* att_src,
                     const float* att_dst, float* a_src, float* a_dst, void* stream) {
    KAGNN_CHECK_ARG(N >= 0 && H >= 1 && C >= 1 && ldx >= (int64_t)H * C, "bad shape");
    if (N == 0) return KAGNN_OK;
    KAGNN_CHECK_ARG(xh && att_src && att_dst && a_src && a_dst, "null array");
    return gat_logits(xh, ldx, N, H, C, att_src, att_dst, a_src, a_dst, as_stream(stream));
}

int kagnn_gat_fwd(const float* xh, int64_t ldx, const float* a_src, const float* a_dst, const int32_t* rowptr,
                  const int32_t* col, int64_t N, int32_t H, int32_t C, const float* bias, float* out, int64_t ldo,
                  float* row_max, float* row_sum, const int32_t* hub_seg, int64_t num_hub_seg, int32_t hub_threshold,
                  void* stream) {
    KAGNN_CHECK_ARG(N >= 0 && H >= 1 && C >= 1 && ldx >= (int64_t)H * C && ldo >= (int64_t)H * C, "bad shape");
    if (N == 0) return KAGNN_OK;
    KAGNN_CHECK_ARG(xh && a_src && a_dst && rowptr && out && row_max && row_sum, "null array");
    return gat_fwd(xh, ldx, a_src, a_dst, rowptr, col, N, H, C, bias, out, ldo, row_max, row_sum, hub_seg, num_hub_seg,
                   hub_threshold, as_stream(stream));
}

int kagnn_gat_bwd(const float* xh, int64_t ldx, const float* gout, int64_t ldg, const float* out, int64_t ldo,
                  const float* bias, const float* a_src, const float* a_dst, const float* row_max,
                  const float* row_sum, const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                  const int32_t* rowptr_t, const int32_t* col_t, const int32_t* perm_t, const float* att_src,
                  const float* att_dst, int64_t N, int32_t H, int32_t C, float* edge_scratch, float* self_scratch,
                  float* g_dst, float* g_src, float* gx, int64_t ldgx, const int32_t* hub_seg, int64_t num_hub_seg,
                  int32_t hub_threshold, void* stream) {
    KAGNN_CHECK_ARG(N >= 0 && H >= 1 && C >= 1 && ldx >= (int64_t)H * C && ldg >= (int64_t)H * C && ldo >= (int64_t)H * C &&
                    ldgx >= (int64_t)H * C, "bad shape");
    if (N == 0) return KAGNN_OK;
    KAGNN_CHECK_ARG(xh && gout && out && a_src && a_dst && row_max && row_sum && rowptr && rowptr_t && att_src && att_dst &&
                    self_scratch && g_dst && g_src && gx, "null array");
    return gat_bwd(xh, ldx, gout, ldg, out, ldo, bias, a_src, a_dst, row_max, row_sum, rowptr, col, perm, rowptr_t, col_t,
                   perm_t, att_src, att_dst, N, H, C, edge_scratch, self_scratch, g_dst, g_src, gx, ldgx, hub_seg, num_hub_seg,
                   hub_threshold, as_stream(stream));
}

int kagnn_gat_att_grad_workspace_bytes(int64_t N, int32_t H, int32_t C, size_t* bytes) {
    KAGNN_CHECK_ARG(bytes && N >= 0 && H >= 1 && C >= 1, "bad argument");
    *bytes = gat_att_grad_ws_bytes(N, H, C);
    return KAGNN_OK;
}

int kagnn_gat_att_grad(const float* xh, int64_t ld, const float* g_src, const float* g_dst, int64_t N, int32_t H,
                       int32_t C, float* g_att_src, float* g_att_dst, void* ws, size_t ws_bytes, void* stream) {
    KAGNN_CHECK_ARG(N >= 0 && H >= 1 && C >= 1 && ld >= (int64_t)H * C, "bad shape");
    KAGNN_CHECK_ARG(g_att_src && g_att_dst && ws && (N == 0 || (xh && g_src && g_dst)), "null array");
    return gat_att_grad(xh, ld, g_src, g_dst, N, H, C, g_att_src, g_att_dst, ws, ws_bytes, as_stream(stream));
}

// ---------------------------------------------------------------- harness loss
int kagnn_softmax_xent_workspace_bytes(int64_t N, size_t* bytes) {
    KAGNN_CHECK_ARG(bytes != nullptr && N >= 0, "null output or negative size");
    *bytes = xent_ws_bytes(N);
    return KAGNN_OK;
}

int kagnn_softmax_xent_fwd(const float* logits, int64_t ld, int64_t N, int32_t C, const int64_t* labels,
                           const uint8_t* mask, int32_t pre_softmax, float* loss, float* row_stats, float* count,
                           void* ws, size_t ws_bytes, void* stream) {
    KAGNN_CHECK_ARG(N >= 0 && C >= 1 && ld >= C, "bad shape");
    KAGNN_CHECK_ARG(loss && count && ws && (N == 0 || (logits && labels && row_stats)), "null array");
    return xent_fwd(logits, ld, N, C, (const long*)labels, mask, pre_softmax, loss, row_stats, count, ws, ws_bytes,
                    as_stream(stream));
}

int kagnn_softmax_xent_bwd(const float* logits, int64_t ld, int64_t N, int32_t C, const int64_t* labels,
                           const uint8_t* mask, int32_t pre_softmax, const float* row_stats, const float* count,
                           const float* g_loss, float* g_logits, int64_t ldg, void* stream) {
    KAGNN_CHECK_ARG(N >= 0 && C >= 1 && ld >= C && ldg >= C, "bad shape");
    KAGNN_CHECK_ARG(N == 0 || (logits && labels && row_stats && count && g_loss && g_logits), "null array");
    return xent_bwd(logits, ld, N, C, (const long*)labels, mask, pre_softmax, row_stats, count, g_loss, g_logits, ldg,
                    as_stream(stream));
}

// mean absolute error of two contiguous fp32 vectors (torch.nn.L1Loss, reduction = "mean"): graph_regression/optuna_zinc.py:58
int kagnn_l1_loss_fwd(const float* pred, const float* target, int64_t n, float* loss, void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(n >= 0 && loss && (n == 0 || (pred && target)), "null array or negative size");
    return l1_loss_fwd(pred, target, n, loss, as_stream(stream));
}

int kagnn_l1_loss_bwd(const float* pred, const float* target, int64_t n, const float* g_loss, float* g_pred, void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(n >= 0 && (n == 0 || (pred && target && g_loss && g_pred)), "null array or negative size");
    return l1_loss_bwd(pred, target, n, g_loss, g_pred, as_stream(stream));
}

// the graph-classification scripts' node features, loss and accuracy bookkeeping (classify.hip)
int kagnn_degree_one_hot(const int32_t* rowptr_by_source, int64_t num_nodes, int32_t num_classes, float* x, int64_t ldx, void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(num_nodes >= 0 && num_nodes < 2147483647LL && num_classes >= 1 && ldx >= num_classes, "bad shape");
    KAGNN_CHECK_ARG(num_nodes == 0 || x, "null array");
    return degree_one_hot(rowptr_by_source, num_nodes, num_classes, x, ldx, as_stream(stream));
}

int kagnn_nll_loss_fwd(const float* logp, int64_t ld, int64_t rows, int32_t classes, const int64_t* y, float* loss_mean,
                       float* loss_sum, void* accum, int32_t* flag, void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(rows >= 0 && classes >= 1 && ld >= classes, "bad shape");
    KAGNN_CHECK_ARG((loss_mean || loss_sum || accum) && flag && (rows == 0 || (logp && y)), "null array");
    KAGNN_CHECK_ARG(((uintptr_t)accum & 7) == 0, "the record must be 8-byte aligned");
    return nll_loss_fwd(logp, ld, rows, classes, (const long*)y, loss_mean, loss_sum, accum, flag, as_stream(stream));
}

int kagnn_nll_loss_bwd(const int64_t* y, int64_t rows, int32_t classes, const float* g_loss, int32_t reduction, float* g_logp,
                       int64_t ldg, void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(rows >= 0 && classes >= 1 && ldg >= classes, "bad shape");
    KAGNN_CHECK_ARG(reduction == KAGNN_REDUCTION_MEAN || reduction == KAGNN_REDUCTION_SUM, "reduction must be KAGNN_REDUCTION_MEAN or _SUM");
    KAGNN_CHECK_ARG(rows == 0 || (y && g_loss && g_logp), "null array");
    return nll_loss_bwd((const long*)y, rows, classes, g_loss, reduction, g_logp, ldg, as_stream(stream));
}

// one Adam update of `count` fp32 parameter tensors (HOST arrays of device pointers and element counts; step = 1, 2, ...: the
// number of this update, for the bias corrections): torch.optim.Adam's rule without amsgrad, one launch per 32 tensors
int kagnn_adam_step(int32_t count, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                    const int64_t* numel, float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(count >= 0 && step >= 1 && (count == 0 || (params && grads && exp_avg && exp_avg_sq && numel)), "null array or bad count / step");
    KAGNN_CHECK_ARG(lr >= 0.0f && beta1 >= 0.0f && beta1 < 1.0f && beta2 >= 0.0f && beta2 < 1.0f && eps >= 0.0f, "bad hyper-parameter");
    for (int k = 0; k < count; ++k)
        KAGNN_CHECK_ARG(numel[k] >= 0 && (numel[k] == 0 || (params[k] && grads[k] && exp_avg[k] && exp_avg_sq[k])), "null tensor");
    static_assert(sizeof(long) == sizeof(int64_t), "LP64");
    return adam_step(count, params, grads, exp_avg, exp_avg_sq, reinterpret_cast<const long*>(numel), lr, beta1, beta2, eps, weight_decay,
                     (long)step, as_stream(stream));
}


// the node-classification experiment's bookkeeping after the logits (nodeclass.hip)
int kagnn_node_eval_workspace_bytes(int64_t num_rows, int32_t num_classes, int32_t num_splits, size_t* bytes) {
    KAGNN_CHECK_ARG(bytes != nullptr && num_rows >= 0 && num_classes >= 1 && num_splits >= 1 && num_splits <= 8, "bad argument");
    *bytes = node_eval_ws_bytes(num_rows, num_classes, num_splits);
    return KAGNN_OK;
}

int kagnn_node_eval(const float* logits, int64_t ld, int64_t num_rows, int32_t num_classes, const int64_t* labels,
                    const uint8_t* split_bits, int32_t num_splits, void* records, int32_t* flag, void* workspace,
                    size_t workspace_bytes, void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(num_rows >= 0 && num_classes >= 1 && ld >= num_classes, "bad shape");
    KAGNN_CHECK_ARG(num_splits >= 1 && num_splits <= 8, "num_splits must be 1..8 (one bit of the row's byte each)");
    KAGNN_CHECK_ARG(records && flag && (num_rows == 0 || (logits && labels && split_bits)), "null array");
    KAGNN_CHECK_ARG(((uintptr_t)records & 7) == 0, "the records must be 8-byte aligned");
    static_assert(sizeof(long) == sizeof(int64_t), "LP64");
    return node_eval(logits, ld, num_rows, num_classes, (const long*)labels, split_bits, num_splits, records, flag, workspace,
                     workspace_bytes, as_stream(stream));
}

int kagnn_early_stop_update(const void* eval_records, int32_t num_splits, int32_t val_split, void* state, void* history,
                            int32_t max_epochs, void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(num_splits >= 1 && num_splits <= 8 && val_split >= 0 && val_split < num_splits && max_epochs >= 0, "bad split or epoch count");
    KAGNN_CHECK_ARG(eval_records && state, "null array");
    KAGNN_CHECK_ARG(((uintptr_t)eval_records & 7) == 0 && ((uintptr_t)history & 7) == 0 && ((uintptr_t)state & 3) == 0, "misaligned record");
    return early_stop_update(eval_records, num_splits, val_split, state, history, max_epochs, as_stream(stream));
}

int kagnn_copy_if(const int32_t* flag, int32_t count, void* const* dst, const void* const* src, const int64_t* bytes, void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(flag && count >= 0 && (count == 0 || (dst && src && bytes)), "null array or bad count");
    for (int k = 0; k < count; ++k) {
        KAGNN_CHECK_ARG(bytes[k] >= 0 && (bytes[k] & 3) == 0, "sizes are multiples of 4 bytes");
        KAGNN_CHECK_ARG(bytes[k] == 0 || (dst[k] && src[k]), "null tensor");
        KAGNN_CHECK_ARG((((uintptr_t)dst[k] | (uintptr_t)src[k]) & 3) == 0, "pointers are 4-byte aligned");
    }
    return copy_if(flag, count, dst, src, reinterpret_cast<const long*>(bytes), as_stream(stream));
}

// the graph-regression experiment's bookkeeping around the models (regress.hip)
int kagnn_l1_loss_meter_fwd(const float* pred, int64_t ldp, const float* target, int64_t ldt, int64_t rows, int32_t targets,
                            const float* scale, float* loss_mean, void* meter, void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(targets >= 1 && targets <= KAGNN_REGRESSION_MAX_TARGETS, "targets must be 1..KAGNN_REGRESSION_MAX_TARGETS (32)");
    KAGNN_CHECK_ARG(rows >= 0 && ldp >= targets && ldt >= targets, "bad shape");
    KAGNN_CHECK_ARG((loss_mean || meter) && (rows == 0 || (pred && target)), "null array");
    KAGNN_CHECK_ARG(((uintptr_t)meter & 7) == 0, "the record must be 8-byte aligned");
    return l1_loss_meter_fwd(pred, ldp, target, ldt, rows, targets, scale, loss_mean, meter, as_stream(stream));
}

int kagnn_regression_epoch_update(void* train_meter, void* val_meter, void* test_meter, int64_t n_train, int64_t n_val, int64_t n_test,
                                  void* state, double* history, int32_t max_epochs, void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(train_meter && val_meter && state && max_epochs >= 0, "null record or negative epoch count");
    KAGNN_CHECK_ARG((((uintptr_t)train_meter | (uintptr_t)val_meter | (uintptr_t)test_meter | (uintptr_t)history) & 7) == 0 &&
                    ((uintptr_t)state & 3) == 0, "misaligned record");
    return regression_epoch_update(train_meter, val_meter, test_meter, n_train, n_val, n_test, state, history, max_epochs,
                                   as_stream(stream));
}

// ---------------------------------------------------------------- dense layer of the MLP baselines (linear.hip)
// exact fp32 in every precision mode; the weight gradient is a fixed-order slab reduction (no atomics)

int kagnn_linear_bwd_weight_workspace_bytes(int64_t N, int32_t in, int32_t out, size_t* bytes) {
    KAGNN_CHECK_ARG(bytes != nullptr && N >= 0 && in >= 1 && out >= 1, "bad argument");
    *bytes = linear_dw_ws_bytes(N, in, out);
    return KAGNN_OK;
}

int kagnn_linear_fwd(const float* x, int64_t ldx, int64_t N, int32_t in, const float* W, const float* bias, int32_t out,
                     int32_t relu, float* y, int64_t ldy, void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(in >= 1 && out >= 1, "in_features/out_features must be >= 1");
    KAGNN_CHECK_ARG(N >= 0 && ldx >= in && ldy >= out, "bad shape");
    KAGNN_CHECK_ARG(relu == 0 || relu == 1, "relu must be 0 or 1");
    if (N == 0) return KAGNN_OK;
    KAGNN_CHECK_ARG(x && W && y, "null array");
    return linear_fwd(x, ldx, N, in, W, bias, out, relu, y, ldy, as_stream(stream));
}

int kagnn_linear_bwd_input(const float* gy, int64_t ldgy, const float* y, int64_t ldy, int64_t N, int32_t out, const float* W,
                           int32_t in, float* gx, int64_t ldgx, void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(in >= 1 && out >= 1, "in_features/out_features must be >= 1");
    KAGNN_CHECK_ARG(N >= 0 && ldgy >= out && ldgx >= in && (!y || ldy >= out), "bad shape");
    if (N == 0) return KAGNN_OK;
    KAGNN_CHECK_ARG(gy && W && gx, "null array");
    return linear_dx(gy, ldgy, y, ldy, N, out, W, in, gx, ldgx, as_stream(stream));
}

int kagnn_linear_bwd_weight(const float* x, int64_t ldx, const float* gy, int64_t ldgy, const float* y, int64_t ldy, int64_t N,
                            int32_t in, int32_t out, float* gW, float* gb, void* ws, size_t ws_bytes, void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(in >= 1 && out >= 1, "in_features/out_features must be >= 1");
    KAGNN_CHECK_ARG(N >= 0 && ldx >= in && ldgy >= out && (!y || ldy >= out), "bad shape");
    KAGNN_CHECK_ARG(gW != nullptr, "null array");
    if (N == 0) {                                   // an empty sum: zeros, no kernel
        KAGNN_HIP(hipMemsetAsync(gW, 0, (size_t)in * out * sizeof(float), as_stream(stream)));
        if (gb) KAGNN_HIP(hipMemsetAsync(gb, 0, (size_t)out * sizeof(float), as_stream(stream)));
        return KAGNN_OK;
    }
    KAGNN_CHECK_ARG(x && gy && ws, "null array");
    KAGNN_CHECK_ARG(((uintptr_t)ws & 15) == 0, "the workspace must be 16-byte aligned");
    return linear_dw(x, ldx, gy, ldgy, y, ldy, N, in, out, gW, gb, (float*)ws, ws_bytes, as_stream(stream));
}

// ---------------------------------------------------------------- dense attention, bias after the softmax (attention.hip)
// exact fp32 in every precision mode; every sum has one owner and a fixed order (no atomics)

static int attention_shape_ok(const char* fn, int64_t B, int64_t Q, int64_t K, int32_t H, int32_t c) {
    KAGNN_CHECK_ARG_AS(fn, B >= 0 && Q >= 0 && K >= 0 && B <= 0x7fffffffL && Q <= 0x7fffffffL && K <= 0x7fffffffL, "batch / num_queries / num_keys must be 0 .. 2^31 - 1");
    KAGNN_CHECK_ARG_AS(fn, H >= 1, "num_heads must be >= 1");
    if (c < 1 || c > 128) return fail(KAGNN_ERR_UNSUPPORTED, "%s: head_dim %ld is outside 1..128", fn, (long)c);
    KAGNN_CHECK_ARG_AS(fn, (int64_t)H * c <= 0x7fffffffL, "num_heads * head_dim must fit int32");
    return KAGNN_OK;
}

int kagnn_attention_fwd(const float* wq, int64_t ldq, const float* wk, int64_t ldk, const float* wv, int64_t ldv, const float* bias,
                        int64_t bias_bs, int64_t bias_rs, const float* gate, int64_t ldgate, int64_t B, int64_t Q, int64_t K,
                        int32_t H, int32_t c, float scale, float* o, int64_t ldo, float* o_ungated, int64_t ldou, float* stats,
                        void* stream) {
    KAGNN_STAGE(stream);
    if (int rc = attention_shape_ok(__func__, B, Q, K, H, c)) return rc;
    const int64_t hc = (int64_t)H * c;
    KAGNN_CHECK_ARG(ldq >= hc && ldk >= hc && ldv >= hc && ldo >= hc, "a row stride is below num_heads * head_dim");
    KAGNN_CHECK_ARG(!gate || ldgate >= hc, "the gate's row stride is below num_heads * head_dim");
    KAGNN_CHECK_ARG(!o_ungated || ldou >= hc, "o_ungated's row stride is below num_heads * head_dim");
    KAGNN_CHECK_ARG(!bias || (bias_bs >= 0 && bias_rs >= 0), "negative bias stride");
    KAGNN_CHECK_ARG(!o_ungated || stats, "o_ungated is written together with stats");
    if (B * Q == 0) return KAGNN_OK;
    KAGNN_CHECK_ARG(wq && o && (K == 0 || (wk && wv)), "null array");
    return attention_fwd(wq, ldq, wk, ldk, wv, ldv, bias, bias_bs, bias_rs, gate, ldgate, B, Q, K, H, c, scale, o, ldo, o_ungated, ldou,
                         stats, as_stream(stream));
}

int kagnn_attention_bwd_workspace_bytes(int64_t B, int64_t Q, int64_t K, int32_t H, int32_t c, int32_t has_gate, size_t* bytes) {
    KAGNN_CHECK_ARG(bytes != nullptr, "null bytes pointer");
    if (int rc = attention_shape_ok(__func__, B, Q, K, H, c)) return rc;
    *bytes = attention_bwd_ws_bytes(B, Q, K, H, c, has_gate != 0);
    return KAGNN_OK;
}

int kagnn_attention_bwd(const float* g_out, int64_t ldgo, const float* wq, int64_t ldq, const float* wk, int64_t ldk, const float* wv,
                        int64_t ldv, const float* bias, int64_t bias_bs, int64_t bias_rs, const float* gate, int64_t ldgate,
                        const float* o_ungated, int64_t ldou, const float* stats, int64_t B, int64_t Q, int64_t K, int32_t H, int32_t c,
                        float scale, float* g_wq, int64_t ldgq, float* g_wk, int64_t ldgk, float* g_wv, int64_t ldgv, float* g_bias,
                        int64_t gb_bs, int64_t gb_rs, float* g_gate, int64_t ldgg, void* ws, size_t ws_bytes, void* stream) {
    KAGNN_STAGE(stream);
    if (int rc = attention_shape_ok(__func__, B, Q, K, H, c)) return rc;
    const int64_t hc = (int64_t)H * c;
    KAGNN_CHECK_ARG(ldgo >= hc && ldq >= hc && ldk >= hc && ldv >= hc && ldou >= hc && ldgq >= hc && ldgk >= hc && ldgv >= hc,
                    "a row stride is below num_heads * head_dim");
    KAGNN_CHECK_ARG(!gate || (ldgate >= hc && ldgg >= hc), "a gate row stride is below num_heads * head_dim");
    KAGNN_CHECK_ARG(!bias || (bias_bs >= 0 && bias_rs >= 0), "negative bias stride");
    KAGNN_CHECK_ARG(!g_bias || (gb_rs >= K && (B <= 1 || gb_bs >= Q * gb_rs)), "g_bias is a dense [B, Q, K] result: overlapping strides");
    KAGNN_CHECK_ARG((gate != nullptr) == (g_gate != nullptr), "g_gate goes with gate");
    if (B * (Q + K) == 0) return KAGNN_OK;
    KAGNN_CHECK_ARG(ws != nullptr && ((uintptr_t)ws & 15) == 0, "the workspace must be non-null and 16-byte aligned");
    KAGNN_CHECK_ARG((Q == 0 || (g_out && wq && o_ungated && stats && g_wq)) && (K == 0 || (wk && wv && g_wk && g_wv)), "null array");
    return attention_bwd(g_out, ldgo, wq, ldq, wk, ldk, wv, ldv, bias, bias_bs, bias_rs, gate, ldgate, o_ungated, ldou, stats, B, Q, K, H,
                         c, scale, g_wq, ldgq, g_wk, ldgk, g_wv, ldgv, g_bias, gb_bs, gb_rs, g_gate, ldgg, (float*)ws, ws_bytes,
                         as_stream(stream));
}

// ---------------------------------------------------------------- per-edge activations of a KANLinear (kan_edge.hip)
// exact fp32 in every precision mode (no `mode` argument); spline orders 1..4; fixed-order slab reductions (no atomics)

int kagnn_kan_edge_abs_sum_workspace_bytes(int64_t N, int32_t in, int32_t out, int32_t G, int32_t K, size_t* bytes) {
    int rc = check_kan_dims(__func__, in, out, G, K, KAGNN_PREC_FP32);
    if (rc) return rc;
    KAGNN_CHECK_ARG(bytes != nullptr && N >= 0, "null output or negative row count");
    *bytes = kan_edge_abs_sum_ws_bytes(N, in, out);
    return KAGNN_OK;
}

int kagnn_kan_edge_abs_sum(const float* x, int64_t ldx, int64_t N, const float* knots, int32_t per_feature_knots, int32_t in,
                           int32_t out, int32_t G, int32_t K, const float* bw, const float* sw, const float* sc, float* S,
                           int64_t ldS, void* ws, size_t ws_bytes, void* stream) {
    KAGNN_STAGE(stream);
    int rc = check_kan_dims(__func__, in, out, G, K, KAGNN_PREC_FP32);
    if (rc) return rc;
    KAGNN_CHECK_ARG(N >= 0 && ldx >= in && ldS >= in, "bad shape");
    KAGNN_CHECK_ARG(per_feature_knots == 0 || per_feature_knots == 1, "per_feature_knots must be 0 or 1");
    KAGNN_CHECK_ARG(S != nullptr, "null array");
    if (N == 0) {                                   // an empty sum: zeros, no kernel
        KAGNN_HIP(hipMemset2DAsync(S, (size_t)ldS * sizeof(float), 0, (size_t)in * sizeof(float), (size_t)out, as_stream(stream)));
        return KAGNN_OK;
    }
    KAGNN_CHECK_ARG(x && knots && sw && ws, "null array");          // base_weight / spline_scaler NULL: the layer has none
    return kan_edge_abs_sum(x, ldx, N, knots, per_feature_knots != 0, in, out, G, K, bw, sw, sc, S, ldS, (float*)ws, ws_bytes,
                            as_stream(stream));
}

int kagnn_kan_edge_abs_sum_bwd_workspace_bytes(int64_t N, int32_t in, int32_t out, int32_t G, int32_t K, size_t* bytes) {
    int rc = check_kan_dims(__func__, in, out, G, K, KAGNN_PREC_FP32);
    if (rc) return rc;
    KAGNN_CHECK_ARG(bytes != nullptr && N >= 0, "null output or negative row count");
    *bytes = kan_edge_abs_sum_bwd_ws_bytes(N, in, out, G + K);
    return KAGNN_OK;
}

int kagnn_kan_edge_abs_sum_bwd(const float* x, int64_t ldx, int64_t N, const float* knots, int32_t per_feature_knots, int32_t in,
                               int32_t out, int32_t G, int32_t K, const float* bw, const float* sw, const float* sc,
                               const float* gS, int64_t ldgS, float* g_bw, float* g_sw, float* g_sc, float* gx, int64_t ldgx,
                               void* ws, size_t ws_bytes, void* stream) {
    KAGNN_STAGE(stream);
    int rc = check_kan_dims(__func__, in, out, G, K, KAGNN_PREC_FP32);
    if (rc) return rc;
    KAGNN_CHECK_ARG(N >= 0 && ldx >= in && ldgS >= in && (!gx || ldgx >= in), "bad shape");
    KAGNN_CHECK_ARG(per_feature_knots == 0 || per_feature_knots == 1, "per_feature_knots must be 0 or 1");
    KAGNN_CHECK_ARG(!g_bw || bw, "a base_weight gradient needs base_weight");
    KAGNN_CHECK_ARG(!g_sc || sc, "a spline_scaler gradient needs spline_scaler");
    if (N == 0) {                                   // empty sums: zeros, no kernel (gx has no rows)
        const size_t e = (size_t)in * out * sizeof(float);
        if (g_bw) KAGNN_HIP(hipMemsetAsync(g_bw, 0, e, as_stream(stream)));
        if (g_sw) KAGNN_HIP(hipMemsetAsync(g_sw, 0, e * (G + K), as_stream(stream)));
        if (g_sc) KAGNN_HIP(hipMemsetAsync(g_sc, 0, e, as_stream(stream)));
        return KAGNN_OK;
    }
    KAGNN_CHECK_ARG(x && knots && sw && gS, "null array");
    KAGNN_CHECK_ARG(!(g_bw || g_sw || g_sc) || ws, "the parameter gradients need the workspace");
    return kan_edge_abs_sum_bwd(x, ldx, N, knots, per_feature_knots != 0, in, out, G, K, bw, sw, sc, gS, ldgS, g_bw, g_sw, g_sc, gx,
                                ldgx, (float*)ws, ws_bytes, as_stream(stream));
}

int kagnn_kan_edge_curves(const float* t, int64_t ldt, int64_t P, const float* knots, int32_t per_feature_knots, int32_t in,
                          int32_t out, int32_t G, int32_t K, const float* bw, const float* sw, const float* sc, float* phi,
                          void* stream) {
    KAGNN_STAGE(stream);
    int rc = check_kan_dims(__func__, in, out, G, K, KAGNN_PREC_FP32);
    if (rc) return rc;
    KAGNN_CHECK_ARG(P >= 0 && (ldt == 0 || ldt >= in), "bad shape");
    KAGNN_CHECK_ARG(per_feature_knots == 0 || per_feature_knots == 1, "per_feature_knots must be 0 or 1");
    if (P == 0) return KAGNN_OK;
    KAGNN_CHECK_ARG(t && knots && sw && phi, "null array");
    return kan_edge_curves(t, ldt, P, knots, per_feature_knots != 0, in, out, G, K, bw, sw, sc, phi, as_stream(stream));
}

int kagnn_kan_edge_moments_workspace_bytes(int64_t N, int32_t in, int32_t out, int32_t G, int32_t K, size_t* bytes) {
    int rc = check_kan_dims(__func__, in, out, G, K, KAGNN_PREC_FP32);
    if (rc) return rc;
    KAGNN_CHECK_ARG(bytes != nullptr && N >= 0, "null output or negative row count");
    *bytes = kan_edge_moments_ws_bytes(N, in, out);
    return KAGNN_OK;
}

int kagnn_kan_edge_moments(const float* x, int64_t ldx, int64_t N, const float* knots, int32_t per_feature_knots, int32_t in,
                           int32_t out, int32_t G, int32_t K, const float* bw, const float* sw, const float* sc, float* mean,
                           int64_t ld_mean, float* m2, int64_t ld_m2, void* ws, size_t ws_bytes, void* stream) {
    KAGNN_STAGE(stream);
    int rc = check_kan_dims(__func__, in, out, G, K, KAGNN_PREC_FP32);
    if (rc) return rc;
    KAGNN_CHECK_ARG(N >= 0 && ldx >= in && (!mean || ld_mean >= in) && (!m2 || ld_m2 >= in), "bad shape");
    KAGNN_CHECK_ARG(per_feature_knots == 0 || per_feature_knots == 1, "per_feature_knots must be 0 or 1");
    KAGNN_CHECK_ARG(mean != nullptr || m2 != nullptr, "mean and m2 are both null");
    if (N == 0) {                                   // no rows: zeros, no kernel
        const size_t w = (size_t)in * sizeof(float);
        if (mean) KAGNN_HIP(hipMemset2DAsync(mean, (size_t)ld_mean * sizeof(float), 0, w, (size_t)out, as_stream(stream)));
        if (m2) KAGNN_HIP(hipMemset2DAsync(m2, (size_t)ld_m2 * sizeof(float), 0, w, (size_t)out, as_stream(stream)));
        return KAGNN_OK;
    }
    KAGNN_CHECK_ARG(x && knots && sw && ws, "null array");          // base_weight / spline_scaler NULL: the layer has none
    return kan_edge_moments(x, ldx, N, knots, per_feature_knots != 0, in, out, G, K, bw, sw, sc, mean, ld_mean, m2, ld_m2, (float*)ws,
                            ws_bytes, as_stream(stream));
}

// ---------------------------------------------------------------- symbolic fits of edge functions (symbolic.hip)
static int check_symbolic_dims(const char* fn, int64_t N, int32_t in, int32_t out, int32_t F) {
    KAGNN_CHECK_ARG_AS(fn, N >= 0 && N < 2147483647LL, "num_rows outside [0, 2^31 - 1)");
    KAGNN_CHECK_ARG_AS(fn, in >= 1 && out >= 1 && in <= 65535, "in_features must be 1..65535, out_features >= 1");
    KAGNN_CHECK_ARG_AS(fn, F >= 1 && F <= KAGNN_SYMBOLIC_NUM_FUNCTIONS, "num_functions must be 1..19");
    return KAGNN_OK;
}

int kagnn_symbolic_fit_workspace_bytes(int64_t N, int32_t in, int32_t out, int32_t F, size_t* bytes) {
    KAGNN_CHECK_ARG(bytes != nullptr, "null output");
    int rc = check_symbolic_dims(__func__, N, in, out, F);
    if (rc) return rc;
    *bytes = symbolic_ws_bytes(N, in, out, F);
    return KAGNN_OK;
}

int kagnn_symbolic_fit(const float* x, int64_t ldx, const float* phi, int64_t N, int32_t in, int32_t out, const int32_t* functions,
                       int32_t F, float a_lo, float a_hi, float b_lo, float b_hi, int32_t grid_number, int32_t iterations,
                       float* params, float* r2, float* tables, float* ranges, int32_t* winners, void* ws, size_t ws_bytes,
                       void* stream) {
    KAGNN_STAGE(stream);
    int rc = check_symbolic_dims(__func__, N, in, out, F);
    if (rc) return rc;
    KAGNN_CHECK_ARG(functions != nullptr, "functions is null (a host array of library ids)");
    for (int f = 0; f < F; ++f) {
        KAGNN_CHECK_ARG(functions[f] >= 0 && functions[f] < KAGNN_SYMBOLIC_NUM_FUNCTIONS, "unknown function id (the library has ids 0..18)");
        for (int g = 0; g < f; ++g) KAGNN_CHECK_ARG(functions[g] != functions[f], "a function id is listed twice");
    }
    KAGNN_CHECK_ARG(grid_number >= 3 && grid_number <= KAGNN_SYMBOLIC_MAX_GRID, "grid_number must be 3..128");
    KAGNN_CHECK_ARG(iterations >= 1 && iterations <= KAGNN_SYMBOLIC_MAX_ITERATIONS, "iterations must be 1..8");
    KAGNN_CHECK_ARG(a_lo - a_lo == 0.0f && a_hi - a_hi == 0.0f && b_lo - b_lo == 0.0f && b_hi - b_hi == 0.0f, "a non-finite range");
    KAGNN_CHECK_ARG(ldx >= in, "ldx smaller than in_features");
    KAGNN_CHECK_ARG(params && r2, "null output");
    if (N == 0) {                                            // nothing to fit: zeros, no launch
        const size_t ne = (size_t)F * out * in;
        KAGNN_HIP(hipMemsetAsync(params, 0, ne * 4 * sizeof(float), as_stream(stream)));
        KAGNN_HIP(hipMemsetAsync(r2, 0, ne * sizeof(float), as_stream(stream)));
        const size_t per_it = ne * (size_t)iterations;
        if (tables) KAGNN_HIP(hipMemsetAsync(tables, 0, per_it * grid_number * grid_number * sizeof(float), as_stream(stream)));
        if (ranges) KAGNN_HIP(hipMemsetAsync(ranges, 0, per_it * 4 * sizeof(float), as_stream(stream)));
        if (winners) KAGNN_HIP(hipMemsetAsync(winners, 0, per_it * sizeof(int32_t), as_stream(stream)));
        return KAGNN_OK;
    }
    KAGNN_CHECK_ARG(x && phi && ws, "null array");
    return symbolic_fit(x, ldx, phi, N, in, out, functions, F, a_lo, a_hi, b_lo, b_hi, grid_number, iterations, params, r2, tables,
                        ranges, winners, ws, ws_bytes, as_stream(stream));
}

// ---------------------------------------------------------------- fixed symbolic edges (symbolic_edges.hip)
static int check_symbolic_edges_dims(const char* fn, int64_t E, int32_t in, int32_t out) {
    KAGNN_CHECK_ARG_AS(fn, in >= 1 && out >= 1, "in_features and out_features must be >= 1");
    KAGNN_CHECK_ARG_AS(fn, E >= 0 && E <= (int64_t)in * out && E < (1LL << 28), "num_edges must be 0..out_features * in_features (below 2^28)");
    return KAGNN_OK;
}

int kagnn_symbolic_edges_plan_bytes(int64_t E, int32_t in, int32_t out, size_t* bytes) {
    KAGNN_CHECK_ARG(bytes != nullptr, "null output");
    int rc = check_symbolic_edges_dims(__func__, E, in, out);
    if (rc) return rc;
    *bytes = symbolic_edges_plan_bytes(E, in, out);
    return KAGNN_OK;
}

int kagnn_symbolic_edges_plan(const int32_t* edges_host, int64_t E, int32_t in, int32_t out, int32_t* plan_host, size_t plan_bytes) {
    int rc = check_symbolic_edges_dims(__func__, E, in, out);
    if (rc) return rc;
    KAGNN_CHECK_ARG(plan_host != nullptr && (E == 0 || edges_host != nullptr), "null array");
    KAGNN_CHECK_ARG(plan_bytes >= symbolic_edges_plan_bytes(E, in, out), "plan buffer too small");
    return symbolic_edges_plan(edges_host, E, in, out, plan_host);
}

int kagnn_symbolic_edges_bwd_workspace_bytes(int64_t N, int64_t E, size_t* bytes) {
    KAGNN_CHECK_ARG(bytes != nullptr, "null output");
    KAGNN_CHECK_ARG(N >= 0 && N < 2147483647LL, "num_rows outside [0, 2^31 - 1)");
    KAGNN_CHECK_ARG(E >= 0 && E < (1LL << 28), "num_edges outside [0, 2^28)");
    *bytes = symbolic_edges_bwd_ws_bytes(N, E);
    return KAGNN_OK;
}

int kagnn_symbolic_edges_fwd(const float* x, int64_t ldx, int64_t N, int32_t in, int32_t out, const int32_t* plan_host,
                             const int32_t* plan_dev, const float* affine, const float* y_in, int64_t ldyin, float* y, int64_t ldy,
                             void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(in >= 1 && out >= 1, "in_features and out_features must be >= 1");
    KAGNN_CHECK_ARG(N >= 0 && N < 2147483647LL, "num_rows outside [0, 2^31 - 1)");
    KAGNN_CHECK_ARG(ldx >= in && ldy >= out && (!y_in || ldyin >= out), "a leading dimension is smaller than its width");
    KAGNN_CHECK_ARG(plan_host != nullptr, "plan_host is null");
    if (N == 0) return KAGNN_OK;
    KAGNN_CHECK_ARG(y != nullptr && y != y_in, "y is null or y_in itself");
    if (plan_host[1] == 0) {                                 // no edge: y = y_in or 0, no launch
        const size_t w = (size_t)out * sizeof(float);
        if (y_in) KAGNN_HIP(hipMemcpy2DAsync(y, (size_t)ldy * sizeof(float), y_in, (size_t)ldyin * sizeof(float), w, (size_t)N,
                                             hipMemcpyDeviceToDevice, as_stream(stream)));
        else KAGNN_HIP(hipMemset2DAsync(y, (size_t)ldy * sizeof(float), 0, w, (size_t)N, as_stream(stream)));
        return KAGNN_OK;
    }
    KAGNN_CHECK_ARG(x && plan_dev && affine, "null array");
    return symbolic_edges_fwd(x, ldx, N, in, out, plan_host, plan_dev, affine, y_in, ldyin, y, ldy, as_stream(stream));
}

int kagnn_symbolic_edges_bwd(const float* x, int64_t ldx, const float* gy, int64_t ldgy, int64_t N, int32_t in, int32_t out,
                             const int32_t* plan_host, const int32_t* plan_dev, const float* affine, float* gx, int64_t ldgx,
                             float* g_affine, void* ws, size_t ws_bytes, void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(in >= 1 && out >= 1, "in_features and out_features must be >= 1");
    KAGNN_CHECK_ARG(N >= 0 && N < 2147483647LL, "num_rows outside [0, 2^31 - 1)");
    KAGNN_CHECK_ARG(ldx >= in && ldgy >= out && (!gx || ldgx >= in), "a leading dimension is smaller than its width");
    KAGNN_CHECK_ARG(plan_host != nullptr, "plan_host is null");
    const int64_t E = plan_host[1];
    KAGNN_CHECK_ARG(E == 0 || g_affine != nullptr, "g_affine is null");
    if (N == 0 || E == 0) {                                  // empty sums: zeros, no launch
        if (gx && N > 0) KAGNN_HIP(hipMemset2DAsync(gx, (size_t)ldgx * sizeof(float), 0, (size_t)in * sizeof(float), (size_t)N, as_stream(stream)));
        if (E > 0 && E <= (int64_t)in * out) KAGNN_HIP(hipMemsetAsync(g_affine, 0, (size_t)E * 4 * sizeof(float), as_stream(stream)));
        return KAGNN_OK;
    }
    KAGNN_CHECK_ARG(x && gy && plan_dev && affine && ws, "null array");
    return symbolic_edges_bwd(x, ldx, gy, ldgy, N, in, out, plan_host, plan_dev, affine, gx, ldgx, g_affine, ws, ws_bytes,
                              as_stream(stream));
}

// ---------------------------------------------------------------- direct peer-to-peer exchange (p2p.hip)

int kagnn_p2p_reduce_scatter(const float* const* parts, int32_t world, int32_t rank, int64_t N, int32_t out, int64_t ld, float* y,
                             int64_t ldy, void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(parts && N >= 0 && out >= 1 && ld >= out && (N == 0 || y), "bad argument");
    return p2p_reduce_scatter(parts, world, rank, N, out, ld, y, ldy, as_stream(stream));
}

int kagnn_p2p_all_gather(const float* const* shards, int32_t world, int64_t N, int32_t w, int64_t lds, float* g, int64_t ldg,
                         void* stream) {
    KAGNN_STAGE(stream);
    KAGNN_CHECK_ARG(shards && N >= 0 && w >= 1 && lds >= w && ldg >= (int64_t)w * world && (N == 0 || g), "bad argument");
    return p2p_all_gather(shards, world, N, w, lds, g, ldg, as_stream(stream));
}


}  // extern "C"
#pragma GCC visibility pop
