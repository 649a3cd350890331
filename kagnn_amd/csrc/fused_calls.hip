// The fused calls of libkagnn_hip.so: one KAN-GIN / KAN-GINE convolution per call, the whole GINE message-passing stack per call,
// the whole graph-regression model per call.  Host orchestration only: each is a fixed sequence of the per-operation entry points
// and launchers (same kernels, same order, same bits as composing them), on ONE caller-provided workspace whose layout is written
// down once per call family (LayerLayout, StackLayout, KmLayout) and read by the size query and by both directions.
#include "host.h"
#include <algorithm>
#include <mutex>

using namespace kagnn;

namespace {
// ---------------------------------------------------------------- one KAN-GIN convolution per call
// the graph side of a convolution: the CSR by destination (forward) or its transpose (backward) with its hub segments
struct GraphSide {
    const int32_t* rowptr; const int32_t* col; const int32_t* hub_seg; int64_t num_hub_seg; int32_t hub_threshold; float self_scale;
};
// the KAN chain of a convolution.  The tables are declared as the backward reads them; the forward, which fills the activations
// and the packs, casts once (bw: forward only -- backward the packs carry it).
struct KanChain {
    int64_t N; int32_t L; const int32_t* widths;
    const float* const* bw; const float* const* sw; const float* const* sc;
    const float* const* acts; const void* const* pack_fwd; const void* const* pack_dx;
    const float* knots; int32_t G, K, mode;
};
// the gathered matrix of the forward (in_col_scale / in_col_shift: it exists only as  scale * x + shift) and where the column
// moments of the output go (both or neither)
struct LayerIn {
    const void* x; int32_t x_dtype; int64_t ldx; const float* in_col_scale; const float* in_col_shift; float* col_mean; float* col_m2;
};
// the gradients of the backward: gy in; gx (optional; + gx_addend) and the weight gradients out
struct LayerGrads {
    const float* gy; int64_t ldgy; void* gx; int32_t gx_dtype; int64_t ldgx; int32_t bf16_gather; const float* gx_addend; int64_t ld_addend;
    float* const* g_bw; float* const* g_sw; float* const* g_sc;
};

// GINE message passing around the same chain (reference graph_regression/models.py:98,107-119: GINEConv(KAN)): the aggregation of
// the forward is kagnn_aggregate_gine (relu(x_j + e_ij) messages, edge attributes in ORIGINAL edge order through `perm`), the last
// step of the backward kagnn_aggregate_gine_bwd on the transposed structure (also the edge-attribute gradient)
struct GineStage {
    const float* x; int64_t ldx; const float* ea; int64_t lde; const int32_t* perm;      // forward: perm of the CSR; backward: of its transpose
    float* g_ea; int64_t ldge;                                                           // backward only (g_ea may be null)
    int accumulate_g_ea = 0;                                                             // backward: g_ea += (the stack's later convolutions)
    int prepacked = 0;                                                                   // forward: the packs were made by the caller (one launch for a whole stack)
};
// the BatchNorm1d (training mode) that follows the layer, for kagnn_gin_kan_layer_bwd_bn
struct BnStage { const float* y; int64_t ldy; const float* weight; const float* mean; const float* rstd; float* g_weight; float* g_bias; };
// the statistics of the PREVIOUS norm's backward, produced by this layer's transposed aggregation (kagnn_gin_kan_layer_bwd_bn_sums):
// prev_y = that norm's input (this convolution's forward input before the folded affine), its saved mean / rstd, sums = out [2][in]
struct StatsOut { const float* y; int64_t ldy; const float* mean; const float* rstd; float* sums; };
// one convolution's piece of a stack call's arena of weight-gradient row slabs (LayerLayout::dw_piece places the layers in it)
// and the record its slab reductions go to instead of being launched (DwDefer, common.h)
struct DwPiece { unsigned char* base; DwDefer* defer; };

// Byte offsets and sizes inside the workspace of one fused-layer call: filled by layer_layout (+ layer_layout_optional), read by
// the size queries and by both directions.
//   forward:   hub partials | forward scratch | fused-aggregation fix-up
//   backward:  hub partials | dW slabs | two gradient matrices | optional BatchNorm stage | optional previous-norm statistics
// The two optional blocks FOLLOW bwd_total (the number kagnn_gin_kan_layer_workspace_bytes reports) in THIS order: the Python host
// path (ops._chain_bwd_buffers, graph_ops.py) sizes one buffer as that total plus the two public extras and relies on the order.
struct LayerLayout {
    // forward (hub partials at offset 0; the launchers behind them are told everything up to the end of the workspace, slack included)
    size_t fwd_hub_bytes, fwd_scratch, fwd_scratch_bytes, fwd_fix, fwd_fix_bytes, fwd_total;
    // backward (hub partials at offset 0)
    size_t bwd_hub_bytes, dw, dw_bytes, g[2], bwd_total;
    size_t bn, bn_ws_bytes, bn_tab, bn_bytes, stats, stats_bytes, bwd_total_all;
    // layer l's slab area inside a DwPiece, last layer first (the order the backward runs in)
    size_t dw_piece[8], dw_piece_bytes[8], dw_pieces_bytes;
    int wmax;                            // the chain's widest INPUT: the width of the two gradient matrices
};

// the optional blocks behind bwd_total: the BatchNorm stage (out = the norm's width, 0: absent) and the previous norm's statistics
// (f0 = the layer's input width, 0: absent)
void layer_layout_optional(LayerLayout& y, int64_t N, int out, int f0, int64_t num_hub_seg_t) {
    y.bn = y.bwd_total;
    y.bn_ws_bytes = out ? bn_ws_bytes(N, out) : 0;
    y.bn_tab = y.bn + al256z(y.bn_ws_bytes);                  // [4][out rounded up to 64] floats: BnBack::tab
    y.bn_bytes = out ? al256z(y.bn_ws_bytes) + al256z(4 * (size_t)((out + 63) & ~63) * sizeof(float)) : 0;
    y.stats = y.bn + y.bn_bytes;
    y.stats_bytes = f0 ? al256z(bn_stats_fold_bytes(aggregate_stats_rows(N, f0, num_hub_seg_t), f0)) : 0;
    y.bwd_total_all = y.stats + y.stats_bytes;
}

// (mode already rewritten by the caller's ModeScope; N, L and widths checked by the caller.  Errors report under the name of the
// query whose numbers these are.)
int layer_layout(int64_t N, int32_t L, const int32_t* widths, int32_t G, int32_t K, int32_t mode, int64_t num_hub_seg,
                 int64_t num_hub_seg_t, LayerLayout& y) {
    static const char fn[] = "kagnn_gin_kan_layer_workspace_bytes";
    size_t fw = 0, dw = 0;
    y.wmax = 0;
    for (int l = 0; l < L; ++l) {
        int rc = check_kan_dims(fn, widths[l], widths[l + 1], G, K, mode);
        if (rc) return rc;
        size_t b = 0;
        rc = (l == L - 1 ? kagnn_kan_fwd_moments_workspace_bytes : kagnn_kan_fwd_workspace_bytes)(N, widths[l], widths[l + 1], G, K, mode, &b);
        if (rc) return rc;
        fw = b > fw ? b : fw;
        rc = kagnn_kan_bwd_weight_workspace_bytes(N, widths[l], widths[l + 1], G, K, mode, &b); if (rc) return rc;
        dw = b > dw ? b : dw;
        y.dw_piece_bytes[l] = al256z(b);
        y.wmax = widths[l] > y.wmax ? widths[l] : y.wmax;
    }
    y.dw_pieces_bytes = 0;
    for (int l = L - 1; l >= 0; --l) { y.dw_piece[l] = y.dw_pieces_bytes; y.dw_pieces_bytes += y.dw_piece_bytes[l]; }
    y.fwd_hub_bytes = al256z(aggregate_bf16_ws_bytes(num_hub_seg, widths[0]));
    y.fwd_scratch = y.fwd_hub_bytes;
    y.fwd_fix = y.fwd_scratch + al256z(fw);
    // (the hub-row fix-up of the aggregation fused into the first KANLinear, narrow first layers: kan_sparse_fwd_agg)
    y.fwd_total = y.fwd_fix + al256z(widths[0] <= 32 ? kan_sparse_fwd_agg_ws_bytes(num_hub_seg, widths[0], widths[1]) : 0) + 256;
    y.fwd_scratch_bytes = y.fwd_total - y.fwd_scratch;
    y.fwd_fix_bytes = y.fwd_total - y.fwd_fix;
    y.bwd_hub_bytes = al256z(aggregate_bf16_ws_bytes(num_hub_seg_t, widths[0]));
    y.dw = y.bwd_hub_bytes;
    y.dw_bytes = al256z(dw);
    const size_t g_bytes = al256z((size_t)N * y.wmax * sizeof(float));      // fp32 [N, wmax], ping-pong
    y.g[0] = y.dw + y.dw_bytes;
    y.g[1] = y.g[0] + g_bytes;
    y.bwd_total = y.g[1] + g_bytes + 256;
    layer_layout_optional(y, N, 0, 0, 0);
    return KAGNN_OK;
}

int layer_fwd_impl(const GraphSide& gr, const KanChain& c, const LayerIn& in, const GineStage* gine, void* workspace,
                   size_t workspace_bytes, void* stream, const char* fn) {
    (void)fn;
    const int64_t N = c.N;
    const int32_t L = c.L, G = c.G, K = c.K, mode = c.mode;
    const int32_t* widths = c.widths;
    float* const* acts = const_cast<float* const*>(c.acts);
    void* const* pack_fwd = const_cast<void* const*>(c.pack_fwd);
    void* const* pack_dx = const_cast<void* const*>(c.pack_dx);
    KAGNN_CHECK_ARG(N >= 0 && L >= 1 && L <= 8 && widths && c.bw && c.sw && acts && pack_fwd && pack_dx, "bad argument");
    KAGNN_CHECK_ARG((in.in_col_scale == nullptr) == (in.in_col_shift == nullptr), "in_col_scale and in_col_shift must both be given or both be null");
    KAGNN_CHECK_ARG(!in.in_col_scale || in.x_dtype == KAGNN_DTYPE_F32, "the column affine of the gathered matrix needs fp32 rows");
    KAGNN_CHECK_ARG((in.col_mean == nullptr) == (in.col_m2 == nullptr), "col_mean and col_m2 must both be given or both be null");
    LayerLayout lay;
    int rc = layer_layout(N, L, widths, G, K, mode, gr.num_hub_seg, 0, lay);
    if (rc) return rc;
    KAGNN_CHECK_ARG(workspace && workspace_bytes >= lay.fwd_total, "workspace too small (kagnn_gin_kan_layer_workspace_bytes)");
    if (N == 0) return KAGNN_OK;
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    // The aggregation fused INTO the first KANLinear (one kernel, north_star's producer -> consumer form) for narrow first
    // layers (<= 32 features: the per-rank slices of the feature-sharded layer), split precision, fp32 rows: KAGNN_FUSE_AGG=1.
    // Off by default -- bit-identical to the two launches (tests/test_gpu_models.py) but not faster: a forward tile pays the
    // gather's two dependent round trips with 2-3 waves per SIMD to hide them, the stand-alone kernel has 8 (N = 1M, E = 10M,
    // layer forward: 0.60 vs 0.56 ms at 8 input features, 1.06 vs 0.62 at 32; profiles/r03_experiments.md).
    const char* fuse_e = getenv("KAGNN_FUSE_AGG");
    const bool fuse_env = fuse_e != nullptr && atoi(fuse_e) != 0;
    const bool fuse = fuse_env && !gine && !in.in_col_scale && in.x_dtype == KAGNN_DTYPE_F32 && mode == KAGNN_PREC_SPLIT && !(L == 1 && in.col_mean) &&
                      use_sparse_fwd(widths[0], widths[1], G, K, mode) &&
                      kan_sparse_fwd_agg_ok(static_cast<const float*>(in.x), in.ldx, N, widths[0], widths[1], G, K);
    // 1. h0 = self_scale * x_i + sum_{j -> i} x_j      (GINE: sum_{j -> i} relu(x_j + e_ij))
    if (gine)
        rc = kagnn_aggregate_gine(static_cast<const float*>(in.x), in.ldx, gine->ea, gine->lde, acts[0], widths[0], gr.rowptr, gr.col, gine->perm, N,
                                  widths[0], gr.self_scale, stream);
    else if (fuse)
        rc = KAGNN_OK;                       // (produced by the first forward kernel, step 3)
    else if (in.x_dtype == KAGNN_DTYPE_BF16)
        rc = kagnn_aggregate_sum_bf16(in.x, in.ldx, acts[0], widths[0], KAGNN_DTYPE_F32, gr.rowptr, gr.col, nullptr, N, widths[0], gr.self_scale,
                                      nullptr, nullptr, nullptr, 0, gr.hub_seg, gr.num_hub_seg, gr.hub_threshold, ws, lay.fwd_hub_bytes, stream);
    else if (in.in_col_scale)
        rc = kagnn_aggregate_sum_affine(static_cast<const float*>(in.x), in.ldx, acts[0], widths[0], gr.rowptr, gr.col, N, widths[0], gr.self_scale,
                                        in.in_col_scale, in.in_col_shift, gr.hub_seg, gr.num_hub_seg, gr.hub_threshold, nullptr, 0, ws,
                                        lay.fwd_hub_bytes, stream);
    else
        rc = kagnn_aggregate_sum(static_cast<const float*>(in.x), in.ldx, acts[0], widths[0], gr.rowptr, gr.col, nullptr, N, widths[0],
                                 gr.self_scale, nullptr, nullptr, nullptr, 0, gr.hub_seg, gr.num_hub_seg, gr.hub_threshold, ws, lay.fwd_hub_bytes,
                                 stream);
    if (rc) return rc;
    // 2. weight packs: one launch for the whole chain where the shapes allow it
    const bool prepacked = gine && gine->prepacked;
    bool batched = L >= 2 && !prepacked;
    int in_[8], out_[8];
    for (int l = 0; l < L; ++l) {
        in_[l] = widths[l]; out_[l] = widths[l + 1];
        batched = batched && use_split_dx(in_[l], out_[l], G, K, mode) && use_sparse_fwd(in_[l], out_[l], G, K, mode) &&
                  kan_fused_pack_ok(in_[l], out_[l], G + K);
    }
    if (batched) {
        rc = kagnn_kan_pack_batch(L, c.bw, c.sw, c.sc, in_, out_, G, K, mode, pack_fwd, pack_dx, stream);
        if (rc) return rc;
    } else if (!prepacked) {
        for (int l = 0; l < L; ++l) {
            rc = kagnn_kan_pack(c.bw[l], c.sw[l], c.sc ? c.sc[l] : nullptr, in_[l], out_[l], G, K, mode, pack_fwd[l], pack_dx[l], stream);
            if (rc) return rc;
        }
    }
    // 3. the chain
    for (int l = 0; l < L; ++l) {
        if (l == 0 && fuse) {
            KAGNN_STAGE_AS("kagnn_kan_linear_fwd+aggregate_sum (one kernel)", stream);
            rc = kan_sparse_fwd_agg(static_cast<const float*>(in.x), in.ldx, N, gr.rowptr, gr.col, gr.hub_seg, gr.num_hub_seg, gr.hub_threshold,
                                    gr.self_scale, c.knots, in_[0], out_[0], G, K, pack_fwd[0], acts[0], in_[0], acts[1], out_[0],
                                    ws + lay.fwd_fix, lay.fwd_fix_bytes, as_stream(stream));
            if (rc) return rc;
            continue;
        }
        if (l == L - 1 && in.col_mean)       // the convolution's output: its column moments for the norm that follows
            rc = kagnn_kan_linear_fwd_moments(acts[l], in_[l], N, c.knots, in_[l], out_[l], G, K, mode, pack_fwd[l], acts[l + 1],
                                              out_[l], in.col_mean, in.col_m2, ws + lay.fwd_scratch, lay.fwd_scratch_bytes, stream);
        else
            rc = kagnn_kan_linear_fwd(acts[l], in_[l], N, c.knots, in_[l], out_[l], G, K, mode, pack_fwd[l], acts[l + 1], out_[l],
                                      ws + lay.fwd_scratch, lay.fwd_scratch_bytes, stream);
        if (rc) return rc;
    }
    return KAGNN_OK;
}

// ---- the backward's fork: weight gradients on a side stream beside the transposed aggregation (layer_bwd_impl)
// One side stream and one event pair per device, created on first use and never destroyed (timing disabled: they only order).
// The mutex is held from the fork to the join of a call: the enqueue of one call's {fork, side-stream work, join} is atomic against
// another host thread's, so the shared events are never re-recorded between a record and the wait that belongs to it (a wait that
// is already enqueued keeps the record it saw), and two calls on one device queue behind each other on the side stream.
struct BwdSide { hipStream_t stream = nullptr; hipEvent_t fork = nullptr, join = nullptr; };
constexpr int kBwdSideMaxDevices = 64;
std::mutex g_bwd_side_mu;
BwdSide g_bwd_side[kBwdSideMaxDevices];

class BwdFork {
    std::unique_lock<std::mutex> lk_;
    BwdSide* s_ = nullptr;
    hipStream_t caller_ = nullptr;
    bool forked_ = false, recorded_ = false;
public:
    BwdFork() = default;
    BwdFork(const BwdFork&) = delete;
    BwdFork& operator=(const BwdFork&) = delete;
    // the device's side stream and events (created here the first time); takes the lock
    int prepare(hipStream_t caller) {
        int dev = 0;
        KAGNN_HIP(hipGetDevice(&dev));
        if (dev < 0 || dev >= kBwdSideMaxDevices) return fail(KAGNN_ERR_UNSUPPORTED, "%s: device index out of range", "layer_bwd");
        lk_ = std::unique_lock<std::mutex>(g_bwd_side_mu);
        BwdSide& s = g_bwd_side[dev];
        // (non-blocking: torch's default stream is the legacy null stream, which every blocking stream synchronises with)
        if (!s.stream) KAGNN_HIP(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
        if (!s.fork) KAGNN_HIP(hipEventCreateWithFlags(&s.fork, hipEventDisableTiming));
        if (!s.join) KAGNN_HIP(hipEventCreateWithFlags(&s.join, hipEventDisableTiming));
        s_ = &s; caller_ = caller;
        return KAGNN_OK;
    }
    // everything launched on the caller's stream so far happens before what the side stream is given from here on
    int fork() {
        KAGNN_HIP(hipEventRecord(s_->fork, caller_));
        KAGNN_HIP(hipStreamWaitEvent(s_->stream, s_->fork, 0));
        forked_ = true;
        return KAGNN_OK;
    }
    hipStream_t side() const { return s_->stream; }
    // everything given to the side stream (all of it: nothing may follow), as the event the caller's stream has to wait for
    int side_done(hipEvent_t* ev) {
        KAGNN_HIP(hipEventRecord(s_->join, s_->stream));
        recorded_ = true;
        *ev = s_->join;
        return KAGNN_OK;
    }
    // the caller's stream has been made to wait for that event (the aggregation's launcher does it between its two parts)
    void joined() { forked_ = false; }
    // the join on every other path out of the call after the fork, error returns included
    int join() {
        if (!forked_) return KAGNN_OK;
        forked_ = false;
        if (!recorded_) KAGNN_HIP(hipEventRecord(s_->join, s_->stream));
        KAGNN_HIP(hipStreamWaitEvent(caller_, s_->join, 0));
        return KAGNN_OK;
    }
    ~BwdFork() { (void)join(); }
};

// the weight gradient whose footprint the co-run launch of the aggregation was sized for (host.h: kAggCorunLds): the cubic
// kan_split_dw_kernel of one 64 x 64 role, one workgroup per CU.  Other shapes run other kernels; they keep their place.
// kAggCorunHeadPct: the share of the aggregation's row groups that runs beside ONE such weight gradient.  At the headline shape
// (N = 1M, E = 10M, 64 features) the held-back row kernel needs 0.41 ms alone and two weight gradients 0.60 ms: with both deferred
// the head is the whole aggregation, launched once, and no tail follows the join (measured best of 35 / 40 / 45 / 50,
// profiles/bwd_corun_priority.md); with one deferred (the node models) half of the rows run beside it.  A graph with other degrees
// moves the balance, not the result: the head that outlasts the weight gradients runs on with four waves per SIMD, the tail of
// a head that ends early waits for them.
constexpr int kAggCorunHeadPct = 50;
bool dw_corun_ok(int in, int out, int G, int K, int mode) {
    return use_split_dw(in, out, G, K, mode) && !g_half_products && K == 3 && G + K <= 8 && in > 32 && in <= 64 && out <= 64;
}

int layer_bwd_impl(const GraphSide& gr, const KanChain& c, const LayerGrads& io, const BnStage* bn, const float* bn_sums_in,
                   const StatsOut* so, const GineStage* gine, const DwPiece* piece, void* workspace, size_t workspace_bytes, void* stream,
                   const char* fn) {
    const int64_t N = c.N;
    const int32_t L = c.L, G = c.G, K = c.K, mode = c.mode;
    const int32_t* widths = c.widths;
    const float* const* acts = c.acts;
    void* const gx = io.gx;
    KAGNN_CHECK_ARG(N >= 0 && L >= 1 && L <= 8 && widths && c.sw && acts && c.pack_dx && io.g_sw, "bad argument");
    KAGNN_CHECK_ARG(!io.gx_addend || (gx && io.gx_dtype == KAGNN_DTYPE_F32 && !io.bf16_gather && io.ld_addend >= widths[0]),
                    "gx_addend needs an fp32 gx and fp32 gather operands");
    LayerLayout lay;
    int rc = layer_layout(N, L, widths, G, K, mode, 0, gr.num_hub_seg, lay);
    if (rc) return rc;
    layer_layout_optional(lay, N, bn ? widths[L] : 0, so ? widths[0] : 0, gr.num_hub_seg);
    KAGNN_CHECK_ARG(!so || (so->y && so->mean && so->rstd && so->sums && so->ldy >= widths[0] && gx && io.gx_dtype == KAGNN_DTYPE_F32 && !io.bf16_gather),
                    "the previous norm's statistics need its input, mean, rstd and an fp32 gx");
    KAGNN_CHECK_ARG(!bn_sums_in || bn, "bn_sums belongs to the BatchNorm stage");
    if (!(workspace && workspace_bytes >= lay.bwd_total_all))
        return fail(KAGNN_ERR_ARG, bn ? "%s: workspace too small (kagnn_gin_kan_layer_workspace_bytes + kagnn_gin_kan_layer_bwd_bn_workspace_bytes)"
                                      : "%s: workspace too small (kagnn_gin_kan_layer_workspace_bytes)", fn);
    if (N == 0) return KAGNN_OK;
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    const int wmax = lay.wmax;
    unsigned char* gbuf[2] = {ws + lay.g[0], ws + lay.g[1]};
    // layer l's weight gradient: its row slabs go to the shared area and their reduction is launched -- or, inside a stack call that
    // reduces the slabs of all its layers in one launch at the end, to the layer's place in the call's arena, and it is recorded
    auto dw_on = [&](void* st, int l, const float* g, long ldg) {
        unsigned char* area = piece ? piece->base + lay.dw_piece[l] : ws + lay.dw;
        const size_t bytes = piece ? lay.dw_piece_bytes[l] : lay.dw_bytes;
        return kan_linear_bwd_weight(acts[l], widths[l], nullptr, g, ldg, N, c.knots, widths[l], widths[l + 1], G, K, mode, c.sw[l],
                                     c.sc ? c.sc[l] : nullptr, io.g_bw ? io.g_bw[l] : nullptr, io.g_sw[l], io.g_sc ? io.g_sc[l] : nullptr,
                                     area, bytes, st, piece ? piece->defer : nullptr);
    };
    // The weight gradients feed nothing inside this call, and they leave the memory system mostly idle while the transposed
    // aggregation at the end of the call is limited by it: those whose operands are still alive after the dX chain -- layer 0's (its
    // gradient rows sit in the ping-pong matrix the last dX does not write) and, without a BatchNorm stage, the last layer's (it
    // reads the caller's gy) -- are launched after the chain on a side stream, beside the aggregation (its co-run launch, host.h);
    // the layers between keep their place, their rows are overwritten by the ping-pong.  Same kernels, operands and slab order:
    // same bits.  KAGNN_BWD_OVERLAP=0 (read per call) keeps the serial order; so do a capturing stream (a captured step keeps the
    // graph it has, without parallel branches) and every shape the co-run launch was not measured at (profiles/bwd_overlap.md).
    BwdFork side;
    struct { int l; const float* g; long ldg; } deferred[2];
    int n_deferred = 0;
    bool overlap = false;
    if (gx && !gine && !piece && !so && !io.bf16_gather && io.gx_dtype == KAGNN_DTYPE_F32 && dw_corun_ok(widths[0], widths[1], G, K, mode)) {
        const char* env = getenv("KAGNN_BWD_OVERLAP");
        const AggArgs probe{reinterpret_cast<const float*>(gbuf[0]), widths[0], static_cast<float*>(gx), io.ldgx, gr.rowptr, gr.col, nullptr, N,
                            widths[0], gr.self_scale, nullptr, nullptr, nullptr, 0, 0x7fffffff, io.gx_addend, io.ld_addend};
        // (a call the aggregation's entry point would refuse -- short leading dimensions, gx inside the workspace -- stays on the
        // serial path and is refused there, with that path's message)
        const bool gx_in_ws = static_cast<unsigned char*>(gx) + (size_t)N * io.ldgx * sizeof(float) > ws &&
                              static_cast<unsigned char*>(gx) < ws + workspace_bytes;
        overlap = (env == nullptr || atoi(env) != 0) && io.ldgx >= widths[0] && (!io.gx_addend || io.ld_addend >= widths[0]) && !gx_in_ws &&
                  aggregate_corun_ok(probe);
        if (overlap) {
            hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
            if (hipStreamIsCapturing(as_stream(stream), &cap) != hipSuccess) { (void)hipGetLastError(); overlap = false; }
            else overlap = cap == hipStreamCaptureStatusNone;
        }
        if (overlap) { rc = side.prepare(as_stream(stream)); if (rc) return rc; }
    }
    // layer l's weight gradient: launched in its place, or noted for the side stream
    auto dw = [&](int l, const float* g, long ldg) {
        const bool alive = l == 0 || (l == L - 1 && !bn);        // (l == L - 1 with a BatchNorm stage: its rows are in gbuf[1], see below)
        if (overlap && alive && dw_corun_ok(widths[l], widths[l + 1], G, K, mode)) {
            deferred[n_deferred++] = {l, g, ldg};
            return (int)KAGNN_OK;
        }
        return dw_on(stream, l, g, ldg);
    };
    const float* g = io.gy;
    long ldg = io.ldgy;
    int cur = 0;
    bool gh0_bf16 = false;
    // the normalisation's backward: statistics pass (column sums -> g_weight, g_bias, the per-column table), then EITHER the
    // last layer's input-gradient kernel applies it to the rows it loads and leaves them for the weight gradient (no pass
    // of its own), OR -- shapes that kernel does not cover -- the stand-alone pass writes them
    bool bn_in_dx = false;
    BnBack bnb{};
    if (bn) {
        const int out = widths[L], ldt = (out + 63) & ~63;
        KAGNN_CHECK_ARG(bn->y && bn->mean && bn->rstd && bn->ldy >= out && N >= 2, "bad BatchNorm stage");
        unsigned char* bws = ws + lay.bn;
        float* tab = reinterpret_cast<float*>(ws + lay.bn_tab);
        bnb = BnBack{bn->y, (long)bn->ldy, tab, ldt, reinterpret_cast<float*>(gbuf[1]), (long)out};
        const int in = widths[L - 1];
        bn_in_dx = mode == KAGNN_PREC_SPLIT && use_split_dx(in, out, G, K, mode) && out <= wmax && !(L == 1 && (gx == nullptr || io.bf16_gather)) &&
                   fits32(N, ldg) && kan_split_dx_bn_ok(ldg, in, out, G, K, bnb, g);
        if (bn_in_dx && bn_sums_in) {        // the column sums came with the gradient (the aggregation that produced g left them)
            KAGNN_STAGE_AS("kagnn_batchnorm_bwd statistics given (in ..._layer_bwd_bn)", stream);
            rc = bn_bwd_stats_given(bn_sums_in, N, out, bn->weight, bn->mean, bn->rstd, bn->g_weight, bn->g_bias, tab, ldt, as_stream(stream));
            if (rc) return rc;
        } else if (bn_in_dx) {
            KAGNN_STAGE_AS("kagnn_batchnorm_bwd statistics (in ..._layer_bwd_bn)", stream);
            rc = bn_bwd_stats(bn->y, bn->ldy, g, ldg, N, out, bn->weight, bn->mean, bn->rstd, bn->g_weight, bn->g_bias, tab, ldt, bws,
                              lay.bn_ws_bytes, as_stream(stream));
            if (rc) return rc;
        } else {
            // (out may exceed the chain's widest INPUT, which sizes the ping-pong matrices: then the stage's own matrix is needed)
            if (out > wmax) return fail(KAGNN_ERR_UNSUPPORTED, "%s: a BatchNorm stage wider than every layer input is not covered", fn);
            KAGNN_STAGE_AS("kagnn_batchnorm_bwd", stream);
            rc = bn_bwd(bn->y, bn->ldy, g, ldg, N, out, bn->weight, bn->mean, bn->rstd, 1, 0.0f, 0ULL, reinterpret_cast<float*>(gbuf[1]), out,
                        bn->g_weight, bn->g_bias, bws, lay.bn_ws_bytes, as_stream(stream));
            if (rc) return rc;
            g = reinterpret_cast<const float*>(gbuf[1]); ldg = out;
        }
    }
    for (int l = L - 1; l >= 0; --l) {
        const int in = widths[l], out = widths[l + 1];
        const bool fused_bn = bn_in_dx && l == L - 1;
        if (fused_bn) {            // input gradient FIRST: it produces the normalised-backward rows the weight gradient reads
            {
                KAGNN_STAGE_AS("kagnn_kan_linear_bwd_input", stream);       // (+ the norm's element-wise backward on the rows it loads)
                rc = kan_split_dx_bn(acts[l], in, g, ldg, N, c.knots, in, out, G, K, c.pack_dx[l], reinterpret_cast<float*>(gbuf[0]), in, bnb,
                                     as_stream(stream));
            }
            if (rc) return rc;
            rc = dw(l, bnb.gy_out, bnb.ldo);
            if (rc) return rc;
            if (l == 0 && gx == nullptr) break;
            g = reinterpret_cast<const float*>(gbuf[0]); ldg = in; cur = 1;
            continue;
        }
        rc = dw(l, g, ldg);
        if (rc) return rc;
        if (l == 0 && gx == nullptr) break;
        // the gathered matrix of the transposed aggregation leaves the dX kernel as bf16 when the mode asks for it
        const bool b16 = l == 0 && io.bf16_gather && mode == KAGNN_PREC_SPLIT && K == 3 && G + K <= 8 && out <= 128 && in % 8 == 0 &&
                         in <= 512 /* the bf16 aggregation's row limit (aggregate_bf16_ok): wider first layers keep fp32 rows */ &&
                         use_split_dx(in, out, G, K, mode);
        // (a stand-alone BatchNorm pass left its rows in gbuf[1]: the first input gradient then writes gbuf[0])
        rc = kagnn_kan_linear_bwd_input(acts[l], in, g, ldg, N, c.knots, in, out, G, K, mode, c.pack_dx[l], gbuf[cur], in,
                                        b16 ? KAGNN_DTYPE_BF16 : KAGNN_DTYPE_F32, stream);
        if (rc) return rc;
        g = reinterpret_cast<const float*>(gbuf[cur]); ldg = in; cur ^= 1;
        gh0_bf16 = b16;
    }
    if (gx == nullptr) return KAGNN_OK;
    const int f0 = widths[0];
    if (overlap) {
        // fork: the side stream takes the noted weight gradients in layer order L-1 .. 0 (one slab area: they stay serial there),
        // this stream the aggregation.  The call never returns with side-stream work this stream has not been made to wait for
        // (on an error return the destructor issues the wait), so nothing later touches the workspace while it is outstanding
        rc = side.fork();
        if (rc) return rc;
        for (int k = 0; k < n_deferred; ++k) {
            rc = dw_on(side.side(), deferred[k].l, deferred[k].g, deferred[k].ldg);
            if (rc) return rc;
        }
        const AggArgs a{g, ldg, static_cast<float*>(gx), io.ldgx, gr.rowptr, gr.col, nullptr, N, f0, gr.self_scale, nullptr, nullptr, nullptr,
                        0, gr.hub_threshold > 0 ? gr.hub_threshold : 0x7fffffff, io.gx_addend, io.ld_addend};
        // the join sits INSIDE the aggregation: kAggCorunHeadPct of the row groups per deferred weight gradient run beside them, held
        // to what a weight-gradient wave leaves free; then this stream waits for the side stream and the rest of the rows, if any,
        // have the machine to themselves (host.h: AggCorun)
        AggCorun corun{std::min(100, kAggCorunHeadPct * n_deferred), nullptr};
        rc = side.side_done(&corun.side_done);
        if (rc) return rc;
        KAGNN_STAGE_AS("kagnn_aggregate_sum", stream);
        rc = aggregate_sum(a, gr.hub_seg, gr.num_hub_seg, reinterpret_cast<float*>(ws), lay.bwd_hub_bytes, as_stream(stream), &corun);
        if (rc) return rc;
        side.joined();
        return KAGNN_OK;
    }
    if (gine)        // GINE: gradient of the relu(x_j + e_ij) messages on the transposed structure -> gx and the edge-attribute gradient
        return gine_bwd(gine->x, gine->ldx, gine->ea, gine->lde, g, ldg, static_cast<float*>(gx), io.ldgx, gine->g_ea, gine->ldge,
                        gr.rowptr, gr.col, gine->perm, N, f0, gr.self_scale, as_stream(stream), gine->accumulate_g_ea);
    if (gh0_bf16 || io.gx_dtype == KAGNN_DTYPE_BF16) {
        const void* src = g;
        if (!gh0_bf16) {                          // fp32 d loss / d h0 but a bf16 result wanted: convert, then the bf16 kernel
            rc = kagnn_rows_to_bf16(g, ldg, gbuf[cur], f0, N, f0, stream);
            if (rc) return rc;
            src = gbuf[cur];
        }
        return kagnn_aggregate_sum_bf16(src, f0, gx, io.ldgx, io.gx_dtype, gr.rowptr, gr.col, nullptr, N, f0, gr.self_scale, nullptr, nullptr,
                                        nullptr, 0, gr.hub_seg, gr.num_hub_seg, gr.hub_threshold, ws, lay.bwd_hub_bytes, stream);
    }
    if (so) {       // the transposed aggregation also leaves the column statistics of gx for the previous norm's backward
        AggArgs a{g, ldg, static_cast<float*>(gx), io.ldgx, gr.rowptr, gr.col, nullptr, N, f0, gr.self_scale, nullptr, nullptr, nullptr,
                  0, gr.hub_threshold > 0 ? gr.hub_threshold : 0x7fffffff, io.gx_addend, io.ld_addend};
        float* partial = reinterpret_cast<float*>(ws + lay.stats);
        a.st_y = so->y; a.st_ldy = so->ldy; a.st_mean = so->mean; a.st_rstd = so->rstd; a.st_partial = partial;
        KAGNN_CHECK_ARG(ldg >= f0 && io.ldgx >= f0 && (!io.gx_addend || io.ld_addend >= f0), "leading dimension smaller than num_feat");
        if (!aggregate_stats_ok(a)) return fail(KAGNN_ERR_UNSUPPORTED, "%s: the previous norm's statistics need 17..256 input features in 16-byte aligned fp32 rows", fn);
        {
            KAGNN_STAGE_AS("kagnn_aggregate_sum", stream);
            rc = aggregate_sum(a, gr.hub_seg, gr.num_hub_seg, reinterpret_cast<float*>(ws), lay.bwd_hub_bytes, as_stream(stream));
            if (rc) return rc;
        }
        KAGNN_STAGE_AS("kagnn_batchnorm_bwd statistics fold", stream);
        const bool hubs = gr.num_hub_seg > 0 && gr.hub_seg != nullptr && gr.hub_threshold > 0;
        return bn_sums_from_partials(partial, aggregate_stats_rows(N, f0, hubs ? gr.num_hub_seg : 0), f0, so->sums, as_stream(stream));
    }
    return kagnn_aggregate_sum_add(g, ldg, static_cast<float*>(gx), io.ldgx, gr.rowptr, gr.col, nullptr, N, f0, gr.self_scale, nullptr,
                                   nullptr, nullptr, 0, gr.hub_seg, gr.num_hub_seg, gr.hub_threshold, io.gx_addend, io.ld_addend, ws,
                                   lay.bwd_hub_bytes, stream);
}

// ---------------------------------------------------------------- the whole GINE stack per call (kagnn_gine_kan_stack_*, below)
// Byte offsets and sizes inside the workspace of one stack call (filled by stack_layout):
//   forward:   one convolution's scratch | BatchNorm workspace | column moments [2][hidden]
//   backward:  one convolution's scratch with its BatchNorm stage | two ping-pong gradient matrices [N, hidden] | dW arena
// The arena holds one slab area per layer of the stack, so that all nconv * L slab reductions run in ONE launch at the end of the call
// (DwDefer, common.h); it is empty past kDwDeferMax layers, and every weight gradient then launches its own reduction.
struct StackLayout {
    LayerLayout layer;                   // one convolution of the stack: no hub segments, the BatchNorm stage behind its backward
    size_t fwd_layer_bytes, bn_ws, bn_ws_bytes, moments, fwd_total;
    size_t bwd_layer_bytes, pp[2], arena, arena_conv_bytes, arena_bytes, bwd_total;      // (arena_conv_bytes: one convolution's DwPiece)
};

int stack_layout(int64_t N, int32_t nconv, int32_t L, const int32_t* widths, int32_t G, int32_t K, int32_t mode, StackLayout& s) {
    int rc = layer_layout(N, L, widths, G, K, mode, 0, 0, s.layer);
    if (rc) return rc;
    layer_layout_optional(s.layer, N, widths[L], 0, 0);
    s.fwd_layer_bytes = al256z(s.layer.fwd_total);
    s.bn_ws = s.fwd_layer_bytes;
    s.bn_ws_bytes = bn_ws_bytes(N, widths[L]);
    s.moments = s.bn_ws + al256z(s.bn_ws_bytes);
    s.fwd_total = s.moments + al256z(2 * (size_t)widths[L] * sizeof(float)) + 256;
    s.bwd_layer_bytes = al256z(s.layer.bwd_total_all);
    const size_t g_bytes = al256z((size_t)N * widths[0] * sizeof(float));
    s.pp[0] = s.bwd_layer_bytes;
    s.pp[1] = s.pp[0] + g_bytes;
    s.arena = s.pp[1] + g_bytes;
    s.arena_conv_bytes = nconv * L <= kDwDeferMax ? s.layer.dw_pieces_bytes : 0;
    s.arena_bytes = s.arena_conv_bytes * (size_t)nconv;
    s.bwd_total = s.arena + s.arena_bytes + 256;
    return KAGNN_OK;
}

// kagnn_gine_kan_stack_fwd; prepacked: the caller has made the packs of all nconv * L layers already (kagnn_kagin_model_fwd, in the
// one launch that also packs its read-out), so the stack's own batched pack launch is skipped where it would have run
int stack_fwd_impl(const float* x, int64_t ldx, const float* edge_attr, int64_t lde, int64_t N, const int32_t* rowptr,
                   const int32_t* col, const int32_t* perm, const float* self_scale, int32_t nconv,
                   int32_t L, const int32_t* widths, const float* const* bw, const float* const* sw,
                   const float* const* sc, const float* knots, int32_t G, int32_t K, int32_t mode,
                   float* const* acts, void* const* pack_fwd, void* const* pack_dx,
                   const float* const* bn_weight, const float* const* bn_bias, float* const* running_mean,
                   float* const* running_var, const float* momentum, const float* eps,
                   float* const* h, float* const* save_mean, float* const* save_rstd,
                   void* workspace, size_t workspace_bytes, void* stream, bool prepacked) {
    static const char fn[] = "kagnn_gine_kan_stack_fwd";
    ModeScope mode_scope_(mode);
    KAGNN_CHECK_ARG_AS(fn, nconv >= 1 && L >= 1 && L <= 8 && widths && self_scale && bw && sw && acts && pack_fwd && pack_dx && bn_weight && bn_bias &&
                       momentum && eps && h && save_mean && save_rstd, "null array");
    KAGNN_CHECK_ARG_AS(fn, widths[0] == widths[L] && N >= 2, "hidden -> hidden chains, at least two rows (batch statistics)");
    StackLayout lay;
    int rc = stack_layout(N, nconv, L, widths, G, K, mode, lay);
    if (rc) return rc;
    KAGNN_CHECK_ARG_AS(fn, workspace && workspace_bytes >= lay.fwd_total, "workspace too small (kagnn_gine_kan_stack_workspace_bytes)");
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    float* mom = reinterpret_cast<float*>(ws + lay.moments);
    const int H = widths[L];
    // one pack launch for the whole stack where the shapes allow it (<= 16 layers on the sparse-forward / split path)
    int in_[16], out_[16];
    bool batch = nconv * L <= 16;
    for (int k = 0; k < nconv * L && batch; ++k) {
        in_[k] = widths[k % L]; out_[k] = widths[k % L + 1];
        batch = use_split_dx(in_[k], out_[k], G, K, mode) && use_sparse_fwd(in_[k], out_[k], G, K, mode) && kan_fused_pack_ok(in_[k], out_[k], G + K);
    }
    if (batch && !prepacked) { rc = kagnn_kan_pack_batch(nconv * L, bw, sw, sc, in_, out_, G, K, mode, pack_fwd, pack_dx, stream); if (rc) return rc; }
    const float* in = x;
    int64_t ldin = ldx;
    for (int i = 0; i < nconv; ++i) {
        GineStage gs{in, ldin, edge_attr, lde, perm, nullptr, 0};
        gs.prepacked = batch ? 1 : 0;
        const GraphSide gr{.rowptr = rowptr, .col = col, .self_scale = self_scale[i]};
        const KanChain c{.N = N, .L = L, .widths = widths, .bw = bw + i * L, .sw = sw + i * L, .sc = sc ? sc + i * L : nullptr,
                         .acts = acts + i * (L + 1), .pack_fwd = pack_fwd + i * L, .pack_dx = pack_dx + i * L, .knots = knots, .G = G, .K = K,
                         .mode = mode};
        const LayerIn li{.x = in, .x_dtype = KAGNN_DTYPE_F32, .ldx = ldin, .col_mean = mom,
                         .col_m2 = mom + H};
        rc = layer_fwd_impl(gr, c, li, &gs, ws, lay.fwd_layer_bytes, stream, fn);
        if (rc) return rc;
        rc = kagnn_batchnorm_fwd(acts[i * (L + 1) + L], H, N, H, bn_weight[i], bn_bias[i], running_mean ? running_mean[i] : nullptr,
                                 running_var ? running_var[i] : nullptr, momentum[i], eps[i], 1, mom, mom + H, 0.0f, 0ULL, h[i], H,
                                 save_mean[i], save_rstd[i], ws + lay.bn_ws, lay.bn_ws_bytes, stream);
        if (rc) return rc;
        in = h[i]; ldin = H;
    }
    return KAGNN_OK;
}
}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int kagnn_gin_kan_layer_workspace_bytes(int64_t N, int32_t L, const int32_t* widths, int32_t G, int32_t K, int32_t mode,
                                        int64_t num_hub_seg, int64_t num_hub_seg_t, size_t* fwd_bytes, size_t* bwd_bytes) {
    ModeScope mode_scope_(mode);
    KAGNN_CHECK_ARG(N >= 0 && L >= 1 && L <= 8 && widths && fwd_bytes && bwd_bytes, "bad argument");
    LayerLayout lay;
    int rc = layer_layout(N, L, widths, G, K, mode, num_hub_seg, num_hub_seg_t, lay);
    if (rc) return rc;
    *fwd_bytes = lay.fwd_total;
    *bwd_bytes = lay.bwd_total;
    return KAGNN_OK;
}

int kagnn_gin_kan_layer_fwd(const void* x, int32_t x_dtype, int64_t ldx, int64_t N, const int32_t* rowptr, const int32_t* col,
                            const int32_t* hub_seg, int64_t num_hub_seg, int32_t hub_threshold, float self_scale,
                            int32_t L, const int32_t* widths, const float* const* bw, const float* const* sw,
                            const float* const* sc, const float* knots, int32_t G, int32_t K, int32_t mode,
                            float* const* acts, void* const* pack_fwd, void* const* pack_dx, float* col_mean,
                            float* col_m2, void* workspace, size_t workspace_bytes, void* stream) {
    ModeScope mode_scope_(mode);
    const GraphSide gr{.rowptr = rowptr, .col = col, .hub_seg = hub_seg, .num_hub_seg = num_hub_seg, .hub_threshold = hub_threshold,
                       .self_scale = self_scale};
    const KanChain c{.N = N, .L = L, .widths = widths, .bw = bw, .sw = sw, .sc = sc, .acts = acts, .pack_fwd = pack_fwd, .pack_dx = pack_dx,
                     .knots = knots, .G = G, .K = K, .mode = mode};
    const LayerIn in{.x = x, .x_dtype = x_dtype, .ldx = ldx, .col_mean = col_mean, .col_m2 = col_m2};
    return layer_fwd_impl(gr, c, in, nullptr, workspace, workspace_bytes, stream, __func__);
}

// The same on an input that exists only as  in_col_scale * x + in_col_shift  (the previous layer's BatchNorm1d, folded into this
// layer's aggregation: kagnn_aggregate_sum_affine); acts[0] receives the aggregate of the NORMALISED rows, as before.
int kagnn_gin_kan_layer_fwd_affine(const float* x, int64_t ldx, int64_t N, const int32_t* rowptr, const int32_t* col,
                                   const int32_t* hub_seg, int64_t num_hub_seg, int32_t hub_threshold, float self_scale,
                                   const float* in_col_scale, const float* in_col_shift,
                                   int32_t L, const int32_t* widths, const float* const* bw, const float* const* sw,
                                   const float* const* sc, const float* knots, int32_t G, int32_t K, int32_t mode,
                                   float* const* acts, void* const* pack_fwd, void* const* pack_dx, float* col_mean,
                                   float* col_m2, void* workspace, size_t workspace_bytes, void* stream) {
    ModeScope mode_scope_(mode);
    const GraphSide gr{.rowptr = rowptr, .col = col, .hub_seg = hub_seg, .num_hub_seg = num_hub_seg, .hub_threshold = hub_threshold,
                       .self_scale = self_scale};
    const KanChain c{.N = N, .L = L, .widths = widths, .bw = bw, .sw = sw, .sc = sc, .acts = acts, .pack_fwd = pack_fwd, .pack_dx = pack_dx,
                     .knots = knots, .G = G, .K = K, .mode = mode};
    const LayerIn in{.x = x, .x_dtype = KAGNN_DTYPE_F32, .ldx = ldx, .in_col_scale = in_col_scale, .in_col_shift = in_col_shift,
                     .col_mean = col_mean, .col_m2 = col_m2};
    return layer_fwd_impl(gr, c, in, nullptr, workspace, workspace_bytes, stream, __func__);
}

// gx_addend (optional, fp32 [N, widths[0]]): gx = <the layer's input gradient> + gx_addend, added inside the transposed
// aggregation's epilogue -- the skip-concat models hand the read-out's gradient of the same activation in here instead of
// letting the tape sum the two in a pass of its own (reference node_classification_clean/models.py:196-202)
int kagnn_gin_kan_layer_bwd_add(const float* gy, int64_t ldgy, int64_t N, const int32_t* rowptr_t, const int32_t* col_t,
                                const int32_t* hub_seg_t, int64_t num_hub_seg_t, int32_t hub_threshold, float self_scale,
                                int32_t L, const int32_t* widths, const float* const* sw, const float* const* sc,
                                const float* knots, int32_t G, int32_t K, int32_t mode, const float* const* acts,
                                const void* const* pack_dx, void* gx, int32_t gx_dtype, int64_t ldgx, int32_t bf16_gather,
                                const float* gx_addend, int64_t ld_addend,
                                float* const* g_bw, float* const* g_sw, float* const* g_sc, void* workspace,
                                size_t workspace_bytes, void* stream) {
    ModeScope mode_scope_(mode);
    const GraphSide gr{.rowptr = rowptr_t, .col = col_t, .hub_seg = hub_seg_t, .num_hub_seg = num_hub_seg_t, .hub_threshold = hub_threshold,
                       .self_scale = self_scale};
    const KanChain c{.N = N, .L = L, .widths = widths, .sw = sw, .sc = sc, .acts = acts, .pack_dx = pack_dx,
                     .knots = knots, .G = G, .K = K, .mode = mode};
    const LayerGrads io{.gy = gy, .ldgy = ldgy, .gx = gx, .gx_dtype = gx_dtype, .ldgx = ldgx, .bf16_gather = bf16_gather, .gx_addend = gx_addend,
                        .ld_addend = ld_addend, .g_bw = g_bw, .g_sw = g_sw, .g_sc = g_sc};
    return layer_bwd_impl(gr, c, io, nullptr, nullptr, nullptr, nullptr, nullptr, workspace, workspace_bytes, stream, __func__);
}

// The backward of  BatchNorm1d(KAN(aggregate(x)))  in training mode -- the convolution plus the norm that follows it in
// every node model (reference node_classification_clean/models.py:198-200) -- given g = d loss / d (norm output):
// the norm's statistics pass (-> g_bn_weight, g_bn_bias), then the chain's backward with the norm's element-wise backward
// applied INSIDE the last layer's input-gradient kernel (no normalisation-backward pass over [N, out]), then the transposed
// aggregation (+ gx_addend).  y = the norm's input (the chain's output), bn_mean / bn_rstd = the statistics its forward saved.
// Workspace: kagnn_gin_kan_layer_workspace_bytes' backward size + kagnn_gin_kan_layer_bwd_bn_workspace_bytes.
int kagnn_gin_kan_layer_bwd_bn_workspace_bytes(int64_t N, int32_t out, size_t* bytes) {
    KAGNN_CHECK_ARG(N >= 0 && out >= 1 && bytes, "bad argument");
    LayerLayout lay{};
    layer_layout_optional(lay, N, out, 0, 0);
    *bytes = lay.bn_bytes;
    return KAGNN_OK;
}

int kagnn_gin_kan_layer_bwd_bn(const float* g, int64_t ldg, const float* y, int64_t ldy, const float* bn_weight,
                               const float* bn_mean, const float* bn_rstd, float* g_bn_weight, float* g_bn_bias,
                               int64_t N, const int32_t* rowptr_t, const int32_t* col_t,
                               const int32_t* hub_seg_t, int64_t num_hub_seg_t, int32_t hub_threshold, float self_scale,
                               int32_t L, const int32_t* widths, const float* const* sw, const float* const* sc,
                               const float* knots, int32_t G, int32_t K, int32_t mode, const float* const* acts,
                               const void* const* pack_dx, void* gx, int32_t gx_dtype, int64_t ldgx, int32_t bf16_gather,
                               const float* gx_addend, int64_t ld_addend,
                               float* const* g_bw, float* const* g_sw, float* const* g_sc, void* workspace,
                               size_t workspace_bytes, void* stream) {
    ModeScope mode_scope_(mode);
    const BnStage bn{y, ldy, bn_weight, bn_mean, bn_rstd, g_bn_weight, g_bn_bias};
    const GraphSide gr{.rowptr = rowptr_t, .col = col_t, .hub_seg = hub_seg_t, .num_hub_seg = num_hub_seg_t, .hub_threshold = hub_threshold,
                       .self_scale = self_scale};
    const KanChain c{.N = N, .L = L, .widths = widths, .sw = sw, .sc = sc, .acts = acts, .pack_dx = pack_dx,
                     .knots = knots, .G = G, .K = K, .mode = mode};
    const LayerGrads io{.gy = g, .ldgy = ldg, .gx = gx, .gx_dtype = gx_dtype, .ldgx = ldgx, .bf16_gather = bf16_gather, .gx_addend = gx_addend,
                        .ld_addend = ld_addend, .g_bw = g_bw, .g_sw = g_sw, .g_sc = g_sc};
    return layer_bwd_impl(gr, c, io, &bn, nullptr, nullptr, nullptr, nullptr, workspace, workspace_bytes, stream, __func__);
}

// kagnn_gin_kan_layer_bwd_bn with the norms' backward STATISTICS travelling with the gradients (round 4): in the node models the
// gradient g arriving at layer l's norm is produced by layer l+1's transposed aggregation (+ the skip gradient it adds), so
//   * prev_y / prev_mean / prev_rstd / prev_sums (all or none): this call's transposed aggregation ALSO leaves
//     prev_sums[0][in] = sum_n gx, prev_sums[1][in] = sum_n gx * xhat_prev  (xhat_prev = (prev_y - prev_mean) * prev_rstd; prev_y is
//     the previous norm's input = this convolution's input before the folded affine) -- from partial sums in the row kernel's
//     epilogue, folded in a fixed order;
//   * bn_sums (or NULL): [2][out] sums for THIS norm made that way by the next layer's call -- the statistics pass over g and y is
//     skipped (only when the norm's element-wise backward runs inside the input-gradient kernel; otherwise ignored).
// Extra workspace behind kagnn_gin_kan_layer_bwd_bn's: kagnn_gin_kan_layer_bwd_bn_sums_workspace_bytes (0 without prev_sums).
int kagnn_gin_kan_layer_bwd_bn_sums_workspace_bytes(int64_t N, int32_t in_features, int64_t num_hub_seg_t, size_t* bytes) {
    KAGNN_CHECK_ARG(N >= 0 && in_features >= 1 && num_hub_seg_t >= 0 && bytes, "bad argument");
    LayerLayout lay{};
    layer_layout_optional(lay, N, 0, in_features, num_hub_seg_t);
    *bytes = lay.stats_bytes;
    return KAGNN_OK;
}

int kagnn_gin_kan_layer_bwd_bn_sums(const float* g, int64_t ldg, const float* y, int64_t ldy, const float* bn_weight,
                                    const float* bn_mean, const float* bn_rstd, float* g_bn_weight, float* g_bn_bias,
                                    const float* bn_sums,
                                    const float* prev_y, int64_t ld_prev_y, const float* prev_mean, const float* prev_rstd,
                                    float* prev_sums,
                                    int64_t N, const int32_t* rowptr_t, const int32_t* col_t,
                                    const int32_t* hub_seg_t, int64_t num_hub_seg_t, int32_t hub_threshold, float self_scale,
                                    int32_t L, const int32_t* widths, const float* const* sw, const float* const* sc,
                                    const float* knots, int32_t G, int32_t K, int32_t mode, const float* const* acts,
                                    const void* const* pack_dx, void* gx, int32_t gx_dtype, int64_t ldgx, int32_t bf16_gather,
                                    const float* gx_addend, int64_t ld_addend,
                                    float* const* g_bw, float* const* g_sw, float* const* g_sc, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    ModeScope mode_scope_(mode);
    const BnStage bn{y, ldy, bn_weight, bn_mean, bn_rstd, g_bn_weight, g_bn_bias};
    const StatsOut so{prev_y, ld_prev_y, prev_mean, prev_rstd, prev_sums};
    KAGNN_CHECK_ARG((prev_sums == nullptr) == (prev_y == nullptr), "prev_y and prev_sums come together");
    const GraphSide gr{.rowptr = rowptr_t, .col = col_t, .hub_seg = hub_seg_t, .num_hub_seg = num_hub_seg_t, .hub_threshold = hub_threshold,
                       .self_scale = self_scale};
    const KanChain c{.N = N, .L = L, .widths = widths, .sw = sw, .sc = sc, .acts = acts, .pack_dx = pack_dx,
                     .knots = knots, .G = G, .K = K, .mode = mode};
    const LayerGrads io{.gy = g, .ldgy = ldg, .gx = gx, .gx_dtype = gx_dtype, .ldgx = ldgx, .bf16_gather = bf16_gather, .gx_addend = gx_addend,
                        .ld_addend = ld_addend, .g_bw = g_bw, .g_sw = g_sw, .g_sc = g_sc};
    return layer_bwd_impl(gr, c, io, &bn, bn_sums, prev_sums ? &so : nullptr, nullptr, nullptr, workspace, workspace_bytes, stream, __func__);
}

int kagnn_gin_kan_layer_bwd(const float* gy, int64_t ldgy, int64_t N, const int32_t* rowptr_t, const int32_t* col_t,
                            const int32_t* hub_seg_t, int64_t num_hub_seg_t, int32_t hub_threshold, float self_scale,
                            int32_t L, const int32_t* widths, const float* const* sw, const float* const* sc,
                            const float* knots, int32_t G, int32_t K, int32_t mode, const float* const* acts,
                            const void* const* pack_dx, void* gx, int32_t gx_dtype, int64_t ldgx, int32_t bf16_gather,
                            float* const* g_bw, float* const* g_sw, float* const* g_sc, void* workspace,
                            size_t workspace_bytes, void* stream) {
    ModeScope mode_scope_(mode);
    return kagnn_gin_kan_layer_bwd_add(gy, ldgy, N, rowptr_t, col_t, hub_seg_t, num_hub_seg_t, hub_threshold, self_scale, L, widths, sw,
                                       sc, knots, G, K, mode, acts, pack_dx, gx, gx_dtype, ldgx, bf16_gather, nullptr, 0, g_bw, g_sw,
                                       g_sc, workspace, workspace_bytes, stream);
}

// ---- the same ONE call per convolution each way around GINE message passing (BASELINE config 4: the ZINC-shaped mini-batch step is
// host- and launch-bound, graph_regression/models.py:107-119, optuna_zinc.py:56-66).  Forward = kagnn_aggregate_gine + one pack
// launch + the chain (column moments of the output for the BatchNorm1d that follows, when col_mean is given); backward = [the norm's
// statistics pass and its element-wise backward inside the last input-gradient kernel, when bn_y is given] + the chain's
// dW / dX + kagnn_aggregate_gine_bwd.  Same kernels, same order, same bits as the per-operation composition.  fp32 rows; the
// structure arrays are those of kagnn_csr_build (forward: by destination; backward: by source), small graphs: no hub segments.
// Workspace: kagnn_gin_kan_layer_workspace_bytes (num_hub_seg = 0) [+ kagnn_gin_kan_layer_bwd_bn_workspace_bytes].
int kagnn_gine_kan_layer_fwd(const float* x, int64_t ldx, const float* edge_attr, int64_t lde, int64_t N, const int32_t* rowptr,
                             const int32_t* col, const int32_t* perm, float self_scale,
                             int32_t L, const int32_t* widths, const float* const* bw, const float* const* sw,
                             const float* const* sc, const float* knots, int32_t G, int32_t K, int32_t mode,
                             float* const* acts, void* const* pack_fwd, void* const* pack_dx, float* col_mean,
                             float* col_m2, void* workspace, size_t workspace_bytes, void* stream) {
    ModeScope mode_scope_(mode);
    KAGNN_CHECK_ARG(N == 0 || (x && edge_attr && perm && widths && ldx >= widths[0] && lde >= widths[0]), "null array or short leading dimension");
    const GineStage gs{x, ldx, edge_attr, lde, perm, nullptr, 0};
    const GraphSide gr{.rowptr = rowptr, .col = col, .self_scale = self_scale};
    const KanChain c{.N = N, .L = L, .widths = widths, .bw = bw, .sw = sw, .sc = sc, .acts = acts, .pack_fwd = pack_fwd, .pack_dx = pack_dx,
                     .knots = knots, .G = G, .K = K, .mode = mode};
    const LayerIn in{.x = x, .x_dtype = KAGNN_DTYPE_F32, .ldx = ldx, .col_mean = col_mean,
                     .col_m2 = col_m2};
    return layer_fwd_impl(gr, c, in, &gs, workspace, workspace_bytes, stream, __func__);
}

int kagnn_gine_kan_layer_bwd(const float* g, int64_t ldg, const float* bn_y, int64_t ld_bn_y, const float* bn_weight,
                             const float* bn_mean, const float* bn_rstd, float* g_bn_weight, float* g_bn_bias,
                             const float* x, int64_t ldx, const float* edge_attr, int64_t lde, int64_t N,
                             const int32_t* rowptr_t, const int32_t* col_t, const int32_t* perm_t, float self_scale,
                             int32_t L, const int32_t* widths, const float* const* sw, const float* const* sc,
                             const float* knots, int32_t G, int32_t K, int32_t mode, const float* const* acts,
                             const void* const* pack_dx, float* gx, int64_t ldgx, float* g_edge_attr, int64_t ldge,
                             float* const* g_bw, float* const* g_sw, float* const* g_sc, void* workspace,
                             size_t workspace_bytes, void* stream) {
    ModeScope mode_scope_(mode);
    KAGNN_CHECK_ARG(N == 0 || (x && edge_attr && perm_t && gx && widths && ldx >= widths[0] && lde >= widths[0] && ldgx >= widths[0]),
                    "null array or short leading dimension (gx is required: the edge-attribute gradient comes out of the same kernel)");
    KAGNN_CHECK_ARG(!g_edge_attr || ldge >= widths[0], "short leading dimension of g_edge_attr");
    const GineStage gs{x, ldx, edge_attr, lde, perm_t, g_edge_attr, ldge};
    const BnStage bn{bn_y, ld_bn_y, bn_weight, bn_mean, bn_rstd, g_bn_weight, g_bn_bias};
    const GraphSide gr{.rowptr = rowptr_t, .col = col_t, .self_scale = self_scale};
    const KanChain c{.N = N, .L = L, .widths = widths, .sw = sw, .sc = sc, .acts = acts, .pack_dx = pack_dx,
                     .knots = knots, .G = G, .K = K, .mode = mode};
    const LayerGrads io{.gy = g, .ldgy = ldg, .gx = gx, .gx_dtype = KAGNN_DTYPE_F32, .ldgx = ldgx, .g_bw = g_bw, .g_sw = g_sw, .g_sc = g_sc};
    return layer_bwd_impl(gr, c, io, bn_y ? &bn : nullptr, nullptr, nullptr, &gs, nullptr, workspace, workspace_bytes, stream, __func__);
}

// ---- the WHOLE message-passing stack of a graph-level model in one call each way (round 5): nconv x {GINE convolution around a KAN
// chain of L layers -> training-mode BatchNorm1d}, every chain hidden -> ... -> hidden with the same widths (reference
// graph_regression/models.py:107-119: `for i in range(n_layers): x = self.bn[i](self.conv[i](x, edge_index, edge_attr))`).  On a
// 256-molecule mini-batch a convolution is ~100 us of device work; as one tape node per convolution the HOST spent ~100 us per node
// each way on argument marshalling and allocations -- the step was host-bound at twice its device time.  Forward: ONE pack launch for
// all nconv * L layers, then per convolution kagnn_aggregate_gine, the chain (column moments from the last kernel) and the
// normalising pass -> h[i].  Backward: per convolution (last first) the norm's statistics pass, its element-wise backward inside
// the last input-gradient kernel, dW / dX, kagnn_aggregate_gine_bwd; the edge-attribute gradients of the nconv convolutions add
// up in g_edge_attr in place.  Same kernels and orders as nconv calls of kagnn_gine_kan_layer_fwd / _bwd: same bits.
// Array arguments: widths [L + 1] (widths[0] == widths[L]); per layer, convolution-major [nconv * L]: base_weight, spline_weight,
// spline_scaler, pack_fwd, pack_dx, g_*; acts [nconv * (L + 1)]; per convolution [nconv]: self_scale / momentum / eps (HOST floats),
// bn_weight, bn_bias, running_mean, running_var (device; the last two NULL arrays or NULL entries: no running statistics), h,
// save_mean, save_rstd, g_bn_weight, g_bn_bias.  Workspace: kagnn_gine_kan_stack_workspace_bytes.
int kagnn_gine_kan_stack_workspace_bytes(int64_t N, int32_t nconv, int32_t L, const int32_t* widths, int32_t G, int32_t K, int32_t mode,
                                         size_t* fwd_bytes, size_t* bwd_bytes) {
    ModeScope mode_scope_(mode);
    KAGNN_CHECK_ARG(N >= 0 && nconv >= 1 && L >= 1 && L <= 8 && widths && fwd_bytes && bwd_bytes, "bad argument");
    KAGNN_CHECK_ARG(widths[0] == widths[L], "every convolution of the stack maps hidden -> hidden");
    StackLayout lay;
    int rc = stack_layout(N, nconv, L, widths, G, K, mode, lay);
    if (rc) return rc;
    *fwd_bytes = lay.fwd_total;
    *bwd_bytes = lay.bwd_total;
    return KAGNN_OK;
}

int kagnn_gine_kan_stack_fwd(const float* x, int64_t ldx, const float* edge_attr, int64_t lde, int64_t N, const int32_t* rowptr,
                             const int32_t* col, const int32_t* perm, const float* self_scale, int32_t nconv,
                             int32_t L, const int32_t* widths, const float* const* bw, const float* const* sw,
                             const float* const* sc, const float* knots, int32_t G, int32_t K, int32_t mode,
                             float* const* acts, void* const* pack_fwd, void* const* pack_dx,
                             const float* const* bn_weight, const float* const* bn_bias, float* const* running_mean,
                             float* const* running_var, const float* momentum, const float* eps,
                             float* const* h, float* const* save_mean, float* const* save_rstd,
                             void* workspace, size_t workspace_bytes, void* stream) {
    return stack_fwd_impl(x, ldx, edge_attr, lde, N, rowptr, col, perm, self_scale, nconv, L, widths, bw, sw, sc, knots, G, K, mode, acts, pack_fwd,
                          pack_dx, bn_weight, bn_bias, running_mean, running_var, momentum, eps, h, save_mean, save_rstd, workspace,
                          workspace_bytes, stream, false);
}

int kagnn_gine_kan_stack_bwd(const float* g, int64_t ldg, const float* x, int64_t ldx, const float* edge_attr, int64_t lde, int64_t N,
                             const int32_t* rowptr_t, const int32_t* col_t, const int32_t* perm_t, const float* self_scale,
                             int32_t nconv, int32_t L, const int32_t* widths, const float* const* sw, const float* const* sc,
                             const float* knots, int32_t G, int32_t K, int32_t mode, const float* const* acts,
                             const void* const* pack_dx, const float* const* h, const float* const* bn_weight,
                             const float* const* save_mean, const float* const* save_rstd,
                             float* gx, int64_t ldgx, float* g_edge_attr, int64_t ldge, float* const* g_bn_weight, float* const* g_bn_bias,
                             float* const* g_bw, float* const* g_sw, float* const* g_sc, void* workspace, size_t workspace_bytes,
                             void* stream) {
    ModeScope mode_scope_(mode);
    KAGNN_CHECK_ARG(nconv >= 1 && L >= 1 && L <= 8 && widths && self_scale && sw && acts && pack_dx && h && bn_weight && save_mean && save_rstd &&
                    g_bn_weight && g_bn_bias && g_sw && gx && x && edge_attr, "null array");
    KAGNN_CHECK_ARG(widths[0] == widths[L] && N >= 2 && ldgx >= widths[0], "hidden -> hidden chains, at least two rows");
    StackLayout lay;
    int rc = stack_layout(N, nconv, L, widths, G, K, mode, lay);
    if (rc) return rc;
    KAGNN_CHECK_ARG(workspace && workspace_bytes >= lay.bwd_total, "workspace too small (kagnn_gine_kan_stack_workspace_bytes)");
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    const int H = widths[0];
    float* pp[2] = {reinterpret_cast<float*>(ws + lay.pp[0]), reinterpret_cast<float*>(ws + lay.pp[1])};
    // every layer's row slabs in an area of their own, all nconv * L slab reductions in one launch after the last convolution
    DwDefer defer{};
    const float* gcur = g;
    int64_t ldcur = ldg;
    for (int i = nconv - 1; i >= 0; --i) {
        const float* in = i == 0 ? x : h[i - 1];
        const int64_t ldin = i == 0 ? ldx : H;
        float* gout = i == 0 ? gx : pp[i & 1];
        const int64_t ldo = i == 0 ? ldgx : H;
        GineStage gs{in, ldin, edge_attr, lde, perm_t, g_edge_attr, ldge};
        gs.accumulate_g_ea = i < nconv - 1 ? 1 : 0;
        const BnStage bn{acts[i * (L + 1) + L], H, bn_weight[i], save_mean[i], save_rstd[i], g_bn_weight[i], g_bn_bias[i]};
        const DwPiece piece{ws + lay.arena + (size_t)(nconv - 1 - i) * lay.arena_conv_bytes, &defer};       // (in the order the backward runs)
        const GraphSide gr{.rowptr = rowptr_t, .col = col_t, .self_scale = self_scale[i]};
        const KanChain c{.N = N, .L = L, .widths = widths, .sw = sw + i * L, .sc = sc ? sc + i * L : nullptr,
                         .acts = acts + i * (L + 1), .pack_dx = pack_dx + i * L, .knots = knots, .G = G, .K = K, .mode = mode};
        const LayerGrads io{.gy = gcur, .ldgy = ldcur, .gx = gout, .gx_dtype = KAGNN_DTYPE_F32, .ldgx = ldo, .g_bw = g_bw ? g_bw + i * L : nullptr,
                            .g_sw = g_sw + i * L, .g_sc = g_sc ? g_sc + i * L : nullptr};
        rc = layer_bwd_impl(gr, c, io, &bn, nullptr, nullptr, &gs, lay.arena_bytes ? &piece : nullptr, ws, lay.bwd_layer_bytes, stream, __func__);
        if (rc) return rc;
        gcur = gout; ldcur = ldo;
    }
    {
        KAGNN_STAGE_AS("kagnn_kan_linear_bwd_weight (slab reductions of the stack)", stream);
        return dw_defer_flush(&defer, as_stream(stream));
    }
}


// ---------------------------------------------------------------- the whole graph-regression model per call (round 6)
// KAGIN.forward of the reference's graph_regression/models.py:107-119 and its backward as ONE library call each way: the sequence of
// this file's own entry points that kagnn_amd/graph_ops.py::_KaginModelFn runs from Python, with the same arguments in the same
// order -- the same kernels, the same bits -- minus ~17 ctypes round trips, ~45 tensor allocations and their pointer tables.
// (inside the extern "C" bracket, where these helpers have always been: km_check / km_layout show in the dynamic symbol table, and
// the export list stays as it is)
namespace {
struct KmLayout {
    // `saved`: byte offsets
    size_t x0, ea, acts, h, stats, packs, pooled, ro_act[KAGNN_MODEL_MAX_READOUT], ro_pf[KAGNN_MODEL_MAX_READOUT], ro_pd[KAGNN_MODEL_MAX_READOUT], saved_total;
    size_t fb, db;                       // one stack layer's forward / input-gradient pack, 256-aligned
    // workspaces: byte offsets of the fixed parts, then the shared scratch of the sub-calls
    size_t fwd_scratch, fwd_total;
    size_t bwd_gy[2], bwd_gh, bwd_gx0, bwd_gea, bwd_scratch, bwd_total;
    size_t grads_floats;
    size_t g_atom[KAGNN_MODEL_MAX_TABLES], g_bond[KAGNN_MODEL_MAX_TABLES], g_bn_w[KAGNN_MODEL_MAX_CONVS], g_bn_b[KAGNN_MODEL_MAX_CONVS];
    size_t g_bw[KAGNN_MODEL_MAX_LAYERS], g_sw[KAGNN_MODEL_MAX_LAYERS], g_sc[KAGNN_MODEL_MAX_LAYERS];
    size_t g_ro_bw[KAGNN_MODEL_MAX_READOUT], g_ro_sw[KAGNN_MODEL_MAX_READOUT], g_ro_sc[KAGNN_MODEL_MAX_READOUT];   // float offsets into grads
    bool ro_batch;                       // the read-out's packs in one launch (kagnn_kan_pack_batch)
};

int km_check(const kagnn_kagin_model_t* m, const char* fn) {
    if (!m) return fail(KAGNN_ERR_ARG, "%s: null model", fn);
    const bool ok = m->num_nodes >= 2 && m->num_edges >= 0 && m->num_graphs >= 1 && m->hidden >= 1 && m->hidden <= 64 &&
                    m->num_atom_tables >= 1 && m->num_atom_tables <= KAGNN_MODEL_MAX_TABLES && m->num_bond_tables >= 1 &&
                    m->num_bond_tables <= KAGNN_MODEL_MAX_TABLES && m->x_stride >= m->num_atom_tables && m->e_stride >= m->num_bond_tables &&
                    m->num_convs >= 1 && m->num_convs <= KAGNN_MODEL_MAX_CONVS && m->num_layers >= 1 && m->num_layers <= 8 &&
                    m->num_convs * m->num_layers <= KAGNN_MODEL_MAX_LAYERS && m->num_readout >= 1 && m->num_readout <= KAGNN_MODEL_MAX_READOUT &&
                    m->readout_widths[0] == m->hidden;
    if (!ok) return fail(KAGNN_ERR_ARG, "%s: sizes outside the limits of kagnn_kagin_model_t (include/kagnn_hip.h)", fn);
    // the per-operation calls the layout is sized with take orders up to KAGNN_MAX_SPLINE_ORDER; the model calls do not
    if (m->spline_order < 1 || m->spline_order > kMaxOrder || m->readout_spline_order < 1 || m->readout_spline_order > kMaxOrder)
        return fail(KAGNN_ERR_UNSUPPORTED, "%s: spline_order and readout_spline_order must be 1..4", fn);
    return KAGNN_OK;
}

int km_layout(const kagnn_kagin_model_t* m, KmLayout& L, const char* fn) {
    int rc = km_check(m, fn);
    if (rc) return rc;
    const size_t N = (size_t)m->num_nodes, E = (size_t)m->num_edges, B = (size_t)m->num_graphs, H = (size_t)m->hidden;
    const int nconv = (int)m->num_convs, nl = (int)m->num_layers, G = (int)m->grid_size, K = (int)m->spline_order, mode = (int)m->mode;
    const int C = G + K;
    size_t fb = 0, db = 0;
    rc = kagnn_kan_pack_bytes((int)H, (int)H, G, K, mode, &fb, &db); if (rc) return rc;
    L.fb = al256z(fb); L.db = al256z(db);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += al256z(bytes); return at; };
    L.x0 = take(N * H * 4);
    L.ea = take((E ? E : 1) * H * 4);
    L.acts = take((size_t)nconv * (nl + 1) * N * H * 4);
    L.h = take((size_t)nconv * N * H * 4);
    L.stats = take((size_t)nconv * 2 * H * 4);
    L.packs = take((size_t)nconv * nl * (L.fb + L.db));
    L.pooled = take(B * H * 4);
    const int nr = (int)m->num_readout;
    bool batch = nr >= 2 && (int)m->readout_spline_order == 3 && (int)m->readout_grid_size + 3 <= 8;
    for (int i = 0; i < nr; ++i) {
        const int fin = (int)m->readout_widths[i], fout = (int)m->readout_widths[i + 1], rm = (int)m->readout_modes[i];
        if (fin < 1 || fout < 1) return fail(KAGNN_ERR_ARG, "%s: read-out widths", fn);
        L.ro_act[i] = i == 0 ? L.pooled : take(B * (size_t)fin * 4);          // input of read-out layer i
        size_t pf = 0, pd = 0;
        rc = kagnn_kan_pack_bytes(fin, fout, (int)m->readout_grid_size, (int)m->readout_spline_order, rm, &pf, &pd); if (rc) return rc;
        L.ro_pf[i] = take(pf); L.ro_pd[i] = take(pd);
        batch = batch && rm == (int)m->readout_modes[0] && (rm == KAGNN_PREC_SPLIT || rm == KAGNN_PREC_HALF) && fout <= 64;
    }
    L.ro_batch = batch;
    L.saved_total = o + 256;
    // forward workspace: the stack's, the read-out forwards' split-K scratch
    int32_t widths[9];
    for (int l = 0; l <= nl; ++l) widths[l] = (int32_t)H;
    StackLayout stack;
    {
        int32_t md = mode;
        ModeScope mode_scope_(md);
        rc = stack_layout((int64_t)N, nconv, nl, widths, G, K, md, stack); if (rc) return rc;
    }
    size_t scratch_f = stack.fwd_total, scratch_b = stack.bwd_total;
    for (int i = 0; i < nr; ++i) {
        const int fin = (int)m->readout_widths[i], fout = (int)m->readout_widths[i + 1], rm = (int)m->readout_modes[i];
        size_t a = 0, b = 0;
        rc = kagnn_kan_fwd_workspace_bytes((int64_t)B, fin, fout, (int)m->readout_grid_size, (int)m->readout_spline_order, rm, &a); if (rc) return rc;
        rc = kagnn_kan_bwd_weight_workspace_bytes((int64_t)B, fin, fout, (int)m->readout_grid_size, (int)m->readout_spline_order, rm, &b); if (rc) return rc;
        scratch_f = scratch_f > a ? scratch_f : a;
        scratch_b = scratch_b > b ? scratch_b : b;
    }
    for (int t = 0; t < (int)m->num_atom_tables; ++t) {
        size_t a = 0;
        rc = kagnn_embedding_bwd_workspace_bytes((int64_t)N, (int)m->atom_rows[t], (int)H, &a); if (rc) return rc;
        scratch_b = scratch_b > a ? scratch_b : a;
    }
    for (int t = 0; t < (int)m->num_bond_tables; ++t) {
        size_t a = 0;
        rc = kagnn_embedding_bwd_workspace_bytes((int64_t)E, (int)m->bond_rows[t], (int)H, &a); if (rc) return rc;
        scratch_b = scratch_b > a ? scratch_b : a;
    }
    L.fwd_scratch = 0; L.fwd_total = al256z(scratch_f) + 256;
    size_t wmax = 1;
    for (int i = 0; i <= nr; ++i) wmax = wmax > (size_t)m->readout_widths[i] ? wmax : (size_t)m->readout_widths[i];
    o = 0;
    L.bwd_gy[0] = take(B * wmax * 4); L.bwd_gy[1] = take(B * wmax * 4);
    L.bwd_gh = take(N * H * 4); L.bwd_gx0 = take(N * H * 4); L.bwd_gea = take((E ? E : 1) * H * 4);
    L.bwd_scratch = o; L.bwd_total = o + al256z(scratch_b) + 256;
    // the flat gradient buffer (floats)
    size_t g = 0;
    for (int t = 0; t < (int)m->num_atom_tables; ++t) { L.g_atom[t] = g; g += (size_t)m->atom_rows[t] * H; }
    for (int t = 0; t < (int)m->num_bond_tables; ++t) { L.g_bond[t] = g; g += (size_t)m->bond_rows[t] * H; }
    for (int i = 0; i < nconv; ++i) {
        L.g_bn_w[i] = g; g += H; L.g_bn_b[i] = g; g += H;
        for (int l = 0; l < nl; ++l) {
            const int k = i * nl + l;
            L.g_bw[k] = g; g += H * H; L.g_sw[k] = g; g += H * H * C; L.g_sc[k] = g; g += H * H;
        }
    }
    for (int i = 0; i < nr; ++i) {
        const size_t fin = (size_t)m->readout_widths[i], fout = (size_t)m->readout_widths[i + 1];
        const size_t Cr = (size_t)(m->readout_grid_size + m->readout_spline_order);
        L.g_ro_bw[i] = g; g += fout * fin; L.g_ro_sw[i] = g; g += fout * fin * Cr;
        L.g_ro_sc[i] = g; if (m->readout_spline_scaler[i]) g += fout * fin;
    }
    L.grads_floats = g;
    return KAGNN_OK;
}
}  // namespace

int kagnn_kagin_model_struct_bytes(void) { return (int)sizeof(kagnn_kagin_model_t); }

int kagnn_kagin_model_sizes(const kagnn_kagin_model_t* m, size_t* saved_bytes, size_t* fwd_ws, size_t* bwd_ws, size_t* grads_floats) {
    KAGNN_CHECK_ARG(saved_bytes && fwd_ws && bwd_ws && grads_floats, "null output");
    KmLayout L;
    int rc = km_layout(m, L, __func__);
    if (rc) return rc;
    *saved_bytes = L.saved_total; *fwd_ws = L.fwd_total; *bwd_ws = L.bwd_total; *grads_floats = L.grads_floats;
    return KAGNN_OK;
}

int kagnn_kagin_model_fwd(const kagnn_kagin_model_t* m, void* stream) {
    KmLayout L;
    int rc = km_layout(m, L, __func__);
    if (rc) return rc;
    KAGNN_CHECK_ARG(m->saved && m->workspace && m->out && m->x_index && m->rowptr && m->seg_ptr && m->knots, "null array");
    KAGNN_CHECK_ARG(m->num_edges == 0 || (m->e_index && m->col && m->perm), "null edge array");       // (a batch of single atoms has none)
    KAGNN_CHECK_ARG((size_t)m->saved_bytes >= L.saved_total && (size_t)m->workspace_bytes >= L.fwd_total,
                    "saved / workspace too small (kagnn_kagin_model_sizes)");
    const int64_t N = m->num_nodes, E = m->num_edges, B = m->num_graphs;
    const int H = (int)m->hidden, nconv = (int)m->num_convs, nl = (int)m->num_layers, G = (int)m->grid_size, K = (int)m->spline_order, mode = (int)m->mode;
    unsigned char* sv = static_cast<unsigned char*>(m->saved);
    unsigned char* ws = static_cast<unsigned char*>(m->workspace);
    float* x0 = reinterpret_cast<float*>(sv + L.x0);
    float* ea = reinterpret_cast<float*>(sv + L.ea);
    // encoders: sum over the feature columns of one table each (models.py:244-281)
    for (int t = 0; t < (int)m->num_atom_tables; ++t) {
        rc = kagnn_embedding_fwd(m->x_index + t, m->x_stride, N, m->atom_table[t], (int32_t)m->atom_rows[t], H, x0, H, t > 0, stream);
        if (rc) return rc;
    }
    if (E == 0) { KAGNN_HIP(hipMemsetAsync(ea, 0, (size_t)H * sizeof(float), as_stream(stream))); }   // (a batch of single atoms: a row nothing reads)
    for (int t = 0; t < (int)m->num_bond_tables; ++t) {
        rc = kagnn_embedding_fwd(m->e_index + t, m->e_stride, E, m->bond_table[t], (int32_t)m->bond_rows[t], H, ea, H, t > 0, stream);
        if (rc) return rc;
    }
    // the GINE stack
    int32_t widths[9];
    for (int l = 0; l <= nl; ++l) widths[l] = H;
    float* acts[KAGNN_MODEL_MAX_CONVS * 9];
    void* pf[KAGNN_MODEL_MAX_LAYERS]; void* pd[KAGNN_MODEL_MAX_LAYERS];
    float* h[KAGNN_MODEL_MAX_CONVS]; float* mean[KAGNN_MODEL_MAX_CONVS]; float* rstd[KAGNN_MODEL_MAX_CONVS];
    const size_t hs = (size_t)N * H * sizeof(float);
    for (int k = 0; k < nconv * (nl + 1); ++k) acts[k] = reinterpret_cast<float*>(sv + L.acts + (size_t)k * hs);
    for (int k = 0; k < nconv * nl; ++k) { pf[k] = sv + L.packs + (size_t)k * L.fb; pd[k] = sv + L.packs + (size_t)nconv * nl * L.fb + (size_t)k * L.db; }
    for (int i = 0; i < nconv; ++i) {
        h[i] = reinterpret_cast<float*>(sv + L.h + (size_t)i * hs);
        mean[i] = reinterpret_cast<float*>(sv + L.stats) + (size_t)(2 * i) * H;
        rstd[i] = reinterpret_cast<float*>(sv + L.stats) + (size_t)(2 * i + 1) * H;
    }
    // ONE pack launch for the stack's layers AND the read-out's where they share grid, order and mode (each layer's pack depends on
    // its own weights only: the same bits as the two launches of the per-operation path)
    const int nr = (int)m->num_readout, rG = (int)m->readout_grid_size, rK = (int)m->readout_spline_order;
    void* rpf[KAGNN_MODEL_MAX_READOUT]; void* rpd[KAGNN_MODEL_MAX_READOUT];
    int32_t rin[KAGNN_MODEL_MAX_READOUT], rout[KAGNN_MODEL_MAX_READOUT];
    for (int i = 0; i < nr; ++i) { rpf[i] = sv + L.ro_pf[i]; rpd[i] = sv + L.ro_pd[i]; rin[i] = (int32_t)m->readout_widths[i]; rout[i] = (int32_t)m->readout_widths[i + 1]; }
    bool packed_all = false;
    {
        int32_t md = mode;
        ModeScope mode_scope_(md);
        bool ok = nconv * nl + nr <= 16 && L.ro_batch && rG == G && rK == K && (int)m->readout_modes[0] == mode &&
                  use_split_dx(H, H, G, K, md) && use_sparse_fwd(H, H, G, K, md) && kan_fused_pack_ok(H, H, G + K);
        for (int i = 0; i < nr && ok; ++i)
            ok = use_split_dx(rin[i], rout[i], G, K, md) && use_sparse_fwd(rin[i], rout[i], G, K, md) && kan_fused_pack_ok(rin[i], rout[i], G + K);
        if (ok) {
            const float* abw[16]; const float* asw[16]; const float* asc[16]; int32_t ain[16], aout[16]; void* apf[16]; void* apd[16];
            int n = 0;
            for (int k = 0; k < nconv * nl; ++k, ++n) { abw[n] = m->base_weight[k]; asw[n] = m->spline_weight[k]; asc[n] = m->spline_scaler[k]; ain[n] = H; aout[n] = H; apf[n] = pf[k]; apd[n] = pd[k]; }
            for (int i = 0; i < nr; ++i, ++n) { abw[n] = m->readout_base_weight[i]; asw[n] = m->readout_spline_weight[i]; asc[n] = m->readout_spline_scaler[i]; ain[n] = rin[i]; aout[n] = rout[i]; apf[n] = rpf[i]; apd[n] = rpd[i]; }
            rc = kagnn_kan_pack_batch(n, abw, asw, asc, ain, aout, G, K, mode, apf, apd, stream);
            if (rc) return rc;
            packed_all = true;
        }
    }
    rc = stack_fwd_impl(x0, H, ea, H, N, m->rowptr, m->col, m->perm, m->self_scale, nconv, nl, widths, m->base_weight, m->spline_weight,
                        m->spline_scaler, m->knots, G, K, mode, acts, pf, pd, m->bn_weight, m->bn_bias,
                        const_cast<float* const*>(m->running_mean), const_cast<float* const*>(m->running_var), m->momentum, m->eps, h, mean, rstd,
                        ws + L.fwd_scratch, (size_t)m->workspace_bytes - L.fwd_scratch, stream, packed_all);
    if (rc) return rc;
    // global_add_pool, then the read-out chain
    float* pooled = reinterpret_cast<float*>(sv + L.pooled);
    rc = kagnn_segment_pool(h[nconv - 1], H, pooled, H, m->seg_ptr, B, H, 0, stream);
    if (rc) return rc;
    if (L.ro_batch && !packed_all) {
        rc = kagnn_kan_pack_batch(nr, m->readout_base_weight, m->readout_spline_weight, m->readout_spline_scaler, rin, rout, rG, rK,
                                  (int32_t)m->readout_modes[0], rpf, rpd, stream);
        if (rc) return rc;
    }
    for (int i = 0; i < nr; ++i) {
        const int rm = (int)m->readout_modes[i];
        if (!L.ro_batch && !packed_all) {
            rc = kagnn_kan_pack(m->readout_base_weight[i], m->readout_spline_weight[i], m->readout_spline_scaler[i], rin[i], rout[i], rG, rK, rm, rpf[i], rpd[i], stream);
            if (rc) return rc;
        }
        const float* xin = reinterpret_cast<const float*>(sv + L.ro_act[i]);
        float* y = i + 1 < nr ? reinterpret_cast<float*>(sv + L.ro_act[i + 1]) : m->out;
        size_t wb = 0;
        rc = kagnn_kan_fwd_workspace_bytes(B, rin[i], rout[i], rG, rK, rm, &wb); if (rc) return rc;
        rc = kagnn_kan_linear_fwd(xin, rin[i], B, m->readout_knots[i], rin[i], rout[i], rG, rK, rm, rpf[i], y, rout[i],
                                  wb ? ws + L.fwd_scratch : nullptr, wb, stream);
        if (rc) return rc;
    }
    return KAGNN_OK;
}

int kagnn_kagin_model_bwd(const kagnn_kagin_model_t* m, void* stream) {
    KmLayout L;
    int rc = km_layout(m, L, __func__);
    if (rc) return rc;
    KAGNN_CHECK_ARG(m->saved && m->workspace && m->g_out && m->grads && m->x_index && m->rowptr_t && m->seg_ptr && m->knots, "null array");
    KAGNN_CHECK_ARG(m->num_edges == 0 || (m->e_index && m->col_t && m->perm_t), "null edge array");
    KAGNN_CHECK_ARG((size_t)m->saved_bytes >= L.saved_total && (size_t)m->workspace_bytes >= L.bwd_total,
                    "saved / workspace too small (kagnn_kagin_model_sizes)");
    const int64_t N = m->num_nodes, E = m->num_edges, B = m->num_graphs;
    const int H = (int)m->hidden, nconv = (int)m->num_convs, nl = (int)m->num_layers, G = (int)m->grid_size, K = (int)m->spline_order, mode = (int)m->mode;
    unsigned char* sv = static_cast<unsigned char*>(m->saved);
    unsigned char* ws = static_cast<unsigned char*>(m->workspace);
    float* gr = m->grads;
    const int nr = (int)m->num_readout, rG = (int)m->readout_grid_size, rK = (int)m->readout_spline_order;
    KAGNN_CHECK_ARG(m->ld_g_out >= m->readout_widths[nr], "ld_g_out smaller than the model's output width");
    // read-out, last layer first: input gradient, then weight gradient (the order of graph_ops._KaginModelFn.backward)
    const float* gy = m->g_out;
    int64_t ldgy = m->ld_g_out;
    for (int i = nr - 1; i >= 0; --i) {
        const int fin = (int)m->readout_widths[i], fout = (int)m->readout_widths[i + 1], rm = (int)m->readout_modes[i];
        const float* xin = reinterpret_cast<const float*>(sv + L.ro_act[i]);
        float* gx = reinterpret_cast<float*>(ws + L.bwd_gy[i & 1]);
        rc = kagnn_kan_linear_bwd_input(xin, fin, gy, ldgy, B, m->readout_knots[i], fin, fout, rG, rK, rm, sv + L.ro_pd[i], gx, fin, KAGNN_DTYPE_F32, stream);
        if (rc) return rc;
        size_t wb = 0;
        rc = kagnn_kan_bwd_weight_workspace_bytes(B, fin, fout, rG, rK, rm, &wb); if (rc) return rc;
        rc = kagnn_kan_linear_bwd_weight(xin, fin, gy, ldgy, B, m->readout_knots[i], fin, fout, rG, rK, rm, m->readout_spline_weight[i],
                                         m->readout_spline_scaler[i], gr + L.g_ro_bw[i], gr + L.g_ro_sw[i],
                                         m->readout_spline_scaler[i] ? gr + L.g_ro_sc[i] : nullptr, ws + L.bwd_scratch, wb, stream);
        if (rc) return rc;
        gy = gx; ldgy = fin;
    }
    // pool backward, the stack, the encoders
    float* gh = reinterpret_cast<float*>(ws + L.bwd_gh);
    rc = kagnn_segment_broadcast(gy, ldgy, gh, H, m->seg_ptr, B, H, 0, stream);
    if (rc) return rc;
    int32_t widths[9];
    for (int l = 0; l <= nl; ++l) widths[l] = H;
    const float* acts[KAGNN_MODEL_MAX_CONVS * 9];
    const void* pd[KAGNN_MODEL_MAX_LAYERS];
    const float* h[KAGNN_MODEL_MAX_CONVS]; const float* mean[KAGNN_MODEL_MAX_CONVS]; const float* rstd[KAGNN_MODEL_MAX_CONVS];
    float* g_bn_w[KAGNN_MODEL_MAX_CONVS]; float* g_bn_b[KAGNN_MODEL_MAX_CONVS];
    float* g_bw[KAGNN_MODEL_MAX_LAYERS]; float* g_sw[KAGNN_MODEL_MAX_LAYERS]; float* g_sc[KAGNN_MODEL_MAX_LAYERS];
    const size_t hs = (size_t)N * H * sizeof(float);
    for (int k = 0; k < nconv * (nl + 1); ++k) acts[k] = reinterpret_cast<const float*>(sv + L.acts + (size_t)k * hs);
    for (int k = 0; k < nconv * nl; ++k) {
        pd[k] = sv + L.packs + (size_t)nconv * nl * L.fb + (size_t)k * L.db;
        g_bw[k] = gr + L.g_bw[k]; g_sw[k] = gr + L.g_sw[k]; g_sc[k] = gr + L.g_sc[k];
    }
    for (int i = 0; i < nconv; ++i) {
        h[i] = reinterpret_cast<const float*>(sv + L.h + (size_t)i * hs);
        mean[i] = reinterpret_cast<const float*>(sv + L.stats) + (size_t)(2 * i) * H;
        rstd[i] = reinterpret_cast<const float*>(sv + L.stats) + (size_t)(2 * i + 1) * H;
        g_bn_w[i] = gr + L.g_bn_w[i]; g_bn_b[i] = gr + L.g_bn_b[i];
    }
    const float* x0 = reinterpret_cast<const float*>(sv + L.x0);
    const float* ea = reinterpret_cast<const float*>(sv + L.ea);
    float* gx0 = reinterpret_cast<float*>(ws + L.bwd_gx0);
    float* gea = reinterpret_cast<float*>(ws + L.bwd_gea);
    rc = kagnn_gine_kan_stack_bwd(gh, H, x0, H, ea, H, N, m->rowptr_t, m->col_t, m->perm_t, m->self_scale, nconv, nl, widths, m->spline_weight,
                                  m->spline_scaler, m->knots, G, K, mode, acts, pd, h, m->bn_weight, mean, rstd, gx0, H, gea, H, g_bn_w, g_bn_b, g_bw, g_sw,
                                  g_sc, ws + L.bwd_scratch, (size_t)m->workspace_bytes - L.bwd_scratch, stream);
    if (rc) return rc;
    for (int t = 0; t < (int)m->num_atom_tables; ++t) {
        size_t wb = 0;
        rc = kagnn_embedding_bwd_workspace_bytes(N, (int32_t)m->atom_rows[t], H, &wb); if (rc) return rc;
        rc = kagnn_embedding_bwd(m->x_index + t, m->x_stride, N, gx0, H, (int32_t)m->atom_rows[t], H, gr + L.g_atom[t], ws + L.bwd_scratch, wb, stream);
        if (rc) return rc;
    }
    for (int t = 0; t < (int)m->num_bond_tables; ++t) {
        size_t wb = 0;
        rc = kagnn_embedding_bwd_workspace_bytes(E, (int32_t)m->bond_rows[t], H, &wb); if (rc) return rc;
        rc = kagnn_embedding_bwd(m->e_index + t, m->e_stride, E, gea, H, (int32_t)m->bond_rows[t], H, gr + L.g_bond[t], ws + L.bwd_scratch, wb, stream);
        if (rc) return rc;
    }
    return KAGNN_OK;
}

}  // extern "C"
#pragma GCC visibility pop
