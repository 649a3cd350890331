// Host-side declarations shared by the translation units of libkagnn_hip.so: every launcher and helper that one .hip file
// defines and another calls, and the scopes and predicates the entry points (api.hip, fused_calls.hip) share.  Included by the
// file that defines a function as well as by the files that call it, so the compiler checks each definition against the one
// prototype; default arguments appear only here.
#pragma once
#include "common.h"

namespace kagnn {

struct RbfArgs;                                     // split_common.h (device-side detail of the *_any launchers)

// ---- aggregate.hip
size_t aggregate_ws_bytes(long num_hub_seg, int F);
// The co-run launch of the row kernel: the backward's transposed aggregation while the layer's deferred weight gradients run on
// a side stream (fused_calls.hip: layer_bwd_impl; measurements: profiles/bwd_overlap.md, profiles/bwd_corun_priority.md).  The row
// groups go in two launches of agg_rows_v4_corun_kernel, or in one when head_pct is 100 (then there is no tail: the head, the wait
// for side_done, the hub kernels).  The HEAD -- the first head_pct per cent of them -- runs beside the weight gradients and must never keep
// one of their workgroups from being placed: a weight-gradient wave holds 352 of a SIMD's 512 registers and its workgroup 2.5 KB of
// a CU's 160 KiB of LDS, so the head asks for kAggCorunLds bytes of dynamic LDS it never touches -- four such requests fit beside
// that workgroup, five do not even alone -- which holds it to four 256-thread workgroups per CU = four waves per SIMD of at most
// kAggCorunVgprs registers each, the 160 a weight-gradient wave leaves, whichever kernel the hardware starts first.  Then the stream
// waits for side_done (the side stream's work) and the TAIL, the remaining row groups, runs with the whole machine.
struct AggCorun { int head_pct; hipEvent_t side_done; };
constexpr unsigned kAggCorunLds = 40000;
constexpr int kAggCorunVgprs = 40;
int aggregate_sum(const AggArgs& a, const int* hub_seg, long num_hub_seg, float* ws, size_t ws_bytes, hipStream_t st,
                  const AggCorun* corun = nullptr);
bool aggregate_corun_ok(const AggArgs& a);
bool aggregate_stats_ok(const AggArgs& a);
long aggregate_stats_rows(long N, int F, long num_hub_seg);
int gcn_deg_inv_sqrt(const int* rowptr, const int* col, long N, float* dis, hipStream_t st);
int gine_fwd(const float* x, long ldx, const float* ea, long lde, float* out, long ldo, const int* rowptr, const int* col, const
             int* perm, long N, int F, float self_scale, hipStream_t st);
int gine_bwd(const float* x, long ldx, const float* ea, long lde, const float* gout, long ldg, float* gx, long ldgx, float* gea,
             long ldge, const int* rowptr, const int* col, const int* perm, long N, int F, float self_scale, hipStream_t st, int
             gea_accumulate = 0);
int segment_pool(const float* x, long ldx, float* out, long ldo, const int* seg, long B, int F, int mean, hipStream_t st);
int segment_bcast(const float* g, long ldg, float* gx, long ldgx, const int* seg, long B, int F, int mean, hipStream_t st);
int embedding_fwd(const int64_t* idx, long stride, long N, const float* table, int V, int F, float* out, long ldo, int accumulate,
                  hipStream_t st);
int embedding_bwd(const int64_t* idx, long stride, long N, const float* g, long ldg, int V, int F, float* g_table, float* ws, size_t
                  ws_bytes, hipStream_t st);
size_t embedding_bwd_ws_bytes(long N, int V, int F);

int aggregate_hub_rows(const AggArgs& a, const int* hub_seg, long num_hub_seg, float* ws, size_t ws_bytes, hipStream_t st);

// ---- aggregate_edge.hip
int aggregate_edge_grad(const EdgeGradArgs& a, const int* hub_seg, long num_hub_seg, hipStream_t st);

// ---- aggregate_bf16.hip
size_t aggregate_bf16_ws_bytes(long num_hub_seg, int F);
bool aggregate_bf16_ok(const void* x, long ldx, const void* out, long ldo, int out_bf16, int F, const float* bias);
int aggregate_sum_bf16(const void* x, long ldx, void* out, long ldo, int out_bf16, const int* rowptr, const int* col, const float*
                       ew, long N, int F, float self_scale, const float* in_scale, const float* out_scale, const float* bias, int
                       skip_self, const int* hub_seg, long num_hub_seg, int hub_threshold, float* ws, size_t ws_bytes, hipStream_t
                       st);
int rows_to_bf16(const float* x, long ldx, void* y, long ldy, long N, int F, hipStream_t st);

// ---- kan_sparse_fwd.hip
bool kan_sparse_fwd_agg_ok(const float* x, long ldx, long N, int in, int out, int G, int K);
size_t kan_sparse_fwd_agg_ws_bytes(long num_hub_seg, int in, int out);
int kan_sparse_fwd_agg(const float* x, long ldx, long N, const int* rowptr, const int* col, const int* hub_seg, long num_hub_seg,
                       int hub_threshold, float self_scale, const float* knots, int in, int out, int G, int K, const void* pack,
                       float* h0, long ldh, float* y, long ldy, void* ws, size_t ws_bytes, hipStream_t st);
bool kan_sparse_fwd_ok(int in, int out, int G, int K);
bool kan_fused_pack_ok(int in, int out, int C);
int kan_fused_pack(const float* bw, const float* sw, const float* sc, int in, int out, int C, void* pack_fwd, void* pack_dx,
                   hipStream_t st);
int kan_fused_pack_batch(int n, const float* const* bw, const float* const* sw, const float* const* sc, const int* in, const int*
                         out, int C, void* const* pack_fwd, void* const* pack_dx, hipStream_t st);
size_t kan_sparse_pack_fwd_bytes(int in, int out, int C);
int kan_sparse_pack_fwd(const float* bw, const float* sw, const float* sc, int in, int out, int C, void* pack_fwd, hipStream_t st);
size_t kan_sparse_fwd_ws_bytes(long N, int in, int out, int C);
int kan_sparse_fwd(const float* x, long ldx, long N, const float* knots, int in, int out, int G, int K, const void* pack, float* y,
                   long ldy, void* ws, size_t ws_bytes, float* col_mean, float* col_m2, hipStream_t st);
bool kan_sparse_fwd_parts_ok(const int* widths, int nparts, int in, int out, int G, int K);
int kan_sparse_fwd_parts(const float* const* parts, const int* widths, const long* lds, int nparts, long N, const float* knots, int
                         in, int out, int G, int K, const void* pack, float* y, long ldy, void* ws, size_t ws_bytes, hipStream_t st,
                         const float* const* part_affine);
bool kan_sparse_fwd_moments_ok(long N, int in, int out, int G, int K);
size_t kan_sparse_fwd_moments_ws_bytes(long N, int out);

// ---- bn.hip
size_t bn_stats_fold_bytes(long B, int F);
int bn_sums_from_partials(float* ws, long B, int F, float* sums, hipStream_t st);
int bn_finish_partials(const float* partial, long B, int F, float* sums, hipStream_t st);
int bn_bwd_stats_given(const float* sums, long N, int F, const float* gamma, const float* save_mean, const float* save_rstd, float*
                       g_gamma, float* g_beta, float* tab, int ldt, hipStream_t st);
int col_moments(const float* x, long ldx, long N, int F, float* col_mean, float* col_m2, void* ws, size_t ws_bytes, hipStream_t st);
size_t bn_ws_bytes(long N, int F);
int bn_fwd(const float* x, long ldx, long N, int F, const float* gamma, const float* beta, float* running_mean, float* running_var,
           float momentum, float eps, int training, const float* col_mean, const float* col_m2, float dropout_p, unsigned long long
           dropout_seed, float* y, long ldy, float* save_mean, float* save_rstd, void* ws, size_t ws_bytes, hipStream_t st);
int bn_bwd(const float* x, long ldx, const float* gy, long ldgy, long N, int F, const float* gamma, const float* save_mean, const
           float* save_rstd, int training, float dropout_p, unsigned long long dropout_seed, float* gx, long ldgx, float* g_gamma,
           float* g_beta, void* ws, size_t ws_bytes, hipStream_t st);
int bn_bwd_stats(const float* x, long ldx, const float* gy, long ldgy, long N, int F, const float* gamma, const float* save_mean,
                 const float* save_rstd, float* g_gamma, float* g_beta, float* tab, int ldt, void* ws, size_t ws_bytes, hipStream_t
                 st);
int bn_stats_affine(const float* col_mean, const float* col_m2, long N, int F, const float* gamma, const float* beta, float*
                    running_mean, float* running_var, float momentum, float eps, float* save_mean, float* save_rstd, float* affine,
                    hipStream_t st);
int moments_finish(const float* partial, int P, int F, float* col_mean, float* col_m2, hipStream_t st);

// ---- csr.hip
int csr_workspace_bytes(long E, long N, size_t* bytes);
int csr_build(const int64_t* key, const int64_t* val, long E, long N, int* rowptr, int* col, int* perm, int T, int* hub_seg, long
              cap, int64_t* nseg_host, void* ws, size_t ws_bytes, hipStream_t st);
bool csr_small_ok(long E, long N);
size_t csr_small_workspace_bytes(long E);
int csr_build_small(const int64_t* src, const int64_t* dst, long E, long N, int* rowptr, int* col, int* perm, int* rowptr_t, int*
                    col_t, int* perm_t, int* flags, void* ws, size_t ws_bytes, hipStream_t st);

// ---- subgraph.hip
int subgraph_workspace_bytes(long N, long E, size_t* bytes);
int k_hop_mark(const int* rowptr, const int* col, long N, const int64_t* seeds, long S, int num_hops, int* hop, int* flags, hipStream_t st);
int subgraph_count(const int* hop, const int* rowptr, const int* col, const int* perm, const int* rowptr_t, const int* col_t, long N, long E,
                   void* ws, size_t ws_bytes, int* counts, hipStream_t st);
int subgraph_fill(const void* ws, size_t ws_bytes, const int* rowptr, const int* col, const int* perm, const int* rowptr_t, const int* col_t,
                  const int* perm_t, long N, long E, long n_sub, long e_sub, int64_t* nodes, int64_t* edge_ids, int64_t* ei, int* rowptr_o,
                  int* col_o, int* perm_o, int* rowptr_to, int* col_to, int* perm_to, hipStream_t st);
int neighbor_sample_mark(const int* rowptr, const int* col, const int* perm, long N, long E, const int64_t* seeds, long S, const int* fanout,
                         int num_levels, unsigned long long seed, int* hop, unsigned char* keep, int* flags, hipStream_t st);
int edge_subgraph_count(const int* hop, const unsigned char* keep, const int* rowptr, const int* col, const int* perm, const int* rowptr_t,
                        const int* col_t, const int* perm_t, long N, long E, void* ws, size_t ws_bytes, int* counts, hipStream_t st);
int edge_subgraph_fill(const void* ws, size_t ws_bytes, const unsigned char* keep, const int* rowptr, const int* col, const int* perm,
                       const int* rowptr_t, const int* col_t, const int* perm_t, long N, long E, long n_sub, long e_sub, int64_t* nodes,
                       int64_t* edge_ids, int64_t* ei, int* rowptr_o, int* col_o, int* perm_o, int* rowptr_to, int* col_to, int* perm_to,
                       hipStream_t st);

// ---- linkpred.hip
size_t edge_keys_ws_bytes(long E);
int edge_keys_build(const int64_t* src, const int64_t* dst, long E, long N, int64_t* keys, int64_t* num_keys, void* ws, size_t ws_bytes,
                    hipStream_t st);
int negative_sample(const int64_t* keys, long K, long N, long num, unsigned long long seed, int T, int64_t* pairs, unsigned char* valid,
                    hipStream_t st);
int bce_logits_fwd(const float* s, const unsigned char* y, const unsigned char* w, long P, float* loss, int64_t* divisor, void* record,
                   void* ws, size_t ws_bytes, hipStream_t st);
int bce_logits_bwd(const float* s, const unsigned char* y, const unsigned char* w, long P, const int64_t* divisor, const float* g_loss,
                   float* g, hipStream_t st);
size_t link_rank_ws_bytes(long P);
int link_rank(const float* s, const unsigned char* y, const unsigned char* wgt, long P, const int* ks_host, int num_ks, int64_t* record,
              void* ws, size_t ws_bytes, hipStream_t st);

// ---- kan_fp32.hip
size_t kan_f32_pack_fwd_bytes(int in, int out, int C);
size_t kan_f32_pack_dx_bytes(int in, int out, int C);
int kan_f32_pack(const float* bw, const float* sw, const float* sc, int in, int out, int C, float* pf, float* pd, hipStream_t st);
int kan_f32_fwd(const float* x, long ldx, long N, const float* knots, int in, int out, int G, int K, const float* pack, float* y,
                long ldy, bool pf, hipStream_t st);
int kan_f32_dx(const float* x, long ldx, const float* gy, long ldgy, long N, const float* knots, int in, int out, int G, int K,
               const float* pack, float* gx, long ldgx, bool pf, hipStream_t st);
size_t kan_f32_dw_ws_bytes(long N, int in, int out, int C);
int kan_f32_dw(const float* x, long ldx, const float* gy, long ldgy, long N, const float* knots, int in, int out, int G, int K,
               const float* sw, const float* sc, float* g_bw, float* g_sw, float* g_sc, float* ws, size_t ws_bytes, bool pf,
               hipStream_t st);
int kan_dw_unpack(const float* gcat, int in, int out, int C, long inP, long outP, const float* sw, const float* sc, float* g_bw,
                  float* g_sw, float* g_sc, hipStream_t st);
int kan_dw_reduce(const float* slab, long NS, long per_slab, float* gcat, hipStream_t st);
void dw_plan(long N, int in, int out, int* NBx, long* rpw);

// ---- kan_high_order.hip (spline orders 5..KAGNN_MAX_SPLINE_ORDER, exact fp32; the packs, slab reduction and unpack are kan_fp32.hip's)
int kan_ho_fwd(const float* x, long ldx, long N, const float* knots, int in, int out, int G, int K, const float* pack, float* y,
               long ldy, bool pf, hipStream_t st);
int kan_ho_dx(const float* x, long ldx, const float* gy, long ldgy, long N, const float* knots, int in, int out, int G, int K,
              const float* pack, float* gx, long ldgx, bool pf, hipStream_t st);
int kan_ho_dw(const float* x, long ldx, const float* gy, long ldgy, long N, const float* knots, int in, int out, int G, int K,
              const float* sw, const float* sc, float* g_bw, float* g_sw, float* g_sc, float* ws, size_t ws_bytes, bool pf,
              hipStream_t st);
int kan_ho_bsplines(const float* x, long ldx, long N, const float* grid, int in, int G, int K, float* bases, hipStream_t st);

// ---- kan_split.hip
size_t kan_split_pack_fwd_bytes(int in, int out, int C);
int kan_split_pack_fwd_noscale(const float* bw, const float* sw, const float* sc, int in, int out, int C, void* pack_fwd,
                               hipStream_t st);
int kan_split_fwd(const float* x, long ldx, long N, const float* knots, int in, int out, int G, int K, const void* pack, float* y,
                  long ldy, void* ws, size_t ws_bytes, hipStream_t st);
size_t kan_split_fwd_ws_bytes(long N, int in, int out, int C);
bool kan_split_fwd_ok(int in, int out, int G, int K);
int kan_split_fwd_any(const float* x, long ldx, long N, const float* knots, int in, int out, int G, int K, const void* pack, float*
                      y, long ldy, const RbfArgs& rb, void* ws, size_t ws_bytes, hipStream_t st);

// ---- kan_split_bwd.hip
size_t kan_split_pack_dx_bytes(int in, int out, int C, int K);
int kan_split_pack_dx_noscale(const float* bw, const float* sw, const float* sc, int in, int out, int C, int K, void* pack_dx,
                              hipStream_t st);
int kan_split_dx(const float* x, long ldx, const float* gy, long ldgy, long N, const float* knots, int in, int out, int G, int K,
                 const void* pack, float* gx, long ldgx, hipStream_t st, int gx16, const float* x_affine);
size_t kan_split_dw_ws_bytes(long N, int in, int out, int C, int K);
int kan_split_dw(const float* x, long ldx, const float* gy, long ldgy, long N, const float* knots, int in, int out, int G, int K,
                 const float* sw, const float* sc, float* g_bw, float* g_sw, float* g_sc, float* ws, size_t ws_bytes, hipStream_t
                 st, const float* x_affine, DwDefer* defer);
bool kan_split_dx_ok(int in, int out, int G, int K);
int kan_split_dx_stats_blocks(long N);
bool kan_split_dx_stats_ok(long N, int in, int out, int G, int K);
int kan_split_dx_stats(const float* x, long ldx, const float* gy, long ldgy, long N, const float* knots, int in, int out, int G, int
                       K, const void* pack, float* gx, long ldgx, hipStream_t st, const float* x_affine, const float* st_mean, const
                       float* st_rstd, float* st_partial);
bool kan_split_dw_ok(int in, int out, int G, int K);
bool kan_split_dx_bn_ok(long ldg, int in, int out, int G, int K, const BnBack& b, const void* g);
int kan_split_dx_bn(const float* x, long ldx, const float* g, long ldg, long N, const float* knots, int in, int out, int G, int K,
                    const void* pack, float* gx, long ldgx, const BnBack& bnb, hipStream_t st);
int kan_split_dx_any(const float* x, long ldx, const float* gy, long ldgy, long N, const float* knots, int in, int out, int G, int
                     K, const void* pack, float* gx, long ldgx, const RbfArgs& rb, hipStream_t st, int gx16);
int kan_split_dw_any(const float* x, long ldx, const float* gy, long ldgy, long N, const float* knots, int in, int out, int G, int
                     K, const float* sw, const float* sc, float* g_bw, float* g_sw, float* g_sc, float* ws, size_t ws_bytes, const
                     RbfArgs& rb, hipStream_t st, DwDefer* defer);
void kan_split_dw_slabs(long N, int in, int out, int C, int K, long* slabs, long* outP);

// ---- fastkan.hip
int fastkan_fwd(const float* x, long ldx, long N, int in, int out, int ng, const float* centers, float den, const float* lnw, const
                float* lnb, float eps, const float* sw, const float* bw, const float* bb, float* y, long ldy, float* stats, void*
                ws, size_t ws_bytes, int mode, hipStream_t st, bool stats_given = false);
bool fastkan_fwd_stats_in_kernel(long N, int in, int out, int ng, int mode);
int fastkan_row_moments(const float* x, long ldx, long N, int in, float* moments, hipStream_t st);
int fastkan_merge_moments(const float* gathered, int P, long N, int in, float eps, float* stats, hipStream_t st);
size_t fastkan_fwd_ws_bytes(long N, int in, int out, int ng, int mode);
size_t fastkan_bwd_ws_bytes(long N, int in, int out, int ng, int mode);
int fastkan_bwd(const float* x, long ldx, const float* gy, long ldgy, long N, int in, int out, int ng, const float* centers, float
                den, const float* lnw, const float* lnb, float eps, const float* sw, const float* bw, const float* stats, float* gx,
                long ldgx, float* g_lnw, float* g_lnb, float* g_sw, float* g_bw, float* g_bb, void* ws, size_t ws_bytes, int mode,
                hipStream_t st, int phase = 0, float* row_sums = nullptr, int in_total = 0);

// the LayerNorm pieces of the layer that its edge kernels (fastkan_edge.hip) run as they are: row statistics (mean, rstd) [N, 2],
// and the backward through the normalisation (gx += ..., both parameter gradients; lnpart: fastkan_ln_bwd_ws_bytes)
int launch_stats(const float* x, long ldx, long N, int in, float eps, float* stats, hipStream_t st);
size_t fastkan_ln_bwd_ws_bytes(long N, int in);
int fastkan_ln_bwd(const float* x, long ldx, const float* gz, long N, int in, const float* lnw, const float* lnb, float eps,
                   const float* stats, float* gx, long ldgx, float* g_lnw, float* g_lnb, float* lnpart, hipStream_t st);

// ---- fastkan_edge.hip (per-edge activations of a FastKANLayer: abs sum over the rows, its backward, sampled curves; exact fp32)
size_t fastkan_edge_abs_sum_ws_bytes(long N, int in, int out, bool layernorm);
size_t fastkan_edge_abs_sum_bwd_ws_bytes(long N, int in, int out, int ng, bool layernorm);
int fastkan_edge_abs_sum(const float* x, long ldx, long N, int in, int out, int ng, const float* centers, float den, const float* lnw,
                         const float* lnb, float eps, const float* sw, const float* bw, float* S, long ldS, void* ws, size_t ws_bytes,
                         hipStream_t st);
int fastkan_edge_abs_sum_bwd(const float* x, long ldx, long N, int in, int out, int ng, const float* centers, float den, const float*
                             lnw, const float* lnb, float eps, const float* sw, const float* bw, const float* gS, long ldgS, float*
                             g_sw, float* g_bw, float* gx, long ldgx, float* g_lnw, float* g_lnb, void* ws, size_t ws_bytes,
                             hipStream_t st);
int fastkan_edge_curves(const float* t, long ldt, const float* tb, long ldtb, long P, int in, int out, int ng, const float* centers,
                        float den, const float* sw, const float* bw, float* phi, hipStream_t st);

// ---- symbolic.hip
size_t symbolic_ws_bytes(long N, int in, int out, int F);
int symbolic_fit(const float* x, long ldx, const float* phi, long N, int in, int out, const int* functions, int F, float alo,
                 float ahi, float blo, float bhi, int Gn, int iterations, float* params, float* r2, float* tables, float* ranges,
                 int* winners, void* ws, size_t ws_bytes, hipStream_t st);

// ---- symbolic_edges.hip (fixed symbolic edges of a KANLinear: sum over a sparse edge list of c f(a x + b) + d, and its backward)
size_t symbolic_edges_plan_bytes(long E, int in, int out);
int symbolic_edges_plan(const int* edges_host, long E, int in, int out, int* plan_host);
size_t symbolic_edges_bwd_ws_bytes(long N, long E);
int symbolic_edges_fwd(const float* x, long ldx, long N, int in, int out, const int* plan_host, const int* plan_dev,
                       const float* affine, const float* y_in, long ldyin, float* y, long ldy, hipStream_t st);
int symbolic_edges_bwd(const float* x, long ldx, const float* gy, long ldgy, long N, int in, int out, const int* plan_host,
                       const int* plan_dev, const float* affine, float* gx, long ldgx, float* g_affine, void* ws, size_t ws_bytes,
                       hipStream_t st);

// ---- gat.hip
int gat_logits(const float* xh, long ld, long N, int H, int C, const float* att_src, const float* att_dst, float* a_s, float* a_d,
               hipStream_t st);
int gat_fwd(const float* xh, long ld, const float* a_s, const float* a_d, const int* rowptr, const int* col, long N, int H, int C,
            const float* bias, float* out, long ldo, float* m, float* z, const int* hub_seg, long num_hub_seg, int hub_threshold,
            hipStream_t st);
int gat_bwd(const float* xh, long ld, const float* gout, long ldg, const float* y, long ldy, const float* bias, const float* a_s,
            const float* a_d, const float* m, const float* z, const int* rowptr, const int* col, const int* perm, const int*
            rowptr_t, const int* col_t, const int* perm_t, const float* att_src, const float* att_dst, long N, int H, int C, float*
            gpre, float* gpre_self, float* g_d, float* g_s, float* gx, long ldgx, const int* hub_seg, long num_hub_seg, int
            hub_threshold, hipStream_t st);
size_t gat_att_grad_ws_bytes(long N, int H, int C);
int gat_att_grad(const float* xh, long ld, const float* g_src, const float* g_dst, long N, int H, int C, float* g_att_src, float*
                 g_att_dst, void* ws, size_t ws_bytes, hipStream_t st);

// ---- kan_grid.hip
int kan_bsplines(const float* x, long ldx, long N, const float* grid, int in, int G, int K, float* bases, hipStream_t st);
size_t kan_grid_resize_ws_bytes(long N, int in, int Cn, int Co);
int kan_grid_resize(const float* x, long ldx, long N, const float* grid_old, const float* grid_new, const float* window, int in,
                    int out, int G_old, int G_new, int K, const float* sw, const float* sc, float* new_sw, int* untouched, void* ws,
                    size_t ws_bytes, hipStream_t st);

// ---- loss.hip
size_t xent_ws_bytes(long N);
int xent_fwd(const float* z, long ld, long N, int C, const long* y, const unsigned char* mask, int pre, float* loss, float* stats,
             float* count, void* ws, size_t ws_bytes, hipStream_t st);
int xent_bwd(const float* z, long ld, long N, int C, const long* y, const unsigned char* mask, int pre, const float* stats, const
             float* count, const float* gloss, float* gz, long ldg, hipStream_t st);
int l1_loss_fwd(const float* p, const float* t, long n, float* loss, hipStream_t st);
int l1_loss_bwd(const float* p, const float* t, long n, const float* g_loss, float* g_p, hipStream_t st);
int adam_step(int count, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, const
              long* numel, float lr, float beta1, float beta2, float eps, float weight_decay, long step, hipStream_t st);

// ---- classify.hip
int degree_one_hot(const int* rowptr, long N, int K, float* x, long ldx, hipStream_t st);
int nll_loss_fwd(const float* logp, long ld, long rows, int C, const long* y, float* loss_mean, float* loss_sum, void* accum, int*
                 flag, hipStream_t st);
int nll_loss_bwd(const long* y, long rows, int C, const float* g_loss, int reduction, float* g_logp, long ldg, hipStream_t st);

// ---- nodeclass.hip
size_t node_eval_ws_bytes(long N, int C, int S);
int node_eval(const float* z, long ld, long N, int C, const long* y, const unsigned char* bits, int S, void* records, int* flag,
              void* ws, size_t ws_bytes, hipStream_t st);
int early_stop_update(const void* records, int S, int val_split, void* state, void* history, int max_epochs, hipStream_t st);
int copy_if(const int* flag, int count, void* const* dst, const void* const* src, const long* bytes, hipStream_t st);

// ---- regress.hip
int l1_loss_meter_fwd(const float* pred, long ldp, const float* target, long ldt, long rows, int T, const float* scale, float*
                      loss_mean, void* meter, hipStream_t st);
int regression_epoch_update(void* train_meter, void* val_meter, void* test_meter, long n_train, long n_val, long n_test, void* state,
                            double* history, int max_epochs, hipStream_t st);

// ---- linear.hip
int linear_fwd(const float* x, long ldx, long N, int in, const float* W, const float* bias, int out, int relu, float* y, long ldy,
               hipStream_t st);
int linear_dx(const float* gy, long ldgy, const float* y, long ldy, long N, int out, const float* W, int in, float* gx, long ldgx,
              hipStream_t st);
void linear_dw_plan(long N, int in, int out, long* slabs, long* rows_per_slab);
size_t linear_dw_ws_bytes(long N, int in, int out);
int linear_dw(const float* x, long ldx, const float* gy, long ldgy, const float* y, long ldy, long N, int in, int out, float* gW,
              float* gb, float* ws, size_t ws_bytes, hipStream_t st);
// c[M,Nc] = a[M,K] b[Nc,K]^T with a row stride on all three (the forward's product without bias / ReLU and a strided weight)
int linear_abt(const float* a, long lda, long M, int K, const float* b, long ldb, long Nc, float* c, long ldc, hipStream_t st);

// ---- attention.hip (dense multi-head attention, bias after the softmax; exact fp32, no atomics)
int attention_fwd(const float* wq, long ldq, const float* wk, long ldk, const float* wv, long ldv, const float* bias, long bias_bs,
                  long bias_rs, const float* gate, long ldg, long B, long Q, long K, int H, int c, float scale, float* o, long ldo,
                  float* o_ungated, long ldou, float* stats, hipStream_t st);
size_t attention_bwd_ws_bytes(long B, long Q, long K, int H, int c, int has_gate);
int attention_bwd(const float* g_out, long ldgo, const float* wq, long ldq, const float* wk, long ldk, const float* wv, long ldv,
                  const float* bias, long bias_bs, long bias_rs, const float* gate, long ldg, const float* o_ungated, long ldou,
                  const float* stats, long B, long Q, long K, int H, int c, float scale, float* g_wq, long ldgq, float* g_wk,
                  long ldgk, float* g_wv, long ldgv, float* g_bias, long gb_bs, long gb_rs, float* g_gate, long ldgg, float* ws,
                  size_t ws_bytes, hipStream_t st);

// ---- kan_edge.hip (per-edge activations phi_{o,i}: abs sum over the rows, its backward, sampled curves; exact fp32, orders 1..4)
size_t kan_edge_abs_sum_ws_bytes(long N, int in, int out);
size_t kan_edge_abs_sum_bwd_ws_bytes(long N, int in, int out, int C);
int kan_edge_abs_sum(const float* x, long ldx, long N, const float* knots, bool pf, int in, int out, int G, int K, const float* bw,
                     const float* sw, const float* sc, float* S, long ldS, float* ws, size_t ws_bytes, hipStream_t st);
int kan_edge_abs_sum_bwd(const float* x, long ldx, long N, const float* knots, bool pf, int in, int out, int G, int K, const float*
                         bw, const float* sw, const float* sc, const float* gS, long ldgS, float* g_bw, float* g_sw, float* g_sc,
                         float* gx, long ldgx, float* ws, size_t ws_bytes, hipStream_t st);
int kan_edge_curves(const float* t, long ldt, long P, const float* knots, bool pf, int in, int out, int G, int K, const float* bw,
                    const float* sw, const float* sc, float* phi, hipStream_t st);
size_t kan_edge_moments_ws_bytes(long N, int in, int out);
int kan_edge_moments(const float* x, long ldx, long N, const float* knots, bool pf, int in, int out, int G, int K, const float* bw,
                     const float* sw, const float* sc, float* mean, long ld_mean, float* m2, long ld_m2, float* ws, size_t ws_bytes,
                     hipStream_t st);

// ---- p2p.hip
int p2p_reduce_scatter(const float* const* parts, int P, int rank, long N, int out, long ld, float* y, long ldy, hipStream_t st);
int p2p_all_gather(const float* const* shards, int P, long N, int w, long lds, float* g, long ldg, hipStream_t st);

// ---- api.hip
// kagnn_kan_linear_bwd_weight[_affine] with the stack call's deferral (DwDefer, common.h) as an argument: defer != nullptr says that
// ws is a piece of that call's slab arena and the slab reduction is recorded instead of launched.  Same stage name, checks and
// messages as the entry point.
int kan_linear_bwd_weight(const float* x, int64_t ldx, const float* x_affine, const float* gy, int64_t ldgy, int64_t N, const float* knots,
                          int32_t in, int32_t out, int32_t G, int32_t K, int32_t mode, const float* sw, const float* sc, float* g_bw,
                          float* g_sw, float* g_sc, void* ws, size_t ws_bytes, void* stream, DwDefer* defer);

// ---------------------------------------------------------------- stage timer (measurement aid; off by default; state in api.hip)
// While enabled, every per-operation entry point -- ALSO when it runs inside kagnn_gin_kan_layer_fwd / _bwd* -- is bracketed by
// HIP events recorded on the stream it launches on, so that bench.py can time the dominant kernel live inside the timed region
// of the product's default path (one library call per convolution each way) instead of composing the layer from per-op calls.
struct StageScope {
    hipStream_t st;
    const char* name;
    hipEvent_t b = nullptr;
    StageScope(const char* nm, void* stream);
    ~StageScope();
};
#define KAGNN_STAGE(stream) kagnn::StageScope stage_scope_(__func__, stream)
#define KAGNN_STAGE_AS(name, stream) kagnn::StageScope stage_scope_(name, stream)

// KAGNN_PREC_HALF is KAGNN_PREC_SPLIT with ONE product per fp32 product: every routing decision below is the split mode's, the
// launchers of the three KAN kernels pick their HALF instantiation while the flag is up (shapes without one run the
// three-product kernels: more accurate, never less).  Entry points call each other with the rewritten mode, so a nested scope
// sees KAGNN_PREC_SPLIT and leaves the flag alone.
struct ModeScope {
    bool prev;
    explicit ModeScope(int32_t& mode) : prev(g_half_products) {
        if (mode == KAGNN_PREC_HALF) { g_half_products = true; mode = KAGNN_PREC_SPLIT; }
    }
    ~ModeScope() { g_half_products = prev; }
};

inline int check_kan_dims(const char* fn, int in, int out, int G, int K, int mode) {
    if (in < 1 || out < 1) return fail(KAGNN_ERR_ARG, "%s: in_features/out_features must be >= 1", fn);
    if (K < 1 || K > kMaxOrder) return fail(KAGNN_ERR_UNSUPPORTED, "%s: spline_order must be 1..4", fn);
    if (G < 1 || G + 2 * K + 1 > kMaxKnots) return fail(KAGNN_ERR_UNSUPPORTED, "%s: grid_size out of range", fn);
    if (mode != KAGNN_PREC_FP32 && mode != KAGNN_PREC_SPLIT && mode != KAGNN_PREC_FP32_GRID) return fail(KAGNN_ERR_ARG, "%s: unknown precision mode", fn);
    return KAGNN_OK;
}
// The per-operation KANLinear calls (pack, forward, both gradients, their workspace queries, the dense bases) also take orders
// kMaxOrder+1 .. KAGNN_MAX_SPLINE_ORDER, in the exact-fp32 modes only and with their own knot bound (kan_high_order.hip).  Every
// other entry point keeps check_kan_dims and so refuses those orders before it launches anything.
constexpr int kHighOrderMaxKnots = 64;
inline bool high_order(int K) { return K > kMaxOrder; }
inline int check_kan_dims_wide(const char* fn, int in, int out, int G, int K, int mode) {
    if (K <= kMaxOrder) return check_kan_dims(fn, in, out, G, K, mode);
    if (in < 1 || out < 1) return fail(KAGNN_ERR_ARG, "%s: in_features/out_features must be >= 1", fn);
    if (K > KAGNN_MAX_SPLINE_ORDER) return fail(KAGNN_ERR_UNSUPPORTED, "%s: spline_order must be 1..16", fn);
    if (mode == KAGNN_PREC_SPLIT) return fail(KAGNN_ERR_UNSUPPORTED, "%s: spline_order above 4 runs with KAGNN_PREC_FP32 or KAGNN_PREC_FP32_GRID only", fn);
    if (mode != KAGNN_PREC_FP32 && mode != KAGNN_PREC_FP32_GRID) return fail(KAGNN_ERR_ARG, "%s: unknown precision mode", fn);
    if (G < 1 || G + 2 * K + 1 > kHighOrderMaxKnots) return fail(KAGNN_ERR_UNSUPPORTED, "%s: grid_size + 2 * spline_order + 1 must be <= 64 at spline_order above 4", fn);
    return KAGNN_OK;
}
// the split path covers the hot shapes; everything else runs the exact-fp32 kernels (still HIP)
// the split kernels address activations through buffer descriptors with 32-bit byte offsets, re-opened at every
// workgroup tile (<= 256 rows forward / input gradient, <= 2^17 rows weight gradient): any N, rows up to 7680 floats
inline bool fits32(long N, long ld) { (void)N; return ld <= 7680; }
inline bool use_split_fwd(int in, int out, int G, int K, int mode) { return mode == KAGNN_PREC_SPLIT && kan_split_fwd_ok(in, out, G, K); }
inline bool use_sparse_fwd(int in, int out, int G, int K, int mode) { return use_split_fwd(in, out, G, K, mode) && kan_sparse_fwd_ok(in, out, G, K); }
inline bool use_split_dx(int in, int out, int G, int K, int mode) { return mode == KAGNN_PREC_SPLIT && kan_split_dx_ok(in, out, G, K); }
inline bool use_split_dw(int in, int out, int G, int K, int mode) { return mode == KAGNN_PREC_SPLIT && kan_split_dw_ok(in, out, G, K); }

inline size_t al256z(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace kagnn
