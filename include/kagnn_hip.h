/*
 * kagnn_hip.h -- C ABI of libkagnn_hip.so, the MI355X (gfx950) implementation of the
 * KAN-GNN layer hot path of RomanBresson/KAGNN.
 *
 * The reference has NO native boundary (it is 100 % Python on torch / torch_geometric); the
 * entry points below are what a ctypes binding inside the reference's layers would call in
 * place of the aten-op sequences cited on each function (paths relative to the reference
 * repository root).  INTEGRATION.md shows that binding.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless the name ends in _host;
 *  - matrices are row-major fp32 with an explicit leading dimension (elements) so column
 *    slices of a wider activation can be passed without a copy;
 *  - index arrays produced by this library are int32 (validated: N, E < 2^31); the edge list
 *    handed in is the reference's int64 `edge_index`;
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream); no call synchronises
 *    the device except kagnn_csr_build (documented there);
 *  - return value 0 = success, negative = error; kagnn_last_error() returns a message for the
 *    calling thread's most recent failure.  Nothing falls back to a CPU path.
 */
#ifndef KAGNN_HIP_H
#define KAGNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KAGNN_OK 0
#define KAGNN_ERR_ARG (-1)      /* bad argument (shape / range / null)            */
#define KAGNN_ERR_HIP (-2)      /* a HIP runtime call or kernel launch failed      */
#define KAGNN_ERR_UNSUPPORTED (-3)

/* precision of the dense contraction (the `mode` argument of the KAN entry points) */
#define KAGNN_PREC_FP32 0       /* v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate    */
#define KAGNN_PREC_SPLIT 1      /* fp16 hi/lo split operands, 3 MFMAs per product, fp32 accumulate */
#define KAGNN_PREC_FP32_GRID 2  /* exact fp32, and `knots` is the whole [in, G+2k+1] grid buffer: per-feature,
                                 * non-uniform knot rows (what KANLinear.update_grid leaves behind)       */
#define KAGNN_PREC_HALF 3       /* BUILD-DEFINED reduced precision (BASELINE config 2 "bf16"; the reference is fp32 only, ekan.py:154-162):
                                 * KAGNN_PREC_SPLIT's kernels with ONE fp16 product per fp32 product -- bases, SiLU, gy and the packed
                                 * weights are evaluated in fp32 and rounded once (RNE, 11 significant bits) after the same exact
                                 * power-of-two scaling, fp32 accumulate: a third of the matrix-core work, ~5e-4 from the fp32 result.
                                 * Cubic layers of <= 8 coefficients; any other shape runs the three-product kernels (more accurate).
                                 * Takes the same packs as KAGNN_PREC_SPLIT.  Never the headline.                              */

/* highest spline_order of the per-operation KANLinear calls (kagnn_kan_pack_bytes, kagnn_kan_pack, kagnn_kan_fwd_workspace_bytes,
 * kagnn_kan_linear_fwd, kagnn_kan_linear_bwd_input, kagnn_kan_bwd_weight_workspace_bytes, kagnn_kan_linear_bwd_weight,
 * kagnn_kan_bsplines).  Orders 5..16 run with KAGNN_PREC_FP32 / KAGNN_PREC_FP32_GRID only (KAGNN_PREC_SPLIT / _HALF return
 * KAGNN_ERR_UNSUPPORTED) and need grid_size + 2 * spline_order + 1 <= 64; every other entry point takes orders 1..4. */
#define KAGNN_MAX_SPLINE_ORDER 16

/* element type of an activation / gradient matrix where an entry point accepts more than fp32 */
#define KAGNN_DTYPE_F32 0
#define KAGNN_DTYPE_BF16 1

int kagnn_version(void);          /* 281 = 280 + kagnn_kan_edge_moments (+ _workspace_bytes); 280 = 279 + kagnn_symbolic_edges_plan (+ _bytes), kagnn_symbolic_edges_fwd, kagnn_symbolic_edges_bwd (+ _workspace_bytes); 279 = 278 + kagnn_symbolic_fit (+ _workspace_bytes); 278 = 277 + kagnn_edge_keys_build (+ _workspace_bytes), kagnn_negative_sample, kagnn_bce_logits_fwd / _bwd, kagnn_link_rank (+ _workspace_bytes); 277 = 276 + kagnn_neighbor_sample_mark, kagnn_edge_subgraph_count, kagnn_edge_subgraph_fill; 276 = 275 + kagnn_k_hop_mark, kagnn_subgraph_count, kagnn_subgraph_fill (+ kagnn_subgraph_workspace_bytes); 273 = 272 with kagnn_kan_grid_refit on kagnn_kan_grid_resize's kernels (up to 46 coefficients; its bits and its workspace size change); 272 = 271 + kagnn_kan_grid_resize (+ _workspace_bytes); 271 = 270 + kagnn_attention_fwd, kagnn_attention_bwd (+ _workspace_bytes); 270 = 269 + kagnn_fastkan_edge_abs_sum, kagnn_fastkan_edge_abs_sum_bwd (+ _workspace_bytes), kagnn_fastkan_edge_curves; 269 = 268 + kagnn_kan_edge_abs_sum, kagnn_kan_edge_abs_sum_bwd (+ _workspace_bytes), kagnn_kan_edge_curves; 268 = 267 + spline orders 5..KAGNN_MAX_SPLINE_ORDER in the per-operation KANLinear calls (no new entry point); 267 = 266 + kagnn_linear_fwd, kagnn_linear_bwd_input, kagnn_linear_bwd_weight (+ _workspace_bytes); 266 = 265 + kagnn_l1_loss_meter_fwd, kagnn_regression_epoch_update; 265 = 264 + kagnn_node_eval, kagnn_early_stop_update, kagnn_copy_if; 264 = 263 + kagnn_degree_one_hot, kagnn_nll_loss_fwd / _bwd; 263 = 262 + kagnn_batch_assemble; 262 = 261 - the fields edge_src, edge_dst, csr_flags of kagnn_kagin_model_t; 261 = 260 + kagnn_fastkan_fwd_stats_in_kernel; 260 = round 6: + the feature-sharded FastKAN entry points kagnn_fastkan_row_moments .. _shard_bwd_finish, + kagnn_kagin_model_*; 250 = 240 + KAGNN_PREC_HALF; 240 = 230 + kagnn_gin_kan_layer_bwd_bn_sums; 230 = 220 + the *_affine entry points of a folded BatchNorm1d; 220 = 210 + the stage timer) */
const char* kagnn_last_error(void);

/* Stage timer -- a measurement aid, off by default (no reference counterpart: the reference times whole epochs with
 * time.time(), node_classification_clean/time_model.py:38-47).  While enabled, every per-operation entry point below
 * (aggregation, weight packs, KANLinear forward / input gradient / weight gradient, FastKAN forward / backward, BatchNorm) is
 * bracketed by HIP events recorded on the stream it launches on -- ALSO when it runs inside kagnn_gin_kan_layer_fwd / _bwd*, so
 * a caller can time one kernel live inside the product's one-call-per-convolution path.  `only`: NULL = every stage, else the
 * one stage name to record (e.g. "kagnn_aggregate_sum").  kagnn_stage_timer_collect waits for the recorded events, sums them by
 * stage name into the caller's arrays (`names`: `capacity` slots of 64 chars) and clears the records. */
int kagnn_stage_timer_enable(const char* only);
int kagnn_stage_timer_disable(void);
int kagnn_stage_timer_collect(char* names, int64_t* launches, double* total_ms, int32_t capacity, int32_t* n_stages);

/* ------------------------------------------------------------------------------------------
 * Graph structure.  Replaces the per-call `index_select` / `scatter_add_` bookkeeping of
 * torch_geometric's MessagePassing.propagate (called from node_classification_clean/
 * models.py:48-56 via GINConv and :31-37 via GCNConv) by a CSR built once per edge_index.
 *
 * kagnn_csr_build: stable sort of the E edges by `key` (values 0..N-1).
 *   rowptr[N+1]  = exclusive prefix sum of the key histogram
 *   perm[E]      = argsort(key, stable)                (bit-exact contract)
 *   col[E]       = val[perm]
 * (key=dst,val=src) gives the forward structure, (key=src,val=dst) its transpose for backward.
 * Rows whose degree exceeds `hub_threshold` are split into segments of L = max(hub_threshold/4, 64)
 * edges, listed in hub_seg[3*i+{0,1,2}] = {row, e_begin, e_end} (a row's segments are contiguous
 * in e and its first one starts at rowptr[row]); *num_hub_seg_host receives their count (never
 * more than E/L + E/hub_threshold + 1, so size hub_seg for 3x that many int32).  This call
 * synchronises `stream` once (to return the count).
 * ------------------------------------------------------------------------------------------ */
int kagnn_csr_workspace_bytes(int64_t num_edges, int64_t num_nodes, size_t* bytes_host);
int kagnn_csr_build(const int64_t* key, const int64_t* val, int64_t num_edges, int64_t num_nodes,
                    int32_t* rowptr, int32_t* col, int32_t* perm,
                    int32_t hub_threshold, int32_t* hub_seg, int64_t hub_seg_capacity,
                    int64_t* num_hub_seg_host,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Small graphs (1 <= E, N <= 65 536; kagnn_csr_small_ok == 1) -- the mini-batches of the graph-level models, whose CSR is rebuilt
 * per batch (reference graph_regression/optuna_zinc.py:56-66 -> torch_geometric's propagate bookkeeping): BOTH structures in ONE
 * launch and with NO host synchronisation.  src / dst = edge_index[0] / edge_index[1] (int64); (rowptr, col, perm) by destination as
 * kagnn_csr_build(key = dst, val = src) makes them, (rowptr_t, col_t, perm_t) by source; same stable order, bit for bit.  Node ids
 * outside [0, num_nodes) are clamped to 0 (no out-of-bounds access follows) and reported in the DEVICE array flags[2] (bit 0: a key,
 * bit 1: a value; [0] destination side, [1] source side), which the caller reads when convenient.  No hub segments.
 * Workspace: kagnn_csr_small_workspace_bytes(E).                                                                                */
int kagnn_csr_small_ok(int64_t num_edges, int64_t num_nodes);
int kagnn_csr_small_workspace_bytes(int64_t num_edges, size_t* bytes_host);
int kagnn_csr_build_small(const int64_t* src, const int64_t* dst, int64_t num_edges, int64_t num_nodes, int32_t* rowptr,
                          int32_t* col, int32_t* perm, int32_t* rowptr_t, int32_t* col_t, int32_t* perm_t, int32_t* flags,
                          void* workspace, size_t workspace_bytes, void* stream);

/* k-hop neighbourhoods and induced subgraphs of an indexed graph (torch_geometric.utils.k_hop_subgraph / subgraph with
 * relabel_nodes=True, flow='source_to_target'; no counterpart in the reference, which explains nothing).  Three calls, in this
 * order, and ONE read-back between the second and the third; nothing here synchronises the stream.  All indices int32.  Every
 * result is a pure function of the inputs (no float, no atomic read-modify-write): two calls return the same bits.
 *
 * kagnn_k_hop_mark: (rowptr, col) = the parent's by-destination CSR.  hop[num_nodes]: the least number of hops from node i to any
 *   seed ALONG edge direction (seeds: 0; not reached within num_hops: -1).  Level-synchronous, one launch per level; a frontier row
 *   is walked by the 64 lanes of a wave.  A seed outside [0, num_nodes) sets the DEVICE int flags[0] = 1 (else 0) and is skipped:
 *   nothing is read or written out of bounds.  num_seeds == 0, num_nodes == 0 or num_hops == 0 launch no level kernel.  num_hops == 0
 *   turns a list of node ids (duplicates allowed) into the selection of an induced subgraph.
 * kagnn_subgraph_count: node i is selected iff hop[i] >= 0 (any int32 array will do); an edge is kept iff both endpoints are
 *   selected (self loops and duplicates as they are).  Takes both structures of the parent (perm_t is not read here) and leaves in
 *   the workspace -- which BEGINS with relabel[num_nodes], the position of node i among the selected nodes in ascending id order
 *   or -1 -- the rank of every kept edge among kept edges in ORIGINAL edge order and where each parent row starts in the subgraph
 *   on both sides.  counts: DEVICE int32[2] = {n_sub, e_sub}, which the caller reads to size the outputs of
 * kagnn_subgraph_fill: nodes[n_sub] int64 (ascending original ids), edge_ids[e_sub] int64 (ascending original edge ids),
 *   edge_index_sub[2, e_sub] int64 (relabelled, in original edge order), and (rowptr, col, perm) / (rowptr_t, col_t, perm_t) of the
 *   subgraph: bit for bit what kagnn_csr_build / kagnn_csr_build_small make from edge_index_sub -- a parent row with entries
 *   dropped is already in stable-sort order, so nothing is sorted.  No hub segments are produced.  n_sub / e_sub must be the count
 *   call's figures; with other figures the contents are meaningless, but nothing is written beyond n_sub + 1 row pointers, n_sub
 *   nodes and e_sub entries.  Arrays of zero length may be NULL.
 * Workspace of both calls (the same memory, untouched in between): kagnn_subgraph_workspace_bytes(num_nodes, num_edges). */
int kagnn_subgraph_workspace_bytes(int64_t num_nodes, int64_t num_edges, size_t* bytes_host);
int kagnn_k_hop_mark(const int32_t* rowptr, const int32_t* col, int64_t num_nodes, const int64_t* seeds, int64_t num_seeds,
                     int32_t num_hops, int32_t* hop, int32_t* flags, void* stream);
int kagnn_subgraph_count(const int32_t* hop, const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                         const int32_t* rowptr_t, const int32_t* col_t, const int32_t* perm_t, int64_t num_nodes, int64_t num_edges,
                         void* workspace, size_t workspace_bytes, int32_t* counts, void* stream);
int kagnn_subgraph_fill(const void* workspace, size_t workspace_bytes, const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                        const int32_t* rowptr_t, const int32_t* col_t, const int32_t* perm_t, int64_t num_nodes, int64_t num_edges,
                        int64_t n_sub, int64_t e_sub, int64_t* nodes, int64_t* edge_ids, int64_t* edge_index_sub,
                        int32_t* rowptr_sub, int32_t* col_sub, int32_t* perm_sub, int32_t* rowptr_t_sub, int32_t* col_t_sub,
                        int32_t* perm_t_sub, void* stream);

/* Fan-out-limited neighbour sampling (GraphSAGE; torch_geometric's NeighborLoader / NeighborSampler, directed, without
 * replacement; no counterpart in the reference, whose node-level scripts are full batch).  The same three calls and the same ONE
 * read-back as above, with an edge selection between the first and the second; all indices int32; no float, no atomic
 * read-modify-write on global memory; every result is a pure function of (graph, seeds as a SET, fanout, seed).
 *
 * kagnn_neighbor_sample_mark: (rowptr, col, perm) = the parent's by-destination CSR.  hop[num_nodes] is filled with -1 and
 *   keep[num_edges] (bytes) with 0; seeds get hop 0, a seed outside [0, num_nodes) sets the DEVICE int flags[0] = 1 (else 0) and is
 *   skipped.  Then one launch per level d = 0 .. num_levels - 1 (1 <= num_levels <= KAGNN_SAMPLE_MAX_LEVELS; fanout_host[d]: a HOST
 *   array, >= 0 a count, -1 all): every row with hop == d selects min(deg, fanout[d]) of its in-edges, sets keep[perm[p]] = 1 for
 *   them and stores d + 1 into hop[col[p]] where it still reads -1 -- a node is expanded once, at the level it is first reached.
 *   WHICH edges a row selects is part of this ABI: the k entries of the row with the smallest pair (key32(seed, e), e), e = perm[p]
 *   the ORIGINAL edge id, where with  mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16  (uint32
 *   arithmetic) and lo = (uint32)seed, hi = (uint32)(seed >> 32):
 *       h1 = mix32(lo + 0x9e3779b9),  h2 = mix32(hi ^ h1 ^ 0x85ebca6b),  key32(seed, e) = mix32(mix32((uint32)e ^ h1) + h2).
 *   The k smallest keys of a row are a uniform k-subset without replacement, independent across rows, and do not depend on the
 *   order of the seeds or on the launch geometry.  Rows of at most 64 entries rank one key per lane by comparison across the wave;
 *   longer rows find the k-th smallest key by a byte-digit radix select (256 bins per wave in LDS, four passes) and resolve ties
 *   at the threshold to the lowest edge ids -- nothing of a row is staged, so a row of any length works at any fan-out.  A fan-out
 *   >= deg takes the whole row without computing a key.
 * kagnn_edge_subgraph_count / kagnn_edge_subgraph_fill: kagnn_subgraph_count / kagnn_subgraph_fill for the subgraph given by an
 *   EDGE selection: the nodes are hop[i] >= 0, the edges exactly keep[e] != 0, in original edge order.  By contract both endpoints
 *   of a kept edge are selected (the mark call's output is such a pair); an edge whose endpoint is not is dropped from the rows, and
 *   every store stays guarded by relabel, n_sub and e_sub as above.  Same outputs, same workspace (size query, layout -- it BEGINS
 *   with relabel[num_nodes] -- and the single read of counts); the by-source side is compacted from (rowptr_t, col_t, perm_t) with
 *   keep[perm_t[p]], so perm_t IS read by the count call here.  keep must be the same array in both calls. */
#define KAGNN_SAMPLE_MAX_LEVELS 16
int kagnn_neighbor_sample_mark(const int32_t* rowptr, const int32_t* col, const int32_t* perm, int64_t num_nodes, int64_t num_edges,
                               const int64_t* seeds, int64_t num_seeds, const int32_t* fanout_host, int32_t num_levels, uint64_t seed,
                               int32_t* hop, uint8_t* keep, int32_t* flags, void* stream);
int kagnn_edge_subgraph_count(const int32_t* hop, const uint8_t* keep, const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                              const int32_t* rowptr_t, const int32_t* col_t, const int32_t* perm_t, int64_t num_nodes,
                              int64_t num_edges, void* workspace, size_t workspace_bytes, int32_t* counts, void* stream);
int kagnn_edge_subgraph_fill(const void* workspace, size_t workspace_bytes, const uint8_t* keep, const int32_t* rowptr,
                             const int32_t* col, const int32_t* perm, const int32_t* rowptr_t, const int32_t* col_t,
                             const int32_t* perm_t, int64_t num_nodes, int64_t num_edges, int64_t n_sub, int64_t e_sub, int64_t* nodes,
                             int64_t* edge_ids, int64_t* edge_index_sub, int32_t* rowptr_sub, int32_t* col_sub, int32_t* perm_sub,
                             int32_t* rowptr_t_sub, int32_t* col_t_sub, int32_t* perm_t_sub, void* stream);

/* Link prediction around an encoder (torch_geometric's recipe: RandomLinkSplit, uniform negative_sampling, a dot-product decoder,
 * BCEWithLogitsLoss, ROC-AUC; no counterpart in the reference snapshot, which has no link-prediction script).  The decoder needs no
 * entry point of its own: the score <z[u], z[v]> of every pair is kagnn_aggregate_edge_grad with x = gout = z over the pair list's
 * by-destination structure, its gradient kagnn_aggregate_sum + kagnn_aggregate_sum_add with the upstream gradient as edge weights.
 * Every result below is a pure function of its inputs -- no float atomics, two calls return the same bits -- and nothing
 * synchronises the stream.  Indices the caller sees are int64.
 *
 * kagnn_edge_keys_build: the edge set of (src, dst) = edge_index[0], edge_index[1] as keys[0 .. *num_keys) = the ascending,
 *   duplicate-free values src * num_nodes + dst (int64; a rocPRIM radix sort and a unique pass); `keys` holds num_edges elements,
 *   num_keys is a DEVICE word.  Ids outside [0, num_nodes) are clamped to 0.  num_edges == 0: only *num_keys = 0 is written.
 *   Workspace: kagnn_edge_keys_workspace_bytes(num_edges).
 * kagnn_negative_sample: `num` slots of uniform negative pairs.  Slot p tries the attempts t = 0 .. attempts - 1 with the counter
 *   c = p * attempts + t:  u = ((uint64)key32(seed, 2c) * num_nodes) >> 32,  v = ((uint64)key32(seed, 2c + 1) * num_nodes) >> 32
 *   (key32: kagnn_neighbor_sample_mark above).  An attempt is valid iff u != v and u * num_nodes + v is not among keys[0 .. num_keys)
 *   (a binary search); the slot takes its FIRST valid attempt: pairs[p] = u, pairs[num + p] = v, valid[p] = 1.  A slot without one
 *   is EMPTY: the pair (0, 0) and valid[p] = 0.  pairs: int64 [2, num]; valid: bytes [num]; a fixed size, so nothing is compacted
 *   or read back.  Refused before any launch: attempts outside 1..KAGNN_NEGATIVE_MAX_ATTEMPTS, 2 * num * attempts >= 2^32,
 *   num_nodes >= 2^31.  num == 0 or num_nodes == 0: nothing is launched.
 * kagnn_bce_logits_fwd: F.binary_cross_entropy_with_logits over the rows of weight 1 (weight NULL: all): loss[0] = the mean of
 *   max(s, 0) - s y + log1p(exp(-|s|)), y = (labels[p] != 0), the term in fp32, the sum in fp64 partials added in a fixed order
 *   (a thread's rows ascending, a fixed tree, the workgroups in index order), divided by divisor[0] = max(rows, 1) -- a DEVICE
 *   int64 the backward reads -- and rounded once.  `record` (NULL: none): one row of kagnn_node_eval's format, WRITTEN in the same
 *   call: {double loss sum; int64 rows with (s > 0) == y; int64 rows}.  A NaN score makes the sum NaN and counts like any other
 *   score.  Up to 4096 rows: one launch, no workspace; above: KAGNN_BCE_WORKSPACE_BYTES of 8-byte aligned workspace.
 * kagnn_bce_logits_bwd: g_scores[p] = (sigmoid(s) - y) * g_loss[0] / divisor[0] on rows of weight 1, exactly 0 elsewhere.
 * kagnn_link_rank: record = int64[8] = {2U, n_pos, n_neg, nan_rows, hits[k0], hits[k1], hits[k2], 0} over the rows of weight 1
 *   whose score is not NaN (those are counted in nan_rows):  2U = sum over positives i and negatives j of (2 if s_i > s_j, 1 if
 *   s_i == s_j), so ROC-AUC = 2U / (2 n_pos n_neg);  hits[k] = the positives STRICTLY above the k-th largest negative score (all
 *   of them when there are fewer than k negatives; 0 for the k's not given).  -0.0 and +0.0 tie, +-Inf are ordinary values.  Exact:
 *   an order-preserving 32-bit key per score, one radix sort with the label as value, an exclusive scan of the negatives, two
 *   binary searches per positive, int64 sums (integer atomics).  ks_host: a HOST array of num_ks <= 3 values >= 1.  Workspace:
 *   kagnn_link_rank_workspace_bytes(num_rows). */
#define KAGNN_NEGATIVE_MAX_ATTEMPTS 32
#define KAGNN_BCE_WORKSPACE_BYTES 6144
int kagnn_edge_keys_workspace_bytes(int64_t num_edges, size_t* bytes_host);
int kagnn_edge_keys_build(const int64_t* src, const int64_t* dst, int64_t num_edges, int64_t num_nodes, int64_t* keys,
                          int64_t* num_keys, void* workspace, size_t workspace_bytes, void* stream);
int kagnn_negative_sample(const int64_t* keys, int64_t num_keys, int64_t num_nodes, int64_t num, uint64_t seed, int32_t attempts,
                          int64_t* pairs, uint8_t* valid, void* stream);
int kagnn_bce_logits_fwd(const float* scores, const uint8_t* labels, const uint8_t* weight, int64_t num_rows, float* loss,
                         int64_t* divisor, void* record, void* workspace, size_t workspace_bytes, void* stream);
int kagnn_bce_logits_bwd(const float* scores, const uint8_t* labels, const uint8_t* weight, int64_t num_rows, const int64_t* divisor,
                         const float* g_loss, float* g_scores, void* stream);
int kagnn_link_rank_workspace_bytes(int64_t num_rows, size_t* bytes_host);
int kagnn_link_rank(const float* scores, const uint8_t* labels, const uint8_t* weight, int64_t num_rows, const int32_t* ks_host,
                    int32_t num_ks, int64_t* record, void* workspace, size_t workspace_bytes, void* stream);

/* in-degree normalisation of GCN (torch_geometric gcn_norm as used by KAGCNConv,
 * node_classification_clean/models.py:31-37): dis[i] = (1 + #non-loop in-edges of i)^-1/2.
 * `rowptr/col` must be the by-destination CSR of the ORIGINAL edge list. */
int kagnn_gcn_deg_inv_sqrt(const int32_t* rowptr, const int32_t* col, int64_t num_nodes,
                           float* dis, void* stream);

/* ------------------------------------------------------------------------------------------
 * Neighbour aggregation (sum).  Replaces x.index_select(0,row) -> scatter_add_(0,col) of
 * MessagePassing.propagate:
 *
 *   out[i,:] = out_scale[i] * ( self_scale * s(i) * x[i,:] + sum_{e in row i} w(e) * s(col[e]) * x[col[e],:] ) + bias[:]
 *
 * with s(j) = in_scale[j] (or 1 when NULL), w(e) = edge_weight[e] in CSR order (or 1 when NULL),
 * out_scale NULL = 1, bias NULL = 0.  `skip_self_loops` != 0 drops edges with col[e]==i (GCN's
 * add_remaining_self_loops).  GIN: self_scale = 1+eps, everything else NULL.  GCN: in_scale =
 * out_scale = dis, self_scale = 1, skip_self_loops = 1, bias = conv bias.  The backward of an
 * aggregation is the same call on the transposed CSR.
 * Deterministic (bit-reproducible run to run): rows listed in hub_seg are summed per segment into
 * `workspace` (kagnn_aggregate_workspace_bytes(num_hub_seg, num_feat) bytes; may be NULL when num_hub_seg
 * is 0) and folded into the row in segment order -- no atomics anywhere.
 * ------------------------------------------------------------------------------------------ */
int kagnn_aggregate_workspace_bytes(int64_t num_hub_seg, int32_t num_feat, size_t* bytes_host);
int kagnn_aggregate_sum(const float* x, int64_t ldx, float* out, int64_t ldo,
                        const int32_t* rowptr, const int32_t* col, const float* edge_weight,
                        int64_t num_nodes, int32_t num_feat, float self_scale,
                        const float* in_scale, const float* out_scale, const float* bias,
                        int32_t skip_self_loops,
                        const int32_t* hub_seg, int64_t num_hub_seg, int32_t hub_threshold,
                        void* workspace, size_t workspace_bytes, void* stream);
/* out = <the aggregation above> + addend (fp32 [num_nodes, num_feat], leading dimension ld_addend; NULL = none), added
 * last, in the kernel's epilogue: where the tape would otherwise sum two gradients of one activation in a pass of its own
 * (the skip-concat models: the read-out's gradient of h_l and the next convolution's -- reference
 * node_classification_clean/models.py:196-202).  Bit-identical to kagnn_aggregate_sum followed by the addition.        */
int kagnn_aggregate_sum_add(const float* x, int64_t ldx, float* out, int64_t ldo,
                            const int32_t* rowptr, const int32_t* col, const float* edge_weight,
                            int64_t num_nodes, int32_t num_feat, float self_scale,
                            const float* in_scale, const float* out_scale, const float* bias,
                            int32_t skip_self_loops,
                            const int32_t* hub_seg, int64_t num_hub_seg, int32_t hub_threshold,
                            const float* addend, int64_t ld_addend,
                            void* workspace, size_t workspace_bytes, void* stream);

/* Gradient of that aggregation with respect to its EDGE WEIGHTS (torch_geometric's GCNConv differentiates through `edge_weight`;
 * GNNExplainer's edge mask, learned edge weights): for every CSR position e of row i, j = col[e],
 *
 *   g_edge_weight[perm ? perm[e] : e] = out_scale[i] * s(j) * < gout[i, :num_feat], x[j, :num_feat] >
 *
 * exactly 0 where `skip_self_loops` and j == i; NULL scales = 1.  `x` is the matrix the forward gathered, `gout` the gradient of
 * its result, `rowptr / col / perm / hub_seg` the by-destination structure of kagnn_csr_build (`perm` NULL: CSR order).  fp32,
 * every width and leading dimension kagnn_aggregate_sum takes (float4 rows where num_feat % 4 == 0, num_feat <= 256 and both
 * operands are 16-byte aligned with leading dimensions % 4 == 0; a scalar kernel otherwise).  `perm` is a permutation, so every
 * output element is written once: no atomics, no workspace, a fixed reduction order -- bit-reproducible run to run.  Rows above
 * `hub_threshold` edges run through their hub segments (one workgroup each).  num_nodes == 0 or num_edges == 0: nothing is
 * launched.                                                                                                                    */
int kagnn_aggregate_edge_grad(const float* x, int64_t ldx, const float* gout, int64_t ldg,
                              const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                              int64_t num_nodes, int64_t num_edges, int32_t num_feat,
                              const float* in_scale, const float* out_scale, int32_t skip_self_loops,
                              const int32_t* hub_seg, int64_t num_hub_seg, int32_t hub_threshold,
                              float* g_edge_weight, void* stream);

/* The same aggregation with bf16 GATHER OPERANDS (`KAGNN_ACT=bf16`; BASELINE.json config 2 -- the reference has no
 * reduced-precision path, SURVEY.md 8(d) makes this a build-defined mode): `x` rows are bf16 (leading dimension in
 * ELEMENTS, a multiple of 8; 16-byte aligned), sums are accumulated in fp32 and written as fp32 (`out_dtype` =
 * KAGNN_DTYPE_F32: the forward, feeding the KAN layer) or bf16 with ONE round-to-nearest-even per element
 * (KAGNN_DTYPE_BF16: the input gradient of a bf16 activation).  Halves the E * num_feat * 4 bytes of the gather.
 * num_feat % 8 == 0, <= 512 (else KAGNN_ERR_UNSUPPORTED: convert to fp32 and call kagnn_aggregate_sum).
 * Deterministic; workspace as for kagnn_aggregate_sum.  kagnn_rows_to_bf16 converts fp32 rows (RNE). */
int kagnn_aggregate_sum_bf16(const void* x, int64_t ldx, void* out, int64_t ldo, int32_t out_dtype,
                             const int32_t* rowptr, const int32_t* col, const float* edge_weight,
                             int64_t num_nodes, int32_t num_feat, float self_scale,
                             const float* in_scale, const float* out_scale, const float* bias,
                             int32_t skip_self_loops,
                             const int32_t* hub_seg, int64_t num_hub_seg, int32_t hub_threshold,
                             void* workspace, size_t workspace_bytes, void* stream);
int kagnn_rows_to_bf16(const float* x, int64_t ldx, void* y, int64_t ldy, int64_t num_rows, int32_t num_feat,
                       void* stream);

/* GINE message: out[i,:] = self_scale*x[i,:] + sum_e relu(x[col[e],:] + edge_attr[perm[e],:])
 * (torch_geometric GINEConv as used by graph_regression/models.py:98,113).              */
int kagnn_aggregate_gine(const float* x, int64_t ldx, const float* edge_attr, int64_t lde,
                         float* out, int64_t ldo, const int32_t* rowptr, const int32_t* col,
                         const int32_t* perm, int64_t num_nodes, int32_t num_feat,
                         float self_scale, void* stream);
/* backward of the GINE message, run on the TRANSPOSED structure (rows = source nodes j, built
 * with key=src,val=dst): for e in row j with target i = col_t[e] and original edge id
 * pe = perm_t[e]:  g = gout[i,:] * (x[j,:] + edge_attr[pe,:] > 0);  g_edge_attr[pe,:] = g;
 * gx[j,:] = self_scale*gout[j,:] + sum_e g.  Deterministic (no atomics); g_edge_attr may be NULL. */
int kagnn_aggregate_gine_bwd(const float* x, int64_t ldx, const float* edge_attr, int64_t lde,
                             const float* gout, int64_t ldg, float* gx, int64_t ldgx,
                             float* g_edge_attr, int64_t ldge,
                             const int32_t* rowptr_t, const int32_t* col_t, const int32_t* perm_t,
                             int64_t num_nodes, int32_t num_feat, float self_scale, void* stream);

/* segmented sum over a SORTED batch vector given as segment offsets (global_add_pool,
 * graph_regression/models.py:117): out[b,:] = sum_{i in [seg[b],seg[b+1])} x[i,:];
 * `mean` != 0 divides by max(count,1) (global_mean_pool).  Backward = kagnn_segment_broadcast. */
int kagnn_segment_pool(const float* x, int64_t ldx, float* out, int64_t ldo,
                       const int32_t* seg_ptr, int64_t num_segments, int32_t num_feat,
                       int32_t mean, void* stream);
int kagnn_segment_broadcast(const float* gout, int64_t ldg, float* gx, int64_t ldgx,
                            const int32_t* seg_ptr, int64_t num_segments, int32_t num_feat,
                            int32_t mean, void* stream);

/* ------------------------------------------------------------------------------------------
 * efficient-KAN layer.  Replaces KANLinear.forward (node_classification_clean/ekan.py:154-162:
 * b_splines :79-112 + scaled_spline_weight :146-152 + two F.linear) and its autograd backward.
 * The [N, in, G+k] basis tensor is never materialised.
 *
 *  knots        : ONE row of the module's `grid` buffer, G+2k+1 fp32 values (uniform grid; the host
 *                 side verifies all rows equal and uniform) -- or, with mode KAGNN_PREC_FP32_GRID,
 *                 the whole buffer [in, G+2k+1] with increasing, possibly non-uniform rows
 *  base_weight  [out,in] or NULL (no SiLU branch), spline_weight [out,in,G+k], spline_scaler [out,in] or NULL
 *
 * kagnn_kan_pack rearranges (base_weight | spline_weight*scaler) into the MFMA fragment order
 * used by fwd (`pack_fwd`) and by the input-gradient kernel (`pack_dx`); call it whenever the
 * parameters change.  Sizes from kagnn_kan_pack_bytes.
 *
 * spline_order 1..4 in every mode; 5..KAGNN_MAX_SPLINE_ORDER with KAGNN_PREC_FP32 / KAGNN_PREC_FP32_GRID (the pack, the
 * forward, both gradients and their workspace queries below; the same fp32 packs and the same ordered fp32 fma chain).
 * ------------------------------------------------------------------------------------------ */
int kagnn_kan_pack_bytes(int32_t in_features, int32_t out_features, int32_t grid_size,
                         int32_t spline_order, int32_t mode, size_t* fwd_bytes_host,
                         size_t* dx_bytes_host);
int kagnn_kan_pack(const float* base_weight, const float* spline_weight,
                   const float* spline_scaler, int32_t in_features, int32_t out_features,
                   int32_t grid_size, int32_t spline_order, int32_t mode,
                   void* pack_fwd, void* pack_dx, void* stream);

/* kagnn_kan_pack for the layers of a chain (<= 8, same grid_size / spline_order / mode) in ONE launch -- a pack
 * launch is ~20 us of latency, not work.  Arrays of n_layers HOST-side entries (device pointers / sizes); `sc` may
 * be NULL (no scalers) or hold NULL entries.  KAGNN_ERR_UNSUPPORTED unless every layer takes the sparse-forward /
 * split-precision path with out_features <= 64 (the caller then packs layer by layer).                          */
int kagnn_kan_pack_batch(int32_t n_layers, const float* const* base_weight, const float* const* spline_weight,
                         const float* const* spline_scaler, const int32_t* in_features,
                         const int32_t* out_features, int32_t grid_size, int32_t spline_order, int32_t mode,
                         void* const* pack_fwd, void* const* pack_dx, void* stream);

/* y[N,out] = silu(x) @ base_weight^T + bases(x) @ (spline_weight*scaler)^T.
 * Inputs with few rows and many features (Cora: 2708 x 1433) split the feature loop over more
 * workgroups and sum per-split partial outputs in a fixed order; that needs a scratch buffer of
 * kagnn_kan_fwd_workspace_bytes() bytes (0 for tall inputs: workspace may then be NULL).        */
int kagnn_kan_fwd_workspace_bytes(int64_t num_rows, int32_t in_features, int32_t out_features,
                                  int32_t grid_size, int32_t spline_order, int32_t mode,
                                  size_t* bytes_host);
int kagnn_kan_linear_fwd(const float* x, int64_t ldx, int64_t num_rows, const float* knots,
                         int32_t in_features, int32_t out_features, int32_t grid_size,
                         int32_t spline_order, int32_t mode, const void* pack_fwd,
                         float* y, int64_t ldy, void* workspace, size_t workspace_bytes,
                         void* stream);

/* The same forward on an input given as COLUMN BLOCKS [x_0 | x_1 | ...] held in different buffers: replaces `self.lay_out(torch.cat(l, dim=1))` of the node models (reference
 * node_classification_clean/models.py:202-203, 256-257) without building the concatenation -- one launch, y written once.
 * x_parts / part_widths / part_ld are HOST arrays of num_parts device pointers / widths / leading dimensions; pack_fwd is
 * the pack of the whole layer (in_features = sum of the widths).  Covered: cubic layers of <= 8 coefficients in the split
 * mode, every block a multiple of 64 columns, <= 512 columns in all, 16-byte aligned rows (leading dimensions: multiples
 * of 4, <= 7680); kagnn_kan_fwd_parts_ok() says (1 / 0) whether a shape is.
 * Anything else returns KAGNN_ERR_UNSUPPORTED (concatenate and call kagnn_kan_linear_fwd).                          */
int kagnn_kan_fwd_parts_ok(const int32_t* part_widths, int32_t num_parts, int32_t in_features, int32_t out_features,
                           int32_t grid_size, int32_t spline_order, int32_t mode);
int kagnn_kan_linear_fwd_parts(const float* const* x_parts, const int32_t* part_widths, const int64_t* part_ld,
                               int32_t num_parts, int64_t num_rows, const float* knots, int32_t in_features, int32_t out_features,
                               int32_t grid_size, int32_t spline_order, int32_t mode, const void* pack_fwd,
                               float* y, int64_t ldy, void* workspace, size_t workspace_bytes, void* stream);

/* The same forward, which also leaves the COLUMN MOMENTS of y in col_mean[out] (mean over the rows) and
 * col_m2[out] (sum of squared deviations from it): the batch statistics of the BatchNorm1d that follows every
 * convolution (node_classification_clean/models.py:198-200), handed to kagnn_batchnorm_fwd so that it needs no
 * statistics pass over y.  Cubic-spline split-precision layers accumulate them in the forward kernel's epilogue
 * (per wave over its row tiles, merged in a fixed order by the pairwise update of Chan et al.: deterministic, no
 * cancellation); every other layer shape runs the plain forward and one column pass.  num_rows >= 1; the workspace
 * (kagnn_kan_fwd_moments_workspace_bytes) is required.                                                          */
int kagnn_kan_fwd_moments_workspace_bytes(int64_t num_rows, int32_t in_features, int32_t out_features,
                                          int32_t grid_size, int32_t spline_order, int32_t mode,
                                          size_t* bytes_host);
int kagnn_kan_linear_fwd_moments(const float* x, int64_t ldx, int64_t num_rows, const float* knots,
                                 int32_t in_features, int32_t out_features, int32_t grid_size,
                                 int32_t spline_order, int32_t mode, const void* pack_fwd,
                                 float* y, int64_t ldy, float* col_mean, float* col_m2,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* gx[N,in] = d loss / d x given gy[N,out] (x is the saved layer input; bases' derivatives are
 * recomputed, nothing but x was saved).  spline_order as kagnn_kan_linear_fwd (5..16: exact-fp32 modes, fp32 rows).  gx_dtype = KAGNN_DTYPE_F32, or KAGNN_DTYPE_BF16 (split-precision
 * B-spline layers with <= 128 outputs: the rows the transposed aggregation gathers next, rounded once) with
 * ldgx in bf16 elements.                                                                    */
int kagnn_kan_linear_bwd_input(const float* x, int64_t ldx, const float* gy, int64_t ldgy,
                               int64_t num_rows, const float* knots, int32_t in_features,
                               int32_t out_features, int32_t grid_size, int32_t spline_order,
                               int32_t mode, const void* pack_dx, void* gx, int64_t ldgx,
                               int32_t gx_dtype, void* stream);

/* parameter gradients: g_base_weight[out,in] (NULL when not wanted), g_spline_weight[out,in,G+k],
 * g_spline_scaler[out,in] (NULL when the layer has no scaler).  `workspace` holds the per-wave
 * partial sums (size from kagnn_kan_bwd_weight_workspace_bytes); deterministic reduction.
 * spline_order as kagnn_kan_linear_fwd (5..16: exact-fp32 modes).                           */
int kagnn_kan_bwd_weight_workspace_bytes(int64_t num_rows, int32_t in_features,
                                         int32_t out_features, int32_t grid_size,
                                         int32_t spline_order, int32_t mode, size_t* bytes_host);
int kagnn_kan_linear_bwd_weight(const float* x, int64_t ldx, const float* gy, int64_t ldgy,
                                int64_t num_rows, const float* knots, int32_t in_features,
                                int32_t out_features, int32_t grid_size, int32_t spline_order,
                                int32_t mode, const float* spline_weight,
                                const float* spline_scaler, float* g_base_weight,
                                float* g_spline_weight, float* g_spline_scaler,
                                void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * One KAN-GIN convolution per call -- GIKANLayer.forward (node_classification_clean/models.py:48-56: GINConv around
 * make_kan's KAN chain, ekan.py:270-275) and its backward; the `gin_kan_fused_fwd / _bwd` of SURVEY.md 8(b).  The call
 * sequences the library's own kernels on `stream` (aggregation, ONE weight-pack launch for the chain, the KANLinear
 * forwards; on the way back per layer the weight and input gradients, then the transposed aggregation); the caller owns
 * every buffer:
 *   widths[L+1]        layer widths: in_features of layer 0 ... out_features of layer L-1 (L <= 8, same grid / order / mode)
 *   acts[L+1]          fp32 [N, widths[l]]: acts[0] receives the aggregate h0, acts[l+1] the output of layer l (acts[L] = y);
 *                      the backward reads acts[0..L-1] (the only saved tensors) -- contiguous, ld = width
 *   pack_fwd/pack_dx   per layer, sized by kagnn_kan_pack_bytes; written by _fwd, pack_dx read by _bwd
 *   x                  [N, widths[0]] fp32 or bf16 (x_dtype; bf16 = the gather-operand mode of kagnn_aggregate_sum_bf16)
 *   _bwd: gx           d loss / d x in gx_dtype, or NULL; `bf16_gather` != 0 lets the first layer's input-gradient kernel
 *                      write d loss / d h0 as bf16 rows for the transposed aggregation (split precision, cubic, <= 8
 *                      coefficients; otherwise it stays fp32); g_base_weight / g_spline_weight / g_spline_scaler per layer
 *   (rowptr, col, hub_seg): by destination for _fwd, the transposed (by source) structure for _bwd
 *   _fwd: col_mean / col_m2  [widths[L]] each or both NULL: the column moments of y for the BatchNorm1d that follows
 *                      (kagnn_kan_linear_fwd_moments; hand them to kagnn_batchnorm_fwd)
 * Workspace sizes from kagnn_gin_kan_layer_workspace_bytes (hub-segment counts of the two directions).  Deterministic.
 * ------------------------------------------------------------------------------------------ */
int kagnn_gin_kan_layer_workspace_bytes(int64_t num_nodes, int32_t num_layers, const int32_t* widths,
                                        int32_t grid_size, int32_t spline_order, int32_t mode,
                                        int64_t num_hub_seg, int64_t num_hub_seg_t,
                                        size_t* fwd_bytes_host, size_t* bwd_bytes_host);
int kagnn_gin_kan_layer_fwd(const void* x, int32_t x_dtype, int64_t ldx, int64_t num_nodes,
                            const int32_t* rowptr, const int32_t* col, const int32_t* hub_seg,
                            int64_t num_hub_seg, int32_t hub_threshold, float self_scale,
                            int32_t num_layers, const int32_t* widths, const float* const* base_weight,
                            const float* const* spline_weight, const float* const* spline_scaler,
                            const float* knots, int32_t grid_size, int32_t spline_order, int32_t mode,
                            float* const* acts, void* const* pack_fwd, void* const* pack_dx,
                            float* col_mean, float* col_m2,
                            void* workspace, size_t workspace_bytes, void* stream);
int kagnn_gin_kan_layer_bwd(const float* gy, int64_t ldgy, int64_t num_nodes, const int32_t* rowptr_t,
                            const int32_t* col_t, const int32_t* hub_seg_t, int64_t num_hub_seg_t,
                            int32_t hub_threshold, float self_scale, int32_t num_layers, const int32_t* widths,
                            const float* const* spline_weight, const float* const* spline_scaler,
                            const float* knots, int32_t grid_size, int32_t spline_order, int32_t mode,
                            const float* const* acts, const void* const* pack_dx, void* gx, int32_t gx_dtype,
                            int64_t ldgx, int32_t bf16_gather, float* const* g_base_weight,
                            float* const* g_spline_weight, float* const* g_spline_scaler,
                            void* workspace, size_t workspace_bytes, void* stream);
/* the same backward with gx = <input gradient> + gx_addend (fp32 [num_nodes, widths[0]]; needs an fp32 gx and
 * bf16_gather == 0): the addition rides in the transposed aggregation's epilogue (kagnn_aggregate_sum_add)            */
int kagnn_gin_kan_layer_bwd_add(const float* gy, int64_t ldgy, int64_t num_nodes, const int32_t* rowptr_t,
                                const int32_t* col_t, const int32_t* hub_seg_t, int64_t num_hub_seg_t,
                                int32_t hub_threshold, float self_scale, int32_t num_layers, const int32_t* widths,
                                const float* const* spline_weight, const float* const* spline_scaler,
                                const float* knots, int32_t grid_size, int32_t spline_order, int32_t mode,
                                const float* const* acts, const void* const* pack_dx, void* gx, int32_t gx_dtype,
                                int64_t ldgx, int32_t bf16_gather, const float* gx_addend, int64_t ld_addend,
                                float* const* g_base_weight, float* const* g_spline_weight,
                                float* const* g_spline_scaler, void* workspace, size_t workspace_bytes, void* stream);

/* The backward of  BatchNorm1d(KAN(aggregate(x)))  in TRAINING mode -- a convolution plus the norm that follows it in every
 * node model (reference node_classification_clean/models.py:198-200) -- given g = d loss / d (norm output) [N, widths[L]]:
 * the norm's statistics pass (column sums -> g_bn_weight, g_bn_bias; either may be NULL), then the chain's backward with the
 * norm's element-wise backward applied INSIDE the last layer's input-gradient kernel (cubic layers of <= 8 coefficients with
 * 32 / 64 outputs; other shapes run the stand-alone pass), then the transposed aggregation (+ gx_addend).  y = the norm's
 * input (= the chain's output), bn_mean / bn_rstd = the batch statistics kagnn_batchnorm_fwd saved, bn_weight NULL = no
 * affine.  Workspace: the backward size of kagnn_gin_kan_layer_workspace_bytes PLUS
 * kagnn_gin_kan_layer_bwd_bn_workspace_bytes(num_nodes, widths[L]).  Needs num_nodes >= 2.                             */
int kagnn_gin_kan_layer_bwd_bn_workspace_bytes(int64_t num_nodes, int32_t out_features, size_t* bytes_host);
int kagnn_gin_kan_layer_bwd_bn(const float* g, int64_t ldg, const float* y, int64_t ldy, const float* bn_weight,
                               const float* bn_mean, const float* bn_rstd, float* g_bn_weight, float* g_bn_bias,
                               int64_t num_nodes, const int32_t* rowptr_t, const int32_t* col_t,
                               const int32_t* hub_seg_t, int64_t num_hub_seg_t, int32_t hub_threshold, float self_scale,
                               int32_t num_layers, const int32_t* widths, const float* const* spline_weight,
                               const float* const* spline_scaler, const float* knots, int32_t grid_size,
                               int32_t spline_order, int32_t mode, const float* const* acts,
                               const void* const* pack_dx, void* gx, int32_t gx_dtype, int64_t ldgx, int32_t bf16_gather,
                               const float* gx_addend, int64_t ld_addend, float* const* g_base_weight,
                               float* const* g_spline_weight, float* const* g_spline_scaler, void* workspace,
                               size_t workspace_bytes, void* stream);

/* kagnn_gin_kan_layer_bwd_bn with the norms' backward STATISTICS travelling with the gradients (round 4; reference
 * node_classification_clean/models.py:198-200 -- in the node models the gradient g arriving at layer l's norm is what layer
 * l+1's transposed aggregation produces, plus the skip gradient added there):
 *   prev_y [N, widths[0]] (ld_prev_y), prev_mean, prev_rstd, prev_sums -- all four or none: this call's transposed aggregation
 *     ALSO leaves prev_sums[0][widths[0]] = sum_n gx, prev_sums[1][widths[0]] = sum_n gx * xhat, xhat = (prev_y - prev_mean) *
 *     prev_rstd, where prev_y is the PREVIOUS norm's input (this convolution's input before the folded affine): the two column
 *     sums that norm's backward starts from.  Partial sums in the row kernel's epilogue (one row pair per workgroup, hub rows
 *     from the merge kernel), folded in a fixed order: deterministic.  Needs an fp32 gx, 17..256 input features (a multiple of
 *     4), 16-byte aligned rows; otherwise KAGNN_ERR_UNSUPPORTED.
 *   bn_sums [2][widths[L]] or NULL: the same two sums for THIS norm, made by the next layer's call -- the statistics pass over
 *     g and y is skipped when the norm's element-wise backward runs inside the input-gradient kernel (ignored otherwise).
 * Workspace: kagnn_gin_kan_layer_bwd_bn's, plus kagnn_gin_kan_layer_bwd_bn_sums_workspace_bytes when prev_sums is given.  */
int kagnn_gin_kan_layer_bwd_bn_sums_workspace_bytes(int64_t num_nodes, int32_t in_features, int64_t num_hub_seg_t,
                                                    size_t* bytes_host);
int kagnn_gin_kan_layer_bwd_bn_sums(const float* g, int64_t ldg, const float* y, int64_t ldy, const float* bn_weight,
                                    const float* bn_mean, const float* bn_rstd, float* g_bn_weight, float* g_bn_bias,
                                    const float* bn_sums,
                                    const float* prev_y, int64_t ld_prev_y, const float* prev_mean, const float* prev_rstd,
                                    float* prev_sums,
                                    int64_t num_nodes, const int32_t* rowptr_t, const int32_t* col_t,
                                    const int32_t* hub_seg_t, int64_t num_hub_seg_t, int32_t hub_threshold, float self_scale,
                                    int32_t num_layers, const int32_t* widths, const float* const* spline_weight,
                                    const float* const* spline_scaler, const float* knots, int32_t grid_size,
                                    int32_t spline_order, int32_t mode, const float* const* acts,
                                    const void* const* pack_dx, void* gx, int32_t gx_dtype, int64_t ldgx, int32_t bf16_gather,
                                    const float* gx_addend, int64_t ld_addend, float* const* g_base_weight,
                                    float* const* g_spline_weight, float* const* g_spline_scaler, void* workspace,
                                    size_t workspace_bytes, void* stream);

/* Embedding-table encoders of the graph-level models (reference graph_regression/models.py:244-281, AtomEncoder / BondEncoder:
 * out = sum over the integer feature columns of one table lookup each), one launch per column each way:
 *   fwd: out[i, :] (+)= table[index[i * index_stride], :]      (accumulate != 0: add to out -- the 2nd, 3rd, ... column)
 *   bwd: g_table[v, :] = sum_{i : index[i * index_stride] == v} g[i, :]   rows in order inside blocks of 128, blocks in order:
 *        deterministic (no atomics)
 * index: int64 (a column of the [N, columns] feature matrix: index_stride = columns); table / g_table: [V, F] contiguous.  An index
 * outside [0, V) -- a device-side assert in torch.nn.functional.embedding -- gives a NaN row in fwd and is skipped in bwd.          */
int kagnn_embedding_fwd(const int64_t* index, int64_t index_stride, int64_t num_rows, const float* table, int32_t num_embeddings,
                        int32_t num_feat, float* out, int64_t ldo, int32_t accumulate, void* stream);
int kagnn_embedding_bwd_workspace_bytes(int64_t num_rows, int32_t num_embeddings, int32_t num_feat, size_t* bytes_host);
int kagnn_embedding_bwd(const int64_t* index, int64_t index_stride, int64_t num_rows, const float* g, int64_t ldg,
                        int32_t num_embeddings, int32_t num_feat, float* g_table, void* workspace, size_t workspace_bytes,
                        void* stream);      /* num_embeddings <= 512; two launches: per-row-block partial tables, then their sum in block order */

/* ---- one library call per GINE convolution each way (round 5; BASELINE config 4 -- the ZINC-shaped mini-batch step is launch- and
 * host-bound).  Replaces: torch_geometric GINEConv around ekan.KAN + the BatchNorm1d that follows it, reference
 * graph_regression/models.py:98,107-119 (called per mini-batch from optuna_zinc.py:56-66).
 * Forward:  acts[0] = self_scale * x_i + sum_{j->i} relu(x_j + edge_attr[perm[e]]) (kagnn_aggregate_gine), ONE pack launch for the
 *   chain, the chain's KANLinear forwards into acts[1..L]; col_mean / col_m2 (both or NULL): the column moments of acts[L] from the
 *   last kernel's epilogue, for kagnn_batchnorm_fwd(col_mean, col_m2).
 * Backward: g = gradient of the chain's output -- or, with bn_y != NULL, of the training-mode BatchNorm1d that follows (bn_y = the
 *   norm's input = acts[L], bn_mean / bn_rstd as saved by its forward; g_bn_weight / g_bn_bias receive its parameter gradients):
 *   statistics pass, then the norm's element-wise backward inside the last layer's input-gradient kernel where the shape allows it
 *   (kagnn_gin_kan_layer_bwd_bn), dW / dX per layer, then kagnn_aggregate_gine_bwd on the TRANSPOSED structure: gx [N, widths[0]]
 *   (required) and g_edge_attr [E, widths[0]] in original edge order (may be NULL).
 * Same kernels and summation orders as the per-operation entry points: bit-identical results.  fp32 rows, no hub segments (mini-batches
 * of small graphs).  Workspace: kagnn_gin_kan_layer_workspace_bytes(..., num_hub_seg = 0, num_hub_seg_t = 0) forward / backward sizes,
 * the backward plus kagnn_gin_kan_layer_bwd_bn_workspace_bytes(num_nodes, widths[L]) when bn_y is given.                              */
int kagnn_gine_kan_layer_fwd(const float* x, int64_t ldx, const float* edge_attr, int64_t lde, int64_t num_nodes,
                             const int32_t* rowptr, const int32_t* col, const int32_t* perm, float self_scale,
                             int32_t num_layers, const int32_t* widths, const float* const* base_weight,
                             const float* const* spline_weight, const float* const* spline_scaler, const float* knots,
                             int32_t grid_size, int32_t spline_order, int32_t mode, float* const* acts,
                             void* const* pack_fwd, void* const* pack_dx, float* col_mean, float* col_m2,
                             void* workspace, size_t workspace_bytes, void* stream);
int kagnn_gine_kan_layer_bwd(const float* g, int64_t ldg, const float* bn_y, int64_t ld_bn_y, const float* bn_weight,
                             const float* bn_mean, const float* bn_rstd, float* g_bn_weight, float* g_bn_bias,
                             const float* x, int64_t ldx, const float* edge_attr, int64_t lde, int64_t num_nodes,
                             const int32_t* rowptr_t, const int32_t* col_t, const int32_t* perm_t, float self_scale,
                             int32_t num_layers, const int32_t* widths, const float* const* spline_weight,
                             const float* const* spline_scaler, const float* knots, int32_t grid_size,
                             int32_t spline_order, int32_t mode, const float* const* acts, const void* const* pack_dx,
                             float* gx, int64_t ldgx, float* g_edge_attr, int64_t ldge, float* const* g_base_weight,
                             float* const* g_spline_weight, float* const* g_spline_scaler, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ---- the WHOLE message-passing stack of a graph-level model in one call each way (round 5):  num_convs x { GINE convolution around a KAN
 * chain of num_layers layers -> training-mode BatchNorm1d }, every chain hidden -> ... -> hidden with the same `widths` (widths[0] ==
 * widths[num_layers]).  Replaces the loop of reference graph_regression/models.py:107-119
 * (`for i in range(n_layers): x = self.bn[i](self.conv[i](x, edge_index, edge_attr))`, dropout 0) as called per mini-batch from
 * optuna_zinc.py:56-66: on a 256-molecule batch a convolution is ~100 us of device work, and as one tape node per convolution the host
 * spent about as long per node each way on argument marshalling -- the step was host-bound at twice its device time.
 * Forward: ONE pack launch for all layers of all convolutions, then per convolution kagnn_aggregate_gine, the chain (column moments
 * from the last kernel) and the normalising pass -> h[i] (the next convolution's input).  Backward: g = gradient of h[num_convs - 1];
 * per convolution, last first: the norm's statistics pass, its element-wise backward inside the last input-gradient kernel, dW / dX,
 * kagnn_aggregate_gine_bwd -> the previous convolution's g; gx = gradient of x; the edge-attribute gradients of all convolutions add
 * up in g_edge_attr [E, widths[0]] (may be NULL).  Same kernels and summation orders as num_convs calls of
 * kagnn_gine_kan_layer_fwd / _bwd: bit-identical.
 * Arrays: per layer, convolution-major [num_convs * num_layers]: base_weight, spline_weight, spline_scaler, pack_fwd, pack_dx, g_*;
 * acts [num_convs * (num_layers + 1)] (acts[i * (L + 1)] = the aggregated input, ... + L = the chain's output = the norm's input);
 * per convolution [num_convs]: self_scale, momentum, eps (HOST floats); bn_weight, bn_bias, running_mean, running_var (the last two
 * arrays or entries may be NULL), h, save_mean, save_rstd, g_bn_weight, g_bn_bias (device).  num_nodes >= 2.                          */
int kagnn_gine_kan_stack_workspace_bytes(int64_t num_nodes, int32_t num_convs, int32_t num_layers, const int32_t* widths,
                                         int32_t grid_size, int32_t spline_order, int32_t mode, size_t* fwd_bytes_host,
                                         size_t* bwd_bytes_host);
int kagnn_gine_kan_stack_fwd(const float* x, int64_t ldx, const float* edge_attr, int64_t lde, int64_t num_nodes,
                             const int32_t* rowptr, const int32_t* col, const int32_t* perm, const float* self_scale,
                             int32_t num_convs, int32_t num_layers, const int32_t* widths, const float* const* base_weight,
                             const float* const* spline_weight, const float* const* spline_scaler, const float* knots,
                             int32_t grid_size, int32_t spline_order, int32_t mode, float* const* acts, void* const* pack_fwd,
                             void* const* pack_dx, const float* const* bn_weight, const float* const* bn_bias,
                             float* const* running_mean, float* const* running_var, const float* momentum, const float* eps,
                             float* const* h, float* const* save_mean, float* const* save_rstd, void* workspace,
                             size_t workspace_bytes, void* stream);
int kagnn_gine_kan_stack_bwd(const float* g, int64_t ldg, const float* x, int64_t ldx, const float* edge_attr, int64_t lde,
                             int64_t num_nodes, const int32_t* rowptr_t, const int32_t* col_t, const int32_t* perm_t,
                             const float* self_scale, int32_t num_convs, int32_t num_layers, const int32_t* widths,
                             const float* const* spline_weight, const float* const* spline_scaler, const float* knots,
                             int32_t grid_size, int32_t spline_order, int32_t mode, const float* const* acts,
                             const void* const* pack_dx, const float* const* h, const float* const* bn_weight,
                             const float* const* save_mean, const float* const* save_rstd, float* gx, int64_t ldgx,
                             float* g_edge_attr, int64_t ldge, float* const* g_bn_weight, float* const* g_bn_bias,
                             float* const* g_base_weight, float* const* g_spline_weight, float* const* g_spline_scaler,
                             void* workspace, size_t workspace_bytes, void* stream);

/* kagnn_kan_linear_bwd_input_affine that ALSO leaves the two column sums the backward of the folded BatchNorm1d starts from (round 4):
 * sums[0][in] = sum_n gx, sums[1][in] = sum_n gx * xhat, xhat = (x - bn_mean) * bn_rstd on the raw rows x (= that norm's input).
 * The read-out's gradient of the LAST convolution's output in the node models (node_classification_clean/models.py:198-203): that
 * norm's incoming gradient IS this gx, so its statistics pass goes away (hand `sums` to kagnn_gin_kan_layer_bwd_bn_sums as bn_sums).
 * Per workgroup one partial row pair (lanes add their 8 rows, the row groups meet by shuffles, the waves in LDS in order), folded by
 * one launch: deterministic.  Covered (kagnn_kan_bwd_input_sums_ok == 1): split precision, cubic layers of <= 8 coefficients,
 * <= 64 inputs (a multiple of 4) and outputs, >= 32768 rows; else KAGNN_ERR_UNSUPPORTED.                                        */
int kagnn_kan_bwd_input_sums_ok(int64_t num_rows, int32_t in_features, int32_t out_features, int32_t grid_size, int32_t spline_order,
                                int32_t mode);
int kagnn_kan_bwd_input_sums_workspace_bytes(int64_t num_rows, int32_t in_features, size_t* bytes_host);
int kagnn_kan_linear_bwd_input_affine_sums(const float* x, int64_t ldx, const float* x_affine, const float* bn_mean,
                                           const float* bn_rstd, const float* gy, int64_t ldgy, int64_t num_rows, const float* knots,
                                           int32_t in_features, int32_t out_features, int32_t grid_size, int32_t spline_order,
                                           int32_t mode, const void* pack_dx, float* gx, int64_t ldgx, float* sums,
                                           void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Adaptive grids.  Replaces the device work of KANLinear.update_grid (ekan.py:164-211) and the dense
 * b_splines (:79-112).  `grid*` are whole grid buffers [in, G+2k+1] with increasing rows.
 * ------------------------------------------------------------------------------------------ */
/* bases[N, in, G+k] = b_splines(x) on per-feature knot rows (ekan.py:79-112).  spline_order 1..KAGNN_MAX_SPLINE_ORDER
 * (above 4: grid_size + 2 * spline_order + 1 <= 64); a non-finite x gives NaN in every basis at orders above 4.  */
int kagnn_kan_bsplines(const float* x, int64_t ldx, int64_t num_rows, const float* grid,
                       int32_t in_features, int32_t grid_size, int32_t spline_order, float* bases,
                       void* stream);

/* the coefficient refit of update_grid (ekan.py:169-177 + curve2coeff :114-144 + :211):
 *   new_spline_weight[o,f,:] = argmin_s || bases_new(x[:,f]) s - bases_old(x[:,f]) (spline_weight*scaler)[o,f,:] ||
 * through per-feature fp64 Gram matrices (one streaming pass over x; no [N,in,out] intermediate), solved by
 * Cholesky; a basis with no sample in its support gets coefficient 0.  spline_order 1..4, grid_size + 2k + 1 <= 48
 * (up to 46 coefficients).  These two are kagnn_kan_grid_resize (below) with grid_size_old = grid_size_new, no window and
 * no count: the same kernels, the same workspace size, the same bits.  Not in place.                         */
int kagnn_kan_grid_refit_workspace_bytes(int64_t num_rows, int32_t in_features, int32_t grid_size,
                                         int32_t spline_order, size_t* bytes_host);
int kagnn_kan_grid_refit(const float* x, int64_t ldx, int64_t num_rows, const float* grid_old,
                         const float* grid_new, int32_t in_features, int32_t out_features,
                         int32_t grid_size, int32_t spline_order, const float* spline_weight,
                         const float* spline_scaler, float* new_spline_weight, void* workspace,
                         size_t workspace_bytes, void* stream);

/* grid resize (the KAN paper's grid extension, and its inverse): the same refit between grids of TWO sizes,
 *   grid_old [in, grid_size_old+2k+1] -> grid_new [in, grid_size_new+2k+1], one spline_order 1..4 for both,
 *   spline_weight [out, in, grid_size_old+k] -> new_spline_weight [out, in, grid_size_new+k],
 * with grid_size + 2k + 1 <= 48 on either side (up to 46 coefficients: three 16-wide blocks of the fp64 Gram matrices).
 * `window` [in, 2] or NULL: row n takes part in feature f's fit only when window[f][0] <= x[n,f] < window[f][1] (rows in the
 * knot extension beyond the new grid's range cannot be represented there and would leak their misfit into the range).
 * `untouched` [in] or NULL: per feature, the number of new bases no participating row reached (coefficient 0).
 * Deterministic (fixed-order slab sums, no atomics); nothing of size num_rows * in * coefficients exists.  Not in place. */
int kagnn_kan_grid_resize_workspace_bytes(int64_t num_rows, int32_t in_features, int32_t grid_size_old, int32_t grid_size_new,
                                          int32_t spline_order, size_t* bytes_host);
int kagnn_kan_grid_resize(const float* x, int64_t ldx, int64_t num_rows, const float* grid_old, const float* grid_new,
                          const float* window, int32_t in_features, int32_t out_features, int32_t grid_size_old,
                          int32_t grid_size_new, int32_t spline_order, const float* spline_weight, const float* spline_scaler,
                          float* new_spline_weight, int32_t* untouched, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-edge activations of a KANLinear: the edge functions
 *   phi_{o,i}(t) = base_weight[o,i] silu(t) + spline_scaler[o,i] sum_c spline_weight[o,i,c] B_c(t)
 * which the layer's forward only sums over i.  Exact fp32 whatever precision the layer runs in (there is no `precision`
 * argument), spline_order 1..4 (above: KAGNN_ERR_UNSUPPORTED).  `knots` is the shared uniform row [G+2k+1]
 * (per_feature_knots 0) or the whole grid buffer [in, G+2k+1] (per_feature_knots 1).  base_weight and spline_scaler may be NULL
 * (a layer without them).  Nothing of size num_rows * out_features is ever stored: the workspaces hold row-slab partials,
 * which are added in index order (no atomics: the same inputs give the same bits).
 * ------------------------------------------------------------------------------------------ */
/* abs_sum[o*ld_abs_sum + i] = sum_n |phi_{o,i}(x[n,i])|  -- a sum, not a mean: results over a partition of the rows add.  A
 * non-finite x[n,i] makes column i NaN.  num_rows 0: zeros.                                                                  */
int kagnn_kan_edge_abs_sum_workspace_bytes(int64_t num_rows, int32_t in_features, int32_t out_features, int32_t grid_size,
                                           int32_t spline_order, size_t* bytes_host);
int kagnn_kan_edge_abs_sum(const float* x, int64_t ldx, int64_t num_rows, const float* knots, int32_t per_feature_knots,
                           int32_t in_features, int32_t out_features, int32_t grid_size, int32_t spline_order,
                           const float* base_weight, const float* spline_weight, const float* spline_scaler, float* abs_sum,
                           int64_t ld_abs_sum, void* workspace, size_t workspace_bytes, void* stream);
/* its backward under the upstream gradient g_abs_sum[out, in], s = sign(phi_{o,i}(x[n,i])) with sign(0) = 0:
 *   g_base_weight[o,i]     = g sum_n s silu(x)            g_spline_weight[o,i,c] = g scaler sum_n s B_c(x)
 *   g_spline_scaler[o,i]   = g sum_n s sum_c w B_c(x)     gx[n,i]                = sum_o g s phi'_{o,i}(x[n,i])
 * Every output may be NULL (not wanted); the workspace is needed for the three parameter gradients only.                      */
int kagnn_kan_edge_abs_sum_bwd_workspace_bytes(int64_t num_rows, int32_t in_features, int32_t out_features, int32_t grid_size,
                                               int32_t spline_order, size_t* bytes_host);
int kagnn_kan_edge_abs_sum_bwd(const float* x, int64_t ldx, int64_t num_rows, const float* knots, int32_t per_feature_knots,
                               int32_t in_features, int32_t out_features, int32_t grid_size, int32_t spline_order,
                               const float* base_weight, const float* spline_weight, const float* spline_scaler,
                               const float* g_abs_sum, int64_t ld_g_abs_sum, float* g_base_weight, float* g_spline_weight,
                               float* g_spline_scaler, float* gx, int64_t ldgx, void* workspace, size_t workspace_bytes,
                               void* stream);
/* phi[p, o, i] (contiguous [num_points, out, in]) at the sample points t[p] (ldt 0: one column shared by every feature) or
 * t[p*ldt + i].                                                                                                                */
int kagnn_kan_edge_curves(const float* t, int64_t ldt, int64_t num_points, const float* knots, int32_t per_feature_knots,
                          int32_t in_features, int32_t out_features, int32_t grid_size, int32_t spline_order,
                          const float* base_weight, const float* spline_weight, const float* spline_scaler, float* phi,
                          void* stream);
/* first and second moments of every edge function over the rows (the edge scale that attribution scores are built on):
 *   mean[o*ld_mean + i] = (1/N) sum_n phi_{o,i}(x[n,i]),   m2[o*ld_m2 + i] = sum_n (phi_{o,i}(x[n,i]) - mean[o,i])^2
 * m2 is the centred SUM of squares: the caller chooses the divisor, and results over a partition of the rows merge by the
 * pairwise formula.  Accumulated about a pivot phi_{o,i}(x[0,i]) in fp32 within a row slab, merged over the slabs in fp64: an
 * edge that sits on an offset keeps its scale.  Either output may be NULL, not both.  A non-finite x[n,i] makes column i of
 * both NaN.  num_rows 0: zeros.                                                                                                 */
int kagnn_kan_edge_moments_workspace_bytes(int64_t num_rows, int32_t in_features, int32_t out_features, int32_t grid_size,
                                           int32_t spline_order, size_t* bytes_host);
int kagnn_kan_edge_moments(const float* x, int64_t ldx, int64_t num_rows, const float* knots, int32_t per_feature_knots,
                           int32_t in_features, int32_t out_features, int32_t grid_size, int32_t spline_order,
                           const float* base_weight, const float* spline_weight, const float* spline_scaler, float* mean,
                           int64_t ld_mean, float* m2, int64_t ld_m2, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * FastKAN layer.  Replaces FastKANLayer.forward (node_classification_clean/fastkan.py:76-85:
 * LayerNorm :77-78, RadialBasisFunction :46-47, SplineLinear :81, base_linear(silu(x)) :82-84)
 * and its autograd backward.  centers = the module's `rbf.grid` parameter (num_grids fp32
 * values, device pointer), denominator as in fastkan.py:44.  `precision` as for the KAN layer
 * (KAGNN_PREC_SPLIT covers num_grids <= 16; the host sums wider layers over groups of centres).  ln_weight/ln_bias NULL = no layernorm; base_weight NULL = no base branch.
 *   spline_weight [out, in*num_grids]  (in major, grid minor), base_weight [out,in], base_bias [out]
 * ------------------------------------------------------------------------------------------ */
int kagnn_fastkan_fwd_workspace_bytes(int64_t num_rows, int32_t in_features,
                                      int32_t out_features, int32_t num_grids,
                                      int32_t precision, size_t* bytes_host);
int kagnn_fastkan_fwd(const float* x, int64_t ldx, int64_t num_rows, int32_t in_features,
                      int32_t out_features, int32_t num_grids, const float* centers,
                      float denominator, const float* ln_weight, const float* ln_bias,
                      float ln_eps, const float* spline_weight, const float* base_weight,
                      const float* base_bias, float* y, int64_t ldy,
                      float* row_stats /* [N,2] = mean, rstd; required when ln_weight != NULL */,
                      int32_t precision, void* workspace, size_t workspace_bytes, void* stream);
/* 1 when kagnn_fastkan_fwd with a layernorm computes the row statistics inside its forward kernel, 0 when it runs a separate
 * statistics pass over x first (split precision: layers of more than one input chunk or more than 8 centres, or
 * KAGNN_FASTKAN_STATS_IN_FWD=0; 0 also for arguments kagnn_fastkan_fwd refuses).                                          */
int kagnn_fastkan_fwd_stats_in_kernel(int64_t num_rows, int32_t in_features, int32_t out_features, int32_t num_grids,
                                      int32_t precision);
int kagnn_fastkan_bwd_workspace_bytes(int64_t num_rows, int32_t in_features,
                                      int32_t out_features, int32_t num_grids,
                                      int32_t precision, size_t* bytes_host);
/* all gradients of one layer: gx[N,in], g_ln_weight[in], g_ln_bias[in],
 * g_spline_weight[out,in*num_grids], g_base_weight[out,in], g_base_bias[out]; `row_stats` is the
 * array kagnn_fastkan_fwd wrote.  No gradient is produced for `centers` (rbf.grid has
 * requires_grad=False, fastkan.py:43).                                                      */
int kagnn_fastkan_bwd(const float* x, int64_t ldx, const float* gy, int64_t ldgy,
                      int64_t num_rows, int32_t in_features, int32_t out_features,
                      int32_t num_grids, const float* centers, float denominator,
                      const float* ln_weight, const float* ln_bias, float ln_eps,
                      const float* spline_weight, const float* base_weight,
                      const float* row_stats, float* gx, int64_t ldgx, float* g_ln_weight,
                      float* g_ln_bias, float* g_spline_weight, float* g_base_weight,
                      float* g_base_bias, int32_t precision, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-edge activations of a FastKAN layer: the edge functions
 *   phi_{o,i}(n) = sum_g spline_weight[o, i*num_grids+g] exp(-((u[n,i] - centers[g]) / denominator)^2) + base_weight[o,i] silu(x[n,i])
 * with u = LayerNorm(x) (ln_weight / ln_bias given) or x, which the layer's forward only sums over i (base_bias is per output and
 * no part of phi: y[n,o] = sum_i phi_{o,i}(n) + base_bias[o]).  Exact fp32 whatever precision the layer runs in (there is no
 * `precision` argument), every num_grids kagnn_fastkan_fwd takes.  base_weight NULL: no base branch.  Nothing of size
 * num_rows * out_features is ever stored: the workspaces hold row-slab partials, which are added in index order (no atomics: the
 * same inputs give the same bits), and with a layernorm the row statistics [N, 2] and, in the backward, d / du [N, in].
 * `layernorm` of the workspace queries: 1 when ln_weight will be given.
 * ------------------------------------------------------------------------------------------ */
/* abs_sum[o*ld_abs_sum + i] = sum_n |phi_{o,i}(n)|  -- a sum, not a mean: results over a partition of the rows add.  num_rows 0:
 * zeros.                                                                                                                        */
int kagnn_fastkan_edge_abs_sum_workspace_bytes(int64_t num_rows, int32_t in_features, int32_t out_features, int32_t num_grids,
                                               int32_t layernorm, size_t* bytes_host);
int kagnn_fastkan_edge_abs_sum(const float* x, int64_t ldx, int64_t num_rows, int32_t in_features, int32_t out_features,
                               int32_t num_grids, const float* centers, float denominator, const float* ln_weight,
                               const float* ln_bias, float ln_eps, const float* spline_weight, const float* base_weight,
                               float* abs_sum, int64_t ld_abs_sum, void* workspace, size_t workspace_bytes, void* stream);
/* its backward under the upstream gradient g_abs_sum[out, in], s = sign(phi_{o,i}(n)) with sign(0) = 0:
 *   g_spline_weight[o, i*G+g] = g sum_n s rbf_g(u[n,i])       g_base_weight[o,i] = g sum_n s silu(x[n,i])
 *   gx, g_ln_weight, g_ln_bias: sum_o g s dphi/du goes back through the layer's LayerNorm backward, sum_o g s base_weight silu'(x)
 *   is added to gx directly.  g_spline_weight, g_base_weight and gx may be NULL (not wanted); with a layernorm gx and the two
 *   layernorm gradients come from one pass: all three or none.                                                                 */
int kagnn_fastkan_edge_abs_sum_bwd_workspace_bytes(int64_t num_rows, int32_t in_features, int32_t out_features, int32_t num_grids,
                                                   int32_t layernorm, size_t* bytes_host);
int kagnn_fastkan_edge_abs_sum_bwd(const float* x, int64_t ldx, int64_t num_rows, int32_t in_features, int32_t out_features,
                                   int32_t num_grids, const float* centers, float denominator, const float* ln_weight,
                                   const float* ln_bias, float ln_eps, const float* spline_weight, const float* base_weight,
                                   const float* g_abs_sum, int64_t ld_g_abs_sum, float* g_spline_weight, float* g_base_weight,
                                   float* gx, int64_t ldgx, float* g_ln_weight, float* g_ln_bias, void* workspace,
                                   size_t workspace_bytes, void* stream);
/* phi[p, o, i] (contiguous [num_points, out, in]): the spline branch at t[p] (ldt 0: one column shared by every feature) or
 * t[p*ldt + i] -- the argument AFTER any layernorm --, the base branch at t_base likewise (t_base NULL: at t).  spline_weight NULL
 * or base_weight NULL leaves that branch out (not both).                                                                        */
int kagnn_fastkan_edge_curves(const float* t, int64_t ldt, const float* t_base, int64_t ldt_base, int64_t num_points,
                              int32_t in_features, int32_t out_features, int32_t num_grids, const float* centers,
                              float denominator, const float* spline_weight, const float* base_weight, float* phi, void* stream);

/* ------------------------------------------------------------------------------------------
 * Feature-sharded FastKAN layer (no counterpart in the reference, which is single-device: this is
 * FastKANLayer.forward, fastkan.py:76-85, when a rank holds `in_features` of the row's P * in_features input columns and the
 * matching slices of layernorm.weight / .bias, spline_linear.weight[:, columns * num_grids], base_linear.weight[:, columns]).
 * LayerNorm (fastkan.py:77-78) is the one operation of the layer that reduces over the sharded axis; the exchange is
 * 2 floats per row each way:
 *   forward : kagnn_fastkan_row_moments  -> moments[n] = (mean, sum of squared deviations from it) over the local columns;
 *             the caller gathers the P arrays ([P][N][2], rank order);  kagnn_fastkan_merge_moments merges a row's P pairs
 *             in rank order (Chan's update: no cancellation, same bits on every rank) -> row_stats[n] = (mean, rstd) over all
 *             P * in_features columns;  kagnn_fastkan_shard_fwd = kagnn_fastkan_fwd with row_stats GIVEN: y = this rank's
 *             partial sums over its columns for ALL outputs (base_bias on one rank only); the caller reduce-scatters them.
 *   backward: kagnn_fastkan_shard_bwd (gy = the gathered [N, out] gradient) = everything but the LayerNorm backward:
 *             g_spline_weight / g_base_weight / g_base_bias (may be NULL) of the local slices, gx = the base-branch part,
 *             d loss / dz kept in `workspace`, row_sums[n] = (sum_f gz*gamma, sum_f gz*gamma*zhat) over the local columns;
 *             the caller sums row_sums over the ranks (all-reduce);  kagnn_fastkan_shard_bwd_finish completes gx and writes
 *             g_ln_weight / g_ln_bias -- SAME shape arguments and SAME workspace (kagnn_fastkan_bwd_workspace_bytes), not
 *             touched between the two calls.  Without layernorm (ln_weight NULL) shard_bwd alone is the whole backward.
 *   num_rows == 0 (a rank or row chunk without rows): every call succeeds and reads no row; the row arrays (x, gy, y, gx, moments,
 *             row_stats, row_sums) may be NULL, the requested weight / bias / LayerNorm gradients are written as zeros.
 * ------------------------------------------------------------------------------------------ */
int kagnn_fastkan_row_moments(const float* x, int64_t ldx, int64_t num_rows, int32_t in_features,
                              float* moments /* [N,2] */, void* stream);
int kagnn_fastkan_merge_moments(const float* gathered /* [P][N][2] */, int32_t num_ranks, int64_t num_rows,
                                int32_t in_features /* per rank */, float ln_eps, float* row_stats /* [N,2] */,
                                void* stream);
int kagnn_fastkan_shard_fwd(const float* x, int64_t ldx, int64_t num_rows, int32_t in_features,
                            int32_t out_features, int32_t num_grids, const float* centers,
                            float denominator, const float* ln_weight, const float* ln_bias,
                            const float* row_stats, const float* spline_weight, const float* base_weight,
                            const float* base_bias, float* y, int64_t ldy, int32_t precision,
                            void* workspace, size_t workspace_bytes, void* stream);
int kagnn_fastkan_shard_bwd(const float* x, int64_t ldx, const float* gy, int64_t ldgy,
                            int64_t num_rows, int32_t in_features, int32_t out_features,
                            int32_t num_grids, const float* centers, float denominator,
                            const float* ln_weight, const float* ln_bias, const float* spline_weight,
                            const float* base_weight, const float* row_stats, float* gx, int64_t ldgx,
                            float* row_sums /* [N,2] */, float* g_spline_weight, float* g_base_weight,
                            float* g_base_bias,
                            int32_t parts /* 1 = input-gradient half (gx, dz, row_sums), 2 = weight-gradient half, 3 = both:
                                             two calls (1 then 2) let the all-reduce of row_sums run beside the weight gradient */,
                            int32_t precision, void* workspace, size_t workspace_bytes, void* stream);
int kagnn_fastkan_shard_bwd_finish(const float* x, int64_t ldx, int64_t num_rows, int32_t in_features,
                                   int32_t in_features_total, int32_t out_features, int32_t num_grids,
                                   const float* ln_weight, const float* ln_bias, const float* row_stats,
                                   const float* row_sums, float* gx, int64_t ldgx, float* g_ln_weight,
                                   float* g_ln_bias, int32_t precision, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * BatchNorm1d over node rows (the epilogue after every convolution of the node / graph models:
 * node_classification_clean/models.py:195-202, torch.nn.BatchNorm1d semantics).  x, y, gy, gx are
 * [num_rows, num_features] row-major with leading dimensions in elements; statistics per column.
 *   training != 0: batch statistics (biased variance) normalise; running_mean / running_var (may be
 *                  NULL) are updated with `momentum` (unbiased variance), save_mean / save_rstd
 *                  receive the batch mean and 1/sqrt(var + eps) for the backward.
 *   training == 0: running statistics normalise; save_mean / save_rstd receive running_mean and
 *                  1/sqrt(running_var + eps).
 * weight / bias may be NULL (affine=False).  The backward writes gx (may be NULL), g_weight and
 * g_bias (either may be NULL) for the same `training` flag as the forward.  Deterministic.
 *
 * Fused epilogue (models.py:198-201: `x = dropout(bn(conv(x)))`):
 *   col_mean / col_m2 (both or neither, training only): the column moments of x from the kernel that produced
 *                  it (kagnn_kan_linear_fwd_moments, kagnn_gin_kan_layer_fwd) -- the statistics pass is skipped;
 *   dropout_p > 0 (training only): y = dropout(bn(x), p) in the same pass; element (row, col) is kept with
 *                  probability 1-p (resolution 2^-16) and scaled by 1/(1-p), decided by a counter-based hash of
 *                  (dropout_seed, row, col / 4) -- a pure function of the seed, NOT torch's Philox stream.  The
 *                  backward regenerates the decisions from the same (dropout_p, dropout_seed): `gy` is the
 *                  gradient of the dropped-out y.  No mask tensor exists.
 * ------------------------------------------------------------------------------------------ */
int kagnn_batchnorm_workspace_bytes(int64_t num_rows, int32_t num_features, size_t* bytes_host);
int kagnn_batchnorm_fwd(const float* x, int64_t ldx, int64_t num_rows, int32_t num_features,
                        const float* weight, const float* bias, float* running_mean,
                        float* running_var, float momentum, float eps, int32_t training,
                        const float* col_mean, const float* col_m2, float dropout_p,
                        uint64_t dropout_seed, float* y,
                        int64_t ldy, float* save_mean, float* save_rstd, void* workspace,
                        size_t workspace_bytes, void* stream);
int kagnn_batchnorm_bwd(const float* x, int64_t ldx, const float* gy, int64_t ldgy,
                        int64_t num_rows, int32_t num_features, const float* weight,
                        const float* save_mean, const float* save_rstd, int32_t training,
                        float dropout_p, uint64_t dropout_seed, float* gx,
                        int64_t ldgx, float* g_weight, float* g_bias, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Attention aggregation of KAGATConv / FASTKAGATConv (node_classification_clean/models.py:39-46,
 * 76-83: torch_geometric GATConv with `lin` = a KAN layer; heads concatenated, negative slope 0.2,
 * existing self loops removed and one added per node, no attention dropout).
 *   xh [N, heads*channels] = lin(x);  att_src / att_dst [heads, channels];  bias [heads*channels] or NULL
 *   kagnn_gat_logits: a_src[N,heads], a_dst[N,heads]
 *   kagnn_gat_fwd   : out [N, heads*channels], and the per-(node, head) softmax maximum / normaliser
 *                     (row_max, row_sum: the only extra state the backward needs)
 *   kagnn_gat_bwd   : gx = d loss / d xh (all three paths), g_src[N,heads] / g_dst[N,heads] = d loss / d a_src,
 *                     a_dst (the caller contracts them with xh for the att_src / att_dst gradients);
 *                     edge_scratch [E*heads] and self_scratch [N*heads] floats.  CSR arrays as built by
 *                     kagnn_csr_build: (rowptr, col, perm) by destination, (rowptr_t, col_t, perm_t) by source;
 *                     hub_seg / num_hub_seg / hub_threshold = the by-destination hub segments (rows with more
 *                     edges get a whole workgroup per head; NULL / 0 disables that).
 * ------------------------------------------------------------------------------------------ */
int kagnn_gat_logits(const float* xh, int64_t ldx, int64_t num_nodes, int32_t heads, int32_t channels,
                     const float* att_src, const float* att_dst, float* a_src, float* a_dst,
                     void* stream);
int kagnn_gat_fwd(const float* xh, int64_t ldx, const float* a_src, const float* a_dst,
                  const int32_t* rowptr, const int32_t* col, int64_t num_nodes, int32_t heads,
                  int32_t channels, const float* bias, float* out, int64_t ldo, float* row_max,
                  float* row_sum, const int32_t* hub_seg, int64_t num_hub_seg, int32_t hub_threshold,
                  void* stream);
int kagnn_gat_bwd(const float* xh, int64_t ldx, const float* gout, int64_t ldg, const float* out,
                  int64_t ldo, const float* bias, const float* a_src, const float* a_dst,
                  const float* row_max, const float* row_sum, const int32_t* rowptr,
                  const int32_t* col, const int32_t* perm, const int32_t* rowptr_t,
                  const int32_t* col_t, const int32_t* perm_t, const float* att_src,
                  const float* att_dst, int64_t num_nodes, int32_t heads, int32_t channels,
                  float* edge_scratch, float* self_scratch, float* g_dst, float* g_src, float* gx,
                  int64_t ldgx, const int32_t* hub_seg, int64_t num_hub_seg, int32_t hub_threshold,
                  void* stream);

/* gradients of GATConv's attention vectors from the per-node terms kagnn_gat_bwd returns:
 *   g_att_src[h,c] = sum_n g_src[n,h] * xh[n, h*C + c],  g_att_dst likewise with g_dst   (heads*channels <= 1024).
 * One pass over xh, deterministic.                                                             */
int kagnn_gat_att_grad_workspace_bytes(int64_t num_nodes, int32_t heads, int32_t channels, size_t* bytes_host);
int kagnn_gat_att_grad(const float* xh, int64_t ld, const float* g_src, const float* g_dst, int64_t num_nodes,
                       int32_t heads, int32_t channels, float* g_att_src, float* g_att_dst,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Loss tail of the timing harness (node_classification_clean/time_model.py:43-45):
 *   out = softmax(logits, dim=1); loss = CrossEntropyLoss()(out[mask], y[mask])
 * pre_softmax = 1 keeps the reference's softmax-before-CrossEntropyLoss (which applies log_softmax again);
 * 0 is plain softmax cross-entropy (utils.py's training loop).  mean over the masked rows; `mask` [N] bytes
 * (torch.bool storage) or NULL = every row; labels int64 in [0, num_classes) (anything else: loss = NaN).
 * loss / count: device scalars (count = number of masked rows, kept for the backward; no host sync);
 * row_stats [N,3] is the only tensor saved.  Deterministic.  g_logits rows outside the mask are written as 0. */
int kagnn_softmax_xent_workspace_bytes(int64_t num_rows, size_t* bytes_host);
int kagnn_softmax_xent_fwd(const float* logits, int64_t ld, int64_t num_rows, int32_t num_classes,
                           const int64_t* labels, const uint8_t* mask, int32_t pre_softmax, float* loss,
                           float* row_stats, float* count, void* workspace, size_t workspace_bytes,
                           void* stream);
int kagnn_softmax_xent_bwd(const float* logits, int64_t ld, int64_t num_rows, int32_t num_classes,
                           const int64_t* labels, const uint8_t* mask, int32_t pre_softmax,
                           const float* row_stats, const float* count, const float* g_loss,
                           float* g_logits, int64_t ldg, void* stream);

/* Loss of the graph-regression scripts (graph_regression/optuna_zinc.py:58: torch.nn.L1Loss()(model(data).squeeze(), data.y)):
 *   loss = mean |pred - target| over n contiguous fp32 elements; g_pred = (g_loss / n) * sign(pred - target).
 * loss / g_loss: device scalars; one launch each way, deterministic (fixed summation order), no host sync. */
int kagnn_l1_loss_fwd(const float* pred, const float* target, int64_t n, float* loss, void* stream);
int kagnn_l1_loss_bwd(const float* pred, const float* target, int64_t n, const float* g_loss, float* g_pred, void* stream);

/* The dense layer of the MLP baselines (torch.nn.Linear, with the torch.nn.ReLU that follows it inside the reference's make_mlp
 * chains; the `lin` of torch_geometric's GCNConv / GATConv):
 *   y[N,out] = x[N,in] @ W[out,in]^T (+ bias[out]) (then max(., 0) when relu = 1)
 * x, y, gy, gx are row-major with a row stride (ld*, in elements) and unit column stride; W [out,in], gW [out,in], bias and
 * gb [out] are contiguous.  Any N >= 0, in >= 1, out >= 1; nothing outside [N, width] of an operand is read or written (the
 * columns between width and ld keep their bytes).
 * Precision: exact fp32 products on the fp32-input matrix instructions, i.e. an ordered fp32 fma chain per output element, in
 * EVERY precision mode -- KAGNN_PREC_* / KAGNN_PRECISION do not apply to these entry points.
 * Mask rule of the gradients: `y` is the SAVED forward output of a relu = 1 call, or NULL for a layer without the fused ReLU.
 * With y given, gy is read as gy (.) m, m = (y > 0): torch's threshold_backward on the result, so the gradient is 0 where
 * y == 0.  With y == NULL, m is all ones.
 *   kagnn_linear_bwd_input :  gx[N,in]  = (gy (.) m) @ W
 *   kagnn_linear_bwd_weight:  gW[out,in] = (gy (.) m)^T @ x ,  gb[out] = column sums of gy (.) m   (gb may be NULL)
 * Determinism: no atomics.  The weight gradient sums the rows in slabs held in `workspace`
 * (kagnn_linear_bwd_weight_workspace_bytes: slabs * out * (in + 1) floats; 16-byte aligned) and adds the slabs in index order,
 * so the same inputs give bit-identical gW and gb from run to run.  N == 0: y / gx are not touched, gW and gb are set to 0. */
int kagnn_linear_bwd_weight_workspace_bytes(int64_t num_rows, int32_t in_features, int32_t out_features, size_t* bytes_host);
int kagnn_linear_fwd(const float* x, int64_t ldx, int64_t num_rows, int32_t in_features, const float* weight, const float* bias,
                     int32_t out_features, int32_t relu, float* y, int64_t ldy, void* stream);
int kagnn_linear_bwd_input(const float* gy, int64_t ldgy, const float* y, int64_t ldy, int64_t num_rows, int32_t out_features,
                           const float* weight, int32_t in_features, float* gx, int64_t ldgx, void* stream);
int kagnn_linear_bwd_weight(const float* x, int64_t ldx, const float* gy, int64_t ldgy, const float* y, int64_t ldy,
                            int64_t num_rows, int32_t in_features, int32_t out_features, float* g_weight, float* g_bias,
                            void* workspace, size_t workspace_bytes, void* stream);

/* Dense multi-head attention with the bias added AFTER the softmax: the core of the reference's AttentionWithFastKANTransform
 * (node_classification_clean/fastkan.py:182-198) between its projections and linear_o, and the backward of that.
 *   s[b,q,k,h] = scale * sum_c wq[b,q,h,c] wk[b,k,h,c]         p = softmax over k of s
 *   a[b,q,k,h] = p + bias[b,q,k]                                (one bias for every head; bias == NULL: a = p)
 *   o[b,q,h,:] = sum_k a[b,q,k,h] wv[b,k,h,:]                   o *= sigmoid(gate[b,q,h,:])   (gate == NULL: no gate)
 * Layouts: wq, gate, o, o_ungated and their gradients are [B * Q, H * c] fp32 rows, wk, wv and theirs [B * K, H * c], each with a
 * row stride in elements (>= H * c) and unit column stride; head h owns columns [h * c, (h + 1) * c).  bias is [B, Q, K] with a
 * batch stride and a row stride in elements and unit stride along K; a batch (or row) stride of 0 broadcasts on the read side.
 * g_bias is a dense [B, Q, K] result (row stride >= K, batch stride >= Q * row stride).  stats is [2][B * Q * H] contiguous: the row
 * maximum m of s, then log(sum_k exp(s - m)).  Limits: 1 <= head_dim <= 128 (else KAGNN_ERR_UNSUPPORTED), num_heads >= 1, batch,
 * num_queries, num_keys 0 .. 2^31 - 1.  Nothing outside [rows, H * c] of an operand is read or written; nothing of size Q * K is
 * allocated or written except g_bias.
 * Forward: one pass over K with an online softmax; writes o, and with stats != NULL also stats and (o_ungated != NULL) the o before
 * the gate -- what the backward takes.  K == 0: o = 0.  B * Q == 0: no launch.
 * Backward (d_o = g_out * sigmoid(gate), the gradient of the ungated o; p recomputed from stats):
 *   dA = <d_o[q,h,:], wv[k,h,:]>    g_wv[k] = sum_q a d_o[q]    g_bias[q,k] = sum_h dA    D[q,h] = sum_k p dA    dS = p (dA - D)
 *   g_wq[q] = scale sum_k dS wk[k]    g_wk[k] = scale sum_q dS wq[q]    g_gate = g_out o_ungated sig (1 - sig)
 * D is summed from p itself when there is a bias: the shortcut <d_o, o> equals D + sum_k bias dA there.  g_bias may be NULL (not
 * computed); g_gate is required exactly when gate is given.  The workspace (kagnn_attention_bwd_workspace_bytes, 16-byte aligned)
 * holds D and, with a gate, d_o: B * Q * H * (1 + c) floats, no term in Q * K.
 * Precision: exact fp32 (ordered fma chains) in EVERY precision mode; KAGNN_PREC_* / KAGNN_PRECISION do not apply.
 * Determinism: no atomics, every sum has one owner and a fixed order: the same inputs give bit-identical results from run to run. */
int kagnn_attention_fwd(const float* wq, int64_t ldq, const float* wk, int64_t ldk, const float* wv, int64_t ldv, const float* bias,
                        int64_t bias_batch_stride, int64_t bias_row_stride, const float* gate, int64_t ldgate, int64_t batch,
                        int64_t num_queries, int64_t num_keys, int32_t num_heads, int32_t head_dim, float scale, float* o, int64_t ldo,
                        float* o_ungated, int64_t ldo_ungated, float* stats, void* stream);
int kagnn_attention_bwd_workspace_bytes(int64_t batch, int64_t num_queries, int64_t num_keys, int32_t num_heads, int32_t head_dim,
                                        int32_t has_gate, size_t* bytes_host);
int kagnn_attention_bwd(const float* g_out, int64_t ldg_out, const float* wq, int64_t ldq, const float* wk, int64_t ldk,
                        const float* wv, int64_t ldv, const float* bias, int64_t bias_batch_stride, int64_t bias_row_stride,
                        const float* gate, int64_t ldgate, const float* o_ungated, int64_t ldo_ungated, const float* stats,
                        int64_t batch, int64_t num_queries, int64_t num_keys, int32_t num_heads, int32_t head_dim, float scale,
                        float* g_wq, int64_t ldg_wq, float* g_wk, int64_t ldg_wk, float* g_wv, int64_t ldg_wv, float* g_bias,
                        int64_t g_bias_batch_stride, int64_t g_bias_row_stride, float* g_gate, int64_t ldg_gate, void* workspace,
                        size_t workspace_bytes, void* stream);

/* What the graph-classification scripts wrap around their models (graph_classification/graph_classification_utils.py).
 *
 * Degree (:31-36), the node features of the unlabeled TU datasets: x = one_hot(clip(degree(edge_index[0]), 0, K - 1), K).float().
 *   rowptr_by_source [num_nodes + 1]: the offsets of the CSR grouped by SOURCE node (rowptr_t of kagnn_csr_build_small); NULL = a
 *   dataset without edges (every row gets its 1 in column 0).  x [num_nodes, num_classes] fp32, row stride ldx >= num_classes;
 *   every element of every row is written (no memset needed), no atomics. */
int kagnn_degree_one_hot(const int32_t* rowptr_by_source, int64_t num_nodes, int32_t num_classes, float* x, int64_t ldx, void* stream);

/* train / val / test (:45-72): F.nll_loss(logp, y) of a mini-batch, reduction 'mean' and 'sum' from the same launch, and the
 * arg-max accuracy count.  logp [rows, classes] fp32 log-probabilities (row stride ld), y [rows] int64.  ONE launch of ONE
 * workgroup (rows <= KAGNN_BATCH_MAX_GRAPHS is the intended size; more rows work at one workgroup's pace).  The sum of
 * -logp[r, y[r]] is taken in fp64 in a fixed order; loss_mean = sum / rows and loss_sum = sum are each rounded once to fp32
 * (either may be NULL; rows == 0: NaN and 0).  accum, when not NULL, is an 8-byte aligned device record
 *   { double nll_sum; int64_t correct; int64_t graphs; }
 * to which the launch ADDS sum, the number of rows whose arg-max over the row equals y[r] (ties: the LOWEST class index; a row
 * holding a NaN is never correct) and rows -- with plain loads and stores: launches on one stream are ordered, so no atomics and
 * the same bits every run.  A label outside [0, classes): loss_mean, loss_sum (and nll_sum) are NaN, *flag is set to 1 (the launch
 * never clears it), the row counts as wrong.  No host synchronisation.
 * Backward: g_logp [rows, classes] (row stride ldg) is written whole: -(g_loss / rows) for KAGNN_REDUCTION_MEAN or -g_loss for
 * KAGNN_REDUCTION_SUM at the label, exactly 0 elsewhere; rows with a label outside [0, classes) are all zero. */
#define KAGNN_REDUCTION_MEAN 0
#define KAGNN_REDUCTION_SUM 1
int kagnn_nll_loss_fwd(const float* logp, int64_t ld, int64_t rows, int32_t classes, const int64_t* y, float* loss_mean,
                       float* loss_sum, void* accum, int32_t* flag, void* stream);
int kagnn_nll_loss_bwd(const int64_t* y, int64_t rows, int32_t classes, const float* g_loss, int32_t reduction, float* g_logp,
                       int64_t ldg, void* stream);

/* What the node-classification experiment does after the logits (node_classification_clean/utils.py: train_total, EarlyStopper),
 * without a read-back: the loss and the accuracies of every split in one pass, the stopper as a device record, the best-weights
 * save as a predicated copy.  All three: no host synchronisation, deterministic.
 *
 * kagnn_node_eval: logits [num_rows, num_classes] fp32 (row stride ld >= num_classes; 1 <= num_classes, tested to 1024), labels
 * [num_rows] int64, split_bits [num_rows] bytes: bit s set = the row belongs to split s (splits may overlap; bits at or above
 * num_splits are ignored; 1 <= num_splits <= 8).  records: an 8-byte aligned device array of num_splits
 *   { double xent_sum; int64_t correct; int64_t rows; }
 * which the call OVERWRITES: the sum over the split's rows of logsumexp(z) - z[y] (the row term max-subtracted in fp32, the sum in
 * fp64 in a fixed order: per-workgroup partials in the workspace, added in index order -- no floating-point atomics, the same
 * bits every run), the number of rows whose arg-max equals the label (ties: the LOWEST class index; a row holding a NaN is never
 * correct, and its term is NaN) and the number of rows.  One read of the logits serves all splits; a row in no split costs its
 * byte only.  A label outside [0, num_classes) in a row of some split: that split's xent_sum is NaN, the row counts as wrong,
 * *flag is set to 1 (the launch never clears it), nothing is read out of bounds.  num_rows == 0: every record is zero.
 *
 * kagnn_early_stop_update: EarlyStopper(patience, min_delta).early_stop(val_loss) of one epoch on the device record
 *   { float min_loss (start: +inf), min_delta; int32_t patience, counter, epochs, best_epoch (start: -1), improved, stopped; }
 * with val_loss = (float)(xent_sum / rows) of eval_records[val_split] (rounded once; rows == 0: NaN) and fp32 comparisons:
 *   val < min_loss: min_loss = val, counter = 0, best_epoch = epochs, improved = 1;
 *   else val >= min_loss + min_delta: ++counter, stopped = 1 once counter >= patience;   anything else (NaN included): nothing.
 * Before the rule the num_splits eval records are copied to history[epochs] (history: [max_epochs][num_splits] records, or
 * NULL); after it epochs is incremented.  With stopped set, or epochs == max_epochs, the launch writes improved = 0 and nothing
 * else: later epochs are inert.
 *
 * kagnn_copy_if: dst[k][0 .. bytes[k]) = src[k][..] for all k < count if the device word *flag != 0, else no store at all.
 * HOST arrays of device pointers (4-byte aligned) and byte counts (multiples of 4), one launch per 32 tensors; 16-byte vectors
 * where both pointers of a tensor allow, 4-byte words otherwise and for the tail.  Parameters and buffers alike go through it as
 * bytes (running statistics, num_batches_tracked, grids): with flag = the record's `improved` it is the best-weights snapshot. */
int kagnn_node_eval_workspace_bytes(int64_t num_rows, int32_t num_classes, int32_t num_splits, size_t* bytes_host);
int kagnn_node_eval(const float* logits, int64_t ld, int64_t num_rows, int32_t num_classes, const int64_t* labels,
                    const uint8_t* split_bits, int32_t num_splits, void* records, int32_t* flag, void* workspace,
                    size_t workspace_bytes, void* stream);
int kagnn_early_stop_update(const void* eval_records, int32_t num_splits, int32_t val_split, void* state, void* history,
                            int32_t max_epochs, void* stream);
int kagnn_copy_if(const int32_t* flag, int32_t count, void* const* dst, const void* const* src, const int64_t* bytes, void* stream);

/* What the graph-regression experiment wraps around its models (graph_regression/optuna_zinc.py:56-92, optuna_qm9.py:56-96:
 * train_model_with_parameters; graph_regression/utils.py:8-16: EarlyStopper), without a read-back.  Both: one launch of one
 * workgroup, no atomics, no host synchronisation, the same bits every run.
 *
 * kagnn_l1_loss_meter_fwd: pred and target are fp32 [rows, targets] with row strides ldp, ldt >= targets;
 * 1 <= targets <= KAGNN_REGRESSION_MAX_TARGETS (more: KAGNN_ERR_ARG).  The term of an element is fabsf(p - t) with scale == NULL,
 * else fabsf(t*s - p*s) / s with s = scale[column] (fp32 [targets]; optuna_qm9.py:72) -- every operation rounded to fp32 on its
 * own, never contracted into a fused multiply-add, so a term has the bits torch's elementwise kernels give it.  Each column's
 * terms are added in fp64 in a fixed order.  loss_mean (may be NULL) = (float)(sum of all terms / (rows * targets)), the column
 * sums added in index order, rounded once; rows == 0: NaN.  meter (may be NULL; not both) is an 8-byte aligned device record
 *   { int64_t graphs; int64_t targets; double abs_sum[KAGNN_REGRESSION_MAX_TARGETS]; }
 * to which the launch ADDS rows and the column sums with plain loads and stores (launches on one stream are ordered) and whose
 * `targets` it writes; rows == 0 leaves it untouched.  A NaN reaches its own column's sum and loss_mean only.  The backward of
 * the unscaled loss is kagnn_l1_loss_bwd with n = rows * targets on contiguous operands.
 *
 * kagnn_regression_epoch_update: what the scripts decide once per epoch, from the three splits' meters.  test_meter == NULL: the
 * validation meter (and n_val) serve as the test split.  n_train / n_val / n_test: the scripts' len(loader.dataset) divisors.
 * Per split s and target t < the meter's `targets` (clamped to 0..32): mae[s][t] = abs_sum[t] / n_s in fp64; the split's figure
 * is the mae added over the targets in index order, divided by their number, rounded once to fp32 (no targets: NaN).
 * history (may be NULL): double [max_epochs][3][KAGNN_REGRESSION_MAX_TARGETS], 8-byte aligned; history[epochs][s][t] = mae[s][t]
 * (0 for t at or beyond the meter's targets).  state: the 4-byte aligned device record
 *   { float min_loss (start: +inf), min_delta, best_val (start: +inf), test_at_best (start: NaN);
 *     int32_t patience, counter, epochs, best_epoch (start: -1), test_epoch (start: -1), improved, stopped, pad; }
 * advanced with fp32 comparisons, in this order:
 *   1. best_val >= val (optuna_zinc.py:75; a tie counts): best_val = val, test_at_best = the test figure, test_epoch = epochs;
 *   2. val < min_loss: min_loss = val, counter = 0, best_epoch = epochs, improved = 1;
 *      else val >= min_loss + min_delta: ++counter, stopped = 1 once counter >= patience; improved = 0;
 *      anything else (NaN included): nothing; improved = 0;
 *   3. ++epochs.
 * With stopped set, or epochs == max_epochs, the launch writes improved = 0 and nothing else of the record or the history.  In
 * every case it zeroes graphs and abs_sum of the three meters for the next epoch. */
#define KAGNN_REGRESSION_MAX_TARGETS 32
int kagnn_l1_loss_meter_fwd(const float* pred, int64_t ldp, const float* target, int64_t ldt, int64_t rows, int32_t targets,
                            const float* scale, float* loss_mean, void* meter, void* stream);
int kagnn_regression_epoch_update(void* train_meter, void* val_meter, void* test_meter, int64_t n_train, int64_t n_val,
                                  int64_t n_test, void* state, double* history, int32_t max_epochs, void* stream);

/* Optimiser of the same scripts (optuna_zinc.py:49,62: torch.optim.Adam(model.parameters(), lr), optimizer.step() per batch): one
 * update of `count` fp32 tensors in one launch per 32 tensors.  HOST arrays of device pointers / element counts; `step` = 1, 2, ...
 * (bias corrections 1 - beta^step are computed on the host in double).  torch's rule without amsgrad:
 *   g += weight_decay * p;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps) */
int kagnn_adam_step(int32_t count, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                    const int64_t* numel, float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, void* stream);

/* ------------------------------------------------------------------------------------------
 * Direct peer-to-peer exchange steps of the feature-sharded layer (no reference counterpart: the reference has no
 * multi-GPU code; contract = BASELINE.json north_star, SURVEY.md 8(b)/(e): "sharded variants", "hand-rolled
 * direct P2P over hipIpcMemHandle peer buffers").  `parts` / `shards`: HOST arrays of `world` DEVICE pointers -- entry p is
 * rank p's exchange buffer as mapped into THIS process (hipIpcOpenMemHandle; own entry = own buffer).  The caller orders the
 * ranks (every peer's buffer complete before the call, not overwritten before every reader is done).
 *   reduce_scatter: y[n][c] = sum_p parts[p][n*ld + rank*(out/world) + c], c < out/world, summed in rank order (deterministic)
 *   all_gather:     g[n][p*w + c] = shards[p][n*lds + c]
 * out/world (resp. w) and the leading dimensions must be multiples of 4 floats, bases 16-byte aligned; world <= 16. */
int kagnn_p2p_reduce_scatter(const float* const* parts, int32_t world, int32_t rank, int64_t num_rows, int32_t out_features,
                             int64_t ld, float* y, int64_t ldy, void* stream);
int kagnn_p2p_all_gather(const float* const* shards, int32_t world, int64_t num_rows, int32_t shard_width, int64_t lds,
                         float* g, int64_t ldg, void* stream);

/* ------------------------------------------------------------------------------------------
 * BatchNorm1d folded into its consumers (round 4).  Reference: node_classification_clean/models.py:198-203 --
 * `x = self.bns[i](self.convs[i](x, edge_index))` feeds the next GINConv and the skip read-out `lay_out(torch.cat(l, dim=1))`.
 * In training mode without dropout the normalised matrix need not exist: kagnn_batchnorm_stats_affine turns the column
 * moments the convolution's last forward kernel produced into (save_mean, save_rstd, running statistics, per-column affine
 * a = gamma * rstd, b = beta - mean * a), and every consumer reads the convolution's raw output y as  a * y + b:
 *   - the next convolution's aggregation: kagnn_aggregate_sum_affine / kagnn_gin_kan_layer_fwd_affine
 *       out_i = a * (self_scale * y_i + sum_{j->i} y_j) + (self_scale + deg_i) * b      (unit edge weights)
 *   - the read-out: kagnn_kan_linear_fwd_parts_affine (per column block), kagnn_kan_linear_bwd_input_affine,
 *     kagnn_kan_linear_bwd_weight_affine (cubic layers, <= 8 coefficients, <= 64 outputs, split precision).
 * Gradients are taken with respect to the NORMALISED input; the norm's own backward (kagnn_gin_kan_layer_bwd_bn,
 * kagnn_batchnorm_bwd) goes on from there, so nothing else changes.  `affine` arrays: 2 * width floats, scales then shifts,
 * 16-byte aligned.
 */
int kagnn_batchnorm_stats_affine(const float* col_mean, const float* col_m2, int64_t num_rows, int32_t num_feat,
                                 const float* gamma, const float* beta, float* running_mean, float* running_var,
                                 float momentum, float eps, float* save_mean, float* save_rstd, float* affine, void* stream);
int kagnn_aggregate_sum_affine(const float* x, int64_t ldx, float* out, int64_t ldo, const int32_t* rowptr, const int32_t* col,
                               int64_t num_nodes, int32_t num_feat, float self_scale, const float* col_scale,
                               const float* col_shift, const int32_t* hub_seg, int64_t num_hub_seg, int32_t hub_threshold,
                               const float* addend, int64_t ld_addend, void* workspace, size_t workspace_bytes, void* stream);
int kagnn_gin_kan_layer_fwd_affine(const float* x, int64_t ldx, int64_t num_nodes, const int32_t* rowptr, const int32_t* col,
                                   const int32_t* hub_seg, int64_t num_hub_seg, int32_t hub_threshold, float self_scale,
                                   const float* in_col_scale, const float* in_col_shift,
                                   int32_t num_layers, const int32_t* widths, const float* const* base_weight,
                                   const float* const* spline_weight, const float* const* spline_scaler, const float* knots,
                                   int32_t grid_size, int32_t spline_order, int32_t mode, float* const* acts,
                                   void* const* pack_fwd, void* const* pack_dx, float* col_mean, float* col_m2,
                                   void* workspace, size_t workspace_bytes, void* stream);
int kagnn_kan_linear_fwd_parts_affine(const float* const* x_parts, const int32_t* part_widths, const int64_t* part_ld,
                                      const float* const* part_affine, int32_t num_parts, int64_t num_rows, const float* knots,
                                      int32_t in_features, int32_t out_features, int32_t grid_size, int32_t spline_order,
                                      int32_t mode, const void* pack_fwd, float* y, int64_t ldy, void* workspace,
                                      size_t workspace_bytes, void* stream);
int kagnn_kan_linear_bwd_input_affine(const float* x, int64_t ldx, const float* x_affine, const float* gy, int64_t ldgy,
                                      int64_t num_rows, const float* knots, int32_t in_features, int32_t out_features,
                                      int32_t grid_size, int32_t spline_order, int32_t mode, const void* pack_dx, void* gx,
                                      int64_t ldgx, int32_t gx_dtype, void* stream);
int kagnn_kan_linear_bwd_weight_affine(const float* x, int64_t ldx, const float* x_affine, const float* gy, int64_t ldgy,
                                       int64_t num_rows, const float* knots, int32_t in_features, int32_t out_features,
                                       int32_t grid_size, int32_t spline_order, int32_t mode, const float* spline_weight,
                                       const float* spline_scaler, float* g_base_weight, float* g_spline_weight,
                                       float* g_spline_scaler, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * The WHOLE graph-regression model per call (round 6; BASELINE config 4).  Replaces, per mini-batch, `KAGIN.forward`
 * of the reference's graph_regression/models.py:107-119 -- `AtomEncoder` / `BondEncoder` embedding sums (:244-281),
 * `n_layers x {GINEConv(KAN) -> BatchNorm1d}` (:98,108-114), `global_add_pool` (:117), the KAN read-out (:118) -- and its
 * autograd backward, called from graph_regression/optuna_zinc.py:56-66.  No new kernels: the call sequences this header's own
 * entry points (kagnn_embedding_fwd, kagnn_gine_kan_stack_fwd, kagnn_segment_pool, kagnn_kan_pack_batch / kagnn_kan_pack,
 * kagnn_kan_linear_fwd; on the way back kagnn_kan_linear_bwd_input / _bwd_weight, kagnn_segment_broadcast,
 * kagnn_gine_kan_stack_bwd, kagnn_embedding_bwd) on `stream` in exactly the order and with exactly the arguments the
 * per-operation host code uses -- same bits.  What it removes is the HOST: a 256-molecule step is ~0.75 ms of device work and
 * the per-operation binding spent as long again in ~19 calls, ~45 allocations and their pointer tables.  Everything the backward
 * needs lives in ONE caller-owned `saved` buffer whose layout only the library knows (kagnn_kagin_model_sizes); all parameter
 * gradients land in ONE flat fp32 buffer `grads`, in the order: atom tables, bond tables, then per convolution bn_weight, bn_bias
 * and per layer base_weight, spline_weight, spline_scaler, then per read-out layer base_weight, spline_weight, spline_scaler
 * (absent scalers take no room).  All fields are 8 bytes wide except the three float arrays at the end.
 * Limits: num_convs * num_layers <= 16, hidden -> hidden chains of width <= 64 on the split path (kagnn_gine_kan_stack_*),
 * <= 8 read-out layers, <= 16 tables per encoder with <= 512 rows, training-mode affine BatchNorm1d, >= 2 nodes.          */
#define KAGNN_MODEL_MAX_LAYERS 16
#define KAGNN_MODEL_MAX_CONVS 16
#define KAGNN_MODEL_MAX_TABLES 16
#define KAGNN_MODEL_MAX_READOUT 8
typedef struct kagnn_kagin_model {
    int64_t num_nodes, num_edges, num_graphs, hidden;
    int64_t num_atom_tables, num_bond_tables, x_stride, e_stride;     /* index matrices: int64 [N, x_stride] / [E, e_stride]; table t reads column t */
    int64_t num_convs, num_layers, grid_size, spline_order, mode;
    int64_t num_readout, readout_grid_size, readout_spline_order;
    int64_t readout_widths[KAGNN_MODEL_MAX_READOUT + 1];               /* hidden, ..., outputs */
    int64_t readout_modes[KAGNN_MODEL_MAX_READOUT];
    int64_t atom_rows[KAGNN_MODEL_MAX_TABLES], bond_rows[KAGNN_MODEL_MAX_TABLES];
    const int64_t* x_index; const int64_t* e_index;
    const float* atom_table[KAGNN_MODEL_MAX_TABLES]; const float* bond_table[KAGNN_MODEL_MAX_TABLES];
    const int32_t* rowptr; const int32_t* col; const int32_t* perm;        /* CSR by destination (kagnn_csr_build_small) */
    const int32_t* rowptr_t; const int32_t* col_t; const int32_t* perm_t;  /* ... and its transpose */
    const int32_t* seg_ptr;                                                /* [num_graphs + 1] node offsets */
    const float* knots;
    const float* base_weight[KAGNN_MODEL_MAX_LAYERS]; const float* spline_weight[KAGNN_MODEL_MAX_LAYERS];
    const float* spline_scaler[KAGNN_MODEL_MAX_LAYERS];
    const float* bn_weight[KAGNN_MODEL_MAX_CONVS]; const float* bn_bias[KAGNN_MODEL_MAX_CONVS];
    float* running_mean[KAGNN_MODEL_MAX_CONVS]; float* running_var[KAGNN_MODEL_MAX_CONVS];      /* NULL: not tracked */
    const float* readout_knots[KAGNN_MODEL_MAX_READOUT];
    const float* readout_base_weight[KAGNN_MODEL_MAX_READOUT]; const float* readout_spline_weight[KAGNN_MODEL_MAX_READOUT];
    const float* readout_spline_scaler[KAGNN_MODEL_MAX_READOUT];      /* NULL entries: no scaler */
    void* saved; int64_t saved_bytes;                                 /* forward writes, backward reads */
    void* workspace; int64_t workspace_bytes;                         /* scratch of the call (forward / backward sizes differ) */
    float* out;                                                       /* forward: [num_graphs, readout_widths[num_readout]] */
    const float* g_out; int64_t ld_g_out;                             /* backward: gradient of `out` */
    float* grads;                                                     /* backward: all parameter gradients, flat */
    float self_scale[KAGNN_MODEL_MAX_CONVS];                          /* 1 + eps of every GINE convolution */
    float momentum[KAGNN_MODEL_MAX_CONVS]; float eps[KAGNN_MODEL_MAX_CONVS];
} kagnn_kagin_model_t;
int kagnn_kagin_model_struct_bytes(void);                             /* sizeof(kagnn_kagin_model_t): a binding checks its mirror */
int kagnn_kagin_model_sizes(const kagnn_kagin_model_t* model, size_t* saved_bytes_host, size_t* fwd_workspace_bytes_host,
                            size_t* bwd_workspace_bytes_host, size_t* grads_floats_host);
int kagnn_kagin_model_fwd(const kagnn_kagin_model_t* model, void* stream);
int kagnn_kagin_model_bwd(const kagnn_kagin_model_t* model, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mini-batch assembly from a DEVICE-RESIDENT dataset of disjoint graphs, one launch per batch.  Replaces, per training step,
 * torch_geometric's DataLoader collation on the host + `data.to(device)` (reference graph_regression/optuna_zinc.py:59-66,
 * graph_classification/graph_classification_utils.py:48-49,109-128) AND the per-batch kagnn_csr_build_small.
 * The dataset is held as "one giant batch in dataset order": graph g owns nodes [node_ptr[g], node_ptr[g+1]) and edges
 * [edge_ptr[g], edge_ptr[g+1]) of the flat arrays (edges grouped by graph, both endpoints inside their own graph -- the
 * caller guarantees it), src_all / dst_all hold node ids in dataset order, and (rowptr_all, col_all, perm_all) /
 * (rowptr_t_all, col_t_all, perm_t_all) are kagnn_csr_build's structures of the WHOLE dataset (by destination / by source; no
 * hub segments are carried over).  A batch = the graphs ids[0..num_graphs) in that order (repeats allowed): per-graph slices of
 * all of those arrays, concatenated, with node and edge offsets rebased.  A stable sort by destination never moves an edge
 * across a graph boundary, so the assembled (rowptr, col, perm, rowptr_t, col_t, perm_t) equal what kagnn_csr_build_small makes
 * from the assembled edge_index, bit for bit.
 *   x_all / edge_attr_all / y_all: opaque rows of x_row_bytes / edge_attr_row_bytes / y_row_bytes bytes (multiples of 4, bases
 *     4-byte aligned; copied with 16-byte accesses where row size and both bases allow, else 8 or 4); edge_attr_all, y_all may
 *     be NULL (row size 0).  The dataset's N and E fit int32.
 *   outputs (caller-allocated): x [num_nodes rows], edge_index [2, num_edges] int64, edge_attr [num_edges rows], y [num_graphs
 *     rows], batch [num_nodes] int64, ptr [num_graphs + 1] int64; rowptr [num_nodes + 1], col, perm, rowptr_t, col_t, perm_t
 *     int32 -- all six (then the dataset's six are required) or all NULL.
 *   num_nodes / num_edges: the batch's totals, which the HOST knows from its copy of node_ptr / edge_ptr.  The kernel scans the
 *     counts itself and verifies them: flags[0] = 1 when an id is outside [0, num_graphs_total), flags[1] = 1 when the scanned
 *     totals differ from num_nodes / num_edges, else 0 -- `flags` is a DEVICE int32[2] the caller reads when convenient (no host
 *     synchronisation here).  On a flagged input nothing is written outside the outputs and every index value written stays
 *     inside the batch (clamped; rows past the scanned totals are empty), so kernels that consume the batch before the flags
 *     are read cannot leave their buffers either; the contents are then meaningless.
 * No workspace.  num_graphs <= KAGNN_BATCH_MAX_GRAPHS: every workgroup scans the batch's counts in LDS (int32 offsets, no
 * pre-pass, no dependency between workgroups); a larger batch is refused with KAGNN_ERR_UNSUPPORTED.
 * struct_bytes = sizeof(kagnn_batch_assemble_t) (checked: KAGNN_ERR_ARG on a mismatch).  All fields are 8 bytes wide.      */
#define KAGNN_BATCH_MAX_GRAPHS 4096
typedef struct kagnn_batch_assemble {
    int64_t struct_bytes;
    int64_t num_graphs_total, num_graphs, num_nodes, num_edges;            /* G of the dataset; B, N, E of this batch */
    int64_t x_row_bytes, edge_attr_row_bytes, y_row_bytes;
    const int64_t* node_ptr; const int64_t* edge_ptr;                      /* [G + 1] each */
    const void* x_all; const void* edge_attr_all; const void* y_all;
    const int64_t* src_all; const int64_t* dst_all;
    const int32_t* rowptr_all; const int32_t* col_all; const int32_t* perm_all;
    const int32_t* rowptr_t_all; const int32_t* col_t_all; const int32_t* perm_t_all;
    const int64_t* ids;                                                    /* [B] */
    void* x; int64_t* edge_index; void* edge_attr; void* y; int64_t* batch; int64_t* ptr;
    int32_t* rowptr; int32_t* col; int32_t* perm; int32_t* rowptr_t; int32_t* col_t; int32_t* perm_t;
    int32_t* flags;                                                        /* [2] */
} kagnn_batch_assemble_t;
int kagnn_batch_assemble_struct_bytes(void);                          /* sizeof(kagnn_batch_assemble_t): a binding checks its mirror */
int kagnn_batch_assemble(const kagnn_batch_assemble_t* a, void* stream);

/* Symbolic fits of edge functions (symbolic.hip; pykan's suggest_symbolic / fit_params, all edges of a layer at once).
 * x [num_rows, in] (row stride ldx), phi [num_rows, out, in] contiguous: the layer's edge functions at those rows, what
 * kagnn_kan_edge_curves / kagnn_fastkan_edge_curves write for t = x.  For every function f of `functions` (HOST int32 ids of
 * the library below), output o and input i the model is  phi_{o,i}(t) ~ c f(a t + b) + d:
 *   params[f, o, i] = (a, b, c, d)     r2[f, o, i]          (f: position in `functions`)
 * Library, argument t in fp32:  0 t   1 t^2   2 t^3   3 t^4   4 1/t   5 1/t^2   6 sqrt(t)   7 1/sqrt(t)   8 exp(t)   9 log(t)
 *   10 |t|   11 sin(t)   12 cos(t)   13 tan(t)   14 tanh(t)   15 sign(t)   16 arctan(t)   17 exp(-t^2)   18 t / (1 + exp(-t)).
 * No singularity protection: a value outside a function's domain is non-finite and falls under the rule.
 * Score of a candidate (a, b) for edge (o, i):  t_n = fmaf(a, x[n,i], b) in fp32, u_n = f(t_n), y_n = phi[n,o,i]; with the
 * means and the centred sums S_uu, S_yy, S_uy:  r2 = S_uy^2 / (S_uu S_yy),  and 0 when the candidate is degenerate: some u_n or
 * one of the sums non-finite, or S_uu / N <= max(1e-5 mean(u^2), 1e-24) (a constant or saturated u, a = 0).  The same
 * threshold on y makes every score of the edge 0.  A non-finite x[n,i] or phi[n,o,i] zeroes the scores of exactly the edges
 * that read it and sets their c, d to NaN; every other edge is bit-equal to a clean run.
 * Search: each axis has Gn = grid_number candidates  v_k = (float)((double)lo + k * ((double)hi - (double)lo) / (Gn - 1));  the
 * best candidate has the largest r2, ties go to the lowest flat index a_id * Gn + b_id.  The zoom is per axis: an interior
 * winner k gives the next range [v_{k-1}, v_{k+1}], k = 0 gives [v_0, v_1], k = Gn - 1 gives [v_{Gn-2}, v_{Gn-1}] (pykan leaves
 * the other axis untouched when one hits the boundary; this does not).  Iteration 1 uses the caller's ranges, later ones
 * per-edge ranges.  (a, b) is the last iteration's winner, c = S_uy / S_uu, d = ybar - c ubar there, r2 its score; if every
 * candidate scored 0: candidate 0, r2 = 0, c = 0, d = ybar.  Deterministic, no atomics.
 * tables / ranges / winners (each may be NULL): every iteration's score table [iterations, F, out, in, Gn, Gn], ranges
 * (a_lo, a_hi, b_lo, b_hi) [iterations, F, out, in, 4] and winning flat index int32 [iterations, F, out, in], written by the
 * same kernels.  Limits: grid_number 3..KAGNN_SYMBOLIC_MAX_GRID, iterations 1..KAGNN_SYMBOLIC_MAX_ITERATIONS, in, out >= 1,
 * in <= 65535; num_rows = 1 makes everything degenerate; num_rows = 0 zero-fills params, r2 and whichever of tables / ranges / winners is given, without a launch.  Nothing
 * beyond `workspace_bytes` of the query is used (the query needs no GPU); nothing of size num_rows x Gn^2 exists. */
#define KAGNN_SYMBOLIC_NUM_FUNCTIONS 19
#define KAGNN_SYMBOLIC_MAX_GRID 128
#define KAGNN_SYMBOLIC_MAX_ITERATIONS 8
int kagnn_symbolic_fit_workspace_bytes(int64_t num_rows, int32_t in_features, int32_t out_features, int32_t num_functions,
                                       size_t* bytes_host);
int kagnn_symbolic_fit(const float* x, int64_t ldx, const float* phi, int64_t num_rows, int32_t in_features, int32_t out_features,
                       const int32_t* functions_host, int32_t num_functions, float a_lo, float a_hi, float b_lo, float b_hi,
                       int32_t grid_number, int32_t iterations, float* params, float* r2, float* tables, float* ranges,
                       int32_t* winners, void* workspace, size_t workspace_bytes, void* stream);

/* Fixed symbolic edges (symbolic_edges.hip; pykan's fix_symbolic): edges of a KANLinear replaced by their formulas, evaluated
 * beside the layer's spline part.  An edge list is E records (o, i, fid) -- output, input, function id of the library above
 * (KAGNN_SYMBOLIC_NUM_FUNCTIONS) -- sorted by (o, i), no pair twice, 0 <= E <= out_features * in_features, with the trainable
 * parameters affine [E, 4] = (a, b, c, d), fp32, contiguous.  All arithmetic is fp32 in every precision mode; no atomics: the
 * same inputs give the same bits, and a row's results do not depend on where the row sits or on num_rows.
 *
 *   t = fmaf(a, x[n,i], b)
 *   s[n,o]   = sum, in list order starting from 0, over the edges of output o, of fmaf(c, f(t), d)
 *   y[n,o]   = y_in[n,o] + s[n,o]     (y_in NULL: y = s; an output without an edge: y_in bit for bit, or 0)
 *   gx[n,i]  = sum, in list order starting from 0, over the edges reading input i, of fmaf(w, a, .),  w = (gy[n,o] * c) * f'(t)
 *              (an input no edge reads: exactly 0; gx NULL: not computed)
 *   g_affine[e] = sums over n of ( w * x[n,i],  w,  gy[n,o] * f(t),  gy[n,o] ): 64 consecutive rows are added in a fixed order,
 *              these sums are added per row slab in row order, and the slabs in index order.
 *
 * f is the library's plain function (sqrt or log outside their domain and 1/x at 0 give what IEEE gives; pykan's
 * singularity-protected variants are deliberately not provided), except that sgn hands a NaN on.  f' is the derivative torch's
 * autograd gives for the same expression: 1, 2t, 3t^2, 4t^3, -1/t^2, -2/t^3, 1/(2 sqrt t), -1/(2 t sqrt t), exp t, 1/t, sgn t
 * (abs: 0 at 0), cos t, -sin t, 1 + tan^2 t, 1 - tanh^2 t, 0 (sgn), 1/(1 + t^2), -2t exp(-t^2), s(1 + t(1 - s)) with
 * s = 1/(1 + exp(-t)) (silu).
 *
 * How the list travels.  kagnn_symbolic_edges_plan validates the HOST list edges_host [E, 3] (int32) once -- range of o, i and
 * fid, the order, duplicates -- and writes a plan of kagnn_symbolic_edges_plan_bytes(E, in, out) bytes into HOST memory.  The
 * caller keeps that block and a byte-for-byte copy of it on the device; forward and backward take both, check the host copy's
 * header against their arguments (nothing else is validated again), read nothing back and do not synchronise.  The plan's
 * words: {magic, E, in, out, 0, 0, 0, 0}, optr[out + 1], records {o, i, fid, 0}, iptr[in + 1], iedge[E] (each array padded to a
 * multiple of 4 words).
 *
 * x [num_rows, in], y_in / y / gy [num_rows, out], gx [num_rows, in]: row-major fp32 with their own leading dimensions; y must
 * not overlap y_in.  E == 0 or num_rows == 0 launch no kernel (y = y_in or 0; gradients 0).  Workspace of the backward:
 * kagnn_symbolic_edges_bwd_workspace_bytes(num_rows, E), a function of its arguments alone (no device needed). */
int kagnn_symbolic_edges_plan_bytes(int64_t num_edges, int32_t in_features, int32_t out_features, size_t* bytes_host);
int kagnn_symbolic_edges_plan(const int32_t* edges_host, int64_t num_edges, int32_t in_features, int32_t out_features,
                              int32_t* plan_host, size_t plan_bytes);
int kagnn_symbolic_edges_bwd_workspace_bytes(int64_t num_rows, int64_t num_edges, size_t* bytes_host);
int kagnn_symbolic_edges_fwd(const float* x, int64_t ldx, int64_t num_rows, int32_t in_features, int32_t out_features,
                             const int32_t* plan_host, const int32_t* plan_dev, const float* affine, const float* y_in,
                             int64_t ldyin, float* y, int64_t ldy, void* stream);
int kagnn_symbolic_edges_bwd(const float* x, int64_t ldx, const float* gy, int64_t ldgy, int64_t num_rows, int32_t in_features,
                             int32_t out_features, const int32_t* plan_host, const int32_t* plan_dev, const float* affine,
                             float* gx, int64_t ldgx, float* g_affine, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KAGNN_HIP_H */
