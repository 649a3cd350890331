// Fixed symbolic edges of a KANLinear (pykan's fix_symbolic): a sparse list of E edges (o, i, function id) with trainable affine
// parameters (a, b, c, d), evaluated next to the spline part of the layer,
//   y[n,o] = y_in[n,o] + sum over the list's edges (o, i), in list order, of fmaf(c, f(fmaf(a, x[n,i], b)), d),
// and its backward: gx[n,i] and the four parameter gradients per edge, sums over the rows.  include/kagnn_hip.h
// (kagnn_symbolic_edges_fwd) holds the normative formulae.  Exact fp32 in every precision mode, no atomics, the same bits on
// every run; nothing of size N x E or N x out x in exists.
//
// The plan.  The list is validated ONCE, on the host (symbolic_edges_plan), into a block of int32 words that the caller keeps
// twice, on the host and on the device: a header (magic, E, in, out), optr[out + 1] (the list is sorted by (o, i): the edges of
// output o are optr[o] .. optr[o + 1]), the records {o, i, fid, 0} (16 bytes each), iptr[in + 1] and iedge[E] (the edge ids sorted
// by (i, o): the edges reading input i, in list order).  Forward and backward check the host header against their arguments and
// read nothing else; the kernels read the device copy.
//
// Mapping, both kernels: a workgroup is ONE wave and owns 64 consecutive rows, lane = row.  The record, the affine parameters
// and the function id of an edge are then the same for all lanes: they come through uniform loads, the switch over the id is a
// scalar branch without divergence, and every transcendental is evaluated once per (row, edge).  Row tiles travel through LDS
// with coalesced global accesses (16 bytes per lane where the widths, strides and base addresses allow it, else 4), in a
// [column][row] layout whose row index is rotated by the column, word (c, r) at c * 64 + ((r + c) & 63): a lane's own
// accesses (fixed c, r = lane) are conflict-free, and so are the transposing accesses of the tile loads and stores (fixed r,
// consecutive c).
//
//   forward    walks the list as it is, output block by output block (32 outputs: the y tile, 8 KB, loaded from y_in or zeroed,
//              stored once).  x: the whole row tile [in][64] in LDS up to 128 columns (32 KB); wider inputs take the direct
//              variant, each lane loading x[n, i] from global memory (a row's columns share cache lines across the edges).
//   backward   walks the list by input (iedge), column block by column block (32 columns: the x tile, 8 KB).  gx[n,i] of a
//              column is one register over that column's edges; it OVERWRITES x[n,i] in the tile, which is then stored
//              coalesced (columns without an edge: exactly 0).  gy: the whole row tile [out][64] in LDS up to 128 outputs, else
//              direct loads.  The four parameter sums of an edge are per-lane values; 16 edges' worth (64 values x 64 lanes,
//              16 KB of LDS) are reduced at a time, lane v adding the 64 rows of value v in a fixed order, and added to the
//              slab's own partial [slab][E][4] in the workspace -- a workgroup owns a slab of rows and walks its tiles in
//              order, so this is a private read-modify-write, the first tile storing.  A second kernel adds the slabs in
//              index order (the project's slab convention).
#include "common.h"
#include "edge_common.h"
#include "host.h"
#include "symbolic_fn.h"

#include <vector>

namespace kagnn {

constexpr int kSeRows = 64;                   // rows per workgroup (one wave)
constexpr int kSeOB = 32;                     // outputs per y tile of the forward
constexpr int kSeCB = 32;                     // columns per x tile of the backward
constexpr int kSeMaxCols = 128;               // widest whole-row tile (x forward, gy backward) held in LDS
constexpr int kSeBatch = 16;                  // edges per reduction of the parameter sums
constexpr int kSeMagic = 0x53594d45;

// ------------------------------------------------------------------------------------------------------------ the plan
static inline long se_up4(long v) { return (v + 3) / 4 * 4; }
static inline long se_off_optr() { return 8; }
static inline long se_off_rec(int out) { return 8 + se_up4((long)out + 1); }
static inline long se_off_iptr(long E, int out) { return se_off_rec(out) + 4 * E; }
static inline long se_off_iedge(long E, int in, int out) { return se_off_iptr(E, out) + se_up4((long)in + 1); }

size_t symbolic_edges_plan_bytes(long E, int in, int out) { return sizeof(int) * (size_t)(se_off_iedge(E, in, out) + se_up4(E)); }

int symbolic_edges_plan(const int* edges, long E, int in, int out, int* plan) {
    const char* fn = "kagnn_symbolic_edges_plan";
    for (long e = 0; e < E; ++e) {
        const int o = edges[3 * e], i = edges[3 * e + 1], f = edges[3 * e + 2];
        if (o < 0 || o >= out || i < 0 || i >= in) return fail(KAGNN_ERR_ARG, "%s: edge %ld is outside [0, out) x [0, in)", fn, e);
        if (f < 0 || f >= KAGNN_SYMBOLIC_NUM_FUNCTIONS) return fail(KAGNN_ERR_ARG, "%s: edge %ld has an unknown function id (the library has ids 0..18)", fn, e);
        if (e > 0) {
            const int po = edges[3 * e - 3], pi = edges[3 * e - 2];
            if (po == o && pi == i) return fail(KAGNN_ERR_ARG, "%s: edge %ld repeats the pair of the edge before it", fn, e);
            if (po > o || (po == o && pi > i)) return fail(KAGNN_ERR_ARG, "%s: the list is not sorted by (o, i) at edge %ld", fn, e);
        }
    }
    const long words = (long)(symbolic_edges_plan_bytes(E, in, out) / sizeof(int));
    for (long w = 0; w < words; ++w) plan[w] = 0;
    plan[0] = kSeMagic; plan[1] = (int)E; plan[2] = in; plan[3] = out;
    int* optr = plan + se_off_optr();
    int* rec = plan + se_off_rec(out);
    int* iptr = plan + se_off_iptr(E, out);
    int* iedge = plan + se_off_iedge(E, in, out);
    for (long e = 0; e < E; ++e) {
        rec[4 * e] = edges[3 * e]; rec[4 * e + 1] = edges[3 * e + 1]; rec[4 * e + 2] = edges[3 * e + 2];
        ++optr[edges[3 * e] + 1];
        ++iptr[edges[3 * e + 1] + 1];
    }
    for (int o = 0; o < out; ++o) optr[o + 1] += optr[o];
    for (int i = 0; i < in; ++i) iptr[i + 1] += iptr[i];
    // (o ascending within an input: the list order restricted to that input)
    std::vector<int> next(iptr, iptr + in);
    for (long e = 0; e < E; ++e) iedge[next[edges[3 * e + 1]]++] = (int)e;
    return KAGNN_OK;
}

static int se_check_plan(const char* fn, const int* plan_host, int in, int out, long* E) {
    if (!plan_host) return fail(KAGNN_ERR_ARG, "%s: plan_host is null", fn);
    if (plan_host[0] != kSeMagic || plan_host[2] != in || plan_host[3] != out || plan_host[1] < 0 || (long)plan_host[1] > (long)in * out)
        return fail(KAGNN_ERR_ARG, "%s: plan_host is not a plan of kagnn_symbolic_edges_plan for these widths", fn);
    *E = plan_host[1];
    return KAGNN_OK;
}

// ------------------------------------------------------------------------------------------------------------ device helpers
__device__ __forceinline__ int se_at(int c, int r) { return c * kSeRows + ((r + c) & (kSeRows - 1)); }

// tile[c][r] = src[(n0 + r) * ld + c0 + c] for r < nrows, c < w; rows beyond nrows: 0
__device__ __forceinline__ void se_load_tile(float* __restrict__ s, const float* __restrict__ src, long ld, long n0, int nrows, int c0,
                                             int w, bool vec, int lane) {
    if (vec) {
        const int w4 = w >> 2;
        for (int idx = lane; idx < kSeRows * w4; idx += 64) {
            const int r = idx / w4, c = (idx - r * w4) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < nrows) v = *reinterpret_cast<const float4*>(src + (n0 + r) * ld + c0 + c);
            s[se_at(c, r)] = v.x; s[se_at(c + 1, r)] = v.y; s[se_at(c + 2, r)] = v.z; s[se_at(c + 3, r)] = v.w;
        }
    } else {
        for (int idx = lane; idx < kSeRows * w; idx += 64) {
            const int r = idx / w, c = idx - r * w;
            s[se_at(c, r)] = r < nrows ? src[(n0 + r) * ld + c0 + c] : 0.0f;
        }
    }
}

__device__ __forceinline__ void se_store_tile(const float* __restrict__ s, float* __restrict__ dst, long ld, long n0, int nrows, int c0,
                                              int w, bool vec, int lane) {
    if (vec) {
        const int w4 = w >> 2;
        for (int idx = lane; idx < kSeRows * w4; idx += 64) {
            const int r = idx / w4, c = (idx - r * w4) * 4;
            if (r < nrows)
                *reinterpret_cast<float4*>(dst + (n0 + r) * ld + c0 + c) =
                    make_float4(s[se_at(c, r)], s[se_at(c + 1, r)], s[se_at(c + 2, r)], s[se_at(c + 3, r)]);
        }
    } else {
        for (int idx = lane; idx < kSeRows * w; idx += 64) {
            const int r = idx / w, c = idx - r * w;
            if (r < nrows) dst[(n0 + r) * ld + c0 + c] = s[se_at(c, r)];
        }
    }
}

// f(t) and f'(t) of function `fid`, which is the same for all lanes: a scalar branch.  (The forward has no use for f': the
// compiler drops its computation after inlining.)
__device__ __forceinline__ void se_eval(int fid, float t, float& f, float& df) {
    switch (fid) {
        case 0: sym_fn_df<0>(t, f, df); break;
        case 1: sym_fn_df<1>(t, f, df); break;
        case 2: sym_fn_df<2>(t, f, df); break;
        case 3: sym_fn_df<3>(t, f, df); break;
        case 4: sym_fn_df<4>(t, f, df); break;
        case 5: sym_fn_df<5>(t, f, df); break;
        case 6: sym_fn_df<6>(t, f, df); break;
        case 7: sym_fn_df<7>(t, f, df); break;
        case 8: sym_fn_df<8>(t, f, df); break;
        case 9: sym_fn_df<9>(t, f, df); break;
        case 10: sym_fn_df<10>(t, f, df); break;
        case 11: sym_fn_df<11>(t, f, df); break;
        case 12: sym_fn_df<12>(t, f, df); break;
        case 13: sym_fn_df<13>(t, f, df); break;
        case 14: sym_fn_df<14>(t, f, df); break;
        case 15: sym_fn_df<15>(t, f, df); break;
        case 16: sym_fn_df<16>(t, f, df); break;
        case 17: sym_fn_df<17>(t, f, df); break;
        default: sym_fn_df<18>(t, f, df); break;
    }
}
static_assert(KAGNN_SYMBOLIC_NUM_FUNCTIONS == 19, "the switch above lists the library");

// ------------------------------------------------------------------------------------------------------------ forward
// grid (ceil(N / 64)); dynamic LDS: (kSeOB + (XLDS ? in : 0)) * 64 floats
template <bool XLDS>
__global__ __launch_bounds__(kSeRows) void se_fwd_kernel(const float* __restrict__ x, long ldx, long N, int in, int out,
                                                         const int* __restrict__ plan, int off_rec, const float4* __restrict__ affine,
                                                         const float* __restrict__ y_in, long ldyin, float* __restrict__ y, long ldy,
                                                         int vec_x, int vec_yin, int vec_y) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* s_y = smem;                                        // [kSeOB][64]
    float* s_x = smem + kSeOB * kSeRows;                      // [in][64]
    const int lane = threadIdx.x;
    const long n0 = (long)blockIdx.x * kSeRows;
    const int nrows = (int)min((long)kSeRows, N - n0);
    const bool live = lane < nrows;
    const int* optr = plan + 8;
    const int4* rec = reinterpret_cast<const int4*>(plan + off_rec);
    if constexpr (XLDS) se_load_tile(s_x, x, ldx, n0, nrows, 0, in, vec_x != 0, lane);
    const float* xrow = x + (n0 + (live ? lane : 0)) * ldx;

    for (int o0 = 0; o0 < out; o0 += kSeOB) {
        const int oc = min(kSeOB, out - o0);
        const int e0 = optr[o0], e1 = optr[o0 + oc];
        __syncthreads();                                      // the previous tile's store has read s_y
        if (y_in) se_load_tile(s_y, y_in, ldyin, n0, nrows, o0, oc, vec_yin != 0 && (oc & 3) == 0, lane);
        else
            for (int idx = lane; idx < kSeRows * oc; idx += 64) s_y[idx] = 0.0f;
        __syncthreads();
        if (e1 > e0) {
            int cur = rec[e0].x;
            float s = 0.0f;
            for (int e = e0; e < e1; ++e) {
                const int4 r4 = rec[e];
                const float4 p = affine[e];
                if (r4.x != cur) {
                    s_y[se_at(cur - o0, lane)] += s;
                    cur = r4.x;
                    s = 0.0f;
                }
                float xv;
                if constexpr (XLDS) xv = s_x[se_at(r4.y, lane)];
                else xv = live ? xrow[r4.y] : 0.0f;
                float f, df;
                se_eval(r4.z, fmaf(p.x, xv, p.y), f, df);
                s += fmaf(p.z, f, p.w);
            }
            s_y[se_at(cur - o0, lane)] += s;
        }
        __syncthreads();
        se_store_tile(s_y, y, ldy, n0, nrows, o0, oc, vec_y != 0 && (oc & 3) == 0, lane);
    }
}

// ------------------------------------------------------------------------------------------------------------ backward
// values v = slot * 4 + q of the batch, q = (ga, gb, gc, gd): lane v adds the 64 rows of its value and adds the sum to the slab's partial
__device__ __forceinline__ void se_flush(const float* __restrict__ s_red, const int* __restrict__ iedge, int kb, int cnt,
                                         float* __restrict__ part, bool first, int lane) {
    __syncthreads();
    if (lane < cnt * 4) {
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll 4
        for (int r = 0; r < kSeRows; r += 4) {
            a0 += s_red[se_at(lane, r)];
            a1 += s_red[se_at(lane, r + 1)];
            a2 += s_red[se_at(lane, r + 2)];
            a3 += s_red[se_at(lane, r + 3)];
        }
        const float sum = (a0 + a1) + (a2 + a3);
        const long at = (long)iedge[kb + (lane >> 2)] * 4 + (lane & 3);
        part[at] = first ? sum : part[at] + sum;
    }
    __syncthreads();
}

// grid (slabs); dynamic LDS: ((GLDS ? out : 0) + kSeCB + 64) * 64 floats
template <bool GLDS>
__global__ __launch_bounds__(kSeRows) void se_bwd_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ gy, long ldgy,
                                                         long N, int in, int out, const int* __restrict__ plan, int off_rec,
                                                         int off_iptr, int off_iedge, int E, const float4* __restrict__ affine,
                                                         float* __restrict__ gx, long ldgx, float* __restrict__ partial,
                                                         int rows_per_slab, int vec_x, int vec_gy, int vec_gx) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* s_red = smem;                                      // [64 values][64]
    float* s_x = smem + 64 * kSeRows;                         // [kSeCB][64]
    float* s_g = s_x + kSeCB * kSeRows;                       // [out][64]
    const int lane = threadIdx.x;
    const int4* rec = reinterpret_cast<const int4*>(plan + off_rec);
    const int* iptr = plan + off_iptr;
    const int* iedge = plan + off_iedge;
    const long nb = (long)blockIdx.x * rows_per_slab, ne = min(N, nb + rows_per_slab);
    float* part = partial + (long)blockIdx.x * E * 4;
    bool first = true;

    for (long n0 = nb; n0 < ne; n0 += kSeRows) {
        const int nrows = (int)min((long)kSeRows, ne - n0);
        const bool live = lane < nrows;
        const float* grow = gy + (n0 + (live ? lane : 0)) * ldgy;
        __syncthreads();                                      // the previous tile's readers are done
        if constexpr (GLDS) se_load_tile(s_g, gy, ldgy, n0, nrows, 0, out, vec_gy != 0, lane);
        int kb = 0;                                           // first edge (in iedge order) of the open batch
        for (int i0 = 0; i0 < in; i0 += kSeCB) {
            const int ic = min(kSeCB, in - i0);
            const int k0 = iptr[i0], k1 = iptr[i0 + ic];
            if (k1 == k0 && !gx) continue;
            __syncthreads();                                  // the previous block's store has read s_x; s_g is written
            if (k1 > k0) se_load_tile(s_x, x, ldx, n0, nrows, i0, ic, vec_x != 0 && (ic & 3) == 0, lane);
            __syncthreads();
            int k = k0;
            for (int c = 0; c < ic; ++c) {
                const int kend = iptr[i0 + c + 1];
                float g = 0.0f;
                if (k < kend) {
                    const float xv = s_x[se_at(c, lane)];
                    for (; k < kend; ++k) {
                        const int e = iedge[k];
                        const int4 r4 = rec[e];
                        const float4 p = affine[e];
                        float gv;
                        if constexpr (GLDS) gv = s_g[se_at(r4.x, lane)];
                        else gv = live ? grow[r4.x] : 0.0f;
                        float f, df;
                        se_eval(r4.z, fmaf(p.x, xv, p.y), f, df);
                        const float w = (gv * p.z) * df;      // gy c f'(t)
                        g = fmaf(w, p.x, g);
                        const int v = (k - kb) * 4;
                        // (a row beyond the tile is no row: its x is the tile's zero padding, and f of that may be anything)
                        s_red[se_at(v, lane)] = live ? w * xv : 0.0f;
                        s_red[se_at(v + 1, lane)] = live ? w : 0.0f;
                        s_red[se_at(v + 2, lane)] = live ? gv * f : 0.0f;
                        s_red[se_at(v + 3, lane)] = live ? gv : 0.0f;
                        if (k - kb == kSeBatch - 1) {
                            se_flush(s_red, iedge, kb, kSeBatch, part, first, lane);
                            kb = k + 1;
                        }
                    }
                }
                if (gx) s_x[se_at(c, lane)] = g;              // x[n, i] is done with: the tile becomes gx
            }
            if (gx) {
                __syncthreads();
                se_store_tile(s_x, gx, ldgx, n0, nrows, i0, ic, vec_gx != 0 && (ic & 3) == 0, lane);
            }
        }
        if (E > kb) se_flush(s_red, iedge, kb, E - kb, part, first, lane);
        first = false;
    }
}

// g_affine[v] = sum_s partial[s][v], v < E * 4, slabs in index order
__global__ __launch_bounds__(256) void se_reduce_kernel(const float* __restrict__ partial, long slabs, long E4, float* __restrict__ dst) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= E4) return;
    float s = 0.0f;
    for (long sl = 0; sl < slabs; ++sl) s += partial[sl * E4 + v];
    dst[v] = s;
}

// ------------------------------------------------------------------------------------------------------------ host
static void se_slabs(long N, long* slabs, long* rows_per_slab) { edge_plan(N, 1, 1024, slabs, rows_per_slab); }

size_t symbolic_edges_bwd_ws_bytes(long N, long E) {
    long S, r;
    se_slabs(N, &S, &r);
    return sizeof(float) * 4 * (size_t)E * (size_t)S + 16;
}

static inline int se_vec(const void* p, long ld, int w) { return (((uintptr_t)p & 15) == 0 && (ld & 3) == 0 && (w & 3) == 0) ? 1 : 0; }

int symbolic_edges_fwd(const float* x, long ldx, long N, int in, int out, const int* plan_host, const int* plan_dev,
                       const float* affine, const float* y_in, long ldyin, float* y, long ldy, hipStream_t st) {
    long E;
    int rc = se_check_plan("kagnn_symbolic_edges_fwd", plan_host, in, out, &E);
    if (rc) return rc;
    const long blocks = (N + kSeRows - 1) / kSeRows;
    if (blocks > 0x7fffffffL) return fail(KAGNN_ERR_UNSUPPORTED, "%s: too many rows for one launch", "kagnn_symbolic_edges_fwd");
    const bool xlds = in <= kSeMaxCols;
    const size_t lds = sizeof(float) * kSeRows * (size_t)(kSeOB + (xlds ? in : 0));
    const float4* aff = reinterpret_cast<const float4*>(affine);
    const int vx = se_vec(x, ldx, in), vyi = y_in ? se_vec(y_in, ldyin, 4) : 0, vy = se_vec(y, ldy, 4);
    if (xlds)
        se_fwd_kernel<true><<<(unsigned)blocks, kSeRows, lds, st>>>(x, ldx, N, in, out, plan_dev, (int)se_off_rec(out), aff, y_in, ldyin, y, ldy,
                                                                    vx, vyi, vy);
    else
        se_fwd_kernel<false><<<(unsigned)blocks, kSeRows, lds, st>>>(x, ldx, N, in, out, plan_dev, (int)se_off_rec(out), aff, y_in, ldyin, y,
                                                                     ldy, vx, vyi, vy);
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

int symbolic_edges_bwd(const float* x, long ldx, const float* gy, long ldgy, long N, int in, int out, const int* plan_host,
                       const int* plan_dev, const float* affine, float* gx, long ldgx, float* g_affine, void* ws, size_t ws_bytes,
                       hipStream_t st) {
    long E;
    int rc = se_check_plan("kagnn_symbolic_edges_bwd", plan_host, in, out, &E);
    if (rc) return rc;
    if (ws_bytes < symbolic_edges_bwd_ws_bytes(N, E)) return fail(KAGNN_ERR_ARG, "%s: workspace too small", "kagnn_symbolic_edges_bwd");
    long S, r;
    se_slabs(N, &S, &r);
    char* p = static_cast<char*>(ws);
    p += (16 - ((uintptr_t)p & 15)) & 15;                    // (the 16 spare bytes of the size cover this)
    float* partial = reinterpret_cast<float*>(p);
    const bool glds = out <= kSeMaxCols;
    const size_t lds = sizeof(float) * kSeRows * (size_t)(64 + kSeCB + (glds ? out : 0));
    const float4* aff = reinterpret_cast<const float4*>(affine);
    const int vx = se_vec(x, ldx, 4), vg = se_vec(gy, ldgy, out), vgx = gx ? se_vec(gx, ldgx, 4) : 0;
    const int oi = (int)se_off_iptr(E, out), oe = (int)se_off_iedge(E, in, out);
    if (glds)
        se_bwd_kernel<true><<<(unsigned)S, kSeRows, lds, st>>>(x, ldx, gy, ldgy, N, in, out, plan_dev, (int)se_off_rec(out), oi, oe, (int)E, aff, gx,
                                                               ldgx, partial, (int)r, vx, vg, vgx);
    else
        se_bwd_kernel<false><<<(unsigned)S, kSeRows, lds, st>>>(x, ldx, gy, ldgy, N, in, out, plan_dev, (int)se_off_rec(out), oi, oe, (int)E, aff, gx,
                                                                ldgx, partial, (int)r, vx, vg, vgx);
    KAGNN_LAUNCH_CHECK();
    const long E4 = E * 4;
    se_reduce_kernel<<<(unsigned)((E4 + 255) / 256), 256, 0, st>>>(partial, S, E4, g_affine);
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

}  // namespace kagnn
