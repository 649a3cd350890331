// What the per-edge activation kernels of a KANLinear (kan_edge.hip: local B-spline bases) and of a FastKANLayer
// (fastkan_edge.hip: Gaussian RBFs, dense over the centres) share, none of which depends on the basis: the workgroup shape, the
// row-slab plan, sign(), and the two fixed-order slab reductions (kernels and launchers live in kan_edge.hip).
#pragma once
#include "common.h"

namespace kagnn {

constexpr int kEdgeThreads = 256;      // four waves
constexpr int kEdgeFT = 4;             // features per workgroup (one per wave)
constexpr int kEdgeOB = 64;            // outputs per tile

// torch's sgn for the backward of abs: 0 at 0, NaN stays NaN
__device__ __forceinline__ float edge_sign(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : v); }

// about `want_blocks` workgroups in all, a slab a multiple of 64 rows and never shorter than 256
inline void edge_plan(long N, long tiles, long want_blocks, long* slabs, long* rows_per_slab) {
    const long want = max(1L, want_blocks / max(1L, tiles));
    long r = (N + want - 1) / want;
    r = max(256L, (r + 63) / 64 * 64);
    *rows_per_slab = r;
    *slabs = max(1L, (N + r - 1) / r);
}

inline bool edge_grid_ok(long gx, long gy, long gz) { return gx <= 0x7fffffffL && gy <= 65535 && gz <= 65535; }

inline long edge_tiles(int in, int out) { return (long)cdiv(in, kEdgeFT) * cdiv(out, kEdgeOB); }

// dst[o*ld + f] = sum_s partial[s][o][f], slabs in index order
int edge_sum_reduce(const float* partial, long slabs, int in, int out, float* dst, long ld, hipStream_t st);
// partial[s][f][c][o], c <= C, slabs added in index order, then with g = gS[o*ldgS + f] and e = o*in + f:
//   g_bw[e] = g T_C,   g_sw[e*C + c] = g sc[e] T_c,   g_sc[e] = g sum_c sw[e*C + c] T_c     (sc NULL: 1; NULL outputs: skipped)
int edge_param_reduce(const float* partial, long slabs, int in, int out, int C, const float* gS, long ldgS, const float* sw,
                      const float* sc, float* g_bw, float* g_sw, float* g_sc, hipStream_t st);

}  // namespace kagnn
