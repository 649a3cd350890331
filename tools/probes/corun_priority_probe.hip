// How fast does the co-run row kernel of the backward's transposed aggregation (agg_rows_v4_corun_kernel<16>, csrc/aggregate.hip)
// gather beside the weight gradients, and what changes that?  The set-up of profiles/bwd_overlap.md section 1, rebuilt: the row
// kernel over ALL rows of the headline's transposed graph (N = 1M, E = 10M by the benchmark's power-law recipe: rows = sources,
// uniform; columns = destinations, skewed), 16 lanes per row, launched with the 40 000 B dynamic-LDS request that holds it to four
// workgroups per CU = four waves per SIMD -- alone, beside one and beside two kagnn_kan_linear_bwd_weight calls (64 -> 64, grid 5,
// order 3, split mode) on a second stream, fork and join by events.  Median of 12 launches per cell.
//   loop "parent": the gather loop the kernel had (indices, then rows, per step of four; one edge at a time for the last 1..3)
//   loop "lean"  : lean_gather as it is in the library now (restated here: the probe links the library for the weight gradient only)
//   prio k       : one s_setprio k at the kernel's entry
// Per cell: the pair's time, the time the weight gradients end, the time the row kernel ends (all from the fork, ms), and the share
// of the rows that were done when the weight gradients ended, estimated as 1 - (row kernel's end - weight gradients' end) / (the
// same kernel's time alone under the same cap).  Also checks that both loops give the same bits.  Prints the table and exits.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -o tools/probes/bin/corun_priority_probe \
//         tools/probes/corun_priority_probe.hip -L kagnn_amd/lib -lkagnn_hip -Wl,-rpath,'$ORIGIN/../../../kagnn_amd/lib'
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>
#include "kagnn_hip.h"

#define HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)
#define LIB(x) do { int r_ = (x); if (r_) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, kagnn_last_error()); exit(1); } } while (0)

constexpr int F = 64, LPR = 16;
constexpr unsigned kLds = 40000;        // host.h: kAggCorunLds

struct Args { const float* x; long ldx; float* out; long ldo; const int* rowptr; const int* col; long N; float self_scale; };

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void add4(float4& a, const float4& v) { a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }

__device__ __forceinline__ void parent_gather(float4& acc, const Args& a, int c4, int s, int t) {
    int e = s;
    for (; e + 4 <= t; e += 4) {
        const int j0 = a.col[e], j1 = a.col[e + 1], j2 = a.col[e + 2], j3 = a.col[e + 3];
        const float4 v0 = ld4(a.x + (long)j0 * a.ldx + c4);
        const float4 v1 = ld4(a.x + (long)j1 * a.ldx + c4);
        const float4 v2 = ld4(a.x + (long)j2 * a.ldx + c4);
        const float4 v3 = ld4(a.x + (long)j3 * a.ldx + c4);
        add4(acc, v0); add4(acc, v1); add4(acc, v2); add4(acc, v3);
    }
    for (; e < t; ++e) add4(acc, ld4(a.x + (long)a.col[e] * a.ldx + c4));
}

__device__ __forceinline__ void lean_gather(float4& acc, const float* xc, unsigned ldb, const int* __restrict__ col, int s, int t) {
    auto row = [&](int j) { return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(xc) + (unsigned long)(unsigned)j * ldb); };
    if (s >= t) return;
    const int* cp = col + s;
    int n = (t - s) >> 2;
    const int r = (t - s) & 3;
    int j0 = 0, j1 = 0, j2 = 0, j3 = 0;
    if (n > 0) { j0 = cp[0]; j1 = cp[1]; j2 = cp[2]; j3 = cp[3]; }
    else { j0 = cp[0]; if (r > 1) j1 = cp[1]; if (r > 2) j2 = cp[2]; }
    while (n > 0) {
        const float4 v0 = row(j0);
        asm volatile("" : "+v"(j1) : : "memory");
        const float4 v1 = row(j1);
        asm volatile("" : "+v"(j2) : : "memory");
        const float4 v2 = row(j2);
        asm volatile("" : "+v"(j3) : : "memory");
        const float4 v3 = row(j3);
        asm volatile("" : : : "memory");
        cp += 4;
        --n;
        if (n > 0) { j0 = cp[0]; j1 = cp[1]; j2 = cp[2]; j3 = cp[3]; }
        else if (r > 0) { j0 = cp[0]; if (r > 1) j1 = cp[1]; if (r > 2) j2 = cp[2]; }
        add4(acc, v0); add4(acc, v1); add4(acc, v2); add4(acc, v3);
    }
    const float4 none = make_float4(-0.0f, -0.0f, -0.0f, -0.0f);
    float4 v0 = none, v1 = none, v2 = none;
    if (r > 0) v0 = row(j0);
    if (r > 1) v1 = row(j1);
    if (r > 2) v2 = row(j2);
    add4(acc, v0); add4(acc, v1); add4(acc, v2);
}

template <bool LEAN, int PRIO>
__global__ __launch_bounds__(256) void rows_kernel(Args a) {
    if constexpr (PRIO > 0) __builtin_amdgcn_s_setprio(PRIO);
    const unsigned wg = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);      // one contiguous eighth per XCD, as the library
    const long gid = (wg * 256L + threadIdx.x) / LPR;
    const int c4 = (threadIdx.x % LPR) * 4;
    if (gid >= a.N) return;
    const int s = a.rowptr[gid], t = a.rowptr[gid + 1];
    float4 acc = ld4(a.x + gid * a.ldx + c4);
    acc.x *= a.self_scale; acc.y *= a.self_scale; acc.z *= a.self_scale; acc.w *= a.self_scale;
    if constexpr (LEAN) lean_gather(acc, a.x + c4, (unsigned)a.ldx * 4u, a.col, s, t);
    else parent_gather(acc, a, c4, s, t);
    *reinterpret_cast<float4*>(a.out + gid * a.ldo + c4) = acc;
}

typedef void (*RowsKernel)(Args);
struct Variant { const char* name; RowsKernel k; };
static const Variant kVariants[] = {
    {"parent prio 0", rows_kernel<false, 0>}, {"parent prio 1", rows_kernel<false, 1>}, {"parent prio 2", rows_kernel<false, 2>},
    {"parent prio 3", rows_kernel<false, 3>}, {"lean   prio 0", rows_kernel<true, 0>},  {"lean   prio 1", rows_kernel<true, 1>},
    {"lean   prio 2", rows_kernel<true, 2>},  {"lean   prio 3", rows_kernel<true, 3>},
};

static float median(std::vector<float> v) { std::sort(v.begin(), v.end()); return 0.5f * (v[(v.size() - 1) / 2] + v[v.size() / 2]); }

int main() {
    const long N = 1000000, E = 10000000;
    const int G = 5, K = 3, C = G + K;
    // the benchmark's recipe (bench.py: powerlaw_graph), transposed: row = source (uniform), column = destination perm[floor(N u^2)]
    std::mt19937_64 rng(0);
    std::vector<int> perm(N);
    std::iota(perm.begin(), perm.end(), 0);
    std::shuffle(perm.begin(), perm.end(), rng);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::vector<int> src(E), dst(E), rowptr(N + 1, 0), col(E);
    for (long e = 0; e < E; ++e) {
        const double u = U(rng);
        dst[e] = perm[std::min<long>((long)std::floor(N * u * u), N - 1)];
        src[e] = (int)(rng() % (unsigned long)N);
        ++rowptr[src[e] + 1];
    }
    int maxdeg = 0;
    for (long i = 0; i < N; ++i) { maxdeg = std::max(maxdeg, rowptr[i + 1]); rowptr[i + 1] += rowptr[i]; }
    { std::vector<int> fill(rowptr.begin(), rowptr.end() - 1); for (long e = 0; e < E; ++e) col[fill[src[e]]++] = dst[e]; }
    std::vector<float> hx((size_t)N * F), hg((size_t)N * F);
    std::uniform_real_distribution<float> Ux(-1.0f, 1.0f);
    for (auto& v : hx) v = Ux(rng);
    for (auto& v : hg) v = Ux(rng);
    std::vector<float> hknots(G + 2 * K + 1), hsw((size_t)F * F * C), hsc((size_t)F * F);
    for (int i = 0; i < G + 2 * K + 1; ++i) hknots[i] = -1.0f + (i - K) * (2.0f / G);
    for (auto& v : hsw) v = 0.1f * Ux(rng);
    for (auto& v : hsc) v = 1.0f + 0.1f * Ux(rng);

    float *x, *g, *out, *ref, *knots, *sw, *sc, *gbw, *gsw, *gsc;
    int *d_rowptr, *d_col;
    void* dws;
    size_t dws_bytes = 0;
    LIB(kagnn_kan_bwd_weight_workspace_bytes(N, F, F, G, K, KAGNN_PREC_SPLIT, &dws_bytes));
    HIP(hipMalloc(&x, hx.size() * 4)); HIP(hipMalloc(&g, hg.size() * 4)); HIP(hipMalloc(&out, hx.size() * 4)); HIP(hipMalloc(&ref, hx.size() * 4));
    HIP(hipMalloc(&knots, hknots.size() * 4)); HIP(hipMalloc(&sw, hsw.size() * 4)); HIP(hipMalloc(&sc, hsc.size() * 4));
    HIP(hipMalloc(&gbw, hsc.size() * 4)); HIP(hipMalloc(&gsw, hsw.size() * 4)); HIP(hipMalloc(&gsc, hsc.size() * 4));
    HIP(hipMalloc(&d_rowptr, rowptr.size() * 4)); HIP(hipMalloc(&d_col, col.size() * 4)); HIP(hipMalloc(&dws, dws_bytes));
    HIP(hipMemcpy(x, hx.data(), hx.size() * 4, hipMemcpyHostToDevice)); HIP(hipMemcpy(g, hg.data(), hg.size() * 4, hipMemcpyHostToDevice));
    HIP(hipMemcpy(knots, hknots.data(), hknots.size() * 4, hipMemcpyHostToDevice));
    HIP(hipMemcpy(sw, hsw.data(), hsw.size() * 4, hipMemcpyHostToDevice)); HIP(hipMemcpy(sc, hsc.data(), hsc.size() * 4, hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_rowptr, rowptr.data(), rowptr.size() * 4, hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_col, col.data(), col.size() * 4, hipMemcpyHostToDevice));

    hipStream_t st, side;
    HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking)); HIP(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
    hipEvent_t e0, e_dw, e_agg, e1;
    HIP(hipEventCreate(&e0)); HIP(hipEventCreate(&e_dw)); HIP(hipEventCreate(&e_agg)); HIP(hipEventCreate(&e1));
    const unsigned grid = (unsigned)(((N * LPR + 255) / 256 + 7) / 8 * 8);
    const Args a{x, F, out, F, d_rowptr, d_col, N, 1.0f};
    printf("transposed graph: N %ld  E %ld  maximum degree %d; row kernel grid %u x 256\n", N, E, maxdeg, grid);

    // the pair: fork, n_dw weight gradients on the side stream, the row kernel on this one, join
    auto pair = [&](RowsKernel k, unsigned lds, int n_dw, float* t_dw, float* t_agg, float* t_pair) {
        HIP(hipEventRecord(e0, st));
        HIP(hipStreamWaitEvent(side, e0, 0));
        for (int i = 0; i < n_dw; ++i)
            LIB(kagnn_kan_linear_bwd_weight(x, F, g, F, N, knots, F, F, G, K, KAGNN_PREC_SPLIT, sw, sc, gbw, gsw, gsc, dws, dws_bytes, side));
        HIP(hipEventRecord(e_dw, side));
        k<<<grid, 256, lds, st>>>(a);
        HIP(hipGetLastError());
        HIP(hipEventRecord(e_agg, st));
        HIP(hipStreamWaitEvent(st, e_dw, 0));
        HIP(hipEventRecord(e1, st));
        HIP(hipStreamSynchronize(st));
        HIP(hipEventElapsedTime(t_dw, e0, e_dw)); HIP(hipEventElapsedTime(t_agg, e0, e_agg)); HIP(hipEventElapsedTime(t_pair, e0, e1));
    };
    auto cell = [&](RowsKernel k, unsigned lds, int n_dw, float* dw, float* agg, float* pr) {
        std::vector<float> a_(12), b_(12), c_(12);
        float t0, t1, t2;
        for (int w = 0; w < 2; ++w) pair(k, lds, n_dw, &t0, &t1, &t2);
        for (int i = 0; i < 12; ++i) pair(k, lds, n_dw, &a_[i], &b_[i], &c_[i]);
        *dw = median(a_); *agg = median(b_); *pr = median(c_);
    };

    // same bits from both loops
    rows_kernel<false, 0><<<grid, 256, 0, st>>>(Args{x, F, ref, F, d_rowptr, d_col, N, 1.0f});
    rows_kernel<true, 0><<<grid, 256, 0, st>>>(a);
    HIP(hipGetLastError());
    HIP(hipStreamSynchronize(st));
    {
        std::vector<float> h0(hx.size()), h1(hx.size());
        HIP(hipMemcpy(h0.data(), ref, h0.size() * 4, hipMemcpyDeviceToHost)); HIP(hipMemcpy(h1.data(), out, h1.size() * 4, hipMemcpyDeviceToHost));
        printf("lean loop against parent loop: %s\n", memcmp(h0.data(), h1.data(), h0.size() * 4) == 0 ? "same bits" : "BITS DIFFER");
    }
    float dw, agg, pr;
    cell(rows_kernel<false, 0>, 0, 0, &dw, &agg, &pr);
    const float parent_free = agg;
    cell(rows_kernel<true, 0>, 0, 0, &dw, &agg, &pr);
    printf("alone, no cap (8 waves per SIMD): parent %.3f  lean %.3f\n", parent_free, agg);
    printf("\n%-14s | %-8s | %-33s | %-33s\n", "row kernel", "alone", "beside 1 weight gradient", "beside 2 weight gradients");
    printf("%-14s | %-8s | %-33s | %-33s\n", "(40 000 B cap)", "ms", "  pair  dW end  rows end  done", "  pair  dW end  rows end  done");
    for (const Variant& v : kVariants) {
        float alone;
        cell(v.k, kLds, 0, &dw, &alone, &pr);
        printf("%-14s | %8.3f |", v.name, alone);
        for (int n_dw = 1; n_dw <= 2; ++n_dw) {
            cell(v.k, kLds, n_dw, &dw, &agg, &pr);
            const float done = agg <= dw ? 1.0f : 1.0f - (agg - dw) / alone;
            printf(" %6.3f %6.3f %8.3f %5.0f%%    |", pr, dw, agg, 100.0f * done);
        }
        printf("\n");
    }
    // the weight gradients alone, for the serial sum
    {
        std::vector<float> one(12), two(12);
        for (int i = 0; i < 12; ++i) {
            float t0, t1;
            HIP(hipEventRecord(e0, side));
            LIB(kagnn_kan_linear_bwd_weight(x, F, g, F, N, knots, F, F, G, K, KAGNN_PREC_SPLIT, sw, sc, gbw, gsw, gsc, dws, dws_bytes, side));
            HIP(hipEventRecord(e_dw, side));
            LIB(kagnn_kan_linear_bwd_weight(x, F, g, F, N, knots, F, F, G, K, KAGNN_PREC_SPLIT, sw, sc, gbw, gsw, gsc, dws, dws_bytes, side));
            HIP(hipEventRecord(e1, side));
            HIP(hipStreamSynchronize(side));
            HIP(hipEventElapsedTime(&t0, e0, e_dw)); HIP(hipEventElapsedTime(&t1, e0, e1));
            one[i] = t0; two[i] = t1;
        }
        printf("\nweight gradients alone: one %.3f  two %.3f\n", median(one), median(two));
    }
    return 0;
}
