// What the reference's graph-regression experiment does around its models (graph_regression/optuna_zinc.py:56-92 and
// optuna_qm9.py:56-96, train_model_with_parameters; graph_regression/utils.py: EarlyStopper).  Per batch the scripts take an L1
// loss and read it back (`loss.item() * data.num_graphs`); the QM9 script adds a [1, 12] per-target absolute error, rescaled by the
// targets' standard deviation; per epoch they compare the validation figure with the best one on the host, run the test pass on a
// hit, and ask the stopper.  Here the per-batch loss and the per-target sums are ONE launch that adds to a device record
// (kagnn_l1_loss_meter_fwd), and everything the scripts decide per epoch is one tiny launch on three such records
// (kagnn_regression_epoch_update) -- a loop built from them never has to read anything back.
#include "common.h"
#include "host.h"

namespace kagnn {

constexpr int kRegMaxTargets = KAGNN_REGRESSION_MAX_TARGETS;
struct RegressionMeter { long long graphs; long long targets; double abs_sum[kRegMaxTargets]; };

// ------------------------------------------------------------------ per target: sum over the rows of |p - t|, or |t s - p s| / s
// ONE workgroup of 1024 threads (a mini-batch is at most KAGNN_BATCH_MAX_GRAPHS rows; more rows just loop).  W = the power of two
// >= T (<= 32) lanes share a row, lane l owns column l: with ld == T a wave's loads are consecutive floats.  Group g = tid / W takes
// rows g, g + 1024 / W, ... in that order and adds its column's terms IN DOUBLE (the addends are fp32 values, so the only rounding
// of a sum is fp64's).  The terms are built from separately rounded fp32 operations (__fsub_rn / __fmul_rn / __fdiv_rn: no
// contraction into an FMA), i.e. they are the values torch's elementwise kernels give.  The 1024 / W partial sums of a column fold
// pairwise through LDS with strides that are multiples of W (fixed tree: deterministic); thread 0 then adds the T column sums in
// index order for the mean.  The record is updated with plain loads and stores: launches on one stream are ordered.
__global__ __launch_bounds__(1024) void l1_loss_meter_fwd_kernel(const float* __restrict__ p, long ldp, const float* __restrict__ t,
                                                                 long ldt, long rows, int T, const float* __restrict__ scale,
                                                                 float* __restrict__ loss_mean, RegressionMeter* __restrict__ meter,
                                                                 int W) {
    __shared__ double s_a[1024];
    const int l = threadIdx.x & (W - 1), g = threadIdx.x / W, G = 1024 / W;
    double a = 0.0;
    if (l < T) {
        if (scale) {
            const float s = scale[l];
            for (long r = g; r < rows; r += G)
                a += (double)__fdiv_rn(fabsf(__fsub_rn(__fmul_rn(t[r * ldt + l], s), __fmul_rn(p[r * ldp + l], s))), s);
        } else {
            for (long r = g; r < rows; r += G) a += (double)fabsf(__fsub_rn(p[r * ldp + l], t[r * ldt + l]));
        }
    }
    s_a[threadIdx.x] = a;
    __syncthreads();
    for (int w = 512; w >= W; w >>= 1) {                        // (w is a multiple of W: thread j and j + w own the same column)
        if ((int)threadIdx.x < w) s_a[threadIdx.x] += s_a[threadIdx.x + w];
        __syncthreads();
    }
    if (loss_mean && threadIdx.x == 0) {
        double total = 0.0;
        for (int c = 0; c < T; ++c) total += s_a[c];
        loss_mean[0] = (float)(total / ((double)rows * (double)T));          // no rows: 0 / 0 = NaN, as torch's mean
    }
    if (meter && rows > 0) {
        if ((int)threadIdx.x < T) meter->abs_sum[threadIdx.x] = meter->abs_sum[threadIdx.x] + s_a[threadIdx.x];
        if (threadIdx.x == 0) {
            meter->graphs = meter->graphs + rows;
            meter->targets = T;
        }
    }
}

int l1_loss_meter_fwd(const float* pred, long ldp, const float* target, long ldt, long rows, int T, const float* scale,
                      float* loss_mean, void* meter, hipStream_t st) {
    int W = 1;
    while (W < T) W <<= 1;
    l1_loss_meter_fwd_kernel<<<1, 1024, 0, st>>>(pred, ldp, target, ldt, rows, T, scale, loss_mean, (RegressionMeter*)meter, W);
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

// ------------------------------------------------------------------ the epoch's figures, `best_val_loss >= val_loss`, EarlyStopper
// One workgroup of 64.  Every thread reads `stopped`, `epochs` and the three meters' target counts BEFORE the barrier.  Thread
// t < 32 then owns target t of every split: mae[s][t] = abs_sum[t] / n_s in fp64 (0 for t >= the meter's targets) goes to LDS and,
// while the record still counts, to history[epochs][s][t]; the same thread zeroes abs_sum[t] of every meter, thread 0 their graph
// counts -- nobody reads another thread's element, so a test meter that IS the validation meter needs no care.  After a second
// barrier thread 0 takes each split's figure -- the mae added over the targets in index order, divided by their number, rounded
// once to fp32 -- and advances the record with fp32 comparisons, the scripts' two rules in the scripts' order.
struct RegressionStopState {
    float min_loss, min_delta, best_val, test_at_best;
    int patience, counter, epochs, best_epoch, test_epoch, improved, stopped, pad;
};

__global__ __launch_bounds__(64) void regression_epoch_update_kernel(RegressionMeter* train, RegressionMeter* val,
                                                                     RegressionMeter* test, long n_train, long n_val, long n_test,
                                                                     RegressionStopState* __restrict__ st, double* __restrict__ history,
                                                                     int max_epochs) {
    __shared__ double s_mae[3][kRegMaxTargets];
    RegressionMeter* const meters[3] = {train, val, test};
    const long n[3] = {n_train, n_val, n_test};
    const int stopped = st->stopped, epochs = st->epochs;
    int T[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const long long m = meters[s]->targets;
        T[s] = m < 0 ? 0 : m > kRegMaxTargets ? kRegMaxTargets : (int)m;       // (a record the host filled: never index past it)
    }
    __syncthreads();
    const bool live = !stopped && epochs < max_epochs;
    const int t = threadIdx.x;
    if (t < kRegMaxTargets) {
        double mae[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) mae[s] = t < T[s] ? meters[s]->abs_sum[t] / (double)n[s] : 0.0;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            s_mae[s][t] = mae[s];
            if (live && history) history[((long)epochs * 3 + s) * kRegMaxTargets + t] = mae[s];
            meters[s]->abs_sum[t] = 0.0;
        }
    }
    if (t == 0) {
#pragma unroll
        for (int s = 0; s < 3; ++s) meters[s]->graphs = 0;
    }
    __syncthreads();
    if (t != 0) return;
    if (!live) {
        st->improved = 0;
        return;
    }
    float fig[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        double sum = 0.0;
        for (int c = 0; c < T[s]; ++c) sum += s_mae[s][c];
        fig[s] = (float)(sum / (double)T[s]);                   // no targets (a meter no launch has fed): 0 / 0 = NaN
    }
    const float v = fig[1];
    if (st->best_val >= v) {                                    // optuna_zinc.py:75: a tie takes the test figure again
        st->best_val = v; st->test_at_best = fig[2]; st->test_epoch = epochs;
    }
    const float lo = st->min_loss;
    int improved = 0;
    if (v < lo) {
        st->min_loss = v; st->counter = 0; st->best_epoch = epochs;
        improved = 1;
    } else if (v >= lo + st->min_delta) {
        const int c = st->counter + 1;
        st->counter = c;
        if (c >= st->patience) st->stopped = 1;
    }
    st->improved = improved;
    st->epochs = epochs + 1;
}

int regression_epoch_update(void* train_meter, void* val_meter, void* test_meter, long n_train, long n_val, long n_test, void* state,
                            double* history, int max_epochs, hipStream_t st) {
    if (test_meter == nullptr) { test_meter = val_meter; n_test = n_val; }
    regression_epoch_update_kernel<<<1, 64, 0, st>>>((RegressionMeter*)train_meter, (RegressionMeter*)val_meter,
                                                     (RegressionMeter*)test_meter, n_train, n_val, n_test, (RegressionStopState*)state,
                                                     history, max_epochs);
    KAGNN_LAUNCH_CHECK();
    return KAGNN_OK;
}

}  // namespace kagnn
