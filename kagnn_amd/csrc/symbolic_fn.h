// The function library of the symbolic fits (symbolic.hip) and of the fixed symbolic edges (symbolic_edges.hip): the 19 functions
// of KAGNN_SYMBOLIC_NUM_FUNCTIONS by id, in fp32 and in fp64, and each function together with its derivative.  The plain
// functions: sqrt or log outside their domain and 1/x at 0 give what IEEE gives (pykan's singularity-protected variants are
// deliberately not here).
#pragma once
#include "common.h"

namespace kagnn {

template <int FID>
__device__ __forceinline__ float sym_fn(float t) {
    if constexpr (FID == 0) return t;
    else if constexpr (FID == 1) return t * t;
    else if constexpr (FID == 2) return t * t * t;
    else if constexpr (FID == 3) { const float q = t * t; return q * q; }
    else if constexpr (FID == 4) return 1.0f / t;
    else if constexpr (FID == 5) return 1.0f / (t * t);
    else if constexpr (FID == 6) return sqrtf(t);
    else if constexpr (FID == 7) return 1.0f / sqrtf(t);
    else if constexpr (FID == 8) return expf(t);
    else if constexpr (FID == 9) return logf(t);
    else if constexpr (FID == 10) return fabsf(t);
    else if constexpr (FID == 11) return sinf(t);
    else if constexpr (FID == 12) return cosf(t);
    else if constexpr (FID == 13) return tanf(t);
    else if constexpr (FID == 14) return tanhf(t);
    else if constexpr (FID == 15) return t > 0.0f ? 1.0f : (t < 0.0f ? -1.0f : 0.0f);
    else if constexpr (FID == 16) return atanf(t);
    else if constexpr (FID == 17) return expf(-(t * t));
    else return t / (1.0f + expf(-t));
}

// the same library in fp64, for the one evaluation per (function, edge) that (c, d) come from: d = ybar - c ubar carries the
// rounding of every u_n times ubar / sigma_u, up to 300 at the degeneracy threshold, which fp32 values of f cannot hold to 2e-5
template <int FID>
__device__ __forceinline__ double sym_fn_d(double t) {
    if constexpr (FID == 0) return t;
    else if constexpr (FID == 1) return t * t;
    else if constexpr (FID == 2) return t * t * t;
    else if constexpr (FID == 3) { const double q = t * t; return q * q; }
    else if constexpr (FID == 4) return 1.0 / t;
    else if constexpr (FID == 5) return 1.0 / (t * t);
    else if constexpr (FID == 6) return sqrt(t);
    else if constexpr (FID == 7) return 1.0 / sqrt(t);
    else if constexpr (FID == 8) return exp(t);
    else if constexpr (FID == 9) return log(t);
    else if constexpr (FID == 10) return fabs(t);
    else if constexpr (FID == 11) return sin(t);
    else if constexpr (FID == 12) return cos(t);
    else if constexpr (FID == 13) return tan(t);
    else if constexpr (FID == 14) return tanh(t);
    else if constexpr (FID == 15) return t > 0.0 ? 1.0 : (t < 0.0 ? -1.0 : 0.0);
    else if constexpr (FID == 16) return atan(t);
    else if constexpr (FID == 17) return exp(-(t * t));
    else return t / (1.0 + exp(-t));
}

// f(t) as sym_fn gives it -- except that sgn hands a NaN on, as every other function does -- and f'(t), the derivative torch's
// autograd gives for the same expression (abs: sgn, 0 at 0; sgn: 0; a NaN argument gives a NaN derivative).  One evaluation of
// the transcendental serves both.
template <int FID>
__device__ __forceinline__ void sym_fn_df(float t, float& f, float& df) {
    if constexpr (FID == 0) { f = t; df = t != t ? t : 1.0f; }
    else if constexpr (FID == 1) { f = t * t; df = 2.0f * t; }
    else if constexpr (FID == 2) { f = t * t * t; df = 3.0f * (t * t); }
    else if constexpr (FID == 3) { const float q = t * t; f = q * q; df = 4.0f * (q * t); }
    else if constexpr (FID == 4) { f = 1.0f / t; df = -(f * f); }
    else if constexpr (FID == 5) { f = 1.0f / (t * t); df = -2.0f * (f / t); }
    else if constexpr (FID == 6) { f = sqrtf(t); df = 0.5f / f; }
    else if constexpr (FID == 7) { f = 1.0f / sqrtf(t); df = -0.5f * (f / t); }
    else if constexpr (FID == 8) { f = expf(t); df = f; }
    else if constexpr (FID == 9) { f = logf(t); df = 1.0f / t; }
    else if constexpr (FID == 10) { f = fabsf(t); df = t > 0.0f ? 1.0f : (t < 0.0f ? -1.0f : (t != t ? t : 0.0f)); }
    else if constexpr (FID == 11) { f = sinf(t); df = cosf(t); }
    else if constexpr (FID == 12) { f = cosf(t); df = -sinf(t); }
    else if constexpr (FID == 13) { f = tanf(t); df = fmaf(f, f, 1.0f); }
    else if constexpr (FID == 14) { f = tanhf(t); df = fmaf(-f, f, 1.0f); }
    else if constexpr (FID == 15) { f = t != t ? t : sym_fn<15>(t); df = t != t ? t : 0.0f; }
    else if constexpr (FID == 16) { f = atanf(t); df = 1.0f / fmaf(t, t, 1.0f); }
    else if constexpr (FID == 17) { f = expf(-(t * t)); df = -2.0f * (t * f); }
    else { const float s = 1.0f / (1.0f + expf(-t)); f = t / (1.0f + expf(-t)); df = s * fmaf(t, 1.0f - s, 1.0f); }
}

}  // namespace kagnn
