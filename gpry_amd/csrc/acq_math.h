// The two finishes the candidate sweep (sweep.hip) and the acquisition ascent (maximize_acq.hip) share, so that both
// compile the same functions: sigma from |V k*|^2, and LogExp.f.
// logexp_value is __host__ __device__ and needs nothing of HIP: the host ranking (kb_rank_core.h) includes this header
// from plain C++, where FinishParams and finish_sd do not exist.
#pragma once
#ifdef __HIPCC__
#include "common.h"
#define GPRY_ACQ_HD __host__ __device__ __forceinline__
#else
#define GPRY_ACQ_HD static inline
#endif
// the register class an empty asm statement pins a double in: a VGPR on the device, an SSE register on an x86-64 host
#if defined(__HIP_DEVICE_COMPILE__)
#define GPRY_ACQ_PIN(x) asm volatile("" : "+v"(x))
#elif defined(__x86_64__)
#define GPRY_ACQ_PIN(x) asm volatile("" : "+x"(x))
#else
#define GPRY_ACQ_PIN(x) asm volatile("" : "+m"(x))
#endif

// LogExp.f on one (mean, std) pair (gpry/acquisition_functions.py:1068-1074): log sqrt(0) = -inf and a
// mean of -inf give -inf, as numpy does under the errstate the reference sets (gp_acquisition.py:1099)
GPRY_ACQ_HD double logexp_value(double y, double sd, double zeta, double baseline, double sigma_n) {
    // std**2 - noise**2 as numpy evaluates it: both squares rounded, then the difference.  Contracted
    // into one FMA the cancellation just above sigma_n moved the result by 1e-9 relative (found by the
    // reference's own F5 edge vectors).  -ffp-contract=fast fuses in the backend whatever the source
    // pragmas say, so the products are pinned behind empty asm statements.
    double s2 = sd * sd, n2 = sigma_n * sigma_n;
    GPRY_ACQ_PIN(s2);
    GPRY_ACQ_PIN(n2);
    double v = s2 - n2;
    if (v < 0.0) v = 0.0;
    double lin = (2.0 * zeta) * (y - baseline);
    GPRY_ACQ_PIN(lin);
    return lin + log(sqrt(v));
}
#ifdef __HIPCC__
// sigma from the sum of squares ss = |V k*|^2; predict_std has no trust-region gate: only the classifier bit zeroes it.
// finish_sd(0.0, ..) is the prior sigma of the bound kernels: the finish sums non-negative per-tile terms (ss >= 0), so
// var = C - ss <= C, and every later step (sqrt, * y_std, and in logexp_value the rounded square, - sigma_n^2, max, log) is
// monotone under round-to-nearest -- the acquisition at the prior sigma is an upper bound of the exact one, bit for bit.
__device__ __forceinline__ double finish_sd(double ss, unsigned mk, const FinishParams& fp) {
    double var = fp.C - ss;
    if (var < 0.0) var = 0.0;
    double sd = sqrt(var) * fp.y_std;
    if (mk & GPRY_MASK_CLASSIFIED_INF) sd = 0.0;
    return sd;
}
#endif
