/*
 * hq_cumul.h -- the running time integrals of a ground-motion quantity at one point (Arias intensity, cumulative absolute
 * velocity, energy density, and the spans the bracketed and uniform durations are read from): the one definition of the fold
 * that the device trackers (hq_k_cum, hq_outputs.h) and the host route (hqh_cum_fold, hq_host.c) share.  Plain C99 that is
 * also C++17; no HIP, no allocation, no libm; under hipcc the function is __host__ __device__, so kernel and host library
 * compile one text.
 *
 * Per point and quantity (displacement, velocity, acceleration) the state is six doubles and three int32:
 *   sum[0..2] = sum of |v_x|, |v_y|, |v_z|          one addition per sample, in time order
 *   sum[3..5] = sum of v_x v_x, v_y v_y, v_z v_z    the product rounded first, then added: never an FMA
 *   span[0]   = first step at which (v_x v_x + v_y v_y) + v_z v_z > thr2, summed in exactly this order; -1 = never
 *   span[1]   = last such step; -1 = never
 *   span[2]   = number of such samples
 * thr2 is the caller's threshold SQUARED (once, by whoever calls).  The comparison is strict: a sample exactly at the
 * threshold does not count, and a NaN sample never does (no comparison with it holds) -- though it stays in the sums from
 * then on, as in any running sum.  Nothing is multiplied here: the step h of the rectangle rule, pi / 2g and the roots are
 * the caller's, so the sums are those of a plain loop over the samples, bit for bit.  The products and sums must not be
 * contracted: under clang the pragma below sees to it; the host library is compiled without FMA.
 */
#ifndef HQ_CUMUL_H
#define HQ_CUMUL_H

#include <stdint.h>

#if defined(__HIPCC__)
#define HQ_CUM_FN __host__ __device__ static inline
#else
#define HQ_CUM_FN static inline
#endif

enum { HQ_CUM_NSUM = 6, HQ_CUM_NSPAN = 3, HQ_CUM_NCURVE = 3 };   /* NCURVE: the rows of `sum` a Husid slot keeps (3..5) */

/* Fold one sample v = (x, y, z) of one quantity, taken at `step`, into the point's state: sum[j * sstride], j = 0..5, and
 * span[j * wstride], j = 0..2 (stride 1 on the host; the number of points in the device's [6][np] / [3][np] tables).
 * The sums are always written, the span only where the threshold was passed. */
HQ_CUM_FN void hq_cum_fold(double x, double y, double z, int32_t step, double thr2, double* sum, int64_t sstride,
                           int32_t* span, int64_t wstride)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double ax = __builtin_fabs(x), ay = __builtin_fabs(y), az = __builtin_fabs(z);
    const double xx = x * x, yy = y * y, zz = z * z;
    const double h = xx + yy;
    const double t = h + zz;
    sum[0] = sum[0] + ax;
    sum[sstride] = sum[sstride] + ay;
    sum[2 * sstride] = sum[2 * sstride] + az;
    sum[3 * sstride] = sum[3 * sstride] + xx;
    sum[4 * sstride] = sum[4 * sstride] + yy;
    sum[5 * sstride] = sum[5 * sstride] + zz;
    if (t > thr2) {
        const int32_t n = span[2 * wstride];
        if (n == 0) span[0] = step;
        span[wstride] = step;
        span[2 * wstride] = n + 1;
    }
}

#endif
