/*
 * hq_peak.h -- the running peak of a ground-motion quantity at one point: the one definition of the fold that the device
 * trackers (hq_k_peak, hq_engine.hip) and the host route (hqh_peak_fold, hq_host.c) share.  Plain C99 that is also C++17;
 * no HIP, no allocation; under hipcc the functions are __host__ __device__, so kernel and host library compile one text.
 *
 * Per point and quantity (displacement, velocity, acceleration) the state is five doubles and two int32:
 *   pk[0..2] = max |v_x|, |v_y|, |v_z|
 *   pk[3]    = max (v_x v_x + v_y v_y)               horizontal, SQUARED (z is depth)
 *   pk[4]    = max (v_x v_x + v_y v_y) + v_z v_z     total, SQUARED, summed in exactly this order
 *   when[0]  = step at which pk[3] was last raised, when[1] = the same for pk[4]; -1 = never
 * A value enters only if it is strictly greater: the FIRST occurrence of a maximum is kept, a sample of exactly 0 leaves
 * `when` at -1 (the state starts at 0 / -1), and a NaN never enters (no comparison with it holds).  The squares stay
 * squared -- no root is taken here, the caller takes sqrt -- and the sums must not be contracted: x x + y y as an FMA
 * differs in the last bit.  Under clang the pragma below sees to it; the host library is compiled without FMA.
 */
#ifndef HQ_PEAK_H
#define HQ_PEAK_H

#include <stdint.h>

#if defined(__HIPCC__)
#define HQ_PEAK_FN __host__ __device__ static inline
#else
#define HQ_PEAK_FN static inline
#endif

enum { HQ_PEAK_NVAL = 5, HQ_PEAK_NWHEN = 2, HQ_PEAK_NQ = 3 };

/* set bits of a quantity mask (HQ_PEAK_DISP | _VEL | _ACC = 1 | 2 | 4): the quantities a state holds, in that order */
HQ_PEAK_FN int32_t hq_peak_nq(int32_t quantities) { return (quantities & 1) + ((quantities >> 1) & 1) + ((quantities >> 2) & 1); }

/* what a recorder must deliver for the mask: derivs of hq_recorder_desc (0 displacement, 1 + velocity, 2 + acceleration) */
HQ_PEAK_FN int32_t hq_peak_derivs(int32_t quantities) { return (quantities & 4) ? 2 : (quantities & 2) ? 1 : 0; }

/* Fold one sample v = (x, y, z) of one quantity, taken at `step`, into the point's state: pk[j * pstride], j = 0..4, and
 * when[j * wstride], j = 0..1 (stride 1 on the host; the number of points in the device's [5][np] / [2][np] tables).
 * Only what is raised is written. */
HQ_PEAK_FN void hq_peak_fold(double x, double y, double z, int32_t step, double* pk, int64_t pstride, int32_t* when,
                             int64_t wstride)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double ax = __builtin_fabs(x), ay = __builtin_fabs(y), az = __builtin_fabs(z);
    const double xx = x * x, yy = y * y, zz = z * z;
    const double h = xx + yy;
    const double t = h + zz;
    if (ax > pk[0]) pk[0] = ax;
    if (ay > pk[pstride]) pk[pstride] = ay;
    if (az > pk[2 * pstride]) pk[2 * pstride] = az;
    if (h > pk[3 * pstride]) { pk[3 * pstride] = h; when[0] = step; }
    if (t > pk[4 * pstride]) { pk[4 * pstride] = t; when[wstride] = step; }
}

#endif
