/*
 * hq_sample.h -- one sample of the motion at a point: interpolate_station_displacements' accumulator (psolve.c:6705-6787),
 * the one text that the recorder (hq_k_record), the peak-motion trackers (hq_k_peak; both in hq_outputs.h) and the host route
 * (hqh_station_kinematics, hq_host.c) compile: bit for bit one result.  Plain C99 / C++17; no HIP, no allocation; __host__ __device__ under hipcc.
 * A point has K nodes; w[c] is node c's weight and row[c] the offset of its 3-vector in a field.  w == NULL: weight 1, the
 * form of a point that IS a node (K = 1, no weight table) -- the sums with weights (1, 0, ..., 0) are 0 + u1, - u2, - u2 + u3
 * exactly (1 u is u, and adding 0 u changes nothing).  Every value is widened to double first (HQ_SAMPLE_REAL is the fields'
 * scalar type: double unless the includer says otherwise -- the engine says hq_real).  One accumulator d[3], started at 0 by
 * the caller, passes through the stages, nodes in the outer loop, axes in the inner:
 *   hq_sample_disp   d += w u1                          d        is the displacement
 *   hq_sample_vel    d -= w u2                          d / dt   the velocity (u1 - u2) / dt
 *   hq_sample_acc    d -= w u2, += w u3, node by node   d / dt2  the acceleration (u1 - 2 u2 + u3) / dt^2
 * The products and sums must not be contracted: a pragma sees to it under clang; gcc builds the host library without FMA.
 */
#ifndef HQ_SAMPLE_H
#define HQ_SAMPLE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define HQ_SAMPLE_FN __host__ __device__ static inline
#else
#define HQ_SAMPLE_FN static inline
#endif
#if defined(__clang__)                                       /* first in a function's body: no contraction, loops unrolled */
#define HQ_SAMPLE_STRICT _Pragma("clang fp contract(off)") _Pragma("unroll")
#else
#define HQ_SAMPLE_STRICT
#endif
#ifndef HQ_SAMPLE_REAL
#define HQ_SAMPLE_REAL double
#endif

HQ_SAMPLE_FN void hq_sample_disp(int K, const double* w, const int64_t* row, const HQ_SAMPLE_REAL* u1, double* d)
{
    HQ_SAMPLE_STRICT
    for (int c = 0; c < K; c++)
        for (int a = 0; a < 3; a++) d[a] = d[a] + (w ? w[c] : 1.0) * (double)u1[row[c] + a];
}

HQ_SAMPLE_FN void hq_sample_vel(int K, const double* w, const int64_t* row, const HQ_SAMPLE_REAL* u2, double* d)
{
    HQ_SAMPLE_STRICT
    for (int c = 0; c < K; c++)
        for (int a = 0; a < 3; a++) d[a] = d[a] - (w ? w[c] : 1.0) * (double)u2[row[c] + a];
}

HQ_SAMPLE_FN void hq_sample_acc(int K, const double* w, const int64_t* row, const HQ_SAMPLE_REAL* u2, const HQ_SAMPLE_REAL* u3, double* d)
{
    HQ_SAMPLE_STRICT
    for (int c = 0; c < K; c++)
        for (int a = 0; a < 3; a++) {
            d[a] = d[a] - (w ? w[c] : 1.0) * (double)u2[row[c] + a];
            d[a] = d[a] + (w ? w[c] : 1.0) * (double)u3[row[c] + a];
        }
}

#endif
