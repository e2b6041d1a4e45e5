/*
 * hq_deform.h -- the running peaks of the ground's deformation at one point (strain, strain rate, dynamic stress, rotation
 * and rotation rate): the one definition of the tensors and of their fold that the device trackers (hq_k_deform,
 * hq_outputs.h) and the host route (hqh_deform_fold, hq_host.c) share.  Plain C99 that is also C++17; no HIP, no allocation,
 * no libm; under hipcc the functions are __host__ __device__, so kernel and host library compile one text.
 *
 * The input is the displacement gradient G[b][a] = d u_a / d x_b = sum_c g[b][c] u_a[c] over the eight nodes of the
 * point's element, g the derivatives of the trilinear shape functions (point_strain, nonlinear.c:873-905; the weights:
 * hqh_gradient_weights).  Row b of G is hq_sample_disp (hq_sample.h) with w = g[b]: the sample of a recorder whose phi is
 * g[b], bit for bit.  The rate gradient is hq_sample_disp on u1, hq_sample_vel on u2 with the same weights, / dt: that
 * recorder's velocity column.  A gradient is passed here as nine doubles, G[3 b + a].
 *   strain    e = (xx, yy, zz, xy, yz, xz), the reference's tensor order: xx = G[0][0], yy = G[1][1], zz = G[2][2],
 *             xy = 0.5 (G[1][0] + G[0][1]), yz = 0.5 (G[2][1] + G[1][2]), xz = 0.5 (G[2][0] + G[0][2])
 *   rotation  w = half the curl: wx = 0.5 (G[1][2] - G[2][1]), wy = 0.5 (G[2][0] - G[0][2]), wz = 0.5 (G[0][1] - G[1][0])
 *   stress    of the strain, point_stress's order of operations (nonlinear.c:907-924): mu2 = 2 mu, lkk = lambda ((xx + yy)
 *             + zz), s_aa = mu2 e_aa + lkk, s_ab = mu2 e_ab -- every product rounded first, never an FMA
 * Per point and tensor (strain, strain rate, stress) the state is ten doubles and two int32 (hq_deform_fold):
 *   vals[0..5] = max |xx|, |yy|, |zz|, |xy|, |yz|, |xz|
 *   vals[6]    = max |(xx + yy) + zz|                  the volumetric measure
 *   vals[7]    = max 6 J2 = ((dxy dxy + dyz dyz) + dzx dzx) + 6.0 ((xy xy + yz yz) + xz xz), dxy = xx - yy, dyz = yy - zz,
 *                dzx = zz - xx, summed in exactly this order; the caller divides by 6, or takes sqrt(vals[7] / 2) of the
 *                stress for von Mises
 *   vals[8]    = max hd hd + 4.0 (xy xy), hd = xx - yy  the largest engineering shear in the horizontal plane, SQUARED
 *   vals[9]    = max |xx + yy|                         the areal strain
 *   when[0]    = step at which vals[7] was last raised, when[1] = the same for vals[6]; -1 = never
 * and per vector (rotation, rotation rate) hq_peak.h's five doubles and two int32: tilt (wx, wy) in the horizontal slot,
 * torsion in z.  A value enters only if it is strictly greater: the FIRST occurrence of a maximum is kept, a sample of
 * exactly 0 leaves `when` at -1 (the state starts at 0 / -1), and a NaN never enters (no comparison with it holds).  No root
 * is taken.  Nothing may be contracted: under clang the pragmas below see to it; the host library is compiled without FMA.
 */
#ifndef HQ_DEFORM_H
#define HQ_DEFORM_H

#include <stdint.h>

#include "hq_peak.h"

#if defined(__HIPCC__)
#define HQ_DEFORM_FN __host__ __device__ static inline
#else
#define HQ_DEFORM_FN static inline
#endif

/* the mask of a deformation tracker; the set bits, in this order, are the blocks of a point's state (include/hq_solver.h
 * states the same enumerators behind the same guard) */
#ifndef HQ_DEFORM_QUANTITIES
#define HQ_DEFORM_QUANTITIES
enum { HQ_DEFORM_STRAIN = 1, HQ_DEFORM_STRAIN_RATE = 2, HQ_DEFORM_STRESS = 4, HQ_DEFORM_ROTATION = 8, HQ_DEFORM_ROTATION_RATE = 16 };
#endif

enum { HQ_DEFORM_NVAL = 10, HQ_DEFORM_NWHEN = 2, HQ_DEFORM_ALL = 31 };

/* tensors and vectors of a mask, and the doubles and int32 of a point's state: 10 nt + 5 nv and 2 (nt + nv) */
HQ_DEFORM_FN int32_t hq_deform_nt(int32_t q) { return (q & 1) + ((q >> 1) & 1) + ((q >> 2) & 1); }
HQ_DEFORM_FN int32_t hq_deform_nv(int32_t q) { return ((q >> 3) & 1) + ((q >> 4) & 1); }
HQ_DEFORM_FN int32_t hq_deform_nvals(int32_t q) { return HQ_DEFORM_NVAL * hq_deform_nt(q) + HQ_PEAK_NVAL * hq_deform_nv(q); }
HQ_DEFORM_FN int32_t hq_deform_nwhen(int32_t q) { return HQ_DEFORM_NWHEN * hq_deform_nt(q) + HQ_PEAK_NWHEN * hq_deform_nv(q); }

HQ_DEFORM_FN void hq_deform_strain(const double* G, double* e)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    e[0] = G[0];
    e[1] = G[4];
    e[2] = G[8];
    e[3] = 0.5 * (G[3] + G[1]);
    e[4] = 0.5 * (G[7] + G[5]);
    e[5] = 0.5 * (G[6] + G[2]);
}

HQ_DEFORM_FN void hq_deform_rotation(const double* G, double* w)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    w[0] = 0.5 * (G[5] - G[7]);
    w[1] = 0.5 * (G[6] - G[2]);
    w[2] = 0.5 * (G[1] - G[3]);
}

HQ_DEFORM_FN void hq_deform_stress(const double* e, double lambda, double mu, double* s)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double mu2 = 2 * mu;
    const double lkk = lambda * ((e[0] + e[1]) + e[2]);
    const double m0 = mu2 * e[0], m1 = mu2 * e[1], m2 = mu2 * e[2];
    s[0] = m0 + lkk;
    s[1] = m1 + lkk;
    s[2] = m2 + lkk;
    s[3] = mu2 * e[3];
    s[4] = mu2 * e[4];
    s[5] = mu2 * e[5];
}

/* Fold one tensor t = (xx, yy, zz, xy, yz, xz), taken at `step`, into the point's state: vals[j * vstride], j = 0..9, and
 * when[j * wstride], j = 0..1 (stride 1 on the host; the number of points in the device's [rows][np] tables).  Only what is
 * raised is written. */
HQ_DEFORM_FN void hq_deform_fold(const double* t, int32_t step, double* vals, int64_t vstride, int32_t* when, int64_t wstride)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double xx = t[0], yy = t[1], zz = t[2], xy = t[3], yz = t[4], xz = t[5];
    for (int j = 0; j < 6; j++) {
        const double a = __builtin_fabs(t[j]);
        if (a > vals[j * vstride]) vals[j * vstride] = a;
    }
    const double ar = xx + yy;
    const double vol = __builtin_fabs(ar + zz);
    const double dxy = xx - yy, dyz = yy - zz, dzx = zz - xx;
    const double pxy = xy * xy, pyz = yz * yz, pxz = xz * xz;
    const double qxy = dxy * dxy, qyz = dyz * dyz, qzx = dzx * dzx;
    const double sh = 6.0 * ((pxy + pyz) + pxz);
    const double j2 = ((qxy + qyz) + qzx) + sh;
    const double p4 = 4.0 * pxy;
    const double hs = qxy + p4;                                  /* (hd = dxy) */
    const double area = __builtin_fabs(ar);
    if (vol > vals[6 * vstride]) { vals[6 * vstride] = vol; when[wstride] = step; }
    if (j2 > vals[7 * vstride]) { vals[7 * vstride] = j2; when[0] = step; }
    if (hs > vals[8 * vstride]) vals[8 * vstride] = hs;
    if (area > vals[9 * vstride]) vals[9 * vstride] = area;
}

/* One due sample of a point: G the gradient of the displacement, R that of the velocity (read only with a rate bit), lambda
 * and mu the moduli (read only with HQ_DEFORM_STRESS); every quantity of the mask folded into its block of the state, the
 * blocks in the order of the mask's bits.  Strides as hq_deform_fold's. */
HQ_DEFORM_FN void hq_deform_point(int32_t quantities, const double* G, const double* R, double lambda, double mu, int32_t step,
                                  double* vals, int64_t vstride, int32_t* when, int64_t wstride)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double e[6], t[6], w[3];
    if (quantities & (HQ_DEFORM_STRAIN | HQ_DEFORM_STRESS)) hq_deform_strain(G, e);
    if (quantities & HQ_DEFORM_STRAIN) {
        hq_deform_fold(e, step, vals, vstride, when, wstride);
        vals += HQ_DEFORM_NVAL * vstride; when += HQ_DEFORM_NWHEN * wstride;
    }
    if (quantities & HQ_DEFORM_STRAIN_RATE) {
        hq_deform_strain(R, t);
        hq_deform_fold(t, step, vals, vstride, when, wstride);
        vals += HQ_DEFORM_NVAL * vstride; when += HQ_DEFORM_NWHEN * wstride;
    }
    if (quantities & HQ_DEFORM_STRESS) {
        hq_deform_stress(e, lambda, mu, t);
        hq_deform_fold(t, step, vals, vstride, when, wstride);
        vals += HQ_DEFORM_NVAL * vstride; when += HQ_DEFORM_NWHEN * wstride;
    }
    if (quantities & HQ_DEFORM_ROTATION) {
        hq_deform_rotation(G, w);
        hq_peak_fold(w[0], w[1], w[2], step, vals, vstride, when, wstride);
        vals += HQ_PEAK_NVAL * vstride; when += HQ_PEAK_NWHEN * wstride;
    }
    if (quantities & HQ_DEFORM_ROTATION_RATE) {
        hq_deform_rotation(R, w);
        hq_peak_fold(w[0], w[1], w[2], step, vals, vstride, when, wstride);
    }
}

#endif
