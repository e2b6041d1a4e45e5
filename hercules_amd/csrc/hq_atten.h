/*
 * hq_atten.h -- BKT constant-Q attenuation (type_of_damping = bkt; calc_conv and constant_Q_addforce, damping.c:110-416):
 * the one text of its arithmetic that the device kernel (hq_k_atten_advance, hq_engine.hip) and the host route
 * (hqh_atten_class_coef / hqh_atten_advance, hq_host.c) compile.  Plain C99 that is also C++17; no HIP, no allocation; under
 * hipcc hq_atten_advance is __host__ __device__.
 *
 * The reference keeps four memory variables per ELEMENT CORNER (conv_shear_1/2, conv_kappa_1/2: [lenum * 8] fvector_t,
 * psolve.c:3322-3325).  The variable of (element e, corner i) is
 *     f <- coef2 u1 + coef1 u2 + exp(-g) f
 * with coefficients that depend on e's ten edata floats only and u1, u2 of node lnid[e][i] only; so does the damping
 * vector coef (u1 - u2) - (a0 f0 + a1 f1) + u1 that enters A D A^T.  Elements with the SAME ten floats that meet at a node
 * therefore carry bit-identical copies, and the state is kept once per (node, class) SLOT, a class being one distinct row
 *     a0_shear, a1_shear, b_shear, g0_shear, g1_shear, a0_kappa, a1_kappa, b_kappa, g0_kappa, g1_kappa
 * (edata_t's order, psolve.h:96: the caller's edata + 4), compared bitwise.
 *
 * Per class the doubles the reference recomputes per element and step are made ONCE on the host (hq_atten_class_coef: the
 * reference's operations in its order, libm's exp), so no transcendental runs on the device.  Per modulus m (0 shear,
 * 1 dilatation) at k[9 m + ..]:
 *     [0] cu1_0 = (g0/2)(1 - g0)   [1] cu2_0 = g0/2   [2] e_0 = exp(-g0)        g0 = (double)row.g0 * rmax
 *     [3] cu1_1 = (g1/2)(1 - g1)   [4] cu2_1 = g1/2   [5] e_1 = exp(-g1)        g1 = (double)row.g1 * rmax
 *     [6] a0   [7] a1   [8] bq = b / rmax                                        rmax = 2 pi freq dt
 * Both branches of the reference fall out of the one formula:
 *   - calc_conv skips a modulus when g0 == 0 || g1 == 0: the class gets cu1 = cu2 = 0 and e = 1 for both variables, and
 *     0 u1 + 0 u2 + 1 f == f for every finite u and every f (a zero variable stays zero, a loaded one stays what it is);
 *   - constant_Q_addforce takes the damping vector = u1 when csum = a0 + a1 + b == 0: the class gets a0 = a1 = bq = 0, and
 *     0 (u1 - u2) - (0 f0 + 0 f1) + u1 == u1 exactly for finite values (x + (+-0) == x; only u1 == -0 comes out +0, which
 *     no sum downstream can tell apart).
 * One skip of the reference is NOT taken: constant_Q_addforce leaves out an element's shear (dilatation) product when all 24
 * values of its damping vector lie within UNDERFLOW_CAP = 1e-20 of zero (vector_is_zero, quake_util.c:49-68), as
 * compute_addforce_effective does for the displacements, and hq_k_element_bkt, like hq_k_element_scatter, multiplies them
 * all the same: a difference of at most 1e-20 times the element's coefficients, ahead of a wave front only.  The memory
 * variables and damping vectors themselves know no such skip.
 * hq_atten_advance is written one IEEE operation per reference operation, contraction off, so memory variables and damping
 * vectors are the reference's bit for bit.
 */
#ifndef HQ_ATTEN_H
#define HQ_ATTEN_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HQ_ATTEN_FN __host__ __device__ static inline
#else
#define HQ_ATTEN_FN static inline
#endif

enum { HQ_ATTEN_NROW = 10,      /* floats of a class row                                                    */
       HQ_ATTEN_NCOEF = 18,     /* doubles of a class (above)                                               */
       HQ_ATTEN_NVAR = 4,       /* memory variables per slot and component: shear 1, 2, dilatation 1, 2     */
       HQ_ATTEN_NSTATE = 12,    /* state rows [var * 3 + component][nslots]                                 */
       HQ_ATTEN_NW = 6 };       /* damping-vector rows: ws x y z, wk x y z                                   */

/* host only: the 18 doubles of a class from its ten floats, Param.theFreq and theDeltaT; -> rmax */
static inline double hq_atten_class_coef(const float* row, double freq, double dt, double* k)
{
    const double rmax = 2. * M_PI * freq * dt;                     /* damping.c:114, :237 */
    for (int m = 0; m < 2; m++) {
        const float* r = row + 5 * m;
        double* q = k + 9 * m;
        if (r[3] != 0 && r[4] != 0) {                              /* damping.c:126, :173 */
            for (int v = 0; v < 2; v++) {
                const double c = r[3 + v];
                const double g = c * rmax;
                const double half = g / 2.;
                q[3 * v + 0] = half * (1. - g);
                q[3 * v + 1] = half;
                q[3 * v + 2] = exp(-g);
            }
        } else {
            for (int v = 0; v < 2; v++) { q[3 * v + 0] = 0.0; q[3 * v + 1] = 0.0; q[3 * v + 2] = 1.0; }
        }
        const double a0 = r[0], a1 = r[1], b = r[2];
        const double csum = a0 + a1 + b;                           /* damping.c:260, :319 */
        if (csum != 0) { q[6] = a0; q[7] = a1; q[8] = b / rmax; }
        else { q[6] = 0.0; q[7] = 0.0; q[8] = 0.0; }
    }
    return rmax;
}

/*
 * One slot, one component: calc_conv's recurrence on the four memory variables f[v * fstride], v = 0..3 (shear 1, 2,
 * dilatation 1, 2), then the two damping vectors of constant_Q_addforce from the NEW variables.  u1, u2: the node's
 * displacement at t and t - dt, widened by the caller; k: the class's 18 doubles.
 */
HQ_ATTEN_FN void hq_atten_advance(double u1, double u2, const double* k, double* f, int64_t fstride, double* ws, double* wk)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double d = u1 - u2;
    double w[2];
    for (int m = 0; m < 2; m++) {
        const double* q = k + 9 * m;
        double* fm = f + 2 * m * fstride;
        const double f0 = (q[0] * u1 + q[1] * u2) + q[2] * fm[0];          /* damping.c:159-161, :206-208 */
        const double f1 = (q[3] * u1 + q[4] * u2) + q[5] * fm[fstride];    /* damping.c:163-165, :210-212 */
        fm[0] = f0;
        fm[fstride] = f1;
        w[m] = (q[8] * d - (q[6] * f0 + q[7] * f1)) + u1;                  /* damping.c:280-290, :340-350 */
    }
    *ws = w[0];
    *wk = w[1];
}

/*
 * The same slot and component in DELTA form (hq_attenuation_set_split): the recurrence above operation for operation, so the
 * memory variables it leaves are hq_atten_advance's bit for bit, and of the damping vectors the part that is not u1 itself,
 *     ds, dk = bq (u1 - u2) - (a0 f0 + a1 f1)        (ws = ds + u1, wk = dk + u1: the final addition is left out).
 * The BKT force is linear in the damping vectors, so mu K_mu ds + kappa K_kappa dk is what attenuation adds to the elastic
 * force of u1.  A class with csum == 0 (a0 = a1 = bq = 0) yields 0 (u1 - u2) - (0 f0 + 0 f1) == +-0: nothing is added.
 */
HQ_ATTEN_FN void hq_atten_advance_delta(double u1, double u2, const double* k, double* f, int64_t fstride, double* ds, double* dk)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double d = u1 - u2;
    double w[2];
    for (int m = 0; m < 2; m++) {
        const double* q = k + 9 * m;
        double* fm = f + 2 * m * fstride;
        const double f0 = (q[0] * u1 + q[1] * u2) + q[2] * fm[0];
        const double f1 = (q[3] * u1 + q[4] * u2) + q[5] * fm[fstride];
        fm[0] = f0;
        fm[fstride] = f1;
        w[m] = q[8] * d - (q[6] * f0 + q[7] * f1);
    }
    *ds = w[0];
    *dk = w[1];
}

#endif /* HQ_ATTEN_H */
