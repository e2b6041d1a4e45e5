/*
 * hq_nonlin.h -- nonlinear soil at the eight quadrature points of an element: rate-independent von Mises and Drucker-Prager
 * plasticity with linear hardening (nonlinear.c: compute_nonlinear_state :1671-1818, compute_addforce_nl :1544-1657, with
 * compute_dLambdaII, compute_dfds and compute_pstrain2 without dt).  The one text the device kernel (hq_k_nl_element,
 * hq_nonlin_dev.h) and the host route (hqh_nonlinear_advance / hqh_nonlinear_force, hq_host.c) share.  Plain C99 that is also
 * C++17; no HIP, no allocation; under hipcc the functions are __host__ __device__.
 *
 * In a nonlinear element the reference leaves the stiffness force out (stiffness.c:46-105) and applies
 *     -dt^2 sum_qp B^T sigma(e - ep) h^3 / 8
 * instead.  point_stress is linear, so that is the elastic force every step kernel already applies plus the CORRECTION
 *     dF = +dt^2 h^3 / 8 sum_qp B^T sigma(ep),
 * and everything behind the force is linear in it (hq_atten_split.h): the step stays as it is, dF enters beside it.
 *
 * Per quadrature point j (local coordinates xi[.][j] qc, qc = 0.577350269189 and the xi signs the reference's), in the
 * reference's order of operations, every product rounded before it is added (no contraction: the pragmas below under clang;
 * the host library is compiled without FMA), division and sqrt IEEE:
 *   strain   point_strain (:873-897) of the element's eight u(t): node by node from 0, xy += 0.5 (dy ux + dx uy)
 *   trial    s = point_stress(e - ep) (:904-925), I1 = (sxx + syy) + szz, oct = I1 / 3, dev = s - oct on the diagonal,
 *            J2 = ((dxx dxx + dyy dyy) + dzz dzz) 0.5 + dxy dxy + dyz dyz + dxz dxz, Fs = alpha I1 + sqrt(J2)
 *   dLambda  FsT = (Fs - k) - s epb; FsT > 0: FsT / ((mu + ((9 kappa) alpha) alpha) + s phi), else 0, with
 *            kappa = lambda + (2 mu) / 3, phi = sqrt(1/2 + (3 alpha) alpha), s the hardening modulus, epb the point's
 *            effective plastic strain
 *   update   ep_c += dLambda (dev_c / (2 sqrt(J2)) [+ alpha on the diagonal]),  epb += dLambda phi
 * The force of a step uses ep as it stood BEFORE that step's update (the reference's pstrains1).
 *
 * Two rules of the reference:
 *   - an element whose eight nodes are all "zero" (every |component| <= 1e-20: get_displacements :1126-1149,
 *     vector_is_all_zero) is not advanced;
 *   - DEVIATION: where dLambda == 0 the state is KEPT AS IT IS.  The reference adds 0 * dfds, which is the same number
 *     wherever J2 > 0 and NaN where J2 == 0 (0 / 0 in compute_dfds): a rigid translation, or an element at rest beside a
 *     moving node, poisons its plastic strain there.  This text does not reproduce that NaN.
 * A skipped element's correction comes from its current ep (the reference would use the strains and pstrains1 of the step
 * that last advanced it; both are 0 for an element that never moved).
 *
 * State per element: ep (6 values, the reference's tensor order xx yy zz xy yz xz) and epb (1 value) per point, doubles,
 * st[(c * 8 + j) * stride], c = 0..6 -- stride 1 on the host ([7][8] per element), Enlpad on the device ([7][8][Enlpad]).
 * Constants per element cons[c * cstride], c = 0..5: h, mu, lambda, alpha, k, hardening modulus.
 *
 * Not here: rate-dependent plasticity (compute_dLambdaII's pow branch), geostatic loading, gravity and bottom reactions,
 * nonlinear station files and yield statistics; on the device also the scatter variant, the float library, partitions and
 * the reference-link stub (include/hq_solver.h).
 */
#ifndef HQ_NONLIN_H
#define HQ_NONLIN_H

#include <stdint.h>

#if defined(__HIPCC__)
#define HQ_NL_FN __host__ __device__ static inline
#else
#define HQ_NL_FN static inline
#endif

#ifndef HQ_NL_MODELS
#define HQ_NL_MODELS
enum { HQ_NL_VONMISES = 1, HQ_NL_DRUCKERPRAGER = 2 };
#endif

enum { HQ_NL_NSTATE = 7, HQ_NL_NCONS = 6 };

#define HQ_NL_QC 0.577350269189          /* nonlinear.c:32 */
#define HQ_NL_ZERO 1e-20                 /* UNDERFLOW_CAP, quake_util.c:36 */

/* xi[a][i] (nonlinear.c:34-36): -1 or +1 by bit a of i */
HQ_NL_FN double hq_nl_xi(int a, int i) { return ((i >> a) & 1) ? 1.0 : -1.0; }

/* compute_qp_dxi / point_dxi (:802-839): the derivatives of node i's shape function at quadrature point j */
HQ_NL_FN void hq_nl_dxi(int i, int j, double jij, double* dx, double* dy, double* dz)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double lx = hq_nl_xi(0, j) * HQ_NL_QC, ly = hq_nl_xi(1, j) * HQ_NL_QC, lz = hq_nl_xi(2, j) * HQ_NL_QC;
    const double x0 = hq_nl_xi(0, i), x1 = hq_nl_xi(1, i), x2 = hq_nl_xi(2, i);
    const double ax = 1.0 + x0 * lx, ay = 1.0 + x1 * ly, az = 1.0 + x2 * lz;
    *dx = jij * x0 * ay * az;
    *dy = jij * ax * x1 * az;
    *dz = jij * ax * ay * x2;
}

/* point_stress (:904-925) */
HQ_NL_FN void hq_nl_stress(const double* e, double mu, double lambda, double* s)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double kk = (e[0] + e[1]) + e[2];
    const double mu2 = 2.0 * mu;
    const double lkk = lambda * kk;
    const double m0 = mu2 * e[0], m1 = mu2 * e[1], m2 = mu2 * e[2];
    s[0] = m0 + lkk;
    s[1] = m1 + lkk;
    s[2] = m2 + lkk;
    s[3] = mu2 * e[3];
    s[4] = mu2 * e[4];
    s[5] = mu2 * e[5];
}

/* are the element's 24 values all "zero" (get_displacements == 0)? */
HQ_NL_FN int hq_nl_at_rest(const double* u)
{
    int moving = 0;
    for (int q = 0; q < 24; q++) moving |= __builtin_fabs(u[q]) > HQ_NL_ZERO;
    return !moving;
}

/* point j's share of the 24 corner forces of the correction, f[3 i + d] += (B_i^T sigma(p)) h^3 / 8 (compute_addforce_nl's
 * addend, :1619-1629, of the stress of the plastic strain p alone) */
HQ_NL_FN void hq_nl_point_force(int j, double jij, double wj, double mu, double lambda, const double* p, double* f)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double s[6];
    hq_nl_stress(p, mu, lambda, s);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 8; i++) {
        double dx, dy, dz;
        hq_nl_dxi(i, j, jij, &dx, &dy, &dz);
        const double a0 = dx * s[0], a1 = dy * s[3], a2 = dz * s[5];
        const double b0 = dy * s[1], b1 = dx * s[3], b2 = dz * s[4];
        const double c0 = dz * s[2], c1 = dy * s[4], c2 = dx * s[5];
        const double fa = ((a0 + a1) + a2) * wj, fb = ((b0 + b1) + b2) * wj, fc = ((c0 + c1) + c2) * wj;
        f[3 * i + 0] += fa;
        f[3 * i + 1] += fb;
        f[3 * i + 2] += fc;
    }
}

/* point j's state one step on: u the element's 24 values [node][3], p the plastic strain (6) and *epb in place */
HQ_NL_FN void hq_nl_point_advance(int j, double jij, const double* u, double mu, double lambda, double alpha, double k, double hard,
                                  double* p, double* epb)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double t[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 8; i++) {
        double dx, dy, dz;
        hq_nl_dxi(i, j, jij, &dx, &dy, &dz);
        const double ux = u[3 * i], uy = u[3 * i + 1], uz = u[3 * i + 2];
        const double xx = dx * ux, yy = dy * uy, zz = dz * uz;
        const double xy0 = dy * ux, xy1 = dx * uy, yz0 = dz * uy, yz1 = dy * uz, xz0 = dz * ux, xz1 = dx * uz;
        const double xy = 0.5 * (xy0 + xy1), yz = 0.5 * (yz0 + yz1), xz = 0.5 * (xz0 + xz1);
        t[0] += xx; t[1] += yy; t[2] += zz;
        t[3] += xy; t[4] += yz; t[5] += xz;
    }
    double e[6], s[6];
    for (int c = 0; c < 6; c++) e[c] = t[c] - p[c];
    hq_nl_stress(e, mu, lambda, s);
    const double I1 = (s[0] + s[1]) + s[2];
    const double oct = I1 / 3.0;
    const double d0 = s[0] - oct, d1 = s[1] - oct, d2 = s[2] - oct;
    const double q0 = d0 * d0, q1 = d1 * d1, q2 = d2 * d2, q3 = s[3] * s[3], q4 = s[4] * s[4], q5 = s[5] * s[5];
    const double J2 = ((((q0 + q1) + q2) * 0.5 + q3) + q4) + q5;
    const double rJ = __builtin_sqrt(J2);
    const double aI = alpha * I1;
    const double Fs = aI + rJ;
    const double mu23 = (2 * mu) / 3;
    const double kappa = lambda + mu23;
    const double a3 = (3 * alpha) * alpha;
    const double phi = __builtin_sqrt(1 / 2. + a3);
    const double sep = hard * *epb;
    const double FsT = (Fs - k) - sep;
    if (!(FsT > 0)) return;
    const double ka = ((9 * kappa) * alpha) * alpha;
    const double sp = hard * phi;
    const double dL = FsT / ((mu + ka) + sp);
    if (dL == 0) return;                       /* (an underflowed quotient: the state as it is, as for FsT <= 0) */
    const double den = 2.0 * rJ;
    const double g0 = d0 / den + alpha, g1 = d1 / den + alpha, g2 = d2 / den + alpha;
    const double g3 = s[3] / den, g4 = s[4] / den, g5 = s[5] / den;
    const double r0 = dL * g0, r1 = dL * g1, r2 = dL * g2, r3 = dL * g3, r4 = dL * g4, r5 = dL * g5;
    p[0] = p[0] + r0; p[1] = p[1] + r1; p[2] = p[2] + r2;
    p[3] = p[3] + r3; p[4] = p[4] + r4; p[5] = p[5] + r5;
    const double de = dL * phi;
    *epb = *epb + de;
}

/*
 * One element, one step: its 24 corner forces of the correction from the state as it stands, f[3 i + d] =
 * (sum_j share_j) dt^2 -- per corner the points added in order from 0, compute_addforce_nl's order -- and then the state
 * advanced (not where the element is at rest).  u [8][3] = u(t) at the element's nodes; cons and st strided as above.
 */
HQ_NL_FN void hq_nl_element(const double* u, const double* cons, int64_t cstride, double dt2, double* st, int64_t stride, double* f)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double h = cons[0], mu = cons[cstride], lambda = cons[2 * cstride], alpha = cons[3 * cstride], k = cons[4 * cstride],
                 hard = cons[5 * cstride];
    const double jij = 0.25 / h;
    const double h3 = h * h * h;
    const double wj = h3 * 0.125;
    const int rest = hq_nl_at_rest(u);
    for (int q = 0; q < 24; q++) f[q] = 0.0;
    /* the point loop stays a loop on the device: unrolled it needs 286 registers instead of 218 and runs 7 % slower
     * (docs/LABNOTES.md); -DHQ_NL_UNROLL_POINTS builds that form */
#if defined(__HIPCC__) && defined(HQ_NL_UNROLL_POINTS)
#pragma unroll
#elif defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int j = 0; j < 8; j++) {
        double p[6], epb;
        for (int c = 0; c < 6; c++) p[c] = st[(int64_t)(c * 8 + j) * stride];
        epb = st[(int64_t)(6 * 8 + j) * stride];
        hq_nl_point_force(j, jij, wj, mu, lambda, p, f);
        if (!rest) {
            hq_nl_point_advance(j, jij, u, mu, lambda, alpha, k, hard, p, &epb);
            for (int c = 0; c < 6; c++) st[(int64_t)(c * 8 + j) * stride] = p[c];
            st[(int64_t)(6 * 8 + j) * stride] = epb;
        }
    }
    for (int q = 0; q < 24; q++) f[q] = f[q] * dt2;
}

#endif
