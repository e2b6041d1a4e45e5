/*
 * hq_sdof.h -- the damped single-degree-of-freedom oscillator of a response spectrum: the one text that the device trackers
 * (hq_k_spec, hq_outputs.h) and the host route (hqh_sdof_coef / hqh_spec_fold, hq_host.c) compile.  Plain C99 that is also
 * C++17; no HIP, no allocation, no libm; under hipcc the functions are __host__ __device__.
 *
 *   x'' + 2 zeta omega x' + omega^2 x = -a_g(t),  omega = 2 pi / T,
 * a_g piecewise linear between samples spaced h apart (Nigam & Jennings 1969).  Per point, period and axis the state is
 * (x, v); the step from sample a0 to sample a1 is exact for that input:
 *   x' = ((A11 x + A12 v) + B11 a0) + B12 a1
 *   v' = ((A21 x + A22 v) + B21 a0) + B22 a1
 * c[8] = {A11, A12, A21, A22, B11, B12, B21, B22}.
 *
 * The textbook closed form of the eight coefficients cancels catastrophically at a simulation's time step (omega h << 1:
 * 2e-5 relative at T = 10 s, h = 3e-4 s), so hq_sdof_coef does not use it.  In the non-dimensional time tau = t / h the
 * vector y = (x, h v, h^2 a, h^2 (a1 - a0)) obeys y' = M y with the constant matrix
 *        |  0      1     0   0 |
 *   M =  | -w^2  -2 z w  -1   0 |      w = omega h,  z = zeta
 *        |  0      0     0   1 |
 *        |  0      0     0   0 |
 * and the step is y(1) = exp(M) y(0).  exp(M) is formed by scaling and squaring: M / 2^s with s the least integer that
 * brings the row-sum norm 1 + 2 z w + w^2 to 1/2 or below (s >= 1), HQ_SDOF_TERMS Taylor terms (0.5^18 / 18! = 6e-22),
 * s squarings.  Additions, multiplications and divisions only, in a fixed order, without contraction: the result does not
 * depend on the compiler or on a libm.  For w << 1 every entry's series is led by its first term and the squarings add
 * terms of one sign, so each coefficient keeps its RELATIVE accuracy (tests/test_spectra_cpu.py: 1e-14 against 60 digits).
 * Host only in practice: once per period at hq_spec_add, and for the host fold.
 *
 * The spectrum state of a point and a period: osc = x[3] then v[3], and
 *   sd[0..2] = max |x_x|, |x_y|, |x_z|
 *   sd[3]    = max (x_x x_x + x_y x_y)     horizontal resultant, SQUARED, summed in this order; its root is RotD100 of SD
 * A value enters only if it is strictly greater: the first occurrence of a maximum is kept and a NaN never enters sd.  A
 * NaN in the input DOES stay in x and v from then on, as in any linear recursive filter: sd then stops at what it held.
 * PSV = omega SD and PSA = omega^2 SD are the caller's to form.
 */
#ifndef HQ_SDOF_H
#define HQ_SDOF_H

#include <stdint.h>

#if defined(__HIPCC__)
#define HQ_SDOF_FN __host__ __device__ static inline
#else
#define HQ_SDOF_FN static inline
#endif

enum { HQ_SDOF_NCOEF = 8, HQ_SDOF_TERMS = 18, HQ_SPEC_NSD = 4, HQ_SPEC_NOSC = 6 };

/* c = a b, 4 x 4 row-major; every sum left to right */
HQ_SDOF_FN void hq_sdof_mul4(const double* a, const double* b, double* c)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++)
            c[4 * i + j] = ((a[4 * i] * b[j] + a[4 * i + 1] * b[4 + j]) + a[4 * i + 2] * b[8 + j]) + a[4 * i + 3] * b[12 + j];
}

/* the eight coefficients of the exact step h for period `period` (s) and `damping` (fraction of critical) */
HQ_SDOF_FN void hq_sdof_coef(double period, double damping, double h, double* c)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double w = 6.283185307179586 * h / period;             /* 2 pi, to the nearest double */
    const double w2 = w * w, zw2 = 2.0 * damping * w;
    double norm = 1.0 + zw2 + w2, scale = 1.0;
    int s = 0;
    do { scale = scale * 0.5; norm = norm * 0.5; s++; } while (norm > 0.5 && s < 60);
    double m[16], e[16], t[16], n[16];
    for (int i = 0; i < 16; i++) { m[i] = 0.0; e[i] = 0.0; t[i] = 0.0; }
    m[1] = scale; m[4] = -w2 * scale; m[5] = -zw2 * scale; m[6] = -scale; m[11] = scale;   /* M / 2^s: exact scalings */
    e[0] = e[5] = e[10] = e[15] = 1.0;
    t[0] = t[5] = t[10] = t[15] = 1.0;
    for (int k = 1; k <= HQ_SDOF_TERMS; k++) {                   /* e = sum of (M / 2^s)^k / k! */
        hq_sdof_mul4(t, m, n);
        for (int i = 0; i < 16; i++) { t[i] = n[i] / (double)k; e[i] = e[i] + t[i]; }
    }
    for (int q = 0; q < s; q++) {
        hq_sdof_mul4(e, e, n);
        for (int i = 0; i < 16; i++) e[i] = n[i];
    }
    const double h2 = h * h;
    c[0] = e[0];                                                 /* x' = E11 x + E12 (h v) + E13 (h^2 a0) + E14 h^2 (a1 - a0) */
    c[1] = e[1] * h;
    c[2] = e[4] / h;                                             /* h v' = E21 x + ... */
    c[3] = e[5];
    c[4] = (e[2] - e[3]) * h2;
    c[5] = e[3] * h2;
    c[6] = (e[6] - e[7]) * h;
    c[7] = e[7] * h;
}

/* one step of one oscillator from sample a0 to sample a1: the two lines of the header's comment, in that order of operations */
HQ_SDOF_FN void hq_sdof_step(const double* c, double a0, double a1, double* x, double* v)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double x0 = *x, v0 = *v;
    *x = ((c[0] * x0 + c[1] * v0) + c[4] * a0) + c[5] * a1;
    *v = ((c[2] * x0 + c[3] * v0) + c[6] * a0) + c[7] * a1;
}

/* Fold one acceleration sample a1 = (ax, ay, az), the sample before it a0, into a point's state for ONE period: the three
 * oscillators step, then the maxima.  osc[(k * 3 + axis) * ostride], k = 0 for x and 1 for v; sd[j * sstride], j = 0..3
 * (stride 1 on the host and on a lane's register copy; the number of points in tables laid out [.][np]).  x and v are
 * always written, sd only where it is raised. */
HQ_SDOF_FN void hq_spec_fold(const double* c, const double* a0, const double* a1, double* osc, int64_t ostride, double* sd,
                             int64_t sstride)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double x[3];
    for (int a = 0; a < 3; a++) {
        double xa = osc[a * ostride], va = osc[(3 + a) * ostride];
        hq_sdof_step(c, a0[a], a1[a], &xa, &va);
        osc[a * ostride] = xa; osc[(3 + a) * ostride] = va;
        x[a] = xa;
        const double m = __builtin_fabs(xa);
        if (m > sd[a * sstride]) sd[a * sstride] = m;
    }
    const double xx = x[0] * x[0], yy = x[1] * x[1];
    const double hh = xx + yy;
    if (hh > sd[3 * sstride]) sd[3 * sstride] = hh;
}

#endif
