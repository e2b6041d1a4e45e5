/*
 * cumul_host_main.c -- hqh_cum_fold and hqh_husid_cross (hercules_amd/csrc/hq_host.c) in a stand-alone program, for the
 * host sanitizers: CPU only, never loaded into Python, no device touched.  The fold case is tests/test_cumul_cpu.py's own,
 * written by `python -m tests.test_cumul_cpu FILE`: inputs and the result of the Python loop; the Husid case is that
 * file's piecewise-linear curve.  From the repository root, with the libraries built:
 *
 *   python -m tests.test_cumul_cpu /tmp/cumul_case.bin
 *   gcc -O1 -g -std=gnu99 -fopenmp -fsanitize=address,undefined -fno-omit-frame-pointer -I include \
 *       -o /tmp/cumul_host_main tests/cumul_host_main.c hercules_amd/csrc/hq_host.c \
 *       -L hercules_amd/csrc -lhq_solver -Wl,-rpath,$PWD/hercules_amd/csrc -lm
 *   ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=halt_on_error=1 /tmp/cumul_host_main /tmp/cumul_case.bin
 *
 * Every array is allocated at its exact size, so a read or write past an end is the sanitizer's to report.  Exit status 0
 * and "ok" if the fold at once and in two chunks equals the Python loop byte for byte and the crossings are exact.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hq_host.h"

static int fail(const char* what)
{
    fprintf(stderr, "cumul_host_main: %s\n", what);
    return 1;
}

static void* take(FILE* f, size_t bytes)
{
    void* p = malloc(bytes ? bytes : 1);
    if (!p || fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "cumul_host_main: short file\n"); exit(2); }
    return p;
}

static void fresh(int64_t n, double* sums, int32_t* span)
{
    for (int64_t i = 0; i < 6 * n; i++) sums[i] = 0.0;
    for (int64_t i = 0; i < n; i++) { span[3 * i] = -1; span[3 * i + 1] = -1; span[3 * i + 2] = 0; }
}

int main(int argc, char** argv)
{
    if (argc != 2) return fail("usage: cumul_host_main FILE");
    FILE* f = fopen(argv[1], "rb");
    if (!f) return fail("cannot open the case file");
    int32_t* hd = (int32_t*)take(f, 4 * sizeof(int32_t));
    const int32_t np = hd[0], q = hd[1], ns = hd[2], cut = hd[3];
    const int32_t nq = (q & 1) + ((q >> 1) & 1) + ((q >> 2) & 1), ncomp = 3 * (1 + ((q & 4) ? 2 : (q & 2) ? 1 : 0));
    const int64_t n = (int64_t)np * nq;
    int32_t* steps = (int32_t*)take(f, sizeof(int32_t) * (size_t)ns);
    double* samples = (double*)take(f, sizeof(double) * (size_t)ns * (size_t)np * (size_t)ncomp);
    double* thr = (double*)take(f, sizeof(double) * (size_t)nq);
    double* want_sums = (double*)take(f, sizeof(double) * 6 * (size_t)n);
    int32_t* want_span = (int32_t*)take(f, sizeof(int32_t) * 3 * (size_t)n);
    fclose(f);
    double* sums = (double*)malloc(sizeof(double) * 6 * (size_t)n);
    int32_t* span = (int32_t*)malloc(sizeof(int32_t) * 3 * (size_t)n);
    if (!sums || !span) return fail("out of memory");
    int bad = 0;

    fresh(n, sums, span);
    if (hqh_cum_fold(np, q, ns, steps, samples, thr, sums, span) != 0) bad += fail("hqh_cum_fold refused the case");
    if (memcmp(sums, want_sums, sizeof(double) * 6 * (size_t)n) != 0) bad += fail("sums differ from the Python loop's");
    if (memcmp(span, want_span, sizeof(int32_t) * 3 * (size_t)n) != 0) bad += fail("span differs from the Python loop's");

    fresh(n, sums, span);
    if (hqh_cum_fold(np, q, cut, steps, samples, thr, sums, span) != 0 ||
        hqh_cum_fold(np, q, ns - cut, steps + cut, samples + (int64_t)cut * np * ncomp, thr, sums, span) != 0)
        bad += fail("hqh_cum_fold refused a chunk");
    if (memcmp(sums, want_sums, sizeof(double) * 6 * (size_t)n) != 0 || memcmp(span, want_span, sizeof(int32_t) * 3 * (size_t)n) != 0)
        bad += fail("two chunks differ from one fold");
    if (hqh_cum_fold(np, q, 0, NULL, NULL, thr, NULL, NULL) != 0 || hqh_cum_fold(np, 0, ns, steps, samples, thr, sums, span) == 0)
        bad += fail("argument checks");

    /* tests/test_cumul_cpu.py: HUSID_* */
    enum { NSLOTS = 5, NSERIES = 3, NFRAC = 6 };
    int32_t* hsteps = (int32_t*)malloc(sizeof(int32_t) * NSLOTS);
    double* curve = (double*)malloc(sizeof(double) * NSLOTS * NSERIES);
    double* total = (double*)malloc(sizeof(double) * NSERIES);
    double* fracs = (double*)malloc(sizeof(double) * NFRAC);
    double* out = (double*)malloc(sizeof(double) * NSERIES * NFRAC);
    if (!hsteps || !curve || !total || !fracs || !out) return fail("out of memory");
    const int32_t hs[NSLOTS] = { 8, 16, 24, 32, 40 };
    const double cv[NSLOTS][NSERIES] = { { 0, 2, 0 }, { 16, 2, 0 }, { 16, 6, 0 }, { 48, 6, 0 }, { 56, 8, 0 } };
    const double tt[NSERIES] = { 64, 8, 0 }, fr[NFRAC] = { 0.125, 0.25, 0.5, 0.75, 0.8125, 0.9375 };
    const double want[2][NFRAC] = { { 12, 16, 28, 32, 36, NAN }, { 6, 8, 20, 24, 34, 38 } };
    memcpy(hsteps, hs, sizeof hs); memcpy(curve, cv, sizeof cv); memcpy(total, tt, sizeof tt); memcpy(fracs, fr, sizeof fr);
    if (hqh_husid_cross(NSLOTS, hsteps, 4.0, NSERIES, curve, total, NFRAC, fracs, out) != 0) bad += fail("hqh_husid_cross refused the case");
    for (int s = 0; s < NSERIES; s++)
        for (int k = 0; k < NFRAC; k++) {
            const double o = out[s * NFRAC + k];
            if (s == 2 || isnan(want[s][k]) ? !isnan(o) : o != want[s][k]) bad += fail("a crossing is not where it was built to be");
        }
    if (hqh_husid_cross(0, NULL, 4.0, NSERIES, NULL, total, NFRAC, fracs, out) != 0 || !isnan(out[0])) bad += fail("no slots: NaN");

    free(hd); free(steps); free(samples); free(thr); free(want_sums); free(want_span); free(sums); free(span);
    free(hsteps); free(curve); free(total); free(fracs); free(out);
    if (!bad) printf("ok\n");
    return bad ? 1 : 0;
}
