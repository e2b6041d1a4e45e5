"""CPU-side checks of the response-spectrum trackers' boundary (include/hq_solver.h: hq_spec_*; include/hq_host.h: hqh_sdof_coef,
hqh_spec_fold; csrc/hq_sdof.h, the one text of the oscillator): the symbols exist and refuse a null context, the ctypes mirror
of hq_spec_desc has the header's layout, the eight coefficients hold 1e-14 relative against mpmath at 60 digits where the
textbook closed form does not, the fold does what a few lines of numpy do and stays within 1e-10 of max |x| of an mpmath
recursion over 2 000 samples, the recursion is stable at T <= h, and hipcc left both forms of hq_k_spec without spills,
scratch or LDS at no more than 128 registers.  No GPU."""
import ctypes
import os
import subprocess
import sys

import mpmath as mp
import numpy as np
import pytest

import hercules_amd as ha
from hercules_amd import build as hbuild
from hercules_amd import capi, host
from tests import test_code_object_cpu as CO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["hq_spec_add", "hq_spec_coefficients", "hq_spec_fetch", "hq_spec_load", "hq_spec_reset", "hq_spec_clear"]
HQ_ERR_ARG = -1
COEF_TOL = 1e-14          # five times what the double-precision scaled Taylor series measured (2.1e-15)
FOLD_TOL = 1e-10          # of max |x|: fifty times the series' worst over these cases (2.0e-12)
DIGITS = 60


@pytest.fixture(scope="module")
def libs():
    hbuild.build()
    return ha.load_library(), capi.load_library(precision="f32")


def test_the_libraries_export_the_entry_points(libs):
    for lib in libs:
        for n in NAMES:
            assert hasattr(lib, n), n
    assert set(NAMES) <= set(capi.EXPORTS)
    hl = host.load_library()
    for n in ("hqh_sdof_coef", "hqh_spec_fold"):
        assert n in host.EXPORTS and hasattr(hl, n), n
    assert libs[0].hq_abi_version() == 6 and libs[1].hq_abi_version() == 6      # additive: no ABI bump


def test_null_context_is_a_bad_argument(libs):
    for lib in libs:
        ids = (ctypes.c_int32 * 1)(0)
        per = (ctypes.c_double * 1)(1.0)
        d = capi._SpecDesc(1, 1, ctypes.cast(ids, ctypes.c_void_p), None, 1, 0, 1, 0, ctypes.cast(per, ctypes.c_void_p), 0.05)
        h, n = ctypes.c_int32(), ctypes.c_int64()
        sd, osc, ap, cf = (ctypes.c_double * 4)(), (ctypes.c_double * 6)(), (ctypes.c_double * 3)(), (ctypes.c_double * 8)()
        assert lib.hq_spec_add(None, ctypes.byref(d), ctypes.byref(h)) == HQ_ERR_ARG
        assert lib.hq_spec_coefficients(None, ctypes.c_int32(0), cf) == HQ_ERR_ARG
        assert lib.hq_spec_fetch(None, ctypes.c_int32(0), sd, osc, ap, ctypes.byref(n)) == HQ_ERR_ARG
        assert lib.hq_spec_load(None, ctypes.c_int32(0), sd, osc, ap, ctypes.c_int64(0)) == HQ_ERR_ARG
        assert lib.hq_spec_reset(None, ctypes.c_int32(0)) == HQ_ERR_ARG
        assert lib.hq_spec_clear(None) == HQ_ERR_ARG


def test_descriptor_mirrors_the_header(libs, tmp_path):
    fields = [f for f, _ in capi._SpecDesc._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hq_host.h"\n'
                   'int main(void) { printf("%zu", sizeof(hq_spec_desc));\n' +
                   "".join('printf(" %%zu", offsetof(hq_spec_desc, %s));\n' % f for f in fields) +
                   'printf(" %d %d\\n", HQ_SPEC_MAX_PERIODS, HQ_SPEC_NVAL); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [int(x) for x in subprocess.check_output([str(exe)], universal_newlines=True).split()]
    assert out[0] == ctypes.sizeof(capi._SpecDesc) == 56
    assert out[1:-2] == [getattr(capi._SpecDesc, f).offset for f in fields]
    assert out[-2:] == [capi.HQ_SPEC_MAX_PERIODS, capi.HQ_SPEC_NVAL] == [32, 4]


# ---------------------------------------------------------------------------------------------------------------------
# the coefficients against mpmath
# ---------------------------------------------------------------------------------------------------------------------

def _mp_coef(T, z, h):
    """expm of the 4 x 4 system of (x, v, a, slope) over h at 60 digits: x' = v, v' = -w^2 x - 2 z w v - a, a' = slope =
    (a1 - a0) / h, slope' = 0 -> the eight coefficients of (a0, a1)."""
    T, z, h = mp.mpf(T), mp.mpf(z), mp.mpf(h)
    w = 2 * mp.pi / T
    M = mp.matrix([[0, 1, 0, 0], [-w * w, -2 * z * w, -1, 0], [0, 0, 0, 1], [0, 0, 0, 0]]) * h
    E = mp.expm(M, method="taylor")
    return [E[0, 0], E[0, 1], E[1, 0], E[1, 1], E[0, 2] - E[0, 3] / h, E[0, 3] / h, E[1, 2] - E[1, 3] / h, E[1, 3] / h]


def _closed_form(T, z, h):
    """The textbook closed form (Nigam & Jennings 1969) in double precision."""
    w = 2 * np.pi / T
    r = np.sqrt(1 - z * z)
    wd = w * r
    e, s, c = np.exp(-z * w * h), np.sin(wd * h), np.cos(wd * h)
    p, q = (2 * z * z - 1) / (w * w * h), 2 * z / (w ** 3 * h)
    a11 = e * (z / r * s + c)
    a12 = e * s / wd
    a21 = -w / r * e * s
    a22 = e * (c - z / r * s)
    b11 = e * ((p + z / w) * s / wd + (q + 1 / w ** 2) * c) - q
    b12 = -e * (p * s / wd + q * c) - 1 / w ** 2 + q
    b21 = e * ((p + z / w) * (c - z / r * s) - (q + 1 / w ** 2) * (wd * s + z * w * c)) + 1 / (w * w * h)
    b22 = -e * (p * (c - z / r * s) - q * (wd * s + z * w * c)) - 1 / (w * w * h)
    return np.array([a11, a12, a21, a22, b11, b12, b21, b22])


def _rel(got, want):
    return max(float(abs((mp.mpf(float(g)) - w) / w)) for g, w in zip(got, want))


def test_coefficients_hold_1e_14_against_mpmath_where_the_closed_form_does_not():
    worst, worst_closed = 0.0, {}
    with mp.workdps(DIGITS):
        for T in (0.02, 0.1, 0.3, 1.0, 3.0, 10.0):
            for h in (3e-3, 1e-3, 3e-4):
                for z in (0.0, 0.05, 0.2):
                    want = _mp_coef(T, z, h)
                    got = host.sdof_coef([T], z, h)[0]
                    err = _rel(got, want)
                    worst = max(worst, err)
                    assert err <= COEF_TOL, (T, h, z, err)
                    worst_closed[(T, h)] = max(worst_closed.get((T, h), 0.0), _rel(_closed_form(T, z, h), want))
    print("series: worst %.2e; closed form: worst %.2e, at T = 10 s, h = 3e-4 s %.2e, at T = 0.1 s, h = 3e-3 s %.2e"
          % (worst, max(worst_closed.values()), worst_closed[(10.0, 3e-4)], worst_closed[(0.1, 3e-3)]))
    assert worst_closed[(0.1, 3e-3)] < 1e-9                 # it IS the closed form of these coefficients ...
    assert worst_closed[(10.0, 3e-4)] > COEF_TOL            # ... and it fails the bar where a simulation steps


def test_coefficients_do_not_depend_on_the_compiler(libs, tmp_path):
    """hq_sdof.h compiled by gcc (the host library) and by the HIP toolchain's clang at -O3 -march=native, where it would
    contract products and sums into FMAs if the header's pragma did not forbid it: one table, bit for bit."""
    clang = os.path.join(os.path.dirname(os.path.realpath(hbuild.HIPCC)), "..", "llvm", "bin", "clang")
    if not os.path.exists(clang):
        clang = os.path.join(os.path.dirname(os.path.realpath(hbuild.HIPCC)), "clang")
    assert os.path.exists(clang), clang
    src = tmp_path / "probe.c"
    src.write_text('#include "hq_sdof.h"\nvoid probe(double T, double z, double h, double* c) { hq_sdof_coef(T, z, h, c); }\n')
    so = tmp_path / "libprobe.so"
    subprocess.check_call([clang, "-O3", "-march=native", "-std=gnu99", "-shared", "-fPIC", "-I",
                           os.path.join(ROOT, "hercules_amd", "csrc"), "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    for T in (0.02, 0.37, 10.0, 1e-3):
        for z in (0.0, 0.05):
            c = (ctypes.c_double * 8)()
            lib.probe(ctypes.c_double(T), ctypes.c_double(z), ctypes.c_double(1e-3), c)
            assert np.array_equal(np.array(c), host.sdof_coef([T], z, 1e-3)[0]), (T, z)


# ---------------------------------------------------------------------------------------------------------------------
# hqh_spec_fold against numpy
# ---------------------------------------------------------------------------------------------------------------------

PERIODS = [0.02, 0.05, 0.1, 0.3, 1.0]


def _numpy_fold(coef, acc, state=None):
    """The two recursion lines and the maxima in numpy, in the stated order of operations; elementwise numpy products and
    sums are single IEEE operations.  acc [k, np, 3] -> sd [np, nper, 4], osc [np, nper, 2, 3], aprev [np, 3]."""
    k, npts = acc.shape[:2]
    nper = len(coef)
    if state is None:
        sd, osc, aprev = np.zeros((npts, nper, 4)), np.zeros((npts, nper, 2, 3)), np.zeros((npts, 3))
    else:
        sd, osc, aprev = [a.copy() for a in state]
    c = [coef[None, :, i, None] for i in range(8)]
    for s in range(k):
        a0, a1 = aprev[:, None, :], acc[s][:, None, :]
        x, v = osc[:, :, 0], osc[:, :, 1]
        xn = ((c[0] * x + c[1] * v) + c[4] * a0) + c[5] * a1
        vn = ((c[2] * x + c[3] * v) + c[6] * a0) + c[7] * a1
        osc = np.stack([xn, vn], axis=2)
        m = np.abs(xn)
        with np.errstate(invalid="ignore"):
            sd[:, :, :3] = np.where(m > sd[:, :, :3], m, sd[:, :, :3])
            hh = xn[:, :, 0] * xn[:, :, 0] + xn[:, :, 1] * xn[:, :, 1]
            sd[:, :, 3] = np.where(hh > sd[:, :, 3], hh, sd[:, :, 3])
        aprev = acc[s].copy()
    return sd, osc, aprev


def _samples(seed, nsamples=37, npts=23):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nsamples, npts, 3)) * 10.0 ** rng.integers(-6, 6, (1, npts, 1))


def _equal(got, want):
    for g, w, name in zip(got, want, ("sd", "osc", "aprev")):
        assert g.shape == w.shape, name
        assert np.array_equal(g, w, equal_nan=True), (name, np.argwhere(g != w)[:5])


def test_fold_equals_numpy_on_random_samples():
    coef = host.sdof_coef(PERIODS, 0.05, 1e-3)
    acc = _samples(1)
    got = host.spec_fold(coef, acc)
    assert got[0].shape == (23, 5, 4) and got[1].shape == (23, 5, 2, 3) and got[2].shape == (23, 3)
    _equal(got, _numpy_fold(coef, acc))
    assert (got[0] > 0).all() and np.array_equal(got[2], acc[-1])
    assert len(np.unique(got[0][:, :, 0])) == 23 * 5


def test_recorder_columns_fold_without_a_copy():
    """acc as columns 6..8 of a derivs = 2 recorder's samples: a strided view, the same numbers."""
    coef = host.sdof_coef(PERIODS, 0.2, 3e-3)
    rec = np.random.default_rng(7).standard_normal((37, 23, 9))
    _equal(host.spec_fold(coef, rec[:, :, 6:9]), _numpy_fold(coef, np.ascontiguousarray(rec[:, :, 6:9])))
    _equal(host.spec_fold(coef, rec[:, :, 6:]), host.spec_fold(coef, np.ascontiguousarray(rec[:, :, 6:9])))


def test_two_calls_in_sequence_equal_one_on_the_concatenation():
    coef = host.sdof_coef(PERIODS, 0.05, 1e-3)
    acc = _samples(4)
    one = host.spec_fold(coef, acc)
    st = host.spec_fold(coef, acc[:17])
    two = host.spec_fold(coef, acc[17:], *st)
    assert all(a is b for a, b in zip(two, st))
    _equal(two, one)
    _equal(host.spec_fold(coef, acc[:0], *[a.copy() for a in two]), one)
    _equal(two, _numpy_fold(coef, acc[17:], _numpy_fold(coef, acc[:17])))


def test_a_tie_keeps_the_first_maximum_and_an_all_zero_point_stays_at_zero():
    """With the coefficients {0, 0, 0, 0, 0, 1, 0, 0} the step is x' = a1: the samples ARE the displacements."""
    coef = np.zeros((1, 8))
    coef[0, 5] = 1.0
    acc = np.zeros((5, 3, 3))
    acc[:, 0, 0] = [1.0, 3.0, -3.0, 3.0, 2.0]
    acc[:, 0, 1] = [0.0, -4.0, 4.0, 0.0, 0.0]
    acc[:, 2, :] = -0.0
    sd, osc, aprev = host.spec_fold(coef, acc)
    assert sd[0, 0].tolist() == [3.0, 4.0, 0.0, 25.0]
    assert (sd[1] == 0).all() and (sd[2] == 0).all() and not np.signbit(sd[2]).any()      # -0.0 never entered
    assert (osc[1] == 0).all() and osc[0, 0, 0].tolist() == [2.0, 0.0, 0.0]
    _equal((sd, osc, aprev), _numpy_fold(coef, acc))
    real = host.sdof_coef(PERIODS, 0.05, 1e-3)
    acc = _samples(2)
    acc[:, 4, :] = 0.0
    acc[:, 6, :2] = 0.0                                      # x and y at rest: the horizontal resultant never raised, z is
    got = host.spec_fold(real, acc)
    assert (got[0][4] == 0).all() and (got[1][4] == 0).all()
    assert (got[0][6][:, [0, 1, 3]] == 0).all() and (got[0][6][:, 2] > 0).all()
    _equal(got, _numpy_fold(real, acc))


def test_a_nan_never_enters_sd_and_stays_in_x_and_v():
    coef = host.sdof_coef(PERIODS, 0.05, 1e-3)
    acc = _samples(3)
    acc[20, 2, :] = np.nan                                   # a whole sample of one point
    acc[9, 3, 1] = np.nan                                    # one component: its axis and the horizontal stop there
    acc[0, 8, :] = np.nan                                    # the very first sample
    got = host.spec_fold(coef, acc)
    assert np.isfinite(got[0]).all()
    assert np.isnan(got[1][2]).all() and np.isnan(got[1][8]).all() and (got[0][8] == 0).all()
    assert np.isnan(got[1][3][:, :, 1]).all() and np.isfinite(got[1][3][:, :, [0, 2]]).all()
    before = host.spec_fold(coef, acc[:20, 2:3])
    assert np.array_equal(got[0][2], before[0][0]) and (got[0][2] > 0).all()
    clean = np.ones(23, bool)
    clean[[2, 3, 8]] = False
    assert np.isfinite(got[1][clean]).all()
    _equal(got, _numpy_fold(coef, acc))


# ---------------------------------------------------------------------------------------------------------------------
# the fold against an mpmath recursion
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,h,z", [(0.05, 1e-3, 0.05), (1.0, 1e-3, 0.05), (10.0, 3e-4, 0.05), (0.3, 3e-3, 0.0), (3.0, 3e-4, 0.2)])
def test_fold_stays_within_1e_10_of_an_mpmath_recursion(T, h, z):
    """2 000 samples of a seeded piecewise-linear series -- a Hann-windowed sine of period 0.7 T plus noise of 0.1 of its
    standard deviation: the double recursion with the library's coefficients against the recursion at 60 digits with
    mpmath's coefficients, sample by sample, within 1e-10 of max |x|."""
    n = 2000
    t = np.arange(n) * h
    sig = np.sin(2 * np.pi * t / (0.7 * T)) * np.hanning(n)
    a = sig + 0.1 * sig.std() * np.random.default_rng(11).standard_normal(n)
    coef = host.sdof_coef([T], z, h)
    acc = np.zeros((n, 1, 3))
    acc[:, 0, 0] = a
    st = host.spec_fold(coef, acc[:0])
    xs = np.zeros(n)
    for k in range(n):
        host.spec_fold(coef, acc[k:k + 1], *st)
        xs[k] = st[1][0, 0, 0, 0]
    with mp.workdps(DIGITS):
        c = _mp_coef(T, z, h)
        x, v, a0 = mp.mpf(0), mp.mpf(0), mp.mpf(0)
        ref, worst = [], mp.mpf(0)
        for k in range(n):
            a1 = mp.mpf(float(a[k]))
            x, v = c[0] * x + c[1] * v + c[4] * a0 + c[5] * a1, c[2] * x + c[3] * v + c[6] * a0 + c[7] * a1
            a0 = a1
            ref.append(x)
            worst = max(worst, abs(mp.mpf(float(xs[k])) - x))
        scale = max(abs(r) for r in ref)
        err = float(worst / scale)
    print("T = %g, h = %g, zeta = %g: %.2e of max |x| = %.3e" % (T, h, z, err, float(scale)))
    assert scale > 0 and st[0][0, 0, 0] == np.abs(xs).max()
    assert err <= FOLD_TOL, err


# ---------------------------------------------------------------------------------------------------------------------
# stability, bad arguments
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ratio", [1.0, 0.5])
def test_the_recursion_is_stable_at_periods_down_to_half_a_step(ratio):
    """T = h and T = 0.5 h, zeta = 0.05, 10 000 samples bounded by 1: x stays bounded.  The bound is the oscillator's
    L-infinity gain, the integral of |impulse response| = coth(pi zeta / (2 sqrt(1 - zeta^2))) / omega^2 = 12.75 / omega^2
    at zeta = 0.05, which the exact step of a piecewise-linear input bounded by 1 cannot exceed; 13 leaves room for rounding."""
    h, z = 1e-3, 0.05
    T = ratio * h
    coef = host.sdof_coef([T], z, h)
    acc = np.random.default_rng(5).uniform(-1.0, 1.0, (10000, 4, 3))
    acc[:, 1, :] = np.sign(acc[:, 1, :])                     # a square-ish input at full amplitude
    acc[:, 2, :] = 1.0                                       # a step: x -> -1 / omega^2
    sd, osc, _ = host.spec_fold(coef, acc)
    w = 2 * np.pi / T
    gain = 1.0 / np.tanh(np.pi * z / (2 * np.sqrt(1 - z * z)))
    assert 12.7 < gain < 12.8
    assert np.isfinite(sd).all() and np.isfinite(osc).all()
    assert (sd[:, 0, :3] <= 13.0 / w ** 2).all(), sd[:, 0, :3] * w ** 2
    assert (sd[:, 0, :3] > 0).all()
    assert abs(osc[2, 0, 0, 0] * w ** 2 + 1.0) < 1e-9       # the step's static displacement


def test_bad_arguments_of_the_host_functions():
    lib = host.load_library()
    c8, sd, osc, ap, acc = ((ctypes.c_double * n)() for n in (8, 4, 6, 3, 3))
    D = ctypes.c_double
    assert lib.hqh_sdof_coef(D(1.0), D(0.05), D(1e-3), c8) == 0 and c8[0] != 0
    for T, z, h in ((0.0, 0.05, 1e-3), (-1.0, 0.05, 1e-3), (np.nan, 0.05, 1e-3), (np.inf, 0.05, 1e-3), (1.0, -0.1, 1e-3),
                    (1.0, 1.0, 1e-3), (1.0, np.nan, 1e-3), (1.0, 0.05, 0.0), (1.0, 0.05, -1e-3), (1.0, 0.05, np.nan),
                    (1.0, 0.05, np.inf)):
        assert lib.hqh_sdof_coef(D(T), D(z), D(h), c8) == HQ_ERR_ARG, (T, z, h)
    assert lib.hqh_sdof_coef(D(1.0), D(0.05), D(1e-3), None) == HQ_ERR_ARG
    L = ctypes.c_int64
    assert lib.hqh_spec_fold(1, 1, c8, 1, acc, L(3), sd, osc, ap) == 0
    assert lib.hqh_spec_fold(-1, 1, c8, 1, acc, L(3), sd, osc, ap) == HQ_ERR_ARG
    assert lib.hqh_spec_fold(1, -1, c8, 1, acc, L(3), sd, osc, ap) == HQ_ERR_ARG
    assert lib.hqh_spec_fold(1, 1, c8, -1, acc, L(3), sd, osc, ap) == HQ_ERR_ARG
    assert lib.hqh_spec_fold(1, 1, c8, 1, acc, L(2), sd, osc, ap) == HQ_ERR_ARG
    assert lib.hqh_spec_fold(1, 1, None, 1, acc, L(3), sd, osc, ap) == HQ_ERR_ARG
    assert lib.hqh_spec_fold(1, 1, c8, 1, None, L(3), sd, osc, ap) == HQ_ERR_ARG
    assert lib.hqh_spec_fold(1, 1, c8, 1, acc, L(3), None, osc, ap) == HQ_ERR_ARG
    assert lib.hqh_spec_fold(1, 1, c8, 1, acc, L(3), sd, None, ap) == HQ_ERR_ARG
    assert lib.hqh_spec_fold(1, 1, c8, 1, acc, L(3), sd, osc, None) == HQ_ERR_ARG
    assert lib.hqh_spec_fold(0, 1, None, 1, None, L(3), None, None, None) == 0
    assert lib.hqh_spec_fold(1, 1, None, 0, None, L(3), None, None, None) == 0
    with pytest.raises(capi.HqError):
        host.spec_fold(np.zeros((2, 7)), np.zeros((1, 1, 3)))
    with pytest.raises(capi.HqError):
        host.spec_fold(np.zeros((2, 8)), np.zeros((1, 1, 2)))
    with pytest.raises(capi.HqError):
        host.spec_fold(np.zeros((2, 8)), np.zeros((1, 1, 3)), np.zeros((1, 2, 4)), np.zeros((1, 2, 2, 3)), np.zeros((2, 3)))


# ---------------------------------------------------------------------------------------------------------------------
# the code object
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("so", ["libhq_solver.so", "libhq_solver_f32.so"])
def test_spec_kernels_have_no_spill_no_scratch_and_at_most_128_registers(libs, tmp_path, monkeypatch, so):
    """hq_k_spec<1> and hq_k_spec<8> sit at the head of every due step beside the stepping kernels: no spilled register, no
    scratch, no LDS, and at most 128 VGPRs -- four waves per SIMD, whose loads (two periods' state each) hide one another."""
    path = os.path.join(ROOT, "hercules_amd", "csrc", so)
    assert os.path.exists(path), path
    monkeypatch.setattr(sys.modules[CO.__name__], "SO", path)
    k = CO._kernel_notes(tmp_path)
    found = {}
    for name, v in k.items():
        for tag in ("hq_k_specILi1EE", "hq_k_specILi8EE"):
            if tag in name:
                found[tag] = v
    assert sorted(found) == ["hq_k_specILi1EE", "hq_k_specILi8EE"], sorted(k)
    for tag, v in found.items():
        print(so, tag, "vgpr", v["vgpr_count"], "sgpr", v["sgpr_count"])
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (tag, v)
        assert v["group_segment_fixed_size"] == 0, (tag, v)
        assert v["vgpr_count"] <= 128, (tag, v)
