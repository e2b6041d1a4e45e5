"""CPU-side checks of the cumulative-intensity trackers' boundary (include/hq_solver.h: hq_cum_*; include/hq_host.h:
hqh_cum_fold, hqh_husid_cross; csrc/hq_cumul.h, the one text of the fold): hqh_cum_fold does what a plain Python loop does, bit
for bit -- exact zeros, a sample exactly at the threshold, a NaN, first_step filtering, every mask, two calls in sequence;
hqh_husid_cross finds the crossings of a piecewise-linear curve exactly; the Arias integral formed from the sums is the
rectangle rule; the symbols exist in the header and in the libraries; and hipcc left both forms of hq_k_cum without spills or
scratch in both libraries.  No GPU.

    python -m tests.test_cumul_cpu FILE

writes the fold case of this file (inputs and the Python loop's result) for tests/cumul_host_main.c, the stand-alone program
that runs the two host functions under the host sanitizers."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hercules_amd as ha
from hercules_amd import build as hbuild
from hercules_amd import capi, host
from tests import test_code_object_cpu as CO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["hq_cum_add", "hq_cum_fetch", "hq_cum_load", "hq_cum_reset", "hq_cum_clear"]
HQ_ERR_ARG = -1
D, V, A = capi.HQ_PEAK_DISP, capi.HQ_PEAK_VEL, capi.HQ_PEAK_ACC
MASKS = [D, V, A, D | V, D | A, V | A, D | V | A]
NPOINTS, NSAMPLES, FIRST_STEP = 7, 300, 12
THRESHOLD = (1.5, 0.75, 1.25)                                # per quantity bit: displacement, velocity, acceleration


@pytest.fixture(scope="module")
def libs():
    hbuild.build()
    return ha.load_library(), capi.load_library(precision="f32")


def _derivs(q):
    return 2 if q & A else 1 if q & V else 0


def _thresholds(q):
    return [THRESHOLD[b] for b in range(3) if q & (1 << b)]


def _case(q):
    """Steps 0, 2, 4, ... and samples [NSAMPLES, NPOINTS, 9] cut to the mask's columns: random values; point 1 all zero; exact
    zeros strewn in; at point 2, sample 40, every quantity's vector is (threshold, 0, 0) -- its total IS the threshold squared,
    which must not count; at point 3 every sample is far below every threshold (never counted); at point 4, sample 100, a
    NaN in the y components; point 5 over every threshold at every sample."""
    rng = np.random.default_rng(20261019)
    steps = (2 * np.arange(NSAMPLES)).astype(np.int32)
    s = rng.uniform(-1.0, 1.0, (NSAMPLES, NPOINTS, 9))
    s[:, 1] = 0.0
    s[rng.uniform(size=s.shape) < 0.05] = 0.0
    for b in range(3):
        s[40, 2, 3 * b:3 * b + 3] = (THRESHOLD[b], 0.0, 0.0)
    s[:, 3] *= 1e-3
    s[100, 4, 1::3] = np.nan
    s[:, 5] += np.sign(s[:, 5]) * 3.0 + (s[:, 5] == 0) * 3.0
    s[40:43, 6, :] = -0.0
    return steps, np.ascontiguousarray(s[:, :, :3 * (1 + _derivs(q))])


def _python_fold(steps, samples, q, thr, first_step=0, sums=None, span=None):
    """The definition, in Python floats (which do not contract): s += abs(x); s += x * x; (xx + yy) + zz > thr * thr."""
    bits = [b for b in range(3) if q & (1 << b)]
    npoints = samples.shape[1]
    if sums is None:
        sums = [[[0.0] * 6 for _ in bits] for _ in range(npoints)]
        span = [[[-1, -1, 0] for _ in bits] for _ in range(npoints)]
    for k in range(len(steps)):
        if steps[k] < first_step:
            continue
        for p in range(npoints):
            for m, b in enumerate(bits):
                x, y, z = (float(v) for v in samples[k, p, 3 * b:3 * b + 3])
                sm, sp = sums[p][m], span[p][m]
                sm[0] += abs(x)
                sm[1] += abs(y)
                sm[2] += abs(z)
                xx, yy, zz = x * x, y * y, z * z
                sm[3] += xx
                sm[4] += yy
                sm[5] += zz
                if (xx + yy) + zz > thr[m] * thr[m]:
                    if sp[2] == 0:
                        sp[0] = int(steps[k])
                    sp[1] = int(steps[k])
                    sp[2] += 1
    return sums, span


def _same(got, want):
    ws, wp = np.array(want[0], np.float64), np.array(want[1], np.int32)
    assert got[0].shape == ws.shape and got[1].shape == wp.shape
    assert np.array_equal(got[1], wp), np.argwhere(got[1] != wp)[:5]
    assert np.array_equal(got[0], ws, equal_nan=True), np.argwhere(got[0] != ws)[:5]


# ---------------------------------------------------------------------------------------------------------------------
# the boundary
# ---------------------------------------------------------------------------------------------------------------------

def test_header_declares_and_both_libraries_export_the_entry_points(libs):
    txt = open(os.path.join(ROOT, "include", "hq_solver.h")).read()
    declared = re.findall(r"HQ_API\s+[\w\s\*]+?\b(hq\w+)\s*\(", txt)
    for n in NAMES:
        assert n in declared, n
        for lib in libs:
            assert hasattr(lib, n), n
    assert set(NAMES) <= set(capi.EXPORTS)
    htxt = open(os.path.join(ROOT, "include", "hq_host.h")).read()
    hlib = host.load_library()
    for n in ("hqh_cum_fold", "hqh_husid_cross"):
        assert re.search(r"HQ_API\s+int\s+%s\s*\(" % n, htxt), n
        assert n in host.EXPORTS and hasattr(hlib, n), n
    assert libs[0].hq_abi_version() == 6 and libs[1].hq_abi_version() == 6      # additive: no ABI bump


def test_null_context_is_a_bad_argument(libs):
    for lib in libs:
        ids = (ctypes.c_int32 * 1)(0)
        d = capi._CumDesc(1, 1, ctypes.cast(ids, ctypes.c_void_p), None, 1, 0, V, 0, 0, 0, (ctypes.c_double * 3)(0, 0, 0))
        h, nf, n = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
        sm, sp = (ctypes.c_double * 6)(), (ctypes.c_int32 * 3)()
        assert lib.hq_cum_add(None, ctypes.byref(d), ctypes.byref(h)) == HQ_ERR_ARG
        assert lib.hq_cum_fetch(None, ctypes.c_int32(0), sm, sp, None, None, ctypes.byref(nf), ctypes.byref(n)) == HQ_ERR_ARG
        assert lib.hq_cum_load(None, ctypes.c_int32(0), sm, sp, None, None, ctypes.c_int32(0), ctypes.c_int64(0)) == HQ_ERR_ARG
        assert lib.hq_cum_reset(None, ctypes.c_int32(0)) == HQ_ERR_ARG
        assert lib.hq_cum_clear(None) == HQ_ERR_ARG


def test_descriptor_mirrors_the_header(libs, tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hq_host.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(hq_cum_desc), offsetof(hq_cum_desc, ids), '
                   'offsetof(hq_cum_desc, quantities), offsetof(hq_cum_desc, husid_slots), offsetof(hq_cum_desc, threshold)); '
                   'return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    size, ids_off, q_off, hs_off, thr_off = [int(x) for x in subprocess.check_output([str(exe)], universal_newlines=True).split()]
    assert size == ctypes.sizeof(capi._CumDesc) == 72
    assert (ids_off, q_off, hs_off, thr_off) == (capi._CumDesc.ids.offset, capi._CumDesc.quantities.offset,
                                                 capi._CumDesc.husid_slots.offset, capi._CumDesc.threshold.offset)


# ---------------------------------------------------------------------------------------------------------------------
# hqh_cum_fold against the Python loop
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("q", MASKS)
def test_fold_equals_a_python_loop(q):
    """300 samples x 7 points, every mask, the samples of steps below first_step dropped as a caller drops a recorder's: bit
    equality.  And the case holds what it claims to: the tie does not count, one point never passes, one always does, the
    NaN stays in its sums and in no count."""
    steps, samples = _case(q)
    thr = _thresholds(q)
    keep = steps >= FIRST_STEP
    got = host.cum_fold(steps[keep], samples[keep], q, thr)
    want = _python_fold(steps, samples, q, thr, FIRST_STEP)
    _same(got, want)
    sums, span = got
    nkept = int(keep.sum())
    assert (sums[1] == 0).all() and (span[1] == (-1, -1, 0)).all()
    assert (span[3] == (-1, -1, 0)).all() and (sums[3] > 0).all()
    assert (span[5, :, 0] == FIRST_STEP).all() and (span[5, :, 1] == steps[-1]).all() and (span[5, :, 2] == nkept).all()
    assert np.isnan(sums[4][:, [1, 4]]).all() and np.isfinite(sums[4][:, [0, 2, 3, 5]]).all()
    assert (span[4, :, 2] < nkept).all()
    # the sample at the threshold: fold it alone -- nothing counted; a hair above -- counted
    one = samples[40:41, 2:3]
    assert (host.cum_fold(steps[40:41], one, q, thr)[1] == (-1, -1, 0)).all()
    above = one * (1.0 + 2.0 ** -52)
    assert (host.cum_fold(steps[40:41], above, q, thr)[1] == (steps[40], steps[40], 1)).all()


@pytest.mark.parametrize("q", [D | V | A, V])
def test_two_chunks_equal_one_fold(q):
    steps, samples = _case(q)
    thr = _thresholds(q)
    whole = host.cum_fold(steps, samples, q, thr)
    sums, span = host.cum_fold(steps[:113], samples[:113], q, thr)
    again = host.cum_fold(steps[113:], samples[113:], q, thr, sums, span)
    assert again[0] is sums and again[1] is span
    assert np.array_equal(sums, whole[0], equal_nan=True) and np.array_equal(span, whole[1])
    _same((sums, span), _python_fold(steps, samples, q, thr))


def test_bad_arguments():
    lib = host.load_library()
    sm, sp, st, smp = (ctypes.c_double * 18)(), (ctypes.c_int32 * 9)(), (ctypes.c_int32 * 1)(), (ctypes.c_double * 9)()
    thr = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    assert lib.hqh_cum_fold(1, 0, 1, st, smp, thr, sm, sp) == HQ_ERR_ARG
    assert lib.hqh_cum_fold(1, 8, 1, st, smp, thr, sm, sp) == HQ_ERR_ARG
    assert lib.hqh_cum_fold(-1, 7, 1, st, smp, thr, sm, sp) == HQ_ERR_ARG
    assert lib.hqh_cum_fold(1, 7, -1, st, smp, thr, sm, sp) == HQ_ERR_ARG
    assert lib.hqh_cum_fold(1, 7, 1, None, smp, thr, sm, sp) == HQ_ERR_ARG
    assert lib.hqh_cum_fold(1, 7, 1, st, smp, None, sm, sp) == HQ_ERR_ARG
    assert lib.hqh_cum_fold(1, 7, 1, st, smp, thr, None, sp) == HQ_ERR_ARG
    for bad in (-1.0, float("nan"), float("inf")):
        assert lib.hqh_cum_fold(1, 7, 1, st, smp, (ctypes.c_double * 3)(0.0, bad, 0.0), sm, sp) == HQ_ERR_ARG
    assert lib.hqh_cum_fold(1, 1, 1, st, smp, (ctypes.c_double * 3)(0.0, -1.0, 0.0), sm, sp) == 0   # (not of the mask: not read)
    assert lib.hqh_cum_fold(0, 7, 1, None, None, thr, None, None) == 0
    assert lib.hqh_cum_fold(1, 7, 1, st, smp, thr, sm, sp) == 0
    one = (ctypes.c_double * 1)(1.0)
    assert lib.hqh_husid_cross(-1, st, ctypes.c_double(0), ctypes.c_int64(1), one, one, 1, one, one) == HQ_ERR_ARG
    assert lib.hqh_husid_cross(1, None, ctypes.c_double(0), ctypes.c_int64(1), one, one, 1, one, one) == HQ_ERR_ARG
    assert lib.hqh_husid_cross(1, st, ctypes.c_double(0), ctypes.c_int64(1), one, None, 1, one, one) == HQ_ERR_ARG
    assert lib.hqh_husid_cross(1, st, ctypes.c_double(0), ctypes.c_int64(1), one, one, 1, one, None) == HQ_ERR_ARG
    assert lib.hqh_husid_cross(0, None, ctypes.c_double(0), ctypes.c_int64(0), None, None, 0, None, None) == 0


# ---------------------------------------------------------------------------------------------------------------------
# hqh_husid_cross
# ---------------------------------------------------------------------------------------------------------------------

HUSID_STEPS = [8, 16, 24, 32, 40]
HUSID_CURVE = [[0.0, 2.0, 0.0], [16.0, 2.0, 0.0], [16.0, 6.0, 0.0], [48.0, 6.0, 0.0], [56.0, 8.0, 0.0]]
HUSID_TOTAL = [64.0, 8.0, 0.0]
HUSID_FRACS = [0.125, 0.25, 0.5, 0.75, 0.8125, 0.9375]
HUSID_STEP0 = 4.0
# series 0: 0 up to step 8, then 2 per step to 16 at step 16, flat, 4 per step to 48 at step 32, 1 per step to 56 at step 40;
# the total 64 lies past the last slot.  Every number is a dyadic rational: the interpolation is exact.
HUSID_WANT0 = [12.0, 16.0, 28.0, 32.0, 36.0, math.nan]      # 8, 16, 32, 48, 52, 60 of 64
# series 1: reaches 2 in slot 0, from (step0, 0) = (4, 0): 0.5 per step; flat; 0.5 per step 16..24; flat; 0.25 per step 32..40
HUSID_WANT1 = [6.0, 8.0, 20.0, 24.0, 34.0, 38.0]            # 1, 2, 4, 6, 6.5, 7.5 of 8


def test_husid_cross_on_a_piecewise_linear_curve():
    out = host.husid_cross(HUSID_STEPS, np.array(HUSID_CURVE), np.array(HUSID_TOTAL), HUSID_FRACS, step0=HUSID_STEP0)
    assert out.shape == (3, 6)
    assert np.array_equal(out[0], HUSID_WANT0, equal_nan=True), out[0]
    assert np.array_equal(out[1], HUSID_WANT1, equal_nan=True), out[1]     # 6.0: a fraction below slot 0 uses step0
    assert np.isnan(out[2]).all()                                          # total = 0
    # a total that is not finite; no slots at all; the trailing shape of cum_fetch's curve
    assert np.isnan(host.husid_cross(HUSID_STEPS, np.array(HUSID_CURVE), np.array([np.inf, np.nan, 1.0]), [0.5])[:2]).all()
    assert np.isnan(host.husid_cross([], np.zeros((0, 3)), np.array(HUSID_TOTAL), [0.5])).all()
    cv = np.array(HUSID_CURVE)[:, None, :, None] * np.ones((1, 2, 1, 3))
    out4 = host.husid_cross(HUSID_STEPS, cv, np.array(HUSID_TOTAL)[None, :, None] * np.ones((2, 1, 3)), HUSID_FRACS, HUSID_STEP0)
    assert out4.shape == (2, 3, 3, 6) and np.array_equal(out4[1, 0, 2], HUSID_WANT0, equal_nan=True)
    assert np.array_equal(out4[0, 1, 1], HUSID_WANT1)


def test_d5_95_of_a_boxcar_is_nine_tenths_of_its_length():
    """A constant acceleration over samples 100 .. 299 (steps = samples), zero elsewhere; every 10th running sum stored: the
    Husid curve is a ramp, and D5-95 read from it is 0.9 x 200 steps."""
    a = np.zeros(400)
    a[100:300] = 2.0
    run = np.cumsum(a * a)
    steps = np.arange(9, 400, 10)
    out = host.husid_cross(steps, run[steps], run[-1:].reshape(()), [0.05, 0.95], step0=-1.0)
    assert abs((out[1] - out[0]) - 180.0) < 1e-9, out


# ---------------------------------------------------------------------------------------------------------------------
# the rectangle rule
# ---------------------------------------------------------------------------------------------------------------------

def test_arias_integral_from_the_sums():
    """a_i = A sin(omega t_i): pi / (2 g) h sum a_i^2 formed from the fold's sums against the same with the exactly summed
    squares (math.fsum) -- within 2 n 2^-53 relative, the bound for a sequential sum of n non-negative terms (n - 1 roundings
    of at most 2^-53 each; the rounding of the products and of the two scalings stays below the other n)."""
    n, h, g, amp, omega = 4000, 2.5e-3, 9.81, 3.7, 2 * math.pi * 1.3
    t = h * np.arange(n)
    acc = np.zeros((n, 1, 9))
    acc[:, 0, 6] = amp * np.sin(omega * t)
    acc[:, 0, 7] = 0.5 * amp * np.cos(omega * t)
    sums, span = host.cum_fold(np.arange(n), acc, A, 0.5 * amp)
    for axis in (0, 1):
        a = acc[:, 0, 6 + axis]
        exact = math.pi / (2 * g) * h * math.fsum(float(v) * float(v) for v in a)
        got = math.pi / (2 * g) * h * sums[0, 0, 3 + axis]
        assert exact > 0 and abs(got - exact) <= 2 * n * 2.0 ** -53 * exact, (axis, got, exact)
        cav = h * sums[0, 0, axis]
        assert abs(cav - h * math.fsum(abs(float(v)) for v in a)) <= 2 * n * 2.0 ** -53 * cav
    # the analytic value over whole periods is A^2 T / 2: the rectangle rule on a sine is that good
    assert abs(h * sums[0, 0, 3] - amp * amp * n * h / 2) < 1e-2 * amp * amp * n * h / 2
    assert 0 < span[0, 0, 2] < n and span[0, 0, 0] >= 0 and span[0, 0, 1] > span[0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------
# the code object
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("so", ["libhq_solver.so", "libhq_solver_f32.so"])
def test_cum_kernels_have_no_spill_and_no_scratch(libs, tmp_path, monkeypatch, so):
    """hq_k_cum<1> and hq_k_cum<8> sit at the head of every due step beside the stepping kernels: no spilled register, no
    scratch, no LDS.  The node form, which a whole surface goes through, also keeps to 64 registers -- eight waves per SIMD."""
    path = os.path.join(ROOT, "hercules_amd", "csrc", so)
    assert os.path.exists(path), path
    monkeypatch.setattr(sys.modules[CO.__name__], "SO", path)
    k = CO._kernel_notes(tmp_path)
    found = {}
    for name, v in k.items():
        for tag in ("hq_k_cumILi1EE", "hq_k_cumILi8EE"):
            if tag in name:
                found[tag] = v
    assert sorted(found) == ["hq_k_cumILi1EE", "hq_k_cumILi8EE"], sorted(k)
    for tag, v in found.items():
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (tag, v)
        assert v["group_segment_fixed_size"] == 0, (tag, v)
    assert found["hq_k_cumILi1EE"]["vgpr_count"] <= 64, found


def _write_case(path):
    """The fold case of this file for tests/cumul_host_main.c: int32 npoints, quantities, nsamples, nkept chunk cut; then steps,
    samples, the three thresholds, and the Python loop's sums and span."""
    q = D | V | A
    steps, samples = _case(q)
    thr = _thresholds(q)
    sums, span = _python_fold(steps, samples, q, thr)
    with open(path, "wb") as f:
        f.write(np.array([NPOINTS, q, NSAMPLES, 113], np.int32).tobytes())
        f.write(steps.tobytes())
        f.write(samples.tobytes())
        f.write(np.array(thr, np.float64).tobytes())
        f.write(np.array(sums, np.float64).tobytes())
        f.write(np.array(span, np.int32).tobytes())


if __name__ == "__main__":
    _write_case(sys.argv[1])
