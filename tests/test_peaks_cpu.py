"""CPU-side checks of the peak-motion trackers' boundary (include/hq_solver.h: hq_peak_*; include/hq_host.h: hqh_peak_fold;
csrc/hq_peak.h, the one text of the fold): the symbols exist in both libraries and refuse a null context, the ctypes mirror of
hq_peak_desc has the header's size, hqh_peak_fold does what a few lines of numpy do -- negative values, ties, all-zero
points, NaNs, two calls in sequence, a mask that skips velocity -- and hipcc left both forms of hq_k_peak without spills or
scratch in both libraries.  No GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import hercules_amd as ha
from hercules_amd import build as hbuild
from hercules_amd import capi, host
from tests import test_code_object_cpu as CO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["hq_peak_add", "hq_peak_fetch", "hq_peak_load", "hq_peak_reset", "hq_peak_clear"]
HQ_ERR_ARG = -1
D, V, A = capi.HQ_PEAK_DISP, capi.HQ_PEAK_VEL, capi.HQ_PEAK_ACC


@pytest.fixture(scope="module")
def libs():
    hbuild.build()
    return ha.load_library(), capi.load_library(precision="f32")


def test_both_libraries_export_the_tracker_entry_points(libs):
    for lib in libs:
        for n in NAMES:
            assert hasattr(lib, n), n
    assert set(NAMES) <= set(capi.EXPORTS)
    assert "hqh_peak_fold" in host.EXPORTS and hasattr(host.load_library(), "hqh_peak_fold")
    assert libs[0].hq_abi_version() == 6 and libs[1].hq_abi_version() == 6      # additive: no ABI bump


def test_null_context_is_a_bad_argument(libs):
    for lib in libs:
        ids = (ctypes.c_int32 * 1)(0)
        d = capi._PeakDesc(1, 1, ctypes.cast(ids, ctypes.c_void_p), None, 1, 0, V, 0)
        h, n = ctypes.c_int32(), ctypes.c_int64()
        pk, wh = (ctypes.c_double * 5)(), (ctypes.c_int32 * 2)()
        assert lib.hq_peak_add(None, ctypes.byref(d), ctypes.byref(h)) == HQ_ERR_ARG
        assert lib.hq_peak_fetch(None, ctypes.c_int32(0), pk, wh, ctypes.byref(n)) == HQ_ERR_ARG
        assert lib.hq_peak_load(None, ctypes.c_int32(0), pk, wh, ctypes.c_int64(0)) == HQ_ERR_ARG
        assert lib.hq_peak_reset(None, ctypes.c_int32(0)) == HQ_ERR_ARG
        assert lib.hq_peak_clear(None) == HQ_ERR_ARG


def test_descriptor_mirrors_the_header(libs, tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hq_host.h"\n'
                   'int main(void) { printf("%zu %zu %zu %d %d %d\\n", sizeof(hq_peak_desc), offsetof(hq_peak_desc, ids), '
                   'offsetof(hq_peak_desc, quantities), HQ_PEAK_DISP, HQ_PEAK_VEL, HQ_PEAK_ACC); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    size, ids_off, q_off, d, v, a = [int(x) for x in subprocess.check_output([str(exe)], universal_newlines=True).split()]
    assert size == ctypes.sizeof(capi._PeakDesc) == 40
    assert ids_off == capi._PeakDesc.ids.offset and q_off == capi._PeakDesc.quantities.offset
    assert (d, v, a) == (D, V, A) == (1, 2, 4)


# ---------------------------------------------------------------------------------------------------------------------
# hqh_peak_fold against numpy
# ---------------------------------------------------------------------------------------------------------------------

def _numpy_fold(steps, samples, quantities):
    """The fold in numpy: per quantity max |x|, |y|, |z|, max of x x + y y and of (x x + y y) + z z with the step of its
    FIRST occurrence (np.argmax's); a maximum of 0 (or no finite comparison at all) leaves `when` at -1; NaNs count as
    -inf.  Elementwise numpy products and sums are single IEEE operations: nothing is contracted."""
    nq = bin(quantities).count("1")
    npts = samples.shape[1]
    peaks, when = np.zeros((npts, nq, 5)), np.full((npts, nq, 2), -1, np.int32)
    qi = 0
    for q in range(3):
        if not quantities & (1 << q):
            continue
        v = samples[:, :, 3 * q:3 * q + 3]
        h = v[:, :, 0] * v[:, :, 0] + v[:, :, 1] * v[:, :, 1]
        t = h + v[:, :, 2] * v[:, :, 2]
        cols = [np.abs(v[:, :, 0]), np.abs(v[:, :, 1]), np.abs(v[:, :, 2]), h, t]
        for j, c in enumerate(cols):
            c = np.where(np.isnan(c), -np.inf, c)
            k = np.argmax(c, axis=0)
            m = c[k, np.arange(npts)]
            peaks[:, qi, j] = np.maximum(m, 0.0)
            if j >= 3:
                when[:, qi, j - 3] = np.where(m > 0.0, np.asarray(steps)[k], -1)
        qi += 1
    return peaks, when


def _samples(seed, nsamples=37, npts=23, derivs=2):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((nsamples, npts, 3 * (1 + derivs))) * 10.0 ** rng.integers(-6, 6, (1, npts, 1))
    steps = (np.arange(nsamples) * 3 + 6).astype(np.int32)
    return steps, s


def test_fold_equals_numpy_on_random_samples():
    steps, s = _samples(1)
    assert (s < 0).any()
    for q, cols in ((D | V | A, 9), (D | V, 6), (D, 3), (V, 6), (A, 9), (V | A, 9)):
        peaks, when = host.peak_fold(steps, s[:, :, :cols], q)
        wp, ww = _numpy_fold(steps, s, q)
        assert peaks.shape == (23, bin(q).count("1"), 5) and when.dtype == np.int32
        assert np.array_equal(peaks, wp) and np.array_equal(when, ww), q
        assert (when >= 6).all() and len(np.unique(when)) > 5


def test_negative_values_count_by_magnitude():
    s = np.zeros((3, 1, 3))
    s[:, 0, 0] = [1.0, -4.0, 3.0]
    s[:, 0, 2] = [-0.5, 0.25, -7.0]
    peaks, when = host.peak_fold([0, 1, 2], s, D)
    assert peaks[0, 0].tolist() == [4.0, 0.0, 7.0, 16.0, 9.0 + 49.0]
    assert when[0, 0].tolist() == [1, 2]


def test_a_tie_keeps_the_first_occurrence():
    s = np.zeros((5, 2, 3))
    s[:, 0, 0] = [1.0, 3.0, -3.0, 3.0, 2.0]              # horizontal 9 at steps 10, 20, 30: 10 stays
    s[:, 1, 1] = [2.0, 2.0, 2.0, 2.0, 2.0]
    peaks, when = host.peak_fold([0, 10, 20, 30, 40], s, D)
    assert when[0, 0].tolist() == [10, 10] and peaks[0, 0, 3] == 9.0
    assert when[1, 0].tolist() == [0, 0]
    assert np.array_equal(peaks, _numpy_fold([0, 10, 20, 30, 40], s, D)[0])


def test_an_all_zero_point_is_never_raised():
    steps, s = _samples(2, derivs=1)
    s[:, 4, :] = 0.0
    s[:, 5, :] = -0.0
    s[:, 6, [0, 1, 3, 4]] = 0.0                          # x and y of both quantities: horizontal never raised, total is
    peaks, when = host.peak_fold(steps, s, D | V)
    assert (peaks[4] == 0).all() and (when[4] == -1).all() and (when[5] == -1).all()
    assert (when[6, :, 0] == -1).all() and (when[6, :, 1] >= 0).all() and (peaks[6, :, 4] > 0).all()
    wp, ww = _numpy_fold(steps, s, D | V)
    assert np.array_equal(peaks, wp) and np.array_equal(when, ww)


def test_a_nan_never_enters_and_later_samples_still_count():
    steps, s = _samples(3)
    s[5, 2, :] = np.nan                                  # a whole sample of one point
    s[7, 3, 4] = np.nan                                  # one component: its own column, the horizontal and the total skip it
    s[0, 8, :] = np.nan                                  # the very first sample
    big = np.abs(s[np.isfinite(s)]).max()
    s[20, 2, :] = 2 * big                                # ... and a later one is the maximum
    peaks, when = host.peak_fold(steps, s, D | V | A)
    assert np.isfinite(peaks).all()
    assert (when[2] == steps[20]).all() and (peaks[2, :, :3] == 2 * big).all()
    assert (when[8] > steps[0]).all()
    wp, ww = _numpy_fold(steps, s, D | V | A)
    assert np.array_equal(peaks, wp) and np.array_equal(when, ww)


def test_two_calls_in_sequence_equal_one_on_the_concatenation():
    steps, s = _samples(4)
    s[30, :, :] = s[10, :, :]                            # ties across the cut: the first call's step stays
    one = host.peak_fold(steps, s, D | A)
    peaks, when = host.peak_fold(steps[:17], s[:17], D | A)
    p2, w2 = host.peak_fold(steps[17:], s[17:], D | A, peaks, when)
    assert p2 is peaks and w2 is when
    assert np.array_equal(peaks, one[0]) and np.array_equal(when, one[1])
    empty = host.peak_fold(steps[:0], s[:0], D | A, peaks.copy(), when.copy())
    assert np.array_equal(empty[0], peaks) and np.array_equal(empty[1], when)


def test_a_mask_that_skips_velocity():
    """DISP | ACC: the samples still have the recorder's nine columns (derivs = 2); the state has two quantities, the
    displacement's and the acceleration's, in that order."""
    steps, s = _samples(5)
    peaks, when = host.peak_fold(steps, s, D | A)
    full = host.peak_fold(steps, s, D | V | A)
    assert peaks.shape == (23, 2, 5)
    assert np.array_equal(peaks, full[0][:, [0, 2]]) and np.array_equal(when, full[1][:, [0, 2]])
    assert not np.array_equal(peaks[:, 1], full[0][:, 1])


def test_bad_arguments():
    lib = host.load_library()
    pk, wh, st, sm = (ctypes.c_double * 15)(), (ctypes.c_int32 * 6)(), (ctypes.c_int32 * 1)(), (ctypes.c_double * 9)()
    assert lib.hqh_peak_fold(1, 0, 1, st, sm, pk, wh) == HQ_ERR_ARG
    assert lib.hqh_peak_fold(1, 8, 1, st, sm, pk, wh) == HQ_ERR_ARG
    assert lib.hqh_peak_fold(-1, 7, 1, st, sm, pk, wh) == HQ_ERR_ARG
    assert lib.hqh_peak_fold(1, 7, -1, st, sm, pk, wh) == HQ_ERR_ARG
    assert lib.hqh_peak_fold(1, 7, 1, None, sm, pk, wh) == HQ_ERR_ARG
    assert lib.hqh_peak_fold(1, 7, 1, st, sm, None, wh) == HQ_ERR_ARG
    assert lib.hqh_peak_fold(0, 7, 1, None, None, None, None) == 0
    assert lib.hqh_peak_fold(1, 7, 1, st, sm, pk, wh) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the code object
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("so", ["libhq_solver.so", "libhq_solver_f32.so"])
def test_peak_kernels_have_no_spill_and_no_scratch(tmp_path, monkeypatch, so):
    """hq_k_peak<1> and hq_k_peak<8> sit at the head of every due step beside the stepping kernels: no spilled register, no
    scratch, no LDS.  The node form, which a whole surface goes through, also keeps to 64 registers -- eight waves per SIMD:
    a gather kernel lives on loads in flight (the element form holds its 8 x 9 gathered values at once instead)."""
    path = os.path.join(ROOT, "hercules_amd", "csrc", so)
    if not os.path.exists(path):
        pytest.skip("%s is not built" % so)
    monkeypatch.setattr(sys.modules[CO.__name__], "SO", path)
    k = CO._kernel_notes(tmp_path)
    found = {}
    for name, v in k.items():
        for tag in ("hq_k_peakILi1EE", "hq_k_peakILi8EE"):
            if tag in name:
                found[tag] = v
    assert sorted(found) == ["hq_k_peakILi1EE", "hq_k_peakILi8EE"], sorted(k)
    for tag, v in found.items():
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (tag, v)
        assert v["group_segment_fixed_size"] == 0, (tag, v)
    assert found["hq_k_peakILi1EE"]["vgpr_count"] <= 64, found
