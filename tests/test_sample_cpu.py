"""hq_sample.h -- the one text of the point sample that hq_k_record, hq_k_peak and hqh_station_kinematics compile -- against
the same sums written in numpy float64 operation by operation (numpy does not contract), bit for bit.  A small C program
with its own main that includes the header, compiled with gcc for double and for float fields; no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from hercules_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hercules_amd", "csrc")

# probe K in out: `in` holds int64 n, nn; then ids [n][8] int64, weights [n][8] double, the fields u1, u2, u3 [nn][3] REAL.
# `out` gets [n][9] doubles: the accumulator behind the displacement, the velocity and the acceleration stage (not divided).
# K = 1: the first node of every point, no weight table.
PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "hq_sample.h"

static void* take(FILE* f, size_t size, size_t count)
{
    void* p = malloc(size * (count ? count : 1));
    if (!p || fread(p, size, count, f) != count) exit(2);
    return p;
}

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    const int K = atoi(argv[1]);
    FILE* f = fopen(argv[2], "rb");
    int64_t hdr[2];
    if (!f || fread(hdr, 8, 2, f) != 2) return 2;
    const size_t n = (size_t)hdr[0], nn = (size_t)hdr[1];
    int64_t* ids = (int64_t*)take(f, 8, 8 * n);
    double* w = (double*)take(f, 8, 8 * n);
    HQ_SAMPLE_REAL* u1 = (HQ_SAMPLE_REAL*)take(f, sizeof(HQ_SAMPLE_REAL), 3 * nn);
    HQ_SAMPLE_REAL* u2 = (HQ_SAMPLE_REAL*)take(f, sizeof(HQ_SAMPLE_REAL), 3 * nn);
    HQ_SAMPLE_REAL* u3 = (HQ_SAMPLE_REAL*)take(f, sizeof(HQ_SAMPLE_REAL), 3 * nn);
    fclose(f);
    FILE* o = fopen(argv[3], "wb");
    if (!o) return 2;
    for (size_t p = 0; p < n; p++) {
        int64_t row[8];
        for (int c = 0; c < 8; c++) row[c] = 3 * ids[8 * p + c];
        const double* wp = K == 1 ? NULL : w + 8 * p;
        double d[3] = { 0.0, 0.0, 0.0 }, out[9];
        hq_sample_disp(K, wp, row, u1, d);
        for (int a = 0; a < 3; a++) out[a] = d[a];
        hq_sample_vel(K, wp, row, u2, d);
        for (int a = 0; a < 3; a++) out[3 + a] = d[a];
        hq_sample_acc(K, wp, row, u2, u3, d);
        for (int a = 0; a < 3; a++) out[6 + a] = d[a];
        if (fwrite(out, 8, 9, o) != 9) return 2;
    }
    return fclose(o) == 0 ? 0 : 2;
}
"""

N, NN = 257, 96


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    """The probe as the host library is built (gcc -O2 -std=gnu99, no FMA), for double and for float fields."""
    d = tmp_path_factory.mktemp("sample")
    (d / "sample_probe.c").write_text(PROGRAM)
    exes = {}
    for name, real in (("f64", "double"), ("f32", "float")):
        exes[name] = d / ("probe_" + name)
        subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-Wall", "-Wextra", "-Werror", "-DHQ_SAMPLE_REAL=" + real, "-I", CSRC,
                               "-o", str(exes[name]), str(d / "sample_probe.c")])
    exes["dir"] = d
    return exes


def _probe(probes, which, K, ids, w, fields):
    d = probes["dir"]
    fin, fout = d / "in.bin", d / "out.bin"
    dtype = np.float64 if which == "f64" else np.float32
    with open(fin, "wb") as f:
        f.write(np.array([len(ids), fields[0].shape[0]], np.int64).tobytes())
        f.write(np.ascontiguousarray(ids, np.int64).tobytes())
        f.write(np.ascontiguousarray(w, np.float64).tobytes())
        for u in fields:
            assert u.dtype == dtype
            f.write(np.ascontiguousarray(u).tobytes())
    subprocess.check_call([str(probes[which]), str(K), str(fin), str(fout)])
    return np.fromfile(fout, np.float64).reshape(len(ids), 9)


def _numpy_stages(ids, w, fields):
    """The header's sums, one numpy float64 operation per C operation, in the header's order: nodes outside, axes inside."""
    u1, u2, u3 = (u.astype(np.float64) for u in fields)
    n = len(ids)
    d = np.zeros((n, 3))
    out = np.zeros((n, 9))
    for c in range(8):
        for a in range(3):
            d[:, a] = d[:, a] + w[:, c] * u1[ids[:, c], a]
    out[:, 0:3] = d
    for c in range(8):
        for a in range(3):
            d[:, a] = d[:, a] - w[:, c] * u2[ids[:, c], a]
    out[:, 3:6] = d
    for c in range(8):
        for a in range(3):
            d[:, a] = d[:, a] - w[:, c] * u2[ids[:, c], a]
            d[:, a] = d[:, a] + w[:, c] * u3[ids[:, c], a]
    out[:, 6:9] = d
    return out


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _case(seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, NN, size=(N, 8))
    w = rng.uniform(0.0, 1.0, size=(N, 8))
    w /= w.sum(axis=1, keepdims=True)                           # trilinear weights sum to 1; the sums do not depend on it
    fields = [(rng.normal(size=(NN, 3)) * 10.0 ** rng.integers(-6, 3, size=(NN, 1))).astype(dtype) for _ in range(3)]
    return ids, w, fields


def test_eight_node_stages_equal_numpy_bit_for_bit(probes):
    for seed in (1, 2, 3):
        ids, w, fields = _case(seed)
        got = _probe(probes, "f64", 8, ids, w, fields)
        assert np.array_equal(_bits(got), _bits(_numpy_stages(ids, w, fields)))
        assert np.all(np.isfinite(got)) and np.count_nonzero(got) > 8 * N


def test_one_node_equals_unit_weights_bit_for_bit(probes):
    """K = 1 without a weight table against K = 8 with weights (1, 0, ..., 0) -- rows of negative zeros, denormals and
    exact cancellations (u1 == u2, u1 - 2 u2 + u3 == 0) among the nodes."""
    for which, dtype in (("f64", np.float64), ("f32", np.float32)):
        ids, w, fields = _case(11, dtype)
        tiny = np.finfo(dtype).tiny
        special = np.array([[-0.0, 0.0, -0.0], [tiny / 4, -tiny / 8, tiny / 2], [-0.0, tiny / 16, 1.0], [0.0, 0.0, 0.0]], dtype)
        for k, u in enumerate(fields):
            u[:8] = np.roll(np.concatenate([special, -special]), k, axis=0)
        fields[1][8:12] = fields[0][8:12]                       # u1 == u2
        fields[2][8:12] = fields[0][8:12]                       # ... == u3
        ids[:16, 0] = np.arange(16) % 12                        # the first nodes of the first points: the special rows
        ids[16:32, 1:] = np.arange(16)[:, None] % 8             # ... and special rows under the zero weights
        w[:] = 0.0
        w[:, 0] = 1.0
        one = _probe(probes, which, 1, ids, w, fields)
        eight = _probe(probes, which, 8, ids, w, fields)
        assert np.array_equal(_bits(one), _bits(eight))
        u1, u2, u3 = (u.astype(np.float64)[ids[:, 0]] for u in fields)
        assert np.array_equal(_bits(one), _bits(np.hstack([0.0 + u1, (0.0 + u1) - u2, ((0.0 + u1) - u2) - u2 + u3])))


def test_float_fields_are_widened_first(probes):
    ids, w, fields = _case(21, np.float32)
    got = _probe(probes, "f32", 8, ids, w, fields)
    wide = _probe(probes, "f64", 8, ids, w, [u.astype(np.float64) for u in fields])
    assert np.array_equal(_bits(got), _bits(wide))
    assert np.array_equal(_bits(got), _bits(_numpy_stages(ids, w, fields)))


def test_host_library_returns_the_probes_bits(probes):
    """hqh_station_kinematics (libhq_host.so) on contiguous [8][3] blocks: the probe's accumulators over dt and dt * dt."""
    lib = host.load_library()
    ids, w, fields = _case(31)
    acc = _probe(probes, "f64", 8, ids, w, fields)
    dt = 1.25e-3
    want = np.hstack([acc[:, 0:3], acc[:, 3:6] / dt, acc[:, 6:9] / (dt * dt)])
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    for derivs in (0, 1, 2):
        ncomp = 3 * (1 + derivs)
        for p in range(0, N, 7):
            blocks = [np.ascontiguousarray(u[ids[p]]) for u in fields]
            out = np.zeros(ncomp)
            phi = np.ascontiguousarray(w[p])
            rc = lib.hqh_station_kinematics(ptr(phi), ptr(blocks[0]), ptr(blocks[1]), ptr(blocks[2]), ctypes.c_double(dt),
                                            ctypes.c_int32(derivs), ptr(out))
            assert rc == 0
            assert np.array_equal(_bits(out), _bits(want[p, :ncomp])), (derivs, p)


def test_sample_header_needs_no_other_header_of_the_package():
    text = open(os.path.join(CSRC, "hq_sample.h")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes == ["<stdint.h>"]
