"""CPU-side checks of the field snapshots' boundary (include/hq_solver.h: hq_snapshot_*; include/hq_host.h:
hqh_solver_run_async, hqh_checkpoint_write_fields): the symbols exist, refuse a null context, the ctypes mirrors have the
header's sizes, and the file half of the checkpoint writer produces the documented format.  No compute calls here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import hercules_amd as ha
from hercules_amd import build as hbuild
from hercules_amd import capi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["hq_snapshot_add", "hq_snapshot_pending", "hq_snapshot_fetch", "hq_snapshot_clear"]
HOST_NAMES = ["hqh_solver_run_async", "hqh_checkpoint_write_fields"]
HQ_ERR_ARG = -1


@pytest.fixture(scope="module")
def libs():
    hbuild.build()
    return ha.load_library(), capi.load_library(precision="f32")


def test_both_libraries_export_the_snapshot_entry_points(libs):
    for lib in libs:
        for n in NAMES:
            assert hasattr(lib, n), n
    assert set(NAMES) <= set(capi.EXPORTS)
    assert libs[0].hq_abi_version() == 6                 # additive: no ABI bump
    hl = host.load_library()
    for n in HOST_NAMES:
        assert hasattr(hl, n), n
    assert set(HOST_NAMES) <= set(host.EXPORTS)
    assert (capi.HQ_SNAP_TM1, capi.HQ_SNAP_TM2, capi.HQ_SNAP_VEL) == (1, 2, 4)


def test_null_context_is_a_bad_argument(libs):
    for lib in libs:
        d = capi._SnapshotDesc(0, 1, 1, 0, capi.HQ_SNAP_TM1, 1)
        h, n, ready, first = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        assert lib.hq_snapshot_add(None, ctypes.byref(d), ctypes.byref(h)) == HQ_ERR_ARG
        assert lib.hq_snapshot_pending(None, ctypes.c_int32(0), ctypes.byref(n), ctypes.byref(ready),
                                       ctypes.byref(first)) == HQ_ERR_ARG
        assert lib.hq_snapshot_fetch(None, ctypes.c_int32(0), None, None, None, ctypes.byref(first)) == HQ_ERR_ARG
        assert lib.hq_snapshot_clear(None) == HQ_ERR_ARG
    rp = host.run_params()
    assert host.load_library().hqh_solver_run_async(None, ctypes.c_double(1e-3), ctypes.c_int32(8), ctypes.byref(rp),
                                                    ctypes.c_int32(0), ctypes.c_int32(1), ctypes.c_int32(1)) == HQ_ERR_ARG


def test_descriptor_and_run_params_mirror_the_header(libs, tmp_path):
    """sizeof(hq_snapshot_desc), asked of a C compiler, is the ctypes mirror's; hqh_run_params has not grown: its size and
    the offset of its last field, device_recorders, are still the mirror's."""
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hq_host.h"\n'
                   'int main(void) { printf("%zu %zu %zu %d %d %d\\n", sizeof(hq_snapshot_desc), sizeof(hqh_run_params), '
                   'offsetof(hqh_run_params, device_recorders), HQ_SNAP_TM1, HQ_SNAP_TM2, HQ_SNAP_VEL); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    dsize, size, off, b1, b2, b4 = [int(v) for v in subprocess.check_output([str(exe)], universal_newlines=True).split()]
    assert dsize == ctypes.sizeof(capi._SnapshotDesc) == 24
    assert [n for n, _ in capi._SnapshotDesc._fields_] == ["first", "count", "rate", "first_step", "fields", "slots"]
    assert size == ctypes.sizeof(host._RunParams)
    assert host._RunParams._fields_[-1][0] == "device_recorders" and off == host._RunParams.device_recorders.offset
    assert (b1, b2, b4) == (capi.HQ_SNAP_TM1, capi.HQ_SNAP_TM2, capi.HQ_SNAP_VEL)


def _numpy_checkpoint(nranks, step, nmax, stripes):
    """checkpoint.out as include/hq_host.h documents it: {groupsize, step, nharboredmax} ints; rank r's stripe at
    12 + 2 r nharboredmax 24: u((step-1) dt) then u(step dt), nharbored fvector_t each.  stripes = {rank: (tm1, tm2)}."""
    end = max(12 + 2 * r * nmax * 24 + 2 * len(t1) * 24 for r, (t1, _) in stripes.items())
    raw = bytearray(end)
    raw[:12] = np.array([nranks, step, nmax], "<i4").tobytes()
    for r, (t1, t2) in stripes.items():
        at = 12 + 2 * r * nmax * 24
        raw[at:at + len(t2) * 24] = np.asarray(t2, "<f8").tobytes()
        raw[at + len(t2) * 24:at + 2 * len(t2) * 24] = np.asarray(t1, "<f8").tobytes()
    return bytes(raw)


def test_checkpoint_write_fields_writes_the_documented_format(libs, tmp_path):
    rng = np.random.default_rng(3)
    n = 37
    tm1, tm2 = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    p = tmp_path / "checkpoint.out0"
    host.checkpoint_write_fields(str(p), 120, tm1, tm2)
    raw = p.read_bytes()
    assert raw == _numpy_checkpoint(1, 120, n, {0: (tm1, tm2)})
    # hqh_checkpoint_read's format checks: the rank count, nharbored <= nharboredmax, both stripes present
    hdr = np.frombuffer(raw[:12], "<i4")
    assert list(hdr) == [1, 120, n] and len(raw) == 12 + 2 * n * 24
    # two ranks of unequal size, rank 0 first (it creates the file), stripes nharboredmax apart
    a1, a2 = rng.standard_normal((5, 3)), rng.standard_normal((5, 3))
    b1, b2 = rng.standard_normal((9, 3)), rng.standard_normal((9, 3))
    q = tmp_path / "checkpoint.out1"
    host.checkpoint_write_fields(str(q), 7, a1, a2, rank=0, nranks=2, nharboredmax=9)
    host.checkpoint_write_fields(str(q), 7, b1, b2, rank=1, nranks=2, nharboredmax=9)
    assert q.read_bytes() == _numpy_checkpoint(2, 7, 9, {0: (a1, a2), 1: (b1, b2)})
    # refused: a rank outside the group, more nodes than nharboredmax, a missing field
    for kw in (dict(rank=2, nranks=2), dict(nharboredmax=n - 1)):
        with pytest.raises(capi.HqError):
            host.checkpoint_write_fields(str(tmp_path / "bad"), 1, tm1, tm2, **kw)
    rc = host.load_library().hqh_checkpoint_write_fields(os.fsencode(str(tmp_path / "bad")), ctypes.c_int32(1),
                                                         ctypes.c_int32(0), ctypes.c_int32(1), ctypes.c_int32(n),
                                                         ctypes.c_int32(n), tm1.ctypes.data_as(ctypes.c_void_p), None)
    assert rc == HQ_ERR_ARG and not (tmp_path / "bad").exists()
