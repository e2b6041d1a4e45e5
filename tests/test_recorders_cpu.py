"""CPU-side checks of the device recorders' boundary (include/hq_solver.h: hq_record_*; include/hq_host.h:
hqh_run_params.device_recorders): the symbols exist in both libraries, refuse a null context, and the ctypes mirror
of hqh_run_params has the header's size.  No compute calls here."""
import ctypes
import os
import subprocess

import pytest

import hercules_amd as ha
from hercules_amd import build as hbuild
from hercules_amd import capi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["hq_record_add", "hq_record_pending", "hq_record_fetch", "hq_record_clear"]
HQ_ERR_ARG = -1


@pytest.fixture(scope="module")
def libs():
    hbuild.build()
    return ha.load_library(), capi.load_library(precision="f32")


def test_both_libraries_export_the_recorder_entry_points(libs):
    for lib in libs:
        for n in NAMES:
            assert hasattr(lib, n), n
    assert set(NAMES) <= set(capi.EXPORTS)
    assert libs[0].hq_abi_version() == 6                 # additive: no ABI bump


def test_null_context_is_a_bad_argument(libs):
    for lib in libs:
        d = capi._RecorderDesc(0, None, None, 1, 0, 1)
        h, n, first = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        out, steps = (ctypes.c_double * 9)(), (ctypes.c_int32 * 1)()
        assert lib.hq_record_add(None, ctypes.byref(d), ctypes.byref(h)) == HQ_ERR_ARG
        assert lib.hq_record_pending(None, ctypes.c_int32(0), ctypes.byref(n), ctypes.byref(first)) == HQ_ERR_ARG
        assert lib.hq_record_fetch(None, ctypes.c_int32(0), ctypes.c_int32(1), out, steps, ctypes.byref(n)) == HQ_ERR_ARG
        assert lib.hq_record_clear(None) == HQ_ERR_ARG


def test_run_params_mirror_the_header(libs, tmp_path):
    """device_recorders is the struct's LAST field and defaults to 0; sizeof(hqh_run_params) and the field's offset, asked
    of a C compiler, are those of the ctypes mirror."""
    assert host.run_params().device_recorders == 0
    assert host.run_params(device_recorders=1).device_recorders == 1
    assert host._RunParams._fields_[-1][0] == "device_recorders"
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hq_host.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(hqh_run_params), '
                   'offsetof(hqh_run_params, device_recorders), sizeof(hq_recorder_desc)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    size, off, dsize = [int(v) for v in subprocess.check_output([str(exe)], universal_newlines=True).split()]
    assert size == ctypes.sizeof(host._RunParams)
    assert off == host._RunParams.device_recorders.offset
    assert dsize == ctypes.sizeof(capi._RecorderDesc)
