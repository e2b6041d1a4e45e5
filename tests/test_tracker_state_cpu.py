"""hq_state_table.h -- a tracker's state table between the device's layout ([slots][rows][np]) and the caller's
([slots][np][rows]) -- against numpy's transposition, written out here.  One C++ program with its own main moves patterned
tables both ways between guarded buffers and writes down what it was given and what came out; the comparison is made in
Python.  No device, no library of the package."""
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hercules_amd", "csrc")

NPS = (0, 1, 3, 257)
ROWS = (1, 3, 5, 24)
# (element size, np, rows, slots): both element types on every shape, then a Husid curve of 0, 1 and 3 filled slots of [nq][3][np]
CASES = ([(es, n, r, 1) for es, n, r in itertools.product((8, 4), NPS, ROWS)] +
         [(8, n, 3 * nq, slots) for slots, nq, n in itertools.product((0, 1, 3), (1, 3), NPS)])

PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "hq_state_table.h"

static const uint64_t GUARD = 0xA5C3965A0FF01E87ull;
enum { NGUARD = 8 };

/* `bytes` of payload with guard words on both sides; the payload starts out as 0xEE */
struct guarded {
    std::vector<uint64_t> words;
    size_t bytes;
    explicit guarded(size_t b) : words(2 * NGUARD + (b + 7) / 8, GUARD), bytes(b) { memset(data(), 0xEE, b); }
    unsigned char* data() { return (unsigned char*)(words.data() + NGUARD); }
    bool intact()
    {
        const std::vector<uint64_t> fresh(words.size(), GUARD);
        const unsigned char* f = (const unsigned char*)fresh.data();
        const unsigned char* w = (const unsigned char*)words.data();
        const size_t lo = 8 * NGUARD, hi = lo + bytes, end = 8 * words.size();
        return memcmp(w, f, lo) == 0 && memcmp(w + hi, f + hi, end - hi) == 0;
    }
};

static void pattern(void* p, size_t esize, size_t n, uint32_t seed)
{
    for (size_t i = 0; i < n; i++) {
        if (esize == 8) ((double*)p)[i] = (double)((int64_t)seed + 3 * (int64_t)i) / 7.0 - 1000.0;
        else ((int32_t*)p)[i] = (int32_t)((seed + (uint32_t)i) * 2654435761u);
    }
}

#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s (esize %zu np %zu rows %zu slots %zu)\n", __LINE__, #cond, \
                                               tb.esize, np, tb.rows, tb.slots); exit(1); } } while (0)

static long ncases = 0;

/* one table: device -> caller, caller -> device, and there and back; every buffer written to the file as it stands */
static void one(FILE* f, size_t esize, size_t np, size_t rows, size_t slots)
{
    const hq_state_table tb = { nullptr, nullptr, esize, rows, slots, 0, 0, false };
    const size_t bytes = hq_state_table_bytes(tb, np), n = rows * slots * np;
    CHECK(bytes == esize * n);
    guarded dev(bytes), to_caller(bytes), caller(bytes), to_dev(bytes), back(bytes);
    pattern(dev.data(), esize, n, 17u);
    pattern(caller.data(), esize, n, 40009u);
    hq_state_transpose(tb, np, true, dev.data(), to_caller.data());
    hq_state_transpose(tb, np, false, caller.data(), to_dev.data());
    hq_state_transpose(tb, np, false, to_caller.data(), back.data());
    CHECK(dev.intact() && to_caller.intact() && caller.intact() && to_dev.intact() && back.intact());
    CHECK(memcmp(back.data(), dev.data(), bytes) == 0);
    const int64_t head[4] = { (int64_t)esize, (int64_t)np, (int64_t)rows, (int64_t)slots };
    fwrite(head, sizeof head, 1, f);
    guarded* all[5] = { &dev, &to_caller, &caller, &to_dev, &back };
    for (guarded* g : all) if (bytes) fwrite(g->data(), 1, bytes, f);
    ncases++;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "wb");
    if (!f) return 2;
    static const size_t nps[4] = { 0, 1, 3, 257 }, nrows[4] = { 1, 3, 5, 24 }, esizes[2] = { 8, 4 }, nslots[3] = { 0, 1, 3 }, nqs[2] = { 1, 3 };
    for (size_t es : esizes) for (size_t np : nps) for (size_t r : nrows) one(f, es, np, r, 1);
    for (size_t s : nslots) for (size_t nq : nqs) for (size_t np : nps) one(f, 8, np, 3 * nq, s);
    if (fclose(f) != 0) return 2;
    printf("ok %ld tables\n", ncases);
    return 0;
}
"""


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """The program's record: per case the five buffers device, device -> caller, caller, caller -> device, there and back."""
    d = tmp_path_factory.mktemp("tracker_state")
    (d / "state_test.cpp").write_text(PROGRAM)
    exe, rec = d / "state_test", d / "tables.bin"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", str(exe),
                           str(d / "state_test.cpp")])
    out = subprocess.run([str(exe), str(rec)], stdout=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, out.stdout[-2000:]         # (the guard words and the round trip are checked in the program)
    assert out.stdout.split() == ["ok", str(len(CASES)), "tables"], out.stdout
    raw, at, got = rec.read_bytes(), 0, []
    while at < len(raw):
        es, n, rows, slots = (int(v) for v in np.frombuffer(raw, np.int64, 4, at))
        at += 32
        dtype, count = (np.float64 if es == 8 else np.int32), n * rows * slots
        bufs = [np.frombuffer(raw, dtype, count, at + k * es * count) for k in range(5)]
        at += 5 * es * count
        got.append(((es, n, rows, slots), bufs))
    return got


def test_the_program_ran_the_cases_of_this_file(tables):
    assert [case for case, _ in tables] == CASES


def test_device_to_caller_is_numpys_transposition(tables):
    for (es, n, rows, slots), (dev, to_caller, _, _, _) in tables:
        want = dev.reshape(slots, rows, n).transpose(0, 2, 1)               # [slots][rows][np] -> [slots][np][rows]
        assert np.array_equal(to_caller.view(np.uint8), np.ascontiguousarray(want).reshape(-1).view(np.uint8)), (es, n, rows, slots)


def test_caller_to_device_is_numpys_transposition(tables):
    for (es, n, rows, slots), (_, _, caller, to_dev, _) in tables:
        want = caller.reshape(slots, n, rows).transpose(0, 2, 1)            # [slots][np][rows] -> [slots][rows][np]
        assert np.array_equal(to_dev.view(np.uint8), np.ascontiguousarray(want).reshape(-1).view(np.uint8)), (es, n, rows, slots)


def test_there_and_back_is_the_identity(tables):
    for case, (dev, _, _, _, back) in tables:
        assert np.array_equal(dev.view(np.uint8), back.view(np.uint8)), case


def test_state_table_header_needs_no_hip_and_no_header_of_the_package():
    text = open(os.path.join(CSRC, "hq_state_table.h")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes == ["<stddef.h>", "<stdint.h>"]
