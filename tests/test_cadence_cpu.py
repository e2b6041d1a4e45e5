"""hq_cadence.h -- which steps an output is due at, the ring of pending slots, and where the runner cuts its batches --
against the loops and expressions it replaced, restated here as the engine and the host runner had them before the
header existed, and against properties that need no old formula at all.  One C program with its own main, compiled as
C99 and as C++17; no device, no library of the package."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hercules_amd", "csrc")

PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "hq_cadence.h"

static long ncases = 0;
#define CHECK(cond, ...) do { ncases++; if (!(cond)) { printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); \
                                                       printf("\n"); exit(1); } } while (0)

/* ---- the formulas before the header (the reference side) ---- */

/* hq_snapshot_due; a recorder's test was step % rate == 0 alone */
static int old_due(int32_t rate, int32_t first_step, int64_t step) { return step >= first_step && step % rate == 0; }

/* hq_snapshot_check_room's loop (hq_record_check_room's with first_step below every step) */
static int64_t old_count(int32_t rate, int32_t first_step, int32_t step, int32_t nsteps)
{
    int64_t due = 0;
    for (int32_t s = 0; s < nsteps; s++) due += old_due(rate, first_step, (int64_t)step + s);
    return due;
}

/* hqh_recorder_open: "first due step >= step0" */
static int64_t old_first_due(int32_t rate, int32_t first_step, int32_t step)
{
    const int64_t from = step > first_step ? step : first_step;
    return (from + rate - 1) / rate * rate;
}

typedef struct { int32_t handle, cap, rate; } old_recorder;
static int32_t old_recorder_limit(const old_recorder* r, int32_t step, int32_t next)
{
    if (r->handle < 0) return next;
    const int64_t first = ((int64_t)step + r->rate - 1) / r->rate * r->rate;
    const int64_t full = first + (int64_t)r->cap * r->rate;                     /* the (cap + 1)-th due step */
    return full < next ? (int32_t)full : next;
}

typedef struct { int32_t handle, rate, first_step, slots; } old_snapshot;
static int32_t old_snapshot_limit(const old_snapshot* sn, int32_t step, int32_t next)
{
    if (sn->handle < 0) return next;
    const int64_t from = step > sn->first_step ? step : sn->first_step;
    const int64_t first = (from + sn->rate - 1) / sn->rate * sn->rate;
    const int64_t full = first + (int64_t)sn->slots * sn->rate;                 /* the (slots + 1)-th due step */
    return full < next ? (int32_t)full : next;
}

/* one run as the runner sees it; a rate of 0: the output is not asked for */
typedef struct {
    int32_t step0, end, win;                                                    /* win 0: no source */
    int32_t station_rate, plane_rate, checkpoint_rate, wavefield_rate;
    int dev_rec, async;
    int32_t cap_st, cap_pl, slots;
} plan_t;

/* hqh_recorder_open's handle: no recorder where the output is off or no step of the run is due */
static old_recorder old_open(int on, int32_t rate, int32_t cap, int32_t step0, int32_t end)
{
    old_recorder r = { -1, cap, rate };
    if (on && ((int64_t)step0 + rate - 1) / rate * rate < end) r.handle = 0;
    return r;
}

/* the runner's "int32_t next = end; ..." block, names as they were */
static int32_t old_next(const plan_t* p, int32_t step, int32_t win_end)
{
    const int F = p->win > 0, u = p->station_rate > 0, pfp = p->plane_rate > 0;
    const int do_ckpt = p->checkpoint_rate > 0, do_wave = p->wavefield_rate > 0, async = p->async;
    const int dev_rec = p->dev_rec && (u || pfp);
    const int32_t end = p->end;
    const old_recorder rst = old_open(dev_rec && u, p->station_rate, p->cap_st, p->step0, end);
    const old_recorder rpl = old_open(dev_rec && pfp, p->plane_rate, p->cap_pl, p->step0, end);
    const old_snapshot sck = { async && do_ckpt ? 0 : -1, do_ckpt ? p->checkpoint_rate : 1, do_ckpt ? p->step0 + 1 : 0, p->slots };
    const old_snapshot swv = { async && do_wave ? 0 : -1, do_wave ? p->wavefield_rate : 1, 0, p->slots };
    int32_t next = end;
    if (F && win_end < next) next = win_end;
    if (u && !dev_rec) {
        int32_t ns = (step / p->station_rate + 1) * p->station_rate;
        if (ns < next) next = ns;
    }
    if (pfp && !dev_rec) {
        int32_t ns = (step / p->plane_rate + 1) * p->plane_rate;
        if (ns < next) next = ns;
    }
    if (do_ckpt && !async) {
        int32_t ns = (step / p->checkpoint_rate + 1) * p->checkpoint_rate;
        if (ns < next) next = ns;
    }
    if (do_wave && !async) {
        int32_t ns = (step / p->wavefield_rate + 1) * p->wavefield_rate;
        if (ns < next) next = ns;
    }
    if (async) {
        next = old_snapshot_limit(&sck, step, next);
        next = old_snapshot_limit(&swv, step, next);
    }
    if (dev_rec) {
        next = old_recorder_limit(&rst, step, next);
        next = old_recorder_limit(&rpl, step, next);
    }
    return next;
}

/* ---- cadence ---- */

static void test_cadence(void)
{
    static const int32_t firsts[4] = { 0, 1, 5, 12 };
    for (int32_t rate = 1; rate <= 7; rate++)
        for (int f = 0; f < 4; f++) {
            const hq_cadence c = { rate, firsts[f] };
            for (int32_t from = 0; from <= 60; from++) {
                CHECK(hq_cadence_due(c, from) == old_due(rate, firsts[f], from), "rate %d first %d step %d", rate, firsts[f], from);
                int64_t first = from;                                           /* by walking, too */
                while (!old_due(rate, firsts[f], first)) first++;
                CHECK(hq_cadence_first_due(c, from) == first, "rate %d first %d from %d", rate, firsts[f], from);
                CHECK(hq_cadence_first_due(c, from) == old_first_due(rate, firsts[f], from), "rate %d first %d from %d", rate, firsts[f], from);
                for (int32_t n = 0; n <= 60; n++)
                    CHECK(hq_cadence_count(c, from, from + n) == old_count(rate, firsts[f], from, n),
                          "rate %d first %d [%d, %d)", rate, firsts[f], from, from + n);
                for (int32_t cap = 1; cap <= 5; cap++) {
                    const old_snapshot sn = { 0, rate, firsts[f], cap };
                    CHECK(hq_cadence_limit(c, from, cap) == old_snapshot_limit(&sn, from, INT32_MAX), "rate %d first %d from %d cap %d",
                          rate, firsts[f], from, cap);
                    int64_t s = from, seen = 0;                                 /* the (cap + 1)-th due step, by walking */
                    for (;; s++) if (old_due(rate, firsts[f], s) && ++seen == cap + 1) break;
                    CHECK(hq_cadence_limit(c, from, cap) == s, "rate %d first %d from %d cap %d", rate, firsts[f], from, cap);
                    if (firsts[f] == 0) {
                        const old_recorder r = { 0, cap, rate };
                        CHECK(hq_cadence_limit(c, from, cap) == old_recorder_limit(&r, from, INT32_MAX), "rate %d from %d cap %d", rate, from, cap);
                    }
                }
            }
            /* near the end of int32_t: the engine's step counter is one, the arithmetic must not be */
            const int32_t a = INT32_MAX - 100;
            for (int32_t n = 0; n <= 100; n++)
                CHECK(hq_cadence_count(c, a, (int64_t)a + n) == old_count(rate, firsts[f], a, n), "rate %d first %d n %d", rate, firsts[f], n);
            /* a step counter set below zero (hq_upload takes any): a recorder is due at the multiples there as well */
            const hq_cadence all = { rate, INT32_MIN };
            for (int32_t from = -20; from <= 0; from++)
                for (int32_t n = 0; n <= 30; n++)
                    CHECK(hq_cadence_count(all, from, from + n) == old_count(rate, INT32_MIN, from, n), "rate %d [%d, %d)", rate, from, from + n);
        }
}

/* ---- ring ---- */

static uint32_t rng_state = 12345u;
static uint32_t rng(void) { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static void test_ring(void)
{
    static const int32_t caps[4] = { 1, 2, 3, 8 };
    for (int ci = 0; ci < 4; ci++) {
        const int32_t cap = caps[ci];
        int32_t storage[8], q_step[8], q_slot[8], qn = 0, pushes = 0, next_step = 0;   /* the naive queue: an array, shifted on pop */
        hq_step_ring r = { storage, cap, 0, 0 };
        for (int op = 0; op < 10000; op++) {
            if (rng() % 2) {
                const int32_t slot = hq_step_ring_push(&r, next_step);
                if (qn == cap) {
                    CHECK(slot == -1, "cap %d op %d: a full ring took a push", cap, op);
                } else {
                    CHECK(slot == pushes % cap, "cap %d op %d: slot %d", cap, op, slot);   /* the p-th push goes to slot p mod cap */
                    q_step[qn] = next_step; q_slot[qn] = slot; qn++; pushes++;
                }
                next_step += 1 + (int32_t)(rng() % 5);
            } else {
                const int32_t n = qn ? (int32_t)(rng() % (uint32_t)(qn + 1)) : 0;
                hq_step_ring_pop(&r, n);
                for (int32_t k = n; k < qn; k++) { q_step[k - n] = q_step[k]; q_slot[k - n] = q_slot[k]; }
                qn -= n;
            }
            CHECK(r.count == qn && hq_step_ring_room(&r) == cap - qn, "cap %d op %d: count %d", cap, op, r.count);
            CHECK(hq_step_ring_first_step(&r) == (qn ? q_step[0] : -1), "cap %d op %d: first step", cap, op);
            for (int32_t k = 0; k < qn; k++) {
                const int32_t slot = hq_step_ring_slot_at(&r, k);
                CHECK(slot == q_slot[k] && storage[slot] == q_step[k], "cap %d op %d: entry %d", cap, op, k);
            }
        }
    }
}

/* ---- batch plan ---- */

static long nplans = 0;

/* due_before[run][checkpoint][rate][k]: the due steps in [step0, step0 + k) of the runs from step0 = 0 and 7, counted by
 * walking them once (a checkpoint is "not at step0"): what the properties below are held against */
static int32_t due_before[2][2][6][52];
static void walk_due_steps(void)
{
    for (int run = 0; run < 2; run++) for (int ck = 0; ck < 2; ck++) for (int32_t rate = 1; rate <= 5; rate++)
        for (int32_t k = 0; k <= 50; k++) {
            const int32_t s = (run ? 7 : 0) + k;
            due_before[run][ck][rate][k + 1] = due_before[run][ck][rate][k] + (s % rate == 0 && !(ck && k == 0));
        }
}

/* the runner's loop without the device: the batch ends of one run, each against old_next and against what a plan must
 * hold whatever the formula.  The new side's arguments are put together as hqh_run_open does. */
static void check_plan(const plan_t* p, int properties)
{
    const int32_t rates[4] = { p->checkpoint_rate, p->wavefield_rate, p->plane_rate, p->station_rate };   /* :4277-4280 */
    const int dev_rec = p->dev_rec && (p->station_rate > 0 || p->plane_rate > 0);
    int64_t sync_rates[4];
    hq_device_output dev[4];
    int nsync = 0, ndev = 0;
    for (int i = 0; i < 4; i++) {
        if (rates[i] <= 0) continue;
        const hq_cadence due = { rates[i], i == 0 ? (int64_t)p->step0 + 1 : p->step0 };
        const int on_device = i < 2 ? p->async : dev_rec;
        if (!on_device) sync_rates[nsync++] = rates[i];
        else if (i < 2 || hq_cadence_count(due, p->step0, p->end) > 0) {        /* no recorder where no step of the run is due */
            dev[ndev].due = due;
            dev[ndev++].room = i < 2 ? p->slots : i == 2 ? p->cap_pl : p->cap_st;
        }
    }
    int32_t step = p->step0, win_end = p->step0;
    nplans++;
    while (step < p->end) {
        if (p->win > 0 && step >= win_end) win_end = step + (p->end - step < p->win ? p->end - step : p->win);
        const int64_t next = hq_batch_end(step, p->end, p->win > 0 ? win_end : p->end, sync_rates, nsync, dev, ndev);
        CHECK(next == old_next(p, step, win_end), "step0 %d end %d win %d rates %d %d %d %d routes %d %d at %d: %lld, was %d", p->step0, p->end,
              p->win, rates[0], rates[1], rates[2], rates[3], p->dev_rec, p->async, step, (long long)next, old_next(p, step, win_end));
        if (properties) {
            CHECK(next > step && next <= p->end, "a batch of [%d, %lld) in a run to %d", step, (long long)next, p->end);
            for (int i = 0; i < 4; i++) {
                if (rates[i] <= 0) continue;
                const int on_device = i < 2 ? p->async : dev_rec;
                const int32_t* before = due_before[p->step0 != 0][i == 0][rates[i]];
                const int32_t held = before[next - p->step0] - before[step - p->step0];          /* due steps in the batch */
                const int32_t inside = before[next - p->step0] - before[step + 1 - p->step0];    /* ... behind its first step */
                if (!on_device) CHECK(inside == 0, "output %d is due inside [%d, %lld)", i, step, (long long)next);
                else CHECK(held <= (i < 2 ? p->slots : i == 2 ? p->cap_pl : p->cap_st), "output %d: %d due steps in [%d, %lld)", i, held, step, (long long)next);
            }
        }
        step = (int32_t)next;
    }
    CHECK(step == p->end, "the batches end at %d, the run at %d", step, p->end);
}

static void test_plans(void)
{
    static const int32_t step0s[2] = { 0, 7 }, wins[3] = { 0, 4, 64 }, rates[5] = { 0, 1, 2, 3, 5 };
    plan_t p;
    walk_due_steps();
    for (int a = 0; a < 2; a++) for (int32_t n = 0; n <= 50; n++) for (int w = 0; w < 3; w++)
    for (int i = 0; i < 5; i++) for (int j = 0; j < 5; j++) for (int k = 0; k < 5; k++) for (int l = 0; l < 5; l++)
    for (p.dev_rec = 0; p.dev_rec <= 1; p.dev_rec++) for (p.async = 0; p.async <= 1; p.async++)
    for (int32_t ring = 1; ring <= (p.dev_rec || p.async ? 3 : 1); ring++) {
        p.step0 = step0s[a]; p.end = p.step0 + n; p.win = wins[w];
        p.station_rate = rates[i]; p.plane_rate = rates[j]; p.checkpoint_rate = rates[k]; p.wavefield_rate = rates[l];
        p.cap_st = ring; p.cap_pl = 4 - ring; p.slots = 1 + ring % 3;           /* 1..3 each, and no two the same */
        check_plan(&p, 1);
    }
    /* below zero the synchronous route alone runs, and cuts as C's truncating division always made it */
    p.dev_rec = p.async = 0; p.cap_st = p.cap_pl = p.slots = 1; p.step0 = -3;
    for (int32_t n = 0; n <= 50; n++) for (int w = 0; w < 3; w++)
    for (int i = 0; i < 5; i++) for (int j = 0; j < 5; j++) for (int k = 0; k < 5; k++) for (int l = 0; l < 5; l++) {
        p.end = p.step0 + n; p.win = wins[w];
        p.station_rate = rates[i]; p.plane_rate = rates[j]; p.checkpoint_rate = rates[k]; p.wavefield_rate = rates[l];
        check_plan(&p, 0);
    }
}

/* ---- the merge ---- */

static void test_merge(void)
{
    for (int64_t a = -1; a <= 6; a++)
        for (int64_t b = -1; b <= 6; b++) {
            const int old = (a < 0 && b < 0) ? -1 : (a >= 0 && (b < 0 || a <= b)) ? 0 : 1;   /* "nck > 0 && (nwv == 0 || sck_step <= swv_step)" */
            CHECK(hq_merge_next(a, b) == old, "heads %lld %lld", (long long)a, (long long)b);
        }
}

int main(void)
{
    test_cadence();
    test_ring();
    test_plans();
    test_merge();
    printf("ok %ld checks %ld plans\n", ncases, nplans);
    return 0;
}
"""


@pytest.fixture(scope="module")
def source(tmp_path_factory):
    d = tmp_path_factory.mktemp("cadence")
    (d / "cadence_test.c").write_text(PROGRAM)
    return d


def _run(exe):
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, out.stdout[-2000:]
    words = out.stdout.split()
    assert words[0] == "ok" and int(words[1]) > 10 ** 6 and int(words[3]) > 10 ** 6, out.stdout


def test_cadence_header_as_c99(source):
    exe = source / "cadence_c"
    subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", str(exe),
                           str(source / "cadence_test.c")])
    _run(exe)


def test_cadence_header_as_cxx17(source):
    exe = source / "cadence_cxx"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-x", "c++", "-I", CSRC, "-o", str(exe),
                           str(source / "cadence_test.c")])
    _run(exe)


def test_cadence_header_needs_no_other_header_of_the_package():
    text = open(os.path.join(CSRC, "hq_cadence.h")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes == ["<stdint.h>"]
