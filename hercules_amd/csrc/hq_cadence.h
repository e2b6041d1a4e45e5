/*
 * hq_cadence.h -- which steps an output is due at, how many of them fit before a ring is full, and where the runner cuts
 * its batches: the one definition the engine (hq_engine.hip) and the host runner (hq_host.c) share.  Plain C99 that is
 * also C++17; no HIP, no allocation, all arithmetic in int64_t (tests/test_cadence_cpu.py holds every function against
 * the loops and expressions it replaced).
 */
#ifndef HQ_CADENCE_H
#define HQ_CADENCE_H

#include <stdint.h>

/* An output every `rate` steps from `first_step` on: the reference's `step % rate == 0` (psolve.c:4277-4280), and for a
 * checkpoint "not at the run's first step" (first_step = step0 + 1).  rate >= 1. */
typedef struct { int64_t rate, first_step; } hq_cadence;

static inline int hq_cadence_due(hq_cadence c, int64_t step) { return step >= c.first_step && step % c.rate == 0; }

/* the first due step >= from (any sign: C's % has the dividend's) */
static inline int64_t hq_cadence_first_due(hq_cadence c, int64_t from)
{
    if (from < c.first_step) from = c.first_step;
    const int64_t r = from % c.rate;
    return r == 0 ? from : r > 0 ? from + c.rate - r : from - r;
}

/* due steps in [a, b) */
static inline int64_t hq_cadence_count(hq_cadence c, int64_t a, int64_t b)
{
    const int64_t first = hq_cadence_first_due(c, a);
    return first < b ? (b - 1 - first) / c.rate + 1 : 0;
}

/* the (cap + 1)-th due step >= from: where a batch that starts at `from` with room for `cap` must end, at the latest */
static inline int64_t hq_cadence_limit(hq_cadence c, int64_t from, int64_t cap)
{
    return hq_cadence_first_due(c, from) + cap * c.rate;
}

/* The next multiple of `rate` after `step`, as the synchronous runner has always cut: the next due step for step >= 0.
 * Below zero (hqh_solver_run_on accepts step0 < 0) C's truncating division skips the negative multiples, and so do the
 * runner's batches: kept as it is. */
static inline int64_t hq_cadence_next_after(int64_t rate, int64_t step) { return (step / rate + 1) * rate; }

/* A ring of pending slots, oldest at `head`, each labelled with its step in the caller's steps[capacity]. */
typedef struct { int32_t* steps; int32_t capacity, head, count; } hq_step_ring;

static inline int32_t hq_step_ring_room(const hq_step_ring* r) { return r->capacity - r->count; }
static inline int32_t hq_step_ring_slot_at(const hq_step_ring* r, int32_t k) { return (int32_t)(((int64_t)r->head + k) % r->capacity); }
static inline int32_t hq_step_ring_first_step(const hq_step_ring* r) { return r->count > 0 ? r->steps[r->head] : -1; }

/* claim the next free slot for `step`; -1: the ring is full */
static inline int32_t hq_step_ring_push(hq_step_ring* r, int32_t step)
{
    if (r->count >= r->capacity) return -1;
    const int32_t slot = hq_step_ring_slot_at(r, r->count++);
    r->steps[slot] = step;
    return slot;
}

/* drop the n <= count oldest */
static inline void hq_step_ring_pop(hq_step_ring* r, int32_t n)
{
    r->head = hq_step_ring_slot_at(r, n);
    r->count -= n;
}

/* An output taken on the device: the batch may hold `room` of its due steps (its ring's or slot set's free capacity). */
typedef struct { hq_cadence due; int64_t room; } hq_device_output;

/* Where the batch that starts at `step` ends: at `end`, at the source window's end (win_end; `end` where there is none),
 * at the next step one of the nsync synchronous outputs prints at -- the host reads the fields there -- or where one of
 * the ndev device outputs would run out of room, whichever comes first.  step < min(end, win_end), so a batch has a step. */
static inline int64_t hq_batch_end(int64_t step, int64_t end, int64_t win_end, const int64_t* sync_rates, int nsync,
                                   const hq_device_output* dev, int ndev)
{
    int64_t next = win_end < end ? win_end : end;
    for (int i = 0; i < nsync; i++) {
        const int64_t s = hq_cadence_next_after(sync_rates[i], step);
        if (s < next) next = s;
    }
    for (int i = 0; i < ndev; i++) {
        const int64_t s = hq_cadence_limit(dev[i].due, step, dev[i].room);
        if (s < next) next = s;
    }
    return next;
}

/* Two step-ordered queues, each given by its head's step (-1: empty; steps are >= 0 on the device routes): which one
 * holds the next item -- 0 the first, also at a tie, 1 the second, -1 neither. */
static inline int hq_merge_next(int64_t first_step, int64_t second_step)
{
    if (first_step < 0 && second_step < 0) return -1;
    return first_step >= 0 && (second_step < 0 || first_step <= second_step) ? 0 : 1;
}

#endif
