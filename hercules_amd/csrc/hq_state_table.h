/*
 * hq_state_table.h -- one table of a tracker's state and its way between the device's layout, [slots][rows][np] (consecutive
 * lanes on consecutive points), and the caller's, [slots][np][rows]; slots is 1 but for a Husid curve.  No HIP type:
 * hq_outputs.h builds the descriptions and makes the copies, tests/test_tracker_state_cpu.py compiles this header alone.
 */
#ifndef HQ_STATE_TABLE_H
#define HQ_STATE_TABLE_H

#include <stddef.h>
#include <stdint.h>

struct hq_state_table {
    void* dev;        /* the device's array */
    void* host;       /* the caller's array for a fetch or a load, or NULL */
    size_t esize;     /* 8: double, 4: int32_t */
    size_t rows;      /* per point and slot */
    size_t slots;     /* the slots that travel */
    size_t whole;     /* the bytes of the device's array, all of which a reset fills */
    int reset;        /* the byte the table is reset with */
    bool optional;    /* a fetch may leave it out */
};
enum { HQ_STATE_MAX_TABLES = 3 };
/* the tables of one tracker, in the order they are reset in: a value built per call, never kept */
struct hq_state_tables { int n; hq_state_table t[HQ_STATE_MAX_TABLES]; };

static inline size_t hq_state_table_bytes(const hq_state_table& tb, size_t np) { return tb.esize * tb.rows * tb.slots * np; }

/* one slot between [nr][np] and [np][nr], either way */
template <typename T>
static void hq_state_transpose_slot(size_t np, size_t nr, bool to_caller, const T* src, T* dst)
{
    for (size_t p = 0, ic = 0; p < np; p++)
        for (size_t r = 0; r < nr; r++, ic++)
            if (to_caller) dst[ic] = src[r * np + p]; else dst[r * np + p] = src[ic];
}

/* every slot of a table of np points from src to dst, hq_state_table_bytes() each: to the caller's layout or from it */
static inline void hq_state_transpose(const hq_state_table& tb, size_t np, bool to_caller, const void* src, void* dst)
{
    for (size_t k = 0, n = tb.rows * np; k < tb.slots; k++) {
        if (tb.esize == sizeof(double)) hq_state_transpose_slot(np, tb.rows, to_caller, (const double*)src + k * n, (double*)dst + k * n);
        else hq_state_transpose_slot(np, tb.rows, to_caller, (const int32_t*)src + k * n, (int32_t*)dst + k * n);
    }
}

#endif /* HQ_STATE_TABLE_H */
