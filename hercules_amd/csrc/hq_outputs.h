/*
 * hq_outputs.h -- the device-side outputs of a context (include/hq_solver.h): sample recorders, peak-motion, response-spectrum,
 * cumulative-intensity and deformation trackers, field snapshots -- their kernels, their state (the structs hq_ctx declares), the launches at
 * the head of a step and the hq_record_* / hq_peak_* / hq_spec_* / hq_cum_* / hq_deform_* / hq_snapshot_* entry points.  Included once by hq_engine.hip, behind hq_ctx and its helpers, ahead of hq_phase.
 * The tracker kinds keep state in place and share everything around it: hq_tracker (points, nsamples), hq_points_ok,
 * hq_quantities_ok, hq_spare_check, hq_tracker_open / _added / _zero / _fetch / _load and hq_trackers_launch.  A new kind
 * provides its kernel, its fold header (as hq_peak.h, hq_sdof.h, hq_cumul.h, hq_deform.h), its struct with reads_spare() and tables()
 * (hq_state_table.h), its *_zero, and the check of its description in its *_add.
 */
#ifndef HQ_OUTPUTS_H
#define HQ_OUTPUTS_H

#include "hq_state_table.h"

/*
 * One sample of a recorder (hq_record_add): interpolate_station_displacements (psolve.c:6705-6787) / Old_planes_print
 * (io_planes.c:176-200) on the device-resident state.  One lane per point, consecutive lanes on consecutive points; ids
 * and phi are stored transposed ([8][np]) so that a wave reads them in whole lines.  Eight gathers of one 3-vector from
 * each of u1 = u(t), u2 = u(t - dt), u3 = u(t - 2 dt) as far as `derivs` needs them, every value widened to double first
 * (hq_real is float in the f32 library), summed by hq_sample.h, the text hqh_station_kinematics (hq_host.c) compiles: the
 * samples must equal the host route's bit for bit (tests/test_gpu_recorders.py).
 * A memory-bound gather of up to 3 x 8 x 24 bytes per point; a plane's points are the bulk of it.
 */
__global__ void __launch_bounds__(256)
hq_k_record(int32_t np, const int32_t* __restrict__ ids, const double* __restrict__ phi,
            const hq_real* __restrict__ u1, const hq_real* __restrict__ u2, const hq_real* __restrict__ u3,
            double dt, double dt2, int32_t derivs, double* __restrict__ out)
{
#pragma clang fp contract(off)
    const int32_t p = (int32_t)(blockIdx.x * 256u + threadIdx.x);
    if (p >= np) return;
    int64_t row[8];
    double w[8];
#pragma unroll
    for (int c = 0; c < 8; c++) {
        row[c] = 3 * (int64_t)ids[(int64_t)c * np + p];
        w[c] = phi[(int64_t)c * np + p];
    }
    double* o = out + (int64_t)p * (3 * (1 + derivs));
    double d[3] = { 0.0, 0.0, 0.0 };
    hq_sample_disp(8, w, row, u1, d);
    for (int a = 0; a < 3; a++) o[a] = d[a];
    if (derivs >= 1) {
        hq_sample_vel(8, w, row, u2, d);
        for (int a = 0; a < 3; a++) o[3 + a] = d[a] / dt;
    }
    if (derivs == 2) {
        hq_sample_acc(8, w, row, u2, u3, d);
        for (int a = 0; a < 3; a++) o[6 + a] = d[a] / dt2;
    }
}

/*
 * One due step of a peak-motion tracker (hq_peak_add): the sample hq_k_record would take at the point -- hq_sample.h's
 * stages, the text the recorder compiles, so that it IS the recorder's sample bit for bit -- folded into the point's
 * running state in place (hq_peak.h) instead of being appended to a ring.
 * One lane per point, no atomics: a point belongs to one lane, and the launches of one stream are ordered.
 *   K = 8: eight nodes and trilinear weights per point (stations, planes), ids and phi transposed to [8][np] as the
 *          recorder's are.
 *   K = 1: the point is a node (surface maps): no weight table -- weight 1, exactly the recorder's sums with weights
 *          (1, 0, ..., 0) (hq_sample.h tells why) -- and one gather per field.
 * The state is [nq][5][np] doubles and [nq][2][np] int32, nq the set bits of `quantities` in the order displacement,
 * velocity, acceleration: a wave reads each of its rows in whole lines, and a lane writes only what it raised -- once a
 * point's peak has passed, the step costs it reads alone.  u2 / u3 are read only if the mask needs them.
 * Bytes per point and step, K = 1, velocity only: 4 (id) + 48 (u1, u2; 24 in the f32 library) + 40 of peaks read (`when`
 * is only ever written); K = 8, all three quantities: 96 of tables + 576 of gathers + 120 of state.
 */
template <int K>
__global__ void __launch_bounds__(256)
hq_k_peak(int32_t np, const int32_t* __restrict__ ids, const double* __restrict__ phi,
          const hq_real* __restrict__ u1, const hq_real* __restrict__ u2, const hq_real* __restrict__ u3,
          double dt, double dt2, int32_t quantities, int32_t step, double* __restrict__ pk, int32_t* __restrict__ when)
{
#pragma clang fp contract(off)
    const int32_t p = (int32_t)(blockIdx.x * 256u + threadIdx.x);
    if (p >= np) return;
    const bool vel = (quantities & HQ_PEAK_VEL) != 0, acc = (quantities & HQ_PEAK_ACC) != 0;
    int64_t row[K];
    double wk[K];
#pragma unroll
    for (int c = 0; c < K; c++) {
        row[c] = 3 * (int64_t)ids[(int64_t)c * np + p];
        if (K > 1) wk[c] = phi[(int64_t)c * np + p];
    }
    const double* w = K > 1 ? wk : nullptr;                      /* (a node: weight 1, hq_sample.h) */
    double* s = pk + p;
    int32_t* sw = when + p;
    double d[3] = { 0.0, 0.0, 0.0 };
    hq_sample_disp(K, w, row, u1, d);
    if (quantities & HQ_PEAK_DISP) {
        hq_peak_fold(d[0], d[1], d[2], step, s, np, sw, np);
        s += (int64_t)HQ_PEAK_NVAL * np; sw += (int64_t)HQ_PEAK_NWHEN * np;
    }
    if (vel || acc) {
        hq_sample_vel(K, w, row, u2, d);
        if (vel) {
            hq_peak_fold(d[0] / dt, d[1] / dt, d[2] / dt, step, s, np, sw, np);
            s += (int64_t)HQ_PEAK_NVAL * np; sw += (int64_t)HQ_PEAK_NWHEN * np;
        }
    }
    if (acc) {
        hq_sample_acc(K, w, row, u2, u3, d);
        hq_peak_fold(d[0] / dt2, d[1] / dt2, d[2] / dt2, step, s, np, sw, np);
    }
}

/* a cumulative tracker's thresholds, squared, by quantity BIT (displacement, velocity, acceleration): a kernel argument, read
 * with constant indices */
struct hq_cum_thr2 { double v[3]; };

/*
 * One due step of a cumulative-intensity tracker (hq_cum_add): the sample hq_k_record would take at the point -- formed
 * exactly as hq_k_peak forms it: hq_sample.h's stages, every value widened to double first, / dt and / dt2 divisions --
 * added into the point's running sums (hq_cumul.h, the text hqh_cum_fold compiles) instead of being appended to a ring.
 * One lane per point, no atomics, no LDS: a point belongs to one lane, and the launches of one stream are ordered.
 * K as in hq_k_peak: 8 nodes and weights per point, or the point is a node.
 * The state is [nq][6][np] doubles and [nq][3][np] int32, nq the set bits of `quantities` in the order displacement,
 * velocity, acceleration: consecutive lanes on consecutive addresses, so a wave reads and writes each row in whole lines.
 * A quantity's six sums are loaded into registers ahead of the arithmetic, folded there (stride 1) and stored back; the
 * span is folded in place and touched only where the threshold was passed.  u2 / u3 are read only if the mask needs them.
 * slot >= 0: a Husid step -- the lane copies the three sums of squares of every quantity, as just folded, to
 * curve[slot][nq][3][np]; the host accounts which due sample fills which slot (hq_cum_launch) and never hands out a slot
 * past the curve's end.  slot = -1 stores nothing.
 * Bytes per point and due step, K = 1, acceleration only (a model, not a measurement): 4 (id) + 72 of gathers (u1, u2,
 * u3; 36 in the f32 library) + 48 of sums read + 48 written = 172, plus 24 on a Husid step; the span adds 4 read and 8-12
 * written on the samples over the threshold only.  K = 8, all three quantities: 96 of tables + 576 of gathers + 288 of sums.
 */
template <int K>
__global__ void __launch_bounds__(256)
hq_k_cum(int32_t np, const int32_t* __restrict__ ids, const double* __restrict__ phi,
         const hq_real* __restrict__ u1, const hq_real* __restrict__ u2, const hq_real* __restrict__ u3,
         double dt, double dt2, int32_t quantities, int32_t step, hq_cum_thr2 thr2, double* __restrict__ sum,
         int32_t* __restrict__ span, double* __restrict__ curve, int32_t slot)
{
#pragma clang fp contract(off)
    const int32_t p = (int32_t)(blockIdx.x * 256u + threadIdx.x);
    if (p >= np) return;
    const bool vel = (quantities & HQ_PEAK_VEL) != 0, acc = (quantities & HQ_PEAK_ACC) != 0;
    int64_t row[K];
    double wk[K];
#pragma unroll
    for (int c = 0; c < K; c++) {
        row[c] = 3 * (int64_t)ids[(int64_t)c * np + p];
        if (K > 1) wk[c] = phi[(int64_t)c * np + p];
    }
    const double* w = K > 1 ? wk : nullptr;                      /* (a node: weight 1, hq_sample.h) */
    double* s = sum + p;
    int32_t* sw = span + p;
    double* cv = slot >= 0 ? curve + (int64_t)slot * HQ_CUM_NCURVE * hq_peak_nq(quantities) * np + p : nullptr;
    /* one quantity: its sums through registers, the span in place, the Husid rows behind the fold */
    auto fold = [&](double x, double y, double z, double t2) {
        double r[HQ_CUM_NSUM];
#pragma unroll
        for (int j = 0; j < HQ_CUM_NSUM; j++) r[j] = s[(int64_t)j * np];
        hq_cum_fold(x, y, z, step, t2, r, 1, sw, np);
#pragma unroll
        for (int j = 0; j < HQ_CUM_NSUM; j++) s[(int64_t)j * np] = r[j];
        if (cv) {
#pragma unroll
            for (int j = 0; j < HQ_CUM_NCURVE; j++) cv[(int64_t)j * np] = r[HQ_CUM_NSUM - HQ_CUM_NCURVE + j];
            cv += (int64_t)HQ_CUM_NCURVE * np;
        }
        s += (int64_t)HQ_CUM_NSUM * np; sw += (int64_t)HQ_CUM_NSPAN * np;
    };
    double d[3] = { 0.0, 0.0, 0.0 };
    hq_sample_disp(K, w, row, u1, d);
    if (quantities & HQ_PEAK_DISP) fold(d[0], d[1], d[2], thr2.v[0]);
    if (vel || acc) {
        hq_sample_vel(K, w, row, u2, d);
        if (vel) fold(d[0] / dt, d[1] / dt, d[2] / dt, thr2.v[1]);
    }
    if (acc) {
        hq_sample_acc(K, w, row, u2, u3, d);
        fold(d[0] / dt2, d[1] / dt2, d[2] / dt2, thr2.v[2]);
    }
}

/*
 * One due step of a deformation tracker (hq_deform_add): the displacement gradient G[b][a] = sum_c g[b][c] u_a[c] over the
 * eight nodes of the point's element -- row b is hq_sample_disp with w = g[b], the sample hq_k_record takes with phi = g[b],
 * every value widened to double first -- and, with a rate bit, the rate gradient: the same accumulators on through
 * hq_sample_vel on u2, / dt, that recorder's velocity column.  Strain, stress and rotation of them are folded into the
 * point's running state in place (hq_deform.h, the text hqh_deform_fold compiles).
 * One lane per point, no atomics, no LDS: a point belongs to one lane, and the launches of one stream are ordered.
 * ids [8][np], the weights [3][8][np], the moduli [2][np] (lambda, mu; read only with HQ_DEFORM_STRESS) and the state
 * [rows][np] doubles / int32 (rows = hq_deform_nvals / _nwhen of the mask, the blocks in the order of its bits) are
 * transposed: consecutive lanes on consecutive addresses, so a wave reads every row in whole lines.
 * Each of the eight node rows is gathered ONCE per field into registers (`ub`, in hq_real, read by hq_sample.h through the
 * constant offsets `at`: every index is a constant once the loops are unrolled) and feeds all three axis sums from there --
 * 8 gathers of 24 (12) bytes per field, not 24.  u2 is gathered into the same registers behind u1's sums, and only if a
 * rate bit is set.  The state is walked as hq_k_peak walks it: a lane reads the rows and writes only what it raised.
 * Registers: 24 weights, 24 gathered values and up to 18 sums are live at once, of the 512 VGPRs a lane of a 256-thread
 * workgroup may have; compiled for gfx950 (-O3, kernel-resource-usage) the kernel takes 130 VGPRs in the f64 library (3
 * waves per SIMD) and 124 in the f32 library (4), no AGPRs, nothing spilled, 0 bytes of scratch.
 * Bytes per point and due step, full mask, f64 (a model, not a measurement): 32 of ids + 192 of weights + 16 of moduli +
 * 384 of gathers (u1, u2; 192 in the f32 library) + 320 of state read (`when` is only ever written) = 944, plus 8 or 12
 * per value raised.  HQ_DEFORM_STRAIN alone: 32 + 192 + 192 + 80 = 496.
 */
__global__ void __launch_bounds__(256)
hq_k_deform(int32_t np, const int32_t* __restrict__ ids, const double* __restrict__ grad, const double* __restrict__ lame,
            const hq_real* __restrict__ u1, const hq_real* __restrict__ u2, double dt, int32_t quantities, int32_t step,
            double* __restrict__ vals, int32_t* __restrict__ when)
{
#pragma clang fp contract(off)
    const int32_t p = (int32_t)(blockIdx.x * 256u + threadIdx.x);
    if (p >= np) return;
    const bool rate = (quantities & (HQ_DEFORM_STRAIN_RATE | HQ_DEFORM_ROTATION_RATE)) != 0;
    const int64_t at[8] = { 0, 3, 6, 9, 12, 15, 18, 21 };        /* a point's nodes in `ub`, a contiguous [8][3] block */
    int64_t row[8];
    double g[3][8];
#pragma unroll
    for (int c = 0; c < 8; c++) row[c] = 3 * (int64_t)ids[(int64_t)c * np + p];
#pragma unroll
    for (int b = 0; b < 3; b++)
#pragma unroll
        for (int c = 0; c < 8; c++) g[b][c] = grad[(int64_t)(8 * b + c) * np + p];
    hq_real ub[24];
    auto gather = [&](const hq_real* __restrict__ u) {
#pragma unroll
        for (int c = 0; c < 8; c++)
#pragma unroll
            for (int a = 0; a < 3; a++) ub[3 * c + a] = u[row[c] + a];
    };
    double G[9] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 }, R[9];
    gather(u1);
#pragma unroll
    for (int b = 0; b < 3; b++) hq_sample_disp(8, g[b], at, ub, G + 3 * b);
    if (rate) {
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = G[i];
        gather(u2);
#pragma unroll
        for (int b = 0; b < 3; b++) hq_sample_vel(8, g[b], at, ub, R + 3 * b);
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = R[i] / dt;
    }
    double lambda = 0.0, mu = 0.0;
    if (quantities & HQ_DEFORM_STRESS) { lambda = lame[p]; mu = lame[(int64_t)np + p]; }
    hq_deform_point(quantities, G, R, lambda, mu, step, vals + p, np, when + p, np);
}

/*
 * One due step of a response-spectrum tracker (hq_spec_add): the acceleration sample hq_k_record takes at the point with
 * derivs = 2 -- hq_sample.h's three stages on u1, u2, u3, every value widened to double first, d / dt2: the recorder's
 * acceleration column bit for bit -- drives, per period, the three oscillators of hq_sdof.h one exact step from the
 * point's previous sample `aprev`, and their |x| is folded into the running maxima (hq_spec_fold, the text hqh_spec_fold
 * compiles).  One lane per point, no atomics, no LDS: a point belongs to one lane, the launches of one stream are ordered.
 * K as in hq_k_peak: 8 nodes and weights per point, or the point is a node.
 * State, all double in both libraries, consecutive lanes on consecutive addresses so that a wave reads whole lines:
 *   aprev [3][np]            the sample of the last due step (0 before the first)
 *   osc   [nper][2][3][np]   x then v
 *   sd    [nper][4][np]      max |x_x|, |x_y|, |x_z|, max (x_x^2 + x_y^2)
 * coef [nper][8] is read with a wave-uniform index: scalar loads, no VGPRs.  The periods are independent chains: period
 * j + 1's ten state values are loaded into registers BEFORE period j's are computed on and stored (the loop is unrolled by
 * two, so the two register sets swap roles without copies), which keeps a period's loads in flight behind the arithmetic
 * of the one before; the fold runs on the register copy (stride 1) and a lane stores x and v always, sd only where raised.
 * The prefetch is unconditional -- behind the last period it re-reads that period's own rows, out of L2 -- because a
 * conditional one ends in register copies that wait for the loads just issued; a scheduling barrier keeps it where it is.
 * Bytes per point and due step, K = 1, f64 (a model, not a measurement): 4 of id + 72 of state gathers (36 in the f32
 * library) + 24 read and 24 written of aprev; per period 80 read (x, v, sd) and 48 written, plus the raised sd.  8 periods:
 * 124 + 8 x 128 = 1148.
 */
template <int K>
__global__ void __launch_bounds__(256)
hq_k_spec(int32_t np, const int32_t* __restrict__ ids, const double* __restrict__ phi,
          const hq_real* __restrict__ u1, const hq_real* __restrict__ u2, const hq_real* __restrict__ u3,
          double dt2, int32_t nper, const double* __restrict__ coef, double* __restrict__ aprev, double* __restrict__ osc,
          double* __restrict__ sd)
{
#pragma clang fp contract(off)
    const int32_t p = (int32_t)(blockIdx.x * 256u + threadIdx.x);
    if (p >= np) return;
    int64_t row[K];
    double wk[K];
#pragma unroll
    for (int c = 0; c < K; c++) {
        row[c] = 3 * (int64_t)ids[(int64_t)c * np + p];
        if (K > 1) wk[c] = phi[(int64_t)c * np + p];
    }
    const double* w = K > 1 ? wk : nullptr;                      /* (a node: weight 1, hq_sample.h) */
    double a0[3], a1[3];
#pragma unroll
    for (int a = 0; a < 3; a++) a0[a] = aprev[(int64_t)a * np + p];
    double oa[HQ_SPEC_NOSC], sa[HQ_SPEC_NSD], ob[HQ_SPEC_NOSC], sb[HQ_SPEC_NSD];   /* two periods' state in registers */
    const int64_t ostep = (int64_t)HQ_SPEC_NOSC * np, sstep = (int64_t)HQ_SPEC_NSD * np;
    auto load = [np](const double* po, const double* ps, double* o, double* s) {
#pragma unroll
        for (int r = 0; r < HQ_SPEC_NOSC; r++) o[r] = po[(int64_t)r * np];
#pragma unroll
        for (int r = 0; r < HQ_SPEC_NSD; r++) s[r] = ps[(int64_t)r * np];
    };
    double* po = osc + p;
    double* ps = sd + p;
    load(po, ps, oa, sa);
    double d[3] = { 0.0, 0.0, 0.0 };
    hq_sample_disp(K, w, row, u1, d);
    hq_sample_vel(K, w, row, u2, d);
    hq_sample_acc(K, w, row, u2, u3, d);
#pragma unroll
    for (int a = 0; a < 3; a++) a1[a] = d[a] / dt2;
    /* period j on the registers (o, s), the next period's loads into (on, sn) ahead of its arithmetic */
    auto period = [&](int32_t j, double* o, double* s, double* on, double* sn) {
        const bool more = j + 1 < nper;                          /* (the last period re-reads its own rows: no branch) */
        load(po + (more ? ostep : 0), ps + (more ? sstep : 0), on, sn);
        __builtin_amdgcn_sched_barrier(0);                       /* (the loads stay ahead of this period's arithmetic) */
        double was[HQ_SPEC_NSD];
#pragma unroll
        for (int r = 0; r < HQ_SPEC_NSD; r++) was[r] = s[r];
        hq_spec_fold(coef + (int64_t)HQ_SDOF_NCOEF * j, a0, a1, o, 1, s, 1);
#pragma unroll
        for (int r = 0; r < HQ_SPEC_NOSC; r++) po[(int64_t)r * np] = o[r];
#pragma unroll
        for (int r = 0; r < HQ_SPEC_NSD; r++)
            if (s[r] != was[r]) ps[(int64_t)r * np] = s[r];
        po += ostep; ps += sstep;
    };
    for (int32_t j = 0; j < nper; j += 2) {                      /* unrolled by two: the register sets swap roles */
        period(j, oa, sa, ob, sb);
        if (j + 1 < nper) period(j + 1, ob, sb, oa, sa);
    }
#pragma unroll
    for (int a = 0; a < 3; a++) aprev[(int64_t)a * np + p] = a1[a];
}

/*
 * One field snapshot (hq_snapshot_add): the rows [first, first + count) of u1 = u(t), u2 = u(t - dt) out of the device's
 * numbering into a staging slot in the caller's (octor) order -- hq_field_to_host's un-permutation, done at HBM speed
 * ahead of the copy instead of on the host behind it.  A streaming permutation: per node 4 bytes of map, 24-48 bytes of
 * state read, 24-72 written; no arithmetic but the velocity's, (double)u1 - (double)u2 over dt, contraction off
 * (hqh_wavefield_write's write_velocity, bit for bit).
 * The OUTPUT is what the lanes are laid over: the slot's fields are flat arrays of 3 count scalars, and a lane owns V =
 * 16 / sizeof(T) consecutive ones (2 doubles, 4 floats -- they may straddle two rows), so every store is a 16-byte store
 * and a wave's stores cover 1 KiB of consecutive output rows.  The reads are gathers of single scalars, lane by lane: the
 * three lanes (or one and a half) of a row read its 24 (12) bytes side by side, and wherever the map runs on -- inside a
 * brick's tile the x-neighbours of the octor order are neighbours on the device too, 64 at a time, and on contexts without
 * a renumbering everywhere -- consecutive lanes read consecutive addresses and the wave's loads merge into whole lines
 * like those of a plain copy.  Where the map jumps, the other rows of the lines it touches are read by the same workgroup
 * (a tile of 256 V consecutive octor rows is a compact cube of the mesh) and come out of L2.
 * A workgroup takes tiles of 256 V rows = 768 lane groups, three per thread (independent: their loads are in flight
 * together); 256 V rows are a multiple of 16 bytes in every field, so each group's stores are aligned.  map == NULL: the
 * device numbers the nodes as the caller does.  o1 / o2 / ov == NULL: that field is not wanted.
 */
template <typename T>
__global__ void __launch_bounds__(256)
hq_k_snapshot(int32_t first, int32_t count, const int32_t* __restrict__ map, const T* __restrict__ u1,
              const T* __restrict__ u2, double dt, T* __restrict__ o1, T* __restrict__ o2, double* __restrict__ ov)
{
#pragma clang fp contract(off)
    constexpr int V = 16 / (int)sizeof(T);
    constexpr int32_t TR = 256 * V;                              /* rows per tile */
    typedef T vecT __attribute__((ext_vector_type(V)));         /* 16 bytes: one global_store_dwordx4 */
    typedef double vecD __attribute__((ext_vector_type(2)));
    const int32_t ntiles = (count + TR - 1) / TR;
    const bool want1 = o1 != nullptr || ov != nullptr, want2 = o2 != nullptr || ov != nullptr;
    for (int32_t tile = (int32_t)blockIdx.x; tile < ntiles; tile += (int32_t)gridDim.x) {
        const int32_t row0 = tile * TR;
        const int32_t nscal = 3 * min(TR, count - row0);         /* scalars of this tile */
        const int64_t base = 3 * (int64_t)row0;
#pragma unroll
        for (int m = 0; m < 3; m++) {
            const int32_t j0 = ((int32_t)threadIdx.x + 256 * m) * V;
            if (j0 >= nscal) continue;
            T a[V], b[V];
#pragma unroll
            for (int k = 0; k < V; k++) {
                const int32_t j = min(j0 + k, nscal - 1);        /* (a lane group past the end re-reads the last scalar) */
                const int32_t n = j / 3;
                const int64_t row = map ? (int64_t)map[row0 + n] : (int64_t)first + row0 + n;
                const int64_t src = 3 * row + (j - 3 * n);
                a[k] = want1 ? u1[src] : (T)0;
                b[k] = want2 ? u2[src] : (T)0;
            }
            const bool whole = j0 + V <= nscal;
            if (o1) {
                if (whole) {
                    vecT w;
#pragma unroll
                    for (int k = 0; k < V; k++) w[k] = a[k];
                    *(vecT*)(o1 + base + j0) = w;
                }
                else {
#pragma unroll
                    for (int k = 0; k < V; k++) if (j0 + k < nscal) o1[base + j0 + k] = a[k];
                }
            }
            if (o2) {
                if (whole) {
                    vecT w;
#pragma unroll
                    for (int k = 0; k < V; k++) w[k] = b[k];
                    *(vecT*)(o2 + base + j0) = w;
                }
                else {
#pragma unroll
                    for (int k = 0; k < V; k++) if (j0 + k < nscal) o2[base + j0 + k] = b[k];
                }
            }
            if (ov) {
                double v[V];
#pragma unroll
                for (int k = 0; k < V; k++) v[k] = ((double)a[k] - (double)b[k]) / dt;
                if (whole) {
#pragma unroll
                    for (int k = 0; k < V; k += 2) { vecD w = { v[k], v[k + 1] }; *(vecD*)(ov + base + j0 + k) = w; }
                } else {
#pragma unroll
                    for (int k = 0; k < V; k++) if (j0 + k < nscal) ov[base + j0 + k] = v[k];
                }
            }
        }
    }
}

/* ---- the outputs' state: the structs hq_ctx declares ---- */

/* what the outputs share (hq_cadence.h): the steps one is due at and the ring of its pending slots, accounted on the
 * host -- which steps are due follows from `step` alone.  (A tracker keeps no ring: capacity 0, never asked for room.) */
struct hq_ctx::hq_output {
    int32_t id = 0;
    hq_cadence due = { 1, 0 };
    hq_step_ring ring = { nullptr, 0, 0, 0 };
    std::vector<int32_t> steps;   /* [capacity] the ring's storage: a move keeps the buffer, and so ring.steps */
    void open(int32_t rate, int64_t first_step, int32_t capacity)
    {
        due = { rate, first_step };
        steps.assign((size_t)capacity, 0);
        ring = { steps.data(), capacity, 0, 0 };
    }
};
/* the points of a recorder or a tracker (hq_points_build): K nodes each, ids and weights transposed so that a wave reads
 * them in whole lines */
struct hq_point_set {
    int32_t np = 0, K = 8;
    hq_dbuf<int32_t> d_ids;       /* [K][np] device numbering */
    hq_dbuf<double> d_phi;        /* [8][np]; NULL for K = 1 */
    int64_t h2d() const { return (K == 8 ? 12 : 4) * (int64_t)K * np; }   /* bytes the upload carried: 4 per id, 8 per weight */
};
/* sample recorders (hq_record_add): rings in device memory */
struct hq_ctx::hq_recorder : hq_ctx::hq_output {
    hq_point_set pts;
    int32_t derivs = 0;
    hq_dbuf<double> d_ring;       /* [capacity][np][3 (1 + derivs)] */
};
/* what the trackers share: a running state per point updated in place by the kind's kernel -- no ring, no pending samples,
 * nothing for hq_run to count.  Each kind says what it is called, whether its launch reads d_u[spare] as u(t - 2 dt)
 * (hq_outputs_enqueue) and which tables its state is, in the order they are reset in (hq_state_table.h) */
struct hq_ctx::hq_tracker : hq_ctx::hq_output {
    hq_point_set pts;
    int64_t nsamples = 0;         /* due steps folded or enqueued so far: accounted here, from `step` alone */
};
template <typename T>
static hq_state_table hq_table(const hq_dbuf<T>& b, const T* host, size_t rows, int reset, bool optional = false, size_t slots = 1)
{
    return { b.get(), const_cast<T*>(host), sizeof(T), rows, slots, b.bytes(), reset, optional };
}
/* peak-motion trackers (hq_peak_add), updated in place by hq_k_peak */
struct hq_ctx::hq_peak_tracker : hq_ctx::hq_tracker {
    static constexpr const char* kind = "peak";
    int32_t quantities = 0, nq = 0;
    hq_dbuf<double> d_pk;         /* [nq][5][np]; 0 before the first sample */
    hq_dbuf<int32_t> d_when;      /* [nq][2][np]; -1 (every byte 0xff) */
    bool reads_spare() const { return (quantities & HQ_PEAK_ACC) != 0; }
    hq_state_tables tables(const double* peaks = nullptr, const int32_t* when = nullptr) const   /* (the caller's arrays, if any) */
    { return { 2, { hq_table(d_pk, peaks, (size_t)nq * HQ_PEAK_NVAL, 0), hq_table(d_when, when, (size_t)nq * HQ_PEAK_NWHEN, 0xff), {} } }; }
};
/* response-spectrum trackers (hq_spec_add): per point the last sample and, per period, three oscillators and their maxima,
 * updated in place by hq_k_spec */
struct hq_ctx::hq_spec_tracker : hq_ctx::hq_tracker {
    static constexpr const char* kind = "spectrum";
    int32_t nper = 0;
    std::vector<double> coef;     /* [nper][8], hq_sdof_coef at h = rate dt: what d_coef holds */
    hq_dbuf<double> d_coef;
    hq_dbuf<double> d_aprev;      /* [3][np]; at rest before the first sample: all 0 */
    hq_dbuf<double> d_osc;        /* [nper][2][3][np] */
    hq_dbuf<double> d_sd;         /* [nper][4][np] */
    bool reads_spare() const { return true; }   /* (tables(): the rows of a point counted across the periods) */
    hq_state_tables tables(const double* sd = nullptr, const double* osc = nullptr, const double* aprev = nullptr) const
    {
        return { 3, { hq_table(d_aprev, aprev, 3, 0, true), hq_table(d_osc, osc, (size_t)nper * HQ_SPEC_NOSC, 0, true),
                      hq_table(d_sd, sd, (size_t)nper * HQ_SPEC_NSD, 0) } };
    }
};
/* cumulative-intensity trackers (hq_cum_add): running sums and threshold spans per point, updated in place by hq_k_cum, and
 * the Husid curve -- the sums of squares as they stood after every husid_every-th due sample, husid_slots of them: which
 * sample fills which slot follows from nsamples alone */
struct hq_ctx::hq_cum_tracker : hq_ctx::hq_tracker {
    static constexpr const char* kind = "cumulative";
    int32_t quantities = 0, nq = 0, husid_every = 0, husid_slots = 0;
    hq_cum_thr2 thr2 = { { 0.0, 0.0, 0.0 } };   /* by quantity bit */
    std::vector<int32_t> curve_steps;           /* [nfilled] the step of the sample each filled slot was stored behind */
    hq_dbuf<double> d_sum;        /* [nq][6][np]; 0 before the first sample */
    hq_dbuf<int32_t> d_span;      /* [nq][3][np]; -1, and the count row 0 (hq_cum_zero) */
    hq_dbuf<double> d_curve;      /* [husid_slots][nq][3][np]; 0; `slots` of them travel (tables()): the filled ones */
    bool reads_spare() const { return (quantities & HQ_PEAK_ACC) != 0; }
    hq_state_tables tables(const double* sums = nullptr, const int32_t* span = nullptr, const double* curve = nullptr, size_t slots = 0) const
    {
        return { 3, { hq_table(d_sum, sums, (size_t)nq * HQ_CUM_NSUM, 0), hq_table(d_curve, curve, (size_t)nq * HQ_CUM_NCURVE, 0, true, slots),
                      hq_table(d_span, span, (size_t)nq * HQ_CUM_NSPAN, 0xff) } };
    }
};
/* deformation trackers (hq_deform_add): the running peaks of strain, strain rate, stress, rotation and rotation rate per
 * point, updated in place by hq_k_deform.  The points are elements with gradient weights in place of phi (pts.d_phi stays
 * empty).  Only u1 and u2 are read: no stream is ever held back, and every variant has them */
struct hq_ctx::hq_deform_tracker : hq_ctx::hq_tracker {
    static constexpr const char* kind = "deformation";
    int32_t quantities = 0;
    hq_dbuf<double> d_grad;       /* [3][8][np] */
    hq_dbuf<double> d_lame;       /* [2][np] lambda, mu; NULL without HQ_DEFORM_STRESS */
    hq_dbuf<double> d_vals;       /* [10 nt + 5 nv][np]; 0 before the first sample */
    hq_dbuf<int32_t> d_when;      /* [2 (nt + nv)][np]; -1 (every byte 0xff) */
    bool reads_spare() const { return false; }
    hq_state_tables tables(const double* vals = nullptr, const int32_t* when = nullptr) const
    {
        return { 2, { hq_table(d_vals, vals, (size_t)hq_deform_nvals(quantities), 0),
                      hq_table(d_when, when, (size_t)hq_deform_nwhen(quantities), 0xff), {} } };
    }
};
/* field snapshots (hq_snapshot_add): per snapshot a ring of `slots` staging slots in device memory and their mirrors in
 * pinned host memory.  A slot holds the fields one behind the other,
 * each at a 256-byte boundary (off[]; the same layout on both sides, so one copy carries a slot).  sstream, the copy
 * stream, exists from the first hq_snapshot_add on: behind each hq_k_snapshot launch ev_output is
 * recorded on the compute stream and waited for by sstream, which copies the slot and records the slot's done event */
struct hq_ctx::hq_snapshot : hq_ctx::hq_output {
    int32_t first = 0, count = 0, fields = 0;
    hq_dbuf<int32_t> d_map;       /* [count] device id of node first + i; NULL on contexts without a renumbering */
    hq_dbuf<char> d_stage;        /* [slots][slot_bytes] */
    char* h_stage = nullptr;      /* the same, pinned host memory */
    size_t off[3] = { 0, 0, 0 };  /* tm1, tm2, vel inside a slot */
    size_t slot_bytes = 0;
    std::vector<hipEvent_t> done; /* [slots] the slot's copy has arrived */
};

/* ---- device outputs: what the three kinds share (hq_cadence.h) ---- */

/* do the due steps of [c->step, c->step + nsteps) fit into every ring's free slots? */
template <typename T>
static bool hq_outputs_have_room(const std::vector<T>& outs, int64_t step, int32_t nsteps)
{
    for (const auto& o : outs)
        if (hq_cadence_count(o.due, step, step + nsteps) > hq_step_ring_room(&o.ring)) return false;
    return true;
}

/* the recorders' rings and the snapshots' slots: what hq_run, hq_group_run and hq_run_timed ask before they enqueue */
static int hq_output_check_room(const hq_ctx* c, int32_t nsteps)
{
    if (!hq_outputs_have_room(c->recs, c->step, nsteps))
        return hq_fail(HQ_ERR_STATE, "a recorder's ring would overflow: fetch its samples first (hq_record_fetch)%s", "");
    if (!hq_outputs_have_room(c->snaps, c->step, nsteps))
        return hq_fail(HQ_ERR_STATE, "a snapshot's slots would run out: fetch the pending ones first (hq_snapshot_fetch)%s", "");
    return HQ_OK;
}

template <typename T>
static T* hq_output_find(std::vector<T>& outs, int32_t handle)
{
    for (auto& o : outs)
        if (o.id == handle) return &o;
    return nullptr;
}

/* the tables of np points from the caller's [np][K] ids and [np][8] weights (K = 8 only): every id checked, device numbering,
 * transposed to [K][np], uploaded ON the compute stream and waited for (hq_devmem.h).  h2d() the caller counts. */
static int hq_points_build(hq_ctx* c, int32_t np, int32_t K, const int32_t* ids_in, const double* phi_in, hq_point_set* ps)
{
    for (int64_t i = 0; i < (int64_t)K * np; i++)
        if (ids_in[i] < 0 || ids_in[i] >= c->N) return hq_fail(HQ_ERR_ARG, "node id out of range%s", "");
    std::vector<int32_t> ids((size_t)np * K);
    std::vector<double> phi(K == 8 ? (size_t)np * 8 : 0);
    for (int32_t p = 0; p < np; p++)
        for (int k = 0; k < K; k++) {
            const int32_t id = ids_in[(size_t)K * p + k];
            ids[(size_t)k * np + p] = c->perm.empty() ? id : c->perm[(size_t)id];
            if (K == 8) phi[(size_t)k * np + p] = phi_in[8 * (size_t)p + k];
        }
    ps->np = np; ps->K = K;
    HQ_TRY(ps->d_ids.put(&c->bytes, ids, c->stream));
    if (K == 8) HQ_TRY(ps->d_phi.put(&c->bytes, phi, c->stream));
    return HQ_OK;
}

/* head of a step: one hq_k_record launch per due recorder on the compute stream, behind the waits phase 0 has already
 * made for the last step's shared displacements and bricks.  On a due step only, the streams whose kernels of THIS
 * step write into d_u[spare] -- which the launch reads as u(t - 2 dt) -- are held back behind it: the bricks' own stream,
 * and the exchange chain's (hq_k_interface_update, the unpack).  The patches follow on the compute stream itself. */
static int hq_record_launch(hq_ctx* c, hq_ctx::hq_recorder& r)
{
    const int32_t slot = hq_step_ring_push(&r.ring, c->step);
    if (slot < 0) return hq_fail(HQ_ERR_STATE, "a recorder's ring is full%s", "");   /* (hq_output_check_room saw to it) */
    if (r.pts.np <= 0) return HQ_OK;
    const int32_t ncomp = 3 * (1 + r.derivs);
    hq_k_record<<<hq_blocks(r.pts.np, 256), 256, 0, c->stream>>>(
        r.pts.np, r.pts.d_ids, r.pts.d_phi, c->d_u[c->now], c->d_u[c->prev], r.derivs == 2 ? c->d_u[c->spare] : c->d_u[c->prev],
        c->dt, c->dt2, r.derivs, r.d_ring + (int64_t)slot * r.pts.np * ncomp);
    return HQ_OK;
}

/* ---- trackers: what is done with every table of every kind alike ---- */

/* the state of one tracker as it is before its first sample: every table filled with its byte on the compute stream, in
 * place when this returns */
static int hq_tracker_zero(hq_ctx* c, hq_ctx::hq_tracker& t, const hq_state_tables& tl)
{
    for (int i = 0; i < tl.n; i++) {
        HQ_HIP(hipMemsetAsync(tl.t[i].dev, tl.t[i].reset, tl.t[i].whole, c->stream));
        HQ_HIP(hipStreamSynchronize(c->stream));
    }
    t.nsamples = 0;
    return HQ_OK;
}
static int hq_peak_zero(hq_ctx* c, hq_ctx::hq_peak_tracker& t) { return hq_tracker_zero(c, t, t.tables()); }
static int hq_spec_zero(hq_ctx* c, hq_ctx::hq_spec_tracker& t) { return hq_tracker_zero(c, t, t.tables()); }
static int hq_deform_zero(hq_ctx* c, hq_ctx::hq_deform_tracker& t) { return hq_tracker_zero(c, t, t.tables()); }

/* the state crosses PCIe as the device keeps it, one copy per table, to or from the caller's array in the caller's layout
 * (hq_state_table.h).  A table without bytes -- no points, no filled slot -- does not travel. */
static int hq_tracker_copy(hq_ctx* c, const hq_ctx::hq_tracker& t, const hq_state_tables& tl, bool to_caller)
{
    const size_t np = (size_t)t.pts.np;
    std::vector<unsigned char> stage[HQ_STATE_MAX_TABLES];
    int64_t bytes = 0;
    for (int i = 0; i < tl.n; i++) {
        const hq_state_table& tb = tl.t[i];
        if (!hq_state_table_bytes(tb, np) || (!tb.host && to_caller && tb.optional)) continue;
        if (!tb.host) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
        stage[i].resize(hq_state_table_bytes(tb, np));
        if (to_caller)
            HQ_HIP(hipMemcpyAsync(stage[i].data(), tb.dev, stage[i].size(), hipMemcpyDeviceToHost, c->stream));
        else {
            hq_state_transpose(tb, np, false, tb.host, stage[i].data());
            HQ_HIP(hipMemcpyAsync(tb.dev, stage[i].data(), stage[i].size(), hipMemcpyHostToDevice, c->stream));
        }
        bytes += (int64_t)stage[i].size();
    }
    if (!bytes) return HQ_OK;
    HQ_HIP(hipStreamSynchronize(c->stream));
    for (int i = 0; i < tl.n && to_caller; i++)
        if (!stage[i].empty()) hq_state_transpose(tl.t[i], np, true, stage[i].data(), tl.t[i].host);
    (to_caller ? c->d2h_bytes : c->h2d_bytes) += bytes;
    return HQ_OK;
}

static int hq_tracker_fetch(hq_ctx* c, const hq_ctx::hq_tracker& t, const hq_state_tables& tl, int64_t* nsamples)
{
    *nsamples = t.nsamples;
    return hq_tracker_copy(c, t, tl, true);
}
static int hq_tracker_load(hq_ctx* c, hq_ctx::hq_tracker& t, const hq_state_tables& tl, int64_t nsamples)
{
    t.nsamples = nsamples;
    return hq_tracker_copy(c, t, tl, false);
}

/* what hq_*_fetch, _load and _reset begin with: the arguments they cannot do without (`args`; `text` if one is missing) and
 * the tracker of that handle (hq_tracker_find); then the device, and the steps enqueued so far behind them */
template <typename T>
static int hq_tracker_find(hq_ctx* c, bool args, const char* text, std::vector<T> hq_ctx::*outs, int32_t handle, T** t)
{
    if (!c || !args) return hq_fail(HQ_ERR_ARG, "%s", text);
    *t = hq_output_find(c->*outs, handle);
    return *t ? HQ_OK : hq_fail(HQ_ERR_ARG, "unknown %s tracker handle", T::kind);
}
template <typename T>
static int hq_tracker_open(hq_ctx* c, bool args, const char* text, std::vector<T> hq_ctx::*outs, int32_t handle, T** t)
{
    HQ_TRY(hq_tracker_find(c, args, text, outs, handle, t));
    HQ_HIP(hipSetDevice(c->device));
    HQ_HIP(hq_quiesce(c));
    return HQ_OK;
}

/* a description's points: a count, 1 or 8 nodes per point, and the arrays that go with them */
static bool hq_points_ok(int32_t npoints, int32_t K, const int32_t* ids, const double* phi)
{
    return npoints >= 0 && (K == 1 || K == 8) && (npoints == 0 || (ids && (K == 1 || phi)));
}
/* a description's mask of HQ_PEAK_DISP | VEL | ACC: some quantity and no other bit */
static bool hq_quantities_ok(int32_t q) { return q != 0 && (q & ~(HQ_PEAK_DISP | HQ_PEAK_VEL | HQ_PEAK_ACC)) == 0; }
/* an output that reads d_u[spare] as u(t - 2 dt) is refused where no kernel keeps it */
static int hq_spare_check(const hq_ctx* c, bool reads_spare)
{
    return reads_spare && c->variant != HQ_VARIANT_PATCH ? hq_fail(HQ_ERR_STATE, "u(t - 2 dt) is kept by the patch variant only%s", "") : HQ_OK;
}

/* head of a step, where hq_record_launch sits and behind the same waits: one hq_k_peak launch per due tracker on the
 * compute stream.  A launch that tracks accelerations reads d_u[spare] as u(t - 2 dt), the buffer THIS step's bricks and
 * exchange chain overwrite: their streams are held back behind it, exactly as behind hq_k_record.  Without accelerations
 * the launch reads d_u[now] and d_u[prev] only, which this step only reads -- and the next step's kernels follow on the
 * compute stream or wait for events recorded behind the launch -- so nothing is held: a velocity map must not serialise
 * every step of its run. */
static void hq_peak_launch(hq_ctx* c, hq_ctx::hq_peak_tracker& t)
{
    t.nsamples++;
    if (t.pts.np <= 0) return;
    const hq_real* u3 = (t.quantities & HQ_PEAK_ACC) ? c->d_u[c->spare] : c->d_u[c->prev];
    const auto k = t.pts.K == 1 ? hq_k_peak<1> : hq_k_peak<8>;
    k<<<hq_blocks(t.pts.np, 256), 256, 0, c->stream>>>(t.pts.np, t.pts.d_ids, t.pts.d_phi, c->d_u[c->now], c->d_u[c->prev], u3,
                                                        c->dt, c->dt2, t.quantities, c->step, t.d_pk, t.d_when);
}

/* head of a step, where hq_peak_launch sits and behind the same waits: one hq_k_spec launch per due tracker on the compute
 * stream.  It reads d_u[spare] as u(t - 2 dt), as an acceleration peak tracker does: the caller holds the streams back. */
static void hq_spec_launch(hq_ctx* c, hq_ctx::hq_spec_tracker& t)
{
    t.nsamples++;
    if (t.pts.np <= 0) return;
    const auto k = t.pts.K == 1 ? hq_k_spec<1> : hq_k_spec<8>;
    k<<<hq_blocks(t.pts.np, 256), 256, 0, c->stream>>>(t.pts.np, t.pts.d_ids, t.pts.d_phi, c->d_u[c->now], c->d_u[c->prev],
                                                        c->d_u[c->spare], c->dt2, t.nper, t.d_coef, t.d_aprev, t.d_osc, t.d_sd);
}

/* a cumulative tracker's own: of the span, first / last step -1 and the count row 0; no Husid slot filled */
static int hq_cum_zero(hq_ctx* c, hq_ctx::hq_cum_tracker& t)
{
    HQ_TRY(hq_tracker_zero(c, t, t.tables()));
    const size_t np = (size_t)t.pts.np;
    for (int32_t q = 0; q < t.nq && np > 0; q++)
        HQ_HIP(hipMemsetAsync(t.d_span + ((size_t)q * HQ_CUM_NSPAN + 2) * np, 0, sizeof(int32_t) * np, c->stream));
    HQ_HIP(hipStreamSynchronize(c->stream));
    t.curve_steps.clear();
    return HQ_OK;
}

/* what hq_peak_add, hq_spec_add and hq_cum_add end with, the description checked and the tables allocated: the points, the
 * state as it is before the first sample, the cadence and a handle.  hq_deform_add builds its own tables -- gradient weights
 * in place of phi -- and ends with hq_tracker_enlist, `h2d` the bytes its uploads carried */
template <typename T, typename D>
static int hq_tracker_enlist(hq_ctx* c, T& t, const D* d, int64_t h2d, int (*zero)(hq_ctx*, T&), std::vector<T> hq_ctx::*outs, int32_t hq_ctx::*next_id, int32_t* handle)
{
    HQ_TRY(zero(c, t));
    c->h2d_bytes += h2d;
    t.due = { d->rate, d->first_step };
    t.id = (c->*next_id)++;
    *handle = t.id;
    (c->*outs).push_back(std::move(t));
    return HQ_OK;
}
template <typename T, typename D>
static int hq_tracker_added(hq_ctx* c, T& t, const D* d, int (*zero)(hq_ctx*, T&), std::vector<T> hq_ctx::*outs, int32_t hq_ctx::*next_id, int32_t* handle)
{
    HQ_TRY(hq_points_build(c, d->npoints, d->nodes_per_point, d->ids, d->phi, &t.pts));
    return hq_tracker_enlist(c, t, d, t.pts.h2d(), zero, outs, next_id, handle);
}

/* hq_peak_reset, hq_spec_reset, hq_cum_reset */
template <typename T>
static int hq_tracker_reset(hq_ctx* c, std::vector<T> hq_ctx::*outs, int32_t handle, int (*zero)(hq_ctx*, T&))
{
    T* t;
    HQ_TRY(hq_tracker_open(c, true, "null argument", outs, handle, &t));
    return zero(c, *t);
}

/* head of a step, where hq_peak_launch sits and behind the same waits: one hq_k_cum launch per due tracker on the compute
 * stream.  As with a peak tracker, only a mask with accelerations reads d_u[spare], and only then does the caller hold the
 * streams back.  The Husid slot is accounted HERE, on the host, from the count of due samples: this sample is number
 * n + 1; every husid_every-th one is stored, into slot (n + 1) / husid_every - 1, as long as that slot exists -- past the
 * last slot the sums go on growing and the curve simply ends. */
static void hq_cum_launch(hq_ctx* c, hq_ctx::hq_cum_tracker& t)
{
    const int64_t n1 = ++t.nsamples;
    int32_t slot = -1;
    if (t.husid_every > 0 && n1 % t.husid_every == 0 && n1 / t.husid_every - 1 < t.husid_slots) {
        slot = (int32_t)(n1 / t.husid_every - 1);
        t.curve_steps.resize((size_t)slot + 1, -1);
        t.curve_steps[(size_t)slot] = c->step;
    }
    if (t.pts.np <= 0) return;
    const hq_real* u3 = (t.quantities & HQ_PEAK_ACC) ? c->d_u[c->spare] : c->d_u[c->prev];
    const auto k = t.pts.K == 1 ? hq_k_cum<1> : hq_k_cum<8>;
    k<<<hq_blocks(t.pts.np, 256), 256, 0, c->stream>>>(t.pts.np, t.pts.d_ids, t.pts.d_phi, c->d_u[c->now], c->d_u[c->prev], u3,
                                                        c->dt, c->dt2, t.quantities, c->step, t.thr2, t.d_sum, t.d_span,
                                                        t.d_curve, slot);
}

/* head of a step, where hq_peak_launch sits and behind the same waits: one hq_k_deform launch per due tracker on the compute
 * stream.  It reads d_u[now] and, with a rate bit, d_u[prev], which this step only reads: nothing is ever held back. */
static void hq_deform_launch(hq_ctx* c, hq_ctx::hq_deform_tracker& t)
{
    t.nsamples++;
    if (t.pts.np <= 0) return;
    hq_k_deform<<<hq_blocks(t.pts.np, 256), 256, 0, c->stream>>>(t.pts.np, t.pts.d_ids, t.d_grad, t.d_lame, c->d_u[c->now], c->d_u[c->prev],
                                                                  c->dt, t.quantities, c->step, t.d_vals, t.d_when);
}

/* what of a snapshot is not device memory: the pinned mirror and the slots' events */
static void hq_output_free(hq_ctx::hq_snapshot& sn)
{
    if (sn.h_stage) hipHostFree(sn.h_stage);
    for (hipEvent_t e : sn.done) if (e) hipEventDestroy(e);
}

/* head of a step, where hq_record_launch sits and behind the same waits: one hq_k_snapshot launch per due snapshot on the
 * compute stream into the next free slot; the copy stream waits for it, carries the slot to its pinned mirror and records
 * the slot's done event.  The launch reads d_u[now] and d_u[prev], which this step only reads; the next step overwrites
 * d_u[prev], and its kernels follow this launch on the compute stream or wait for events recorded behind it.  The bricks'
 * and the exchange chain's streams are held back behind the launch all the same, as they are behind hq_k_record: the
 * launch then has the memory system to itself and its time is the whole of what a snapshot adds to its step. */
static int hq_snapshot_launch(hq_ctx* c, hq_ctx::hq_snapshot& sn)
{
    const int32_t slot = hq_step_ring_push(&sn.ring, c->step);
    if (slot < 0) return hq_fail(HQ_ERR_STATE, "a snapshot's slots are all pending%s", "");   /* (hq_output_check_room saw to it) */
    char* d = sn.d_stage + (size_t)slot * sn.slot_bytes;
    constexpr int32_t tile_rows = 256 * (16 / (int32_t)sizeof(hq_real));
    const int64_t ntiles = ((int64_t)sn.count + tile_rows - 1) / tile_rows;
    hq_k_snapshot<hq_real><<<(unsigned)std::min<int64_t>(ntiles, 8192), 256, 0, c->stream>>>(
        sn.first, sn.count, sn.d_map, c->d_u[c->now], c->d_u[c->prev], c->dt,
        (sn.fields & HQ_SNAP_TM1) ? (hq_real*)(d + sn.off[0]) : nullptr,
        (sn.fields & HQ_SNAP_TM2) ? (hq_real*)(d + sn.off[1]) : nullptr,
        (sn.fields & HQ_SNAP_VEL) ? (double*)(d + sn.off[2]) : nullptr);
    HQ_HIP(hipEventRecord(c->ev_output, c->stream));
    HQ_HIP(hipStreamWaitEvent(c->sstream, c->ev_output, 0));    /* (the record just made, whatever ev_output names later) */
    HQ_HIP(hipMemcpyAsync(sn.h_stage + (size_t)slot * sn.slot_bytes, d, sn.slot_bytes, hipMemcpyDeviceToHost, c->sstream));
    HQ_HIP(hipEventRecord(sn.done[(size_t)slot], c->sstream));
    c->d2h_bytes += (int64_t)sn.slot_bytes;
    return HQ_OK;
}

/* one launch per due tracker of one kind, of those that read d_u[spare] (`spare`) or of those that do not.  True if a launch
 * was made that the step's other streams must stay behind */
template <typename T>
static bool hq_trackers_launch(hq_ctx* c, std::vector<T>& trackers, bool spare, void (*launch)(hq_ctx*, T&))
{
    bool held = false;
    for (auto& t : trackers)
        if (t.reads_spare() == spare && hq_cadence_due(t.due, c->step)) {
            launch(c, t);
            held |= spare && t.pts.np > 0;
        }
    return held;
}

/* The head of a step: every due output in solver_run's order (psolve.c:4277-4280: checkpoint / wavefield, then planes /
 * stations), then the trackers.  The launches that the step's other streams must stay behind (every snapshot, every recorder,
 * a peak or cumulative tracker of accelerations, a spectrum tracker: the comments above tell why) go first; ONE record of ev_output behind the last of them -- a
 * snapshot's own serves if nothing followed it -- holds the bricks' stream and the exchange chain's, on the patch variant,
 * where there is such a stream.  The trackers that need no hold follow that record: the streams never wait for them. */
static int hq_outputs_enqueue(hq_ctx* c, bool brick_stream)
{
    const bool hold_b = brick_stream && c->bstream, hold_c = c->overlap && c->cstream;   /* the streams there are to hold */
    bool hold = false, recorded = false;         /* recorded: ev_output's record is behind the last launch so far */
    for (auto& sn : c->snaps)
        if (hq_cadence_due(sn.due, c->step)) { HQ_TRY(hq_snapshot_launch(c, sn)); hold = recorded = true; }
    for (auto& r : c->recs)
        if (hq_cadence_due(r.due, c->step)) { HQ_TRY(hq_record_launch(c, r)); if (r.pts.np > 0) { hold = true; recorded = false; } }
    /* the trackers that read u(t - 2 dt): a peak or cumulative tracker of accelerations, every spectrum tracker */
    bool held = hq_trackers_launch(c, c->peaks, true, hq_peak_launch);
    held |= hq_trackers_launch(c, c->specs, true, hq_spec_launch);
    held |= hq_trackers_launch(c, c->cums, true, hq_cum_launch);
    if (held) { hold = true; recorded = false; }
    if (hold && c->variant == HQ_VARIANT_PATCH && (hold_b || hold_c)) {
        if (!recorded) HQ_HIP(hipEventRecord(c->ev_output, c->stream));
        if (hold_b) HQ_HIP(hipStreamWaitEvent(c->bstream, c->ev_output, 0));
        if (hold_c) HQ_HIP(hipStreamWaitEvent(c->cstream, c->ev_output, 0));
    }
    hq_trackers_launch(c, c->peaks, false, hq_peak_launch);     /* the other trackers: no stream waits for them */
    hq_trackers_launch(c, c->cums, false, hq_cum_launch);
    hq_trackers_launch(c, c->deforms, false, hq_deform_launch);
    return HQ_OK;
}

/* every snapshot goes (the caller has waited for every stream that serves them); the other kinds are device memory only */
static void hq_outputs_drop(std::vector<hq_ctx::hq_snapshot>& snaps)
{
    for (auto& sn : snaps) hq_output_free(sn);
    snaps.clear();
}

/* hq_record_clear, hq_peak_clear, hq_spec_clear, hq_cum_clear: every output of one kind goes, behind the steps enqueued so far */
template <typename T>
static int hq_outputs_clear(hq_ctx* c, std::vector<T> hq_ctx::*outs)
{
    if (!c) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    if ((c->*outs).empty()) return HQ_OK;
    HQ_HIP(hipSetDevice(c->device));
    HQ_HIP(hq_quiesce(c));
    (c->*outs).clear();
    return HQ_OK;
}

/* ---- sample recorders: entry points (include/hq_solver.h) ---- */

extern "C" int hq_record_add(hq_ctx* c, const hq_recorder_desc* d, int32_t* handle)
{
    if (!c || !d || !handle) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    if (d->npoints < 0 || d->rate <= 0 || d->capacity <= 0 || d->derivs < 0 || d->derivs > 2 ||
        (d->npoints > 0 && (!d->ids || !d->phi)))
        return hq_fail(HQ_ERR_ARG, "bad recorder description%s", "");
    HQ_TRY(hq_spare_check(c, d->derivs == 2));
    HQ_HIP(hipSetDevice(c->device));
    hq_ctx::hq_recorder r;
    r.derivs = d->derivs;
    HQ_TRY(hq_points_build(c, d->npoints, 8, d->ids, d->phi, &r.pts));
    HQ_TRY(r.d_ring.alloc(&c->bytes, (size_t)d->capacity * (size_t)d->npoints * 3 * (size_t)(1 + d->derivs)));
    c->h2d_bytes += r.pts.h2d();
    r.open(d->rate, INT32_MIN, d->capacity);                     /* every multiple of the rate, wherever `step` is set to */
    r.id = c->rec_next_id++;
    *handle = r.id;
    c->recs.push_back(std::move(r));
    return HQ_OK;
}

extern "C" int hq_record_pending(hq_ctx* c, int32_t handle, int32_t* nsamples, int32_t* first_step)
{
    if (!c || !nsamples) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    const hq_ctx::hq_recorder* r = hq_output_find(c->recs, handle);
    if (!r) return hq_fail(HQ_ERR_ARG, "unknown recorder handle%s", "");
    *nsamples = r->ring.count;
    if (first_step) *first_step = hq_step_ring_first_step(&r->ring);
    return HQ_OK;
}

extern "C" int hq_record_fetch(hq_ctx* c, int32_t handle, int32_t max_samples, double* out, int32_t* steps,
                               int32_t* nfetched)
{
    if (!c || !out || !steps || !nfetched || max_samples < 0) return hq_fail(HQ_ERR_ARG, "bad argument%s", "");
    hq_ctx::hq_recorder* r = hq_output_find(c->recs, handle);
    if (!r) return hq_fail(HQ_ERR_ARG, "unknown recorder handle%s", "");
    *nfetched = 0;
    const int32_t n = std::min(max_samples, r->ring.count), head = r->ring.head;
    if (n == 0) return HQ_OK;
    HQ_HIP(hipSetDevice(c->device));
    HQ_HIP(hq_quiesce(c));
    const size_t row = (size_t)r->pts.np * 3 * (size_t)(1 + r->derivs);          /* doubles per sample */
    const int32_t first = std::min(n, r->ring.capacity - head);              /* up to the ring's end, then from its start */
    if (row > 0) {
        HQ_TRY(hq_copy_wait(out, r->d_ring + (size_t)head * row, sizeof(double) * row * (size_t)first, hipMemcpyDeviceToHost, c->stream));
        if (n > first)
            HQ_TRY(hq_copy_wait(out + (size_t)first * row, r->d_ring, sizeof(double) * row * (size_t)(n - first), hipMemcpyDeviceToHost, c->stream));
    }
    for (int32_t k = 0; k < n; k++) steps[k] = r->steps[(size_t)hq_step_ring_slot_at(&r->ring, k)];
    c->d2h_bytes += 8 * (int64_t)row * n;
    hq_step_ring_pop(&r->ring, n);
    *nfetched = n;
    return HQ_OK;
}

extern "C" int hq_record_clear(hq_ctx* c) { return hq_outputs_clear(c, &hq_ctx::recs); }

/* ---- peak-motion trackers: entry points (include/hq_solver.h) ---- */

extern "C" int hq_peak_add(hq_ctx* c, const hq_peak_desc* d, int32_t* handle)
{
    if (!c || !d || !handle) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    if (!hq_points_ok(d->npoints, d->nodes_per_point, d->ids, d->phi) || d->rate < 1 || !hq_quantities_ok(d->quantities))
        return hq_fail(HQ_ERR_ARG, "bad peak tracker description%s", "");
    HQ_TRY(hq_spare_check(c, (d->quantities & HQ_PEAK_ACC) != 0));
    HQ_HIP(hipSetDevice(c->device));
    hq_ctx::hq_peak_tracker t;
    t.quantities = d->quantities; t.nq = hq_peak_nq(d->quantities);
    const size_t n = (size_t)t.nq * (size_t)d->npoints;
    HQ_TRY(t.d_pk.alloc(&c->bytes, HQ_PEAK_NVAL * n));
    HQ_TRY(t.d_when.alloc(&c->bytes, HQ_PEAK_NWHEN * n));
    return hq_tracker_added(c, t, d, hq_peak_zero, &hq_ctx::peaks, &hq_ctx::peak_next_id, handle);
}

extern "C" int hq_peak_fetch(hq_ctx* c, int32_t handle, double* peaks, int32_t* when, int64_t* nsamples)
{
    hq_ctx::hq_peak_tracker* t;
    HQ_TRY(hq_tracker_open(c, peaks && when && nsamples, "null argument", &hq_ctx::peaks, handle, &t));
    return hq_tracker_fetch(c, *t, t->tables(peaks, when), nsamples);
}

extern "C" int hq_peak_load(hq_ctx* c, int32_t handle, const double* peaks, const int32_t* when, int64_t nsamples)
{
    hq_ctx::hq_peak_tracker* t;
    HQ_TRY(hq_tracker_open(c, peaks && when && nsamples >= 0, "bad argument", &hq_ctx::peaks, handle, &t));
    return hq_tracker_load(c, *t, t->tables(peaks, when), nsamples);
}

extern "C" int hq_peak_reset(hq_ctx* c, int32_t handle) { return hq_tracker_reset(c, &hq_ctx::peaks, handle, hq_peak_zero); }

extern "C" int hq_peak_clear(hq_ctx* c) { return hq_outputs_clear(c, &hq_ctx::peaks); }

/* ---- response-spectrum trackers: entry points (include/hq_solver.h) ---- */

extern "C" int hq_spec_add(hq_ctx* c, const hq_spec_desc* d, int32_t* handle)
{
    if (!c || !d || !handle) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    if (!hq_points_ok(d->npoints, d->nodes_per_point, d->ids, d->phi) || d->rate < 1 || d->nperiods < 1 ||
        d->nperiods > HQ_SPEC_MAX_PERIODS || !d->periods || !(d->damping >= 0.0 && d->damping < 1.0))
        return hq_fail(HQ_ERR_ARG, "bad spectrum tracker description%s", "");
    for (int32_t j = 0; j < d->nperiods; j++)                    /* finite and positive (x - x is NaN for an infinity) */
        if (!(d->periods[j] > 0.0) || d->periods[j] - d->periods[j] != 0.0)
            return hq_fail(HQ_ERR_ARG, "a period of a spectrum tracker is not finite and positive%s", "");
    HQ_TRY(hq_spare_check(c, true));
    HQ_HIP(hipSetDevice(c->device));
    hq_ctx::hq_spec_tracker t;
    t.nper = d->nperiods;
    t.coef.resize((size_t)HQ_SDOF_NCOEF * (size_t)t.nper);
    for (int32_t j = 0; j < t.nper; j++)
        hq_sdof_coef(d->periods[j], d->damping, (double)d->rate * c->dt, t.coef.data() + (size_t)HQ_SDOF_NCOEF * j);
    const size_t np = (size_t)d->npoints, n = np * (size_t)t.nper;
    HQ_TRY(t.d_coef.put(&c->bytes, t.coef, c->stream));
    HQ_TRY(t.d_aprev.alloc(&c->bytes, 3 * np));
    HQ_TRY(t.d_osc.alloc(&c->bytes, HQ_SPEC_NOSC * n));
    HQ_TRY(t.d_sd.alloc(&c->bytes, HQ_SPEC_NSD * n));
    HQ_TRY(hq_tracker_added(c, t, d, hq_spec_zero, &hq_ctx::specs, &hq_ctx::spec_next_id, handle));
    c->h2d_bytes += (int64_t)(sizeof(double) * HQ_SDOF_NCOEF * (size_t)d->nperiods);   /* (the coefficients) */
    return HQ_OK;
}

extern "C" int hq_spec_coefficients(hq_ctx* c, int32_t handle, double* coef)
{
    if (!c || !coef) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    const hq_ctx::hq_spec_tracker* t = hq_output_find(c->specs, handle);
    if (!t) return hq_fail(HQ_ERR_ARG, "unknown spectrum tracker handle%s", "");
    std::copy(t->coef.begin(), t->coef.end(), coef);
    return HQ_OK;
}

extern "C" int hq_spec_fetch(hq_ctx* c, int32_t handle, double* sd, double* osc, double* aprev, int64_t* nsamples)
{
    hq_ctx::hq_spec_tracker* t;
    HQ_TRY(hq_tracker_open(c, sd && nsamples, "null argument", &hq_ctx::specs, handle, &t));
    return hq_tracker_fetch(c, *t, t->tables(sd, osc, aprev), nsamples);
}

extern "C" int hq_spec_load(hq_ctx* c, int32_t handle, const double* sd, const double* osc, const double* aprev, int64_t nsamples)
{
    hq_ctx::hq_spec_tracker* t;
    HQ_TRY(hq_tracker_open(c, sd && osc && aprev && nsamples >= 0, "bad argument", &hq_ctx::specs, handle, &t));
    return hq_tracker_load(c, *t, t->tables(sd, osc, aprev), nsamples);
}

extern "C" int hq_spec_reset(hq_ctx* c, int32_t handle) { return hq_tracker_reset(c, &hq_ctx::specs, handle, hq_spec_zero); }

extern "C" int hq_spec_clear(hq_ctx* c) { return hq_outputs_clear(c, &hq_ctx::specs); }

/* ---- cumulative-intensity trackers: entry points (include/hq_solver.h) ---- */

extern "C" int hq_cum_add(hq_ctx* c, const hq_cum_desc* d, int32_t* handle)
{
    if (!c || !d || !handle) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    if (!hq_points_ok(d->npoints, d->nodes_per_point, d->ids, d->phi) || d->rate < 1 || !hq_quantities_ok(d->quantities))
        return hq_fail(HQ_ERR_ARG, "bad cumulative tracker description%s", "");
    if (!((d->husid_every == 0 && d->husid_slots == 0) || (d->husid_every >= 1 && d->husid_slots >= 1)))
        return hq_fail(HQ_ERR_ARG, "husid_every and husid_slots are both 0 or both >= 1%s", "");
    const int32_t nq = hq_peak_nq(d->quantities);
    for (int32_t q = 0; q < nq; q++)                             /* finite and >= 0 (x - x is NaN for an infinity) */
        if (!(d->threshold[q] >= 0.0) || d->threshold[q] - d->threshold[q] != 0.0)
            return hq_fail(HQ_ERR_ARG, "a threshold of a cumulative tracker is not finite and >= 0%s", "");
    HQ_TRY(hq_spare_check(c, (d->quantities & HQ_PEAK_ACC) != 0));
    HQ_HIP(hipSetDevice(c->device));
    hq_ctx::hq_cum_tracker t;
    t.quantities = d->quantities; t.nq = nq;
    t.husid_every = d->husid_every; t.husid_slots = d->husid_slots;
    for (int32_t b = 0, q = 0; b < HQ_PEAK_NQ; b++)              /* mask order -> quantity bit; squared once, here */
        if (d->quantities & (1 << b)) { t.thr2.v[b] = d->threshold[q] * d->threshold[q]; q++; }
    const size_t n = (size_t)nq * (size_t)d->npoints;
    HQ_TRY(t.d_sum.alloc(&c->bytes, HQ_CUM_NSUM * n));
    HQ_TRY(t.d_span.alloc(&c->bytes, HQ_CUM_NSPAN * n));
    HQ_TRY(t.d_curve.alloc(&c->bytes, HQ_CUM_NCURVE * n * (size_t)d->husid_slots));
    return hq_tracker_added(c, t, d, hq_cum_zero, &hq_ctx::cums, &hq_ctx::cum_next_id, handle);
}

/* only the filled slots of the curve travel */
extern "C" int hq_cum_fetch(hq_ctx* c, int32_t handle, double* sums, int32_t* span, double* curve, int32_t* curve_steps,
                            int32_t* nfilled, int64_t* nsamples)
{
    hq_ctx::hq_cum_tracker* t;
    HQ_TRY(hq_tracker_open(c, sums && span && nfilled && nsamples, "null argument", &hq_ctx::cums, handle, &t));
    *nfilled = (int32_t)t->curve_steps.size();
    if (curve_steps) std::copy(t->curve_steps.begin(), t->curve_steps.end(), curve_steps);
    return hq_tracker_fetch(c, *t, t->tables(sums, span, curve, t->curve_steps.size()), nsamples);
}

extern "C" int hq_cum_load(hq_ctx* c, int32_t handle, const double* sums, const int32_t* span, const double* curve,
                           const int32_t* curve_steps, int32_t nfilled, int64_t nsamples)
{
    hq_ctx::hq_cum_tracker* t;
    HQ_TRY(hq_tracker_find(c, sums && span && nsamples >= 0 && nfilled >= 0 && (nfilled == 0 || (curve && curve_steps)), "bad argument",
                           &hq_ctx::cums, handle, &t));
    /* the slots that nsamples due samples fill: the accounting of hq_cum_launch goes on from nsamples alone */
    const int64_t filled = t->husid_every > 0 ? std::min<int64_t>(nsamples / t->husid_every, t->husid_slots) : 0;
    if (nfilled != filled) return hq_fail(HQ_ERR_ARG, "nfilled is not what nsamples due samples fill of this tracker's curve%s", "");
    HQ_HIP(hipSetDevice(c->device));
    HQ_HIP(hq_quiesce(c));
    t->curve_steps.assign(curve_steps, curve_steps + nfilled);
    return hq_tracker_load(c, *t, t->tables(sums, span, curve, (size_t)nfilled), nsamples);
}

extern "C" int hq_cum_reset(hq_ctx* c, int32_t handle) { return hq_tracker_reset(c, &hq_ctx::cums, handle, hq_cum_zero); }

extern "C" int hq_cum_clear(hq_ctx* c) { return hq_outputs_clear(c, &hq_ctx::cums); }

/* ---- deformation trackers: entry points (include/hq_solver.h) ---- */

extern "C" int hq_deform_add(hq_ctx* c, const hq_deform_desc* d, int32_t* handle)
{
    if (!c || !d || !handle) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    const bool stress = (d->quantities & HQ_DEFORM_STRESS) != 0;
    if (d->npoints < 0 || d->rate < 1 || d->quantities == 0 || (d->quantities & ~HQ_DEFORM_ALL) != 0 ||
        (d->npoints > 0 && (!d->ids || !d->grad || (stress && !d->lame))))
        return hq_fail(HQ_ERR_ARG, "bad deformation tracker description%s", "");
    const size_t np = (size_t)d->npoints;
    for (size_t i = 0; i < 8 * np; i++)
        if (d->ids[i] < 0 || d->ids[i] >= c->N) return hq_fail(HQ_ERR_ARG, "node id out of range%s", "");
    for (size_t i = 0; stress && i < 2 * np; i++)                /* finite (x - x is NaN for an infinity), mu >= 0 */
        if (d->lame[i] - d->lame[i] != 0.0 || ((i & 1) && !(d->lame[i] >= 0.0)))
            return hq_fail(HQ_ERR_ARG, "a modulus of a deformation tracker is not finite, or mu < 0%s", "");
    HQ_HIP(hipSetDevice(c->device));
    hq_ctx::hq_deform_tracker t;
    t.quantities = d->quantities;
    /* device numbering; every table transposed so that consecutive lanes read consecutive addresses */
    std::vector<int32_t> ids(8 * np);
    std::vector<double> grad(24 * np), lame(stress ? 2 * np : 0);
    for (size_t p = 0; p < np; p++) {
        for (size_t k = 0; k < 8; k++) {
            const int32_t id = d->ids[8 * p + k];
            ids[k * np + p] = c->perm.empty() ? id : c->perm[(size_t)id];
        }
        for (size_t k = 0; k < 24; k++) grad[k * np + p] = d->grad[24 * p + k];
        for (size_t k = 0; stress && k < 2; k++) lame[k * np + p] = d->lame[2 * p + k];
    }
    t.pts.np = d->npoints; t.pts.K = 8;
    HQ_TRY(t.pts.d_ids.put(&c->bytes, ids, c->stream));
    HQ_TRY(t.d_grad.put(&c->bytes, grad, c->stream));
    if (stress) HQ_TRY(t.d_lame.put(&c->bytes, lame, c->stream));
    HQ_TRY(t.d_vals.alloc(&c->bytes, (size_t)hq_deform_nvals(d->quantities) * np));
    HQ_TRY(t.d_when.alloc(&c->bytes, (size_t)hq_deform_nwhen(d->quantities) * np));
    const int64_t h2d = (int64_t)(sizeof(int32_t) * ids.size() + sizeof(double) * (grad.size() + lame.size()));
    return hq_tracker_enlist(c, t, d, h2d, hq_deform_zero, &hq_ctx::deforms, &hq_ctx::deform_next_id, handle);
}

extern "C" int hq_deform_fetch(hq_ctx* c, int32_t handle, double* vals, int32_t* when, int64_t* nsamples)
{
    hq_ctx::hq_deform_tracker* t;
    HQ_TRY(hq_tracker_open(c, vals && when && nsamples, "null argument", &hq_ctx::deforms, handle, &t));
    return hq_tracker_fetch(c, *t, t->tables(vals, when), nsamples);
}

extern "C" int hq_deform_load(hq_ctx* c, int32_t handle, const double* vals, const int32_t* when, int64_t nsamples)
{
    hq_ctx::hq_deform_tracker* t;
    HQ_TRY(hq_tracker_open(c, vals && when && nsamples >= 0, "bad argument", &hq_ctx::deforms, handle, &t));
    return hq_tracker_load(c, *t, t->tables(vals, when), nsamples);
}

extern "C" int hq_deform_reset(hq_ctx* c, int32_t handle) { return hq_tracker_reset(c, &hq_ctx::deforms, handle, hq_deform_zero); }

extern "C" int hq_deform_clear(hq_ctx* c) { return hq_outputs_clear(c, &hq_ctx::deforms); }

/* ---- field snapshots: entry points (include/hq_solver.h) ---- */

extern "C" int hq_snapshot_add(hq_ctx* c, const hq_snapshot_desc* d, int32_t* handle)
{
    if (!c || !d || !handle) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    const int32_t all = HQ_SNAP_TM1 | HQ_SNAP_TM2 | HQ_SNAP_VEL;
    if (d->count < 1 || d->first < 0 || (int64_t)d->first + d->count > c->N || d->rate < 1 || d->slots < 1 ||
        d->fields == 0 || (d->fields & ~all) != 0)
        return hq_fail(HQ_ERR_ARG, "bad snapshot description%s", "");
    HQ_HIP(hipSetDevice(c->device));
    hq_ctx::hq_snapshot sn;
    sn.first = d->first; sn.count = d->count; sn.fields = d->fields;
    auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t n3 = 3 * (size_t)d->count;
    size_t at = 0;
    sn.off[0] = at; if (d->fields & HQ_SNAP_TM1) at += pad(sizeof(hq_real) * n3);
    sn.off[1] = at; if (d->fields & HQ_SNAP_TM2) at += pad(sizeof(hq_real) * n3);
    sn.off[2] = at; if (d->fields & HQ_SNAP_VEL) at += pad(sizeof(double) * n3);
    sn.slot_bytes = at;
    const bool had_stream = c->sstream != nullptr;
    int rc = sn.d_stage.alloc(&c->bytes, sn.slot_bytes * (size_t)d->slots);
    if (rc == HQ_OK && !c->perm.empty())                         /* perm[first .. first + count): the caller's id -> the device's */
        rc = sn.d_map.put(&c->bytes, c->perm.data() + d->first, (size_t)d->count, c->stream);
    if (rc == HQ_OK && hipHostMalloc((void**)&sn.h_stage, sn.slot_bytes * (size_t)d->slots, hipHostMallocDefault) != hipSuccess) {
        sn.h_stage = nullptr;
        rc = hq_fail(HQ_ERR_NOMEM, "hipHostMalloc failed for the snapshot's pinned buffers%s", "");
    }
    hipError_t e = hipSuccess;
    if (rc == HQ_OK && !c->sstream) e = hipStreamCreateWithFlags(&c->sstream, hipStreamNonBlocking);
    sn.done.assign((size_t)d->slots, nullptr);
    for (int32_t k = 0; k < d->slots && rc == HQ_OK && e == hipSuccess; k++)
        e = hipEventCreateWithFlags(&sn.done[(size_t)k], hipEventDisableTiming);
    if (rc != HQ_OK || e != hipSuccess) {                        /* (the device memory unwinds by scope) */
        hq_output_free(sn);
        if (!had_stream && c->sstream) { hipStreamDestroy(c->sstream); c->sstream = nullptr; }
        (void)hipGetLastError();
        return rc != HQ_OK ? rc : hq_fail(HQ_ERR_DEVICE, "hq_snapshot_add failed: %s", hipGetErrorString(e));
    }
    if (sn.d_map) c->h2d_bytes += 4 * (int64_t)d->count;
    sn.open(d->rate, d->first_step, d->slots);
    sn.id = c->snap_next_id++;
    *handle = sn.id;
    c->snaps.push_back(std::move(sn));
    return HQ_OK;
}

extern "C" int hq_snapshot_pending(hq_ctx* c, int32_t handle, int32_t* npending, int32_t* nready, int32_t* first_step)
{
    if (!c || !npending) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    const hq_ctx::hq_snapshot* sn = hq_output_find(c->snaps, handle);
    if (!sn) return hq_fail(HQ_ERR_ARG, "unknown snapshot handle%s", "");
    *npending = sn->ring.count;
    if (nready) {
        int32_t n = 0;
        for (int32_t k = 0; k < sn->ring.count; k++)
            n += hipEventQuery(sn->done[(size_t)hq_step_ring_slot_at(&sn->ring, k)]) == hipSuccess;
        (void)hipGetLastError();                                 /* (hipErrorNotReady is an answer, not an error) */
        *nready = n;
    }
    if (first_step) *first_step = hq_step_ring_first_step(&sn->ring);
    return HQ_OK;
}

/* `bytes` from the pinned mirror into the caller's array; the large ones on all host threads (one thread moves ~10 GB/s) */
static void hq_host_copy(void* dst, const void* src, size_t bytes)
{
    const size_t chunk = (size_t)4 << 20;
    const int64_t nchunks = (int64_t)((bytes + chunk - 1) / chunk);
#pragma omp parallel for schedule(static) if (nchunks > 4)
    for (int64_t k = 0; k < nchunks; k++) {
        const size_t at = (size_t)k * chunk;
        memcpy((char*)dst + at, (const char*)src + at, std::min(chunk, bytes - at));
    }
}

extern "C" int hq_snapshot_fetch(hq_ctx* c, int32_t handle, hq_real* tm1, hq_real* tm2, double* vel, int32_t* step)
{
    if (!c || !step) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    hq_ctx::hq_snapshot* sn = hq_output_find(c->snaps, handle);
    if (!sn) return hq_fail(HQ_ERR_ARG, "unknown snapshot handle%s", "");
    if ((tm1 && !(sn->fields & HQ_SNAP_TM1)) || (tm2 && !(sn->fields & HQ_SNAP_TM2)) || (vel && !(sn->fields & HQ_SNAP_VEL)))
        return hq_fail(HQ_ERR_ARG, "the snapshot does not hold a field that an output pointer was given for%s", "");
    *step = -1;
    if (sn->ring.count == 0) return HQ_OK;
    HQ_HIP(hipSetDevice(c->device));
    HQ_HIP(hipEventSynchronize(sn->done[(size_t)sn->ring.head]));   /* this slot's copy -- not the steps enqueued behind it */
    const char* h = sn->h_stage + (size_t)sn->ring.head * sn->slot_bytes;
    const size_t n3 = 3 * (size_t)sn->count;
    if (tm1) hq_host_copy(tm1, h + sn->off[0], sizeof(hq_real) * n3);
    if (tm2) hq_host_copy(tm2, h + sn->off[1], sizeof(hq_real) * n3);
    if (vel) hq_host_copy(vel, h + sn->off[2], sizeof(double) * n3);
    *step = hq_step_ring_first_step(&sn->ring);
    hq_step_ring_pop(&sn->ring, 1);
    return HQ_OK;
}

extern "C" int hq_snapshot_clear(hq_ctx* c)
{
    if (!c) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    if (c->snaps.empty()) return HQ_OK;
    HQ_HIP(hipSetDevice(c->device));
    HQ_HIP(hq_quiesce(c));
    HQ_HIP(hipStreamSynchronize(c->sstream));
    hq_outputs_drop(c->snaps);
    hipStreamDestroy(c->sstream); c->sstream = nullptr;   /* (the copy stream goes with the snapshots: here and in hq_destroy) */
    return HQ_OK;
}

#endif
