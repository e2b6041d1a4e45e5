"""Response-spectrum trackers (hq_spec_add / _coefficients / _fetch / _load / _reset / _clear, include/hq_solver.h): the
oscillators hq_k_spec keeps per point and period on the device, against the project's own pinned chain.

A tracker's input is hq_k_record's acceleration column bit for bit, and its recursion is csrc/hq_sdof.h, the text hqh_spec_fold
compiles for the host.  So every tracker here gets a RECORDER TWIN on the same context -- the same points (for a tracker of
single nodes the node repeated 8 times with weights (1, 0, ..., 0)), the same rate, derivs = 2, room for the whole run -- and
the expectation is np.array_equal between hq_spec_fetch (sd, osc, aprev, nsamples) and host.spec_fold of the twin's acceleration
columns with hq_spec_coefficients' table, which must itself equal host.sdof_coef.  The comparison is made on ONE trajectory,
never between two solvers (tests/test_gpu_recorders.py tells why).  A recorder knows no first_step: samples of earlier steps are
dropped before the fold.  Against the oracle the bar is the project's relative L-inf one, 1e-9 of every column's maximum over
the points, on the root of the squared column."""
import ctypes

import numpy as np
import pytest

import hercules_amd as ha
from hercules_amd import capi, host
from tests.test_gpu_peaks import (BATCHES, CADENCES, NSTEPS, _add_twin, _c1_solver, big_box, brick_mode, c1,  # noqa: F401
                                  c1_oracle)
from tests.test_gpu_recorders import _field

pytestmark = pytest.mark.gpu

TOL = 1e-9
PERIODS = [0.01, 0.02, 0.05, 0.1, 0.3]                     # an odd count: the loop's unrolled pair and its tail
ZETA = 0.05


def _fold_twin(s, t, coef, first_step=0, into=None):
    """host.spec_fold of the acceleration columns of everything the twin holds (from first_step on) -> (sd, osc, aprev, n)."""
    steps, vals = s.record_fetch(t)
    keep = steps >= first_step
    sd, osc, aprev = host.spec_fold(coef, vals[keep][:, :, 6:9], *(into or (None, None, None)))
    return sd, osc, aprev, int(keep.sum())


def _same(got, want):
    assert got[3] == want[3], (got[3], want[3])
    for g, w, name in zip(got[:3], want[:3], ("sd", "osc", "aprev")):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5])


def _coef(s, h, periods, zeta, step_h):
    coef = s.spec_coefficients(h)
    assert np.array_equal(coef, host.sdof_coef(periods, zeta, step_h))
    return coef


# ---------------------------------------------------------------------------------------------------------------------
# 1 + 2. the C1 box from rest: against the twins, against the oracle
# ---------------------------------------------------------------------------------------------------------------------

def _c1_run(c1, precision, rate, first):
    """-> [(tracker's fetch, twin's fold)] for the surface map (K = 1) and the stations (K = 8)."""
    s = _c1_solver(c1, precision)
    cap = NSTEPS // rate + 1
    hs = [s.spec_add(c1["surface"], None, rate=rate, first_step=first, periods=PERIODS, damping=ZETA),
          s.spec_add(c1["ids"], c1["phi"], rate=rate, first_step=first, periods=PERIODS, damping=ZETA)]
    ts = [_add_twin(s, c1["surface"], None, rate, cap), _add_twin(s, c1["ids"], c1["phi"], rate, cap)]
    for n in BATCHES:
        s.run(n)
    assert s.info()["step"] == NSTEPS
    out = [(s.spec_fetch(h), _fold_twin(s, t, _coef(s, h, PERIODS, ZETA, rate * c1["dt"]), first)) for h, t in zip(hs, ts)]
    s.close()
    return out


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("rate,first", CADENCES)
def test_trackers_equal_their_recorder_twins(c1, brick_mode, precision, rate, first):
    """240 steps in batches of 7, 93 and 140, five periods: the surface map (289 points: two workgroups, the second partial)
    and the station tracker (5 points: a partial wave) equal the fold of their twins' acceleration columns bit for bit."""
    out = _c1_run(c1, precision, rate, first)
    for got, want in out:
        _same(got, want)
        assert got[3] == len(range(first, NSTEPS, rate))
        assert got[0].shape[1:] == (5, 4) and (got[0] > 0).all()          # the wave reached every point on every axis
        assert np.isfinite(got[1]).all() and (got[1] != 0).all()
    assert len(np.unique(out[0][0][0][:, :, 3])) > 500


def _rooted(sd):
    r = sd.copy()
    r[:, :, 3] = np.sqrt(r[:, :, 3])
    return r


@pytest.mark.parametrize("rate,first", CADENCES)
def test_trackers_match_the_oracle(c1, c1_oracle, brick_mode, rate, first):
    """The same run against the oracle (double): its accelerations folded by host.spec_fold; every column of sd within 1e-9
    of that column's maximum over the points, the root of the squared column.  And, on the ORACLE's values alone, the case
    is worth the name, for every period: no (point, axis) of the surface map peaks at the first sample, at most 25 % at the
    last one, the peaks fall on at least 30 distinct samples."""
    steps = np.arange(first, NSTEPS, rate)
    coef = host.sdof_coef(PERIODS, ZETA, rate * c1["dt"])
    want = [host.spec_fold(coef, smp[steps][:, :, 6:9]) for smp in c1_oracle]
    acc = np.ascontiguousarray(c1_oracle[0][steps][:, :, 6:9])
    st = host.spec_fold(coef, acc[:0])
    absx = np.zeros((len(steps),) + st[1][:, :, 0].shape)
    for k in range(len(steps)):
        host.spec_fold(coef, acc[k:k + 1], *st)
        absx[k] = np.abs(st[1][:, :, 0])
    assert np.array_equal(st[0], want[0][0]) and np.array_equal(absx.max(axis=0), want[0][0][:, :, :3])
    when = absx.argmax(axis=0)                               # [np, nper, 3]: the first occurrence of the maximum
    for j, T in enumerate(PERIODS):
        first_frac, last_frac = float((when[:, j] == 0).mean()), float((when[:, j] == len(steps) - 1).mean())
        distinct = len(np.unique(when[:, j]))
        print("rate %d, T = %g: %.1f%% peak at the first sample, %.1f%% at the last, %d distinct peak samples"
              % (rate, T, 100 * first_frac, 100 * last_frac, distinct))
        assert first_frac == 0.0 and last_frac <= 0.25 and distinct >= 30
    worst = 0.0
    for (got, _), w, name in zip(_c1_run(c1, "f64", rate, first), want, ("surface", "stations")):
        g, ws = _rooted(got[0]), _rooted(w[0])
        for j in range(len(PERIODS)):
            for col in range(4):
                err, scale = np.abs(g[:, j, col] - ws[:, j, col]).max(), ws[:, j, col].max()
                print("%s period %d column %d: err %.3e of %.3e" % (name, j, col, err, scale))
                assert scale > 0 and err <= TOL * scale, (name, j, col, err, scale)
                worst = max(worst, err / scale)
    print("worst: %.3e" % worst)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the u(t - 2 dt) hazard
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nper", [1, 32])
@pytest.mark.parametrize("brick_stream", [1, 0])
def test_samples_are_folded_before_the_bricks_overwrite_the_oldest_field(big_box, brick_mode, brick_stream, nper):
    """d_u[spare] is u(t - 2 dt) AND the buffer the step's kernels write u(t + dt) into: with the bricks on a stream of their
    own nothing but the tracker's event orders its launch ahead of them (the twin's launch comes BEFORE hq_k_spec is
    enqueued, so an event behind it would not cover the tracker).  24 steps enqueued by ONE hq_run, one period and the
    maximum of 32: equal to the twin."""
    b = big_box
    periods = np.geomspace(2e-3, 0.05, nper) if nper > 1 else np.array([2e-3])
    s = b["box"].create_solver(tm1=b["u1"], tm2=b["u2"], options={"brick_stream": brick_stream})
    s.set_source(b["loaded"], b["F"])
    h = s.spec_add(b["nodes"], None, rate=1, periods=periods, damping=ZETA)
    t = _add_twin(s, b["nodes"], None, 1, 24)
    s.run(24)
    got = s.spec_fetch(h)
    want = _fold_twin(s, t, _coef(s, h, periods, ZETA, b["dt"]))
    info = s.info()
    s.close()
    if brick_mode == "bricks":
        assert info["brick_units"] > 0 and info["brick_stream"] == brick_stream
    else:
        assert info["brick_units"] == 0
    assert got[3] == 24 and got[0].shape == (257, nper, 4) and (got[0] > 0).all()
    _same(got, want)


# ---------------------------------------------------------------------------------------------------------------------
# 4. two partitions in one process
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("overlap", [0, 1])
def test_two_partitions_track_through_group_run(brick_mode, overlap):
    """Two partitions of a 32 x 32 x 16 box in one process (hq_group_link), 30 steps in one hq_group_run (overlap = 1: the
    exchange chain on a stream of its own, which a spectrum tracker's due step holds back).  Each rank tracks all the nodes
    it shares with the other and some of its own (K = 1) and stations around the cut (K = 8, rate 2): equal to the twins,
    and a shared node's sd is the same on both ranks, bit for bit -- its displacement is."""
    nx, ny, nz, h, dt = 32, 32, 16, 15.0, 3e-4
    boxes = [host.Box(nx, ny, nz, h, dt, 30.0, rank=r, nranks=2) for r in range(2)]
    L = np.array([nx * h, ny * h, nz * h])
    pts = np.random.default_rng(5).uniform(0.0, 1.0, (24, 3)) * L
    periods = [3e-3, 0.01, 0.03]
    nodes, stations, gids, nshared = [], [], [], []
    for bx in boxes:
        sch = bx.schedule()
        sh = np.unique(np.concatenate([m for _, m in sch["c"] + sch["s"]])).astype(np.int32)
        assert len(sh) > 0
        ijk = bx.node_ijk[sh].astype(np.int64)
        gids.append((ijk[:, 2] * (ny + 1) + ijk[:, 1]) * (nx + 1) + ijk[:, 0])
        own = np.setdiff1d(np.arange(bx.info["nharbored"], dtype=np.int32), sh)[::37]
        nodes.append(np.concatenate([sh, own]).astype(np.int32))
        nshared.append(len(sh))
        ids, phi, mine = bx.stations(pts)
        stations.append((ids[mine != 0], phi[mine != 0]))
    assert sorted(gids[0]) == sorted(gids[1])
    assert len(stations[0][0]) + len(stations[1][0]) == len(pts) and min(len(st[0]) for st in stations) > 0
    fields = [_field(bx, 31) for bx in boxes]
    solvers = [bx.create_solver(tm1=u, tm2=0.999 * u, options={"overlap": overlap}) for bx, u in zip(boxes, fields)]
    capi.group_link(solvers)
    hn = [s.spec_add(n, None, rate=1, periods=periods, damping=ZETA) for s, n in zip(solvers, nodes)]
    hs = [s.spec_add(ids, phi, rate=2, periods=periods, damping=0.2) for s, (ids, phi) in zip(solvers, stations)]
    tn = [_add_twin(s, n, None, 1, 30) for s, n in zip(solvers, nodes)]
    ts = [_add_twin(s, ids, phi, 2, 15) for s, (ids, phi) in zip(solvers, stations)]
    capi.group_run(solvers, 30)
    got_n = [s.spec_fetch(h) for s, h in zip(solvers, hn)]
    got_s = [s.spec_fetch(h) for s, h in zip(solvers, hs)]
    want_n = [_fold_twin(s, t, _coef(s, h, periods, ZETA, dt)) for s, t, h in zip(solvers, tn, hn)]
    want_s = [_fold_twin(s, t, _coef(s, h, periods, 0.2, 2 * dt)) for s, t, h in zip(solvers, ts, hs)]
    for s in solvers:
        s.close()
    for bx in boxes:
        bx.close()
    for r in range(2):
        assert got_n[r][3] == 30 and got_s[r][3] == 15
        assert (got_n[r][0] > 0).all()
        _same(got_n[r], want_n[r])
        _same(got_s[r], want_s[r])
    a, b = np.argsort(gids[0]), np.argsort(gids[1])          # the shared nodes lead each rank's list: pair them by position
    assert np.array_equal(got_n[0][0][:nshared[0]][a], got_n[1][0][:nshared[1]][b])


# ---------------------------------------------------------------------------------------------------------------------
# 5. all kinds due on one step
# ---------------------------------------------------------------------------------------------------------------------

def test_all_kinds_due_on_one_step(big_box, brick_mode):
    """A snapshot, a recorder, an acceleration peak tracker and a spectrum tracker on one context, all at rate 2, 24 steps in
    one hq_run: each equals what it equals alone on that trajectory -- the recorder a rate-1 recorder's every second sample,
    the snapshot's u(t) the recorder's displacement columns at its nodes (unit weights: the row itself), the trackers the
    folds of the recorder's samples."""
    b = big_box
    nodes, dt = b["nodes"], b["dt"]
    periods = [2e-3, 5e-3, 0.02]
    s = b["box"].create_solver(tm1=b["u1"], tm2=b["u2"])
    s.set_source(b["loaded"], b["F"])
    hsn = s.snapshot_add(rate=2, fields=capi.HQ_SNAP_TM1, slots=12)
    hr = _add_twin(s, nodes, None, 2, 12)
    hp = s.peak_add(nodes, None, rate=2, quantities=capi.HQ_PEAK_ACC)
    hq = s.spec_add(nodes, None, rate=2, periods=periods, damping=ZETA)
    hr1 = _add_twin(s, nodes, None, 1, 24)
    s.run(24)
    steps, vals = s.record_fetch(hr)
    steps1, vals1 = s.record_fetch(hr1)
    pk = s.peak_fetch(hp)
    sp = s.spec_fetch(hq)
    coef = _coef(s, hq, periods, ZETA, 2 * dt)
    snaps = [s.snapshot_fetch(hsn) for _ in range(12)]
    s.close()
    assert np.array_equal(steps, np.arange(0, 24, 2)) and np.array_equal(steps1, np.arange(24))
    assert np.array_equal(vals, vals1[::2]) and np.abs(vals[:, :, 6:]).max() > 0
    assert [sn[0] for sn in snaps] == list(steps)
    for k, sn in enumerate(snaps):
        assert np.array_equal(np.asarray(sn[1], np.float64)[nodes], vals[k][:, :3])
    wp = host.peak_fold(steps, vals, capi.HQ_PEAK_ACC)
    assert pk[2] == 12 and np.array_equal(pk[0], wp[0]) and np.array_equal(pk[1], wp[1])
    _same(sp, host.spec_fold(coef, vals[:, :, 6:9]) + (12,))
    assert (sp[0] > 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 6. semantics on C1
# ---------------------------------------------------------------------------------------------------------------------

def test_an_empty_tracker_is_accepted(c1):
    s = _c1_solver(c1)
    h1 = s.spec_add(np.zeros(0, np.int32), None, rate=2, periods=PERIODS)
    h8 = s.spec_add(np.zeros((0, 8), np.int32), np.zeros((0, 8)), rate=1, first_step=3, periods=[0.1])
    s.run(10)
    sd, osc, aprev, n = s.spec_fetch(h1)
    assert sd.shape == (0, 5, 4) and osc.shape == (0, 5, 2, 3) and aprev.shape == (0, 3) and n == 5
    assert s.spec_fetch(h8)[3] == 7
    assert s.spec_coefficients(h8).shape == (1, 8)
    s.spec_load(h1, sd, osc, aprev, 3)
    assert s.spec_fetch(h1)[3] == 3
    s.spec_reset(h1)
    assert s.spec_fetch(h1)[3] == 0
    s.close()


def test_reset_and_load_resume_a_run(c1, brick_mode):
    """Fetch at step 100, reset (zeros, no samples), run 5, load what was fetched, run on to 240: the fold of the samples
    < 100, then the samples >= 105 folded into that state."""
    s = _c1_solver(c1)
    h = s.spec_add(c1["surface"], None, rate=1, periods=PERIODS, damping=ZETA)
    t = _add_twin(s, c1["surface"], None, 1, NSTEPS)
    coef = _coef(s, h, PERIODS, ZETA, c1["dt"])
    s.run(7)
    s.run(93)
    saved = s.spec_fetch(h)
    assert saved[3] == 100 and (saved[0] > 0).any()
    _same(s.spec_fetch(h), saved)                            # a fetch leaves the state in place
    only_sd = s.spec_fetch(h, osc=False, aprev=False)
    assert only_sd[1] is None and only_sd[2] is None and np.array_equal(only_sd[0], saved[0])
    s.spec_reset(h)
    sd, osc, aprev, n = s.spec_fetch(h)
    assert n == 0 and (sd == 0).all() and (osc == 0).all() and (aprev == 0).all() and sd.shape == saved[0].shape
    s.run(5)                                                 # ... and tracks on from rest
    sd, osc, aprev, n = s.spec_fetch(h)
    assert n == 5 and (sd > 0).any() and not np.array_equal(sd, saved[0])
    s.spec_load(h, *saved)
    _same(s.spec_fetch(h), saved)
    s.run(135)
    got = s.spec_fetch(h)
    steps, vals = s.record_fetch(t)
    s.close()
    st = host.spec_fold(coef, vals[steps < 100][:, :, 6:9])
    _same(st + (100,), saved)
    want = host.spec_fold(coef, vals[steps >= 105][:, :, 6:9], *st)
    _same(got, want + (235,))


def test_upload_keeps_the_state_and_moves_the_due_steps(c1, brick_mode):
    s = _c1_solver(c1)
    h = s.spec_add(c1["ids"], c1["phi"], rate=2, periods=PERIODS, damping=ZETA)
    t = _add_twin(s, c1["ids"], c1["phi"], 2, 32)
    coef = _coef(s, h, PERIODS, ZETA, 2 * c1["dt"])
    s.run(41)                                                # samples of steps 0, 2, ..., 40
    before = s.spec_fetch(h)
    tm1, tm2 = s.download()
    s.upload(tm1 * 1000.0, tm2 * 1000.0, 250)
    _same(s.spec_fetch(h), before)
    _same(before, _fold_twin(s, t, coef))
    s.run(3)                                                 # ... and of 250 and 252
    got = s.spec_fetch(h)
    steps, vals = s.record_fetch(t)
    s.close()
    assert before[3] == 21 and got[3] == 23 and np.array_equal(steps, [250, 252])
    want = host.spec_fold(coef, vals[:, :, 6:9], *[a.copy() for a in before[:3]])
    _same(got, want + (23,))
    assert (got[0] > before[0]).any()                        # the scaled field raised maxima


def test_bad_descriptions_and_cleared_handles(c1):
    ids, phi, surface = c1["ids"], c1["phi"], c1["surface"]
    sc = _c1_solver(c1, variant=ha.HQ_VARIANT_SCATTER)
    with pytest.raises(ha.HqError, match="patch variant"):   # HQ_ERR_STATE, as hq_gather3
        sc.spec_add(surface, None, periods=PERIODS)
    d = capi._SpecDesc(5, 8, ids.ctypes.data, phi.ctypes.data, 1, 0, 1, 0, np.array([0.1]).ctypes.data, 0.05)
    assert sc._lib.hq_spec_add(sc._h, ctypes.byref(d), ctypes.byref(ctypes.c_int32())) == -6      # HQ_ERR_STATE
    sc.close()

    s = _c1_solver(c1)
    bad8, bad1 = ids.copy(), surface.copy()
    bad8[3, 5] = s.N
    bad1[-1] = s.N
    ok = dict(ids=ids, phi=phi, periods=PERIODS)
    for kw in (dict(ids=bad8, phi=phi, periods=PERIODS), dict(ids=bad1, phi=None, periods=PERIODS),
               dict(ids=-1 - surface, phi=None, periods=PERIODS), dict(ok, rate=0), dict(ok, rate=-2), dict(ok, periods=[]),
               dict(ok, periods=np.full(33, 0.1)), dict(ok, periods=[0.1, 0.0]), dict(ok, periods=[0.1, -1.0]),
               dict(ok, periods=[np.nan]), dict(ok, periods=[np.inf, 0.1]), dict(ok, damping=-0.01), dict(ok, damping=1.0),
               dict(ok, damping=np.nan), dict(ok, damping=np.inf)):
        kw = dict(kw)
        with pytest.raises(ha.HqError):
            s.spec_add(kw.pop("ids"), kw.pop("phi"), **kw)
    lib = s._lib
    hh = ctypes.c_int32(-1)
    per = np.array([0.1, 0.2])
    for npts, k, i, p, q in ((-1, 8, ids, phi, per), (5, 4, ids, phi, per), (5, 0, ids, phi, per), (5, 8, None, phi, per),
                             (5, 8, ids, None, per), (5, 1, None, None, per), (5, 8, ids, phi, None)):
        d = capi._SpecDesc(npts, k, None if i is None else i.ctypes.data, None if p is None else p.ctypes.data, 1, 0, 2, 0,
                           None if q is None else q.ctypes.data, 0.05)
        assert lib.hq_spec_add(s._h, ctypes.byref(d), ctypes.byref(hh)) == -1
    good = capi._SpecDesc(5, 8, ids.ctypes.data, phi.ctypes.data, 1, 0, 2, 0, per.ctypes.data, 0.05)
    assert lib.hq_spec_add(s._h, ctypes.byref(good), None) == -1 and lib.hq_spec_add(s._h, None, ctypes.byref(hh)) == -1
    sd, osc, ap, cf, n = np.zeros(5 * 2 * 4), np.zeros(5 * 2 * 6), np.zeros(15), np.zeros(16), ctypes.c_int64()
    P = capi._ptr
    for handle in (0, 7, -1):                                # nothing was added
        assert lib.hq_spec_fetch(s._h, handle, P(sd), P(osc), P(ap), ctypes.byref(n)) == -1
        assert lib.hq_spec_load(s._h, handle, P(sd), P(osc), P(ap), ctypes.c_int64(0)) == -1
        assert lib.hq_spec_coefficients(s._h, handle, P(cf)) == -1
        assert lib.hq_spec_reset(s._h, handle) == -1
    bytes0 = s.info()["device_bytes"]
    h = s.spec_add(ids, phi, rate=1, periods=per)
    assert lib.hq_spec_fetch(s._h, h, None, P(osc), P(ap), ctypes.byref(n)) == -1
    assert lib.hq_spec_fetch(s._h, h, P(sd), P(osc), P(ap), None) == -1
    assert lib.hq_spec_fetch(s._h, h, P(sd), None, None, ctypes.byref(n)) == 0
    assert lib.hq_spec_coefficients(s._h, h, None) == -1
    assert lib.hq_spec_load(s._h, h, P(sd), None, P(ap), ctypes.c_int64(0)) == -1
    assert lib.hq_spec_load(s._h, h, P(sd), P(osc), None, ctypes.c_int64(0)) == -1
    assert lib.hq_spec_load(s._h, h, None, P(osc), P(ap), ctypes.c_int64(0)) == -1
    assert lib.hq_spec_load(s._h, h, P(sd), P(osc), P(ap), ctypes.c_int64(-1)) == -1
    h1 = s.spec_add(surface, None, rate=1, periods=PERIODS)
    assert h1 != h
    assert s.info()["device_bytes"] >= bytes0 + 5 * (8 * 12 + 8 * (3 + 2 * 10)) + 289 * (4 + 8 * (3 + 5 * 10))
    s.run(2)
    s.record_clear()                                         # spectrum trackers are neither recorders ...
    s.snapshot_clear()                                       # ... nor snapshots ...
    s.peak_clear()                                           # ... nor peak trackers
    assert s.spec_fetch(h)[3] == 2 and s.spec_fetch(h1)[3] == 2
    s.spec_clear()
    assert s.info()["device_bytes"] == bytes0
    for dead in (h, h1):
        assert lib.hq_spec_fetch(s._h, dead, P(sd), P(osc), P(ap), ctypes.byref(n)) == -1
        assert lib.hq_spec_reset(s._h, dead) == -1
        with pytest.raises(ha.HqError):
            s.spec_fetch(dead)
    s.run(10)                                                # tracks nothing
    s.spec_clear()                                           # nothing to drop: no error
    h2 = s.spec_add(ids, phi, rate=1, periods=per)
    assert h2 not in (h, h1) and s.spec_fetch(h2)[3] == 0   # handles are not reused
    s.close()


@pytest.mark.parametrize("runner", ["sync", "async"])
def test_a_tracker_survives_the_runners(c1, runner):
    """hqh_solver_run_on with device_recorders = 1 and hqh_solver_run_async drop their own recorders and snapshots and leave a
    caller's spectrum tracker alone: 60 steps in two calls, stations every 2 steps with accelerations; the tracker on the same
    stations at the same rate equals a fold of the samples the station callback was handed (hq_k_record's, same trajectory)."""
    box = c1["box"]
    loaded, pattern = box.point_source(500.0, 500.0, 100.0, 0.0, 90.0, 0.0)
    calls = []
    rp = box.run_params(loaded=loaded, pattern=pattern, moment=1e15, rise_time=0.02, source_window=16, device_recorders=1,
                        station_ids=c1["ids"], station_phi=c1["phi"], station_rate=2, station_derivs=2,
                        station_fn=lambda step, vals: calls.append((step, vals)))
    s = box.create_solver()
    h = s.spec_add(c1["ids"], c1["phi"], rate=2, periods=PERIODS, damping=ZETA)
    coef = _coef(s, h, PERIODS, ZETA, 2 * c1["dt"])
    for step0, n in ((0, 23), (23, 37)):
        if runner == "sync":
            box.solver_run(s, rp, step0, n)
        else:
            box.solver_run_async(s, rp, step0, n, slots=1)
    got = s.spec_fetch(h)
    with pytest.raises(ha.HqError):
        s.record_pending(0)                                  # the runner left no recorder behind
    s.close()
    assert [c[0] for c in calls] == list(range(0, 60, 2))
    want = host.spec_fold(coef, np.array([c[1] for c in calls])[:, :, 6:9])
    assert (want[0] > 0).all()
    _same(got, want + (30,))


# ---------------------------------------------------------------------------------------------------------------------
# 7. no traffic between fetches
# ---------------------------------------------------------------------------------------------------------------------

def test_nothing_crosses_pcie_until_a_fetch(c1):
    s = _c1_solver(c1)
    h1 = s.spec_add(c1["surface"], None, rate=1, periods=PERIODS)
    h8 = s.spec_add(c1["ids"], c1["phi"], rate=3, periods=[0.1, 0.2])
    s.sync()
    before = s.info()
    s.run(100)
    s.sync()
    after = s.info()
    assert after["pcie_d2h_bytes"] == before["pcie_d2h_bytes"] and after["pcie_h2d_bytes"] == before["pcie_h2d_bytes"]
    s.spec_fetch(h1, osc=False, aprev=False)
    a = s.info()
    assert a["pcie_d2h_bytes"] - after["pcie_d2h_bytes"] == 8 * 289 * (4 * 5) and a["pcie_h2d_bytes"] == after["pcie_h2d_bytes"]
    s.spec_fetch(h1)
    b = s.info()
    assert b["pcie_d2h_bytes"] - a["pcie_d2h_bytes"] == 8 * 289 * (4 * 5 + 6 * 5 + 3)
    s.spec_fetch(h1, osc=True, aprev=False)
    c = s.info()
    assert c["pcie_d2h_bytes"] - b["pcie_d2h_bytes"] == 8 * 289 * (4 * 5 + 6 * 5)
    s.spec_fetch(h8, osc=False, aprev=True)
    assert s.info()["pcie_d2h_bytes"] - c["pcie_d2h_bytes"] == 8 * 5 * (4 * 2 + 3)
    s.close()
