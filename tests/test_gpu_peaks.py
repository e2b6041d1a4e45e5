"""Peak-motion trackers (hq_peak_add / _fetch / _load / _reset / _clear, include/hq_solver.h): the running PGD / PGV / PGA state
hq_k_peak keeps per point on the device, against the project's own pinned chain.

A tracker's sample is hq_k_record's sample bit for bit, and its fold is csrc/hq_peak.h, the text hqh_peak_fold compiles for the
host.  So every tracker here gets a RECORDER TWIN on the same context -- the same points, the same rate, derivs = 2 (1 in the
scatter variant, which keeps no u(t - 2 dt)), room for the whole run; for a tracker of single nodes the twin's points are the
node repeated 8 times with weights (1, 0, ..., 0) -- and the expectation is np.array_equal between hq_peak_fetch and
hqh_peak_fold(hq_record_fetch), for the values, `when` and nsamples.  The comparison has to be made on ONE trajectory: two
identically built solvers differ in the last bits (tests/test_gpu_recorders.py tells why).  A recorder knows no first_step:
samples of earlier steps are dropped before the fold.  Against the oracle the bar is the project's relative L-inf one, 1e-9 of
every column's maximum over the points, on the roots of the squared columns."""
import ctypes

import numpy as np
import pytest

import hercules_amd as ha
from hercules_amd import capi, host
from oracle import herc_oracle as ho
from tests import helpers as H
from tests.test_gpu_recorders import _field, _unit_points

pytestmark = pytest.mark.gpu

TOL = 1e-9
D, V, A = capi.HQ_PEAK_DISP, capi.HQ_PEAK_VEL, capi.HQ_PEAK_ACC
ALL = D | V | A


@pytest.fixture(params=["bricks", "patches-only"])
def brick_mode(request, monkeypatch):
    """As shipped (hq_k_brick takes the simple nodes of uniform regions) and with HQ_NO_BRICKS=1 (patches everywhere)."""
    if request.param == "patches-only":
        monkeypatch.setenv("HQ_NO_BRICKS", "1")
    else:
        monkeypatch.delenv("HQ_NO_BRICKS", raising=False)
    return request.param


def _derivs(q):
    return 2 if q & A else 1 if q & V else 0


def _add_twin(s, ids, phi, rate, capacity, derivs=2):
    if phi is None:
        ids, phi = _unit_points(ids)
    return s.record_add(ids, phi, rate=rate, derivs=derivs, capacity=capacity)


def _fold_twin(s, h, q, first_step=0, into=None):
    """hqh_peak_fold of everything the twin holds (from first_step on) -> (peaks, when, samples folded)."""
    steps, vals = s.record_fetch(h)
    keep = steps >= first_step
    vals = np.ascontiguousarray(vals[keep][:, :, :3 * (1 + _derivs(q))])
    peaks, when = host.peak_fold(steps[keep], vals, q, *(into or (None, None)))
    return peaks, when, int(keep.sum())


def _same(got, want):
    assert got[2] == want[2], (got[2], want[2])
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape
    assert np.array_equal(got[1], want[1]), np.argwhere(got[1] != want[1])[:5]
    assert np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:5]


# ---------------------------------------------------------------------------------------------------------------------
# 1 + 2. the C1 box from rest: against the twins, against the oracle
# ---------------------------------------------------------------------------------------------------------------------

NSTEPS = 240
BATCHES = (7, 93, 140)
CADENCES = [(1, 0), (3, 6)]


@pytest.fixture(scope="module")
def c1():
    """16 x 16 x 8, h = 62.5, dt = 1e-3, at rest; one loaded node at grid position (4, 5, 3) pushed by
    (1, 0.5, -0.7) 1e9 sin^2(pi k / 40) for k < 40; the 289 nodes of the z = 0 face and the five C1 stations."""
    box = host.Box(H.C1_NX, H.C1_NY, H.C1_NZ, H.C1_H, 1e-3, 5.0)
    ijk = box.node_ijk
    loaded = np.nonzero((ijk[:, 0] == 4) & (ijk[:, 1] == 5) & (ijk[:, 2] == 3))[0].astype(np.int32)
    assert len(loaded) == 1
    k = np.arange(40)
    F = (np.sin(np.pi * k / 40) ** 2)[:, None, None] * 1e9 * np.array([1.0, 0.5, -0.7])[None, None, :]
    surface = np.nonzero(ijk[:, 2] == 0)[0].astype(np.int32)
    assert len(surface) == 289
    ids, phi, mine = box.stations(H.C1_STATIONS)
    assert mine.all()
    yield dict(box=box, loaded=loaded, F=F, surface=surface, ids=ids, phi=phi, dt=1e-3)
    box.close()


def _c1_solver(c1, precision="f64", variant=ha.HQ_VARIANT_AUTO):
    s = c1["box"].create_solver(precision=precision, variant=variant)
    s.set_source(c1["loaded"], c1["F"])
    return s


def _c1_run(c1, precision, rate, first):
    """The run of tests 1 and 2 -> [(tracker's fetch, twin's fold)] for the surface map (K = 1) and the stations (K = 8)."""
    s = _c1_solver(c1, precision)
    cap = NSTEPS // rate + 1
    hs = [s.peak_add(c1["surface"], None, rate=rate, first_step=first, quantities=ALL),
          s.peak_add(c1["ids"], c1["phi"], rate=rate, first_step=first, quantities=ALL)]
    ts = [_add_twin(s, c1["surface"], None, rate, cap), _add_twin(s, c1["ids"], c1["phi"], rate, cap)]
    for n in BATCHES:
        s.run(n)
    assert s.info()["step"] == NSTEPS
    out = [(s.peak_fetch(h), _fold_twin(s, t, ALL, first)) for h, t in zip(hs, ts)]
    s.close()
    return out


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("rate,first", CADENCES)
def test_trackers_equal_their_recorder_twins(c1, brick_mode, precision, rate, first):
    """240 steps in batches of 7, 93 and 140, all three quantities: the surface map and the station tracker equal the fold of
    their twins' samples bit for bit -- values, steps and the count of samples."""
    out = _c1_run(c1, precision, rate, first)
    for got, want in out:
        _same(got, want)
        assert got[2] == len(range(first, NSTEPS, rate))
        assert (got[0][:, :, 4] > 0).all() and (got[1] >= max(first, 1)).all()   # the wave reached every point, after first_step
    assert len(np.unique(out[0][0][1])) > 20


@pytest.fixture(scope="module")
def c1_oracle(c1):
    """The oracle's run, once: u at the head of every step at the surface nodes and at the stations' nodes -> the samples a
    recorder would take there (displacement, (u1 - u2) / dt, (u1 - 2 u2 + u3) / dt^2; the fields before step 0 are zero)."""
    box, dt = c1["box"], c1["dt"]
    N = box.info["nharbored"]
    o1, o2 = np.zeros((N, 3)), np.zeros((N, 3))
    caps = np.concatenate([c1["surface"], c1["ids"].reshape(-1)])
    cap = ho.solver_run(box.lnid, box.etable.copy(), box.ntable.copy(), o1, o2, 0, NSTEPS, dt,
                        loaded_lnid=c1["loaded"], forces=c1["F"], cap_lnid=caps)
    ns = len(c1["surface"])
    u = [cap[:, :ns], np.einsum("sn,tsnd->tsd", c1["phi"], cap[:, ns:].reshape(NSTEPS, len(c1["phi"]), 8, 3))]
    out = []
    for d in u:
        d1 = np.concatenate([np.zeros_like(d[:1]), d[:-1]])
        d2 = np.concatenate([np.zeros_like(d[:2]), d[:-2]])
        out.append(np.concatenate([d, (d - d1) / dt, (d - 2 * d1 + d2) / dt ** 2], axis=2))
    return out


def _rooted(peaks):
    p = peaks.copy()
    p[:, :, 3:] = np.sqrt(p[:, :, 3:])
    return p


@pytest.mark.parametrize("rate,first", CADENCES)
def test_trackers_match_the_oracle(c1, c1_oracle, brick_mode, rate, first):
    """The same run against the oracle (double): every column of `peaks` within 1e-9 of that column's maximum over the
    points, roots of the squared columns.  And, on the ORACLE's values, the case is worth the name: no surface point peaks at
    the first sample, at most 10 % at the last one, the horizontal-velocity peaks fall on at least 20 distinct steps."""
    steps = np.arange(first, NSTEPS, rate, dtype=np.int32)
    want = [host.peak_fold(steps, np.ascontiguousarray(smp[steps]), ALL) for smp in c1_oracle]
    when = want[0][1]
    assert (when >= 0).all()
    first_frac, last_frac = float((when == steps[0]).mean()), float((when == steps[-1]).mean())
    distinct = [len(np.unique(when[:, q, 0])) for q in range(3)]
    print("rate %d: %.1f%% peak at the first sample, %.1f%% at the last, distinct peak steps %r" % (rate, 100 * first_frac,
                                                                                                  100 * last_frac, distinct))
    assert not (when == steps[0]).any()
    assert (when == steps[-1]).mean(axis=0).max() <= 0.10
    assert distinct[1] >= 20
    for (got, _), (wp, ww), name in zip(_c1_run(c1, "f64", rate, first), want, ("surface", "stations")):
        g, w = _rooted(got[0]), _rooted(wp)
        for q in range(3):
            for j in range(5):
                err, scale = np.abs(g[:, q, j] - w[:, q, j]).max(), w[:, q, j].max()
                print("%s quantity %d column %d: err %.3e of %.3e" % (name, q, j, err, scale))
                assert scale > 0 and err <= TOL * scale, (name, q, j, err, scale)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the u(t - 2 dt) hazard
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big_box():
    """tests/test_gpu_recorders.py's big_box -- full 64 x 8 brick tiles -- with a seeded start field; 257 nodes (two
    workgroups) spread over the brick interior, both z faces and the x / y shell."""
    nx, ny, nz, h, dt = 64, 64, 32, 15.0, 3e-4
    box = host.Box(nx, ny, nz, h, dt, 30.0)
    L = np.array([nx * h, ny * h, nz * h])
    loaded, pattern = box.point_source(L[0] / 2, L[1] / 2, L[2] / 2, 30.0, 70.0, 10.0)
    rp = box.run_params(loaded=loaded, pattern=pattern, moment=1e13, rise_time=20 * dt, source_window=64)
    F = box.source_table(rp, 0, 24)
    u = _field(box, 77)
    ijk = box.node_ijk
    shell = (ijk[:, 0] == 0) | (ijk[:, 0] == nx) | (ijk[:, 1] == 0) | (ijk[:, 1] == ny)
    classes = [np.nonzero(~shell & (ijk[:, 2] == 0))[0], np.nonzero(~shell & (ijk[:, 2] == nz))[0], np.nonzero(shell)[0],
               np.nonzero(~shell & (ijk[:, 2] > 0) & (ijk[:, 2] < nz))[0]]
    rng = np.random.default_rng(20261018)
    nodes = np.concatenate([rng.choice(c, n, replace=False) for c, n in zip(classes, (48, 48, 64, 97))]).astype(np.int32)
    assert len(nodes) == 257 and len(np.unique(nodes)) == 257
    yield dict(box=box, nodes=nodes, loaded=loaded, F=F, u1=u, u2=0.999 * u, dt=dt)
    box.close()


@pytest.mark.parametrize("quantities", [ALL, V])
@pytest.mark.parametrize("brick_stream", [1, 0])
def test_samples_are_folded_before_the_bricks_overwrite_the_oldest_field(big_box, brick_mode, brick_stream, quantities):
    """d_u[spare] is u(t - 2 dt) AND the buffer the step's kernels write u(t + dt) into: with the bricks on a stream of their
    own nothing but the tracker's event orders an acceleration tracker's launch ahead of them (the twin's event is recorded
    BEFORE hq_k_peak is enqueued, so it does not cover it).  24 steps enqueued by ONE hq_run, with accelerations and once more
    with velocities only, which hold nothing back: equal to the twin."""
    b = big_box
    s = b["box"].create_solver(tm1=b["u1"], tm2=b["u2"], options={"brick_stream": brick_stream})
    s.set_source(b["loaded"], b["F"])
    h = s.peak_add(b["nodes"], None, rate=1, quantities=quantities)
    t = _add_twin(s, b["nodes"], None, 1, 24)
    s.run(24)
    got = s.peak_fetch(h)
    want = _fold_twin(s, t, quantities)
    info = s.info()
    s.close()
    if brick_mode == "bricks":
        assert info["brick_units"] > 0 and info["brick_stream"] == brick_stream
    else:
        assert info["brick_units"] == 0
    assert got[2] == 24 and got[0].shape == (257, 3 if quantities == ALL else 1, 5)
    assert (got[0][:, -1] > 0).all() and len(np.unique(got[1])) > 3
    _same(got, want)


# ---------------------------------------------------------------------------------------------------------------------
# 4. two partitions in one process
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("overlap", [0, 1])
def test_two_partitions_track_through_group_run(brick_mode, overlap):
    """Two partitions of a 32 x 32 x 16 box in one process (hq_group_link), 30 steps in one hq_group_run (overlap = 1: the
    exchange chain on a stream of its own, which an acceleration tracker's due step holds back).  Each rank tracks all the
    nodes it shares with the other and some of its own (K = 1) and stations around the cut (K = 8): equal to the twins, and
    a shared node's displacement peaks are the same on both ranks -- its displacement is, bit for bit."""
    nx, ny, nz, h, dt = 32, 32, 16, 15.0, 3e-4
    boxes = [host.Box(nx, ny, nz, h, dt, 30.0, rank=r, nranks=2) for r in range(2)]
    L = np.array([nx * h, ny * h, nz * h])
    pts = np.random.default_rng(5).uniform(0.0, 1.0, (24, 3)) * L
    nodes, stations, gids = [], [], []
    for bx in boxes:
        sch = bx.schedule()
        sh = np.unique(np.concatenate([m for _, m in sch["c"] + sch["s"]])).astype(np.int32)
        assert len(sh) > 0
        ijk = bx.node_ijk[sh].astype(np.int64)
        gids.append((ijk[:, 2] * (ny + 1) + ijk[:, 1]) * (nx + 1) + ijk[:, 0])
        own = np.setdiff1d(np.arange(bx.info["nharbored"], dtype=np.int32), sh)[::37]
        nodes.append(np.concatenate([sh, own]).astype(np.int32))
        ids, phi, mine = bx.stations(pts)
        stations.append((ids[mine != 0], phi[mine != 0]))
    assert sorted(gids[0]) == sorted(gids[1])
    assert len(stations[0][0]) + len(stations[1][0]) == len(pts) and min(len(st[0]) for st in stations) > 0
    fields = [_field(bx, 31) for bx in boxes]
    solvers = [bx.create_solver(tm1=u, tm2=0.999 * u, options={"overlap": overlap}) for bx, u in zip(boxes, fields)]
    capi.group_link(solvers)
    hn = [s.peak_add(n, None, rate=1, quantities=ALL) for s, n in zip(solvers, nodes)]
    hs = [s.peak_add(ids, phi, rate=2, quantities=D | A) for s, (ids, phi) in zip(solvers, stations)]
    tn = [_add_twin(s, n, None, 1, 30) for s, n in zip(solvers, nodes)]
    ts = [_add_twin(s, ids, phi, 2, 15) for s, (ids, phi) in zip(solvers, stations)]
    capi.group_run(solvers, 30)
    got_n = [s.peak_fetch(h) for s, h in zip(solvers, hn)]
    got_s = [s.peak_fetch(h) for s, h in zip(solvers, hs)]
    want_n = [_fold_twin(s, t, ALL) for s, t in zip(solvers, tn)]
    want_s = [_fold_twin(s, t, D | A) for s, t in zip(solvers, ts)]
    for s in solvers:
        s.close()
    for bx in boxes:
        bx.close()
    for r in range(2):
        assert got_n[r][2] == 30 and got_s[r][2] == 15 and got_s[r][0].shape[1] == 2
        assert (got_n[r][0][:, 0, 4] > 0).all()
        _same(got_n[r], want_n[r])
        _same(got_s[r], want_s[r])
    a, b = np.argsort(gids[0]), np.argsort(gids[1])          # the shared nodes lead each rank's list: pair them by position
    assert np.array_equal(got_n[0][0][a, 0], got_n[1][0][b, 0]) and np.array_equal(got_n[0][1][a, 0], got_n[1][1][b, 0])


# ---------------------------------------------------------------------------------------------------------------------
# 5. semantics on C1
# ---------------------------------------------------------------------------------------------------------------------

def test_an_empty_tracker_is_accepted(c1):
    s = _c1_solver(c1)
    h1 = s.peak_add(np.zeros(0, np.int32), None, rate=2, quantities=V)
    h8 = s.peak_add(np.zeros((0, 8), np.int32), np.zeros((0, 8)), rate=1, first_step=3, quantities=ALL)
    s.run(10)
    p, w, n = s.peak_fetch(h1)
    assert p.shape == (0, 1, 5) and w.shape == (0, 1, 2) and n == 5
    assert s.peak_fetch(h8)[2] == 7
    s.peak_reset(h1)
    assert s.peak_fetch(h1)[2] == 0
    s.close()


def test_reset_and_load_resume_a_run(c1, brick_mode):
    """Fetch at step 100, reset (zeros, -1, no samples), load what was fetched, run on: the uninterrupted twin's fold."""
    s = _c1_solver(c1)
    h = s.peak_add(c1["surface"], None, rate=1, quantities=ALL)
    t = _add_twin(s, c1["surface"], None, 1, NSTEPS)
    s.run(7)
    s.run(93)
    saved = s.peak_fetch(h)
    assert saved[2] == 100 and (saved[0] > 0).any()
    again = s.peak_fetch(h)                                  # a fetch leaves the state in place
    _same(again, saved)
    s.peak_reset(h)
    p, w, n = s.peak_fetch(h)
    assert n == 0 and (p == 0).all() and (w == -1).all() and p.shape == saved[0].shape
    s.run(5)                                                 # ... and tracks on from there: nothing of the first 100 steps
    p, w, n = s.peak_fetch(h)
    assert n == 5 and w.max() >= 100 and ((w == -1) | (w >= 100)).all()
    s.peak_load(h, *saved)
    _same(s.peak_fetch(h), saved)
    s.run(135)
    got = s.peak_fetch(h)
    steps, vals = s.record_fetch(t)
    s.close()
    keep = (steps < 100) | (steps >= 105)                    # the five steps between reset and load were folded into a state
    want = host.peak_fold(steps[keep], np.ascontiguousarray(vals[keep]), ALL)      # that the load replaced
    _same(got, (want[0], want[1], 235))


def test_upload_keeps_the_state_and_moves_the_due_steps(c1, brick_mode):
    s = _c1_solver(c1)
    h = s.peak_add(c1["ids"], c1["phi"], rate=2, quantities=D | V)
    t = _add_twin(s, c1["ids"], c1["phi"], 2, 32, derivs=1)
    s.run(41)                                                # samples of steps 0, 2, ..., 40
    before = s.peak_fetch(h)
    tm1, tm2 = s.download()
    s.upload(tm1 * 1000.0, tm2 * 1000.0, 250)
    _same(s.peak_fetch(h), before)
    _same(before, _fold_twin(s, t, D | V))
    s.run(3)                                                 # ... and of 250 and 252
    got = s.peak_fetch(h)
    steps, vals = s.record_fetch(t)
    s.close()
    assert before[2] == 21 and got[2] == 23 and np.array_equal(steps, [250, 252])
    want = host.peak_fold(steps, vals, D | V, before[0].copy(), before[1].copy())
    _same(got, (want[0], want[1], 23))
    assert (got[1] >= 250).any()                             # the scaled field raised peaks


def test_bad_descriptions_and_cleared_handles(c1):
    ids, phi, surface = c1["ids"], c1["phi"], c1["surface"]
    sc = _c1_solver(c1, variant=ha.HQ_VARIANT_SCATTER)
    for q in (A, ALL, V | A):
        with pytest.raises(ha.HqError, match="patch variant"):         # HQ_ERR_STATE, as hq_gather3
            sc.peak_add(surface, None, quantities=q)
    h = sc.peak_add(surface, None, rate=1, quantities=D | V)             # ... velocities it has
    t = _add_twin(sc, surface, None, 1, 60, derivs=1)
    sc.run(60)
    got, want = sc.peak_fetch(h), _fold_twin(sc, t, D | V)
    sc.close()
    assert (got[0] > 0).any()
    _same(got, want)

    s = _c1_solver(c1)
    bad8, bad1 = ids.copy(), surface.copy()
    bad8[3, 5] = s.N
    bad1[-1] = s.N
    for kw in (dict(ids=bad8, phi=phi), dict(ids=bad1, phi=None), dict(ids=-1 - surface, phi=None),
               dict(ids=ids, phi=phi, rate=0), dict(ids=ids, phi=phi, rate=-2), dict(ids=ids, phi=phi, quantities=0),
               dict(ids=ids, phi=phi, quantities=8), dict(ids=ids, phi=phi, quantities=ALL | 16)):
        with pytest.raises(ha.HqError):
            s.peak_add(kw.pop("ids"), kw.pop("phi"), **kw)
    lib = s._lib
    hh = ctypes.c_int32(-1)
    for npts, k, i, p in ((-1, 8, ids, phi), (5, 4, ids, phi), (5, 0, ids, phi), (5, 8, None, phi), (5, 8, ids, None), (5, 1, None, None)):
        d = capi._PeakDesc(npts, k, None if i is None else i.ctypes.data, None if p is None else p.ctypes.data, 1, 0, V, 0)
        assert lib.hq_peak_add(s._h, ctypes.byref(d), ctypes.byref(hh)) == -1
    ok = capi._PeakDesc(5, 8, ids.ctypes.data, phi.ctypes.data, 1, 0, V, 0)
    assert lib.hq_peak_add(s._h, ctypes.byref(ok), None) == -1 and lib.hq_peak_add(s._h, None, ctypes.byref(hh)) == -1
    pk, wh, n = np.zeros(25), np.zeros(10, np.int32), ctypes.c_int64()
    for handle in (0, 7, -1):                                # nothing was added
        assert lib.hq_peak_fetch(s._h, handle, capi._ptr(pk), capi._ptr(wh), ctypes.byref(n)) == -1
        assert lib.hq_peak_load(s._h, handle, capi._ptr(pk), capi._ptr(wh), ctypes.c_int64(0)) == -1
        assert lib.hq_peak_reset(s._h, handle) == -1
    bytes0 = s.info()["device_bytes"]
    h = s.peak_add(ids, phi, rate=1, quantities=V)
    assert lib.hq_peak_fetch(s._h, h, None, capi._ptr(wh), ctypes.byref(n)) == -1
    assert lib.hq_peak_fetch(s._h, h, capi._ptr(pk), capi._ptr(wh), None) == -1
    assert lib.hq_peak_load(s._h, h, capi._ptr(pk), None, ctypes.c_int64(0)) == -1
    h1 = s.peak_add(surface, None, rate=1, quantities=ALL)
    assert h1 != h
    assert s.info()["device_bytes"] >= bytes0 + 5 * (8 * 12 + 48) + 289 * (4 + 3 * 48)
    s.run(2)
    s.record_clear()                                         # trackers are neither recorders ...
    s.snapshot_clear()                                       # ... nor snapshots
    assert s.peak_fetch(h)[2] == 2 and s.peak_fetch(h1)[2] == 2
    s.peak_clear()
    assert s.info()["device_bytes"] == bytes0
    for dead in (h, h1):
        assert lib.hq_peak_fetch(s._h, dead, capi._ptr(pk), capi._ptr(wh), ctypes.byref(n)) == -1
        assert lib.hq_peak_reset(s._h, dead) == -1
    s.run(10)                                                # tracks nothing
    s.peak_clear()                                           # nothing to drop: no error
    h2 = s.peak_add(ids, phi, rate=1, quantities=V)
    assert h2 not in (h, h1) and s.peak_fetch(h2)[2] == 0   # handles are not reused
    s.close()


@pytest.mark.parametrize("runner", ["sync", "async"])
def test_a_tracker_survives_the_runners(c1, runner):
    """hqh_solver_run_on with device_recorders = 1 and hqh_solver_run_async drop their own recorders and snapshots and leave a
    caller's tracker alone: 60 steps in two calls, stations every 2 steps with accelerations; the tracker on the same stations
    at the same rate equals a fold of the samples the station callback was handed (hq_k_record's, on the same trajectory)."""
    box = c1["box"]
    loaded, pattern = box.point_source(500.0, 500.0, 100.0, 0.0, 90.0, 0.0)
    calls = []
    rp = box.run_params(loaded=loaded, pattern=pattern, moment=1e15, rise_time=0.02, source_window=16, device_recorders=1,
                        station_ids=c1["ids"], station_phi=c1["phi"], station_rate=2, station_derivs=2,
                        station_fn=lambda step, vals: calls.append((step, vals)))
    s = box.create_solver()
    h = s.peak_add(c1["ids"], c1["phi"], rate=2, quantities=ALL)
    for step0, n in ((0, 23), (23, 37)):
        if runner == "sync":
            box.solver_run(s, rp, step0, n)
        else:
            box.solver_run_async(s, rp, step0, n, slots=1)
    got = s.peak_fetch(h)
    with pytest.raises(ha.HqError):
        s.record_pending(0)                                  # the runner left no recorder behind
    s.close()
    steps = np.array([c[0] for c in calls], np.int32)
    assert np.array_equal(steps, np.arange(0, 60, 2))
    want = host.peak_fold(steps, np.array([c[1] for c in calls]), ALL)
    assert (want[0][:, :, 4] > 0).all()
    _same(got, (want[0], want[1], 30))


# ---------------------------------------------------------------------------------------------------------------------
# 6. no traffic between fetches
# ---------------------------------------------------------------------------------------------------------------------

def test_nothing_crosses_pcie_until_a_fetch(c1):
    s = _c1_solver(c1)
    h1 = s.peak_add(c1["surface"], None, rate=1, quantities=V)
    h8 = s.peak_add(c1["ids"], c1["phi"], rate=3, quantities=ALL)
    s.sync()
    before = s.info()
    s.run(100)
    s.sync()
    after = s.info()
    assert after["pcie_d2h_bytes"] == before["pcie_d2h_bytes"] and after["pcie_h2d_bytes"] == before["pcie_h2d_bytes"]
    s.peak_fetch(h1)
    mid = s.info()
    assert mid["pcie_d2h_bytes"] - after["pcie_d2h_bytes"] == 48 * 289 * 1 and mid["pcie_h2d_bytes"] == after["pcie_h2d_bytes"]
    s.peak_fetch(h8)
    assert s.info()["pcie_d2h_bytes"] - mid["pcie_d2h_bytes"] == 48 * 5 * 3
    s.close()
