"""Cumulative-intensity trackers (hq_cum_add / _fetch / _load / _reset / _clear, include/hq_solver.h): the running sums, the
threshold spans and the Husid curve hq_k_cum keeps per point on the device, against the project's own pinned chain.

A tracker's sample is hq_k_record's sample bit for bit, and its fold is csrc/hq_cumul.h, the text hqh_cum_fold compiles for the
host.  So every tracker here gets a RECORDER TWIN on the same context -- the same points, the same rate, derivs = 2, room for
the whole run; for a tracker of single nodes the twin's points are the node repeated 8 times with weights (1, 0, ..., 0) --
and the expectation is np.array_equal between hq_cum_fetch and hqh_cum_fold(hq_record_fetch), for the sums, the span and
nsamples, and between Husid slot k and the twin's fold cut off behind that slot's step.  The comparison has to be made on ONE
trajectory: two identically built solvers differ in the last bits (tests/test_gpu_recorders.py tells why).  A recorder knows
no first_step: samples of earlier steps are dropped before the fold.

The fixture is the C1 box of tests/test_gpu_peaks.py, built here: 16 x 16 x 8, h = 62.5, dt = 1e-3, from rest, a sin^2 push
on one node for 40 steps; 240 steps in batches of 7, 93 and 140; the 289 nodes of the z = 0 face with K = 1 (two workgroups,
the second one ragged) and the five C1 stations with K = 8."""
import ctypes

import numpy as np
import pytest

import hercules_amd as ha
from hercules_amd import capi, host
from oracle import herc_oracle as ho
from tests import helpers as H

pytestmark = pytest.mark.gpu

TOL = 1e-9
D, V, A = capi.HQ_PEAK_DISP, capi.HQ_PEAK_VEL, capi.HQ_PEAK_ACC
ALL = D | V | A
NSTEPS = 240
BATCHES = (7, 93, 140)
CADENCES = [(1, 0), (3, 6)]
HUSID_EVERY, HUSID_SLOTS = 7, 20                             # 7 divides no batch boundary; 240 samples would fill 34 slots


@pytest.fixture(params=["bricks", "patches-only"])
def brick_mode(request, monkeypatch):
    """As shipped (hq_k_brick takes the simple nodes of uniform regions) and with HQ_NO_BRICKS=1 (patches everywhere)."""
    if request.param == "patches-only":
        monkeypatch.setenv("HQ_NO_BRICKS", "1")
    else:
        monkeypatch.delenv("HQ_NO_BRICKS", raising=False)
    return request.param


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
    yield dict(box=box, loaded=loaded, F=F, surface=surface, ids=ids, phi=phi, dt=1e-3, thr={})
    box.close()


def _solver(c1, precision="f64", variant=ha.HQ_VARIANT_AUTO):
    s = c1["box"].create_solver(precision=precision, variant=variant)
    s.set_source(c1["loaded"], c1["F"])
    return s


def _add_twin(s, ids, phi, rate, capacity, derivs=2):
    if phi is None:                                          # a node as a point: itself 8 times, weights (1, 0, ..., 0)
        flat = np.asarray(ids, np.int32).reshape(-1)
        ids = np.repeat(flat[:, None], 8, axis=1)
        phi = np.zeros((len(flat), 8))
        phi[:, 0] = 1.0
    return s.record_add(ids, phi, rate=rate, derivs=derivs, capacity=capacity)


def _derivs(q):
    return 2 if q & A else 1 if q & V else 0


def _thr_of(thr3, q):
    return [thr3[b] for b in range(3) if q & (1 << b)]


def _thresholds(c1, precision):
    """Per quantity, half the largest total (root of x x + y y + z z) over the surface nodes, the stations and the whole run,
    taken from the samples of recorder twins of a run of this very case (once per precision): some points pass it, some
    never do.  A threshold is a description of the tracker and has to exist before the run it is used in."""
    if precision not in c1["thr"]:
        s = _solver(c1, precision)
        ts = [_add_twin(s, c1["surface"], None, 1, NSTEPS), _add_twin(s, c1["ids"], c1["phi"], 1, NSTEPS)]
        for n in BATCHES:
            s.run(n)
        vals = np.concatenate([s.record_fetch(t)[1] for t in ts], axis=1)
        s.close()
        c1["thr"][precision] = [0.5 * float(np.sqrt((vals[:, :, 3 * b:3 * b + 3] ** 2).sum(axis=2).max())) for b in range(3)]
        assert all(t > 0 for t in c1["thr"][precision])
    return c1["thr"][precision]


def _due(rate, first, upto=NSTEPS):
    return np.array([s for s in range(upto) if s >= first and s % rate == 0], np.int32)


def _fold_twin(samples, q, thr3, first_step=0, last_step=None, into=None):
    """hqh_cum_fold of a twin's (steps, samples [k, np, 9]) from first_step to last_step -> (sums, span, samples folded)."""
    steps, vals = samples
    keep = steps >= first_step
    if last_step is not None:
        keep &= steps <= last_step
    v = np.ascontiguousarray(vals[keep][:, :, :3 * (1 + _derivs(q))])    # (the columns up to derivs(q), as peak_fold's)
    sums, span = host.cum_fold(steps[keep], v, q, _thr_of(thr3, q), *(into or (None, None)))
    return sums, span, int(keep.sum())


def _same(got, want):
    """(sums, span, nsamples) of a fetch (its curve left out) and of a twin's fold."""
    assert got[2] == want[2], (got[2], want[2])
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape
    assert np.array_equal(got[1], want[1]), np.argwhere(got[1] != want[1])[:5]
    assert np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:5]


def _state(f):
    """cum_fetch's (sums, span, curve, curve_steps, nsamples) -> what _same compares."""
    return f[0], f[1], f[4]


# ---------------------------------------------------------------------------------------------------------------------
# 1 - 3. the C1 box from rest: against the twins, the Husid curve, against the oracle
# ---------------------------------------------------------------------------------------------------------------------

def _c1_run(c1, precision, rate, first):
    """One run -> thresholds, and per point set ("surface" K = 1, "stations" K = 8): the fetches of an ALL tracker with a Husid
    curve and of a velocity-only tracker without one, and the twin's samples."""
    thr3 = _thresholds(c1, precision)
    s = _solver(c1, precision)
    cap = NSTEPS // rate + 1
    sets = [("surface", c1["surface"], None), ("stations", c1["ids"], c1["phi"])]
    hs = []
    for _, ids, phi in sets:
        hs.append((s.cum_add(ids, phi, rate=rate, first_step=first, quantities=ALL, threshold=thr3,
                             husid_every=HUSID_EVERY, husid_slots=HUSID_SLOTS),
                   s.cum_add(ids, phi, rate=rate, first_step=first, quantities=V, threshold=thr3[1]),
                   _add_twin(s, ids, phi, rate, cap)))
    for n in BATCHES:
        s.run(n)
    assert s.info()["step"] == NSTEPS
    out = {name: dict(all=s.cum_fetch(ha_), vel=s.cum_fetch(hv), twin=s.record_fetch(t)) for (name, _, _), (ha_, hv, t) in zip(sets, hs)}
    s.close()
    return thr3, out


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("rate,first", CADENCES)
def test_trackers_equal_their_recorder_twins(c1, brick_mode, precision, rate, first):
    """240 steps in batches of 7, 93 and 140; masks ALL and VEL alone: the surface map and the station tracker equal the fold
    of their twins' samples bit for bit -- sums, span and the count of samples.  The threshold, half the largest total of the
    twins' samples, is passed by some points and never by others."""
    thr3, out = _c1_run(c1, precision, rate, first)
    ndue = len(_due(rate, first))
    for name, o in out.items():
        _same(_state(o["all"]), _fold_twin(o["twin"], ALL, thr3, first))
        _same(_state(o["vel"]), _fold_twin(o["twin"], V, thr3, first))
        assert o["all"][4] == ndue and o["vel"][4] == ndue
        assert o["vel"][2].shape[0] == 0 and len(o["vel"][3]) == 0          # no curve was asked for
        assert (o["all"][0][:, :, 3:].sum(axis=2) > 0).all()                # the wave reached every point
    span = out["surface"]["all"][1]
    for q in range(3):                                       # both kinds of point occur, for every quantity
        assert (span[:, q, 2] > 0).any() and (span[:, q, 2] == 0).any(), q
        never = span[:, q, 2] == 0
        assert (span[never, q, :2] == -1).all() and (span[~never, q, 0] >= max(first, 1)).all()
        assert (span[~never, q, 1] >= span[~never, q, 0]).all()


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("rate,first", CADENCES)
def test_husid_slots_are_the_twin_cut_off_at_their_steps(c1, brick_mode, precision, rate, first):
    """husid_every = 7 divides no batch boundary, husid_slots = 20 is fewer than the 34 slots the 240 samples of rate 1 would
    fill: nfilled == 20 there (at rate 3 from step 6 there are 78 samples: the 11 slots they fill); curve_steps are the steps
    of samples 7, 14, ... counted from the first due one; slot k equals the twin's fold cut off behind that step, bit for bit;
    and the sums themselves keep growing past the last slot."""
    thr3, out = _c1_run(c1, precision, rate, first)
    due = _due(rate, first)
    nfilled = min(len(due) // HUSID_EVERY, HUSID_SLOTS)
    if rate == 1:
        assert nfilled == HUSID_SLOTS == 20
    for name, o in out.items():
        sums, span, curve, csteps, n = o["all"]
        assert n == len(due) and curve.shape == (nfilled,) + sums.shape[:2] + (3,)
        assert np.array_equal(csteps, due[HUSID_EVERY - 1::HUSID_EVERY][:nfilled])
        for k in range(nfilled):
            want = _fold_twin(o["twin"], ALL, thr3, first, last_step=int(csteps[k]))
            assert want[2] == HUSID_EVERY * (k + 1)
            assert np.array_equal(curve[k], want[0][:, :, 3:]), (name, k)
        assert (sums[:, :, 3:] >= curve[-1]).all()
        if rate == 1:
            assert (sums[:, :, 3:] > curve[-1]).any()


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
    out = {}
    for name, d in zip(("surface", "stations"), u):
        d1 = np.concatenate([np.zeros_like(d[:1]), d[:-1]])
        d2 = np.concatenate([np.zeros_like(d[:2]), d[:-2]])
        out[name] = np.concatenate([d, (d - d1) / dt, (d - 2 * d1 + d2) / dt ** 2], axis=2)
    return out


@pytest.mark.parametrize("rate,first", CADENCES)
def test_sums_match_the_oracle(c1, c1_oracle, brick_mode, rate, first):
    """The same run against the oracle (double): sum |v| and sum v v formed in numpy from the oracle's captured fields; every
    column of `sums` within 1e-9 of that column's maximum over the points.  `span` is the twin's business alone: a threshold
    tie is a matter of the last bit.
    Measured on an MI355X: the worst column over both cadences, both brick modes and both point sets is 2.3e-13 of its
    maximum (the stations' sum of squared x displacements, with bricks, at either cadence); without bricks 8.3e-14."""
    _, out = _c1_run(c1, "f64", rate, first)
    due = _due(rate, first)
    worst = 0.0
    for name, smp in c1_oracle.items():
        v = smp[due].reshape(len(due), smp.shape[1], 3, 3)                 # [sample, point, quantity, axis]
        want = np.concatenate([np.abs(v).sum(axis=0), (v * v).sum(axis=0)], axis=2)
        got = out[name]["all"][0]
        assert got.shape == want.shape
        for q in range(3):
            for j in range(6):
                err, scale = np.abs(got[:, q, j] - want[:, q, j]).max(), want[:, q, j].max()
                print("%s quantity %d column %d: err %.3e of %.3e = %.3e" % (name, q, j, err, scale, err / scale))
                worst = max(worst, err / scale)
                assert scale > 0 and err <= TOL * scale, (name, q, j, err, scale)
    print("worst relative error of a column: %.3e" % worst)


# ---------------------------------------------------------------------------------------------------------------------
# 4. life cycle
# ---------------------------------------------------------------------------------------------------------------------

def _same_fetch(a, b):
    _same(_state(a), _state(b))
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def test_reset_clear_and_load_resume_a_run(c1, brick_mode):
    """Fetch at step 100 -> reset: zeros / -1 / no samples / no slots.  Then fetch, clear, a NEW tracker, load, run on: the
    uninterrupted twin's fold, bit for bit, the curve and curve_steps included."""
    thr3 = _thresholds(c1, "f64")
    kw = dict(rate=1, quantities=ALL, threshold=thr3, husid_every=HUSID_EVERY, husid_slots=HUSID_SLOTS)
    s = _solver(c1)
    h = s.cum_add(c1["surface"], None, **kw)
    t = _add_twin(s, c1["surface"], None, 1, NSTEPS)
    s.run(7)
    s.run(93)
    saved = s.cum_fetch(h)
    assert saved[4] == 100 and (saved[0] > 0).any() and len(saved[3]) == 14
    _same_fetch(s.cum_fetch(h), saved)                       # a fetch leaves the state in place
    s.cum_reset(h)
    sums, span, curve, csteps, n = s.cum_fetch(h)
    assert n == 0 and (sums == 0).all() and (span[:, :, :2] == -1).all() and (span[:, :, 2] == 0).all()
    assert sums.shape == saved[0].shape and len(csteps) == 0 and curve.shape[0] == 0
    s.run(5)                                                 # ... and folds on from there: nothing of the first 100 steps
    sums, span, curve, csteps, n = s.cum_fetch(h)
    assert n == 5 and len(csteps) == 0 and ((span[:, :, 0] == -1) | (span[:, :, 0] >= 100)).all()
    s.cum_clear()
    with pytest.raises(ha.HqError):
        s.cum_fetch(h)
    h2 = s.cum_add(c1["surface"], None, **kw)
    assert h2 != h                                           # handles are not reused
    s.cum_load(h2, *saved)
    _same_fetch(s.cum_fetch(h2), saved)
    s.run(135)
    got = s.cum_fetch(h2)
    twin = s.record_fetch(t)
    s.close()
    steps, vals = twin
    keep = (steps < 100) | (steps >= 105)                    # the five steps between reset and load went into a state
    kept = (steps[keep], vals[keep])                         # that the clear dropped
    _same(_state(got), _fold_twin(kept, ALL, thr3))
    assert got[4] == 235 and len(got[3]) == HUSID_SLOTS
    assert np.array_equal(got[3], steps[keep][HUSID_EVERY - 1::HUSID_EVERY][:HUSID_SLOTS])
    for k in (0, 13, 14, 19):                                # slots from before the load, and from behind it
        want = _fold_twin(kept, ALL, thr3, last_step=int(got[3][k]))
        assert np.array_equal(got[2][k], want[0][:, :, 3:]), k
    # a load whose nfilled does not fit its nsamples is refused
    s2 = _solver(c1)
    h3 = s2.cum_add(c1["surface"], None, **kw)
    with pytest.raises(ha.HqError):
        s2.cum_load(h3, saved[0], saved[1], saved[2][:3], saved[3][:3], saved[4])
    s2.close()


def test_upload_keeps_the_state_and_moves_the_due_steps(c1, brick_mode):
    thr3 = _thresholds(c1, "f64")
    s = _solver(c1)
    h = s.cum_add(c1["ids"], c1["phi"], rate=2, quantities=ALL, threshold=thr3, husid_every=4, husid_slots=8)
    t = _add_twin(s, c1["ids"], c1["phi"], 2, 32)
    s.run(41)                                                # samples of steps 0, 2, ..., 40
    before = s.cum_fetch(h)
    twin0 = s.record_fetch(t)
    tm1, tm2 = s.download()
    s.upload(tm1 * 1000.0, tm2 * 1000.0, 250)
    _same_fetch(s.cum_fetch(h), before)
    _same(_state(before), _fold_twin(twin0, ALL, thr3))
    s.run(7)                                                 # ... and of 250, 252, 254, 256
    got = s.cum_fetch(h)
    twin1 = s.record_fetch(t)
    s.close()
    assert before[4] == 21 and got[4] == 25 and np.array_equal(twin1[0], [250, 252, 254, 256])
    assert np.array_equal(before[3], [6, 14, 22, 30, 38]) and np.array_equal(got[3], [6, 14, 22, 30, 38, 254])
    want = _fold_twin(twin1, ALL, thr3, into=(before[0].copy(), before[1].copy()))
    _same(_state(got), (want[0], want[1], 25))
    assert (got[1][:, :, 1] >= 250).any()                    # the scaled field passed the threshold


def test_an_empty_tracker_is_accepted(c1):
    s = _solver(c1)
    h1 = s.cum_add(np.zeros(0, np.int32), None, rate=2, quantities=V, husid_every=2, husid_slots=3)
    h8 = s.cum_add(np.zeros((0, 8), np.int32), np.zeros((0, 8)), rate=1, first_step=3, quantities=ALL, threshold=[1.0, 2.0, 3.0])
    s.run(10)
    sums, span, curve, csteps, n = s.cum_fetch(h1)
    assert sums.shape == (0, 1, 6) and span.shape == (0, 1, 3) and curve.shape == (2, 0, 1, 3) and n == 5
    assert np.array_equal(csteps, [2, 6])
    assert s.cum_fetch(h8)[4] == 7
    s.cum_reset(h1)
    assert s.cum_fetch(h1)[4] == 0 and len(s.cum_fetch(h1)[3]) == 0
    s.close()


def test_other_clears_leave_the_tracker_and_the_bytes_are_accounted(c1):
    """hq_record_clear, hq_snapshot_clear, hq_peak_clear and hq_spec_clear leave a cumulative tracker alive; device_bytes rises
    by the documented amount -- 12 K np of tables (4 np for K = 1) + np nq (60 + 24 husid_slots) -- and falls back after
    hq_cum_clear; pcie_d2h_bytes rises by exactly the fetched bytes, and nothing crosses PCIe between fetches."""
    s = _solver(c1)
    bytes0 = s.info()["device_bytes"]
    h1 = s.cum_add(c1["surface"], None, rate=1, quantities=A, husid_every=HUSID_EVERY, husid_slots=HUSID_SLOTS)
    bytes1 = s.info()["device_bytes"]
    assert bytes1 - bytes0 == 289 * 4 + 289 * 1 * (60 + 24 * HUSID_SLOTS)
    h8 = s.cum_add(c1["ids"], c1["phi"], rate=3, quantities=ALL)
    assert s.info()["device_bytes"] - bytes1 == 5 * 96 + 5 * 3 * 60 + 8       # (an absent curve still has an address: 8 bytes)
    s.record_add(c1["ids"], c1["phi"], rate=1, derivs=2, capacity=16)
    s.peak_add(c1["surface"], None, rate=1, quantities=V)
    s.spec_add(c1["surface"], None, rate=1, periods=(0.5,))
    s.run(10)
    s.record_clear()
    s.snapshot_clear()
    s.peak_clear()
    s.spec_clear()
    s.sync()
    before = s.info()
    s.run(90)
    s.sync()
    after = s.info()
    assert after["pcie_d2h_bytes"] == before["pcie_d2h_bytes"] and after["pcie_h2d_bytes"] == before["pcie_h2d_bytes"]
    f1 = s.cum_fetch(h1)
    mid = s.info()
    assert f1[4] == 100 and len(f1[3]) == 14
    assert mid["pcie_d2h_bytes"] - after["pcie_d2h_bytes"] == 289 * (60 + 24 * 14) and mid["pcie_h2d_bytes"] == after["pcie_h2d_bytes"]
    s.cum_fetch(h1, curve=False)
    assert s.info()["pcie_d2h_bytes"] - mid["pcie_d2h_bytes"] == 289 * 60
    mid = s.info()
    assert s.cum_fetch(h8)[4] == 34
    assert s.info()["pcie_d2h_bytes"] - mid["pcie_d2h_bytes"] == 5 * 3 * 60
    s.cum_clear()
    assert s.info()["device_bytes"] == bytes0
    s.run(5)                                                 # folds nothing
    s.cum_clear()                                            # nothing to drop: no error
    s.close()


def test_the_three_kinds_share_one_context_and_one_state_path(c1):
    """One tracker of each kind on the stations (K = 8) and one on the surface (K = 1), in one context.  Handles count per
    kind from 0; a clear of one kind leaves the others' state bit for bit, does not hand a handle out again, and a cleared
    handle is refused by name.  The six states fetched at step 12 are loaded into two contexts with the same uploaded fields
    and step -- this one, and a fresh one with the same six trackers -- and on each a fetch returns what was loaded, bit for
    bit.  Each context then gets recorder twins and runs 12 more steps: on its own trajectory every tracker equals the
    loaded state with the twin's 12 samples folded into it (host.peak_fold, spec_fold, cum_fold), bit for bit, the third
    Husid slot and curve_steps included.

    Last, as the issue sets it, the two contexts' fetches are compared with np.array_equal.  That compares two
    trajectories, which the patch kernels' fp64 LDS atomics do not step alike (tests/test_gpu_recorders.py): on an MI355X
    it held in 1 of 5 runs; in the others the surface trackers differed in the last bits at the wave front (peaks in 12 of
    4 335 values by up to 1.4e-34 at a scale of 1.5e-3, sums in 11 of 5 202 by up to 1.9e-34 at 4.8e-3, sd 6 of 2 312, osc 13
    of 3 468, aprev 2 of 867), as the fields of two contexts without any tracker do (88 of 7 803 values, up to 1.0e-25 at
    1.2e-4); the station trackers, `when`, the spans, the curves, curve_steps and nsamples were equal."""
    kinds = ("peak", "spec", "cum")
    sets = [(c1["ids"], c1["phi"]), (c1["surface"], None)]
    add = dict(peak=lambda s, i, p: s.peak_add(i, p, rate=1, quantities=ALL),
               spec=lambda s, i, p: s.spec_add(i, p, rate=1, periods=(0.05, 0.2)),
               cum=lambda s, i, p: s.cum_add(i, p, rate=1, quantities=ALL, husid_every=5, husid_slots=3))
    fetch = lambda s, kind, h: getattr(s, kind + "_fetch")(h)

    def same(x, y):
        assert len(x) == len(y) and all(np.array_equal(u, v) for u, v in zip(x, y))

    a = _solver(c1)
    for kind in kinds:
        assert [add[kind](a, i, p) for i, p in sets] == [0, 1]
    a.run(12)
    saved = {(kind, h): fetch(a, kind, h) for kind in kinds for h in (0, 1)}
    assert all(f[-1] == 12 for f in saved.values()) and np.array_equal(saved["cum", 0][3], [4, 9])
    assert all((saved[kind, h][0] != 0).any() for kind in kinds for h in (0, 1))
    a.peak_clear()
    for kind in ("spec", "cum"):
        for h in (0, 1):
            same(fetch(a, kind, h), saved[kind, h])
    assert [a.peak_add(i, p, rate=1, quantities=ALL) for i, p in sets] == [2, 3]
    with pytest.raises(ha.HqError, match="unknown peak tracker handle"):
        a.peak_fetch(0)
    b = _solver(c1)
    for kind in kinds:
        assert [add[kind](b, i, p) for i, p in sets] == [0, 1]
    tm1, tm2 = a.download()
    after = {}
    for name, s, first_peak in (("a", a, 2), ("b", b, 0)):
        handle = lambda kind, h: h + (first_peak if kind == "peak" else 0)
        s.upload(tm1, tm2, 12)
        for (kind, h), f in saved.items():
            getattr(s, kind + "_load")(handle(kind, h), *f)
        for (kind, h), f in saved.items():
            same(fetch(s, kind, handle(kind, h)), f)
        twins = [_add_twin(s, i, p, 1, 12) for i, p in sets]
        s.run(12)
        after[name] = {(kind, h): fetch(s, kind, handle(kind, h)) for kind, h in saved}
        for h, t in enumerate(twins):                        # this context's own trajectory: the loaded state, folded on
            steps, vals = s.record_fetch(t)
            assert np.array_equal(steps, np.arange(12, 24)) and vals.shape[2] == 9
            peaks, when, _ = saved["peak", h]
            same(after[name]["peak", h], host.peak_fold(steps, vals, ALL, peaks.copy(), when.copy()) + (24,))
            coef = s.spec_coefficients(h)
            same(after[name]["spec", h], host.spec_fold(coef, vals[:, :, 6:9], *[x.copy() for x in saved["spec", h][:3]]) + (24,))
            sums, span, curve, csteps, _ = saved["cum", h]
            got = after[name]["cum", h]
            same(_state(got), host.cum_fold(steps, vals, ALL, 0.0, sums.copy(), span.copy()) + (24,))
            slot2 = host.cum_fold(steps[:3], vals[:3], ALL, 0.0, sums.copy(), span.copy())[0][:, :, 3:]     # behind step 14
            assert np.array_equal(got[3], [4, 9, 14]) and np.array_equal(got[2][:2], curve) and np.array_equal(got[2][2], slot2)
        assert all(f[-1] == 24 and not np.array_equal(f[0], saved[key][0]) for key, f in after[name].items())
    a.close()
    b.close()
    for key in saved:                                        # the issue's bar: two contexts, fetch for fetch
        same(after["a"][key], after["b"][key])


@pytest.mark.parametrize("runner", ["sync", "async"])
def test_a_tracker_survives_the_runners(c1, runner):
    """hqh_solver_run_on with device_recorders = 1 and hqh_solver_run_async drop their own recorders and snapshots and leave a
    caller's cumulative tracker alone: it equals a fold of the samples the station callback was handed."""
    box = c1["box"]
    loaded, pattern = box.point_source(500.0, 500.0, 100.0, 0.0, 90.0, 0.0)
    calls = []
    rp = box.run_params(loaded=loaded, pattern=pattern, moment=1e15, rise_time=0.02, source_window=16, device_recorders=1,
                        station_ids=c1["ids"], station_phi=c1["phi"], station_rate=2, station_derivs=2,
                        station_fn=lambda step, vals: calls.append((step, vals)))
    s = box.create_solver()
    h = s.cum_add(c1["ids"], c1["phi"], rate=2, quantities=ALL, husid_every=5, husid_slots=4)
    for step0, n in ((0, 23), (23, 37)):
        if runner == "sync":
            box.solver_run(s, rp, step0, n)
        else:
            box.solver_run_async(s, rp, step0, n, slots=1)
    got = s.cum_fetch(h)
    s.close()
    steps = np.array([c[0] for c in calls], np.int32)
    assert np.array_equal(steps, np.arange(0, 60, 2))
    want = host.cum_fold(steps, np.array([c[1] for c in calls]), ALL, 0.0)
    assert (want[0][:, :, 3:].sum(axis=2) > 0).all()
    _same(_state(got), (want[0], want[1], 30))
    assert np.array_equal(got[3], [8, 18, 28, 38])


# ---------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------------

def test_bad_descriptions_and_unknown_handles(c1):
    ids, phi, surface = c1["ids"], c1["phi"], c1["surface"]
    sc = _solver(c1, variant=ha.HQ_VARIANT_SCATTER)
    for q in (A, ALL, V | A):
        with pytest.raises(ha.HqError, match="patch variant"):         # HQ_ERR_STATE, as hq_gather3
            sc.cum_add(surface, None, quantities=q)
    h = sc.cum_add(surface, None, rate=1, quantities=D | V, threshold=[0.0, 0.0])      # ... velocities it has
    t = _add_twin(sc, surface, None, 1, 60, derivs=1)
    sc.run(60)
    got, want = sc.cum_fetch(h), _fold_twin(sc.record_fetch(t), D | V, [0.0, 0.0, 0.0])
    sc.close()
    assert (got[0] > 0).any()
    _same(_state(got), want)

    s = _solver(c1)
    assert s._lib.hq_cum_clear(s._h) == 0                    # before any tracker: a no-op
    bad8, bad1 = ids.copy(), surface.copy()
    bad8[3, 5] = s.N
    bad1[-1] = s.N
    for kw in (dict(ids=bad8, phi=phi), dict(ids=bad1, phi=None), dict(ids=-1 - surface, phi=None),
               dict(ids=ids, phi=phi, rate=0), dict(ids=ids, phi=phi, rate=-2), dict(ids=ids, phi=phi, quantities=0),
               dict(ids=ids, phi=phi, quantities=8), dict(ids=ids, phi=phi, quantities=ALL | 16),
               dict(ids=ids, phi=phi, husid_every=1, husid_slots=0), dict(ids=ids, phi=phi, husid_every=0, husid_slots=1),
               dict(ids=ids, phi=phi, husid_every=-1, husid_slots=-1), dict(ids=ids, phi=phi, husid_every=-1, husid_slots=4),
               dict(ids=ids, phi=phi, threshold=-1.0), dict(ids=ids, phi=phi, threshold=float("nan")),
               dict(ids=ids, phi=phi, threshold=float("inf")),
               dict(ids=ids, phi=phi, quantities=ALL, threshold=[0.0, 0.0, -1e-300]),
               dict(ids=ids, phi=phi, quantities=ALL, threshold=[0.0, float("nan"), 0.0])):
        with pytest.raises(ha.HqError):
            s.cum_add(kw.pop("ids"), kw.pop("phi"), **kw)
    lib = s._lib
    hh = ctypes.c_int32(-1)
    thr = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    for npts, k, i, p in ((-1, 8, ids, phi), (5, 4, ids, phi), (5, 0, ids, phi), (5, 8, None, phi), (5, 8, ids, None), (5, 1, None, None)):
        d = capi._CumDesc(npts, k, None if i is None else i.ctypes.data, None if p is None else p.ctypes.data, 1, 0, V, 0, 0, 0, thr)
        assert lib.hq_cum_add(s._h, ctypes.byref(d), ctypes.byref(hh)) == -1
    ok = capi._CumDesc(5, 8, ids.ctypes.data, phi.ctypes.data, 1, 0, V, 0, 0, 0, thr)
    assert lib.hq_cum_add(s._h, ctypes.byref(ok), None) == -1 and lib.hq_cum_add(s._h, None, ctypes.byref(hh)) == -1
    sm, sp, n, nf = np.zeros(30), np.zeros(15, np.int32), ctypes.c_int64(), ctypes.c_int32()
    for handle in (0, 7, -1):                                # nothing was added
        assert lib.hq_cum_fetch(s._h, handle, capi._ptr(sm), capi._ptr(sp), None, None, ctypes.byref(nf), ctypes.byref(n)) == -1
        assert lib.hq_cum_load(s._h, handle, capi._ptr(sm), capi._ptr(sp), None, None, 0, ctypes.c_int64(0)) == -1
        assert lib.hq_cum_reset(s._h, handle) == -1
    h = s.cum_add(ids, phi, rate=1, quantities=V, husid_every=2, husid_slots=2)
    assert lib.hq_cum_fetch(s._h, h, None, capi._ptr(sp), None, None, ctypes.byref(nf), ctypes.byref(n)) == -1
    assert lib.hq_cum_fetch(s._h, h, capi._ptr(sm), None, None, None, ctypes.byref(nf), ctypes.byref(n)) == -1
    assert lib.hq_cum_fetch(s._h, h, capi._ptr(sm), capi._ptr(sp), None, None, None, ctypes.byref(n)) == -1
    assert lib.hq_cum_fetch(s._h, h, capi._ptr(sm), capi._ptr(sp), None, None, ctypes.byref(nf), None) == -1
    assert lib.hq_cum_fetch(s._h, h, capi._ptr(sm), capi._ptr(sp), None, None, ctypes.byref(nf), ctypes.byref(n)) == 0
    assert lib.hq_cum_load(s._h, h, capi._ptr(sm), None, None, None, 0, ctypes.c_int64(0)) == -1
    assert lib.hq_cum_load(s._h, h, None, capi._ptr(sp), None, None, 0, ctypes.c_int64(0)) == -1
    assert lib.hq_cum_load(s._h, h, capi._ptr(sm), capi._ptr(sp), None, None, 0, ctypes.c_int64(-1)) == -1
    assert lib.hq_cum_load(s._h, h, capi._ptr(sm), capi._ptr(sp), None, None, 1, ctypes.c_int64(2)) == -1    # a slot without its arrays
    assert lib.hq_cum_load(s._h, h, capi._ptr(sm), capi._ptr(sp), None, None, 0, ctypes.c_int64(2)) == -1    # 2 samples fill a slot
    assert lib.hq_cum_load(s._h, h, capi._ptr(sm), capi._ptr(sp), None, None, 0, ctypes.c_int64(1)) == 0
    s.cum_clear()
    for dead in (h,):
        assert lib.hq_cum_fetch(s._h, dead, capi._ptr(sm), capi._ptr(sp), None, None, ctypes.byref(nf), ctypes.byref(n)) == -1
        assert lib.hq_cum_reset(s._h, dead) == -1
    s.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. a context without cumulative trackers
# ---------------------------------------------------------------------------------------------------------------------

def test_a_context_without_trackers_is_untouched(c1, brick_mode):
    """A solver that never adds a cumulative tracker and a second, identically built one that tracks accelerations on the
    whole surface: the same step, the same device_bytes once the tracker is gone, and a final field equal to the recorder
    tests' own bar for two separately run solvers (1e-9 relative L-inf).  hq_cum_clear before any tracker is a no-op."""
    a, b = _solver(c1), _solver(c1)
    assert a._lib.hq_cum_clear(a._h) == 0
    assert a.info()["device_bytes"] == b.info()["device_bytes"]
    b.cum_add(c1["surface"], None, rate=1, quantities=ALL, husid_every=HUSID_EVERY, husid_slots=HUSID_SLOTS)
    for n in BATCHES:
        a.run(n)
        b.run(n)
    b.cum_clear()
    ia, ib = a.info(), b.info()
    ua, ub = a.download(), b.download()
    a.close()
    b.close()
    assert ia["step"] == ib["step"] == NSTEPS and ia["device_bytes"] == ib["device_bytes"]
    assert np.abs(ua[0]).max() > 0
    assert H.rel_linf(ub[0], ua[0]) < TOL and H.rel_linf(ub[1], ua[1]) < TOL
