"""Device-side sample recorders (hq_record_add / _pending / _fetch / _clear, include/hq_solver.h; hqh_run_params.
device_recorders, include/hq_host.h): what solver_output_stations / solver_output_planes read at the top of the loop body
(psolve.c:4279-4280, :6679-6787; io_planes.c:176-200), sampled by hq_k_record between host syncs.

The yardstick everywhere is the existing host route -- hq_gather / hq_gather3 at every print step and the trilinear sums of
hqh_station_kinematics on the host -- whose results are pinned to the reference's own station and plane files.  The device
sums run in the same order of operations without contraction, so every comparison with that route ON THE SAME STATE is
np.array_equal; the bars against the golden files are the existing tests' own (6e-7 of a column group's maximum for the
7-digit station files, 1e-9 relative L-inf for the plane files).

"The same state" cannot come from a second, identically built solver: the element-form patch kernels accumulate element
forces with fp64 LDS atomics (hq_patch.h), so two runs of one and the same build differ in the last bits.  Measured on an
MI355X with the unchanged host route run twice on examples/simple (300 steps, five stations, accelerations): 2 172 of 4 500
displacement values differ (by up to 7.2e-12 at a scale of 8.6e2 in the file's units), the final fields differ, and
accelerations differ by up to 4.5e-7 at a scale of 1.4e5 -- while recorder and hq_gather3 + host sums on ONE solver agreed in
all 13 500 values.  So the bit-for-bit comparisons below are made on one trajectory:
  * test_recorder_equals_the_gather_route_on_the_same_solver steps a recording solver one step at a time and gathers in front
    of every step (the route of the issue, word for word), and pins that a point with weights (1, 0, ..., 0) records its
    node's row EXACTLY;
  * where the steps run in batches (which is what is to be tested) an auxiliary recorder of such unit-weight points, at every
    step, supplies the rows hq_gather3 would have returned at the head of each step of the SAME batch: u(t) is its sample of the
    step, u(t - dt) that of the step before, u(t - 2 dt) that of two steps before; hqh_station_kinematics sums them on the host.
Two separately run solvers are compared with the project's parity bar (1e-9 relative L-inf), not bit for bit."""
import ctypes
import shutil

import numpy as np
import pytest

import hercules_amd as ha
from hercules_amd import capi, host
from tests import helpers as H

pytestmark = pytest.mark.gpu

TOL = 1e-9


@pytest.fixture(params=["bricks", "patches-only"])
def brick_mode(request, monkeypatch):
    """As shipped (hq_k_brick takes the simple nodes of uniform regions) and with HQ_NO_BRICKS=1 (patches everywhere)."""
    if request.param == "patches-only":
        monkeypatch.setenv("HQ_NO_BRICKS", "1")
    else:
        monkeypatch.delenv("HQ_NO_BRICKS", raising=False)
    return request.param


def _field(box, seed, amp=1e-3):
    """A start field that is a function of the node's GLOBAL grid position: the same on every partition that harbors it."""
    ijk = box.node_ijk.astype(np.int64)
    gid = (ijk[:, 2] * (box.ny + 1) + ijk[:, 1]) * (box.nx + 1) + ijk[:, 0]
    u = np.empty((len(gid), 3))
    for d in range(3):
        x = (gid * 3 + d + seed) * np.int64(2654435761) % np.int64(2 ** 31)
        u[:, d] = (x.astype(np.float64) / 2 ** 30 - 1.0) * amp
    return u


def _kinematics(phi, rows, dt, derivs):
    """hqh_station_kinematics (the host route's sums) on gathered node rows: rows = (tm1, tm2, tm3), each [n * 8, 3] in the
    solver's real type (widened to double here, exactly) or None -> [n, 3 (1 + derivs)]."""
    lib = host.load_library()
    n = len(phi)
    phi = np.ascontiguousarray(phi, np.float64)
    t = [None if r is None else np.ascontiguousarray(np.asarray(r, np.float64).reshape(n, 24)) for r in rows]
    out = np.zeros((n, 3 * (1 + derivs)))
    for s in range(n):
        p = [ctypes.c_void_p(phi.ctypes.data + 64 * s)]
        p += [None if a is None else ctypes.c_void_p(a.ctypes.data + 192 * s) for a in t]
        rc = lib.hqh_station_kinematics(p[0], p[1], p[2], p[3], ctypes.c_double(dt), ctypes.c_int32(derivs),
                                        ctypes.c_void_p(out.ctypes.data + 8 * out.shape[1] * s))
        assert rc == 0
    return out


def _gather_sample(s, ids, phi, dt, derivs):
    if derivs == 2:
        rows = s.gather3(ids)
    else:
        g = s.gather(ids)
        rows = (g[0], g[1] if derivs else None, None)
    return _kinematics(phi, rows, dt, derivs)


def _per_step_route(s, ids, phi, dt, derivs, rate, nsteps, step=lambda s: s.run(1)):
    """The host route on solver `s`: one step at a time, hq_gather[3] + host kinematics at the head of every due step."""
    steps, vals = [], []
    for _ in range(nsteps):
        k = s.info()["step"]
        if k % rate == 0:
            steps.append(k)
            vals.append(_gather_sample(s, ids, phi, dt, derivs))
        step(s)
    return np.array(steps, np.int32), np.array(vals).reshape(len(steps), len(phi), 3 * (1 + derivs))


def _unit_points(ids):
    """The 8 nodes of every point as recorder points of their own with weights (1, 0, ..., 0): their displacement sample is the
    node's row itself (1 x + 0 x + ... = x exactly)."""
    flat = np.asarray(ids, np.int32).reshape(-1)
    phi = np.zeros((len(flat), 8))
    phi[:, 0] = 1.0
    return np.repeat(flat[:, None], 8, axis=1), phi


def _add_rows_recorder(s, ids, capacity):
    uid, uphi = _unit_points(ids)
    return s.record_add(uid, uphi, rate=1, derivs=0, capacity=capacity)


def _route_from_rows(rows, tm2_first, tm3_first, first, due, phi, dt, derivs):
    """The host route on the node rows an auxiliary unit-weight recorder took at EVERY step from `first` on (rows [k, n * 8, 3]);
    tm2_first / tm3_first: u(t - dt) / u(t - 2 dt) at those nodes at step `first` (what the solver was given)."""
    seq = [np.asarray(tm3_first, np.float64), np.asarray(tm2_first, np.float64)] + list(rows)
    out = [_kinematics(phi, (seq[k - first + 2], seq[k - first + 1], seq[k - first]), dt, derivs) for k in due]
    return np.array(out).reshape(len(due), len(phi), 3 * (1 + derivs))


def _start_rows(s, ids, u2):
    """u(t - dt) and u(t - 2 dt) at the points' nodes of a solver created with tm2 = u2: u2 in the solver's real type; zero."""
    r = np.asarray(u2, s.real)[np.asarray(ids).reshape(-1)].astype(np.float64)
    return r, np.zeros_like(r)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_recorder_equals_the_gather_route_on_the_same_solver(c1, precision):
    """One solver, stepped one step at a time, hq_gather3 + hqh_station_kinematics in front of every step, while a recorder
    (rate 1, accelerations) samples the same steps: equal bit for bit; and unit-weight points record their node's row."""
    s = _c1_solver(c1, precision)
    ids, phi = c1["ids"], c1["phi"]
    h = s.record_add(ids, phi, rate=1, derivs=2, capacity=40)
    hr = _add_rows_recorder(s, ids, 40)
    rows = []

    def step(s):
        rows.append(np.asarray(s.gather(ids)[0], np.float64))
        s.run(1)
    steps, vals = _per_step_route(s, ids, phi, c1["dt"], 2, 1, 40, step=step)
    rs, rv = s.record_fetch(h)
    _, got_rows = s.record_fetch(hr)
    s.close()
    assert np.array_equal(rs, steps) and np.abs(vals[2:, :, 6:]).max() > 0
    assert np.array_equal(rv, vals)
    assert np.array_equal(got_rows, np.array(rows))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reference's stations
# ---------------------------------------------------------------------------------------------------------------------

def test_reference_stations_through_the_runner(tmp_path):
    """examples/simple driven by the reference's force file, five stations with velocities and accelerations at every step:
    hqh_solver_run with device_recorders = 1, in two calls, calls station_fn in the step sequence of the host-gather run,
    with its values to the parity bar (two solver runs are not bit-reproducible: module docstring) -- and those match the
    reference's own station files (tests/golden/c1_stations_va) within the existing test's bar."""
    g = H.load("c1_stations_va")
    ref = g["stations"]                                  # [5, steps, 10]
    nsteps = 300
    assert ref.shape[1] >= nsteps
    ff = tmp_path / "force_process.0"
    host.forcefile_write(str(ff), g["loaded_lnid"], g["forces"])
    box = host.Box(H.C1_NX, H.C1_NY, H.C1_NZ, H.C1_H, 1e-3, 5.0)
    ids, phi, mine = box.stations(H.C1_STATIONS)
    assert mine.all()
    calls = {0: [], 1: []}
    for dev in (0, 1):
        s = box.create_solver()
        rp = box.run_params(loaded=g["loaded_lnid"], force_file=str(ff), source_window=128, station_ids=ids,
                            station_phi=phi, station_rate=1, station_derivs=2, device_recorders=dev,
                            station_fn=lambda step, vals, dev=dev: calls[dev].append((step, vals)))
        if dev:
            box.solver_run(s, rp, 0, 120)
            assert s.record_clear() is None              # the runner left no recorder behind: nothing to drop, no error
            box.solver_run(s, rp, 120, nsteps - 120)
        else:
            box.solver_run(s, rp, 0, nsteps)
        s.close()
    assert [c[0] for c in calls[0]] == list(range(nsteps))
    assert [c[0] for c in calls[1]] == list(range(nsteps))
    a = np.array([c[1] for c in calls[0]])
    b = np.array([c[1] for c in calls[1]])
    assert a.shape == b.shape == (nsteps, 5, 9)
    assert np.abs(a).max() > 0
    for k in range(3):                                   # two separately run solvers: the parity bar (module docstring)
        err = H.rel_linf(b[:, :, 3 * k:3 * k + 3], a[:, :, 3 * k:3 * k + 3])
        print("column group %d: device recorders vs host gathers %.3e" % (k, err))
        assert err < TOL
    for k in range(3):
        want = ref[:, :nsteps, 1 + 3 * k:4 + 3 * k]
        scale = np.abs(want).max()
        err = np.abs(b[:, :, 3 * k:3 * k + 3].transpose(1, 0, 2) - want).max()
        print("column group %d: err %.3e, bar %.3e" % (k, err, 6e-7 * scale))
        assert err <= 6e-7 * scale, (k, err, scale)
    box.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the brick-stream hazard
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big_box():
    nx, ny, nz, h, dt = 64, 64, 32, 15.0, 3e-4
    box = host.Box(nx, ny, nz, h, dt, 30.0)
    L = np.array([nx * h, ny * h, nz * h])
    corners = np.array([[(c >> 0) & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)], np.float64)
    pts = [np.where(corners > 0, L - 1.0, 1.0), L[None, :] / 2 + np.array([[3.0, -2.0, 1.0]]),
           np.random.default_rng(20261017).uniform(0.0, 1.0, (55, 3)) * L]
    ids, phi, mine = box.stations(np.concatenate(pts))
    assert len(ids) == 64 and mine.all()
    loaded, pattern = box.point_source(L[0] / 2, L[1] / 2, L[2] / 2, 30.0, 70.0, 10.0)
    rp = box.run_params(loaded=loaded, pattern=pattern, moment=1e13, rise_time=20 * dt, source_window=64)
    F = box.source_table(rp, 0, 40)
    u = _field(box, 77)
    yield dict(box=box, ids=ids, phi=phi, loaded=loaded, F=F, u1=u, u2=0.999 * u, dt=dt)
    box.close()


@pytest.mark.parametrize("brick_stream", [1, 0])
def test_samples_are_taken_before_the_bricks_overwrite_the_oldest_field(big_box, brick_mode, brick_stream):
    """d_u[spare] is u(t - 2 dt) AND the buffer the step's kernels write u(t + dt) into: with the bricks on a stream of
    their own nothing but the recorder's event orders hq_k_record ahead of them.  64 stations (the domain's 8 corner
    elements, the centre, random points), accelerations at every step, 40 steps in ONE hq_run: the samples equal what
    the host sums yield on the rows of the SAME batch (auxiliary unit-weight recorder, module docstring), bit for bit, and an
    identical solver that is stopped and gathered (hq_gather3) at every step to the parity bar."""
    b = big_box
    s = b["box"].create_solver(tm1=b["u1"], tm2=b["u2"], options={"brick_stream": brick_stream})
    s.set_source(b["loaded"], b["F"])
    h = s.record_add(b["ids"], b["phi"], rate=1, derivs=2, capacity=40)
    hr = _add_rows_recorder(s, b["ids"], 40)             # reads u(t) only: nothing of a step overwrites that
    s.run(40)
    assert s.record_pending(h) == (40, 0)
    steps, vals = s.record_fetch(h)
    assert s.record_pending(h) == (0, -1)
    rsteps, rows = s.record_fetch(hr)
    info = s.info()
    if brick_mode == "bricks":
        assert info["brick_units"] > 0 and info["brick_stream"] == brick_stream
    else:
        assert info["brick_units"] == 0
    tm2, tm3 = _start_rows(s, b["ids"], b["u2"])
    s.close()
    assert np.array_equal(steps, np.arange(40)) and np.array_equal(rsteps, steps)
    rvals = _route_from_rows(rows, tm2, tm3, 0, steps, b["phi"], b["dt"], 2)
    assert vals.shape == (40, 64, 9) and np.abs(rvals[:, :, 6:]).max() > 0
    assert np.array_equal(vals, rvals)
    # ... and against a second, identical solver that is stopped and gathered (hq_gather3) at every step: the parity bar
    r = b["box"].create_solver(tm1=b["u1"], tm2=b["u2"], options={"brick_stream": brick_stream})
    r.set_source(b["loaded"], b["F"])
    _, gvals = _per_step_route(r, b["ids"], b["phi"], b["dt"], 2, 1, 40)
    r.close()
    for k in range(3):
        assert H.rel_linf(vals[:, :, 3 * k:3 * k + 3], gvals[:, :, 3 * k:3 * k + 3]) < TOL


@pytest.mark.parametrize("brick_stream", [1, 0])
def test_all_three_kinds_due_on_one_step_share_one_hold(big_box, brick_mode, brick_stream):
    """Recorders, trackers and a snapshot on ONE solver beside the bricks' stream, 40 steps in ONE hq_run: every step has a
    recorder with accelerations, the unit-weight rows recorder, a K = 8 tracker of all three quantities and a K = 1 velocity
    tracker (which holds nothing back) due, every fourth a snapshot of tm1 | tm2 | vel over all nodes as well -- the head
    of such a step holds the other streams once, behind the last launch that reads what they overwrite.  All comparisons
    are made on this one trajectory (module docstring), bit for bit."""
    b = big_box
    ids, phi, dt = b["ids"], b["phi"], b["dt"]
    flat = np.asarray(ids).reshape(-1)
    ALL = capi.HQ_PEAK_DISP | capi.HQ_PEAK_VEL | capi.HQ_PEAK_ACC
    s = b["box"].create_solver(tm1=b["u1"], tm2=b["u2"], options={"brick_stream": brick_stream})
    s.set_source(b["loaded"], b["F"])
    h = s.record_add(ids, phi, rate=1, derivs=2, capacity=40)
    hr = _add_rows_recorder(s, ids, 40)
    hp8 = s.peak_add(ids, phi, rate=1, quantities=ALL)
    hp1 = s.peak_add(np.ascontiguousarray(ids[:, 0]), None, rate=1, quantities=capi.HQ_PEAK_VEL)
    hs = s.snapshot_add(rate=4, fields=capi.HQ_SNAP_TM1 | capi.HQ_SNAP_TM2 | capi.HQ_SNAP_VEL, slots=10)
    s.run(40)
    assert s.record_pending(h) == (40, 0) and s.record_pending(hr) == (40, 0)
    npending, _, first = s.snapshot_pending(hs)
    assert (npending, first) == (10, 0)
    steps, vals = s.record_fetch(h)
    rsteps, rows = s.record_fetch(hr)
    pk8, when8, n8 = s.peak_fetch(hp8)
    pk1, when1, n1 = s.peak_fetch(hp1)
    snaps = [s.snapshot_fetch(hs) for _ in range(10)]
    assert s.record_pending(h) == (0, -1) and s.snapshot_pending(hs)[0] == 0 and s.snapshot_fetch(hs)[0] == -1
    info = s.info()
    if brick_mode == "bricks":
        assert info["brick_units"] > 0 and info["brick_stream"] == brick_stream
    else:
        assert info["brick_units"] == 0
    tm2, tm3 = _start_rows(s, ids, b["u2"])
    s.close()
    assert np.array_equal(steps, np.arange(40)) and np.array_equal(rsteps, steps)
    assert [sn[0] for sn in snaps] == list(range(0, 40, 4))
    # the recorder: the host route on the rows of the same batch
    rvals = _route_from_rows(rows, tm2, tm3, 0, steps, phi, dt, 2)
    assert vals.shape == (40, 64, 9) and np.abs(rvals[:, :, 6:]).max() > 0
    assert np.array_equal(vals, rvals)
    # the K = 8 tracker: the fold of the recorder's samples
    want8 = host.peak_fold(steps, vals, ALL)
    assert n8 == 40 and pk8.shape == (64, 3, 5) and (pk8[:, :, 4] > 0).all()
    assert np.array_equal(pk8, want8[0]) and np.array_equal(when8, want8[1])
    # the K = 1 tracker: the fold of (0 + u1, (0 + u1 - u2) / dt) at the stations' first nodes, from the rows recorder
    u1 = np.asarray(rows, np.float64)[:, 0::8, :]
    u2 = np.concatenate([tm2[None, 0::8, :], u1[:-1]])
    d = 0.0 + u1
    want1 = host.peak_fold(steps, np.ascontiguousarray(np.concatenate([d, (d - u2) / dt], axis=2)), capi.HQ_PEAK_VEL)
    assert n1 == 40 and pk1.shape == (64, 1, 5) and (pk1[:, 0, 4] > 0).all()
    assert np.array_equal(pk1, want1[0]) and np.array_equal(when1, want1[1])
    # the snapshots: u(t) and u(t - dt) at the stations' nodes are the rows of that step and of the step before
    for step, s1, s2, sv in snaps:
        assert np.array_equal(np.asarray(s1, np.float64)[flat], rows[step])
        assert np.array_equal(np.asarray(s2, np.float64)[flat], rows[step - 1] if step else tm2)
        assert sv.shape == s1.shape and np.abs(sv).max() > 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. two partitions in one process
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("overlap", [0, 1])
def test_two_partitions_record_through_group_run(brick_mode, overlap):
    """(overlap = 1: the exchange chain on a stream of its own, which a due step holds back behind hq_k_record.)  Two partitions of a 32 x 32 x 16 box in one process (hq_group_link): each rank records the stations whose element it
    owns -- points on both sides of the cut, among them the centres of elements that touch it -- with velocities, every
    second step, 30 steps in one hq_group_run; equal to the per-step hq_gather route on an identical pair."""
    nx, ny, nz, h, dt = 32, 32, 16, 15.0, 3e-4
    boxes = [host.Box(nx, ny, nz, h, dt, 30.0, rank=r, nranks=2) for r in range(2)]
    L = np.array([nx * h, ny * h, nz * h])
    pts = [np.random.default_rng(5).uniform(0.0, 1.0, (24, 3)) * L]
    shared = []
    for bx in boxes:
        sch = bx.schedule()
        sh = np.unique(np.concatenate([m for _, m in sch["c"] + sch["s"]]))
        assert len(sh) > 0
        shared.append(sh)
        touching = np.nonzero(np.isin(bx.lnid, sh).any(axis=1))[0]
        pick = touching[:: max(1, len(touching) // 6)][:6]
        pts.append((bx.node_ijk[bx.lnid[pick]].min(axis=1) + 0.5) * h)       # centres of elements that touch the cut
    pts = np.concatenate(pts)
    stations = []
    for bx, sh in zip(boxes, shared):
        ids, phi, mine = bx.stations(pts)
        ids, phi = ids[mine != 0], phi[mine != 0]
        assert len(ids) >= 6 and np.isin(ids, sh).any()
        stations.append((ids, phi))
    assert len(stations[0][0]) + len(stations[1][0]) == len(pts)
    fields = [_field(bx, 31) for bx in boxes]
    out = []
    for recorded in (True, False):
        solvers = [bx.create_solver(tm1=u, tm2=0.999 * u, options={"overlap": overlap}) for bx, u in zip(boxes, fields)]
        capi.group_link(solvers)
        if recorded:
            hs = [s.record_add(ids, phi, rate=2, derivs=1, capacity=15) for s, (ids, phi) in zip(solvers, stations)]
            hrs = [_add_rows_recorder(s, ids, 32) for s, (ids, phi) in zip(solvers, stations)]
            capi.group_run(solvers, 30)
            out.append([s.record_fetch(hd) for s, hd in zip(solvers, hs)])
            same = []
            for s, hr, (ids, phi), u in zip(solvers, hrs, stations, fields):
                rsteps, rows = s.record_fetch(hr)
                assert np.array_equal(rsteps, np.arange(30))
                tm2, tm3 = _start_rows(s, ids, 0.999 * u)
                same.append(_route_from_rows(rows, tm2, tm3, 0, range(0, 30, 2), phi, dt, 1))
            with pytest.raises(ha.HqError):              # 15 slots, all free again, but 16 due steps
                capi.group_run(solvers, 31)
            assert [s.info()["step"] for s in solvers] == [30, 30]
        else:
            steps, vals = [], [[], []]
            for k in range(30):
                if k % 2 == 0:
                    steps.append(k)
                    for r in range(2):
                        vals[r].append(_gather_sample(solvers[r], stations[r][0], stations[r][1], dt, 1))
                capi.group_run(solvers, 1)
            out.append([(np.array(steps, np.int32), np.array(v)) for v in vals])
        for s in solvers:
            s.close()
    for r in range(2):
        assert np.array_equal(out[0][r][0], np.arange(0, 30, 2)) and np.array_equal(out[1][r][0], out[0][r][0])
        assert out[0][r][1].shape == (15, len(stations[r][0]), 6) and np.abs(out[1][r][1][:, :, 3:]).max() > 0
        assert np.array_equal(out[0][r][1], same[r])                      # the rows of the same batch: bit for bit
        for k in range(2):                                                # an identical pair, gathered per step: parity bar
            assert H.rel_linf(out[0][r][1][:, :, 3 * k:3 * k + 3], out[1][r][1][:, :, 3 * k:3 * k + 3]) < TOL
    for bx in boxes:
        bx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. cadence, ring and errors on the C1 box
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def c1():
    box = host.Box(H.C1_NX, H.C1_NY, H.C1_NZ, H.C1_H, 1e-3, 5.0)
    ids, phi, mine = box.stations(H.C1_STATIONS + [(33.0, 977.0, 412.5), (999.0, 1.0, 499.0)])
    assert mine.all()
    loaded, pattern = box.point_source(500.0, 500.0, 100.0, 0.0, 90.0, 0.0)
    rp = box.run_params(loaded=loaded, pattern=pattern, moment=1e15, rise_time=0.02, source_window=64)
    F = box.source_table(rp, 0, 64)
    u = _field(box, 5)
    yield dict(box=box, ids=ids, phi=phi, loaded=loaded, F=F, u1=u, u2=0.999 * u, dt=1e-3)
    box.close()


def _c1_solver(c1, precision="f64", variant=ha.HQ_VARIANT_AUTO):
    s = c1["box"].create_solver(tm1=c1["u1"], tm2=c1["u2"], precision=precision, variant=variant)
    s.set_source(c1["loaded"], c1["F"])
    return s


def _cadence(c1, precision):
    s = _c1_solver(c1, precision)
    h = s.record_add(c1["ids"], c1["phi"], rate=3, derivs=2, capacity=8)
    hr = _add_rows_recorder(s, c1["ids"], 16)
    assert s.record_pending(h) == (0, -1)
    for n, pending in ((1, 1), (7, 3), (2, 4), (5, 5)):
        s.run(n)
        assert s.record_pending(h) == (pending, 0)
    steps, vals = s.record_fetch(h)
    rsteps, rows = s.record_fetch(hr)
    tm2, tm3 = _start_rows(s, c1["ids"], c1["u2"])
    s.close()
    assert vals.dtype == np.float64 and np.array_equal(steps, [0, 3, 6, 9, 12]) and np.array_equal(rsteps, np.arange(15))
    rvals = _route_from_rows(rows, tm2, tm3, 0, steps, c1["phi"], c1["dt"], 2)
    assert np.abs(rvals[1:, :, 6:]).max() > 0
    assert np.array_equal(vals, rvals)


def test_cadence_across_calls(c1, brick_mode):
    """rate = 3 over run(1), run(7), run(2), run(5): the steps recorded are 0, 3, 6, 9, 12 -- step 0 is the initial state, the
    state after the last step is not sampled -- hq_record_pending agrees after every call, the values are the host route's."""
    _cadence(c1, "f64")


def test_two_recorders_at_once(c1, brick_mode):
    """Two recorders on one context (every step with accelerations; every tenth step, displacements) deliver what each
    delivers alone."""
    def run(which):
        s = _c1_solver(c1)
        hs = [s.record_add(c1["ids"], c1["phi"], rate=rate, derivs=dv, capacity=32) for rate, dv in which]
        hr = _add_rows_recorder(s, c1["ids"], 32)
        s.run(25)
        got = [s.record_fetch(h) for h in hs]
        rows = s.record_fetch(hr)[1]
        tm2, tm3 = _start_rows(s, c1["ids"], c1["u2"])
        s.close()
        want = [_route_from_rows(rows, tm2, tm3, 0, g[0], c1["phi"], c1["dt"], dv) for g, (_, dv) in zip(got, which)]
        return got, want
    a, b = (1, 2), (10, 0)
    (both, want), (only_a, want_a), (only_b, want_b) = run([a, b]), run([a]), run([b])
    assert np.array_equal(both[0][0], np.arange(25)) and np.array_equal(both[1][0], [0, 10, 20])
    assert both[0][1].shape == (25, 7, 9) and both[1][1].shape == (3, 7, 3)
    # each delivers the host route's numbers on its own run's rows, together and alone; two runs agree to the parity bar
    for got, ref in ((both[0], want[0]), (both[1], want[1]), (only_a[0], want_a[0]), (only_b[0], want_b[0])):
        assert np.array_equal(got[1], ref)
    assert np.array_equal(both[0][0], only_a[0][0]) and np.array_equal(both[1][0], only_b[0][0])
    assert H.rel_linf(both[1][1], only_b[0][1]) < TOL and H.rel_linf(both[0][1][:, :, :3], only_a[0][1][:, :, :3]) < TOL
    assert np.array_equal(both[1][1], both[0][1][::10, :, :3]) and np.abs(both[1][1]).max() > 0


def test_ring_overflow_is_refused_before_anything_is_enqueued(c1, brick_mode):
    s = _c1_solver(c1)
    h = s.record_add(c1["ids"], c1["phi"], rate=1, derivs=0, capacity=4)
    hr = _add_rows_recorder(s, c1["ids"], 64)            # (never the ring that is short of room)
    with pytest.raises(ha.HqError):
        s.run(5)
    assert s.info()["step"] == 0 and s.record_pending(h) == (0, -1)
    with pytest.raises(ha.HqError):
        s.run_timed(5)
    assert s.info()["step"] == 0
    s.run(4)
    steps, vals = s.record_fetch(h, 2)
    assert np.array_equal(steps, [0, 1]) and vals.shape == (2, 7, 3)
    assert s.record_pending(h) == (2, 2)
    with pytest.raises(ha.HqError):
        s.run(3)
    assert s.info()["step"] == 4
    steps2, vals2 = s.record_fetch(h)
    assert np.array_equal(steps2, [2, 3])
    s.run(4)                                             # the ring wraps: slots 0..3 again
    steps3, vals3 = s.record_fetch(h)
    assert np.array_equal(steps3, [4, 5, 6, 7]) and s.info()["step"] == 8
    rsteps, rows = s.record_fetch(hr)
    tm2, tm3 = _start_rows(s, c1["ids"], c1["u2"])
    s.close()
    assert np.array_equal(rsteps, np.arange(8))
    rvals = _route_from_rows(rows, tm2, tm3, 0, range(8), c1["phi"], c1["dt"], 0)
    assert np.array_equal(np.concatenate([vals, vals2, vals3]), rvals)


def test_upload_keeps_recorders_and_moves_the_due_steps(c1, brick_mode):
    s = _c1_solver(c1)
    h = s.record_add(c1["ids"], c1["phi"], rate=2, derivs=1, capacity=8)
    hr = _add_rows_recorder(s, c1["ids"], 8)
    s.run(3)                                             # samples of steps 0 and 2 stay pending across the upload
    tm1, tm2 = s.download()
    s.upload(tm1 * 0.5, tm2 * 0.25, 250)
    assert s.record_pending(h) == (2, 0) and s.record_pending(hr) == (3, 0)
    s.run(3)
    steps, vals = s.record_fetch(h)
    rsteps, rows = s.record_fetch(hr)
    s.close()
    assert np.array_equal(steps, [0, 2, 250, 252]) and np.array_equal(rsteps, [0, 1, 2, 250, 251, 252])
    flat = c1["ids"].reshape(-1)
    assert np.array_equal(rows[3], (tm1 * 0.5)[flat])    # the uploaded field is what step 250 samples
    rvals = _route_from_rows(rows[3:], (tm2 * 0.25)[flat], np.zeros((len(flat), 3)), 250, [250, 252], c1["phi"], c1["dt"], 1)
    assert np.abs(rvals).max() > 0 and np.array_equal(vals[2:], rvals)


def test_bad_descriptions_and_cleared_handles(c1, brick_mode):
    ids, phi = c1["ids"], c1["phi"]
    sc = _c1_solver(c1, variant=ha.HQ_VARIANT_SCATTER)
    with pytest.raises(ha.HqError):                      # u(t - 2 dt) is kept by the patch variant only, as hq_gather3 says
        sc.record_add(ids, phi, rate=1, derivs=2, capacity=4)
    h = sc.record_add(ids, phi, rate=1, derivs=1, capacity=4)       # ... velocities it has
    hr = _add_rows_recorder(sc, ids, 4)
    sc.run(3)
    steps, vals = sc.record_fetch(h)
    rows = sc.record_fetch(hr)[1]
    tm2, tm3 = _start_rows(sc, ids, c1["u2"])
    sc.close()
    assert np.array_equal(steps, [0, 1, 2])
    assert np.array_equal(vals, _route_from_rows(rows, tm2, tm3, 0, steps, phi, c1["dt"], 1))

    s = _c1_solver(c1)
    bad = ids.copy()
    bad[3, 5] = s.N
    for kw in (dict(ids=bad, rate=1, capacity=4), dict(ids=-1 - ids, rate=1, capacity=4), dict(ids=ids, rate=0, capacity=4),
               dict(ids=ids, rate=1, capacity=0), dict(ids=ids, rate=1, capacity=4, derivs=3),
               dict(ids=ids, rate=1, capacity=4, derivs=-1)):
        with pytest.raises(ha.HqError):
            s.record_add(kw.pop("ids"), phi, **kw)
    with pytest.raises(ha.HqError):
        s.record_pending(0)                              # nothing was added
    bytes0 = s.info()["device_bytes"]
    h = s.record_add(ids, phi, rate=1, derivs=0, capacity=4)
    assert s.info()["device_bytes"] >= bytes0 + 4 * 7 * 3 * 8 + 7 * 8 * 12
    s.run(2)
    s.record_clear()
    assert s.info()["device_bytes"] == bytes0
    with pytest.raises(ha.HqError):
        s.record_pending(h)
    with pytest.raises(ha.HqError):
        s.record_fetch(h)
    s.run(10)                                            # records nothing, overflows nothing
    h2 = s.record_add(ids, phi, rate=1, derivs=0, capacity=4)
    assert h2 != h and s.record_pending(h2) == (0, -1)
    s.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. no traffic between fetches
# ---------------------------------------------------------------------------------------------------------------------

def test_nothing_crosses_pcie_between_fetches(c1):
    s = _c1_solver(c1)
    h = s.record_add(c1["ids"], c1["phi"], rate=1, derivs=2, capacity=100)
    s.sync()
    before = s.info()
    s.run(100)
    s.sync()
    after = s.info()
    assert after["pcie_d2h_bytes"] == before["pcie_d2h_bytes"] and after["pcie_h2d_bytes"] == before["pcie_h2d_bytes"]
    steps, vals = s.record_fetch(h)
    assert len(steps) == 100
    assert s.info()["pcie_d2h_bytes"] - after["pcie_d2h_bytes"] == 8 * 100 * len(c1["ids"]) * 9
    s.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. planes
# ---------------------------------------------------------------------------------------------------------------------

def test_plane_files_are_those_of_the_host_path(tmp_path):
    """test_output_planes_written_by_the_c_solver_run's set-up (tests/golden/c1_planes) with device_recorders = 1: the
    files have the layout of a device_recorders = 0 run and its values to the parity bar (two solver runs are not
    bit-reproducible: module docstring), and are within 1e-9 of the reference's own."""
    g = H.load("c1_planes")
    box = host.Box(H.C1_NX, H.C1_NY, H.C1_NZ, H.C1_H, 1e-3, 5.0)
    lonc, latc = g["surface_corners_lon_lat"][:, 0], g["surface_corners_lon_lat"][:, 1]
    planes = []
    for spec in g["plane_specs"]:
        lat, lon, depth, ds, ns, dd, nd, strike, dip = spec
        x, y = host.domain_coords(lon, lat, lonc, latc, g["domain_xyz"][0], g["domain_xyz"][1])
        pts = host.plane_points((x, y, depth), ds, int(ns), dd, int(nd), strike, dip)
        ids, phi, mine = box.stations(pts)
        assert mine.all()
        planes.append((ids, phi))
    ff = tmp_path / "force_process.0"
    host.forcefile_write(str(ff), g["loaded_lnid"], g["forces"])
    nsteps = int(round(float(g["end_time"]) / float(g["dt"])))
    for dev in (0, 1):
        d = tmp_path / ("dev%d" % dev)
        d.mkdir()
        s = box.create_solver()
        rp = box.run_params(loaded=g["loaded_lnid"], force_file=str(ff), source_window=64, planes=planes,
                            plane_rate=int(g["plane_rate"]), plane_dir=str(d), device_recorders=dev)
        box.solver_run(s, rp, 0, 150)            # in two calls: the second one appends
        box.solver_run(s, rp, 150, nsteps - 150)
        s.close()
    for i, (ids, _) in enumerate(planes):
        a = (tmp_path / "dev0" / ("planedisplacements.%d" % i)).read_bytes()
        b = (tmp_path / "dev1" / ("planedisplacements.%d" % i)).read_bytes()
        assert len(a) > 0 and len(a) == len(b)
        got = np.frombuffer(b, "<f8").reshape(-1, len(ids), 3)
        ref = g["plane%d" % i]
        assert got.shape == ref.shape
        assert H.rel_linf(got, ref) < TOL
        assert H.rel_linf(got, np.frombuffer(a, "<f8").reshape(got.shape)) < TOL     # two solver runs: module docstring
    box.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the f32 library
# ---------------------------------------------------------------------------------------------------------------------

def test_f32_library_records_doubles_of_the_widened_floats(c1):
    """libhq_solver_f32.so keeps the state in floats; the recorder widens every value to double BEFORE the sums, so its
    samples are the host kinematics of the hq_gather3 floats widened to double, bit for bit."""
    _cadence(c1, "f32")


# ---------------------------------------------------------------------------------------------------------------------
# 8. all four outputs at once, on every route
# ---------------------------------------------------------------------------------------------------------------------

def test_all_outputs_on_every_route(tmp_path):
    """The C1 box driven by the reference's force file with every output of the runner asked for at once -- stations
    (with velocities and accelerations) every 2 steps, planes every 3, both 4D files every 4, checkpoints every 5 -- over
    24 steps in a call of 7 and a call of 17, on identical solvers: device_recorders 0 / 1 x hqh_solver_run_on /
    hqh_solver_run_async(slots = 1).  Every route hands on the same steps in the same order; the values are those of the
    synchronous host route to the bars the tests of each output apply (two solver runs: module docstring), the 4D and
    checkpoint headers byte for byte; and no route leaves a recorder or a snapshot on its solver."""
    from tests.test_gpu_snapshots import TOL as SNAP_TOL, _checkpoint, _payload
    g, gp = H.load("c1_wavefield"), H.load("c1_planes")
    box = host.Box(H.C1_NX, H.C1_NY, H.C1_NZ, H.C1_H, 1e-3, 5.0)
    N, E = box.info["nharbored"], box.info["lenum"]
    ff = tmp_path / "force_process.0"
    host.forcefile_write(str(ff), g["loaded_lnid"], g["forces"])
    st_ids, st_phi, mine = box.stations(H.C1_STATIONS)
    assert mine.all()
    lonc, latc = gp["surface_corners_lon_lat"][:, 0], gp["surface_corners_lon_lat"][:, 1]
    planes = []
    for lat, lon, depth, ds, ns, dd, nd, strike, dip in gp["plane_specs"]:
        x, y = host.domain_coords(lon, lat, lonc, latc, gp["domain_xyz"][0], gp["domain_xyz"][1])
        ids, phi, mine = box.stations(host.plane_points((x, y, depth), ds, int(ns), dd, int(nd), strike, dip))
        assert mine.all()
        planes.append((ids, phi))
    made = {}
    for q, name in (("disp", "displacement"), ("vel", "velocity")):
        made[q] = str(tmp_path / (q + ".h4d"))
        host.wavefield_create(made[q], name, N, E, (1000.0, 1000.0, 500.0), 1000.0 / 2 ** 30, 1e-3, 4, 24)
    routes = [(dev, runner) for runner in ("sync", "async") for dev in (0, 1)]
    calls, dirs, nbytes = {}, {}, {}
    for route in routes:
        dev, runner = route
        d = tmp_path / ("%s%d" % (runner, dev))
        d.mkdir()
        dirs[route], calls[route] = d, []
        for q in made:
            shutil.copy(made[q], str(d / (q + ".h4d")))
        s = box.create_solver()
        rp = box.run_params(loaded=g["loaded_lnid"], force_file=str(ff), source_window=8, device_recorders=dev,
                            station_ids=st_ids, station_phi=st_phi, station_rate=2, station_derivs=2,
                            station_fn=lambda step, vals, route=route: calls[route].append((step, vals)),
                            planes=planes, plane_rate=3, plane_dir=str(d),
                            wavefield_rate=4, wavefield_disp_file=str(d / "disp.h4d"), wavefield_vel_file=str(d / "vel.h4d"),
                            wavefield_total_nodes=N, checkpoint_rate=5, checkpoint_dir=str(d))
        for step0, nsteps in ((0, 7), (7, 17)):
            assert s.info()["step"] == step0
            if runner == "sync":
                box.solver_run(s, rp, step0, nsteps)
            else:
                box.solver_run_async(s, rp, step0, nsteps, slots=1)
        assert s.info()["step"] == 24
        nbytes[route] = s.info()["device_bytes"]
        with pytest.raises(ha.HqError):
            s.record_pending(0)                          # the runner left no recorder behind
        with pytest.raises(ha.HqError):
            s.snapshot_pending(0)                        # ... and no snapshot
        s.close()
    box.close()
    base = (0, "sync")
    want = np.array([c[1] for c in calls[base]])
    assert want.shape == (12, 5, 9) and np.abs(want).max() > 0
    for route in routes:
        assert nbytes[route] == nbytes[base], route
        # stations: the callback's steps, then its values per column group
        assert [c[0] for c in calls[route]] == list(range(0, 24, 2)), route
        got = np.array([c[1] for c in calls[route]])
        for k in range(3):
            err = H.rel_linf(got[:, :, 3 * k:3 * k + 3], want[:, :, 3 * k:3 * k + 3])
            print("%s stations, column group %d: %.3e" % (route, k, err))
            assert err < TOL
        # planes: eight records (steps 0, 3, ..., 21) in every file, the second call's appended to the first's
        for i, (ids, _) in enumerate(planes):
            a = (dirs[base] / ("planedisplacements.%d" % i)).read_bytes()
            b = (dirs[route] / ("planedisplacements.%d" % i)).read_bytes()
            assert len(a) == len(b) == 8 * len(ids) * 24, (route, i)
            err = H.rel_linf(np.frombuffer(b, "<f8"), np.frombuffer(a, "<f8"))
            print("%s plane %d: %.3e" % (route, i, err))
            assert err < TOL
        # 4D files: the created header untouched, six output steps (0, 4, ..., 20)
        for q in made:
            ha_, a = _payload(str(dirs[base] / (q + ".h4d")), N)
            hb_, b = _payload(str(dirs[route] / (q + ".h4d")), N)
            assert ha_ == hb_ == open(made[q], "rb").read()[:136]
            assert a.shape == b.shape == (6, N, 3) and np.abs(a[1:]).max() > 0
            for k in range(6):
                err = H.rel_linf(b[k], a[k]) if np.abs(a[k]).max() > 0 else float(np.abs(b[k]).max())
                print("%s %s output step %d: %.3e" % (route, q, k, err))
                assert err < SNAP_TOL
        # checkpoints: the second call wrote steps 10, 15, 20 into .out0, .out1, .out0 (the first one step 5 into .out0)
        for n, step in (("checkpoint.out0", 20), ("checkpoint.out1", 15)):
            sa, sb = _checkpoint(str(dirs[base] / n), N), _checkpoint(str(dirs[route] / n), N)
            assert sa[0] == sb[0] and list(np.frombuffer(sb[0], "<i4")) == [1, step, N], (route, n)
            assert H.rel_linf(sb[1], sa[1]) < SNAP_TOL and H.rel_linf(sb[2], sa[2]) < SNAP_TOL
