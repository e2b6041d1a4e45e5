"""Asynchronous field snapshots (hq_snapshot_add / _pending / _fetch / _clear, include/hq_solver.h; hqh_solver_run_async,
include/hq_host.h): what the 4D output and the checkpoints read at the top of the loop body (psolve.c:4277-4278), copied out
by hq_k_snapshot in octor order and carried to pinned host memory beside the steps.

The yardstick everywhere is hq_download ON THE SAME SOLVER: a snapshot of step s must be the very arrays hq_download would
have returned at the head of step s, bit for bit (np.array_equal), and its velocity the numpy expression
(tm1.astype(f64) - tm2.astype(f64)) / dt of them, bit for bit.  Where the steps run in one batch -- which is what is to be
tested -- hq_download cannot be called in between, and an auxiliary unit-weight recorder (tests/test_gpu_recorders.py's
device: weights (1, 0, ..., 0) record the node's row exactly) supplies the rows of the SAME batch.  Two separately run
solvers are not bit-reproducible here (fp64 LDS atomics in the element-form patches, see that module's docstring); they
are compared with the project's parity bar, 1e-9 relative L-inf.

One case of the issue had to be mended.  It asks for a snapshot with rate 1, first_step 7 and ONE slot, then run(5) -- but
with rate 1 all five steps are due, and the room check the same issue specifies refuses that call before anything is
enqueued.  Both halves are kept: the rate-1 call IS refused (asserted), and the snapshot that is then compared has rate 7,
so that of the steps 7..11 only step 7 is due and the five steps do rewrite all three state buffers behind it; the overflow
is then provoked with run(3), whose last step, 14, is the next due one."""
import ctypes
import shutil

import numpy as np
import pytest

import hercules_amd as ha
from hercules_amd import capi, host
from tests import helpers as H

pytestmark = pytest.mark.gpu

TOL = 1e-9
ALL = capi.HQ_SNAP_TM1 | capi.HQ_SNAP_TM2 | capi.HQ_SNAP_VEL
BOTH = capi.HQ_SNAP_TM1 | capi.HQ_SNAP_TM2


@pytest.fixture(params=["bricks", "patches-only"])
def brick_mode(request, monkeypatch):
    """As shipped (hq_k_brick takes the simple nodes of uniform regions) and with HQ_NO_BRICKS=1 (patches everywhere)."""
    if request.param == "patches-only":
        monkeypatch.setenv("HQ_NO_BRICKS", "1")
    else:
        monkeypatch.delenv("HQ_NO_BRICKS", raising=False)
    return request.param


def _field_at(ijk, nx, ny, seed, amp=1e-3):
    """tests/test_gpu_recorders.py's _field: a start field that is a function of the node's GLOBAL grid position, so the
    same on every partition that harbors it; no value is zero."""
    ijk = np.asarray(ijk).astype(np.int64)
    gid = (ijk[:, 2] * (ny + 1) + ijk[:, 1]) * (nx + 1) + ijk[:, 0]
    u = np.empty((len(gid), 3))
    for d in range(3):
        x = (gid * 3 + d + seed) * np.int64(2654435761) % np.int64(2 ** 31)
        u[:, d] = (x.astype(np.float64) / 2 ** 30 - 1.0) * amp
    return u


def _field(box, seed, amp=1e-3):
    return _field_at(box.node_ijk, box.nx, box.ny, seed, amp)


def _unit_points(nodes):
    flat = np.asarray(nodes, np.int32).reshape(-1)
    phi = np.zeros((len(flat), 8))
    phi[:, 0] = 1.0
    return np.repeat(flat[:, None], 8, axis=1), phi


def _add_rows_recorder(s, nodes, capacity):
    uid, uphi = _unit_points(nodes)
    return s.record_add(uid, uphi, rate=1, derivs=0, capacity=capacity)


def _vel(d1, d2, dt):
    """write_velocity's arithmetic as hqh_wavefield_write states it, in numpy."""
    return (d1.astype(np.float64) - d2.astype(np.float64)) / dt


@pytest.fixture(scope="module")
def c1():
    box = host.Box(H.C1_NX, H.C1_NY, H.C1_NZ, H.C1_H, 1e-3, 5.0)
    loaded, pattern = box.point_source(500.0, 500.0, 100.0, 0.0, 90.0, 0.0)
    rp = box.run_params(loaded=loaded, pattern=pattern, moment=1e15, rise_time=0.02, source_window=64)
    F = box.source_table(rp, 0, 64)
    u = _field(box, 5)
    yield dict(box=box, loaded=loaded, F=F, u1=u, u2=0.999 * u, dt=1e-3)
    box.close()


def _c1_solver(c1, precision="f64", variant=ha.HQ_VARIANT_AUTO):
    s = c1["box"].create_solver(tm1=c1["u1"], tm2=c1["u2"], precision=precision, variant=variant)
    s.set_source(c1["loaded"], c1["F"])
    return s


# ---------------------------------------------------------------------------------------------------------------------
# 1. / 2. a snapshot equals the download
# ---------------------------------------------------------------------------------------------------------------------

def _snapshot_equals_the_download(s, dt):
    s.run(7)
    d1, d2 = s.download()
    assert d1.dtype == s.real and np.abs(d1).max() > 0 and not np.array_equal(d1, d2)
    # the issue's literal case: rate 1 and one slot cannot hold the five due steps of run(5) -- refused, nothing enqueued
    h1 = s.snapshot_add(fields=ALL, rate=1, first_step=7, slots=1)
    with pytest.raises(ha.HqError):
        s.run(5)
    assert s.info()["step"] == 7 and s.snapshot_pending(h1) == (0, 0, -1)
    s.snapshot_clear()
    h = s.snapshot_add(fields=ALL, rate=7, first_step=7, slots=1)          # (module docstring: the mended case)
    assert h != h1
    s.run(5)                             # now, prev and spare are all rewritten behind the snapshot of step 7
    assert s.snapshot_pending(h)[0::2] == (1, 7)
    with pytest.raises(ha.HqError):      # step 14 is due and the slot is still occupied
        s.run(3)
    assert s.info()["step"] == 12
    step, tm1, tm2, vel = s.snapshot_fetch(h)
    e1, e2 = s.download()
    assert step == 7
    assert tm1.dtype == s.real and tm2.dtype == s.real and vel.dtype == np.float64
    assert not np.array_equal(e1, d1) and not np.array_equal(e2, d2)       # (the state has moved on)
    assert np.array_equal(tm1, d1) and np.array_equal(tm2, d2)
    assert np.array_equal(vel, _vel(d1, d2, dt)) and np.abs(vel).max() > 0
    s.run(3)                             # the slot is free again: step 14 is taken
    assert s.snapshot_pending(h)[0::2] == (1, 14)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_snapshot_equals_the_download(c1, brick_mode, precision):
    s = _c1_solver(c1, precision)
    info = s.info()
    print("C1 box, %s, %s: brick units %d, patches %d" % (brick_mode, precision, info["brick_units"], info["npatches"]))
    assert brick_mode == "bricks" or info["brick_units"] == 0
    _snapshot_equals_the_download(s, c1["dt"])
    s.close()


def test_snapshot_equals_the_download_in_the_scatter_variant(c1):
    s = _c1_solver(c1, variant=ha.HQ_VARIANT_SCATTER)
    assert s.info()["variant"] == ha.HQ_VARIANT_SCATTER
    _snapshot_equals_the_download(s, c1["dt"])
    s.close()


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_snapshot_equals_the_download_with_hanging_nodes(brick_mode, precision):
    """The smallest two-level box the GPU parity tests build (16 x 8, 6 fine layers over 3 coarse ones): hanging nodes, a
    renumbering that is not the identity wherever there are bricks, patches along the level interface."""
    nx, ny = 16, 8
    ob = host.OctBox(nx, ny, 6, 3, 31.25, 1e-3, 5.0)
    u = _field_at(ob.node_xyz, nx, ny, 9)
    s = ob.create_solver(tm1=u, tm2=0.999 * u, precision=precision)
    info = s.info()
    print("two-level box: %d nodes, %d hanging, brick units %d, patches %d" % (ob.N, ob.ldnnum, info["brick_units"], info["npatches"]))
    assert ob.ldnnum > 0
    _snapshot_equals_the_download(s, 1e-3)
    s.close(); ob.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the ordering hazard
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
    nodes = ids.reshape(-1)                               # 512: the 8 corner elements', the centre element's, random ones
    loaded, pattern = box.point_source(L[0] / 2, L[1] / 2, L[2] / 2, 30.0, 70.0, 10.0)
    rp = box.run_params(loaded=loaded, pattern=pattern, moment=1e13, rise_time=20 * dt, source_window=64)
    F = box.source_table(rp, 0, 40)
    u = _field(box, 77)
    yield dict(box=box, nodes=nodes, loaded=loaded, F=F, u1=u, u2=0.999 * u, dt=dt)
    box.close()


@pytest.mark.parametrize("brick_stream", [1, 0])
def test_snapshots_inside_one_batch_are_those_of_their_steps(big_box, brick_mode, brick_stream):
    """Rate 4, 10 slots, 40 steps in ONE hq_run, the bricks on a stream of their own or not: every snapshot's tm1 rows at
    512 nodes are the auxiliary recorder's sample of that step of the same batch, its tm2 rows the sample of the step
    before, bit for bit; whole fields against an identical solver that is stopped and downloaded at those steps to the
    parity bar; and a second snapshot of a range that is no multiple of a wave or a workgroup equals the slice."""
    b = big_box
    nodes = b["nodes"]
    opts = {"brick_stream": brick_stream}
    s = b["box"].create_solver(tm1=b["u1"], tm2=b["u2"], options=opts)
    s.set_source(b["loaded"], b["F"])
    h = s.snapshot_add(fields=BOTH, rate=4, slots=10)
    hp = s.snapshot_add(first=1001, count=4099, fields=ALL, rate=4, slots=10)
    hr = _add_rows_recorder(s, nodes, 40)
    s.run(40)
    assert s.snapshot_pending(h)[0::2] == (10, 0) and s.snapshot_pending(hp)[0::2] == (10, 0)
    info = s.info()                                      # (the bricks' stream is made at the first step)
    if brick_mode == "bricks":
        assert info["brick_units"] > 0 and info["brick_stream"] == brick_stream
    else:
        assert info["brick_units"] == 0
    rsteps, rows = s.record_fetch(hr)                    # [40, 512, 3]
    assert np.array_equal(rsteps, np.arange(40))
    snaps = []
    for k in range(0, 40, 4):
        step, tm1, tm2, vel = s.snapshot_fetch(h)
        assert step == k and vel is None
        assert np.array_equal(tm1[nodes], rows[k])
        assert np.array_equal(tm2[nodes], rows[k - 1] if k else np.asarray(b["u2"])[nodes])
        pstep, p1, p2, pv = s.snapshot_fetch(hp)
        assert pstep == k and p1.shape == (4099, 3)
        assert np.array_equal(p1, tm1[1001:5100]) and np.array_equal(p2, tm2[1001:5100])
        assert np.array_equal(pv, _vel(tm1[1001:5100], tm2[1001:5100], b["dt"]))
        snaps.append((tm1, tm2))
    assert s.snapshot_fetch(h)[0] == -1 and s.snapshot_fetch(hp)[0] == -1
    s.close()
    assert np.abs(snaps[-1][0] - snaps[0][0]).max() > 0
    r = b["box"].create_solver(tm1=b["u1"], tm2=b["u2"], options=opts)
    r.set_source(b["loaded"], b["F"])
    for k, (tm1, tm2) in zip(range(0, 40, 4), snaps):
        d1, d2 = r.download()
        assert H.rel_linf(tm1, d1) < TOL and H.rel_linf(tm2, d2) < TOL, k
        r.run(4)
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. two partitions in one process
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("overlap", [0, 1])
def test_two_partitions_snapshot_through_group_run(brick_mode, overlap):
    """Two partitions of a 32 x 32 x 16 box (hq_group_link), the exchange chain on a stream of its own or not: each rank
    snapshots every fifth step, 6 slots, 30 steps in one hq_group_run; the rows at the SHARED nodes -- the ones the chain
    writes -- are the auxiliary recorders' of the same batch, bit for bit."""
    nx, ny, nz, h, dt = 32, 32, 16, 15.0, 3e-4
    boxes = [host.Box(nx, ny, nz, h, dt, 30.0, rank=r, nranks=2) for r in range(2)]
    shared = []
    for bx in boxes:
        sch = bx.schedule()
        sh = np.unique(np.concatenate([m for _, m in sch["c"] + sch["s"]]))
        assert len(sh) > 0
        shared.append(sh)
    fields = [_field(bx, 31) for bx in boxes]
    solvers = [bx.create_solver(tm1=u, tm2=0.999 * u, options={"overlap": overlap}) for bx, u in zip(boxes, fields)]
    capi.group_link(solvers)
    hs = [s.snapshot_add(fields=BOTH, rate=5, slots=6) for s in solvers]
    hrs = [_add_rows_recorder(s, sh, 64) for s, sh in zip(solvers, shared)]
    capi.group_run(solvers, 30)
    for s, hd, hr, sh, u in zip(solvers, hs, hrs, shared, fields):
        assert s.snapshot_pending(hd) == (6, 6, 0)       # (group_run syncs every member)
        rsteps, rows = s.record_fetch(hr)
        assert np.array_equal(rsteps, np.arange(30))
        for k in range(0, 30, 5):
            step, tm1, tm2, _ = s.snapshot_fetch(hd)
            assert step == k
            assert np.array_equal(tm1[sh], rows[k])
            assert np.array_equal(tm2[sh], rows[k - 1] if k else (0.999 * u)[sh])
        assert np.abs(rows[29] - rows[0]).max() > 0
    with pytest.raises(ha.HqError):                      # steps 30 .. 60: 7 due, 6 slots free
        capi.group_run(solvers, 31)
    assert [s.info()["step"] for s in solvers] == [30, 30]
    for s in solvers:
        s.close()
    for bx in boxes:
        bx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. ring and errors on the C1 box
# ---------------------------------------------------------------------------------------------------------------------

def test_ring_order_and_pending_counts(c1, brick_mode):
    s = _c1_solver(c1)
    h = s.snapshot_add(fields=BOTH, rate=2, slots=4)
    assert s.snapshot_pending(h) == (0, 0, -1) and s.snapshot_fetch(h) == (-1, None, None, None)
    s.run(7)                                             # un-synced: steps 0, 2, 4, 6 are taken or enqueued
    n, ready, first = s.snapshot_pending(h)
    assert (n, first) == (4, 0) and 0 <= ready <= 4
    with pytest.raises(ha.HqError):
        s.run(2)                                         # step 8 is due, no slot is free
    assert s.info()["step"] == 7
    s.sync()
    assert s.snapshot_pending(h) == (4, 4, 0)
    got = [s.snapshot_fetch(h)[0] for _ in range(2)]
    assert got == [0, 2] and s.snapshot_pending(h) == (2, 2, 4)
    s.run(4)                                             # the ring wraps: steps 8, 10 into the freed slots
    got += [s.snapshot_fetch(h)[0] for _ in range(5)]
    assert got == [0, 2, 4, 6, 8, 10, -1] and s.info()["step"] == 11
    s.close()


def test_bad_descriptions_are_refused(c1):
    s = _c1_solver(c1)
    N = s.N
    bytes0 = s.info()["device_bytes"]
    for kw in (dict(first=-1, count=4), dict(first=N - 3, count=4), dict(first=N, count=1), dict(count=0), dict(count=-5),
               dict(rate=0), dict(rate=-2), dict(slots=0), dict(slots=-1), dict(fields=0), dict(fields=8), dict(fields=ALL | 16)):
        with pytest.raises(ha.HqError):
            s.snapshot_add(**kw)
    lib, hd = s._lib, ctypes.c_int32()
    d = capi._SnapshotDesc(0, N, 1, 0, BOTH, 1)
    assert lib.hq_snapshot_add(s._h, None, ctypes.byref(hd)) == -1 and lib.hq_snapshot_add(s._h, ctypes.byref(d), None) == -1
    assert s.info()["device_bytes"] == bytes0            # a refused add keeps nothing
    with pytest.raises(ha.HqError):
        s.snapshot_pending(0)                            # nothing was added: an unknown handle
    step = ctypes.c_int32(5)
    assert lib.hq_snapshot_fetch(s._h, ctypes.c_int32(0), None, None, None, ctypes.byref(step)) == -1
    h = s.snapshot_add(fields=capi.HQ_SNAP_TM1, slots=2)
    assert s.info()["device_bytes"] >= bytes0 + 2 * N * 24
    s.run(1)
    buf = np.empty((N, 3))
    p = buf.ctypes.data_as(ctypes.c_void_p)
    for args in ((None, p, None), (None, None, p), (p, p, p)):            # an output pointer for a field it lacks
        assert lib.hq_snapshot_fetch(s._h, ctypes.c_int32(h), args[0], args[1], args[2], ctypes.byref(step)) == -1
    assert lib.hq_snapshot_fetch(s._h, ctypes.c_int32(h), p, None, None, None) == -1
    assert lib.hq_snapshot_pending(s._h, ctypes.c_int32(h), None, None, None) == -1
    assert s.snapshot_pending(h)[0::2] == (1, 0)         # none of the refused calls consumed it
    assert lib.hq_snapshot_fetch(s._h, ctypes.c_int32(h), None, None, None, ctypes.byref(step)) == 0 and step.value == 0
    assert s.snapshot_pending(h) == (0, 0, -1)           # NULL for a field it has: allowed, the slot is freed
    s.close()


def test_upload_keeps_and_clear_drops(c1, brick_mode):
    s = _c1_solver(c1)
    bytes0 = s.info()["device_bytes"]
    h = s.snapshot_add(fields=ALL, rate=2, slots=6)
    s.run(3)                                             # steps 0 and 2 stay pending across the upload
    d1, d2 = s.download()
    s.upload(d1 * 0.5, d2 * 0.25, 250)
    assert s.snapshot_pending(h)[0::2] == (2, 0)
    s.run(3)                                             # 250, 252
    got = [s.snapshot_fetch(h) for _ in range(4)]
    assert [g[0] for g in got] == [0, 2, 250, 252]
    assert np.array_equal(got[0][1], np.asarray(c1["u1"])) and np.array_equal(got[0][2], np.asarray(c1["u2"]))
    assert np.array_equal(got[2][1], d1 * 0.5) and np.array_equal(got[2][2], d2 * 0.25)
    assert np.array_equal(got[2][3], _vel(d1 * 0.5, d2 * 0.25, c1["dt"]))
    s.run(2)                                             # 254 pending when everything is dropped
    assert s.snapshot_pending(h)[0::2] == (1, 254)
    s.snapshot_clear()
    assert s.info()["device_bytes"] == bytes0
    with pytest.raises(ha.HqError):
        s.snapshot_pending(h)
    with pytest.raises(ha.HqError):
        s.snapshot_fetch(h)
    s.run(10)                                            # takes nothing, overflows nothing
    h2 = s.snapshot_add(slots=1)
    assert h2 != h and s.snapshot_pending(h2) == (0, 0, -1)
    s.snapshot_clear()
    s.snapshot_clear()                                   # nothing to drop: no error
    s.close()


def test_fetching_without_a_sync_does_not_disturb_the_run(c1, brick_mode):
    """hq_snapshot_fetch right behind an asynchronous hq_run -- it waits for its own slot's copy only -- and further runs
    behind it: every snapshot is the plain solver's download of its step and the final field is that of a solver that
    never snapshotted, to the parity bar."""
    s = _c1_solver(c1)
    h = s.snapshot_add(fields=BOTH, rate=10, slots=2)
    got = []
    for _ in range(3):
        s.run(20)
        got += [s.snapshot_fetch(h) for _ in range(2)]   # no sync in between
    assert [g[0] for g in got] == [0, 10, 20, 30, 40, 50]
    a1, a2 = s.download()
    s.close()
    r = _c1_solver(c1)
    for g in got:
        d1, d2 = r.download()
        assert H.rel_linf(g[1], d1) < TOL and H.rel_linf(g[2], d2) < TOL, g[0]
        r.run(10)
    b1, b2 = r.download()
    r.close()
    assert H.rel_linf(a1, b1) < TOL and H.rel_linf(a2, b2) < TOL


# ---------------------------------------------------------------------------------------------------------------------
# 6. the runner
# ---------------------------------------------------------------------------------------------------------------------

def _payload(path, N):
    raw = open(path, "rb").read()
    return raw[:136], np.frombuffer(raw[136:], "<f8").reshape(-1, N, 3)


def _checkpoint(path, N):
    raw = open(path, "rb").read()
    assert len(raw) == 12 + 2 * N * 24
    return raw[:12], np.frombuffer(raw[12:12 + N * 24], "<f8").reshape(N, 3), np.frombuffer(raw[12 + N * 24:], "<f8").reshape(N, 3)


def test_async_runner_writes_the_files_of_the_synchronous_one(tmp_path):
    """The C1 box driven by the reference's force file, checkpoints every 20 steps, both 4D files every 15:
    hqh_solver_run_async(slots = 2) against hqh_solver_run_on on an identical solver, 60 steps and then 30 more in a
    second call.  The 4D files start as copies of ONE created file each, so the 136-byte headers must come out
    byte-identical; payloads to the parity bar per quantity (two solver runs)."""
    g = H.load("c1_wavefield")
    box = host.Box(H.C1_NX, H.C1_NY, H.C1_NZ, H.C1_H, 1e-3, 5.0)
    N, E = box.info["nharbored"], box.info["lenum"]
    ff = tmp_path / "force_process.0"
    host.forcefile_write(str(ff), g["loaded_lnid"], g["forces"])
    made = {}
    for q, name in (("disp", "displacement"), ("vel", "velocity")):
        made[q] = str(tmp_path / (q + ".h4d"))
        host.wavefield_create(made[q], name, N, E, (1000.0, 1000.0, 500.0), 1000.0 / 2 ** 30, 1e-3, 15, 90)
    final, dirs = {}, {}
    for route in ("sync", "async"):
        d = tmp_path / route
        d.mkdir()
        dirs[route] = d
        paths = {q: str(d / (q + ".h4d")) for q in made}
        for q in made:
            shutil.copy(made[q], paths[q])
        s = box.create_solver()
        rp = box.run_params(loaded=g["loaded_lnid"], force_file=str(ff), source_window=64, wavefield_rate=15,
                            wavefield_disp_file=paths["disp"], wavefield_vel_file=paths["vel"], wavefield_total_nodes=N,
                            checkpoint_rate=20, checkpoint_dir=str(d))
        if route == "sync":
            box.solver_run(s, rp, 0, 60)
            box.solver_run(s, rp, 60, 30)
            bytes0 = s.info()["device_bytes"]            # (the context and the source tables both routes upload)
        else:
            box.solver_run_async(s, rp, 0, 60, slots=2)
            assert s.info()["step"] == 60 and s.info()["device_bytes"] == bytes0
            mid = {n: _checkpoint(str(d / n), N) for n in ("checkpoint.out0", "checkpoint.out1")}
            assert [int(np.frombuffer(mid[n][0], "<i4")[1]) for n in sorted(mid)] == [20, 40]
            with pytest.raises(ha.HqError):
                s.snapshot_pending(0)                    # the runner left no snapshot behind
            assert s.snapshot_clear() is None            # ... nothing to drop, no error
            with pytest.raises(ha.HqError):              # step0 must be the context's own counter
                box.solver_run_async(s, rp, 59, 1, slots=2)
            box.solver_run_async(s, rp, 60, 30, slots=1)
            assert s.info()["step"] == 90 and s.info()["device_bytes"] == bytes0
        final[route] = s.download()
        s.close()
    for q in made:
        ha_, a = _payload(str(dirs["sync"] / (q + ".h4d")), N)
        hb_, b = _payload(str(dirs["async"] / (q + ".h4d")), N)
        assert ha_ == hb_ == open(made[q], "rb").read()[:136]
        assert a.shape == b.shape == (6, N, 3) and np.abs(a[1:]).max() > 0
        for k in range(6):
            err = H.rel_linf(b[k], a[k]) if np.abs(a[k]).max() > 0 else float(np.abs(b[k]).max())
            print("%s output step %d: async vs sync %.3e" % (q, k, err))
            assert err < TOL
    # the second call wrote step 80 into checkpoint.out0 on both routes; step 40 is still in checkpoint.out1
    for n, step in (("checkpoint.out0", 80), ("checkpoint.out1", 40)):
        sa, sb = _checkpoint(str(dirs["sync"] / n), N), _checkpoint(str(dirs["async"] / n), N)
        assert sa[0] == sb[0] and list(np.frombuffer(sb[0], "<i4")) == [1, step, N]
        assert H.rel_linf(sb[1], sa[1]) < TOL and H.rel_linf(sb[2], sa[2]) < TOL
    assert H.rel_linf(final["async"][0], final["sync"][0]) < TOL and H.rel_linf(final["async"][1], final["sync"][1]) < TOL
    # hqh_checkpoint_read of an async checkpoint restores a solver that continues to the same bar
    s = box.create_solver()
    assert host.checkpoint_read(s, str(dirs["async"] / "checkpoint.out1")) == 40 and s.info()["step"] == 40
    rp = box.run_params(loaded=g["loaded_lnid"], force_file=str(ff), source_window=64)
    box.solver_run(s, rp, 40, 50)
    c1_, c2_ = s.download()
    s.close(); box.close()
    assert H.rel_linf(c1_, final["async"][0]) < TOL and H.rel_linf(c2_, final["async"][1]) < TOL


def test_async_runner_against_the_references_4d_files(tmp_path):
    """tests/golden/c1_wavefield holds the reference's own disp.h4d / vel.h4d for 349 steps at rate 100: the asynchronous
    runner at that cadence meets the bars test_4d_wavefield_files_written_by_the_c_solver_run applies to the synchronous
    one (1e-9 for displacements, 1e-7 for velocities: a difference of two fields over dt)."""
    g = H.load("c1_wavefield")
    box = host.Box(H.C1_NX, H.C1_NY, H.C1_NZ, H.C1_H, 1e-3, 5.0)
    N, E = box.info["nharbored"], box.info["lenum"]
    ff = tmp_path / "force_process.0"
    host.forcefile_write(str(ff), g["loaded_lnid"], g["forces"])
    paths = {q: str(tmp_path / (q + ".h4d")) for q in ("disp", "vel")}
    for q, name in (("disp", "displacement"), ("vel", "velocity")):
        host.wavefield_create(paths[q], name, N, E, (1000.0, 1000.0, 500.0), 1000.0 / 2 ** 30, 1e-3, 100, 349)
    s = box.create_solver()
    rp = box.run_params(loaded=g["loaded_lnid"], force_file=str(ff), source_window=64, wavefield_rate=100,
                        wavefield_disp_file=paths["disp"], wavefield_vel_file=paths["vel"], wavefield_total_nodes=N)
    box.solver_run_async(s, rp, 0, 120, slots=2)
    box.solver_run_async(s, rp, 120, 229, slots=2)      # 349 steps in all, as the reference ran
    for q in ("disp", "vel"):
        ref, ours = g[q + "_np1"].tobytes(), open(paths[q], "rb").read()
        assert len(ours) == len(ref)
        assert ours[:32] == ref[:32] and ours[48:128] == ref[48:128]
        a = np.frombuffer(ours[136:], "<f8").reshape(4, N, 3)
        b = np.frombuffer(ref[136:], "<f8").reshape(4, N, 3)
        assert not a[0].any() and not b[0].any()
        for k in range(1, 4):
            assert H.rel_linf(a[k], b[k]) < (TOL if q == "disp" else 1e-7)
    s.close(); box.close()


def test_async_runner_against_the_references_checkpoints(tmp_path):
    """tests/golden/c1_short holds the reference's checkpoints of steps 400 and 800: the asynchronous runner at that
    cadence meets test_checkpoints_at_the_references_cadence's bar."""
    g = H.load("c1_short")
    N = H.c1_problem()["N"]
    ff = tmp_path / "force_process.0"
    host.forcefile_write(str(ff), g["loaded_lnid"], g["forces"])
    box = host.Box(H.C1_NX, H.C1_NY, H.C1_NZ, H.C1_H, 1e-3, 5.0)
    s = box.create_solver()
    rp = box.run_params(loaded=g["loaded_lnid"], force_file=str(ff), source_window=128, checkpoint_rate=400,
                        checkpoint_dir=str(tmp_path))
    box.solver_run_async(s, rp, 0, 1000, slots=1)
    s.close(); box.close()
    assert list(g["ckpt_steps"]) == [400, 800]
    for k, name in enumerate(("checkpoint.out0", "checkpoint.out1")):
        hdr, tm2, tm1 = _checkpoint(str(tmp_path / name), N)
        assert list(np.frombuffer(hdr, "<i4")) == [1, int(g["ckpt_steps"][k]), N]
        assert H.rel_linf(tm1, g["ckpt_tm1"][k]) < TOL and H.rel_linf(tm2, g["ckpt_tm2"][k]) < TOL
