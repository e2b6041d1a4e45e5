"""Deformation trackers (hq_deform_add / _fetch / _load / _reset / _clear, include/hq_solver.h): the running peaks of strain,
strain rate, stress, rotation and rotation rate hq_k_deform keeps per point on the device.

Row b of a tracker's displacement gradient is hq_k_record's sample with phi = grad[:, b, :], bit for bit, its rate gradient
that recorder's velocity column, and its fold is csrc/hq_deform.h, the text hqh_deform_fold compiles for the host.  So every
tracker here gets THREE RECORDER TWINS on the same context -- the same points, phi = grad[:, b, :], derivs = 1, the same rate,
room for the whole run -- and the expectation is np.array_equal between hq_deform_fetch and hqh_deform_fold of the twins'
samples, for vals, when and nsamples.  The comparison has to be made on ONE trajectory: two identically built solvers differ
in the last bits (tests/test_gpu_recorders.py tells why).  A recorder knows no first_step: samples of earlier steps are dropped
before the fold.

The fixture is the C1 box of tests/test_gpu_peaks.py and test_gpu_cumul.py, built here: 16 x 16 x 8, h = 62.5, dt = 1e-3, from
rest, a sin^2 push on the node (4, 5, 3) for 40 steps; 240 steps in batches of 7, 93 and 140.  The points: the 256 centres of
the top element layer and the 16 of row j = 0 of the layer below (272: two workgroups, the second one ragged), the five C1
stations (off-centre), one point, and no point at all."""
import ctypes

import numpy as np
import pytest

import hercules_amd as ha
from hercules_amd import capi, host
from oracle import herc_oracle as ho
from tests import helpers as H

pytestmark = pytest.mark.gpu

TOL = 1e-9
E, ER, S, W, WR = (capi.HQ_DEFORM_STRAIN, capi.HQ_DEFORM_STRAIN_RATE, capi.HQ_DEFORM_STRESS, capi.HQ_DEFORM_ROTATION,
                   capi.HQ_DEFORM_ROTATION_RATE)
ALL = capi.HQ_DEFORM_ALL
NSTEPS = 240
BATCHES = (7, 93, 140)
CADENCES = [(1, 0), (3, 6)]
SETS = ("map", "stations", "one", "none")


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
    """The box, its source, and per point set (ids [n, 8], grad [n, 3, 8], lame [n, 2])."""
    box = host.Box(H.C1_NX, H.C1_NY, H.C1_NZ, H.C1_H, 1e-3, 5.0)
    ijk = box.node_ijk
    loaded = np.nonzero((ijk[:, 0] == 4) & (ijk[:, 1] == 5) & (ijk[:, 2] == 3))[0].astype(np.int32)
    assert len(loaded) == 1
    k = np.arange(40)
    F = (np.sin(np.pi * k / 40) ** 2)[:, None, None] * 1e9 * np.array([1.0, 0.5, -0.7])[None, None, :]
    h = H.C1_H
    centres = [((i + 0.5) * h, (j + 0.5) * h, 0.5 * h) for j in range(H.C1_NY) for i in range(H.C1_NX)]
    centres += [((i + 0.5) * h, 0.5 * h, 1.5 * h) for i in range(H.C1_NX)]
    xyz = dict(map=np.array(centres), stations=np.array(H.C1_STATIONS), one=np.array([(430.0, 520.0, 170.0)]), none=np.zeros((0, 3)))
    assert len(xyz["map"]) == 272
    sets = {}
    for name, x in xyz.items():
        ids, grad, mine = box.station_gradients(x)
        assert mine.all()
        sets[name] = (ids, grad, box.station_moduli(x))
    assert (np.ptp(np.abs(sets["stations"][1]), axis=2) > 0).all()      # off-centre: an axis' eight weights differ in size
    yield dict(box=box, loaded=loaded, F=F, sets=sets, dt=1e-3)
    box.close()


def _solver(c1, precision="f64", variant=ha.HQ_VARIANT_AUTO):
    s = c1["box"].create_solver(precision=precision, variant=variant)
    s.set_source(c1["loaded"], c1["F"])
    return s


def _add_twins(s, ids, grad, rate, capacity):
    """Three recorders whose phi tables are the gradient weights of the three axes."""
    return [s.record_add(ids, np.ascontiguousarray(grad[:, b, :]), rate=rate, derivs=1, capacity=capacity) for b in range(3)]


def _fetch_twins(s, twins, npoints):
    """(steps [k], gsamples [k, np, 2, 3, 3]) of three twins: recorder b's columns 0..2 and 3..5 are rows b of G and of its rate."""
    got = [s.record_fetch(t) for t in twins]
    steps = got[0][0]
    assert all(np.array_equal(g[0], steps) for g in got)
    gs = np.zeros((len(steps), npoints, 2, 3, 3))
    for b, (_, v) in enumerate(got):
        gs[:, :, 0, b, :] = v[:, :, 0:3]
        gs[:, :, 1, b, :] = v[:, :, 3:6]
    return steps, gs


def _due(rate, first, upto=NSTEPS):
    return np.array([s for s in range(upto) if s >= first and s % rate == 0], np.int32)


def _fold(samples, q, lame, first_step=0, into=None):
    """hqh_deform_fold of the twins' (steps, gsamples) from first_step on -> (vals, when, samples folded)."""
    steps, gs = samples
    keep = steps >= first_step
    vals, when = host.deform_fold(steps[keep], gs[keep], q, lame if q & S else None, *(into or (None, None)))
    return vals, when, int(keep.sum())


def _same(got, want):
    assert got[2] == want[2], (got[2], want[2])
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape
    assert np.array_equal(got[1], want[1]), np.argwhere(got[1] != want[1])[:5]
    assert np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:5]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the C1 box from rest: against the twins
# ---------------------------------------------------------------------------------------------------------------------

def _c1_run(c1, precision, rate, first, variant=ha.HQ_VARIANT_AUTO):
    """One run -> per point set the fetches of a full-mask tracker with moduli and of a STRAIN_RATE tracker without, and the
    twins' samples."""
    s = _solver(c1, precision, variant)
    cap = NSTEPS // rate + 1
    hs = {}
    for name in SETS:
        ids, grad, lame = c1["sets"][name]
        hs[name] = (s.deform_add(ids, grad, lame, rate=rate, first_step=first, quantities=ALL),
                    s.deform_add(ids, grad, None, rate=rate, first_step=first, quantities=ER),
                    _add_twins(s, ids, grad, rate, cap) if len(ids) else None)
    for n in BATCHES:
        s.run(n)
    assert s.info()["step"] == NSTEPS
    out = {}
    for name, (h_all, h_rate, twins) in hs.items():
        npts = len(c1["sets"][name][0])
        out[name] = dict(all=s.deform_fetch(h_all), rate=s.deform_fetch(h_rate),
                         twin=_fetch_twins(s, twins, npts) if twins else (_due(rate, 0), np.zeros((len(_due(rate, 0)), 0, 2, 3, 3))))
    s.close()
    return out


def _check_run(c1, out, rate, first):
    ndue = len(_due(rate, first))
    for name in SETS:
        o, lame = out[name], c1["sets"][name][2]
        npts = len(lame)
        assert o["all"][0].shape == (npts, 40) and o["all"][1].shape == (npts, 10) and o["rate"][0].shape == (npts, 10)
        _same(o["all"], _fold(o["twin"], ALL, lame, first))
        _same(o["rate"], _fold(o["twin"], ER, None, first))
        assert o["all"][2] == ndue and o["rate"][2] == ndue
        assert np.array_equal(o["rate"][0], o["all"][0][:, 10:20]) and np.array_equal(o["rate"][1], o["all"][1][:, 2:4])
        if npts:
            assert (o["all"][0][:, [7, 17, 27, 34, 39]] > 0).all()       # the wave reached every point, in every block
            assert (o["all"][1] >= max(first, 1)).all()


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("rate,first", CADENCES)
def test_trackers_equal_their_recorder_twins(c1, brick_mode, precision, rate, first):
    """240 steps in batches of 7, 93 and 140; the full mask with the moduli of station_moduli, and STRAIN_RATE alone, which is
    given no moduli: every point set equals the fold of its three twins' samples bit for bit -- vals, when and the count."""
    _check_run(c1, _c1_run(c1, precision, rate, first), rate, first)


def test_the_scatter_variant_has_them_too(c1):
    """Only u(t) and u(t - dt) are read: the scatter variant, which keeps no u(t - 2 dt), takes the full mask."""
    _check_run(c1, _c1_run(c1, "f64", 3, 6, variant=ha.HQ_VARIANT_SCATTER), 3, 6)


# ---------------------------------------------------------------------------------------------------------------------
# 2. against the oracle
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def c1_oracle(c1):
    """The oracle's run, once: u at the head of every step at the nodes of the map's and the stations' elements -> per set the
    displacement gradient and its rate at every step, [NSTEPS, np, 2, 3, 3] (the fields before step 0 are zero), and U, the
    largest |u| it captured."""
    box, dt = c1["box"], c1["dt"]
    N = box.info["nharbored"]
    o1, o2 = np.zeros((N, 3)), np.zeros((N, 3))
    names = ("map", "stations")
    caps = np.concatenate([c1["sets"][n][0].reshape(-1) for n in names])
    cap = ho.solver_run(box.lnid, box.etable.copy(), box.ntable.copy(), o1, o2, 0, NSTEPS, dt,
                        loaded_lnid=c1["loaded"], forces=c1["F"], cap_lnid=caps)
    out, at = {"U": float(np.abs(cap).max())}, 0
    for n in names:
        ids, grad, _ = c1["sets"][n]
        u = cap[:, at:at + ids.size].reshape(NSTEPS, len(ids), 8, 3)
        at += ids.size
        G = np.einsum("pbc,tpca->tpba", grad, u)
        G1 = np.concatenate([np.zeros_like(G[:1]), G[:-1]])
        out[n] = np.stack([G, (G - G1) / dt], axis=2)
    return out


def _linear_measures(t):
    """|xx|, |yy|, |zz|, |xy|, |yz|, |xz|, |xx + yy + zz|, |xx + yy| of tensors t [..., 6] -> [..., 8]."""
    return np.concatenate([np.abs(t), np.abs(t[..., :3].sum(axis=-1, keepdims=True)), np.abs(t[..., :2].sum(axis=-1, keepdims=True))], axis=-1)


def _strain6(G):
    return np.stack([G[..., 0, 0], G[..., 1, 1], G[..., 2, 2], 0.5 * (G[..., 1, 0] + G[..., 0, 1]), 0.5 * (G[..., 2, 1] + G[..., 1, 2]),
                     0.5 * (G[..., 2, 0] + G[..., 0, 2])], axis=-1)


@pytest.mark.parametrize("rate,first", CADENCES)
def test_linear_peaks_match_the_oracle(c1, c1_oracle, brick_mode, rate, first):
    """The same run against the oracle (double): numpy forms G from the oracle's captured fields, and from it the six
    component peaks, vals[6] and vals[9] of the strain, of the strain rate and of the stress, and the three component peaks of
    the rotation and its rate.  The fields agree within TOL = 1e-9 of the run's largest |u| = U (the bar tests/test_gpu_peaks.py
    and test_gpu_cumul.py hold them to), so an entry G[b][a] agrees within d_b = TOL U sum_c |g_bc|, and linearly from there:
    d_0, d_1, d_2 for xx, yy, zz; 0.5 (d_b + d_a) for a shear or a rotation component; d_0 + d_1 + d_2 and d_0 + d_1 for the
    volumetric and the areal measure; a rate entry within 2 d_b / dt; a stress within 2 mu d(e) + |lambda| (d_0 + d_1 + d_2)
    on the diagonal and 2 mu d(e) off it.  A peak of |v| moves by no more than v does.  The squared measures vals[7], vals[8]
    are the twins' and the CPU restatement's business.
    Measured on an MI355X: the worst value over both cadences, both brick modes and both point sets is 4.3e-6 of its bound
    (a stress component of the map, with bricks, at rate 1; without bricks 2.0e-6)."""
    out = _c1_run(c1, "f64", rate, first)
    due, dt, worst = _due(rate, first), c1["dt"], 0.0
    for name in ("map", "stations"):
        ids, grad, lame = c1["sets"][name]
        G = c1_oracle[name][due]                             # [k, np, 2, 3, 3]
        d = TOL * c1_oracle["U"] * np.abs(grad).sum(axis=2)   # [np, 3]
        de = np.stack([d[:, 0], d[:, 1], d[:, 2], 0.5 * (d[:, 1] + d[:, 0]), 0.5 * (d[:, 2] + d[:, 1]), 0.5 * (d[:, 2] + d[:, 0])], axis=1)
        dlin = np.concatenate([de, d.sum(axis=1, keepdims=True), d[:, :2].sum(axis=1, keepdims=True)], axis=1)      # [np, 8]
        lam, mu = lame[:, 0:1], lame[:, 1:2]
        ds = 2 * mu * de
        ds[:, :3] += np.abs(lam) * d.sum(axis=1, keepdims=True)
        dslin = np.concatenate([ds, ds[:, :3].sum(axis=1, keepdims=True), ds[:, :2].sum(axis=1, keepdims=True)], axis=1)
        e, er = _strain6(G[:, :, 0]), _strain6(G[:, :, 1])
        st = 2 * mu[None] * e
        st[..., :3] += (lam[None] * e[..., :3].sum(axis=-1, keepdims=True))
        rot = lambda g: np.stack([0.5 * (g[..., 1, 2] - g[..., 2, 1]), 0.5 * (g[..., 2, 0] - g[..., 0, 2]), 0.5 * (g[..., 0, 1] - g[..., 1, 0])], axis=-1)
        drot = np.stack([0.5 * (d[:, 1] + d[:, 2]), 0.5 * (d[:, 2] + d[:, 0]), 0.5 * (d[:, 0] + d[:, 1])], axis=1)
        got = out[name]["all"][0]
        cols = [0, 1, 2, 3, 4, 5, 6, 9]
        for label, want, bound, at in (("strain", _linear_measures(e).max(axis=0), dlin, 0),
                                       ("strain rate", _linear_measures(er).max(axis=0), 2 * dlin / dt, 10),
                                       ("stress", _linear_measures(st).max(axis=0), dslin, 20),
                                       ("rotation", np.abs(rot(G[:, :, 0])).max(axis=0), drot, None),
                                       ("rotation rate", np.abs(rot(G[:, :, 1])).max(axis=0), 2 * drot / dt, None)):
            g = got[:, [at + c for c in cols]] if at is not None else got[:, 30:33] if label == "rotation" else got[:, 35:38]
            err = np.abs(g - want)
            assert want.max() > 0 and (bound > 0).all()
            print("%s %s: largest error %.3e, %.3e of its bound" % (name, label, err.max(), (err / bound).max()))
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (name, label, np.argwhere(err > bound)[:5])
    print("worst error over its bound: %.3e" % worst)


# ---------------------------------------------------------------------------------------------------------------------
# 3. life cycle
# ---------------------------------------------------------------------------------------------------------------------

def test_reset_and_load_resume_a_run_and_upload_keeps_the_tracker(c1, brick_mode):
    """One context.  Fetch at step 100; reset leaves zeros and -1; load puts the fetched state back; the run goes on; the
    final state equals the twins' fold of the whole run, bit for bit.  Then hq_upload: the state stays, the due steps follow
    the new step number."""
    ids, grad, lame = c1["sets"]["map"]
    s = _solver(c1)
    h = s.deform_add(ids, grad, lame, rate=1, quantities=ALL)
    twins = _add_twins(s, ids, grad, 1, NSTEPS + 8)
    s.run(7)
    s.run(93)
    saved = s.deform_fetch(h)
    assert saved[2] == 100 and (saved[0] > 0).any()
    _same(s.deform_fetch(h), saved)                          # a fetch leaves the state in place
    s.deform_reset(h)
    vals, when, n = s.deform_fetch(h)
    assert n == 0 and (vals == 0).all() and (when == -1).all() and vals.shape == saved[0].shape
    s.deform_load(h, *saved)
    _same(s.deform_fetch(h), saved)
    s.run(140)
    got = s.deform_fetch(h)
    whole = _fetch_twins(s, twins, len(ids))
    _same(got, _fold(whole, ALL, lame))
    assert got[2] == NSTEPS and not np.array_equal(got[0], saved[0])
    tm1, tm2 = s.download()
    s.upload(tm1 * 1000.0, tm2 * 1000.0, 500)
    _same(s.deform_fetch(h), got)
    s.run(6)                                                 # samples of steps 500 .. 505 of the scaled field
    after = s.deform_fetch(h)
    later = _fetch_twins(s, twins, len(ids))
    s.close()
    assert np.array_equal(later[0], np.arange(500, 506))
    want = _fold(later, ALL, lame, into=(got[0].copy(), got[1].copy()))
    _same(after, (want[0], want[1], NSTEPS + 6))
    assert (after[1] >= 500).any()


def test_clears_accounting_and_handles(c1):
    """device_bytes grows at add by the documented amount -- np (32 + 192 [+ 16]) of tables and np (88 nt + 48 nv) of state --
    and shrinks at clear; pcie_d2h_bytes grows by exactly the fetched bytes and by nothing between fetches; the other kinds'
    clears leave a deformation tracker alone; handles are not reused."""
    ids, grad, lame = c1["sets"]["map"]
    i5, g5, l5 = c1["sets"]["stations"]
    s = _solver(c1)
    assert s._lib.hq_deform_clear(s._h) == 0                 # before any tracker: a no-op
    bytes0 = s.info()["device_bytes"]
    h1 = s.deform_add(ids, grad, lame, rate=1, quantities=ALL)
    bytes1 = s.info()["device_bytes"]
    assert bytes1 - bytes0 == 272 * (32 + 192 + 16) + 272 * (88 * 3 + 48 * 2)
    h2 = s.deform_add(i5, g5, None, rate=3, quantities=E | WR)
    assert s.info()["device_bytes"] - bytes1 == 5 * (32 + 192) + 5 * (88 + 48)
    assert (h1, h2) == (0, 1)
    s.record_add(i5, np.ascontiguousarray(g5[:, 0, :]), rate=1, derivs=1, capacity=16)
    s.peak_add(ids[:, 0], None, rate=1, quantities=capi.HQ_PEAK_VEL)
    s.cum_add(ids[:, 0], None, rate=1, quantities=capi.HQ_PEAK_VEL)
    s.run(10)
    s.record_clear()
    s.snapshot_clear()
    s.peak_clear()
    s.spec_clear()
    s.cum_clear()
    s.sync()
    before = s.info()
    s.run(90)
    s.sync()
    after = s.info()
    assert after["pcie_d2h_bytes"] == before["pcie_d2h_bytes"] and after["pcie_h2d_bytes"] == before["pcie_h2d_bytes"]
    f1 = s.deform_fetch(h1)
    mid = s.info()
    assert f1[2] == 100 and (f1[0] > 0).any()
    assert mid["pcie_d2h_bytes"] - after["pcie_d2h_bytes"] == 272 * (88 * 3 + 48 * 2) and mid["pcie_h2d_bytes"] == after["pcie_h2d_bytes"]
    assert s.deform_fetch(h2)[2] == 34
    assert s.info()["pcie_d2h_bytes"] - mid["pcie_d2h_bytes"] == 5 * (88 + 48)
    s.deform_clear()
    assert s.info()["device_bytes"] == bytes0
    with pytest.raises(ha.HqError, match="unknown deformation tracker handle"):
        s.deform_fetch(h1)
    assert s.deform_add(i5, g5, l5, quantities=S) == 2       # handles are not reused
    s.run(5)
    s.deform_clear()
    s.deform_clear()                                         # nothing to drop: no error
    s.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------------------------------

def test_bad_descriptions_and_unknown_handles(c1):
    ids, grad, lame = c1["sets"]["stations"]
    s = _solver(c1)
    bad = ids.copy()
    bad[3, 5] = s.N
    neg = ids.copy()
    neg[0, 0] = -1
    nan_l, inf_l, neg_mu = lame.copy(), lame.copy(), lame.copy()
    nan_l[2, 0], inf_l[4, 1], neg_mu[1, 1] = float("nan"), float("inf"), -1.0
    for kw in (dict(ids=bad), dict(ids=neg), dict(rate=0), dict(rate=-2), dict(quantities=0), dict(quantities=32),
               dict(quantities=ALL | 64), dict(quantities=-1), dict(lame=None, quantities=S), dict(lame=None, quantities=ALL),
               dict(lame=nan_l, quantities=S), dict(lame=inf_l, quantities=E | S), dict(lame=neg_mu, quantities=ALL)):
        args = dict(ids=ids, grad=grad, lame=lame, quantities=ALL)
        args.update(kw)
        with pytest.raises(ha.HqError):
            s.deform_add(args.pop("ids"), args.pop("grad"), args.pop("lame"), **args)
    assert s.deform_add(ids, grad, neg_mu, quantities=E | W) == 0      # moduli that no bit of the mask reads are not read
    lib = s._lib
    hh = ctypes.c_int32(-1)
    for npts, i, g, l, q in ((-1, ids, grad, lame, ALL), (5, None, grad, lame, ALL), (5, ids, None, lame, ALL), (5, ids, grad, None, S)):
        d = capi._DeformDesc(npts, None if i is None else i.ctypes.data, None if g is None else g.ctypes.data,
                             None if l is None else l.ctypes.data, 1, 0, q, 0)
        assert lib.hq_deform_add(s._h, ctypes.byref(d), ctypes.byref(hh)) == -1
    ok = capi._DeformDesc(5, ids.ctypes.data, grad.ctypes.data, lame.ctypes.data, 1, 0, ALL, 0)
    assert lib.hq_deform_add(s._h, ctypes.byref(ok), None) == -1 and lib.hq_deform_add(s._h, None, ctypes.byref(hh)) == -1
    v, w, n = np.zeros(5 * 40), np.zeros(5 * 10, np.int32), ctypes.c_int64()
    for handle in (1, 7, -1):                                # only handle 0 exists
        assert lib.hq_deform_fetch(s._h, handle, capi._ptr(v), capi._ptr(w), ctypes.byref(n)) == -1
        assert lib.hq_deform_load(s._h, handle, capi._ptr(v), capi._ptr(w), ctypes.c_int64(0)) == -1
        assert lib.hq_deform_reset(s._h, handle) == -1
    h = s.deform_add(ids, grad, lame, quantities=ALL)
    assert lib.hq_deform_fetch(s._h, h, None, capi._ptr(w), ctypes.byref(n)) == -1
    assert lib.hq_deform_fetch(s._h, h, capi._ptr(v), None, ctypes.byref(n)) == -1
    assert lib.hq_deform_fetch(s._h, h, capi._ptr(v), capi._ptr(w), None) == -1
    assert lib.hq_deform_fetch(s._h, h, capi._ptr(v), capi._ptr(w), ctypes.byref(n)) == 0
    assert lib.hq_deform_load(s._h, h, None, capi._ptr(w), ctypes.c_int64(0)) == -1
    assert lib.hq_deform_load(s._h, h, capi._ptr(v), None, ctypes.c_int64(0)) == -1
    assert lib.hq_deform_load(s._h, h, capi._ptr(v), capi._ptr(w), ctypes.c_int64(-1)) == -1
    assert lib.hq_deform_load(s._h, h, capi._ptr(v), capi._ptr(w), ctypes.c_int64(3)) == 0
    assert s.deform_fetch(h)[2] == 3
    with pytest.raises(ha.HqError):
        s.deform_load(h, np.zeros((5, 39)), np.zeros((5, 10), np.int32), 0)
    s.deform_clear()
    assert lib.hq_deform_fetch(s._h, h, capi._ptr(v), capi._ptr(w), ctypes.byref(n)) == -1
    assert lib.hq_deform_reset(s._h, h) == -1
    s.close()
