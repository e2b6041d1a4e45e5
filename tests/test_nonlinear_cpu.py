"""Nonlinear soil beside the patch and brick step (hq_nonlinear_set; csrc/hq_nonlin.h, csrc/hq_nonlin_dev.h), without a device.

tests/nl_reference.py restates the reference's nonlinear step in numpy, in two forms: (A) the reference's own (the stress force
instead of the stiffness force in nonlinear elements) and (B) the correction beside the elastic step, in the device's order.

  fixtures   c1_nl_vm, c1_nl_dp, c5_two_level_nl (tests/golden/make_golden_nonlinear.py): at the later checkpoint the reference
             is >= 1e-2 rel. L-inf off its own elastic run (recomputed here with the C oracle), and ep > 0 in more than 1 % and
             fewer than 90 % of the quadrature points; (A) run from rest reproduces both checkpoints BIT FOR BIT, as the BKT
             restatement reproduces its own
  (B)        against the fixtures, measured here (rel. L-inf of tm1 at the two checkpoints; the GPU test's bound is 8 x these):
                 c1_nl_vm 1.73e-12 5.74e-12    c1_nl_dp 2.03e-12 3.40e-12    c5_two_level_nl 2.52e-12 6.49e-12
  host       hqh_nonlinear_constants == nl_reference.constants == the fixtures' elems / cons, bit for bit (alphakay and
             cohefriction, interpolated rows, the Vs window); hqh_nonlinear_advance == nl_reference.advance bit for bit on every
             one-step case, its corner forces == nl_reference.corner_forces == hqh_nonlinear_force
  rules      J2 == 0 with dLambda == 0 keeps the state finite and as it was (the reference's NaN is not reproduced); an element
             whose 24 values are within 1e-20 of zero is not advanced
  one step   (B) in double against the np.longdouble restatement, per node and component: |got - ref| <= b 2^-53 T with T the sum
             of the magnitudes of all addends, the correction's included.  b measured here (the GPU bound is b x 64):
                 bricks 3.14   no_bricks 3.14   two_level 3.07   n1 2.58   n63 2.60   n64 2.70   n65 2.72   faces 2.15   empty 2.38
             (empty is the elastic step alone: the C oracle's against the extended one)
  teeth      the criterion rejects a force built from the UPDATED plastic strain, a wrong sign, a missing dt^2, a quadrature
             point left out and hanging nodes not distributed
  plan       hq_nonlinear_plan_check: 0 faults, the header's bytes; planted faults are counted
  exports    both libraries, ABI 6; hq_k_nl_element in the gfx950 code object without scratch
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import hercules_amd as ha
from hercules_amd import build as hbuild
from hercules_amd import capi, host
from oracle import herc_oracle as ho
from tests import helpers as H
from tests import nl_reference as R
from tests import test_code_object_cpu as CO

EPS = 2.0 ** -53
SEED, STATE_SEED = 4242, 4343
FIXTURES = ("c1_nl_vm", "c1_nl_dp", "c5_two_level_nl")
NAMES = ["hq_nonlinear_set", "hq_nonlinear_info", "hq_nonlinear_fetch", "hq_nonlinear_load", "hq_nonlinear_clear",
         "hq_nonlinear_plan_check", "hq_nonlinear_plan_tables", "hq_nonlinear_table_faults"]
KERNELS = ["hq_k_nl_element", "hq_k_atten_apply_at", "hq_k_atten_node_sum"]
# rel. L-inf of form (B)'s tm1 against the fixtures' two checkpoints, measured by test_form_b_against_the_fixtures (printed
# there), rounded up to three figures
B_AGAINST_FIXTURE = {"c1_nl_vm": (1.73e-12, 5.74e-12), "c1_nl_dp": (2.03e-12, 3.40e-12), "c5_two_level_nl": (2.52e-12, 6.49e-12)}
# the worst ratio of form (B) in double on the one-step cases, measured by test_form_b_against_the_extended_reference (printed
# there), rounded up to three figures
B_ONE_STEP = {"bricks": 3.14, "no_bricks": 3.14, "two_level": 3.07, "n1": 2.58, "n63": 2.60, "n64": 2.70, "n65": 2.72, "faces": 2.15,
              "empty": 2.38}

needs_longdouble = pytest.mark.skipif(not np.finfo(np.longdouble).eps < 1e-18, reason="np.longdouble is no wider than double here")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.fixture(scope="module")
def libs():
    hbuild.build()
    return ha.load_library(), capi.load_library(precision="f32")


# ---------------------------------------------------------------------------------------------
# the fixtures
# ---------------------------------------------------------------------------------------------
def problem_of(name, g):
    """The fixture's mesh with the Rayleigh tables solver_init leaves (edata as it stands after it)."""
    mat = g["mat_vs_vp_rho"]
    freq = float(g["freq"])
    if name.startswith("c1"):
        lnid, node_ijk, elem_ijk, edge = ho.mesh_from_elem_ticks(g["elem_ticks"], H.C1_FAR_TICKS)
        E, N = len(lnid), len(node_ijk)
        edata = np.empty((E, 4), np.float32)
        edata[:, 0] = np.float32(1000.0 / 2 ** 30 * edge)
        edata[:, 1], edata[:, 2], edata[:, 3] = mat[:, 1], mat[:, 0], mat[:, 2]
        et, nt = ho.solver_init(lnid, edata, ho.face_bits(elem_ijk, H.C1_NX, H.C1_NY, H.C1_NZ), N, 1e-3, freq)
        return dict(lnid=lnid, etable=et, ntable=nt, dangling=None, N=N, E=E, dt=1e-3, edata=edata, freq=freq,
                    node_xyz=(np.asarray(node_ijk, np.int64) * (1 << 20)).astype(np.int32))
    m = ho.octree_mesh_from_elem_ticks(g["elem_ticks"], H.C1_FAR_TICKS)
    E, N = len(m["lnid"]), len(m["node_q"])
    edata = np.empty((E, 4), np.float32)
    edata[:, 0] = (1000.0 / 2 ** 30 * m["emin"] * m["elem_size"].astype(np.float64)).astype(np.float32)
    edata[:, 1], edata[:, 2], edata[:, 3] = mat[:, 1], mat[:, 0], mat[:, 2]
    et, nt = ho.solver_init(m["lnid"], edata, m["face"], N, 1e-3, freq)
    ho.compute_adjust(nt, 0, m["dangling"])
    return dict(lnid=m["lnid"], etable=et, ntable=nt, dangling=m["dangling"], N=N, E=E, dt=1e-3, edata=edata, freq=freq,
                node_xyz=(m["node_q"].astype(np.int64) * m["emin"]).astype(np.int32))


@functools.lru_cache(maxsize=None)
def golden_problem(name):
    g = H.load(name)
    return g, problem_of(name, g)


@functools.lru_cache(maxsize=None)
def golden_run(name, form="a"):
    """The restatement's run of a fixture from rest, once per process -> {step: (tm1, tm2, pstrain, ep)}, read-only."""
    g, p = golden_problem(name)
    steps = [int(s) for s in g["ckpt_steps"]]
    run = R.run_a if form == "a" else R.run_b
    kept = run(p, g["elems"], g["cons"], steps[-1], g["loaded_lnid"], g["forces"], keep=steps)
    for v in kept.values():
        for a in v:
            a.flags.writeable = False
    return kept


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_conditions_and_form_a_bitwise(name):
    g, p = golden_problem(name)
    steps = [int(s) for s in g["ckpt_steps"]]
    sibling = "c1_bkt" if name.startswith("c1") else "c5_two_level_bkt"
    # the size the BKT fixtures have: the same arrays plus elems / cons / props, and fields of a yielding run deflate a little
    # worse (c5_two_level_nl: 650 567 bytes against 645 046) -- 5 % over the sibling at the most
    assert os.path.getsize(os.path.join(H.GOLDEN, name + ".npz")) <= 1.05 * os.path.getsize(os.path.join(H.GOLDEN, sibling + ".npz"))
    elems, cons = R.constants(p["edata"], int(g["model"]), g["props"], float(g["vs_min"]), float(g["vs_cut"]))
    assert np.array_equal(elems, g["elems"]) and np.array_equal(bits(cons), bits(g["cons"]))
    if name.startswith("c5"):
        assert len(p["dangling"][0]) > 0 and 0 < len(elems) < p["E"]            # hanging nodes, a linear / nonlinear interface
    else:
        assert len(elems) == p["E"]
    # the elastic sibling: the C oracle's run of the same input
    tm1, tm2 = np.zeros((p["N"], 3)), np.zeros((p["N"], 3))
    ho.solver_run(p["lnid"], p["etable"], p["ntable"], tm1, tm2, 0, steps[-1], p["dt"], loaded_lnid=g["loaded_lnid"], forces=g["forces"],
                  dangling=p["dangling"])
    off = H.rel_linf(g["ckpt_tm1"][-1], tm2)                                 # (the oracle leaves the latest field in its second array)
    kept = golden_run(name)
    yielded = float((kept[steps[-1]][3] > 0).mean())
    print("\n[nonlinear] %s: off the elastic run %.3e (the generator: %.3e), yielded %.3f, nonlinear elements %d of %d"
          % (name, off, float(g["elastic_off"][-1]), yielded, len(elems), p["E"]))
    assert off >= 1e-2 and float(g["elastic_off"][-1]) >= 1e-2
    assert 0.01 < yielded < 0.9 and abs(yielded - float(g["yielded"])) < 1e-12
    for k, s in enumerate(steps):
        tm1, tm2 = kept[s][:2]
        d1, d2 = H.rel_linf(tm1, g["ckpt_tm1"][k]), H.rel_linf(tm2, g["ckpt_tm2"][k])
        print("[nonlinear] %s step %d: form (A) rel L-inf %.3e %.3e, max |u| %.3e" % (name, s, d1, d2, np.abs(g["ckpt_tm1"][k]).max()))
        assert np.array_equal(tm1, g["ckpt_tm1"][k]) and np.array_equal(tm2, g["ckpt_tm2"][k]), (s, d1, d2)
        assert np.isfinite(kept[s][2]).all() and np.isfinite(kept[s][3]).all()


@pytest.mark.parametrize("name", FIXTURES)
def test_form_b_against_the_fixtures(name):
    g, p = golden_problem(name)
    steps = [int(s) for s in g["ckpt_steps"]]
    kept, a = golden_run(name, "b"), golden_run(name)
    d = [H.rel_linf(kept[s][0], g["ckpt_tm1"][k]) for k, s in enumerate(steps)]
    print("\n[nonlinear] %s: form (B) against the fixture, rel L-inf %s (recorded %s); yielded points that differ from (A)'s: %d"
          % (name, ["%.2e" % x for x in d], B_AGAINST_FIXTURE[name], int(((kept[steps[-1]][3] > 0) != (a[steps[-1]][3] > 0)).sum())))
    for k in range(len(steps)):
        assert d[k] <= 1e-6                                                  # (the issue: else move the checkpoint earlier)
        assert 0.9 * B_AGAINST_FIXTURE[name][k] <= d[k] <= B_AGAINST_FIXTURE[name][k], (d, B_AGAINST_FIXTURE[name])   # the recorded figures are the run's


# ---------------------------------------------------------------------------------------------
# the one-step cases (tests/test_gpu_nonlinear.py runs the same on the device)
# ---------------------------------------------------------------------------------------------
BOX = (9, 9, 9)                                                      # the smallest box the planner still gives brick units (below)
SMALL = (7, 5, 4)
PROPS = {R.VONMISES: [[100, 0, 2e5, 0, 0, 2e9], [9000, 0, 2e5, 0, 0, 2e9]],
         R.DRUCKERPRAGER: [[100, 0.1, 2e5, 0, 0, 2e9], [9000, 0.05, 4e5, 0, 0, 1e9]]}


@functools.lru_cache(maxsize=None)
def box(shape):
    nx, ny, nz = shape
    p = H.uniform_box(nx, ny, nz)
    edata = np.empty((p["E"], 4), np.float32)
    edata[:] = (62.5, 6000.0, 3464.0, 2700.0)
    return dict(p, edata=edata)


@functools.lru_cache(maxsize=None)
def two_level():
    q = H.two_level_mesh(16, 8, 6, 3)
    return dict(q, node_xyz=q["node_q"])


def _spread(E, n):
    return np.unique(np.linspace(0, E - 1, n).astype(np.int32))


def _boundary(shape):
    nx, ny, nz = shape
    elem_ijk = np.asarray(ho.uniform_mesh(nx, ny, nz)[0])
    return np.nonzero(ho.face_bits(elem_ijk, nx, ny, nz))[0].astype(np.int32)


# case -> (mesh, hq_options of the GPU test's context, model, the nonlinear elements of the mesh's E)
CASES = {
    "bricks": (lambda: box(BOX), {}, R.DRUCKERPRAGER, lambda p: np.arange(p["E"], dtype=np.int32)),
    "no_bricks": (lambda: box(BOX), {"no_bricks": 1}, R.VONMISES, lambda p: np.arange(p["E"], dtype=np.int32)),
    "two_level": (two_level, {}, R.DRUCKERPRAGER, lambda p: np.nonzero(p["mesh"]["elem_size"] == 1)[0].astype(np.int32)),
    "n1": (lambda: box(SMALL), {}, R.VONMISES, lambda p: np.array([0], np.int32)),
    "n63": (lambda: box(SMALL), {}, R.DRUCKERPRAGER, lambda p: _spread(p["E"], 63)),
    "n64": (lambda: box(SMALL), {}, R.VONMISES, lambda p: _spread(p["E"], 64)),
    "n65": (lambda: box(SMALL), {}, R.DRUCKERPRAGER, lambda p: _spread(p["E"], 65)),
    "faces": (lambda: box(SMALL), {}, R.DRUCKERPRAGER, lambda p: _boundary(SMALL)),
    "empty": (lambda: box(SMALL), {}, R.VONMISES, lambda p: np.zeros(0, np.int32)),
}


def case_inputs(case):
    """(p, options, model, elems, cons, u1, u2, pstrain0, ep0) of a case."""
    make, options, model, pick = CASES[case]
    p = make()
    elems_all, cons_all = R.constants(p["edata"], model, PROPS[model], 0.0, 10000.0)
    assert len(elems_all) == p["E"]
    elems = pick(p)
    cons = np.ascontiguousarray(cons_all[elems])
    u1, u2 = H.step_fields(p["N"], SEED, p["dangling"])
    ps, ep = R.yielding_state(p, elems, cons, u1, STATE_SEED)
    return p, options, model, elems, cons, u1, u2, ps, ep


@functools.lru_cache(maxsize=None)
def reference(case):
    """(p, options, model, elems, cons, u1, u2, ps0, ep0, ref, T, got_b, ps1, ep1, b) of a case, once per process, read-only:
    ref, T the np.longdouble step, got_b form (B) in double with the state it leaves, b its worst ratio."""
    p, options, model, elems, cons, u1, u2, ps, ep = case_inputs(case)
    ref, T = R.extended(p, elems, cons, u1, u2, ps)
    got, ps1, ep1 = R.step_b(p, elems, cons, u1, u2, ps, ep)
    b = float((np.abs(got - ref) / (EPS * T)).max())
    for a in (u1, u2, ps, ep, ref, T, got, ps1, ep1, cons, elems):
        a.flags.writeable = False
    return p, options, model, elems, cons, u1, u2, ps, ep, ref, T, got, ps1, ep1, b


def desc_of(p):
    return H.solver_desc(dict(p, node_xyz=p["node_xyz"]))


def test_the_brick_box_is_the_smallest_that_gets_units(libs):
    nx, ny, nz = BOX
    assert capi.brick_plan_check(desc_of(box(BOX)))["brick_nodes"] > 0
    for smaller in ((nx - 1, ny, nz), (nx, ny - 1, nz), (nx, ny, nz - 1)):
        assert capi.brick_plan_check(desc_of(box(smaller)))["brick_nodes"] == 0, smaller


@needs_longdouble
@pytest.mark.parametrize("case", sorted(CASES))
def test_form_b_against_the_extended_reference(libs, case):
    p, options, model, elems, cons, u1, u2, ps, ep, ref, T, got, ps1, ep1, b = reference(case)
    n = len(elems)
    moved = int(((ep1 != ep) | (ps1 != ps).any(axis=2)).sum())
    print("\n[nonlinear] B_restatement %-10s %.3f   elements %d, points that yield %d of %d" % (case, b, n, moved, 8 * n))
    assert 0.9 * B_ONE_STEP[case] <= b <= B_ONE_STEP[case], b
    if n:
        assert 0.25 < moved / (8.0 * n) < 0.75                               # about half the points yield
        corr = np.abs(R.correction(p, elems, cons, ps, p["N"]) / p["ntable"][:, :1])
        assert corr.max() > 1e-3 * np.abs(got).max()                          # the correction is not a rounding error of the step
    # the host text: the state bit for bit, the corner forces bit for bit
    hp, he = ps.copy(), ep.copy()
    ef = host.nonlinear_advance(np.asarray(p["lnid"])[elems], cons, u1, p["dt"], hp, he)
    assert np.array_equal(bits(hp), bits(ps1)) and np.array_equal(bits(he), bits(ep1))
    want = R.corner_forces(cons, p["dt"], ps)
    assert np.array_equal(bits(ef), bits(want))
    assert np.array_equal(bits(host.nonlinear_force(cons, p["dt"], ps)), bits(want))


TEETH = {"updated": dict(updated=True), "sign": dict(sign=-1.0), "no_dt2": dict(no_dt2=True), "point": dict(skip_point=5),
         "no_distribution": dict(no_distribution=True)}


@needs_longdouble
@pytest.mark.parametrize("tooth", sorted(TEETH))
def test_criterion_rejects_the_planted_faults(libs, tooth):
    case = "two_level" if tooth == "no_distribution" else "n65"
    p, options, model, elems, cons, u1, u2, ps, ep, ref, T, got, ps1, ep1, b = reference(case)
    B = 64.0 * B_ONE_STEP[case]
    assert (np.abs(got - ref) <= B * EPS * T).all()
    bad = R.step_b(p, elems, cons, u1, u2, ps, ep, **TEETH[tooth])[0]
    tripped = np.nonzero((np.abs(bad - ref) > B * EPS * T).any(axis=1))[0]
    touched = np.unique(np.asarray(p["lnid"])[elems])
    if tooth == "no_distribution":
        ids, ptr, anc = [np.asarray(a, np.int64) for a in p["dangling"]]
        concerned = np.union1d(np.unique(anc), ids)
        assert np.isin(np.unique(anc), tripped).mean() >= 0.9
    else:
        concerned = touched
        assert len(tripped) >= 0.9 * len(concerned)
    print("\n[nonlinear] tooth %-16s tripped %d of %d concerned (of %d nodes)" % (tooth, len(tripped), len(concerned), p["N"]))
    assert len(tripped) > 0 and np.isin(tripped, concerned).all()


# ---------------------------------------------------------------------------------------------
# the two rules
# ---------------------------------------------------------------------------------------------
def test_where_j2_is_zero_the_state_is_kept_and_stays_finite(libs):
    """J2 == 0 with dLambda == 0, the case in which the reference's 0 * dfds is NaN.  An exact J2 == 0 of a MOVING element
    (a rigid translation leaves strains of rounding size, and a J2 above 0) is made here by moduli so small that the squares of
    the deviator underflow: the deviator itself is not 0, so the reference's dev / (2 sqrt(J2)) is infinite and 0 * that NaN."""
    p = box(SMALL)
    lnid = np.asarray(p["lnid"], np.int64)
    cons = R.constants(p["edata"], R.VONMISES, PROPS[R.VONMISES], 0.0, 10000.0)[1].copy()
    cons[:, 1] = cons[:, 2] = 1e-160                                             # mu, lambda
    cons[:, 4] = 0.0                                                             # k: FsT = sqrt(J2) - 0 = 0, not > 0
    u1 = H.step_fields(p["N"], SEED)[0]
    ps0 = np.random.default_rng(3).uniform(-1e-6, 1e-6, (p["E"], 8, 6))
    s = R.stress(R.strains(u1[lnid], R.dxi(cons[:, 0])) - ps0, cons[:, 1], cons[:, 2])
    o = ((s[:, :, 0] + s[:, :, 1]) + s[:, :, 2]) / 3.0
    dev = s[:, :, 0] - o
    J2 = ((dev * dev + (s[:, :, 1] - o) ** 2) + (s[:, :, 2] - o) ** 2) * 0.5 + s[:, :, 3] ** 2 + s[:, :, 4] ** 2 + s[:, :, 5] ** 2
    assert not J2.any() and dev.all() and not R.at_rest(u1[lnid]).any()
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.isnan(0.0 * (dev / (2.0 * np.sqrt(J2)))).all()                 # what the reference would add
    ps, ep = ps0.copy(), np.zeros((p["E"], 8))
    host.nonlinear_advance(p["lnid"], cons, u1, p["dt"], ps, ep)
    assert np.isfinite(ps).all() and np.array_equal(bits(ps), bits(ps0)) and not ep.any()
    ps1, ep1 = R.advance(u1[lnid], cons, ps0, np.zeros((p["E"], 8)))
    assert np.array_equal(bits(ps1), bits(ps0)) and not ep1.any()


def test_an_element_at_rest_is_not_advanced(libs):
    p = box(SMALL)
    elems = np.array([3, 77], np.int32)
    cons = R.constants(p["edata"], R.VONMISES, PROPS[R.VONMISES], 0.0, 10000.0)[1][elems]
    lnid = np.asarray(p["lnid"])[elems]
    u1 = np.zeros((p["N"], 3))
    u1[lnid[0]] = 1e-20                                                          # "zero": |x| <= 1e-20
    u1[lnid[1]] = np.random.default_rng(1).uniform(-1e-3, 1e-3, (8, 3))
    ps = np.random.default_rng(2).uniform(-1e-5, 1e-5, (2, 8, 6))               # would yield at once: k is far below its stress
    ep = np.zeros((2, 8))
    ps0 = ps.copy()
    ef = host.nonlinear_advance(lnid, cons, u1, p["dt"], ps, ep)
    assert np.array_equal(bits(ps[0]), bits(ps0[0])) and not ep[0].any()          # at rest: kept
    assert (ps[1] != ps0[1]).any() and (ep[1] > 0).any()                          # moving: advanced
    assert np.array_equal(bits(ef), bits(R.corner_forces(cons, p["dt"], ps0)))    # the force is the old state's either way
    u1[lnid[0][0], 1] = 1.1e-20                                                   # one component above the cap: advanced
    ps, ep = ps0.copy(), np.zeros((2, 8))
    host.nonlinear_advance(lnid, cons, u1, p["dt"], ps, ep)
    assert (ps[0] != ps0[0]).any()


# ---------------------------------------------------------------------------------------------
# the constants
# ---------------------------------------------------------------------------------------------
def test_constants_are_the_restatements(libs):
    rng = np.random.default_rng(11)
    E = 400
    edata = np.empty((E, 4), np.float32)
    edata[:, 0] = rng.choice([15.625, 31.25, 62.5], E)
    edata[:, 2] = rng.uniform(80.0, 4000.0, E)                                    # Vs
    edata[:, 1] = edata[:, 2] * rng.choice([1.2, 1.732, 2.5, 3.5, 10.0], E)       # Vp: lambda < 0, plain, capped
    edata[:, 3] = rng.uniform(1500.0, 2800.0, E)
    edata[:5, 2] = (100.0, 500.0, 2000.0, 499.99, 2000.01)                        # on the limits and the window's ends
    table = {R.ALPHAKAY: [[100, 0.02, 1e5, 0, 0, 1e8], [500, 0.05, 3e5, 0, 0, 2e8], [2000, 0.11, 9e5, 0, 0, 5e8]],
             R.COHEFRICTION: [[100, 2e4, 20.0, 0, 0, 1e8], [500, 5e4, 28.0, 0, 0, 2e8], [2000, 9e4, 35.0, 0, 0, 5e8]]}
    for properties in (R.ALPHAKAY, R.COHEFRICTION):
        for model in (R.VONMISES, R.DRUCKERPRAGER):
            for lo, hi in ((0.0, 10000.0), (499.99, 2000.0), (5000.0, 6000.0)):
                want = R.constants(edata, model, table[properties], lo, hi, properties)
                got = host.nonlinear_constants(edata, model, table[properties], lo, hi, properties)
                assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1])), (properties, model, lo, hi)
                if model == R.VONMISES:
                    assert not got[1][:, 3].any()
    assert len(R.constants(edata, 1, table[0], 5000.0, 6000.0)[0]) == 0
    assert (np.diff(R.constants(edata, 2, table[0], 0.0, 10000.0)[1][:, 3]) != 0).any()      # the rows are interpolated
    for bad in (dict(model=3), dict(properties=2)):
        kw = dict(model=1, properties=0)
        kw.update(bad)
        with pytest.raises(ha.HqError):
            host.nonlinear_constants(edata, kw["model"], table[0], 0.0, 1e4, kw["properties"])
    with pytest.raises(ha.HqError):
        host.nonlinear_constants(edata, 1, [[500, 0, 1, 0, 0, 0], [100, 0, 1, 0, 0, 0]], 0.0, 1e4)
    with pytest.raises(ha.HqError):
        host.nonlinear_constants(edata, 1, [[100, 0, np.nan, 0, 0, 0]], 0.0, 1e4)


@pytest.mark.parametrize("name", FIXTURES)
def test_host_constants_of_the_fixtures(libs, name):
    g, p = golden_problem(name)
    elems, cons = host.nonlinear_constants(p["edata"], int(g["model"]), g["props"], float(g["vs_min"]), float(g["vs_cut"]))
    assert np.array_equal(elems, g["elems"]) and np.array_equal(bits(cons), bits(g["cons"]))


# ---------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------
def nl_bytes(p, elems, touched):
    """include/hq_solver.h's formula; touched = the touched nodes (any numbering: only hanging or not matters)."""
    n = len(elems)
    if n == 0:
        return 0
    Ep = (n + 63) & ~63
    out = 720 * Ep + 4 * (len(touched) + 1) + 32 * n + 36 * len(touched)
    if p["dangling"] is not None and len(p["dangling"][0]):
        ids, ptr, anc = [np.asarray(a, np.int64) for a in p["dangling"]]
        corner = np.unique(np.asarray(p["lnid"])[elems])
        rows = np.nonzero(np.isin(ids, corner))[0]
        pairs = np.concatenate([anc[ptr[r]:ptr[r + 1]] for r in rows]) if len(rows) else np.zeros(0, np.int64)
        if len(pairs):
            out += 8 * len(np.unique(pairs)) + 4 + 8 * len(pairs)
    return out


def touched_nodes(p, elems):
    corner = np.unique(np.asarray(p["lnid"])[elems])
    if p["dangling"] is None or not len(p["dangling"][0]):
        return corner
    ids, ptr, anc = [np.asarray(a, np.int64) for a in p["dangling"]]
    rows = np.nonzero(np.isin(ids, corner))[0]
    extra = np.concatenate([anc[ptr[r]:ptr[r + 1]] for r in rows]) if len(rows) else np.zeros(0, np.int64)
    return np.union1d(corner, extra)


@pytest.mark.parametrize("case", sorted(CASES))
def test_plan_check(libs, case):
    p, options, model, elems, cons = case_inputs(case)[:5]
    d = desc_of(p)
    touched = touched_nodes(p, elems)
    rep = capi.nonlinear_plan_check(d, model, elems, cons)
    assert rep == dict(elements=len(elems), touched_nodes=len(touched) if len(elems) else 0, faults=0,
                       device_bytes=nl_bytes(p, elems, touched)), rep
    if not len(elems):
        return
    tnode, epos, nptr, nent, sd = capi.nonlinear_plan_tables(d, model, elems, cons)
    n, T = len(elems), len(tnode)
    Ep = (n + 63) & ~63
    assert T == len(touched) and (np.diff(tnode) > 0).all() and len(nptr) == T + 1 and nptr[-1] == 8 * n
    assert np.array_equal(np.sort(epos), np.arange(n)) and len(np.unique(nent)) == 8 * n and (nent % Ep < n).all()
    assert capi.nonlinear_table_faults(d, model, elems, cons, tnode, epos, nptr, nent, sd) == 0
    # planted: a node twice in the list, two entries of a node swapped, an entry naming another corner, a short table, a pair dropped
    if T > 1:
        twice = tnode.copy()
        twice[1] = twice[0]
        assert capi.nonlinear_table_faults(d, model, elems, cons, twice, epos, nptr, nent, sd) > 0
        moved = tnode.copy()
        moved[-1] += 1 if tnode[-1] + 1 < p["N"] else -1
        if (np.diff(moved) > 0).all():
            assert capi.nonlinear_table_faults(d, model, elems, cons, moved, epos, nptr, nent, sd) > 0
    if n > 1:
        two = epos.copy()
        two[1] = two[0]
        assert capi.nonlinear_table_faults(d, model, elems, cons, tnode, two, nptr, nent, sd) > 0
    short = nptr.copy()
    short[-1] -= 1
    assert capi.nonlinear_table_faults(d, model, elems, cons, tnode, epos, short, nent, sd) > 0
    if (np.diff(nptr) >= 2).any():
        q = int(nptr[int(np.argmax(np.diff(nptr) >= 2))])
        bad = nent.copy()
        bad[q], bad[q + 1] = nent[q + 1], nent[q]
        assert capi.nonlinear_table_faults(d, model, elems, cons, tnode, epos, nptr, bad, sd) == 1
        bad = nent.copy()
        bad[q] = nent[q + 1]
        assert capi.nonlinear_table_faults(d, model, elems, cons, tnode, epos, nptr, bad, sd) >= 2
    if case == "two_level":
        assert len(sd) > 0
        assert capi.nonlinear_table_faults(d, model, elems, cons, tnode, epos, nptr, nent, sd[:-1]) == 1
        wrong = sd.copy()
        wrong[0, 2] += 1
        assert capi.nonlinear_table_faults(d, model, elems, cons, tnode, epos, nptr, nent, wrong) == 1
    else:
        assert len(sd) == 0


def test_plan_check_refuses_what_set_refuses(libs):
    p, options, model, elems, cons = case_inputs("n65")[:5]
    d = desc_of(p)
    for kw, text in ((dict(model=3), "unknown model"), (dict(elems=elems[::-1]), "ascending"), (dict(elems=elems + p["E"]), "out of range"),
                     (dict(cons=np.where(np.arange(6) == 4, -1.0, cons)), "k must be"), (dict(cons=np.where(np.arange(6) == 0, 0.0, cons)), "h must be"),
                     (dict(cons=np.where(np.arange(6) == 1, -1.0, cons)), "mu must be"), (dict(cons=np.where(np.arange(6) == 2, np.inf, cons)), "not finite"),
                     (dict(model=1, cons=np.where(np.arange(6) == 3, 0.1, cons)), "alpha must be 0")):
        a = dict(model=model, elems=elems, cons=cons)
        a.update(kw)
        with pytest.raises(ha.HqError, match="hq error -1: .*" + text):
            capi.nonlinear_plan_check(d, a["model"], a["elems"], a["cons"])


# ---------------------------------------------------------------------------------------------
# exports
# ---------------------------------------------------------------------------------------------
def test_both_libraries_export_the_entry_points(libs):
    for lib in libs:
        for n in NAMES:
            assert hasattr(lib, n), n
        assert lib.hq_abi_version() == 6                                   # additive: no ABI bump
    assert set(NAMES) <= set(capi.EXPORTS)
    h = host.load_library()
    for n in ("hqh_nonlinear_constants", "hqh_nonlinear_advance", "hqh_nonlinear_force"):
        assert n in host.EXPORTS and hasattr(h, n)


def test_null_arguments_are_refused(libs):
    for lib in libs:
        out = (ctypes.c_int64 * 4)()
        d = capi._NonlinearDesc(1, 0, None, None)
        assert lib.hq_nonlinear_set(None, ctypes.byref(d)) == -1
        assert lib.hq_nonlinear_info(None, out) == -1
        assert lib.hq_nonlinear_fetch(None, None, None) == -1
        assert lib.hq_nonlinear_load(None, None, None) == -1
        assert lib.hq_nonlinear_clear(None) == -1
        assert lib.hq_nonlinear_plan_check(None, None, out) == -1
        assert lib.hq_nonlinear_plan_tables(None, None, None, None, None, None, None, None) == -1
        assert lib.hq_nonlinear_table_faults(None, None, None, None, None, None, None, ctypes.c_int64(0), None) == -1


def test_kernels_in_the_code_object_without_scratch(libs, tmp_path):
    k = CO._kernel_notes(tmp_path)
    for tag in KERNELS:
        assert any(tag in name for name in k), (tag, sorted(k))
    nl = [v for name, v in k.items() if "hq_k_nl_element" in name]
    assert len(nl) == 1
    print("\n[nonlinear] hq_k_nl_element: %s" % nl[0])
    assert nl[0]["private_segment_fixed_size"] == 0 and nl[0]["vgpr_spill_count"] == 0 and nl[0]["sgpr_spill_count"] == 0
