"""Nonlinear soil beside the patch and brick step on the device (hq_nonlinear_set: hq_k_nl_element and hq_k_atten_node_sum on a
stream of their own, hq_k_distribute / hq_k_atten_apply_at / hq_k_adjust_assign behind the step).  The reference side, the plan,
the two rules and the criterion's teeth, without a device: tests/test_nonlinear_cpu.py.

One step per node and component: tm1 = u1 and tm2 = u2 drawn independently (tests/helpers.step_fields), the plastic strains and
ep LOADED so that about half the points yield (nl_reference.yielding_state), run(1).  Reference: nl_reference.extended in
np.longdouble; bound per node and component
    |got - ref| <= b 64 2^-53 T,
T the sum of the magnitudes of all addends, the correction's included, b the worst ratio of form (B) in double on the same
inputs (tests/test_nonlinear_cpu.B_ONE_STEP: 2.15 .. 3.14).  After the step the fetched state is hqh_nonlinear_advance's on the
same fields, bit for bit.
Worst device ratio |got - ref| / (2^-53 T) measured on an MI355X (bounds 138 .. 201):
    bricks 3.52   no_bricks 4.22   two_level 3.91   n1 3.10   n63 2.89   n64 2.98   n65 3.64   faces 2.96   empty 3.10

Checkpoints: the fixtures' runs from rest; bound 8 x the difference between form (B) in double and the fixture
(test_nonlinear_cpu.B_AGAINST_FIXTURE) -- summation order is the only freedom left, and yielding amplifies it.
Measured on an MI355X, rel. L-inf of tm1 at steps 100 / 200: c1_nl_vm 1.74e-12 / 5.77e-12 (bounds 1.38e-11 / 4.59e-11),
c1_nl_dp 2.04e-12 / 3.42e-12 (1.62e-11 / 2.72e-11), c5_two_level_nl 2.52e-12 / 6.47e-12 (2.02e-11 / 5.19e-11).

Determinism, restart and the context that never had it: on box32 without bricks (stencil patches), the one mesh on which two
fresh ELASTIC contexts leave identical bits (tests/test_gpu_attenuation_split.py's docstring).
"""
import functools

import numpy as np
import pytest

import hercules_amd as ha
from hercules_amd import capi, host
from tests import helpers as H
from tests import nl_reference as R
from tests import test_gpu_recorders as GR
from tests import test_nonlinear_cpu as C

if not np.finfo(np.longdouble).eps < 1e-18:
    pytest.skip("np.longdouble is no wider than double here: no extended reference", allow_module_level=True)

pytestmark = pytest.mark.gpu

SCATTER, PATCH = ha.HQ_VARIANT_SCATTER, ha.HQ_VARIANT_PATCH
EPS = 2.0 ** -53
bits = C.bits


def solver(p, u1=None, u2=None, variant=PATCH, options=None, **kw):
    return ha.Solver(p["lnid"], p["etable"], p["ntable"], p["dt"], tm1=u1, tm2=u2, dangling=p["dangling"], node_xyz=p["node_xyz"],
                     variant=variant, options=options or None, **kw)


def worst(got, ref, T):
    q = (np.abs(got.astype(np.longdouble) - ref) / (EPS * T)).astype(np.float64)
    n, d = np.unravel_index(np.argmax(q), q.shape)
    return float(q[n, d]), int(n), int(d)


@pytest.mark.parametrize("case", sorted(C.CASES))
def test_one_step_from_independent_fields_and_a_loaded_state(case):
    p, options, model, elems, cons, u1, u2, ps, ep, ref, T, _, ps1, ep1, b = C.reference(case)
    B = 64.0 * C.B_ONE_STEP[case]
    s = solver(p, u1, u2, options=options)
    try:
        elastic, before = s.dominant_kernel(), s.info()["device_bytes"]
        s.set_nonlinear(model, elems, cons)
        assert s.dominant_kernel() == elastic and s.info()["variant"] == PATCH
        s.nonlinear_load(ps, ep)
        a, e = s.nonlinear_fetch()
        assert np.array_equal(bits(a), bits(ps)) and np.array_equal(bits(e), bits(ep))
        s.run(1)
        got, old = s.download()
        state, nonfinite, info, ninfo = s.nonlinear_fetch(), s.check_finite(), s.info(), s.nonlinear_info()
    finally:
        s.close()
    if case == "bricks":
        assert info["brick_nodes"] > 0
    elif case == "no_bricks":
        assert info["brick_nodes"] == 0
    elif case == "two_level":
        assert len(p["dangling"][0]) > 0 and 0 < len(elems) < p["E"]
    touched = C.touched_nodes(p, elems)
    assert ninfo == dict(elements=len(elems), touched_nodes=len(touched) if len(elems) else 0, device_bytes=C.nl_bytes(p, elems, touched)), ninfo
    assert info["device_bytes"] - before == ninfo["device_bytes"]
    assert nonfinite == 0 and np.array_equal(old, u1)
    w = worst(got, ref, T)
    print("\n[nonlinear] %-10s nodes %6d elements %5d touched %5d brick nodes %5d worst %.2f x 2^-53 T at node %d.%d (bound %g)"
          % (case, p["N"], len(elems), ninfo["touched_nodes"], info["brick_nodes"], w[0], w[1], w[2], B))
    assert w[0] <= B, (w, got[w[1]], np.asarray(ref[w[1]], np.float64))
    # the state: hqh_nonlinear_advance on the same fields, bit for bit
    hp, he = ps.copy(), ep.copy()
    host.nonlinear_advance(np.asarray(p["lnid"])[elems], cons, u1, p["dt"], hp, he)
    assert np.array_equal(bits(state[0]), bits(hp)) and np.array_equal(bits(state[1]), bits(he))
    assert np.array_equal(bits(hp), bits(ps1)) and np.array_equal(bits(he), bits(ep1))


@pytest.mark.parametrize("name", C.FIXTURES)
def test_checkpoint_steps_against_the_fixtures(name):
    g, p = C.golden_problem(name)
    steps = [int(x) for x in g["ckpt_steps"]]
    s = solver(p)
    try:
        s.set_nonlinear(int(g["model"]), g["elems"], g["cons"])
        s.set_source(g["loaded_lnid"], g["forces"])
        done, d = 0, []
        for k, step in enumerate(steps):
            s.run(step - done)
            done = step
            tm1, tm2 = s.download()
            d.append((H.rel_linf(tm1, g["ckpt_tm1"][k]), H.rel_linf(tm2, g["ckpt_tm2"][k])))
        ep = s.nonlinear_fetch()[1]
        nonfinite = s.check_finite()
    finally:
        s.close()
    print("\n[nonlinear] %s: device against the fixture at steps %s, rel L-inf %s (bounds %s), yielded %.3f"
          % (name, steps, [("%.2e" % a, "%.2e" % b) for a, b in d], ["%.2e" % (8 * x) for x in C.B_AGAINST_FIXTURE[name]], (ep > 0).mean()))
    assert nonfinite == 0
    for k in range(len(steps)):
        assert max(d[k]) <= 8.0 * C.B_AGAINST_FIXTURE[name][k], (k, d)
    assert 0.01 < (ep > 0).mean() < 0.9


# ---------------------------------------------------------------------------------------------
# determinism, restart, a context without
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def box32():
    """box32 without bricks, every element in the top quarter of the depth and every third one below nonlinear; fields and a
    loaded state of the one-step kind."""
    p = H.source_mesh("box32")
    nx, ny, nz = p["shape"]
    edata = np.empty((p["E"], 4), np.float32)
    edata[:] = (10.0, 6000.0, 3464.0, 2700.0)
    elems_all, cons_all = host.nonlinear_constants(edata, R.DRUCKERPRAGER, C.PROPS[R.DRUCKERPRAGER], 0.0, 10000.0)
    pick = np.zeros(p["E"], bool)
    pick[::3] = True
    pick[: p["E"] // 4] = True
    elems = np.nonzero(pick)[0].astype(np.int32)
    cons = np.ascontiguousarray(cons_all[elems])
    u1, u2 = H.step_fields(p["N"], C.SEED)
    ps, ep = R.yielding_state(p, elems, cons, u1, C.STATE_SEED)
    for a in (elems, cons, u1, u2, ps, ep):
        a.flags.writeable = False
    return p, elems, cons, u1, u2, ps, ep


OPT32 = {"no_bricks": 1}


def run32(plan):
    """plan(s, inputs) on a fresh box32 context -> what it returns."""
    inputs = box32()
    p, elems, cons, u1, u2, ps, ep = inputs
    s = solver(p, u1, u2, options=OPT32)
    try:
        return plan(s, inputs)
    finally:
        s.close()


def _twenty(s, inputs):
    p, elems, cons, u1, u2, ps, ep = inputs
    s.set_nonlinear(R.DRUCKERPRAGER, elems, cons)
    s.nonlinear_load(ps, ep)
    s.run(20)
    return s.download() + s.nonlinear_fetch() + (s.check_finite(),)


def _ten_and_ten(s, inputs):
    p, elems, cons, u1, u2, ps, ep = inputs
    s.set_nonlinear(R.DRUCKERPRAGER, elems, cons)
    s.nonlinear_load(ps, ep)
    s.run(10)
    tm1, tm2 = s.download()
    a, e = s.nonlinear_fetch()
    s.upload(tm1, tm2, 10)
    z = s.nonlinear_fetch()
    assert not z[0].any() and not z[1].any()                                       # hq_upload zeroes the state
    s.nonlinear_load(a, e)
    s.run(10)
    return s.download() + s.nonlinear_fetch() + (s.check_finite(),)


def test_two_runs_leave_identical_bits_and_a_restart_continues_them():
    a, b, c = run32(_twenty), run32(_twenty), run32(_ten_and_ten)
    assert a[4] == 0 and (a[3] > 0).any() and (a[2] != box32()[5]).any()           # finite, and the state moved
    for k in range(4):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
        assert np.array_equal(bits(a[k]), bits(c[k])), k


def test_a_context_without_it_steps_as_before():
    def plain(s, inputs):
        before = s.info()["device_bytes"]
        assert s.nonlinear_info() == dict(elements=0, touched_nodes=0, device_bytes=0)
        s.run(10)
        return s.download(), before

    def set_and_cleared(s, inputs):
        p, elems, cons, u1, u2, ps, ep = inputs
        before = s.info()["device_bytes"]
        s.set_nonlinear(R.DRUCKERPRAGER, elems, cons)
        info = s.nonlinear_info()
        assert info["device_bytes"] == C.nl_bytes(p, elems, C.touched_nodes(p, elems)) > 0
        assert s.info()["device_bytes"] - before == info["device_bytes"]
        z = s.nonlinear_fetch()
        assert not z[0].any() and not z[1].any()                                   # the state starts at zero
        s.nonlinear_load(ps, ep)
        s.clear_nonlinear()
        assert s.info()["device_bytes"] == before and s.nonlinear_info()["device_bytes"] == 0
        with pytest.raises(ha.HqError, match="hq error -6"):
            s.nonlinear_fetch()
        s.run(10)
        return s.download(), before

    def set_empty(s, inputs):
        before = s.info()["device_bytes"]
        s.set_nonlinear(R.VONMISES, np.zeros(0, np.int32), np.zeros((0, 6)))
        assert s.nonlinear_info() == dict(elements=0, touched_nodes=0, device_bytes=0) and s.info()["device_bytes"] == before
        s.run(10)
        return s.download(), before

    (a, na), (b, nb), (c, nc) = run32(plain), run32(set_and_cleared), run32(set_empty)
    assert na == nb == nc
    for k in range(2):
        assert np.array_equal(bits(a[k]), bits(b[k])) and np.array_equal(bits(a[k]), bits(c[k])), k


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was():
    p, options, model, elems, cons, u1, u2, ps, ep, ref, T, _, ps1, ep1, b = C.reference("n65")
    B = 64.0 * C.B_ONE_STEP["n65"]
    # a scatter context
    s = solver(p, u1, u2, variant=SCATTER)
    try:
        with pytest.raises(ha.HqError, match=r"hq error -6: .*HQ_VARIANT_PATCH"):
            s.set_nonlinear(model, elems, cons)
        assert s.nonlinear_info()["elements"] == 0 and s.dominant_kernel() == "hq_k_element_scatter"
    finally:
        s.close()
    # the float library
    s = ha.Solver(p["lnid"], p["etable"], p["ntable"], p["dt"], dangling=None, node_xyz=p["node_xyz"], variant=PATCH, precision="f32")
    try:
        with pytest.raises(ha.HqError, match=r"hq error -6: .*float library"):
            s.set_nonlinear(model, elems, cons)
    finally:
        s.close()
    # partitions: nranks > 1, a linked group, a transport
    from tests import bkt_reference as BK
    q = BK.four_class_partition(4)
    g = q["glob"]
    solvers = []
    try:
        for r, part in enumerate(q["parts"]):
            solvers.append(ha.Solver(part["lnid"], q["ets"][r], q["nts"][r], g["dt"], an_sched=part["an_sched"], dn_sched=part["dn_sched"],
                                     rank=r, nranks=4, node_xyz=q["node_xyz"][r], variant=PATCH))
        some = np.arange(4, dtype=np.int32)
        with pytest.raises(ha.HqError, match=r"hq error -6: .*out of scope"):
            solvers[0].set_nonlinear(model, some, cons[:4])
        capi.group_link(solvers)
        with pytest.raises(ha.HqError, match=r"hq error -6: .*out of scope"):
            solvers[1].set_nonlinear(model, some, cons[:4])
        assert all(x.nonlinear_info()["elements"] == 0 for x in solvers)
    finally:
        for x in solvers:
            x.close()
    s = solver(p, u1, u2)                                            # one rank with a transport of its own
    try:
        s.comm_init_host(lambda recvs, sends, tag: None)
        with pytest.raises(ha.HqError, match=r"hq error -6: .*out of scope"):
            s.set_nonlinear(model, elems, cons)
        assert s.nonlinear_info()["elements"] == 0
    finally:
        s.close()
    # a context with attenuation: split on a patch context, and the scatter kind (refused as a scatter context)
    q = BK.problem("four7x5x4")
    s = solver(q)
    try:
        s.set_attenuation(q["coef"], q["freq"], split=True)
        with pytest.raises(ha.HqError, match=r"hq error -6: .*attenuation"):
            s.set_nonlinear(model, elems[elems < q["E"]], cons[elems < q["E"]])
        assert s.attenuation_split() and s.nonlinear_info()["elements"] == 0
    finally:
        s.close()
    s = solver(q, variant=SCATTER)
    try:
        s.set_attenuation(q["coef"], q["freq"])
        with pytest.raises(ha.HqError, match=r"hq error -6"):
            s.set_nonlinear(model, elems[elems < q["E"]], cons[elems < q["E"]])
    finally:
        s.close()
    # the description's own faults, and what a nonlinear context refuses: it stays as it was, and a correct call then succeeds
    s = solver(p, u1, u2, options=options)
    try:
        s.set_nonlinear(model, elems, cons)
        s.nonlinear_load(ps, ep)
        before = s.info()["device_bytes"]
        col = np.arange(6)
        for kw, text in ((dict(model=0), "unknown model"), (dict(model=3), "unknown model"), (dict(elems=elems[::-1]), "ascending"),
                         (dict(elems=np.where(np.arange(len(elems)) == 3, elems[2], elems)), "ascending"),
                         (dict(elems=elems + p["E"]), "out of range"), (dict(elems=elems - 1), "out of range"),
                         (dict(cons=np.where(col == 2, np.nan, cons)), "not finite"), (dict(cons=np.where(col == 5, np.inf, cons)), "not finite"),
                         (dict(cons=np.where(col == 0, 0.0, cons)), "h must be"), (dict(cons=np.where(col == 1, -1.0, cons)), "mu must be"),
                         (dict(cons=np.where(col == 4, -1.0, cons)), "k must be"),
                         (dict(model=R.VONMISES, cons=np.where(col == 3, 0.1, cons)), "alpha must be 0")):
            a = dict(model=model, elems=elems, cons=cons)
            a.update(kw)
            with pytest.raises(ha.HqError, match=r"hq error -1: .*" + text):
                s.set_nonlinear(a["model"], a["elems"], a["cons"])
        with pytest.raises(ha.HqError):
            s.set_nonlinear(model, elems, cons[:-1])
        with pytest.raises(ha.HqError, match=r"hq error -6: .*nonlinear soil"):
            s.comm_init(b"\0" * 128)
        with pytest.raises(ha.HqError, match=r"hq error -6: .*nonlinear soil"):
            s.comm_init_host(lambda recvs, sends, tag: None)
        with pytest.raises(ha.HqError, match=r"hq error -6: .*nonlinear soil"):
            s.comm_init_ipc(b"\0" * capi.IPC_BLOB_BYTES)
        with pytest.raises(ha.HqError, match=r"hq error -6: .*nonlinear soil"):
            capi.group_link([s])
        coef = np.zeros((p["E"], 10), np.float32)
        with pytest.raises(ha.HqError, match=r"hq error -6: .*nonlinear soil"):
            s.set_attenuation(coef, 5.0, split=True)
        with pytest.raises(ha.HqError, match=r"hq error -6"):
            s.set_attenuation(coef, 5.0)
        bad = ps.copy()
        bad[1, 2, 3] = np.nan
        with pytest.raises(ha.HqError, match=r"hq error -1: .*not finite"):
            s.nonlinear_load(bad, ep)
        assert s.info()["device_bytes"] == before and s.nonlinear_info()["elements"] == len(elems)
        st = s.nonlinear_fetch()
        assert np.array_equal(bits(st[0]), bits(ps)) and np.array_equal(bits(st[1]), bits(ep))
        s.run(1)
        w = worst(s.download()[0], ref, T)
        assert w[0] <= B, w
        s.set_nonlinear(model, elems, cons)                                          # a correct call after them: a fresh state
        st = s.nonlinear_fetch()
        assert not st[0].any() and not st[1].any() and s.info()["device_bytes"] == before
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------
# outputs on a nonlinear context
# ---------------------------------------------------------------------------------------------
def test_recorders_and_a_peak_tracker_equal_the_host_fold_of_the_runs_samples():
    """derivs = 2 reads u(t - 2 dt), the buffer the apply kernel writes: three steps enqueued as ONE batch against the rows an
    auxiliary unit-weight recorder took on the same trajectory, then three steps one at a time against hq_gather3; the peak
    tracker of the same points against hqh_peak_fold of the recorder's six samples."""
    p, options, model, elems, cons, u1, u2, ps, ep = C.reference("n65")[:9]
    rng = np.random.default_rng(5)
    ids = np.ascontiguousarray(np.asarray(p["lnid"])[[3, 77, 139]], np.int32)
    phi = rng.uniform(0.0, 0.25, (3, 8))
    quantities = capi.HQ_PEAK_DISP | capi.HQ_PEAK_VEL | capi.HQ_PEAK_ACC
    s = solver(p, u1, u2, options={"no_bricks": 1})
    try:
        s.set_nonlinear(model, elems, cons)
        s.nonlinear_load(ps, ep)
        h = s.record_add(ids, phi, 1, derivs=2, capacity=8)
        hr = GR._add_rows_recorder(s, ids, 8)
        hp = s.peak_add(ids, phi, rate=1, quantities=quantities)
        s.run(3)
        steps, vals = s.record_fetch(h)
        _, rows = s.record_fetch(hr)
        tm2, tm3 = GR._start_rows(s, ids, u2)
        want = GR._route_from_rows(rows, tm2, tm3, 0, [0, 1, 2], phi, p["dt"], 2)
        steps2, want2 = GR._per_step_route(s, ids, phi, p["dt"], 2, 1, 3)
        _, vals2 = s.record_fetch(h)
        peaks, when, nsamples = s.peak_fetch(hp)
    finally:
        s.close()
    assert list(steps) == [0, 1, 2] and list(steps2) == [3, 4, 5] and nsamples == 6
    assert np.abs(vals[2][:, 6:]).max() > 0
    assert np.array_equal(bits(vals), bits(want))
    assert np.array_equal(bits(vals2), bits(want2))
    fp, fw = host.peak_fold(np.concatenate([steps, steps2]), np.concatenate([vals, vals2]), quantities)
    assert np.array_equal(bits(peaks), bits(fp)) and np.array_equal(when, fw)
