"""BKT constant-Q attenuation on the device (hq_attenuation_*: hq_k_atten_advance + hq_k_element_bkt in the scatter step).
The reference side, the slot plan and the criterion's teeth, without a device: tests/test_attenuation_cpu.py and
tests/bkt_reference.py (the reference's step restated, pinned bit for bit to the real program's checkpoints).

One step per node, the project's criterion (tests/test_gpu_step_terms.py): tm1 = u1 and tm2 = u2 drawn independently
(tests/helpers.step_fields), the memory variables LOADED with independent random values of the fields' size, consistent per
(node, class) slot, then run(1).  Reference: bkt_reference.extended_sums + helpers.extended_step in np.longdouble; T = the same
expression with every product replaced by its absolute value, the memory-variable terms included.  Bound per node and component
    |got - ref| <= B 2^-53 T,    B = 16 max(B_restatement, 4) = 64
B_restatement = the double restatement's own worst ratio on the same inputs, measured on the CPU:
    uniform9x7x5 0.87   four7x5x4 0.82 (every third node loaded: 0.82)   two_level 1.04   four7x5x4 on 4 ranks 1.05
Worst device ratio |got - ref| / (2^-53 T) measured on an MI355X:
    uniform9x7x5 0.78   four7x5x4 0.82 (loaded 0.76)   two_level 1.00   4 ranks 0.68 - 0.73;  hq_phase_force on four7x5x4 0.55 (of 2^-53 tf)
    the run of c1_bkt: fields 7.8e-15 relative at step 400, 6.5e-15 at step 800; memory variables 2.3e-15 at step 800
After the step the fetched memory variables are the host text's (hqh_atten_advance over the slot plan) bit for bit: they contain
no sum whose order can vary.

The run: all 800 steps of c1_bkt from rest with the fixture's forces against the restatement (= the reference's checkpoints,
bit for bit) under the relative tolerance 1e-9 at which tests/test_gpu_parity.py:62-63 holds the scatter variant's Rayleigh
run of c1_short (TOL there), fields at both checkpoints and the memory variables at the last."""
import functools

import numpy as np
import pytest

import hercules_amd as ha
from hercules_amd import capi, host
from tests import bkt_reference as R
from tests import helpers as H
from tests import test_attenuation_cpu as C

if not np.finfo(np.longdouble).eps < 1e-18:
    pytest.skip("np.longdouble is no wider than double here: no extended reference", allow_module_level=True)

pytestmark = pytest.mark.gpu

SCATTER, PATCH = ha.HQ_VARIANT_SCATTER, ha.HQ_VARIANT_PATCH
EPS = 2.0 ** -53
TOL = 1e-9                                                       # tests/test_gpu_parity.py:62-63
bits = C.bits


def solver(p, u1=None, u2=None, variant=SCATTER, **kw):
    return ha.Solver(p["lnid"], p["etable"], p["ntable"], p["dt"], tm1=u1, tm2=u2, dangling=p["dangling"], node_xyz=p["node_xyz"],
                     variant=variant, **kw)


@functools.lru_cache(maxsize=None)
def reference(name, loaded):
    """(p, plan, u1, u2, conv0, ids, F, ref, T, conv_host, B) of a case, computed once and read-only: conv_host = the memory
    variables after the step by the host text over the slot plan, in the per-corner layout."""
    p, plan, u1, u2, conv0, ids, F = C.step_inputs(name, loaded)
    ref, T, _ = C.extended(p, u1, u2, conv0, ids, F)
    conv = conv0.copy()
    rest = R.bkt_step(p["lnid"], p["etable"], p["ntable"], p["coef"], p["freq"], p["dt"], u1, u2, conv, p["dangling"], ids, F)
    b = float((np.abs(rest - ref) / (EPS * T)).max())
    assert b < 4.0, b                                             # (a broken reference cannot inflate the bar)
    k, _ = host.atten_class_coef(plan["rows"], p["freq"], p["dt"])
    mv, _ = host.atten_advance(plan["slot_node"], plan["slot_class"], k, u1, u2, R.corners_to_slots(plan, conv0))
    conv_host = R.slots_to_corners(plan, mv)
    assert np.array_equal(bits(conv_host), bits(conv))
    for a in (u1, u2, conv0, ref, T, conv_host):
        a.flags.writeable = False
    return p, plan, u1, u2, conv0, ids, F, ref, T, conv_host, 16.0 * max(b, 4.0)


def worst(got, ref, T):
    q = (np.abs(got.astype(np.longdouble) - ref) / (EPS * T)).astype(np.float64)
    n, d = np.unravel_index(np.argmax(q), q.shape)
    return float(q[n, d]), int(n), int(d)


@pytest.mark.parametrize("name,loaded", [("uniform9x7x5", False), ("four7x5x4", False), ("four7x5x4", True), ("two_level", False)])
def test_one_step_from_independent_fields_and_memory_variables(name, loaded):
    p, plan, u1, u2, conv0, ids, F, ref, T, conv_host, B = reference(name, loaded)
    s = solver(p, u1, u2)
    try:
        s.set_attenuation(p["coef"], p["freq"])
        assert s.dominant_kernel() == "hq_k_element_bkt" and s.info()["variant"] == SCATTER
        assert s.attenuation_info()["slots"] == len(plan["slot_node"]) and s.attenuation_info()["classes"] == len(plan["rows"])
        s.load_attenuation_state(*conv0)
        if loaded:
            s.set_source(ids, F[None])
        s.run(1)
        got, old = s.download()
        state = s.attenuation_state()
        nonfinite = s.check_finite()
    finally:
        s.close()
    assert nonfinite == 0 and np.array_equal(old, u1)
    w = worst(got, ref, T)
    print("\n[attenuation] %-14s %-7s nodes %5d slots %5d worst %.2f x 2^-53 T at node %d.%d (bound %g)"
          % (name, "loaded" if loaded else "", p["N"], len(plan["slot_node"]), w[0], w[1], w[2], B))
    assert w[0] <= B, (w, got[w[1]], np.asarray(ref[w[1]], np.float64))
    for v in range(4):
        assert np.array_equal(bits(state[v]), bits(conv_host[v])), v


def test_phase_force_exposes_the_bkt_force():
    p, plan, u1, u2, conv0, _, _, _, _, conv_host, B = reference("four7x5x4", False)
    f, tf, _ = R.extended_sums(p["lnid"], p["etable"], p["coef"], p["freq"], p["dt"], u1, u2, conv0, p["N"])
    s = solver(p, u1, u2)
    try:
        s.set_attenuation(p["coef"], p["freq"])
        s.load_attenuation_state(*conv0)
        s.phase_force()
        got = s.download_force()
        state = s.attenuation_state()
    finally:
        s.close()
    w = worst(got, f, tf)
    print("\n[attenuation] hq_phase_force four7x5x4: worst %.2f x 2^-53 tf at node %d.%d" % w)
    assert w[0] <= B, w
    for v in range(4):
        assert np.array_equal(bits(state[v]), bits(conv_host[v])), v


def test_one_step_on_four_ranks_in_one_process():
    """The four-class box on 4 contexts linked in one process: every harbored copy of every rank against the one-domain
    reference, and every rank's memory variables -- at shared nodes too -- against the host text."""
    q = R.four_class_partition(4)
    g = q["glob"]
    plan = R.slot_plan(g["lnid"], g["coef"])
    u1, u2 = H.step_fields(g["N"], C.SEED)
    conv0 = R.random_state(plan, C.STATE_SEED)
    ref, T, _ = C.extended(g, u1, u2, conv0)
    conv = conv0.copy()
    rest = R.bkt_step(g["lnid"], g["etable"], g["ntable"], g["coef"], g["freq"], g["dt"], u1, u2, conv, None)
    b = float((np.abs(rest - ref) / (EPS * T)).max())
    assert b < 4.0, b
    B = 16.0 * max(b, 4.0)
    k, _ = host.atten_class_coef(plan["rows"], g["freq"], g["dt"])
    mv, _ = host.atten_advance(plan["slot_node"], plan["slot_class"], k, u1, u2, R.corners_to_slots(plan, conv0))
    conv_host = R.slots_to_corners(plan, mv).reshape(4, g["E"], 8, 3)
    c0 = conv0.reshape(4, g["E"], 8, 3)
    solvers = []
    try:
        shared = 0
        for r, part in enumerate(q["parts"]):
            assert np.array_equal(q["gid"][r][np.asarray(part["lnid"])], np.asarray(g["lnid"])[part["elems"]])      # the same corners
            s = ha.Solver(part["lnid"], q["ets"][r], q["nts"][r], g["dt"], tm1=u1[q["gid"][r]], tm2=u2[q["gid"][r]],
                          an_sched=part["an_sched"], dn_sched=part["dn_sched"], rank=r, nranks=4, node_xyz=q["node_xyz"][r], variant=SCATTER)
            solvers.append(s)
            s.set_attenuation(q["coefs"][r], g["freq"])
            s.load_attenuation_state(*[np.ascontiguousarray(c0[v][part["elems"]]).reshape(-1, 3) for v in range(4)])
            shared += sum(len(m) for _, m in part["an_sched"]["s"])
        assert shared > 0
        capi.group_link(solvers)
        capi.group_run(solvers, 1)
        got = [s.download()[0] for s in solvers]
        states = [s.attenuation_state() for s in solvers]
    finally:
        for s in solvers:
            s.close()
    ratios = []
    for r, part in enumerate(q["parts"]):
        w = worst(got[r], ref[q["gid"][r]], T[q["gid"][r]])
        ratios.append(w[0])
        assert w[0] <= B, (r, w)
        for v in range(4):
            want = np.ascontiguousarray(conv_host[v][part["elems"]]).reshape(-1, 3)
            assert np.array_equal(bits(states[r][v]), bits(want)), (r, v)
    print("\n[attenuation] four7x5x4 on 4 ranks: B_restatement %.2f, worst per rank %s x 2^-53 T" % (b, ["%.2f" % x for x in ratios]))


def test_c1_bkt_run_against_the_restatement():
    g, p = C.golden_problem("c1_bkt")
    kept = C.golden_run("c1_bkt")
    s = ha.Solver(p["lnid"], p["etable"], p["ntable"], p["dt"], variant=SCATTER)
    try:
        s.set_attenuation(p["coef"], p["freq"])
        s.set_source(g["loaded_lnid"], g["forces"])
        done = 0
        for step in [int(x) for x in g["ckpt_steps"]]:
            s.run(step - done)
            done = step
            tm1, tm2 = s.download()
            d = H.rel_linf(tm1, kept[step][0]), H.rel_linf(tm2, kept[step][1])
            print("\n[attenuation] c1_bkt step %d: rel L-inf %.2e %.2e" % (step, d[0], d[1]))
            assert max(d) < TOL, (step, d)
        state = s.attenuation_state()
    finally:
        s.close()
    for v in range(2):                                           # (c1's dilatation is off: its variables stay 0)
        d = H.rel_linf(state[v], kept[done][2][v])
        print("[attenuation] c1_bkt memory variable %d at step %d: rel L-inf %.2e" % (v, done, d))
        assert d < TOL, (v, d)
    assert not state[2].any() and not state[3].any() and not kept[done][2][2:].any()


def test_state_fetch_load_upload_clear_and_info():
    p, plan, u1, u2, conv0, _, _, _, _, _, _ = reference("four7x5x4", False)
    Epad = (p["E"] + 63) & ~63
    s, plain = solver(p, u1, u2), solver(p, u1, u2)
    try:
        before = s.info()["device_bytes"]
        assert s.attenuation_info() == dict(classes=0, slots=0, device_bytes=0)
        s.set_attenuation(p["coef"], p["freq"])
        info = s.attenuation_info()
        ns, nc = len(plan["slot_node"]), len(plan["rows"])
        assert info == dict(classes=nc, slots=ns, device_bytes=144 * ns + 32 * Epad + 8 * ns + 144 * nc), info
        assert s.info()["device_bytes"] - before == info["device_bytes"]
        assert all(not a.any() for a in s.attenuation_state())                      # the memory variables start at 0
        s.load_attenuation_state(*conv0)
        a = s.attenuation_state()
        assert all(np.array_equal(bits(a[v]), bits(conv0[v])) for v in range(4))
        s.load_attenuation_state(*a)
        b = s.attenuation_state()
        assert all(np.array_equal(bits(a[v]), bits(b[v])) for v in range(4))        # fetch -> load -> fetch: identical bits
        # two corners of one slot that differ: refused, the node named, the state kept
        slot = int(np.argmax(np.bincount(plan["eslot"].ravel()) > 1))               # a slot that several corners read
        twin = np.argwhere(plan["eslot"] == slot)
        assert len(twin) > 1
        bad = [x.copy() for x in conv0]
        bad[1][8 * twin[1][0] + twin[1][1], 2] += 1e-9
        with pytest.raises(ha.HqError, match=r"hq error -1: .*node %d " % int(plan["slot_node"][slot])):
            s.load_attenuation_state(*bad)
        assert all(np.array_equal(bits(s.attenuation_state()[v]), bits(conv0[v])) for v in range(4))
        s.upload(u1, u2, 0)                                                          # hq_upload zeroes the memory variables
        assert all(not x.any() for x in s.attenuation_state())
        s.clear_attenuation()
        assert s.info()["device_bytes"] == before and s.dominant_kernel() == "hq_k_element_scatter"
        with pytest.raises(ha.HqError, match="hq error -6"):
            s.attenuation_state()
        s.run(1)
        plain.run(1)
        assert H.rel_linf(s.download()[0], plain.download()[0]) < TOL               # back to the step of the eTable
    finally:
        s.close()
        plain.close()


def test_refusals_leave_the_context_as_it_was():
    p, plan, u1, u2, conv0, _, _, ref, T, _, B = reference("four7x5x4", False)
    coef, freq = p["coef"], p["freq"]
    # the patch variant
    s = solver(p, u1, u2, variant=PATCH)
    try:
        with pytest.raises(ha.HqError, match=r"hq error -6: .*HQ_VARIANT_SCATTER"):
            s.set_attenuation(coef, freq)
        assert s.attenuation_info()["slots"] == 0
    finally:
        s.close()
    # the float library
    s = ha.Solver(p["lnid"], p["etable"], p["ntable"], p["dt"], dangling=None, node_xyz=p["node_xyz"], variant=SCATTER, precision="f32")
    try:
        with pytest.raises(ha.HqError, match=r"hq error -6: .*float library"):
            s.set_attenuation(coef, freq)
    finally:
        s.close()
    # an eTable with Rayleigh terms
    nx, ny, nz = p["shape"]
    damped = H.uniform_box(nx, ny, nz, h=20.0, dt=p["dt"], freq=20.0)
    assert (damped["etable"][:, 2:] != 0).any()
    s = ha.Solver(damped["lnid"], damped["etable"], damped["ntable"], p["dt"], node_xyz=damped["node_xyz"], variant=SCATTER)
    try:
        with pytest.raises(ha.HqError, match=r"hq error -1: .*c3 or c4"):
            s.set_attenuation(coef, freq)
    finally:
        s.close()
    # freq and coefficients; every refusal leaves an attenuated context attenuated as it was, and a correct call then succeeds
    s = solver(p, u1, u2)
    try:
        s.set_attenuation(coef, freq)
        s.load_attenuation_state(*conv0)
        for f in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ha.HqError, match=r"hq error -1: .*freq"):
                s.set_attenuation(coef, f)
        for v in (np.nan, np.inf):
            bad = coef.copy()
            bad[17, 3] = v
            with pytest.raises(ha.HqError, match=r"hq error -1: .*not finite"):
                s.set_attenuation(bad, freq)
        with pytest.raises(ha.HqError):
            s.set_attenuation(coef[:-1], freq)
        assert all(np.array_equal(bits(s.attenuation_state()[v]), bits(conv0[v])) for v in range(4))
        s.run(1)
        w = worst(s.download()[0], ref, T)
        assert w[0] <= B, w
        s.set_attenuation(coef, freq)                                                # a correct call after them: a fresh state
        assert all(not x.any() for x in s.attenuation_state())
    finally:
        s.close()


def test_a_recorder_on_an_attenuated_context_returns_the_gathered_samples():
    p, plan, u1, u2, conv0, _, _, _, _, _, _ = reference("four7x5x4", False)
    rng = np.random.default_rng(5)
    ids = np.ascontiguousarray(np.asarray(p["lnid"])[[3, 77, 139]], np.int32)
    phi = rng.uniform(0.0, 0.25, (3, 8))
    s = solver(p, u1, u2)
    try:
        s.set_attenuation(p["coef"], p["freq"])
        s.load_attenuation_state(*conv0)
        h = s.record_add(ids, phi, 1)
        want = []
        for _ in range(3):
            u, _ = s.gather(ids.reshape(-1))
            u = u.reshape(3, 8, 3)
            d = np.zeros((3, 3))
            for c in range(8):                                   # hq_sample_disp's order: d = d + w u, node by node
                d = d + phi[:, c:c + 1] * u[:, c, :]
            want.append(d)
            s.run(1)
        steps, vals = s.record_fetch(h)
    finally:
        s.close()
    assert list(steps) == [0, 1, 2] and np.array_equal(bits(vals), bits(np.stack(want)))
