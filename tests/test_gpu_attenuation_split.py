"""BKT attenuation beside the patch and brick step on the device (hq_attenuation_set_split: hq_k_atten_advance_delta,
hq_k_atten_corner_force, hq_k_atten_node_sum on a stream of their own, hq_k_distribute / hq_k_atten_apply / hq_k_adjust_assign
behind the step).  The reference side, the plan and the criterion's teeth, without a device: tests/test_attenuation_split_cpu.py.

One step per node, the criterion of tests/test_gpu_attenuation.py: tm1 = u1 and tm2 = u2 drawn independently
(tests/helpers.step_fields), the memory variables LOADED with independent random values (bkt_reference.random_state), run(1).
Reference: test_attenuation_cpu.extended in np.longdouble; bound per node and component
    |got - ref| <= B 2^-53 T,    B = 16 max(b, 4) = 64
b = the double restatement of the split step's own worst ratio on the same inputs, measured on the CPU (b < 4 asserted there):
    uniform70x20x12 1.34   four70x20x12 1.40   uniform32 1.40   four7x5x4 1.12 (every third node loaded: 1.12)   two_level 1.14
Worst device ratio |got - ref| / (2^-53 T) measured on an MI355X:
    uniform70x20x12 1.51   four70x20x12 1.50   uniform32 1.38   four7x5x4 1.27 (loaded 1.27)   two_level 1.58
After the step the fetched memory variables are the host text's (hqh_atten_advance over the slot plan) bit for bit.

Determinism, and the step after hq_attenuation_clear against a never-attenuated twin: the correction chain has one summation
order, so two fresh contexts leave identical bits wherever the ELASTIC step does.  That is uniform32 (stencil patches) alone of
the cases above: measured on an MI355X, two fresh unattenuated contexts differ after three steps in 1 481 (uniform70x20x12),
1 123 (four70x20x12), 154 (four7x5x4) and 336 (two_level) values -- the element-form patch kernels add with LDS atomics
(tests/test_gpu_recorders.py's docstring) -- and in none on uniform32.  So both tests run on uniform32."""
import numpy as np
import pytest

import hercules_amd as ha
from hercules_amd import capi
from tests import bkt_reference as R
from tests import helpers as H
from tests import test_attenuation_cpu as C
from tests import test_attenuation_split_cpu as S
from tests import test_gpu_recorders as GR

if not np.finfo(np.longdouble).eps < 1e-18:
    pytest.skip("np.longdouble is no wider than double here: no extended reference", allow_module_level=True)

pytestmark = pytest.mark.gpu

SCATTER, PATCH = ha.HQ_VARIANT_SCATTER, ha.HQ_VARIANT_PATCH
EPS = 2.0 ** -53
TOL = 1e-9                                                       # tests/test_gpu_parity.py:62-63
bits = C.bits


def solver(p, u1=None, u2=None, variant=PATCH, options=None, **kw):
    return ha.Solver(p["lnid"], p["etable"], p["ntable"], p["dt"], tm1=u1, tm2=u2, dangling=p["dangling"], node_xyz=p["node_xyz"],
                     variant=variant, options=options or None, **kw)


def worst(got, ref, T):
    q = (np.abs(got.astype(np.longdouble) - ref) / (EPS * T)).astype(np.float64)
    n, d = np.unravel_index(np.argmax(q), q.shape)
    return float(q[n, d]), int(n), int(d)


def one_step(case):
    """(u, u(t - dt), state, nonfinite, info) of one attenuated step of a fresh split context from the case's inputs."""
    p, plan, u1, u2, conv0, ids, F, options = S.reference(case)[:8]
    s = solver(p, u1, u2, options=options)
    try:
        elastic = s.dominant_kernel()
        s.set_attenuation(p["coef"], p["freq"], split=True)
        assert s.attenuation_split() and s.dominant_kernel() == elastic and s.info()["variant"] == PATCH
        s.load_attenuation_state(*conv0)
        if ids is not None:
            s.set_source(ids, F[None])
        s.run(1)
        got, old = s.download()
        return got, old, s.attenuation_state(), s.check_finite(), s.info(), s.attenuation_info()
    finally:
        s.close()


@pytest.mark.parametrize("case", sorted(S.CASES))
def test_one_step_from_independent_fields_and_memory_variables(case):
    p, plan, u1, u2, conv0, ids, F, options, ref, T, conv_host, b, _ = S.reference(case)
    assert b < 4.0
    B = 16.0 * max(b, 4.0)
    got, old, state, nonfinite, info, ainfo = one_step(case)
    if case == "uniform70x20x12":
        assert 2 * info["brick_nodes"] > p["N"], info["brick_nodes"]
    elif case == "four70x20x12":
        assert info["brick_nodes"] > 0
        assert (R.classes_seen(plan, p["N"]) > 1).any()
    elif options.get("no_bricks"):
        assert info["brick_nodes"] == 0
    if case == "two_level":
        assert len(p["dangling"][0]) > 0
    assert ainfo["slots"] == len(plan["slot_node"]) and ainfo["classes"] == len(plan["rows"])
    assert nonfinite == 0 and np.array_equal(old, u1)
    w = worst(got, ref, T)
    print("\n[attenuation split] %-18s nodes %6d slots %6d brick nodes %6d worst %.2f x 2^-53 T at node %d.%d (bound %g)"
          % (case, p["N"], len(plan["slot_node"]), info["brick_nodes"], w[0], w[1], w[2], B))
    assert w[0] <= B, (w, got[w[1]], np.asarray(ref[w[1]], np.float64))
    for v in range(4):
        assert np.array_equal(bits(state[v]), bits(conv_host[v])), v


def test_two_fresh_contexts_leave_identical_bits():
    a, b = one_step("uniform32"), one_step("uniform32")
    assert np.array_equal(bits(a[0]), bits(b[0]))
    for v in range(4):
        assert np.array_equal(bits(a[2][v]), bits(b[2][v])), v


def test_ten_steps_against_the_scatter_variant():
    p, plan, u1, u2, conv0 = S.reference("four70x20x12")[:5]
    out = []
    for variant, split in ((PATCH, True), (SCATTER, False)):
        s = solver(p, u1, u2, variant=variant)
        try:
            s.set_attenuation(p["coef"], p["freq"], split=split)
            s.load_attenuation_state(*conv0)
            s.run(10)
            out.append((s.download(), s.attenuation_state(), s.check_finite()))
        finally:
            s.close()
    (ua, sa, na), (ub, sb, nb) = out
    assert na == 0 and nb == 0
    d = [H.rel_linf(ua[k], ub[k]) for k in range(2)] + [H.rel_linf(sa[v], sb[v]) for v in range(4)]
    print("\n[attenuation split] ten steps of four70x20x12, split against scatter: rel L-inf fields %.2e %.2e, memory variables %s"
          % (d[0], d[1], ["%.2e" % x for x in d[2:]]))
    assert max(d) < TOL, d


def test_a_recorder_with_accelerations_returns_the_gathered_samples():
    """derivs = 2 reads u(t - 2 dt), the buffer the apply kernels write: three steps enqueued as ONE batch against the rows an
    auxiliary unit-weight recorder took on the same trajectory, then three steps one at a time against hq_gather3."""
    p, plan, u1, u2, conv0 = S.reference("four7x5x4")[:5]
    rng = np.random.default_rng(5)
    ids = np.ascontiguousarray(np.asarray(p["lnid"])[[3, 77, 139]], np.int32)
    phi = rng.uniform(0.0, 0.25, (3, 8))
    s = solver(p, u1, u2, options={"no_bricks": 1})
    try:
        s.set_attenuation(p["coef"], p["freq"], split=True)
        s.load_attenuation_state(*conv0)
        h = s.record_add(ids, phi, 1, derivs=2, capacity=8)
        hr = GR._add_rows_recorder(s, ids, 8)
        s.run(3)
        steps, vals = s.record_fetch(h)
        _, rows = s.record_fetch(hr)
        tm2, tm3 = GR._start_rows(s, ids, u2)
        want = GR._route_from_rows(rows, tm2, tm3, 0, [0, 1, 2], phi, p["dt"], 2)
        steps2, want2 = GR._per_step_route(s, ids, phi, p["dt"], 2, 1, 3)
        _, vals2 = s.record_fetch(h)
    finally:
        s.close()
    assert list(steps) == [0, 1, 2] and list(steps2) == [3, 4, 5]
    assert np.abs(vals[2][:, 6:]).max() > 0
    assert np.array_equal(bits(vals), bits(want))
    assert np.array_equal(bits(vals2), bits(want2))


def test_clear_gives_the_bytes_back_and_the_elastic_step():
    p, plan, u1, u2, conv0, _, _, options = S.reference("uniform32")[:8]
    s, plain = solver(p, u1, u2, options=options), solver(p, u1, u2, options=options)
    try:
        before = s.info()["device_bytes"]
        assert s.attenuation_info() == dict(classes=0, slots=0, device_bytes=0) and not s.attenuation_split()
        s.set_attenuation(p["coef"], p["freq"], split=True)
        info = s.attenuation_info()
        assert info["device_bytes"] == S.split_bytes(p, len(plan["slot_node"]), len(plan["rows"])), info
        assert s.info()["device_bytes"] - before == info["device_bytes"]
        assert all(not a.any() for a in s.attenuation_state())                      # the memory variables start at 0
        s.load_attenuation_state(*conv0)
        a = s.attenuation_state()
        assert all(np.array_equal(bits(a[v]), bits(conv0[v])) for v in range(4))
        s.upload(u1, u2, 0)                                                          # hq_upload zeroes the memory variables
        assert all(not x.any() for x in s.attenuation_state())
        s.clear_attenuation()
        assert s.info()["device_bytes"] == before and not s.attenuation_split()
        with pytest.raises(ha.HqError, match="hq error -6"):
            s.attenuation_state()
        s.run(1)
        plain.run(1)
        assert np.array_equal(bits(s.download()[0]), bits(plain.download()[0]))     # the step of a never-attenuated twin
    finally:
        s.close()
        plain.close()


@pytest.mark.parametrize("case", ["four70x20x12", "two_level"])
def test_info_is_the_headers_formula(case):
    p, plan = S.reference(case)[:2]
    s = solver(p)
    try:
        before = s.info()["device_bytes"]
        s.set_attenuation(p["coef"], p["freq"], split=True)
        info = s.attenuation_info()
        assert sorted(info) == ["classes", "device_bytes", "slots"]
        assert info["device_bytes"] == S.split_bytes(p, len(plan["slot_node"]), len(plan["rows"])), info
        assert s.info()["device_bytes"] - before == info["device_bytes"]
    finally:
        s.close()


def test_refusals_leave_the_context_as_it_was():
    p, plan, u1, u2, conv0, _, _, _, ref, T, _, b, _ = S.reference("four7x5x4")
    B = 16.0 * max(b, 4.0)
    coef, freq = p["coef"], p["freq"]
    # hq_attenuation_set on a patch context: today's message
    s = solver(p, u1, u2)
    try:
        with pytest.raises(ha.HqError, match=r"hq error -6: .*HQ_VARIANT_SCATTER"):
            s.set_attenuation(coef, freq)
        assert s.attenuation_info()["slots"] == 0
    finally:
        s.close()
    # a scatter context: the text names hq_attenuation_set
    s = solver(p, u1, u2, variant=SCATTER)
    try:
        with pytest.raises(ha.HqError, match=r"hq error -6: .*hq_attenuation_set\b"):
            s.set_attenuation(coef, freq, split=True)
        assert s.attenuation_info()["slots"] == 0 and s.dominant_kernel() == "hq_k_element_scatter"
    finally:
        s.close()
    # the float library
    s = ha.Solver(p["lnid"], p["etable"], p["ntable"], p["dt"], dangling=None, node_xyz=p["node_xyz"], variant=PATCH, precision="f32")
    try:
        with pytest.raises(ha.HqError, match=r"hq error -6: .*float library"):
            s.set_attenuation(coef, freq, split=True)
    finally:
        s.close()
    # partitions: nranks > 1, a linked group, a transport
    q = R.four_class_partition(4)
    g = q["glob"]
    solvers = []
    try:
        for r, part in enumerate(q["parts"]):
            solvers.append(ha.Solver(part["lnid"], q["ets"][r], q["nts"][r], g["dt"], an_sched=part["an_sched"], dn_sched=part["dn_sched"],
                                     rank=r, nranks=4, node_xyz=q["node_xyz"][r], variant=PATCH))
        with pytest.raises(ha.HqError, match=r"hq error -6: .*out of scope"):
            solvers[0].set_attenuation(q["coefs"][0], g["freq"], split=True)
        capi.group_link(solvers)
        with pytest.raises(ha.HqError, match=r"hq error -6: .*out of scope"):
            solvers[1].set_attenuation(q["coefs"][1], g["freq"], split=True)
        assert all(s.attenuation_info()["slots"] == 0 for s in solvers)
    finally:
        for s in solvers:
            s.close()
    s = solver(p, u1, u2)                                            # one rank with a transport of its own
    try:
        s.comm_init_host(lambda recvs, sends, tag: None)
        with pytest.raises(ha.HqError, match=r"hq error -6: .*out of scope"):
            s.set_attenuation(coef, freq, split=True)
        assert s.attenuation_info()["slots"] == 0
    finally:
        s.close()
    # an eTable with Rayleigh terms
    nx, ny, nz = p["shape"]
    damped = H.uniform_box(nx, ny, nz, h=20.0, dt=p["dt"], freq=20.0)
    assert (damped["etable"][:, 2:] != 0).any()
    s = ha.Solver(damped["lnid"], damped["etable"], damped["ntable"], p["dt"], node_xyz=damped["node_xyz"], variant=PATCH)
    try:
        with pytest.raises(ha.HqError, match=r"hq error -1: .*c3 or c4"):
            s.set_attenuation(coef, freq, split=True)
    finally:
        s.close()
    # freq, coefficients, transports and groups on a split context: it stays attenuated as it was, and a correct call then succeeds
    s = solver(p, u1, u2, options={"no_bricks": 1})
    try:
        s.set_attenuation(coef, freq, split=True)
        s.load_attenuation_state(*conv0)
        before = s.info()["device_bytes"]
        for f in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ha.HqError, match=r"hq error -1: .*freq"):
                s.set_attenuation(coef, f, split=True)
        for v in (np.nan, np.inf):
            bad = coef.copy()
            bad[17, 3] = v
            with pytest.raises(ha.HqError, match=r"hq error -1: .*not finite"):
                s.set_attenuation(bad, freq, split=True)
        with pytest.raises(ha.HqError):
            s.set_attenuation(coef[:-1], freq, split=True)
        with pytest.raises(ha.HqError, match=r"hq error -6: .*HQ_VARIANT_SCATTER"):
            s.set_attenuation(coef, freq)
        with pytest.raises(ha.HqError, match=r"hq error -6: .*split attenuation"):
            s.comm_init(b"\0" * 128)
        with pytest.raises(ha.HqError, match=r"hq error -6: .*split attenuation"):
            s.comm_init_host(lambda recvs, sends, tag: None)
        with pytest.raises(ha.HqError, match=r"hq error -6: .*split attenuation"):
            s.comm_init_ipc(b"\0" * capi.IPC_BLOB_BYTES)
        with pytest.raises(ha.HqError, match=r"hq error -6: .*split attenuation"):
            capi.group_link([s])
        assert s.attenuation_split() and s.info()["device_bytes"] == before
        assert all(np.array_equal(bits(s.attenuation_state()[v]), bits(conv0[v])) for v in range(4))
        s.run(1)
        w = worst(s.download()[0], ref, T)
        assert w[0] <= B, w
        s.set_attenuation(coef, freq, split=True)                                    # a correct call after them: a fresh state
        assert all(not x.any() for x in s.attenuation_state()) and s.info()["device_bytes"] == before
    finally:
        s.close()
