"""BKT attenuation beside the patch and brick step (hq_attenuation_set_split; csrc/hq_atten_split.h), without a device.

split_step() restates the split step in numpy doubles: the ELASTIC step (tests/bkt_reference.bkt_step with all-zero rows: every
damping vector is u1 itself), the delta vectors ds, dk by the host text (hqh_atten_advance_delta over the slot plan), the
element forces of (ds, dk), dF summed per node in element order as hq_k_atten_node_sum does, compute_adjust DISTRIBUTION of dF,
u_new += dF / n_t[0], compute_adjust ASSIGNMENT.  It is compared with the extended reference of the attenuated step
(test_attenuation_cpu.extended, np.longdouble) on every mesh tests/test_gpu_attenuation_split.py uses; its worst ratio b of
|got - ref| / (2^-53 T) sets the device bound B = 16 max(b, 4), the rule of tests/test_gpu_attenuation.py, with b < 4 asserted.

b measured here:  uniform70x20x12 1.34   four70x20x12 1.40   uniform32 1.40   four7x5x4 1.12 (every third node loaded: 1.12)
two_level 1.14

  teeth    the criterion trips at the nodes concerned, and only there: the final division left out, dF's distribution left out,
           dk taken for ds, one (element, corner) entry dropped from a node's list
  state    the memory variables of the delta advance == hqh_atten_advance's, bit for bit
  plan     hq_attenuation_split_plan_check: 0 faults on the meshes, the bytes of the header's formula; a fault planted in a
           copy of the tables is counted
  exports  both libraries, ABI 6; the new kernels in the gfx950 code object, by name
"""
import functools

import numpy as np
import pytest

import hercules_amd as ha
from hercules_amd import build as hbuild
from hercules_amd import capi, host
from oracle import herc_oracle as ho
from tests import bkt_reference as R
from tests import helpers as H
from tests import test_attenuation_cpu as C
from tests import test_code_object_cpu as CO

EPS = 2.0 ** -53
NAMES = ["hq_attenuation_set_split", "hq_attenuation_split_plan_check", "hq_attenuation_split_plan_tables",
         "hq_attenuation_split_table_faults"]
KERNELS = ["hq_k_atten_advance_delta", "hq_k_atten_corner_force", "hq_k_atten_node_sum", "hq_k_atten_apply"]
bits = C.bits

# case -> (problem, hq_options of the GPU test's context, every third node loaded)
CASES = {
    "uniform70x20x12": (lambda: R.uniform_problem(70, 20, 12), {}, False),
    "four70x20x12": (lambda: R.four_class_problem(70, 20, 12), {}, False),
    "uniform32": (lambda: R.uniform_problem(32, 32, 32), {"no_bricks": 1}, False),
    "four7x5x4": (lambda: R.problem("four7x5x4"), {"no_bricks": 1}, False),
    "four7x5x4_loaded": (lambda: R.problem("four7x5x4"), {"no_bricks": 1}, True),
    "two_level": (lambda: R.problem("two_level"), {}, False),
}

needs_longdouble = C.needs_longdouble


@pytest.fixture(scope="module")
def libs():
    hbuild.build()
    return ha.load_library(), capi.load_library(precision="f32")


def case_inputs(case):
    """(p, plan, u1, u2, conv0, loaded ids, F, options) of a case: test_attenuation_cpu.step_inputs for any problem."""
    make, options, loaded = CASES[case]
    p = make()
    plan = R.slot_plan(p["lnid"], p["coef"])
    u1, u2 = H.step_fields(p["N"], C.SEED, p["dangling"])
    conv0 = R.random_state(plan, C.STATE_SEED)
    ids = F = None
    if loaded:
        ids = np.arange(0, p["N"], 3, dtype=np.int32)
        F = np.ascontiguousarray(H.rest_forces(p["ntable"][:, 0], p["dt"], C.SEED + 1)[ids])
    return p, plan, u1, u2, conv0, ids, F, options


def host_state(p, plan, u1, u2, conv0, delta=False):
    """The memory variables after one step by the host text over the slot plan, per corner, and the rows w [6, nslots]."""
    k, _ = host.atten_class_coef(plan["rows"], p["freq"], p["dt"])
    mv, w = host.atten_advance(plan["slot_node"], plan["slot_class"], k, u1, u2, R.corners_to_slots(plan, conv0), delta=delta)
    return R.slots_to_corners(plan, mv), w


def split_step(p, plan, u1, u2, conv0, ids=None, F=None, no_division=False, no_distribution=False, dk_for_ds=False, drop=None):
    """The split step in doubles (the module's docstring) -> (u_new [N, 3], the memory variables per corner).  The keywords
    plant the faults of the teeth test; drop = (element, corner) whose entry is left out of its node's sum."""
    lnid = np.asarray(p["lnid"], np.int64)
    E, N = len(lnid), p["N"]
    nt = np.asarray(p["ntable"], np.float64)
    dangling = p["dangling"]
    hanging = dangling is not None and len(dangling[0]) > 0
    elastic = R.bkt_step(p["lnid"], p["etable"], p["ntable"], np.zeros((E, 10), np.float32), p["freq"], p["dt"], u1, u2, R.new_state(E),
                         dangling, ids, F)
    conv, w = host_state(p, plan, u1, u2, conv0, delta=True)
    es = plan["eslot"]
    ds = np.stack([w[d][es] for d in range(3)], axis=2)              # [E, 8, 3]
    dk = np.stack([w[3 + d][es] for d in range(3)], axis=2)
    ef = R.element_forces(np.asarray(p["etable"], np.float64), dk if dk_for_ds else ds, dk)
    if drop is not None:
        ef[drop[0], drop[1]] = 0.0
    dF = np.zeros((N, 3))
    np.add.at(dF, lnid.reshape(-1), ef.reshape(-1, 3))               # element order, inside an element corner order
    if hanging and not no_distribution:
        ho.compute_adjust(dF, 0, dangling)
    new = np.ascontiguousarray(elastic + (dF if no_division else dF / nt[:, :1]))
    if hanging:
        ho.compute_adjust(new, 1, dangling)
    return new, conv


@functools.lru_cache(maxsize=None)
def reference(case):
    """(p, plan, u1, u2, conv0, ids, F, options, ref, T, conv_host, b) of a case, once per process and read-only."""
    p, plan, u1, u2, conv0, ids, F, options = case_inputs(case)
    ref, T, _ = C.extended(p, u1, u2, conv0, ids, F)
    got, conv = split_step(p, plan, u1, u2, conv0, ids, F)
    b = float((np.abs(got - ref) / (EPS * T)).max())
    conv_host, _ = host_state(p, plan, u1, u2, conv0)
    for a in (u1, u2, conv0, ref, T, conv_host, conv):
        a.flags.writeable = False
    return p, plan, u1, u2, conv0, ids, F, options, ref, T, conv_host, b, conv


@needs_longdouble
@pytest.mark.parametrize("case", sorted(CASES))
def test_restated_split_step_against_the_extended_reference(libs, case):
    p, plan, u1, u2, conv0, ids, F, options, ref, T, conv_host, b, conv = reference(case)
    print("\n[attenuation split] B_restatement %-18s %.3f" % (case, b))
    assert b < 4.0, b
    # the memory variables of the delta advance are hqh_atten_advance's bit for bit, and the restatement's own per-corner arrays'
    assert np.array_equal(bits(conv), bits(conv_host))
    mine = conv0.copy()
    R.calc_conv(np.asarray(p["lnid"], np.int64), R.class_coef(p["coef"], p["freq"], p["dt"]), u1, u2, mine)
    assert np.array_equal(bits(conv), bits(mine))


@needs_longdouble
def test_delta_vectors_are_the_damping_vectors_without_u1(libs):
    p, plan, u1, u2, conv0, _, _, _, _, _, _, _, _ = reference("four7x5x4")
    _, w = host_state(p, plan, u1, u2, conv0)
    _, dw = host_state(p, plan, u1, u2, conv0, delta=True)
    un = np.concatenate([u1[plan["slot_node"]].T, u1[plan["slot_node"]].T])
    assert np.array_equal(bits(dw + un), bits(w))                       # the one addition the delta form leaves out
    K = R.class_coef(plan["rows"], p["freq"], p["dt"])
    off = ~K["csum_on"][plan["slot_class"]]                             # csum == 0: nothing is added
    assert off[:, 0].any() and not dw[:3, off[:, 0]].any() and not dw[3:, off[:, 1]].any()


@needs_longdouble
@pytest.mark.parametrize("tooth", ["no_division", "no_distribution", "dk_for_ds", "entry_dropped"])
def test_criterion_trips_at_the_nodes_concerned_and_only_there(libs, tooth):
    case = "two_level" if tooth == "no_distribution" else "four7x5x4"
    p, plan, u1, u2, conv0, ids, F, _, ref, T, _, b, _ = reference(case)
    B = 16.0 * max(b, 4.0)
    lnid = np.asarray(p["lnid"], np.int64)
    K = R.class_coef(p["coef"], p["freq"], p["dt"])
    damped = np.unique(lnid[K["csum_on"].any(axis=1)])                  # nodes with an element that adds anything
    if tooth == "no_division":
        kw, concerned = dict(no_division=True), damped
    elif tooth == "dk_for_ds":
        kw, concerned = dict(dk_for_ds=True), damped
    elif tooth == "no_distribution":
        ids_, ptr, anc = [np.asarray(a, np.int64) for a in p["dangling"]]
        kw = dict(no_distribution=True)
        anchors = np.unique(anc)
        # an anchor loses its hanging nodes' shares; a hanging node is the mean of its anchors
        concerned = np.union1d(anchors, ids_)
    else:
        e, i = p["E"] // 2, 5
        assert K["csum_on"][e].any()
        kw, concerned = dict(drop=(e, i)), np.array([lnid[e, i]])
    got, _ = split_step(p, plan, u1, u2, conv0, ids, F, **kw)
    tripped = np.nonzero((np.abs(got - ref) > B * EPS * T).any(axis=1))[0]
    print("\n[attenuation split] tooth %-16s tripped %d of %d concerned (of %d nodes)" % (tooth, len(tripped), len(concerned), p["N"]))
    assert len(tripped) > 0 and np.isin(tripped, concerned).all(), (tooth, len(tripped), len(concerned))
    assert len(concerned) < p["N"] or tooth in ("no_division", "dk_for_ds")
    if tooth == "entry_dropped":
        assert list(tripped) == list(concerned)
    elif tooth == "no_distribution":
        assert np.isin(anchors, tripped).mean() >= 0.9
    else:
        assert len(tripped) >= 0.9 * len(concerned)
    good, _ = split_step(p, plan, u1, u2, conv0, ids, F)
    assert (np.abs(good - ref) <= B * EPS * T).all()


# ---------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------
def desc_of(p):
    return H.solver_desc(dict(p, node_xyz=p["node_xyz"]))


def split_bytes(p, slots, classes):
    """include/hq_solver.h's formula."""
    E, N = p["E"], p["N"]
    Epad = (E + 63) & ~63
    n = 144 * slots + 32 * Epad + 8 * slots + 144 * classes + 192 * Epad + 48 * E + 4 * (N + 1) + 32 * N
    if p["dangling"] is not None and len(p["dangling"][0]):
        n += 8 * len(np.unique(p["dangling"][2])) + 4 + 8 * len(p["dangling"][2])
    return n


@pytest.mark.parametrize("case", [c for c in sorted(CASES) if c != "four7x5x4_loaded"])
def test_split_plan_check(libs, case):
    p = CASES[case][0]()
    plan = R.slot_plan(p["lnid"], p["coef"])
    d = desc_of(p)
    rep = capi.attenuation_split_plan_check(d, p["coef"])
    assert rep == dict(classes=len(plan["rows"]), slots=len(plan["slot_node"]), faults=0,
                       device_bytes=split_bytes(p, len(plan["slot_node"]), len(plan["rows"]))), rep
    epos, nptr, nent, sd = capi.attenuation_split_plan_tables(d)
    E, N = p["E"], p["N"]
    Epad = (E + 63) & ~63
    assert len(nptr) == N + 1 and nptr[0] == 0 and nptr[-1] == 8 * E and len(nent) == 8 * E
    assert np.array_equal(np.sort(epos), np.arange(E))                                                 # the device's element order
    assert len(np.unique(nent)) == 8 * E and (nent % Epad < E).all() and (nent // Epad < 8).all()      # every corner exactly once
    elem = np.argsort(epos)[nent % Epad]                                                               # the caller's element of every entry
    inside = np.ones(8 * E, bool)
    inside[nptr[:-1][np.diff(nptr) > 0]] = False
    assert (np.diff(elem)[inside[1:]] > 0).all()                                                       # per node: the caller's element order
    assert capi.attenuation_split_table_faults(d, epos, nptr, nent, sd) == 0
    twice = epos.copy()
    twice[1] = twice[0]
    assert capi.attenuation_split_table_faults(d, twice, nptr, nent, sd) > 0
    # planted faults, each counted: an entry naming another corner, two entries of a node out of element order, a pair dropped
    node = int(np.argmax(np.diff(nptr) >= 2))
    q = int(nptr[node])
    bad = nent.copy()
    bad[q] = nent[q + 1]
    assert capi.attenuation_split_table_faults(d, epos, nptr, bad, sd) >= 2                                  # one twice, one never
    bad = nent.copy()
    bad[q], bad[q + 1] = nent[q + 1], nent[q]
    assert capi.attenuation_split_table_faults(d, epos, nptr, bad, sd) == 1
    short = nptr.copy()
    short[-1] -= 1
    assert capi.attenuation_split_table_faults(d, epos, short, nent, sd) > 0
    if len(sd):
        assert capi.attenuation_split_table_faults(d, epos, nptr, nent, sd[:-1]) == 1
        wrong = sd.copy()
        wrong[0, 2] += 1
        assert capi.attenuation_split_table_faults(d, epos, nptr, nent, wrong) == 1
    else:
        assert p["dangling"] is None


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
    assert "hqh_atten_advance_delta" in host.EXPORTS and hasattr(h, "hqh_atten_advance_delta")


def test_null_arguments_are_refused(libs):
    import ctypes
    for lib in libs:
        out = (ctypes.c_int64 * 4)()
        d = capi._AttenuationDesc(None, 1.0)
        assert lib.hq_attenuation_set_split(None, ctypes.byref(d)) == -1
        assert lib.hq_attenuation_split_plan_check(None, None, out) == -1
        assert lib.hq_attenuation_split_plan_tables(None, None, None, None, None, None) == -1
        assert lib.hq_attenuation_split_table_faults(None, None, None, None, None, ctypes.c_int64(0), None) == -1


def test_kernels_in_the_code_object(tmp_path):
    k = CO._kernel_notes(tmp_path)
    for tag in KERNELS:
        assert any(tag in name for name in k), (tag, sorted(k))
