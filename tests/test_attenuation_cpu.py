"""BKT constant-Q attenuation without a device (include/hq_solver.h: hq_attenuation_*; csrc/hq_atten.h, hq_atten_plan.h;
include/hq_host.h: hqh_atten_class_coef / hqh_atten_advance).  The reference side is tests/bkt_reference.py: the reference's
per-element-corner step restated in numpy doubles, and the same step in np.longdouble through the element matrices.

  fixtures   (tests/golden/c1_bkt.npz, c5_two_level_bkt.npz, from the real reference run with type_of_damping = bkt by
             tests/golden/make_golden_attenuation.py) pin the restatement to the reference's checkpoints bit for bit
  slot form  hqh_atten_advance over the slot plan == the restatement's per-corner arrays, memory variables and damping
             vectors, bit for bit: every step of c1_bkt, and the four-class 7 x 5 x 4 box whose nodes see 1, 2, 4 and 8 classes
             (both moduli on, shear only, dilatation only, all zero; eight DISTINCT rows around one node need twins of the
             four: bkt_reference.four_class_problem)
  plan       hq_attenuation_plan_check against the (node, class) pairs counted in numpy
  teeth      the per-node criterion of tests/test_gpu_attenuation.py trips at the nodes concerned, and only there
  exports    every new symbol in both libraries, ABI 6, csrc/hq_atten.h alone under g++, hq_element_force_bkt under g++
             against the restatement's unrolled sums, the two kernels' registers in the gfx950 code object

B_restatement, the double restatement's own worst |step - ref| / (2^-53 T) on the GPU test's inputs (measured here, pinned
below 4 so that B = 16 max(B_restatement, 4) = 64):  uniform9x7x5 0.87   four7x5x4 0.82   two_level 1.04;  every third node
loaded on four7x5x4: 0.82."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import hercules_amd as ha
from hercules_amd import build as hbuild
from hercules_amd import capi, host
from oracle import herc_oracle as ho
from tests import bkt_reference as R
from tests import helpers as H
from tests import test_code_object_cpu as CO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["hq_attenuation_set", "hq_attenuation_info", "hq_attenuation_fetch", "hq_attenuation_load", "hq_attenuation_clear",
         "hq_attenuation_plan_check"]
EPS = 2.0 ** -53
SEED, STATE_SEED = 5150, 977
MESHES = ("uniform9x7x5", "four7x5x4", "two_level")
bits = lambda a: np.ascontiguousarray(a).view(np.int64)

needs_longdouble = pytest.mark.skipif(not np.finfo(np.longdouble).eps < 1e-18, reason="np.longdouble is no wider than double here")


@pytest.fixture(scope="module")
def libs():
    hbuild.build()
    return ha.load_library(), capi.load_library(precision="f32")


def step_inputs(name, loaded=False):
    """(p, plan, u1, u2, conv0, loaded ids, F) of a mesh: independent fields, independent memory variables of the fields' size
    consistent per slot, and (loaded) every third node forced."""
    p = R.problem(name)
    plan = R.slot_plan(p["lnid"], p["coef"])
    u1, u2 = H.step_fields(p["N"], SEED, p["dangling"])
    conv0 = R.random_state(plan, STATE_SEED)
    ids = F = None
    if loaded:
        ids = np.arange(0, p["N"], 3, dtype=np.int32)
        F = np.ascontiguousarray(H.rest_forces(p["ntable"][:, 0], p["dt"], SEED + 1)[ids])
    return p, plan, u1, u2, conv0, ids, F


def extended(p, u1, u2, conv0, ids=None, F=None, **teeth):
    f, tf, conv = R.extended_sums(p["lnid"], p["etable"], p["coef"], p["freq"], p["dt"], u1, u2, conv0, p["N"], **teeth)
    ref, T = H.extended_step(p["lnid"], p["etable"], p["ntable"], u1, u2, p["dangling"], loaded=ids, F=F, dt=p["dt"], sums=(f, tf))
    return ref, T, conv


# ---------------------------------------------------------------------------------------------
# the restatement is the reference: checkpoints of the real program under type_of_damping = bkt
# ---------------------------------------------------------------------------------------------
def golden_problem(name):
    """(g, p) of a BKT fixture: the sibling's mesh (tests/helpers) with undamped tables and the fixture's own coefficients."""
    g = H.load(name)
    if name == "c1_bkt":
        p = H.c1_problem("none")
        p = dict(p, dangling=None, freq=float(g["freq"]))
    else:
        m = ho.octree_mesh_from_elem_ticks(g["elem_ticks"], H.C1_FAR_TICKS)
        E, N = len(m["lnid"]), len(m["node_q"])
        mat = g["mat_vs_vp_rho"]
        edata = np.empty((E, 4), np.float32)
        edata[:, 0] = (1000.0 / 2 ** 30 * m["emin"] * m["elem_size"].astype(np.float64)).astype(np.float32)
        edata[:, 1], edata[:, 2], edata[:, 3] = mat[:, 1], mat[:, 0], mat[:, 2]
        et, nt = ho.solver_init(m["lnid"], edata, m["face"], N, 1e-3, float(g["freq"]), damping=ho.DAMP_NONE)
        ho.compute_adjust(nt, 0, m["dangling"])
        p = dict(lnid=m["lnid"], etable=et, ntable=nt, dangling=m["dangling"], N=N, E=E, dt=1e-3, freq=float(g["freq"]))
    assert g["coef"].shape == (p["E"], 10) and g["coef"].dtype == np.float32
    return g, dict(p, coef=g["coef"])


@functools.lru_cache(maxsize=None)
def golden_run(name):
    """The restatement's run of a fixture from rest with its forces, once per process (tests/test_gpu_attenuation.py shares
    it) -> {step: (tm1, tm2, conv)} at the fixture's checkpoints, read-only; under "slot" the first step at which
    hqh_atten_advance over the slot plan, driven beside the run from the same fields, left memory variables or damping vectors
    that are not the per-corner arrays' bit for bit (None: never)."""
    g, p = golden_problem(name)
    steps = [int(s) for s in g["ckpt_steps"]]
    follower = SlotFollower(p) if name == "c1_bkt" else None       # (the issue's case; the octree run is the pin alone)
    kept = R.bkt_run(p["lnid"], p["etable"], p["ntable"], p["coef"], p["freq"], p["dt"], steps[-1], g["loaded_lnid"], g["forces"],
                     p["dangling"], keep=steps, observer=follower)[3]
    for v in kept.values():
        for a in v:
            a.flags.writeable = False
    if follower is not None:
        kept["slot"], kept["slot_steps"] = follower.first_bad, follower.steps
    return kept


@pytest.mark.parametrize("name", ["c1_bkt", "c5_two_level_bkt"])
def test_checkpoints_bitwise(name):
    """The restatement run from rest with the fixture's forces equals the reference's checkpoints bit for bit, as
    tests/test_oracle_golden.py::test_checkpoints_bitwise holds the C oracle to c1_none and c1_mass."""
    g, p = golden_problem(name)
    steps = [int(s) for s in g["ckpt_steps"]]
    assert os.path.getsize(os.path.join(H.GOLDEN, name + ".npz")) <= os.path.getsize(os.path.join(H.GOLDEN, name.replace("c1_bkt", "c1_short").replace("_bkt", "") + ".npz"))
    if name != "c1_bkt":
        assert len(p["dangling"][0]) > 0 and (g["coef"][:, 8] != 0).any() and len(np.unique(g["coef"], axis=0)) >= 2
    kept = golden_run(name)
    for k, s in enumerate(steps):
        tm1, tm2, _ = kept[s]
        d1, d2 = H.rel_linf(tm1, g["ckpt_tm1"][k]), H.rel_linf(tm2, g["ckpt_tm2"][k])
        print("\n[attenuation] %s step %d: rel L-inf %.3e %.3e, max |u| %.3e" % (name, s, d1, d2, np.abs(g["ckpt_tm1"][k]).max()))
        assert np.array_equal(tm1, g["ckpt_tm1"][k]) and np.array_equal(tm2, g["ckpt_tm2"][k]), (s, d1, d2)
    assert np.abs(g["ckpt_tm1"][-1]).max() > 100.0                          # the wave is really there


def test_slot_form_equals_element_form_on_every_step_of_c1_bkt(libs):
    """(the follower rides in golden_run: one run of the restatement serves the pin, this test and the GPU run)"""
    g, _ = golden_problem("c1_bkt")
    kept = golden_run("c1_bkt")
    assert kept["slot_steps"] == int(g["ckpt_steps"][-1]) == 800 and kept["slot"] is None, kept["slot"]
    assert np.abs(kept[800][2]).max() > 1.0                                 # the memory variables are really there


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
    for n in ("hqh_atten_class_coef", "hqh_atten_advance"):
        assert n in host.EXPORTS and hasattr(h, n), n


def test_null_arguments_are_refused(libs):
    for lib in libs:
        out = (ctypes.c_int64 * 4)()
        d = capi._AttenuationDesc(None, 1.0)
        assert lib.hq_attenuation_set(None, ctypes.byref(d)) == -1
        assert lib.hq_attenuation_info(None, out) == -1
        assert lib.hq_attenuation_fetch(None, None, None, None, None) == -1
        assert lib.hq_attenuation_load(None, None, None, None, None) == -1
        assert lib.hq_attenuation_clear(None) == -1
        assert lib.hq_attenuation_plan_check(None, None, out) == -1
    assert ctypes.sizeof(capi._AttenuationDesc) == 16


def test_header_compiles_alone_under_gxx(tmp_path):
    src = tmp_path / "probe.cc"
    src.write_text('#include "hq_atten.h"\n#include <stdio.h>\nint main() { float r[10] = {0.04f, 0.06f, 0.02f, 0.06f, 0.9f, 0, 0, 0, 0, 0}; '
                   'double k[HQ_ATTEN_NCOEF], f[4] = {0, 0, 0, 0}, ws, wk; double rmax = hq_atten_class_coef(r, 5.0, 1e-3, k); '
                   'hq_atten_advance(1.0, 0.5, k, f, 1, &ws, &wk); printf("%.17g %.17g %.17g %.17g\\n", rmax, f[0], ws, wk); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "hercules_amd", "csrc"), "-o", str(exe), str(src)])
    rmax, f0, ws, wk = [float(x) for x in subprocess.check_output([str(exe)], universal_newlines=True).split()]
    K = R.class_coef(np.array([0.04, 0.06, 0.02, 0.06, 0.9, 0, 0, 0, 0, 0], np.float32), 5.0, 1e-3)
    assert rmax == K["rmax"] and f0 == K["cu1"][0, 0, 0] * 1.0 + K["cu2"][0, 0, 0] * 0.5
    assert wk == 1.0 and ws != 1.0                                          # dilatation off: the damping vector is u1 itself


def test_class_coefficients_are_the_restatements(libs):
    rows = np.concatenate([R.CLASSES, R.four_class_problem()["coef"]])
    for freq, dt in ((20.0, 0.5 * 20.0 / 6000.0), (5.0, 1e-3)):
        k, rmax = host.atten_class_coef(rows, freq, dt)
        K = R.class_coef(rows, freq, dt)
        assert rmax == K["rmax"]
        for m in range(2):
            q = k[:, 9 * m:9 * m + 9]
            on, cs = K["on"][:, m], K["csum_on"][:, m]
            for v in range(2):
                assert np.array_equal(bits(q[on, 3 * v]), bits(K["cu1"][on, m, v])) and np.array_equal(bits(q[on, 3 * v + 1]), bits(K["cu2"][on, m, v]))
                assert np.array_equal(bits(q[on, 3 * v + 2]), bits(K["ex"][on, m, v]))
                assert (q[~on, 3 * v] == 0).all() and (q[~on, 3 * v + 1] == 0).all() and (q[~on, 3 * v + 2] == 1).all()    # the skip
            assert np.array_equal(bits(q[cs, 6]), bits(K["a"][cs, m, 0])) and np.array_equal(bits(q[cs, 8]), bits(K["bq"][cs, m]))
            assert (q[~cs, 6:9] == 0).all()                                 # csum == 0: the damping vector is u1
    # the all-zero class's twin has a0 = -a1 != 0 and csum == 0: the reference's branch, not the formula with a0, a1
    twin = np.nonzero((rows[:, 0] != 0) & (rows[:, 0] + rows[:, 1] + rows[:, 2] == 0))[0]
    assert len(twin) >= 1 and (k[twin, 6:9] == 0).all()


def test_element_force_bkt_is_the_unrolled_sums(tmp_path):
    """hq_element_force_bkt (csrc/hq_kernels.h) under g++ against the restatement's aTransposeU / firstVector_mu /
    firstVector_kappa / au on random damping vectors: the butterfly sums in another order, so the comparison is to a few ulps
    of the sum of magnitudes, far below the 1e-6 a wrong coefficient or a swapped mode would leave."""
    rng = np.random.default_rng(3)
    E = 64
    ws, wk = rng.standard_normal((E, 8, 3)), rng.standard_normal((E, 8, 3))
    et = np.zeros((E, 4))
    et[:, 0], et[:, 1] = rng.uniform(0.5, 2.0, E), rng.uniform(-1.0, 3.0, E)
    want = R.element_forces(et, ws, wk)
    src = tmp_path / "probe.cc"
    src.write_text('#define HQ_KERNEL_MATH_HOST_CHECK 1\n#include "hq_kernels.h"\n#include <stdio.h>\n'
                   'int main(int argc, char** argv) { FILE* f = fopen(argv[1], "rb"); FILE* o = fopen(argv[2], "wb"); double in[50];\n'
                   '  while (fread(in, 8, 50, f) == 50) { double v[6][8];\n'
                   '    for (int n = 0; n < 8; n++) for (int c = 0; c < 3; c++) { v[c][n] = in[3 * n + c]; v[3 + c][n] = in[24 + 3 * n + c]; }\n'
                   '    hq_element_force_bkt(v[0], v[1], v[2], v[3], v[4], v[5], in[48], in[49]);\n'
                   '    double out[24]; for (int n = 0; n < 8; n++) for (int c = 0; c < 3; c++) out[3 * n + c] = v[c][n];\n'
                   '    fwrite(out, 8, 24, o); }\n  fclose(o); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "hercules_amd", "csrc"), "-o", str(exe), str(src)])
    np.concatenate([ws.reshape(E, 24), wk.reshape(E, 24), et[:, :2]], axis=1).tofile(str(tmp_path / "in.bin"))
    subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    got = np.fromfile(str(tmp_path / "out.bin")).reshape(E, 8, 3)
    scale = (np.abs(et[:, :2]).sum(axis=1) * (np.abs(ws).sum(axis=(1, 2)) + np.abs(wk).sum(axis=(1, 2))))[:, None, None]
    assert (np.abs(got - want) <= 64 * EPS * scale).all(), float((np.abs(got - want) / scale).max())
    wrong = R.element_forces(et, ws, wk, kappa_without_c1=True)
    assert (np.abs(wrong - want) > 1e-3 * scale).any()


def test_kernels_in_the_code_object(tmp_path):
    """hq_k_atten_advance and hq_k_element_bkt as hipcc left them for gfx950: no spill, no scratch, no LDS, and at most 128
    registers each -- the rule tests/test_code_object_cpu.py holds the brick kernels to: four waves per SIMD, here two
    256-thread workgroups per SIMD pair, with the element kernel's 48 gathered doubles (96 registers) and the butterfly inside
    it.  The counts themselves are in docs/LABNOTES.md (110 and 78 when this was written)."""
    k = CO._kernel_notes(tmp_path)
    found = {tag: v for name, v in k.items() for tag in ("hq_k_atten_advance", "hq_k_element_bkt") if tag in name}
    assert sorted(found) == ["hq_k_atten_advance", "hq_k_element_bkt"], sorted(k)
    print("\n[attenuation] code object:", found)
    for tag, v in found.items():
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (tag, v)
        assert v["group_segment_fixed_size"] == 0, (tag, v)
        assert v["vgpr_count"] <= 128, (tag, v)


# ---------------------------------------------------------------------------------------------
# the slot plan
# ---------------------------------------------------------------------------------------------
def desc_of(p):
    return H.solver_desc(dict(p, node_xyz=p["node_xyz"]))


def test_plan_check_uniform_box(libs):
    p = R.problem("uniform9x7x5")
    rep = capi.attenuation_plan_check(desc_of(p), p["coef"])
    Epad = (p["E"] + 63) & ~63
    assert rep == dict(classes=1, slots=p["N"], device_bytes=144 * p["N"] + 32 * Epad + 8 * p["N"] + 144, faults=0), rep
    assert rep["device_bytes"] < 768 * p["E"]                               # per slot, not per element corner


def test_plan_check_four_class_box(libs):
    p = R.problem("four7x5x4")
    plan = R.slot_plan(p["lnid"], p["coef"])
    pairs = {(int(n), p["coef"][e].tobytes()) for e in range(p["E"]) for n in p["lnid"][e]}     # counted independently
    seen = R.classes_seen(plan, p["N"])
    assert {1, 2, 4, 8} <= set(np.unique(seen).tolist()), np.unique(seen)
    kinds = {(bool(r[3] != 0 and r[4] != 0), bool(r[8] != 0 and r[9] != 0)) for r in plan["rows"]}
    assert kinds == {(True, True), (True, False), (False, True), (False, False)}
    rep = capi.attenuation_plan_check(desc_of(p), p["coef"])
    Epad = (p["E"] + 63) & ~63
    assert rep["classes"] == len(plan["rows"]) == 8 and rep["slots"] == len(pairs) == len(plan["slot_node"]) and rep["faults"] == 0, rep
    assert rep["device_bytes"] == 152 * rep["slots"] + 32 * Epad + 144 * rep["classes"]


def test_plan_check_two_level_octree(libs):
    p = R.problem("two_level")
    rep = capi.attenuation_plan_check(desc_of(p), p["coef"])
    plan = R.slot_plan(p["lnid"], p["coef"])
    hanging = np.asarray(p["dangling"][0])
    assert len(hanging) > 0 and np.isin(hanging, plan["slot_node"]).all()   # every hanging node has a slot
    assert rep["classes"] == 2 and rep["slots"] == len(plan["slot_node"]) > p["N"] and rep["faults"] == 0, rep
    assert (R.classes_seen(plan, p["N"]) >= 1).all()
    bad = p["coef"].copy()
    bad[3, 2] = np.nan
    with pytest.raises(capi.HqError, match="not finite"):
        capi.attenuation_plan_check(desc_of(p), bad)


# ---------------------------------------------------------------------------------------------
# slot form == element form
# ---------------------------------------------------------------------------------------------
class SlotFollower:
    """hqh_atten_advance over the slot plan beside the restatement's per-corner arrays: an observer of R.bkt_run (or called
    by hand) that advances its slot state from the same fields and compares memory variables and damping vectors bit for bit
    (a damping vector that is 0 compares by ==: the csum == 0 branch hands on u1 itself, and a -0 of u1 comes out +0 of
    the one formula).  first_bad: None or (step, what)."""

    def __init__(self, p, conv0=None):
        self.p, self.plan = p, R.slot_plan(p["lnid"], p["coef"])
        self.K = R.class_coef(p["coef"], p["freq"], p["dt"])
        self.k, _ = host.atten_class_coef(self.plan["rows"], p["freq"], p["dt"])
        self.lnid = np.asarray(p["lnid"], np.int64)
        self.mv = R.corners_to_slots(self.plan, R.new_state(p["E"]) if conv0 is None else conv0)
        self.first_bad, self.steps = None, 0

    def __call__(self, s, u1, u2, conv):
        plan, es = self.plan, self.plan["eslot"]
        self.mv, w = host.atten_advance(plan["slot_node"], plan["slot_class"], self.k, u1, u2, self.mv)
        self.steps += 1
        if self.first_bad is not None:
            return
        if not np.array_equal(bits(R.slots_to_corners(plan, self.mv)), bits(conv)):
            self.first_bad = (s, "memory variables")
            return
        ws, wk = R.damping_vectors(self.lnid, self.K, u1, u2, conv)
        for d in range(3):
            for got, want in ((w[d][es], ws[:, :, d]), (w[3 + d][es], wk[:, :, d])):
                nz = want != 0
                if not (np.array_equal(got, want) and np.array_equal(bits(got[nz]), bits(want[nz]))):
                    self.first_bad = (s, "damping vectors")


def assert_slot_form_follows(p, nsteps, fields):
    """nsteps of calc_conv on fields(step) -> (u1, u2), from random memory variables (one step) or from rest, a SlotFollower
    beside them."""
    plan = R.slot_plan(p["lnid"], p["coef"])
    conv = R.random_state(plan, STATE_SEED) if nsteps == 1 else R.new_state(p["E"])
    follower = SlotFollower(p, conv)
    for s in range(nsteps):
        u1, u2 = fields(s)
        R.calc_conv(follower.lnid, follower.K, u1, u2, conv)
        follower(s, u1, u2, conv)
    assert follower.first_bad is None and follower.steps == nsteps, follower.first_bad


def test_slot_form_equals_element_form_on_the_four_class_box(libs):
    p = R.problem("four7x5x4")
    seq = [H.step_fields(p["N"], SEED + s) for s in range(4)]
    assert_slot_form_follows(p, 1, lambda s: seq[0])
    assert_slot_form_follows(p, 4, lambda s: seq[s])


# ---------------------------------------------------------------------------------------------
# B_restatement and the criterion's teeth
# ---------------------------------------------------------------------------------------------
@needs_longdouble
@pytest.mark.parametrize("name,loaded", [(m, False) for m in MESHES] + [("four7x5x4", True)])
def test_restatement_against_the_extended_reference(name, loaded):
    p, plan, u1, u2, conv0, ids, F = step_inputs(name, loaded)
    conv = conv0.copy()
    got = R.bkt_step(p["lnid"], p["etable"], p["ntable"], p["coef"], p["freq"], p["dt"], u1, u2, conv, p["dangling"], ids, F)
    ref, T, cref = extended(p, u1, u2, conv0, ids, F)
    b = float((np.abs(got - ref) / (EPS * T)).max())
    print("\n[attenuation] B_restatement %-14s %s %.3f" % (name, "loaded" if loaded else "", b))
    assert b < 4.0, b
    assert (np.abs(conv - cref) <= 4 * EPS * np.abs(cref).max()).all()


@needs_longdouble
@pytest.mark.parametrize("tooth", ["a0_shear", "conv_after_force", "kappa_without_c1"])
def test_criterion_trips_at_the_nodes_concerned_and_only_there(tooth):
    p, plan, u1, u2, conv0, _, _ = step_inputs("four7x5x4")
    ref, T, _ = extended(p, u1, u2, conv0)
    B = 64.0
    lnid = np.asarray(p["lnid"], np.int64)
    coef, teeth = p["coef"], {}
    if tooth == "a0_shear":
        target = plan["rows"][0]                                            # class 0: both moduli on
        hit = (p["coef"].view(np.uint32) == target.view(np.uint32)).all(axis=1)
        coef = p["coef"].copy()
        coef[hit, 0] = np.float32(coef[hit, 0].astype(np.float64) * (1 + 1e-6))
        assert (coef[hit, 0] != p["coef"][hit, 0]).all()
        concerned = np.unique(lnid[hit])
    elif tooth == "conv_after_force":
        teeth = dict(conv_after_force=True)
        K = R.class_coef(p["coef"], p["freq"], p["dt"])
        concerned = np.unique(lnid[K["on"].any(axis=1)])
    else:
        teeth = dict(kappa_without_c1=True)
        concerned = np.arange(p["N"])                                       # wk is u1 itself even where dilatation is off
    got = R.bkt_step(p["lnid"], p["etable"], p["ntable"], coef, p["freq"], p["dt"], u1, u2, conv0.copy(), p["dangling"], **teeth)
    tripped = np.nonzero((np.abs(got - ref) > B * EPS * T).any(axis=1))[0]
    assert len(tripped) > 0 and np.isin(tripped, concerned).all(), (tooth, len(tripped), len(concerned))
    if tooth == "a0_shear":                                                # (every node of this box touches an element with a modulus on)
        assert len(concerned) < p["N"]                                     # some nodes are not concerned, and they pass
    assert len(tripped) >= 0.9 * len(concerned), (tooth, len(tripped), len(concerned))
    good = R.bkt_step(p["lnid"], p["etable"], p["ntable"], p["coef"], p["freq"], p["dt"], u1, u2, conv0.copy(), p["dangling"])
    assert (np.abs(good - ref) <= B * EPS * T).all()
