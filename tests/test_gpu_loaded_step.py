"""Loaded step per node: source forces on a MOVING field -- ONE step from two independent fields (tm1 = u1, tm2 = u2) with
hq_set_source, every kernel form against the extended-precision restatement of the oracle's loaded step, per node and
component.  The reference side, the conditions and the mutations that show the check has teeth, without a device:
tests/test_loaded_step_cpu.py.

The two per-node families each leave out what the other covers.  tests/test_gpu_sources.py loads every node and steps from
REST: all stiffness and damping sums are exactly zero, so a kernel that ASSIGNS F dt^2 to its accumulator equals one that
ADDS it bit for bit, and so does a patch whose virtual accumulator of a loaded hanging node loses that node's stiffness
partial.  tests/test_gpu_step_terms.py steps from independent fields and never calls hq_set_source: every kernel runs with
F == nullptr and the host tables behind the source lookup are never built.  The reference does both in every step of a
source's rise time: compute_addforce_s assigns the load (psolve.c:5912-5928), the element loops add to it, compute_adjust
distributes the sum of both from the hanging nodes (:5936-5987), the update divides.  The only runs in which a load met a
non-zero field were held to 1e-9 of the field's maximum; a relative error of 1e-6 in ONE loaded node's stiffness sum passes
that (tests/test_loaded_step_cpu.py, mutation b).

Cases, fields and counters: tests/test_gpu_step_terms.py's CASES / CHECKS / make, by import.  Forces:
H.rest_forces(n_t[:, 0], dt, 4711) -- F dt^2 / m0 is sign * uniform(0.5, 1) * 1e-3, the size of the fields, so the load
moves the result by a third of the field's maximum and neither part hides the other.  F stays double in both builds, as
hq_set_source takes it.  Run: create with tm1 = u1, tm2 = u2; assert the kernel form from the counters; set_source(loaded,
F[loaded][None]); run(1); download; check_finite() == 0; the downloaded old field equals u1 bit for bit.
  phase "all"     every key of ST.CASES, f64 and f32 twins: every node loaded, hanging nodes included -- on c5_gradient_branch
                  and two_level a loaded hanging node's F_h + stiffness_h goes through the virtual accumulators to its anchors.
  phase "sparse"  one f64 case per kernel family (SPARSE): every third node id loaded.  A brick unit or patch without an
                  entry would have to own only ids that miss the stride, which none of these meshes allows for a unit of
                  more than a few nodes, and hq_info has no count of the units that own a loaded node: nothing is
                  asserted about it in this phase.  Hence:
  phase "few"     the same cases with TWO loaded nodes, fewer than the context has brick units and patches together, neither
                  of them hanging (a plain node has one owner; only a hanging node has virtual accumulators in further
                  patches): at least one unit or patch owns no loaded node and runs beside ones that do, inside a launch
                  that was handed F -- asserted from hq_info (brick_units + npatches > the number of loaded nodes).  Not
                  for scatter, which has neither (hq_k_source runs one thread per loaded node).
Reference: tests/helpers.extended_step(..., loaded, F, dt) -- force[loaded] += F dt^2 in np.longdouble, T += |F dt^2|, both
BEFORE the hanging-node distribution.  Criterion: the step-terms module's own, unchanged.
  f64   |got - ref| <= B 2^-53 T per node and component, B = 16 max(B_oracle, 4), B_oracle = that problem's LOADED oracle
        step (tests/helpers.oracle_loaded_step) against the reference, asserted <= 64.
  f32   the additive bound 2^-24 |ref| + B 2^-53 T (hanging nodes: ST.float_rounding) and ST.rounded_step: plain nodes equal
        float32(ref) wherever the band lies inside one float, the undetermined share stays within ST.UNDETERMINED_CAP (a
        condition on the inputs, met by the reference side without a device), every hanging node equals ST.hanging_assignment
        of the library's own stored anchors bit for bit.
B_oracle measured (tests/test_loaded_step_cpu.py prints and pins them; all below 4, so B = 64 everywhere), phase all | sparse | few:
    two_level           1.97 | 1.49 | 1.39  (float oracle, of 2^-24 T: 1.94)       box32x32x16  1.98 | 1.98 | 1.68  (float 2.04)
    box70x20x12         2.41 | 1.68 | 1.64  (float 2.31)                            box32        1.99 | 1.89 | 1.56  (float 2.06)
    het70x20x12         rayleigh 2.92 | 2.97 | 2.97   mass 3.08   none 2.89         (float 2.99 / 2.93 / 2.62)
    c5_gradient_branch  rayleigh 3.28 | 2.79 | 2.95   mass 2.65   none 2.54         (float 2.87 / 2.60 / 2.76)
    the further cases' tables (other seeds): box32x32x16 2.06, 1.98; two_level 1.60, 1.73

Further cases, on box32x32x16 default (bricks) and on two_level with no_bricks:
  same nodes   set_source with a first F, again with the same ids and a second F (only the force table travels: device_bytes
               unchanged), upload(u1, u2, step=0), run(1): the reference of the SECOND F.
  window       upload(u1, u2, step=7), set_source(ids, F3 [3 rows], step0=6), run(1): row 1.
  duplicate    (also scatter on two_level) a valid load; a list with one id named twice is refused with HQ_ERR_ARG and the
               id in the message; device_bytes unchanged; run(1) equals the reference of the VALID load: hq_set_source keeps
               the source it had.  (hq_k_source assigns, the brick and patch kernels add: the variants would disagree.)

Finding: none.  Measured on an MI355X, 117 cases in 11.0 s with the references (tests/test_gpu_step_terms.py, whose fields and
unloaded references these share, then takes 2.8 s instead of its 7.4 s alone; the slowest case 1.1 s, box32 with its
reference).  Worst |got - ref| / (2^-53 T) per kernel family (the bound is 64), phase all; sparse and few where they ran:
    hq_k_brick (default, brick_cz = 5, by component, per-node rows), both boxes           1.90 - 2.11; sparse, few 2.01 - 2.05
    hq_k_patch_stencil subsets 1.52 (sparse, few 1.79), full lattices 2.50, element lattice rows and patch_no_uniform 2.42
    hq_k_brick_het unpacked: het70x20x12 3.47 / 3.15 / 3.28 (rayleigh / mass / none; sparse, few 3.54), ragged c5_gradient_branch 3.80 / 3.06 / 3.09
    hq_k_brick_het<PACKED>:  het70x20x12 3.74 / 3.70 / 3.28, ragged c5_gradient_branch 3.62 / 3.76 / 3.09 (sparse, few 4.18)
    hq_k_patch_step, hq_k_patch_pers (w form and patch_wform = 0): het70x20x12 2.19, two_level 1.38 - 1.55 (sparse 1.38, few 1.24)
    hq_k_patch_seed, patch_no_iso / _ntsame / _dedup / _lattice: het70x20x12 4.32 - 4.48 (mass 4.79, none 4.87), two_level 2.22 (sparse, few 2.98)
    scatter: het70x20x12 2.58 - 2.69, two_level 1.61 (sparse 1.24)
    same nodes 2.07 (bricks) / 2.30 (patches only); window 1.87 / 2.81; duplicate 2.05 / 2.98 / 1.38 (scatter)
    float state, all 47 twins: mismatches 0; got != float32(ref) inside the band 0; undetermined 0 in 23 of them, 1 of 58 149
    (box70x20x12 and het70x20x12 under Rayleigh and mass damping) or 1 of 107 811 (box32) in the others -- the reference side's own
    counts; 0.979 - 0.998 of the additive f32 bound.
The geometry keys of tests/test_gpu_step_terms.py (patch plans off the default geometry, 58 with the float twins) ride in
phase "all"; worst |got - ref| / (2^-53 T): hq_k_patch_stencil on box32 1.52 (psplit100 2.50); hq_k_patch_step big 1.50 / 1.55 /
2.68 / 2.19 (box32 / two_level / c5_gradient_branch / het70x20x12), threads64 and threads192 1.55 / 2.56, pmax8-step 1.46 / 2.56;
hq_k_patch_seed two_level 1.86 - 2.22, c5_gradient_branch 4.40, het70x20x12 4.32; float twins: mismatches 0, off float32(ref) 0,
undetermined 0, or 1 of 107 811 (box32) and 1 of 58 149 (het70x20x12) as at the default geometry; 0.979 - 0.995 of the f32 bound.
175 cases in 14.9 s with them (117 in 11.0 s before; the 58 alone 5.3 s, the slowest 1.1 s)."""
import functools

import numpy as np
import pytest

import hercules_amd as ha
from tests import helpers as H
from tests import test_gpu_step_terms as ST        # (its module-level guard skips this module too where longdouble is narrow)

pytestmark = pytest.mark.gpu

EPS = ST.EPS
SEED_F = 4711
FEW = 2                                                          # loaded nodes of the phase "few": fewer than any case's units + patches
NB = ST.NB

# one f64 case per kernel family for the phases "sparse" and "few"
SPARSE = ("brick-box32x32x16", "brick-cz5-box70x20x12", "het-ragged-packed-c5_gradient_branch-rayleigh", "het-het70x20x12-rayleigh",
          "patch_step-two_level", "patch_pers-two_level", "patch_seed-two_level", "stencil-subsets-box32", "scatter-two_level")
CASES = dict(ST.CASES)
# the further cases' contexts: the brick box as shipped, two_level with no_bricks and nothing else set
WINDOW_CASES = {"bricks": "brick-box32x32x16", "patches-only": "no_bricks-two_level"}
CASES["no_bricks-two_level"] = ST._case("two_level", ("patches_only",), options=dict(NB))


def _chk_patches_only(s, p, name):
    info = s.info()
    assert info["brick_nodes"] == 0 and info["npatches"] > 0 and s.dominant_kernel().startswith("hq_k_patch"), (s.dominant_kernel(), info)


CHECKS = dict(ST.CHECKS, patches_only=lambda: _chk_patches_only)


# ---------------------------------------------------------------------------------------------
# the reference side (shared with tests/test_loaded_step_cpu.py)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def element_sums(mesh, damping, precision):
    """H.extended_element_sums of the step-terms fields of a (mesh, damping, precision): shared by every load on it."""
    p = H.step_mesh(mesh, damping)
    nt, u1, u2 = ST.reference(mesh, damping, precision)[:3]
    sums = H.extended_element_sums(p["lnid"], p["etable"], p["N"], u1, u2)
    for a in sums:
        a.flags.writeable = False
    return sums


@functools.lru_cache(maxsize=None)
def forces(mesh, damping, precision, seed=SEED_F):
    """F [N, 3] double: H.rest_forces on the n_t rows of that precision (float rows widened)."""
    p = H.step_mesh(mesh, damping)
    F = H.rest_forces(ST.reference(mesh, damping, precision)[0][:, 0], p["dt"], seed)
    F.flags.writeable = False
    return F


def loaded_ids(p, phase, k=0):
    """all: every node; sparse: every third node id; few: k nodes that do not hang, spread evenly over the ids."""
    if phase == "all":
        return np.arange(p["N"], dtype=np.int32)
    if phase == "sparse":
        return np.arange(0, p["N"], 3, dtype=np.int32)
    assert phase == "few" and k >= 1
    plain = np.nonzero(~H.node_classes(p["N"], p["dangling"])[0])[0]
    return np.unique(plain[np.linspace(0, len(plain) - 1, k + 2).astype(np.int64)[1:-1]]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def reference(mesh, damping="rayleigh", precision="f64", phase="all", k=0, seed=SEED_F):
    """(loaded, F [N, 3], ref, T, B_oracle) of a loaded step on ST.reference's rows and fields: computed once, read-only.
    B_oracle: the C oracle of that precision, loaded alike, against ref in units of 2^-53 T (float: 2^-24 T)."""
    p = H.step_mesh(mesh, damping)
    nt, u1, u2 = ST.reference(mesh, damping, precision)[:3]
    loaded, F = loaded_ids(p, phase, k), forces(mesh, damping, precision, seed)
    ref, T = H.extended_step(p["lnid"], p["etable"], nt, u1, u2, p["dangling"], loaded=loaded, F=F[loaded], dt=p["dt"],
                             sums=element_sums(mesh, damping, precision))
    o = H.oracle_loaded_step(p, nt, u1, u2, loaded, F[loaded])
    b = float((np.abs(o - ref) / ((2.0 ** -24 if precision == "f32" else EPS) * T)).max())
    for a in (loaded, ref, T):
        a.flags.writeable = False
    return loaded, F, ref, T, b


def bound_factor(mesh, damping, phase="all", k=0, seed=SEED_F):
    """B = 16 * max(B_oracle, 4), B_oracle of the DOUBLE oracle's loaded step on that problem."""
    b = reference(mesh, damping, "f64", phase, k, seed)[4]
    assert b <= 64.0, b                                          # (a broken reference cannot raise the bar)
    return 16.0 * max(b, 4.0)


def float_model(p, nt, u1, u2, loaded, F):
    """ST.float_model extended by the load: the DOUBLE oracle's loaded step on the widened float rows and fields (F dt^2
    stays double and is added to a double accumulator), rounded once; then hq_k_adjust_assign's text on the rounded state."""
    wide = lambda a: np.ascontiguousarray(a, np.float64)
    out = H.oracle_loaded_step(p, wide(nt), wide(u1), wide(u2), loaded, F).astype(np.float32)
    if p["dangling"] is not None and len(p["dangling"][0]):
        ids, want, _ = ST.hanging_assignment(out, p["dangling"])
        out[ids] = want
    return out


# ---------------------------------------------------------------------------------------------
# one loaded step on the device and its verdict
# ---------------------------------------------------------------------------------------------
def verdict(tag, case, c, p, got, old, nonfinite, u1, ref, T, B, family):
    f32 = c["precision"] == "f32"
    bits = np.int32 if f32 else np.int64
    assert nonfinite == 0 and np.isfinite(got).all()
    assert got.dtype == (np.float32 if f32 else np.float64)
    assert np.array_equal(old.view(bits), u1.view(bits)), "the old field is not the uploaded tm1"
    w = ST.worst(got, ref, T, B, f32, p["dangling"])
    print("\n[loaded-step] %-48s %-12s %-8s nodes %6d worst %.3f of the bound (node %d.%d) = %.2f x 2^-53 T%s"
          % (case, tag, c["damping"], p["N"], w[0], w[1], w[2], w[3], " (f32: mostly the state's rounding)" if f32 else ""))
    assert w[0] <= 1.0, (w, got[w[1]], np.asarray(ref[w[1]], np.float64), ST.branch_of(p, w[1]))
    if f32:
        r = ST.rounded_step(got, ref, T, B, p["dangling"])
        print("[loaded-step] %-48s %-12s float32(double step): mismatches %d, undetermined %d of %d, got != float32(ref) inside the band %d; %s"
              % (case, tag, r["mismatches"], r["undetermined"], r["plain"], r["off_centre"], family[0]))
        ST.assert_rounded_step("%s-%s" % (case, tag), r, family, ST.branch_of(p, r["first"][0]) if r["first"] else None)


def context(c, p, nt, u1, u2):
    """The case's context on tm1 = u1, tm2 = u2 with its kernel form asserted -> (solver, family); the caller closes it."""
    s = ST.make(c, p, nt, u1, u2)
    try:
        assert s.info()["variant"] == c["variant"]
        CHECKS[c["check"][0]](*c["check"][1:])(s, p, c["mesh"])
        return s, ST.family_of(s)
    except BaseException:
        s.close()
        raise


PARAMS = [(k, "all") for k in ST.CASES] + [(k, ph) for ph in ("sparse", "few") for k in SPARSE if (ph, ST.CASES[k]["variant"]) != ("few", ST.SCATTER)]


@pytest.mark.parametrize("case,phase", PARAMS, ids=["%s-%s" % kp for kp in PARAMS])
def test_one_loaded_step_from_independent_fields(case, phase):
    c = CASES[case]
    assert phase == "all" or c["precision"] == "f64"
    p = H.step_mesh(c["mesh"], c["damping"])
    nt, u1, u2 = ST.reference(c["mesh"], c["damping"], c["precision"])[:3]
    s, family = context(c, p, nt, u1, u2)
    try:
        k = FEW if phase == "few" else 0
        loaded, F, ref, T, _ = reference(c["mesh"], c["damping"], c["precision"], phase, k)
        if phase == "few":       # fewer plain loaded nodes than units and patches: one of them owns none
            info = s.info()
            assert len(loaded) == FEW < info["brick_units"] + info["npatches"], (len(loaded), info)
            assert not H.node_classes(p["N"], p["dangling"])[0][loaded].any()
        B = bound_factor(c["mesh"], c["damping"], phase, k)
        s.set_source(loaded, F[loaded][None])
        s.run(1)
        got, old = s.download()
        nonfinite = s.check_finite()
    finally:
        s.close()
    verdict(phase, case, c, p, got, old, nonfinite, u1, ref, T, B, family)


@pytest.mark.parametrize("which", list(WINDOW_CASES), ids=list(WINDOW_CASES))
def test_same_nodes_path_meets_a_moving_field(which):
    """The second call names the same ids: only the force table travels (hq_set_source's same-nodes path), and the step
    applies the SECOND table to a field that moves."""
    case = WINDOW_CASES[which]
    c = CASES[case]
    p = H.step_mesh(c["mesh"], c["damping"])
    nt, u1, u2 = ST.reference(c["mesh"], c["damping"])[:3]
    loaded, F2, ref, T, _ = reference(c["mesh"], c["damping"], "f64", "all", 0, SEED_F + 1)
    F1 = forces(c["mesh"], c["damping"], "f64")
    assert np.abs(F1 - F2).min() > 0
    B = bound_factor(c["mesh"], c["damping"], "all", 0, SEED_F + 1)
    s, family = context(c, p, nt, u1, u2)
    try:
        s.set_source(loaded, F1[loaded][None])
        held = s.info()["device_bytes"]
        s.set_source(loaded, F2[loaded][None])
        assert s.info()["device_bytes"] == held
        s.upload(u1, u2, step=0)
        s.run(1)
        got, old = s.download()
        nonfinite = s.check_finite()
    finally:
        s.close()
    verdict("same-nodes", case, c, p, got, old, nonfinite, u1, ref, T, B, family)


@pytest.mark.parametrize("which", list(WINDOW_CASES), ids=list(WINDOW_CASES))
def test_window_that_does_not_start_at_step_zero(which):
    """upload(..., step=7), a table of three rows from step0 = 6: the step applies row 1."""
    case = WINDOW_CASES[which]
    c = CASES[case]
    p = H.step_mesh(c["mesh"], c["damping"])
    nt, u1, u2 = ST.reference(c["mesh"], c["damping"])[:3]
    loaded, F, ref, T, _ = reference(c["mesh"], c["damping"], "f64", "all", 0, SEED_F + 3)
    F3 = np.stack([forces(c["mesh"], c["damping"], "f64", SEED_F + 2)[loaded], F[loaded], forces(c["mesh"], c["damping"], "f64", SEED_F + 4)[loaded]])
    B = bound_factor(c["mesh"], c["damping"], "all", 0, SEED_F + 3)
    s, family = context(c, p, nt, u1, u2)
    try:
        s.upload(u1, u2, step=7)
        s.set_source(loaded, F3, step0=6)
        s.run(1)
        assert s.info()["step"] == 8
        got, old = s.download()
        nonfinite = s.check_finite()
    finally:
        s.close()
    verdict("window", case, c, p, got, old, nonfinite, u1, ref, T, B, family)


DUPLICATE_CASES = ("brick-box32x32x16", "no_bricks-two_level", "scatter-two_level")


@pytest.mark.parametrize("case", DUPLICATE_CASES, ids=list(DUPLICATE_CASES))
def test_a_node_named_twice_is_refused_and_the_source_stays(case):
    """hq_set_source refuses a list that names a node twice (HQ_ERR_ARG = -1, the id in hq_last_error) before anything is
    reset: device_bytes unchanged, and the next step is the loaded step of the VALID list under the loaded criterion."""
    c = CASES[case]
    p = H.step_mesh(c["mesh"], c["damping"])
    nt, u1, u2 = ST.reference(c["mesh"], c["damping"])[:3]
    loaded, F, ref, T, _ = reference(c["mesh"], c["damping"], "f64", "sparse")
    B = bound_factor(c["mesh"], c["damping"], "sparse")
    twice = int(loaded[len(loaded) // 2])
    longer = np.append(loaded, np.int32(twice))                  # one entry more than the accepted list
    swapped = loaded.copy()                                      # as long as the accepted list: not the same-nodes path
    swapped[0] = twice
    s, family = context(c, p, nt, u1, u2)
    try:
        s.set_source(loaded, F[loaded][None])
        held = s.info()["device_bytes"]
        for ids in (longer, swapped):
            with pytest.raises(ha.HqError, match=r"hq error -1: .*\b%d\b.*twice" % twice):
                s.set_source(ids, 2.0 * F[ids][None])
            assert s.info()["device_bytes"] == held
        s.run(1)
        got, old = s.download()
        nonfinite = s.check_finite()
    finally:
        s.close()
    verdict("duplicate", case, c, p, got, old, nonfinite, u1, ref, T, B, family)
