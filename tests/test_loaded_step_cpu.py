"""One LOADED step from two independent fields, the reference side, on a machine without a device (the device side:
tests/test_gpu_loaded_step.py, the loaded cases of tests/test_gpu_partition_step.py and the float cases of
tests/test_gpu_sources.py, whose problems, forces, references and bounds are the ones used here).

1. tests/helpers.extended_step with its defaults returns what it returned before it took a load (np.array_equal on ref and T,
   with and without shared element sums), and a load moves the result by 0.25 - 0.34 of its maximum
   (partitions, where a shared node is loaded by every rank that harbors it: 0.44 - 0.63).
2. B_oracle of every (mesh, damping, precision, phase) of the device modules: the C oracle's loaded step
   (tests/helpers.oracle_loaded_step; partitions: the single-rank oracle on the assembled global tables with the load summed
   over the ranks) against the reference, printed; the double ones are pinned below 4, so B = 64 everywhere.
3. The float model -- the double oracle's loaded step on the widened float rows and fields, rounded once, hanging nodes by
   hq_k_adjust_assign's text -- meets ST.rounded_step with 0 mismatches and the undetermined components under
   ST.UNDETERMINED_CAP on every f32 problem: phases all and sparse of every (mesh, damping) with a float case, the two float
   partition problems, and the from-rest problems of tests/test_gpu_sources.py (box32x32x16, ragged c5_basin, phases plain
   and all).  The float C oracle, which rounds F dt^2 into a float accumulator, does not meet it.
4. Mutations, each applied to the oracle's result or its inputs:
   (a) "assign": at one loaded interior node the stiffness and damping sum is dropped.  The loaded criterion trips at that
       node alone; the same mutant stepped from rest equals the unmutated step bit for bit, and without a load it is the
       unmutated step, which the unloaded criterion passes.
   (b) the same node's sum scaled by 1 - 1e-9: passes rel_linf < 1e-9 (the criterion of test_source_windows_...), trips the
       loaded criterion at that node alone.
   (c) at one loaded hanging node only F_h dt^2 / deps reaches the anchors, its stiffness partial is lost: trips at exactly
       its anchors and at the hanging nodes assigned from them.
   (d) f32, F dt^2 rounded to float before the add: rounded_step rejects 932 of 3 294 components on two_level and 15 252 of
       55 539 on box32x32x16; the additive f32 bound beside it sees 578 and 8 896 of them."""
import numpy as np
import pytest

from oracle import herc_oracle as ho
from tests import helpers as H
from tests import test_gpu_loaded_step as G        # (the step-terms module's guard skips this module too where longdouble is narrow)
from tests import test_gpu_partition_step as GP
from tests import test_gpu_sources as S

ST = G.ST
EPS = G.EPS


def _id(t):
    return "-".join(str(v) for v in t)


def _problems():
    out = set()
    for case, phase in G.PARAMS:
        c = G.CASES[case]
        out.add((c["mesh"], c["damping"], c["precision"], phase, G.FEW if phase == "few" else 0, G.SEED_F))
    for case in G.WINDOW_CASES.values():
        c = G.CASES[case]
        out |= {(c["mesh"], c["damping"], "f64", "all", 0, G.SEED_F + 1), (c["mesh"], c["damping"], "f64", "all", 0, G.SEED_F + 3)}
    for case in G.DUPLICATE_CASES:
        c = G.CASES[case]
        out.add((c["mesh"], c["damping"], "f64", "sparse", 0, G.SEED_F))
    return sorted(out)


PROBLEMS = _problems()
F32_MESHES = sorted({(m, d) for m, d, pr, _, _, _ in PROBLEMS if pr == "f32"})


# ---------------------------------------------------------------------------------------------
# 1. the reference with its defaults is the one it was
# ---------------------------------------------------------------------------------------------
def test_extended_step_with_its_defaults_is_unchanged():
    mesh, damping = "two_level", "rayleigh"
    p = H.step_mesh(mesh, damping)
    nt, u1, u2, ref, T, _ = ST.reference(mesh, damping)
    sums = G.element_sums(mesh, damping, "f64")
    for kw in (dict(), dict(loaded=None, F=None, dt=None), dict(sums=sums), dict(loaded=np.zeros(0, np.int32), F=np.zeros((0, 3)), dt=p["dt"])):
        r2, t2 = H.extended_step(p["lnid"], p["etable"], nt, u1, u2, p["dangling"], **kw)
        assert np.array_equal(r2, ref) and np.array_equal(t2, T), kw
    # a load is added before the distribution: at a plain node that is neither anchor nor hanging it is F dt^2 / m0 on top
    loaded, F, lref, lT, _ = G.reference(mesh, damping)
    hanging, anchor = H.node_classes(p["N"], p["dangling"])
    own = ~hanging & ~anchor
    L = np.longdouble
    add = F.astype(L) * (L(p["dt"]) * L(p["dt"])) / nt[:, :1].astype(L)
    assert np.abs((lref - ref)[own] - add[own]).max() <= 4 * np.finfo(L).eps * np.abs(lref).max()
    assert np.abs((lT - T)[own] - np.abs(add)[own]).max() <= 4 * np.finfo(L).eps * np.abs(lT).max()
    assert (np.abs(lref - ref)[hanging] > 0).all() and (lT[anchor] > T[anchor] + np.abs(add)[anchor]).all()


# ---------------------------------------------------------------------------------------------
# 2. B_oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem", PROBLEMS, ids=[_id(t) for t in PROBLEMS])
def test_loaded_oracle_step_against_the_extended_reference(problem):
    mesh, damping, precision, phase, k, seed = problem
    p = H.step_mesh(mesh, damping)
    loaded, F, ref, T, b = G.reference(*problem)
    unloaded = ST.reference(mesh, damping, precision)[3]
    moved = float(np.abs(ref - unloaded).max() / np.abs(ref).max())
    print("\n[loaded-step] B_oracle %-20s %-8s %s %-6s seed %d: %.2f%s; loaded %d of %d, the load moves the result by %.2f of its maximum"
          % (mesh, damping, precision, phase, seed, b, " (of 2^-24 T)" if precision == "f32" else "", len(loaded), p["N"], moved))
    assert np.isfinite(b) and b <= 64.0
    assert len(np.unique(loaded)) == len(loaded) == {"all": p["N"], "sparse": (p["N"] + 2) // 3, "few": G.FEW}[phase]
    assert 0.25 < moved < 0.6                                    # neither part hides the other
    if precision == "f64":
        assert b < 4.0 and G.bound_factor(mesh, damping, phase, k, seed) == 64.0


LOADED_PARTITIONS = list(GP.LOADED_CASES)


@pytest.mark.parametrize("case", LOADED_PARTITIONS, ids=LOADED_PARTITIONS)
def test_loaded_oracle_step_on_the_partitioned_problems(case):
    """Every rank loads all it harbors with forces of its own; the reference carries the sum over the ranks, T the sum of the
    magnitudes.  A node that several ranks harbor gets several loads: T there exceeds |sum| dt^2 / m0."""
    c = GP.LOADED_CASES[case]
    q = GP.problem_of(c)
    L = GP.loaded_reference(c)
    copies = np.zeros(q["N"], np.int64)
    for r, g in enumerate(q["gid"]):
        copies[g] += 1
        assert L["Fr"][r].shape == (len(g), 3) and np.abs(L["Fr"][r]).min() > 0
    moved = float(np.abs(L["ref"] - q["ref"]).max() / np.abs(L["ref"]).max())
    print("\n[loaded-step] B_oracle partitions %-24s %.2f%s; nodes with 1 / 2 / more loads %d / %d / %d; the load moves the result by %.2f of its maximum"
          % (case, L["B_oracle"], " (of 2^-24 T)" if c["precision"] == "f32" else "", (copies == 1).sum(), (copies == 2).sum(),
             (copies > 2).sum(), moved))
    assert copies.min() >= 1 and (copies > 1).sum() > 0
    assert np.isfinite(L["B_oracle"]) and L["B_oracle"] <= 64.0 and moved > 0.25
    if c["precision"] == "f64":
        assert L["B_oracle"] < 4.0 and GP.loaded_bound_factor(c) == 64.0
    shared = copies > 1                                          # sum of magnitudes, not magnitude of the sum
    dt2m = q["dt"] ** 2 / np.abs(np.asarray(q["ntable"][:, :1], np.float64))
    hanging, anchor = H.node_classes(q["N"], q["dangling"])
    sel = shared & ~hanging & ~anchor
    if sel.any():
        gain = np.asarray(L["T"] - q["T"], np.float64)[sel]
        assert (gain >= np.abs(L["total"])[sel] * dt2m[sel] * (1 - 1e-12)).all() and (gain > np.abs(L["total"])[sel] * dt2m[sel] * 1.01).any()


# ---------------------------------------------------------------------------------------------
# 3. the float model under the load
# ---------------------------------------------------------------------------------------------
def _meets(tag, got, ref, T, B, dangling):
    r = ST.rounded_step(got, ref, T, B, dangling)
    print("\n[loaded-step] float32(double oracle) %-44s mismatches %d, undetermined %d of %d (cap %d), got != float32(ref) %d"
          % (tag, r["mismatches"], r["undetermined"], r["plain"], int(ST.UNDETERMINED_CAP * r["plain"]), r["off_centre"]))
    assert r["hanging_exact"]
    ST.assert_rounded_step(tag, r, "float32(double oracle)")
    assert ST.additive_bound_trips(got, ref, T, B, dangling) == 0   # the criterion implies the additive bound
    return r


@pytest.mark.parametrize("phase", ["all", "sparse"])
@pytest.mark.parametrize("mesh,damping", F32_MESHES, ids=["%s-%s" % m for m in F32_MESHES])
def test_rounded_double_loaded_step_meets_the_float_criterion(mesh, damping, phase):
    p = H.step_mesh(mesh, damping)
    nt, u1, u2 = ST.reference(mesh, damping, "f32")[:3]
    loaded, F, ref, T, _ = G.reference(mesh, damping, "f32", phase)
    B = G.bound_factor(mesh, damping, phase)
    assert B == 64.0
    _meets("%s-%s-%s" % (mesh, damping, phase), G.float_model(p, nt, u1, u2, loaded, F[loaded]), ref, T, B, p["dangling"])


F32_PARTITIONS = [k for k in LOADED_PARTITIONS if GP.LOADED_CASES[k]["precision"] == "f32"]


@pytest.mark.parametrize("case", F32_PARTITIONS, ids=F32_PARTITIONS)
def test_rounded_double_loaded_step_meets_the_float_criterion_on_partitions(case):
    c = GP.LOADED_CASES[case]
    q = GP.problem_of(c)
    L = GP.loaded_reference(c)
    wide = lambda a: np.ascontiguousarray(a, np.float64)
    o1, o2 = wide(q["u2"]), wide(q["u1"])
    ho.solver_run(np.ascontiguousarray(q["lnid"], np.int32), wide(q["etable"]), wide(q["ntable"]), o1, o2, 0, 1, q["dt"],
                  damping=q.get("kind", ho.DAMP_RAYLEIGH), loaded_lnid=np.arange(q["N"], dtype=np.int32), forces=L["total"][None],
                  dangling=q["dangling"])
    got = o2.astype(np.float32)
    if q["dangling"] is not None:
        ids, want, _ = ST.hanging_assignment(got, q["dangling"])
        got[ids] = want
    _meets(case, got, L["ref"], L["T"], GP.loaded_bound_factor(c), q["dangling"])


FROM_REST = [(k, ph) for k, ph in S.PARAMS if S.CASES[k]["precision"] == "f32"]


@pytest.mark.parametrize("case,phase", FROM_REST, ids=["%s-%s" % kp for kp in FROM_REST])
def test_rounded_double_step_from_rest_meets_the_float_criterion(case, phase):
    """The float cases of tests/test_gpu_sources.py (box32x32x16, ragged c5_basin; phases plain and all): the double oracle's
    step from rest on the widened float rows, rounded once, under S.rounded_reference."""
    name = S.CASES[case]["mesh"]
    p = S._mesh(name)
    assert sorted({S.CASES[k]["mesh"] for k, _ in FROM_REST}) == ["box32x32x16", "c5_basin"]
    loaded, F, _ = S._reference(name, phase, "f32")
    ref, T, B = S.rounded_reference(name, phase)
    nt = np.ascontiguousarray(p["ntable"], np.float32).astype(np.float64)
    got = H.oracle_step_from_rest(p["lnid"], p["etable"], nt, p["dt"], loaded, F[loaded], p["dangling"]).astype(np.float32)
    if p["dangling"] is not None:
        ids, want, _ = ST.hanging_assignment(got, p["dangling"])
        got[ids] = want
    assert 64.0 <= B < 80.0 and (T > 0).all()                    # (c5_basin, all: B_oracle 4.05 where loaded hanging nodes meet at an anchor)
    _meets("from rest %s-%s (B = %.1f)" % (case, phase, B), got, ref, T, B, p["dangling"])


@pytest.mark.parametrize("mesh", ["two_level", "box32x32x16"])
def test_float_oracle_does_not_meet_the_loaded_float_criterion(mesh):
    p = H.step_mesh(mesh)
    nt, u1, u2 = ST.reference(mesh, "rayleigh", "f32")[:3]
    loaded, F, ref, T, _ = G.reference(mesh, "rayleigh", "f32")
    got = H.oracle_loaded_step(p, nt, u1, u2, loaded, F[loaded])
    r = ST.rounded_step(got, ref, T, G.bound_factor(mesh, "rayleigh"), p["dangling"])
    print("\n[loaded-step] the float oracle on %s: %d of %d components are not float32(double step)" % (mesh, r["mismatches"], r["plain"]))
    assert got.dtype == np.float32 and r["mismatches"] > r["plain"] // 10


# ---------------------------------------------------------------------------------------------
# 4. mutations
# ---------------------------------------------------------------------------------------------
MUT = ("c5_gradient_branch", "rayleigh")


def _tripped(got, ref, T, B):
    return set(np.nonzero((np.abs(got - ref) > B * EPS * T).any(axis=1))[0].tolist())


def _interior_node(p):
    """A node with eight elements and no dashpot that neither hangs nor anchors, in the middle of the id range."""
    nt = p["ntable"]
    hanging, anchor = H.node_classes(p["N"], p["dangling"])
    ok = (nt[:, 1] == nt[:, 2]) & (nt[:, 1] == nt[:, 3]) & (np.bincount(p["lnid"].ravel(), minlength=p["N"]) == 8) & ~hanging & ~anchor
    cand = np.nonzero(ok)[0]
    return int(cand[len(cand) // 2])


def _mutant(p, nt, u1, u2, loaded, F, scale_at, scale):
    """The oracle's loaded step with the stiffness and damping sum at the node `scale_at` multiplied by `scale` -- where that
    node is LOADED: the mutation sits on the path a kernel takes for a node it has a source entry for.  The values at the
    nodes that depend on it come from the reference's own expression on the mutated sums, rounded to double; every other
    node keeps the oracle's value.  -> (got, the nodes whose reference value changed)"""
    got = H.oracle_loaded_step(p, nt, u1, u2, loaded, F) if len(loaded) else ST.oracle_step(p, nt, u1, u2)
    if scale_at not in set(np.asarray(loaded).tolist()):
        return got, set()
    sums = G.element_sums(MUT[0], MUT[1], "f64")
    force = sums[0].copy()
    force[scale_at] *= np.longdouble(scale)
    kw = dict(loaded=loaded, F=F, dt=p["dt"])
    ref = H.extended_step(p["lnid"], p["etable"], nt, u1, u2, p["dangling"], sums=sums, **kw)[0]
    mut = H.extended_step(p["lnid"], p["etable"], nt, u1, u2, p["dangling"], sums=(force, sums[1]), **kw)[0]
    changed = np.nonzero((mut != ref).any(axis=1))[0]
    got[changed] = mut[changed].astype(np.float64)
    return got, set(changed.tolist())


def test_mutations_trip_the_loaded_criterion_where_the_others_pass():
    mesh, damping = MUT
    p = H.step_mesh(mesh, damping)
    nt, u1, u2, uref, uT, _ = ST.reference(mesh, damping)
    loaded, F, ref, T, _ = G.reference(mesh, damping)
    B = G.bound_factor(mesh, damping)
    oracle = H.oracle_loaded_step(p, nt, u1, u2, loaded, F[loaded])
    assert B == 64.0 and not _tripped(oracle, ref, T, B)
    n = _interior_node(p)
    # (a) "assign": the sum dropped at one loaded interior node
    got, changed = _mutant(p, nt, u1, u2, loaded, F[loaded], n, 0.0)
    hit = _tripped(got, ref, T, B)
    over = float((np.abs(got[n] - ref[n]) / (B * EPS * T[n])).max())
    print("\n[loaded-step] (a) assign at node %d: tripped %s, %.1e x the bound" % (n, sorted(hit), over))
    assert changed == {n} and hit == {n} and over > 1e9
    #     from rest the mutant IS the unmutated step: all sums are zero, F dt^2 / m0 either way, bit for bit
    rest = H.oracle_step_from_rest(p["lnid"], p["etable"], nt, p["dt"], loaded, F[loaded], p["dangling"])
    assert np.array_equal(rest[n], F[n] * (p["dt"] * p["dt"]) / nt[n, 0])
    zero = np.zeros_like(u1)
    zsum = H.extended_element_sums(p["lnid"], p["etable"], p["N"], zero, zero)
    assert not zsum[0].any() and not zsum[1].any()               # (0 x 0 = 0: scaling the sum at n changes nothing there)
    #     without a load the mutant's path is not taken: the unloaded step-terms criterion sees the oracle's own step
    none = np.zeros(0, np.int32)
    got0, changed0 = _mutant(p, nt, u1, u2, none, np.zeros((0, 3)), n, 0.0)
    assert not changed0 and not _tripped(got0, uref, uT, ST.bound_factor(mesh, damping))
    # (b) the same node's sum x (1 - 1e-9)
    got, changed = _mutant(p, nt, u1, u2, loaded, F[loaded], n, 1.0 - 1e-9)
    hit = _tripped(got, ref, T, B)
    rel = H.rel_linf(got, oracle)
    print("[loaded-step] (b) sum x (1 - 1e-9) at node %d: rel_linf %.2e against the oracle (the bar of the windows test: 1e-9), tripped %s, %.1f x the bound"
          % (n, rel, sorted(hit), float((np.abs(got[n] - ref[n]) / (B * EPS * T[n])).max())))
    assert changed == {n} and rel < 1e-9 and hit == {n}
    # (c) a loaded hanging node whose stiffness partial is lost on the way to its anchors
    ids, ptr, anc = [np.asarray(a, np.int64) for a in p["dangling"]]
    j = len(ids) // 2
    h, mine = int(ids[j]), set(anc[ptr[j]:ptr[j + 1]].tolist())
    users = {int(ids[i]) for i in range(len(ids)) if mine & set(anc[ptr[i]:ptr[i + 1]].tolist())}
    got, changed = _mutant(p, nt, u1, u2, loaded, F[loaded], h, 0.0)
    hit = _tripped(got, ref, T, B)
    print("[loaded-step] (c) hanging node %d keeps F_h only: anchors %s, hanging nodes assigned from them %s; tripped %s"
          % (h, sorted(mine), sorted(users), sorted(hit)))
    assert h in users and changed == mine | users and hit == mine | users


# components the additive f32 bound sees | components rounded_step rejects, with F dt^2 rounded to float before the add
ROUNDED_LOAD = {"two_level": (578, 932), "box32x32x16": (8896, 15252)}


@pytest.mark.parametrize("mesh", list(ROUNDED_LOAD))
def test_a_load_rounded_to_float_before_the_add_is_seen(mesh):
    """(d) What a float kernel would do if it formed F dt^2 in hq_real: the double oracle handed float32(F dt^2) (dt = 1 in
    its source term: the tables carry the time step already), rounded once."""
    p = H.step_mesh(mesh)
    nt, u1, u2 = ST.reference(mesh, "rayleigh", "f32")[:3]
    loaded, F, ref, T, _ = G.reference(mesh, "rayleigh", "f32")
    B = G.bound_factor(mesh, "rayleigh")
    wide = lambda a: np.ascontiguousarray(a, np.float64)
    load = (F[loaded] * (p["dt"] * p["dt"])).astype(np.float32).astype(np.float64)
    o1, o2 = wide(u2), wide(u1)
    ho.solver_run(p["lnid"], p["etable"], wide(nt), o1, o2, 0, 1, 1.0, damping=p["kind"], loaded_lnid=loaded, forces=load[None],
                  dangling=p["dangling"])
    got = o2.astype(np.float32)
    if p["dangling"] is not None:
        ids, want, _ = ST.hanging_assignment(got, p["dangling"])
        got[ids] = want
    # the same construction with the load left in double is the float model itself
    o1, o2 = wide(u2), wide(u1)
    ho.solver_run(p["lnid"], p["etable"], wide(nt), o1, o2, 0, 1, 1.0, damping=p["kind"], loaded_lnid=loaded,
                  forces=(F[loaded] * (p["dt"] * p["dt"]))[None], dangling=p["dangling"])
    plainmodel = G.float_model(p, nt, u1, u2, loaded, F[loaded])
    hanging = H.node_classes(p["N"], p["dangling"])[0]
    assert np.array_equal(o2.astype(np.float32)[~hanging], plainmodel[~hanging])
    r = ST.rounded_step(got, ref, T, B, p["dangling"])
    old = ST.additive_bound_trips(got, ref, T, B, p["dangling"])
    print("\n[loaded-step] (d) %-12s F dt^2 rounded to float before the add: the additive f32 bound trips %d, float32(ref) mismatches %d of %d"
          % (mesh, old, r["mismatches"], r["plain"]))
    assert r["mismatches"] > r["plain"] // 10
    if ROUNDED_LOAD[mesh] is not None:
        assert (old, r["mismatches"]) == ROUNDED_LOAD[mesh]
