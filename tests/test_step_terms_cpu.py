"""One step from two independent fields, the reference side, on a machine without a device (the device side:
tests/test_gpu_step_terms.py, whose cases, fields, reference and bound are the ones used here).

1. The C oracle's single step against tests/helpers.extended_step (np.longdouble) on every mesh and damping kind of the
   device cases, in double and with the float oracle on float n_t rows and fields: the worst |oracle - ref| / (2^-53 T)
   (float: 2^-24 T) per mesh is B_oracle, the yardstick of the device bound B = 16 * max(B_oracle, 4).  It is printed
   and must not exceed 64 (a broken reference cannot inflate the bar); no value is fixed in advance.
2. The check has teeth: one element's c3, c4 scaled by 1 + 2^-23 (a float ulp in zeta), one capped element given its
   uncapped lambda, one n_t row's m1 scaled by 1 + 1e-9 -- each exceeds the device bound at every node of the mutated
   element (at the node of the row), and nowhere else.
3. The planner's counters the device cases rely on, from the host-only plan checks -- the f32 cases on n_t rows rounded
   to float, as the float library's planner gets them: NTSAME and the stencil tables come out the same, packing does not
   (per-element units pack only without damping: G.float_rows_pack).
4. The float library's criterion, one step = float32(double step) (G.rounded_step).  The model -- the double oracle on
   the widened float rows and fields, rounded once, hanging nodes by hq_k_adjust_assign's text -- meets it completely on
   every (mesh, damping) pair with an f32 device case: 0 mismatches, exact hanging sums, undetermined components 0 of
   107 811 (box32), 55 539 (box32x32x16), 58 149 (box70x20x12, het70x20x12 x 3 dampings), 17 550 (c5_gradient_branch x 3)
   and 3 294 (two_level); the cap is 1 in 10 000.  It has teeth where the additive f32 bound has none.  Components over
   the additive bound | components the criterion rejects, whole-table mutations of the model (seed 5150, B = 64):
       het70x20x12   every c1 x (1 + 1e-9)      0 |     8 of 58 149
       het70x20x12   every c1 x (1 + 1e-8)      4 |   100
       het70x20x12   every m2 x (1 + 1e-9)     67 |  1186      (m2: all three columns of the row)
       box32x32x16   every c1 x (1 + 1e-9)    148 |   599 of 55 539
       box32x32x16   every c1 x (1 + 1e-8)   1401 |  3933
       box32x32x16   every m2 x (1 + 1e-9)    632 |  2284
   The float C oracle rounds every local force and does NOT meet the criterion (28 355 of 58 149 components of
   het70x20x12): it is not the reference of this check."""
import numpy as np
import pytest

from oracle import herc_oracle as ho
from tests import helpers as H
from tests import test_gpu_step_terms as G         # (its module-level guard skips this module too where longdouble is narrow)

MESHES = sorted({(c["mesh"], c["damping"]) for c in G.CASES.values()})
MESHES_F32 = sorted({(c["mesh"], c["damping"]) for c in G.CASES.values() if c["precision"] == "f32"})


_oracle_step = G.oracle_step


@pytest.mark.parametrize("mesh,damping", MESHES, ids=["%s-%s" % m for m in MESHES])
def test_oracle_step_against_the_extended_reference(mesh, damping):
    p = H.step_mesh(mesh, damping)
    nt, u1, u2, ref, T, b = G.reference(mesh, damping)
    hanging, _ = H.node_classes(p["N"], p["dangling"])
    assert min(np.abs(u1[~hanging]).min(), np.abs(u2[~hanging]).min()) >= 0.5e-3 * (1 - 1e-6)        # nothing near zero
    assert np.abs(u1 - u2).max() > 1.5e-3 and np.median(np.abs(u1 - u2)) > 0.2e-3                    # u2 is not u1
    q = np.abs(_oracle_step(p, nt, u1, u2) - ref) / (G.EPS * T)
    assert b == float(q.max())
    share = 1.0 - (np.abs(nt[:, 1:4] * u1) + np.abs(nt[:, 4:7] * u2)) / np.abs(nt[:, :1]) / T
    print("\n[step-terms] B_oracle %-20s %-8s %.2f (node %d); dt %.3e, median share of the element forces in T %.3f"
          % (mesh, damping, b, int(np.argmax(q.max(axis=1))), p["dt"], float(np.median(share))))
    assert np.isfinite(b) and b <= 64.0
    assert float(np.median(share)) > 0.01                        # the force term is not lost beside 2 u1 - u2
    if "labels" in p:                                            # every branch in >= 10 % of the elements
        assert all(p["labels"][k].sum() * 10 >= p["E"] for k in H.BRANCHES)
        assert (damping == "rayleigh") == bool(p["etable"][:, 2].any()) and (damping == "rayleigh") == (p["material"][0] != 0)


@pytest.mark.parametrize("mesh,damping", MESHES_F32, ids=["%s-%s" % m for m in MESHES_F32])
def test_float_oracle_step_against_the_extended_reference(mesh, damping):
    p = H.step_mesh(mesh, damping)
    nt, u1, u2, ref, T, b = G.reference(mesh, damping, "f32")
    assert nt.dtype == u1.dtype == _oracle_step(p, nt, u1, u2).dtype == np.float32
    print("\n[step-terms] B_oracle (float, of 2^-24 T) %-20s %-8s %.2f" % (mesh, damping, b))
    assert np.isfinite(b) and b <= 64.0


# ---------------------------------------------------------------------------------------------
# 4. the float library's criterion: one step is float32(double step)
# ---------------------------------------------------------------------------------------------
float_model, old_bound_trips = G.float_model, G.additive_bound_trips


@pytest.mark.parametrize("mesh,damping", MESHES_F32, ids=["%s-%s" % m for m in MESHES_F32])
def test_rounded_double_step_meets_the_float_criterion(mesh, damping):
    """The criterion is satisfiable with B = 64 on every (mesh, damping) that has an f32 device case: the model has no
    mismatch, no inexact hanging sum and stays under the cap of undetermined components."""
    p = H.step_mesh(mesh, damping)
    nt, u1, u2, ref, T, _ = G.reference(mesh, damping, "f32")
    B = G.bound_factor(mesh, damping)
    got = float_model(p, nt, u1, u2)
    r = G.rounded_step(got, ref, T, B, p["dangling"])
    print("\n[step-terms] float32(double oracle) %-20s %-8s mismatches %d, undetermined %d of %d (cap %d), got != float32(ref) %d"
          % (mesh, damping, r["mismatches"], r["undetermined"], r["plain"], int(G.UNDETERMINED_CAP * r["plain"]), r["off_centre"]))
    assert B == 64.0
    assert r["hanging_exact"]                                    # the double sum of 2 or 4 stored floats: its order cannot matter
    G.assert_rounded_step("%s-%s" % (mesh, damping), r, "float32(double oracle)")
    assert old_bound_trips(got, ref, T, B, p["dangling"]) == 0   # the criterion implies the additive bound


# (mesh, what is scaled, by 1 + this) -> (components over the old f32 bound, components the new criterion rejects), counted
# here and pinned; the first row's 0 is the point: a float kernel form with every c1 off by 1e-9 passed the old bound
TEETH = {("het70x20x12", "c1", 1e-9): (0, 8), ("het70x20x12", "c1", 1e-8): (4, 100), ("het70x20x12", "m2", 1e-9): (67, 1186),
         ("box32x32x16", "c1", 1e-9): (148, 599), ("box32x32x16", "c1", 1e-8): (1401, 3933), ("box32x32x16", "m2", 1e-9): (632, 2284)}


@pytest.mark.parametrize("mesh,what,eps", list(TEETH), ids=["%s-%s-%g" % k for k in TEETH])
def test_float_criterion_has_teeth(mesh, what, eps):
    p = H.step_mesh(mesh, "rayleigh")
    nt, u1, u2, ref, T, _ = G.reference(mesh, "rayleigh", "f32")
    B = G.bound_factor(mesh, "rayleigh")
    et, nt2 = p["etable"].copy(), np.ascontiguousarray(nt, np.float64)
    if what == "c1":
        et[:, 0] *= 1.0 + eps
    else:
        nt2[:, 1:4] *= 1.0 + eps
    got = float_model(p, nt2, u1, u2, et)
    r = G.rounded_step(got, ref, T, B, p["dangling"])
    old, new = old_bound_trips(got, ref, T, B, p["dangling"]), r["mismatches"]
    with pytest.raises(AssertionError, match=r"plain node %d component %d got .* float ulps apart.*kernel family mutated model" % r["first"][:2]):
        G.assert_rounded_step("teeth", r, "mutated model", G.branch_of(p, r["first"][0]))   # the message a device case would give
    print("\n[step-terms] teeth %-12s every %s x (1 + %g): the old f32 bound trips %d, float32(ref) mismatches %d of %d"
          % (mesh, what, eps, old, new, ref.size))
    assert new > 0
    if (mesh, what, eps) == ("het70x20x12", "c1", 1e-9):
        assert old == 0                                          # every c1 of the per-element mesh off by 1e-9 passed the old bound
    assert (old, new) == TEETH[(mesh, what, eps)]


def test_one_float_ulp_is_a_mismatch_at_plain_and_at_hanging_nodes():
    """One component one float ulp off: at a hanging node exactly that component is rejected (its anchors are untouched);
    at an anchor the anchor's component, and that of a hanging node which averages it where the rounded mean moves."""
    mesh, damping = "c5_gradient_branch", "rayleigh"
    p = H.step_mesh(mesh, damping)
    nt, u1, u2, ref, T, _ = G.reference(mesh, damping, "f32")
    B = G.bound_factor(mesh, damping)
    ids, ptr, anc = [np.asarray(a, np.int64) for a in p["dangling"]]
    good = float_model(p, nt, u1, u2)
    bad = good.copy()
    bad[ids[0], 1] = np.nextafter(bad[ids[0], 1], np.float32(np.inf))
    r = G.rounded_step(bad, ref, T, B, p["dangling"])
    assert r["mismatches"] == 1 and r["first"][:3] == (int(ids[0]), 1, "hanging") and r["first"][5] == 1, r
    a = int(anc[ptr[0]])
    bad = good.copy()
    bad[a, 2] = np.nextafter(bad[a, 2], np.float32(-np.inf))
    users = int(sum(a in anc[ptr[k]:ptr[k + 1]] for k in range(len(ids))))
    r = G.rounded_step(bad, ref, T, B, p["dangling"])
    # (a hanging node that averages it moves by a half or a quarter of that ulp: its own rounding may or may not follow, and
    #  either way it must equal the assignment from the stored anchors, so it is rejected only if it did not follow)
    assert users >= 1 and 1 <= r["mismatches"] <= 1 + users, (users, r)


def test_float_oracle_does_not_meet_the_float_criterion():
    """The float C oracle rounds every local force: it is NOT float32(double step) and cannot serve as the reference of
    the float library's one-step criterion."""
    mesh, damping = "het70x20x12", "rayleigh"
    p = H.step_mesh(mesh, damping)
    nt, u1, u2, ref, T, _ = G.reference(mesh, damping, "f32")
    got = _oracle_step(p, nt, u1, u2)
    r = G.rounded_step(got, ref, T, G.bound_factor(mesh, damping), p["dangling"])
    print("\n[step-terms] the float oracle on %s: %d of %d components are not float32(double step)" % (mesh, r["mismatches"], r["plain"]))
    assert got.dtype == np.float32 and r["mismatches"] > r["plain"] // 10


# ---------------------------------------------------------------------------------------------
# 2. mutations
# ---------------------------------------------------------------------------------------------
def _interior(p, mask):
    """The elements of `mask` none of whose nodes carries a dashpot or lies on a face, stiffest damping first."""
    nt = p["ntable"]
    plain_node = (nt[:, 1] == nt[:, 2]) & (nt[:, 1] == nt[:, 3]) & (np.bincount(p["lnid"].ravel(), minlength=p["N"]) == 8)
    ok = np.nonzero(mask & plain_node[p["lnid"]].all(axis=1))[0]
    return ok[np.argsort(-p["etable"][ok, 2], kind="stable")]


def _tripped(p, got, ref, T, B):
    """The nodes at which some component exceeds the device bound."""
    return set(np.nonzero((np.abs(got - ref) > B * G.EPS * T).any(axis=1))[0].tolist())


def test_mutations_trip_the_bound_at_the_mutated_elements_nodes_only():
    mesh, damping = "het70x20x12", "rayleigh"
    p = H.step_mesh(mesh, damping)
    nt, u1, u2, ref, T, _ = G.reference(mesh, damping)
    B = G.bound_factor(mesh, damping)
    assert B == 64.0 and not _tripped(p, _oracle_step(p, nt, u1, u2), ref, T, B)
    lab = p["labels"]
    # a float ulp in zeta: c3 and c4 of one element (zeta = 10 / Vs below the threshold: the quotient is what rounds)
    e = int(_interior(p, ~lab["zeta_capped"])[0])
    et = p["etable"].copy()
    et[e, 2:4] *= 1.0 + 2.0 ** -23
    hit = _tripped(p, _oracle_step(p, nt, u1, u2, et), ref, T, B)
    print("\n[step-terms] zeta ulp in element %d (beta %.3f): tripped nodes %s" % (e, p["etable"][e, 2] / p["etable"][e, 0], sorted(hit)))
    assert hit == set(p["lnid"][e].tolist())
    # a capped element with its uncapped lambda = rho Vp^2 - 2 mu (psolve.c:3242-3250, float products)
    e = int(_interior(p, lab["capped"])[0])
    h, vp, vs, rho = [np.float32(v) for v in p["edata"][e]]
    lam = float(rho * vp * vp) - 2.0 * float(rho * vs * vs)
    capped = float(rho * vs * vs) * 3.0 * 3.0 - 2.0 * float(rho * vs * vs)
    et = p["etable"].copy()
    assert abs(et[e, 1] - p["dt"] ** 2 * float(h) * capped / 9) <= 1e-15 * et[e, 1] and lam > 1.01 * capped
    et[e, 1] *= lam / capped
    et[e, 3] *= lam / capped
    hit = _tripped(p, _oracle_step(p, nt, u1, u2, et), ref, T, B)
    print("[step-terms] uncapped lambda in element %d (x %.2f): tripped nodes %s" % (e, lam / capped, sorted(hit)))
    assert hit == set(p["lnid"][e].tolist())
    # 1e-9 in one row's m1
    n = int(p["lnid"][e][3])
    nt2 = np.array(nt)
    nt2[n, 4:7] *= 1.0 + 1e-9
    hit = _tripped(p, _oracle_step(p, nt2, u1, u2), ref, T, B)
    print("[step-terms] m1 (1 + 1e-9) at node %d: tripped nodes %s" % (n, sorted(hit)))
    assert hit == {n}


# ---------------------------------------------------------------------------------------------
# 3. the planner's counters behind the device cases
# ---------------------------------------------------------------------------------------------
def _plans(monkeypatch, c):
    """(brick report, patch report, stencil report) of a device case, its options through the environment."""
    from hercules_amd import capi
    for k, v in (c["options"] or {}).items():
        monkeypatch.setenv("HQ_" + k.upper(), str(v))
    d = H.solver_desc(H.step_mesh(c["mesh"], c["damping"]), pack=c["pack"], precision=c["precision"])
    out = capi.brick_plan_check(d), capi.plan_check(d), capi.stencil_plan_check(d)
    assert all(r["faults"] == 0 for r in out), (c, out)
    return out


# (the f32 cases with their n_t rows rounded to float, as the float library's planner gets them: NTSAME and packing read them)
# (the geometry cases' plans: tests/test_patch_geometry_cpu.py)
_PLANNED = [k for k, c in G.CASES.items() if c["variant"] == G.PATCH and c["check"][0] != "geometry"]


@pytest.mark.parametrize("case", _PLANNED, ids=_PLANNED)
def test_planner_counters_of_the_device_cases(case, monkeypatch):
    c = G.CASES[case]
    p = H.step_mesh(c["mesh"], c["damping"])
    o = c["options"] or {}
    b, pp, st = _plans(monkeypatch, c)
    packed = b["packed_units"]
    packs = c["precision"] == "f64" or G.float_rows_pack(c["damping"])      # float rows: only undamped ones come out of two doubles
    if c["check"][0] in ("het", "gradient"):                               # what the device case's own check expects
        assert bool(c["check"][1]) == (packed > 0)
    if o.get("no_bricks"):
        assert b["brick_nodes"] == 0 and pp["patches"] > 0
        if c["mesh"] == "box32":
            assert pp["patches"] == 64 and st["tables"] == 64 and st["full_lattices"] == 8
            assert pp["lattice_patches"] == 8
        else:
            assert pp["patches"] >= 3                                # element-form patches: irregular shells, or per-element material
        if o.get("patch_no_dedup"):
            assert pp["distinct_row_blocks"] == 0
        return
    assert 2 * b["brick_nodes"] > p["N"] and b["units"] > 0          # hq_dominant_kernel: hq_k_brick
    if c["mesh"] == "het70x20x12":
        # more than half the nodes in per-element units and >= 10 % of the elements in every branch: every branch is
        # inside a unit, packed or not
        assert b["het_units"] == b["units"] and b["ragged_het_units"] == 0
        assert packed == (0 if o.get("brick_no_pack") or not packs else b["het_units"])
    elif c["mesh"] == "c5_gradient_branch":
        assert b["ragged_het_units"] >= 2 and b["het_units"] >= b["ragged_het_units"]
        assert (packed > 0) == (bool(c["pack"]) and packs)
    else:
        nx, ny, nz = p["shape"]
        wide = nx - 1 if nx - 1 < 64 else 64 * ((nx - 1) // 64)
        assert b["het_units"] == 0 and packed == 0
        if o.get("brick_no_ntsame"):                                 # (the face planes then stay with the patches)
            assert b["units_one_nt_row"] == 0
        else:                                                        # both z faces ride: nz + 1 planes, whole 64-wide tiles in x
            assert b["brick_nodes"] == wide * (ny - 1) * (nz + 1) and b["units_one_nt_row"] == b["units"]
