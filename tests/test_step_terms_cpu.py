"""One step from two independent fields, the reference side, on a machine without a device (the device side:
tests/test_gpu_step_terms.py, whose cases, fields, reference and bound are the ones used here).

1. The C oracle's single step against tests/helpers.extended_step (np.longdouble) on every mesh and damping kind of the
   device cases, in double and with the float oracle on float n_t rows and fields: the worst |oracle - ref| / (2^-53 T)
   (float: 2^-24 T) per mesh is B_oracle, the yardstick of the device bound B = 16 * max(B_oracle, 4).  It is printed
   and must not exceed 64 (a broken reference cannot inflate the bar); no value is fixed in advance.
2. The check has teeth: one element's c3, c4 scaled by 1 + 2^-23 (a float ulp in zeta), one capped element given its
   uncapped lambda, one n_t row's m1 scaled by 1 + 1e-9 -- each exceeds the device bound at every node of the mutated
   element (at the node of the row), and nowhere else.
3. The planner's counters the device cases rely on, from the host-only plan checks."""
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
    d = H.solver_desc(H.step_mesh(c["mesh"], c["damping"]), pack=c["pack"])
    out = capi.brick_plan_check(d), capi.plan_check(d), capi.stencil_plan_check(d)
    assert all(r["faults"] == 0 for r in out), (c, out)
    return out


_PLANNED = [k for k, c in G.CASES.items() if c["precision"] == "f64" and c["variant"] == G.PATCH]


@pytest.mark.parametrize("case", _PLANNED, ids=_PLANNED)
def test_planner_counters_of_the_device_cases(case, monkeypatch):
    c = G.CASES[case]
    p = H.step_mesh(c["mesh"], c["damping"])
    o = c["options"] or {}
    b, pp, st = _plans(monkeypatch, c)
    packed = b["packed_units"]
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
        assert packed == (0 if o.get("brick_no_pack") else b["het_units"])
    elif c["mesh"] == "c5_gradient_branch":
        assert b["ragged_het_units"] >= 2 and b["het_units"] >= b["ragged_het_units"]
        assert (packed > 0) == bool(c["pack"])
    else:
        nx, ny, nz = p["shape"]
        wide = nx - 1 if nx - 1 < 64 else 64 * ((nx - 1) // 64)
        assert b["het_units"] == 0 and packed == 0
        if o.get("brick_no_ntsame"):                                 # (the face planes then stay with the patches)
            assert b["units_one_nt_row"] == 0
        else:                                                        # both z faces ride: nz + 1 planes, whole 64-wide tiles in x
            assert b["brick_nodes"] == wide * (ny - 1) * (nz + 1) and b["units_one_nt_row"] == b["units"]
