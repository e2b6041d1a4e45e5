"""Brick kernels on degenerate footprints, the side that needs no device (the device side: tests/test_gpu_brick_edges.py,
whose plans, cases, fields, reference and bound are the ones used here).

1. Every (mesh, options) pair of the device cases through the host-only plan check: no faults, and the counters PINNED --
   columns, units, brick nodes, units with one n_t row, per-element / ragged / packed units, the smallest nx, ny and np of
   any unit, the fewest nodes a ragged plane owns.  They say by arithmetic which footprints exist (65 x 9 interior nodes in
   four columns of which the smallest unit is 1 x 1 can only be 64 x 8, 1 x 8, 64 x 1, 1 x 1) and that the bricks, not the
   patches, step them; a planner change that takes a degenerate unit away from a mesh shows here.
2. The C oracle's single step against tests/helpers.extended_step on every mesh and damping kind of the device cases:
   B_oracle, printed, at most 64 (tests/test_gpu_step_terms.bound_factor); no value is fixed in advance.
3. The criterion sees a wrong ring or exchange value where these meshes put one: u1 of the single node of the 1 x 1
   column's middle plane (of one node of the 62 x 1 row) scaled by 1 + 1e-9 exceeds the device bound at that node and its
   26 neighbours, and nowhere else.
4. The float cases: their plans on n_t rows rounded to float are the pinned ones, except that per-element units pack only
   without damping; and the criterion of a float state (tests/test_gpu_step_terms.rounded_step: one step = float32(double
   step)) is met by the rounded double oracle on every mesh and damping kind of those cases, undetermined components
   printed and under the cap (1 of 30 261 on edge130x10x6, 1 of 72 150 on hetedge64x9x36, 0 elsewhere)."""
import numpy as np
import pytest

from tests import helpers as H
from tests import test_gpu_brick_edges as E
from tests import test_gpu_step_terms as G

# counters of capi.brick_plan_check, pinned: (columns, units, brick_nodes, units_one_nt_row, het_units, packed_units,
# ragged_units, ragged_nodes, ragged_het_units, ragged_het_nodes, min nx, min ny, min np, fewest nodes of a ragged plane,
# one-plane units with both faces)
_KEYS = ("columns", "units", "brick_nodes", "units_one_nt_row", "het_units", "packed_units", "ragged_units", "ragged_nodes",
         "ragged_het_units", "ragged_het_nodes", "min_unit_nx", "min_unit_ny", "min_unit_np", "ragged_min_plane_nodes",
         "units_one_plane_both_faces")
PINNED = {
    # 65 x 9 interior nodes x (7 planes + both z faces) = 5265; the 7 planes of a column in ceil(7 / cz) even chunks
    "edge66x10x8": (4, 4, 65 * 9 * 9, 4, 0, 0, 0, 0, 0, 0, 1, 1, 7, 0, 0),
    "edge66x10x8-cz2": (4, 16, 5265, 16, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0),
    "edge66x10x8-cz3": (4, 12, 5265, 12, 0, 0, 0, 0, 0, 0, 1, 1, 2, 0, 0),
    "edge66x10x8-cz5": (4, 8, 5265, 8, 0, 0, 0, 0, 0, 0, 1, 1, 3, 0, 0),
    # per-node n_t rows: the face planes stay with the patches, 65 x 9 x 7 = 4095
    "edge66x10x8-pernode-cz2": (4, 16, 65 * 9 * 7, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0),
    # one interior plane with both faces: 65 x 9 x 3 = 1755; without the faces 585
    "edge66x10x2": (4, 4, 65 * 9 * 3, 4, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 4),
    "edge66x10x2-nofaces": (4, 4, 65 * 9, 4, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0),
    "edge3x10x8": (2, 2, 2 * 9 * 9, 2, 0, 0, 0, 0, 0, 0, 2, 1, 7, 0, 0),
    "edge3x3x2": (1, 1, 2 * 2 * 3, 1, 0, 0, 0, 0, 0, 0, 2, 2, 1, 0, 1),
    # 129 x 9 interior nodes x 7; the 1 x 1 column of 5 planes is below brick_minnodes = 8 and stays with the patches
    "edge130x10x6": (5, 5, 129 * 9 * 7 - 7, 5, 0, 0, 0, 0, 0, 0, 1, 1, 5, 0, 0),
    # 35 planes under the automatic cz = 8: five units of 7 planes per column
    "edge66x10x36": (4, 20, 65 * 9 * 37, 20, 0, 0, 0, 0, 0, 0, 1, 1, 7, 0, 0),
    "hetedge65x9x8-packed": (4, 4, 64 * 8 * 7, 0, 4, 4, 0, 0, 0, 0, 2, 1, 7, 0, 0),
    "hetedge65x9x8-nopack": (4, 4, 64 * 8 * 7, 0, 4, 0, 0, 0, 0, 0, 2, 1, 7, 0, 0),
    "hetedge64x9x36-packed": (4, 20, 63 * 8 * 35, 0, 20, 20, 0, 0, 0, 0, 1, 1, 7, 0, 0),
    "hetedge64x9x36-nopack": (4, 20, 63 * 8 * 35, 0, 20, 0, 0, 0, 0, 0, 1, 1, 7, 0, 0),
    "hetedge3x9x8-packed": (2, 2, 2 * 8 * 7, 0, 2, 2, 0, 0, 0, 0, 2, 1, 7, 0, 0),
    "hetedge3x9x8-nopack": (2, 2, 2 * 8 * 7, 0, 2, 0, 0, 0, 0, 0, 2, 1, 7, 0, 0),
    "two70x10x8s37": (8, 8, 4437, 6, 2, 0, 4, 3969, 0, 0, 1, 1, 7, 27, 0),
    "two70x10x8s68": (7, 7, 5499, 5, 2, 0, 3, 245, 2, 70, 2, 1, 7, 3, 0),
    "two66x10x8s64": (5, 5, 4111, 3, 2, 0, 2, 3969, 2, 70, 1, 1, 7, 3, 0),
}


def test_every_plan_of_the_device_cases_is_pinned():
    assert set(PINNED) == set(E.PLANS) and {c["plan"] for c in E.CASES.values()} == set(E.PLANS)


@pytest.mark.parametrize("plan", list(E.PLANS), ids=list(E.PLANS))
def test_the_planner_makes_the_degenerate_units(plan):
    pl = E.PLANS[plan]
    dampings = ("rayleigh", "mass", "none") if plan in E.HET_PLANS else ("rayleigh",)
    for damping in dampings:                                         # (the plan does not depend on the damping kind)
        rep = E.plan_report(plan, damping)
        got = tuple(rep[k] for k in _KEYS)
        print("\n[brick-edges] plan %-26s %-8s %s" % (plan, damping, dict(zip(_KEYS, got))))
        assert rep["faults"] == 0 and rep["neighbours_checked"] > 0, rep
        assert got == PINNED[plan], dict(zip(_KEYS, zip(got, PINNED[plan])))
        assert rep["brick_nodes"] + rep["patch_nodes"] == H.step_mesh(pl["mesh"], damping)["N"]


@pytest.mark.parametrize("plan", list(E.UNIFORM_PLANS) + list(E.HET_PLANS))
def test_the_brick_nodes_are_the_nodes_of_the_named_footprints(plan):
    """tests/test_gpu_brick_edges.footprint_classes sorts every node by arithmetic on its lattice position; the classes a
    mesh is named for hold nodes, and the plan's brick nodes are exactly the nodes of the classes the bricks are expected
    to step: with 4 (or 2, 5) columns and that count, every one of these footprints is a brick column and none of its nodes
    is a patch node."""
    pl = E.PLANS[plan]
    mesh, o = pl["mesh"], pl["options"]
    names, label = E.footprint_classes(mesh)
    size = {k: int((label == i).sum()) for i, k in enumerate(names)}
    assert all(size.get(k, 0) > 0 for k in E.NAMED_EDGES[mesh]), (size, E.NAMED_EDGES[mesh])
    faces_ride = not (mesh.startswith("het") or o.get("brick_no_faces") or o.get("brick_no_ntsame"))
    stepped = {k for k in names if k != "shell" and (faces_ride or not k.endswith("z face"))}
    if mesh == "edge130x10x6":                                     # 1 x 1 x 5 planes < brick_minnodes = 8
        stepped -= {"1 x 1", "1 x 1 z face"}
    rep = E.plan_report(plan)
    assert rep["brick_nodes"] == sum(size[k] for k in stepped), (rep["brick_nodes"], size, sorted(stepped))
    # (edge130x10x6 has two 64 x 8 and two 64 x 1 columns: a class there is two tiles)
    assert rep["columns"] == len({k.replace(" z face", "") for k in stepped}) + (2 if mesh == "edge130x10x6" else 0)
    if mesh == "edge66x10x8":
        assert (size["1 x 1"], size["1 x 1 z face"], size["1 x 8"], size["64 x 1"]) == (7, 2, 56, 448)


@pytest.mark.parametrize("mesh", list(E.RAGGED_PLANS))
def test_the_ragged_meshes_named_footprints_hold_nodes(mesh):
    names, label = E.footprint_classes(mesh)
    assert all(k in names for k in E.NAMED_EDGES[mesh]), (names, E.NAMED_EDGES[mesh])
    # the nodes whose eight elements differ are those of the boundary plane, 9 x 7 interior ones: two per-element units
    rep = E.plan_report(mesh)
    boundary = sum(int((label == i).sum()) for i, k in enumerate(names) if "boundary" in k and not k.endswith("z face"))
    assert boundary == 9 * 7 and rep["het_units"] == 2


MESHES = sorted({(E.PLANS[c["plan"]]["mesh"], c["damping"]) for c in E.CASES.values()})
MESHES_F32 = sorted({(E.PLANS[c["plan"]]["mesh"], c["damping"]) for c in E.CASES.values() if c["precision"] == "f32"})


@pytest.mark.parametrize("mesh,damping", MESHES, ids=["%s-%s" % m for m in MESHES])
def test_oracle_step_against_the_extended_reference(mesh, damping):
    p = H.step_mesh(mesh, damping)
    nt, u1, u2, ref, T, b = G.reference(mesh, damping)
    assert min(np.abs(u1).min(), np.abs(u2).min()) >= 0.5e-3 * (1 - 1e-6) and np.abs(u1 - u2).max() > 1.5e-3
    share = 1.0 - (np.abs(nt[:, 1:4] * u1) + np.abs(nt[:, 4:7] * u2)) / np.abs(nt[:, :1]) / T
    print("\n[brick-edges] B_oracle %-16s %-8s %.2f; dt %.3e, median share of the element forces in T %.3f"
          % (mesh, damping, b, p["dt"], float(np.median(share))))
    assert np.isfinite(b) and b <= 64.0 and G.bound_factor(mesh, damping) == 16.0 * max(b, 4.0)
    assert float(np.median(share)) > 0.01                        # the force term is not lost beside 2 u1 - u2
    if "labels" in p:                                            # every branch in >= 10 % of the elements
        assert all(p["labels"][k].sum() * 10 >= p["E"] for k in H.BRANCHES)
        assert (damping == "rayleigh") == bool(p["etable"][:, 2].any())


@pytest.mark.parametrize("mesh,damping", MESHES_F32, ids=["%s-%s" % m for m in MESHES_F32])
def test_float_oracle_step_against_the_extended_reference(mesh, damping):
    p = H.step_mesh(mesh, damping)
    nt, u1, u2, ref, T, b = G.reference(mesh, damping, "f32")
    assert nt.dtype == u1.dtype == G.oracle_step(p, nt, u1, u2).dtype == np.float32
    print("\n[brick-edges] B_oracle (float, of 2^-24 T) %-16s %-8s %.2f" % (mesh, damping, b))
    assert np.isfinite(b) and b <= 64.0


@pytest.mark.parametrize("mesh,damping", MESHES_F32, ids=["%s-%s" % m for m in MESHES_F32])
def test_rounded_double_step_meets_the_float_criterion(mesh, damping):
    """The float cases' criterion (tests/test_gpu_step_terms.rounded_step: one step = float32(double step)) is satisfiable
    on these meshes and fields: the double oracle on the widened float rows, rounded once, has no mismatch and stays under
    the cap of undetermined components."""
    p = H.step_mesh(mesh, damping)
    nt, u1, u2, ref, T, _ = G.reference(mesh, damping, "f32")
    B = G.bound_factor(mesh, damping)
    got = G.float_model(p, nt, u1, u2)
    r = G.rounded_step(got, ref, T, B, None)
    print("\n[brick-edges] float32(double oracle) %-16s %-8s mismatches %d, undetermined %d of %d (cap %d)"
          % (mesh, damping, r["mismatches"], r["undetermined"], r["plain"], int(G.UNDETERMINED_CAP * r["plain"])))
    G.assert_rounded_step("%s-%s" % (mesh, damping), r, "float32(double oracle)")
    assert G.additive_bound_trips(got, ref, T, B, None) == 0


F32_CASES = [k for k, c in E.CASES.items() if c["precision"] == "f32"]


@pytest.mark.parametrize("case", F32_CASES, ids=F32_CASES)
def test_the_float_rows_leave_the_pinned_plan(case):
    """The n_t rows are rounded to float before the planner sees them; NTSAME and packing read them.  The plan of a float
    case is the pinned one, except that per-element units pack only where the rows are undamped (G.float_rows_pack)."""
    c = E.CASES[case]
    rep = E.plan_report(c["plan"], c["damping"], "f32")
    want = dict(zip(_KEYS, PINNED[c["plan"]]))
    if not G.float_rows_pack(c["damping"]):
        want["packed_units"] = 0
    assert rep["faults"] == 0 and {k: rep[k] for k in _KEYS} == want, (rep, want)
    if case.endswith("-packed-none"):
        assert rep["packed_units"] == rep["het_units"] > 0       # the packed form of the float build is what these two run


def _node_at(p, X, Y, Z):
    hit = np.nonzero((p["node_ijk"] == (X, Y, Z)).all(axis=1))[0]
    assert len(hit) == 1
    return int(hit[0])


# (mesh, the mutated node's lattice position, what it is)
MUTATIONS = [("edge66x10x8", (65, 9, 4), "the single node of the 1 x 1 column's middle plane"),
             ("hetedge65x9x8", (31, 8, 4), "a node of the 62 x 1 row's middle plane")]


@pytest.mark.parametrize("mesh,at,what", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_a_wrong_value_at_a_degenerate_footprint_trips_its_neighbours_only(mesh, at, what):
    """What a kernel that loads a wrong ring, DPP or exchange value for such a node would compute: u1 of that one node off
    by 1e-9 of itself.  The tripped nodes are the node and its 26 neighbours -- in the 1 x 1 column all 8 in-plane
    neighbours are ring nodes of three other footprints --, no more and no fewer."""
    p = H.step_mesh(mesh)
    nx, ny, nz = p["shape"]
    tx, ty = (62, 7) if mesh.startswith("het") else (64, 8)
    # the node lies where the docstring says: last tile column / row, whose extent is 1
    assert (at[1] - 1) // ty == (ny - 2) // ty and ny - 1 - ((at[1] - 1) // ty) * ty == 1
    if mesh == "edge66x10x8":
        assert (at[0] - 1) // tx == (nx - 2) // tx and nx - 1 - ((at[0] - 1) // tx) * tx == 1
    nt, u1, u2, ref, T, _ = G.reference(mesh)
    B = G.bound_factor(mesh, "rayleigh")
    trip = lambda got: set(np.nonzero((np.abs(got - ref) > B * G.EPS * T).any(axis=1))[0].tolist())
    assert B == 64.0 and not trip(G.oracle_step(p, nt, u1, u2))
    n = _node_at(p, *at)
    near = {_node_at(p, at[0] + dx, at[1] + dy, at[2] + dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)}
    bad = np.array(u1)
    bad[n] *= 1.0 + 1e-9
    hit = trip(G.oracle_step(p, nt, bad, u2))
    print("\n[brick-edges] %s, %s (node %d) x (1 + 1e-9): %d nodes tripped" % (mesh, what, n, len(hit)))
    assert len(near) == 27 and hit == near, (sorted(hit - near), sorted(near - hit))
