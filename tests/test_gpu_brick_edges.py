"""Brick kernels on degenerate footprints: ONE step from two independent fields, per node, on units the comfortable meshes
of tests/test_gpu_step_terms.py and tests/test_gpu_sources.py never produce.  The reference side, the pinned plans and the
mutations, without a device: tests/test_brick_edges_cpu.py.

hq_brick_plan_host cuts edge tiles as min(64, what is left) x min(8, what is left) (62 x 7 for hq_k_brick_het), chunks a
column into units of at most cz planes, lets a one-plane unit carry both z faces and a ragged plane own a few nodes.  The
host-only plan check follows tables; what the KERNELS make of such a unit record -- `active = lx < nx && ly < ny`, the ring
lanes t < 2 (nx + 2) + 2 ny, the face code at k == 0, 1, np + 1 (which coincide for np = 1), local = (k - 2) nxy + sidx of
the sources, the DPP x-sum, the LDS y-exchange at row ny and the float build's separate ring-B load of the per-element
kernel -- is only seen on the device.  The meshes (tests/helpers.edge_mesh), each for one named edge:

  edge66x10x8      65 x 9 interior nodes = footprints 64 x 8, 1 x 8, 64 x 1, 1 x 1; brick_cz = 2, 3, 5: units of 1, 2, 3 planes
  edge66x10x2      ONE interior plane that carries both z face planes (np = 1: top and bottom face code in one unit)
  edge3x10x8       2 x 8 and 2 x 1;  edge3x3x2: 2 x 2 x 1 + both faces, 12 nodes, the smallest brick there is
  edge130x10x6     two full 64-wide tiles with a brick on either side, then the 1-wide column
  edge66x10x36     the same four footprints 35 planes tall under the automatic cz (8): five units per column
  hetedge65x9x8    62 x 7, 2 x 7, 62 x 1, 2 x 1;  hetedge64x9x36: 62 x 7, 1 x 7, 62 x 1, 1 x 1, 20 units;  hetedge3x9x8: 2 x 7, 2 x 1
  two70x10x8s37 / s68, two66x10x8s64   a material boundary inside a tile: ragged units of both kernels whose planes own
                   as few as 27 / 3 / 3 nodes (brick_ragged_minfill = 1)

Every case: the context's counters equal the host-only plan check's for the same options (the bricks, not the patches,
step these nodes; the numbers themselves are pinned in tests/test_brick_edges_cpu.py), one step against
tests/helpers.extended_step per node and component with the bound of tests/test_gpu_step_terms.py
    |got - ref| <= B 2^-53 T,   B = 16 max(B_oracle, 4) = 64      (float state: + 2^-24 |ref|)
over ALL nodes, nothing non-finite, the old field handed back bit for bit.  A float state is also held to
tests/test_gpu_step_terms.rounded_step: got == float32(double step) bit for bit, undetermined components at most 1 in
10 000 -- 16 f32 cases, one or more for every footprint class above: cz = 2 (also by component and with per-node rows), both
faces in one unit, 2 x 8 / 2 x 1, the 12-node brick, the two full tiles, five units per column, the per-element kernel
unpacked on all three het meshes (float n_t rows under Rayleigh damping do not pack: the plan compared with hq_info is the
host-only one of the FLOAT rows) and <PACKED> without damping on hetedge65x9x8 and hetedge64x9x36, all three ragged
boundaries.  Measured: 0 mismatches, 0 components off float32(ref), undetermined 1 of 30 261 (edge130x10x6) and 1 of
72 150 (hetedge64x9x36, rayleigh), 0 elsewhere.  Then every node loaded from rest
(tests/test_gpu_sources.py's criterion, unchanged) and six steps against the oracle at the suite's 1e-9.

Footprint classes (footprint_classes below): a node's tile extent by arithmetic on its lattice position, "z face" for its
nodes on a z face plane (brick nodes where the faces ride: the uniform plans without brick_no_faces / brick_no_ntsame;
elsewhere the patches step them), "shell" for the x / y faces (always the patches').

Worst |got - ref| / (2^-53 T) per kernel family and footprint class on an MI355X (the bound is 64; no case failed, no
kernel or planner change was needed; 65 cases in 7.8 s with the float twins, 52 in 6.9 s before them, the slowest 0.8 s):
  hq_k_brick (one n_t row; cz = default, 2, 3, 5, auto 8; faces riding)
      64 x 8 1.90 - 2.03 (z face 1.54 - 1.81)   1 x 8 1.10 - 1.80 (z face 0.80 - 1.08)   64 x 1 1.32 - 1.86 (z face 1.33 - 1.56)
      1 x 1 0.34 - 1.49 (z face 0.33 - 0.53)    2 x 8 1.60 (1.29)   2 x 1 1.18 (0.42)   2 x 2 x 1 plane 0.94 (both faces 1.03)
      np = 1 units (cz = 2; edge66x10x2 with both faces in one unit): the same figures as the taller units of the same mesh
  hq_k_brick<PERNODE> (brick_no_ntsame, cz = 2)      64 x 8 1.90   1 x 8 1.44   64 x 1 1.67   1 x 1 1.42
  brick_by_component = 1                             64 x 8 1.91 - 2.03   1 x 8 1.10 - 1.80   64 x 1 1.32 - 1.86   1 x 1 0.34 - 1.49
  hq_k_brick_het unpacked (rayleigh / mass / none)   62 x 7 3.47 / 3.72 / 3.71   1 x 7 3.25 / 3.55 / 2.59   2 x 7 2.72 / 2.66 / 2.42
                                                     62 x 1 3.21 / 3.64 / 3.87   2 x 1 2.19 / 2.10 / 1.55    1 x 1 1.84 / 2.40 / 2.23
  hq_k_brick_het<PACKED>                             62 x 7 4.73 / 5.17 / 3.71   1 x 7 3.31 / 4.26 / 2.59   2 x 7 3.98 / 2.96 / 2.42
                                                     62 x 1 3.94 / 4.45 / 3.87   2 x 1 3.10 / 2.35 / 1.55    1 x 1 2.47 / 2.70 / 2.23
  ragged units of both kernels (two...s..)           soft side 1.86 - 3.32   boundary plane (per-element) 0.88 - 1.77   hard side 0.57 - 1.84
  float state (of 2^-24 |ref| + B 2^-53 T)           0.998 (brick, cz = 2), 0.991 (unpacked het), 0.999 (ragged): the state's rounding
  the shell and the faces the patches step           0.85 - 1.12 (one material), 2.0 - 2.6 (per-element)
Every node loaded from rest: 2.2e-16 of the node's own value on all three meshes (bound 1e-14).  Six steps: 7.9e-16 - 5.4e-15
of the field's maximum (bound 1e-9).
"""
import functools
import os

import numpy as np
import pytest

import hercules_amd as ha
from hercules_amd import capi
from oracle import herc_oracle as ho
from tests import helpers as H
from tests import test_gpu_sources as S
from tests import test_gpu_step_terms as G         # (its module-level guard skips this module too where longdouble is narrow)

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------
# the plans: (mesh, planner options, hand edata + material over) -- the rows of the module docstring
# ---------------------------------------------------------------------------------------------
_ONE, _EIGHT = {"brick_minnodes": 1}, {"brick_minnodes": 8}
_RAG = dict(_EIGHT, brick_ragged_minfill=1)


def _plan(mesh, options, pack=False):
    return dict(mesh=mesh, options=dict(options), pack=pack)


UNIFORM_PLANS = {
    "edge66x10x8": _plan("edge66x10x8", _ONE),
    "edge66x10x8-cz2": _plan("edge66x10x8", dict(_ONE, brick_cz=2)),
    "edge66x10x8-cz3": _plan("edge66x10x8", dict(_ONE, brick_cz=3)),
    "edge66x10x8-cz5": _plan("edge66x10x8", dict(_ONE, brick_cz=5)),
    "edge66x10x8-pernode-cz2": _plan("edge66x10x8", dict(_ONE, brick_cz=2, brick_no_ntsame=1)),
    "edge66x10x2": _plan("edge66x10x2", dict(_ONE, brick_minz=1)),
    "edge66x10x2-nofaces": _plan("edge66x10x2", dict(_ONE, brick_minz=1, brick_no_faces=1)),
    "edge3x10x8": _plan("edge3x10x8", _EIGHT),
    "edge3x3x2": _plan("edge3x3x2", dict(_ONE, brick_minz=1)),
    "edge130x10x6": _plan("edge130x10x6", _EIGHT),
    "edge66x10x36": _plan("edge66x10x36", _EIGHT),
}
HET_MESHES = ("hetedge65x9x8", "hetedge64x9x36", "hetedge3x9x8")
HET_PLANS = {}
for _m in HET_MESHES:
    HET_PLANS[_m + "-packed"] = _plan(_m, _EIGHT, pack=True)
    HET_PLANS[_m + "-nopack"] = _plan(_m, dict(_EIGHT, brick_no_pack=1), pack=True)
RAGGED_PLANS = {k: _plan(k, _RAG) for k in ("two70x10x8s37", "two70x10x8s68", "two66x10x8s64")}
PLANS = dict(UNIFORM_PLANS, **HET_PLANS, **RAGGED_PLANS)


@functools.lru_cache(maxsize=None)
def plan_report(plan, damping="rayleigh", precision="f64"):
    """capi.brick_plan_check of a plan (host only), its options through the environment for the length of the call.
    precision "f32": on the n_t rows rounded to float, as the float library's planner gets them."""
    pl = PLANS[plan]
    env = {"HQ_" + k.upper(): str(v) for k, v in pl["options"].items()}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return capi.brick_plan_check(H.solver_desc(H.step_mesh(pl["mesh"], damping), pack=pl["pack"], precision=precision))
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


# what hq_get_info says of the same plan
INFO_OF_REPORT = (("brick_nodes", "brick_nodes"), ("units", "brick_units"), ("het_units", "brick_units_het"),
                  ("ragged_units", "brick_units_ragged"), ("ragged_het_units", "brick_units_ragged_het"),
                  ("packed_units", "brick_units_packed"))


@functools.lru_cache(maxsize=None)
def footprint_classes(mesh):
    """(names, label [N]): every node's place on the planner's tile grid -- 64 x 8 from the first interior node, 62 x 7 on
    the per-element meshes --, by arithmetic on its lattice position:
      "64 x 8", "1 x 8", "64 x 1", "1 x 1", ...   the footprint of the tile column it lies in (interior planes)
      "... z face"                                the same footprint's node on a z face plane (brick nodes where faces ride)
      "shell"                                     the x and y faces: always the patches'
    The two-material meshes mix kernels around the boundary plane x = split: there the class is the footprint and the
    side -- "soft" (x < split), "boundary" (x == split: per-element nodes), "hard"."""
    p = H.step_mesh(mesh)
    nx, ny, nz = p["shape"]
    X, Y, Z = [np.asarray(p["node_ijk"])[:, d].astype(np.int64) for d in range(3)]
    tx, ty = (62, 7) if mesh.startswith("hetedge") else (64, 8)
    ti, tj = (X - 1) // tx, (Y - 1) // ty
    wx, wy = np.minimum(tx, nx - 1 - ti * tx), np.minimum(ty, ny - 1 - tj * ty)
    shell = (X == 0) | (X == nx) | (Y == 0) | (Y == ny)
    side = np.zeros(len(X), np.int64)
    if mesh.startswith("two"):
        split = int(mesh.split("s")[1])
        side = 1 + (X >= split).astype(np.int64) + (X > split).astype(np.int64)
    key = np.where(shell, -1, ((wx * 100 + wy) * 2 + ((Z == 0) | (Z == nz))) * 4 + side)
    codes, label = np.unique(key, return_inverse=True)
    names = []
    for c in codes:
        if c < 0:
            names.append("shell")
            continue
        s, f, w = int(c % 4), int(c // 4 % 2), int(c // 8)
        names.append("%d x %d%s%s" % (w // 100, w % 100, ("", " soft", " boundary", " hard")[s], " z face" if f else ""))
    return tuple(names), label


def footprint(mesh, node):
    names, label = footprint_classes(mesh)
    return "ijk (%d, %d, %d) in %s" % (*[int(v) for v in H.step_mesh(mesh)["node_ijk"][node]], names[label[node]])


def worst_by_footprint(mesh, got, ref, T, f32=False):
    """{class: (worst |got - ref| / (2^-53 T) over its nodes, nodes)} -- what a case prints and the docstring records.
    f32: in units of 2^-24 |ref| + 2^-53 T, the state's one rounding and one unit of the sums."""
    names, label = footprint_classes(mesh)
    unit = G.EPS * T + (G.float_rounding(ref, None) if f32 else 0.0)
    q = (np.abs(got.astype(np.longdouble) - ref) / unit).max(axis=1).astype(np.float64)
    return {name: (float(q[label == i].max()), int((label == i).sum())) for i, name in enumerate(names)}


# the footprint classes a mesh is here FOR: each must hold nodes (a mesh edited to a comfortable size would lose them)
NAMED_EDGES = {
    "edge66x10x8": ("1 x 8", "64 x 1", "1 x 1", "1 x 1 z face"), "edge66x10x2": ("1 x 1", "1 x 1 z face", "64 x 8 z face"),
    "edge3x10x8": ("2 x 8", "2 x 1"), "edge3x3x2": ("2 x 2", "2 x 2 z face"), "edge130x10x6": ("1 x 8", "64 x 1", "1 x 1"),
    "edge66x10x36": ("1 x 8", "64 x 1", "1 x 1"), "hetedge65x9x8": ("2 x 7", "62 x 1", "2 x 1"),
    "hetedge64x9x36": ("1 x 7", "62 x 1", "1 x 1"), "hetedge3x9x8": ("2 x 7", "2 x 1"),
    "two70x10x8s37": ("64 x 8 boundary", "64 x 1 boundary", "5 x 1 hard"),
    "two70x10x8s68": ("5 x 8 soft", "5 x 8 boundary", "5 x 1 boundary", "5 x 8 hard"),
    "two66x10x8s64": ("64 x 8 boundary", "64 x 1 boundary", "1 x 8 hard", "1 x 1 hard"),
}


# ---------------------------------------------------------------------------------------------
# one step from independent fields
# ---------------------------------------------------------------------------------------------
def _case(plan, damping="rayleigh", precision="f64", **extra):
    return dict(plan=plan, damping=damping, precision=precision, extra=extra)


CASES = {k: _case(k) for k in PLANS}
for _k in UNIFORM_PLANS:
    CASES[_k + "-bycomp"] = _case(_k, brick_by_component=1)
for _k in ("edge66x10x8-cz2", "hetedge65x9x8-nopack", "two70x10x8s68"):
    CASES["f32-" + _k] = _case(_k, precision="f32")
for _k in HET_PLANS:
    for _d in ("mass", "none"):
        CASES["%s-%s" % (_k, _d)] = _case(_k, _d)
# float twins of the footprint classes the three f32 cases above do not reach: per-node rows, both z faces in one unit,
# 2 x 8 / 2 x 1 / 2 x 2, two full tiles beside the 1-wide column, five units per column, 1 x 7 / 1 x 1 / 2 x 7 of the
# per-element kernel, the other two ragged boundaries.  Float n_t rows pack only without damping (G.float_rows_pack): the
# packed form on degenerate footprints has its float cases there; assert_runs_the_checked_plan compares hq_info with the
# host-only plan of the FLOAT rows, tests/test_brick_edges_cpu.py pins what that plan is
for _k in ("edge66x10x8-pernode-cz2", "edge66x10x2", "edge3x10x8", "edge3x3x2", "edge130x10x6", "edge66x10x36",
           "hetedge64x9x36-nopack", "hetedge3x9x8-nopack", "two70x10x8s37", "two66x10x8s64"):
    CASES["f32-" + _k] = _case(_k, precision="f32")
CASES["f32-edge66x10x8-cz2-bycomp"] = _case("edge66x10x8-cz2", precision="f32", brick_by_component=1)
for _k in ("hetedge65x9x8-packed", "hetedge64x9x36-packed"):
    CASES["f32-%s-none" % _k] = _case(_k, "none", precision="f32")


def make(c, p, nt, u1=None, u2=None):
    pl = PLANS[c["plan"]]
    kw = dict(edata=p["edata"], material=p["material"]) if pl["pack"] else {}
    return ha.Solver(p["lnid"], p["etable"], nt, p["dt"], tm1=u1, tm2=u2, dangling=None, node_xyz=p["node_xyz"],
                     variant=G.PATCH, options=dict(pl["options"], **c["extra"]), precision=c["precision"], **kw)


def assert_runs_the_checked_plan(s, c):
    """The context's counters are the host-only plan check's for the same options, and its options are the case's."""
    rep, info, o = plan_report(c["plan"], c["damping"], c["precision"]), s.info(), s.options()
    assert rep["faults"] == 0 and info["variant"] == G.PATCH
    for r, i in INFO_OF_REPORT:
        assert rep[r] == info[i], (c, r, rep[r], i, info[i])
    assert info["brick_units_pernode"] == rep["units"] - rep["units_one_nt_row"] - rep["het_units"], (rep, info)
    for k, v in dict(PLANS[c["plan"]]["options"], **c["extra"]).items():
        assert o[k] == v, (k, o[k], v)
    return rep


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_one_step_on_degenerate_footprints(case):
    c = CASES[case]
    mesh = PLANS[c["plan"]]["mesh"]
    p = H.step_mesh(mesh, c["damping"])
    f32 = c["precision"] == "f32"
    nt, u1, u2, ref, T, _ = G.reference(mesh, c["damping"], c["precision"])
    B = G.bound_factor(mesh, c["damping"])
    s = make(c, p, nt, u1, u2)
    try:
        rep = assert_runs_the_checked_plan(s, c)
        family = G.family_of(s)
        s.run(1)
        got, old = s.download()
        nonfinite = s.check_finite()
    finally:
        s.close()
    assert nonfinite == 0 and np.isfinite(got).all()
    assert got.dtype == old.dtype == u1.dtype == (np.float32 if f32 else np.float64) and got.shape == ref.shape
    assert np.array_equal(old.view(np.uint8), np.asarray(u1).view(np.uint8))          # the old field, bit for bit
    w = G.worst(got, ref, T, B, f32, None)                                               # over every node: none is left out
    by = worst_by_footprint(mesh, got, ref, T, f32)
    assert sum(n for _, n in by.values()) == p["N"] and all(by[k][1] > 0 for k in NAMED_EDGES[mesh]), (sorted(by), NAMED_EDGES[mesh])
    print("\n[brick-edges] %-36s %-8s nodes %6d (bricks %6d in %2d units) worst %.3f of the bound at node %d.%d: %s%s"
          % (case, c["damping"], p["N"], rep["brick_nodes"], rep["units"], w[0], w[1], w[2], footprint(mesh, w[1]),
             " (f32: the state's rounding, 2^-24 |ref|, is nearly all of the bound)" if f32 else ""))
    print("[brick-edges]     |got - ref| / (%s2^-53 T) by footprint: " % ("2^-24 |ref| + " if f32 else "")
          + " | ".join("%s %.3g" % (k, v[0]) for k, v in by.items()))
    assert w[0] <= 1.0, (w, footprint(mesh, w[1]), got[w[1]], np.asarray(ref[w[1]], np.float64), G.branch_of(p, w[1]))
    if f32:                                                        # one step of the float library is float32(double step)
        r = G.rounded_step(got, ref, T, B, None)
        print("[brick-edges]     float32(double step): mismatches %d, undetermined %d of %d, got != float32(ref) inside the band %d"
              % (r["mismatches"], r["undetermined"], r["plain"], r["off_centre"]))
        G.assert_rounded_step(case, r, family, (footprint(mesh, r["first"][0]), G.branch_of(p, r["first"][0])) if r["first"] else None)


# ---------------------------------------------------------------------------------------------
# every node loaded, one step from rest: tests/test_gpu_sources.py's cases on these meshes (its bounds, its reference)
# ---------------------------------------------------------------------------------------------
def _chk_plan(plan):
    def chk(s, p, name):
        rep = assert_runs_the_checked_plan(s, _case(plan))
        assert 2 * rep["brick_nodes"] > p["N"] and s.dominant_kernel() == "hq_k_brick"
    return chk


SOURCE_CASES = {k: S._case(PLANS[k]["mesh"], _chk_plan(k), options=PLANS[k]["options"], pack=PLANS[k]["pack"])
                for k in ("edge66x10x8-cz2", "edge66x10x2", "hetedge65x9x8-packed")}


@pytest.mark.parametrize("case", list(SOURCE_CASES), ids=list(SOURCE_CASES))
def test_every_node_loaded_on_degenerate_footprints(case):
    """The kernels' `local` index of a loaded node on 1-wide columns, one-plane units and both face planes: a source that
    lands on a neighbour, in another plane or not at all shows at that node (1e-14 of its own value)."""
    S.one_step_from_rest(case, SOURCE_CASES[case], "all")


# ---------------------------------------------------------------------------------------------
# six steps: each of the three state buffers is written twice by the degenerate units
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["edge66x10x8-cz2", "hetedge64x9x36-packed", "two70x10x8s68"])
def test_six_steps_on_degenerate_footprints(plan):
    c = _case(plan)
    mesh = PLANS[plan]["mesh"]
    p = H.step_mesh(mesh)
    nt, u1, u2, _, _, _ = G.reference(mesh)
    o1, o2 = u2.copy(), u1.copy()
    ho.solver_run(p["lnid"], p["etable"], np.ascontiguousarray(nt), o1, o2, 0, 6, p["dt"], damping=p["kind"], dangling=None)
    s = make(c, p, nt, u1, u2)
    try:
        assert_runs_the_checked_plan(s, c)
        s.run(6)
        tm1, tm2 = s.download()
        nonfinite = s.check_finite()
    finally:
        s.close()
    e1, e2 = H.rel_linf(tm1, o2), H.rel_linf(tm2, o1)
    print("\n[brick-edges] six steps %-28s rel_linf %.2e %.2e (max |u| %.2e)" % (plan, e1, e2, np.abs(o2).max()))
    assert nonfinite == 0 and e1 < S.TOL_RUN and e2 < S.TOL_RUN, (e1, e2)
