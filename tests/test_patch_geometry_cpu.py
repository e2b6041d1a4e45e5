"""Patch plans off the default geometry, the reference side, on a machine without a device (the device side: the geometry
keys of tests/test_gpu_step_terms.py -- and through it tests/test_gpu_loaded_step.py -- and of
tests/test_gpu_partition_step.py, whose geometries, meshes and partitions are the ones used here).

hq_options.patch_threads / _pmax / _pmerge / _psplit / _nlmax / _vmax (HQ_PATCH_* in the environment) decide what the patch
kernels index by: workgroup size against owned nodes, the LDS image, the WFORM flag, hstride, the planner's halving path,
whether the persistent kernels take the plan at all, how many patches meet the work queue, the stencil kernel's shape tables.
The host-only checks (hq_plan_check, hq_stencil_plan_check) plan what hq_create plans without bricks and verify the plan
against the mesh; here, for every (mesh, geometry) pair of the device cases and every rank of the partition cases:
1. the plan is clean (faults == 0) and every patch respects the geometry (patches >= N / pmax);
2. the structural condition that makes the case mean what it is there for holds on the report (STRUCTURE below);
3. two geometries of one mesh that differ in a field the planner reads give different plans, and each differs from the
   default plan (patch_threads and patch_pipe belong to the launch: those plans ARE the default plan);
4. the settings the planner cannot serve are refused with a message, and a geometry whose accumulators alone exceed the LDS
   budget is refused as such (hq_patch_cfg_of's loop used to run nlmax through zero and the unsigned wrap-around, and the plan
   was then refused by accident as "a single node reaches more neighbours than LDS can stage")."""
import pytest

from hercules_amd import capi
from tests import helpers as H
from tests import test_gpu_step_terms as ST        # (its module-level guard skips this module too where longdouble is narrow)
from tests import test_gpu_partition_step as GP

PLANNER_FIELDS = ("patch_pmax", "patch_pmerge", "patch_psplit", "patch_nlmax", "patch_vmax")


def _planner_part(g):
    """What of a geometry the planner reads: its fields but threads and pipe, and whether there are coordinates."""
    return (tuple(sorted((k, v) for k, v in ST.GEOMETRY[g].items() if k in PLANNER_FIELDS)), ST.geometry_has_xyz(g))


def _hanging(p):
    return p["dangling"] is not None and len(p["dangling"][0]) > 0


# (mesh or None = every mesh, geometry) -> a condition on (plan, stencil or None, default plan, default stencil, the mesh)
STRUCTURE = {
    (None, "threads64"): lambda pl, st, d, ds, p: pl == d and st == ds,                     # the launch changes, the plan does not
    (None, "threads192"): lambda pl, st, d, ds, p: pl == d and st == ds,
    (None, "pmax8"): lambda pl, st, d, ds, p: 8 * pl["patches"] >= p["N"] and pl["lattice_patches"] == 0,
    (None, "pmax8-step"): lambda pl, st, d, ds, p: 8 * pl["patches"] >= p["N"] and pl["lattice_patches"] == 0,
    ("box32", "pmax8"): lambda pl, st, d, ds, p: st["tables"] == pl["patches"] and st["full_lattices"] == 0,
    ("box32", "pmax27-pmerge1"): lambda pl, st, d, ds, p: 27 * pl["patches"] >= p["N"] and st["tables"] == pl["patches"],
    ("c5_gradient_branch", "pmax27-pmerge1"): lambda pl, st, d, ds, p: 27 * pl["patches"] >= p["N"],
    (None, "nlmax72"): lambda pl, st, d, ds, p: 64 * pl["patches"] > p["N"] and pl["patches"] > d["patches"],
    ("box32", "psplit100"): lambda pl, st, d, ds, p: 0 < st["tables"] < pl["patches"],       # stencil and element form side by side
    ("c5_gradient_branch", "psplit100"): lambda pl, st, d, ds, p: pl["patches"] > d["patches"],
    ("box32", "pmax728"): lambda pl, st, d, ds, p: (pl["lattice_patches"] == 0 < d["lattice_patches"] == ds["full_lattices"] == st["full_lattices"]
                                                    and st["tables"] == pl["patches"]),
    ("box32", "nlmax776"): lambda pl, st, d, ds, p: pl["lattice_patches"] == 0 and st["tables"] == pl["patches"] > d["patches"],
    (None, "nlmax776"): lambda pl, st, d, ds, p: pl["patches"] > d["patches"],
    (None, "pmax1016"): lambda pl, st, d, ds, p: pl["pairs"] != d["pairs"],
    (None, "big"): lambda pl, st, d, ds, p: pl["patches"] < d["patches"] and pl["lattice_patches"] == 0,
    ("box32", "big"): lambda pl, st, d, ds, p: st["tables"] == 0 < ds["tables"],             # a uniform box with no stencil patch
    ("two_level", "big"): lambda pl, st, d, ds, p: pl["patches"] < 8,                        # fewer patches than XCD slots
    (None, "vmax8"): lambda pl, st, d, ds, p: pl["patches"] > d["patches"],                  # halved for the hanging-node accumulators
    (None, "vmax40"): lambda pl, st, d, ds, p: pl["patches"] > d["patches"],
    (None, "noxyz-pmerge100"): lambda pl, st, d, ds, p: st is None and 100 * pl["patches"] >= p["N"] and pl["lattice_patches"] == 0,
    (None, "noxyz-pmerge37-pmax64"): lambda pl, st, d, ds, p: st is None and 37 * pl["patches"] >= p["N"] and pl["lattice_patches"] == 0,
}


@pytest.mark.parametrize("mesh,g", ST.GEOMETRY_PAIRS, ids=["%s-%s" % (g, m) for m, g in ST.GEOMETRY_PAIRS])
def test_geometry_plans_are_clean_and_mean_what_the_case_is_about(mesh, g):
    p = H.step_mesh(mesh)
    plan, st = ST.host_plans(mesh, "rayleigh", g)
    default, dst = ST.host_plans(mesh, "rayleigh", None)
    cfg = ST.patch_cfg(ST.GEOMETRY[g], _hanging(p))
    print("\n[geometry] %-24s %-20s N %6d: patches %d -> %d, pairs %d -> %d, lattice %d -> %d, tables %d -> %s (full %d -> %s); cfg %s"
          % (g, mesh, p["N"], default["patches"], plan["patches"], default["pairs"], plan["pairs"], default["lattice_patches"],
             plan["lattice_patches"], dst["tables"], st and st["tables"], dst["full_lattices"], st and st["full_lattices"], cfg))
    assert plan["faults"] == 0 and default["faults"] == 0 and dst["faults"] == 0 and (st is None or st["faults"] == 0)
    assert (st is None) == (not ST.geometry_has_xyz(g)) and (st is None or st["patches"] == plan["patches"])
    assert cfg["pmax"] * plan["patches"] >= p["N"] and plan["pairs"] >= p["E"]
    if cfg["pmax"] < ST.HQ_LAT_ACC or cfg["nlmax"] < 1000:
        assert plan["lattice_patches"] == 0                      # a lattice patch is 9^3 owned nodes in a 10^3 image
    conditions = [STRUCTURE[k] for k in ((mesh, g), (None, g)) if k in STRUCTURE]
    assert conditions, "no structural condition for %s on %s" % (g, mesh)
    for cond in conditions:
        assert cond(plan, st, default, dst, p), (mesh, g, plan, st, default, dst)
    if _planner_part(g)[0]:
        assert plan != default
    # which kernel steps the element-form patches follows from the options alone: the device check's expectation
    assert ST.steps_per_patch(ST.GEOMETRY[g], _hanging(p)) == (g == "big" or g.startswith("threads") or g.endswith("-step"))


@pytest.mark.parametrize("mesh", list(ST.GEOMETRY_MESHES))
def test_two_geometries_of_one_mesh_give_two_plans(mesh):
    reports = {}
    for g in ST.GEOMETRY_MESHES[mesh]:
        reports.setdefault(_planner_part(g), []).append(ST.host_plans(mesh, "rayleigh", g)[0])
    reports.setdefault(((), True), []).append(ST.host_plans(mesh, "rayleigh", None)[0])
    for same in reports.values():                                # (pmax8 / pmax8-step, threads64 / threads192 / the defaults)
        assert all(r == same[0] for r in same), same
    keys = list(reports)
    assert len(keys) >= 4
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            assert reports[a][0] != reports[b][0], (mesh, a, b, reports[a][0])


# ---------------------------------------------------------------------------------------------
# the partition cases: every rank
# ---------------------------------------------------------------------------------------------
PARTITION_GEOMETRY = [k for k, c in dict(GP.CASES, **GP.LOADED_CASES).items() if any(f in c["options"] for f in ST._GEOMETRY_FIELDS[2:])]


def _box_reports(c, fn):
    boxes = H.box_step_boxes(c["mesh"], c["nranks"])
    try:
        with pytest.MonkeyPatch.context() as mp:
            ST.plan_environment(mp, c["options"])
            return [getattr(b, fn)() for b in boxes]
    finally:
        for b in boxes:
            b.close()


@pytest.mark.parametrize("case", PARTITION_GEOMETRY, ids=PARTITION_GEOMETRY)
def test_geometry_plans_of_the_partition_cases(case):
    c = dict(GP.CASES, **GP.LOADED_CASES)[case]
    q = GP.problem_of(c)
    plain = dict(c, options={})
    if c["kind"] == "box":
        plans, defaults = _box_reports(c, "plan_check"), _box_reports(plain, "plan_check")
    else:
        plans, defaults = GP.rank_plans(c, q), GP.rank_plans(plain, q)
    hanging = [c["kind"] == "oct" and len(part["dangling"][0]) > 0 for part in (q["parts"] if c["kind"] == "oct" else [None] * c["nranks"])]
    sizes = [len(g) for g in q["gid"]]
    print("\n[geometry] %-28s patches per rank %s (default %s)" % (case, [r["patches"] for r in plans], [r["patches"] for r in defaults]))
    for r, (plan, default) in enumerate(zip(plans, defaults)):
        cfg = ST.patch_cfg(c["options"], hanging[r])
        assert plan["faults"] == 0 and default["faults"] == 0, (r, plan, default)
        assert cfg["pmax"] * plan["patches"] >= sizes[r], (r, plan, cfg)
        if c["options"].get("patch_pmax") == 1500:               # "big": interface and interior work in one patch
            assert plan["patches"] == 1 <= default["patches"], (r, plan, default)
        elif c["options"].get("patch_pmax") == 8:                # two orders of magnitude more entries in d_order and the queue
            assert plan["patches"] >= 20 * default["patches"] and plan["lattice_patches"] == 0, (r, plan, default)
        else:                                                    # (a smaller image or fewer accumulators halve where they do not fit)
            assert plan["patches"] >= default["patches"], (r, plan, default)
    assert sum(plan["patches"] for plan in plans) != sum(default["patches"] for default in defaults), (plans, defaults)
    # one planner for every rank: the options decide the kernel of the element-form patches as on one rank
    assert ST.steps_per_patch(c["options"], True) == (("kernel", "hq_k_patch_step") in c["route"])


def test_small_cubes_keep_the_stencil_route_of_the_box_partitions():
    """The box_stencil route's conditions (GP.check_route) for patch_pmax = 8 on the two ranks of GP.BOX_STENCIL[2], from the
    boxes' own stencil_plan_check: shape tables on every rank, ragged ones among them (none is a full 9^3 lattice), and a rank
    that owns interface nodes has nothing but lattice subsets -- hq_k_patch_stencil's launch ahead of the exchange."""
    c = GP.CASES["box-2-stencil-pmax8-ov0"]
    assert c["options"]["patch_pmax"] == 8 and c["route"] == ("box_stencil",)
    q = GP.problem_of(c)
    owns = [any(k.startswith("owned-interface") for k in kinds) for kinds in GP.node_kinds(q)]
    tables = _box_reports(c, "stencil_plan_check")
    print("\n[geometry] box-2-stencil-pmax8: owns interface nodes %s, tables %s" % (owns, tables))
    assert all(st["faults"] == 0 and st["tables"] > 0 and st["full_lattices"] < st["tables"] for st in tables), tables
    assert any(o and st["tables"] == st["patches"] for o, st in zip(owns, tables)), (owns, tables)


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
ALL_CHECKS = ("plan_check", "stencil_plan_check", "brick_plan_check")


def _refused(monkeypatch, mesh, options, *words, checks=ALL_CHECKS):
    """Every check of `checks` refuses the mesh under the options with HQ_ERR_ARG and all the words -> the messages."""
    ST.plan_environment(monkeypatch, options)
    d = H.solver_desc(H.step_mesh(mesh))
    out = []
    for check in checks:
        with pytest.raises(capi.HqError) as e:
            getattr(capi, check)(d)
        assert str(e.value).startswith("hq error -1: patch plan: ") and all(w in str(e.value) for w in words), (check, str(e.value))
        out.append(str(e.value))
    return out


@pytest.mark.parametrize("mesh,options", ST.REFUSED, ids=["%s-%s" % (m, "-".join("%s%d" % (k[6:], v) for k, v in o.items())) for m, o in ST.REFUSED])
def test_settings_the_planner_cannot_serve_are_refused(mesh, options, monkeypatch):
    """One node's element neighbours and hanging-node accumulators exceed what the setting leaves: halving ends at one node.
    The two checks that plan the whole mesh without bricks, as hq_create does under no_bricks = 1 (hq_brick_plan_check plans
    the shell behind the bricks alone, which two_level's setting still fits)."""
    _refused(monkeypatch, mesh, options, ST.REFUSAL, checks=ALL_CHECKS[:2])
    ST.plan_environment(monkeypatch, {})                         # the same description plans clean at the defaults
    assert capi.plan_check(H.solver_desc(H.step_mesh(mesh)))["faults"] == 0


@pytest.mark.parametrize("options", [dict(patch_pmax=6900), dict(patch_pmax=3400, patch_vmax=3500), dict(patch_pmax=6820)],
                         ids=["pmax6900", "pmax3400-vmax3500", "pmax6820"])
def test_accumulators_over_the_lds_budget_are_refused_as_such(options, monkeypatch):
    """3 (pmax + vmax) doubles of accumulators beside an image of at least 8 rows must fit 160 KiB: 6 900 owned nodes alone are
    165 600 bytes; 6 820 (+ 0 on a mesh without hanging nodes: box32) leave 160 bytes, less than 8 rows of 48.  The refusal
    names the fields and the budget, in every host-only check (hq_create_opts refuses with the same text: hq_patch_build)."""
    cfg = ST.patch_cfg(options, False)
    assert (6 * cfg["nlmax"] + 3 * (cfg["pmax"] + cfg["vmax"])) * 8 > ST.LDS_BUDGET and 8 <= cfg["nlmax"] < 16
    _refused(monkeypatch, "box32", options, "patch_pmax = %d" % options["patch_pmax"], "patch_vmax = %d" % options.get("patch_vmax", 0),
             "LDS budget of %d bytes" % ST.LDS_BUDGET)
    if "patch_vmax" not in options:                              # hanging nodes: the planner's own 384 accumulators count too
        _refused(monkeypatch, "two_level", options, "patch_pmax = %d" % options["patch_pmax"], "patch_vmax = 384", "LDS budget")


def test_the_largest_accumulators_that_leave_an_image_reach_the_planner(monkeypatch):
    """One step inside the budget: pmax = 6 800 leaves 640 bytes, an image of 13 rows; the loop stops at nlmax = 8 as it
    always did, and what refuses box32 then is the planner itself (no node of it fits 8 rows with its neighbours), in its own
    words and not in the budget's."""
    cfg = ST.patch_cfg(dict(patch_pmax=6800), False)
    assert (6 * cfg["nlmax"] + 3 * cfg["pmax"]) * 8 <= ST.LDS_BUDGET and cfg["nlmax"] == 8
    for msg in _refused(monkeypatch, "box32", dict(patch_pmax=6800)):
        assert "LDS budget" not in msg and "patch_pmax" not in msg, msg
