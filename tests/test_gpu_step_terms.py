"""Damping and material terms per node: ONE step from two independent fields (tm1 = u1, tm2 = u2, run(1)), every kernel
form against an extended-precision restatement of the oracle's step, per node and component.  The reference side and the
planner's counters of these cases, without a device: tests/test_step_terms_cpu.py.

The seeded short runs of the suite start from tm2 close to tm1 and are held to 1e-9 of the field's maximum: the Rayleigh
fold w = u1 + beta (u1 - u2) then carries about 1e-3 of what is summed, and a relative error of 1e-4 in one element's beta,
one branch of the material expansion (hq_material_coef on the device: hq_k_brick_het<PACKED>) or one kernel form passes.
Here u1 and u2 are drawn independently (sign * uniform(0.5, 1) * 1e-3, tests/helpers.step_fields), so u1 - u2 is as large
as the fields and the m1 u2 term of the update (psolve.c:4072-4114) is independent of the m2 u1 term; the time step puts the
stiffest element at (Vp dt / h)^2 = 0.25; het70x20x12 and c5_gradient_branch carry materials of every branch of
mu_and_lambda and both sides of the zeta threshold in at least 10 % of the elements each (tests/helpers.branch_materials),
with Rayleigh, mass and no damping.

Reference: tests/helpers.extended_step (np.longdouble; ref = the new displacement, T = the same expression with every
product replaced by its absolute value).  Bound, per node and component:
    |got - ref| <= B * 2^-53 * T,   B = 16 * max(B_oracle, 4) = 64
B_oracle = the C oracle's own worst |oracle - ref| / (2^-53 T) on the same mesh and fields, computed with the reference
(reference() below) and pinned below 64 by tests/test_step_terms_cpu.py.  Measured:
    het70x20x12         rayleigh 2.97   mass 3.01   none 3.03      (float oracle, in 2^-24 T: rayleigh 2.92)
    c5_gradient_branch  rayleigh 2.95   mass 2.85   none 2.90
    box70x20x12 1.64    box32x32x16 1.68 (float 1.63)    box32 1.56    two_level 1.39 (float 1.36)
(all below 4, so B = 64 everywhere.)
The factor 16: the butterfly A D A^T and the plane-sum forms do up to about 4 times the oracle's operations on
intermediates up to 8 times the size of a term; packed units add their documented 1e-15 on m2, inside the bound.  An error
of one float ulp in zeta is 6e-8 of the damping share -- tests/test_step_terms_cpu.py shows that, a capped element given
its uncapped lambda and 1e-9 in one m1 tripping this bound at the nodes concerned only.
precision="f32": float32 n_t rows and fields, ref from the widened floats, bound 2^-24 |ref| + B 2^-53 T (the library
rounds the state once).  At a hanging node the float term is (deps + 1) 2^-24 mean|ref(anchors)| instead (float_rounding
below); measured there 0.38 x 2^-24 mean|ref(anchors)|, 31 times 2^-24 of its own value.

The float library per node (rounded_step below).  That additive bound is nearly all rounding of the state: every c1 of
het70x20x12 off by 1e-9 passes it (tests/test_step_terms_cpu.py).  But the float library rounds the state ONCE and every
sum inside a kernel is double, so what it must return is float32(double step), and that is held to the bit.  Every f64
key has an "f32-" twin (the same mesh, options, damping and CHECKS entry on float32 rows and fields) under
    lo = float32(ref - B 2^-53 T), hi = float32(ref + B 2^-53 T)      (round to nearest from np.longdouble; B as above)
    plain node, lo == hi    got == lo bit for bit (int32 views)
    plain node, lo != hi    "undetermined": got is one of the floats in [lo, hi]; at most 1 component in 10 000 per case
                            (UNDETERMINED_CAP: a condition on the inputs, which the reference side meets without a device)
    hanging node            got == float32(sum over its anchors, in list order, of float64(got[anchor]) / deps) bit for bit,
                            from the library's OWN anchors: the text of hq_k_adjust_assign; the double sum is exact
                            (asserted), so its order cannot matter, and the anchors are plain nodes
with the additive bound still asserted beside it.  A form that does not exist in the float build: a per-element unit packs
only if its n_t rows come back out of the two doubles {m0, m0 - m1} to 1e-15; rows rounded to float do so only without
damping (m1 = m0, m2 = 2 m0), so the "het-packed" and "het-ragged-packed" twins under Rayleigh and mass damping assert
from hq_info that hq_k_brick_het runs them UNPACKED (brick_units_packed == 0 with the same per-element units:
float_rows_pack, float_twin) and the twins without damping run hq_k_brick_het<PACKED> on a float state.
Measured on an MI355X, every f32 case (47 here, 16 in tests/test_gpu_brick_edges.py, 13 in tests/test_gpu_partition_step.py):
    mismatches 0; got != float32(ref) inside the band 0 -- every component of every kernel form is the correctly rounded
    reference itself;  undetermined 0 of 3 294 - 107 811 plain components per case here
(hq_k_brick default / brick_cz = 5 / by component / per-node rows on both boxes; hq_k_patch_stencil subsets, full lattices,
element lattice rows, patch_no_uniform; hq_k_brick_het unpacked on het70x20x12 and ragged c5_gradient_branch under all three
dampings, <PACKED> without damping; hq_k_patch_step, hq_k_patch_pers in the w form and with patch_wform = 0, hq_k_patch_seed
with patch_no_iso / _ntsame / _dedup / _lattice on het70x20x12 and two_level; scatter on both).

Worst |got - ref| / (2^-53 T) per kernel family on an MI355X (the bound is 64; 93 cases in 7.4 s of which the f32 ones
take 2.7 s, the slowest 1.1 s; 49 cases took 6.3 s before the f32 twins):
    hq_k_brick (default, brick_cz = 5, by component, per-node rows), both boxes          2.0 - 2.1
    hq_k_patch_stencil (subsets / full lattices), element lattice rows, patch_no_uniform  1.8 - 2.4
    hq_k_brick_het unpacked: het70x20x12 3.5 / 3.8 / 3.7 (rayleigh / mass / none), ragged c5_gradient_branch 3.6 / 4.1 / 3.4
    hq_k_brick_het<PACKED>:  het70x20x12 4.5 / 5.0 / 3.7,                          ragged c5_gradient_branch 4.2 / 4.9 / 3.4
    hq_k_patch_step, hq_k_patch_pers (w form and patch_wform = 0): het70x20x12 2.7, two_level 1.2 - 1.4
    hq_k_patch_seed, patch_no_iso / _ntsame / _dedup / _lattice: het70x20x12 5.3 (mass 6.1, none 5.8), two_level 3.0
    scatter: het70x20x12 2.6 - 2.7, two_level 1.2
    float state: 0.997 (brick) and 0.995 (unpacked het) of the f32 bound at plain nodes

Patch plans off the default geometry (GEOMETRY: hq_options.patch_threads / _pmax / _pmerge / _psplit / _nlmax / _vmax, each
with no_bricks = 1; 29 f64 keys "<geometry>-<mesh>" and their f32 twins; the plans without a device:
tests/test_patch_geometry_cpu.py).  Everything above runs the patch kernels at the planner's defaults (512 threads, pmax 768,
pmerge 512, nlmax 1024, vmax 384); the geometry decides what they index by -- the strided loops of hq_k_patch_step against 64
and 192 threads, the image size and o2off of the w form, hstride, the halving path, whether the persistent kernels take the
plan (nlmax <= 1024), thousands of 8-node patches in the work queue or fewer than the 8 XCD slots, hq_k_patch_stencil's shape
tables of 2 x 2 x 2 cubes, contexts without coordinates.  The criterion, reference, fields and bound are the ones above.  The
"geometry" check asserts on the context that npatches and patch_pairs are hq_plan_check's under the HQ_PATCH_* equivalents,
that the plan is not the default one, the kernel (hq_dominant_kernel names hq_k_patch_stencil where stencil patches are the
majority, so the kernel of the element-form patches is seen only where they are) and stencil_patches against
hq_stencil_plan_check's tables -- equal on box32 and two_level; 0 on het70x20x12 and c5_gradient_branch, where every element
has its own material, no patch has uniform coefficients and `tables` counts shapes alone (2 726 of them under pmax8).
Three settings the planner refuses (REFUSED) raise HqError at hq_create_opts, and a default context created next passes.
Finding: none in the kernels; every device plan was the host-only check's.  hq_patch_cfg_of's loop had no lower end (a
geometry whose accumulators alone exceed LDS was refused by accident, through an unsigned wrap-around): repaired, with a
refusal of its own.  Measured on an MI355X, worst |got - ref| / (2^-53 T), unloaded (loaded: tests/test_gpu_loaded_step.py):
    hq_k_patch_stencil on box32: pmax8, pmax27-pmerge1, pmax728, nlmax776 1.79; psplit100 (with element-form patches) 2.39
    hq_k_patch_step: big 1.29 (box32) / 1.38 (two_level) / 2.55 (c5_gradient_branch) / 2.65 (het70x20x12); threads64 and
      threads192 1.38 / 2.55; pmax8-step 1.56 (two_level) / 2.55
    hq_k_patch_seed: two_level pmax8 and nlmax72 1.88 (beside the stencil majority), vmax8 2.28, noxyz-pmerge100 2.98;
      c5_gradient_branch pmax8, pmax27-pmerge1, psplit100, pmax1016, vmax40, noxyz-pmerge37-pmax64 6.55;
      het70x20x12 pmax8, nlmax72, nlmax776, noxyz-pmerge100 5.30
    float twins, all 29: mismatches 0, undetermined 0, got != float32(ref) inside the band 0; 0.971 - 1.000 of the f32 bound
154 cases in 11.8 s with the geometry keys and the three refusals (61 more than the 93 in 7.4 s; alone they take 4.6 s, the
slowest pmax8-box32 1.4 s with its 4 880 patches planned twice, on the host and for the device, then pmax8-het70x20x12 0.6 s)."""
import functools

import numpy as np
import pytest

import hercules_amd as ha
from oracle import herc_oracle as ho
from tests import helpers as H
from tests import test_gpu_sources as S

if not np.finfo(np.longdouble).eps < 1e-18:
    pytest.skip("np.longdouble is no wider than double here (eps %.1e): no extended reference" % np.finfo(np.longdouble).eps,
                allow_module_level=True)

pytestmark = pytest.mark.gpu

PATCH, SCATTER = ha.HQ_VARIANT_PATCH, ha.HQ_VARIANT_SCATTER
EPS = 2.0 ** -53
SEED = 5150


def oracle_step(p, nt, u1, u2, etable=None):
    """The C oracle's new displacement from tm1 = u1, tm2 = u2 (ho.solver_run takes the newest array last), in nt's type."""
    o1, o2 = u2.copy(), u1.copy()
    ho.solver_run(p["lnid"], p["etable"] if etable is None else etable, np.ascontiguousarray(nt), o1, o2, 0, 1, p["dt"],
                  damping=p["kind"], dangling=p["dangling"])
    assert np.array_equal(o1, u1)
    return o2


@functools.lru_cache(maxsize=None)
def reference(mesh, damping="rayleigh", precision="f64"):
    """(ntable, u1, u2, ref, T, B_oracle) of a mesh, damping kind and precision: computed once, shared read-only among the
    cases.  B_oracle: the C oracle of that precision against ref, in units of 2^-53 T (float: 2^-24 T)."""
    p = H.step_mesh(mesh, damping)
    real = np.float32 if precision == "f32" else np.float64
    nt = np.ascontiguousarray(p["ntable"], real)
    u1, u2 = H.step_fields(p["N"], SEED, p["dangling"], real)
    ref, T = H.extended_step(p["lnid"], p["etable"], nt, u1, u2, p["dangling"])
    b = float((np.abs(oracle_step(p, nt, u1, u2) - ref) / ((2.0 ** -24 if precision == "f32" else EPS) * T)).max())
    for a in (nt, u1, u2, ref, T):
        a.flags.writeable = False
    return nt, u1, u2, ref, T, b


def bound_factor(mesh, damping):
    """B = 16 * max(B_oracle, 4), B_oracle of the double oracle on that mesh."""
    b = reference(mesh, damping)[5]
    assert b <= 64.0, b                                          # (a broken reference cannot inflate the bar)
    return 16.0 * max(b, 4.0)


# ---------------------------------------------------------------------------------------------
# the counters that say the kernel form is there: a case's check = (kind, arguments), evaluated on its context
# ---------------------------------------------------------------------------------------------
def _chk_het(packed):
    def chk(s, p, name):
        info = s.info()
        assert s.dominant_kernel() == "hq_k_brick" and 2 * info["brick_nodes"] > p["N"], info
        assert info["brick_units_het"] == info["brick_units"] > 0 and info["brick_units_ragged"] == 0, info
        assert info["brick_units_packed"] == (info["brick_units_het"] if packed else 0), info
    return chk


def _chk_gradient(pack):
    def chk(s, p, name):
        info = s.info()
        assert info["brick_units_ragged_het"] >= 2 and info["brick_units_het"] >= info["brick_units_ragged_het"], info
        assert (info["brick_units_packed"] > 0) == bool(pack), info
    return chk


def _chk_patches(kernel, **opts):
    """Patches only, element-form ones among them, the kernel that runs them, the options as resolved."""
    def chk(s, p, name):
        info, o = s.info(), s.options()
        assert info["brick_nodes"] == 0 and s.dominant_kernel() == kernel, (s.dominant_kernel(), info)
        assert info["npatches"] > info["stencil_patches"], info
        for k, v in opts.items():
            assert o[k] == v, (k, o[k])
        if opts.get("patch_no_lattice"):
            assert info["lattice_patches"] == 0, info
        if opts.get("patch_no_uniform"):
            assert info["stencil_patches"] == 0, info            # a stencil patch is a uniform one
    return chk


# ---------------------------------------------------------------------------------------------
# patch plans off the default geometry (the planner's defaults: 512 threads, pmax 768, pmerge 512, nlmax 1024, vmax 384)
# ---------------------------------------------------------------------------------------------
GEOMETRY = {
    "threads64": dict(patch_pipe=0, patch_threads=64), "threads192": dict(patch_pipe=0, patch_threads=192),
    "pmax8": dict(patch_pmax=8), "pmax8-step": dict(patch_pmax=8, patch_pipe=0, patch_threads=64),
    "pmax27-pmerge1": dict(patch_pmax=27, patch_pmerge=1), "nlmax72": dict(patch_pmax=64, patch_nlmax=72),
    "psplit100": dict(patch_pmax=343, patch_psplit=100), "pmax728": dict(patch_pmax=728), "nlmax776": dict(patch_nlmax=776),
    "pmax1016": dict(patch_pmax=1016, patch_nlmax=1024), "big": dict(patch_pmax=1500, patch_nlmax=2400),
    "vmax8": dict(patch_vmax=8), "vmax16": dict(patch_vmax=16), "vmax40": dict(patch_vmax=40),
    "noxyz-pmerge100": dict(patch_pmerge=100), "noxyz-pmerge37-pmax64": dict(patch_pmerge=37, patch_pmax=64),
}
GEOMETRY_MESHES = {                                              # het70x20x12: Rayleigh only (the damping kinds are covered at the default geometry)
    "box32": ("pmax8", "pmax27-pmerge1", "psplit100", "pmax728", "nlmax776", "big"),
    "two_level": ("threads64", "threads192", "pmax8", "pmax8-step", "nlmax72", "big", "vmax8", "noxyz-pmerge100"),
    "c5_gradient_branch": ("threads64", "threads192", "pmax8", "pmax8-step", "pmax27-pmerge1", "psplit100", "pmax1016", "big", "vmax40",
                           "noxyz-pmerge37-pmax64"),
    "het70x20x12": ("pmax8", "nlmax72", "nlmax776", "big", "noxyz-pmerge100"),
}
GEOMETRY_PAIRS = [(m, g) for m, gs in GEOMETRY_MESHES.items() for g in gs]
# settings the planner refuses: one node's neighbours (the hanging-node accumulators among them) do not fit what is left
REFUSED = [("two_level", dict(patch_vmax=1)), ("c5_gradient_branch", dict(patch_vmax=8)),
           ("c5_gradient_branch", dict(patch_pmax=64, patch_nlmax=72))]
REFUSAL = "a single node reaches more neighbours than LDS can stage"
_GEOMETRY_FIELDS = ("patch_pipe", "patch_threads", "patch_pmax", "patch_pmerge", "patch_psplit", "patch_nlmax", "patch_vmax")
HQ_PERS_THREADS, HQ_LAT_ACC, LDS_BUDGET = 1024, 729, 160 * 1024  # hq_patch.h


def geometry_has_xyz(g):
    return not g.startswith("noxyz")


def patch_cfg(options, hanging):
    """hq_patch_cfg_of restated: the geometry the planner works with, out of the options (-1 or absent = the default)."""
    o = {k: v for k, v in (options or {}).items() if v != -1}
    threads = (min(max(o.get("patch_threads", 512), 64), 1024)) & ~63
    pmax = max(o.get("patch_pmax", 768), 8)
    pmerge = max(min(o.get("patch_pmerge", 512), pmax), 1)
    psplit = o.get("patch_psplit", 0)
    psplit = pmax if psplit > pmax or psplit < 8 else psplit
    nlmax = min(max(o.get("patch_nlmax", 1024), pmax + 8), 0x7fff)
    vmax = o.get("patch_vmax", 0)
    if hanging and vmax == 0:
        vmax = 384
    while (6 * nlmax + 3 * (pmax + vmax)) * 8 > LDS_BUDGET and nlmax >= 16:
        nlmax -= 8
    return dict(threads=threads, pmax=pmax, pmerge=pmerge, psplit=psplit, nlmax=nlmax, vmax=vmax, pipe=o.get("patch_pipe", 6))


def steps_per_patch(options, hanging):
    """hq_patch_uses_pers, as far as the options decide it: hq_k_patch_step runs the element-form patches where patch_pipe
    is 0 or the image exceeds the persistent kernels' 1024 rows (a patch of more than 1024 elements or an LDS budget
    exceeded would also send a plan there: the geometries here keep pmax + vmax far below the 2 718 at which 12 x 1024 rows
    and the accumulators no longer fit)."""
    cfg = patch_cfg(options, hanging)
    assert cfg["nlmax"] > HQ_PERS_THREADS or (12 * max(cfg["nlmax"], 1000) + 3 * (cfg["pmax"] + cfg["vmax"]) + 36) * 8 <= LDS_BUDGET, cfg
    return cfg["pipe"] not in (4, 6) or cfg["nlmax"] > HQ_PERS_THREADS


def plan_environment(mp, options):
    """The HQ_PATCH_* equivalents of a case's geometry on a pytest.MonkeyPatch: hq_plan_check and its kin take no options
    and read the environment (HQ_ALLOW_ENV = 1, tests/conftest.py).  Every geometry variable the case does not name is unset."""
    for k in _GEOMETRY_FIELDS:
        mp.delenv("HQ_" + k.upper(), raising=False)
    for k, v in (options or {}).items():
        if k in _GEOMETRY_FIELDS:
            mp.setenv("HQ_" + k.upper(), str(v))


@functools.lru_cache(maxsize=None)
def host_plans(mesh, damping, g):
    """The host-only checks of a step_mesh under the geometry g (a GEOMETRY key, or None = the defaults) -> (hq_plan_check's
    report, hq_stencil_plan_check's or None without coordinates).  They plan what hq_create plans under no_bricks = 1."""
    from hercules_amd import capi
    p = H.step_mesh(mesh, damping)
    xyz = g is None or geometry_has_xyz(g)
    with pytest.MonkeyPatch.context() as mp:
        plan_environment(mp, GEOMETRY[g] if g else {})
        d = H.solver_desc(p if xyz else dict(p, node_xyz=None))
        return capi.plan_check(d), (capi.stencil_plan_check(d) if xyz else None)


def single_element_nodes(p):
    """The nodes of a mesh that lie in exactly one element (the corners of the domain, and hanging nodes on its edges)."""
    return int((np.bincount(np.asarray(p["lnid"]).ravel(), minlength=p["N"]) == 1).sum())


def _chk_geometry(g):
    """The plan on the device is the one the host-only check reports, it is not the default plan, and the kernel and the
    counter the geometry is about.  hq_dominant_kernel names hq_k_patch_stencil where more than half the patches are stencil
    patches, else the kernel of the element-form ones: hq_k_patch_step where steps_per_patch() says so, else
    hq_k_patch_seed.  A stencil patch needs a lattice-subset shape table AND one (c1, c2, beta) for all its elements:
    hq_stencil_plan_check's `tables` counts the shapes whatever the coefficients, so stencil_patches == tables holds where a
    level has one material (box32, two_level); with a material of its own in every element (branch_materials:
    het70x20x12, c5_gradient_branch, no two eTable rows equal) only a patch of ONE element can be one, and the nodes of such
    a patch lie in no other element."""
    opts, xyz = GEOMETRY[g], geometry_has_xyz(g)

    def chk(s, p, name):
        info, o = s.info(), s.options()
        assert info["brick_nodes"] == 0 and o["no_bricks"] == 1, info
        for k, v in opts.items():
            assert o[k] == v, (k, o[k], v)
        plan, st = host_plans(name, p["damping"], g)
        default = host_plans(name, p["damping"], None)[0]
        assert plan["faults"] == 0 and (st is None or st["faults"] == 0), (plan, st)
        print("\n[geometry] %-24s %-20s device: patches %d pairs %d lattice %d stencil %d ragged %d %s | host: patches %d pairs %d lattice %d tables %s | default %d"
              % (g, name, info["npatches"], info["patch_pairs"], info["lattice_patches"], info["stencil_patches"], info["ragged_patches"],
                 s.dominant_kernel(), plan["patches"], plan["pairs"], plan["lattice_patches"], st and st["tables"], default["patches"]))
        assert (info["npatches"], info["patch_pairs"]) == (plan["patches"], plan["pairs"]), (info, plan)
        if (name, g) == ("box32", "pmax728"):                     # one below HQ_LAT_ACC: no lattice rows, stencil tables still made
            assert info["lattice_patches"] == 0 < info["stencil_patches"] and default["lattice_patches"] > 0, (info, default)
        elif g == "pmax1016":                                    # the same cubes, merged otherwise: the pairs differ
            assert info["patch_pairs"] != default["pairs"], (info, default)
        elif g.startswith("threads"):                            # the workgroup changes (asserted above), the plan is the default one
            assert (info["npatches"], info["patch_pairs"]) == (default["patches"], default["pairs"]), (info, default)
        else:
            assert info["npatches"] != default["patches"], (info, default)
        element = "hq_k_patch_step" if steps_per_patch(opts, p["dangling"] is not None and len(p["dangling"][0]) > 0) else "hq_k_patch_seed"
        kernel = "hq_k_patch_stencil" if 2 * info["stencil_patches"] > info["npatches"] else element
        assert s.dominant_kernel() == kernel, (s.dominant_kernel(), kernel, info)
        if (name, g) == ("box32", "big"):                        # an image over 1024 rows: no persistent kernel, no stencil patch
            assert info["stencil_patches"] == st["tables"] == 0 and s.dominant_kernel() == "hq_k_patch_step", (info, st)
        elif name == "box32" and g in ("pmax8", "pmax27-pmerge1", "pmax728", "nlmax776"):
            assert info["stencil_patches"] == info["npatches"] == st["tables"] and s.dominant_kernel() == "hq_k_patch_stencil", (info, st)
        elif not xyz:                                            # no coordinates: no lattice, no stencil
            assert info["stencil_patches"] == info["lattice_patches"] == 0, info
        elif "labels" in p:
            assert len(np.unique(p["etable"][:, :3], axis=0)) == p["E"]
            assert info["stencil_patches"] <= min(st["tables"], single_element_nodes(p)), (info, st)
            assert info["npatches"] > info["stencil_patches"] and s.dominant_kernel() == element, info
        else:                                                    # (hq_k_patch_stencil has launches of its own, whatever steps the others)
            assert info["stencil_patches"] == st["tables"], (info, st)
    return chk


CHECKS = {"geometry": _chk_geometry,
          "brick": lambda: S._chk_brick, "brick_cz": lambda: S._chk_brick_cz, "bycomp": lambda: S._chk_bycomp,
          "pernode": lambda: S._chk_pernode, "stencil_all": lambda: S._chk_stencil_all, "stencil_full": lambda: S._chk_stencil_full,
          "no_stencil": lambda: S._chk_no_stencil, "scatter": lambda: S._chk_scatter, "het": _chk_het, "gradient": _chk_gradient,
          "patches": lambda kernel, opts: _chk_patches(kernel, **opts)}


def _case(mesh, check, damping="rayleigh", variant=PATCH, options=None, precision="f64", pack=False, xyz=True):
    """xyz = False: the context is created without node coordinates (hq_desc.node_xyz = NULL)."""
    return dict(mesh=mesh, check=check, damping=damping, variant=variant, options=options, precision=precision, pack=pack, xyz=xyz)


DAMPINGS = ("rayleigh", "mass", "none")
NB = {"no_bricks": 1}
CASES = {}
for _b in ("box70x20x12", "box32x32x16"):
    CASES["brick-" + _b] = _case(_b, ("brick",))
    CASES["brick-cz5-" + _b] = _case(_b, ("brick_cz",), options={"brick_cz": 5})
    CASES["brick-bycomp-" + _b] = _case(_b, ("bycomp",), options={"brick_by_component": 1})
    CASES["brick-pernode-" + _b] = _case(_b, ("pernode",), options={"brick_no_ntsame": 1})
CASES.update({
    "stencil-subsets-box32": _case("box32", ("stencil_all",), options=dict(NB, patch_ragged=1)),
    "stencil-full-box32": _case("box32", ("stencil_full",), options=dict(NB, patch_ragged=0)),
    "element-lattice-rows-box32": _case("box32", ("no_stencil",), options=dict(NB, patch_no_stencil=1)),
    "no-uniform-box32": _case("box32", ("patches", "hq_k_patch_seed", dict(patch_no_uniform=1)), options=dict(NB, patch_no_uniform=1)),
})
for _d in DAMPINGS:
    CASES["het-packed-het70x20x12-" + _d] = _case("het70x20x12", ("het", True), _d, pack=True)
    CASES["het-het70x20x12-" + _d] = _case("het70x20x12", ("het", False), _d, options={"brick_no_pack": 1}, pack=True)
    CASES["het-ragged-packed-c5_gradient_branch-" + _d] = _case("c5_gradient_branch", ("gradient", 1), _d, options=H.RAGGED_PLAN, pack=True)
    CASES["het-ragged-c5_gradient_branch-" + _d] = _case("c5_gradient_branch", ("gradient", 0), _d, options=H.RAGGED_PLAN)
    CASES["scatter-het70x20x12-" + _d] = _case("het70x20x12", ("scatter",), _d, variant=SCATTER)
    if _d != "rayleigh":
        CASES["patch_seed-het70x20x12-" + _d] = _case("het70x20x12", ("patches", "hq_k_patch_seed", dict(patch_pipe=6)), _d,
                                                      options=dict(NB, patch_pipe=6))
CASES["scatter-two_level"] = _case("two_level", ("scatter",), variant=SCATTER)
for _m in ("het70x20x12", "two_level"):
    for _k, _kernel, _o in (("patch_step", "hq_k_patch_step", {"patch_pipe": 0}), ("patch_pers", "hq_k_patch_pers", {"patch_pipe": 4}),
                            ("patch_seed", "hq_k_patch_seed", {"patch_pipe": 6}),
                            ("patch_pers-u1u2", "hq_k_patch_pers", {"patch_pipe": 4, "patch_wform": 0}),
                            ("no-iso", "hq_k_patch_seed", {"patch_no_iso": 1}), ("no-ntsame", "hq_k_patch_seed", {"patch_no_ntsame": 1}),
                            ("no-dedup", "hq_k_patch_seed", {"patch_no_dedup": 1}), ("no-lattice", "hq_k_patch_seed", {"patch_no_lattice": 1})):
        CASES["%s-%s" % (_k, _m)] = _case(_m, ("patches", _kernel, dict(_o)), options=dict(NB, **_o))
CASES.update({
    "f32-brick-box32x32x16": _case("box32x32x16", ("brick",), precision="f32"),
    "f32-het-het70x20x12": _case("het70x20x12", ("het", False), options={"brick_no_pack": 1}, pack=True, precision="f32"),
    "f32-patch_seed-two_level": _case("two_level", ("patches", "hq_k_patch_seed", dict(patch_pipe=6)), options=dict(NB, patch_pipe=6),
                                      precision="f32"),
})
for _m, _g in GEOMETRY_PAIRS:                                    # "<geometry>-<mesh>": no_bricks = 1 on top of the geometry's fields
    CASES["%s-%s" % (_g, _m)] = _case(_m, ("geometry", _g), options=dict(NB, **GEOMETRY[_g]), xyz=geometry_has_xyz(_g))


def float_rows_pack(damping):
    """Whether per-element units can pack when the n_t rows arrive as floats.  The planner packs a unit only if every
    owned row comes back out of the two doubles {m0, m0 - m1}: m1 exactly and m2 = 2 m0 - (m0 - m1) to 1e-15.  Rows rounded
    to float keep that relation only where it is exact to begin with: without damping m1 = m0 and m2 = 2 m0 (a power of
    two times the same float).  With Rayleigh or mass damping m2 and 2 m0 - m1 differ by the rows' float rounding, about
    6e-8, at every node, so hq_k_brick_het runs unpacked there -- the form does not exist in the float build."""
    return damping == "none"


def float_twin(c):
    """The f32 twin of an f64 case: the same mesh, options, damping and CHECKS entry on float32 n_t rows and fields.  A
    check that expects packed units expects them only where float rows can pack; elsewhere it asserts from hq_info that
    the unpacked form runs instead (brick_units_packed == 0 with the same per-element units)."""
    check = c["check"]
    if check[0] in ("het", "gradient") and check[1] and not float_rows_pack(c["damping"]):
        check = (check[0], type(check[1])(0))
    return dict(c, precision="f32", check=check)


# every f64 key has an f32- twin (two of the three older f32 cases carry their twin's name already; "f32-het-het70x20x12"
# keeps its own and equals "f32-het-het70x20x12-rayleigh")
for _k in [k for k, c in CASES.items() if c["precision"] == "f64"]:
    CASES["f32-" + _k] = float_twin(CASES[_k])


def make(c, p, nt, u1, u2):
    kw = dict(edata=p["edata"], material=p["material"]) if c["pack"] else {}
    return ha.Solver(p["lnid"], p["etable"], nt, p["dt"], tm1=u1, tm2=u2, dangling=p["dangling"], node_xyz=p["node_xyz"] if c["xyz"] else None,
                     variant=c["variant"], options=c["options"], precision=c["precision"], **kw)


def float_rounding(ref, dangling):
    """The state's rounding in a float run, per node and component: 2^-24 |ref| where the update is rounded once.  A
    hanging node is the mean of its anchors' STORED values, summed in float as compute_adjust does it (psolve.c:5936-6039):
    the anchors' own rounding, one rounding per quotient and one per partial sum, (deps + 1) 2^-24 mean|ref(anchors)|,
    whatever cancels in the mean."""
    r = 2.0 ** -24 * np.abs(ref)
    if dangling is not None and len(dangling[0]):
        ids, ptr, anc = [np.asarray(a, np.int64) for a in dangling]
        deps = np.diff(ptr)
        mean = np.zeros((len(ids), 3), np.longdouble)
        np.add.at(mean, np.repeat(np.arange(len(ids)), deps), np.abs(ref[anc]) / np.repeat(deps, deps)[:, None])
        r[ids] = 2.0 ** -24 * (deps + 1)[:, None] * mean
    return r


def worst(got, ref, T, B, f32=False, dangling=None):
    """(largest |got - ref| / bound, its node, its component, the same figure in units of 2^-53 T)."""
    err = np.abs(got.astype(np.longdouble) - ref)
    bound = B * EPS * T + (float_rounding(ref, dangling) if f32 else 0.0)
    q = (err / bound).astype(np.float64)
    n, d = np.unravel_index(np.argmax(q), q.shape)
    return float(q[n, d]), int(n), int(d), float((err / (EPS * T)).max())


# ---------------------------------------------------------------------------------------------
# the float library: one step is float32(double step), per node and component
# ---------------------------------------------------------------------------------------------
UNDETERMINED_CAP = 1e-4                                          # of a case's plain components: a condition, not a measurement


def _ordered(x):
    """float32 -> int64 that counts floats in order (the distance of two of them is their distance in ulps)."""
    i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def hanging_assignment(got, dangling):
    """hq_k_adjust_assign restated on the library's OWN output: per hanging node the anchors' stored floats widened,
    each divided by deps, summed in double in list order, rounded once.  -> (ids, expected float32 [n, 3], exact): exact
    says that the double sum equals the same sum in np.longdouble in either order, so the order cannot matter."""
    ids, ptr, anc = [np.asarray(a, np.int64) for a in dangling]
    deps = np.diff(ptr)
    s = np.zeros((len(ids), 3), np.float64)
    fwd, bwd = np.zeros((len(ids), 3), np.longdouble), np.zeros((len(ids), 3), np.longdouble)
    for j in range(int(deps.max()) if len(ids) else 0):
        sel = np.nonzero(j < deps)[0]
        s[sel] += got[anc[ptr[sel] + j]].astype(np.float64) / deps[sel, None].astype(np.float64)
        fwd[sel] += got[anc[ptr[sel] + j]].astype(np.longdouble) / deps[sel, None].astype(np.longdouble)
        bwd[sel] += got[anc[ptr[sel + 1] - 1 - j]].astype(np.longdouble) / deps[sel, None].astype(np.longdouble)
    exact = bool(np.array_equal(s.astype(np.longdouble), fwd) and np.array_equal(fwd, bwd))
    return ids, s.astype(np.float32), exact


def rounded_step(got, ref, T, B, dangling=None, nodes=None):
    """The float library rounds the state ONCE and sums in double: what it returns is float32(double step).  With
    lo = float32(ref - B 2^-53 T) and hi = float32(ref + B 2^-53 T), both rounded to nearest from np.longdouble:
      plain node, lo == hi    got equals it bit for bit                                           (else a mismatch)
      plain node, lo != hi    "undetermined": got is one of the floats in [lo, hi]                (else a mismatch); counted
      hanging node            got == hanging_assignment() of got's own anchors, bit for bit       (else a mismatch)
    nodes: a mask of the nodes that count (a rank's copies among a global field); None = all.
    -> dict(mismatches, undetermined, plain = the plain components counted, share = undetermined / plain,
            off_centre = plain components with got != float32(ref) (inside the band then, unless they are mismatches),
            hanging_exact, first = None or (node, component, "plain" / "hanging", got, expected = float32(ref) or the
            assignment, their distance in float ulps, lo, hi))."""
    assert got.dtype == np.float32 and got.shape == ref.shape
    L = np.longdouble
    half = L(B) * L(EPS) * T
    lo, hi, mid = (ref - half).astype(np.float32), (ref + half).astype(np.float32), ref.astype(np.float32)
    bits = lambda a: np.ascontiguousarray(a).view(np.int32)
    count = np.ones(len(got), bool) if nodes is None else np.asarray(nodes, bool).copy()
    plain = count.copy()
    expected, exact = mid.copy(), True
    bad = np.zeros(got.shape, bool)
    if dangling is not None and len(dangling[0]):
        ids, want, exact = hanging_assignment(got, dangling)
        plain[ids] = False
        expected[ids] = want
        bad[ids] = (bits(got[ids]) != bits(want)) & count[ids, None]
    determined = bits(lo) == bits(hi)
    ok = np.where(determined, bits(got) == bits(lo), (got >= lo) & (got <= hi))
    bad |= ~ok & plain[:, None]
    undetermined = int((~determined & plain[:, None]).sum())
    nplain = 3 * int(plain.sum())
    first = None
    if bad.any():
        n, d = [int(v) for v in np.argwhere(bad)[0]]
        first = (n, d, "plain" if plain[n] else "hanging", float(got[n, d]), float(expected[n, d]),
                 abs(int(_ordered(got[n, d:d + 1])[0]) - int(_ordered(expected[n, d:d + 1])[0])), float(lo[n, d]), float(hi[n, d]))
    return dict(mismatches=int(bad.sum()), undetermined=undetermined, plain=nplain, share=undetermined / max(nplain, 1),
                off_centre=int(((bits(got) != bits(mid)) & plain[:, None]).sum()), hanging_exact=exact, first=first)


def assert_rounded_step(case, r, family, branches=None):
    """0 mismatches and the cap, with a message that names the node, the figures, the kernel family and the branches."""
    f = r["first"]
    assert r["mismatches"] == 0, (
        "%s: %d components are not float32(double step); the first: %s node %d component %d got %.9g expected %.9g (%d float ulps "
        "apart; band [%.9g, %.9g]); kernel family %s; branch_of %s" % ((case, r["mismatches"], f[2], f[0], f[1]) + f[3:] + (family, branches)))
    assert r["hanging_exact"], (case, "the double sum of a hanging node's anchors is not exact: its order would matter")
    assert r["undetermined"] <= UNDETERMINED_CAP * r["plain"], (case, r["undetermined"], r["plain"])


def float_model(p, nt, u1, u2, etable=None):
    """The stand-in for the float library on a machine without a device: the DOUBLE C oracle on the widened float n_t rows
    and fields (`dangling` given), rounded once to float32; then hq_k_adjust_assign's text on the rounded state (a hanging
    node is the rounded double mean of its anchors' STORED floats -- so for the model the hanging rule checks only the
    sum's exactness; the anchors are plain nodes under the first two rules)."""
    wide = lambda a: np.ascontiguousarray(a, np.float64)
    out = oracle_step(p, wide(nt), wide(u1), wide(u2), etable).astype(np.float32)
    if p["dangling"] is not None and len(p["dangling"][0]):
        ids, want, _ = hanging_assignment(out, p["dangling"])
        out[ids] = want
    return out


def additive_bound_trips(got, ref, T, B, dangling):
    """The components over 2^-24 |ref| + B 2^-53 T (hanging nodes: float_rounding): the f32 bound that worst() asserts."""
    return int((np.abs(got.astype(np.longdouble) - ref) > B * EPS * T + float_rounding(ref, dangling)).sum())


def family_of(s):
    """The kernel family of a context from its counters, for a failure's message."""
    info = s.info()
    return (s.dominant_kernel(),) + tuple("%s=%d" % (k, info[k]) for k in ("brick_units", "brick_units_het", "brick_units_packed",
                                                                          "brick_units_ragged_het", "npatches", "stencil_patches"))


def branch_of(p, node):
    """The branch labels of the elements around a node (meshes with branch_materials), for a failure's message."""
    if "labels" not in p:
        return None
    elems = np.nonzero((np.asarray(p["lnid"]) == node).any(axis=1))[0]
    return {int(e): [k for k in H.BRANCHES if p["labels"][k][e]] for e in elems}


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_one_step_from_independent_fields(case):
    c = CASES[case]
    p = H.step_mesh(c["mesh"], c["damping"])
    f32 = c["precision"] == "f32"
    nt, u1, u2, ref, T, _ = reference(c["mesh"], c["damping"], c["precision"])
    B = bound_factor(c["mesh"], c["damping"])
    s = make(c, p, nt, u1, u2)
    try:
        assert s.info()["variant"] == c["variant"]
        CHECKS[c["check"][0]](*c["check"][1:])(s, p, c["mesh"])
        family = family_of(s)
        s.run(1)
        got, old = s.download()
        nonfinite = s.check_finite()
    finally:
        s.close()
    assert nonfinite == 0 and np.isfinite(got).all()
    assert got.dtype == (np.float32 if f32 else np.float64)
    w = worst(got, ref, T, B, f32, p["dangling"])
    print("\n[step-terms] %-48s %-8s nodes %6d worst %.3f of the bound (node %d.%d) = %.2f x 2^-53 T%s"
          % (case, c["damping"], p["N"], w[0], w[1], w[2], w[3], " (f32: mostly the state's rounding)" if f32 else ""))
    assert w[0] <= 1.0, (w, got[w[1]], np.asarray(ref[w[1]], np.float64), branch_of(p, w[1]))
    if f32:
        r = rounded_step(got, ref, T, B, p["dangling"])
        print("[step-terms] %-48s float32(double step): mismatches %d, undetermined %d of %d, got != float32(ref) inside the band %d; %s"
              % (case, r["mismatches"], r["undetermined"], r["plain"], r["off_centre"], family[0]))
        assert_rounded_step(case, r, family, branch_of(p, r["first"][0]) if r["first"] else None)


@pytest.mark.parametrize("mesh,options", REFUSED, ids=["%s-%s" % (m, "-".join("%s%d" % (k[6:], v) for k, v in o.items())) for m, o in REFUSED])
def test_a_refused_geometry_leaves_the_next_context_whole(mesh, options):
    """A geometry the planner cannot serve is refused at hq_create_opts with HQ_ERR_ARG and its message (never stepped
    wrongly); a default-geometry context of the same mesh created next in the same process passes its per-node step."""
    p = H.step_mesh(mesh)
    nt, u1, u2, ref, T, _ = reference(mesh)
    B = bound_factor(mesh, "rayleigh")
    with pytest.raises(ha.HqError, match=r"hq error -1: .*" + REFUSAL):
        make(_case(mesh, None, options=dict(NB, **options)), p, nt, u1, u2).close()
    s = make(_case(mesh, None, options=dict(NB)), p, nt, u1, u2)
    try:
        info = s.info()
        assert info["brick_nodes"] == 0 and info["npatches"] == host_plans(mesh, "rayleigh", None)[0]["patches"], info
        s.run(1)
        got, _ = s.download()
        nonfinite = s.check_finite()
    finally:
        s.close()
    w = worst(got, ref, T, B)
    print("\n[step-terms] refused %s on %s, then the defaults: worst %.3f of the bound = %.2f x 2^-53 T" % (options, mesh, w[0], w[3]))
    assert nonfinite == 0 and w[0] <= 1.0, w
