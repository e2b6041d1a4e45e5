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
rounds the state once).


At a hanging node the float term is (deps + 1) 2^-24 mean|ref(anchors)| instead: its value is the float mean of its anchors'
stored values (float_rounding below); measured there 0.38 x 2^-24 mean|ref(anchors)|, 31 times 2^-24 of its own value.

Worst |got - ref| / (2^-53 T) per kernel family on an MI355X (the bound is 64; 49 cases in 6.3 s, the slowest 1.1 s):
    hq_k_brick (default, brick_cz = 5, by component, per-node rows), both boxes          2.0 - 2.1
    hq_k_patch_stencil (subsets / full lattices), element lattice rows, patch_no_uniform  1.8 - 2.4
    hq_k_brick_het unpacked: het70x20x12 3.5 / 3.8 / 3.7 (rayleigh / mass / none), ragged c5_gradient_branch 3.6 / 4.1 / 3.4
    hq_k_brick_het<PACKED>:  het70x20x12 4.5 / 5.0 / 3.7,                          ragged c5_gradient_branch 4.2 / 4.9 / 3.4
    hq_k_patch_step, hq_k_patch_pers (w form and patch_wform = 0): het70x20x12 2.7, two_level 1.2 - 1.4
    hq_k_patch_seed, patch_no_iso / _ntsame / _dedup / _lattice: het70x20x12 5.3 (mass 6.1, none 5.8), two_level 3.0
    scatter: het70x20x12 2.6 - 2.7, two_level 1.2
    float state: 0.997 (brick) and 0.995 (unpacked het) of the f32 bound at plain nodes"""
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


CHECKS = {"brick": lambda: S._chk_brick, "brick_cz": lambda: S._chk_brick_cz, "bycomp": lambda: S._chk_bycomp,
          "pernode": lambda: S._chk_pernode, "stencil_all": lambda: S._chk_stencil_all, "stencil_full": lambda: S._chk_stencil_full,
          "no_stencil": lambda: S._chk_no_stencil, "scatter": lambda: S._chk_scatter, "het": _chk_het, "gradient": _chk_gradient,
          "patches": lambda kernel, opts: _chk_patches(kernel, **opts)}


def _case(mesh, check, damping="rayleigh", variant=PATCH, options=None, precision="f64", pack=False):
    return dict(mesh=mesh, check=check, damping=damping, variant=variant, options=options, precision=precision, pack=pack)


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


def make(c, p, nt, u1, u2):
    kw = dict(edata=p["edata"], material=p["material"]) if c["pack"] else {}
    return ha.Solver(p["lnid"], p["etable"], nt, p["dt"], tm1=u1, tm2=u2, dangling=p["dangling"], node_xyz=p["node_xyz"],
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
