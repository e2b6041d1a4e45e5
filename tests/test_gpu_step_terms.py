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
