"""Halo exchange per node: ONE step from two independent fields (tm1 = u1, tm2 = u2) on PARTITIONS -- contexts linked in one
process (capi.group_link / group_run(solvers, 1)) and ranks in processes of their own -- every harbored copy of every rank
against an extended-precision restatement of the oracle's step on the global mesh, per node and component.  The reference
side, the coverage conditions and the mutations that show the check has teeth, without a device:
tests/test_partition_step_cpu.py.

What a partitioned step adds to tests/test_gpu_step_terms.py is arithmetic of its own: hq_k_interface_update is the only
place an owned interface node gets (f + m2 u1 - m1 u2) / m0, from the patch kernels' partial force in its d_iforce slot plus
the sharers' records (found through fcv, the ptr -> pos loop where a node has several sharers), rounded once and stored into
the peers' buffers or the packed send buffer; the patch kernels' interface form; hq_k_distribute on d_iforce for hanging
nodes that other ranks share; the routes the records travel.  The seeded 20-step partition tests start from tm2 close to
tm1 and hold 1e-9 of the field's maximum: a relative error of 1e-9 in one interface node's m1 is 1e-12 there
(tests/test_partition_step_cpu.py shows it passing that criterion and tripping this one at that node alone).

Problems (tests/helpers.partition_step_problem: ho.octree_partition + ho.multi_rank_init on the raw material rows at
tests/helpers.step_mesh's dt; fields tests/helpers.step_fields): c5_gradient_branch on 8 and 5 ranks (every branch of
mu_and_lambda on every rank, hanging nodes with anchors on other ranks, up to 4 sharers of a node, 308 dn s-records on 8
ranks), two_level on 5, het70x20x12 on 3 (per-element material on plane partition boundaries), and the C host's own
partitions of a uniform box at dt = 0.5 h / Vp (host.Box; the reference is assembled from the boxes' own tables): 32 x 16 x
16 on 2 and 8 ranks, the smallest box on which the planner's host-only check reports brick nodes on every rank.  Behind
bricks the shell's patches are element-form ones: no box from 32 x 16 x 16 to 64 x 64 x 32 has a stencil patch then
(hq_info.stencil_patches = 0 on every rank of 32 x 16 x 16, 32 x 32 x 16, 32^3, 64 x 32 x 32 and 64 x 64 x 32, on 2 and on 8
ranks, on an MI355X), so hq_k_patch_stencil's launch ahead of the exchange has cases of its own with no_bricks = 1: 32 x 32 x
16 on 2 ranks and 32^3 on 8, where every rank has lattice-subset patches and a rank that owns interface nodes has no others.

Reference: tests/helpers.extended_step (np.longdouble) on the global mesh with the global eTable assembled by element and
the global n_t assembled from the OWNERS' rows (the mass exchange sums in another order than a single rank does).  Bound,
per node and component, for every copy on every rank:
    |got - ref[gid]| <= B * 2^-53 * T[gid],   B = 16 * max(B_oracle, 4) = 64
B_oracle = the worst |ho.multi_rank_run's single step - ref| / (2^-53 T) over all ranks' copies (boxes: the C oracle's
single-rank step on the assembled tables), pinned below 64 by tests/test_partition_step_cpu.py.  Measured:
    c5_gradient_branch  8 ranks: rayleigh 2.95  mass 2.85  none 2.90  (float, of 2^-24 T: 2.97)    5 ranks: rayleigh 2.95 (float 2.97)
    two_level           5 ranks: 1.41 (float 1.38)
    het70x20x12         3 ranks: rayleigh 2.97  mass 3.01  none 3.03
    box 32x16x16        2 and 8 ranks: 1.48 (float 1.64)    box 32x32x16 2 ranks 1.63    box 32x32x32 8 ranks 1.76
(all below 4, so B = 64 everywhere.)  The factor 16 of tests/test_gpu_step_terms.py carries over: the interface sum adds
at most (sharers) additions -- 4 here -- of terms that T already counts, so nothing is widened.
precision="f32": bound 2^-24 |ref| + B 2^-53 T, at hanging nodes test_gpu_step_terms.float_rounding -- and beside it
test_gpu_step_terms.rounded_step: one step of the float library is float32(double step) bit for bit (undetermined
components, whose band straddles a float rounding boundary, at most 1 in 10 000), for every copy on every rank:
hq_k_interface_update rounds once, and a hanging node whose anchors live elsewhere still equals the rounded double mean of
the anchors' stored values as that rank holds them.  It is evaluated on the first copy of every global node; every other
copy equals it bit for bit (asserted first).  Float twins: c5_gradient_branch on 8 (patch_seed, patch_step, patch_pers in
the w form and with patch_wform = 0, scatter), two_level on 5, het70x20x12 on 3 (Rayleigh: float n_t rows do not pack --
test_gpu_step_terms.float_rows_pack -- so hq_info must say brick_units_packed == 0, with and without brick_no_pack; no
damping: hq_k_brick_het<PACKED> on a float state), the brick box on 2, the stencil boxes without bricks on 2 and 8, and
the IPC case between processes.  Measured on an MI355X: 0 mismatches and 0 components off float32(ref) in all 13;
undetermined 0 except the stencil boxes (1 of 55 539 and 2 of 107 811, the reference side's own counts).

Every case also asserts, per rank: check_finite() == 0; every copy of a global node equals the first one seen bit for bit;
the downloaded old field equals u1[gid] bit for bit; hq_info.transport (4 = linked in one process, 2 = IPC, 3 = host-staged)
and variant; the kernel form from the counters; the options as resolved.  hq_info has no count of the stencil patches that
own interface nodes: the brick boxes assert brick_nodes > 0 on every rank, the stencil boxes stencil_patches > 0 on every rank
and stencil_patches == npatches on a rank that owns interface nodes.  het70x20x12 on 3 ranks has per-element units on every
rank (the planner's host-only check: 3 / 3 / 4, ragged on ranks 1 and 2), packed unless brick_no_pack.

Worst |got - ref| / (2^-53 T) per kernel family and route on an MI355X (the bound is 64; all | owned interface nodes = the
non-owned copies of them | hanging nodes).  The interface figure is the same on every route of a problem: the sums and the
update of hq_k_interface_update do not depend on how the records travel.
    hq_k_patch_seed, c5_gradient_branch on 8 and on 5 ranks, overlap 0 / 1, no_fused_share, group_copies, debug_halo,
      patch_merge_rounds = 0, no_bricks, and between processes (IPC fused, IPC with its own pack kernel, host-staged):
                                             rayleigh 6.55 | 2.47 | 4.53    mass 4.91 | 2.40 | 3.55    none 4.92 | 2.24 | 4.65
    hq_k_patch_step, hq_k_patch_pers (w form and patch_wform = 0), c5_gradient_branch on 8:        2.55 | 2.47 | 2.07
    ragged per-element brick units (H.RAGGED_PLAN) on c5_gradient_branch on 8: packed 3.75, unpacked 3.49 | 2.47 | 2.07
    scatter: c5_gradient_branch rayleigh 2.55 | 2.47 | 2.07, mass 2.82 | 2.40 | 2.05; two_level 1.26 | 1.26 | 0.80; het70x20x12 2.65 | 2.55
    two_level on 5 (patch, group_copies):                                                          2.98 | 1.26 | 1.23
    hq_k_brick_het<PACKED> on het70x20x12 on 3: rayleigh 4.49 | 2.55    mass 4.97 | 2.21    none 3.23 | 2.58;  brick_no_pack 3.54 | 2.55
    hq_k_brick on the box, 2 ranks 1.72 | 1.12, 8 ranks 1.72 | 1.21 (overlap, brick_by_component, no_fused_share alike)
    hq_k_patch_stencil on the boxes without bricks: 2 ranks 1.73 | 1.05, 8 ranks 1.84 | 1.37
    float state: 0.992 (c5_gradient_branch on 8), 0.975 (two_level), 0.992 (box), 0.995 (IPC between processes) of the f32 bound
The same step LOADED (LOADED_CASES, loaded_reference below): every rank calls hq_set_source for ALL the nodes it harbors with
forces of its own ahead of the step, so the load meets every stiffness and damping sum on its way through the interface
launch, d_iforce, the contribution exchange and the hanging-node schedules; hanging nodes with anchors on other ranks are
loaded on both sides.  The reference is the global extended step loaded with the sum over the ranks, T with sum_r |F_r dt^2|
(not |sum_r F_r| dt^2: the device sums the ranks' contributions in messenger order and they may cancel); B_oracle = the
single-rank C oracle on the assembled tables with the summed load, pinned below 4 by tests/test_loaded_step_cpu.py:
    c5_gradient_branch on 8: 3.22 (float 3.03)   het70x20x12 on 3: 3.43   two_level on 5: 2.04   box 32x16x16 on 2: 2.19 (float
    2.12)   box 32x32x16 on 2 without bricks: 2.49
Measured on an MI355X (all | owned interface = non-owned | hanging): c5_gradient_branch on 8, patch, overlap 0 and 1:
5.09 | 1.94 | 4.19; scatter 2.65 | 2.65 | 2.02; het70x20x12 on 3 packed 3.82 | 2.21; two_level on 5 1.96 | 1.20 | 1.30; the brick
box 1.81 | 1.21; the stencil box 1.59 | 1.30; the float twins (c5 on 8, the brick box): 0 mismatches, 0 off float32(ref),
undetermined 0 of 17 550 and 1 of 28 611 (the reference side's own count), 0.997 and 0.987 of the f32 bound.  Not covered: the
routes between processes carry the same d_iforce records whatever filled them; the unloaded cases cover them.
68 cases in 26 s on the device, the nine loaded ones 1.6 s of it (59 in 26 s before them; 50 in 25 s before the nine float twins, which take 0.1 - 0.7 s each); the slowest are the
four between processes (2.6 - 3.9 s: five processes start), of the others the first of a problem (2.1 s with its
reference), then 0.2 - 0.7 s each.

Patch plans off the default geometry (ST.GEOMETRY with no_bricks = 1, overlap 1).  At the defaults a rank of
c5_gradient_branch on 8 has 2 - 3 patches and one of two_level on 5 has 1: the interface ordering d_order[nb | ne | nr | ns]
and the persistent queue are stepped with almost nothing in them.  c5-8-pmax8 gives every rank 140 - 175 patches (two_level-5-
pmax8: 41 - 57; the stencil box on 2 ranks: 1 296 and 1 352 subsets of 2 x 2 x 2 nodes), c5-8-pmax8-patch_step one workgroup of
64 threads per patch, c5-8-pmax27-pmerge1 59 - 70 cubes that are never merged, c5-8-nlmax776 a smaller image, c5-8-big ONE patch
per rank (interface and interior work in it, hq_k_patch_step), c5-8-vmax16 halving for the hanging-node accumulators; float
twins f32-c5-8-pmax8 and f32-box-2-stencil-pmax8-ov0, and loaded-c5-8-pmax8.  check_route asserts for every case without
bricks that each rank's npatches is hq_plan_check's on that rank's description (rank_plans; the plans and what they mean
without a device: tests/test_patch_geometry_cpu.py).  Finding: none.  Measured on an MI355X (all | owned interface = non-owned |
hanging, x 2^-53 T): c5-8-pmax8, -pmax27-pmerge1, -nlmax776, -vmax16 6.55 | 2.47 | 4.53 -- the default plan's figures to the
digit; c5-8-pmax8-patch_step and c5-8-big 2.55 | 2.47 | 2.07; two_level-5-pmax8 1.62 | 1.27 | 1.23; box-2-stencil-pmax8-ov0
1.73 | 1.14; loaded-c5-8-pmax8 5.09 | 1.94 | 4.19; the float twins 0 mismatches, 0 off float32(ref), undetermined 0 of 17 550 and
1 of 55 539 (the reference side's own count), 0.992 and 0.997 of the f32 bound.
79 cases in 33 s with them (68 in 26 s before; the 11 alone take 3.4 s, 0.1 - 0.3 s each -- the rest of the difference is the
four cases between processes, 3.8 - 4.9 s each in that run)."""
import numpy as np
import pytest

import hercules_amd as ha
from tests import helpers as H
from tests import test_gpu_step_terms as ST        # (its module-level guard skips this module too where longdouble is narrow)

pytestmark = pytest.mark.gpu

PATCH, SCATTER = ha.HQ_VARIANT_PATCH, ha.HQ_VARIANT_SCATTER
EPS = ST.EPS
BOX_BRICKS = (32, 16, 16)                                     # bricks on every rank, on 2 and on 8 ranks
BOX_STENCIL = {2: (32, 32, 16), 8: (32, 32, 32)}              # no_bricks = 1: lattice-subset patches on every rank


def problem_of(c):
    if c["kind"] == "box":
        return H.box_step_problem(c["mesh"], c["nranks"], c["precision"])
    return H.partition_step_problem(c["mesh"], c["nranks"], c["damping"], c["precision"])


def bound_factor(q):
    """B = 16 * max(B_oracle, 4), B_oracle of the DOUBLE oracle on that problem (as in tests/test_gpu_step_terms.py)."""
    if q["precision"] == "f32":
        q = (H.box_step_problem(q["shape"], q["nranks"]) if "shape" in q else
             H.partition_step_problem(q["mesh"], q["nranks"], q["damping"]))
    b = q["B_oracle"]
    assert b <= 64.0, b                                          # (a broken reference cannot inflate the bar)
    return 16.0 * max(b, 4.0)


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
def _oct(mesh, nranks, overlap, damping="rayleigh", variant=PATCH, options=None, precision="f64", pack=False, route=()):
    return dict(kind="oct", mesh=mesh, nranks=nranks, damping=damping, variant=variant, options=dict(options or {}, overlap=overlap),
                precision=precision, pack=pack, route=tuple(route))


def _box(nranks, overlap, options=None, precision="f64"):
    stencil = bool((options or {}).get("no_bricks"))
    return dict(kind="box", mesh=BOX_STENCIL[nranks] if stencil else BOX_BRICKS, nranks=nranks, damping="rayleigh", variant=PATCH,
                options=dict(options or {}, overlap=overlap), precision=precision, pack=False, route=("box_stencil" if stencil else "box",))


C5, NOBRICKS = "c5_gradient_branch", ("no_bricks",)
CASES = {}
for _ov in (0, 1):
    for _d in ("rayleigh", "mass", "none"):
        CASES["c5-8-patch-ov%d-%s" % (_ov, _d)] = _oct(C5, 8, _ov, _d, route=NOBRICKS)
        CASES["het-3-patch-ov%d-%s" % (_ov, _d)] = _oct("het70x20x12", 3, _ov, _d, pack=True, route=("het",))
    CASES["c5-5-patch-ov%d" % _ov] = _oct(C5, 5, _ov, route=NOBRICKS)
    for _d in ("rayleigh", "mass"):
        CASES["c5-8-scatter-ov%d-%s" % (_ov, _d)] = _oct(C5, 8, _ov, _d, variant=SCATTER, route=("scatter",))
    CASES["two_level-5-patch-ov%d" % _ov] = _oct("two_level", 5, _ov, route=NOBRICKS)
    CASES["box-2-ov%d-bycomp%d" % (_ov, _ov)] = _box(2, _ov, {"brick_by_component": _ov})
    CASES["box-8-ov%d-bycomp%d" % (_ov, 1 - _ov)] = _box(8, _ov, {"brick_by_component": 1 - _ov})
CASES.update({
    "c5-8-no_fused_share": _oct(C5, 8, 1, options={"no_fused_share": 1}, route=NOBRICKS),
    "c5-8-group_copies": _oct(C5, 8, 1, options={"group_copies": 1}, route=NOBRICKS),
    "c5-8-debug_halo": _oct(C5, 8, 1, options={"debug_halo": 1}, route=NOBRICKS + ("debug_halo",)),
    "c5-8-merge_rounds0": _oct(C5, 8, 1, options={"patch_merge_rounds": 0}, route=NOBRICKS),
    "c5-8-patch_step": _oct(C5, 8, 1, options={"patch_pipe": 0}, route=NOBRICKS + (("kernel", "hq_k_patch_step"),)),
    "c5-8-patch_pers": _oct(C5, 8, 1, options={"patch_pipe": 4}, route=NOBRICKS + (("kernel", "hq_k_patch_pers"),)),
    "c5-8-patch_seed": _oct(C5, 8, 1, options={"patch_pipe": 6}, route=NOBRICKS + (("kernel", "hq_k_patch_seed"),)),
    "c5-8-patch_pers-u1u2": _oct(C5, 8, 1, options={"patch_pipe": 4, "patch_wform": 0}, route=NOBRICKS + (("kernel", "hq_k_patch_pers"),)),
    "c5-8-no_bricks": _oct(C5, 8, 1, options={"no_bricks": 1}, route=NOBRICKS),
    "c5-8-ragged-packed": _oct(C5, 8, 1, options=H.RAGGED_PLAN, pack=True, route=("ragged",)),
    "c5-8-ragged": _oct(C5, 8, 1, options=H.RAGGED_PLAN, route=("ragged",)),
    "two_level-5-scatter": _oct("two_level", 5, 1, variant=SCATTER, route=("scatter",)),
    "two_level-5-group_copies": _oct("two_level", 5, 1, options={"group_copies": 1}, route=NOBRICKS),
    "het-3-no_pack": _oct("het70x20x12", 3, 1, options={"brick_no_pack": 1}, pack=True, route=("het",)),
    "het-3-scatter": _oct("het70x20x12", 3, 1, variant=SCATTER, route=("scatter",)),
    "box-2-no_fused_share": _box(2, 1, {"no_fused_share": 1}),
    "box-8-no_fused_share": _box(8, 1, {"no_fused_share": 1}),
    "box-2-stencil-ov0": _box(2, 0, {"no_bricks": 1}),
    "box-8-stencil-ov1": _box(8, 1, {"no_bricks": 1}),
    "f32-c5-8": _oct(C5, 8, 1, precision="f32", route=NOBRICKS),
    "f32-two_level-5": _oct("two_level", 5, 1, precision="f32", route=NOBRICKS),
    "f32-box-2": _box(2, 1, precision="f32"),
    # float twins of the forms above that had none (the criterion: ST.rounded_step on every copy of every rank)
    "f32-het-3": _oct("het70x20x12", 3, 1, pack=True, precision="f32", route=("het",)),
    "f32-het-3-none": _oct("het70x20x12", 3, 1, "none", pack=True, precision="f32", route=("het",)),
    "f32-het-3-no_pack": _oct("het70x20x12", 3, 1, options={"brick_no_pack": 1}, pack=True, precision="f32", route=("het",)),
    "f32-box-2-stencil-ov0": _box(2, 0, {"no_bricks": 1}, precision="f32"),
    "f32-box-8-stencil-ov1": _box(8, 1, {"no_bricks": 1}, precision="f32"),
    "f32-c5-8-scatter": _oct(C5, 8, 1, variant=SCATTER, precision="f32", route=("scatter",)),
    "f32-c5-8-patch_step": _oct(C5, 8, 1, options={"patch_pipe": 0}, precision="f32", route=NOBRICKS + (("kernel", "hq_k_patch_step"),)),
    "f32-c5-8-patch_pers": _oct(C5, 8, 1, options={"patch_pipe": 4}, precision="f32", route=NOBRICKS + (("kernel", "hq_k_patch_pers"),)),
    "f32-c5-8-patch_pers-u1u2": _oct(C5, 8, 1, options={"patch_pipe": 4, "patch_wform": 0}, precision="f32",
                                     route=NOBRICKS + (("kernel", "hq_k_patch_pers"),)),
})


def _geometry(g, **more):
    """no_bricks = 1 and the fields of a geometry of tests/test_gpu_step_terms.py (ST.GEOMETRY)."""
    return dict(ST.NB, **dict(ST.GEOMETRY[g], **more))


STEP = (("kernel", "hq_k_patch_step"),)
CASES.update({
    # patch plans off the default geometry: 140 - 175 patches per rank instead of 2 - 3, one workgroup per patch, cubes that are
    # never merged, a smaller image, ONE patch per rank (interface and interior work in it), halving for the hanging nodes
    "c5-8-pmax8": _oct(C5, 8, 1, options=_geometry("pmax8"), route=NOBRICKS),
    "c5-8-pmax8-patch_step": _oct(C5, 8, 1, options=_geometry("pmax8-step"), route=NOBRICKS + STEP),
    "c5-8-pmax27-pmerge1": _oct(C5, 8, 1, options=_geometry("pmax27-pmerge1"), route=NOBRICKS),
    "c5-8-nlmax776": _oct(C5, 8, 1, options=_geometry("nlmax776"), route=NOBRICKS),
    "c5-8-big": _oct(C5, 8, 1, options=_geometry("big"), route=NOBRICKS + STEP),
    "c5-8-vmax16": _oct(C5, 8, 1, options=_geometry("vmax16"), route=NOBRICKS),
    "two_level-5-pmax8": _oct("two_level", 5, 1, options=_geometry("pmax8"), route=NOBRICKS),
    "box-2-stencil-pmax8-ov0": _box(2, 0, _geometry("pmax8")),
    "f32-c5-8-pmax8": _oct(C5, 8, 1, options=_geometry("pmax8"), precision="f32", route=NOBRICKS),
    "f32-box-2-stencil-pmax8-ov0": _box(2, 0, _geometry("pmax8"), precision="f32"),
})

# ranks in processes of their own (tests/_hq_rank_worker.py, kind "step"): c5_gradient_branch on 5 ranks
PROCESS_CASES = {
    "ipc-fused": dict(mesh=C5, nranks=5, transport="ipc", precision="f64", env={"HQ_OVERLAP": "1"}),
    "ipc-no_fused_share": dict(mesh=C5, nranks=5, transport="ipc", precision="f64", env={"HQ_OVERLAP": "1", "HQ_NO_FUSED_SHARE": "1"}),
    "host": dict(mesh=C5, nranks=5, transport="host", precision="f64", env={"HQ_OVERLAP": "1"}),
    "ipc-f32": dict(mesh=C5, nranks=5, transport="ipc", precision="f32", env={"HQ_OVERLAP": "1"}),
}


# ---------------------------------------------------------------------------------------------
# the route a case is about, from every rank's counters and resolved options
# ---------------------------------------------------------------------------------------------
def rank_plans(c, q, boxes=()):
    """hq_plan_check's report of every rank of a case whose contexts have no bricks, under the HQ_PATCH_* equivalents of the
    case's options (ST.plan_environment): what hq_create plans there.  Boxes: their own plan_check()."""
    from hercules_amd import capi
    with pytest.MonkeyPatch.context() as mp:
        ST.plan_environment(mp, c["options"])
        if c["kind"] == "box":
            return [b.plan_check() for b in boxes]
        return [capi.plan_check(H.rank_desc(q, r)) for r in range(c["nranks"])]


def check_route(c, solvers, q, boxes=()):
    """On the linked contexts, before the step."""
    infos = [s.info() for s in solvers]
    if "no_bricks" in c["route"] or "box_stencil" in c["route"]:  # patches alone: the plan is the host-only check's
        plans = rank_plans(c, q, boxes)
        assert [p["faults"] for p in plans] == [0] * c["nranks"], plans
        assert [i["npatches"] for i in infos] == [p["patches"] for p in plans], (infos, plans)
        print("\n[partition-step] patches per rank %s" % [i["npatches"] for i in infos])
    for r, (s, info) in enumerate(zip(solvers, infos)):
        o, kernel = s.options(), s.dominant_kernel()
        assert info["transport"] == 4 and info["variant"] == c["variant"] and info["nranks"] == c["nranks"], (r, info)
        for k, v in c["options"].items():
            assert o[k] == v, (r, k, o[k])
        assert info["debug_halo"] == int("debug_halo" in c["route"]), (r, info)
        for tag in c["route"]:
            if tag == "no_bricks":                               # patches alone: element form, lattice subsets through the stencil kernel
                assert info["brick_nodes"] == 0 and info["npatches"] > 0 and kernel.startswith("hq_k_patch"), (r, kernel, info)
            elif tag == "scatter":
                assert kernel == "hq_k_element_scatter", (r, kernel)
            elif tag == "box":
                assert info["brick_nodes"] > 0 and info["brick_units_het"] == 0 and kernel == "hq_k_brick", (r, kernel, info)
            elif tag == "box_stencil":
                assert info["brick_nodes"] == 0 and info["stencil_patches"] > 0 and info["ragged_patches"] > 0, (r, info)
            elif tag == "het":                                   # (float n_t rows pack only without damping: ST.float_rows_pack)
                packs = not c["options"].get("brick_no_pack") and (c["precision"] == "f64" or ST.float_rows_pack(c["damping"]))
                assert info["brick_units_packed"] == (info["brick_units_het"] if packs else 0), (r, info)
            elif tag == "ragged":                                # what the counters report: partitions this small need not have bricks
                assert info["brick_units_het"] >= info["brick_units_ragged_het"], (r, info)
                assert (info["brick_units_packed"] > 0) == (bool(c["pack"]) and info["brick_units_het"] > 0), (r, info)
            elif isinstance(tag, tuple) and tag[0] == "kernel":
                assert kernel in (tag[1], "hq_k_patch_stencil"), (r, kernel)
    if "box_stencil" in c["route"]:
        # a rank that owns interface nodes and has stencil patches only: hq_k_patch_stencil's launch ahead of the exchange
        owns = [any(k.startswith("owned-interface") for k in kinds) for kinds in node_kinds(q)]
        assert any(o and i["stencil_patches"] == i["npatches"] for o, i in zip(owns, infos)), (owns, infos)
    if "het" in c["route"]:
        assert sum(i["brick_units_het"] for i in infos) > 0 and sum(i["brick_nodes"] for i in infos) > 0, infos
    if "ragged" in c["route"]:
        assert sum(i["brick_units_ragged_het"] for i in infos) >= 2, infos
    return infos


def make_solvers(c, q):
    """-> (solvers, boxes): rank r's context on u1[gid], u2[gid]; the caller closes both."""
    solvers, boxes = [], []
    try:
        if c["kind"] == "box":
            boxes = H.box_step_boxes(c["mesh"], c["nranks"])
            for r, b in enumerate(boxes):
                solvers.append(b.create_solver(variant=c["variant"], tm1=q["u1"][q["gid"][r]], tm2=q["u2"][q["gid"][r]],
                                               options=c["options"], precision=c["precision"]))
        else:
            for r, part in enumerate(q["parts"]):
                kw = dict(edata=q["edata"][r], material=q["material"]) if c["pack"] else {}
                solvers.append(ha.Solver(part["lnid"], q["ets"][r], q["nts"][r], q["dt"], tm1=q["u1"][q["gid"][r]],
                                         tm2=q["u2"][q["gid"][r]], dangling=part["dangling"], an_sched=part["an_sched"],
                                         dn_sched=part["dn_sched"], rank=r, nranks=c["nranks"], node_xyz=q["node_xyz"][r],
                                         variant=c["variant"], options=c["options"], precision=c["precision"], **kw))
    except BaseException:
        close_all(solvers, boxes)
        raise
    return solvers, boxes


def close_all(solvers, boxes):
    for s in solvers:
        s.close()
    for b in boxes:
        b.close()


def node_kinds(q):
    """Per rank, a label for every node: owned-interface (with its sharers) / non-owned / hanging / interior."""
    out = []
    if "parts" in q:
        for cl in H.partition_classes(q):
            out.append(np.where(cl["hanging"], "hanging", np.where(cl["foreign"], "non-owned",
                       np.where(cl["interface"], np.char.add("owned-interface/", cl["sharers"].astype(str)), "interior"))))
    else:
        copies = np.zeros(q["N"], np.int64)
        for g in q["gid"]:
            copies[g] += 1
        for r, g in enumerate(q["gid"]):
            out.append(np.where(q["owner"][r] != r, "non-owned", np.where(copies[g] > 1, np.char.add("owned-interface/", (copies[g] - 1).astype(str)),
                                                                         "interior")))
    return out


def check_fields(name, q, fields, olds, B, family=None):
    """The bound, the copies and the old field for every rank's download; prints the [partition-step] line.  A float
    state: also ST.rounded_step, one step = float32(double step), for every copy (family: the kernels, for its message)."""
    f32 = q["precision"] == "f32"
    bits = np.int32 if f32 else np.int64
    kinds = node_kinds(q)
    first, have = np.zeros((q["N"], 3), q["real"]), np.zeros(q["N"], bool)
    top, by_kind = (-1.0,), {}
    for r, (g, u, old) in enumerate(zip(q["gid"], fields, olds)):
        assert u.dtype == q["real"] and np.isfinite(u).all(), r
        assert np.array_equal(old.view(bits), q["u1"][g].view(bits)), ("the old field is not the uploaded tm1", r)
        full = np.array(q["ref"])                                # this rank's copies among the reference's own values
        full[g] = u
        w = ST.worst(full, q["ref"], q["T"], B, f32, q["dangling"])
        local = int(np.nonzero(g == w[1])[0][0]) if w[0] > 0 else 0
        if w[0] > top[0]:
            top = (w[0], r, local, w[2], w[3], str(kinds[r][local]))
        ratio = (np.abs(u.astype(np.longdouble) - q["ref"][g]) / (EPS * q["T"][g])).max(axis=1).astype(np.float64)
        for k in ("owned-interface", "non-owned", "hanging", "interior"):
            sel = np.char.startswith(kinds[r].astype(str), k)
            if sel.any():
                by_kind[k] = max(by_kind.get(k, 0.0), float(ratio[sel].max()))
        seen = have[g]
        assert np.array_equal(first[g[seen]].view(bits), u[seen].view(bits)), ("copies of one node differ", r)
        first[g[~seen]] = u[~seen]
        have[g] = True
    print("\n[partition-step] %-28s worst %.3f of the bound = %.2f x 2^-53 T: rank %d node %d.%d (%s)%s | by class, x 2^-53 T: %s"
          % (name, top[0], top[4], top[1], top[2], top[3], top[5], " (f32: mostly the state's rounding)" if f32 else "",
             "  ".join("%s %.2f" % kv for kv in by_kind.items())))
    assert have.all()
    assert top[0] <= 1.0, top
    if f32:
        # every copy equals `first` bit for bit (asserted above): what holds for it holds for every copy on every rank, a
        # hanging node's anchors included -- the values that rank holds are these
        r = ST.rounded_step(first, q["ref"], q["T"], B, q["dangling"])
        print("[partition-step] %-28s float32(double step): mismatches %d, undetermined %d of %d, got != float32(ref) inside the band %d"
              % (name, r["mismatches"], r["undetermined"], r["plain"], r["off_centre"]))
        where = None
        if r["first"]:
            n = r["first"][0]
            where = dict(ranks={rk: str(kinds[rk][int(np.nonzero(g == n)[0][0])]) for rk, g in enumerate(q["gid"]) if (g == n).any()},
                         branch_of=ST.branch_of(dict(lnid=q["lnid"], labels=q["labels"]), n) if q.get("labels") is not None else None)
        ST.assert_rounded_step(name, r, family, where)


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_one_step_from_independent_fields_on_partitions(case):
    from hercules_amd import capi
    c = CASES[case]
    q = problem_of(c)
    B = bound_factor(q)
    solvers, boxes = make_solvers(c, q)
    try:
        capi.group_link(solvers)
        infos = check_route(c, solvers, q, boxes)
        family = (sorted({s.dominant_kernel() for s in solvers}),) + tuple(
            "%s=%d" % (k, sum(i[k] for i in infos)) for k in ("brick_units", "brick_units_het", "brick_units_packed", "npatches", "stencil_patches"))
        capi.group_run(solvers, 1)
        got = [s.download() for s in solvers]
        nonfinite = [s.check_finite() for s in solvers]
    finally:
        close_all(solvers, boxes)
    assert nonfinite == [0] * c["nranks"], nonfinite
    check_fields(case, q, [g[0] for g in got], [g[1] for g in got], B, family)


# ---------------------------------------------------------------------------------------------
# the same step LOADED: every rank loads all it harbors, on a field that moves
# ---------------------------------------------------------------------------------------------
LOADED_CASES = {
    "loaded-c5-8-patch-ov0": _oct(C5, 8, 0, route=NOBRICKS),
    "loaded-c5-8-patch-ov1": _oct(C5, 8, 1, route=NOBRICKS),
    "loaded-c5-8-scatter": _oct(C5, 8, 1, variant=SCATTER, route=("scatter",)),
    "loaded-het-3-packed": _oct("het70x20x12", 3, 1, pack=True, route=("het",)),
    "loaded-two_level-5": _oct("two_level", 5, 1, route=NOBRICKS),
    "loaded-box-2": _box(2, 1),
    "loaded-box-2-stencil": _box(2, 0, {"no_bricks": 1}),
    "loaded-f32-c5-8-patch": _oct(C5, 8, 1, precision="f32", route=NOBRICKS),
    "loaded-f32-box-2": _box(2, 1, precision="f32"),
    "loaded-c5-8-pmax8": _oct(C5, 8, 1, options=_geometry("pmax8"), route=NOBRICKS),
}
LOADED_SEED = 31000                                              # rank r: H.rest_forces(..., LOADED_SEED + r), as tests/test_gpu_sources.py
_LOADED = {}


def loaded_reference(c):
    """The loaded step of a case's problem: rank r loads ALL the nodes it harbors (owned, merely harbored, hanging) with
    forces of its own, H.rest_forces on the global n_t rows with seed LOADED_SEED + r, taken at its nodes.  The reference is
    the global H.extended_step loaded with every rank's table in turn -- force gets the sum over ranks and T the sum of
    |F_r dt^2|, not |sum F_r| dt^2: the device sums the ranks' contributions in messenger order and they may cancel.
    B_oracle: the single-rank C oracle on the assembled global tables with the summed load (double sum in rank order).
    Built once per problem, read-only.  -> dict(Fr = per rank [its nodes, 3], total [N, 3], ref, T, B_oracle)"""
    key = (c["kind"], c["mesh"], c["nranks"], c["damping"], c["precision"])
    if key in _LOADED:
        return _LOADED[key]
    from oracle import herc_oracle as ho
    q = problem_of(c)
    N = q["N"]
    tables, total = [], np.zeros((N, 3))
    for r, g in enumerate(q["gid"]):
        Fk = np.zeros((N, 3))
        Fk[g] = H.rest_forces(q["ntable"][:, 0], q["dt"], LOADED_SEED + r)[g]
        tables.append(Fk)
        total += Fk
    every = np.arange(N, dtype=np.int32)
    ref, T = H.extended_step(q["lnid"], q["etable"], q["ntable"], q["u1"], q["u2"], q["dangling"], loaded=every, F=tables, dt=q["dt"])
    o1, o2 = np.array(q["u2"]), np.array(q["u1"])
    ho.solver_run(np.ascontiguousarray(q["lnid"], np.int32), np.ascontiguousarray(q["etable"]), np.ascontiguousarray(q["ntable"]), o1, o2, 0, 1,
                  q["dt"], damping=q.get("kind", ho.DAMP_RAYLEIGH), loaded_lnid=every, forces=total[None], dangling=q["dangling"])
    b = float((np.abs(o2 - ref) / ((2.0 ** -24 if c["precision"] == "f32" else EPS) * T)).max())
    out = H._freeze(dict(Fr=[np.ascontiguousarray(Fk[g]) for Fk, g in zip(tables, q["gid"])], total=total, ref=ref, T=T, B_oracle=b,
                         oracle=o2))
    _LOADED[key] = out
    return out


def loaded_bound_factor(c):
    """B = 16 * max(B_oracle, 4), B_oracle of the DOUBLE oracle's loaded step on that problem."""
    b = loaded_reference(dict(c, precision="f64"))["B_oracle"]
    assert b <= 64.0, b                                          # (a broken reference cannot raise the bar)
    return 16.0 * max(b, 4.0)


@pytest.mark.parametrize("case", list(LOADED_CASES), ids=list(LOADED_CASES))
def test_one_loaded_step_on_partitions(case):
    """hq_set_source on every rank ahead of the step from independent fields: the load through the interface launch of the
    patch kernels, d_iforce, the contribution exchange and the hanging-node schedules, where every stiffness and damping
    sum is in play -- hanging nodes with anchors on other ranks are loaded on both sides (c5_gradient_branch, two_level).
    The routes between processes carry the same d_iforce records whatever filled them: the unloaded cases cover them."""
    from hercules_amd import capi
    c = LOADED_CASES[case]
    q = problem_of(c)
    L = loaded_reference(c)
    B = loaded_bound_factor(c)
    solvers, boxes = make_solvers(c, q)
    try:
        for r, s in enumerate(solvers):
            s.set_source(np.arange(len(q["gid"][r]), dtype=np.int32), L["Fr"][r][None])
        capi.group_link(solvers)
        infos = check_route(c, solvers, q, boxes)
        family = (sorted({s.dominant_kernel() for s in solvers}),) + tuple(
            "%s=%d" % (k, sum(i[k] for i in infos)) for k in ("brick_units", "brick_units_het", "brick_units_packed", "npatches", "stencil_patches"))
        capi.group_run(solvers, 1)
        got = [s.download() for s in solvers]
        nonfinite = [s.check_finite() for s in solvers]
    finally:
        close_all(solvers, boxes)
    assert nonfinite == [0] * c["nranks"], nonfinite
    check_fields(case, dict(q, ref=L["ref"], T=L["T"]), [g[0] for g in got], [g[1] for g in got], B, family)


# ---------------------------------------------------------------------------------------------
# between processes
# ---------------------------------------------------------------------------------------------
def _flat(sched):
    """{"c": [(peer, mapping)], "s": [...]} -> arrays for an .npz: peers, offsets, the mappings end to end."""
    out = {}
    for k in ("c", "s"):
        items = sched[k]
        out[k + "_peer"] = np.array([p for p, _ in items], np.int32)
        out[k + "_ptr"] = np.concatenate([[0], np.cumsum([len(m) for _, m in items])]).astype(np.int64)
        out[k + "_map"] = np.concatenate([np.asarray(m, np.int32) for _, m in items]) if items else np.zeros(0, np.int32)
    return out


@pytest.mark.parametrize("case", list(PROCESS_CASES), ids=list(PROCESS_CASES))
def test_one_step_from_independent_fields_between_processes(case, tmp_path):
    """Five ranks of c5_gradient_branch in processes of their own (six with this one): the fused hq_k_interface_update<1>
    over the IPC transport, the same with the sharing packed by its own kernel, the host-staged transport, a float state."""
    from tests.test_gpu_multiprocess import _launch
    c = PROCESS_CASES[case]
    q = H.partition_step_problem(c["mesh"], c["nranks"], "rayleigh", c["precision"])
    B = bound_factor(q)
    for r, part in enumerate(q["parts"]):
        sch = {"%s_%s" % (w, k): v for w in ("an", "dn") for k, v in _flat(part[w + "_sched"]).items()}
        np.savez(str(tmp_path / ("rank%d_in.npz" % r)), lnid=part["lnid"], etable=q["ets"][r], ntable=q["nts"][r], dt=q["dt"],
                 tm1=q["u1"][q["gid"][r]], tm2=q["u2"][q["gid"][r]], node_xyz=q["node_xyz"][r], gid=q["gid"][r],
                 dn_ids=part["dangling"][0], dn_ptr=part["dangling"][1], dn_anchors=part["dangling"][2],
                 precision=c["precision"], **sch)
    out = _launch(tmp_path, c["nranks"], "step", 1, dict(c["env"], HQ_TEST_TRANSPORT=c["transport"]))
    for r, z in enumerate(out):
        assert np.array_equal(z["gid"], q["gid"][r])
        assert int(z["transport"]) == (2 if c["transport"] == "ipc" else 3) and int(z["nonfinite"]) == 0, r
        assert str(z["kernel"]).startswith("hq_k_patch") and int(z["brick_nodes"]) == 0, (r, str(z["kernel"]))
    check_fields("processes-" + case, q, [z["tm1"] for z in out], [z["tm2"] for z in out], B, sorted({str(z["kernel"]) for z in out}))
