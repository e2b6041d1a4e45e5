"""Source forces on EVERY node: per-node parity of compute_addforce_s (psolve.c:5912-5928) in every stepping kernel.

Each stepping kernel has its own arithmetic for finding "my" loaded node -- hq_k_brick (regular planes, the top and the
bottom face plane, ragged units), hq_k_brick_het (four instantiations), hq_k_patch_step / _pers / _seed / _stencil,
hq_k_source of the scatter variant -- and the host builds the tables behind them (hq_brick_set_source,
hq_patch_set_source with its "virtual accumulators" for loaded hanging nodes, hq_set_source's same-nodes path).

A. One step from rest (tm1 = tm2 = None) with every node loaded by a force of its own: all stiffness and damping sums are
   exactly zero, so the oracle leaves u(1)[n][d] = F[n][d] * dt^2 / n_t[n][0] at a plain node and every node's result
   depends on its own force only.  The comparison is per node and per component, relative to that node's OWN value:
   a source that is missed, lands on a neighbour or another component, is applied twice or meets the wrong mass row
   shows at that node.  Forces: sign * uniform(0.5, 1) * 1e-3 * n_t[n][0] / dt^2, so every expected value is about 1e-3.
   Meshes with hanging nodes run twice: phase "plain" loads every non-hanging node, phase "all" the hanging ones too.
   Bounds on |got - ref|, ref = the oracle's own single step (with dangling=):
     loaded, neither hanging nor anchor, fp64 : 1e-14 * |ref| per node and component (the kernels multiply by a rounded
                                                reciprocal where the reference divides: at most 3 half-ulps; packed n_t
                                                rows equal the caller's to 1e-15)
     anchors and hanging nodes, fp64          : 1e-14 * max|ref| (F_a + sum F_h / deps may cancel, other order of the sum)
     precision="f32", plain nodes             : 2e-7 * |ref| against the float oracle on float n_t rows (the float
                                                reference rounds F * dt^2 and the quotient, the library rounds once:
                                                1.5 float ulps)
     precision="f32", every node              : one step of the float library is float32(double step)
                                                (tests/test_gpu_step_terms.rounded_step) against tests/helpers.extended_step
                                                with zero fields, T = the summed |F dt^2| terms over m0, B from the double
                                                oracle's own step from rest: plain nodes AND anchors equal float32(ref)
                                                wherever the band lies inside one float, every hanging node equals
                                                hanging_assignment of the library's own stored anchors bit for bit
                                                (rounded_reference() below; the reference side meets the cap without a
                                                device: tests/test_loaded_step_cpu.py).  B = 64; 64.8 on c5_basin with
                                                the hanging nodes loaded (B_oracle 4.05).  Measured on an MI355X, all
                                                three cases: 0 mismatches, 0 undetermined, 0 off float32(ref)
   Nothing may be non-finite.
B. Partitions over the in-process transport: as in the reference every rank loads ALL of its harbored nodes (owned,
   merely harbored, hanging) with forces of its own; the oracle is the single-rank run loaded with the sum over ranks.
   Every harbored copy within 1e-14 * max|ref|; the copies of one global node bit-equal.
C. The window of hq_set_source (step0, nsteps), the same-nodes path, a rebuild for a longer table, a permuted list,
   a subset and the empty list, stepped along with the oracle: rel_linf < 1e-9.

The same node id twice in one loaded list: hq_set_source refuses it (the reference ASSIGNS force = F * dt2 and so does
hq_k_source, the patch and brick kernels ADD; Global.theNodesLoadedList holds every node once) --
tests/test_gpu_loaded_step.py, test_a_node_named_twice_is_refused_and_the_source_stays.  A load on a field that MOVES, where
assigning and adding differ: the same module."""
import functools

import numpy as np
import pytest

import hercules_amd as ha
from oracle import herc_oracle as ho
from tests import helpers as H

pytestmark = pytest.mark.gpu

TOL_PLAIN = 1e-14        # of the node's own value
TOL_FIELD = 1e-14        # of the field's maximum: anchors, hanging nodes, partitions
TOL_PLAIN_F32 = 2e-7
TOL_RUN = 1e-9           # several steps, stiffness sums in play: the suite's bar

PATCH, SCATTER = ha.HQ_VARIANT_PATCH, ha.HQ_VARIANT_SCATTER
RAGGED_PLAN = H.RAGGED_PLAN


# ---------------------------------------------------------------------------------------------
# meshes: tests/helpers.source_mesh (shared with the oracle-side pins and the planner-counter checks of
# tests/test_sources_oracle_cpu.py) + make(): a context on the mesh
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mesh(name):
    p = dict(H.source_mesh(name))

    def make(variant=PATCH, options=None, precision="f64", ntable=None, pack=False):
        if "box" in p:
            return p["box"].create_solver(variant=variant, options=options, precision=precision)
        kw = dict(edata=p["edata"], material=p["material"]) if pack else {}
        return ha.Solver(p["lnid"], p["etable"], p["ntable"] if ntable is None else ntable, p["dt"], dangling=p["dangling"],
                         node_xyz=p["node_xyz"], variant=variant, options=options, precision=precision, **kw)
    p["make"] = make
    return p


@functools.lru_cache(maxsize=None)
def _reference(name, phase, precision="f64"):
    """(loaded, F [N, 3], ref [N, 3]) -- the oracle's single step, computed once per mesh / phase / precision and shared
    (read-only) among the cases."""
    p = _mesh(name)
    nt = np.ascontiguousarray(p["ntable"], np.float32 if precision == "f32" else np.float64)
    F = H.rest_forces(nt[:, 0], p["dt"], 4711)
    hanging, _ = H.node_classes(p["N"], p["dangling"])
    loaded = np.arange(p["N"], dtype=np.int32) if phase == "all" else np.nonzero(~hanging)[0].astype(np.int32)
    ref = H.oracle_step_from_rest(p["lnid"], p["etable"], nt, p["dt"], loaded, F[loaded], p["dangling"]).astype(np.float64)
    for a in (loaded, F, ref):
        a.flags.writeable = False
    return loaded, F, ref


@functools.lru_cache(maxsize=None)
def rounded_reference(name, phase):
    """(ref, T, B) of the float cases' second criterion: tests/helpers.extended_step (np.longdouble) from zero fields on the
    float n_t rows with _reference's load; B = 16 * max(B_oracle, 4), B_oracle = the DOUBLE oracle's step from rest on the
    widened rows against ref in units of 2^-53 T (asserted <= 64).  None where np.longdouble is no wider than double."""
    if not np.finfo(np.longdouble).eps < 1e-18:
        return None
    p = _mesh(name)
    loaded, F, _ = _reference(name, phase, "f32")
    nt = np.ascontiguousarray(p["ntable"], np.float32)
    zero = np.zeros((p["N"], 3), np.float32)
    ref, T = H.extended_step(p["lnid"], p["etable"], nt, zero, zero, p["dangling"], loaded=loaded, F=F[loaded], dt=p["dt"])
    o = H.oracle_step_from_rest(p["lnid"], p["etable"], nt.astype(np.float64), p["dt"], loaded, F[loaded], p["dangling"])
    with np.errstate(invalid="ignore"):                          # (phase "plain": a node nobody loads has ref = T = 0)
        b = float(np.nanmax(np.where(T > 0, np.abs(o - ref) / (2.0 ** -53 * T), 0.0)))
    assert not np.abs(o[np.asarray(T == 0)]).any() and b <= 64.0, b
    for a in (ref, T):
        a.flags.writeable = False
    return ref, T, 16.0 * max(b, 4.0)


@functools.lru_cache(maxsize=None)
def _default_info(name):
    """hq_get_info of the mesh's context as shipped (PATCH variant, no options)."""
    s = _mesh(name)["make"]()
    info = s.info()
    s.close()
    return info


# ---------------------------------------------------------------------------------------------
# A. the cases: (mesh, variant, options, make-keywords, the counters that say the kernel is there)
# ---------------------------------------------------------------------------------------------
def _faces_ride(s, p):
    """hq_k_brick with HQ_BK_TOPFACE and HQ_BK_BOTFACE: both z faces' interiors are brick nodes (nz + 1 planes); x in
    whole 64-wide tiles, the partial tile in y included; the shell stays with the patches."""
    nx, ny, nz = p["shape"]
    wide = nx - 1 if nx - 1 < 64 else 64 * ((nx - 1) // 64)
    info = s.info()
    assert s.dominant_kernel() == "hq_k_brick" and info["brick_nodes"] == wide * (ny - 1) * (nz + 1), info
    assert info["npatches"] > 0 and info["brick_units_het"] == 0 and info["brick_units_ragged"] == 0
    return info


def _chk_brick(s, p, name):
    assert _faces_ride(s, p)["brick_units_pernode"] == 0


def _chk_brick_cz(s, p, name):
    info = _faces_ride(s, p)
    assert info["brick_units"] > _default_info(name)["brick_units"] > 0 and s.options()["brick_cz"] == 5


def _chk_bycomp(s, p, name):
    _chk_brick(s, p, name)
    assert s.options()["brick_by_component"] == 1


def _chk_pernode(s, p, name):
    info = s.info()
    assert s.dominant_kernel() == "hq_k_brick"
    assert info["brick_units"] > 0 and info["brick_units_pernode"] == info["brick_units"] and info["brick_units_het"] == 0


def _chk_two_material(ragged):
    def chk(s, p, name):
        info = s.info()
        assert (info["brick_units_ragged"] >= 8) == bool(ragged) and (info["brick_units_het"] == 0) == bool(ragged), info
    return chk


def _chk_lateral(packed):
    def chk(s, p, name):
        info = s.info()
        assert info["brick_units_het"] > 0, info
        assert info["brick_units_packed"] == (info["brick_units_het"] if packed else 0)
    return chk


def _chk_basin(s, p, name):
    assert s.info()["brick_units_ragged"] >= 2


def _chk_gradient(pack):
    def chk(s, p, name):
        info = s.info()
        assert info["brick_units_ragged_het"] >= 2 and info["brick_units_het"] >= info["brick_units_ragged_het"], info
        assert (info["brick_units_packed"] > 0) == bool(pack)
    return chk


def _chk_stencil_all(s, p, name):
    info = s.info()                                 # all 64 patches are lattice subsets, far faces and dashpots included
    assert info["brick_nodes"] == 0 and s.dominant_kernel() == "hq_k_patch_stencil" and info["ragged_patches"] > 0
    assert info["stencil_patches"] == info["npatches"]


def _chk_stencil_full(s, p, name):
    info = s.info()                                 # 8 full lattices through hq_k_patch_stencil, the subsets in element form
    assert info["brick_nodes"] == 0 and s.dominant_kernel() == "hq_k_patch_seed" and info["ragged_patches"] == 0
    assert 0 < info["stencil_patches"] < info["npatches"]


def _chk_no_stencil(s, p, name):
    info = s.info()                                 # the lattice patches through the element kernel's lattice rows
    assert info["brick_nodes"] == 0 and info["stencil_patches"] == 0 and info["lattice_patches"] > 0
    assert s.dominant_kernel() == "hq_k_patch_seed"


def _chk_pipe(want):
    def chk(s, p, name):
        info = s.info()
        assert info["brick_nodes"] == 0 and s.dominant_kernel() == want, (s.dominant_kernel(), info)
        assert info["npatches"] > info["stencil_patches"]
    return chk


def _chk_scatter(s, p, name):
    assert s.info()["variant"] == SCATTER and s.dominant_kernel() == "hq_k_element_scatter"


def _case(mesh, check, variant=PATCH, options=None, precision="f64", **kw):
    return dict(mesh=mesh, check=check, variant=variant, options=options, precision=precision, kw=kw)


CASES = {}
for _b in ("box32x32x16", "box70x20x12"):
    CASES["brick-" + _b] = _case(_b, _chk_brick)
    CASES["brick-cz5-" + _b] = _case(_b, _chk_brick_cz, options={"brick_cz": 5})
    CASES["brick-bycomp-" + _b] = _case(_b, _chk_bycomp, options={"brick_by_component": 1})
    CASES["brick-pernode-" + _b] = _case(_b, _chk_pernode, options={"brick_no_ntsame": 1})
CASES.update({
    "brick-ragged-two_material": _case("two_material", _chk_two_material(1), options={"brick_ragged": 1}),
    "het-two_material": _case("two_material", _chk_two_material(0), options={"brick_ragged": 0}),
    "het-packed-lateral": _case("lateral", _chk_lateral(True)),
    "het-lateral": _case("lateral", _chk_lateral(False), options={"brick_no_pack": 1}),
    "brick-ragged-c5_basin": _case("c5_basin", _chk_basin, options=RAGGED_PLAN),
    "het-ragged-packed-c5_gradient": _case("c5_gradient", _chk_gradient(1), options=RAGGED_PLAN, pack=True),
    "het-ragged-c5_gradient": _case("c5_gradient", _chk_gradient(0), options=RAGGED_PLAN, pack=False),
    "stencil-subsets-box32": _case("box32", _chk_stencil_all, options={"no_bricks": 1, "patch_ragged": 1}),
    "stencil-full-box32": _case("box32", _chk_stencil_full, options={"no_bricks": 1, "patch_ragged": 0}),
    "element-lattice-rows-box32": _case("box32", _chk_no_stencil, options={"no_bricks": 1, "patch_no_stencil": 1}),
    "patch_step-two_level": _case("two_level", _chk_pipe("hq_k_patch_step"), options={"no_bricks": 1, "patch_pipe": 0}),
    "patch_pers-two_level": _case("two_level", _chk_pipe("hq_k_patch_pers"), options={"no_bricks": 1, "patch_pipe": 4}),
    "patch_seed-two_level": _case("two_level", _chk_pipe("hq_k_patch_seed"), options={"no_bricks": 1, "patch_pipe": 6}),
    "scatter-box32x32x16": _case("box32x32x16", _chk_scatter, variant=SCATTER),
    "scatter-two_level": _case("two_level", _chk_scatter, variant=SCATTER),
    "f32-brick-box32x32x16": _case("box32x32x16", _chk_brick, precision="f32"),
    "f32-brick-ragged-c5_basin": _case("c5_basin", _chk_basin, options=RAGGED_PLAN, precision="f32"),
})
_HANGING = ("c5_basin", "c5_gradient", "two_level")
PARAMS = [(k, ph) for k, c in CASES.items() for ph in (("plain", "all") if c["mesh"] in _HANGING else ("all",))]


def _worst(err, scale, mask):
    """(largest err / scale over the masked nodes, its node, its component); scale an array like err or a number."""
    q = np.where(mask[:, None], err / scale, 0.0)
    n, d = np.unravel_index(np.argmax(q), q.shape)
    return float(q[n, d]), int(n), int(d)


@pytest.mark.parametrize("case,phase", PARAMS, ids=["%s-%s" % kp for kp in PARAMS])
def test_one_step_from_rest_with_every_node_loaded(case, phase):
    one_step_from_rest(case, CASES[case], phase)


def one_step_from_rest(case, c, phase):
    """A. for one case (a _case(...) on a tests/helpers.source_mesh): shared with tests/test_gpu_brick_edges.py, whose
    meshes put the same criterion on degenerate brick units."""
    p = _mesh(c["mesh"])
    f32 = c["precision"] == "f32"
    loaded, F, ref = _reference(c["mesh"], phase, c["precision"])
    kw = dict(c["kw"], ntable=np.ascontiguousarray(p["ntable"], np.float32)) if f32 else c["kw"]
    s = p["make"](variant=c["variant"], options=c["options"], precision=c["precision"], **kw)
    try:
        assert s.info()["variant"] == c["variant"]
        c["check"](s, p, c["mesh"])
        info, kernel = s.info(), s.dominant_kernel()
        s.set_source(loaded, F[loaded][None])
        s.run(1)
        got, tm2 = s.download()
        nonfinite = s.check_finite()
    finally:
        s.close()
    assert nonfinite == 0 and np.isfinite(got).all()
    assert got.dtype == (np.float32 if f32 else np.float64) and not tm2.any()
    hanging, anchor = H.node_classes(p["N"], p["dangling"])
    is_loaded = np.zeros(p["N"], bool)
    is_loaded[loaded] = True
    plain = is_loaded & ~hanging & ~anchor
    assert plain.sum() > p["N"] // 3 and np.abs(ref[plain]).min() > 0.4e-3
    err = np.abs(got.astype(np.float64) - ref)
    wp = _worst(err, np.abs(ref) + (~plain)[:, None], plain)
    scale = np.abs(ref).max()
    wo = _worst(err, scale, ~plain) if (~plain).any() else (0.0, -1, -1)
    print("\n[sources] %-40s %-5s plain nodes %6d worst %.3e of own value (node %d.%d) | anchors + hanging %5d worst %.3e of max (node %d.%d)"
          % (case, phase, plain.sum(), wp[0], wp[1], wp[2], (~plain).sum(), wo[0], wo[1], wo[2]))
    assert wp[0] <= (TOL_PLAIN_F32 if f32 else TOL_PLAIN), ("plain node", wp, got[wp[1]], ref[wp[1]])
    if not f32:
        assert wo[0] <= TOL_FIELD, ("anchor or hanging node", wo, got[wo[1]], ref[wo[1]], bool(hanging[wo[1]]))
    elif rounded_reference(c["mesh"], phase) is not None:
        from tests import test_gpu_step_terms as ST              # (it imports this module: not at the top)
        xref, T, B = rounded_reference(c["mesh"], phase)
        r = ST.rounded_step(got, xref, T, B, p["dangling"])
        print("[sources] %-40s %-5s float32(double step): mismatches %d, undetermined %d of %d, got != float32(ref) inside the band %d"
              % (case, phase, r["mismatches"], r["undetermined"], r["plain"], r["off_centre"]))
        ST.assert_rounded_step("%s-%s" % (case, phase), r, (kernel, "brick_units=%d" % info["brick_units"], "npatches=%d" % info["npatches"]))


# ---------------------------------------------------------------------------------------------
# B. partitions: every rank loads all it harbors
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _partition_problem(kind):
    """-> dict(nranks, make_boxes, maps(boxes), N, per-rank forces over the GLOBAL nodes, ref of the summed load)."""
    from hercules_amd import host
    if kind == "box":
        nx, ny, nz, h, dt, freq, nranks = 32, 16, 16, 20.0, 4e-4, 20.0, 2
        u = H.uniform_box(nx, ny, nz, h=h, dt=dt, freq=freq)
        lnid, node_ijk, et, nt = u["lnid"], u["node_ijk"], u["etable"], u["ntable"]
        key = lambda ijk: (np.asarray(ijk, np.int64)[:, 2] * (ny + 1) + np.asarray(ijk, np.int64)[:, 1]) * (nx + 1) + np.asarray(ijk, np.int64)[:, 0]
        lut = np.empty(len(node_ijk), np.int64)
        lut[key(node_ijk)] = np.arange(len(node_ijk))
        make_boxes = lambda: [host.Box(nx, ny, nz, h, dt, freq, rank=r, nranks=nranks) for r in range(nranks)]
        gids = lambda b: lut[key(b.node_ijk)]
        dangling = None
    else:
        nranks = 5
        p = H.two_level_mesh(16, 8, 6, 3)
        lnid, et, nt, dt, dangling = p["lnid"], p["etable"], p["ntable"], p["dt"], p["dangling"]
        make_boxes = lambda: [host.OctBox(16, 8, 6, 3, 31.25, dt, 5.0, rank=r, nranks=nranks) for r in range(nranks)]
        gids = lambda b: np.asarray(b.gid, np.int64).copy()
    N = len(nt)
    Fr = [H.rest_forces(nt[:, 0], dt, 31000 + r) for r in range(nranks)]        # rank r's force for global node g: Fr[r][g]
    boxes = make_boxes()
    maps = [gids(b) for b in boxes]
    for b in boxes:
        b.close()
    total = np.zeros((N, 3))
    for m, f in zip(maps, Fr):
        assert len(np.unique(m)) == len(m)
        total[m] += f[m]
    ref = H.oracle_step_from_rest(lnid, et, nt, dt, np.arange(N), total, dangling)
    ref.flags.writeable = False
    return dict(nranks=nranks, make_boxes=make_boxes, maps=maps, N=N, Fr=Fr, ref=ref)


@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("variant", [PATCH, SCATTER], ids=["patch", "scatter"])
@pytest.mark.parametrize("kind", ["box", "octbox"])
def test_every_rank_loads_all_its_harbored_nodes(kind, variant, overlap):
    """host.Box(32, 16, 16) on 2 ranks, host.OctBox(16, 8, 6, 3) on 5 (hanging nodes shared between ranks): the source
    through the interface launch of the patch kernels, the contribution exchange and the hanging-node schedules."""
    from hercules_amd import capi
    q = _partition_problem(kind)
    boxes = q["make_boxes"]()
    solvers = []
    try:
        for r, b in enumerate(boxes):
            s = b.create_solver(variant=variant, options={"overlap": overlap})
            solvers.append(s)
            assert s.info()["variant"] == variant
            m = q["maps"][r]
            s.set_source(np.arange(len(m), dtype=np.int32), q["Fr"][r][m][None])
        capi.group_link(solvers)
        capi.group_run(solvers, 1)
        fields = [s.download()[0] for s in solvers]
    finally:
        for s in solvers:
            s.close()
        for b in boxes:
            b.close()
    ref = q["ref"]
    scale = np.abs(ref).max()
    first = np.zeros((q["N"], 3))
    have = np.zeros(q["N"], bool)
    worst = 0.0
    for r, (m, u) in enumerate(zip(q["maps"], fields)):
        assert np.isfinite(u).all(), r
        worst = max(worst, float(np.abs(u - ref[m]).max() / scale))
        old = have[m]
        assert np.array_equal(first[m[old]].view(np.int64), u[old].view(np.int64)), ("copies of one node differ", r)
        first[m[~old]] = u[~old]
        have[m] = True
    print("\n[sources] partitions %-6s variant %d overlap %d: worst harbored copy %.3e of max" % (kind, variant, overlap, worst))
    assert have.all() and worst <= TOL_FIELD, worst


# ---------------------------------------------------------------------------------------------
# C. the window of hq_set_source
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,options", [("box32x32x16", None), ("two_level", {"no_bricks": 1})], ids=["bricks", "patches-only"])
def test_source_windows_same_nodes_rebuilds_subsets_and_the_empty_list(mesh, options):
    """hq_set_source(ids, F, step0) stage by stage, the oracle stepped along on the same state with each stage's table
    zero-padded to the whole run (its rows are indexed by the absolute step).  hq_info.device_bytes follows the tables: a
    repeated call leaves it unchanged, a subset reports less, the empty list gives back all a source ever took."""
    p = _mesh(mesh)
    N, dt = p["N"], p["dt"]
    total = 40
    every = np.arange(N, dtype=np.int32)
    rows = lambda k, seed: np.stack([H.rest_forces(p["ntable"][:, 0], dt, seed + i) for i in range(k)])     # [k, N, 3]
    o1, o2 = np.zeros((N, 3)), np.zeros((N, 3))
    state = {"step": 0}
    s = p["make"](options=options)

    def advance(n, ids, F, step0, what):
        """n steps on both sides; ids / F [k, len(ids), 3] / step0: what the ORACLE is loaded with."""
        table = np.zeros((total, len(ids), 3))
        table[step0:step0 + len(F)] = F
        ho.solver_run(p["lnid"], p["etable"], p["ntable"], o1, o2, state["step"], n, dt,
                      loaded_lnid=ids if len(ids) else None, forces=table, dangling=p["dangling"])
        s.run(n)
        state["step"] += n
        assert s.info()["step"] == state["step"] <= total
        tm1, tm2 = s.download()
        e1, e2 = H.rel_linf(tm1, o2), H.rel_linf(tm2, o1)
        print("[sources] windows %-12s %-28s step %2d: %.2e %.2e" % (mesh, what, state["step"], e1, e2))
        assert e1 < TOL_RUN and e2 < TOL_RUN, (what, e1, e2)

    try:
        bytes0 = s.info()["device_bytes"]
        # 1. a window that opens at step 2: the steps before it apply nothing
        F = rows(3, 100)
        s.set_source(every, F, step0=2)
        s.run(2)
        tm1, tm2 = s.download()
        assert not tm1.any() and not tm2.any()
        ho.solver_run(p["lnid"], p["etable"], p["ntable"], o1, o2, 0, 2, dt, dangling=p["dangling"])
        assert not o1.any() and not o2.any()
        state["step"] = 2
        # 2. steps 2 to 4 forced, 5 and 6 free
        advance(5, every, F, 2, "first window")
        # 3. the same ids, a shorter table, a later step0: only the force table travels (same_nodes)
        F = rows(2, 200)
        s.set_source(every, F, step0=8)
        advance(4, every, F, 8, "same nodes, shorter table")
        # 4. a longer table than the first: beyond the capacity, everything is rebuilt
        F = rows(5, 300)
        s.set_source(every, F, step0=11)
        advance(6, every, F, 11, "same nodes, longer table")
        # 5. the same nodes in another order, F permuted alike: other tables, the same physics (the oracle keeps its order)
        perm = np.random.default_rng(5).permutation(N)
        F = rows(3, 400)
        s.set_source(every[perm], F[:, perm], step0=17)
        bytes5 = s.info()["device_bytes"]
        s.set_source(every[perm], F[:, perm], step0=17)      # the same call again: nothing more is held
        assert s.info()["device_bytes"] == bytes5 > bytes0
        advance(4, every, F, 17, "permuted list")
        # 6. a proper subset
        sub = every[::3]
        F = rows(3, 500)[:, sub]
        s.set_source(sub, F, step0=22)
        bytes6 = s.info()["device_bytes"]
        assert bytes0 < bytes6 < bytes5
        s.set_source(sub[::-1], F[:, ::-1], step0=22)        # other ids: every table is rebuilt, the old ones are given back
        assert s.info()["device_bytes"] == bytes6
        s.set_source(sub, F, step0=22)
        assert s.info()["device_bytes"] == bytes6
        advance(5, sub, F, 22, "subset")
        # 7. the empty list: the run goes on unforced
        s.set_source(np.zeros(0, np.int32), np.zeros((0, 0, 3)))
        advance(3, np.zeros(0, np.int32), np.zeros((0, 0, 3)), 0, "empty list")
        assert s.info()["device_bytes"] == bytes0
        assert s.check_finite() == 0
    finally:
        s.close()
