"""One step from two independent fields on PARTITIONS, the reference side, on a machine without a device (the device side:
tests/test_gpu_partition_step.py, whose problems, fields, reference and bound are the ones used here).

1. The ranks' tables (tests/helpers.partition_step_problem: ho.octree_partition + ho.multi_rank_init on the RAW material
   rows): per-rank eTable and edata equal the single-rank ones bit for bit; the owners' n_t rows differ from the
   single-rank rows by the mass exchange's summation order alone (H.rel_linf <= 4e-16: measured 1.75e-16 on
   c5_gradient_branch, m0 itself bit-equal) -- which is why the reference takes the rows the ranks hold.
2. B_oracle of every problem of the device file: ho.multi_rank_run's single step (the uniform boxes: the C oracle on the
   tables assembled from the C host's partitions) against tests/helpers.extended_step, <= 64; printed.
3. Coverage conditions, so that another partition cannot hollow the device test out: owned interface nodes with more than
   one sharer (the ptr -> pos loop of hq_k_interface_update), hanging nodes with anchors owned elsewhere, dn s-records
   (hq_k_distribute on d_iforce), every material branch on every rank.
4. Mutations in the Python simulation of the exchange (ho.multi_rank_run), each of which must exceed the device bound at
   the nodes concerned -- in every copy -- and nowhere outside them and the hanging nodes that depend on them:
   two records of one c-list messenger swapped (what HQ_TEST_SWAP_RANK does); one owner's m1 at one interface node
   scaled by 1 + 1e-9; one shared hanging node's distribution skipped.
5. The m1 mutation under the criterion the partition tests used so far (one step from tm2 = tm1 + 1e-6 noise, the error
   over the field's maximum): below 1e-9 -- that criterion does not see it.
6. The f32 problems: the rounded double oracle on the global float tables meets the float criterion
   (tests/test_gpu_step_terms.rounded_step) with undetermined components under the cap (0; the stencil boxes 1 of 55 539
   and 2 of 107 811); het70x20x12's ranks pack their per-element units on float rows only without damping."""
import numpy as np
import pytest

from oracle import herc_oracle as ho
from tests import helpers as H
from tests import test_gpu_partition_step as G     # (its module-level guard skips this module too where longdouble is narrow)

EPS = G.EPS
OCT = sorted({(c["mesh"], c["nranks"], c["damping"], c["precision"]) for c in G.CASES.values() if c["kind"] == "oct"} |
             {(c["mesh"], c["nranks"], "rayleigh", c["precision"]) for c in G.PROCESS_CASES.values()})
BOX = sorted({(c["mesh"], c["nranks"], c["precision"]) for c in G.CASES.values() if c["kind"] == "box"})
OCT_F64_RAYLEIGH = sorted({(m, n) for m, n, d, pr in OCT if d == "rayleigh" and pr == "f64"})
HANGING_MESHES = {m for m, _ in OCT_F64_RAYLEIGH if m != "het70x20x12"}


def _id(t):
    return "-".join(str(v) for v in t)


# ---------------------------------------------------------------------------------------------
# 1. tables
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,nranks", OCT_F64_RAYLEIGH, ids=[_id(t) for t in OCT_F64_RAYLEIGH])
def test_rank_tables_against_the_single_rank_tables(mesh, nranks):
    q = H.partition_step_problem(mesh, nranks)
    p = H.step_mesh(mesh)
    assert np.array_equal(q["etable"], p["etable"])                                   # (het70x20x12: elements in the same order)
    for r, part in enumerate(q["parts"]):
        assert np.array_equal(q["ets"][r], p["etable"][part["elems"]]), r
        assert np.array_equal(q["edata"][r], p["edata"][part["elems"]]), r            # rewritten from raw = the single rank's
    if mesh == "het70x20x12":                       # other node numbering than ho.uniform_mesh: matched by coordinates
        key = lambda xyz: (np.asarray(xyz, np.int64) >> 20) @ np.array([1, 1 << 10, 1 << 20])
        order = np.argsort(key(p["node_xyz"]))
        single = p["ntable"][order[np.searchsorted(key(p["node_xyz"])[order], key(q["xyz"]))]]
    else:
        single = p["ntable"]
        assert np.array_equal(q["lnid"], p["lnid"])
    rel = H.rel_linf(q["ntable"], single)
    rows = float((np.abs(q["ntable"] - single) / np.abs(single).max(axis=1, keepdims=True)).max())
    print("\n[partition-step] %-20s %d ranks: owners' n_t rows against the single rank's: rel_linf %.3e, of the row's largest %.3e; m0 equal: %s"
          % (mesh, nranks, rel, rows, np.array_equal(q["ntable"][:, 0], single[:, 0])))
    assert rel <= 4e-16
    assert rows <= 8 * 2.0 ** -53                   # eight elements' terms in another order


# ---------------------------------------------------------------------------------------------
# 2. B_oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,nranks,damping,precision", OCT, ids=[_id(t) for t in OCT])
def test_partitioned_oracle_step_against_the_extended_reference(mesh, nranks, damping, precision):
    q = H.partition_step_problem(mesh, nranks, damping, precision)
    u1, u2 = q["u1"], q["u2"]
    hanging, _ = H.node_classes(q["N"], q["dangling"])
    assert u1.dtype == q["ntable"].dtype == q["oracle"][0].dtype == q["real"]
    assert min(np.abs(u1[~hanging]).min(), np.abs(u2[~hanging]).min()) >= 0.5e-3 * (1 - 1e-6)
    assert np.abs(u1 - u2).max() > 1.5e-3
    print("\n[partition-step] B_oracle %-20s %d ranks %-8s %s %.2f%s" % (mesh, nranks, damping, precision, q["B_oracle"],
                                                                          " (of 2^-24 T)" if precision == "f32" else ""))
    assert np.isfinite(q["B_oracle"]) and q["B_oracle"] <= 64.0
    assert G.bound_factor(q) == 64.0 or precision == "f32"
    have = np.zeros(q["N"], bool)
    for g in q["gid"]:
        have[g] = True
    assert have.all()


@pytest.mark.parametrize("shape,nranks,precision", BOX, ids=[_id(t) for t in BOX])
def test_box_oracle_step_against_the_extended_reference(shape, nranks, precision):
    q = H.box_step_problem(shape, nranks, precision)
    print("\n[partition-step] B_oracle box %s %d ranks %s %.2f" % ("x".join(map(str, shape)), nranks, precision, q["B_oracle"]))
    assert np.isfinite(q["B_oracle"]) and q["B_oracle"] <= 64.0
    # the C host's partitions carry the single rank's rows: the same homogeneous sums on every rank
    single = H.uniform_box(*shape, h=H.BOX_STEP["h"], dt=q["dt"], freq=H.BOX_STEP["freq"])
    assert np.array_equal(q["etable"], single["etable"])
    if precision == "f64":
        assert H.rel_linf(q["ntable"], single["ntable"]) <= 4e-16


F32_PROBLEMS = [("oct",) + t for t in OCT if t[3] == "f32"] + [("box",) + t for t in BOX if t[2] == "f32"]


@pytest.mark.parametrize("problem", F32_PROBLEMS, ids=[_id(t) for t in F32_PROBLEMS])
def test_rounded_double_step_meets_the_float_criterion_on_the_partitioned_problems(problem):
    """The float cases' criterion (tests/test_gpu_step_terms.rounded_step) is satisfiable on every f32 problem of the device
    file: the double oracle on the widened global float tables and fields, rounded once, hanging nodes assigned from the
    stored floats -- no mismatch, exact hanging sums, undetermined components under the cap."""
    ST = G.ST
    q = (H.partition_step_problem(*problem[1:]) if problem[0] == "oct" else H.box_step_problem(*problem[1:]))
    wide = lambda a: np.ascontiguousarray(a, np.float64)
    o1, o2 = wide(q["u2"]), wide(q["u1"])
    ho.solver_run(np.ascontiguousarray(q["lnid"], np.int32), q["etable"], wide(q["ntable"]), o1, o2, 0, 1, q["dt"],
                  damping=q.get("kind", ho.DAMP_RAYLEIGH), dangling=q["dangling"])
    got = o2.astype(np.float32)
    if q["dangling"] is not None:
        ids, want, _ = ST.hanging_assignment(got, q["dangling"])
        got[ids] = want
    r = ST.rounded_step(got, q["ref"], q["T"], G.bound_factor(q), q["dangling"])
    print("\n[partition-step] float32(double oracle) %-40s mismatches %d, undetermined %d of %d (cap %d)"
          % (_id(problem[1:]), r["mismatches"], r["undetermined"], r["plain"], int(ST.UNDETERMINED_CAP * r["plain"])))
    ST.assert_rounded_step(_id(problem[1:]), r, "float32(double oracle)")


@pytest.mark.parametrize("damping", ["rayleigh", "none"])
def test_float_rows_pack_only_without_damping_on_the_het_partitions(damping):
    """What the f32 het70x20x12 cases on 3 ranks assert from hq_info, from the planner's host-only check on the ranks' float
    rows: every per-element unit packs without damping, none with Rayleigh damping (ST.float_rows_pack)."""
    from hercules_amd import capi
    q = H.partition_step_problem("het70x20x12", 3, damping, "f32")
    reps = [capi.brick_plan_check(H.rank_desc(q, r, pack=True)) for r in range(3)]
    assert all(b["faults"] == 0 and b["het_units"] > 0 for b in reps), reps
    assert [b["packed_units"] for b in reps] == [b["het_units"] if G.ST.float_rows_pack(damping) else 0 for b in reps], reps


def test_box_partitions_have_bricks_and_stencil_patches_on_every_rank():
    """The planner's host-only checks on the boxes of the device cases.  BOX_BRICKS: brick nodes on every rank, on 2 and on
    8 ranks (behind bricks the shell's patches are element-form ones on every size tried up to 64 x 64 x 32: no stencil
    patch on the interface there).  BOX_STENCIL, planned without bricks as no_bricks = 1 does: lattice-subset tables on
    every rank, and a rank that owns interface nodes has nothing else -- hq_k_patch_stencil's launch ahead of the exchange."""
    for nranks in (2, 8):
        boxes = H.box_step_boxes(G.BOX_BRICKS, nranks)
        try:
            plans = [b.brick_plan_check() for b in boxes]
        finally:
            for b in boxes:
                b.close()
        assert all(bp["faults"] == 0 and bp["brick_nodes"] > 0 and bp["patch_nodes"] > 0 for bp in plans), (nranks, plans)
    for nranks, shape in G.BOX_STENCIL.items():
        q = H.box_step_problem(shape, nranks)
        owns = [any(k.startswith("owned-interface") for k in kinds) for kinds in G.node_kinds(q)]
        boxes = H.box_step_boxes(shape, nranks)
        try:
            plans = [b.stencil_plan_check() for b in boxes]
        finally:
            for b in boxes:
                b.close()
        assert all(st["faults"] == 0 and st["tables"] > 0 for st in plans), (nranks, plans)
        assert any(o and st["tables"] == st["patches"] for o, st in zip(owns, plans)), (nranks, owns, plans)


# ---------------------------------------------------------------------------------------------
# 3. coverage
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,nranks", OCT_F64_RAYLEIGH, ids=[_id(t) for t in OCT_F64_RAYLEIGH])
def test_the_partitions_reach_what_the_device_cases_are_about(mesh, nranks):
    q = H.partition_step_problem(mesh, nranks)
    cl = H.partition_classes(q)
    multi = [int((c["sharers"] > 1).sum()) for c in cl]
    far = [int((np.asarray(p["owner"])[np.asarray(p["dangling"][2])] != r).sum()) if len(p["dangling"][0]) else 0
           for r, p in enumerate(q["parts"])]
    dn_s = sum(len(m) for p in q["parts"] for _, m in p["dn_sched"]["s"])
    print("\n[partition-step] %-20s %d ranks: owned interface nodes %s, with several sharers %s (most sharers %d), anchors owned elsewhere %s, dn s-records %d"
          % (mesh, nranks, [int(c["interface"].sum()) for c in cl], multi, max(int(c["sharers"].max()) for c in cl), far, dn_s))
    assert sum(int(c["interface"].sum()) for c in cl) > 0
    if mesh in HANGING_MESHES:
        assert max(multi) >= 8 and max(far) >= 1 and dn_s > 0
    if q["labels"] is not None:
        for r, p in enumerate(q["parts"]):
            for k in H.BRANCHES:
                assert q["labels"][k][p["elems"]].mean() >= 0.08, (r, k)


# ---------------------------------------------------------------------------------------------
# 4. mutations
# ---------------------------------------------------------------------------------------------
def _step(q, parts=None, nts=None, distribute=None, u1=None, u2=None):
    """ho.multi_rank_run's single step of the problem with pieces replaced -> per-rank new displacement."""
    u1, u2 = (q["u1"] if u1 is None else u1), (q["u2"] if u2 is None else u2)
    o1, o2 = [np.ascontiguousarray(u2[g]) for g in q["gid"]], [np.ascontiguousarray(u1[g]) for g in q["gid"]]
    n = q["nranks"]
    ho.multi_rank_run(parts or q["parts"], q["ets"], nts or q["nts"], o1, o2, 0, 1, q["dt"], [[]] * n, [None] * n, distribute=distribute)
    return o2


def _tripped(q, fields, B):
    """(global nodes at which SOME copy exceeds the device bound, those at which EVERY copy does)."""
    some, every = np.zeros(q["N"], bool), np.ones(q["N"], bool)
    for g, u in zip(q["gid"], fields):
        bad = (np.abs(u - q["ref"][g]) > B * EPS * q["T"][g]).any(axis=1)
        some[g] |= bad
        every[g] &= bad
    return set(np.nonzero(some)[0].tolist()), set(np.nonzero(some & every)[0].tolist())


def _dependants(q, nodes):
    """The hanging nodes (global) that have one of `nodes` for an anchor."""
    ids, ptr, anc = [np.asarray(a, np.int64) for a in q["dangling"]]
    hit = np.isin(anc, sorted(nodes))
    return set(ids[np.unique(np.searchsorted(ptr, np.nonzero(hit)[0], side="right") - 1)].tolist())


def _mutable(part):
    return dict(part, an_sched={k: [(peer, np.array(m)) for peer, m in v] for k, v in part["an_sched"].items()})


@pytest.fixture(scope="module")
def problem():
    q = H.partition_step_problem("c5_gradient_branch", 8)
    B = G.bound_factor(q)
    assert B == 64.0 and _tripped(q, q["oracle"], B) == (set(), set())
    return q, B


def test_swapped_records_trip_the_bound_at_their_nodes_only(problem):
    q, B = problem
    cl = H.partition_classes(q)
    # a rank that sends two records to an owner for whom both nodes have several sharers: the pos loop's nodes
    pick = None
    for part in q["parts"]:
        for k, (owner, m) in enumerate(part["an_sched"]["c"]):
            theirs = {int(g): i for i, g in enumerate(q["gid"][owner])}
            for a in range(len(m) - 1):
                ga, gb = int(part["nodes"][m[a]]), int(part["nodes"][m[a + 1]])
                if cl[owner]["sharers"][theirs[ga]] > 1 and cl[owner]["sharers"][theirs[gb]] > 1 and pick is None:
                    pick = (part["rank"], k, a, owner, ga, gb)
    assert pick is not None
    r, k, a, owner, ga, gb = pick
    parts = [_mutable(p) if p["rank"] == r else p for p in q["parts"]]
    parts[r]["an_sched"]["c"][k][1][[a, a + 1]] = parts[r]["an_sched"]["c"][k][1][[a + 1, a]]
    some, every = _tripped(q, _step(q, parts=parts), B)
    print("\n[partition-step] rank %d's records %d, %d to rank %d swapped (nodes %d, %d): tripped %s" % (r, a, a + 1, owner, ga, gb, sorted(some)))
    assert {ga, gb} <= every                                     # the owner's sum is wrong, and every copy carries it
    assert some <= {ga, gb} | _dependants(q, {ga, gb})


def test_one_m1_at_an_interface_node_trips_the_bound_there_only_and_passes_the_old_criterion(problem):
    q, B = problem
    cl = H.partition_classes(q)
    r = int(np.argmax([int((c["sharers"] > 1).sum()) for c in cl]))
    i = int(np.nonzero((cl[r]["sharers"] > 1) & ~cl[r]["hanging"])[0][0])
    g = int(q["gid"][r][i])
    nts = [np.array(nt) for nt in q["nts"]]
    nts[r][i, 4:7] *= 1.0 + 1e-9
    some, every = _tripped(q, _step(q, nts=nts), B)
    print("\n[partition-step] m1 (1 + 1e-9) at rank %d's node %d (global %d, %d sharers): tripped %s" % (r, i, g, cl[r]["sharers"][i], sorted(some)))
    assert {g} <= every and some <= {g} | _dependants(q, {g})
    # the old criterion: one step from tm2 = tm1 + 1e-6 * noise, the error over the field's maximum
    rng = np.random.default_rng(99)
    v1 = rng.uniform(-1, 1, (q["N"], 3)) * 1e-3
    v2 = v1 + rng.uniform(-1, 1, (q["N"], 3)) * 1e-6
    ho.compute_adjust(v1, 1, q["dangling"])
    ho.compute_adjust(v2, 1, q["dangling"])
    ref, _ = H.extended_step(q["lnid"], q["etable"], q["ntable"], v1, v2, q["dangling"])
    old = max(H.rel_linf(u, ref[gid].astype(np.float64)) for u, gid in zip(_step(q, nts=nts, u1=v1, u2=v2), q["gid"]))
    clean = max(H.rel_linf(u, ref[gid].astype(np.float64)) for u, gid in zip(_step(q, u1=v1, u2=v2), q["gid"]))
    print("[partition-step] the same m1 under the old criterion (rel_linf after one step from tm2 = tm1 + 1e-6 noise): %.3e (unmutated %.3e)" % (old, clean))
    assert clean < old < 1e-9


def test_a_skipped_distribution_trips_the_bound_at_the_anchors_only(problem):
    q, B = problem
    # a hanging node other ranks contribute to (a dn s-record: on the device hq_k_distribute's, not the patch kernels')
    r = int(np.argmax([sum(len(m) for _, m in p["dn_sched"]["s"]) for p in q["parts"]]))
    part = q["parts"][r]
    ids, ptr, anc = [np.asarray(a) for a in part["dangling"]]
    shared = set(int(i) for _, m in part["dn_sched"]["s"] for i in m)
    k = next(k for k, i in enumerate(ids) if int(i) in shared)
    keep = np.arange(len(ids)) != k
    deps = np.diff(ptr)
    short = (ids[keep], np.concatenate([[0], np.cumsum(deps[keep])]).astype(np.int32), anc[np.repeat(keep, deps)])
    distribute = [short if p["rank"] == r else p["dangling"] for p in q["parts"]]
    anchors = set(int(g) for g in part["nodes"][anc[ptr[k]:ptr[k + 1]]])
    some, every = _tripped(q, _step(q, distribute=distribute), B)
    print("\n[partition-step] rank %d's hanging node %d (global %d) not distributed to its anchors %s: tripped %s"
          % (r, ids[k], part["nodes"][ids[k]], sorted(anchors), sorted(some)))
    assert anchors <= every and some <= anchors | _dependants(q, anchors)
    assert int(part["nodes"][ids[k]]) in some                     # itself the mean of those anchors
