"""Source forces on EVERY node, the reference side, on a machine without a device: what the oracle's own single step
from rest leaves at a loaded node, class by class.  A per-node comparison of the stepping kernels' source lookups
(docs/LABNOTES.md, "Source forces on every node") takes its bounds from these figures.

From zero arrays every stiffness and damping sum is exactly zero, so solver_compute_displacement (psolve.c:4072-4114)
sees f = F * dt^2 + 0 and leaves f / n_t[n][0]: a node's result depends on its own force only.  A loaded hanging node
hands F * dt^2 / deps to each of its anchors (compute_adjust DISTRIBUTION, psolve.c:5936-6039) and then takes the
mean of their displacements (ASSIGNMENT)."""
import numpy as np
import pytest

from oracle import herc_oracle as ho
from tests import helpers as H


def _uniform():
    return H.source_mesh("box32x32x16")


def _two_level():
    return H.source_mesh("two_level")


def _edge(name):
    return lambda: H.source_mesh(name)


# (edge66x10x2, hetedge65x9x8: the degenerate-footprint meshes tests/test_gpu_brick_edges.py loads on every node)
@pytest.mark.parametrize("mesh", [_uniform, _two_level, _edge("edge66x10x2"), _edge("hetedge65x9x8")],
                         ids=["uniform", "two_level", "edge66x10x2", "hetedge65x9x8"])
def test_a_plain_loaded_node_is_its_force_over_its_mass_bit_for_bit(mesh):
    """Every node loaded (hanging ones too, where there are any): at every node that is neither hanging nor an anchor --
    dashpot faces included, their n_t rows differ per axis but column 0 is the divisor -- u(1) == F * dt^2 / n_t[n][0],
    the same two roundings in the same order."""
    p = mesh()
    N, dt = p["N"], p["dt"]
    F = H.rest_forces(p["ntable"][:, 0], dt, 20240)
    u = H.oracle_step_from_rest(p["lnid"], p["etable"], p["ntable"], dt, np.arange(N), F, p["dangling"])
    hanging, anchor = H.node_classes(N, p["dangling"])
    plain = ~hanging & ~anchor
    assert plain.sum() > N // 2 and np.isfinite(u).all()
    want = (F * (dt * dt)) / p["ntable"][:, :1]
    assert np.array_equal(u[plain], want[plain])
    assert np.abs(want[plain]).min() >= 0.49e-3 and np.abs(want[plain]).max() <= 1.01e-3


@pytest.mark.parametrize("hanging_loaded", [False, True])
def test_anchors_take_their_hanging_nodes_share_and_hanging_nodes_the_mean(hanging_loaded):
    """two_level_mesh(16, 8, 6, 3), 108 hanging nodes: an anchor ends at (F_a + sum F_h / deps_h) * dt^2 / m to
    1e-14 of the field's maximum (the oracle adds the rounded shares one by one), a hanging node at the mean of its
    anchors, summed in the table's order: bit for bit."""
    p = _two_level()
    N, dt = p["N"], p["dt"]
    ids, ptr, anc = [np.asarray(a, np.int64) for a in p["dangling"]]
    hanging, anchor = H.node_classes(N, p["dangling"])
    assert hanging.sum() == 108 and not (hanging & anchor).any()
    F = H.rest_forces(p["ntable"][:, 0], dt, 20241)
    loaded = np.arange(N) if hanging_loaded else np.nonzero(~hanging)[0]
    u = H.oracle_step_from_rest(p["lnid"], p["etable"], p["ntable"], dt, loaded, F[loaded], p["dangling"])
    deps = np.diff(ptr)
    total = F.copy()
    total[hanging] = 0.0
    if hanging_loaded:
        np.add.at(total, anc, np.repeat(F[ids] / deps[:, None], deps, axis=0))
    closed = total * (dt * dt) / p["ntable"][:, :1]
    scale = np.abs(closed).max()
    assert np.abs(u[anchor] - closed[anchor]).max() <= 1e-14 * scale
    assert np.array_equal(u[~anchor & ~hanging], closed[~anchor & ~hanging])
    mean = np.zeros((len(ids), 3))
    for j in range(int(deps.max())):
        has = deps > j
        mean[has] += u[anc[ptr[:-1][has] + j]] / deps[has, None]
    assert np.array_equal(u[ids], mean)
    assert np.abs(u[ids]).max() > 0


@pytest.mark.parametrize("kind", ["box-2", "octbox-5"])
def test_ranks_that_each_load_all_they_harbor_sum_to_the_single_rank_run(kind):
    """As in the reference, every rank loads ALL of its harbored nodes -- owned, merely harbored, hanging -- with forces
    of its own; the contribution exchanges sum them at the owners.  ho.multi_rank_run on octor's partitions -- the
    32 x 16 x 16 uniform box on 2 ranks (as one octree level), the two-level box on 5 -- against the single-rank run
    loaded with the sum over ranks: within 1e-14 of the field's maximum at every harbored copy (the sums are taken in
    another order), and the copies of one node, of which there are many, are the owner's value bit for bit."""
    if kind == "box-2":
        p, nranks = H.two_level_mesh(32, 16, 16, 0, h_fine=20.0, dt=4e-4, freq=20.0), 2
        assert len(p["dangling"][0]) == 0 and p["N"] == 33 * 17 * 17
    else:
        p, nranks = _two_level(), 5
    N, dt = p["N"], p["dt"]
    m = p["mesh"]
    parts = ho.octree_partition(m, nranks, list(p["far"]))
    eds = [np.ascontiguousarray(p["edata"][q["elems"]]) for q in parts]
    fcs = [np.ascontiguousarray(m["face"][q["elems"]]) for q in parts]
    ets, nts = ho.multi_rank_init(parts, eds, fcs, dt, p["freq"])
    Fr = [H.rest_forces(p["ntable"][:, 0], dt, 977 + r) for r in range(nranks)]
    total = np.zeros((N, 3))
    for q, f in zip(parts, Fr):
        total[q["nodes"]] += f[q["nodes"]]
    ref = H.oracle_step_from_rest(p["lnid"], p["etable"], p["ntable"], dt, np.arange(N), total, p["dangling"])
    tm1s = [np.zeros((len(q["nodes"]), 3)) for q in parts]
    tm2s = [np.zeros((len(q["nodes"]), 3)) for q in parts]
    ho.multi_rank_run(parts, ets, nts, tm1s, tm2s, 0, 1, dt, [np.arange(len(q["nodes"]), dtype=np.int32) for q in parts],
                      [f[q["nodes"]][None] for q, f in zip(parts, Fr)])
    scale = np.abs(ref).max()
    first, have, shared = np.zeros((N, 3)), np.zeros(N, bool), 0
    for q, u in zip(parts, tm2s):
        g = np.asarray(q["nodes"], np.int64)
        assert np.isfinite(u).all()
        assert np.abs(u - ref[g]).max() <= 1e-14 * scale, q["rank"]
        old = have[g]
        shared += int(old.sum())
        assert np.array_equal(first[g[old]].view(np.int64), u[old].view(np.int64)), q["rank"]
        first[g[~old]] = u[~old]
        have[g] = True
    assert have.all() and shared >= (17 * 17 if kind == "box-2" else 100)      # copies on more than one rank exist


# the planner's counters the device cases of tests/test_gpu_sources.py rely on, from the host-only plan checks: a planner
# change that takes a kernel away from one of these meshes shows here, on a machine without a device
def _plans(monkeypatch, name, **env):
    from hercules_amd import capi
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    d = H.solver_desc(H.source_mesh(name))
    out = capi.brick_plan_check(d), capi.plan_check(d), capi.stencil_plan_check(d)
    for k in env:
        monkeypatch.delenv(k)
    assert all(r["faults"] == 0 for r in out), (name, env, out)
    return out


_RAGGED_ENV = {"HQ_BRICK_" + k[len("brick_"):].upper(): v for k, v in H.RAGGED_PLAN.items()}


@pytest.mark.parametrize("name,wide", [("box32x32x16", 31), ("box70x20x12", 64)])
def test_planner_counters_of_the_uniform_source_meshes(name, wide, monkeypatch):
    """hq_k_brick with both z faces riding (nz + 1 planes), whole 64-wide tiles in x and the partial tile in y; more units
    with brick_cz = 5; n_t rows of their own with brick_no_ntsame = 1 (the face planes then stay with the patches)."""
    nx, ny, nz = H.source_mesh(name)["shape"]
    b, _, _ = _plans(monkeypatch, name)
    assert b["brick_nodes"] == wide * (ny - 1) * (nz + 1) and b["units_one_nt_row"] == b["units"] > 0 and b["het_units"] == 0
    assert 2 * b["brick_nodes"] > H.source_mesh(name)["N"]                     # hq_dominant_kernel: hq_k_brick
    c, _, _ = _plans(monkeypatch, name, HQ_BRICK_CZ=5)
    assert c["units"] > b["units"] and c["brick_nodes"] == b["brick_nodes"]
    n, _, _ = _plans(monkeypatch, name, HQ_BRICK_NO_NTSAME=1)
    assert n["units"] > 0 and n["units_one_nt_row"] == 0 and n["het_units"] == 0 and 2 * n["brick_nodes"] > H.source_mesh(name)["N"]


def test_planner_counters_of_the_per_element_and_ragged_source_meshes(monkeypatch):
    r1, _, _ = _plans(monkeypatch, "two_material", HQ_BRICK_RAGGED=1)
    r0, _, _ = _plans(monkeypatch, "two_material", HQ_BRICK_RAGGED=0)
    assert r1["ragged_units"] >= 8 and r1["het_units"] == 0 and r0["ragged_units"] == 0 and r0["het_units"] > 0
    lat, _, _ = _plans(monkeypatch, "lateral")
    assert lat["het_units"] == lat["units"] > 0
    basin, _, _ = _plans(monkeypatch, "c5_basin", **_RAGGED_ENV)
    grad, _, _ = _plans(monkeypatch, "c5_gradient", **_RAGGED_ENV)
    assert basin["ragged_units"] >= 2 and grad["ragged_het_units"] >= 2 and grad["het_units"] >= grad["ragged_het_units"]


def test_planner_counters_of_the_patches_only_source_meshes(monkeypatch):
    b, p, st = _plans(monkeypatch, "box32", HQ_NO_BRICKS=1)
    assert b["brick_nodes"] == 0 and p["patches"] == 64 and p["lattice_patches"] == 8
    assert st["tables"] == 64 and st["full_lattices"] == 8                      # every patch a lattice subset, far faces included
    b, p, st = _plans(monkeypatch, "two_level", HQ_NO_BRICKS=1)
    assert b["brick_nodes"] == 0 and p["patches"] > st["tables"]                 # element-form patches exist
