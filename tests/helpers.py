"""Shared set-up of the reference's examples/simple case (C1) from the golden
fixtures: mesh in octor order, eTable/nTable from the oracle's solver_init."""
import os
import re

import numpy as np

from oracle import herc_oracle as ho

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# octor root: 1000 m x 1000 m x 500 m -> farendp = (2^30, 2^30, 2^29) ticks (octor.c:4120-4140)
C1_FAR_TICKS = (2 ** 30, 2 ** 30, 2 ** 29)
C1_NX, C1_NY, C1_NZ = 16, 16, 8
C1_H = 62.5
C1_STATIONS = [(500.0 + 100.0 * i, 500.0 + 100.0 * i, 100.0) for i in range(5)]


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def c1_mesh():
    g = load("c1_short")
    lnid, node_ijk, elem_ijk, edge = ho.mesh_from_elem_ticks(g["elem_ticks"], C1_FAR_TICKS)
    mat = g["mat_vs_vp_rho"]
    edata = np.empty((len(lnid), 4), np.float32)
    edata[:, 0] = np.float32(1000.0 / 2 ** 30 * edge)
    edata[:, 1] = mat[:, 1]
    edata[:, 2] = mat[:, 0]
    edata[:, 3] = mat[:, 2]
    return lnid, node_ijk, elem_ijk, edata


def c1_problem(damping="rayleigh", real=np.float64):
    """real: solver_float (psolve.h:60-64) -- float32 = the tables as the reference's -DSINGLE_PRECISION_SOLVER build sums them."""
    lnid, node_ijk, elem_ijk, edata = c1_mesh()
    face = ho.face_bits(elem_ijk, C1_NX, C1_NY, C1_NZ)
    etable, ntable = ho.solver_init(lnid, edata.copy(), face, len(node_ijk), 1e-3, 5.0,
                                    damping=ho.DAMPING_BY_NAME[damping], real=real)
    return dict(lnid=lnid, node_ijk=node_ijk, elem_ijk=elem_ijk, edata=edata, face=face,
                etable=etable, ntable=ntable, N=len(node_ijk), E=len(lnid), dt=1e-3,
                damping=ho.DAMPING_BY_NAME[damping])


def rel_linf(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


def c5_problem(name="c5_two_level", real=np.float64):
    """One of the reference's own octree meshes (c5_two_level: soft layer refined one level
    deeper, 800 hanging nodes; c5_three_level: three element sizes and three materials that
    take every branch of mu_and_lambda) rebuilt from its flat dump, with eTable / nTable as
    solver_init leaves them (incl. the hanging-node mass distribution, psolve.c:3498-3507)."""
    g = load(name)
    m = ho.octree_mesh_from_elem_ticks(g["elem_ticks"], C1_FAR_TICKS)
    E, N = len(m["lnid"]), len(m["node_q"])
    mat = g["mat_vs_vp_rho"]
    tick = 1000.0 / 2 ** 30
    edata = np.empty((E, 4), np.float32)
    edata[:, 0] = (tick * m["emin"] * m["elem_size"].astype(np.float64)).astype(np.float32)
    edata[:, 1], edata[:, 2], edata[:, 3] = mat[:, 1], mat[:, 0], mat[:, 2]
    etable, ntable = ho.solver_init(m["lnid"], edata, m["face"], N, 1e-3, float(g["freq"]), real=real)
    ho.compute_adjust(ntable, 0, m["dangling"])
    return dict(lnid=m["lnid"], node_q=m["node_q"], etable=etable, ntable=ntable, dangling=m["dangling"],
                N=N, E=E, dt=1e-3, emin=m["emin"], golden=g, elem_size=m["elem_size"], edata=edata, freq=float(g["freq"]))


def c5_material(p):
    """(bBase, threshold_damping, threshold_vpvs) that c5_problem's solver_init combined p["edata"] with: hq_desc.mat_*."""
    return (ho.setab(p["freq"], ho.DAMP_RAYLEIGH)[1], 0.05, 3.0)


def two_level_mesh(nx, ny, nz_fine, nz_coarse, soft=(3000.0, 1732.0, 2200.0), hard=(6000.0, 3464.0, 2700.0),
                   h_fine=31.25, dt=1e-3, freq=5.0):
    """A layered box meshed on two octree levels, in octor's conventions: the top
    nz_fine layers of fine elements (nx x ny, edge h) over nz_coarse layers of elements of
    edge 2h -- the shape the reference's mesher produced for tests/golden/c5_two_level
    (where this construction is pinned bit-for-bit).  nx, ny, nz_fine even.
    -> dict like c5_problem()."""
    assert nx % 2 == 0 and ny % 2 == 0 and nz_fine % 2 == 0
    corners = np.array([[(c >> 0) & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)], np.int64)
    fi, fj, fk = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz_fine), indexing="ij")
    fine_ll = np.stack([fi.ravel(), fj.ravel(), fk.ravel()], 1).astype(np.int64)
    ci, cj, ck = np.meshgrid(np.arange(nx // 2), np.arange(ny // 2), np.arange(nz_coarse), indexing="ij")
    coarse_ll = np.stack([2 * ci.ravel(), 2 * cj.ravel(), nz_fine + 2 * ck.ravel()], 1).astype(np.int64)
    ll = np.concatenate([fine_ll, coarse_ll])
    size = np.concatenate([np.ones(len(fine_ll), np.int64), 2 * np.ones(len(coarse_ll), np.int64)])
    order = np.argsort(ho.zvalue(ll[:, 0], ll[:, 1], ll[:, 2]), kind="stable")   # octree pre-order
    ll, size = ll[order], size[order]
    ticks = ll[:, None, :] + corners[None, :, :] * size[:, None, None]
    far = (nx, ny, nz_fine + 2 * nz_coarse)
    m = ho.octree_mesh_from_elem_ticks(ticks, far)
    E, N = len(m["lnid"]), len(m["node_q"])
    edata = np.empty((E, 4), np.float32)
    edata[:, 0] = (h_fine * m["elem_size"]).astype(np.float32)
    is_fine = m["elem_size"] == 1
    for col, (a, b) in enumerate(zip(soft, hard)):
        edata[:, 1 + col] = np.where(is_fine, a, b)
    etable, ntable = ho.solver_init(m["lnid"], edata, m["face"], N, dt, freq)
    ho.compute_adjust(ntable, 0, m["dangling"])
    return dict(lnid=m["lnid"], node_q=m["node_q"], etable=etable, ntable=ntable, dangling=m["dangling"],
                N=N, E=E, dt=dt, emin=1, mesh=m, edata=edata, far=far, freq=freq)


def c5_np8_problem(name="c5_two_level_np8", real=np.float64):
    """One of the reference's octree meshes on several MPI ranks (c5_two_level_np8; c5_basin_np8 /
    c5_basin_np5: the laterally refined basin): octor's per-rank tables restated
    from the global view (ho.octree_partition), per-rank eTable / nTable after the mass
    exchange, the reference's per-rank force files and checkpoint stripes."""
    g = load(name)
    base = load(str(g["base"]))
    nranks = int(g["nranks"])
    m = ho.octree_mesh_from_elem_ticks(base["elem_ticks"], C1_FAR_TICKS)
    far_q = [f // m["emin"] for f in C1_FAR_TICKS]
    parts = ho.octree_partition(m, nranks, far_q)
    mat = base["mat_vs_vp_rho"]
    tick = 1000.0 / 2 ** 30
    E = len(m["lnid"])
    edata = np.empty((E, 4), np.float32)
    edata[:, 0] = (tick * m["emin"] * m["elem_size"].astype(np.float64)).astype(np.float32)
    edata[:, 1], edata[:, 2], edata[:, 3] = mat[:, 1], mat[:, 0], mat[:, 2]
    eds = [np.ascontiguousarray(edata[p["elems"]]) for p in parts]
    fcs = [np.ascontiguousarray(m["face"][p["elems"]]) for p in parts]
    ets, nts = ho.multi_rank_init(parts, eds, fcs, 1e-3, float(base["freq"]), real=real)
    return dict(golden=g, base=base, mesh=m, parts=parts, ets=ets, nts=nts, dt=1e-3, nranks=nranks, edata=edata,
                loaded=[g["loaded_lnid_%d" % r] for r in range(nranks)],
                forces=[g["forces_%d" % r] for r in range(nranks)])


# the material databases tests/golden/make_golden.py wrote with oracle/make_cvm (level-4 octants of 62.5 m), as grids in the
# MESH's axes [k][y][x]: cvm_query(east = y, north = x) (psolve.c:1352), so make_cvm's octant index i runs along mesh y
CVM_MODELS = {
    "c5_two_level": dict(layers=[(0, 3000, 1732, 2200), (2, 6000, 3464, 2700)], vscut=500, freq=5.0),
    "c5_three_level": dict(layers=[(0, 1500, 150, 1800), (2, 2500, 2000, 2300), (4, 6000, 3464, 2700)], vscut=100, freq=0.25),
    "c5_layered": dict(layers=[(0, 800, 200, 1700), (1, 1500, 450, 2000), (3, 2600, 1200, 2300)], vscut=100, freq=0.5),
    "c5_basin": dict(background=(6000, 3464, 2700), vscut=100, freq=5.0,
                     regions=[("dip", 3.2, -0.3, -0.12, 3000, 1732, 2200), ("box", 12, 16, 9, 13, 0, 2, 1500, 866, 1800)]),
    # the same basin with a velocity gradient (make_cvm's `grad`): a material of its own in every database octant
    "c5_gradient": dict(background=(6000, 3464, 2700), vscut=100, freq=5.0,
                        regions=[("dip", 3.2, -0.3, -0.12, 3000, 1732, 2200), ("box", 12, 16, 9, 13, 0, 2, 1500, 866, 1800),
                                 ("grad", 0.10, -0.06, 0.12)]),
}


def cvm_grid(name, level=4):
    """-> vp, vs, rho [nz][ny][nx] float32 (mesh axes), cell edge in metres."""
    spec = CVM_MODELS[name]
    n, nz = 1 << level, 1 << (level - 1)
    k, i, j = np.meshgrid(np.arange(nz), np.arange(n), np.arange(n), indexing="ij")     # [k][mesh y = i][mesh x = j]
    out = [np.zeros((nz, n, n), np.float32) for _ in range(3)]
    if "layers" in spec:
        for k0, vp, vs, rho in spec["layers"]:
            for a, v in zip(out, (vp, vs, rho)):
                a[k >= k0] = v
    else:
        for a, v in zip(out, spec["background"]):
            a[:] = v
        grade = None
        for r in spec["regions"]:
            if r[0] == "grad":               # make_cvm.c: evaluated in double, the products rounded to float
                grade = 1.0 + r[1] * (i + 0.5) / n + r[2] * (j + 0.5) / n + r[3] * (k + 0.5) / nz
                continue
            if r[0] == "box":
                sel = (i >= r[1]) & (i < r[2]) & (j >= r[3]) & (j < r[4]) & (k >= r[5]) & (k < r[6])
                mat = r[7:]
            else:
                sel = k + 0.5 < r[1] + r[2] * (i + 0.5) + r[3] * (j + 0.5)
                mat = r[4:]
            for a, v in zip(out, mat):
                a[sel] = v
        if grade is not None:
            out[0] = (out[0].astype(np.float64) * grade).astype(np.float32)
            out[1] = (out[1].astype(np.float64) * grade).astype(np.float32)
            out[2] = (out[2].astype(np.float64) * (1.0 + (grade - 1.0) / 2.0)).astype(np.float32)
    return out[0], out[1], out[2], 1000.0 / n


def np8_stripe(g, step, rank, n):
    """(tm2, tm1) of one rank from its raw checkpoint stripe (io_checkpoint.c:93-118)."""
    s = g["ckpt%d_stripe_%d" % (int(step), rank)]
    return s[:3 * n].reshape(n, 3), s[3 * n:6 * n].reshape(n, 3)


# ---------------------------------------------------------------------------------------------
# dependency-cone windows of an octree mesh (oracle parity at sizes the oracle cannot run whole): oracle/windows.py
# ---------------------------------------------------------------------------------------------
from oracle.windows import hanging_kinds, lateral_windows, octree_window, octree_window_oracle    # noqa: E402,F401


def lap_timer(name):
    """-> lap(what): with HQ_TEST_LAPS=1 prints where a long test's time goes (stderr; run pytest with -s)."""
    import os
    import sys
    import time
    t = [time.time()]

    def lap(what):
        if os.environ.get("HQ_TEST_LAPS"):
            now = time.time()
            sys.stderr.write("  [%s] %-40s %7.1f s\n" % (name, what, now - t[0]))
            t[0] = now
    return lap


def two_material_leaves(nx=128, ny=32, nz=32, split=37, h=100.0):
    """Leaves (pre-order) of a uniform nx x ny x nz box whose material changes at the element column i = split -- a material
    boundary INSIDE a level that is not aligned with the 64-wide brick tiles: the tile that straddles it holds simple nodes
    of two materials.  -> (elem_ticks, elem_edge, edata [E,4] = h, Vp, Vs, rho, far_ticks)"""
    e = 1 << 23
    i, j, k = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    i, j, k = i.ravel(), j.ravel(), k.ravel()
    order = np.argsort(ho.zvalue(i, j, k), kind="stable")
    i, j, k = i[order], j[order], k[order]
    ticks = (np.stack([i, j, k], 1).astype(np.int64) * e).astype(np.uint32)
    edata = np.empty((len(i), 4), np.float32)
    edata[:] = (h, 6000.0, 3464.0, 2700.0)
    edata[i < split] = (h, 3000.0, 1732.0, 2200.0)
    return ticks, np.full(len(i), e, np.uint32), edata, (nx * e, ny * e, nz * e)


# ---------------------------------------------------------------------------------------------
# source forces on every node, one step from rest (tests/test_sources_oracle_cpu.py)
# ---------------------------------------------------------------------------------------------
def rest_forces(nt0, dt, seed):
    """A force of its own for every node and component: sign * uniform(0.5, 1) * 1e-3 * n_t[n][0] / dt^2 -- one step from
    rest then leaves about 1e-3 at every plain node and nothing near zero.  nt0 = the n_t rows' first column. -> [N, 3]"""
    rng = np.random.default_rng(seed)
    n = len(nt0)
    sign = rng.choice([-1.0, 1.0], (n, 3))
    return sign * rng.uniform(0.5, 1.0, (n, 3)) * (1e-3 / dt ** 2) * np.asarray(nt0, np.float64)[:, None]


def node_classes(n, dangling):
    """-> (hanging, anchor): boolean masks over the n nodes of a mesh with the hanging-node table `dangling` (or None)."""
    hanging, anchor = np.zeros(n, bool), np.zeros(n, bool)
    if dangling is not None:
        hanging[np.asarray(dangling[0])] = True
        anchor[np.asarray(dangling[2])] = True
    return hanging, anchor


def oracle_step_from_rest(lnid, etable, ntable, dt, loaded, F, dangling=None):
    """u(1) of the oracle's own single step from zero arrays with the nodes `loaded` forced by F [len(loaded), 3]; the
    arrays have ntable's type (float32: the oracle's -DSINGLE_PRECISION_SOLVER build)."""
    n = len(ntable)
    o1, o2 = np.zeros((n, 3), ntable.dtype), np.zeros((n, 3), ntable.dtype)
    ho.solver_run(lnid, np.ascontiguousarray(etable, np.float64), np.ascontiguousarray(ntable), o1, o2, 0, 1, dt,
                  loaded_lnid=np.ascontiguousarray(loaded, np.int32), forces=np.ascontiguousarray(F, np.float64)[None],
                  dangling=dangling)
    return o2


def uniform_box(nx, ny, nz, h=62.5, dt=1e-3, freq=5.0, vp=6000.0, vs=3464.0, rho=2700.0):
    """A homogeneous box with the oracle's own tables (ho.uniform_mesh + ho.solver_init) -> dict like two_level_mesh()."""
    elem_ijk, lnid, node_ijk = ho.uniform_mesh(nx, ny, nz)
    edata = np.empty((len(lnid), 4), np.float32)
    edata[:] = (h, vp, vs, rho)
    et, nt = ho.solver_init(lnid, edata, ho.face_bits(elem_ijk, nx, ny, nz), len(node_ijk), dt, freq)
    return dict(lnid=lnid, node_ijk=node_ijk, etable=et, ntable=nt, dt=dt, dangling=None, N=len(node_ijk), E=len(lnid),
                shape=(nx, ny, nz), node_xyz=(np.asarray(node_ijk, np.int64) * (1 << 20)).astype(np.int32))


RAGGED_PLAN = {"brick_ragged_minfill": 12, "brick_minnodes": 48, "brick_minz": 2}      # tests/test_gpu_parity.py test_ragged_*
_SOURCE_MESHES = {}


def source_mesh(name, damping="rayleigh"):
    """The meshes of the every-node-loaded source tests (tests/test_gpu_sources.py on the device,
    tests/test_sources_oracle_cpu.py for the oracle's side and the planner's counters), built once: the smallest ones
    the suite reaches each kernel with.  -> dict(lnid, etable, ntable, dt, dangling, N, node_xyz[, box | edata, material])
    het70x20x12 (box70x20x12's geometry) and c5_gradient_branch (c5_gradient's) carry branch_materials per element,
    labels included, with the tables of the damping kind (rayleigh, mass, none) at step_mesh's time step; the edge...,
    hetedge... and two...s.. boxes of edge_mesh() as they are."""
    if is_edge_mesh(name):
        return edge_mesh(name, damping)
    if name in ("het70x20x12", "c5_gradient_branch"):
        if (name, damping) not in _SOURCE_MESHES:
            _SOURCE_MESHES[(name, damping)] = _branch_mesh(name, damping)
        return _SOURCE_MESHES[(name, damping)]
    assert damping == "rayleigh"
    if name in _SOURCE_MESHES:
        return _SOURCE_MESHES[name]
    from hercules_amd import host
    if name == "box32x32x16":
        p = uniform_box(32, 32, 16)
    elif name == "box70x20x12":                 # x extent no multiple of 64, y no multiple of 8: partial tiles
        p = uniform_box(70, 20, 12)
    elif name == "box32":                       # 64 patches of 8^3 without bricks, 8 of them full lattices
        p = uniform_box(32, 32, 32, h=10.0, dt=2e-4)
    elif name in ("two_material", "lateral"):
        if name == "two_material":              # (reduced from 128 x 32 x 32: 28 033 nodes, still 8 ragged units)
            ticks, edge, edata, far = two_material_leaves(nx=96, ny=16, nz=16)
            box = host.OctBox.from_leaves(ticks, edge, edata, far, 1e-3, 2.0)
            xyz = box.node_xyz
        else:
            box = host.Box(32, 32, 32, 12.5, 2e-4, 50.0, lateral_classes=61, lateral_amp=0.1)
            xyz = None
        p = dict(lnid=box.lnid, etable=box.etable, ntable=box.ntable, dt=box.dt, dangling=None, N=len(box.ntable),
                 node_xyz=xyz, box=box)
    elif name in ("c5_basin", "c5_gradient"):
        q = c5_problem(name)
        p = dict(lnid=q["lnid"], etable=q["etable"], ntable=q["ntable"], dt=q["dt"], dangling=q["dangling"], N=q["N"],
                 node_xyz=(q["node_q"].astype(np.int64) * q["emin"]).astype(np.int32), edata=q["edata"], material=c5_material(q))
    elif name == "two_level":
        q = two_level_mesh(16, 8, 6, 3)
        p = dict(q, node_xyz=q["node_q"])
    else:
        raise KeyError(name)
    _SOURCE_MESHES[name] = p
    return p


def solver_desc(p, pack=False, precision="f64"):
    """hq_desc (capi._Desc) of a source_mesh() for the host-only plan checks (capi.brick_plan_check, plan_check,
    stencil_plan_check); the arrays it points to are kept alive on the returned object.  pack: with p's edata and
    material (hq_desc.edata / mat_*), as a context that may pack its per-element units gets them.  precision "f32": the
    n_t rows rounded to float and widened again, as the float library's planners see them (hq_prepare.h)."""
    import ctypes
    from hercules_amd import capi
    d = capi._Desc()
    if precision == "f32":
        assert "box" not in p
        p = dict(p, ntable=np.ascontiguousarray(p["ntable"], np.float32).astype(np.float64))
    if "box" in p:
        fill = p["box"]._lib.hqh_octbox_desc if hasattr(p["box"], "gid") else p["box"]._lib.hqh_box_desc
        assert fill(p["box"]._h, ctypes.byref(d)) == 0
        d.variant = capi.HQ_VARIANT_PATCH
        return d
    keep = [np.ascontiguousarray(p["lnid"], np.int32), np.ascontiguousarray(p["etable"], np.float64),
            np.ascontiguousarray(p["ntable"], np.float64),
            None if p["node_xyz"] is None else np.ascontiguousarray(p["node_xyz"], np.int32)]    # (None: hq_desc.node_xyz = NULL)
    d.lenum, d.nharbored = len(keep[0]), len(keep[2])
    d.lnid, d.eTable, d.nTable, d.node_xyz = [capi._ptr(a) for a in keep]
    if p["dangling"] is not None:
        dn = [np.ascontiguousarray(a, np.int32) for a in p["dangling"]]
        keep += dn
        d.ldnnum = len(dn[0])
        d.dn_ldnid, d.dn_ptr, d.dn_lanid = [capi._ptr(a) for a in dn]
    d.deltaT, d.rank, d.nranks, d.variant = p["dt"], 0, 1, capi.HQ_VARIANT_PATCH
    if pack:
        keep.append(np.ascontiguousarray(p["edata"], np.float32))
        d.edata = capi._ptr(keep[-1])
        d.mat_bbase, d.mat_threshold_damping, d.mat_threshold_vpvs = [float(v) for v in p["material"]]
    d._keep = keep
    return d


# ---------------------------------------------------------------------------------------------
# one step from two independent fields, term by term (tests/test_step_terms_cpu.py, tests/test_gpu_step_terms.py)
# ---------------------------------------------------------------------------------------------
def extended_element_sums(lnid, etable, N, u1, u2):
    """The element loops of extended_step alone: (force [N, 3], tf [N, 3]) in np.longdouble, the stiffness and damping
    forces summed per node and the same sums of absolute products.  They depend on the mesh, the eTable and the fields
    only, so the references of one (mesh, damping, precision) -- unloaded, every node loaded, every third -- share them
    (extended_step(..., sums=) takes them read-only and copies)."""
    L = np.longdouble
    assert np.finfo(L).eps < 1e-18, "np.longdouble is no wider than double here: the test modules skip before they get here"
    lnid = np.asarray(lnid, np.int64)
    E = len(lnid)
    et = np.asarray(etable).astype(L)
    u1, u2 = np.asarray(u1).astype(L), np.asarray(u2).astype(L)
    # [8][8][3][3] blocks -> [24 = (i, k)][24 = (j, l)]
    A1, A2 = [np.asarray(K).reshape(8, 8, 3, 3).transpose(0, 2, 1, 3).reshape(24, 24).astype(L) for K in ho.compute_K()]
    U = u1[lnid].reshape(E, 24)
    D = (u1 - u2)[lnid].reshape(E, 24)
    c = [et[:, k:k + 1] for k in range(4)]
    f = -(c[0] * (U @ A1.T) + c[1] * (U @ A2.T)) - (c[2] * (D @ A1.T) + c[3] * (D @ A2.T))
    aU, aD, a1, a2 = np.abs(U), np.abs(D), np.abs(A1), np.abs(A2)
    t = np.abs(c[0]) * (aU @ a1.T) + np.abs(c[1]) * (aU @ a2.T) + np.abs(c[2]) * (aD @ a1.T) + np.abs(c[3]) * (aD @ a2.T)
    force, tf = np.zeros((N, 3), L), np.zeros((N, 3), L)
    np.add.at(force, lnid.reshape(-1), f.reshape(-1, 3))
    np.add.at(tf, lnid.reshape(-1), t.reshape(-1, 3))
    return force, tf


def extended_step(lnid, etable, ntable, u1, u2, dangling=None, loaded=None, F=None, dt=None, sums=None):
    """The oracle's step (oracle/herc_oracle.c: ho_solver_run with the conventional element matrices) restated in
    np.longdouble, the inputs taken as given and widened: element forces -(c1 K1 + c2 K2) u1 - (c3 K1 + c4 K2)(u1 - u2)
    with K1, K2 of ho.compute_K(), compute_adjust DISTRIBUTION of the forces, the per-axis update
    (f + m2[d] u1 - m1[d] u2) / m0 with the 7-double n_t row, compute_adjust ASSIGNMENT.
    loaded, F [len(loaded), 3] (double), dt: compute_addforce_s (psolve.c:5912-5928) -- force[loaded] gets F dt^2, dt^2
    formed in np.longdouble from the double dt, and T gets |F dt^2| -- BEFORE the hanging-node distribution, as the
    reference assigns the load ahead of the element loops and distributes the sum of both (psolve.c:5936-5987).  Every
    node is named once.  F may be a list of such tables (the ranks' loads on one node): force gets their sum and T the
    sum of their absolute values, not the absolute value of their sum -- the terms may cancel.
    sums: extended_element_sums(...) of the same mesh and fields, computed elsewhere (left unchanged).
    -> (ref [N, 3] = the new displacement, T [N, 3] = the same expression with every product replaced by its absolute
    value: the node's own scale of summed magnitudes), both np.longdouble."""
    L = np.longdouble
    assert np.finfo(L).eps < 1e-18, "np.longdouble is no wider than double here: the test modules skip before they get here"
    N = len(ntable)
    nt = np.asarray(ntable).astype(L)
    if sums is None:
        force, tf = extended_element_sums(lnid, etable, N, u1, u2)
    else:
        force, tf = sums[0].copy(), sums[1].copy()
    u1, u2 = np.asarray(u1).astype(L), np.asarray(u2).astype(L)
    if loaded is not None and len(loaded):
        ld = np.asarray(loaded, np.int64)
        assert len(np.unique(ld)) == len(ld) and dt is not None
        dt2 = L(float(dt)) * L(float(dt))
        for Fk in (F if isinstance(F, (list, tuple)) else [F]):
            Fk = np.asarray(Fk)
            assert Fk.dtype == np.float64 and Fk.shape == (len(ld), 3)
            load = Fk.astype(L) * dt2
            force[ld] += load
            tf[ld] += np.abs(load)
    if dangling is not None and len(dangling[0]):
        ids, ptr, anc = [np.asarray(a, np.int64) for a in dangling]
        deps = np.diff(ptr)
        assert not np.isin(anc, ids).any()                       # no anchor is itself hanging: the order of the loop is free
        for table in (force, tf):
            np.add.at(table, anc, np.repeat(table[ids] / deps[:, None].astype(L), deps, axis=0))
    ref = (force + nt[:, 1:4] * u1 - nt[:, 4:7] * u2) / nt[:, :1]
    T = (tf + np.abs(nt[:, 1:4] * u1) + np.abs(nt[:, 4:7] * u2)) / np.abs(nt[:, :1])
    if dangling is not None and len(dangling[0]):
        for table in (ref, T):
            mean = np.zeros((len(ids), 3), L)
            np.add.at(mean, np.repeat(np.arange(len(ids)), deps), table[anc] / np.repeat(deps, deps)[:, None].astype(L))
            table[ids] = mean
    return ref, T


def oracle_loaded_step(p, nt, u1, u2, loaded, F, etable=None):
    """The C oracle's new displacement from tm1 = u1, tm2 = u2 with the nodes `loaded` forced by F [len(loaded), 3]
    (double, as hq_set_source takes it), in nt's type: the twin of extended_step(..., loaded, F, dt).  p: a step_mesh
    (lnid, etable, dt, kind, dangling).  The float build keeps its force accumulator in float, so F dt^2 is rounded
    before the element sums are added: the reference's own behaviour, and not what the float library does."""
    o1, o2 = u2.copy(), u1.copy()
    ho.solver_run(p["lnid"], np.ascontiguousarray(p["etable"] if etable is None else etable, np.float64), np.ascontiguousarray(nt),
                  o1, o2, 0, 1, p["dt"], damping=p["kind"], loaded_lnid=np.ascontiguousarray(loaded, np.int32),
                  forces=np.ascontiguousarray(F, np.float64)[None], dangling=p["dangling"])
    assert np.array_equal(o1, u1)
    return o2


def step_fields(n, seed, dangling=None, real=np.float64):
    """(u1, u2), drawn independently as sign * uniform(0.5, 1) * 1e-3 per node and component (the shape of rest_forces:
    nothing near zero, u1 - u2 as large as the fields); hanging nodes take the mean of their anchors in both."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        u = np.ascontiguousarray(rng.choice([-1.0, 1.0], (n, 3)) * rng.uniform(0.5, 1.0, (n, 3)) * 1e-3, real)
        if dangling is not None and len(dangling[0]):
            ho.compute_adjust(u, 1, dangling)
        out.append(u)
    return out[0], out[1]


BRANCHES = ("plain", "capped", "fixed", "zeta_capped")


def branch_materials(E, seed, thr_damping=0.05, thr_vpvs=3.0):
    """Per-element (Vp, Vs, rho) float32 through every branch of mu_and_lambda (psolve.c:3236-3272) and both sides of
    the damping threshold (psolve.c:3397-3401), drawn as tests/test_kernel_math_cpu.py draws them but shuffled over the
    elements: Vs in 80 - 4000 (log-uniform: a quarter below 200, where 10 / Vs passes the threshold), a quarter of the
    elements with Vp / Vs in 3 - 12 (capped), an eighth with Vp^2 < 2 Vs^2 (negative lambda: solver_init rewrites Vp).
    -> (vp, vs, rho, labels): labels = {name: bool [E]} for BRANCHES, from the edata before and after ho.solver_init
    rewrote it; plain / capped / fixed exclude each other, zeta_capped is independent of them.  Each holds >= 10 %."""
    rng = np.random.default_rng(seed)
    vs = np.exp(rng.uniform(np.log(80.0), np.log(4000.0), E)).astype(np.float32)
    ratio = np.where(rng.random(E) < 0.25, rng.uniform(3.0, 12.0, E), rng.uniform(1.5, 3.0, E))
    neg = rng.permutation(E)[: E // 8]
    ratio[neg] = rng.uniform(0.9, 1.4, len(neg))
    vp = (vs * ratio).astype(np.float32)
    rho = rng.uniform(1500.0, 3000.0, E).astype(np.float32)
    before = np.stack([np.full(E, 10.0, np.float32), vp, vs, rho], 1).copy()
    after = before.copy()
    ho.solver_init(np.arange(8 * E, dtype=np.int32).reshape(E, 8), after, np.zeros(E, np.uint8), 8 * E, 1e-3, 5.0,
                   thr_damping=thr_damping, thr_vpvs=thr_vpvs)      # disjoint elements: only the rewrite of Vp matters
    fixed = after[:, 1] != before[:, 1]
    capped = ~fixed & (before[:, 1].astype(np.float64) > before[:, 2].astype(np.float64) * thr_vpvs)
    zeta = (np.float32(10.0) / vs).astype(np.float64) > thr_damping
    labels = dict(plain=~fixed & ~capped, capped=capped, fixed=fixed, zeta_capped=zeta)
    for k in BRANCHES:
        assert labels[k].sum() * 10 >= E, (k, int(labels[k].sum()), E)
    assert np.array_equal(fixed, np.isin(np.arange(E), neg))
    return vp, vs, rho, labels


def _quarter_cfl_dt(edata, thr_vpvs=3.0):
    """dt at which the stiffest element has (Vp dt / h)^2 = 0.25, Vp as the solver uses it (capped at thr_vpvs Vs; the
    edata as solver_init left it): one step needs no stability, only a force that is not lost beside 2 u1 - u2."""
    ed = np.asarray(edata, np.float64)
    return float(0.5 / (np.minimum(ed[:, 1], thr_vpvs * ed[:, 2]) / ed[:, 0]).max())


def _branch_tables(lnid, h, face, N, seed, damping, freq, dangling=None):
    """branch_materials on a mesh -> (edata as solver_init left it, etable, ntable, dt, labels, material, raw edata)."""
    kind = ho.DAMPING_BY_NAME[damping]
    vp, vs, rho, labels = branch_materials(len(lnid), seed)
    raw = np.ascontiguousarray(np.stack([np.asarray(h, np.float32) * np.ones(len(lnid), np.float32), vp, vs, rho], 1))
    probe = raw.copy()
    ho.solver_init(lnid, probe, face, N, 1e-3, freq, damping=kind)           # (the rewritten Vp does not depend on dt)
    dt = _quarter_cfl_dt(probe)
    edata = raw.copy()
    etable, ntable = ho.solver_init(lnid, edata, face, N, dt, freq, damping=kind)
    assert np.array_equal(edata, probe)
    if dangling is not None:
        ho.compute_adjust(ntable, 0, dangling)
    return edata, etable, ntable, dt, labels, (ho.setab(freq, kind)[1], 0.05, 3.0), raw


def _branch_mesh(name, damping):
    if name == "het70x20x12":
        nx, ny, nz, h, freq = 70, 20, 12, 62.5, 5.0
        elem_ijk, lnid, node_ijk = ho.uniform_mesh(nx, ny, nz)
        edata, et, nt, dt, labels, material, raw = _branch_tables(lnid, h, ho.face_bits(elem_ijk, nx, ny, nz), len(node_ijk),
                                                                  7012, damping, freq)
        return dict(lnid=lnid, etable=et, ntable=nt, dt=dt, dangling=None, N=len(node_ijk), E=len(lnid), shape=(nx, ny, nz),
                    node_xyz=(np.asarray(node_ijk, np.int64) * (1 << 20)).astype(np.int32), edata=edata, material=material,
                    labels=labels, damping=damping, raw_edata=raw)
    g = load("c5_gradient")
    m = ho.octree_mesh_from_elem_ticks(g["elem_ticks"], C1_FAR_TICKS)
    h = (1000.0 / 2 ** 30 * m["emin"] * m["elem_size"].astype(np.float64)).astype(np.float32)
    edata, et, nt, dt, labels, material, raw = _branch_tables(m["lnid"], h, m["face"], len(m["node_q"]), 7013, damping,
                                                              float(g["freq"]), m["dangling"])
    return dict(lnid=m["lnid"], etable=et, ntable=nt, dt=dt, dangling=m["dangling"], N=len(m["node_q"]), E=len(m["lnid"]),
                node_xyz=(m["node_q"].astype(np.int64) * m["emin"]).astype(np.int32), edata=edata, material=material,
                labels=labels, damping=damping, raw_edata=raw)


# ---------------------------------------------------------------------------------------------
# boxes whose extents leave the brick planner degenerate units (tests/test_brick_edges_cpu.py, tests/test_gpu_brick_edges.py)
# ---------------------------------------------------------------------------------------------
_EDGE_NAME = re.compile(r"^(edge|hetedge|two)(\d+)x(\d+)x(\d+)(?:s(\d+))?$")
_EDGE_SEEDS = {"hetedge65x9x8": 7101, "hetedge64x9x36": 7102, "hetedge3x9x8": 7103}
_EDGE_MESHES = {}


def is_edge_mesh(name):
    return _EDGE_NAME.match(name) is not None


def edge_mesh(name, damping="rayleigh"):
    """A box of nx x ny x nz elements (h = 62.5) named for the footprints its interior leaves on the planner's tile grid --
    (nx - 1) mod 64 == 1 gives a column ONE node wide, (ny - 1) mod 8 == 1 a row one node deep, (nz - 1) mod cz == 1 a unit
    of one plane; 62 and 7 for the per-element kernel's tiles:
      edgeAxBxC      one material (hq_k_brick), like uniform_box
      hetedgeAxBxC   branch_materials per element (hq_k_brick_het), like het70x20x12; edata / material for the packed form
      twoAxBxCsS     the soft material in the element columns i < S, the hard one beyond (two_material_leaves' recipe):
                     the tile that straddles i = S is ragged, the nodes of the plane x = S are per-element ones
    dt at a quarter of the stiffest element's CFL square (the step meshes' rule), tables of the damping kind (edge / two:
    rayleigh).  Built once.  -> dict like step_mesh's, with shape, node_ijk, elem_ijk."""
    key = (name, damping)
    if key in _EDGE_MESHES:
        return _EDGE_MESHES[key]
    m = _EDGE_NAME.match(name)
    family, (nx, ny, nz), split = m.group(1), [int(v) for v in m.group(2, 3, 4)], m.group(5)
    assert (family == "two") == (split is not None), name
    h, freq = 62.5, 5.0
    elem_ijk, lnid, node_ijk = ho.uniform_mesh(nx, ny, nz)
    face, N = ho.face_bits(elem_ijk, nx, ny, nz), len(node_ijk)
    xyz = (np.asarray(node_ijk, np.int64) * (1 << 20)).astype(np.int32)
    common = dict(lnid=lnid, dangling=None, N=N, E=len(lnid), shape=(nx, ny, nz), node_xyz=xyz, node_ijk=np.asarray(node_ijk),
                  elem_ijk=np.asarray(elem_ijk), damping=damping)
    if family == "hetedge":
        edata, et, nt, dt, labels, material, raw = _branch_tables(lnid, h, face, N, _EDGE_SEEDS[name], damping, freq)
        p = dict(common, etable=et, ntable=nt, dt=dt, edata=edata, material=material, labels=labels, raw_edata=raw)
    else:
        assert damping == "rayleigh"
        edata = np.empty((len(lnid), 4), np.float32)
        edata[:] = (h, 6000.0, 3464.0, 2700.0)
        if split is not None:
            assert 0 < int(split) < nx
            edata[np.asarray(elem_ijk)[:, 0] < int(split)] = (h, 3000.0, 1732.0, 2200.0)
        dt = _quarter_cfl_dt(edata)
        raw = edata.copy()
        et, nt = ho.solver_init(lnid, edata, face, N, dt, freq)
        assert np.array_equal(edata, raw)                          # plain materials: solver_init rewrites nothing
        p = dict(common, etable=et, ntable=nt, dt=dt, edata=edata, material=(ho.setab(freq, ho.DAMP_RAYLEIGH)[1], 0.05, 3.0))
    _EDGE_MESHES[key] = p
    return p


_STEP_MESHES = {}


def step_mesh(name, damping="rayleigh"):
    """A mesh of the one-step term tests with the time step at a quarter of the stiffest element's CFL square and the
    tables of the damping kind: source_mesh's new entries as they are, its homogeneous ones rebuilt at that dt."""
    key = (name, damping)
    if key in _STEP_MESHES:
        return _STEP_MESHES[key]
    kind = ho.DAMPING_BY_NAME[damping]
    if is_edge_mesh(name):
        p = edge_mesh(name, damping)
    elif name in ("het70x20x12", "c5_gradient_branch"):
        p = source_mesh(name, damping)
    elif name in ("box32x32x16", "box70x20x12", "box32"):
        assert damping == "rayleigh"
        shape, h = {"box32x32x16": ((32, 32, 16), 62.5), "box70x20x12": ((70, 20, 12), 62.5), "box32": ((32, 32, 32), 10.0)}[name]
        p = uniform_box(*shape, h=h, dt=0.5 * h / 6000.0)
    elif name == "two_level":
        assert damping == "rayleigh"
        q = two_level_mesh(16, 8, 6, 3, dt=0.5 * 31.25 / 3000.0)
        p = dict(q, node_xyz=q["node_q"])
    else:
        raise KeyError(name)
    p = dict(p, damping=damping, kind=kind)
    _STEP_MESHES[key] = p
    return p


# ---------------------------------------------------------------------------------------------
# the same step on partitions (tests/test_partition_step_cpu.py, tests/test_gpu_partition_step.py)
# ---------------------------------------------------------------------------------------------
STEP_SEED = 5150
_PARTITION_MESHES, _PARTITIONS, _PARTITION_PROBLEMS = {}, {}, {}


def _partition_mesh(name):
    """-> (m = ho.octree_mesh_from_elem_ticks(...), far_q, freq, node_xyz [N, 3] int32) of a step_mesh, the uniform
    het70x20x12 as an octree of one level (ho.uniform_mesh lists its elements in Z-order = octor's pre-order)."""
    if name in _PARTITION_MESHES:
        return _PARTITION_MESHES[name]
    if name == "c5_gradient_branch":
        g = load("c5_gradient")
        m = ho.octree_mesh_from_elem_ticks(g["elem_ticks"], C1_FAR_TICKS)
        out = (m, [f // m["emin"] for f in C1_FAR_TICKS], float(g["freq"]), (m["node_q"].astype(np.int64) * m["emin"]).astype(np.int32))
    elif name == "two_level":
        q = step_mesh("two_level")
        out = (q["mesh"], list(q["far"]), q["freq"], np.ascontiguousarray(q["node_q"], np.int32))
    elif name == "het70x20x12":
        nx, ny, nz = 70, 20, 12
        elem_ijk, _, _ = ho.uniform_mesh(nx, ny, nz)
        ll = np.asarray(elem_ijk, np.int64)
        assert np.all(np.diff(ho.zvalue(ll[:, 0], ll[:, 1], ll[:, 2]).astype(np.int64)) > 0)       # Z-order
        corners = np.array([[(c >> 0) & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)], np.int64)
        m = ho.octree_mesh_from_elem_ticks(ll[:, None, :] + corners[None, :, :], (nx, ny, nz))
        assert len(m["dangling"][0]) == 0
        out = (m, [nx, ny, nz], 5.0, (m["node_q"].astype(np.int64) * (1 << 20)).astype(np.int32))
    else:
        raise KeyError(name)
    _PARTITION_MESHES[name] = out
    return out


def _freeze(x):
    if isinstance(x, np.ndarray):
        x.flags.writeable = False
    elif isinstance(x, dict):
        for v in x.values():
            _freeze(v)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _freeze(v)
    return x


def mesh_partition(name, nranks):
    """ho.octree_partition of a step_mesh on nranks ranks, built once and read-only."""
    if (name, nranks) not in _PARTITIONS:
        m, far_q, _, _ = _partition_mesh(name)
        _PARTITIONS[(name, nranks)] = _freeze(ho.octree_partition(m, nranks, far_q))
    return _PARTITIONS[(name, nranks)]


def partition_step_problem(mesh, nranks, damping="rayleigh", precision="f64"):
    """One step from two independent fields on a step_mesh cut into nranks ranks (ho.octree_partition), the ranks' tables
    from ho.multi_rank_init on the RAW (h, Vp, Vs, rho) rows (solver_init rewrites Vp where lambda is negative: a second
    solver_init on the rewritten rows gives other tables) at step_mesh's dt.  Built once per argument list, read-only.
    -> dict(parts (with an_sched, dn_sched, lnid, dangling, nodes, owner, elems), gid = the ranks' nodes, ets, nts, edata
    (per rank, as solver_init left them), node_xyz (per rank), xyz (global), u1, u2 (global: step_fields), etable = the
    global eTable assembled by elems, ntable = the global n_t assembled from the OWNERS' rows (the mass exchange sums in
    another order than one rank: the reference takes the rows the ranks hold), ref, T = extended_step of them,
    B_oracle = the worst |multi_rank_run's single step - ref| / (2^-53 T) (float: 2^-24 T) over all ranks' copies,
    oracle = that step's per-rank result, lnid, dangling, dt, N, E, kind, material, labels (branch meshes), real)."""
    key = (mesh, nranks, damping, precision)
    if key in _PARTITION_PROBLEMS:
        return _PARTITION_PROBLEMS[key]
    p = step_mesh(mesh, damping)
    m, far_q, freq, xyz = _partition_mesh(mesh)
    parts = mesh_partition(mesh, nranks)
    real = np.float32 if precision == "f32" else np.float64
    raw = p["raw_edata"] if "raw_edata" in p else p["edata"]         # (two_level: plain materials, nothing is rewritten)
    E, N, dt = len(m["lnid"]), len(m["node_q"]), p["dt"]
    assert raw.shape == (E, 4)
    eds = [np.ascontiguousarray(raw[q["elems"]]) for q in parts]
    fcs = [np.ascontiguousarray(m["face"][q["elems"]]) for q in parts]
    ets, nts = ho.multi_rank_init(parts, eds, fcs, dt, freq, damping=p["kind"], real=real)
    gid = [np.asarray(q["nodes"], np.int64) for q in parts]
    etable, ntable = np.zeros((E, 4)), np.full((N, 7), np.nan, real)
    for q, et, nt, g in zip(parts, ets, nts, gid):
        etable[q["elems"]] = et
        own = np.asarray(q["owner"]) == q["rank"]
        ntable[g[own]] = nt[own]
    assert np.isfinite(ntable).all()                                  # every node has an owner
    dangling = m["dangling"] if len(m["dangling"][0]) else None
    u1, u2 = step_fields(N, STEP_SEED, dangling, real)
    ref, T = extended_step(m["lnid"], etable, ntable, u1, u2, dangling)
    o1, o2 = [np.ascontiguousarray(u2[g]) for g in gid], [np.ascontiguousarray(u1[g]) for g in gid]
    ho.multi_rank_run(parts, ets, nts, o1, o2, 0, 1, dt, [[]] * nranks, [None] * nranks)
    unit = 2.0 ** -24 if precision == "f32" else 2.0 ** -53
    b = max(float((np.abs(o - ref[g]) / (unit * T[g])).max()) for o, g in zip(o2, gid))
    out = dict(mesh=mesh, nranks=nranks, damping=damping, precision=precision, real=real, parts=parts, gid=gid, ets=ets, nts=nts,
               edata=eds, node_xyz=[np.ascontiguousarray(xyz[g]) for g in gid], xyz=xyz, u1=u1, u2=u2, etable=etable,
               ntable=ntable, ref=ref, T=T, B_oracle=b, oracle=o2, lnid=m["lnid"], dangling=dangling, dt=dt, N=N, E=E,
               kind=p["kind"], freq=freq, material=p.get("material", (ho.setab(freq, p["kind"])[1], 0.05, 3.0)),
               labels=p.get("labels"))
    _PARTITION_PROBLEMS[key] = _freeze(out)
    return out


def partition_classes(prob):
    """Per rank, boolean masks over its nodes: owned interface nodes (named in an an_sched s-list), the count of their
    sharers, nodes owned by another rank, hanging nodes."""
    out = []
    for q in prob["parts"]:
        n = len(q["nodes"])
        sharers = np.zeros(n, np.int64)
        for _, mapping in q["an_sched"]["s"]:
            sharers[np.asarray(mapping)] += 1
        out.append(dict(sharers=sharers, interface=sharers > 0, foreign=np.asarray(q["owner"]) != q["rank"],
                        hanging=np.asarray(q["is_dangling"], bool)))
    return out


def rank_desc(prob, r, pack=False):
    """hq_desc (capi._Desc) of one rank of a partition_step_problem with its schedules, for the host-only plan checks."""
    import ctypes  # noqa: F401
    from hercules_amd import capi
    q = prob["parts"][r]
    d = capi._Desc()
    keep = [np.ascontiguousarray(q["lnid"], np.int32), np.ascontiguousarray(prob["ets"][r], np.float64),
            np.ascontiguousarray(prob["nts"][r], np.float64), np.ascontiguousarray(prob["node_xyz"][r], np.int32)]
    d.lenum, d.nharbored = len(keep[0]), len(keep[2])
    d.lnid, d.eTable, d.nTable, d.node_xyz = [capi._ptr(a) for a in keep]
    if len(q["dangling"][0]):
        dn = [np.ascontiguousarray(a, np.int32) for a in q["dangling"]]
        keep += dn
        d.ldnnum = len(dn[0])
        d.dn_ldnid, d.dn_ptr, d.dn_lanid = [capi._ptr(a) for a in dn]
    d.an_sched = capi._schedule(q["an_sched"], keep)
    d.dn_sched = capi._schedule(q["dn_sched"], keep)
    d.deltaT, d.rank, d.nranks, d.variant = prob["dt"], r, prob["nranks"], capi.HQ_VARIANT_PATCH
    if pack:
        keep.append(np.ascontiguousarray(prob["edata"][r], np.float32))
        d.edata = capi._ptr(keep[-1])
        d.mat_bbase, d.mat_threshold_damping, d.mat_threshold_vpvs = [float(v) for v in prob["material"]]
    d._keep = keep
    return d


BOX_STEP = dict(h=20.0, freq=20.0, vp=6000.0)               # host.Box's default material; dt = 0.5 h / Vp
_BOX_PROBLEMS = {}


def box_step_boxes(shape, nranks):
    """The nranks partitions of the uniform box `shape` as the C host cuts them (host.Box), at dt = 0.5 h / Vp."""
    from hercules_amd import host
    h = BOX_STEP["h"]
    return [host.Box(shape[0], shape[1], shape[2], h, 0.5 * h / BOX_STEP["vp"], BOX_STEP["freq"], rank=r, nranks=nranks)
            for r in range(nranks)]


def box_step_problem(shape, nranks, precision="f64"):
    """The partitioned one-step problem on host.Box partitions, the reference assembled from the boxes' OWN tables: global
    eTable by element, global n_t from the owners' rows (precision f32: rounded to float as host._solver_from_desc hands
    them over).  Nodes and elements numbered as ho.uniform_mesh does.  B_oracle: the C oracle's single-rank step on the
    assembled tables.  Built once, read-only.  -> dict(gid, nts, u1, u2, etable, ntable, ref, T, B_oracle, lnid, dt, N, E,
    owner, dangling=None)"""
    key = (tuple(shape), nranks, precision)
    if key in _BOX_PROBLEMS:
        return _BOX_PROBLEMS[key]
    nx, ny, nz = shape
    real = np.float32 if precision == "f32" else np.float64
    _, lnid, node_ijk = ho.uniform_mesh(nx, ny, nz)
    lnid = np.asarray(lnid, np.int64)
    N, E = len(node_ijk), len(lnid)
    code = lambda ijk: (np.asarray(ijk, np.int64)[:, 2] * (ny + 1) + np.asarray(ijk, np.int64)[:, 1]) * (nx + 1) + np.asarray(ijk, np.int64)[:, 0]
    lut = np.full((nx + 1) * (ny + 1) * (nz + 1), -1, np.int64)
    lut[code(node_ijk)] = np.arange(N)
    elem_of = {int(k): e for e, k in enumerate(lnid.min(axis=1))}
    assert len(elem_of) == E
    etable, ntable = np.full((E, 4), np.nan), np.full((N, 7), np.nan, real)
    gid, nts, owner = [], [], []
    boxes = box_step_boxes(shape, nranks)
    try:
        dt = boxes[0].dt
        for r, b in enumerate(boxes):
            g = lut[code(b.node_ijk)]
            assert (g >= 0).all() and len(np.unique(g)) == len(g)
            nt = np.ascontiguousarray(b.ntable, real)
            own = np.asarray(b.owner) == r
            ntable[g[own]] = nt[own]
            etable[[elem_of[int(k)] for k in g[np.asarray(b.lnid, np.int64)].min(axis=1)]] = b.etable
            gid.append(g)
            nts.append(nt)
            owner.append(np.array(b.owner))
    finally:
        for b in boxes:
            b.close()
    assert np.isfinite(etable).all() and np.isfinite(ntable).all()
    u1, u2 = step_fields(N, STEP_SEED, None, real)
    ref, T = extended_step(lnid, etable, ntable, u1, u2, None)
    o1, o2 = u2.copy(), u1.copy()
    ho.solver_run(lnid.astype(np.int32), etable, ntable, o1, o2, 0, 1, dt)
    b_oracle = float((np.abs(o2 - ref) / ((2.0 ** -24 if precision == "f32" else 2.0 ** -53) * T)).max())
    out = dict(shape=tuple(shape), nranks=nranks, precision=precision, real=real, gid=gid, nts=nts, owner=owner, u1=u1, u2=u2,
               etable=etable, ntable=ntable, ref=ref, T=T, B_oracle=b_oracle, lnid=lnid, dt=dt, N=N, E=E, dangling=None)
    _BOX_PROBLEMS[key] = _freeze(out)
    return out
