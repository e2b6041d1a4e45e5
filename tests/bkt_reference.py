"""The reference's BKT constant-Q step (type_of_damping = bkt) restated, for the attenuation tests: no device, no library.

bkt_step() is solver_run's body under BKT (psolve.c:3995-3999 inside :4265-4319) in numpy doubles, element by element as
the reference has it: per-element-CORNER memory variables (conv_shear_1/2, conv_kappa_1/2: [E * 8, 3], cindex = eindex * 8 + i),
calc_conv (damping.c:110-222) with its skip of a modulus whose g0 or g1 is 0, then constant_Q_addforce (:228-416) with its
csum == 0 branch, the vector_is_zero skips (an element whose 24 values are all within 1e-20 of zero adds nothing) and the unrolled sums of aTransposeU / firstVector_mu / firstVector_kappa / au
(stiffness.c:245-424) in their written order, the nodal sums in element order; exp is math.exp (libm's, as C's).  Every numpy
operation below is one IEEE double operation per element, in the order of the C expression it restates.

extended_sums() is the same force in np.longdouble in ANOTHER form -- through the conventional element matrices K1, K2 of
oracle.herc_oracle.compute_K(): A D_mu A^T = -c1 (K1 - 2/3 K2) and A D_kappa A^T = -(c2 + 2/3 c1) K2 -- with T, the same
expression with every product replaced by its absolute value, the memory-variable terms included; tests/helpers.extended_step
finishes the step from them (sums=).

Four made-up classes (CLASSES) serve the tests: no table of the reference is held here; the fixtures carry their own rows.
"""
import math

import numpy as np

from oracle import herc_oracle as ho

NAMES = ("a0_shear", "a1_shear", "b_shear", "g0_shear", "g1_shear", "a0_kappa", "a1_kappa", "b_kappa", "g0_kappa", "g1_kappa")
# both moduli on, shear only, dilatation only, all zero (the values are of the size the reference's rows have; made up)
CLASSES = np.array([[0.0373, 0.0641, 0.0158, 0.0611, 0.9163, 0.0185, 0.0319, 0.0079, 0.0427, 0.7731],
                    [0.0482, 0.0815, 0.0203, 0.0539, 0.8811, 0.0, 0.0, 0.0, 0.0, 0.0],
                    [0.0, 0.0, 0.0, 0.0, 0.0, 0.0251, 0.0433, 0.0107, 0.0467, 0.8125],
                    [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]], np.float32)

UNDERFLOW_CAP = 1e-20                                            # quake_util.c:36: an element whose damping vector is below it is skipped
_exp = np.frompyfunc(math.exp, 1, 1)


def class_coef(coef, freq, dt):
    """Per element (or class) row of ten floats: the doubles calc_conv and constant_Q_addforce form, in their order.
    -> dict(rmax, on [n, 2] = the modulus is convolved, cu1, cu2, ex [n, 2, 2] (modulus, variable), csum_on [n, 2],
    a [n, 2, 2], bq [n, 2])."""
    c = np.ascontiguousarray(coef, np.float32).reshape(-1, 10).astype(np.float64)
    rmax = 2. * math.pi * freq * dt
    n = len(c)
    on, csum_on = np.zeros((n, 2), bool), np.zeros((n, 2), bool)
    cu1, cu2, ex = np.zeros((n, 2, 2)), np.zeros((n, 2, 2)), np.ones((n, 2, 2))
    a, bq = np.zeros((n, 2, 2)), np.zeros((n, 2))
    for m in range(2):
        r = c[:, 5 * m:5 * m + 5]
        on[:, m] = (r[:, 3] != 0) & (r[:, 4] != 0)
        for v in range(2):
            g = r[:, 3 + v] * rmax
            half = g / 2.
            cu2[:, m, v] = half
            cu1[:, m, v] = half * (1. - g)
            ex[:, m, v] = _exp(-g).astype(np.float64)
        csum_on[:, m] = (r[:, 0] + r[:, 1] + r[:, 2]) != 0
        a[:, m, 0], a[:, m, 1] = r[:, 0], r[:, 1]
        bq[:, m] = r[:, 2] / rmax
    return dict(rmax=rmax, on=on, cu1=cu1, cu2=cu2, ex=ex, csum_on=csum_on, a=a, bq=bq)


def new_state(E):
    """The four arrays of the reference, calloc'ed: [4 (shear 1, shear 2, kappa 1, kappa 2), E * 8, 3]."""
    return np.zeros((4, E * 8, 3))


def calc_conv(lnid, K, u1, u2, conv):
    """damping.c:110-222, in place on conv [4, E * 8, 3]."""
    E = len(lnid)
    U1, U2 = u1[lnid], u2[lnid]                                   # [E, 8, 3]
    for m in range(2):
        sel = K["on"][:, m]
        for v in range(2):
            f = conv[2 * m + v].reshape(E, 8, 3)
            c1, c2, e = [K[k][:, m, v][:, None, None] for k in ("cu1", "cu2", "ex")]
            new = c1 * U1 + c2 * U2 + e * f
            f[sel] = new[sel]


def damping_vectors(lnid, K, u1, u2, conv):
    """damping.c:254-371 -> (shear, kappa) [E, 8, 3] each."""
    E = len(lnid)
    U1, U2 = u1[lnid], u2[lnid]
    out = []
    for m in range(2):
        f0, f1 = conv[2 * m].reshape(E, 8, 3), conv[2 * m + 1].reshape(E, 8, 3)
        a0, a1, bq = K["a"][:, m, 0][:, None, None], K["a"][:, m, 1][:, None, None], K["bq"][:, m][:, None, None]
        w = bq * (U1 - U2) - (a0 * f0 + a1 * f1) + U1
        out.append(np.where(K["csum_on"][:, m][:, None, None], w, U1))
    return out[0], out[1]


_ATU = ["----++++", "--++--++", "-+-+-+-+", "++----++", "+-+--+-+", "+--++--+", "-++-+--+"]      # atu[1..7] over u[0..7]
_AU = ["+---+++-", "+--++--+", "+-+--+-+", "+-++--+-", "++----++", "++-+-+--", "+++-+---", "++++++++"]


def _signed_sum(signs, terms):
    acc = terms[0] if signs[0] == "+" else -terms[0]
    for s, t in zip(signs[1:], terms[1:]):
        acc = acc + t if s == "+" else acc - t
    return acc


def _atransposeu(w):
    """aTransposeU (stiffness.c:245-289): w [E, 8, 3] -> atu: list of 24 arrays [E]."""
    zero = np.zeros(len(w))
    atu = []
    for comp in range(3):                                         # reformU: u[comp * 8 + node]
        u = [w[:, n, comp] for n in range(8)]
        atu.append(zero)
        atu += [_signed_sum(s, u) for s in _ATU]
    return atu


def _first_vector_mu(t, b):
    """firstVector_mu (stiffness.c:351-379) -> dict index -> addend."""
    return {1: b * (t[19] + t[1]), 2: b * (t[11] + t[2]), 3: b * (4. * t[3] - 2. * (t[10] + t[17])) / 3.,
            4: b * (t[13] + t[22] + 2. * t[4]) / 3., 5: b * (7. * t[5] - 2. * t[12]) / 9., 6: b * (7. * t[6] - 2. * t[20]) / 9.,
            7: (10. * b * t[7]) / 27.,
            9: b * (t[18] + t[9]), 10: b * (4. * t[10] - 2. * (t[3] + t[17])) / 3., 11: b * (t[11] + t[2]),
            12: b * (7. * t[12] - 2. * t[5]) / 9., 13: b * (t[4] + t[22] + 2. * t[13]) / 3., 14: b * (7. * t[14] - 2. * t[21]) / 9.,
            15: (10. * b * t[15]) / 27.,
            17: b * (4. * t[17] - 2. * (t[3] + t[10])) / 3., 18: b * (t[18] + t[9]), 19: b * (t[19] + t[1]),
            20: b * (7. * t[20] - 2. * t[6]) / 9., 21: b * (7. * t[21] - 2. * t[14]) / 9., 22: b * (t[4] + t[13] + 2. * t[22]) / 3.,
            23: (10. * b * t[23]) / 27.}


def _first_vector_kappa(t, k):
    """firstVector_kappa (stiffness.c:321-349) -> dict index -> addend (the others add 0.)."""
    return {3: k * (t[3] + t[10] + t[17]), 5: k * (t[5] + t[12]) / 3., 6: k * (t[6] + t[20]) / 3., 7: k * t[7] / 9.,
            10: k * (t[10] + t[3] + t[17]), 12: k * (t[12] + t[5]) / 3., 14: k * (t[14] + t[21]) / 3., 15: k * t[15] / 9.,
            17: k * (t[17] + t[3] + t[10]), 20: k * (t[20] + t[6]) / 3., 21: k * (t[21] + t[14]) / 3., 23: k * t[23] / 9.}


def element_forces(etable, ws, wk, kappa_without_c1=False):
    """damping.c:373-398 -> localForce [E, 8, 3].  kappa_without_c1: the wrong kappa = -0.5625 c2 (a test's tooth)."""
    E = len(ws)
    c1, c2 = etable[:, 0], etable[:, 1]
    kappa = -0.5625 * (c2 + (0.0 if kappa_without_c1 else 2. / 3. * c1))
    mu = -0.5625 * c1
    fv = [np.zeros(E) for _ in range(24)]
    for w, first, coef in ((ws, _first_vector_mu, mu), (wk, _first_vector_kappa, kappa)):
        live = (np.abs(w.reshape(E, 24)) > UNDERFLOW_CAP).any(axis=1)      # vector_is_zero(...) != 0, quake_util.c:49-68
        for i, add in first(_atransposeu(w), coef).items():
            fv[i] = fv[i] + np.where(live, add, 0.0)
    out = np.zeros((E, 8, 3))
    for comp in range(3):                                         # au + reformF: resVec[node].f[comp] += finVec[comp * 8 + node]
        for n in range(8):
            out[:, n, comp] = out[:, n, comp] + _signed_sum(_AU[n], fv[8 * comp:8 * comp + 8])
    return out


def bkt_forces(lnid, etable, coef, freq, dt, u1, u2, conv, force=None, conv_after_force=False, kappa_without_c1=False):
    """calc_conv + constant_Q_addforce: advances conv in place and adds the element forces to force [N, 3] (None: zeros) in
    element order.  conv_after_force: the wrong order (a test's tooth).  -> (force, ws, wk)."""
    lnid = np.asarray(lnid, np.int64)
    K = class_coef(coef, freq, dt)
    if force is None:
        force = np.zeros((len(u1), 3))
    if not conv_after_force:
        calc_conv(lnid, K, u1, u2, conv)
    ws, wk = damping_vectors(lnid, K, u1, u2, conv)
    np.add.at(force, lnid.reshape(-1), element_forces(np.asarray(etable, np.float64), ws, wk, kappa_without_c1).reshape(-1, 3))
    if conv_after_force:
        calc_conv(lnid, K, u1, u2, conv)
    return force, ws, wk


def bkt_step(lnid, etable, ntable, coef, freq, dt, u1, u2, conv, dangling=None, loaded=None, F=None, **teeth):
    """One step of solver_run under BKT from tm1 = u1, tm2 = u2 (psolve.c:4265-4319): compute_addforce_s, calc_conv,
    constant_Q_addforce, compute_adjust DISTRIBUTION, solver_compute_displacement, compute_adjust ASSIGNMENT.  conv is
    advanced in place.  -> the new displacement [N, 3] (the next step's tm1; u1 becomes its tm2)."""
    nt = np.asarray(ntable, np.float64)
    force = np.zeros((len(nt), 3))
    if loaded is not None and len(loaded):
        force[np.asarray(loaded, np.int64)] = np.asarray(F, np.float64) * (dt * dt)      # psolve.c:5917-5927: F * theDeltaTSquared
    bkt_forces(lnid, etable, coef, freq, dt, u1, u2, conv, force, **teeth)
    hanging = dangling is not None and len(dangling[0]) > 0
    if hanging:
        ho.compute_adjust(force, 0, dangling)
    force += nt[:, 1:4] * u1 - nt[:, 4:7] * u2                   # psolve.c:4086-4091
    new = np.ascontiguousarray(force / nt[:, :1])
    if hanging:
        ho.compute_adjust(new, 1, dangling)
    return new


def bkt_run(lnid, etable, ntable, coef, freq, dt, nsteps, loaded=None, forces=None, dangling=None, keep=(), observer=None):
    """nsteps from rest with forces [nsteps, nloaded, 3] (missing steps: none).  -> (tm1, tm2, conv, {step: (tm1, tm2, conv)}
    for the steps in keep, taken AFTER that many steps).  observer(s, u1, u2, conv): called after step s with the fields it
    started from and the memory variables it left."""
    N = len(ntable)
    tm1, tm2, conv = np.zeros((N, 3)), np.zeros((N, 3)), new_state(len(lnid))
    kept = {}
    for s in range(nsteps):
        F = forces[s] if forces is not None and s < len(forces) else None
        new = bkt_step(lnid, etable, ntable, coef, freq, dt, tm1, tm2, conv, dangling, loaded if F is not None else None, F)
        if observer is not None:
            observer(s, tm1, tm2, conv)
        tm1, tm2 = new, tm1
        if s + 1 in keep:
            kept[s + 1] = (tm1.copy(), tm2.copy(), conv.copy())
    return tm1, tm2, conv, kept


# ---------------------------------------------------------------------------------------------
# the slot form: one copy of the state per (node, class)
# ---------------------------------------------------------------------------------------------
def slot_plan(lnid, coef):
    """The library's plan counted independently: classes = distinct rows (bitwise) in order of first appearance, slots = the
    sorted distinct (node, class) pairs, node-major.  -> dict(rows [nc, 10], eclass [E], slot_node, slot_class, eslot [E, 8])."""
    lnid = np.asarray(lnid, np.int64)
    bits = np.ascontiguousarray(coef, np.float32).reshape(-1, 10).view(np.uint32)
    _, first, inverse = np.unique(bits, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first)                                     # classes in order of first appearance
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    eclass = rank[np.asarray(inverse).reshape(-1)]
    nc = len(order)
    key = lnid * nc + eclass[:, None]
    slots = np.unique(key)
    return dict(rows=np.ascontiguousarray(coef, np.float32).reshape(-1, 10)[first[order]], eclass=eclass.astype(np.int32),
                slot_node=(slots // nc).astype(np.int32), slot_class=(slots % nc).astype(np.int32),
                eslot=np.searchsorted(slots, key).astype(np.int32))


def corners_to_slots(plan, conv):
    """conv [4, E * 8, 3] -> mv [12, nslots] (row = variable * 3 + component); asserts that corners of one slot agree."""
    ns = len(plan["slot_node"])
    es = plan["eslot"].reshape(-1)
    mv = np.zeros((12, ns))
    for v in range(4):
        for d in range(3):
            mv[3 * v + d, es] = conv[v][:, d]
            assert np.array_equal(mv[3 * v + d, es].view(np.int64), conv[v][:, d].view(np.int64)), "corners of one slot differ"
    return mv


def slots_to_corners(plan, mv):
    """mv [12, nslots] -> conv [4, E * 8, 3]."""
    es = plan["eslot"].reshape(-1)
    return np.stack([np.stack([mv[3 * v + d, es] for d in range(3)], axis=1) for v in range(4)])


def random_state(plan, seed, scale=1e-3):
    """Independent random memory variables of the fields' size, consistent per slot -> conv [4, E * 8, 3]."""
    rng = np.random.default_rng(seed)
    ns = len(plan["slot_node"])
    mv = rng.choice([-1.0, 1.0], (12, ns)) * rng.uniform(0.5, 1.0, (12, ns)) * scale
    return slots_to_corners(plan, mv)


# ---------------------------------------------------------------------------------------------
# the extended-precision reference of one step
# ---------------------------------------------------------------------------------------------
def extended_sums(lnid, etable, coef, freq, dt, u1, u2, conv, N, kappa_without_c1=False):
    """(force [N, 3], tf [N, 3], conv_new [4, E * 8, 3]) in np.longdouble: calc_conv and constant_Q_addforce from the given
    doubles (fields, memory variables, eTable, and the class doubles class_coef forms: they are inputs of the step), through
    K1, K2; tf = the same sums of absolute products.  conv is not changed."""
    L = np.longdouble
    lnid = np.asarray(lnid, np.int64)
    E = len(lnid)
    K = class_coef(coef, freq, dt)
    U1, U2 = np.asarray(u1).astype(L)[lnid], np.asarray(u2).astype(L)[lnid]
    D = U1 - U2
    new = np.array(conv, dtype=L)
    tnew = np.abs(new)
    w, tw = [], []
    for m in range(2):
        for v in range(2):
            f = new[2 * m + v].reshape(E, 8, 3)
            tfv = tnew[2 * m + v].reshape(E, 8, 3)
            c1, c2, e = [K[k][:, m, v].astype(L)[:, None, None] for k in ("cu1", "cu2", "ex")]
            sel = K["on"][:, m]
            f[sel] = (c1 * U1 + c2 * U2 + e * f)[sel]
            tfv[sel] = (np.abs(c1 * U1) + np.abs(c2 * U2) + np.abs(e) * tfv)[sel]
        f0, f1 = new[2 * m].reshape(E, 8, 3), new[2 * m + 1].reshape(E, 8, 3)
        t0, t1 = tnew[2 * m].reshape(E, 8, 3), tnew[2 * m + 1].reshape(E, 8, 3)
        a0, a1, bq = [x.astype(L)[:, None, None] for x in (K["a"][:, m, 0], K["a"][:, m, 1], K["bq"][:, m])]
        on = K["csum_on"][:, m][:, None, None]
        w.append(np.where(on, bq * D - (a0 * f0 + a1 * f1) + U1, U1).reshape(E, 24))
        tw.append(np.where(on, np.abs(bq * D) + np.abs(a0) * t0 + np.abs(a1) * t1 + np.abs(U1), np.abs(U1)).reshape(E, 24))
    A1, A2 = [np.asarray(M).reshape(8, 8, 3, 3).transpose(0, 2, 1, 3).reshape(24, 24).astype(L) for M in ho.compute_K()]
    et = np.asarray(etable).astype(L)
    c1, c2 = et[:, 0:1], et[:, 1:2]
    two3 = L(2) / L(3)
    ck = c2 + (0 if kappa_without_c1 else two3 * c1)
    f = -(c1 * (w[0] @ A1.T) - two3 * c1 * (w[0] @ A2.T)) - ck * (w[1] @ A2.T)
    a1, a2 = np.abs(A1), np.abs(A2)
    t = np.abs(c1) * (tw[0] @ a1.T) + two3 * np.abs(c1) * (tw[0] @ a2.T) + (np.abs(c2) + two3 * np.abs(c1)) * (tw[1] @ a2.T)
    force, tf = np.zeros((N, 3), L), np.zeros((N, 3), L)
    np.add.at(force, lnid.reshape(-1), f.reshape(-1, 3))
    np.add.at(tf, lnid.reshape(-1), t.reshape(-1, 3))
    return force, tf, new


# ---------------------------------------------------------------------------------------------
# the meshes of the tests: undamped tables (under BKT compute_setab yields a = b = 0, psolve.c:5869)
# ---------------------------------------------------------------------------------------------
_MESHES = {}


def four_class_elements(nx=7, ny=5, nz=4):
    """The class (a CLASSES row) of every element of an nx x ny x nz box (ho.uniform_mesh's order): (i + 2 j + 3 k) % 4
    where i < 4, columns (i + 2 j) % 4 beyond, and class 0 in the layer k == nz - 1, so that nodes see 1, 2 and 4 classes
    (8: four_class_problem).  What the nodes see is COUNTED by classes_seen() and asserted by the tests, not taken from
    this description."""
    elem_ijk, lnid, node_ijk = ho.uniform_mesh(nx, ny, nz)
    i, j, k = [np.asarray(elem_ijk)[:, a].astype(np.int64) for a in range(3)]
    cls = np.where(i < 4, (i + 2 * j + 3 * k) % 4, (i + 2 * j) % 4)
    cls = np.where(k == nz - 1, 0, cls)
    return cls.astype(np.int64)


def four_class_problem(nx=7, ny=5, nz=4, h=20.0, vp=6000.0, vs=3464.0, rho=2700.0, freq=20.0):
    """The four-class box: undamped tables at dt = 0.5 h / Vp, coef [E, 10] from CLASSES.  In the block i, j, k < 2 the eight
    elements around node (1, 1, 1) get eight DISTINCT rows (the four classes and a twin of each with a0_shear / a0_kappa
    / b_shear moved by one float ulp, the all-zero class's twin with a0_shear = 1e-30 and a1_shear = -1e-30: csum == 0 still),
    so that node sees 8 classes."""
    key = ("four", nx, ny, nz)
    if key in _MESHES:
        return _MESHES[key]
    elem_ijk, lnid, node_ijk = ho.uniform_mesh(nx, ny, nz)
    E, N = len(lnid), len(node_ijk)
    dt = 0.5 * h / vp
    edata = np.empty((E, 4), np.float32)
    edata[:] = (h, vp, vs, rho)
    et, nt = ho.solver_init(lnid, edata, ho.face_bits(elem_ijk, nx, ny, nz), N, dt, freq, damping=ho.DAMP_NONE)
    cls = four_class_elements(nx, ny, nz)
    coef = CLASSES[cls].copy()
    ijk = np.asarray(elem_ijk).astype(np.int64)
    block = np.nonzero((ijk < 2).all(axis=1))[0]
    assert len(block) == 8
    for q, e in enumerate(block):
        c = q % 4
        coef[e] = CLASSES[c]
        if q >= 4:
            if c == 3:
                coef[e, 0], coef[e, 1] = np.float32(1e-30), np.float32(-1e-30)
            else:
                col = 5 if c == 2 else 0
                coef[e, col] = np.nextafter(coef[e, col], np.float32(1))
    p = dict(lnid=lnid, etable=et, ntable=nt, dt=dt, freq=freq, dangling=None, N=N, E=E, coef=coef, node_ijk=node_ijk,
             node_xyz=(np.asarray(node_ijk, np.int64) * (1 << 20)).astype(np.int32), shape=(nx, ny, nz))
    _MESHES[key] = p
    return p


def uniform_problem(nx=9, ny=7, nz=5, h=20.0, vp=6000.0, vs=3464.0, rho=2700.0, freq=20.0, cls=0):
    key = ("uniform", nx, ny, nz, cls)
    if key in _MESHES:
        return _MESHES[key]
    elem_ijk, lnid, node_ijk = ho.uniform_mesh(nx, ny, nz)
    E, N = len(lnid), len(node_ijk)
    dt = 0.5 * h / vp
    edata = np.empty((E, 4), np.float32)
    edata[:] = (h, vp, vs, rho)
    et, nt = ho.solver_init(lnid, edata, ho.face_bits(elem_ijk, nx, ny, nz), N, dt, freq, damping=ho.DAMP_NONE)
    p = dict(lnid=lnid, etable=et, ntable=nt, dt=dt, freq=freq, dangling=None, N=N, E=E, coef=np.tile(CLASSES[cls], (E, 1)),
             node_ijk=node_ijk, node_xyz=(np.asarray(node_ijk, np.int64) * (1 << 20)).astype(np.int32), shape=(nx, ny, nz))
    _MESHES[key] = p
    return p


def two_level_problem():
    """tests/helpers.step_mesh("two_level") with undamped tables; the fine (soft) level gets class 0, the coarse one class 1."""
    if "two_level" in _MESHES:
        return _MESHES["two_level"]
    from tests import helpers as H
    q = H.step_mesh("two_level")
    m = q["mesh"]
    et, nt = ho.solver_init(m["lnid"], q["edata"].copy(), m["face"], q["N"], q["dt"], q["freq"], damping=ho.DAMP_NONE)
    ho.compute_adjust(nt, 0, m["dangling"])
    coef = CLASSES[np.where(m["elem_size"] == 1, 0, 1)].copy()
    p = dict(lnid=q["lnid"], etable=et, ntable=nt, dt=q["dt"], freq=q["freq"], dangling=q["dangling"], N=q["N"], E=q["E"], coef=coef,
             node_xyz=q["node_q"], mesh=m)
    _MESHES["two_level"] = p
    return p


def four_class_partition(nranks=4):
    """The four-class box as an octree of one level cut into nranks ranks (ho.octree_partition, the existing partition
    helpers' route: tests/helpers._partition_mesh does the same for het70x20x12), undamped tables from ho.multi_rank_init.
    -> dict(parts, gid, ets, nts, coefs (per rank), node_xyz (per rank), glob = the one-domain problem on the octree's node
    numbering with the n_t rows the OWNERS hold)."""
    key = ("four-partition", nranks)
    if key in _MESHES:
        return _MESHES[key]
    p = four_class_problem()
    nx, ny, nz = p["shape"]
    elem_ijk, _, _ = ho.uniform_mesh(nx, ny, nz)
    ll = np.asarray(elem_ijk, np.int64)
    assert np.all(np.diff(ho.zvalue(ll[:, 0], ll[:, 1], ll[:, 2]).astype(np.int64)) > 0)       # Z-order = octor's pre-order
    corners = np.array([[(c >> 0) & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)], np.int64)
    m = ho.octree_mesh_from_elem_ticks(ll[:, None, :] + corners[None, :, :], (nx, ny, nz))
    assert len(m["dangling"][0]) == 0
    parts = ho.octree_partition(m, nranks, [nx, ny, nz])
    E, N = len(m["lnid"]), len(m["node_q"])
    edata = np.empty((E, 4), np.float32)
    edata[:] = (20.0, 6000.0, 3464.0, 2700.0)
    eds = [np.ascontiguousarray(edata[q["elems"]]) for q in parts]
    fcs = [np.ascontiguousarray(m["face"][q["elems"]]) for q in parts]
    ets, nts = ho.multi_rank_init(parts, eds, fcs, p["dt"], p["freq"], damping=ho.DAMP_NONE)
    gid = [np.asarray(q["nodes"], np.int64) for q in parts]
    etable, ntable = np.zeros((E, 4)), np.full((N, 7), np.nan)
    for q, et, nt, g in zip(parts, ets, nts, gid):
        etable[q["elems"]] = et
        own = np.asarray(q["owner"]) == q["rank"]
        ntable[g[own]] = nt[own]
    assert np.isfinite(ntable).all()
    xyz = (m["node_q"].astype(np.int64) * (1 << 20)).astype(np.int32)
    glob = dict(lnid=m["lnid"], etable=etable, ntable=ntable, dt=p["dt"], freq=p["freq"], dangling=None, N=N, E=E, coef=p["coef"],
                node_xyz=xyz)
    out = dict(parts=parts, gid=gid, ets=ets, nts=nts, coefs=[np.ascontiguousarray(p["coef"][q["elems"]]) for q in parts],
               node_xyz=[np.ascontiguousarray(xyz[g]) for g in gid], glob=glob, nranks=nranks)
    _MESHES[key] = out
    return out


def problem(name):
    return {"uniform9x7x5": uniform_problem, "four7x5x4": four_class_problem, "two_level": two_level_problem}[name]()


def classes_seen(plan, N):
    """Per node: how many slots (classes) it has."""
    return np.bincount(plan["slot_node"], minlength=N)
