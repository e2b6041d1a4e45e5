"""The reference's nonlinear soil step (include_nonlinear_analysis = yes, material_plasticity_type = rate_independant) restated,
for the nonlinear tests: no device, no library.

Set-up (nonlinear_solver_init, nonlinear.c:626-749): constants() maps edata and the property table to the nonlinear elements
and their six constants h, mu, lambda, alpha, k, hardening modulus.

Per quadrature point (compute_nonlinear_state :1671-1818 with compute_dLambdaII, compute_dfds, compute_pstrain2; the force of
compute_addforce_nl :1544-1657): dxi(), strains(), stress(), advance(), corner_forces().  Every numpy operation is one IEEE
operation per element, in the order of the C expression it restates; with L = np.longdouble the same expressions serve as the
extended reference (the inputs taken as given and widened).  Two rules: an element whose 24 values of u(t) are all within 1e-20
of zero is not advanced; where dLambda == 0 the state is kept (the reference adds 0 * dfds: NaN where J2 == 0 -- the library's
documented deviation, and the restatement's).

Two forms of the step:
  (A) step_a()  the reference's own: source, the stiffness force of the LINEAR elements (compute_addforce_effective,
                stiffness.c:180-237), damping over all elements (damping_addforce, damping.c:29-103), then
                -dt^2 sum_qp B^T sigma(e - ep) h^3 / 8 of the nonlinear ones with ep as it stood before the step's update;
                compute_adjust, solver_compute_displacement, compute_adjust.  run_a() marches it from rest.
  (B) step_b()  the correction form in the device's order: the ELASTIC step of all elements (the C oracle's), dF = +dt^2 h^3 / 8
                sum_qp B^T sigma(ep) summed per node in element order, distributed, u_new += dF / n_t[0], assigned again.
"""
import math

import numpy as np

from oracle import herc_oracle as ho
from tests.bkt_reference import _AU, _atransposeu, _signed_sum

VONMISES, DRUCKERPRAGER = 1, 2
ALPHAKAY, COHEFRICTION = 0, 1
QC = 0.577350269189                                                  # nonlinear.c:32
XI = np.array([[-1, 1, -1, 1, -1, 1, -1, 1], [-1, -1, 1, 1, -1, -1, 1, 1], [-1, -1, -1, -1, 1, 1, 1, 1]], np.float64)
UNDERFLOW_CAP = 1e-20                                                # quake_util.c:36
PI = 3.14159265358979323846264338327                                 # psolve.c:70


# ---------------------------------------------------------------------------------------------
# set-up
# ---------------------------------------------------------------------------------------------
def interpolate(props, col, vs):
    """interpolate_property_value (nonlinear.c:102-136) on column col of props [rows, 6]."""
    lim = props[:, 0]
    if vs <= lim[0]:
        return float(props[0, col])
    if vs > lim[-1]:
        return float(props[-1, col])
    vs0 = vs1 = p0 = p1 = 0.0
    for i in range(len(props) - 1):
        if lim[i] < vs <= lim[i + 1]:
            vs0, vs1, p0, p1 = float(lim[i]), float(lim[i + 1]), float(props[i, col]), float(props[i + 1, col])
    return p0 + (vs - vs0) * ((p1 - p0) / (vs1 - vs0))


def constants(edata, model, props, vs_min, vs_cut, properties=ALPHAKAY, thr_vpvs=3.0):
    """-> (elems [n] int32, cons [n, 6]).  edata [E, 4] float32 = h, Vp, Vs, rho as they stand after solver_init."""
    f = np.float32
    props = np.asarray(props, np.float64).reshape(-1, 6)
    elems, cons = [], []
    for e, (h, Vp, Vs, rho) in enumerate(np.asarray(edata, np.float32)):
        if not (float(Vs) <= vs_cut and float(Vs) >= vs_min):
            continue
        mu = float(f(f(rho * Vs) * Vs))                                                  # mu_and_lambda, psolve.c:3236-3272
        if float(Vp) > float(Vs) * thr_vpvs:
            lam = float(f(f(rho * Vs) * Vs)) * thr_vpvs * thr_vpvs - 2 * mu
        else:
            lam = float(f(f(rho * Vp) * Vp)) - 2 * mu
        if lam < 0:
            Vp = f(2.45 * float(Vs)) if Vs < 500 else f(2 * float(Vs)) if Vs < 1200 else f(1.87 * float(Vs))
            lam = float(f(f(rho * Vp) * Vp))
        assert lam >= 0
        vs = float(Vs)
        alpha = 0.0
        if properties == ALPHAKAY:
            if model == DRUCKERPRAGER:
                alpha = interpolate(props, 1, vs)
            k = interpolate(props, 2, vs)
        else:
            phi = interpolate(props, 2, vs) * PI / 180.0
            c = interpolate(props, 1, vs)
            if model == DRUCKERPRAGER:
                alpha = 2 * math.sin(phi) / (math.sqrt(3.0) * (3 - math.sin(phi)))
            k = 6 * c * math.cos(phi) / (math.sqrt(3.0) * (3 - math.sin(phi)))
        elems.append(e)
        cons.append([float(h), mu, lam, alpha, k, interpolate(props, 5, vs)])
    return np.asarray(elems, np.int32), np.asarray(cons, np.float64).reshape(-1, 6)


# ---------------------------------------------------------------------------------------------
# the quadrature points
# ---------------------------------------------------------------------------------------------
def dxi(h, L=np.float64):
    """compute_qp_dxi / point_dxi (:802-839) -> [n, 8 (node i), 8 (point j), 3]."""
    h = np.asarray(h).astype(L).reshape(-1)
    jij = L(0.25) / h
    out = np.empty((len(h), 8, 8, 3), L)
    for j in range(8):
        lx, ly, lz = [L(XI[a, j]) * L(QC) for a in range(3)]
        for i in range(8):
            x0, x1, x2 = [L(XI[a, i]) for a in range(3)]
            ax, ay, az = L(1.0) + x0 * lx, L(1.0) + x1 * ly, L(1.0) + x2 * lz
            out[:, i, j, 0] = jij * x0 * ay * az
            out[:, i, j, 1] = jij * ax * x1 * az
            out[:, i, j, 2] = jij * ax * ay * x2
    return out


def strains(U, D):
    """point_strain (:873-897) at the eight points: U [n, 8, 3], D = dxi(h) -> [n, 8 (point), 6]."""
    n = len(U)
    t = np.zeros((n, 8, 6), D.dtype)
    for i in range(8):
        dx, dy, dz = D[:, i, :, 0], D[:, i, :, 1], D[:, i, :, 2]
        ux, uy, uz = U[:, i, 0][:, None], U[:, i, 1][:, None], U[:, i, 2][:, None]
        t[:, :, 0] = t[:, :, 0] + dx * ux
        t[:, :, 1] = t[:, :, 1] + dy * uy
        t[:, :, 2] = t[:, :, 2] + dz * uz
        t[:, :, 3] = t[:, :, 3] + 0.5 * (dy * ux + dx * uy)
        t[:, :, 4] = t[:, :, 4] + 0.5 * (dz * uy + dy * uz)
        t[:, :, 5] = t[:, :, 5] + 0.5 * (dz * ux + dx * uz)
    return t


def stress(e, mu, lam, absolute=False):
    """point_stress (:904-925): e [n, 8, 6], mu / lam [n].  absolute: every product by its absolute value."""
    mu, lam = mu[:, None], lam[:, None]
    if absolute:
        e, mu, lam = np.abs(e), np.abs(mu), np.abs(lam)
    kk = (e[:, :, 0] + e[:, :, 1]) + e[:, :, 2]
    mu2 = 2.0 * mu
    lkk = lam * kk
    s = np.empty_like(e)
    for c in range(3):
        s[:, :, c] = mu2 * e[:, :, c] + lkk
    for c in range(3, 6):
        s[:, :, c] = mu2 * e[:, :, c]
    return s


def at_rest(U):
    """get_displacements == 0 (:1126-1149): all 24 values within 1e-20 of zero."""
    return ~(np.abs(np.asarray(U, np.float64).reshape(len(U), 24)) > UNDERFLOW_CAP).any(axis=1)


def advance(U, cons, pstrain, ep, L=np.float64):
    """compute_nonlinear_state on U [n, 8, 3] = u(t) at the elements' nodes -> (pstrain, ep) one step on (copies)."""
    U = np.asarray(U).astype(L)
    c = np.asarray(cons).astype(L)
    p, eb = np.array(pstrain, dtype=L), np.array(ep, dtype=L)
    mu, lam, alpha, k, hard = [c[:, q] for q in range(1, 6)]
    t = strains(U, dxi(c[:, 0], L))
    s = stress(t - p, mu, lam)
    I1 = (s[:, :, 0] + s[:, :, 1]) + s[:, :, 2]
    oct_ = I1 / L(3.0)
    d0, d1, d2 = s[:, :, 0] - oct_, s[:, :, 1] - oct_, s[:, :, 2] - oct_
    J2 = ((((d0 * d0 + d1 * d1) + d2 * d2) * L(0.5) + s[:, :, 3] * s[:, :, 3]) + s[:, :, 4] * s[:, :, 4]) + s[:, :, 5] * s[:, :, 5]
    rJ = np.sqrt(J2)
    a_ = alpha[:, None]
    Fs = a_ * I1 + rJ
    kappa = lam + (2 * mu) / 3
    phi = np.sqrt(L(1) / L(2.) + (3 * alpha) * alpha)
    FsT = (Fs - k[:, None]) - hard[:, None] * eb
    den = ((mu + ((9 * kappa) * alpha) * alpha) + hard * phi)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        dL = np.where(FsT > 0, FsT / den, L(0.0))
        two = L(2.0) * rJ
        g = np.stack([d0 / two + a_, d1 / two + a_, d2 / two + a_, s[:, :, 3] / two, s[:, :, 4] / two, s[:, :, 5] / two], axis=2)
        pn = p + dL[:, :, None] * g
        en = eb + dL * phi[:, None]
    yields = (dL != 0) & ~at_rest(U)[:, None]                            # dLambda == 0: kept as it is; at rest: not advanced
    return np.where(yields[:, :, None], pn, p), np.where(yields, en, eb)


def corner_forces(cons, dt, pstrain, L=np.float64, absolute=False, skip_point=None, no_dt2=False, tensor=None):
    """The 24 corner forces of the correction, dt^2 h^3 / 8 sum_j (B_i^T sigma(p_j)), in compute_addforce_nl's order
    (:1603-1650) -> [n, 8, 3].  tensor: the stress of THAT strain [n, 8, 6] instead of pstrain's (form A passes e - ep).
    skip_point / no_dt2: teeth."""
    c = np.asarray(cons).astype(L)
    h = c[:, 0]
    D = dxi(h, L)
    s = stress(np.asarray(pstrain if tensor is None else tensor).astype(L), c[:, 1], c[:, 2], absolute)
    if absolute:
        D = np.abs(D)
    wj = ((h * h * h) * L(0.125))[:, None]
    f = np.zeros((len(c), 8, 3), L)
    for i in range(8):
        for j in range(8):
            if j == skip_point:
                continue
            dx, dy, dz = D[:, i, j, 0], D[:, i, j, 1], D[:, i, j, 2]
            sj = s[:, j]
            f[:, i, 0] = f[:, i, 0] + (((dx * sj[:, 0] + dy * sj[:, 3]) + dz * sj[:, 5]) * wj[:, 0])
            f[:, i, 1] = f[:, i, 1] + (((dy * sj[:, 1] + dx * sj[:, 3]) + dz * sj[:, 4]) * wj[:, 0])
            f[:, i, 2] = f[:, i, 2] + (((dz * sj[:, 2] + dy * sj[:, 4]) + dx * sj[:, 5]) * wj[:, 0])
    if no_dt2:
        return f
    dt = L(float(dt))
    return f * (dt * dt)


# ---------------------------------------------------------------------------------------------
# form (A): the reference's own step
# ---------------------------------------------------------------------------------------------
def _first_vector(t, a, c, b):
    """firstVector (stiffness.c:291-319) -> list of 24 arrays."""
    z = np.zeros_like(t[1])
    return [z, b * (t[19] + t[1]), b * (t[11] + t[2]), a * t[3] + c * (t[10] + t[17]), b * (t[13] + t[22] + 2. * t[4]) / 3.,
            ((a + b) * t[5] + c * t[12]) / 3., ((a + b) * t[6] + c * t[20]) / 3., ((a + 2. * b) * t[7]) / 9.,
            z, b * (t[18] + t[9]), a * t[10] + c * (t[3] + t[17]), b * (t[11] + t[2]), ((a + b) * t[12] + c * t[5]) / 3.,
            b * (t[4] + t[22] + 2. * t[13]) / 3., ((a + b) * t[14] + c * t[21]) / 3., (a + 2. * b) * t[15] / 9.,
            z, a * t[17] + c * (t[3] + t[10]), b * (t[18] + t[9]), b * (t[19] + t[1]), ((a + b) * t[20] + c * t[6]) / 3.,
            ((a + b) * t[21] + c * t[14]) / 3., b * (t[4] + t[13] + 2. * t[22]) / 3., (a + 2. * b) * t[23] / 9.]


def stiffness_forces(etable, U):
    """compute_addforce_effective's localForce of the elements given (stiffness.c:200-226): U [n, 8, 3] -> [n, 8, 3]."""
    n = len(U)
    c1, c2 = etable[:, 0], etable[:, 1]
    a, c, b = -0.5625 * (c2 + 2 * c1), -0.5625 * c2, -0.5625 * c1
    live = (np.abs(U.reshape(n, 24)) > UNDERFLOW_CAP).any(axis=1)
    fv = _first_vector(_atransposeu(U), a, c, b)
    out = np.zeros((n, 8, 3))
    for comp in range(3):
        for node in range(8):
            out[:, node, comp] = out[:, node, comp] + np.where(live, _signed_sum(_AU[node], fv[8 * comp:8 * comp + 8]), 0.0)
    return out


def damping_forces(etable, dU, K):
    """damping_addforce's localForce (damping.c:47-87): dU [E, 8, 3] = u1 - u2 at the nodes, K = ho.compute_K()."""
    E = len(dU)
    K1, K2 = K
    c3, c4 = etable[:, 2], etable[:, 3]
    live = (np.abs(dU.reshape(E, 24)) > UNDERFLOW_CAP).any(axis=1)
    out = np.zeros((E, 8, 3))
    for i in range(8):
        for j in range(8):
            for M, c in ((K1[i][j], -c3), (K2[i][j], -c4)):               # MultAddMatVec, quake_util.c:107-122
                for row in range(3):
                    tmp = np.zeros(E)
                    for col in range(3):
                        tmp = tmp + M[row][col] * dU[:, j, col]
                    out[:, i, row] = out[:, i, row] + c * tmp
    out[~live] = 0.0
    return out


def _finish(force, ntable, u1, u2, dangling):
    """compute_adjust DISTRIBUTION, solver_compute_displacement (psolve.c:4086-4106), compute_adjust ASSIGNMENT."""
    nt = np.asarray(ntable, np.float64)
    hanging = dangling is not None and len(dangling[0]) > 0
    if hanging:
        ho.compute_adjust(force, 0, dangling)
    force = force + (nt[:, 1:4] * u1 - nt[:, 4:7] * u2)
    new = np.ascontiguousarray(force / nt[:, :1])
    if hanging:
        ho.compute_adjust(new, 1, dangling)
    return new


def step_a(p, elems, cons, u1, u2, pstrain, ep, loaded=None, F=None, K=None):
    """One step of solver_run with nonlinear soil from tm1 = u1, tm2 = u2 -> (u_new, pstrain, ep) (copies).  p: lnid, etable,
    ntable, dt, dangling."""
    lnid = np.asarray(p["lnid"], np.int64)
    et = np.asarray(p["etable"], np.float64)
    E, N, dt = len(lnid), len(p["ntable"]), p["dt"]
    K = K if K is not None else ho.compute_K()
    nl = np.zeros(E, bool)
    nl[elems] = True
    U = u1[lnid]
    # solver_nonlinear_state: pstrains1 <- pstrains2 and the strains, then the update
    rest = at_rest(U[elems])
    t = strains(U[elems], dxi(cons[:, 0]))
    p2, e2 = advance(U[elems], cons, pstrain, ep)
    force = np.zeros((N, 3))
    if loaded is not None and len(loaded):
        force[np.asarray(loaded, np.int64)] = np.asarray(F, np.float64) * (dt * dt)
    lin = np.nonzero(~nl)[0]
    np.add.at(force, lnid[lin].reshape(-1), stiffness_forces(et[lin], U[lin]).reshape(-1, 3))
    np.add.at(force, lnid.reshape(-1), damping_forces(et, U - u2[lnid], K).reshape(-1, 3))
    # compute_addforce_nl: sigma(e - ep1); an element at rest keeps the strains it had -- 0 where it never moved, all this
    # restatement carries (module docstring of csrc/hq_nonlin.h)
    fn = corner_forces(cons, dt, None, tensor=np.where(rest[:, None, None], 0.0, t) - pstrain, no_dt2=True) * (dt * dt)
    np.subtract.at(force, lnid[elems].reshape(-1), fn.reshape(-1, 3))
    return _finish(force, p["ntable"], u1, u2, p["dangling"]), p2, e2


def run_a(p, elems, cons, nsteps, loaded=None, forces=None, keep=()):
    """nsteps of form (A) from rest -> {step: (tm1, tm2, pstrain, ep)} after the steps in keep."""
    N, n = len(p["ntable"]), len(elems)
    tm1, tm2, ps, ep = np.zeros((N, 3)), np.zeros((N, 3)), np.zeros((n, 8, 6)), np.zeros((n, 8))
    K = ho.compute_K()
    kept = {}
    for s in range(nsteps):
        F = forces[s] if forces is not None and s < len(forces) else None
        new, ps, ep = step_a(p, elems, cons, tm1, tm2, ps, ep, loaded if F is not None else None, F, K)
        tm1, tm2 = new, tm1
        if s + 1 in keep:
            kept[s + 1] = (tm1.copy(), tm2.copy(), ps.copy(), ep.copy())
    return kept


# ---------------------------------------------------------------------------------------------
# form (B): the correction beside the elastic step, in the device's order
# ---------------------------------------------------------------------------------------------
def elastic_step(p, u1, u2, loaded=None, F=None):
    """The C oracle's step of ALL elements from tm1 = u1, tm2 = u2 (tests/helpers.oracle_loaded_step's way)."""
    o1, o2 = u2.copy(), u1.copy()
    kw = {}
    if loaded is not None and len(loaded):
        kw = dict(loaded_lnid=np.ascontiguousarray(loaded, np.int32), forces=np.ascontiguousarray(F, np.float64)[None])
    ho.solver_run(p["lnid"], np.ascontiguousarray(p["etable"], np.float64), np.ascontiguousarray(p["ntable"], np.float64), o1, o2, 0, 1,
                  p["dt"], dangling=p["dangling"], **kw)
    return o2


def correction(p, elems, cons, pstrain, N, no_distribution=False, **teeth):
    """dF [N, 3]: the corner forces of the state summed per node in element order (inside an element corner order) and
    distributed from the hanging nodes."""
    lnid = np.asarray(p["lnid"], np.int64)[elems]
    ef = corner_forces(cons, p["dt"], pstrain, **teeth)
    dF = np.zeros((N, 3), ef.dtype)
    np.add.at(dF, lnid.reshape(-1), ef.reshape(-1, 3))
    if p["dangling"] is not None and len(p["dangling"][0]) and not no_distribution:
        if dF.dtype == np.float64:
            ho.compute_adjust(dF, 0, p["dangling"])
        else:
            ids, ptr, anc = [np.asarray(a, np.int64) for a in p["dangling"]]
            deps = np.diff(ptr)
            np.add.at(dF, anc, np.repeat(dF[ids] / deps[:, None].astype(dF.dtype), deps, axis=0))
    return dF


def step_b(p, elems, cons, u1, u2, pstrain, ep, loaded=None, F=None, updated=False, sign=1.0, **teeth):
    """One step in the correction form -> (u_new, pstrain, ep).  updated (the force from the UPDATED plastic strain), sign,
    and correction()'s keywords plant the faults of the teeth test."""
    lnid = np.asarray(p["lnid"], np.int64)
    nt = np.asarray(p["ntable"], np.float64)
    new = elastic_step(p, u1, u2, loaded, F)
    p2, e2 = advance(u1[lnid[elems]], cons, pstrain, ep)
    dF = correction(p, elems, cons, p2 if updated else pstrain, len(nt), **teeth)
    new = np.ascontiguousarray(new + sign * dF / nt[:, :1])
    if p["dangling"] is not None and len(p["dangling"][0]):
        ho.compute_adjust(new, 1, p["dangling"])
    return new, p2, e2


def run_b(p, elems, cons, nsteps, loaded=None, forces=None, keep=()):
    """nsteps of form (B) from rest -> {step: (tm1, tm2, pstrain, ep)}."""
    N, n = len(p["ntable"]), len(elems)
    tm1, tm2, ps, ep = np.zeros((N, 3)), np.zeros((N, 3)), np.zeros((n, 8, 6)), np.zeros((n, 8))
    kept = {}
    for s in range(nsteps):
        F = forces[s] if forces is not None and s < len(forces) else None
        new, ps, ep = step_b(p, elems, cons, tm1, tm2, ps, ep, loaded if F is not None else None, F)
        tm1, tm2 = new, tm1
        if s + 1 in keep:
            kept[s + 1] = (tm1.copy(), tm2.copy(), ps.copy(), ep.copy())
    return kept


def extended(p, elems, cons, u1, u2, pstrain, loaded=None, F=None):
    """One step in np.longdouble -> (ref [N, 3], T [N, 3]): tests/helpers.extended_step of the elastic step with the
    correction's corner forces added to its element sums, T the sum of the magnitudes of all addends, the correction's
    included."""
    from tests import helpers as H
    L = np.longdouble
    N = len(p["ntable"])
    force, tf = H.extended_element_sums(p["lnid"], p["etable"], N, u1, u2)
    lnid = np.asarray(p["lnid"], np.int64)[elems]
    np.add.at(force, lnid.reshape(-1), corner_forces(cons, p["dt"], pstrain, L).reshape(-1, 3))
    np.add.at(tf, lnid.reshape(-1), corner_forces(cons, p["dt"], pstrain, L, absolute=True).reshape(-1, 3))
    return H.extended_step(p["lnid"], p["etable"], p["ntable"], u1, u2, p["dangling"], loaded=loaded, F=F, dt=p["dt"], sums=(force, tf))


def yielding_state(p, elems, cons, u1, seed, fraction=0.5):
    """A loaded state for the one-step tests: independent random plastic strains of the strains' size, and ep set per point so
    that about `fraction` of the points yield under u1: ep = (Fs - k) / s moved up or down by a tenth (hardening > 0), or --
    without hardening -- plastic strains as they are and whatever yields."""
    rng = np.random.default_rng(seed)
    n = len(elems)
    lnid = np.asarray(p["lnid"], np.int64)[elems]
    t = strains(u1[lnid], dxi(cons[:, 0]))
    scale = np.abs(t).max() if n else 0.0
    ps = rng.choice([-1.0, 1.0], (n, 8, 6)) * rng.uniform(0.25, 0.5, (n, 8, 6)) * scale
    mu, lam, alpha, k, hard = [cons[:, q] for q in range(1, 6)]
    s = stress(t - ps, mu, lam)
    I1 = (s[:, :, 0] + s[:, :, 1]) + s[:, :, 2]
    o = I1 / 3.0
    J2 = ((s[:, :, 0] - o) ** 2 + (s[:, :, 1] - o) ** 2 + (s[:, :, 2] - o) ** 2) * 0.5 + s[:, :, 3] ** 2 + s[:, :, 4] ** 2 + s[:, :, 5] ** 2
    Fs = alpha[:, None] * I1 + np.sqrt(J2)
    up = rng.uniform(size=(n, 8)) < fraction
    with np.errstate(divide="ignore", invalid="ignore"):
        ep = np.where(hard[:, None] > 0, (Fs - k[:, None]) / hard[:, None] * np.where(up, 0.9, 1.1), 0.0)
    ep = np.where(np.isfinite(ep), np.maximum(ep, 0.0), 0.0)
    return np.ascontiguousarray(ps), np.ascontiguousarray(ep)
