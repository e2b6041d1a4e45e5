"""CPU-side checks of the deformation trackers' boundary (include/hq_solver.h: hq_deform_*; include/hq_host.h:
hqh_gradient_weights, hqh_station_gradients, hqh_station_moduli, hqh_deform_fold; csrc/hq_deform.h, the one text of the
tensors and their fold): the header compiles alone as C99 and as C++17; the gradient weights sum to zero, reproduce a linear
field and are the difference quotient of hqh_stations' phi; hqh_deform_fold does what a numpy float64 restatement of the
documented order of operations does, bit for bit, for every single bit and the full mask; the fold's semantics (strictly
greater, first occurrence, zeros, NaN) and point_stress's order; the argument errors; the symbols; and what hipcc made of
hq_k_deform.  No GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hercules_amd as ha
from hercules_amd import build as hbuild
from hercules_amd import capi, host
from tests import test_code_object_cpu as CO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hercules_amd", "csrc")
NAMES = ["hq_deform_add", "hq_deform_fetch", "hq_deform_load", "hq_deform_reset", "hq_deform_clear"]
HOST_NAMES = ["hqh_gradient_weights", "hqh_station_gradients", "hqh_station_moduli", "hqh_deform_fold"]
HQ_ERR_ARG = -1
E, ER, S, W, WR = (capi.HQ_DEFORM_STRAIN, capi.HQ_DEFORM_STRAIN_RATE, capi.HQ_DEFORM_STRESS, capi.HQ_DEFORM_ROTATION,
                   capi.HQ_DEFORM_ROTATION_RATE)
ALL = capi.HQ_DEFORM_ALL
U = 2.0 ** -53
SIGN = np.array([[1.0 if c & (1 << a) else -1.0 for c in range(8)] for a in range(3)])      # s_a(c)


@pytest.fixture(scope="module")
def libs():
    hbuild.build()
    return ha.load_library(), capi.load_library(precision="f32")


# ---------------------------------------------------------------------------------------------------------------------
# the boundary
# ---------------------------------------------------------------------------------------------------------------------

def test_header_compiles_alone_as_c99_and_as_cpp17(tmp_path):
    src = '#include "hq_deform.h"\nint hq_deform_probe(void) { return hq_deform_nvals(HQ_DEFORM_ALL) + hq_deform_nwhen(31); }\n'
    for name, cmd in (("probe.c", ["gcc", "-std=c99", "-pedantic"]), ("probe.cpp", ["g++", "-std=c++17"])):
        f = tmp_path / name
        f.write_text(src)
        subprocess.check_call(cmd + ["-Wall", "-Wextra", "-Werror", "-I", CSRC, "-c", "-o", str(tmp_path / (name + ".o")), str(f)])


def test_header_declares_and_both_libraries_export_the_entry_points(libs):
    txt = open(os.path.join(ROOT, "include", "hq_solver.h")).read()
    declared = re.findall(r"HQ_API\s+[\w\s\*]+?\b(hq\w+)\s*\(", txt)
    for n in NAMES:
        assert n in declared, n
        for lib in libs:
            assert hasattr(lib, n), n
    assert set(NAMES) <= set(capi.EXPORTS)
    htxt = open(os.path.join(ROOT, "include", "hq_host.h")).read()
    hlib = host.load_library()
    for n in HOST_NAMES:
        assert re.search(r"HQ_API\s+int\s+%s\s*\(" % n, htxt), n
        assert n in host.EXPORTS and hasattr(hlib, n), n
    assert libs[0].hq_abi_version() == 6 and libs[1].hq_abi_version() == 6      # additive: no ABI bump
    assert (E, ER, S, W, WR, ALL) == (1, 2, 4, 8, 16, 31)
    for word, value in (("STRAIN", 1), ("STRAIN_RATE", 2), ("STRESS", 4), ("ROTATION", 8), ("ROTATION_RATE", 16)):
        for path in (os.path.join(ROOT, "include", "hq_solver.h"), os.path.join(CSRC, "hq_deform.h")):
            assert re.search(r"HQ_DEFORM_%s = %d\b" % (word, value), open(path).read()), (word, path)


def test_null_context_is_a_bad_argument(libs):
    for lib in libs:
        ids, g = (ctypes.c_int32 * 8)(), (ctypes.c_double * 24)()
        d = capi._DeformDesc(1, ctypes.cast(ids, ctypes.c_void_p), ctypes.cast(g, ctypes.c_void_p), None, 1, 0, E, 0)
        h, n = ctypes.c_int32(), ctypes.c_int64()
        v, w = (ctypes.c_double * 10)(), (ctypes.c_int32 * 2)()
        assert lib.hq_deform_add(None, ctypes.byref(d), ctypes.byref(h)) == HQ_ERR_ARG
        assert lib.hq_deform_fetch(None, ctypes.c_int32(0), v, w, ctypes.byref(n)) == HQ_ERR_ARG
        assert lib.hq_deform_load(None, ctypes.c_int32(0), v, w, ctypes.c_int64(0)) == HQ_ERR_ARG
        assert lib.hq_deform_reset(None, ctypes.c_int32(0)) == HQ_ERR_ARG
        assert lib.hq_deform_clear(None) == HQ_ERR_ARG


def test_descriptor_mirrors_the_header(libs, tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hq_host.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(hq_deform_desc), offsetof(hq_deform_desc, ids), '
                   'offsetof(hq_deform_desc, grad), offsetof(hq_deform_desc, lame), offsetof(hq_deform_desc, rate), '
                   'offsetof(hq_deform_desc, quantities)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], universal_newlines=True).split()]
    D = capi._DeformDesc
    assert got == [ctypes.sizeof(D), D.ids.offset, D.grad.offset, D.lame.offset, D.rate.offset, D.quantities.offset]
    assert got[0] == 48


# ---------------------------------------------------------------------------------------------------------------------
# hqh_gradient_weights, hqh_station_gradients, hqh_station_moduli
# ---------------------------------------------------------------------------------------------------------------------

# local coordinates: the centre, an interior point, a point on an element face (x = +1), a corner of the cube -- all dyadic
LCS = [(0.0, 0.0, 0.0), (0.25, -0.5, 0.375), (1.0, 0.125, -0.75), (-1.0, 1.0, 1.0)]
EDGES = [62.5, 31.25]


@pytest.mark.parametrize("h", EDGES)
@pytest.mark.parametrize("lc", LCS)
def test_weights_sum_to_zero_and_are_the_documented_product(h, lc):
    g = host.gradient_weights(h, lc)
    assert g.shape == (3, 8)
    for b in range(3):
        a1, a2 = [a for a in range(3) if a != b]
        want = SIGN[b] * ((1 + SIGN[a1] * lc[a1]) * (1 + SIGN[a2] * lc[a2]) / (4 * h))
        assert np.array_equal(g[b], want), (b, g[b], want)
        for c in range(8):                                   # the two corners that differ in axis b alone cancel exactly
            assert g[b][c] == -g[b][c ^ (1 << b)]
        assert abs(g[b].sum()) <= 8 * U * np.abs(g[b]).sum()
        assert sum(g[b][c] + g[b][c ^ (1 << b)] for c in range(8)) == 0.0
    assert np.abs(g).sum() > 0


@pytest.mark.parametrize("h", EDGES)
@pytest.mark.parametrize("lc", LCS)
def test_weights_reproduce_a_linear_field(h, lc):
    """u = A x + c on an element of edge h whose near corner is at a dyadic position: every nodal value is exact, and G[b][a]
    = sum_c g[b][c] u_a[c], summed in hq_sample.h's order, is A[a][b] within 8 x 2^-53 sum_c |g_bc| |u_a[c]|."""
    A = np.array([[0.5, -1.25, 2.0], [3.0, 0.75, -0.125], [-2.5, 1.5, 0.25]])
    cst = np.array([4.0, -8.0, 0.5])
    corner0 = h * np.array([3.0, 5.0, 2.0])
    xyz = corner0[None, :] + h * (0.5 * (SIGN.T + 1.0))      # [8, 3]
    u = xyz @ A.T + cst[None, :]                             # u[c][a]
    assert np.array_equal(u, np.array([[sum(A[a][b] * xyz[c][b] for b in range(3)) + cst[a] for a in range(3)] for c in range(8)]))
    g = host.gradient_weights(h, lc)
    for b in range(3):
        for a in range(3):
            acc = 0.0
            for c in range(8):
                acc = acc + g[b][c] * u[c][a]
            bound = 8 * U * float(np.sum(np.abs(g[b]) * np.abs(u[:, a])))
            assert abs(acc - A[a][b]) <= bound, (b, a, acc, A[a][b], bound)


@pytest.fixture(scope="module", params=EDGES)
def box(request):
    h = request.param
    layers = [(0.0, 2000.0, 400.0, 1800.0), (2.5 * h, 4500.0, 2600.0, 2400.0), (5.5 * h, 6000.0, 3464.0, 2700.0)]
    b = host.Box(8, 8, 8, h, 1e-3, 5.0, layers=layers)
    yield b
    b.close()


def test_station_gradients_are_the_difference_quotient_of_phi(box):
    """hqh_stations' phi is linear in each coordinate, so its central difference over +- d inside the element IS the
    derivative, up to the rounding of phi: each phi <= 1 carries at most 6 roundings (three 1 + s lc, two products, one
    division), the difference one more -- 16 x 2^-53 / (2 d) covers the quotient.  On an element face the quotient along the
    face's normal is taken one-sided, into the element the point is located in (as exact, for a linear function).  The ids
    and `mine` are hqh_stations' own."""
    h = box.h
    centre = h * (np.array([3.0, 4.0, 2.0]) + 0.5)
    pts = np.array([centre + 0.5 * h * np.array(lc) for lc in LCS[:3]] + [h * (np.array([i, j, 0.0]) + 0.5) for i in (0, 7) for j in (0, 7)])
    ids, grad, mine = box.station_gradients(pts)
    ids0, phi0, mine0 = box.stations(pts)
    assert np.array_equal(ids, ids0) and np.array_equal(mine, mine0) and mine.all()
    d = h / 8
    for p, x in enumerate(pts):
        e = np.floor(x / h)
        lc = 2 * (x - (e + 0.5) * h) / h
        assert np.array_equal(grad[p], host.gradient_weights(h, lc))
        for b in range(3):
            lo, hi = x.copy(), x.copy()
            lo[b] -= d
            hi[b] += d
            if lo[b] < e[b] * h:                             # on the element's near face: one-sided, into the element
                lo[b] = x[b]
            i2, phi2, _ = box.stations(np.array([lo, hi]))
            assert np.array_equal(i2[0], ids[p]) and np.array_equal(i2[1], ids[p])
            quot = (phi2[1] - phi2[0]) / (hi[b] - lo[b])
            assert np.abs(quot - grad[p][b]).max() <= 16 * U / (hi[b] - lo[b]), (p, b, quot, grad[p][b])
    with pytest.raises(ha.HqError):
        box.station_gradients([(-1.0, 10.0, 10.0)])
    assert box.station_gradients(np.zeros((0, 3)))[1].shape == (0, 3, 8)


def test_station_moduli_are_mu_and_lambda_of_the_element(box):
    """mu = rho Vs Vs in float, lambda = rho Vp Vp (float) - 2 mu, with the Vp / Vs cap at threshold_vpvs = 3 (the soft top
    layer: Vp / Vs = 5), as mu_and_lambda computes them; and c1 = dt^2 h mu / 9, c2 = dt^2 h lambda / 9 of the element table
    are formed from these very numbers."""
    h = box.h
    pts = np.array([h * (np.array([3.0, 4.0, k]) + 0.5) for k in range(8)] + [h * np.array([8.0, 8.0, 8.0])])
    lame = box.station_moduli(pts)
    assert lame.shape == (9, 2)
    f = np.float32
    for k in range(9):
        kk = min(k, 7)
        vp, vs, rho = (2000.0, 400.0, 1800.0) if (kk + 0.5) < 2.5 else (4500.0, 2600.0, 2400.0) if (kk + 0.5) < 5.5 else (6000.0, 3464.0, 2700.0)
        mu = float(f(rho) * f(vs) * f(vs))
        if vp > vs * 3.0:
            lam = float(f(rho) * f(vs) * f(vs)) * 3.0 * 3.0 - 2 * mu
        else:
            lam = float(f(rho) * f(vp) * f(vp)) - 2 * mu
        assert lam > 0 and (lame[k] == (lam, mu)).all(), (k, lame[k], lam, mu)
    ids, _, _ = box.stations(pts[:8])
    elem = [int(np.nonzero((box.lnid == ids[k]).all(axis=1))[0][0]) for k in range(8)]
    hf, dt2 = float(f(h)), 1e-3 * 1e-3
    for k in range(8):
        assert box.etable[elem[k], 0] == dt2 * hf * lame[k, 1] / 9 and box.etable[elem[k], 1] == dt2 * hf * lame[k, 0] / 9
    with pytest.raises(ha.HqError):
        box.station_moduli([(0.0, 0.0, 9 * h)])


def test_argument_errors_of_the_host_functions(box):
    lib = host.load_library()
    g, lc = (ctypes.c_double * 24)(), (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    assert lib.hqh_gradient_weights(ctypes.c_double(62.5), lc, g) == 0
    assert lib.hqh_gradient_weights(ctypes.c_double(62.5), None, g) == HQ_ERR_ARG
    assert lib.hqh_gradient_weights(ctypes.c_double(62.5), lc, None) == HQ_ERR_ARG
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.hqh_gradient_weights(ctypes.c_double(bad), lc, g) == HQ_ERR_ARG
    assert lib.hqh_gradient_weights(ctypes.c_double(62.5), (ctypes.c_double * 3)(0.0, float("nan"), 0.0), g) == HQ_ERR_ARG
    xyz, ids, mine, lame = (ctypes.c_double * 3)(10.0, 10.0, 10.0), (ctypes.c_int32 * 8)(), (ctypes.c_int32 * 1)(), (ctypes.c_double * 2)()
    assert lib.hqh_station_gradients(box._h, 1, xyz, ids, g, mine) == 0
    assert lib.hqh_station_gradients(None, 1, xyz, ids, g, mine) == HQ_ERR_ARG
    assert lib.hqh_station_gradients(box._h, -1, xyz, ids, g, mine) == HQ_ERR_ARG
    assert lib.hqh_station_gradients(box._h, 1, None, ids, g, mine) == HQ_ERR_ARG
    assert lib.hqh_station_gradients(box._h, 1, xyz, None, g, mine) == HQ_ERR_ARG
    assert lib.hqh_station_gradients(box._h, 1, xyz, ids, None, mine) == HQ_ERR_ARG
    assert lib.hqh_station_gradients(box._h, 1, xyz, ids, g, None) == HQ_ERR_ARG
    assert lib.hqh_station_gradients(box._h, 0, None, None, None, None) == 0
    assert lib.hqh_station_moduli(box._h, 1, xyz, lame) == 0
    assert lib.hqh_station_moduli(None, 1, xyz, lame) == HQ_ERR_ARG
    assert lib.hqh_station_moduli(box._h, -1, xyz, lame) == HQ_ERR_ARG
    assert lib.hqh_station_moduli(box._h, 1, None, lame) == HQ_ERR_ARG
    assert lib.hqh_station_moduli(box._h, 1, xyz, None) == HQ_ERR_ARG
    assert lib.hqh_station_moduli(box._h, 0, None, None) == 0
    outside = (ctypes.c_double * 3)(10.0, -10.0, 10.0)
    assert lib.hqh_station_gradients(box._h, 1, outside, ids, g, mine) == HQ_ERR_ARG
    assert lib.hqh_station_moduli(box._h, 1, outside, lame) == HQ_ERR_ARG
    # hqh_deform_fold
    st, gs, v, w = (ctypes.c_int32 * 1)(), (ctypes.c_double * 18)(), (ctypes.c_double * 40)(), (ctypes.c_int32 * 10)()
    lm = (ctypes.c_double * 2)(1.0, 1.0)
    assert lib.hqh_deform_fold(1, ALL, lm, 1, st, gs, v, w) == 0
    assert lib.hqh_deform_fold(1, 0, lm, 1, st, gs, v, w) == HQ_ERR_ARG
    assert lib.hqh_deform_fold(1, 32, lm, 1, st, gs, v, w) == HQ_ERR_ARG
    assert lib.hqh_deform_fold(1, ALL | 64, lm, 1, st, gs, v, w) == HQ_ERR_ARG
    assert lib.hqh_deform_fold(-1, ALL, lm, 1, st, gs, v, w) == HQ_ERR_ARG
    assert lib.hqh_deform_fold(1, ALL, lm, -1, st, gs, v, w) == HQ_ERR_ARG
    assert lib.hqh_deform_fold(1, ALL, None, 1, st, gs, v, w) == HQ_ERR_ARG      # STRESS without moduli
    assert lib.hqh_deform_fold(1, ALL & ~S, None, 1, st, gs, v, w) == 0           # ... which no other bit reads
    for bad in ((float("nan"), 1.0), (float("inf"), 1.0), (1.0, float("nan")), (1.0, float("-inf")), (1.0, -1e-300)):
        assert lib.hqh_deform_fold(1, S, (ctypes.c_double * 2)(*bad), 1, st, gs, v, w) == HQ_ERR_ARG
    assert lib.hqh_deform_fold(1, S, (ctypes.c_double * 2)(-1.0, 0.0), 1, st, gs, v, w) == 0     # (lambda < 0 is a material)
    assert lib.hqh_deform_fold(1, ALL, lm, 1, None, gs, v, w) == HQ_ERR_ARG
    assert lib.hqh_deform_fold(1, ALL, lm, 1, st, None, v, w) == HQ_ERR_ARG
    assert lib.hqh_deform_fold(1, ALL, lm, 1, st, gs, None, w) == HQ_ERR_ARG
    assert lib.hqh_deform_fold(1, ALL, lm, 1, st, gs, v, None) == HQ_ERR_ARG
    assert lib.hqh_deform_fold(0, ALL, None, 1, None, None, None, None) == 0
    assert lib.hqh_deform_fold(1, E, None, 0, None, None, None, None) == 0
    with pytest.raises(ha.HqError):
        host.deform_fold([0], np.zeros((1, 2, 2, 3, 2)), E)
    with pytest.raises(ha.HqError):
        host.deform_fold([0], np.zeros((1, 2, 2, 3, 3)), E, vals=np.zeros((2, 5)), when=np.zeros((2, 2), np.int32))


# ---------------------------------------------------------------------------------------------------------------------
# hqh_deform_fold against a numpy restatement
# ---------------------------------------------------------------------------------------------------------------------

def _strain(G):
    """G [..., 3, 3] = G[b][a] -> (xx, yy, zz, xy, yz, xz), the documented expressions."""
    half = G.dtype.type(0.5)
    return [G[..., 0, 0], G[..., 1, 1], G[..., 2, 2], half * (G[..., 1, 0] + G[..., 0, 1]), half * (G[..., 2, 1] + G[..., 1, 2]),
            half * (G[..., 2, 0] + G[..., 0, 2])]


def _rotation(G):
    half = G.dtype.type(0.5)
    return [half * (G[..., 1, 2] - G[..., 2, 1]), half * (G[..., 2, 0] - G[..., 0, 2]), half * (G[..., 0, 1] - G[..., 1, 0])]


def _stress(e, lam, mu):
    mu2 = mu.dtype.type(2) * mu
    lkk = lam * ((e[0] + e[1]) + e[2])
    return [mu2 * e[0] + lkk, mu2 * e[1] + lkk, mu2 * e[2] + lkk, mu2 * e[3], mu2 * e[4], mu2 * e[5]]


def _tensor_measures(t):
    """The ten candidates of a tensor's block; [7] raises when[0], [6] raises when[1]."""
    xx, yy, zz, xy, yz, xz = t
    six, four = xx.dtype.type(6.0), xx.dtype.type(4.0)
    dxy, dyz, dzx = xx - yy, yy - zz, zz - xx
    j2 = ((dxy * dxy + dyz * dyz) + dzx * dzx) + six * ((xy * xy + yz * yz) + xz * xz)
    return [np.abs(v) for v in t] + [np.abs((xx + yy) + zz), j2, dxy * dxy + four * (xy * xy), np.abs(xx + yy)], (7, 6)


def _vector_measures(w):
    x, y, z = w
    hz = x * x + y * y
    return [np.abs(x), np.abs(y), np.abs(z), hz, hz + z * z], (3, 4)


def numpy_fold(steps, gs, q, lame=None, dtype=np.float64):
    """The definition in numpy arrays of `dtype` over the points, sample by sample; numpy never contracts a product into a
    sum.  Returns (vals [np, nvals], when [np, nwhen])."""
    gs = np.asarray(gs, dtype)
    npts = gs.shape[1]
    blocks = [b for b in (E, ER, S, W, WR) if q & b]
    vals = [np.zeros((npts, 10 if b in (E, ER, S) else 5), dtype) for b in blocks]
    when = [np.full((npts, 2), -1, np.int32) for b in blocks]
    if q & S:
        lam, mu = np.asarray(lame[:, 0], dtype), np.asarray(lame[:, 1], dtype)
    for k, step in enumerate(steps):
        G, R = gs[k, :, 0], gs[k, :, 1]
        for i, b in enumerate(blocks):
            if b == E:
                cand, wcols = _tensor_measures(_strain(G))
            elif b == ER:
                cand, wcols = _tensor_measures(_strain(R))
            elif b == S:
                cand, wcols = _tensor_measures(_stress(_strain(G), lam, mu))
            else:
                cand, wcols = _vector_measures(_rotation(G if b == W else R))
            for j, c in enumerate(cand):
                with np.errstate(invalid="ignore"):
                    up = c > vals[i][:, j]                   # strictly greater; False for a NaN
                vals[i][up, j] = c[up]
                if j in wcols:
                    when[i][up, wcols.index(j)] = step
    return np.concatenate(vals, axis=1), np.concatenate(when, axis=1)


NSAMPLES, NPOINTS = 40, 50


def _case():
    """40 samples x 50 points of random gradients and rate gradients at steps 3, 6, ...; strains of 1e-4, rates of 1e-2;
    exact zeros strewn in, point 1 all zero, point 2 repeats one sample (a tie must not move `when`); moduli of rock."""
    rng = np.random.default_rng(20261020)
    steps = (3 * (1 + np.arange(NSAMPLES))).astype(np.int32)
    gs = rng.uniform(-1.0, 1.0, (NSAMPLES, NPOINTS, 2, 3, 3))
    gs[:, :, 0] *= 1e-4
    gs[:, :, 1] *= 1e-2
    gs[rng.uniform(size=gs.shape) < 0.05] = 0.0
    gs[:, 1] = 0.0
    gs[:, 2] = gs[0, 2]
    lame = np.stack([rng.uniform(1e9, 4e10, NPOINTS), rng.uniform(1e8, 3e10, NPOINTS)], axis=1)
    lame[3] = (-2e9, 5e9)                                    # a negative lambda is a material, too
    lame[4] = (1e10, 0.0)                                    # a fluid
    return steps, gs, lame


@pytest.mark.parametrize("q", [E, ER, S, W, WR, ALL, E | W, ER | S | WR])
def test_fold_equals_the_numpy_restatement(q):
    steps, gs, lame = _case()
    vals, when = host.deform_fold(steps, gs, q, lame if q & S else None)
    want = numpy_fold(steps, gs, q, lame)
    nt, nv = bin(q & 7).count("1"), bin(q & 24).count("1")
    assert vals.shape == (NPOINTS, 10 * nt + 5 * nv) and when.shape == (NPOINTS, 2 * (nt + nv))
    assert np.array_equal(when, want[1]), np.argwhere(when != want[1])[:5]
    assert np.array_equal(vals, want[0]), np.argwhere(vals != want[0])[:5]
    assert (vals[1] == 0).all() and (when[1] == -1).all()              # the all-zero point
    assert (when[2] == steps[0]).all() and (vals[2] > 0).any()         # the repeated sample: its first occurrence
    assert (vals[[0, 3] + list(range(5, NPOINTS))] > 0).all()
    if q == S:                                               # the fluid: a pressure and no shear
        assert (vals[4, 3:6] == 0).all() and vals[4, 7] == 0 and vals[4, 8] == 0 and (vals[4, [0, 1, 2, 6, 9]] > 0).all()
        assert when[4, 0] == -1 and when[4, 1] > 0
    # two calls in sequence equal one on the concatenation
    v2, w2 = host.deform_fold(steps[:17], gs[:17], q, lame if q & S else None)
    again = host.deform_fold(steps[17:], gs[17:], q, lame if q & S else None, v2, w2)
    assert again[0] is v2 and np.array_equal(v2, vals) and np.array_equal(w2, when)


def test_fold_is_within_a_few_ulp_of_a_longdouble_restatement():
    """A check of the formulas, not of the bits: the same fold in np.longdouble.  Every value is a maximum over the samples
    of an expression of at most four levels of additions of rounded products, so it lies within 16 x 2^-53 of the exact one
    relative to the sum of the magnitudes that enter it: S = 6 max |G| for a strain or a rotation, (2 mu + 3 |lambda|) S
    for a stress, and S^2 (x 6) for the squared measures."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is no wider than float64 here")
    steps, gs, lame = _case()
    vals, when = host.deform_fold(steps, gs, ALL, lame)
    ref, _ = numpy_fold(steps, gs, ALL, lame, dtype=np.longdouble)
    sg, sr = 6 * np.abs(gs[:, :, 0]).max(axis=(0, 2, 3)), 6 * np.abs(gs[:, :, 1]).max(axis=(0, 2, 3))
    ss = (2 * lame[:, 1] + 3 * np.abs(lame[:, 0])) * sg
    scales = []
    for s in (sg, sr, ss):
        scales += [s] * 7 + [6 * s * s, 6 * s * s, s]
    for s in (sg, sr):
        scales += [s] * 3 + [s * s] * 2
    scale = np.stack(scales, axis=1)
    err = np.abs(vals.astype(np.longdouble) - ref).astype(np.float64)
    assert (err <= 16 * U * scale).all(), np.argwhere(err > 16 * U * scale)[:5]
    nz = ref != 0
    rel = (err[nz] / np.abs(ref[nz]).astype(np.float64)).max()
    print("largest relative difference to the longdouble fold: %.3e" % rel)


# ---------------------------------------------------------------------------------------------------------------------
# the fold's semantics
# ---------------------------------------------------------------------------------------------------------------------

def _g(xx=0.0, yy=0.0, zz=0.0, g10=0.0, g01=0.0, g21=0.0, g12=0.0, g20=0.0, g02=0.0):
    return np.array([[xx, g01, g02], [g10, yy, g12], [g20, g21, zz]])       # G[b][a]


def _samples(gs, rs=None):
    gs = np.array(gs)
    out = np.zeros((len(gs), 1, 2, 3, 3))
    out[:, 0, 0] = gs
    if rs is not None:
        out[:, 0, 1] = np.array(rs)
    return out


def test_fold_semantics_strictly_greater_first_occurrence_zero_and_nan():
    big, small = _g(xx=2e-4, g10=1e-4, g01=3e-4), _g(xx=1e-4, yy=1e-5)
    steps = np.array([5, 6, 7, 8, 9], np.int32)
    vals, when = host.deform_fold(steps, _samples([small, big, big, small, -big]), E)
    assert (when[0] == (6, 6)).all()                          # the first of the equal maxima, and -big raises nothing
    assert vals[0, 0] == 2e-4 and vals[0, 3] == 0.5 * (1e-4 + 3e-4) and vals[0, 6] == 2e-4 and vals[0, 9] == 2e-4
    # zeros (and negative zeros) enter nothing
    z = _samples([np.zeros((3, 3)), -np.zeros((3, 3))], [np.zeros((3, 3)), np.zeros((3, 3))])
    vals, when = host.deform_fold([0, 1], z, ALL, np.array([[1e10, 1e10]]))
    assert (vals == 0).all() and (when == -1).all() and not np.signbit(vals).any()
    # a NaN never enters, whatever it stands in, and what is finite beside it still does
    nan = _g(xx=float("nan"), yy=1e-4, g21=2e-4, g12=2e-4)
    vals, when = host.deform_fold([3, 4], _samples([nan, small], [nan, small]), ALL, np.array([[1e10, 1e10]]))
    assert np.isfinite(vals).all()
    assert vals[0, 1] == 1e-4 and vals[0, 4] == 2e-4         # |yy| and |yz| of the NaN sample
    assert vals[0, 0] == 1e-4 and (when[0, :2] == (4, 4)).all()          # xx, 6 J2 and the volume only from the clean sample
    assert (when[0, 2:6] == (4, 4, 4, 4)).all()
    # a pure rotation strains nothing; a pure strain rotates nothing
    spin = _g(g10=-1e-4, g01=1e-4, g21=2e-4, g12=-2e-4)
    vals, when = host.deform_fold([7], _samples([spin]), E | W)
    assert (vals[0, :10] == 0).all() and (when[0, :2] == -1).all()
    assert vals[0, 10] == 2e-4 and vals[0, 11] == 0.0 and vals[0, 12] == 1e-4 and vals[0, 13] == 2e-4 * 2e-4 and (when[0, 2:] == (7, 7)).all()
    vals, when = host.deform_fold([7], _samples([_g(g10=1e-4, g01=1e-4)]), E | W)
    assert vals[0, 3] == 1e-4 and (vals[0, 10:] == 0).all() and (when[0, 2:] == -1).all()


def test_the_measures_of_a_known_tensor():
    """xx = 3, yy = 1, zz = -2, xy = 0.5 (1 + 2), yz = 0.5 (4 + 0), xz = 0.5 (-1 - 1), small integers and halves: exact."""
    G = _g(xx=3.0, yy=1.0, zz=-2.0, g10=1.0, g01=2.0, g21=4.0, g12=0.0, g20=-1.0, g02=-1.0)
    vals, when = host.deform_fold([11], _samples([G]), E | W)
    assert list(vals[0, :6]) == [3.0, 1.0, 2.0, 1.5, 2.0, 1.0]
    assert vals[0, 6] == 2.0 and vals[0, 9] == 4.0
    assert vals[0, 7] == (4.0 + 9.0 + 25.0) + 6.0 * (2.25 + 4.0 + 1.0)
    assert vals[0, 8] == 4.0 + 4.0 * 2.25
    assert list(vals[0, 10:13]) == [2.0, 0.0, 0.5]            # wx = 0.5 (0 - 4), wy = 0.5 (-1 + 1), wz = 0.5 (2 - 1)
    assert vals[0, 13] == 4.0 and vals[0, 14] == 4.25 and (when[0] == 11).all()


def test_stress_is_formed_in_point_stress_order():
    """mu2 e_aa + lkk with both products rounded first: a case in which the FMA forms of either product give other bits, and
    in which 2 (mu e) differs from (2 mu) e never (a power of two) -- the value is that of the documented order in Python
    floats."""
    lam, mu = 1.2345678901234567e10, 3.3333333333333335e9
    G = _g(xx=1.1e-4 / 3, yy=-0.7e-4 / 3, zz=0.9e-4 / 7, g10=1e-5 / 3, g01=2e-5 / 7)
    vals, _ = host.deform_fold([1], _samples([G]), S, np.array([[lam, mu]]))
    xx, yy, zz = float(G[0, 0]), float(G[1, 1]), float(G[2, 2])
    xy = 0.5 * (float(G[1, 0]) + float(G[0, 1]))
    mu2 = 2 * mu
    lkk = lam * ((xx + yy) + zz)
    s = [mu2 * xx + lkk, mu2 * yy + lkk, mu2 * zz + lkk, mu2 * xy]
    assert [vals[0, j] for j in range(4)] == [abs(v) for v in s]
    assert vals[0, 6] == abs((s[0] + s[1]) + s[2]) and vals[0, 9] == abs(s[0] + s[1])


# ---------------------------------------------------------------------------------------------------------------------
# the code object
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("so", ["libhq_solver.so", "libhq_solver_f32.so"])
def test_deform_kernel_has_no_spill_and_no_scratch(libs, tmp_path, monkeypatch, so):
    """hq_k_deform holds 24 weights, 24 gathered values and 18 sums per lane: no spilled register, no scratch, no LDS, and no
    more than 256 VGPRs (two waves per SIMD)."""
    path = os.path.join(CSRC, so)
    assert os.path.exists(path), path
    monkeypatch.setattr(sys.modules[CO.__name__], "SO", path)
    k = CO._kernel_notes(tmp_path)
    found = [v for name, v in k.items() if "hq_k_deform" in name]
    assert len(found) == 1, sorted(k)
    v = found[0]
    assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, v
    assert v["group_segment_fixed_size"] == 0 and v["vgpr_count"] <= 256, v
