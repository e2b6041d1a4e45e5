#!/usr/bin/env python3
"""Generate the BKT fixtures tests/golden/c1_bkt.npz and c5_two_level_bkt.npz from the REAL reference run with
type_of_damping = bkt (make_golden.run_reference; needs the reference tree and oracle/_ref/psolve, as make_golden.py does).
Nothing here is imported by the tests; they read the .npz files this script wrote.

Each fixture holds what its Rayleigh sibling holds (mesh dump, force file, two checkpoints) without the station traces, and
  freq   Param.theFreq
  coef   [E, 10] float32: the ten attenuation coefficients per element in edata_t's order (psolve.h:96), as NUMBERS.
They are derived HERE, at generation time, the way mesh_correct_properties does (psolve.c:7239-7311): Qs from the element's
Vs, Qp = 2 Qs, Qk from both, and the row of the reference's quality-factor table that Search_Quality_Table (quake_util.c:128-163)
picks -- the table itself is read out of the reference's source text when this script runs and is kept nowhere in this
repository.  (The reference loads 18 of its rows into a zeroed array of 26, so a Q beyond the last loaded row falls on that
row: c1's Qs = 403 gets the 120 row.  That is pinned as it is.)  simulation_velocity_profile_freq_hz = 0: no velocity
correction; use_infinite_qk = no.

Usage: python tests/golden/make_golden_attenuation.py [c1_bkt] [c5_two_level_bkt]
"""
import os
import re
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402


def quality_table():
    """The table as constract_Quality_Factor_Table leaves it in Global.theQTABLE: parsed from the reference's psolve.c."""
    text = open(os.path.join(G.REF, "quake", "forward", "psolve.c")).read()
    body = re.search(r"local_QTABLE\[(\d+)\]\[6\]\s*=\s*\{(.*?)\};", text, re.S)
    rows = [[float(v) for v in r.replace("\n", " ").split(",")] for r in re.findall(r"\{([^{}]*)\}", body.group(2))]
    loaded = int(re.search(r"for\s*\(\s*i\s*=\s*0;\s*i\s*<\s*(\d+);\s*i\+\+\s*\)\s*\{\s*for\s*\(\s*j\s*=\s*0;\s*j\s*<\s*6", text).group(1))
    size = int(re.search(r"theQTABLE\[(\d+)\]\[6\];", text).group(1))
    table = np.zeros((size, 6))
    table[:loaded] = np.array(rows)[:loaded]
    return table


def search(Q, table):
    """Search_Quality_Table, quake_util.c:128-163."""
    if not Q <= 500:
        return -1
    best = 1000.0
    for i in range(len(table)):
        diff = abs(Q - table[i, 0])
        if diff < best:
            best = diff
        else:
            return i - 1
    return -2


def coefficients(mat_vs_vp_rho, table):
    """psolve.c:7239-7311 per element -> [E, 10] float32 (edata_t's fields are floats)."""
    out = np.zeros((len(mat_vs_vp_rho), 10), np.float32)
    for e, (Vs, Vp, _) in enumerate(np.asarray(mat_vs_vp_rho, np.float32)):
        Vs, Vp = float(Vs), float(Vp)
        ratio = float(np.float32(Vs) / np.float32(Vp))                     # vs_vp_Ratio: a float division stored in a double
        vs = Vs * 0.001
        L = 4. / 3. * ratio * ratio
        Qs = 10.5 + vs * (-16. + vs * (153. + vs * (-103. + vs * (34.7 + vs * (-5.29 + vs * 0.31)))))
        Qp = 2. * Qs
        Qk = (1. - L) / (1. / Qp - L / Qs)
        for m, Q in enumerate((Qs, Qk)):
            i = search(Q, table)
            assert i != -2 and i < len(table), (Q, Vs)
            if i >= 0:                                                      # a0, a1, b, g0, g1 <- columns 1, 2, 5, 3, 4
                out[e, 5 * m:5 * m + 5] = table[i, [1, 2, 5, 3, 4]]
    return out


def case(name, end_time, ckpt_rate, **kw):
    run, out = G.run_reference(name, end_time, ckpt_rate, damping="bkt", **kw)
    ids, F = G.read_forces(run)
    elem_ticks, mat = G.read_mesh(run)
    ck = {}
    for f in ("checkpoint.out0", "checkpoint.out1"):
        step, blocks = G.read_checkpoint(os.path.join(run, "out", "checkpoints", f))
        ck[step] = blocks[0]
    coef = coefficients(mat, quality_table())
    np.savez_compressed(os.path.join(HERE, name + ".npz"), elem_ticks=elem_ticks, mat_vs_vp_rho=mat, loaded_lnid=ids, forces=F,
                        ckpt_steps=np.array(sorted(ck)), ckpt_tm2=np.stack([ck[s][0] for s in sorted(ck)]),
                        ckpt_tm1=np.stack([ck[s][1] for s in sorted(ck)]), dt=1e-3, end_time=float(end_time),
                        freq=float(kw.get("freq") or 5.0), coef=coef)
    shutil.rmtree(run)
    rows = np.unique(coef, axis=0)
    print(name, "ok", sorted(ck), "classes", len(rows), "dilatation on in", int((coef[:, 8] != 0).sum()), "of", len(coef), "elements")


CASES = {
    # the c1_short set-up (examples/simple: 16 x 16 x 8 elements, one material)
    "c1_bkt": lambda: case("c1_bkt", "1.0", 400),
    # c5_two_level's layers (a soft layer refined one level deeper, hanging nodes: the Vs rule sees the same Vs), shorter than
    # its sibling.  With c5_two_level's own Vp / Vs = 1.732 in both layers Qk = 10 Qs > 500 and the reference switches the
    # dilatation off everywhere, so the soft layer's Vp is 4800 here (Vp / Vs = 2.77: Qs = 145, Qk = 367 <= 500, both
    # on the last loaded row): one class with both moduli on, one (the half-space, Qs = 403, Qk = 4029) with shear only
    "c5_two_level_bkt": lambda: case("c5_two_level_bkt", "0.3", 100, cvm_args=[2, 4800, 1732, 2200, 6000, 3464, 2700], vscut=500, freq=5.0),
}

if __name__ == "__main__":
    if not os.path.exists(G.PSOLVE):
        sys.exit("build oracle/_ref/psolve first (oracle/build_ref.sh)")
    for c in (sys.argv[1:] or list(CASES)):
        CASES[c]()
