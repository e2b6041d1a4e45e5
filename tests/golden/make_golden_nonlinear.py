#!/usr/bin/env python3
"""Generate the nonlinear-soil fixtures tests/golden/c1_nl_vm.npz, c1_nl_dp.npz and c5_two_level_nl.npz from the REAL reference
run with include_nonlinear_analysis = yes, material_plasticity_type = rate_independant (make_golden.run_reference with the
nonlinear keys added to the parameter text; needs the reference tree and oracle/_ref/psolve, as make_golden.py does).  Nothing
here is imported by the tests; they read the .npz files this script wrote.

Each fixture holds what its Rayleigh sibling holds (mesh dump, force file, two checkpoints) without the station traces, and
  model, properties, vs_min, vs_cut   the material model (1 von Mises, 2 Drucker-Prager), the property columns' meaning
                                      (0 alphakay), the Vs window of isThisElementNonLinear
  props [rows, 6]                     material_properties_list: Vs, alpha, k, strain rate, sensitivity, hardening modulus
  elems [n], cons [n, 6]              derived HERE by the restatement (tests/nl_reference.constants): the nonlinear elements and
                                      h, mu, lambda, alpha, k, hardening modulus of each
  elastic_off [2]                     rel. L-inf of the checkpoints against the reference's own run of the same input with
                                      include_nonlinear_analysis = no
  yielded                             the fraction of quadrature points with ep > 0 at the later checkpoint (the restatement's)
Conditions, checked here and again by tests/test_nonlinear_cpu.py: elastic_off[1] >= 1e-2, 0.01 < yielded < 0.9.
Geostatic times are 0: no gravity, no bottom reactions.

Usage: python tests/golden/make_golden_nonlinear.py [c1_nl_vm] [c1_nl_dp] [c5_two_level_nl]
"""
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_golden as G  # noqa: E402

ELASTIC_KEYS = G.EXTRA_KEYS
MODEL_NAMES = {1: "vonMises", 2: "DruckerPrager"}


def nonlinear_keys(model, props, vs_min, vs_cut):
    rows = "\n".join(" ".join("%.17g" % v for v in r) for r in props)
    return ELASTIC_KEYS.replace("include_nonlinear_analysis = no", "include_nonlinear_analysis = yes") + """
nonlinear_shear_velocity_cut = %.17g
nonlinear_shear_velocity_min = %.17g
geostatic_loading_time_sec = 0
geostatic_cushion_time_sec = 0
material_model = %s
material_properties_type = alphakay
material_plasticity_type = rate_independant
material_properties_count = %d
material_properties_list =
%s
""" % (vs_cut, vs_min, MODEL_NAMES[model], len(props), rows)


def checkpoints(run):
    ck = {}
    for f in ("checkpoint.out0", "checkpoint.out1"):
        step, blocks = G.read_checkpoint(os.path.join(run, "out", "checkpoints", f))
        ck[step] = blocks[0]
    return ck


def problem(name, g):
    """The fixture's mesh with Rayleigh tables, as tests/test_nonlinear_cpu.golden_problem builds it."""
    from tests import test_nonlinear_cpu as C
    return C.problem_of(name, g)


def case(name, end_time, ckpt_rate, model, props, vs_min, vs_cut, **kw):
    from tests import helpers as H
    from tests import nl_reference as R
    props = np.asarray(props, np.float64).reshape(-1, 6)
    G.EXTRA_KEYS = nonlinear_keys(model, props, vs_min, vs_cut)
    try:
        run, out = G.run_reference(name, end_time, ckpt_rate, **kw)
    finally:
        G.EXTRA_KEYS = ELASTIC_KEYS
    ids, F = G.read_forces(run)
    elem_ticks, mat = G.read_mesh(run)
    ck = checkpoints(run)
    shutil.rmtree(run)
    run, out = G.run_reference(name + "_elastic", end_time, ckpt_rate, **kw)
    el = checkpoints(run)
    shutil.rmtree(run)
    steps = sorted(ck)
    assert sorted(el) == steps
    off = np.array([H.rel_linf(ck[s][1], el[s][1]) for s in steps])
    g = dict(elem_ticks=elem_ticks, mat_vs_vp_rho=mat, loaded_lnid=ids, forces=F[:steps[-1]], ckpt_steps=np.array(steps),
             ckpt_tm2=np.stack([ck[s][0] for s in steps]), ckpt_tm1=np.stack([ck[s][1] for s in steps]), dt=1e-3,
             end_time=float(end_time), freq=float(kw.get("freq") or 5.0), model=model, properties=0, vs_min=float(vs_min),
             vs_cut=float(vs_cut), props=props, elastic_off=off)
    p = problem(name, g)
    elems, cons = R.constants(p["edata"], model, props, vs_min, vs_cut)
    kept = R.run_a(p, elems, cons, steps[-1], ids, F, keep=steps)
    d = [H.rel_linf(kept[s][0], ck[s][1]) for s in steps]
    yielded = float((kept[steps[-1]][3] > 0).mean())
    print(name, "steps", steps, "off the elastic run %s" % off, "nonlinear elements %d of %d" % (len(elems), len(mat)),
          "yielded %.3f" % yielded, "restatement (A) against the checkpoints %s" % d)
    assert off[-1] >= 1e-2 and 0.01 < yielded < 0.9, (off, yielded)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), elems=elems, cons=cons, yielded=yielded, **g)
    print(name, "ok", os.path.getsize(os.path.join(HERE, name + ".npz")), "bytes")


WINDOW_ALL = (0.0, 10000.0)
CASES = {
    # examples/simple (2048 elements, one material, Rayleigh damping), every element nonlinear.  The source of that example is
    # enormous (fields of hundreds of metres, stresses near 1e12 Pa), hence the size of k.  k = 3e11 leaves the run >= 1e-2 off
    # the elastic one but yields in 0.5 - 0.7 % of the quadrature points by step 200; 2e11 (von Mises) and 1.5e11
    # (Drucker-Prager) bring that to 1.5 %, and 2e11 the soft layer of the two-level mesh to 1.3 %
    "c1_nl_vm": lambda: case("c1_nl_vm", "0.3", 100, 1, [[100, 0, 2e11, 0, 0, 0], [9000, 0, 2e11, 0, 0, 0]], *WINDOW_ALL),
    "c1_nl_dp": lambda: case("c1_nl_dp", "0.3", 100, 2, [[100, 0.1, 1.5e11, 0, 0, 1e10], [9000, 0.1, 1.5e11, 0, 0, 1e10]], *WINDOW_ALL),
    # c5_two_level_bkt's layers under Rayleigh damping; the window takes the soft layer (Vs 1732) alone: hanging nodes and a
    # linear / nonlinear interface
    "c5_two_level_nl": lambda: case("c5_two_level_nl", "0.3", 100, 1, [[100, 0, 2e11, 0, 0, 0], [9000, 0, 2e11, 0, 0, 0]], 0.0, 2000.0,
                                    cvm_args=[2, 4800, 1732, 2200, 6000, 3464, 2700], vscut=500, freq=5.0),
}

if __name__ == "__main__":
    if not os.path.exists(G.PSOLVE):
        sys.exit("build oracle/_ref/psolve first (oracle/build_ref.sh)")
    for c in (sys.argv[1:] or list(CASES)):
        CASES[c]()
