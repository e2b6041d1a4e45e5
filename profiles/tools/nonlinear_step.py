"""What does nonlinear soil cost on a patch context?  One uniform box (default 256 x 256 x 128, bench.py's c2 shape: the 8 M-element
box), Rayleigh tables, ms per step of

  elastic   the patch context as it is (bricks + shell patches): the step the correction pass runs beside
            (--parent-lib: a second `parent` row with the same step on another library, e.g. the parent commit's
            libhq_solver.so, passed to the child as HQ_SOLVER_LIB -- a context WITHOUT nonlinear soil against its parent)
  top       hq_nonlinear_set with the top eighth of the depth nonlinear (Drucker-Prager, linear hardening)
  all       ... with every element nonlinear

    python profiles/tools/nonlinear_step.py [--box 256 256 128] [--steps 100] [--warmup 20] [--runs 5] [--rounds 2]
                                            [--limit 300] [--parent-lib PATH]

Every configuration is a child process of its own under `timeout` (--limit seconds), one after the other; the first child
that fails ends the run.  A child times `runs` windows of `steps` steps with the host clock around hq_run + hq_sync (the step
uses up to three streams: events on one of them would not see the others) after `warmup` steps, and prints every window; the
parent runs the list `rounds` times, alternating the configurations, and reports per configuration the median over all windows
and their spread (min - max).
The pass's traffic model (csrc/hq_nonlin_dev.h), per nonlinear element of a uniform region (one touched node per element):
state 896 B read and written, corner forces 192 B written and 192 B read again, constants 48 B, node ids 32 B, the gathered
fields 24 B from HBM (192 B requested), the node table 32 + 4 B, dF 24 B written and read, the apply 12 + 8 + 24 + 24 B:
1536 B, set against the HBM peak -- 8.0 TB/s by the specification, 6.29 TB/s as a float4 copy reaches (MI355X_MICROARCH.md).
The yield constant is set far below the stresses of the run (k = 1 Pa, hardening mu / 10), so every point that the wave has
reached yields and takes the long branch: the cost of a fully yielding region."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12
PASS_BYTES_PER_ELEMENT = 896 + 192 + 192 + 48 + 32 + 24 + (32 + 4) + (24 + 24) + (12 + 8 + 24 + 24)
NEW_EXPORTS = ("hq_nonlinear_set", "hq_nonlinear_info", "hq_nonlinear_fetch", "hq_nonlinear_load", "hq_nonlinear_clear",
               "hq_nonlinear_plan_check", "hq_nonlinear_plan_tables", "hq_nonlinear_table_faults")


def child(a):
    from hercules_amd import capi, host
    if os.environ.get("HQ_SOLVER_LIB") and a.child == "parent":
        # an older library (the parent commit's) lacks the nonlinear entry points, which this child never calls
        capi.EXPORTS = [n for n in capi.EXPORTS if n not in NEW_EXPORTS]
    nx, ny, nz = a.box
    h, dt, freq = 1000.0 / nx, 1.8e-4 * 256 / nx, 100.0 * nx / 256      # bench.py's c2 scaled with the edge
    box = host.Box(nx, ny, nz, h, dt, freq)
    s = box.create_solver(variant=capi.HQ_VARIANT_PATCH)
    try:
        N, E = box.info["nharbored"], box.info["lenum"]
        total = (a.steps + a.warmup) * a.runs
        loaded, pattern = box.point_source(nx * h / 2, ny * h / 2, nz * h / 8, 30.0, 70.0, 10.0)
        rp = box.run_params(loaded=loaded, pattern=pattern, moment=1e13, rise_time=20 * dt, source_window=total)
        s.set_source(loaded, box.source_table(rp, 0, total))
        ninfo, yielded = dict(elements=0, touched_nodes=0, device_bytes=0), 0.0
        if a.child in ("top", "all"):
            edata = np.empty((E, 4), np.float32)
            edata[:, 0] = h
            edata[:, 1:] = box.material()
            mu = float(edata[0, 3]) * float(edata[0, 2]) ** 2
            props = [[100.0, 0.1, 1.0, 0.0, 0.0, mu / 10], [9000.0, 0.1, 1.0, 0.0, 0.0, mu / 10]]
            elems, cons = host.nonlinear_constants(edata, capi.HQ_NL_DRUCKERPRAGER, props, 0.0, 1e9)
            if a.child == "top":
                keep = np.asarray(box.node_ijk)[np.asarray(box.lnid)[:, 0], 2] < max(nz // 8, 1)
                elems, cons = elems[keep], cons[keep]
            s.set_nonlinear(capi.HQ_NL_DRUCKERPRAGER, elems, cons)
            ninfo = s.nonlinear_info()
        info = s.info()
        times = []
        for run in range(a.runs):
            s.run(a.warmup)
            s.sync()
            t0 = time.perf_counter()
            s.run(a.steps)
            s.sync()
            times.append(1e3 * (time.perf_counter() - t0) / a.steps)
        assert s.check_finite() == 0
        if ninfo["elements"]:
            yielded = float((s.nonlinear_fetch()[1] > 0).mean())
        print("RESULT " + json.dumps(dict(mode=a.child, nodes=N, elements=E, brick_nodes=info["brick_nodes"], nl_elements=ninfo["elements"],
                                          touched=ninfo["touched_nodes"], nl_gb=ninfo["device_bytes"] / 1e9, yielded=yielded,
                                          device_gb=info["device_bytes"] / 1e9, ms=times)), flush=True)
    finally:
        s.close()
        box.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--box", type=int, nargs=3, default=[256, 256, 128])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child", default=None, choices=["elastic", "parent", "top", "all"])
    a = ap.parse_args()
    if a.child:
        return child(a)
    modes = [("elastic", None)] + ([("parent", a.parent_lib)] if a.parent_lib else []) + [("top", None), ("all", None)]
    ms, last = {m: [] for m, _ in modes}, {}
    for rnd in range(a.rounds):
        for mode, lib in modes:
            env = dict(os.environ)
            if lib:
                env["HQ_SOLVER_LIB"] = os.path.abspath(lib)
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", mode, "--box"] + \
                  [str(v) for v in a.box] + ["--steps", str(a.steps), "--warmup", str(a.warmup), "--runs", str(a.runs)]
            out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, universal_newlines=True)
            sys.stdout.write(out.stdout)
            if out.returncode != 0:
                sys.exit("%s: exit status %d -- nothing more is started" % (mode, out.returncode))
            r = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
            ms[mode] += r["ms"]
            last[mode] = r
    print("box %d x %d x %d, %d nodes; %d windows of %d steps per configuration; ms per step: median (min - max)"
          % (a.box[0], a.box[1], a.box[2], last["elastic"]["nodes"], a.rounds * a.runs, a.steps))
    med = {}
    for mode, lib in modes:
        v = np.array(ms[mode])
        med[mode] = float(np.median(v))
        print("  %-8s %8.3f  (%.3f - %.3f)%s" % (mode, med[mode], v.min(), v.max(), "   library %s" % lib if lib else ""))
    if "parent" in med:
        print("  without nonlinear soil against the parent library: %+.3f ms (%+.2f %%)"
              % (med["elastic"] - med["parent"], 100 * (med["elastic"] - med["parent"]) / med["parent"]))
    for mode in ("top", "all"):
        r, add = last[mode], med[mode] - med["elastic"]
        moved = PASS_BYTES_PER_ELEMENT * r["nl_elements"]
        print("  %-4s %9d nonlinear elements (%.1f %%), %d touched nodes, %.3f GB added, yielded %.3f: +%.3f ms; model %d B per element ="
              " %.2f GB: %.3f ms at 6.29 TB/s, %.3f at 8.0 TB/s"
              % (mode, r["nl_elements"], 100.0 * r["nl_elements"] / r["elements"], r["touched"], r["nl_gb"], r["yielded"], add,
                 PASS_BYTES_PER_ELEMENT, moved / 1e9, 1e3 * moved / HBM_COPY, 1e3 * moved / HBM_SPEC))


if __name__ == "__main__":
    main()
