"""What does an attenuated step cost on a patch context?  One uniform box (default 256 x 256 x 128, bench.py's c2 shape: the
8 M-element box), one attenuation class, undamped tables, ms per step of

  elastic   the patch context as it is (bricks + shell patches): the step the correction chain runs beside
  split     the same context with hq_attenuation_set_split
  scatter   a scatter context with hq_attenuation_set  (--scatter-lib: the library to take this figure on, e.g. the parent
            commit's libhq_solver.so; passed to the child as HQ_SOLVER_LIB)
  inline    split on a library built with -DHQ_ATTEN_SPLIT_INLINE (--inline-lib): the correction chain ON the compute stream
            instead of beside the step -- what the overlap buys

    python profiles/tools/atten_split_step.py [--box 256 256 128] [--steps 100] [--warmup 20] [--runs 5] [--rounds 2]
                                              [--limit 300] [--scatter-lib PATH] [--inline-lib PATH]

Every configuration is a child process of its own under `timeout` (--limit seconds), one after the other; the first child
that fails ends the run.  A child times `runs` windows of `steps` steps with the host clock around hq_run + hq_sync (the step
uses up to three streams: events on one of them would not see the others) after `warmup` steps, and prints every window; the
parent runs the list `rounds` times, alternating the configurations, and reports per configuration the median over all windows
and their spread (min - max).
The correction chain's traffic model (csrc/hq_atten_split.h), per node of a uniform region: advance 288 B, corner force 32 +
16 + 192 + ~48 of gathered rows, node sum 32 + 4 + 192 + 24, apply 80: 908 B, set against the HBM peak -- 8.0 TB/s by the
specification, 6.29 TB/s as a float4 copy reaches (MI355X_MICROARCH.md)."""
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
CHAIN_BYTES_PER_NODE = 288 + (32 + 16 + 192 + 48) + (32 + 4 + 192 + 24) + 80
# a made-up class with both moduli on (tests/bkt_reference.CLASSES[0]): one class, as in a uniform region
ROW = np.array([0.0373, 0.0641, 0.0158, 0.0611, 0.9163, 0.0185, 0.0319, 0.0079, 0.0427, 0.7731], np.float32)
NEW_EXPORTS = ("hq_attenuation_set_split", "hq_attenuation_split_plan_check", "hq_attenuation_split_plan_tables",
               "hq_attenuation_split_table_faults")


def child(a):
    from hercules_amd import capi, host
    if os.environ.get("HQ_SOLVER_LIB") and a.child == "scatter":
        # an older library (the parent commit's) lacks the entry points of the split form, which this child never calls
        capi.EXPORTS = [n for n in capi.EXPORTS if n not in NEW_EXPORTS]
    nx, ny, nz = a.box
    h, dt, freq = 1000.0 / nx, 1.8e-4 * 256 / nx, 100.0 * nx / 256      # bench.py's c2 scaled with the edge
    box = host.Box(nx, ny, nz, h, dt, freq, damping="none")
    s = box.create_solver(variant=capi.HQ_VARIANT_SCATTER if a.child == "scatter" else capi.HQ_VARIANT_PATCH)
    try:
        N, E = box.info["nharbored"], box.info["lenum"]
        total = (a.steps + a.warmup) * a.runs
        loaded, pattern = box.point_source(nx * h / 2, ny * h / 2, nz * h / 8, 30.0, 70.0, 10.0)
        rp = box.run_params(loaded=loaded, pattern=pattern, moment=1e13, rise_time=20 * dt, source_window=total)
        s.set_source(loaded, box.source_table(rp, 0, total))
        if a.child != "elastic":
            s.set_attenuation(np.tile(ROW, (E, 1)), freq, **({} if a.child == "scatter" else {"split": True}))
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
        print("RESULT " + json.dumps(dict(mode=a.child, nodes=N, elements=E, brick_nodes=info["brick_nodes"], kernel=s.dominant_kernel(),
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
    ap.add_argument("--scatter-lib", default=None)
    ap.add_argument("--inline-lib", default=None)
    ap.add_argument("--child", default=None, choices=["elastic", "split", "scatter", "inline"])
    a = ap.parse_args()
    if a.child:
        return child(a)
    modes = [("elastic", None), ("split", None), ("scatter", a.scatter_lib)] + ([("inline", a.inline_lib)] if a.inline_lib else [])
    ms, nodes = {m: [] for m, _ in modes}, 0
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
            nodes = r["nodes"]
    print("box %d x %d x %d, %d nodes; %d windows of %d steps per configuration; ms per step: median (min - max)"
          % (a.box[0], a.box[1], a.box[2], nodes, a.rounds * a.runs, a.steps))
    med = {}
    for mode, lib in modes:
        v = np.array(ms[mode])
        med[mode] = float(np.median(v))
        print("  %-8s %8.3f  (%.3f - %.3f)%s" % (mode, med[mode], v.min(), v.max(), "   library %s" % lib if lib else ""))
    add = med["split"] - med["elastic"]
    moved = CHAIN_BYTES_PER_NODE * nodes
    print("  split / scatter: %.2f x faster; the correction adds %.3f ms to the elastic step" % (med["scatter"] / med["split"], add))
    print("  traffic model %d B per node = %.2f GB per step: %.3f ms at the 6.29 TB/s of a copy, %.3f at the 8.0 TB/s specification"
          % (CHAIN_BYTES_PER_NODE, moved / 1e9, 1e3 * moved / HBM_COPY, 1e3 * moved / HBM_SPEC))
    if add > 0:
        print("  if the added time were the chain alone: %.2f TB/s, %.0f %% of the specification, %.0f %% of the copy rate"
              % (moved / (add * 1e-3) / 1e12, 100 * moved / (add * 1e-3) / HBM_SPEC, 100 * moved / (add * 1e-3) / HBM_COPY))
    if "inline" in med:
        print("  chain on the compute stream: %.3f ms; beside the step: %.3f ms: the overlap buys %.3f ms per step"
              % (med["inline"], med["split"], med["inline"] - med["split"]))


if __name__ == "__main__":
    main()
