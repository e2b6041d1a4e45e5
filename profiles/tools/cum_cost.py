"""What does a cumulative-intensity map cost per step?  K steps of a uniform box, three ways on ONE solver in one session: no
tracker; an acceleration PEAK tracker on every node of the z = 0 face (K = 1: single nodes) at every step -- the yardstick,
hq_k_peak; and an acceleration CUMULATIVE tracker on the same nodes at every step with a Husid slot every 64th sample.  Both
trackers read u(t - 2 dt) and hold the bricks' and the exchange chain's streams back behind their launch.

    python profiles/tools/cum_cost.py [--box 512 512 256] [--steps 200] [--warmup 20] [--runs 5] [--husid-every 64]

The configurations take turns, run by run, so that drift of the box's clocks or of the host lands on all of them alike.
Every run starts from the same state (hq_upload of a seeded field, step 0) with the same source; the time is a host clock
around hq_run + hq_sync of K steps after a warm-up of W.  Prints one line per run, then per configuration the median and
what it adds to the no-tracker median per step, beside the bytes per point and due step the models of the kernels predict
(hq_outputs.h): hq_k_cum<1>, acceleration only, 4 of id + 72 of gathers (36 in the f32 library) + 48 of sums read + 48
written, + 24 on a Husid step; hq_k_peak<1> 4 + 72 + 40 of peaks read.  The trackers' state is fetched at the end of every
run, so the maps are real.  Under `rocprofv3 --kernel-trace --stats -- python profiles/tools/cum_cost.py --runs 1` the kernel
statistics give hq_k_cum's own time."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hercules_amd import capi, host  # noqa: E402

A = capi.HQ_PEAK_ACC
CONFIGS = ["none", "peak acc", "cum acc"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--box", type=int, nargs=3, default=[512, 512, 256])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--husid-every", type=int, default=64)
    ap.add_argument("--brick-stream", type=int, default=-1)
    ap.add_argument("--precision", default="f64", choices=["f64", "f32"])
    a = ap.parse_args()
    nx, ny, nz = a.box
    h, dt, freq = 1000.0 / nx, 9.0e-5 * 512 / nx, 200.0 * nx / 512      # bench.py's c3 scaled with the edge
    t0 = time.perf_counter()
    box = host.Box(nx, ny, nz, h, dt, freq, solver_float=4 if a.precision == "f32" else 8)
    N = box.info["nharbored"]
    opts = {"brick_stream": a.brick_stream} if a.brick_stream >= 0 else None
    s = box.create_solver(options=opts, precision=a.precision)
    surface = np.nonzero(box.node_ijk[:, 2] == 0)[0].astype(np.int32)
    real_bytes = np.dtype(s.real).itemsize
    total = a.steps + a.warmup
    slots = total // a.husid_every + 1
    print("box %d x %d x %d: %d nodes, %d on the z = 0 face; brick_stream %d; created in %.1f s" %
          (nx, ny, nz, N, len(surface), s.info()["brick_stream"], time.perf_counter() - t0), flush=True)
    loaded, pattern = box.point_source(nx * h / 2, ny * h / 2, nz * h / 8, 30.0, 70.0, 10.0)
    rp = box.run_params(loaded=loaded, pattern=pattern, moment=1e13, rise_time=20 * dt, source_window=total)
    F = box.source_table(rp, 0, total)
    ijk = box.node_ijk.astype(np.int64)
    u = (((ijk[:, 0] * 73856093) ^ (ijk[:, 1] * 19349663) ^ (ijk[:, 2] * 83492791)) % 2048 / 1024.0 - 1.0)[:, None] * \
        np.array([1e-6, -7e-7, 4e-7])[None, :]
    times = {name: [] for name in CONFIGS}
    try:
        for run in range(a.runs):
            for name in CONFIGS:
                s.peak_clear()
                s.cum_clear()
                s.upload(u, 0.999 * u, 0)
                s.set_source(loaded, F)
                hp = s.peak_add(surface, None, rate=1, quantities=A) if name == "peak acc" else None
                hc = s.cum_add(surface, None, rate=1, quantities=A, threshold=0.0, husid_every=a.husid_every,
                               husid_slots=slots) if name == "cum acc" else None
                s.run(a.warmup)
                s.sync()
                t = time.perf_counter()
                s.run(a.steps)
                s.sync()
                wall = time.perf_counter() - t
                times[name].append(wall)
                extra = ""
                if hp is not None:
                    extra = "; %d samples" % s.peak_fetch(hp)[2]
                if hc is not None:
                    sums, span, curve, csteps, n = s.cum_fetch(hc)
                    extra = "; %d samples, %d Husid slots, largest sum of a^2 %.3e" % (n, len(csteps), float(sums[:, 0, 3:].max()))
                print("%-10s run %d: %9.3f us per step%s" % (name, run, 1e6 * wall / a.steps, extra), flush=True)
    finally:
        s.close()
        box.close()
    med = {k: float(np.median(v)) for k, v in times.items()}
    model = {"peak acc": 4 + 9 * real_bytes + 40, "cum acc": 4 + 9 * real_bytes + 96}
    print("steps %d, warm-up %d, runs %d; medians:" % (a.steps, a.warmup, a.runs))
    for name in CONFIGS:
        line = "%-10s %9.3f us per step (min %.3f, max %.3f)" % (name, 1e6 * med[name] / a.steps, 1e6 * min(times[name]) / a.steps,
                                                                  1e6 * max(times[name]) / a.steps)
        if name != "none":
            b = model[name]
            line += "; %+8.3f us per step over none; model %d B per point = %.1f MB per due step" % (
                1e6 * (med[name] - med["none"]) / a.steps, b, b * len(surface) / 1e6)
            if name == "cum acc":
                line += " (+ 24 B per point on every %dth)" % a.husid_every
        print(line)
    spread = 1e6 * (max(times["none"]) - min(times["none"])) / a.steps
    print("spread of the no-tracker runs: %.3f us per step" % spread)


if __name__ == "__main__":
    main()
