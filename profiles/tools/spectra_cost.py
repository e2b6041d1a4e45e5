"""What does a response-spectrum map cost per step?  K steps of a uniform box, four ways on ONE solver in one session: no
tracker; an acceleration-only peak map of every node of the z = 0 face (K = 1: single nodes) at every step -- the launch
that reads the same three fields and holds the same streams back; a spectrum map of the same nodes with 8 periods at every
step; and the same at every fourth step.

    python profiles/tools/spectra_cost.py [--box 512 512 256] [--steps 200] [--warmup 20] [--runs 5] [--periods 8]

The configurations take turns, run by run, so that drift of the box's clocks or of the host lands on all of them alike.
Every run starts from the same state (hq_upload of a seeded field, step 0) with the same source; the time is a host clock
around hq_run + hq_sync of K steps after a warm-up of W.  Prints one line per run, then per configuration the median and
what it adds to the no-tracker median per step and per DUE step, beside the bytes per point and due step the models of
hq_k_peak and hq_k_spec predict (hq_outputs.h).  For hq_k_spec<1>: 4 of id + 24 per field gathered (12 in the f32 library)
x 3 + 24 read and 24 written of aprev; per period 80 read (x, v, sd) and 48 written (x, v); the stores of raised sd come on
top.  The tracker's state is fetched at the end of every run, so the map is real.  Under `rocprofv3 --kernel-trace --stats
-- python profiles/tools/spectra_cost.py --runs 1` the kernel statistics give hq_k_spec's own time."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hercules_amd import capi, host  # noqa: E402

CONFIGS = [("none", None, 1), ("peak acc rate 1", "peak", 1), ("spectrum rate 1", "spec", 1), ("spectrum rate 4", "spec", 4)]


def model_bytes(kind, nper, real_bytes):
    """Bytes per point and due step of hq_k_peak<1> with HQ_PEAK_ACC alone (reads; raised peaks not counted) and of
    hq_k_spec<1> (reads and the stores of x, v and aprev; raised sd not counted)."""
    gathers = 4 + 3 * 3 * real_bytes
    if kind == "peak":
        return gathers + 40
    return gathers + 24 + 24 + nper * (80 + 48)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--box", type=int, nargs=3, default=[512, 512, 256])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--periods", type=int, default=8)
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
    periods = np.geomspace(20 * dt, 2000 * dt, a.periods)
    print("box %d x %d x %d: %d nodes, %d on the z = 0 face; brick_stream %d; %d periods %.3g .. %.3g s; created in %.1f s" %
          (nx, ny, nz, N, len(surface), s.info()["brick_stream"], a.periods, periods[0], periods[-1],
           time.perf_counter() - t0), flush=True)
    loaded, pattern = box.point_source(nx * h / 2, ny * h / 2, nz * h / 8, 30.0, 70.0, 10.0)
    rp = box.run_params(loaded=loaded, pattern=pattern, moment=1e13, rise_time=20 * dt, source_window=a.steps + a.warmup)
    F = box.source_table(rp, 0, a.steps + a.warmup)
    ijk = box.node_ijk.astype(np.int64)
    u = (((ijk[:, 0] * 73856093) ^ (ijk[:, 1] * 19349663) ^ (ijk[:, 2] * 83492791)) % 2048 / 1024.0 - 1.0)[:, None] * \
        np.array([1e-6, -7e-7, 4e-7])[None, :]
    times = {name: [] for name, _, _ in CONFIGS}
    try:
        for run in range(a.runs):
            for name, kind, rate in CONFIGS:
                s.peak_clear()
                s.spec_clear()
                s.upload(u, 0.999 * u, 0)
                s.set_source(loaded, F)
                hp = s.peak_add(surface, None, rate=rate, quantities=capi.HQ_PEAK_ACC) if kind == "peak" else None
                hs = s.spec_add(surface, None, rate=rate, periods=periods, damping=0.05) if kind == "spec" else None
                s.run(a.warmup)
                s.sync()
                t = time.perf_counter()
                s.run(a.steps)
                s.sync()
                wall = time.perf_counter() - t
                times[name].append(wall)
                extra = ""
                if hp is not None:
                    peaks, when, n = s.peak_fetch(hp)
                    extra = "; %d samples, largest PGA %.3e" % (n, float(np.sqrt(peaks[:, 0, 4].max())))
                if hs is not None:
                    sd, _, _, n = s.spec_fetch(hs, osc=False, aprev=False)
                    extra = "; %d samples, largest SD per period %s" % (n, " ".join("%.2e" % v for v in np.sqrt(sd[:, :, 3].max(axis=0))))
                print("%-18s run %d: %9.3f us per step%s" % (name, run, 1e6 * wall / a.steps, extra), flush=True)
    finally:
        s.close()
        box.close()
    med = {k: float(np.median(v)) for k, v in times.items()}
    print("steps %d, warm-up %d, runs %d; medians:" % (a.steps, a.warmup, a.runs))
    for name, kind, rate in CONFIGS:
        line = "%-18s %9.3f us per step (min %.3f, max %.3f)" % (name, 1e6 * med[name] / a.steps, 1e6 * min(times[name]) / a.steps,
                                                                1e6 * max(times[name]) / a.steps)
        if kind:
            due = len(range(a.warmup + (-a.warmup) % rate, a.warmup + a.steps, rate))
            add = med[name] - med["none"]
            b = model_bytes(kind, a.periods, real_bytes)
            line += "; %+8.3f us per step, %+8.3f us per due step over none; model %d B per point = %.1f MB per due step" % (
                1e6 * add / a.steps, 1e6 * add / due, b, b * len(surface) / 1e6)
            if add > 0:
                line += " = %.0f GB/s" % (b * len(surface) * due / add / 1e9)
        print(line)
    spread = 1e6 * (max(times["none"]) - min(times["none"])) / a.steps
    print("spread of the no-tracker runs: %.3f us per step" % spread)


if __name__ == "__main__":
    main()
