"""What does a deformation map cost per step?  K steps of a uniform box, two ways on ONE solver in one session: no tracker;
and a full-mask DEFORMATION tracker (strain, strain rate, stress, rotation, rotation rate) on the centres of the surface
elements at every step.  The tracker reads u(t) and u(t - dt) only and holds no stream back.

    python profiles/tools/deform_cost.py [--box 512 512 256] [--steps 200] [--warmup 20] [--runs 3] [--quantities 31]

The configurations take turns, run by run, so that drift of the box's clocks or of the host lands on both alike.  Every run
starts from the same state (hq_upload of a seeded field, step 0) with the same source; the time is hq_run_timed's over K steps
after a warm-up of W (its total, a host clock around enqueue and sync).  Prints one line per run, then per configuration the
median and what the tracker adds per due step, beside the bytes per point and due step the kernel's model predicts
(hq_outputs.h: full mask, 32 of ids + 192 of weights + 16 of moduli + 48 x sizeof(hq_real) of gathers + 320 of state read).
The tracker's state is fetched at the end of every run, so the map is real.  Under `rocprofv3 --kernel-trace --stats -- python
profiles/tools/deform_cost.py --runs 1` the kernel statistics give hq_k_deform's own time."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hercules_amd import capi, host  # noqa: E402

CONFIGS = ["none", "deform"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--box", type=int, nargs=3, default=[512, 512, 256])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--quantities", type=int, default=capi.HQ_DEFORM_ALL)
    ap.add_argument("--precision", default="f64", choices=["f64", "f32"])
    a = ap.parse_args()
    nx, ny, nz = a.box
    q = a.quantities
    h, dt, freq = 1000.0 / nx, 9.0e-5 * 512 / nx, 200.0 * nx / 512      # bench.py's c3 scaled with the edge
    t0 = time.perf_counter()
    box = host.Box(nx, ny, nz, h, dt, freq, solver_float=4 if a.precision == "f32" else 8)
    N = box.info["nharbored"]
    s = box.create_solver(precision=a.precision)
    ii, jj = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing="ij")
    xyz = np.stack([(ii.reshape(-1) + 0.5) * h, (jj.reshape(-1) + 0.5) * h, np.full(ii.size, 0.5 * h)], axis=1)
    ids, grad, mine = box.station_gradients(xyz)
    lame = box.station_moduli(xyz)
    assert mine.all()
    real_bytes = np.dtype(s.real).itemsize
    total = a.steps + a.warmup
    print("box %d x %d x %d: %d nodes, %d surface-element centres; mask %d; created in %.1f s" %
          (nx, ny, nz, N, len(ids), q, time.perf_counter() - t0), flush=True)
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
                s.deform_clear()
                s.upload(u, 0.999 * u, 0)
                s.set_source(loaded, F)
                hd = s.deform_add(ids, grad, lame, rate=1, quantities=q) if name == "deform" else None
                s.run(a.warmup)
                s.sync()
                wall_ms, _ = s.run_timed(a.steps)
                times[name].append(wall_ms)
                extra = ""
                if hd is not None:
                    vals, when, n = s.deform_fetch(hd)
                    extra = "; %d samples, largest value of the first block %.3e" % (n, float(vals[:, :6].max()))
                print("%-7s run %d: %9.3f us per step%s" % (name, run, 1e3 * wall_ms / a.steps, extra), flush=True)
    finally:
        s.close()
        box.close()
    med = {k: float(np.median(v)) for k, v in times.items()}
    nt, nv = bin(q & 7).count("1"), bin(q & 24).count("1")
    fields = 2 if q & 18 else 1
    model = 32 + 192 + (16 if q & 4 else 0) + 24 * real_bytes * fields + 8 * (10 * nt + 5 * nv)
    print("steps %d, warm-up %d, runs %d; medians:" % (a.steps, a.warmup, a.runs))
    for name in CONFIGS:
        line = "%-7s %9.4f ms per step (min %.4f, max %.4f)" % (name, med[name] / a.steps, min(times[name]) / a.steps,
                                                                max(times[name]) / a.steps)
        if name != "none":
            line += "; %+8.3f us per due step over none; model %d B per point = %.1f MB per due step" % (
                1e3 * (med[name] - med["none"]) / a.steps, model, model * len(ids) / 1e6)
        print(line)
    print("spread of the no-tracker runs: %.3f us per step" % (1e3 * (max(times["none"]) - min(times["none"])) / a.steps))


if __name__ == "__main__":
    main()
