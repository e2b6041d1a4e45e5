"""What does a 4D output step cost?  K steps of a uniform box with a wavefield output every R steps, three ways on ONE
solver in one session: no output at all, the synchronous runner (hqh_solver_run_on: hq_download at every output step)
and the asynchronous one (hqh_solver_run_async: field snapshots carried to pinned host memory beside the steps).

    python profiles/tools/snapshot_overlap.py [--box 512 512 256] [--steps 400] [--rate 100] [--runs 3] [--slots 2]
                                              [--quantity disp|vel|both] [--routes none,sync,async] [--dir DIR]

The files go to DIR (default: a temporary directory on /dev/shm, so that no disk is measured) and are removed again.
Every run starts from the same state (hq_upload of zeros, step 0) and the same source; the wall time is that of the
runner call, which ends with hq_sync.  Prints one line per run and a summary: the per-output stall of the synchronous
route = (sync - none) / outputs, what an output adds on the asynchronous one = (async - none) / outputs.
Under `rocprofv3 --kernel-trace --stats -- python profiles/tools/snapshot_overlap.py --routes async --runs 1` the kernel
statistics give hq_k_snapshot's own time."""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hercules_amd import host  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--box", type=int, nargs=3, default=[512, 512, 256])
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--rate", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--slots", type=int, default=2)
    ap.add_argument("--quantity", default="disp", choices=["disp", "vel", "both"])
    ap.add_argument("--routes", default="none,sync,async")
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    nx, ny, nz = a.box
    h, dt, freq = 1000.0 / nx, 9.0e-5 * 512 / nx, 200.0 * nx / 512      # bench.py's c3 scaled with the edge
    t0 = time.perf_counter()
    box = host.Box(nx, ny, nz, h, dt, freq)
    N, E = box.info["nharbored"], box.info["lenum"]
    s = box.create_solver()
    print("box %d x %d x %d: %d nodes, one field %.3f GB; created in %.1f s" % (nx, ny, nz, N, N * 24 / 1e9, time.perf_counter() - t0), flush=True)
    loaded, pattern = box.point_source(nx * h / 2, ny * h / 2, nz * h / 2, 30.0, 70.0, 10.0)
    zeros = np.zeros((N, 3))
    base = a.dir or tempfile.mkdtemp(prefix="hq_snap_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    os.makedirs(base, exist_ok=True)
    outputs = (a.steps - 1) // a.rate + 1
    times = {}
    try:
        for route in a.routes.split(","):
            for run in range(a.runs):
                kw = {}
                if route != "none":
                    for q, name in (("disp", "displacement"), ("vel", "velocity")):
                        if a.quantity in (q, "both"):
                            p = os.path.join(base, q + ".h4d")
                            host.wavefield_create(p, name, N, E, (nx * h, ny * h, nz * h), nx * h / 2 ** 30, dt, a.rate, a.steps)
                            kw["wavefield_%s_file" % q] = p
                    kw.update(wavefield_rate=a.rate, wavefield_total_nodes=N)
                rp = box.run_params(loaded=loaded, pattern=pattern, moment=1e13, rise_time=20 * dt, source_window=a.steps, **kw)
                s.upload(zeros, zeros, 0)
                s.sync()
                d2h0 = s.info()["pcie_d2h_bytes"]
                t = time.perf_counter()
                if route == "async":
                    box.solver_run_async(s, rp, 0, a.steps, slots=a.slots)
                else:
                    box.solver_run(s, rp, 0, a.steps)
                wall = time.perf_counter() - t
                times.setdefault(route, []).append(wall)
                print("%-5s run %d: %8.3f s for %d steps, %d outputs, %.2f GB device -> host" %
                      (route, run, wall, a.steps, outputs if route != "none" else 0, (s.info()["pcie_d2h_bytes"] - d2h0) / 1e9), flush=True)
                for f in os.listdir(base):
                    os.remove(os.path.join(base, f))
    finally:
        s.close()
        box.close()
        if not a.dir:
            shutil.rmtree(base, ignore_errors=True)
    best = {r: min(v) for r, v in times.items()}
    for r, v in times.items():
        print("%-5s best %.3f s, median %.3f s  (%.3f ms per step at best)" % (r, best[r], float(np.median(v)), 1e3 * best[r] / a.steps))
    if "none" in best:
        for r in ("sync", "async"):
            if r in best:
                print("%-5s: %+.3f s over no output = %.3f s per output step = %.0f steps' worth; wall %.1f %% over no output" %
                      (r, best[r] - best["none"], (best[r] - best["none"]) / outputs,
                       (best[r] - best["none"]) / outputs / (best["none"] / a.steps), 100.0 * (best[r] / best["none"] - 1.0)))


if __name__ == "__main__":
    main()
