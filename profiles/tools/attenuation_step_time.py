"""What does BKT attenuation cost per step?  One process, one uniform box (default 256 x 256 x 128 = the 8 M-element box the
scatter variant is timed on in docs/LABNOTES.md), the scatter variant, two contexts one after the other:

  (a) the Rayleigh scatter step of the box's own eTable: hq_k_source, hq_k_element_scatter, hq_k_update
  (b) the attenuated step on undamped tables: hq_k_source, hq_k_atten_advance, hq_k_element_bkt, hq_k_update

    python profiles/tools/attenuation_step_time.py [--box 256 256 128] [--steps 50] [--warmup 5] [--runs 3] [--limit 120]

Times are hq_run_timed's: the whole step (events around K steps on the compute stream) and the dominant kernel alone (events
around every launch of hq_k_element_scatter in (a), of hq_k_element_bkt in (b)).  The split of (b): hq_k_element_bkt is
measured; hq_k_atten_advance is what (b)'s step has beyond its element kernel LESS what (a)'s step has beyond its own (the
source and update kernels and the launch gaps, which the two steps share) -- a difference, named as such in the output.  Under
`rocprofv3 --kernel-trace --stats -- python profiles/tools/attenuation_step_time.py --runs 1` the kernel statistics give each
kernel's own time directly.
The advance kernel's compulsory traffic, 288 B per slot (48 of fields, 96 of memory variables read and 96 written, 48 of damping
vectors written), is set against the HBM peak: 8.0 TB/s by the specification, 6.29 TB/s as a float4 copy reaches
(MI355X_MICROARCH.md).  --limit: seconds after which a timed batch counts as hung and the process ends (SIGALRM)."""
import argparse
import os
import signal
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from hercules_amd import capi, host  # noqa: E402

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12
# a made-up class with both moduli on (tests/bkt_reference.CLASSES[0]): one class, as in a uniform region
ROW = np.array([0.0373, 0.0641, 0.0158, 0.0611, 0.9163, 0.0185, 0.0319, 0.0079, 0.0427, 0.7731], np.float32)


def timed(s, a, label):
    out = []
    for run in range(a.runs):
        s.run(a.warmup)
        s.sync()
        signal.alarm(a.limit)
        total_ms, kernel_ms = s.run_timed(a.steps)
        signal.alarm(0)
        out.append((1e3 * total_ms / a.steps, 1e3 * kernel_ms))
        print("%-10s run %d: step %9.2f us, %s %9.2f us" % (label, run, out[-1][0], s.dominant_kernel(), out[-1][1]), flush=True)
    return np.median(np.array(out), axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--box", type=int, nargs=3, default=[256, 256, 128])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120)
    a = ap.parse_args()
    nx, ny, nz = a.box
    h, dt, freq = 1000.0 / nx, 9.0e-5 * 512 / nx, 200.0 * nx / 512      # bench.py's c3 scaled with the edge
    res = {}
    for label, damping in (("rayleigh", "rayleigh"), ("attenuated", "none")):
        t0 = time.perf_counter()
        box = host.Box(nx, ny, nz, h, dt, freq, damping=damping)
        s = box.create_solver(variant=capi.HQ_VARIANT_SCATTER)
        try:
            N, E = box.info["nharbored"], box.info["lenum"]
            total = (a.steps + a.warmup) * a.runs
            loaded, pattern = box.point_source(nx * h / 2, ny * h / 2, nz * h / 8, 30.0, 70.0, 10.0)
            rp = box.run_params(loaded=loaded, pattern=pattern, moment=1e13, rise_time=20 * dt, source_window=total)
            s.set_source(loaded, box.source_table(rp, 0, total))
            before = s.info()["device_bytes"]
            if label == "attenuated":
                s.set_attenuation(np.tile(ROW, (E, 1)), freq)
                ai = s.attenuation_info()
                res["slots"], res["bytes"] = ai["slots"], s.info()["device_bytes"] - before
                assert res["bytes"] == ai["device_bytes"] and ai["slots"] == N and ai["classes"] == 1, ai
            print("%-10s box %d x %d x %d: %d elements, %d nodes, %.2f GB on the device; created in %.1f s"
                  % (label, nx, ny, nz, E, N, s.info()["device_bytes"] / 1e9, time.perf_counter() - t0), flush=True)
            res[label] = timed(s, a, label)
            assert s.check_finite() == 0
        finally:
            s.close()
            box.close()
    (ra, rk), (at, ak) = res["rayleigh"], res["attenuated"]
    adv = (at - ak) - (ra - rk)
    ns = res["slots"]
    print("steps %d, warm-up %d, runs %d; medians, us per step:" % (a.steps, a.warmup, a.runs))
    print("(a) rayleigh   step %9.2f   hq_k_element_scatter %9.2f   the rest (source, update, gaps) %8.2f" % (ra, rk, ra - rk))
    print("(b) attenuated step %9.2f   hq_k_element_bkt     %9.2f   hq_k_atten_advance %8.2f (by difference)   the rest as (a)" % (at, ak, adv))
    print("    attenuation adds %+.2f us per step (%.2f x); state %d slots, %.1f B per node (%.1f B per element; 768 per element in the reference)"
          % (at - ra, at / ra, ns, res["bytes"] / ns, res["bytes"] / (nx * ny * nz)))
    moved = 288.0 * ns
    if adv > 0:
        rate = moved / (adv * 1e-6)
        print("    hq_k_atten_advance: 288 B x %d slots = %.1f MB per step -> %.2f TB/s if nothing else moves: %.0f %% of the 8.0 TB/s "
              "specification, %.0f %% of the 6.29 TB/s a copy reaches; at the copy rate it would take %.1f us"
              % (ns, moved / 1e6, rate / 1e12, 100 * rate / HBM_SPEC, 100 * rate / HBM_COPY, 1e6 * moved / HBM_COPY))


if __name__ == "__main__":
    main()
