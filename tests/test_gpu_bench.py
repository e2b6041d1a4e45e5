"""bench.py itself on the GPU: a --full line carries its own parity (config.parity_*: oracle cone windows stepped on
the timed context behind the timed region), on one rank and on ranks that share this box's one GPU -- the N > 1 path
the driver's scaling run takes (launcher, rendezvous, transport selection with both device-side transports brought up
and timed, partitioned stepping), minus a second GPU."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*argv, env_extra=None, timeout=900):
    """One bench.py run -> its JSON line.  No retry: round 5 started a failed run of ranks sharing the GPU a second time
    (one unexplained failure in ~20 runs, output not kept).  Round 6 kept the output, and the one failure that came was a
    PARITY failure (0.37): hq_upload's null-stream hipMemset landing behind the first step's kernels when eight processes
    time-slice one GPU -- fixed (docs/LABNOTES.md, round 6; profiles/r06/ipc_8_ranks_with_parity_loop_40x.txt: 40 of 40
    afterwards).  A failure here is a finding: its stdout and stderr go to gpurun_out/bench_failures/ first."""
    import time
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.update(env_extra or {})
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(argv), cwd=ROOT, env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=timeout)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    if not (out.returncode == 0 and len(lines) == 1):
        keep = os.path.join(ROOT, "gpurun_out", "bench_failures")
        os.makedirs(keep, exist_ok=True)
        name = os.path.join(keep, "%d_%s" % (int(time.time()), "_".join(a.strip("-") for a in argv)[:80]))
        open(name + ".stdout", "w").write(out.stdout)
        open(name + ".stderr", "w").write(out.stderr)
    assert out.returncode == 0 and len(lines) == 1, (out.returncode, out.stdout[-1500:], out.stderr[-3000:])
    return json.loads(lines[0])


def test_one_rank_line_carries_its_parity():
    d = _bench("--workload", "m1", "--steps", "20", "--warmup", "5", "--full", "--no-pmc", "--no-cpu-baseline")
    c = d["config"]
    assert d["n_gpus"] == 1 and c["finite"] and c["brick_nodes"] > 0
    assert c["parity_windows"] >= 4 and c["parity_nodes"] > 4 * 11 ** 3 and c["parity_worst"] <= c["parity_tol"] == 1e-9


def test_a_plain_line_is_the_headline_alone():
    """`bench.py` without --full: set-up, warm-up, the timed steps and the line -- no counter passes, no CPU baseline, no
    parity windows -- with the headline keys of a --full line."""
    d = _bench("--workload", "m1", "--steps", "20", "--warmup", "5")
    c = d["config"]
    assert d["n_gpus"] == 1 and d["steps"] == 20 and d["warmup"] == 5 and c["finite"] and c["brick_nodes"] > 0
    assert d["unit"] == "element-updates/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - c["elements"]) <= 1e-9 * c["elements"]
    assert "cpu_baseline" not in d and c["parity_windows"] is None and d["roofline"]["traffic"] is None
    assert d["roofline"]["traffic_source"].startswith("unmeasured: plain run")


@pytest.mark.parametrize("world,transport", [(2, "auto"), (4, "ipc"), (2, "host")])
def test_ranks_sharing_the_gpu_carry_their_parity(world, transport):
    """HQ_BENCH_SHARE_GPU=1: the ranks of `bench.py --gpus N` on one device (RCCL refuses that, so `auto` times the IPC
    transport alone and keeps it).  Every rank's windows sit on ITS partition interfaces: pack, transport, interface
    update and unpack of the run that was timed are inside the checked cones.  At most four ranks: with bench.py's
    launcher and this process, at most six processes hold the GPU."""
    d = _bench("--gpus", str(world), "--workload", "c2" if world == 4 else "m1", "--steps", "10", "--warmup", "3", "--full",
               env_extra={"HQ_BENCH_SHARE_GPU": "1", "HQ_BENCH_TRANSPORT": transport})
    c = d["config"]
    assert d["n_gpus"] == world and c["finite"]
    assert ("IPC" in c["transport"] or "ipc" in c["transport"].lower()) if transport != "host" else "host" in c["transport"].lower()
    assert c["parity_windows"] >= 4 * world and c["parity_worst"] <= 1e-9


@pytest.mark.parametrize("wl,windows", [("m1h", 4), ("o4s", 4), ("o3s", 3)])
def test_lines_of_lateral_material_and_octree_workloads_carry_parity(wl, windows):
    """m1h: material of its own in every element (hq_k_brick_het<PACKED>; the windows are boxes with the big box's
    classes).  o4s / o3s: octree workloads on one rank (windows centred on hanging nodes, true table rows)."""
    d = _bench("--workload", wl, "--steps", "10", "--warmup", "3", "--full", "--no-pmc", "--no-cpu-baseline")
    c = d["config"]
    assert c["finite"] and c["parity_windows"] >= windows and c["parity_worst"] <= 1e-9


def test_partitions_of_an_octree_workload_carry_parity_too():
    """Round-5 review 2a: an N > 1 line of an OCTREE workload used to print `parity_windows: null`.  Now rank 0 builds the
    whole mesh behind the timed region, cuts oracle windows around hanging nodes the partitions SHARE and broadcasts
    (node key, value) records; every rank checks the nodes it harbors on the context -- partition and transport -- that was
    timed.  o4gs: the small basin with a velocity gradient (per-element kernels, ragged units, hanging nodes of all kinds)
    on two ranks sharing this box's GPU over the IPC transport."""
    d = _bench("--gpus", "2", "--workload", "o4gs", "--steps", "10", "--warmup", "3", "--repeats", "2", "--full",
               env_extra={"HQ_BENCH_SHARE_GPU": "1", "HQ_BENCH_TRANSPORT": "ipc"})
    c = d["config"]
    assert d["n_gpus"] == 2 and c["finite"] and "IPC" in c["transport"]
    assert c["parity_windows"] >= 3 and c["parity_nodes"] > 500 and c["parity_worst"] <= 1e-9
    assert len(c["ms_per_step_runs"]) == 2


def test_the_drivers_launcher_form_on_ranks_sharing_the_gpu():
    """`python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port P bench.py
    --gpus 2 --steps K --warmup W`: the form the driver's scaling run uses (RANK / LOCAL_RANK / WORLD_SIZE from the
    launcher), here with both ranks on this box's one GPU."""
    import socket
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", HQ_BENCH_SHARE_GPU="1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
                          "--gpus", "2", "--steps", "10", "--warmup", "3", "--workload", "m1", "--full"], cwd=ROOT, env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=900)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1, (out.returncode, out.stdout[-1500:], out.stderr[-3000:])
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["finite"] and d["config"]["parity_worst"] <= 1e-9
    assert d["scaling"] == "strong" and d["steps"] == 10 and d["warmup"] == 3
