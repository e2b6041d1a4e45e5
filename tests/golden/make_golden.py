#!/usr/bin/env python3
"""Generate the golden fixtures under tests/golden/ from the REAL reference.

Runs only in the build container (needs /root/reference and the binary that
oracle/build_ref.sh builds from it, oracle/_ref/psolve).  Nothing here is
imported by the tests; the tests read the .npz files this script wrote.

For every case the reference's examples/simple input (physics.in +
numerical.in merged into the single parameters file today's psolve wants,
psolve.c:7351, plus the 16 keys it requires, psolve.c:748-778) is run in a
scratch directory and the following is captured:

* mesh    : per-element node tick coordinates and (Vs,Vp,rho), from the
            reference's own flat dump (meshformatlab.c:52-250)
* forces  : out/srctmp/force_process.<rank> (quakesource.c:2453-2466)
* ckpt    : checkpoint.out{0,1} (io_checkpoint.c:29-130): header
            {groupsize, step, nharboredmax}; per rank tm2 then tm1
* stations: out/stations/station.<i> text (psolve.c:6679-6795)
* expected: the station traces the reference ships in
            examples/simple/expected-out/stations (independent pin)

Usage: python tests/golden/make_golden.py [case ...]
"""
import bz2
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

REF = os.environ.get("HERC_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PSOLVE = os.path.join(ROOT, "oracle", "_ref", "psolve")
MPI = os.environ.get("HERC_MPI_DIR", "/opt/conda")

EXTRA_KEYS = """
softening_factor = 0
use_progressive_meshing = 0
4D_output_file = out/disp.q4d
cvmdb_input_file = simple_case.e
mesh_etree_output_file = out/mesh.e
planes_input_file = in/planes.in
include_nonlinear_analysis = no
stiffness_calculation_method = {stiffness}
print_matrix_k = {printk}
print_station_velocities = no
print_station_accelerations = no
include_buildings = no
mesh_coordinates_for_matlab = yes
mesh_coordinates_directory_for_matlab = out/matlab
mesh_corners_matlab =
0 0 1000 1000 0 500
implement_drm = no
simulation_velocity_profile_freq_hz = 0
use_infinite_qk = no
"""


def run_reference(tag, end_time, ckpt_rate, stiffness="effective", damping="rayleigh",
                  nranks=1, printk="no", freq=None, dt=None, cvm_args=None, vscut=None, planes=None,
                  plane_rate=50, station_derivs=0, wavefield_rate=0, single=False):
    """Run the reference in a scratch dir; return (dir, stdout).  single: the program built with
    -DSINGLE_PRECISION_SOLVER (oracle/_ref/psolve_f32; psolve.h:60-64)."""
    run = tempfile.mkdtemp(prefix="herc_%s_" % tag, dir="/tmp")
    src = os.path.join(REF, "examples", "simple")
    shutil.copytree(os.path.join(src, "in"), os.path.join(run, "in"))
    shutil.copy(os.path.join(src, "simple_case.e"), run)
    for root, dirs, files in os.walk(run):
        for n in dirs + files:
            os.chmod(os.path.join(root, n), 0o755)
    if cvm_args is not None:
        # layered material database written with the reference's own etree/cvm libraries
        os.remove(os.path.join(run, "simple_case.e"))
        subprocess.check_call([os.path.join(ROOT, "oracle", "_ref", "make_cvm"),
                               os.path.join(run, "simple_case.e")] + [str(a) for a in cvm_args])
    for d in ("checkpoints", "planes", "srctmp", "stations", "matlab"):
        os.makedirs(os.path.join(run, "out", d))
    text = open(os.path.join(run, "in", "physics.in")).read() + \
        open(os.path.join(run, "in", "numerical.in")).read() + \
        EXTRA_KEYS.format(stiffness=stiffness, printk=printk)

    def setkey(t, key, val):
        return re.sub(r"(?m)^%s\s*=.*$" % re.escape(key), "%s = %s" % (key, val), t)

    text = setkey(text, "simulation_end_time_sec", end_time)
    text = setkey(text, "checkpointing_rate", ckpt_rate)
    text = setkey(text, "type_of_damping", damping)
    if wavefield_rate:
        # the parallel 4D output (output.c:886-1404): both quantities, every wavefield_rate steps
        text = setkey(text, "output_parallel", 1)
        text = setkey(text, "output_displacement", 1)
        text = setkey(text, "output_velocity", 1)
        text = setkey(text, "simulation_output_rate", wavefield_rate)
        text = setkey(text, "output_displacement_file", "out/disp.h4d")
        text = setkey(text, "output_velocity_file", "out/vel.h4d")
    if station_derivs >= 1:
        text = setkey(text, "print_station_velocities", "yes")
    if station_derivs >= 2:
        text = setkey(text, "print_station_accelerations", "yes")
    if vscut is not None:
        text = setkey(text, "simulation_shear_velocity_min", vscut)
    if freq is not None:
        text = setkey(text, "simulation_wave_max_freq_hz", freq)
    if dt is not None:
        text = setkey(text, "simulation_delta_time_sec", dt)
    if planes:
        # io_planes.c: "output_planes =" is followed by one line per plane
        # (lat long depth  dStrike nStrike  dDip nDip  strike dip), read from planes_input_file
        text = setkey(text, "number_output_planes", len(planes))
        text = setkey(text, "output_planes_print_rate", plane_rate)
        open(os.path.join(run, "in", "planes.in"), "w").write(
            "output_planes =\n" + "\n".join(" ".join(str(v) for v in p) for p in planes) + "\n")
    open(os.path.join(run, "parameters.in"), "w").write(text)
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(MPI, "lib"))
    out = subprocess.run([os.path.join(MPI, "bin", "mpiexec"), "-np", str(nranks), PSOLVE + ("_f32" if single else ""),
                          "parameters.in"], cwd=run, env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, universal_newlines=True)
    if out.returncode != 0:
        sys.stderr.write(out.stdout[-3000:])
        raise RuntimeError("reference run %s failed" % tag)
    return run, out.stdout


def read_mesh(run, rank=0):
    c = np.fromfile(os.path.join(run, "out", "matlab", "mesh_coordinates.%d" % rank), "<i4")
    m = np.fromfile(os.path.join(run, "out", "matlab", "mesh_data.%d" % rank), "<f4")
    return c.reshape(-1, 8, 3), m.reshape(-1, 3)


def read_forces(run, rank=0):
    p = os.path.join(run, "out", "srctmp", "force_process.%d" % rank)
    if not os.path.exists(p):
        return np.zeros(0, np.int32), np.zeros((0, 0, 3))
    b = open(p, "rb").read()
    n = int(np.frombuffer(b[:4], "<i4")[0])
    ids = np.frombuffer(b[4:4 + 4 * n], "<i4").copy()
    F = np.frombuffer(b[4 + 4 * n:], "<f8").reshape(-1, n, 3).copy()
    return ids, F


def read_checkpoint(path, harbored=None, real="<f8"):
    """-> (step, [ (tm2, tm1) per rank ]).  io_checkpoint.c:76-112.  real: "<f4" for a file psolve_f32 wrote
    (rows of three solver_float)."""
    b = open(path, "rb").read()
    groupsize, step, nmax = [int(v) for v in np.frombuffer(b[:12], "<i4")]
    row = 3 * np.dtype(real).itemsize
    out = []
    for r in range(groupsize):
        n = nmax if harbored is None else harbored[r]
        off = 12 + 2 * r * nmax * row
        tm2 = np.frombuffer(b[off:off + n * row], real).reshape(n, 3).copy()
        off += n * row
        tm1 = np.frombuffer(b[off:off + n * row], real).reshape(n, 3).copy()
        out.append((tm2, tm1))
    return step, out


def read_station_text(text, ncol=4):
    rows = [l.split() for l in text.splitlines() if l.strip() and not l.lstrip().startswith("#")]
    return np.array([[float(v) for v in r[:ncol]] for r in rows])


def read_stations(run, n=5, ncol=4):
    return np.stack([read_station_text(open(os.path.join(run, "out", "stations", "station.%d" % i)).read(), ncol)
                     for i in range(n)])


def parse_K(stdout):
    """print_matrix_k = yes dump (psolve.c:3183-3225): every float on the
    lines between the K1/K2 banners."""
    nums = {}
    cur = None
    for line in stdout.splitlines():
        s = line.strip()
        m = re.match(r"^\s*(K1|K2|K3)\b", s)
        if "Stiffness Matrix K1" in s or s.startswith("K1"):
            cur = "K1"; nums[cur] = []; continue
        if "Stiffness Matrix K2" in s or s.startswith("K2"):
            cur = "K2"; nums[cur] = []; continue
        if cur:
            vals = re.findall(r"[-+]?\d+\.\d+(?:[eE][-+]?\d+)?", s)
            if vals:
                nums[cur] += [float(v) for v in vals]
    return nums


def case_short(name, **kw):
    run, out = run_reference(name, "1.0", 400, **kw)
    ids, F = read_forces(run)
    elem_ticks, mat = read_mesh(run)
    ck = {}
    for f in ("checkpoint.out0", "checkpoint.out1"):
        step, blocks = read_checkpoint(os.path.join(run, "out", "checkpoints", f))
        ck[step] = blocks[0]
    st = read_stations(run)
    np.savez_compressed(os.path.join(HERE, name + ".npz"),
                        elem_ticks=elem_ticks, mat_vs_vp_rho=mat, loaded_lnid=ids, forces=F,
                        ckpt_steps=np.array(sorted(ck)),
                        ckpt_tm2=np.stack([ck[s][0] for s in sorted(ck)]),
                        ckpt_tm1=np.stack([ck[s][1] for s in sorted(ck)]),
                        stations=st, dt=1e-3, end_time=1.0, freq=5.0)
    shutil.rmtree(run)
    print(name, "ok", sorted(ck))


def case_stations_va():
    """Station files with the velocity and acceleration columns (print_station_velocities /
    print_station_accelerations = yes, psolve.c:6737-6787; the accelerations make the solver keep
    tm3, :4093-4101): 600 steps, all five stations, 10 columns; the first lines of station.0 verbatim
    for the text format."""
    run, out = run_reference("c1_stations_va", "0.6", 0, station_derivs=2)
    ids, F = read_forces(run)
    st = read_stations(run, ncol=10)
    head = open(os.path.join(run, "out", "stations", "station.0")).read()
    lines = head.split("\n")
    np.savez_compressed(os.path.join(HERE, "c1_stations_va.npz"), loaded_lnid=ids, forces=F,
                        stations=st, station0_text="\n".join(lines[:120]),
                        station0_lines_300_320="\n".join(lines[-300:-280]), dt=1e-3, end_time=0.6, freq=5.0)
    shutil.rmtree(run)
    print("c1_stations_va ok", st.shape, repr(lines[:4]))


def case_wavefield():
    """The 4D output files (output.c:886-1404: out_hdr_t header, then every simulation_output_rate
    steps all nodes' displacement (disp.h4d) / velocity (tm1 - tm2) / dt (vel.h4d) in global node
    order): 350 steps, rate 100 -> 4 output steps; one rank and eight ranks (same bytes expected
    apart from the header's random id and date)."""
    arrays = {}
    for nranks in (1, 8):
        run, out = run_reference("c1_wavefield", "0.35", 0, wavefield_rate=100, nranks=nranks)
        for q in ("disp", "vel"):
            arrays["%s_np%d" % (q, nranks)] = np.frombuffer(open(os.path.join(run, "out", q + ".h4d"), "rb").read(), np.uint8)
        if nranks == 1:
            ids, F = read_forces(run)
        shutil.rmtree(run)
    np.savez_compressed(os.path.join(HERE, "c1_wavefield.npz"), loaded_lnid=ids, forces=F, rate=100,
                        dt=1e-3, end_time=0.35, freq=5.0, **arrays)
    print("c1_wavefield ok", {k: v.shape for k, v in arrays.items()},
          "np1 == np8 past the header:", np.array_equal(arrays["disp_np1"][136:], arrays["disp_np8"][136:]),
          np.array_equal(arrays["vel_np1"][136:], arrays["vel_np8"][136:]))


def case_planes():
    """Two output planes (io_planes.c), one horizontal at depth, one dipping 60 degrees with a
    strike of 30; every grid point inside the mesh."""
    planes = [(300.0, 200.0, 100.0, 50.0, 9, 40.0, 7, 0.0, 0.0),
              (250.0, 300.0, 20.0, 45.0, 8, 35.0, 6, 30.0, 60.0)]
    run, out = run_reference("c1_planes", "0.4", 400, planes=planes, plane_rate=50)
    ids, F = read_forces(run)
    arrays = {}
    for i, p in enumerate(planes):
        raw = np.fromfile(os.path.join(run, "out", "planes", "planedisplacements.%d" % i), "<f8")
        arrays["plane%d" % i] = raw.reshape(-1, p[4] * p[6], 3)
    np.savez_compressed(os.path.join(HERE, "c1_planes.npz"), loaded_lnid=ids, forces=F,
                        plane_specs=np.array(planes), plane_rate=50,
                        surface_corners_lon_lat=np.array([[0.0, 0.0], [0.0, 1000.0], [1000.0, 1000.0], [1000.0, 0.0]]),
                        domain_xyz=np.array([1000.0, 1000.0, 500.0]), dt=1e-3, end_time=0.4, freq=5.0, **arrays)
    shutil.rmtree(run)
    print("c1_planes ok", {k: v.shape for k, v in arrays.items()})


def case_full():
    run, out = run_reference("c1_full", "20", 6000, printk="yes")
    ids, F = read_forces(run)
    ck = {}
    for f in ("checkpoint.out0", "checkpoint.out1"):
        step, blocks = read_checkpoint(os.path.join(run, "out", "checkpoints", f))
        ck[step] = blocks[0]
    st = read_stations(run)
    exp = []
    for i in range(5):
        raw = bz2.open(os.path.join(REF, "examples", "simple", "expected-out", "stations",
                                    "station.%d.bz2" % i)).read().decode()
        exp.append(read_station_text(raw))
    exp = np.stack(exp)
    # forces: the source is a scalar time function times a fixed nodal pattern,
    # but keep the raw table (float64, exact) so nothing is re-derived.
    np.savez_compressed(os.path.join(HERE, "c1_full.npz"),
                        loaded_lnid=ids, forces=F,
                        ckpt_steps=np.array(sorted(ck)),
                        ckpt_tm2=np.stack([ck[s][0] for s in sorted(ck)]),
                        ckpt_tm1=np.stack([ck[s][1] for s in sorted(ck)]),
                        stations_every20=st[:, ::20, :], expected_every20=exp[:, ::20, :],
                        stations_head=st[:, :400, :], expected_head=exp[:, :400, :],
                        max_abs_run_vs_expected=np.abs(st[:, :exp.shape[1], 1:] - exp[:, :st.shape[1], 1:]).max(),
                        dt=1e-3, end_time=20.0, freq=5.0)
    open(os.path.join(HERE, "c1_full_stdout_K.txt"), "w").write(
        "\n".join(l for l in out.splitlines() if re.search(r"K[123]|^\s*[-+]?\d+\.\d+", l))[:200000])
    shutil.rmtree(run)
    print("c1_full ok", sorted(ck), "run-vs-expected max abs",
          np.abs(st[:, :exp.shape[1], 1:] - exp[:, :st.shape[1], 1:]).max())


def case_mid():
    """Mid-size pin: the same material database at f = 40 Hz, dt = 0.5 ms makes
    the reference's mesher refine examples/simple to 128 x 128 x 64 = 1 048 576 elements /
    1 081 665 nodes.  One rank, 300 steps, checkpoint at step 200 (52 MB: too big to commit), so
    the fixture keeps the force file, the field at 4096 seeded-random nodes plus the 256 nodes of
    largest |u|, each with its tick coordinates (from the reference's own mesh.e, read with the
    repo's etree reader), and field-wide maxima and sums."""
    sys.path.insert(0, ROOT)
    from hercules_amd import host as hhost
    run, out = run_reference("c2_mid", "0.15", 200, freq=40, dt=0.0005)
    ids, F = read_forces(run)
    step, blocks = read_checkpoint(os.path.join(run, "out", "checkpoints", "checkpoint.out0"))
    assert step == 200, step
    tm2, tm1 = blocks[0]
    ticks, level, vals = hhost.etree_read(os.path.join(run, "out", "mesh.e"))
    nid, edata = hhost.mesh_payload(vals)
    E, N = len(nid), len(tm1)
    edge = 1 << (30 - int(level[0]))                  # octor ticks per element edge (PIXELLEVEL 30, octor.h)
    assert (level == level[0]).all()
    node_ticks = np.zeros((N, 3), np.int64)
    for c in range(8):
        off = np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], np.int64) * edge
        node_ticks[nid[:, c]] = ticks.astype(np.int64) + off
    rng = np.random.default_rng(12345)
    amp = np.abs(tm1).max(axis=1)
    sample = np.unique(np.concatenate([rng.choice(N, 4096, replace=False), np.argsort(amp)[-256:], ids]))
    np.savez_compressed(os.path.join(HERE, "c2_mid.npz"),
                        elements=E, nodes=N, edge_ticks=edge, edata=edata[0],
                        loaded_lnid=ids, loaded_ticks=node_ticks[ids], forces=F[:200],
                        sample_lnid=sample.astype(np.int32), sample_ticks=node_ticks[sample],
                        sample_tm1=tm1[sample], sample_tm2=tm2[sample],
                        max_abs_tm1=np.abs(tm1).max(), max_abs_tm2=np.abs(tm2).max(),
                        sum_tm1=tm1.sum(axis=0), sum_abs_tm1=np.abs(tm1).sum(axis=0),
                        ckpt_step=200, dt=0.0005, freq=40.0, end_time=0.15)
    shutil.rmtree(run)
    print("c2_mid ok", E, N, "max |tm1|", np.abs(tm1).max())


def case_np(nranks):
    name = "c1_np%d" % nranks
    run, out = run_reference(name, "1.0", 400, nranks=nranks)
    meshes = [read_mesh(run, r) for r in range(nranks)]
    harbored = []
    per_rank = {}
    sched = open(os.path.join(run, "stat-sched.txt")).read() if os.path.exists(os.path.join(run, "stat-sched.txt")) else ""
    meshstat = open(os.path.join(run, "stat-mesh.txt")).read() if os.path.exists(os.path.join(run, "stat-mesh.txt")) else ""
    forces = [read_forces(run, r) for r in range(nranks)]
    arrays = {}
    ckfiles = {}
    for f in ("checkpoint.out0", "checkpoint.out1"):
        step, blocks = read_checkpoint(os.path.join(run, "out", "checkpoints", f))
        ckfiles[step] = blocks
    for r in range(nranks):
        arrays["elem_ticks_%d" % r] = meshes[r][0]
        arrays["loaded_lnid_%d" % r] = forces[r][0]
        arrays["forces_%d" % r] = forces[r][1]
        for s in sorted(ckfiles):
            arrays["ckpt%d_tm2_%d" % (s, r)] = ckfiles[s][r][0]
            arrays["ckpt%d_tm1_%d" % (s, r)] = ckfiles[s][r][1]
    st = read_stations(run)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), ckpt_steps=np.array(sorted(ckfiles)),
                        stations=st, stat_sched=np.array(sched), stat_mesh=np.array(meshstat),
                        dt=1e-3, end_time=1.0, freq=5.0, **arrays)
    shutil.rmtree(run)
    print(name, "ok")


def case_cvm():
    """The material databases of the octree cases that the tests mesh without the reference's tools, as oracle/make_cvm
    writes them on the reference's own etree + cvm libraries: tests/golden/cvm/<name>.e."""
    sys.path.insert(0, ROOT)
    from tests.test_host_partition import _cvm_args
    os.makedirs(os.path.join(HERE, "cvm"), exist_ok=True)
    for name in ("c5_basin", "c5_gradient", "c5_three_level"):
        subprocess.check_call([os.path.join(ROOT, "oracle", "_ref", "make_cvm"), os.path.join(HERE, "cvm", name + ".e")] +
                              _cvm_args(name))
    print("cvm ok")


def case_two_level():
    """Soft top layer (2 octant layers = 125 m, Vs 1732) over the stiff half-space: the
    reference's Vs rule refines the top one level deeper -> 2:1 interface with hanging nodes."""
    _octree_case("c5_two_level", "1.0", 400, [2, 3000, 1732, 2200, 6000, 3464, 2700], 500, 5.0)


def case_three_level():
    """Three materials chosen to take every branch of mu_and_lambda / the damping threshold
    (psolve.c:3236-3272, 3397-3401): a very soft layer (Vp/Vs = 10 > cap 3, zeta capped), a
    layer with Vp^2 < 2 Vs^2 (negative lambda -> Vp rewritten) and the stiff half-space; at
    f = 0.25 Hz the Vs rule leaves elements of 62.5, 125 and 250 m: a three-level octree."""
    _octree_case("c5_three_level", "0.4", 100,
                 ["layers", 3, 0, 1500, 150, 1800, 2, 2500, 2000, 2300, 4, 6000, 3464, 2700], 100, 0.25)


def case_layered():
    """A layered model that makes the mesher do everything the layered-column helper
    (hqh_layered_column) restates: Vs rule on the minimum of a leaf's samples (three materials:
    Vs 200 / 450 / 1200 m/s over 0-62.5 / 62.5-187.5 / 187.5-500 m; f = 0.5 Hz, 8 points per
    wavelength: edges of 31.25, 62.5 and 250 m), then 2:1 balancing (the 250 m leaves next to
    62.5 m ones are split), several materials inside one level."""
    _octree_case("c5_layered", "0.1", 30,
                 ["layers", 3, 0, 800, 200, 1700, 1, 1500, 450, 2000, 3, 2600, 1200, 2300], 100, 0.5,
                 keep_mesh_etree=True)


def case_single(name, end_time, ckpt_rate, cvm_args=None, vscut=None, freq=None, **kw):
    """-DSINGLE_PRECISION_SOLVER (psolve.h:60-64): tm1 / tm2 / force and the n_t rows are floats, e_t and every local
    the reference declares double stay double.  Same inputs as the double-precision cases; checkpoints are rows of three
    floats, stations the usual text."""
    run, out = run_reference(name, end_time, ckpt_rate, cvm_args=cvm_args, vscut=vscut, freq=freq, single=True, **kw)
    ids, F = read_forces(run)
    elem_ticks, mat = read_mesh(run)
    ck = {}
    for f in ("checkpoint.out0", "checkpoint.out1"):
        step, blocks = read_checkpoint(os.path.join(run, "out", "checkpoints", f), real="<f4")
        ck[step] = blocks[0]
    st = read_stations(run)
    m = re.search(r"Total dangling nodes:\s+(\d+)", out)
    np.savez_compressed(os.path.join(HERE, name + ".npz"),
                        elem_ticks=elem_ticks, mat_vs_vp_rho=mat, loaded_lnid=ids, forces=F,
                        ckpt_steps=np.array(sorted(ck)),
                        ckpt_tm2=np.stack([ck[s][0] for s in sorted(ck)]),
                        ckpt_tm1=np.stack([ck[s][1] for s in sorted(ck)]),
                        stations=st, dt=1e-3, end_time=float(end_time), freq=5.0 if freq is None else freq,
                        total_dangling=int(m.group(1)) if m else 0)
    shutil.rmtree(run)
    print(name, "ok", sorted(ck), ck[sorted(ck)[0]][0].dtype)


BASIN_CVM = ["regions", 4, 6000, 3464, 2700, 2,
             "dip", 3.2, -0.3, -0.12, 3000, 1732, 2200,          # a sediment wedge thinning towards +x, +y
             "box", 12, 16, 9, 13, 0, 2, 1500, 866, 1800]        # a soft box at the surface against the far-x face


# the same basin with a velocity gradient: every database octant has a material of its own (what a real CVM gives --
# setrec's 27-sample average differs from element to element, psolve.c:1307-1397), so NO two neighbouring coarse elements
# share (c1, c2, beta) and the per-element-coefficient kernels run inside every octree level, beside hanging nodes
GRADIENT_CVM = ["regions", 4, 6000, 3464, 2700, 3,
                "dip", 3.2, -0.3, -0.12, 3000, 1732, 2200,
                "box", 12, 16, 9, 13, 0, 2, 1500, 866, 1800,
                "grad", 0.10, -0.06, 0.12]


def case_basin():
    """A LATERALLY refined octree (BASELINE config 5's "basin" in miniature): the material varies with
    (i, j, k) -- a dipping sediment wedge and a soft box against a domain face -- so the reference's Vs rule
    (psolve.c:1308 setrec, :2185 toexpand, quake_util.c:215 vsrule) and 2:1 balancing (octor.c:4398) leave
    refinement interfaces with x-, y- and z-normal faces, staircase corners and hanging nodes of every
    orientation (X/Y/ZEDGE, XY/XZ/YZ faces, on domain faces too: node_setproperty octor.c:3294).
    5429 elements on three levels, 1196 hanging nodes."""
    _octree_case("c5_basin", "0.3", 100, BASIN_CVM, 100, 5.0)


def case_octree_np(name, base, nranks, end_time, ckpt_rate, cvm_args, vscut, freq, single=False):
    """The same octree models on `nranks` MPI ranks: per-rank element dumps, force files and
    checkpoint stripes pin octor's multi-rank tables (block partition, ownership by containing
    leaf, direct + indirect sharing octor.c:5516-6040, dnodeTable of owned hanging nodes)."""
    run, out = run_reference(name, end_time, ckpt_rate, cvm_args=cvm_args, vscut=vscut, freq=freq, nranks=nranks, single=single)
    real, row = ("<f4", 12) if single else ("<f8", 24)          # -DSINGLE_PRECISION_SOLVER: rows of three floats
    # A rank's stripe holds nharbored (not nharboredmax) records per field, so the raw stripes
    # are kept and parsed by whoever knows each rank's nharbored (io_checkpoint.c:93-118).
    ckfiles = {}
    nmax = 0
    for f in ("checkpoint.out0", "checkpoint.out1"):
        b = open(os.path.join(run, "out", "checkpoints", f), "rb").read()
        groupsize, step, nmax = [int(v) for v in np.frombuffer(b[:12], "<i4")]
        ckfiles[step] = [np.frombuffer(b[12 + 2 * r * nmax * row: 12 + 2 * (r + 1) * nmax * row], real).copy()
                         for r in range(groupsize)]
    arrays = {"nharboredmax": nmax}
    for r in range(nranks):
        et, _ = read_mesh(run, r)
        ids, F = read_forces(run, r)
        arrays["elem_ticks_%d" % r] = et
        arrays["loaded_lnid_%d" % r] = ids
        arrays["forces_%d" % r] = F
        for s_ in sorted(ckfiles):
            arrays["ckpt%d_stripe_%d" % (s_, r)] = ckfiles[s_][r]
    meshstat = open(os.path.join(run, "stat-mesh.txt")).read() if os.path.exists(os.path.join(run, "stat-mesh.txt")) else ""
    sched = open(os.path.join(run, "stat-sched.txt")).read() if os.path.exists(os.path.join(run, "stat-sched.txt")) else ""
    np.savez_compressed(os.path.join(HERE, name + ".npz"), ckpt_steps=np.array(sorted(ckfiles)), nranks=nranks,
                        base=np.array(base), stat_mesh=np.array(meshstat), stat_sched=np.array(sched), **arrays)
    shutil.rmtree(run)
    print(name, "ok", sorted(ckfiles))


def _octree_case(name, end_time, ckpt_rate, cvm_args, vscut, freq, keep_mesh_etree=False):
    run, out = run_reference(name, end_time, ckpt_rate, cvm_args=cvm_args, vscut=vscut, freq=freq)
    extra = {}
    if keep_mesh_etree:
        # the mesh database the reference wrote (mesh_output, psolve.c:2361-2562), bz2-compressed
        extra["mesh_e_bz2"] = np.frombuffer(bz2.compress(open(os.path.join(run, "out", "mesh.e"), "rb").read()), np.uint8)
    ids, F = read_forces(run)
    elem_ticks, mat = read_mesh(run)
    ck = {}
    for f in ("checkpoint.out0", "checkpoint.out1"):
        step, blocks = read_checkpoint(os.path.join(run, "out", "checkpoints", f))
        ck[step] = blocks[0]
    st = read_stations(run)
    counts = {k: int(re.search(k + r":\s+(\d+)", out).group(1))
              for k in ("Total elements", "Total nodes", "Total dangling nodes")}
    np.savez_compressed(os.path.join(HERE, name + ".npz"),
                        elem_ticks=elem_ticks, mat_vs_vp_rho=mat, loaded_lnid=ids, forces=F,
                        ckpt_steps=np.array(sorted(ck)),
                        ckpt_tm2=np.stack([ck[s][0] for s in sorted(ck)]),
                        ckpt_tm1=np.stack([ck[s][1] for s in sorted(ck)]),
                        stations=st, dt=1e-3, end_time=float(end_time), freq=freq,
                        total_elements=counts["Total elements"], total_nodes=counts["Total nodes"],
                        total_dangling=counts["Total dangling nodes"], **extra)
    shutil.rmtree(run)
    print(name, "ok", counts, sorted(ck))


CASES = {
    "c1_short": lambda: case_short("c1_short"),
    "c1_conv": lambda: case_short("c1_conv", stiffness="conventional"),
    "c1_none": lambda: case_short("c1_none", damping="none"),
    "c1_mass": lambda: case_short("c1_mass", damping="mass"),
    "c1_full": case_full,
    "c1_planes": case_planes,
    "c1_wavefield": case_wavefield,
    "c1_stations_va": case_stations_va,
    "c1_np8": lambda: case_np(8),
    # the same run on 4 ranks: few enough processes to share one GPU (tests/test_gpu_reference_link.py)
    "c1_np4": lambda: case_np(4),
    "cvm": case_cvm,
    "c2_mid": case_mid,
    "c5_two_level": case_two_level,
    "c5_three_level": case_three_level,
    "c5_layered": case_layered,
    "c5_two_level_np8": lambda: case_octree_np("c5_two_level_np8", "c5_two_level", 8, "0.5", 200,
                                               [2, 3000, 1732, 2200, 6000, 3464, 2700], 500, 5.0),
    "c5_basin": case_basin,
    "c5_gradient": lambda: _octree_case("c5_gradient", "0.3", 100, GRADIENT_CVM, 100, 5.0),
    "c5_gradient_np8": lambda: case_octree_np("c5_gradient_np8", "c5_gradient", 8, "0.3", 100, GRADIENT_CVM, 100, 5.0),
    "c5_basin_np8": lambda: case_octree_np("c5_basin_np8", "c5_basin", 8, "0.3", 100, BASIN_CVM, 100, 5.0),
    "c5_basin_np5": lambda: case_octree_np("c5_basin_np5", "c5_basin", 5, "0.3", 100, BASIN_CVM, 100, 5.0),
    # the reference's single-precision build on the uniform box (effective and conventional stiffness) and on the
    # two-level octree (compute_adjust on float tables)
    "c1_f32": lambda: case_single("c1_f32", "1.0", 400),
    "c1_conv_f32": lambda: case_single("c1_conv_f32", "0.5", 200, stiffness="conventional"),
    "c5_two_level_f32": lambda: case_single("c5_two_level_f32", "0.5", 200, [2, 3000, 1732, 2200, 6000, 3464, 2700], 500, 5.0),
    # ... and on 8 MPI ranks: the reference's exchanges of float records (schedule_senddata on solver_float, psolve.c:4985-5073),
    # the mass exchange on float n_t rows at init, shared hanging nodes
    "c5_two_level_np8_f32": lambda: case_octree_np("c5_two_level_np8_f32", "c5_two_level", 8, "0.3", 100,
                                                   [2, 3000, 1732, 2200, 6000, 3464, 2700], 500, 5.0, single=True),
    # (a 5-rank run of the three-level mesh was tried and is NOT a fixture: on 5 ranks the
    #  reference's mesher refines that model uniformly, so it pins nothing the others do not)
}

if __name__ == "__main__":
    if not os.path.exists(PSOLVE):
        sys.exit("build oracle/_ref/psolve first (oracle/build_ref.sh)")
    for c in (sys.argv[1:] or list(CASES)):
        CASES[c]()
