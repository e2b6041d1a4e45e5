"""ctypes binding of include/hq_solver.h (the stub a Python host would use).

Fails loudly when the native library is missing or no gfx950 device is present:
there is no fallback implementation.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBPATH = os.environ.get("HQ_SOLVER_LIB") or os.path.join(_HERE, "csrc", "libhq_solver.so")   # (HQ_SOLVER_LIB: experiment builds, profiles/tools)

HQ_VARIANT_AUTO, HQ_VARIANT_SCATTER, HQ_VARIANT_PATCH = 0, 1, 2
IPC_BLOB_BYTES = 4096                   # HQ_IPC_BLOB_BYTES

EXPORTS = ["hq_device_count", "hq_last_error", "hq_create", "hq_destroy", "hq_get_info", "hq_get_info_sized", "hq_abi_version", "hq_comm_init_ipc_n",
           "hq_options_init", "hq_create_opts", "hq_get_options", "hq_real_bytes",
           "hq_comm_unique_id", "hq_comm_init", "hq_comm_selftest", "hq_group_link", "hq_group_run", "hq_set_source", "hq_run", "hq_sync", "hq_gather", "hq_gather3",
           "hq_download", "hq_upload", "hq_phase_force", "hq_phase_update", "hq_download_force",
           "hq_run_timed", "hq_dominant_kernel", "hq_plan_check", "hq_stencil_plan_check", "hq_check_finite",
           "hq_stencil_coefficients", "hq_brick_plan_check", "hq_brick_plan_check_n", "hq_comm_init_host",
           "hq_comm_ipc_export", "hq_comm_init_ipc", "hq_comm_init_loopback",
           "hq_record_add", "hq_record_pending", "hq_record_fetch", "hq_record_clear",
           "hq_snapshot_add", "hq_snapshot_pending", "hq_snapshot_fetch", "hq_snapshot_clear",
           "hq_peak_add", "hq_peak_fetch", "hq_peak_load", "hq_peak_reset", "hq_peak_clear",
           "hq_spec_add", "hq_spec_coefficients", "hq_spec_fetch", "hq_spec_load", "hq_spec_reset", "hq_spec_clear",
           "hq_cum_add", "hq_cum_fetch", "hq_cum_load", "hq_cum_reset", "hq_cum_clear",
           "hq_deform_add", "hq_deform_fetch", "hq_deform_load", "hq_deform_reset", "hq_deform_clear",
           "hq_attenuation_set", "hq_attenuation_info", "hq_attenuation_fetch", "hq_attenuation_load", "hq_attenuation_clear",
           "hq_attenuation_plan_check", "hq_attenuation_set_split", "hq_attenuation_split_plan_check", "hq_attenuation_split_plan_tables",
           "hq_attenuation_split_table_faults",
           "hq_nonlinear_set", "hq_nonlinear_info", "hq_nonlinear_fetch", "hq_nonlinear_load", "hq_nonlinear_clear", "hq_nonlinear_plan_check",
           "hq_nonlinear_plan_tables", "hq_nonlinear_table_faults"]
HQ_SNAP_TM1, HQ_SNAP_TM2, HQ_SNAP_VEL = 1, 2, 4
HQ_PEAK_DISP, HQ_PEAK_VEL, HQ_PEAK_ACC = 1, 2, 4
HQ_SPEC_MAX_PERIODS, HQ_SPEC_NVAL = 32, 4
HQ_DEFORM_STRAIN, HQ_DEFORM_STRAIN_RATE, HQ_DEFORM_STRESS, HQ_DEFORM_ROTATION, HQ_DEFORM_ROTATION_RATE = 1, 2, 4, 8, 16
HQ_DEFORM_ALL = 31
HQ_NL_VONMISES, HQ_NL_DRUCKERPRAGER = 1, 2


class HqError(RuntimeError):
    pass


# hq_host_exchange_fn (include/hq_solver.h)
HOST_EXCHANGE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                    ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int32,
                                    ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64),
                                    ctypes.POINTER(ctypes.c_void_p), ctypes.c_int32)


class _Messenger(ctypes.Structure):
    _fields_ = [("procid", ctypes.c_int32), ("nodecount", ctypes.c_int32),
                ("mapping", ctypes.c_void_p)]


class _Schedule(ctypes.Structure):
    _fields_ = [("c_count", ctypes.c_int32), ("first_c", ctypes.POINTER(_Messenger)),
                ("s_count", ctypes.c_int32), ("first_s", ctypes.POINTER(_Messenger))]


class _Desc(ctypes.Structure):
    _fields_ = [("lenum", ctypes.c_int32), ("nharbored", ctypes.c_int32), ("ldnnum", ctypes.c_int32),
                ("lnid", ctypes.c_void_p), ("node_xyz", ctypes.c_void_p),
                ("dn_ldnid", ctypes.c_void_p), ("dn_ptr", ctypes.c_void_p), ("dn_lanid", ctypes.c_void_p),
                ("eTable", ctypes.c_void_p), ("nTable", ctypes.c_void_p),
                ("tm1", ctypes.c_void_p), ("tm2", ctypes.c_void_p),
                ("an_sched", _Schedule), ("dn_sched", _Schedule),
                ("deltaT", ctypes.c_double), ("rank", ctypes.c_int32), ("nranks", ctypes.c_int32),
                ("variant", ctypes.c_int32), ("reserved", ctypes.c_int32), ("node_gnid", ctypes.c_void_p),
                ("edata", ctypes.c_void_p), ("mat_bbase", ctypes.c_double), ("mat_threshold_damping", ctypes.c_double),
                ("mat_threshold_vpvs", ctypes.c_double)]


class _AttenuationDesc(ctypes.Structure):
    _fields_ = [("coef", ctypes.c_void_p), ("freq", ctypes.c_double)]


class _NonlinearDesc(ctypes.Structure):
    _fields_ = [("model", ctypes.c_int32), ("nelems", ctypes.c_int32), ("elems", ctypes.c_void_p), ("cons", ctypes.c_void_p)]


def _nonlinear_desc(model, elems, cons, who):
    """hq_nonlinear_desc of elems [n] and cons [n, 6]; the arrays are kept alive on the returned object."""
    elems = np.ascontiguousarray(elems, np.int32).reshape(-1)
    cons = np.ascontiguousarray(cons, np.float64).reshape(-1, 6)
    if len(cons) != len(elems):
        raise HqError("%s: cons %r is not [%d, 6]" % (who, cons.shape, len(elems)))
    d = _NonlinearDesc(int(model), len(elems), _ptr(elems) if len(elems) else None, _ptr(cons) if len(elems) else None)
    d._keep = (elems, cons)
    return d


class _RecorderDesc(ctypes.Structure):
    _fields_ = [("npoints", ctypes.c_int32), ("ids", ctypes.c_void_p), ("phi", ctypes.c_void_p),
                ("rate", ctypes.c_int32), ("derivs", ctypes.c_int32), ("capacity", ctypes.c_int32)]


class _SnapshotDesc(ctypes.Structure):
    _fields_ = [("first", ctypes.c_int32), ("count", ctypes.c_int32), ("rate", ctypes.c_int32),
                ("first_step", ctypes.c_int32), ("fields", ctypes.c_int32), ("slots", ctypes.c_int32)]


class _PeakDesc(ctypes.Structure):
    _fields_ = [("npoints", ctypes.c_int32), ("nodes_per_point", ctypes.c_int32), ("ids", ctypes.c_void_p),
                ("phi", ctypes.c_void_p), ("rate", ctypes.c_int32), ("first_step", ctypes.c_int32),
                ("quantities", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class _SpecDesc(ctypes.Structure):
    _fields_ = [("npoints", ctypes.c_int32), ("nodes_per_point", ctypes.c_int32), ("ids", ctypes.c_void_p),
                ("phi", ctypes.c_void_p), ("rate", ctypes.c_int32), ("first_step", ctypes.c_int32),
                ("nperiods", ctypes.c_int32), ("reserved", ctypes.c_int32), ("periods", ctypes.c_void_p),
                ("damping", ctypes.c_double)]


class _CumDesc(ctypes.Structure):
    _fields_ = [("npoints", ctypes.c_int32), ("nodes_per_point", ctypes.c_int32), ("ids", ctypes.c_void_p),
                ("phi", ctypes.c_void_p), ("rate", ctypes.c_int32), ("first_step", ctypes.c_int32),
                ("quantities", ctypes.c_int32), ("husid_every", ctypes.c_int32), ("husid_slots", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("threshold", ctypes.c_double * 3)]


class _DeformDesc(ctypes.Structure):
    _fields_ = [("npoints", ctypes.c_int32), ("ids", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("lame", ctypes.c_void_p),
                ("rate", ctypes.c_int32), ("first_step", ctypes.c_int32), ("quantities", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class _Info(ctypes.Structure):
    _fields_ = [("variant", ctypes.c_int32), ("npatches", ctypes.c_int32),
                ("patch_pairs", ctypes.c_int64), ("device_bytes", ctypes.c_int64),
                ("step", ctypes.c_int32), ("nranks", ctypes.c_int32),
                ("lattice_patches", ctypes.c_int32), ("stencil_patches", ctypes.c_int32),
                ("ragged_patches", ctypes.c_int32), ("brick_units", ctypes.c_int32),
                ("brick_nodes", ctypes.c_int64), ("brick_units_pernode", ctypes.c_int32),
                ("brick_units_het", ctypes.c_int32), ("pcie_h2d_bytes", ctypes.c_int64),
                ("pcie_d2h_bytes", ctypes.c_int64), ("transport", ctypes.c_int32), ("ipc_arena_coarse", ctypes.c_int32),
                ("ipc_arena_kind", ctypes.c_int32), ("debug_halo", ctypes.c_int32),
                ("brick_units_packed", ctypes.c_int32), ("brick_units_ragged", ctypes.c_int32),
                ("brick_stream", ctypes.c_int32), ("brick_units_ragged_het", ctypes.c_int32), ("timed_steps", ctypes.c_int64),
                ("t_step_us", ctypes.c_double), ("t_shell_us", ctypes.c_double), ("t_interior_us", ctypes.c_double),
                ("t_chain_us", ctypes.c_double), ("t_chain_exposed_us", ctypes.c_double)]


# hq_options (include/hq_solver.h): int32 fields in the header's order, two doubles, two more int32
OPTION_FIELDS = ["no_bricks", "brick_cz", "brick_minz", "brick_minnodes", "brick_no_het", "brick_no_ntsame", "brick_by_component",
                 "brick_stream", "brick_no_faces", "brick_half_tiles", "brick_no_pack", "patch_pipe", "patch_threads", "patch_pmax", "patch_pmerge", "patch_psplit", "patch_nlmax",
                 "patch_vmax", "patch_ragged", "patch_no_lattice", "patch_no_stencil", "patch_no_uniform", "patch_no_iso",
                 "patch_no_ntsame", "patch_no_dedup", "patch_wform", "patch_merge_rounds", "overlap", "no_overlap", "reserve_cus",
                 "cu_mask", "no_fused_share", "group_copies", "debug_halo", "ipc_arena"]


class Options(ctypes.Structure):
    """hq_options.  Options(brick_cz=16, debug_halo=1): every other field stays -1 = library default."""
    _fields_ = ([("size", ctypes.c_uint64)] + [(n, ctypes.c_int32) for n in OPTION_FIELDS] +
                [("ipc_timeout_ms", ctypes.c_double), ("loopback_delay_us", ctypes.c_double),
                 ("verbose", ctypes.c_int32), ("quiet", ctypes.c_int32),
                 ("brick_ragged", ctypes.c_int32), ("brick_ragged_minfill", ctypes.c_int32),
                 ("allow_env", ctypes.c_int32), ("brick_ragged_het", ctypes.c_int32), ("reserved0", ctypes.c_int32),
                 ("phase_timing", ctypes.c_int32)])

    def __init__(self, **kw):
        super().__init__()
        load_library().hq_options_init(ctypes.byref(self), ctypes.c_uint64(ctypes.sizeof(self)))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("hq_options has no field %r" % k)
            setattr(self, k, v)

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "size"}


_lib = None
_lib_f32 = None
# the float build stays anchored in the package (HQ_SOLVER_LIB names an experiment build of the fp64 library only);
# HQ_SOLVER_LIB_F32 names an experiment build of the float one
_LIBPATH_F32 = os.environ.get("HQ_SOLVER_LIB_F32") or os.path.join(_HERE, "csrc", "libhq_solver_f32.so")


def load_library(path=None, precision="f64"):
    """dlopen libhq_solver.so; raises HqError if it was not built.
    precision="f32": libhq_solver_f32.so -- the same sources with -DHQ_SINGLE_PRECISION_SOLVER (hq_real = float: the
    reference's -DSINGLE_PRECISION_SOLVER, psolve.h:60-64); a separately named build, never the default."""
    global _lib, _lib_f32
    if precision == "f32" and path is None:
        if _lib_f32 is None:
            _lib_f32 = load_library(_LIBPATH_F32)
            if _lib_f32.hq_real_bytes() != 4:
                raise HqError("%s was not built with -DHQ_SINGLE_PRECISION_SOLVER" % _LIBPATH_F32)
        return _lib_f32
    if _lib is not None and path is None:
        return _lib
    p = path or _LIBPATH
    if not os.path.exists(p):
        raise HqError("native library %s is missing: run `python -m hercules_amd.build` "
                      "(there is no Python/CPU fallback)" % p)
    # libhq_solver.so and its _f32 build export the same names: only the fp64 one joins the global scope (libhq_host.so's
    # references must never bind to the float build, whichever was loaded first); both are linked -Bsymbolic, so calls
    # between their own entry points stay inside the library they belong to
    # (which of the two a file is, is asked of the file -- hq_real_bytes -- not read off its name)
    probe = ctypes.CDLL(p, mode=ctypes.RTLD_LOCAL)
    lib = probe if probe.hq_real_bytes() == 4 else ctypes.CDLL(p, mode=ctypes.RTLD_GLOBAL)
    lib.hq_last_error.restype = ctypes.c_char_p
    lib.hq_dominant_kernel.restype = ctypes.c_char_p
    lib.hq_dominant_kernel.argtypes = [ctypes.c_void_p]
    for name in EXPORTS:
        getattr(lib, name)          # AttributeError if the ABI is incomplete
    if path is None:
        _lib = lib
    return lib


def device_count():
    return int(load_library().hq_device_count())


def _check(rc, lib=None):
    if rc != 0:
        raise HqError("hq error %d: %s" % (rc, (lib or load_library()).hq_last_error().decode()))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


_PAD = np.zeros(1)


def _ptr_or_pad(a):
    """_ptr, but an empty array has no address worth passing: a pad's instead (nothing is read or written there)."""
    return None if a is None else _ptr(a if a.size else _PAD)


# the trackers' kinds: the prefix of their entry points -> the word of their error texts
_TRACKER_KINDS = {"peak": "peak", "spec": "spectrum", "cum": "cumulative", "deform": "deformation"}


def _no_trackers():
    """Solver._trackers of a fresh context: per kind, handle -> the shape its fetch and load size their arrays by."""
    return {kind: {} for kind in _TRACKER_KINDS}


def _schedule(sched, keep):
    """sched = {"c": [(procid, mapping ndarray), ...], "s": [...]} or None."""
    out = _Schedule()
    if not sched:
        return out
    for key, cnt, first in (("c", "c_count", "first_c"), ("s", "s_count", "first_s")):
        items = sched.get(key, [])
        arr = (_Messenger * max(len(items), 1))()
        for i, (procid, mapping) in enumerate(items):
            m = np.ascontiguousarray(mapping, np.int32)
            keep.append(m)
            arr[i].procid = int(procid)
            arr[i].nodecount = len(m)
            arr[i].mapping = m.ctypes.data
        keep.append(arr)
        setattr(out, cnt, len(items))
        setattr(out, first, ctypes.cast(arr, ctypes.POINTER(_Messenger)))
    return out


class Solver:
    """One device-resident partition (hq_ctx)."""

    def __init__(self, lnid, etable, ntable, dt, tm1=None, tm2=None, node_xyz=None,
                 dangling=None, an_sched=None, dn_sched=None, rank=0, nranks=1,
                 variant=HQ_VARIANT_AUTO, device=0, options=None, edata=None, material=None, precision="f64"):
        """options: an Options (hq_options) or a dict of its fields; None = hq_create's defaults.
        precision: "f64", or "f32" = libhq_solver_f32.so (hq_real = float: ntable, tm1, tm2 and everything gathered or
        downloaded are float32 arrays, as the reference's -DSINGLE_PRECISION_SOLVER arrays are).
        edata [E,4] float32 (edgesize, Vp, Vs, rho as solver_init left them) + material = (bBase, threshold_damping,
        threshold_vpvs): hq_desc.edata / mat_* -- lets hq_k_brick_het keep 12 bytes per element."""
        lib = load_library(precision=precision)
        self.real = np.float32 if precision == "f32" else np.float64
        if lib.hq_real_bytes() != np.dtype(self.real).itemsize:
            raise HqError("library and precision %r disagree about sizeof(hq_real)" % precision)
        if isinstance(options, dict):
            options = Options(**options)
        keep = []
        lnid = np.ascontiguousarray(lnid, np.int32)
        etable = np.ascontiguousarray(etable, np.float64)
        ntable = np.ascontiguousarray(ntable, self.real)
        d = _Desc()
        d.lenum, d.nharbored = lnid.shape[0], ntable.shape[0]
        d.lnid, d.eTable, d.nTable = _ptr(lnid), _ptr(etable), _ptr(ntable)
        keep += [lnid, etable, ntable]
        if node_xyz is not None:
            node_xyz = np.ascontiguousarray(node_xyz, np.int32)
            keep.append(node_xyz)
            d.node_xyz = _ptr(node_xyz)
        for name, a in (("tm1", tm1), ("tm2", tm2)):
            if a is not None:
                a = np.ascontiguousarray(a, self.real)
                keep.append(a)
                setattr(d, name, _ptr(a))
        if dangling is not None:
            ids, ptr, anchors = [np.ascontiguousarray(x, np.int32) for x in dangling]
            keep += [ids, ptr, anchors]
            d.ldnnum = len(ids)
            d.dn_ldnid, d.dn_ptr, d.dn_lanid = _ptr(ids), _ptr(ptr), _ptr(anchors)
        if edata is not None:
            edata = np.ascontiguousarray(edata, np.float32)
            assert edata.shape == (lnid.shape[0], 4) and material is not None
            keep.append(edata)
            d.edata = _ptr(edata)
            d.mat_bbase, d.mat_threshold_damping, d.mat_threshold_vpvs = [float(v) for v in material]
        d.an_sched = _schedule(an_sched, keep)
        d.dn_sched = _schedule(dn_sched, keep)
        d.deltaT, d.rank, d.nranks, d.variant = dt, rank, nranks, variant
        self._h = ctypes.c_void_p()
        self.N, self.E = d.nharbored, d.lenum
        self._lib = lib
        self._trackers = _no_trackers()
        if options is None:
            _check(lib.hq_create(ctypes.byref(d), ctypes.c_int(device), ctypes.byref(self._h)), lib)
        else:
            _check(lib.hq_create_opts(ctypes.byref(d), ctypes.c_int(device), ctypes.byref(options), ctypes.byref(self._h)), lib)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.hq_destroy(self._h)
            self._h = ctypes.c_void_p()

    __del__ = close

    def info(self):
        i = _Info()
        _check(self._lib.hq_get_info_sized(self._h, ctypes.byref(i), ctypes.c_uint64(ctypes.sizeof(i))), self._lib)
        return {k: getattr(i, k) for k, _ in _Info._fields_}

    def options(self):
        """hq_get_options: what the context runs with, as resolved at hq_create_opts."""
        o = Options()
        _check(self._lib.hq_get_options(self._h, ctypes.byref(o), ctypes.c_uint64(ctypes.sizeof(o))), self._lib)
        return o.as_dict()

    def set_source(self, loaded_lnid, forces, step0=0):
        ids = np.ascontiguousarray(loaded_lnid, np.int32)
        F = np.ascontiguousarray(forces, np.float64)
        nsteps = F.shape[0] if len(ids) else 0
        _check(self._lib.hq_set_source(self._h, ctypes.c_int32(len(ids)), _ptr(ids),
                                       ctypes.c_int32(step0), ctypes.c_int32(nsteps), _ptr(F)), self._lib)

    def comm_init(self, id128):
        buf = (ctypes.c_char * 128).from_buffer_copy(bytes(id128))
        _check(self._lib.hq_comm_init(self._h, buf), self._lib)

    def comm_init_host(self, exchange):
        """hq_comm_init_host: `exchange(recvs, sends, tag)` is called at every halo exchange with
        recvs = [(peer, float64 array to fill)], sends = [(peer, float64 array)] -- views of the engine's pinned
        staging buffers -- and must return when everything has arrived (the caller's MPI / gloo / ...)."""
        import numpy as np

        def view(ptr, n):
            return np.ctypeslib.as_array(ctypes.cast(ctypes.c_void_p(ptr), ctypes.POINTER(ctypes.c_double)), shape=(int(n),))

        def trampoline(user, nrecv, rpeer, rcount, rbuf, nsend, speer, scount, sbuf, tag):
            try:
                exchange([(rpeer[i], view(rbuf[i], rcount[i])) for i in range(nrecv)],
                         [(speer[i], view(sbuf[i], scount[i])) for i in range(nsend)], tag)
                return 0
            except Exception:                       # never unwind through the C frames
                import traceback
                traceback.print_exc()
                return 1
        self._host_exchange = HOST_EXCHANGE_FN(trampoline)          # keep the thunk alive with the context
        _check(self._lib.hq_comm_init_host(self._h, self._host_exchange, None), self._lib)

    def comm_ipc_export(self):
        """hq_comm_ipc_export: this rank's HQ_IPC_BLOB_BYTES blob (bytes) for the host to all-gather."""
        buf = (ctypes.c_char * IPC_BLOB_BYTES)()
        _check(self._lib.hq_comm_ipc_export(self._h, buf), self._lib)
        return bytes(buf)

    def comm_init_ipc(self, blobs):
        """hq_comm_init_ipc: `blobs` = every rank's export, in rank order (list of bytes or one bytes object)."""
        raw = blobs if isinstance(blobs, (bytes, bytearray)) else b"".join(blobs)
        if len(raw) % IPC_BLOB_BYTES:
            raise HqError("comm_init_ipc: %d bytes is not a whole number of %d-byte blobs" % (len(raw), IPC_BLOB_BYTES))
        buf = (ctypes.c_char * len(raw)).from_buffer_copy(bytes(raw))
        _check(self._lib.hq_comm_init_ipc_n(self._h, buf, ctypes.c_int32(len(raw) // IPC_BLOB_BYTES)), self._lib)

    def comm_init_loopback(self):
        _check(self._lib.hq_comm_init_loopback(self._h), self._lib)

    def comm_selftest(self, count=1024):
        _check(self._lib.hq_comm_selftest(self._h, ctypes.c_int32(count)), self._lib)

    def run(self, nsteps):
        _check(self._lib.hq_run(self._h, ctypes.c_int32(nsteps)), self._lib)

    def sync(self):
        _check(self._lib.hq_sync(self._h), self._lib)

    def check_finite(self):
        """Count of NaN / infinite values in tm1, tm2 (solver_check_nan, psolve.c:3769-3782)."""
        n = ctypes.c_int64()
        _check(self._lib.hq_check_finite(self._h, ctypes.byref(n)), self._lib)
        return int(n.value)

    def run_timed(self, nsteps):
        tot, ker = ctypes.c_double(), ctypes.c_double()
        _check(self._lib.hq_run_timed(self._h, ctypes.c_int32(nsteps), ctypes.byref(tot), ctypes.byref(ker)), self._lib)
        return tot.value, ker.value

    def dominant_kernel(self):
        return self._lib.hq_dominant_kernel(self._h).decode()

    def download(self, want_tm2=True):
        """(tm1, tm2) = u(step dt), u((step - 1) dt); tm2 is None with want_tm2=False."""
        tm1 = np.empty((self.N, 3), self.real)
        tm2 = np.empty((self.N, 3), self.real) if want_tm2 else None
        _check(self._lib.hq_download(self._h, _ptr(tm1), _ptr(tm2)), self._lib)
        return tm1, tm2

    def upload(self, tm1, tm2, step):
        a = np.ascontiguousarray(tm1, self.real)
        b = np.ascontiguousarray(tm2, self.real)
        _check(self._lib.hq_upload(self._h, _ptr(a), _ptr(b), ctypes.c_int32(step)), self._lib)

    def gather(self, lnid):
        ids = np.ascontiguousarray(np.asarray(lnid).reshape(-1), np.int32)
        o1 = np.empty((len(ids), 3), self.real)
        o2 = np.empty((len(ids), 3), self.real)
        _check(self._lib.hq_gather(self._h, ctypes.c_int32(len(ids)), _ptr(ids), _ptr(o1), _ptr(o2)), self._lib)
        return o1, o2

    def gather3(self, lnid):
        """tm1, tm2 and tm3 = u((step - 2) dt) at the given nodes (patch variant)."""
        ids = np.ascontiguousarray(np.asarray(lnid).reshape(-1), np.int32)
        o = [np.empty((len(ids), 3), self.real) for _ in range(3)]
        _check(self._lib.hq_gather3(self._h, ctypes.c_int32(len(ids)), _ptr(ids), _ptr(o[0]), _ptr(o[1]), _ptr(o[2])), self._lib)
        return tuple(o)

    def record_add(self, ids, phi, rate, derivs=0, capacity=1024):
        """hq_record_add: a device recorder of the points (ids [n,8], phi [n,8]) -- a sample at the head of every step
        that is a multiple of `rate`, kept in a ring of `capacity` samples on the device.  Returns its handle."""
        ids = np.ascontiguousarray(np.asarray(ids).reshape(-1, 8), np.int32)
        phi = np.ascontiguousarray(np.asarray(phi).reshape(-1, 8), np.float64)
        if len(ids) != len(phi):
            raise HqError("record_add: %d rows of ids, %d of phi" % (len(ids), len(phi)))
        d = _RecorderDesc(len(ids), ids.ctypes.data, phi.ctypes.data, int(rate), int(derivs), int(capacity))
        h = ctypes.c_int32(-1)
        _check(self._lib.hq_record_add(self._h, ctypes.byref(d), ctypes.byref(h)), self._lib)
        if not hasattr(self, "_recorders"):
            self._recorders = {}
        self._recorders[h.value] = (len(ids), 3 * (1 + int(derivs)))
        return h.value

    def record_pending(self, handle):
        """hq_record_pending: (samples taken or enqueued and not yet fetched, step of the oldest or -1)."""
        n, first = ctypes.c_int32(), ctypes.c_int32()
        _check(self._lib.hq_record_pending(self._h, ctypes.c_int32(handle), ctypes.byref(n), ctypes.byref(first)), self._lib)
        return n.value, first.value

    def record_fetch(self, handle, max_samples=None):
        """hq_record_fetch: (steps [k], values [k, npoints, 3 (1 + derivs)] float64) of the oldest pending samples, at
        most max_samples (None: all of them); waits for the enqueued steps."""
        pending, _ = self.record_pending(handle)                # (raises on an unknown handle)
        npoints, ncomp = self._recorders[handle]
        want = pending if max_samples is None else min(int(max_samples), pending)
        steps = np.zeros(max(want, 1), np.int32)
        vals = np.zeros((max(want, 1), npoints, ncomp))
        got = ctypes.c_int32()
        _check(self._lib.hq_record_fetch(self._h, ctypes.c_int32(handle), ctypes.c_int32(want), _ptr(vals), _ptr(steps),
                                         ctypes.byref(got)), self._lib)
        return steps[:got.value].copy(), vals[:got.value].copy()

    def record_clear(self):
        """hq_record_clear: drop every recorder of the context and its device memory."""
        _check(self._lib.hq_record_clear(self._h), self._lib)
        self._recorders = {}

    def snapshot_add(self, first=0, count=None, rate=1, first_step=0, fields=HQ_SNAP_TM1, slots=1):
        """hq_snapshot_add: a field snapshot of the nodes [first, first + count) (None: up to the last node) at the head
        of every step s >= first_step with s % rate == 0; `fields` a mask of HQ_SNAP_TM1 | TM2 | VEL, `slots` snapshots
        may be pending at once.  Returns its handle."""
        count = self.N - int(first) if count is None else int(count)
        d = _SnapshotDesc(int(first), count, int(rate), int(first_step), int(fields), int(slots))
        h = ctypes.c_int32(-1)
        _check(self._lib.hq_snapshot_add(self._h, ctypes.byref(d), ctypes.byref(h)), self._lib)
        if not hasattr(self, "_snapshots"):
            self._snapshots = {}
        self._snapshots[h.value] = (count, int(fields))
        return h.value

    def snapshot_pending(self, handle):
        """hq_snapshot_pending: (snapshots taken or enqueued and not yet fetched, those of them that have arrived in host
        memory, step of the oldest or -1).  Waits for nothing."""
        n, ready, first = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _check(self._lib.hq_snapshot_pending(self._h, ctypes.c_int32(handle), ctypes.byref(n), ctypes.byref(ready),
                                             ctypes.byref(first)), self._lib)
        return n.value, ready.value, first.value

    def snapshot_fetch(self, handle):
        """hq_snapshot_fetch: (step, tm1, tm2, vel) of the OLDEST pending snapshot -- tm1, tm2 [count, 3] in the solver's
        precision, vel [count, 3] float64, None for a field the snapshot lacks; (-1, None, None, None) if nothing is
        pending.  Waits for that snapshot's copy only, not for the steps enqueued behind it."""
        self.snapshot_pending(handle)                           # (raises on an unknown handle)
        count, fields = self._snapshots[handle]
        tm1 = np.empty((count, 3), self.real) if fields & HQ_SNAP_TM1 else None
        tm2 = np.empty((count, 3), self.real) if fields & HQ_SNAP_TM2 else None
        vel = np.empty((count, 3), np.float64) if fields & HQ_SNAP_VEL else None
        step = ctypes.c_int32(-1)
        _check(self._lib.hq_snapshot_fetch(self._h, ctypes.c_int32(handle), _ptr(tm1), _ptr(tm2), _ptr(vel),
                                           ctypes.byref(step)), self._lib)
        if step.value < 0:
            return -1, None, None, None
        return step.value, tm1, tm2, vel

    def snapshot_clear(self):
        """hq_snapshot_clear: wait, then drop every snapshot of the context and its memory."""
        _check(self._lib.hq_snapshot_clear(self._h), self._lib)
        self._snapshots = {}

    @staticmethod
    def _points(ids, phi, who):
        """(ids, phi, nodes per point) of a tracker's description: ids [n] single nodes with phi None, ids and phi [n,8] else."""
        if phi is None:
            return np.ascontiguousarray(np.asarray(ids).reshape(-1), np.int32), None, 1
        ids = np.ascontiguousarray(np.asarray(ids).reshape(-1, 8), np.int32)
        phi = np.ascontiguousarray(np.asarray(phi).reshape(-1, 8), np.float64)
        if len(ids) != len(phi):
            raise HqError("%s: %d rows of ids, %d of phi" % (who, len(ids), len(phi)))
        return ids, phi, 8

    def _tracker_add(self, kind, desc, shape):
        """hq_<kind>_add; `shape` is what the kind's fetch and load size their arrays by."""
        h = ctypes.c_int32(-1)
        _check(getattr(self._lib, "hq_%s_add" % kind)(self._h, ctypes.byref(desc), ctypes.byref(h)), self._lib)
        self._trackers[kind][h.value] = shape
        return h.value

    def _tracker_shape(self, kind, handle):
        if handle not in self._trackers[kind]:
            raise HqError("unknown %s tracker handle %r" % (_TRACKER_KINDS[kind], handle))
        return self._trackers[kind][handle]

    def _tracker_reset(self, kind, handle):
        _check(getattr(self._lib, "hq_%s_reset" % kind)(self._h, ctypes.c_int32(handle)), self._lib)

    def _tracker_clear(self, kind):
        _check(getattr(self._lib, "hq_%s_clear" % kind)(self._h), self._lib)
        self._trackers[kind] = {}

    def peak_add(self, ids, phi=None, rate=1, first_step=0, quantities=HQ_PEAK_VEL):
        """hq_peak_add: a peak-motion tracker.  phi [n,8] with ids [n,8]: points inside elements, as record_add's; phi
        None: ids [n] are single nodes (a surface map).  A sample is folded in at the head of every step s >= first_step
        with s % rate == 0; `quantities` a mask of HQ_PEAK_DISP | VEL | ACC.  Returns its handle."""
        ids, phi, k = self._points(ids, phi, "peak_add")
        d = _PeakDesc(len(ids), k, _ptr(ids), _ptr(phi), int(rate), int(first_step), int(quantities), 0)
        return self._tracker_add("peak", d, (len(ids), bin(int(quantities) & 7).count("1")))

    def peak_fetch(self, handle):
        """hq_peak_fetch: (peaks [npoints, nq, 5] float64, when [npoints, nq, 2] int32, nsamples) -- per quantity of the
        mask max |x|, |y|, |z|, the horizontal and the total SQUARED, and the steps the last two were last raised at (-1:
        never).  Waits for the enqueued steps; the state stays on the device."""
        npoints, nq = self._tracker_shape("peak", handle)
        peaks = np.zeros((npoints, nq, 5))
        when = np.full((npoints, nq, 2), -1, np.int32)
        n = ctypes.c_int64()
        _check(self._lib.hq_peak_fetch(self._h, ctypes.c_int32(handle), _ptr_or_pad(peaks), _ptr_or_pad(when), ctypes.byref(n)), self._lib)
        return peaks, when, int(n.value)

    def peak_load(self, handle, peaks, when, nsamples):
        """hq_peak_load: put back what peak_fetch returned (a run that restarts from a checkpoint)."""
        npoints, nq = self._tracker_shape("peak", handle)
        peaks = np.ascontiguousarray(peaks, np.float64)
        when = np.ascontiguousarray(when, np.int32)
        if peaks.shape != (npoints, nq, 5) or when.shape != (npoints, nq, 2):
            raise HqError("peak_load: the arrays are not those of peak_fetch")
        _check(self._lib.hq_peak_load(self._h, ctypes.c_int32(handle), _ptr_or_pad(peaks), _ptr_or_pad(when),
                                      ctypes.c_int64(int(nsamples))), self._lib)

    def peak_reset(self, handle):
        """hq_peak_reset: peaks 0, when -1, nsamples 0."""
        self._tracker_reset("peak", handle)

    def peak_clear(self):
        """hq_peak_clear: drop every tracker of the context and its device memory."""
        self._tracker_clear("peak")

    def spec_add(self, ids, phi=None, rate=1, first_step=0, periods=(1.0,), damping=0.05):
        """hq_spec_add: a response-spectrum tracker.  Points as peak_add's (phi None: single nodes).  At the head of every
        step s >= first_step with s % rate == 0 the point's acceleration sample drives one damped oscillator per period
        (seconds) and axis, step h = rate dt; the maxima of |x| are SD -- PSV = omega SD, PSA = omega^2 SD are the
        caller's.  Returns its handle."""
        ids, phi, k = self._points(ids, phi, "spec_add")
        periods = np.ascontiguousarray(np.asarray(periods, np.float64).reshape(-1))
        d = _SpecDesc(len(ids), k, _ptr(ids), _ptr(phi), int(rate), int(first_step), len(periods), 0,
                      _ptr(periods) if len(periods) else None, float(damping))
        return self._tracker_add("spec", d, (len(ids), len(periods)))

    def spec_coefficients(self, handle):
        """hq_spec_coefficients: [nperiods, 8] = A11, A12, A21, A22, B11, B12, B21, B22 per period, as the kernel reads them."""
        _, nper = self._tracker_shape("spec", handle)
        coef = np.zeros((nper, 8))
        _check(self._lib.hq_spec_coefficients(self._h, ctypes.c_int32(handle), _ptr(coef)), self._lib)
        return coef

    def spec_fetch(self, handle, osc=True, aprev=True):
        """hq_spec_fetch: (sd [npoints, nperiods, 4], osc [npoints, nperiods, 2, 3] or None, aprev [npoints, 3] or None,
        nsamples) -- per period max |x| per axis and the horizontal resultant SQUARED; the oscillators (x then v) and the
        last sample as they stand.  Waits for the enqueued steps; the state stays on the device."""
        npoints, nper = self._tracker_shape("spec", handle)
        sd = np.zeros((npoints, nper, 4))
        o = np.zeros((npoints, nper, 2, 3)) if osc else None
        a = np.zeros((npoints, 3)) if aprev else None
        n = ctypes.c_int64()
        _check(self._lib.hq_spec_fetch(self._h, ctypes.c_int32(handle), _ptr_or_pad(sd), _ptr_or_pad(o), _ptr_or_pad(a),
                                       ctypes.byref(n)), self._lib)
        return sd, o, a, int(n.value)

    def spec_load(self, handle, sd, osc, aprev, nsamples):
        """hq_spec_load: put back what spec_fetch returned (a run that restarts from a checkpoint)."""
        npoints, nper = self._tracker_shape("spec", handle)
        if sd is None or osc is None or aprev is None:
            raise HqError("spec_load: sd, osc and aprev are all required")
        sd = np.ascontiguousarray(sd, np.float64)
        osc = np.ascontiguousarray(osc, np.float64)
        aprev = np.ascontiguousarray(aprev, np.float64)
        if sd.shape != (npoints, nper, 4) or osc.shape != (npoints, nper, 2, 3) or aprev.shape != (npoints, 3):
            raise HqError("spec_load: the arrays are not those of spec_fetch")
        _check(self._lib.hq_spec_load(self._h, ctypes.c_int32(handle), _ptr_or_pad(sd), _ptr_or_pad(osc), _ptr_or_pad(aprev),
                                      ctypes.c_int64(int(nsamples))), self._lib)

    def spec_reset(self, handle):
        """hq_spec_reset: the oscillators at rest, sd 0, the previous sample 0, nsamples 0."""
        self._tracker_reset("spec", handle)

    def spec_clear(self):
        """hq_spec_clear: drop every spectrum tracker of the context and its device memory."""
        self._tracker_clear("spec")

    def cum_add(self, ids, phi=None, rate=1, first_step=0, quantities=HQ_PEAK_ACC, threshold=0.0, husid_every=0, husid_slots=0):
        """hq_cum_add: a cumulative-intensity tracker (Arias, CAV, energy density, durations).  Points as peak_add's (phi
        None: single nodes).  At the head of every step s >= first_step with s % rate == 0 the sample of every quantity of
        the mask is added into sum |v| and sum v v per axis, and counted where its total exceeds `threshold` (a scalar, or
        one value per quantity of the mask in mask order).  husid_every >= 1: the sums of squares after every
        husid_every-th due sample are kept, husid_slots of them (the Husid curve).  Returns its handle."""
        ids, phi, k = self._points(ids, phi, "cum_add")
        nq = bin(int(quantities) & 7).count("1")
        thr = np.broadcast_to(np.asarray(threshold, np.float64), (nq,)) if np.ndim(threshold) == 0 else np.asarray(threshold, np.float64).reshape(-1)
        if len(thr) != nq:
            raise HqError("cum_add: %d thresholds for %d quantities" % (len(thr), nq))
        d = _CumDesc(len(ids), k, _ptr(ids), _ptr(phi), int(rate), int(first_step), int(quantities), int(husid_every),
                     int(husid_slots), 0, (ctypes.c_double * 3)(*([float(v) for v in thr] + [0.0] * (3 - nq))))
        return self._tracker_add("cum", d, (len(ids), nq, int(husid_slots)))

    def cum_fetch(self, handle, curve=True):
        """hq_cum_fetch: (sums [npoints, nq, 6] float64, span [npoints, nq, 3] int32, curve [nfilled, npoints, nq, 3] or None,
        curve_steps [nfilled] int32, nsamples) -- per quantity of the mask sum |x|, |y|, |z|, sum x x, y y, z z; the first and
        the last step over the threshold (-1: never) and the count of such samples; the sums of squares as they stood behind
        the samples of curve_steps.  Nothing is multiplied by the step h = rate dt: that is the caller's.  Waits for the
        enqueued steps; the state stays on the device."""
        npoints, nq, slots = self._tracker_shape("cum", handle)
        sums = np.zeros((npoints, nq, 6))
        span = np.zeros((npoints, nq, 3), np.int32)
        cv = np.zeros((max(slots, 1), npoints, nq, 3)) if curve else None
        steps = np.zeros(max(slots, 1), np.int32)
        nf, n = ctypes.c_int32(), ctypes.c_int64()
        _check(self._lib.hq_cum_fetch(self._h, ctypes.c_int32(handle), _ptr_or_pad(sums), _ptr_or_pad(span), _ptr_or_pad(cv),
                                      _ptr(steps), ctypes.byref(nf), ctypes.byref(n)), self._lib)
        return sums, span, (cv[:nf.value].copy() if curve else None), steps[:nf.value].copy(), int(n.value)

    def cum_load(self, handle, sums, span, curve, curve_steps, nsamples):
        """hq_cum_load: put back what cum_fetch returned (a run that restarts from a checkpoint)."""
        npoints, nq, _ = self._tracker_shape("cum", handle)
        sums = np.ascontiguousarray(sums, np.float64)
        span = np.ascontiguousarray(span, np.int32)
        steps = np.ascontiguousarray(curve_steps, np.int32).reshape(-1)
        nf = len(steps)
        if nf and curve is None:
            raise HqError("cum_load: curve_steps without a curve")
        cv = np.zeros((0, npoints, nq, 3)) if curve is None else np.ascontiguousarray(curve, np.float64)
        if sums.shape != (npoints, nq, 6) or span.shape != (npoints, nq, 3) or cv.shape != (nf, npoints, nq, 3):
            raise HqError("cum_load: the arrays are not those of cum_fetch")
        _check(self._lib.hq_cum_load(self._h, ctypes.c_int32(handle), _ptr_or_pad(sums), _ptr_or_pad(span), _ptr_or_pad(cv),
                                     _ptr_or_pad(steps), ctypes.c_int32(nf), ctypes.c_int64(int(nsamples))), self._lib)

    def cum_reset(self, handle):
        """hq_cum_reset: sums and counts 0, first / last step -1, no Husid slot filled, nsamples 0."""
        self._tracker_reset("cum", handle)

    def cum_clear(self):
        """hq_cum_clear: drop every cumulative tracker of the context and its device memory."""
        self._tracker_clear("cum")

    def deform_add(self, ids, grad, lame=None, rate=1, first_step=0, quantities=HQ_DEFORM_STRAIN):
        """hq_deform_add: a deformation tracker.  ids [n,8] and grad [n,3,8] as Box.station_gradients returns them; lame
        [n,2] = lambda, mu per point (Box.station_moduli), needed with HQ_DEFORM_STRESS only.  At the head of every step s >=
        first_step with s % rate == 0 the displacement gradient at every point (and, with a rate bit, the velocity's) is
        formed and the strain, strain rate, stress, rotation and rotation rate of the mask are folded into running peaks.
        Returns its handle."""
        ids = np.ascontiguousarray(np.asarray(ids).reshape(-1, 8), np.int32)
        grad = np.ascontiguousarray(np.asarray(grad, np.float64).reshape(-1, 3, 8))
        if len(ids) != len(grad):
            raise HqError("deform_add: %d rows of ids, %d of grad" % (len(ids), len(grad)))
        if lame is not None:
            lame = np.ascontiguousarray(np.asarray(lame, np.float64).reshape(-1, 2))
            if len(lame) != len(ids):
                raise HqError("deform_add: %d rows of ids, %d of lame" % (len(ids), len(lame)))
        q = int(quantities)
        d = _DeformDesc(len(ids), _ptr_or_pad(ids), _ptr_or_pad(grad), _ptr_or_pad(lame), int(rate), int(first_step), q, 0)
        nt, nv = bin(q & 7).count("1"), bin(q & 24).count("1")
        return self._tracker_add("deform", d, (len(ids), 10 * nt + 5 * nv, 2 * (nt + nv)))

    def deform_fetch(self, handle):
        """hq_deform_fetch: (vals [npoints, 10 nt + 5 nv] float64, when [npoints, 2 (nt + nv)] int32, nsamples) -- one block
        per set bit of the mask, in the order of the bits.  A tensor's block (strain, strain rate, stress): max |xx|, |yy|,
        |zz|, |xy|, |yz|, |xz|, max |xx + yy + zz|, max 6 J2, the horizontal engineering shear SQUARED, max |xx + yy|, and in
        `when` the steps 6 J2 and the volumetric measure were last raised at (-1: never).  A vector's block (rotation,
        rotation rate): peak_fetch's five values and two steps, the tilt in the horizontal slot.  Waits for the enqueued
        steps; the state stays on the device."""
        npoints, nvals, nwhen = self._tracker_shape("deform", handle)
        vals = np.zeros((npoints, nvals))
        when = np.full((npoints, nwhen), -1, np.int32)
        n = ctypes.c_int64()
        _check(self._lib.hq_deform_fetch(self._h, ctypes.c_int32(handle), _ptr_or_pad(vals), _ptr_or_pad(when), ctypes.byref(n)), self._lib)
        return vals, when, int(n.value)

    def deform_load(self, handle, vals, when, nsamples):
        """hq_deform_load: put back what deform_fetch returned (a run that restarts from a checkpoint)."""
        npoints, nvals, nwhen = self._tracker_shape("deform", handle)
        vals = np.ascontiguousarray(vals, np.float64)
        when = np.ascontiguousarray(when, np.int32)
        if vals.shape != (npoints, nvals) or when.shape != (npoints, nwhen):
            raise HqError("deform_load: the arrays are not those of deform_fetch")
        _check(self._lib.hq_deform_load(self._h, ctypes.c_int32(handle), _ptr_or_pad(vals), _ptr_or_pad(when),
                                        ctypes.c_int64(int(nsamples))), self._lib)

    def deform_reset(self, handle):
        """hq_deform_reset: values 0, when -1, nsamples 0."""
        self._tracker_reset("deform", handle)

    def deform_clear(self):
        """hq_deform_clear: drop every deformation tracker of the context and its device memory."""
        self._tracker_clear("deform")

    def set_attenuation(self, coef, freq, split=False):
        """hq_attenuation_set: BKT constant-Q attenuation from the ten floats per element coef [E, 10] (edata_t's order:
        a0_shear, a1_shear, b_shear, g0_shear, g1_shear, then the same for kappa) and Param.theFreq.  Scatter variant, double
        library; the memory variables start at 0.  split: hq_attenuation_set_split, the correction pass beside the step of a
        context of the patch variant."""
        coef = np.ascontiguousarray(coef, np.float32)
        if coef.shape != (self.E, 10):
            raise HqError("set_attenuation: coef %r is not [%d, 10]" % (coef.shape, self.E))
        d = _AttenuationDesc(_ptr(coef), float(freq))
        fn = self._lib.hq_attenuation_set_split if split else self._lib.hq_attenuation_set
        _check(fn(self._h, ctypes.byref(d)), self._lib)

    def attenuation_split(self):
        """Is the context's attenuation the split form (hq_attenuation_info's out[3])?"""
        out = (ctypes.c_int64 * 4)()
        _check(self._lib.hq_attenuation_info(self._h, out), self._lib)
        return bool(out[3])

    def attenuation_info(self):
        """hq_attenuation_info -> dict(classes, slots, device_bytes); all 0 without attenuation."""
        out = (ctypes.c_int64 * 4)()
        _check(self._lib.hq_attenuation_info(self._h, out), self._lib)
        return dict(classes=int(out[0]), slots=int(out[1]), device_bytes=int(out[2]))

    def attenuation_state(self):
        """hq_attenuation_fetch -> (shear1, shear2, kappa1, kappa2), each [E * 8, 3] in the reference's layout
        (cindex = eindex * 8 + i)."""
        out = [np.empty((self.E * 8, 3)) for _ in range(4)]
        _check(self._lib.hq_attenuation_fetch(self._h, *[_ptr(a) for a in out]), self._lib)
        return tuple(out)

    def load_attenuation_state(self, shear1, shear2, kappa1, kappa2):
        """hq_attenuation_load: four arrays [E * 8, 3] as attenuation_state returns them; corners that share a (node, class)
        slot must agree bit for bit."""
        arrs = [np.ascontiguousarray(a, np.float64) for a in (shear1, shear2, kappa1, kappa2)]
        for a in arrs:
            if a.shape != (self.E * 8, 3):
                raise HqError("load_attenuation_state: an array of shape %r is not [%d, 3]" % (a.shape, self.E * 8))
        _check(self._lib.hq_attenuation_load(self._h, *[_ptr(a) for a in arrs]), self._lib)

    def clear_attenuation(self):
        """hq_attenuation_clear: back to the Rayleigh step of the context's eTable."""
        _check(self._lib.hq_attenuation_clear(self._h), self._lib)

    def set_nonlinear(self, model, elems, cons):
        """hq_nonlinear_set: rate-independent plasticity (HQ_NL_VONMISES, HQ_NL_DRUCKERPRAGER) at the quadrature points of the
        elements `elems` [n] (the caller's numbering, strictly ascending) with cons [n, 6] = h, mu, lambda, alpha, k, hardening
        modulus (host.nonlinear_constants): a correction pass beside the step of a context of the patch variant, double
        library.  The plastic strains start at 0."""
        d = _nonlinear_desc(model, elems, cons, "set_nonlinear")
        _check(self._lib.hq_nonlinear_set(self._h, ctypes.byref(d)), self._lib)

    def nonlinear_info(self):
        """hq_nonlinear_info -> dict(elements, touched_nodes, device_bytes); all 0 without."""
        out = (ctypes.c_int64 * 4)()
        _check(self._lib.hq_nonlinear_info(self._h, out), self._lib)
        return dict(elements=int(out[0]), touched_nodes=int(out[1]), device_bytes=int(out[2]))

    def nonlinear_fetch(self):
        """hq_nonlinear_fetch -> (pstrain [n, 8, 6], ep [n, 8]): the caller's element order, the reference's quadrature order
        and tensor order (xx yy zz xy yz xz)."""
        n = self.nonlinear_info()["elements"]
        pstrain, ep = np.zeros((n, 8, 6)), np.zeros((n, 8))
        _check(self._lib.hq_nonlinear_fetch(self._h, _ptr_or_pad(pstrain), _ptr_or_pad(ep)), self._lib)
        return pstrain, ep

    def nonlinear_load(self, pstrain, ep):
        """hq_nonlinear_load: the two arrays as nonlinear_fetch returns them."""
        n = self.nonlinear_info()["elements"]
        pstrain, ep = np.ascontiguousarray(pstrain, np.float64), np.ascontiguousarray(ep, np.float64)
        if pstrain.shape != (n, 8, 6) or ep.shape != (n, 8):
            raise HqError("nonlinear_load: arrays of shape %r, %r are not [%d, 8, 6], [%d, 8]" % (pstrain.shape, ep.shape, n, n))
        _check(self._lib.hq_nonlinear_load(self._h, _ptr_or_pad(pstrain), _ptr_or_pad(ep)), self._lib)

    def clear_nonlinear(self):
        """hq_nonlinear_clear: the context steps as it did before; the added bytes go."""
        _check(self._lib.hq_nonlinear_clear(self._h), self._lib)

    def phase_force(self):
        _check(self._lib.hq_phase_force(self._h), self._lib)

    def phase_update(self):
        _check(self._lib.hq_phase_update(self._h), self._lib)

    def download_force(self):
        f = np.empty((self.N, 3))
        _check(self._lib.hq_download_force(self._h, _ptr(f)), self._lib)
        return f


PLAN_REPORT = ("patches", "lattice_patches", "pairs", "distinct_row_blocks", "gather_passes", "gather_instructions",
               "lattice_gather_passes", "faults")


def plan_check(desc):
    """hq_plan_check on a filled _Desc: the planner's host-only self-check (no device needed)."""
    rep = (ctypes.c_int64 * 8)()
    _check(load_library().hq_plan_check(ctypes.byref(desc), rep))
    return dict(zip(PLAN_REPORT, [int(v) for v in rep]))


STENCIL_PLAN_REPORT = ("patches", "tables", "full_lattices", "boundary_nodes", "corners_checked", "faults")


def stencil_plan_check(desc):
    """hq_stencil_plan_check on a filled _Desc: the stencil kernel's tables against the mesh (no device needed)."""
    rep = (ctypes.c_int64 * 6)()
    _check(load_library().hq_stencil_plan_check(ctypes.byref(desc), rep))
    return dict(zip(STENCIL_PLAN_REPORT, [int(v) for v in rep]))


BRICK_PLAN_REPORT = ("brick_nodes", "columns", "units", "units_one_nt_row", "het_units", "neighbours_checked",
                     "patch_nodes", "faults", "ragged_units", "ragged_nodes", "ragged_het_units", "ragged_het_nodes", "packed_units",
                     "min_unit_nx", "min_unit_ny", "min_unit_np", "ragged_min_plane_nodes", "units_one_plane_both_faces")


def brick_plan_check(desc):
    """hq_brick_plan_check on a filled _Desc: the brick planner against the mesh's connectivity (no device needed)."""
    rep = (ctypes.c_int64 * len(BRICK_PLAN_REPORT))()
    _check(load_library().hq_brick_plan_check_n(ctypes.byref(desc), rep, ctypes.c_int32(len(BRICK_PLAN_REPORT))))
    return dict(zip(BRICK_PLAN_REPORT, [int(v) for v in rep]))


ATTENUATION_PLAN_REPORT = ("classes", "slots", "device_bytes", "faults")


def attenuation_plan_check(desc, coef):
    """hq_attenuation_plan_check on a filled _Desc and coef [E, 10] float32: the slot plan, host only (no device needed)."""
    coef = np.ascontiguousarray(coef, np.float32)
    if coef.shape != (desc.lenum, 10):
        raise HqError("attenuation_plan_check: coef %r is not [%d, 10]" % (coef.shape, desc.lenum))
    rep = (ctypes.c_int64 * 4)()
    _check(load_library().hq_attenuation_plan_check(ctypes.byref(desc), _ptr(coef), rep))
    return dict(zip(ATTENUATION_PLAN_REPORT, [int(v) for v in rep]))


def attenuation_split_plan_check(desc, coef):
    """hq_attenuation_split_plan_check on a filled _Desc and coef [E, 10] float32: slot plan, node -> (element, corner) table and
    hanging-node lists of a split context, host only (no device needed)."""
    coef = np.ascontiguousarray(coef, np.float32)
    if coef.shape != (desc.lenum, 10):
        raise HqError("attenuation_split_plan_check: coef %r is not [%d, 10]" % (coef.shape, desc.lenum))
    rep = (ctypes.c_int64 * 4)()
    _check(load_library().hq_attenuation_split_plan_check(ctypes.byref(desc), _ptr(coef), rep))
    return dict(zip(ATTENUATION_PLAN_REPORT, [int(v) for v in rep]))


def attenuation_split_plan_tables(desc):
    """hq_attenuation_split_plan_tables -> (epos [E], nptr [N + 1], nent [8 E], sd [H, 3]) int32, in the numbering hq_create
    gives desc."""
    lib = load_library()
    counts = (ctypes.c_int64 * 3)()
    _check(lib.hq_attenuation_split_plan_tables(ctypes.byref(desc), None, None, None, None, counts))
    epos = np.zeros(desc.lenum, np.int32)
    nptr, nent, sd = np.zeros(counts[0], np.int32), np.zeros(counts[1], np.int32), np.zeros((counts[2], 3), np.int32)
    _check(lib.hq_attenuation_split_plan_tables(ctypes.byref(desc), _ptr(epos), _ptr(nptr), _ptr(nent), _ptr(sd), counts))
    return epos, nptr, nent, sd


def attenuation_split_table_faults(desc, epos, nptr, nent, sd):
    """hq_attenuation_split_table_faults: the faults the split plan check counts in the given tables."""
    epos, nptr, nent = [np.ascontiguousarray(a, np.int32) for a in (epos, nptr, nent)]
    sd = np.ascontiguousarray(sd, np.int32).reshape(-1, 3)
    if len(nptr) != desc.nharbored + 1 or len(nent) != 8 * desc.lenum or len(epos) != desc.lenum:
        raise HqError("attenuation_split_table_faults: tables of %d, %d entries for %d nodes, %d elements" % (len(nptr), len(nent), desc.nharbored, desc.lenum))
    faults = ctypes.c_int64()
    _check(load_library().hq_attenuation_split_table_faults(ctypes.byref(desc), _ptr(epos), _ptr(nptr), _ptr(nent), _ptr(sd) if len(sd) else None,
                                                            ctypes.c_int64(len(sd)), ctypes.byref(faults)))
    return int(faults.value)


NONLINEAR_PLAN_REPORT = ("elements", "touched_nodes", "device_bytes", "faults")


def nonlinear_plan_check(desc, model, elems, cons):
    """hq_nonlinear_plan_check on a filled _Desc: the touched-node list and the node -> (element, corner) table of a nonlinear
    context, host only (no device needed)."""
    nl = _nonlinear_desc(model, elems, cons, "nonlinear_plan_check")
    rep = (ctypes.c_int64 * 4)()
    _check(load_library().hq_nonlinear_plan_check(ctypes.byref(desc), ctypes.byref(nl), rep))
    return dict(zip(NONLINEAR_PLAN_REPORT, [int(v) for v in rep]))


def nonlinear_plan_tables(desc, model, elems, cons):
    """hq_nonlinear_plan_tables -> (tnode [T], epos [n], nptr [T + 1], nent [8 n], sd [H, 3]) int32: the touched nodes in the
    numbering hq_create gives desc, the tables on touched-node indices."""
    lib = load_library()
    nl = _nonlinear_desc(model, elems, cons, "nonlinear_plan_tables")
    counts = (ctypes.c_int64 * 4)()
    _check(lib.hq_nonlinear_plan_tables(ctypes.byref(desc), ctypes.byref(nl), None, None, None, None, None, counts))
    tnode, epos = np.zeros(counts[0], np.int32), np.zeros(nl.nelems, np.int32)
    nptr, nent, sd = np.zeros(counts[1], np.int32), np.zeros(counts[2], np.int32), np.zeros((counts[3], 3), np.int32)
    _check(lib.hq_nonlinear_plan_tables(ctypes.byref(desc), ctypes.byref(nl), _ptr_or_pad(tnode), _ptr_or_pad(epos), _ptr_or_pad(nptr),
                                        _ptr_or_pad(nent), _ptr_or_pad(sd), counts))
    return tnode, epos, nptr, nent, sd


def nonlinear_table_faults(desc, model, elems, cons, tnode, epos, nptr, nent, sd):
    """hq_nonlinear_table_faults: the faults the nonlinear plan check counts in the given tables."""
    nl = _nonlinear_desc(model, elems, cons, "nonlinear_table_faults")
    tnode, epos, nptr, nent = [np.ascontiguousarray(a, np.int32) for a in (tnode, epos, nptr, nent)]
    sd = np.ascontiguousarray(sd, np.int32).reshape(-1, 3)
    if len(nptr) != len(tnode) + 1 or len(nent) != 8 * nl.nelems or len(epos) != nl.nelems:
        raise HqError("nonlinear_table_faults: tables of %d, %d entries for %d nodes, %d elements" % (len(nptr), len(nent), len(tnode), nl.nelems))
    faults = ctypes.c_int64()
    _check(load_library().hq_nonlinear_table_faults(ctypes.byref(desc), ctypes.byref(nl), _ptr(tnode), _ptr(epos), _ptr(nptr), _ptr(nent),
                                                    _ptr(sd) if len(sd) else None, ctypes.c_int64(len(sd)), ctypes.byref(faults)))
    return int(faults.value)


def comm_unique_id():
    buf = (ctypes.c_char * 128)()
    _check(load_library().hq_comm_unique_id(buf))
    return bytes(buf)


def group_link(solvers):
    """hq_group_link: solvers[i] must hold rank i of len(solvers)."""
    arr = (ctypes.c_void_p * len(solvers))(*[s._h for s in solvers])
    lib = solvers[0]._lib                       # (the group's library: libhq_solver.so or its _f32 build)
    _check(lib.hq_group_link(arr, ctypes.c_int32(len(solvers))), lib)


def group_run(solvers, nsteps):
    arr = (ctypes.c_void_p * len(solvers))(*[s._h for s in solvers])
    lib = solvers[0]._lib
    _check(lib.hq_group_run(arr, ctypes.c_int32(len(solvers)), ctypes.c_int32(nsteps)), lib)
    for s in solvers:
        s.sync()
