/*
 * hq_solver.h -- C-ABI of the MI355X (gfx950) explicit time-stepping engine.
 *
 * Drop-in boundary for the hot path of CMU-Quake/hercules quake/forward
 * (SURVEY.md s8b).  The reference has no plugin registry: the seam is a set
 * of C functions called from solver_run() (psolve.c:4241-4324) that work on
 * the caller-owned plain arrays of mesh_t (octor.h:166-179) and mysolver_t
 * (psolve.h:295-312).  Each entry point below names the reference function(s)
 * it replaces.  Plain pointers and sizes only; no HIP, torch or C++ types.
 *
 * Ownership : the caller owns every host buffer it passes; the context owns
 *             all device memory, streams and events.
 * Errors    : every call returns HQ_OK (0) or a negative hq_status; nothing
 *             aborts the process (the reference MPI_Abort()s, util.h:128).
 * Threading : one context per GPU / mesh partition; calls on one context must
 *             not overlap.  hq_run() only enqueues work; hq_sync(), hq_gather(),
 *             hq_download() wait for it.
 */
#ifndef HQ_SOLVER_H
#define HQ_SOLVER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HQ_API __attribute__((visibility("default")))

typedef struct hq_ctx hq_ctx;

typedef enum {
    HQ_OK            =  0,
    HQ_ERR_ARG       = -1,   /* bad argument / inconsistent description     */
    HQ_ERR_NOMEM     = -2,   /* host or device allocation failed            */
    HQ_ERR_DEVICE    = -3,   /* HIP runtime error (see hq_last_error)       */
    HQ_ERR_NODEVICE  = -4,   /* no gfx950 device / kernel image not loadable */
    HQ_ERR_COMM      = -5,   /* RCCL error                                  */
    HQ_ERR_STATE     = -6    /* call not valid in the context's state       */
} hq_status;

/* Element-kernel variants (hq_desc.variant). */
enum {
    HQ_VARIANT_AUTO    = 0,  /* = PATCH                                                        */
    HQ_VARIANT_SCATTER = 1,  /* element kernel + fp64 atomics, node kernel                     */
    HQ_VARIANT_PATCH   = 2   /* owner-computes patches, one fused kernel (+ interface kernels  */
                             /* on partitions); anchors of hanging nodes must be anchored      */
};

/*
 * One neighbour's shared-node list: messenger_t (psolve.h:230-249).
 * `mapping` holds local node ids in the order both sides agreed on
 * (ascending global id in the reference, psolve.c:4704-4863).
 */
typedef struct {
    int32_t        procid;
    int32_t        nodecount;
    const int32_t* mapping;
} hq_messenger;

/*
 * solver_float (psolve.h:60-64): the type of the caller's tm1 / tm2 arrays and n_t rows.  The reference's
 * -DSINGLE_PRECISION_SOLVER makes it float; the library built with -DHQ_SINGLE_PRECISION_SOLVER
 * (libhq_solver_f32.so, same sources) then takes and returns floats at these places and keeps the device-resident
 * state in floats (36 instead of 72 compulsory bytes per node and step); e_t, the source table and every sum inside
 * a kernel stay double, as the reference's own locals do.  A client compiles with the same macro and checks
 * hq_real_bytes() == sizeof(hq_real).  A separately named dtype with its own oracle build and tolerance
 * (tests/test_gpu_single_precision.py); never the headline.
 */
#ifdef HQ_SINGLE_PRECISION_SOLVER
typedef float hq_real;
#else
typedef double hq_real;
#endif

/*
 * One communication schedule: schedule_t (psolve.h:255-274).
 * c-list: ranks that OWN nodes I harbor -- I send them force contributions and
 *         receive displacements from them.
 * s-list: ranks that harbor nodes I OWN -- the reverse.
 */
typedef struct {
    int32_t             c_count;
    const hq_messenger* first_c;
    int32_t             s_count;
    const hq_messenger* first_s;
} hq_schedule;

/*
 * Everything solver_run() reads, as plain arrays.
 */
typedef struct {
    /* mesh_t */
    int32_t        lenum;        /* elements on this partition               */
    int32_t        nharbored;    /* nodes harbored (owned + shared copies)   */
    int32_t        ldnnum;       /* dangling (hanging) nodes owned           */
    const int32_t* lnid;         /* [lenum][8]  elem_t.lnid (octor.h:110-115) */
    const int32_t* node_xyz;     /* [nharbored][3] node_t.x,y,z in ticks (octor.h:133-147); optional
                                    (NULL): only used to place patch cuts on octree cubes */
    /* dnodeTable (octor.h:153-158) as CSR: node dn_ldnid[k] hangs on
     * anchors dn_lanid[dn_ptr[k] .. dn_ptr[k+1])  (deps = 2 or 4)            */
    const int32_t* dn_ldnid;
    const int32_t* dn_ptr;
    const int32_t* dn_lanid;
    /* mysolver_t */
    const double*  eTable;       /* [lenum][4]      e_t  c1..c4 (psolve.h:196-198) */
    const hq_real* nTable;       /* [nharbored][7]  n_t  (psolve.h:210-214)   */
    const hq_real* tm1;          /* [nharbored][3]  u(t)      or NULL = 0     */
    const hq_real* tm2;          /* [nharbored][3]  u(t-dt)   or NULL = 0     */
    hq_schedule    an_sched;     /* anchored-node schedule  (mysolver_t.an_sched) */
    hq_schedule    dn_sched;     /* dangling-node schedule  (mysolver_t.dn_sched) */
    /* Param */
    double         deltaT;       /* Param.theDeltaT (source force = F * dt^2) */
    int32_t        rank, nranks; /* Global.myID, Global.theGroupSize          */
    int32_t        variant;      /* HQ_VARIANT_*                              */
    int32_t        reserved;
    const int64_t* node_gnid;    /* [nharbored] node_t.gnid (octor.h:133-147); optional (NULL): only used by
                                    HQ_DEBUG_HALO, which falls back to a mix of node_xyz */
    /* ABI 5.  What solver_init built eTable FROM, optional (NULL / 0): edata_t of every element as solver_init left it
     * (psolve.h:95-97; mu_and_lambda may have rewritten Vp, psolve.c:3253-3263) and the constants it combined them with.
     * Where given, the kernel for meshes whose material differs from element to element (hq_k_brick_het) keeps 12 bytes per
     * element -- rho, Vs, Vp -- instead of the 24 of (c1, c2, beta), and rebuilds the caller's very doubles on the fly:
     * hq_create checks every element bit for bit against eTable first and keeps the 24 bytes wherever one differs.
     * The n_t rows of such units travel as {mass_simple, mass_simple - mass_minusaM}: mass_minusaM comes out EXACTLY,
     * mass2_minusaM as 2 m0 - (m0 - m1), equal to the caller's to 1e-15 relative (checked per node; a node that misses keeps
     * its unit unpacked) -- NOT bit for bit: the reference sums it in another order (psolve.c:3436-3471).  The difference is
     * of the class of the element sums' own order; tests/test_gpu_fullsize.py pins 10 000 steps against the unpacked form. */
    const float*  edata;         /* [lenum][4] edgesize (m), Vp, Vs, rho                                             */
    double mat_bbase;            /* Global.theBBase (compute_setab, psolve.c:5813-5876)                              */
    double mat_threshold_damping;/* Param.theThresholdDamping                                                        */
    double mat_threshold_vpvs;   /* Param.theThresholdVpVs                                                           */
} hq_desc;

typedef struct {
    int32_t variant;             /* variant actually built                    */
    int32_t npatches;            /* patch variant: number of patches          */
    int64_t patch_pairs;         /* patch variant: sum of per-patch elements  */
    int64_t device_bytes;        /* device memory owned by the context        */
    int32_t step;                /* next step to be executed                  */
    int32_t nranks;
    int32_t lattice_patches;     /* patch variant: patches with rows and lanes on one lattice (conflict-free LDS) */
    int32_t stencil_patches;     /* patch variant: patches stepped by hq_k_patch_stencil                          */
    int32_t ragged_patches;      /* patch variant: of the stencil patches, the lattice SUBSETS (faces, far-face cubes) */
    int32_t brick_units;         /* patch variant: workgroup units of hq_k_brick (tile column x planes)          */
    int64_t brick_nodes;         /* patch variant: nodes stepped by hq_k_brick (the rest belongs to the patches)  */
    int32_t brick_units_pernode; /* of brick_units: uniform coefficients, n_t rows of their own (hq_k_brick<true>)  */
    int32_t brick_units_het;     /* of brick_units: per-element coefficients (hq_k_brick_het)                      */
    int64_t pcie_h2d_bytes;      /* bytes the entry points moved host -> device since hq_create returned (source   */
    int64_t pcie_d2h_bytes;      /* windows, gather ids, uploads, host-staged halos) and device -> host (gathers,   */
                                 /* downloads, host-staged halos): what a run costs on PCIe between outputs         */
    int32_t transport;           /* 0 none, 1 RCCL, 2 IPC, 3 host-staged, 4 in-process group, 5 loopback (diagnostic)  */
    int32_t ipc_arena_coarse;    /* IPC: 1 if the receive arena had to be coarse-grained memory (ranks of one device only) */
    int32_t ipc_arena_kind;      /* IPC: 0 fine-grained, 1 uncached, 2 coarse-grained device memory                        */
    int32_t debug_halo;          /* 1: every halo record is checked on receipt (HQ_DEBUG_HALO / hq_options.debug_halo)     */
    int32_t brick_units_packed;  /* of brick_units_het: coefficients as three floats, n_t rows as two doubles (hq_desc.edata) */
    int32_t brick_units_ragged;  /* of the units with one n_t row: partly filled tiles (HQ_BK_RAGGED, hq_options.brick_ragged) */
    /* ABI 6 */
    int32_t brick_stream;        /* 1: the shell's patches run on the compute stream BESIDE the bricks, which have a stream of their own */
    int32_t brick_units_ragged_het; /* of brick_units_het: partly filled tiles (hq_k_brick_het<., RAGGED>, hq_options.brick_ragged_het) */
    /* Where a step's device time goes -- the library's share of the reference's per-phase report (print_timing_stat,
     * psolve.c:6041-6266: "Compute addforces e", "... schedule send data", ...), from HIP events, averaged over
     * `timed_steps` steps: every step of a context with hq_options.phase_timing = 1, every fourth step of an hq_run_timed batch.
     * microseconds per step; the phases overlap, so they do not add up to t_step_us. */
    int64_t timed_steps;
    double  t_step_us;           /* first kernel's start -> last kernel's end (compute streams and exchange chain)       */
    double  t_shell_us;          /* patch launches: the shell behind the bricks, or every node where there are no bricks
                                    (element force + nodal update + hanging nodes inside patches)                         */
    double  t_interior_us;       /* brick launches (element force + nodal update of the bulk)                            */
    double  t_chain_us;          /* exchange chain, its release (interface patches done) -> displacements shared: pack,
                                    transport, interface update, unpack, compute_adjust between ranks -- waits for the
                                    neighbours' records included                                                          */
    double  t_chain_exposed_us;  /* of it, what ran AFTER the step's compute kernels had ended (not hidden)                */
} hq_info;

/* Number of gfx950 devices visible (0 if none / no HIP runtime). */
HQ_API int hq_device_count(void);

/* Text of the last error on this thread ("" if none). */
HQ_API const char* hq_last_error(void);

/*
 * Build the device-resident solver state.
 * Replaces: the calloc()s of solver_init (psolve.c:3317-3325) and
 * stiffness_init (stiffness.c:101-105); consumes the eTable/nTable that
 * solver_init computed (psolve.c:3360-3473) and the schedules of
 * schedule_build (psolve.c:4704-4863).
 */
HQ_API int hq_create(const hq_desc* desc, int device, hq_ctx** out);

/*
 * Typed options (ABI 5).  The reference steers its solver through one explicit parameter struct (Param, psolve.c:193-284);
 * this is the library's: everything that selects kernels, plans or transports, per CONTEXT -- two contexts of one process
 * may differ, and nothing depends on the environment unless the caller wants it to.  hq_options_init fills every field
 * with "library default" (-1); hq_create_opts(desc, device, NULL, &ctx) == hq_create(desc, device, &ctx).
 * The environment: an HQ_* variable of a field's name overrides the field ONLY where the caller allows it --
 * hq_options.allow_env = 1, or allow_env = -1 in a process that sets HQ_ALLOW_ENV=1 (experiments, profiles/tools, the
 * test suite); a host program that passes allow_env = 0 cannot be steered by a stray variable.  Every setting is
 * resolved ONCE, at hq_create_opts; hq_get_options returns exactly that: what the context runs with (switches as 0 / 1,
 * -1 where the library's default applies).
 * `size` = sizeof(hq_options) of the caller: a newer library treats the fields an older client does not know as -1.
 */
typedef struct {
    uint64_t size;
    /* which kernels */
    int32_t no_bricks;           /* HQ_NO_BRICKS          1: no z-marching brick kernels, patches everywhere             */
    int32_t brick_cz;            /* HQ_BRICK_CZ           planes per brick unit (default: 32, shorter on small meshes)   */
    int32_t brick_minz;          /* HQ_BRICK_MINZ         shortest run of planes worth a tile column (4)                 */
    int32_t brick_minnodes;      /* HQ_BRICK_MINNODES     fewest nodes worth a tile column (512)                         */
    int32_t brick_no_het;        /* HQ_BRICK_NO_HET       1: no per-element-coefficient brick units (hq_k_brick_het)     */
    int32_t brick_no_ntsame;     /* HQ_BRICK_NO_NTSAME    1: n_t rows per node even where a unit shares one              */
    int32_t brick_by_component;  /* HQ_BRICK_BY_COMPONENT 1 / 0: the 100-register / 118-register form of hq_k_brick
                                                          (default: 100 on contexts with a transport)                   */
    int32_t brick_stream;        /* HQ_BRICK_STREAM       1: bricks on a stream of their own beside the patches          */
    int32_t brick_no_faces;      /* HQ_BRICK_NO_FACES     1: the domain's z faces stay with the patches instead of being stepped as
                                                          the first / last plane of the tile columns under them           */
    int32_t brick_half_tiles;    /* HQ_BRICK_HALF_TILES   (only with brick_ragged = 0) 0: no second planner round with 32-wide full tiles   */
    int32_t brick_no_pack;       /* HQ_BRICK_NO_PACK      1: per-element coefficients as 24-byte (c1, c2, beta) even where
                                                          hq_desc.edata would let them travel as 12 bytes                */
    int32_t patch_pipe;          /* HQ_PATCH_PIPE         6 hq_k_patch_seed (default), 4 hq_k_patch_pers, 0 hq_k_patch_step */
    int32_t patch_threads;       /* HQ_PATCH_THREADS      workgroup size of the patch kernels (512)                      */
    int32_t patch_pmax;          /* HQ_PATCH_PMAX         owned nodes per patch (768)                                    */
    int32_t patch_pmerge;        /* HQ_PATCH_PMERGE       neighbouring cubes are merged up to this (512)                 */
    int32_t patch_psplit;        /* HQ_PATCH_PSPLIT       a cube with more owned nodes is halved (pmax)                  */
    int32_t patch_nlmax;         /* HQ_PATCH_NLMAX        owned + halo nodes staged in LDS (1024)                        */
    int32_t patch_vmax;          /* HQ_PATCH_VMAX         extra accumulators for hanging nodes (set by the planner)      */
    int32_t patch_ragged;        /* HQ_PATCH_RAGGED       lattice-subset patches: 0 element form, 1 stencil form, 2 stencil
                                                          form except on the partition interface                        */
    int32_t patch_no_lattice;    /* HQ_PATCH_NO_LATTICE   1: no lattice patches                                          */
    int32_t patch_no_stencil;    /* HQ_PATCH_NO_STENCIL   1: lattice patches through the element kernels                 */
    int32_t patch_no_uniform;    /* HQ_PATCH_NO_UNIFORM   1: per-element coefficients even in uniform patches            */
    int32_t patch_no_iso;        /* HQ_PATCH_NO_ISO       1: 7-double n_t rows everywhere                                */
    int32_t patch_no_ntsame;     /* HQ_PATCH_NO_NTSAME    1: n_t rows per node even where a patch shares one             */
    int32_t patch_no_dedup;      /* HQ_PATCH_NO_DEDUP     1: every patch keeps its own connectivity rows                 */
    int32_t patch_wform;         /* HQ_PATCH_WFORM        0: hq_k_patch_pers keeps u1, u2 instead of w in LDS            */
    int32_t patch_merge_rounds;  /* HQ_PATCH_MERGE_ROUNDS one patch launch where the shell is at most this many rounds (1) */
    /* the exchange chain */
    int32_t overlap;             /* HQ_OVERLAP            1 / 0: the chain on its own stream beside the interior kernels
                                                          (default: yes between processes / GPUs, no inside one process) */
    int32_t no_overlap;          /* HQ_NO_OVERLAP         1: never create the exchange stream                            */
    int32_t reserve_cus;         /* HQ_RESERVE_CUS        CUs the interior launch leaves to the chain (8)                */
    int32_t cu_mask;             /* HQ_CU_MASK            1: compute stream with a CU mask that leaves reserve_cus free  */
    int32_t no_fused_share;      /* HQ_NO_FUSED_SHARE     1: the displacement sharing packed by its own kernel           */
    int32_t group_copies;        /* HQ_GROUP_COPIES       1: in-process groups exchange through peer copies              */
    int32_t debug_halo;          /* HQ_DEBUG_HALO         1: every halo record checked on receipt (-DDEBUG, psolve.c:5002-5007) */
    /* the IPC transport */
    int32_t ipc_arena;           /* HQ_IPC_ARENA          0 fine-grained, 1 uncached, 2 coarse-grained; default: first that exports */
    double  ipc_timeout_ms;      /* HQ_IPC_TIMEOUT_MS     a wait for a neighbour's records gives up after this (20 000)  */
    double  loopback_delay_us;   /* HQ_LOOPBACK_DELAY_US  diagnostic: loopback flags raised this late                    */
    /* messages */
    int32_t verbose;             /* HQ_PATCH_VERBOSE      1: where hq_create's time goes; 2: the brick planner's too     */
    int32_t quiet;               /* HQ_QUIET              1: no advice on stderr                                         */
    /* (added behind the others) */
    int32_t brick_ragged;        /* HQ_BRICK_RAGGED       0: no partly filled tile columns beside level interfaces and material
                                                          boundaries (the second planner round is then brick_half_tiles')    */
    int32_t brick_ragged_minfill;/* HQ_BRICK_RAGGED_MINFILL fewest nodes a plane of such a column owns, of 512 (128)        */
    /* (ABI 6) */
    int32_t allow_env;           /* 1: HQ_* environment variables override the fields above; 0: the environment is ignored;
                                    -1 (default): honoured only in a process that sets HQ_ALLOW_ENV=1 (experiments, tests) */
    int32_t brick_ragged_het;    /* HQ_BRICK_RAGGED_HET   0: no partly filled tiles of the per-element kernel (hq_k_brick_het<., RAGGED>):
                                                          beside level interfaces of a mesh whose material differs from element to
                                                          element the nodes then stay with the patches                       */
    int32_t reserved0;
    int32_t phase_timing;        /* HQ_PHASE_TIMING       1: every step records where its device time goes (six events per
                                                          step; hq_info.t_*_us) -- the library's share of print_timing_stat
                                                          (psolve.c:6041-6266); hq_run_timed batches always do          */
} hq_options;

HQ_API void hq_options_init(hq_options* opts, uint64_t size);
HQ_API int  hq_create_opts(const hq_desc* desc, int device, const hq_options* opts, hq_ctx** out);
/* what the context runs with (resolved at hq_create_opts); writes min(size, sizeof) bytes */
HQ_API int  hq_get_options(hq_ctx* ctx, hq_options* out, uint64_t size);

/* solver_delete (psolve.c:3627-3649). */
HQ_API int hq_destroy(hq_ctx* ctx);

/*
 * hq_info carries no size field of its own, so the call does: hq_get_info_sized writes min(size, sizeof(hq_info))
 * bytes, and the hq_get_info() of this header passes the caller's own sizeof -- a client compiled against an older
 * (shorter) hq_info is never written past its struct, a newer one gets what this library knows and zeros behind.
 * The exported SYMBOL hq_get_info is kept for binaries built against the headers that had no hq_get_info_sized; the
 * last of those ended its struct with brick_nodes, so the symbol writes those 56 bytes and never more.
 * hq_abi_version() == HQ_ABI_VERSION is the check a separately compiled client makes at start-up.
 */
#define HQ_ABI_VERSION 6
HQ_API int hq_abi_version(void);
/* sizeof(hq_real) of the library that is loaded: 8 (libhq_solver.so), 4 (libhq_solver_f32.so) */
HQ_API int hq_real_bytes(void);
HQ_API int hq_get_info_sized(hq_ctx* ctx, hq_info* info, uint64_t size);
HQ_API int hq_get_info(hq_ctx* ctx, hq_info* info);
#ifndef HQ_SOLVER_IMPLEMENTATION
#define hq_get_info(ctx, info) hq_get_info_sized((ctx), (info), (uint64_t)sizeof(hq_info))
#endif

/*
 * Multi-GPU: one RCCL communicator over the ranks that hold the partitions.
 * Rank 0 obtains a 128-byte id, the host code broadcasts it (MPI_Bcast in the
 * reference's world), every rank calls hq_comm_init.
 * Replaces: solver_run_init_comm / schedule_prepare (psolve.c:3785-3808).
 */
HQ_API int hq_comm_unique_id(void* id128);
HQ_API int hq_comm_init(hq_ctx* ctx, const void* id128);
/* Diagnostic: one grouped ncclRecv + ncclSend of `count` doubles from this rank to itself, through
 * the entry points and on the stream the halo exchange uses, checked on the host.  Lets a
 * single-GPU box exercise the RCCL binding (a communicator of one rank is enough). */
HQ_API int hq_comm_selftest(hq_ctx* ctx, int32_t count);

/*
 * Host-staged transport: the halo records travel through pinned host memory and the CALLER's transport -- in the
 * reference's world the MPI_Irecv / MPI_Isend / MPI_Waitall of schedule_senddata (psolve.c:5013-5033) on
 * comm_solver -- for systems without RCCL between the ranks' GPUs, or several ranks on one GPU.  At each of the (up
 * to four) exchanges of a step the engine packs on the device, copies the records to the host and calls
 * `fn(user, nrecv, recv_peer, recv_count, recv_buf, nsend, send_peer, send_count, send_buf, tag)`: counts in
 * doubles, one entry per neighbour with records, `tag` = 0..3 names the exchange (anchored-node contribution /
 * sharing, dangling-node contribution / sharing); `fn` must have received everything when it returns 0.
 * The exchange chain runs on its own stream as with RCCL: only that stream is waited for.
 */
typedef int (*hq_host_exchange_fn)(void* user, int32_t nrecv, const int32_t* recv_peer, const int64_t* recv_count,
                                   double* const* recv_buf, int32_t nsend, const int32_t* send_peer,
                                   const int64_t* send_count, const double* const* send_buf, int32_t tag);
HQ_API int hq_comm_init_host(hq_ctx* ctx, hq_host_exchange_fn fn, void* user);

/*
 * Device-to-device transport between PROCESSES of one node without RCCL: direct peer stores over xGMI (or inside one
 * GPU that several ranks share) into receive buffers exported through HIP IPC -- the "direct peer stores" design of
 * SURVEY s5 for schedule_senddata (psolve.c:4945-5079): pack (psolve.c:4985-5011) writes each record where its
 * receiver's unpack (:5035-5073) reads it, and the MPI_Waitall (:5033) becomes a wait on one epoch flag per sending
 * neighbour in the receiver's own memory.  No host hop, no collective, no library between the two GPUs.
 *   1. every rank: hq_comm_ipc_export(ctx, blob)            blob: HQ_IPC_BLOB_BYTES bytes
 *   2. the host all-gathers the blobs in rank order          (MPI_Allgather on comm_solver in the reference's world)
 *   3. every rank: hq_comm_init_ipc(ctx, all_blobs)          all_blobs: nranks x HQ_IPC_BLOB_BYTES
 * A rank whose neighbour stops sending does not spin for ever: a wait longer than HQ_IPC_TIMEOUT_MS (default 20 000)
 * gives up, and the next hq_sync returns HQ_ERR_COMM.
 * HQ_DEBUG_HALO (the reference's -DDEBUG exchange, psolve.c:5002-5007, 5058-5069) is carried: every record travels with
 * a check word -- its node's global id, mixed with the number of the exchange and the record's own three values -- in
 * an id arena beside the record arena; a record that is misrouted, stale (an earlier exchange's) or torn fails the
 * receiver's check and the next hq_sync returns HQ_ERR_COMM.  Every rank of the run must set it.  The receive arena is
 * fine-grained device memory, uncached device memory where the runtime will not export that, coarse-grained as the last
 * resort (ranks of one device only): hq_info.ipc_arena_kind says which.
 * Where the host driver exports device memory through dmabuf only (the MI355X pool this was built on), the process needs
 * HSA_ENABLE_IPC_MODE_LEGACY=0 in its environment BEFORE its first HIP call, or hipIpcGetMemHandle fails with "invalid
 * argument" (hq_comm_ipc_export then returns HQ_ERR_DEVICE with that text; RCCL needs the same setting).
 */
#define HQ_IPC_BLOB_BYTES 4096
HQ_API int hq_comm_ipc_export(hq_ctx* ctx, void* blob);
HQ_API int hq_comm_init_ipc(hq_ctx* ctx, const void* all_blobs);
/* the same with the number of blobs the caller holds (must be nranks): a short gather is refused, not read past its end */
HQ_API int hq_comm_init_ipc_n(hq_ctx* ctx, const void* all_blobs, int32_t nblobs);
/* Diagnostic (profiles/tools/rank_alone_trace.py): the IPC transport with this rank as its own only peer -- every record
 * it sends lands in its own receive buffers and raises its own flags.  The displacements of interface nodes are then
 * WRONG by construction; the step's kernels, streams and waits are exactly those of a rank whose neighbours answer
 * with zero latency. */
HQ_API int hq_comm_init_loopback(hq_ctx* ctx);

/*
 * In-process transport for hosts that drive several partitions from ONE process
 * (and for tests on a single GPU): ctxs[i] must be the context of rank i of n.
 * The halo records then travel by device-to-device copies ordered with HIP
 * events; hq_group_run enqueues `nsteps` steps for all members in lockstep
 * (hq_run on a linked context is not allowed to run alone).
 */
HQ_API int hq_group_link(hq_ctx** ctxs, int32_t n);
HQ_API int hq_group_run(hq_ctx** ctxs, int32_t n, int32_t nsteps);

/*
 * Source forces for steps [step0, step0+nsteps): F[nsteps][nloaded][3], the
 * payload of force_process.<rank> (quakesource.c:2453-2466).
 * Replaces: read_myForces (psolve.c:3651-3667) + compute_addforce_s (:5912-5928).
 * Steps outside the window apply no source.
 * Every node is named at most once, as in the reference's theNodesLoadedList:
 * compute_addforce_s ASSIGNS F dt^2, the scatter variant's source kernel does the
 * same and the brick and patch kernels ADD it, so a node named twice would get
 * one row in one variant and the sum in the other.  Such a list is refused with
 * HQ_ERR_ARG (hq_last_error() names the node) and the context keeps the source
 * it had.  A call with the same node list as the last accepted one only uploads
 * the force table and is not checked again.
 */
HQ_API int hq_set_source(hq_ctx* ctx, int32_t nloaded, const int32_t* loaded_lnid,
                         int32_t step0, int32_t nsteps, const double* F);

/*
 * Enqueue `nsteps` iterations of the solver_run loop body (psolve.c:4265-4319):
 * tm1/tm2 swap, source force, stiffness + Rayleigh damping force
 * (compute_addforce_effective stiffness.c:180-237 + damping_addforce
 * damping.c:29-103), force contribution exchange and hanging-node
 * distribution (psolve.c:4298-4301), nodal update (solver_compute_displacement
 * psolve.c:4072-4114), displacement sharing and hanging-node assignment
 * (psolve.c:4312-4315).  Asynchronous.
 */
HQ_API int hq_run(hq_ctx* ctx, int32_t nsteps);

/*
 * Wait for all enqueued work.  With HQ_DEBUG_HALO=1 in the environment at hq_create (the reference's
 * -DDEBUG build, psolve.c:5002-5007, 5058-5069) every halo record travels with the global identity of
 * its node and the receiver checks it: hq_sync then returns HQ_ERR_COMM if any record arrived for
 * another node than the schedule names.
 */
HQ_API int hq_sync(hq_ctx* ctx);

/*
 * solver_check_nan (psolve.c:3769-3782) on the device-resident tm1, tm2 (and force in the scatter
 * variant): *nonfinite = count of NaN / infinite values.  The reference aborts; here the caller decides.
 */
HQ_API int hq_check_finite(hq_ctx* ctx, int64_t* nonfinite);

/*
 * State as the NEXT loop iteration sees it after its swap -- what stations,
 * planes and checkpoints read (psolve.c:4271-4280): tm1 = u(step*dt),
 * tm2 = u((step-1)*dt).  Either output may be NULL.
 * hq_gather replaces the tm1[] reads of interpolate_station_displacements
 * (psolve.c:6679-6710) / planes; hq_download those of checkpoint_write
 * (io_checkpoint.c:98-112) and the 4D output (output.c:1265).
 */
HQ_API int hq_gather(hq_ctx* ctx, int32_t n, const int32_t* lnid, hq_real* tm1_out, hq_real* tm2_out);
/*
 * The same with tm3 = u((step-2)*dt), which the reference keeps when station accelerations are
 * printed (solver_compute_displacement psolve.c:4093-4101; read at :6762-6778).  The patch variant
 * has it for free -- it is the buffer the next step overwrites; zero before the second step and
 * after hq_upload, as the reference's calloc'ed tm3 is.  HQ_ERR_STATE in the scatter variant.
 */
HQ_API int hq_gather3(hq_ctx* ctx, int32_t n, const int32_t* lnid, hq_real* tm1_out, hq_real* tm2_out,
                      hq_real* tm3_out);
HQ_API int hq_download(hq_ctx* ctx, hq_real* tm1, hq_real* tm2);
/* checkpoint_read (io_checkpoint.c:134-236): overwrite the fields, set the step. */
HQ_API int hq_upload(hq_ctx* ctx, const hq_real* tm1, const hq_real* tm2, int32_t step);

/*
 * Sample recorders (additive under ABI 6): what solver_output_stations / solver_output_planes read at the top of the
 * loop body (psolve.c:4279-4280, :6679-6787; io_planes.c:176-200), taken ON THE DEVICE, so that a host which prints
 * stations every step no longer stops the queue with an hq_gather per print step.  A recorder is a list of points,
 * each the trilinear sum over the 8 nodes of its element; at the head of every step s with s % rate == 0 -- before any
 * of that step's kernels, on exactly the state hq_gather3 documents -- one launch of hq_k_record appends one sample to
 * a ring in device memory:  out[sample][point][3 (1 + derivs)], always double, in both libraries (the f32 library
 * widens each state value first): displacement; with derivs >= 1 the velocity (u1 - u2) / dt; with derivs == 2 the
 * acceleration (u1 - 2 u2 + u3) / dt^2 -- summed by csrc/hq_sample.h, the text hqh_station_kinematics compiles, so
 * the numbers equal the host route's bit for bit.  Step 0 records the initial state; the state after the last step is
 * not sampled until a further step begins.
 * The ring is accounted on the host: which steps are due follows from the step counter alone.  hq_run, hq_group_run
 * and hq_run_timed count the due steps of the call against the free slots of every recorder BEFORE they enqueue
 * anything and return HQ_ERR_STATE, with nothing enqueued and the step counter unchanged, if a ring would overflow.
 * hq_record_fetch waits for the enqueued work (as hq_gather does), delivers the oldest samples first -- at most
 * max_samples; steps[k] is the step number of out's sample k -- and leaves the rest pending.  hq_record_pending waits
 * for nothing: *nsamples counts the samples taken or enqueued, *first_step (may be NULL) is the oldest one's step, -1
 * if there is none.  hq_upload keeps recorders and pending samples; the due steps follow the new step number.
 * hq_record_clear drops every recorder of the context and its memory (hq_destroy does, too); handles are not reused.
 * Errors: HQ_ERR_ARG for null pointers, npoints < 0, rate <= 0, capacity <= 0, derivs outside 0..2, an id outside
 * [0, nharbored), an unknown handle; HQ_ERR_STATE for derivs == 2 in the scatter variant (as hq_gather3).
 * A context without recorders enqueues exactly what it did before they existed.
 */
typedef struct {
    int32_t        npoints;
    const int32_t* ids;       /* [npoints][8] local node ids (octor numbering), as hqh_stations returns them */
    const double*  phi;       /* [npoints][8] trilinear weights */
    int32_t        rate;      /* a sample at every step that is a multiple of rate (> 0) */
    int32_t        derivs;    /* 0 displacement; 1 + velocity; 2 + acceleration (patch variant only) */
    int32_t        capacity;  /* samples the device ring holds (> 0) */
} hq_recorder_desc;
HQ_API int hq_record_add(hq_ctx* ctx, const hq_recorder_desc* desc, int32_t* handle);
HQ_API int hq_record_pending(hq_ctx* ctx, int32_t handle, int32_t* nsamples, int32_t* first_step);
HQ_API int hq_record_fetch(hq_ctx* ctx, int32_t handle, int32_t max_samples, double* out, int32_t* steps,
                           int32_t* nfetched);
HQ_API int hq_record_clear(hq_ctx* ctx);

/*
 * Field snapshots (additive under ABI 6): what the 4D output (solver_output_wavefield psolve.c:3858-3864, output.c:1265)
 * and checkpoint_write (io_checkpoint.c:98-112) read at the top of the loop body, taken WITHOUT stopping the queue.  A
 * snapshot is a range of nodes [first, first + count) in the caller's (octor) numbering; at the head of every step
 * s >= first_step with s % rate == 0 -- where hq_k_record sits, on exactly the state hq_download documents for that step --
 * one launch of hq_k_snapshot copies the fields out of the device's own numbering into a staging slot in device memory,
 * in octor order; a copy stream of the context then carries the slot to pinned host memory while the steps s, s + 1, ...
 * run, and hq_snapshot_fetch hands it over.  tm1 and tm2 are bit copies in hq_real; vel[n][a] = ((double)tm1 - (double)tm2)
 * / dt without contraction, write_velocity's arithmetic as hqh_wavefield_write states it (always double, in both
 * libraries) -- a velocity-only output moves 24 bytes per node instead of 48.
 * `slots` snapshots may be pending (taken or enqueued, not yet fetched) at once; the ring is accounted on the host as the
 * recorders' is: hq_run, hq_group_run and hq_run_timed count the due steps of the call against the free slots BEFORE they
 * enqueue anything and return HQ_ERR_STATE, with nothing enqueued and the step counter unchanged, if a slot would be
 * missing.  hq_snapshot_fetch delivers the OLDEST pending snapshot and frees its slot; it waits only for that slot's copy
 * -- never for the steps enqueued behind it; tm1 / tm2 / vel may be given only for fields the snapshot has (NULL skips
 * one), *step is the snapshot's step, -1 (and nothing else written) if none is pending.  hq_snapshot_pending waits for
 * nothing: *npending counts the snapshots taken or enqueued, *nready those of them whose copy has arrived, *first_step
 * the oldest one's step or -1 (either of the last two may be NULL).  hq_sync and hq_destroy also wait for the copies.
 * hq_upload keeps snapshots and pending slots; the due steps follow the new step number.  hq_snapshot_clear waits, then
 * drops every snapshot of the context and its memory; handles are not reused.  Both variants.
 * Errors: HQ_ERR_ARG for null pointers, a range outside [0, nharbored), count < 1, rate < 1, slots < 1, fields 0 or with
 * unknown bits, an unknown handle, an output pointer for a field the snapshot lacks; HQ_ERR_NOMEM if the staging slots
 * (device), the id map or the pinned host buffers cannot be allocated -- nothing is kept then.
 * A context without snapshots enqueues exactly what it did before they existed.
 */
enum { HQ_SNAP_TM1 = 1, HQ_SNAP_TM2 = 2, HQ_SNAP_VEL = 4 };
typedef struct {
    int32_t first, count;     /* local node ids [first, first + count), octor numbering; count >= 1 */
    int32_t rate;             /* a snapshot at the head of every step s >= first_step with s % rate == 0 */
    int32_t first_step;
    int32_t fields;           /* mask of HQ_SNAP_*; non-zero, no unknown bits */
    int32_t slots;            /* snapshots that may be pending at once (>= 1) */
} hq_snapshot_desc;
HQ_API int hq_snapshot_add(hq_ctx* ctx, const hq_snapshot_desc* desc, int32_t* handle);
HQ_API int hq_snapshot_pending(hq_ctx* ctx, int32_t handle, int32_t* npending, int32_t* nready, int32_t* first_step);
HQ_API int hq_snapshot_fetch(hq_ctx* ctx, int32_t handle, hq_real* tm1, hq_real* tm2, double* vel, int32_t* step);
HQ_API int hq_snapshot_clear(hq_ctx* ctx);

/*
 * Peak-motion trackers (additive under ABI 6): the running PGD / PGV / PGA map -- the largest displacement, velocity and
 * acceleration every point saw over the run -- kept ON THE DEVICE.  A peak is a reduction over time: one slot per point
 * updated in place has no ring, cuts no batch, moves nothing over PCIe until it is fetched and never stops the queue;
 * the other route is a recorder at rate 1 and a fold of every sample on the host (hqh_peak_fold, hq_host.h).
 * A tracker is a list of points: with nodes_per_point = 8 the trilinear sum over the 8 nodes of an element, as a
 * recorder's; with nodes_per_point = 1 single nodes (a surface map), with no weights at all.  At the head of every step
 * s >= first_step with s % rate == 0 -- where hq_k_record sits, before any of that step's kernels, on exactly the state
 * hq_gather3 documents -- one launch of hq_k_peak forms the sample hq_k_record would take at the point (every value
 * widened to double first, csrc/hq_sample.h's order of operations, no contraction: the recorder's sample bit for
 * bit) and folds it into the point's state.  Per point and quantity q of the mask, in the order displacement, velocity
 * (u1 - u2) / dt, acceleration (u1 - 2 u2 + u3) / dt^2, that state is (csrc/hq_peak.h):
 *   peaks[p][q][0..2] = max |v_x|, |v_y|, |v_z|
 *   peaks[p][q][3]    = max (v_x v_x + v_y v_y)             horizontal, SQUARED (z is depth)
 *   peaks[p][q][4]    = max (v_x v_x + v_y v_y) + v_z v_z   total, SQUARED, summed in this order
 *   when[p][q][0]     = the step at which [3] was last raised, when[p][q][1] the same for [4]; -1 = never
 * always double, in both libraries.  A value enters only if it is strictly greater: the first occurrence of a maximum
 * is kept, a sample of exactly 0 leaves `when` at -1, a NaN never enters.  The device takes no root -- the caller takes
 * sqrt of [3] and [4] -- so the state equals the host fold of a recorder's samples of the same run bit for bit.
 * Step 0 samples the initial state; as with recorders, the state after the last step is not sampled until a further
 * step begins.
 * hq_peak_fetch waits for the enqueued work (as hq_record_fetch does), copies the state out -- peaks [np][nq][5], when
 * [np][nq][2], nq the number of set bits of `quantities` -- and leaves it in place; *nsamples counts the due steps folded
 * so far, accounted on the host from the step counter.  It adds exactly the fetched bytes, 48 np nq, to
 * hq_info.pcie_d2h_bytes; between fetches a tracker moves nothing.  hq_peak_load puts fetched values back (a run that
 * restarts from a checkpoint); hq_peak_reset zeroes the state, sets `when` to -1 and nsamples to 0.  hq_upload keeps
 * trackers and their state; the due steps follow the new step number.  hq_peak_clear drops every tracker of the context
 * and its memory (hq_destroy does, too); handles are not reused.  Trackers are neither recorders nor snapshots:
 * hq_record_clear, hq_snapshot_clear and the hqh_solver_run* runners leave them alone, and no run call has anything to
 * count for them -- add a tracker, run through any runner, fetch.  The device memory counts in hq_info.device_bytes.
 * Only a tracker with HQ_PEAK_ACC reads u(t - 2 dt), the buffer the step's own kernels overwrite: its due steps hold the
 * streams of those kernels back behind the launch, as a recorder's do; a displacement / velocity map holds nothing.
 * Errors: HQ_ERR_ARG for null pointers, npoints < 0, nodes_per_point not 1 or 8, rate < 1, quantities 0 or with unknown
 * bits, an id outside [0, nharbored), an unknown handle; HQ_ERR_STATE for HQ_PEAK_ACC in the scatter variant (as
 * hq_gather3); HQ_ERR_NOMEM if the device memory cannot be allocated -- nothing is kept then.  npoints == 0 is valid.
 * A context without trackers enqueues exactly what it did before they existed.
 */
enum { HQ_PEAK_DISP = 1, HQ_PEAK_VEL = 2, HQ_PEAK_ACC = 4 };
typedef struct {
    int32_t        npoints;
    int32_t        nodes_per_point;  /* 8: ids [np][8] + phi [np][8], as hqh_stations returns them; 1: ids [np], phi ignored (may be NULL) */
    const int32_t* ids;              /* local node ids, octor numbering */
    const double*  phi;
    int32_t        rate, first_step; /* a sample at the head of every step s >= first_step with s % rate == 0 */
    int32_t        quantities;       /* mask of HQ_PEAK_*; non-zero, no unknown bits */
    int32_t        reserved;
} hq_peak_desc;
HQ_API int hq_peak_add(hq_ctx* ctx, const hq_peak_desc* desc, int32_t* handle);
HQ_API int hq_peak_fetch(hq_ctx* ctx, int32_t handle, double* peaks, int32_t* when, int64_t* nsamples);
HQ_API int hq_peak_load(hq_ctx* ctx, int32_t handle, const double* peaks, const int32_t* when, int64_t nsamples);
HQ_API int hq_peak_reset(hq_ctx* ctx, int32_t handle);
HQ_API int hq_peak_clear(hq_ctx* ctx);

/*
 * Response-spectrum trackers (additive under ABI 6): SD at a handful of periods per surface node or station -- what
 * ShakeMap-style products and building codes are written in -- kept ON THE DEVICE.  A spectrum is a recursive filter plus a
 * running maximum: a state of fixed size per point and period, a reduction over time in the sense a peak is.  The other
 * route is a recorder at rate 1 with derivs = 2 and a filter over every sample on the host (hqh_spec_fold, hq_host.h).
 * The oscillator is x'' + 2 zeta omega x' + omega^2 x = -a_g(t), omega = 2 pi / T, with a_g piecewise linear between the
 * samples (Nigam & Jennings); its step is h = rate x dt and exact for that input (csrc/hq_sdof.h).  The eight
 * coefficients of the step come from a scaled Taylor series of the 4 x 4 propagator in non-dimensional variables --
 * additions, multiplications and divisions only, no libm, one result whatever compiler built the library -- because the
 * textbook closed form cancels catastrophically at a simulation's time step (2e-5 relative at T = 10 s, h = 3e-4 s; the
 * series holds 1e-14, tests/test_spectra_cpu.py).  hq_spec_coefficients delivers the table [nperiods][8] = {A11, A12,
 * A21, A22, B11, B12, B21, B22} as the kernel reads it; it equals hqh_sdof_coef's bit for bit.
 * Points, rate and first_step are a peak tracker's.  At the head of every step s >= first_step with s % rate == 0 one
 * launch of hq_k_spec forms the acceleration sample hq_k_record takes at the point with derivs = 2 -- (u1 - 2 u2 + u3) /
 * dt^2 on the state hq_gather3 documents, the recorder's column bit for bit -- and, per period, steps three oscillators
 * (one per axis) from the point's previous sample to this one and folds |x| into the maxima.  The sample taken at the
 * head of step s is the acceleration at time (s - 1) dt: u1 = u(s dt), u2 and u3 the two fields before it.  The state
 * starts at rest with the previous sample 0, so the first due sample is the end of a ramp from 0 over h.  Per point:
 *   sd[p][j][0..2]   = max |x_x|, |x_y|, |x_z| of period j
 *   sd[p][j][3]      = max (x_x x_x + x_y x_y)      horizontal resultant, SQUARED, summed in this order: its root is
 *                                                   RotD100 of SD
 *   osc[p][j][0][0..2] = x, osc[p][j][1][0..2] = v  the oscillators as they stand
 *   aprev[p][0..2]   = the last sample folded
 * always double, in both libraries.  A value enters sd only if it is strictly greater: a NaN never enters sd, though a
 * NaN sample does stay in x and v from then on, as in any linear filter.  The device multiplies nothing further: the
 * caller forms PSV = omega SD and PSA = omega^2 SD (and takes the root of [3]), so the state equals hqh_spec_fold of a
 * recorder's acceleration columns of the same run bit for bit.
 * hq_spec_fetch waits for the enqueued work (as hq_peak_fetch does), copies the state out -- sd [np][nper][4]; osc
 * [np][nper][2][3] and aprev [np][3], either of which may be NULL -- and leaves it in place; *nsamples counts the due steps
 * folded so far.  It adds exactly the fetched bytes, 8 np (4 nper [+ 6 nper] [+ 3]), to hq_info.pcie_d2h_bytes; between
 * fetches a tracker moves nothing.  hq_spec_load puts fetched values back (all three arrays required); hq_spec_reset
 * puts the state at rest: zeros, nsamples 0.  hq_upload keeps trackers and their state; the due steps follow the new step
 * number.  hq_spec_clear drops every spectrum tracker of the context and its memory (hq_destroy does, too); handles are
 * not reused.  hq_record_clear, hq_snapshot_clear, hq_peak_clear and the hqh_solver_run* runners leave them alone, and no
 * run call has anything to count for them.  The device memory counts in hq_info.device_bytes.  Every due step reads
 * u(t - 2 dt), so it holds the bricks' and the exchange chain's streams back behind the launch, as a recorder's does.
 * Errors: HQ_ERR_ARG for null pointers, npoints < 0, nodes_per_point not 1 or 8, rate < 1, nperiods outside 1 ..
 * HQ_SPEC_MAX_PERIODS, a period that is not finite or not positive, damping outside [0, 1) or NaN, an id outside [0,
 * nharbored), an unknown handle; HQ_ERR_STATE in the scatter variant, which keeps no u(t - 2 dt) (as hq_gather3);
 * HQ_ERR_NOMEM if the device memory cannot be allocated -- nothing is kept then.  npoints == 0 is valid.
 * A context without spectrum trackers enqueues exactly what it did before they existed.
 */
enum { HQ_SPEC_MAX_PERIODS = 32, HQ_SPEC_NVAL = 4 };
typedef struct {
    int32_t        npoints;
    int32_t        nodes_per_point;  /* 8: ids [np][8] + phi [np][8]; 1: ids [np], phi ignored (may be NULL) */
    const int32_t* ids;              /* local node ids, octor numbering */
    const double*  phi;
    int32_t        rate, first_step; /* a sample at the head of every step s >= first_step with s % rate == 0 */
    int32_t        nperiods;         /* 1 .. HQ_SPEC_MAX_PERIODS */
    int32_t        reserved;
    const double*  periods;          /* [nperiods] seconds, finite, > 0 */
    double         damping;          /* fraction of critical, 0 <= damping < 1 */
} hq_spec_desc;
HQ_API int hq_spec_add(hq_ctx* ctx, const hq_spec_desc* desc, int32_t* handle);
HQ_API int hq_spec_coefficients(hq_ctx* ctx, int32_t handle, double* coef);
HQ_API int hq_spec_fetch(hq_ctx* ctx, int32_t handle, double* sd, double* osc, double* aprev, int64_t* nsamples);
HQ_API int hq_spec_load(hq_ctx* ctx, int32_t handle, const double* sd, const double* osc, const double* aprev, int64_t nsamples);
HQ_API int hq_spec_reset(hq_ctx* ctx, int32_t handle);
HQ_API int hq_spec_clear(hq_ctx* ctx);

/*
 * Cumulative-intensity trackers (additive under ABI 6): the time integrals landslide, liquefaction and damage models are
 * written in -- Arias intensity Ia = pi / (2 g) int a^2 dt, cumulative absolute velocity CAV = int |a| dt, the specific
 * energy density int v^2 dt -- and the durations that go with them, kept ON THE DEVICE.  An integral over time is a
 * reduction over time in the sense a peak is: a state of fixed size per point folded in place, no ring, no batch cut,
 * nothing over PCIe until it is fetched.  The other route is a recorder at rate 1 with derivs = 2 and a loop over every
 * sample on the host (hqh_cum_fold, hq_host.h).
 * Points, rate, first_step and the mask `quantities` are a peak tracker's.  At the head of every step s >= first_step with
 * s % rate == 0 -- where hq_k_record sits, on exactly the state hq_gather3 documents -- one launch of hq_k_cum forms the
 * sample hq_k_record would take at the point (every value widened to double first, csrc/hq_sample.h's order of operations,
 * / dt and / dt^2 divisions, no contraction: the recorder's sample bit for bit) and adds it in.  Per point and quantity q
 * of the mask, in the order displacement, velocity, acceleration, the state is (csrc/hq_cumul.h):
 *   sums[p][q][0..2] = sum of |v_x|, |v_y|, |v_z|         one addition per due sample, in time order
 *   sums[p][q][3..5] = sum of v_x v_x, v_y v_y, v_z v_z   the product rounded first, then added: never an FMA
 *   span[p][q][0]    = the first step at which (v_x v_x + v_y v_y) + v_z v_z > threshold[q]^2; -1 = never
 *   span[p][q][1]    = the last such step; -1 = never
 *   span[p][q][2]    = the number of such samples
 * sums always double, in both libraries.  threshold[q] belongs to quantity q of the mask, in mask order; it is squared once,
 * on the host.  The comparison is strict: a sample exactly at the threshold does not count and a NaN sample never does,
 * though a NaN does stay in the sums from then on, as in any running sum.
 * The rectangle rule: the device multiplies by NOTHING, so the state equals hqh_cum_fold of a recorder's samples of the same
 * run bit for bit.  With h = rate x dt the caller forms CAV = h sums[..][acc][0..2], Ia = pi / (2 g) h sums[..][acc][3..5]
 * per axis (their sum for the total), the energy density h sums[..][vel][3..5]; the bracketed duration is (span[1] -
 * span[0]) dt and the uniform duration span[2] h.  As with recorders, step 0 samples the initial state, the sample taken at
 * the head of step s is the displacement at time s dt (the acceleration the one centred on (s - 1) dt), and the state after the last step is not
 * sampled until a further step begins.
 * The Husid curve: with husid_every >= 1 the three sums of squares of every quantity, as they stand after every
 * husid_every-th due sample (counted from the first due one: samples husid_every, 2 husid_every, ...), are kept in device
 * memory, husid_slots of them at most; further samples are still folded into the sums, the curve simply ends.  Which sample
 * fills which slot is accounted on the host when the step is enqueued.  Significant durations (D5-75, D5-95) come out of
 * one run without a second pass: hqh_husid_cross (hq_host.h) finds where a curve crosses a fraction of its total.
 * husid_every = husid_slots = 0: no curve.
 * hq_cum_fetch waits for the enqueued work (as hq_peak_fetch does), copies the state out -- sums [np][nq][6], span
 * [np][nq][3], nq the number of set bits of `quantities`; curve [nfilled][np][nq][3] and curve_steps [nfilled], the step of
 * the sample each slot was stored behind, either of which may be NULL (give them room for husid_slots entries) -- and leaves
 * it in place; *nfilled counts the slots filled or enqueued, *nsamples the due steps folded so far, both accounted on the
 * host.  It adds exactly the fetched bytes, 60 np nq (+ 24 np nq nfilled with the curve), to hq_info.pcie_d2h_bytes; between
 * fetches a tracker moves nothing.  hq_cum_load puts fetched values back (a run that restarts from a checkpoint): the same
 * arrays, curve and curve_steps required unless nfilled == 0, and nfilled must be what nsamples due samples fill, min(nsamples
 * / husid_every, husid_slots), because the slots go on from nsamples.  hq_cum_reset zeroes the sums and the counts, sets the
 * first and last steps to -1, nsamples and nfilled to 0.  hq_upload keeps trackers, their state and their curve; the due steps
 * follow the new step number.  hq_cum_clear drops every cumulative tracker of the context and its memory (hq_destroy does,
 * too); handles are not reused.  hq_record_clear, hq_snapshot_clear, hq_peak_clear, hq_spec_clear and the hqh_solver_run*
 * runners leave them alone, and no run call has anything to count for them.  The device memory -- 12 K np of tables (4 np
 * for K = 1) + np nq (60 + 24 husid_slots) -- counts in hq_info.device_bytes.
 * Only a tracker with HQ_PEAK_ACC reads u(t - 2 dt), the buffer the step's own kernels overwrite: its due steps hold the
 * bricks' and the exchange chain's streams back behind the launch, as a recorder's do; other masks hold nothing.
 * Errors: HQ_ERR_ARG for null pointers, npoints < 0, nodes_per_point not 1 or 8, rate < 1, quantities 0 or with unknown
 * bits, husid_every and husid_slots not both 0 or both >= 1, a threshold (of a quantity in the mask) that is negative, NaN
 * or infinite, an id outside [0, nharbored), an unknown handle, an nfilled that does not fit nsamples (hq_cum_load);
 * HQ_ERR_STATE for HQ_PEAK_ACC in the scatter variant (as hq_gather3); HQ_ERR_NOMEM if the device memory cannot be
 * allocated -- nothing is kept then.  npoints == 0 is valid.
 * A context without cumulative trackers enqueues exactly what it did before they existed.
 */
typedef struct {
    int32_t        npoints;
    int32_t        nodes_per_point;  /* 8: ids [np][8] + phi [np][8]; 1: ids [np], phi ignored (may be NULL) */
    const int32_t* ids;              /* local node ids, octor numbering */
    const double*  phi;
    int32_t        rate, first_step; /* a sample at the head of every step s >= first_step with s % rate == 0 */
    int32_t        quantities;       /* mask of HQ_PEAK_*; non-zero, no unknown bits */
    int32_t        husid_every, husid_slots;   /* 0, 0: no curve; else both >= 1 */
    int32_t        reserved;
    double         threshold[3];     /* per quantity of the mask, in mask order; finite, >= 0; the rest is not read */
} hq_cum_desc;
HQ_API int hq_cum_add(hq_ctx* ctx, const hq_cum_desc* desc, int32_t* handle);
HQ_API int hq_cum_fetch(hq_ctx* ctx, int32_t handle, double* sums, int32_t* span, double* curve, int32_t* curve_steps,
                        int32_t* nfilled, int64_t* nsamples);
HQ_API int hq_cum_load(hq_ctx* ctx, int32_t handle, const double* sums, const int32_t* span, const double* curve,
                       const int32_t* curve_steps, int32_t nfilled, int64_t nsamples);
HQ_API int hq_cum_reset(hq_ctx* ctx, int32_t handle);
HQ_API int hq_cum_clear(hq_ctx* ctx);

/*
 * Deformation trackers (additive under ABI 6): the running peaks of the ground's DEFORMATION -- peak ground strain for
 * pipelines and tunnels, peak dynamic stress (von Mises, volumetric) for triggering studies, tilt and torsion for rotational
 * seismology -- kept ON THE DEVICE.  A peak of strain is a reduction over time in the sense a peak of motion is: a state of
 * fixed size per point folded in place, no ring, no batch cut, nothing over PCIe until it is fetched.  The other route is
 * three recorders at rate 1 whose phi tables are the gradient weights, nine columns per point and step over PCIe, and a
 * fold on the host (hqh_deform_fold, hq_host.h).
 * A point lies in an element: ids are its eight nodes and grad[b][c] = d phi_c / d x_b the derivatives of their trilinear
 * shape functions at the point (hqh_gradient_weights, hqh_station_gradients; point_strain, nonlinear.c:873-905, evaluates
 * the same sums).  At the head of every step s >= first_step with s % rate == 0 -- where hq_k_record sits, before any of that
 * step's kernels, on exactly the state hq_gather documents -- one launch of hq_k_deform forms the displacement gradient
 * G[b][a] = d u_a / d x_b = sum_c grad[b][c] u_a[c]: row b is the sample hq_k_record would take with phi = grad[b] (every
 * value widened to double first, csrc/hq_sample.h's order of operations, no contraction), bit for bit, and the rate
 * gradient is that recorder's velocity column, (sum_c grad[b][c] u1 - grad[b][c] u2) / dt.  From them (csrc/hq_deform.h):
 *   strain    (xx, yy, zz, xy, yz, xz), the reference's tensor order: xx = G[0][0], yy = G[1][1], zz = G[2][2],
 *             xy = 0.5 (G[1][0] + G[0][1]), yz = 0.5 (G[2][1] + G[1][2]), xz = 0.5 (G[2][0] + G[0][2]) -- tensor shear, half
 *             the engineering shear
 *   rotation  half the curl: wx = 0.5 (G[1][2] - G[2][1]), wy = 0.5 (G[2][0] - G[0][2]), wz = 0.5 (G[0][1] - G[1][0])
 *   stress    of the displacement's strain and the point's moduli, point_stress's order of operations (nonlinear.c:
 *             907-924): mu2 = 2 mu, lkk = lambda ((xx + yy) + zz), s_aa = mu2 e_aa + lkk, s_ab = mu2 e_ab, products
 *             rounded first
 * The state of a point is one block per set bit of `quantities`, in the order of the bits: ten doubles and two int32 per
 * tensor (HQ_DEFORM_STRAIN, _STRAIN_RATE, _STRESS), then five doubles and two int32 per vector (HQ_DEFORM_ROTATION,
 * _ROTATION_RATE) -- vals [np][10 nt + 5 nv], when [np][2 (nt + nv)], nt and nv the set bits among the first three and the
 * last two.  A tensor's block:
 *   vals[0..5] = max |xx|, |yy|, |zz|, |xy|, |yz|, |xz|
 *   vals[6]    = max |(xx + yy) + zz|     the volumetric measure (3 x the mean stress, for a stress)
 *   vals[7]    = max 6 J2 = ((dxy dxy + dyz dyz) + dzx dzx) + 6.0 ((xy xy + yz yz) + xz xz) with dxy = xx - yy, dyz = yy - zz,
 *                dzx = zz - xx, summed in this order: the caller divides by 6, or takes sqrt(vals[7] / 2) of a stress
 *                block for the peak von Mises stress
 *   vals[8]    = max hd hd + 4.0 (xy xy), hd = xx - yy: the largest engineering shear in the horizontal plane, SQUARED
 *   vals[9]    = max |xx + yy|            the areal strain
 *   when[0]    = the step at which vals[7] was last raised, when[1] the same for vals[6]; -1 = never
 * A vector's block is a peak tracker's (csrc/hq_peak.h): max |wx|, |wy|, |wz|, max (wx wx + wy wy) -- the tilt, SQUARED --
 * max (wx wx + wy wy) + wz wz, and the steps the last two were last raised at; the torsion is the z slot.
 * Always double, in both libraries.  A value enters only if it is strictly greater: the first occurrence of a maximum is
 * kept, a sample of exactly 0 leaves `when` at -1, a NaN never enters.  The device takes no root, so the state equals
 * hqh_deform_fold of three recorders' samples of the same run bit for bit.  Step 0 samples the initial state; as with
 * recorders, the state after the last step is not sampled until a further step begins.
 * hq_deform_fetch waits for the enqueued work (as hq_peak_fetch does), copies the state out and leaves it in place;
 * *nsamples counts the due steps folded so far, accounted on the host from the step counter.  It adds exactly the fetched
 * bytes, np (88 nt + 48 nv), to hq_info.pcie_d2h_bytes; between fetches a tracker moves nothing.  hq_deform_load puts
 * fetched values back (a run that restarts from a checkpoint); hq_deform_reset zeroes the state, sets `when` to -1 and
 * nsamples to 0.  hq_upload keeps trackers and their state; the due steps follow the new step number.  hq_deform_clear drops
 * every deformation tracker of the context and its memory (hq_destroy does, too); handles are not reused.  hq_record_clear,
 * hq_snapshot_clear, hq_peak_clear, hq_spec_clear, hq_cum_clear and the hqh_solver_run* runners leave them alone, and no
 * run call has anything to count for them.  The device memory -- np (32 of ids + 192 of weights [+ 16 of moduli]) of
 * tables and np (88 nt + 48 nv) of state -- counts in hq_info.device_bytes.
 * The launch reads u(t) and u(t - dt) only (the latter only with a rate bit), which the step's own kernels only read: it
 * holds no stream back, and every variant has it, the scatter variant included.
 * Errors: HQ_ERR_ARG for null pointers, npoints < 0, rate < 1, quantities 0 or with unknown bits, HQ_DEFORM_STRESS without
 * lame, a modulus that is NaN or infinite or mu < 0, an id outside [0, nharbored), an unknown handle; HQ_ERR_NOMEM if the
 * device memory cannot be allocated -- nothing is kept then.  npoints == 0 is valid.
 * A context without deformation trackers enqueues exactly what it did before they existed.
 */
#ifndef HQ_DEFORM_QUANTITIES
#define HQ_DEFORM_QUANTITIES
enum { HQ_DEFORM_STRAIN = 1, HQ_DEFORM_STRAIN_RATE = 2, HQ_DEFORM_STRESS = 4, HQ_DEFORM_ROTATION = 8, HQ_DEFORM_ROTATION_RATE = 16 };
#endif
typedef struct {
    int32_t        npoints;
    const int32_t* ids;              /* [npoints][8] local node ids (octor numbering), as hqh_station_gradients returns them */
    const double*  grad;             /* [npoints][3][8] grad[p][b][c] = d phi_c / d x_b at the point */
    const double*  lame;             /* [npoints][2] lambda, mu of the point's element; NULL unless HQ_DEFORM_STRESS */
    int32_t        rate, first_step; /* a sample at the head of every step s >= first_step with s % rate == 0 */
    int32_t        quantities;       /* mask of HQ_DEFORM_*; non-zero, no unknown bits */
    int32_t        reserved;
} hq_deform_desc;
HQ_API int hq_deform_add(hq_ctx* ctx, const hq_deform_desc* desc, int32_t* handle);
HQ_API int hq_deform_fetch(hq_ctx* ctx, int32_t handle, double* vals, int32_t* when, int64_t* nsamples);
HQ_API int hq_deform_load(hq_ctx* ctx, int32_t handle, const double* vals, const int32_t* when, int64_t nsamples);
HQ_API int hq_deform_reset(hq_ctx* ctx, int32_t handle);
HQ_API int hq_deform_clear(hq_ctx* ctx);

/*
 * BKT constant-Q attenuation (type_of_damping = bkt: calc_conv and constant_Q_addforce, damping.c:110-416), scatter
 * variant, double library.  With attenuation set the step is
 *     hq_k_source -> hq_k_atten_advance -> hq_k_element_bkt -> (exchanges, hq_k_distribute) -> hq_k_update
 * and everything but the two kernels in the middle runs as it does without.
 *
 * coef: the ten floats per element a0_shear, a1_shear, b_shear, g0_shear, g1_shear, a0_kappa, a1_kappa, b_kappa, g0_kappa,
 * g1_kappa in edata_t's order (psolve.h:96) -- the caller's edata + 4; freq: Param.theFreq.  The library holds no Q table and
 * no Qs(Vs) rule: those are mesh-time (mesh_correct_properties, psolve.c:7239-7329) and stay the caller's.
 *
 * State.  The reference keeps four memory variables per element corner (768 B per element).  A corner's variable depends
 * on its element's ten floats and its node's history only, so the library keeps one copy per (node, class) SLOT, a class
 * being one distinct row of the ten floats (bitwise): bit for bit the reference's values (csrc/hq_atten.h states why both
 * of the reference's branches fall out of one formula).  Device bytes added, exactly (hq_info.device_bytes grows by it, and
 * hq_attenuation_info / hq_attenuation_plan_check report it):
 *     144 nslots  (12 rows of memory variables + 6 rows of damping vectors, double, SoA [row][nslots])
 *   +  32 Epad    (the slot of every element corner, int32 [8][Epad], Epad = lenum rounded up to 64)
 *   +   8 nslots  (every slot's node and class, int32)
 *   + 144 nclasses (18 doubles per class)
 * In a uniform region that is 152 B per node.
 *
 * hq_attenuation_set: between steps; the memory variables start at 0; set again replaces plan and state.  It refuses, with
 * the context left as it was: a context of the patch variant (HQ_ERR_STATE: create with HQ_VARIANT_SCATTER), the float
 * library (HQ_ERR_STATE), an eTable with any c3 or c4 != 0 (HQ_ERR_ARG: under BKT compute_setab yields a = b = 0,
 * psolve.c:5869), freq <= 0 or not finite, a coefficient that is not finite (HQ_ERR_ARG).
 * hq_attenuation_info: out = {classes, slots, device bytes added, 0 (1: hq_attenuation_set_split)}; all 0 on a context without
 * attenuation.
 * hq_attenuation_fetch / _load speak the reference's layout: four arrays [lenum * 8][3] (cindex = eindex * 8 + i) for
 * conv_shear_1, conv_shear_2, conv_kappa_1, conv_kappa_2.  fetch leaves out an array passed as NULL; load needs all four
 * and refuses (HQ_ERR_ARG, the text names the node) an input in which two corners of one slot differ, or a value that is
 * not finite.  hq_upload zeroes the memory variables -- the reference's own restart (io_checkpoint.c carries tm1 / tm2
 * only and the arrays are calloc'ed); an exact restart is hq_upload followed by hq_attenuation_load.
 * hq_attenuation_clear: back to the Rayleigh step of the context's eTable; the added bytes go.
 * hq_attenuation_plan_check: host only, no device -- the slot plan of `desc` (lnid, nharbored, the hanging-node table) under
 * `coef`: report = {classes, slots, device bytes an attenuated context adds, faults}, faults counting element corners whose
 * slot is not (their node, their class), slots out of node-major order and hanging nodes without a slot.
 * On an attenuated context hq_dominant_kernel names hq_k_element_bkt, and hq_phase_force runs the two kernels (every call
 * advances the memory variables one step, as calc_conv does).
 * Not here: attenuation INSIDE the patch and brick kernels (beside them: hq_attenuation_set_split, below), the float library, the
 * Q table and the velocity correction.
 */
typedef struct {
    const float* coef;               /* [lenum][10], order above */
    double freq;                     /* Param.theFreq            */
} hq_attenuation_desc;
HQ_API int hq_attenuation_set(hq_ctx* ctx, const hq_attenuation_desc* desc);
HQ_API int hq_attenuation_info(hq_ctx* ctx, int64_t out[4]);
HQ_API int hq_attenuation_fetch(hq_ctx* ctx, double* shear1, double* shear2, double* kappa1, double* kappa2);
HQ_API int hq_attenuation_load(hq_ctx* ctx, const double* shear1, const double* shear2, const double* kappa1, const double* kappa2);
HQ_API int hq_attenuation_clear(hq_ctx* ctx);
HQ_API int hq_attenuation_plan_check(const hq_desc* desc, const float* coef, int64_t report[4]);

/*
 * BKT attenuation on a context of the PATCH variant: a correction pass beside the step (csrc/hq_atten_split.h), double library,
 * one context alone.  Under BKT c3 = c4 = 0 and the patch and brick kernels apply mu K_mu + kappa K_kappa to u1; the BKT force
 * is that elastic force plus dF = mu K_mu ds + kappa K_kappa dk, with ds, dk the damping vectors without their final + u1
 * (hq_atten_advance_delta).  The rest of the step is linear in the force, so the attenuated step is the unchanged elastic step,
 *     (patches, bricks)  ||  hq_k_atten_advance_delta -> hq_k_atten_corner_force -> hq_k_atten_node_sum   (a stream of its own)
 * followed on the compute stream by
 *     hq_k_distribute (dF's hanging nodes) -> hq_k_atten_apply (u_new += dF / n_t[0]) -> hq_k_adjust_assign (u_new).
 * dF is summed per node through a host-built table in element order, without atomics: two runs give identical bits.  The
 * result differs from the scatter variant's attenuated step by rounding only (two more roundings per node and component).
 *
 * hq_attenuation_set_split: desc, state and the rules of hq_attenuation_set; the memory variables are hq_attenuation_set's bit for
 * bit.  It refuses, the context left as it was: a scatter context (HQ_ERR_STATE: call hq_attenuation_set), the float library
 * (HQ_ERR_STATE), a context with nranks > 1, a linked group or any transport (HQ_ERR_STATE), an eTable with c3 or c4 != 0, a bad
 * freq, a coefficient that is not finite (HQ_ERR_ARG).  On a split context hq_comm_init*, hq_group_link refuse (HQ_ERR_STATE).
 * hq_attenuation_info: out[3] = 1.  _fetch / _load / _clear and hq_upload as on a scatter context (the per-corner layout in the
 * caller's element order and node numbering).  hq_dominant_kernel keeps naming the step kernel.
 * Device bytes added, exactly (N = nharbored, E = lenum, Epad = E rounded up to 64; A = distinct anchors, H = (hanging node,
 * anchor) pairs of the hanging-node table):
 *     144 nslots + 32 Epad + 8 nslots + 144 nclasses     (as hq_attenuation_set; the damping-vector rows hold ds, dk)
 *   + 192 Epad            (corner forces, double [3][8][Epad])
 *   +  48 E               (c1, c2 and the node -> (element, corner) entries)
 *   +   4 (N + 1) + 32 N  (the table's row pointers; dF [N][3] and the mass row n_t[n][0])
 *   +   8 A + 4 + 8 H     (dF's distribution tables; nothing where no node hangs)
 * For this call every context of the patch variant keeps, on the HOST, its element table, c1 / c2 and the mass row: 48 B per
 * element + 8 B per node.
 * hq_attenuation_split_plan_check: host only -- report = {classes, slots, the bytes above, faults}; faults add to
 * hq_attenuation_plan_check's those of the node -> (element, corner) table (every corner exactly once, under its own node, in
 * the caller's element order; the device's own element order a permutation) and of the hanging-node lists (every (node, anchor) pair once, with the node's number of anchors).
 * hq_attenuation_split_plan_tables hands out the tables of `desc` in the numbering hq_create gives it (counts = {N + 1, 8 E, H};
 * epos [E] = the place the device gives the caller's element (the elements sorted by their lowest device node, for locality),
 * nptr [N + 1], nent [8 E] with entry = corner * Epad + epos[element], per node in the CALLER's element order, sd [H][3] =
 * {hanging node, anchor, anchors of the node}; a NULL array is left out), and hq_attenuation_split_table_faults counts the
 * faults of tables given to it: the same check.
 * Not here: partitions and transports, the float library, folding the correction into the brick and patch kernels, the Q
 * table and the velocity correction, the reference-link stub.
 */
HQ_API int hq_attenuation_set_split(hq_ctx* ctx, const hq_attenuation_desc* desc);
HQ_API int hq_attenuation_split_plan_check(const hq_desc* desc, const float* coef, int64_t report[4]);
HQ_API int hq_attenuation_split_plan_tables(const hq_desc* desc, int32_t* epos, int32_t* nptr, int32_t* nent, int32_t* sd,
                                            int64_t counts[3]);
HQ_API int hq_attenuation_split_table_faults(const hq_desc* desc, const int32_t* epos, const int32_t* nptr, const int32_t* nent,
                                             const int32_t* sd, int64_t nsd, int64_t* faults);

/*
 * Nonlinear soil (include_nonlinear_analysis = yes, plasticity_model = rate_independant: nonlinear.c) on a context of the PATCH
 * variant: rate-independent von Mises and Drucker-Prager plasticity with linear hardening at the eight quadrature points of
 * every nonlinear element, as a correction pass beside the unchanged step (csrc/hq_nonlin.h has the text, point by point;
 * csrc/hq_nonlin_dev.h the plan and the kernel).  Double library, one context alone.
 *
 * In a nonlinear element the reference applies -dt^2 sum_qp B^T sigma(e - ep) h^3 / 8 instead of the stiffness force.
 * point_stress is linear, so that is the elastic force the patch and brick kernels already apply plus
 *     dF = +dt^2 h^3 / 8 sum_qp B^T sigma(ep),
 * ep the plastic strain as it stood BEFORE this step's update (the reference's pstrains1).  Everything behind the force is
 * linear in it, Rayleigh terms included, so the step is the unchanged step,
 *     (patches, bricks)  ||  hq_k_nl_element -> hq_k_atten_node_sum              (a stream of its own)
 * followed on the compute stream by
 *     hq_k_distribute (dF's hanging nodes) -> hq_k_atten_apply_at (u_new += dF / n_t[0]) -> hq_k_adjust_assign (u_new),
 * over the nonlinear elements and the nodes they touch only.  dF is summed per node through a host-built table in the
 * caller's element order, without atomics: wherever the elastic step leaves identical bits, two runs do.
 *
 * desc: model HQ_NL_VONMISES or HQ_NL_DRUCKERPRAGER; elems [nelems], the nonlinear elements in the caller's numbering,
 * strictly ascending (the reference's myNonlinElementsMapping); cons [nelems][6] = h (edgesize), mu, lambda, alpha, k, hardening
 * modulus per element (hqh_nonlinear_constants derives them as nonlinear_solver_init does).
 * State: ONE copy of the plastic strain (6 values: xx yy zz xy yz xz) and of the effective plastic strain per quadrature
 * point, double -- 448 B per element where the reference keeps 1664 B (strains, stresses, two plastic strains, two ep).
 *
 * Two rules of the reference, and one deviation: an element whose eight nodes are all "zero" (every |component| <= 1e-20,
 * get_displacements) is not advanced.  Where the plastic multiplier dLambda == 0 the state is KEPT AS IT IS: the reference
 * adds 0 * dfds there, the same number wherever J2 > 0 but NaN where J2 == 0 (a rigid translation poisons its plastic
 * strain); the library does not reproduce that NaN.
 *
 * hq_nonlinear_set: between steps; the state starts at 0; set again replaces plan and state; nelems == 0 is valid (the context
 * then enqueues what it did before, and refuses what a nonlinear context refuses).  It refuses, the context left as it was:
 * a scatter context, the float library, a context with nranks > 1, a linked group or any transport, a context with
 * attenuation of either kind (all HQ_ERR_STATE); an unknown model, ids out of range or not strictly ascending, a constant
 * that is not finite, h <= 0, mu < 0, k < 0, alpha != 0 under von Mises (all HQ_ERR_ARG).  On a nonlinear context
 * hq_comm_init*, hq_group_link and hq_attenuation_set* refuse (HQ_ERR_STATE).
 * hq_nonlinear_info: out = {nonlinear elements, touched nodes, device bytes added, 0}; all 0 without.
 * hq_nonlinear_fetch / _load: pstrain [nelems][8][6] and ep [nelems][8] in the caller's element order and the reference's
 * quadrature order (point j at xi[.][j] qc); fetch leaves out an array passed as NULL, load needs both and refuses a value
 * that is not finite (HQ_ERR_ARG).  hq_upload zeroes the state, as the reference's restart does (calloc, nonlinear.c:651-664);
 * an exact restart is hq_upload followed by hq_nonlinear_load.
 * hq_nonlinear_clear: the added bytes go; the context steps as it did before.
 * Device bytes added, exactly (hq_info.device_bytes grows by it); 0 for nelems == 0, else with Enlpad = nelems rounded up to 64,
 * T = touched nodes (the nodes of the nonlinear elements and the anchors of the hanging ones among them), A = distinct anchors
 * and H = (hanging node, anchor) pairs of the touched hanging nodes:
 *     448 Enlpad            (state, double [7][8][Enlpad])
 *   + 192 Enlpad            (corner forces, double [3][8][Enlpad])
 *   +  48 Enlpad + 32 Enlpad (constants [6][Enlpad], node ids [8][Enlpad])
 *   +   4 (T + 1) + 32 nelems (the node -> (element, corner) table)
 *   +  36 T                 (dF [T][3], the mass n_t[n][0], the node id)
 *   +   8 A + 4 + 8 H       (dF's distribution tables; nothing where no touched node hangs)
 * hq_nonlinear_plan_check: host only -- report = {nonlinear elements, touched nodes, the bytes above, faults}: the touched-node
 * list (ascending, every corner under its own node, every listed node needed), the touched hanging nodes against the mesh's
 * table, and hq_attenuation_split_plan_check's counts on the tables.  hq_nonlinear_plan_tables hands out the tables in the
 * numbering hq_create gives `desc` (counts = {T, T + 1, 8 nelems, H}; tnode [T], epos [nelems], nptr, nent, sd [H][3] on
 * touched-node indices; a NULL array is left out) and hq_nonlinear_table_faults counts the faults of tables given to it.
 * Not here: rate-dependent plasticity (compute_dLambdaII's pow branch); geostatic loading, gravity and bottom reactions;
 * nonlinear station files and yield statistics; the scatter variant, the float library, partitions and the reference-link
 * stub.
 */
#ifndef HQ_NL_MODELS
#define HQ_NL_MODELS
enum { HQ_NL_VONMISES = 1, HQ_NL_DRUCKERPRAGER = 2 };
#endif
typedef struct {
    int32_t model, nelems;
    const int32_t* elems;            /* nonlinear elements, caller's numbering, strictly ascending */
    const double* cons;              /* [nelems][6] h, mu, lambda, alpha, k, hardening modulus     */
} hq_nonlinear_desc;
HQ_API int hq_nonlinear_set(hq_ctx* ctx, const hq_nonlinear_desc* desc);
HQ_API int hq_nonlinear_info(hq_ctx* ctx, int64_t out[4]);
HQ_API int hq_nonlinear_fetch(hq_ctx* ctx, double* pstrain, double* ep);
HQ_API int hq_nonlinear_load(hq_ctx* ctx, const double* pstrain, const double* ep);
HQ_API int hq_nonlinear_clear(hq_ctx* ctx);
HQ_API int hq_nonlinear_plan_check(const hq_desc* desc, const hq_nonlinear_desc* nl, int64_t report[4]);
HQ_API int hq_nonlinear_plan_tables(const hq_desc* desc, const hq_nonlinear_desc* nl, int32_t* tnode, int32_t* epos, int32_t* nptr,
                                    int32_t* nent, int32_t* sd, int64_t counts[4]);
HQ_API int hq_nonlinear_table_faults(const hq_desc* desc, const hq_nonlinear_desc* nl, const int32_t* tnode, const int32_t* epos,
                                     const int32_t* nptr, const int32_t* nent, const int32_t* sd, int64_t nsd, int64_t* faults);

/*
 * Single phases, for per-function parity tests against the reference loops
 * (scatter variant only; the patch variant fuses them):
 *   hq_phase_force : force += stiffness + damping element forces of the
 *                    current (tm1,tm2), after the swap and the source force
 *   hq_phase_update: solver_compute_displacement + zeroing of force
 *   hq_download_force: copy the force accumulator [nharbored][3]
 */
HQ_API int hq_phase_force(hq_ctx* ctx);
HQ_API int hq_phase_update(hq_ctx* ctx);
HQ_API int hq_download_force(hq_ctx* ctx, double* force);

/*
 * Timed run for bench.py: enqueues nsteps like hq_run between two HIP events
 * on the context's compute stream and additionally brackets every launch of
 * the dominant kernel with events.  Returns wall ms for the whole batch and
 * the average ms per launch of the dominant kernel.
 */
HQ_API int hq_run_timed(hq_ctx* ctx, int32_t nsteps, double* total_ms, double* kernel_ms_avg);

/*
 * Host-only self-check of the patch planner (needs no device; eTable / nTable are not read): refuses a description
 * hq_create refuses, plans `desc` WITHOUT bricks -- every node a patch node, hq_create's plan under
 * hq_options.no_bricks or without node_xyz -- and verifies the element rows, accumulate flags and node coverage of
 * every patch.
 * report = {patches, lattice patches, (patch, element) pairs, distinct element-row blocks,
 *           LDS passes of the gathers, gather instructions (per 32-lane group), gather passes of the
 *           lattice patches (23 groups x 8 corners each when free of bank conflicts), faults}.
 */
HQ_API int hq_plan_check(const hq_desc* desc, int64_t report[8]);

/*
 * Host-only self-check of what hq_k_patch_stencil reads (needs no device; desc->node_xyz required, eTable / nTable are
 * not read), on the plan WITHOUT bricks that hq_plan_check checks: every patch-shape
 * table (lattice rows, element masks, boundary lists) against the mesh's connectivity, and the element-matrix blocks
 * of the boundary phase against the kernels' own element arithmetic.
 * report = {patches, patches with a table, full lattices among them, boundary nodes, element corners checked, faults}.
 */
HQ_API int hq_stencil_plan_check(const hq_desc* desc, int64_t report[6]);

/*
 * Host-only self-check of the brick planner (needs no device; desc->node_xyz required): plans the bricks -- the bulk
 * of uniformly refined, homogeneous regions, stepped by hq_k_brick on a tile-major node numbering of the device's own
 * -- with hq_create's own host half (it refuses what hq_create refuses) and verifies them, and the patches planned
 * behind them on the renumbered description, against the mesh's connectivity alone: permutation, coverage, the eight
 * equal elements and the dashpot-free n_t row of every brick node, and every neighbour the kernel will read.
 * report = {brick nodes, tile columns, units, units with one n_t row, units with per-element coefficients
 *           (hq_k_brick_het), neighbours checked, patch nodes, faults}.
 */
HQ_API int hq_brick_plan_check(const hq_desc* desc, int64_t report[8]);
/* ... with report[8] = units that own only part of their tile (ragged, one n_t row), report[9] = the nodes those own,
 * report[10] / [11] = the same for the ragged units of the per-element kernel, report[12] = the per-element units kept in
 * the packed form (desc->edata given and every coefficient reproduced bit for bit), ragged ones included,
 * report[13] / [14] / [15] = the smallest nx, ny and np (planes) of any unit, report[16] = the fewest nodes a ragged unit
 * of either kernel owns in one of its planes (0: there is no ragged unit), report[17] = units of ONE plane that carry
 * both z faces; n >= 8 entries, those past the last one named here are zeroed */
HQ_API int hq_brick_plan_check_n(const hq_desc* desc, int64_t* report, int32_t n);

/*
 * Host-only: the sixteen coefficients {p1[6], p2[6], q1[2], q2[2]} of the assembled 27-point stencil
 * S = c1 S1 + c2 S2 that hq_k_patch_stencil applies on uniform lattice patches -- the same operator
 * -(c1 K1 + c2 K2) that compute_addforce_effective + damping_addforce apply element by element
 * (stiffness.c:180-237, damping.c:29-103), assembled per node.  Diagonal blocks S[d][a][a]: class
 * (d_a != 0) + 2 x (number of the other two offsets that are non-zero); off-diagonal S[d][a][b] =
 * q[d_c != 0] sgn(d_a) sgn(d_b).  HQ_ERR_STATE if the symmetry check of the tables failed.
 */
HQ_API int hq_stencil_coefficients(double out[16]);

/* Name of the dominant kernel as it appears in rocprofv3 kernel traces. */
HQ_API const char* hq_dominant_kernel(hq_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* HQ_SOLVER_H */
