/*
 * hq_engine.hip -- MI355X (gfx950) engine behind include/hq_solver.h.
 *
 * Device-resident restatement of the body of solver_run()
 * (quake/forward/psolve.c:4265-4319) for one mesh partition:
 *
 *   source force      compute_addforce_s               psolve.c:5912-5928
 *   element force     compute_addforce_effective       stiffness.c:180-237
 *                   + damping_addforce                 damping.c:29-103   (fused, hq_kernels.h)
 *   hanging nodes     compute_adjust                   psolve.c:5936-6039
 *   halo exchange     schedule_senddata                psolve.c:4945-5079 (RCCL send/recv)
 *   nodal update      solver_compute_displacement      psolve.c:4072-4114
 *
 * Two element-kernel variants:
 *   SCATTER  one thread per element, SoA connectivity, fp64 hardware atomics
 *            into the nodal force array, separate nodal-update kernel.  Works
 *            for any mesh/partition (hanging nodes, halo exchange).
 *   PATCH    owner-computes: the Z-ordered node range is cut into patches; a
 *            workgroup stages the displacements of its patch (+ one ring of
 *            neighbours) in LDS, evaluates every element touching the patch,
 *            accumulates forces of OWNED nodes in LDS and finishes the
 *            central-difference update in the same kernel.  The force vector
 *            never exists in HBM.  (see hq_patch.h)
 *
 * There is no CPU fallback: without a gfx950 device hq_create() fails with
 * HQ_ERR_NODEVICE.
 */
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <vector>

#define HQ_SOLVER_IMPLEMENTATION 1
#include "../../include/hq_solver.h"
#include "hq_devmem.h"
#include "hq_kernels.h"
#include "hq_opts.h"
#include "hq_cadence.h"
#include "hq_peak.h"
#include "hq_cumul.h"
#include "hq_deform.h"
#include "hq_sdof.h"
#include "hq_atten.h"
#define HQ_SAMPLE_REAL hq_real
#include "hq_sample.h"
#include "hq_patch.h"
#include "hq_brick.h"

/* (hq_fail, HQ_HIP, HQ_TRY: hq_devmem.h) */
extern "C" const char* hq_last_error(void) { return g_err; }

/* ------------------------------------------------------------------------ */
/* RCCL, resolved lazily so that single-GPU use never loads it              */
/* ------------------------------------------------------------------------ */

/* The prototypes, the id's size and the datatype enumerators are rccl.h's OWN (compile time); only the library is
 * looked up at run time.  A header that moved an enumerator or changed a signature breaks the build, not a halo. */
#include <rccl/rccl.h>
typedef ncclUniqueId hq_nccl_id;
typedef ncclComm_t hq_nccl_comm;
struct hq_rccl {
    void* handle;
    decltype(&ncclGetUniqueId) GetUniqueId;
    decltype(&ncclCommInitRank) CommInitRank;
    decltype(&ncclCommDestroy) CommDestroy;
    decltype(&ncclSend) Send;
    decltype(&ncclRecv) Recv;
    decltype(&ncclGroupStart) GroupStart;
    decltype(&ncclGroupEnd) GroupEnd;
    decltype(&ncclGetErrorString) GetErrorString;
};
static hq_rccl g_rccl = {};
static const ncclDataType_t HQ_NCCL_INT64 = ncclInt64, HQ_NCCL_DOUBLE = ncclFloat64;
static_assert(sizeof(hq_nccl_id) == 128, "hq_comm_unique_id hands out 128 bytes (include/hq_solver.h)");
static_assert(sizeof(double) == 8 && sizeof(int64_t) == 8, "halo records are ncclFloat64, check words ncclInt64");

static int hq_rccl_load(void)
{
    if (g_rccl.handle) return HQ_OK;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return hq_fail(HQ_ERR_COMM, "cannot load librccl: %s", dlerror());
#define HQ_SYM(field, name)                                                     \
    *(void**)(&g_rccl.field) = dlsym(h, name);                                  \
    if (!g_rccl.field) return hq_fail(HQ_ERR_COMM, "librccl lacks %s", name);
    HQ_SYM(GetUniqueId, "ncclGetUniqueId")
    HQ_SYM(CommInitRank, "ncclCommInitRank")
    HQ_SYM(CommDestroy, "ncclCommDestroy")
    HQ_SYM(Send, "ncclSend")
    HQ_SYM(Recv, "ncclRecv")
    HQ_SYM(GroupStart, "ncclGroupStart")
    HQ_SYM(GroupEnd, "ncclGroupEnd")
    HQ_SYM(GetErrorString, "ncclGetErrorString")
#undef HQ_SYM
    g_rccl.handle = h;
    return HQ_OK;
}

#define HQ_NCCL(call)                                                                     \
    do {                                                                                  \
        ncclResult_t r_ = (call);                                                         \
        if (r_ != ncclSuccess) return hq_fail(HQ_ERR_COMM, "%s: %s", #call, g_rccl.GetErrorString(r_)); \
    } while (0)

static inline unsigned hq_blocks(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

/*
 * compute_adjust DISTRIBUTION (psolve.c:5942-5987) without atomics and in ONE summation order: the entries are
 * grouped by the anchor they add to (CSR, host-built), inside an anchor in the order of the reference's loop --
 * hanging nodes in table order, their anchors in list order -- so an anchor several hanging nodes hang on gets its
 * parts in the same order on every run.  Anchors are never hanging nodes themselves (hq_create refuses that), so no
 * row is read and written in the same launch.  ids: node ids (scatter variant, force table), interface slots or the
 * rows of a correction pass.
 */
__global__ void hq_k_distribute(int32_t ndst, const int32_t* __restrict__ dst, const int32_t* __restrict__ ptr,
                                const int32_t* __restrict__ src, const int32_t* __restrict__ deps, double* __restrict__ table)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ndst * 3) return;
    int k = t / 3, d = t - 3 * k;
    double* p = &table[3 * (int64_t)dst[k] + d];
    double v = *p;
    for (int32_t q = ptr[k]; q < ptr[k + 1]; q++) v += table[3 * (int64_t)src[q] + d] / (double)(uint32_t)deps[q];
    *p = v;
}

/* hq_k_distribute's tables, grouped by the anchor (destination) the entries add to, and their launch: the shared hanging nodes
 * of the patch variant on the interface table (slots), all hanging nodes of the scatter variant on the force table (nodes),
 * the hanging nodes of a correction pass on its dF (hq_correction.h) */
struct hq_distribution {
    int32_t n = 0;                    /* destinations (anchors)                              */
    hq_dbuf<int32_t> d_dst;           /* [n]                                                 */
    hq_dbuf<int32_t> d_ptr;           /* [n + 1]                                             */
    hq_dbuf<int32_t> d_src;           /* [entries] hanging node (slot / id)                  */
    hq_dbuf<int32_t> d_deps;          /* [entries] its number of anchors                     */
    int64_t bytes() const { return (int64_t)(d_dst.bytes() + d_ptr.bytes() + d_src.bytes() + d_deps.bytes()); }
    /* {src, dst, deps} triples in the reference's loop order; inside an anchor the entries keep that order.  The tables are
     * counted in *ledger (NULL: uncounted); no triples: n = 0 and nothing is allocated */
    int build(const std::vector<int32_t>& sd, int64_t* ledger, hipStream_t st)
    {
        const size_t cnt = sd.size() / 3;
        *this = hq_distribution();
        if (!cnt) return HQ_OK;
        std::vector<int32_t> order(cnt);
        for (size_t i = 0; i < cnt; i++) order[i] = (int32_t)i;
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return sd[3 * (size_t)a + 1] < sd[3 * (size_t)b + 1]; });
        std::vector<int32_t> dst, ptr(1, 0), src, deps;
        for (size_t k = 0; k < cnt; k++) {
            const size_t i = (size_t)order[k];
            if (dst.empty() || dst.back() != sd[3 * i + 1]) { if (!dst.empty()) ptr.push_back((int32_t)src.size()); dst.push_back(sd[3 * i + 1]); }
            src.push_back(sd[3 * i]); deps.push_back(sd[3 * i + 2]);
        }
        ptr.push_back((int32_t)src.size());
        HQ_TRY(d_dst.put(ledger, dst, st)); HQ_TRY(d_ptr.put(ledger, ptr, st));
        HQ_TRY(d_src.put(ledger, src, st)); HQ_TRY(d_deps.put(ledger, deps, st));
        n = (int32_t)dst.size();
        return HQ_OK;
    }
    void launch(double* table, hipStream_t st) const
    {
        if (n) hq_k_distribute<<<hq_blocks(n * 3, 256), 256, 0, st>>>(n, d_dst, d_ptr, d_src, d_deps, table);
    }
};

#include "hq_atten_plan.h"
#include "hq_correction.h"
#include "hq_atten_split.h"
#include "hq_nonlin_dev.h"

/* ------------------------------------------------------------------------ */
/* context                                                                  */
/* ------------------------------------------------------------------------ */

/* BKT attenuation of a scatter context (hq_attenuation_set; hq_atten.h, hq_atten_plan.h): the slot plan and the state on the
 * device, the plan's corner table on the host for fetch / load in the reference's per-corner layout.  split: of a patch
 * context (hq_attenuation_set_split; hq_atten_split.h) -- d_w then holds the delta vectors, and c1 / c2 and the correction
 * pass exist */
struct hq_atten_dev {
    bool on = false, split = false;
    int32_t nclasses = 0, nslots = 0;
    int32_t Epad = 0;                /* the stride of eslot (split: of the correction pass as well)    */
    int64_t bytes = 0;               /* the device bytes of everything below (the headers' formulas)   */
    hq_dbuf<int32_t> d_eslot;        /* [8][Epad]                                          */
    hq_dbuf<int32_t> d_slot_node;    /* [nslots]                                           */
    hq_dbuf<int32_t> d_slot_class;   /* [nslots]                                           */
    hq_dbuf<double> d_ktab;          /* [nclasses][HQ_ATTEN_NCOEF]                         */
    hq_dbuf<double> d_mv;            /* [HQ_ATTEN_NSTATE][nslots] memory variables         */
    hq_dbuf<double> d_w;             /* [HQ_ATTEN_NW][nslots] damping vectors of this step */
    std::vector<int32_t> h_eslot, h_slot_node;
    hq_dbuf<double> d_c1, d_c2;      /* split: [E], the correction's element order         */
    hq_correction corr;              /* split: over all E elements and all N nodes         */
};

/* Nonlinear soil of a patch context (hq_nonlinear_set; hq_nonlin.h, hq_nonlin_dev.h): state, constants and node ids on the
 * device over the nonlinear elements, the correction pass over them and the nodes they touch; the place of every element of
 * the caller's list on the host, for fetch / load in the caller's order */
struct hq_nl_dev {
    bool on = false;
    int32_t model = 0, nel = 0, Enlpad = 0, nt = 0;
    int64_t bytes = 0;               /* hq_nl_bytes */
    hq_dbuf<double> d_st;            /* [7][8][Enlpad] plastic strain (6) and effective plastic strain per point */
    hq_dbuf<double> d_cons;          /* [6][Enlpad]                                                               */
    hq_dbuf<int32_t> d_lnid;         /* [8][Enlpad] device node ids                                               */
    hq_correction corr;              /* over the nel elements and the nt touched nodes, listed in corr.d_tnode    */
    std::vector<int32_t> h_epos;     /* [nel] */
};

struct hq_dev_messenger {
    int32_t procid, nodecount;
    int32_t offset;          /* first record in the packed buffer */
};

struct hq_dev_schedule {
    std::vector<hq_dev_messenger> c, s;   /* c: owners of nodes I harbor; s: sharers of nodes I own */
    hq_dbuf<int32_t> d_cmap;     /* node ids, concatenated c-list mappings           */
    hq_dbuf<int32_t> d_smap;
    int32_t* d_cmap_f = nullptr; /* the same entries as indices into the force table: views of d_cmap / d_smap (scatter: */
    int32_t* d_smap_f = nullptr; /* node ids again) or of the slot tables below (patch: interface slots)                 */
    hq_dbuf<int32_t> d_cslot, d_sslot;
    hq_dbuf<double> d_c_out;     /* contribution send   [ctotal][3]                   */
    hq_dbuf<double> d_s_out;     /* sharing      send   [stotal][3]                   */
    double*  d_c_in = nullptr;   /* sharing      recv   [ctotal][3]: views of the two buffers below, or of the IPC arena */
    double*  d_s_in = nullptr;   /* contribution recv   [stotal][3]                   */
    hq_dbuf<double> c_in_mem, s_in_mem;
    int32_t  ctotal = 0, stotal = 0;
    /* HQ_DEBUG_HALO: every record travels with the global identity of its node (psolve.c:5002-5007) */
    hq_dbuf<int64_t> d_c_out_id, d_c_in_id, d_s_out_id, d_s_in_id;
    /* in-process transport (hq_group_link): where every record of the contribution / sharing send lands in its peer's
     * receive buffer -- the pack kernel writes there directly (one kernel per exchange, no copies) */
    hq_dbuf<double*> d_c_dst, d_s_dst;
    /* host-staged transport (hq_comm_init_host): pinned mirrors of the four record buffers */
    double*  h_c_out = nullptr;
    double*  h_c_in = nullptr;
    double*  h_s_out = nullptr;
    double*  h_s_in = nullptr;
    /* ... and, under HQ_DEBUG_HALO, of the four check-word buffers */
    int64_t* h_c_out_id = nullptr;
    int64_t* h_c_in_id = nullptr;
    int64_t* h_s_out_id = nullptr;
    int64_t* h_s_in_id = nullptr;
};

struct hq_ctx {
    hq_options opts;                  /* the caller's options as hq_create_opts resolved them: per context, so that a host --
                                       * or a test process -- can differ between contexts; -1 = the library's default */
    int device = 0;
    hipStream_t stream = nullptr;
    int32_t E = 0, N = 0, ldnnum = 0;
    int32_t variant = HQ_VARIANT_SCATTER;
    int32_t step = 0;
    int32_t rank = 0, nranks = 1;
    double dt = 0, dt2 = 0;
    int64_t bytes = 0;
    int64_t h2d_bytes = 0, d2h_bytes = 0;    /* what crossed PCIe through the entry points since hq_create returned (hq_info) */
    hq_dbuf<int32_t> d_gather_ids;           /* hq_gather's scratch (not counted in `bytes`) */
    hq_dbuf<hq_real> d_gather_out;
    int32_t gather_cap = 0;

    /* element data, SoA */
    int32_t Epad = 0;
    hq_dbuf<int32_t> d_lnid;        /* [8][Epad] */
    hq_dbuf<double> d_c1, d_c2, d_beta;
    bool etable_damped = false;     /* some c3 or c4 of the caller's eTable is not 0 */
    hq_atten_dev att;
    hq_nl_dev nl;
    /* patch variant, for hq_attenuation_set_split (which gets no mesh): the element table in device numbering and the caller's
     * element order, c1 / c2 and n_t[n][0], kept on the HOST (48 B per element + 8 B per node; nothing on the device) */
    std::vector<int32_t> h_lnid;
    std::vector<double> h_c1, h_c2, h_mass;
    hipStream_t astream = nullptr;  /* the correction chain's head beside the step (from the first hq_attenuation_set_split on) */
    hipEvent_t ev_att_fork = nullptr, ev_att_done = nullptr;
    /* node data */
    double* d_nt = nullptr;         /* [N][7]; behind bricks only the rows of the nodes nt_first .. N - 1 exist (d_nt_rows), */
    hq_dbuf<double> d_nt_rows;      /* d_nt = d_nt_rows - 7 nt_first: no kernel reads a brick node's 7-double row */
    hq_dbuf<hq_real> d_u[3];        /* the state in solver_float (psolve.h:60-64) */
    int now = 0, prev = 1, spare = 2;
    hq_dbuf<double> d_force;
    /* source window */
    int32_t nloaded = 0, src_step0 = 0, src_nsteps = 0;
    hq_dbuf<int32_t> d_loaded;
    hq_dbuf<double> d_F;
    std::vector<int32_t> h_loaded;  /* the loaded nodes (device numbering) of the window in place, and the */
    size_t F_capacity = 0;          /* doubles d_F holds: the next window of the same nodes reuses both    */
    /* hanging nodes */
    hq_dbuf<int32_t> d_dn_id, d_dn_ptr, d_dn_anchor;
    /* halo */
    hq_dev_schedule an, dn;
    hq_nccl_comm comm = nullptr;
    hq_host_exchange_fn host_xchg = nullptr; /* host-staged transport (hq_comm_init_host): the caller's MPI, ... */
    void* host_user = nullptr;
    std::vector<hq_ctx*>* group = nullptr;   /* in-process transport (hq_group_link) */
    bool group_owner = false;
    bool share_packed = false;               /* this step's hq_k_interface_update wrote the sharing records as well */
    struct hq_ipc_state* ipc = nullptr;      /* device-to-device transport between processes (hq_comm_init_ipc) */
    hipEvent_t ev_sent = nullptr;
    /* patch variant with an interface: the exchange chain runs on its own stream
     * beside the interior patches */
    hipStream_t cstream = nullptr;
    hipEvent_t ev_bnd = nullptr, ev_shared = nullptr, ev_an_shared = nullptr, ev_assigned = nullptr;
    /* HQ_BRICK_STREAM=1: the bricks on a stream of their own beside the patches (hq_use_brick_stream; opt-in) */
    hipStream_t bstream = nullptr;
    hipEvent_t ev_patches = nullptr, ev_bricks = nullptr;
    bool overlap = false;             /* exchange chain on cstream beside the interior patches               */
    bool stream_masked = false;       /* the compute stream leaves reserve_cus CUs to the exchange stream (hq_mask_compute_stream) */
    bool can_overlap = false;         /* the stream and events for it exist (hq_setup_interface)             */
    int reserve_cus = 8;              /* CUs the interior launch leaves to the exchange chain (HQ_RESERVE_CUS) */
    /* patch variant: nodes on the partition interface */
    int32_t nI = 0, nOI = 0;
    hq_dbuf<double> d_iforce;         /* [nI][3] partial / summed force of interface nodes */
    hq_dbuf<int32_t> d_oi_node;       /* [nOI] interface nodes I own                        */
    hq_dbuf<int32_t> d_oi_slot;
    hq_dbuf<int32_t> d_oi_ptr;        /* [nOI+1] CSR: records of an.d_s_in to add, in       */
    hq_dbuf<int32_t> d_oi_pos;        /*         messenger order (fixed summation order)    */
    hq_dbuf<int32_t> d_oi_fc;         /* [nOI] first record | number of records << 24       */
    /* compute_adjust DISTRIBUTION: the shared hanging nodes of the patch variant on the interface table (slots), all
     * hanging nodes of the scatter variant on the force table (nodes) */
    hq_distribution dist;
    /* patch variant */
    hq_patch_plan plan;
    /* bricks (hq_brick.h): the device numbers the nodes its own way -- tile columns first -- and every entry point
     * that takes or returns node ids or node-ordered arrays translates; perm empty: identity */
    hq_brick_plan bricks;
    std::vector<int32_t> perm;        /* caller's node id -> device id */
    /* HQ_DEBUG_HALO (the reference's -DDEBUG exchange, psolve.c:5002-5007, 5058-5069) */
    bool debug_halo = false;
    /* HQ_DEBUG_HALO over the IPC and the host-staged transport: exchanges counted on both sides (part of the check word) */
    unsigned long long dbg_send_epoch[4] = { 0, 0, 0, 0 }, dbg_recv_epoch[4] = { 0, 0, 0, 0 };
    hq_dbuf<int64_t> d_gkey;          /* [N] global identity of every harbored node          */
    hq_dbuf<int32_t> d_halo_err;      /* [4] records whose identity did not match; non-finite values seen by hq_check_finite;
                                       * [2] IPC waits that timed out */
    /* device-side phase split (hq_options.phase_timing; every hq_run_timed batch): per step six events -- step start,
     * shell end, interior start / end, chain start / end -- in a ring of slots harvested when they are reused or asked for
     * (hq_info.t_*_us: the library's print_timing_stat, psolve.c:6041-6266) */
    enum { HQ_CLK_STEP0 = 0, HQ_CLK_SHELL1, HQ_CLK_INT0, HQ_CLK_INT1, HQ_CLK_CHAIN0, HQ_CLK_CHAIN1, HQ_CLK_N, HQ_CLK_SLOTS = 64 };
    struct hq_clock_slot { hipEvent_t e[HQ_CLK_N] = {}; bool used[HQ_CLK_N] = {}; bool pending = false; };
    bool clock_skip = false;          /* this step is not one of a timed batch's sampled steps */
    std::vector<hq_clock_slot> clock;
    size_t clock_at = 0;
    double clk_us[5] = { 0, 0, 0, 0, 0 };   /* step, shell, interior, chain, chain behind the interior's end */
    int64_t clk_steps = 0;
    /* device outputs (recorders, trackers, snapshots).  hq_outputs.h, included ahead of hq_phase, DEFINES the structs: no code
     * above that include may touch recs, peaks, specs, cums, deforms or snaps.  ev_output: recorded behind a due step's launches for the streams to wait on */
    struct hq_output; struct hq_recorder; struct hq_tracker; struct hq_peak_tracker; struct hq_spec_tracker; struct hq_cum_tracker; struct hq_deform_tracker; struct hq_snapshot;
    std::vector<hq_recorder> recs;
    int32_t rec_next_id = 0;
    std::vector<hq_peak_tracker> peaks;
    int32_t peak_next_id = 0;
    std::vector<hq_spec_tracker> specs;
    int32_t spec_next_id = 0;
    std::vector<hq_cum_tracker> cums;
    int32_t cum_next_id = 0;
    std::vector<hq_deform_tracker> deforms;
    int32_t deform_next_id = 0;
    std::vector<hq_snapshot> snaps;
    int32_t snap_next_id = 0;
    hipStream_t sstream = nullptr;              /* the snapshots' copy stream: from the first hq_snapshot_add on */
    hipEvent_t ev_output = nullptr;
    /* timing */
    std::vector<hipEvent_t> ev;     /* per-launch marks */
    hipEvent_t ev_span[2] = { nullptr, nullptr };
    bool timing = false;
    size_t ev_used = 0;
};

/*
 * hq_comm_init_ipc: what a rank exports (one fixed-size blob, all-gathered by the caller's transport) and what it keeps.
 * Exchange x = 0 anchored-node contribution (received in an.d_s_in), 1 anchored-node sharing (an.d_c_in),
 * 2 dangling-node contribution (dn.d_s_in), 3 dangling-node sharing (dn.d_c_in) -- the `tag` of the host-staged transport.
 */
enum { HQ_IPC_MAXNB = 64, HQ_IPC_MAGIC = 0x48514950 /* "HQIP" */ };
struct hq_ipc_blob {
    uint32_t magic, version;
    int32_t rank, nranks, device, pid;
    int32_t coarse, reserved;                        /* reserved: the arena's dump row (in doubles), loopback only      */
    char busid[32];                                  /* PCI bus id of the device: device ordinals differ between processes */
    uint64_t arena_bytes, arena_addr;                /* arena_addr: usable by members of the exporting process only */
    hipIpcMemHandle_t mem;
    uint64_t buf_off[4];                             /* receive buffer of exchange x in the arena (bytes)            */
    uint64_t flag_off;                               /* flags [4][HQ_IPC_MAXNB] uint64 in the arena (bytes)          */
    uint64_t id_off[4];                              /* HQ_DEBUG_HALO: check words [records] int64 of exchange x (bytes); 0: none */
    int32_t nrecv[4];
    struct { int32_t procid, offset, count; } recv[4][HQ_IPC_MAXNB];
};
static_assert(sizeof(hq_ipc_blob) <= HQ_IPC_BLOB_BYTES, "hq_ipc_blob must fit HQ_IPC_BLOB_BYTES");

struct hq_ipc_state {
    void* arena = nullptr;
    size_t arena_bytes = 0;
    bool coarse = false, ready = false, loopback = false;
    int arena_kind = 0;                              /* 0 fine-grained, 1 uncached, 2 coarse-grained */
    hq_ipc_blob mine;
    std::vector<void*> opened;                       /* hipIpcOpenMemHandle results to close */
    unsigned long long* d_flags = nullptr;           /* in the arena */
    hq_dbuf<double*> d_dst[4];                       /* where every send record of exchange x lands */
    hq_dbuf<unsigned long long*> d_sig[4];           /* the flags exchange x raises at its peers     */
    hq_dbuf<int64_t*> d_dst_id[4];                   /* HQ_DEBUG_HALO: where every record's check word lands */
    int64_t* d_in_id[4] = { nullptr, nullptr, nullptr, nullptr };           /* ... and where this rank's arrive (in the arena)      */
    int32_t nsig[4] = { 0, 0, 0, 0 };
    unsigned long long wait_mask[4] = { 0, 0, 0, 0 };
    unsigned long long send_epoch[4] = { 0, 0, 0, 0 }, recv_epoch[4] = { 0, 0, 0, 0 };
    hq_dbuf<uint32_t> d_done;                        /* [4] last-block counters (not counted) */
    unsigned long long timeout_ticks = 2000000000ull; /* 20 s of the 100 MHz clock (HQ_IPC_TIMEOUT_MS) */
    unsigned long long delay_ticks = 0;              /* loopback only: flags raised this late (HQ_LOOPBACK_DELAY_US) */
};

/* ------------------------------------------------------------------------ */
/* kernels: scatter variant                                                 */
/* ------------------------------------------------------------------------ */

/* force[lnid] = F * dt^2 (assignment): compute_addforce_s, psolve.c:5917-5927 */
__global__ void hq_k_source(int32_t nloaded, const int32_t* __restrict__ loaded,
                            const double* __restrict__ F, double dt2, double* __restrict__ force)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < nloaded * 3) {
        int i = t / 3, d = t - 3 * i;
        force[3 * (int64_t)loaded[i] + d] = F[t] * dt2;
    }
}

/*
 * One thread per element; connectivity and coefficients are SoA so a wave
 * reads them as contiguous 256-/512-byte rows.  Nodal displacements are
 * gathered from the Z-ordered AoS node arrays (neighbouring elements share
 * cache lines) and the 24 force components go out as fp64 hardware atomics.
 */
__global__ void __launch_bounds__(256)
hq_k_element_scatter(int32_t E, int32_t Epad, const int32_t* __restrict__ lnid,
                     const double* __restrict__ c1v, const double* __restrict__ c2v,
                     const double* __restrict__ betav, const hq_real* __restrict__ u1,
                     const hq_real* __restrict__ u2, double* __restrict__ force)
{
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const double beta = betav[e];
    int32_t id[8];
    double X[8], Y[8], Z[8];
#pragma unroll
    for (int n = 0; n < 8; n++) id[n] = lnid[(int64_t)n * Epad + e];
#pragma unroll
    for (int n = 0; n < 8; n++) {
        const hq_real* p1 = u1 + 3 * (int64_t)id[n];
        const hq_real* p2 = u2 + 3 * (int64_t)id[n];
        double a0 = p1[0], a1 = p1[1], a2 = p1[2];
        X[n] = a0 + beta * (a0 - p2[0]);
        Y[n] = a1 + beta * (a1 - p2[1]);
        Z[n] = a2 + beta * (a2 - p2[2]);
    }
    hq_element_force(X, Y, Z, c1v[e], c2v[e]);
#pragma unroll
    for (int n = 0; n < 8; n++) {
        double* f = force + 3 * (int64_t)id[n];
        unsafeAtomicAdd(f + 0, X[n]);
        unsafeAtomicAdd(f + 1, Y[n]);
        unsafeAtomicAdd(f + 2, Z[n]);
    }
}

/*
 * BKT attenuation, first half (calc_conv and the damping vectors of constant_Q_addforce, damping.c:110-371; the text is
 * hq_atten.h's): one thread per (node, class) slot.  State and damping vectors are SoA [row][nslots], so a wave reads and
 * writes 512-byte rows; slots are node-major, so the six field values of consecutive slots are consecutive (or the same)
 * 24-byte rows.  Per slot: 48 B of fields, 96 B of memory variables read and written, 48 B of damping vectors written.
 * The class's 18 doubles come through the scalar cache where the whole wave is of one class (nearly every wave).
 */
static __device__ __forceinline__ void hq_atten_slot(int32_t s, int64_t nslots, const double* __restrict__ k,
                                                     const hq_real* __restrict__ p1, const hq_real* __restrict__ p2,
                                                     double* __restrict__ mv, double* __restrict__ w)
{
#pragma unroll
    for (int d = 0; d < 3; d++) {
        double f[HQ_ATTEN_NVAR], ws, wk;
#pragma unroll
        for (int v = 0; v < HQ_ATTEN_NVAR; v++) f[v] = mv[(int64_t)(3 * v + d) * nslots + s];
        hq_atten_advance((double)p1[d], (double)p2[d], k, f, 1, &ws, &wk);
#pragma unroll
        for (int v = 0; v < HQ_ATTEN_NVAR; v++) mv[(int64_t)(3 * v + d) * nslots + s] = f[v];
        w[(int64_t)d * nslots + s] = ws;
        w[(int64_t)(3 + d) * nslots + s] = wk;
    }
}

__global__ void __launch_bounds__(256)
hq_k_atten_advance(int32_t nslots, const int32_t* __restrict__ slot_node, const int32_t* __restrict__ slot_class,
                   const double* __restrict__ ktab, const hq_real* __restrict__ u1, const hq_real* __restrict__ u2,
                   double* __restrict__ mv, double* __restrict__ w)
{
    const int32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nslots) return;
    const int64_t row = 3 * (int64_t)slot_node[s];
    const int32_t cls = slot_class[s];
    const int32_t cls0 = __builtin_amdgcn_readfirstlane(cls);
    if (__all(cls == cls0)) hq_atten_slot(s, nslots, ktab + HQ_ATTEN_NCOEF * cls0, u1 + row, u2 + row, mv, w);
    else hq_atten_slot(s, nslots, ktab + HQ_ATTEN_NCOEF * cls, u1 + row, u2 + row, mv, w);
}

/*
 * BKT attenuation, second half (damping.c:373-410): one thread per element gathers the shear and dilatation damping
 * vectors at its eight slots (SoA rows: neighbouring elements share cache lines as they do in the node arrays), runs the
 * fused butterfly and adds the 24 force components with fp64 hardware atomics, as hq_k_element_scatter does.  beta is
 * not read: under BKT c3 = c4 = 0 (compute_setab, psolve.c:5869).
 */
__global__ void __launch_bounds__(256)
hq_k_element_bkt(int32_t E, int32_t Epad, int32_t nslots, const int32_t* __restrict__ lnid, const int32_t* __restrict__ eslot,
                 const double* __restrict__ c1v, const double* __restrict__ c2v, const double* __restrict__ w,
                 double* __restrict__ force)
{
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    double X[8], Y[8], Z[8], P[8], Q[8], R[8];
#pragma unroll
    for (int n = 0; n < 8; n++) {
        const double* ws = w + eslot[(int64_t)n * Epad + e];
        X[n] = ws[0];
        Y[n] = ws[(int64_t)nslots];
        Z[n] = ws[2 * (int64_t)nslots];
        P[n] = ws[3 * (int64_t)nslots];
        Q[n] = ws[4 * (int64_t)nslots];
        R[n] = ws[5 * (int64_t)nslots];
    }
    hq_element_force_bkt(X, Y, Z, P, Q, R, c1v[e], c2v[e]);
#pragma unroll
    for (int n = 0; n < 8; n++) {
        double* f = force + 3 * (int64_t)lnid[(int64_t)n * Epad + e];
        unsafeAtomicAdd(f + 0, X[n]);
        unsafeAtomicAdd(f + 1, Y[n]);
        unsafeAtomicAdd(f + 2, Z[n]);
    }
}

/* solver_compute_displacement (psolve.c:4078-4111): one thread per scalar */
__global__ void __launch_bounds__(256)
hq_k_update(int64_t n3, const double* __restrict__ nt, const hq_real* __restrict__ u1,
            hq_real* __restrict__ u2, double* __restrict__ force)
{
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n3) return;
    int64_t n = t / 3;
    int d = (int)(t - 3 * n);
    const double* np = nt + 7 * n;
    double f = force[t];
    f += np[1 + d] * (double)u1[t] - np[4 + d] * (double)u2[t];
    u2[t] = (hq_real)(f / np[0]);
    force[t] = 0.0;
}

/* compute_adjust ASSIGNMENT (psolve.c:5992-6035) */
__global__ void hq_k_adjust_assign(int32_t ldnnum, const int32_t* __restrict__ dn_id,
                                   const int32_t* __restrict__ dn_ptr,
                                   const int32_t* __restrict__ dn_anchor, hq_real* __restrict__ table)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ldnnum * 3) return;
    int k = t / 3, d = t - 3 * k;
    int32_t lo = dn_ptr[k], hi = dn_ptr[k + 1];
    double deps = (double)(uint32_t)(hi - lo);
    double s = 0.0;
    for (int32_t p = lo; p < hi; p++) s += (double)table[3 * (int64_t)dn_anchor[p] + d] / deps;
    table[3 * (int64_t)dn_id[k] + d] = (hq_real)s;
}

/* schedule_senddata pack (psolve.c:4985-5011) / unpack (:5035-5073) */
/* (T: the table's type -- forces are doubles, displacements hq_real; the records travel as doubles either way) */
template <typename T>
__global__ void hq_k_pack(int32_t count, const int32_t* __restrict__ map,
                          const T* __restrict__ table, double* __restrict__ out)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count * 3) return;
    int i = t / 3, d = t - 3 * i;
    out[t] = (double)table[3 * (int64_t)map[i] + d];
}

/* in-process transport: record i goes where its peer expects it (dst[i]: base of the record in the peer's buffer) */
template <typename T>
__global__ void hq_k_pack_to_peers(int32_t count, const int32_t* __restrict__ map, const T* __restrict__ table,
                                   double* const* __restrict__ dst)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count * 3) return;
    int i = t / 3, d = t - 3 * i;
    dst[i][d] = (double)table[3 * (int64_t)map[i] + d];
}

/*
 * Device-to-device transport between PROCESSES (hq_comm_init_ipc): the same direct peer stores, into receive buffers
 * the peers exported through HIP IPC, ordered by epoch flags in the receivers' arenas instead of HIP events -- an event
 * cannot order streams of two processes without a host handshake per exchange, a counter in memory can.
 * Hand-off (MI355X_MICROARCH.md, "valid forms"): the records leave as system-scope (sc0 sc1, write-through) stores, every
 * storing wave waits for its stores (s_waitcnt vmcnt(0)), and behind a workgroup barrier one lane adds to a device-scope
 * counter; the workgroup whose add comes last stores the epoch of this exchange to one flag per receiving peer.  No
 * fence: a release fence is an L2 write-back and an acquire an L2 invalidate, per workgroup and per poll -- they halved
 * the brick launch running beside them (first trace of round 4).  The receiver polls with relaxed system-scope loads
 * and reads the records in a LATER kernel (its start is the acquire); the arena is fine-grained memory, which no L2
 * holds stale.
 */
/* loopback diagnostic only (HQ_LOOPBACK_DELAY_US): the flags are raised `ticks` of the 100 MHz clock late, as if the
 * records had a link to cross -- how much transport latency does a rank's step hide? */
static __device__ __forceinline__ void hq_ipc_delay(unsigned long long ticks)
{
    if (!ticks) return;
    const unsigned long long t0 = wall_clock64();
    while ((unsigned long long)wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}

template <typename T>
__global__ void hq_k_pack_to_peers_sig(int32_t count, const int32_t* __restrict__ map, const T* __restrict__ table,
                                       double* const* __restrict__ dst, uint32_t* __restrict__ done, int32_t nsig,
                                       unsigned long long* const* __restrict__ sig, unsigned long long epoch,
                                       unsigned long long delay_ticks)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < count * 3) {
        int i = t / 3, d = t - 3 * i;
        __hip_atomic_store(dst[i] + d, (double)table[3 * (int64_t)map[i] + d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    __shared__ int s_last;
    if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
    __syncthreads();
    if (!s_last) return;
    if (threadIdx.x == 0) __hip_atomic_store(done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((int)threadIdx.x < nsig) {
        hq_ipc_delay(delay_ticks);
        __hip_atomic_store(sig[threadIdx.x], epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

/* the receiving side: one lane per sending peer polls (relaxed system-scope loads, s_sleep between them) until that
 * peer's flag has reached this exchange's epoch; a wait that lasts longer than `timeout_ticks` of the 100 MHz wall clock
 * gives up and counts an error that hq_sync reports -- a rank that died must not leave its neighbours' GPUs spinning
 * for ever.  The records are read by the kernels enqueued behind this one. */
__global__ void hq_k_ipc_wait(const unsigned long long* __restrict__ flags, unsigned long long mask, unsigned long long epoch,
                              unsigned long long timeout_ticks, int32_t* __restrict__ err)
{
    const int j = threadIdx.x;
    if (!((mask >> j) & 1ull)) return;
    const unsigned long long t0 = wall_clock64();
    while (__hip_atomic_load(&flags[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < epoch) {
        __builtin_amdgcn_s_sleep(16);
        if (wall_clock64() - t0 > timeout_ticks) { atomicAdd(err, 1); return; }
    }
}

template <typename T>
__global__ void hq_k_unpack(int32_t count, const int32_t* __restrict__ map,
                            const double* __restrict__ in, T* __restrict__ table, int add)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count * 3) return;
    int i = t / 3, d = t - 3 * i;
    T* p = &table[3 * (int64_t)map[i] + d];
    *p = (T)(add ? ((double)*p + in[t]) : in[t]);
}

/* the sharing unpack of the IPC transport with the wait folded in: every workgroup polls the senders' flags before it
 * reads a record, and reads the records system-scope (hq_k_interface_update<1> has the reasoning) */
template <typename T>
__global__ void __launch_bounds__(256)
hq_k_unpack_ipc(int32_t count, const int32_t* __restrict__ map, const double* in, T* __restrict__ table,
                const unsigned long long* __restrict__ flags, unsigned long long mask, unsigned long long epoch,
                unsigned long long timeout_ticks, int32_t* __restrict__ err)
{
    const int j = threadIdx.x;
    if (j < 64 && ((mask >> j) & 1ull)) {
        const unsigned long long t0 = wall_clock64();
        while (__hip_atomic_load(&flags[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < epoch) {
            __builtin_amdgcn_s_sleep(16);
            if (wall_clock64() - t0 > timeout_ticks) { atomicAdd(err, 1); break; }
        }
    }
    __syncthreads();
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count * 3) return;
    int i = t / 3, d = t - 3 * i;
    table[3 * (int64_t)map[i] + d] = (T)__hip_atomic_load(in + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

/* HQ_DEBUG_HALO: the sender's node identities beside the records, checked on receipt */
__global__ void hq_k_pack_id(int32_t count, const int32_t* __restrict__ map, const int64_t* __restrict__ gkey,
                             int64_t* __restrict__ out)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < count) out[t] = gkey[map[t]];
}

__global__ void hq_k_check_id(int32_t count, const int32_t* __restrict__ map, const int64_t* __restrict__ gkey,
                              const int64_t* __restrict__ in, int32_t* __restrict__ err)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < count && in[t] != gkey[map[t]]) atomicAdd(err, 1);
}

/* HQ_DEBUG_HALO on the transports that STORE records where the peer reads them (IPC) or stage them through the host: the
 * reference's -DDEBUG sends the node id with every record (psolve.c:5002-5007, 5058-5069); here the check word also binds
 * the record's payload and the number of the exchange, so that a record that is stale (an earlier exchange's), torn or
 * misrouted fails the receiver's check: word = id ^ mix(exchange) ^ bits(x) ^ rotl(bits(y), 21) ^ rotl(bits(z), 42) */
static __device__ __forceinline__ int64_t hq_check_word(int64_t id, unsigned long long epoch, double x, double y, double z)
{
    const unsigned long long a = (unsigned long long)__double_as_longlong(x), b = (unsigned long long)__double_as_longlong(y),
                             cc = (unsigned long long)__double_as_longlong(z);
    return (int64_t)((unsigned long long)id ^ (epoch * 0x9E3779B97F4A7C15ull) ^ a ^ ((b << 21) | (b >> 43)) ^ ((cc << 42) | (cc >> 22)));
}

/* vmap: the rows of `table` the records are packed from (node ids or interface slots); nmap: the nodes they belong to.
 * dst != NULL: every word goes where the peer reads it (system-scope store; the flags are raised by the record kernel
 * enqueued BEHIND this one); else out[i] */
template <typename T>
__global__ void hq_k_pack_check(int32_t count, const int32_t* __restrict__ vmap, const int32_t* __restrict__ nmap,
                                const T* __restrict__ table, const int64_t* __restrict__ gkey, unsigned long long epoch,
                                int64_t* const* __restrict__ dst, int64_t* __restrict__ out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const T* r = table + 3 * (int64_t)vmap[i];
    const int64_t w = hq_check_word(gkey[nmap[i]], epoch, (double)r[0], (double)r[1], (double)r[2]);   /* as the record travels */
    if (dst) __hip_atomic_store(dst[i], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else out[i] = w;
}

__global__ void hq_k_verify_check(int32_t count, const int32_t* __restrict__ nmap, const int64_t* __restrict__ gkey,
                                  unsigned long long epoch, const double* rec, const int64_t* words, int32_t* __restrict__ err)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const double x = __hip_atomic_load(rec + 3 * (int64_t)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM),
                 y = __hip_atomic_load(rec + 3 * (int64_t)i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM),
                 z = __hip_atomic_load(rec + 3 * (int64_t)i + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const int64_t w = __hip_atomic_load(words + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (w != hq_check_word(gkey[nmap[i]], epoch, x, y, z)) atomicAdd(err, 1);
}

/* solver_check_nan (psolve.c:3769-3782): count the values that are not finite */
template <typename T>
__global__ void hq_k_count_nonfinite(int64_t n, const T* __restrict__ a, int32_t* __restrict__ cnt)
{
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double v = (double)a[i];
        bad += !(fabs(v) <= 1.7976931348623157e308);          /* NaN and +-inf fail the comparison */
    }
    if (bad) atomicAdd(cnt, bad);
}

__global__ void hq_k_gather(int32_t n, const int32_t* __restrict__ ids,
                            const hq_real* __restrict__ a, const hq_real* __restrict__ b,
                            hq_real* __restrict__ oa, hq_real* __restrict__ ob)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 3) return;
    int i = t / 3, d = t - 3 * i;
    oa[t] = a[3 * (int64_t)ids[i] + d];
    ob[t] = b[3 * (int64_t)ids[i] + d];
}

/* ------------------------------------------------------------------------ */
/* helpers                                                                  */
/* ------------------------------------------------------------------------ */

static int hq_build_schedule(hq_ctx* c, const hq_schedule* in, hq_dev_schedule* out)
{
    auto load = [&](int32_t count, const hq_messenger* list, std::vector<hq_dev_messenger>& v,
                    hq_dbuf<int32_t>& d_map, hq_dbuf<double>& d_out, hq_dbuf<double>& d_in, int32_t* total, hq_dbuf<int64_t>& d_out_id,
                    hq_dbuf<int64_t>& d_in_id) -> int {
        std::vector<int32_t> map;
        for (int32_t i = 0; i < count; i++) {
            if (list[i].nodecount < 0 || (list[i].nodecount > 0 && !list[i].mapping))
                return hq_fail(HQ_ERR_ARG, "messenger with bad mapping%s", "");
            if (list[i].procid < 0 || list[i].procid >= c->nranks || list[i].procid == c->rank)
                return hq_fail(HQ_ERR_ARG, "messenger with bad procid%s", "");
            hq_dev_messenger m = { list[i].procid, list[i].nodecount, (int32_t)map.size() };
            for (int32_t k = 0; k < list[i].nodecount; k++) {
                int32_t id = list[i].mapping[k];
                if (id < 0 || id >= c->N) return hq_fail(HQ_ERR_ARG, "messenger node id out of range%s", "");
                map.push_back(id);
            }
            v.push_back(m);
        }
        *total = (int32_t)map.size();
        if (*total) {
            HQ_TRY(d_map.put(&c->bytes, map, c->stream));
            HQ_TRY(d_out.alloc(&c->bytes, map.size() * 3));
            HQ_TRY(d_in.alloc(&c->bytes, map.size() * 3));
            if (c->debug_halo) {
                HQ_TRY(d_out_id.alloc(&c->bytes, map.size()));
                HQ_TRY(d_in_id.alloc(&c->bytes, map.size()));
            }
        }
        return HQ_OK;
    };
    HQ_TRY(load(in->c_count, in->first_c, out->c, out->d_cmap, out->d_c_out, out->c_in_mem, &out->ctotal,
                out->d_c_out_id, out->d_c_in_id));
    HQ_TRY(load(in->s_count, in->first_s, out->s, out->d_smap, out->d_s_out, out->s_in_mem, &out->stotal,
                out->d_s_out_id, out->d_s_in_id));
    out->d_c_in = out->c_in_mem; out->d_s_in = out->s_in_mem;
    out->d_cmap_f = out->d_cmap;
    out->d_smap_f = out->d_smap;
    return HQ_OK;
}

static bool hq_ipc_ready(const hq_ctx* c);
/* a transport that is in place (an IPC arena that was exported but never connected is none: bench.py falls back from it) */
static bool hq_has_transport(const hq_ctx* c) { return c->comm || c->group || c->host_xchg || hq_ipc_ready(c); }
static int hq_refuse_split(const hq_ctx* c, const char* what);

static hq_dev_schedule* hq_peer_schedule(hq_ctx* peer, hq_ctx* me, hq_dev_schedule* mine)
{
    return (mine == &me->an) ? &peer->an : &peer->dn;
}

/*
 * schedule_senddata (psolve.c:4945-5079) on device buffers, in two halves so that
 * several in-process partitions can be stepped in lockstep:
 *   send half : pack (psolve.c:4985-5011) and hand the records to the transport
 *   recv half : wait for the neighbours' records, unpack (:5035-5073)
 * contribution: c-list out (to owners),  s-list in, table[...] += record
 * sharing     : s-list out (to sharers), c-list in, table[...]  = record
 * Transport: RCCL grouped send/recv over xGMI (hq_comm_init) or device-to-device
 * copies between contexts of one process (hq_group_link).
 */
/* (T: double for a force table, hq_real for a displacement field) */
template <typename T>
static int hq_xchg_send(hq_ctx* c, hq_dev_schedule* s, const T* table, bool contribution, bool force_table)
{
    hipStream_t xs = c->overlap ? c->cstream : c->stream;
    std::vector<hq_dev_messenger>& snd = contribution ? s->c : s->s;
    std::vector<hq_dev_messenger>& rcv = contribution ? s->s : s->c;
    if (snd.empty() && rcv.empty()) return HQ_OK;
    const int32_t* d_map = contribution ? (force_table ? s->d_cmap_f : s->d_cmap)
                                        : (force_table ? s->d_smap_f : s->d_smap);
    double* d_out = contribution ? s->d_c_out : s->d_s_out;
    double* d_in = contribution ? s->d_s_in : s->d_c_in;
    int32_t total = contribution ? s->ctotal : s->stotal;
    if (!hq_has_transport(c))
        return hq_fail(HQ_ERR_STATE, "halo exchange needs hq_comm_init, hq_comm_init_ipc, hq_comm_init_host or hq_group_link%s", "");
    /* the anchored-node sharing of the patch variant: hq_k_interface_update has written the records already */
    const bool prepacked = !contribution && s == &c->an && c->share_packed;
    if (prepacked) c->share_packed = false;
    if (hq_ipc_ready(c)) {
        /* between processes: the records are written where the peers read them, the last block raises the peers' flags */
        hq_ipc_state* I = c->ipc;
        if (prepacked) return HQ_OK;
        const int x = (s == &c->an ? 0 : 2) + (contribution ? 0 : 1);
        if (total) {
            if (c->debug_halo)      /* the check words first: they are in place when the record kernel raises the flags */
                hq_k_pack_check<<<hq_blocks(total, 256), 256, 0, xs>>>(total, d_map, contribution ? s->d_cmap : s->d_smap, table, c->d_gkey,
                                                                      ++c->dbg_send_epoch[x], I->d_dst_id[x], nullptr);
            I->send_epoch[x]++;
            hq_k_pack_to_peers_sig<<<hq_blocks((int64_t)total * 3, 256), 256, 0, xs>>>(total, d_map, table, I->d_dst[x], I->d_done + x,
                                                                                     I->nsig[x], I->d_sig[x], I->send_epoch[x], I->delay_ticks);
        }
        return HQ_OK;
    }
    double* const* d_dst = contribution ? s->d_c_dst : s->d_s_dst;
    if (c->group && d_dst && !c->debug_halo) {
        /* all partitions in one process: the records are written where the peers read them */
        if (total && !prepacked)
            hq_k_pack_to_peers<<<hq_blocks((int64_t)total * 3, 256), 256, 0, xs>>>(total, d_map, table, d_dst);
        HQ_HIP(hipEventRecord(c->ev_sent, xs));
        return HQ_OK;
    }
    if (total && !prepacked)
        hq_k_pack<<<hq_blocks((int64_t)total * 3, 256), 256, 0, xs>>>(total, d_map, table, d_out);
    /* HQ_DEBUG_HALO: the global identity of every record's node travels with it (psolve.c:5002-5007) */
    int64_t* d_out_id = contribution ? s->d_c_out_id : s->d_s_out_id;
    int64_t* d_in_id = contribution ? s->d_s_in_id : s->d_c_in_id;
    if (c->debug_halo && total && !c->host_xchg)
        hq_k_pack_id<<<hq_blocks(total, 256), 256, 0, xs>>>(total, contribution ? s->d_cmap : s->d_smap, c->d_gkey, d_out_id);
    if (c->group) {
        for (auto& m : snd) {
            if (!m.nodecount) continue;
            hq_ctx* peer = (*c->group)[m.procid];
            hq_dev_schedule* ps = hq_peer_schedule(peer, c, s);
            std::vector<hq_dev_messenger>& prcv = contribution ? ps->s : ps->c;
            double* p_in = contribution ? ps->d_s_in : ps->d_c_in;
            const hq_dev_messenger* pm = nullptr;
            for (auto& q : prcv) if (q.procid == c->rank) pm = &q;
            if (!pm || pm->nodecount != m.nodecount)
                return hq_fail(HQ_ERR_ARG, "neighbour schedules do not match%s", "");
            HQ_HIP(hipMemcpyAsync(p_in + 3 * (int64_t)pm->offset, d_out + 3 * (int64_t)m.offset,
                                  sizeof(double) * 3 * (size_t)m.nodecount, hipMemcpyDeviceToDevice, xs));
            if (c->debug_halo) {
                if (!peer->debug_halo) return hq_fail(HQ_ERR_STATE, "HQ_DEBUG_HALO must be set for every member of a group%s", "");
                int64_t* p_in_id = contribution ? ps->d_s_in_id : ps->d_c_in_id;
                HQ_HIP(hipMemcpyAsync(p_in_id + pm->offset, d_out_id + m.offset, sizeof(int64_t) * (size_t)m.nodecount,
                                      hipMemcpyDeviceToDevice, xs));
            }
        }
        HQ_HIP(hipEventRecord(c->ev_sent, xs));
    } else if (c->host_xchg) {
        /* records through pinned host memory and the caller's transport (the MPI_Irecv / MPI_Isend / MPI_Waitall of
         * schedule_senddata, psolve.c:5013-5033, stay the caller's): pack -> D2H -> callback -> H2D, on the exchange
         * stream; only that stream is waited for, the interior kernels keep running on the compute stream */
        double** ph_out = contribution ? &s->h_c_out : &s->h_s_out;
        double** ph_in = contribution ? &s->h_s_in : &s->h_c_in;
        const int32_t total_in = contribution ? s->stotal : s->ctotal;
        int64_t** ph_out_id = contribution ? &s->h_c_out_id : &s->h_s_out_id;
        int64_t** ph_in_id = contribution ? &s->h_s_in_id : &s->h_c_in_id;
        if (c->debug_halo) {
            /* the check words travel as a second message per neighbour (tag + 4), 8 bytes per record */
            const int xd = (s == &c->an ? 0 : 2) + (contribution ? 0 : 1);
            if (total && !*ph_out_id) HQ_HIP(hipHostMalloc((void**)ph_out_id, sizeof(int64_t) * (size_t)total, hipHostMallocDefault));
            if (total_in && !*ph_in_id) HQ_HIP(hipHostMalloc((void**)ph_in_id, sizeof(int64_t) * (size_t)total_in, hipHostMallocDefault));
            if (total) {
                hq_k_pack_check<<<hq_blocks(total, 256), 256, 0, xs>>>(total, d_map, contribution ? s->d_cmap : s->d_smap, table, c->d_gkey,
                                                                      ++c->dbg_send_epoch[xd], nullptr, d_out_id);
                HQ_HIP(hipMemcpyAsync(*ph_out_id, d_out_id, sizeof(int64_t) * (size_t)total, hipMemcpyDeviceToHost, xs));
            }
        }
        if (total && !*ph_out) HQ_HIP(hipHostMalloc((void**)ph_out, sizeof(double) * 3 * (size_t)total, hipHostMallocDefault));
        if (total_in && !*ph_in) HQ_HIP(hipHostMalloc((void**)ph_in, sizeof(double) * 3 * (size_t)total_in, hipHostMallocDefault));
        if (total) HQ_HIP(hipMemcpyAsync(*ph_out, d_out, sizeof(double) * 3 * (size_t)total, hipMemcpyDeviceToHost, xs));
        c->d2h_bytes += 24 * (int64_t)total;
        c->h2d_bytes += 24 * (int64_t)total_in;
        HQ_HIP(hipStreamSynchronize(xs));
        std::vector<int32_t> rp, sp;
        std::vector<int64_t> rn, sn;
        std::vector<double*> rb;
        std::vector<const double*> sb;
        for (auto& m : rcv) if (m.nodecount) { rp.push_back(m.procid); rn.push_back(3 * (int64_t)m.nodecount); rb.push_back(*ph_in + 3 * (int64_t)m.offset); }
        for (auto& m : snd) if (m.nodecount) { sp.push_back(m.procid); sn.push_back(3 * (int64_t)m.nodecount); sb.push_back(*ph_out + 3 * (int64_t)m.offset); }
        const int32_t tag = (s == &c->an ? 0 : 2) + (contribution ? 0 : 1);
        if (c->host_xchg(c->host_user, (int32_t)rp.size(), rp.data(), rn.data(), rb.data(), (int32_t)sp.size(), sp.data(), sn.data(),
                         sb.data(), tag) != 0)
            return hq_fail(HQ_ERR_COMM, "the host transport's exchange callback failed%s", "");
        if (total_in) HQ_HIP(hipMemcpyAsync(d_in, *ph_in, sizeof(double) * 3 * (size_t)total_in, hipMemcpyHostToDevice, xs));
        if (c->debug_halo) {
            std::vector<double*> rbi;
            std::vector<const double*> sbi;
            std::vector<int64_t> rni, sni;
            for (auto& m : rcv) if (m.nodecount) { rni.push_back((int64_t)m.nodecount); rbi.push_back((double*)(*ph_in_id + m.offset)); }
            for (auto& m : snd) if (m.nodecount) { sni.push_back((int64_t)m.nodecount); sbi.push_back((const double*)(*ph_out_id + m.offset)); }
            if (c->host_xchg(c->host_user, (int32_t)rp.size(), rp.data(), rni.data(), rbi.data(), (int32_t)sp.size(), sp.data(), sni.data(),
                             sbi.data(), tag + 4) != 0)
                return hq_fail(HQ_ERR_COMM, "the host transport's exchange callback failed%s", "");
            if (total_in) HQ_HIP(hipMemcpyAsync(d_in_id, *ph_in_id, sizeof(int64_t) * (size_t)total_in, hipMemcpyHostToDevice, xs));
            c->d2h_bytes += 8 * (int64_t)total;
            c->h2d_bytes += 8 * (int64_t)total_in;
        }
    } else {
        HQ_NCCL(g_rccl.GroupStart());
        for (auto& m : rcv)
            if (m.nodecount)
                HQ_NCCL(g_rccl.Recv(d_in + 3 * (int64_t)m.offset, (size_t)m.nodecount * 3, HQ_NCCL_DOUBLE,
                                    m.procid, c->comm, xs));
        for (auto& m : snd)
            if (m.nodecount)
                HQ_NCCL(g_rccl.Send(d_out + 3 * (int64_t)m.offset, (size_t)m.nodecount * 3, HQ_NCCL_DOUBLE,
                                    m.procid, c->comm, xs));
        if (c->debug_halo) {
            for (auto& m : rcv)
                if (m.nodecount)
                    HQ_NCCL(g_rccl.Recv(d_in_id + m.offset, (size_t)m.nodecount, HQ_NCCL_INT64, m.procid, c->comm, xs));
            for (auto& m : snd)
                if (m.nodecount)
                    HQ_NCCL(g_rccl.Send(d_out_id + m.offset, (size_t)m.nodecount, HQ_NCCL_INT64, m.procid, c->comm, xs));
        }
        HQ_NCCL(g_rccl.GroupEnd());
    }
    return HQ_OK;
}

/* HQ_DEBUG_HALO: every received record must name the node it is unpacked into (psolve.c:5058-5069);
 * mismatches are counted and reported by hq_sync */
static void hq_xchg_check(hq_ctx* c, hq_dev_schedule* s, bool contribution, hipStream_t xs)
{
    if (!c->debug_halo) return;
    const int32_t total = contribution ? s->stotal : s->ctotal;
    if (total && (c->host_xchg || hq_ipc_ready(c))) {
        /* check words (see hq_k_pack_check); the IPC transport's callers have waited for the flags already */
        const int x = (s == &c->an ? 0 : 2) + (contribution ? 0 : 1);
        const int64_t* words = hq_ipc_ready(c) ? c->ipc->d_in_id[x] : (contribution ? s->d_s_in_id : s->d_c_in_id);
        hq_k_verify_check<<<hq_blocks(total, 256), 256, 0, xs>>>(total, contribution ? s->d_smap : s->d_cmap, c->d_gkey, ++c->dbg_recv_epoch[x],
                                                                contribution ? s->d_s_in : s->d_c_in, words, c->d_halo_err);
        return;
    }
    if (total)
        hq_k_check_id<<<hq_blocks(total, 256), 256, 0, xs>>>(total, contribution ? s->d_smap : s->d_cmap, c->d_gkey,
                                                              contribution ? s->d_s_in_id : s->d_c_in_id, c->d_halo_err);
}

/* IPC transport: the exchange stream waits until every sending peer's flag has reached this exchange's epoch */
static void hq_ipc_wait(hq_ctx* c, hq_dev_schedule* s, bool contribution, hipStream_t xs)
{
    hq_ipc_state* I = c->ipc;
    const int x = (s == &c->an ? 0 : 2) + (contribution ? 0 : 1);
    if (!I->wait_mask[x]) return;
    I->recv_epoch[x]++;
    hq_k_ipc_wait<<<1, 64, 0, xs>>>(I->d_flags + (size_t)x * HQ_IPC_MAXNB, I->wait_mask[x], I->recv_epoch[x], I->timeout_ticks,
                                   c->d_halo_err + 2);
}

template <typename T>
static int hq_xchg_recv(hq_ctx* c, hq_dev_schedule* s, T* table, bool contribution, bool force_table)
{
    hipStream_t xs = c->overlap ? c->cstream : c->stream;
    std::vector<hq_dev_messenger>& rcv = contribution ? s->s : s->c;
    if (rcv.empty()) return HQ_OK;
    const int32_t* d_map = contribution ? (force_table ? s->d_smap_f : s->d_smap)
                                        : (force_table ? s->d_cmap_f : s->d_cmap);
    double* d_in = contribution ? s->d_s_in : s->d_c_in;
    if (c->group)
        for (auto& m : rcv)
            if (m.nodecount) HQ_HIP(hipStreamWaitEvent(xs, (*c->group)[m.procid]->ev_sent, 0));
    if (hq_ipc_ready(c) && !contribution && s->ctotal && !c->debug_halo) {
        /* IPC sharing: wait and unpack in one kernel */
        hq_ipc_state* I = c->ipc;
        const int x = (s == &c->an ? 0 : 2) + 1;
        const unsigned long long ep = I->wait_mask[x] ? ++I->recv_epoch[x] : 0;
        hq_k_unpack_ipc<<<hq_blocks((int64_t)s->ctotal * 3, 256), 256, 0, xs>>>(s->ctotal, d_map, d_in, table,
            I->d_flags + (size_t)x * HQ_IPC_MAXNB, I->wait_mask[x], ep, I->timeout_ticks, c->d_halo_err + 2);
        HQ_HIP(hipGetLastError());
        return HQ_OK;
    }
    if (hq_ipc_ready(c)) hq_ipc_wait(c, s, contribution, xs);
    hq_xchg_check(c, s, contribution, xs);
    if (!contribution) {
        /* sharing: every non-owned node has exactly one owner, one launch covers all records */
        int32_t total = s->ctotal;
        if (total)
            hq_k_unpack<<<hq_blocks((int64_t)total * 3, 256), 256, 0, xs>>>(total, d_map, d_in, table, 0);
    } else {
        /* contribution: one launch per neighbour: a node may receive from several sharers and
         * the sums stay in a fixed order (the reference walks its messenger list) */
        for (auto& m : rcv)
            if (m.nodecount)
                hq_k_unpack<<<hq_blocks((int64_t)m.nodecount * 3, 256), 256, 0, xs>>>(
                    m.nodecount, d_map + m.offset, d_in + 3 * (int64_t)m.offset, table, 1);
    }
    HQ_HIP(hipGetLastError());
    return HQ_OK;
}

/* wait for everything enqueued on the context's streams */
static hipError_t hq_quiesce(hq_ctx* c)
{
    hipError_t e = hipStreamSynchronize(c->stream);
    if (c->cstream) {
        hipError_t e2 = hipStreamSynchronize(c->cstream);
        if (e == hipSuccess) e = e2;
    }
    if (c->bstream) {
        hipError_t e2 = hipStreamSynchronize(c->bstream);
        if (e == hipSuccess) e = e2;
    }
    if (c->astream) {
        hipError_t e2 = hipStreamSynchronize(c->astream);
        if (e == hipSuccess) e = e2;
    }
    return e;
}

/* ---- the phase clock ---- */
static void hq_clock_harvest(hq_ctx* c, hq_ctx::hq_clock_slot& sl, bool wait)
{
    if (!sl.pending) return;
    for (int k = 0; k < hq_ctx::HQ_CLK_N; k++)
        if (sl.used[k] && (wait ? hipEventSynchronize(sl.e[k]) : hipEventQuery(sl.e[k])) != hipSuccess) return;   /* not done yet */
    auto span = [&](int a, int b, double* us) {
        float ms = 0;
        if (!sl.used[a] || !sl.used[b] || hipEventElapsedTime(&ms, sl.e[a], sl.e[b]) != hipSuccess) return false;
        *us = 1e3 * (double)ms;
        return true;
    };
    double shell = 0, interior = 0, chain = 0, t_int_end = 0, t_chain_end = 0, t_shell_end = 0;
    span(hq_ctx::HQ_CLK_STEP0, hq_ctx::HQ_CLK_SHELL1, &shell);
    span(hq_ctx::HQ_CLK_INT0, hq_ctx::HQ_CLK_INT1, &interior);
    span(hq_ctx::HQ_CLK_CHAIN0, hq_ctx::HQ_CLK_CHAIN1, &chain);
    span(hq_ctx::HQ_CLK_STEP0, hq_ctx::HQ_CLK_SHELL1, &t_shell_end);
    span(hq_ctx::HQ_CLK_STEP0, hq_ctx::HQ_CLK_INT1, &t_int_end);
    span(hq_ctx::HQ_CLK_STEP0, hq_ctx::HQ_CLK_CHAIN1, &t_chain_end);
    const double compute_end = std::max(t_shell_end, t_int_end);
    c->clk_us[0] += std::max(compute_end, t_chain_end);
    c->clk_us[1] += shell;
    c->clk_us[2] += interior;
    c->clk_us[3] += chain;
    c->clk_us[4] += std::max(0.0, t_chain_end - compute_end);
    c->clk_steps++;
    sl.pending = false;
    for (int k = 0; k < hq_ctx::HQ_CLK_N; k++) sl.used[k] = false;
}

static void hq_clock_harvest_all(hq_ctx* c, bool wait)
{
    for (auto& sl : c->clock) hq_clock_harvest(c, sl, wait);
}

static bool hq_clock_on(const hq_ctx* c) { return hq_set(c->opts.phase_timing) || c->timing; }

/* a new step: take the next slot of the ring (the step that used it HQ_CLK_SLOTS steps ago is long done) */
static void hq_clock_begin(hq_ctx* c)
{
    if (!hq_clock_on(c)) return;
    /* a timed batch (bench.py's timed region) samples every fourth step: six more event records per step are host time
     * that a rank of a multi-GPU run, whose step is ~160 us, should not pay in full; hq_options.phase_timing records all */
    if (!hq_set(c->opts.phase_timing) && (c->step & 3) != 0) {
        c->clock_skip = true;
        return;
    }
    c->clock_skip = false;
    if (c->clock.empty()) c->clock.resize(hq_ctx::HQ_CLK_SLOTS);
    c->clock_at = (c->clock_at + 1) % c->clock.size();
    hq_ctx::hq_clock_slot& sl = c->clock[c->clock_at];
    hq_clock_harvest(c, sl, true);
    sl.pending = true;
}

static void hq_clock(hq_ctx* c, int k, hipStream_t st)
{
    if (!hq_clock_on(c) || c->clock.empty() || c->clock_skip) return;
    hq_ctx::hq_clock_slot& sl = c->clock[c->clock_at];
    if (!sl.pending) return;
    if (!sl.e[k] && hipEventCreate(&sl.e[k]) != hipSuccess) { sl.e[k] = nullptr; return; }
    if (hipEventRecord(sl.e[k], st) == hipSuccess) sl.used[k] = true;
}

static void hq_mark(hq_ctx* c)
{
    if (c->timing && c->ev_used < c->ev.size()) hipEventRecord(c->ev[c->ev_used++], c->stream);
}

/* ------------------------------------------------------------------------ */
/* the step                                                                 */
/* ------------------------------------------------------------------------ */

static int hq_launch_source(hq_ctx* c)
{
    int32_t k = c->step - c->src_step0;
    if (c->nloaded > 0 && k >= 0 && k < c->src_nsteps)
        hq_k_source<<<hq_blocks(c->nloaded * 3, 64), 64, 0, c->stream>>>(
            c->nloaded, c->d_loaded, c->d_F + (int64_t)k * c->nloaded * 3, c->dt2, c->d_force);
    return HQ_OK;
}

static int hq_launch_element_scatter(hq_ctx* c)
{
    if (c->att.on) {                                         /* BKT: calc_conv, then constant_Q_addforce (psolve.c:3995-3999) */
        const hq_atten_dev& A = c->att;
        hq_k_atten_advance<<<hq_blocks(A.nslots, 256), 256, 0, c->stream>>>(
            A.nslots, A.d_slot_node, A.d_slot_class, A.d_ktab, c->d_u[c->now], c->d_u[c->prev], A.d_mv, A.d_w);
        hq_mark(c);                                          /* (hq_run_timed brackets the dominant kernel: hq_k_element_bkt) */
        hq_k_element_bkt<<<hq_blocks(c->E, 256), 256, 0, c->stream>>>(
            c->E, c->Epad, A.nslots, c->d_lnid, A.d_eslot, c->d_c1, c->d_c2, A.d_w, c->d_force);
        hq_mark(c);
        return HQ_OK;
    }
    hq_mark(c);
    hq_k_element_scatter<<<hq_blocks(c->E, 256), 256, 0, c->stream>>>(
        c->E, c->Epad, c->d_lnid, c->d_c1, c->d_c2, c->d_beta, c->d_u[c->now], c->d_u[c->prev], c->d_force);
    hq_mark(c);
    return HQ_OK;
}

static int hq_launch_update(hq_ctx* c)
{
    int64_t n3 = (int64_t)c->N * 3;
    hq_k_update<<<hq_blocks(n3, 256), 256, 0, c->stream>>>(n3, c->d_nt, c->d_u[c->now], c->d_u[c->prev],
                                                          c->d_force);
    return HQ_OK;
}

/*
 * Interface nodes this rank owns: own partial force + the sharers' records
 * (the "+=" unpack of schedule_senddata, psolve.c:5035-5073, in messenger order)
 * + solver_compute_displacement + the PACK of the displacement sharing (psolve.c:4312, :4985-5011), in one kernel:
 * the records a node receives contributions in and the records its new displacement is shared in are the same
 * entries of the s-list, so the thread that finishes a node also writes it where the transport takes it from
 * (s_out: the packed send buffer of RCCL / host-staged / copying transports) or where the sharers read it (s_dst:
 * direct peer stores of the in-process and IPC transports).
 * IPC = 1: the IPC transport's wait and signal are folded in -- every workgroup polls the contribution flags before it
 * reads a record (relaxed system-scope loads, and the records are read system-scope too: no cache holds them stale),
 * and the workgroup that finishes last raises the sharing flags (see hq_k_pack_to_peers_sig).
 */
struct hq_ipc_args {
    const unsigned long long* wait_flags;            /* this rank's flags of the contribution exchange */
    unsigned long long wait_mask, wait_epoch, timeout_ticks;
    int32_t* err;
    uint32_t* done;
    int32_t nsig;
    unsigned long long* const* sig;
    unsigned long long sig_epoch;
    unsigned long long delay_ticks;                  /* loopback diagnostic: HQ_LOOPBACK_DELAY_US */
};

template <int IPC>
__global__ void __launch_bounds__(256)
hq_k_interface_update(int32_t n, const int32_t* __restrict__ node, const int32_t* __restrict__ slot,
                      const int32_t* __restrict__ ptr, const int32_t* __restrict__ pos, const int32_t* __restrict__ fcv,
                      const double* __restrict__ iforce, const double* rec,
                      const double* __restrict__ nt, const hq_real* __restrict__ u1,
                      const hq_real* __restrict__ u2, hq_real* __restrict__ un, double* __restrict__ s_out,
                      double* const* __restrict__ s_dst, hq_ipc_args ia)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (IPC) {
        const int j = threadIdx.x;
        if (j < 64 && ((ia.wait_mask >> j) & 1ull)) {
            const unsigned long long t0 = wall_clock64();
            while (__hip_atomic_load(&ia.wait_flags[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < ia.wait_epoch) {
                __builtin_amdgcn_s_sleep(16);
                if (wall_clock64() - t0 > ia.timeout_ticks) { atomicAdd(ia.err, 1); break; }
            }
        }
        __syncthreads();
    }
    if (t < n * 3) {
        int i = t / 3, d = t - 3 * i;
        /* fcv[i] = the node's FIRST record (low 24 bits: almost every interface node has exactly one sharer) and its
         * number of records (high 8): record and destination are then loads of the second level, beside n_t, u1, u2 and
         * the own partial force, instead of a third one behind ptr -> pos -- this kernel runs one workgroup per CU beside
         * the brick launch, where every level of dependent loads costs microseconds */
        int64_t g = node[i];
        const int32_t fc = fcv[i];
        const int32_t first = fc & 0xffffff, cnt = (int32_t)((uint32_t)fc >> 24);
        const double* np = nt + 7 * g;
        double f = iforce[3 * (int64_t)slot[i] + d];
        double* p0 = (s_dst && cnt) ? s_dst[first] : nullptr;
        if (cnt)
            f += IPC ? __hip_atomic_load(rec + 3 * (int64_t)first + d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
                     : rec[3 * (int64_t)first + d];
        const int32_t k0 = cnt > 1 ? ptr[i] : 0;
        for (int32_t k = 1; k < cnt; k++)                            /* messenger order: pos[k0] == first */
            f += IPC ? __hip_atomic_load(rec + 3 * (int64_t)pos[k0 + k] + d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
                     : rec[3 * (int64_t)pos[k0 + k] + d];
        f += (np[1 + d] * (double)u1[3 * g + d] - np[4 + d] * (double)u2[3 * g + d]);
        const double v = (double)(hq_real)(f / np[0]);        /* what the owner keeps is what its sharers get */
        un[3 * g + d] = (hq_real)v;
        if (s_dst) {
            if (cnt) {
                if (IPC) __hip_atomic_store(p0 + d, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                else p0[d] = v;
            }
            for (int32_t k = 1; k < cnt; k++) {
                if (IPC) __hip_atomic_store(s_dst[pos[k0 + k]] + d, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                else s_dst[pos[k0 + k]][d] = v;
            }
        } else if (s_out) {
            if (cnt) s_out[3 * (int64_t)first + d] = v;
            for (int32_t k = 1; k < cnt; k++) s_out[3 * (int64_t)pos[k0 + k] + d] = v;
        }
    }
    if (IPC) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        __shared__ int s_last;
        if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(ia.done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
        __syncthreads();
        if (!s_last) return;
        if (threadIdx.x == 0) __hip_atomic_store(ia.done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((int)threadIdx.x < ia.nsig) {
            hq_ipc_delay(ia.delay_ticks);
            __hip_atomic_store(ia.sig[threadIdx.x], ia.sig_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

/*
 * One iteration of the solver_run loop body (psolve.c:4286-4316) as NPHASE
 * phases; a phase never waits for a neighbour's data that the neighbour has
 * not been asked to send in an earlier phase, so in-process groups enqueue
 * phase k for every member before phase k+1.
 */
enum { HQ_NPHASE = 9 };

/* the bricks on a stream of their own (HQ_BRICK_STREAM=1, opt-in)?  Within a step they depend on nothing the patches
 * write, so they could start beside them.  Measured on a rank of 8 alone (profiles/r04/rank_alone_trace.txt): 187 us
 * per step against 172 with the bricks behind the patches -- the patches that own no interface node then queue for
 * slots the resident brick workgroups hold (their launch stretches from 14 to 110 us) and the chain's kernels with
 * them.  Kept for boxes where the shell is larger than one round of workgroups; parity-tested (HQ_OVERLAP=1 tests). */
static bool hq_use_brick_stream(hq_ctx* c)
{
    /* (a context alone: the patches of the thin shell left behind the bricks are latency-bound gathers, 1 TB/s; beside the
     *  bandwidth-bound brick launch they cost next to nothing, ahead of it their 30 us count in full) */
    /* measured (profiles/r05/ab_brick_stream.txt, one box, back to back): the 189 M-element basin 3.10 -> 3.00 ms and the
     * laterally refined one 2.19 -> 2.09 ms per step (8 716 / 30 293 patches), but the 64 M box 1.028 -> 1.052 and the 8 M box
     * 0.145 -> 0.153 (2 003 / 491 patches: the two cross-stream waits per step cost more than the thin shell's launch):
     * on by default only where the shell is more than eight rounds of patch workgroups (two per CU) */
    const bool solo = !hq_has_transport(c) && c->nranks == 1 && c->plan.npatches > 16 * c->plan.grid_cus;
    /* (default: on a context that steps alone, where the shell's patch launch then runs BESIDE the first round of brick
     *  workgroups instead of ahead of it) */
    const bool want = hq_given(c->opts.brick_stream) ? c->opts.brick_stream != 0 : solo;
    if (!want || !(c->overlap || (!hq_has_transport(c) && c->nranks == 1)) || c->stream_masked || c->bricks.nunits <= 0 || c->plan.npatches <= 0) return false;
    if (!c->bstream) {
        int prio_lo = 0, prio_hi = 0;
        if (hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) != hipSuccess) return false;
        int prio = prio_lo;
#ifdef HQ_EXPERIMENT            /* profiles/tools only: which of the two streams should the dispatcher prefer? */
        if (getenv("HQ_X_BRICK_PRIO")) prio = !strcmp(getenv("HQ_X_BRICK_PRIO"), "high") ? prio_hi : (prio_lo + prio_hi) / 2;
#endif
        if (hipStreamCreateWithPriority(&c->bstream, hipStreamNonBlocking, prio) != hipSuccess) { c->bstream = nullptr; return false; }
        if (hipEventCreateWithFlags(&c->ev_patches, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_bricks, hipEventDisableTiming) != hipSuccess) return false;
        /* everything enqueued so far is on the compute stream: the first brick launch goes behind it */
        hipEventRecord(c->ev_patches, c->stream);
        hipEventRecord(c->ev_bricks, c->stream);
    }
    return true;
}

#include "hq_outputs.h"

/*
 * A correction pass in the step (hq_correction.h), and where its launches stand among the step's streams.
 * Head (phase 0: fork, the pass's own element kernels, sum): it may read u(t) and u(t - dt), the pass's own state and nothing
 * this step writes.  So it forks onto the correction stream behind everything the compute stream has seen so far -- the last
 * step's join, which read dF and wrote what is now u(t) -- and runs beside this step's patches and bricks.
 * Tail (phase 8: join): it adds to un, so it waits for every step kernel of this step -- the compute stream's own, which it
 * follows in stream order, and the bricks' through their event where they run on a stream of their own -- and for the head.
 * un is the buffer this step's head-of-step outputs read as u(t - 2 dt): the step kernels that wrote it waited for them
 * (hq_outputs_enqueue), and the join's launches lie behind those kernels.  The next step's bricks read and overwrite what the
 * join touches, and on their own stream they wait for ev_patches: it is recorded again behind the join (as behind the
 * assignment of phase 6).
 * HQ_ATTEN_SPLIT_INLINE (profiles/tools/atten_split_step.py): the whole chain ON the compute stream, to price the overlap.
 */
static int hq_correction_fork(hq_ctx* c, hipStream_t* as)
{
#ifdef HQ_ATTEN_SPLIT_INLINE
    *as = c->stream;
#else
    *as = c->astream;
    HQ_HIP(hipEventRecord(c->ev_att_fork, c->stream));
    HQ_HIP(hipStreamWaitEvent(*as, c->ev_att_fork, 0));
#endif
    return HQ_OK;
}

/* the end of the head: the corner forces the pass's kernels left in ef, summed per row */
static int hq_correction_sum(hq_ctx* c, const hq_correction& K, hipStream_t as)
{
    hq_k_atten_node_sum<<<hq_blocks(K.rows, 256), 256, 0, as>>>(K.rows, K.stride, K.d_nptr, K.d_nent, K.d_ef, K.d_dF);
#ifndef HQ_ATTEN_SPLIT_INLINE
    HQ_HIP(hipEventRecord(c->ev_att_done, as));
#endif
    return HQ_OK;
}

/* dF's hanging nodes to their anchors, un += dF / n_t[0], the hanging nodes of un assigned again */
static int hq_correction_join(hq_ctx* c, const hq_correction& K, hq_real* un)
{
    if (!K.nelem) return HQ_OK;
    if (c->bstream) HQ_HIP(hipStreamWaitEvent(c->stream, c->ev_bricks, 0));
#ifndef HQ_ATTEN_SPLIT_INLINE
    HQ_HIP(hipStreamWaitEvent(c->stream, c->ev_att_done, 0));
#endif
    K.dist.launch(K.d_dF, c->stream);
    const int64_t n3 = 3 * (int64_t)K.rows;
    if (K.d_tnode) hq_k_atten_apply_at<<<hq_blocks(n3, 256), 256, 0, c->stream>>>(n3, K.d_tnode, K.d_mass, K.d_dF, un);
    else hq_k_atten_apply<<<hq_blocks(n3, 256), 256, 0, c->stream>>>(n3, K.d_mass, K.d_dF, un);
    if (c->ldnnum)
        hq_k_adjust_assign<<<hq_blocks(c->ldnnum * 3, 256), 256, 0, c->stream>>>(c->ldnnum, c->d_dn_id, c->d_dn_ptr, c->d_dn_anchor, un);
    if (c->bstream) HQ_HIP(hipEventRecord(c->ev_patches, c->stream));
    return HQ_OK;
}

/* a split context's head (hq_atten_split.h): the delta advance and the corner force */
static int hq_atten_split_head(hq_ctx* c)
{
    const hq_atten_dev& A = c->att;
    hipStream_t as;
    HQ_TRY(hq_correction_fork(c, &as));
    hq_k_atten_advance_delta<<<hq_blocks(A.nslots, 256), 256, 0, as>>>(
        A.nslots, A.d_slot_node, A.d_slot_class, A.d_ktab, c->d_u[c->now], c->d_u[c->prev], A.d_mv, A.d_w);
    hq_k_atten_corner_force<<<hq_blocks(c->E, 256), 256, 0, as>>>(c->E, A.Epad, A.nslots, A.d_eslot, A.d_c1, A.d_c2, A.d_w, A.corr.d_ef);
    return hq_correction_sum(c, A.corr, as);
}

/* a nonlinear context's head (hq_nonlin_dev.h): the element kernel; nothing without elements */
static int hq_nl_head(hq_ctx* c)
{
    const hq_nl_dev& L = c->nl;
    if (!L.nel) return HQ_OK;
    hipStream_t as;
    HQ_TRY(hq_correction_fork(c, &as));
    hq_k_nl_element<<<hq_blocks(L.nel, 256), 256, 0, as>>>(L.nel, L.Enlpad, L.d_lnid, L.d_cons, c->d_u[c->now], c->dt2, L.d_st, L.corr.d_ef);
    return hq_correction_sum(c, L.corr, as);
}

static int hq_phase(hq_ctx* c, int ph)
{
    const bool patch = (c->variant == HQ_VARIANT_PATCH);
    double* ftab = patch ? c->d_iforce : c->d_force;
    hq_real* unew = patch ? c->d_u[c->spare] : c->d_u[c->prev];
    switch (ph) {
    case 0:
        if (patch) {
            int32_t k = c->step - c->src_step0;
            const double* F = (c->nloaded > 0 && k >= 0 && k < c->src_nsteps)
                                  ? c->d_F + (int64_t)k * c->nloaded * 3 : nullptr;
            int32_t nb = c->plan.nb, ne = c->plan.ne;
            /* Behind bricks a partition's element-form patches are few: where all of them are at most TWO rounds of
             * workgroups (two per CU; HQ_PATCH_MERGE_ROUNDS) the patches that own no interface node join the interface
             * patches' launch instead of following it behind a 7 us launch gap -- an eighth of the 64M box has 964
             * patches: 20 + 7 + 14 us in two launches, 27 us in one (rank-alone trace: 175.5 -> 170.7 us per step; the
             * chain then starts 7 us later and still ends 20 us before the brick launch does) */
            if (c->overlap && !hq_patch_uses_pers(&c->plan) && nb > 0 && nb + ne <= 2 * hq_value_or(c->opts.patch_merge_rounds, 2) * c->plan.grid_cus) { nb += ne; ne = 0; }
            const bool bs = hq_use_brick_stream(c);
            if (c->overlap) HQ_HIP(hipStreamWaitEvent(c->stream, c->ev_shared, 0));   /* last step's shared displacements */
            if (bs) {
                HQ_HIP(hipStreamWaitEvent(c->stream, c->ev_bricks, 0));               /* ... and its bricks */
                /* the bricks' own stream: behind the last step's chain (they read shared nodes in their rings and overwrite
                 * the buffer its interface update read) and the last step's patches (ring rows; the buffer those read as
                 * u(t - dt)) -- ev_patches still names THAT record here, this step's comes below */
                if (c->ev_shared) HQ_HIP(hipStreamWaitEvent(c->bstream, c->ev_shared, 0));
                HQ_HIP(hipStreamWaitEvent(c->bstream, c->ev_patches, 0));
            }
            if (c->att.split) HQ_TRY(hq_atten_split_head(c));
            if (c->nl.on) HQ_TRY(hq_nl_head(c));
            HQ_TRY(hq_outputs_enqueue(c, bs));     /* solver_write_checkpoint / _output_wavefield / _planes / _stations, :4277-4280 */
            auto launch_bricks = [&]() {
                if (c->bricks.nunits > 0)
                    hq_brick_launch(&c->bricks, c->d_u[c->now], c->d_u[c->prev], c->d_u[c->spare], c->plan.d_nt3, F, c->dt2,
                                    bs ? c->bstream : c->stream, hq_given(c->opts.brick_by_component) ? c->opts.brick_by_component != 0 : c->overlap);
                if (bs) hipEventRecord(c->ev_bricks, c->bstream);
            };
            hq_mark(c);
            hq_clock_begin(c);
            hq_clock(c, hq_ctx::HQ_CLK_STEP0, c->stream);
            if (bs) hq_clock(c, hq_ctx::HQ_CLK_INT0, c->bstream);       /* the bricks start beside the shell */
            bool chain_marked = false;
            auto chain_released = [&]() {                               /* the exchange stream may go: the interface patches are enqueued */
                if (!chain_marked && c->overlap) hq_clock(c, hq_ctx::HQ_CLK_CHAIN0, c->cstream);
                chain_marked = true;
            };
            if (c->plan.ns > 0 || c->plan.nr > 0) {
                /* ONE persistent launch for all element-form patches, the interface patches at the head of its
                 * queue; the exchange chain starts behind it and runs beside the stencil kernel -- the bulk of the
                 * partition, in small workgroups that leave CUs to the chain's kernels as they retire */
                /* with the chain on its own stream only the patches that own interface nodes go ahead of the event: the
                 * other element-form patches (all of them on octree or layered partitions) run beside the exchange */
                const int32_t head = c->overlap ? nb : nb + ne;
                hq_patch_launch(&c->plan, 0, head, c->d_u[c->now], c->d_u[c->prev], c->d_u[c->spare], c->d_nt, F, c->dt2,
                                c->d_iforce, c->stream);
                hq_patch_launch_stencil(&c->plan, 0, c->d_u[c->now], c->d_u[c->prev], c->d_u[c->spare], c->d_nt, F, c->dt2,
                                        c->d_iforce, c->stream);      /* the stencil patches on the partition interface */
                if (c->overlap) {
                    HQ_HIP(hipEventRecord(c->ev_bnd, c->stream));
                    HQ_HIP(hipStreamWaitEvent(c->cstream, c->ev_bnd, 0));
                    chain_released();
                    hq_patch_launch(&c->plan, nb, ne, c->d_u[c->now], c->d_u[c->prev], c->d_u[c->spare], c->d_nt, F, c->dt2,
                                    c->d_iforce, c->stream, c->reserve_cus);
                }
                hq_patch_launch_stencil(&c->plan, 1, c->d_u[c->now], c->d_u[c->prev], c->d_u[c->spare], c->d_nt, F, c->dt2,
                                        c->d_iforce, c->stream);
            } else {
                /* no stencil patches (octree regions, layered material): interface patches first, then the interior
                 * launch, which leaves `reserve_cus` CUs to the chain */
                if (c->overlap) {
                    hq_patch_launch(&c->plan, 0, nb, c->d_u[c->now], c->d_u[c->prev], c->d_u[c->spare], c->d_nt, F, c->dt2,
                                    c->d_iforce, c->stream);
                    HQ_HIP(hipEventRecord(c->ev_bnd, c->stream));
                    HQ_HIP(hipStreamWaitEvent(c->cstream, c->ev_bnd, 0));
                    chain_released();
                    hq_patch_launch(&c->plan, nb, ne, c->d_u[c->now], c->d_u[c->prev], c->d_u[c->spare], c->d_nt, F,
                                    c->dt2, c->d_iforce, c->stream, c->reserve_cus);
                } else {                         /* one stream: one persistent launch over all of them */
                    hq_patch_launch(&c->plan, 0, nb + ne, c->d_u[c->now], c->d_u[c->prev], c->d_u[c->spare], c->d_nt, F,
                                    c->dt2, c->d_iforce, c->stream);
                }
            }
            /* the bricks: simple nodes only, never on the interface -- interior work beside the exchange chain */
            if (bs) HQ_HIP(hipEventRecord(c->ev_patches, c->stream));
            hq_clock(c, hq_ctx::HQ_CLK_SHELL1, c->stream);
            if (!bs) hq_clock(c, hq_ctx::HQ_CLK_INT0, c->stream);
            launch_bricks();
            hq_clock(c, hq_ctx::HQ_CLK_INT1, bs ? c->bstream : c->stream);
            if (!c->overlap && hq_has_transport(c)) hq_clock(c, hq_ctx::HQ_CLK_CHAIN0, c->stream);   /* the chain follows on this stream */
            /* (bricks on their own stream: the marks on this stream see the shell only -- hq_run_timed takes the step's
             *  kernel time from the phase clock's events instead, and a timed batch enqueues exactly what hq_run does) */
            hq_mark(c);
        } else {
            HQ_TRY(hq_outputs_enqueue(c, false));
            HQ_TRY(hq_launch_source(c));                                   /* :4288 */
            HQ_TRY(hq_launch_element_scatter(c));                          /* :4290-4291 */
        }
        return HQ_OK;
    case 1: return hq_xchg_send(c, &c->dn, ftab, true, true);                        /* :4298 */
    case 2:
        HQ_TRY(hq_xchg_recv(c, &c->dn, ftab, true, true));
        if (patch) {
            /* hanging nodes nobody shares were distributed inside the patches; the shared ones here */
            c->dist.launch(c->d_iforce, c->overlap ? c->cstream : c->stream);
        } else {                                                           /* :4299 */
            c->dist.launch(c->d_force, c->stream);
        }
        return HQ_OK;
    case 3: return hq_xchg_send(c, &c->an, ftab, true, true);                        /* :4301 */
    case 4:
        if (patch) {
            hipStream_t xs = c->overlap ? c->cstream : c->stream;
            if (c->group)
                for (auto& m : c->an.s)
                    if (m.nodecount) HQ_HIP(hipStreamWaitEvent(xs, (*c->group)[m.procid]->ev_sent, 0));
            /* HQ_DEBUG_HALO over the IPC transport: wait for the flags here, check, and leave the update unfused */
            const bool ipc_dbg = hq_ipc_ready(c) && c->debug_halo;
            if (ipc_dbg) hq_ipc_wait(c, &c->an, true, xs);
            hq_xchg_check(c, &c->an, true, xs);
            c->share_packed = false;
            if (c->nOI) {
                /* the update also packs the displacement sharing (phase 5 then only hands the records on) */
                hq_ipc_args ia = {};
                const bool fuse = !hq_set(c->opts.no_fused_share) && !(c->debug_halo && (hq_ipc_ready(c) || c->host_xchg));
                double* s_out = fuse ? c->an.d_s_out : nullptr;
                double* const* s_dst = nullptr;
                if (fuse && c->group && c->an.d_s_dst && !c->debug_halo) s_dst = c->an.d_s_dst;
                if (hq_ipc_ready(c)) {
                    hq_ipc_state* I = c->ipc;
                    if (fuse) {
                        s_dst = I->d_dst[1];
                        ia.wait_flags = I->d_flags;                     /* exchange 0: anchored-node contribution */
                        ia.wait_mask = I->wait_mask[0];
                        if (ia.wait_mask) ia.wait_epoch = ++I->recv_epoch[0];
                        ia.timeout_ticks = I->timeout_ticks;
                        ia.err = c->d_halo_err + 2;
                        ia.done = I->d_done + 1;
                        ia.nsig = I->nsig[1];
                        ia.sig = I->d_sig[1];
                        ia.sig_epoch = c->an.stotal ? ++I->send_epoch[1] : 0;
                        ia.delay_ticks = I->delay_ticks;
                        hq_k_interface_update<1><<<hq_blocks(c->nOI * 3, 256), 256, 0, xs>>>(
                            c->nOI, c->d_oi_node, c->d_oi_slot, c->d_oi_ptr, c->d_oi_pos, c->d_oi_fc, c->d_iforce, c->an.d_s_in,
                            c->d_nt, c->d_u[c->now], c->d_u[c->prev], unew, nullptr, s_dst, ia);
                        c->share_packed = true;
                        return HQ_OK;
                    }
                    if (!ipc_dbg) hq_ipc_wait(c, &c->an, true, xs);
                }
                hq_k_interface_update<0><<<hq_blocks(c->nOI * 3, 256), 256, 0, xs>>>(
                    c->nOI, c->d_oi_node, c->d_oi_slot, c->d_oi_ptr, c->d_oi_pos, c->d_oi_fc, c->d_iforce, c->an.d_s_in,
                    c->d_nt, c->d_u[c->now], c->d_u[c->prev], unew, s_dst ? nullptr : s_out, s_dst, ia);
                c->share_packed = fuse;
            } else if (hq_ipc_ready(c) && !ipc_dbg) {
                hq_ipc_wait(c, &c->an, true, xs);
            }
        } else {
            HQ_TRY(hq_xchg_recv(c, &c->an, ftab, true, true));
            HQ_TRY(hq_launch_update(c));                                   /* :4305 */
        }
        return HQ_OK;
    case 5: return hq_xchg_send(c, &c->an, unew, false, false);                      /* :4312 */
    case 6:
        HQ_TRY(hq_xchg_recv(c, &c->an, unew, false, false));
        if (c->ldnnum) {                                                   /* :4313 */
            /* the assignment reads anchors that the interior patches (compute stream) and the sharing
             * exchange (exchange stream) wrote, and the dangling-node sharing below packs what it writes */
            if (c->overlap) {
                HQ_HIP(hipEventRecord(c->ev_an_shared, c->cstream));
                HQ_HIP(hipStreamWaitEvent(c->stream, c->ev_an_shared, 0));
            }
            hq_k_adjust_assign<<<hq_blocks(c->ldnnum * 3, 256), 256, 0, c->stream>>>(
                c->ldnnum, c->d_dn_id, c->d_dn_ptr, c->d_dn_anchor, unew);
            if (c->overlap) {
                HQ_HIP(hipEventRecord(c->ev_assigned, c->stream));
                HQ_HIP(hipStreamWaitEvent(c->cstream, c->ev_assigned, 0));
            }
            /* the bricks of the NEXT step read hanging nodes (a simple node beside a level interface has them for
             * neighbours): where they run on a stream of their own, the event they wait for must lie BEHIND this
             * assignment, not only behind the patches (round 6: in an hq_run_timed batch the assignment is held back until
             * the step's bricks have ended and would otherwise run beside the next step's) */
            if (c->bstream) HQ_HIP(hipEventRecord(c->ev_patches, c->stream));
        }
        return HQ_OK;
    case 7: return hq_xchg_send(c, &c->dn, unew, false, false);                      /* :4315 */
    case 8:
        HQ_TRY(hq_xchg_recv(c, &c->dn, unew, false, false));
        if (patch) {
            if (c->att.split) HQ_TRY(hq_correction_join(c, c->att.corr, unew));
            if (c->nl.on) HQ_TRY(hq_correction_join(c, c->nl.corr, unew));
            if (c->overlap) HQ_HIP(hipEventRecord(c->ev_shared, c->cstream));
            if (hq_has_transport(c)) hq_clock(c, hq_ctx::HQ_CLK_CHAIN1, c->overlap ? c->cstream : c->stream);
            int n = c->now, p = c->prev, sp = c->spare;
            c->now = sp; c->prev = n; c->spare = p;
        } else {
            std::swap(c->now, c->prev);                                    /* :4271-4273 of the next iteration */
        }
        c->step++;
        return HQ_OK;
    }
    return HQ_OK;
}

static int hq_step(hq_ctx* c)
{
    for (int ph = 0; ph < HQ_NPHASE; ph++) HQ_TRY(hq_phase(c, ph));
    return HQ_OK;
}

/* ------------------------------------------------------------------------ */
/* C-ABI                                                                    */
/* ------------------------------------------------------------------------ */

/*
 * Patch variant on a partition: nodes named in the anchored-node schedule form
 * the "interface".  The patch kernel stores their partial force in a compact
 * table (one slot per interface node) instead of trusting its own update; the
 * contribution exchange adds the neighbours' partials to the owner's slot, the
 * owner updates the node (hq_k_interface_update) and shares the result.
 */
static int hq_setup_interface(hq_ctx* c, const hq_desc* d)
{
    if (c->an.ctotal == 0 && c->an.stotal == 0 && c->dn.ctotal == 0 && c->dn.stotal == 0) return HQ_OK;
    /*
     * Interface set: every node named in a schedule, plus the anchors of owned hanging nodes that
     * other ranks share (their force is complete only after the dangling-node contribution
     * exchange, psolve.c:4298-4299, so the anchors cannot be finished inside the patch kernel).
     */
    std::vector<int32_t> slot((size_t)c->N, -1);
    std::vector<char> nonowned((size_t)c->N, 0), dn_shared((size_t)c->N, 0);
    int32_t nI = 0;
    auto slot_of = [&](int32_t n) { if (slot[n] < 0) slot[n] = nI++; return slot[n]; };
    auto translate = [&](int32_t count, const hq_messenger* list, std::vector<int32_t>& out, char* mark) {
        for (int32_t i = 0; i < count; i++)
            for (int32_t k = 0; k < list[i].nodecount; k++) {
                out.push_back(slot_of(list[i].mapping[k]));
                if (mark) mark[list[i].mapping[k]] = 1;
            }
    };
    std::vector<int32_t> an_ss, an_cs, dn_ss, dn_cs;
    translate(d->an_sched.s_count, d->an_sched.first_s, an_ss, nullptr);
    translate(d->an_sched.c_count, d->an_sched.first_c, an_cs, nonowned.data());
    translate(d->dn_sched.s_count, d->dn_sched.first_s, dn_ss, dn_shared.data());
    translate(d->dn_sched.c_count, d->dn_sched.first_c, dn_cs, nonowned.data());
    std::vector<int32_t> sd;                                /* {src slot, dst slot, deps} */
    for (int32_t k = 0; k < c->ldnnum; k++) {
        int32_t dnode = d->dn_ldnid[k];
        if (!dn_shared[dnode]) continue;
        int32_t deps = d->dn_ptr[k + 1] - d->dn_ptr[k];
        for (int32_t a = d->dn_ptr[k]; a < d->dn_ptr[k + 1]; a++) {
            sd.push_back(slot_of(dnode));
            sd.push_back(slot_of(d->dn_lanid[a]));
            sd.push_back(deps);
        }
    }
    /* a node I own (s-list) cannot also be one I receive from its owner (c-list) */
    for (int32_t i = 0; i < d->an_sched.s_count; i++)
        for (int32_t k = 0; k < d->an_sched.first_s[i].nodecount; k++)
            if (nonowned[d->an_sched.first_s[i].mapping[k]])
                return hq_fail(HQ_ERR_ARG, "a node is listed both as owned (s-list) and as harbored from another rank (c-list)%s", "");
    std::vector<int32_t> oin, ois;
    for (int32_t n = 0; n < c->N; n++)
        if (slot[n] >= 0 && !nonowned[n]) { oin.push_back(n); ois.push_back(slot[n]); }
    c->nI = nI;
    c->nOI = (int32_t)oin.size();
    HQ_TRY(c->d_iforce.alloc(&c->bytes, (size_t)nI * 3));
    HQ_TRY(c->d_iforce.fill(0, c->stream));
    auto upload = [&](const std::vector<int32_t>& v, hq_dbuf<int32_t>& dst) -> int {
        return v.empty() ? HQ_OK : dst.put(&c->bytes, v, c->stream);
    };
    /* the schedules' entries as interface slots: memory of their own, and the force-table views point there */
    auto slots = [&](const std::vector<int32_t>& v, hq_dbuf<int32_t>& mem, int32_t** view) -> int {
        HQ_TRY(upload(v, mem));
        if (mem) *view = mem;
        return HQ_OK;
    };
    HQ_TRY(slots(an_cs, c->an.d_cslot, &c->an.d_cmap_f));
    HQ_TRY(slots(an_ss, c->an.d_sslot, &c->an.d_smap_f));
    HQ_TRY(slots(dn_cs, c->dn.d_cslot, &c->dn.d_cmap_f));
    HQ_TRY(slots(dn_ss, c->dn.d_sslot, &c->dn.d_smap_f));
    HQ_TRY(c->dist.build(sd, &c->bytes, c->stream));
    if (c->nOI) {
        /* records of the anchored-node contribution receive buffer per owned interface node,
         * messenger order */
        std::vector<int32_t> oi_index((size_t)nI, -1), ptr((size_t)c->nOI + 1, 0), pos(an_ss.size());
        for (int32_t i = 0; i < c->nOI; i++) oi_index[ois[i]] = i;
        for (size_t r = 0; r < an_ss.size(); r++) ptr[oi_index[an_ss[r]] + 1]++;
        for (int32_t i = 0; i < c->nOI; i++) ptr[i + 1] += ptr[i];
        std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
        for (size_t r = 0; r < an_ss.size(); r++) pos[fill[oi_index[an_ss[r]]]++] = (int32_t)r;
        if (an_ss.size() >= (size_t)1 << 24) return hq_fail(HQ_ERR_ARG, "more than 16M records in the anchored-node s-lists%s", "");
        std::vector<int32_t> fc((size_t)c->nOI, 0);
        for (int32_t i = 0; i < c->nOI; i++) {
            const int32_t cnt = ptr[(size_t)i + 1] - ptr[(size_t)i];
            if (cnt > 255) return hq_fail(HQ_ERR_ARG, "a node is shared by more than 255 ranks%s", "");
            fc[(size_t)i] = cnt ? (int32_t)(((uint32_t)cnt << 24) | (uint32_t)pos[(size_t)ptr[(size_t)i]]) : 0;
        }
        if (pos.empty()) pos.push_back(0);
        HQ_TRY(upload(fc, c->d_oi_fc));
        HQ_TRY(upload(oin, c->d_oi_node));
        HQ_TRY(upload(ois, c->d_oi_slot));
        HQ_TRY(upload(ptr, c->d_oi_ptr));
        HQ_TRY(upload(pos, c->d_oi_pos));
    }
    HQ_TRY(hq_patch_set_interface(c->opts, &c->plan, slot.data(), (int64_t)c->N, &c->bytes, c->stream));
    if (!hq_set(c->opts.no_overlap)) {
        /* the exchange chain is short and latency-bound: let its kernels (and RCCL's) get CUs ahead
         * of the thousands of interior patch workgroups queued on the compute stream */
        int prio_lo = 0, prio_hi = 0;
        HQ_HIP(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
        int prio = prio_hi;
#ifdef HQ_EXPERIMENT            /* profiles/tools only: does the chain's priority cost the brick launch beside it? */
        if (getenv("HQ_X_CHAIN_PRIO")) prio = !strcmp(getenv("HQ_X_CHAIN_PRIO"), "low") ? prio_lo : (prio_lo + prio_hi) / 2;
#endif
        HQ_HIP(hipStreamCreateWithPriority(&c->cstream, hipStreamNonBlocking, prio));
        HQ_HIP(hipEventCreateWithFlags(&c->ev_bnd, hipEventDisableTiming));
        HQ_HIP(hipEventCreateWithFlags(&c->ev_shared, hipEventDisableTiming));
        HQ_HIP(hipEventCreateWithFlags(&c->ev_an_shared, hipEventDisableTiming));
        HQ_HIP(hipEventCreateWithFlags(&c->ev_assigned, hipEventDisableTiming));
        HQ_HIP(hipEventRecord(c->ev_shared, c->cstream));
        /* whether the chain really runs beside the interior patches is decided with the transport:
         * hq_comm_init (RCCL between GPUs: yes) / hq_group_link (copies inside one GPU: no, see there) */
        c->can_overlap = true;
        c->reserve_cus = hq_value_or(c->opts.reserve_cus, 8);
    }
    return HQ_OK;
}

extern "C" int hq_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    int ok = 0;
    for (int i = 0; i < n; i++) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, i) == hipSuccess && strncmp(p.gcnArchName, "gfx950", 6) == 0) ok++;
    }
    return ok;
}

/* a node-ordered field [N][3] between the caller's numbering and the device's (c->perm; empty: the same) */
static int hq_field_to_device(hq_ctx* c, const hq_real* host, hq_real* dev)
{
    const size_t bytes = sizeof(hq_real) * 3 * (size_t)c->N;
    c->h2d_bytes += (int64_t)bytes;
    if (c->perm.empty()) return hq_copy_wait(dev, host, bytes, hipMemcpyHostToDevice, c->stream);
    std::vector<hq_real> tmp;
    try { tmp.resize(3 * (size_t)c->N); } catch (...) { return hq_fail(HQ_ERR_NOMEM, "out of host memory%s", ""); }
    const int32_t* pm = c->perm.data();
#pragma omp parallel for schedule(static) if (c->N > 262144)     /* small fields: a parallel region costs more than the loop */
    for (int64_t n = 0; n < (int64_t)c->N; n++) {
        const int64_t q = pm[n];
        tmp[(size_t)(3 * q)] = host[3 * n]; tmp[(size_t)(3 * q + 1)] = host[3 * n + 1]; tmp[(size_t)(3 * q + 2)] = host[3 * n + 2];
    }
    return hq_copy_wait(dev, tmp.data(), bytes, hipMemcpyHostToDevice, c->stream);
}

static int hq_field_to_host(hq_ctx* c, const hq_real* dev, hq_real* host)
{
    const size_t bytes = sizeof(hq_real) * 3 * (size_t)c->N;
    c->d2h_bytes += (int64_t)bytes;
    if (c->perm.empty()) return hq_copy_wait(host, dev, bytes, hipMemcpyDeviceToHost, c->stream);
    std::vector<hq_real> tmp;
    try { tmp.resize(3 * (size_t)c->N); } catch (...) { return hq_fail(HQ_ERR_NOMEM, "out of host memory%s", ""); }
    HQ_TRY(hq_copy_wait(tmp.data(), dev, bytes, hipMemcpyDeviceToHost, c->stream));
    const int32_t* pm = c->perm.data();
#pragma omp parallel for schedule(static) if (c->N > 262144)     /* small fields: a parallel region costs more than the loop */
    for (int64_t n = 0; n < (int64_t)c->N; n++) {
        const int64_t q = pm[n];
        host[3 * n] = tmp[(size_t)(3 * q)]; host[3 * n + 1] = tmp[(size_t)(3 * q + 1)]; host[3 * n + 2] = tmp[(size_t)(3 * q + 2)];
    }
    return HQ_OK;
}

static int hq_create_impl(const hq_desc* d, int device, const hq_options& opts, hq_ctx** out);

#include "hq_prepare.h"

extern "C" void hq_options_init(hq_options* o, uint64_t size)
{
    if (!o || size < sizeof(uint64_t)) return;         /* a struct that cannot even hold its size field is left alone */
    hq_options full;
    hq_options_defaults(&full);
    memcpy(o, &full, (size_t)std::min<uint64_t>(size, sizeof(full)));
    o->size = std::min<uint64_t>(size, sizeof(full));
}

extern "C" int hq_create_opts(const hq_desc* d, int device, const hq_options* opts, hq_ctx** out)
{
    if (opts && opts->size < sizeof(uint64_t)) return hq_fail(HQ_ERR_ARG, "hq_options.size is not set (hq_options_init)%s", "");
    hq_options full;
    hq_options_resolve(&full, opts);                   /* the environment is read here, once, and only if allowed */
    return hq_create_impl(d, device, full, out);
}

extern "C" int hq_create(const hq_desc* d, int device, hq_ctx** out) { return hq_create_opts(d, device, nullptr, out); }

extern "C" int hq_get_options(hq_ctx* c, hq_options* out, uint64_t size)
{
    if (!c || !out || size < sizeof(uint64_t)) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    memcpy(out, &c->opts, (size_t)std::min<uint64_t>(size, sizeof(c->opts)));
    out->size = std::min<uint64_t>(size, sizeof(c->opts));
    return HQ_OK;
}

static int hq_create_impl(const hq_desc* d, int device, const hq_options& opts, hq_ctx** out)
{
    if (!d || !out) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return hq_fail(HQ_ERR_NODEVICE, "no HIP device: this engine has no CPU path%s", "");
    if (device < 0 || device >= ndev) return hq_fail(HQ_ERR_ARG, "device index out of range%s", "");
    hipDeviceProp_t prop;
    HQ_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return hq_fail(HQ_ERR_NODEVICE, "device is %s, kernels are built for gfx950 only", prop.gcnArchName);
    HQ_HIP(hipSetDevice(device));
    const int variant = d->variant == HQ_VARIANT_AUTO ? HQ_VARIANT_PATCH : d->variant;
    if (variant != HQ_VARIANT_SCATTER && variant != HQ_VARIANT_PATCH) return hq_fail(HQ_ERR_ARG, "unknown variant%s", "");
    if (variant == HQ_VARIANT_PATCH && !d->node_xyz) {
        static bool warned = false;
        if (!warned && !hq_set(opts.quiet)) {
            warned = true;
            fprintf(stderr, "hq_create: hq_desc.node_xyz is NULL -- no bricks, no lattice / stencil patches (fixed runs of the node "
                            "order, element-form kernels only): expect about a third of the throughput; pass node_t.x/y/z\n");
        }
    }

    /* everything that needs no device (hq_prepare.h): from here on `d` is the description in DEVICE numbering (c->perm
     * maps the caller's ids); the start fields alone are still the caller's */
    const hq_real *h_tm1 = d->tm1, *h_tm2 = d->tm2;
    hq_prep prep;
    HQ_TRY(hq_prepare(d, opts, HQ_PREP_COEF | HQ_PREP_NT | (variant == HQ_VARIANT_PATCH ? HQ_PREP_BRICKS : 0), &prep));
    d = &prep.desc;
    std::vector<char>().swap(prep.excl);
    const hq_brick_host& BH = prep.bricks;
    const double* ntab = prep.ntab;

    hq_ctx* c = new (std::nothrow) hq_ctx();
    if (!c) return hq_fail(HQ_ERR_NOMEM, "out of host memory%s", "");
    c->device = device;
    c->opts = opts;
    c->E = d->lenum; c->N = d->nharbored; c->ldnnum = d->ldnnum;
    c->dt = d->deltaT; c->dt2 = d->deltaT * d->deltaT;
    c->rank = d->rank; c->nranks = d->nranks > 0 ? d->nranks : 1;
    c->variant = variant;
    c->perm = std::move(prep.perm);
    int rc = HQ_OK;
    auto bail = [&](int r) { hq_destroy(c); return r; };
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess)
        return bail(hq_fail(HQ_ERR_DEVICE, "hipStreamCreate failed%s", ""));
    if (hipEventCreateWithFlags(&c->ev_sent, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_output, hipEventDisableTiming) != hipSuccess)
        return bail(hq_fail(HQ_ERR_DEVICE, "hipEventCreate failed%s", ""));

    /* HQ_PATCH_VERBOSE: where hq_create's time goes */
    const bool verbose = hq_set(opts.verbose);
    auto t_last = std::chrono::steady_clock::now();
    auto lap = [&](const char* what, double s = -1.0) {
        const auto now = std::chrono::steady_clock::now();
        if (verbose) fprintf(stderr, "hq_create: %-34s %7.2f s\n", what, s >= 0.0 ? s : std::chrono::duration<double>(now - t_last).count());
        t_last = now;
    };
    if (prep.brick_plan_s > 0.0) lap("brick plan", prep.brick_plan_s);
    if (BH.nb > 0) lap("renumbering", prep.renumber_s);

    /* node state */
    size_t n3 = (size_t)c->N * 3;
    int nbuf = (variant == HQ_VARIANT_PATCH) ? 3 : 2;
    for (int b = 0; b < nbuf; b++) {
        if ((rc = c->d_u[b].alloc(&c->bytes, n3)) != HQ_OK || (rc = c->d_u[b].fill(0, c->stream)) != HQ_OK) return bail(rc);
    }
    {
        /* brick nodes are updated from the 3-double rows (plan.d_nt3) or the unit's record: their 7-double rows stay on
         * the host (189 M-element basin: 10.5 GB less to upload and to hold) */
        const int64_t nt_first = (variant == HQ_VARIANT_PATCH) ? BH.nb : 0;
        const size_t rows = (size_t)std::max<int64_t>(c->N - nt_first, 1);
        if ((rc = c->d_nt_rows.alloc(&c->bytes, rows * 7)) != HQ_OK) return bail(rc);
        if (c->N > nt_first && (rc = c->d_nt_rows.upload(ntab + 7 * nt_first, 7 * (size_t)(c->N - nt_first), c->stream)) != HQ_OK) return bail(rc);
        c->d_nt = c->d_nt_rows - 7 * nt_first;
    }
    lap("state buffers, n_t rows");
    if (h_tm1 && (rc = hq_field_to_device(c, h_tm1, c->d_u[c->now])) != HQ_OK) return bail(rc);
    if (h_tm2 && (rc = hq_field_to_device(c, h_tm2, c->d_u[c->prev])) != HQ_OK) return bail(rc);
    lap("start fields");

    if (c->ldnnum) {
        int32_t na = d->dn_ptr[c->ldnnum];
        if ((rc = c->d_dn_id.put(&c->bytes, d->dn_ldnid, (size_t)c->ldnnum, c->stream)) != HQ_OK ||
            (rc = c->d_dn_ptr.put(&c->bytes, d->dn_ptr, (size_t)c->ldnnum + 1, c->stream)) != HQ_OK ||
            (rc = c->d_dn_anchor.put(&c->bytes, d->dn_lanid, (size_t)na, c->stream)) != HQ_OK)
            return bail(rc);
    }

    if ((rc = c->d_halo_err.alloc(&c->bytes, 4)) != HQ_OK || (rc = c->d_halo_err.fill(0, c->stream)) != HQ_OK) return bail(rc);
    if (hq_set(opts.debug_halo) && c->nranks > 1) {
        /* the reference's -DDEBUG exchange: every halo record carries the global id of its node and the
         * receiver checks it (psolve.c:5002-5007, 5058-5069).  Identity = node_t.gnid where the caller
         * passes it, else a 64-bit mix of the node's coordinates (equal on every rank that harbors it). */
        if (!d->node_gnid && !d->node_xyz)
            return bail(hq_fail(HQ_ERR_ARG, "HQ_DEBUG_HALO needs hq_desc.node_gnid or node_xyz%s", ""));
        std::vector<int64_t> key((size_t)c->N);
        for (int64_t n = 0; n < c->N; n++) {
            if (d->node_gnid) { key[(size_t)n] = d->node_gnid[n]; continue; }
            uint64_t h = 0x9E3779B97F4A7C15ull;
            for (int k = 0; k < 3; k++) {
                h ^= (uint64_t)(uint32_t)d->node_xyz[3 * n + k];
                h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 29;
            }
            key[(size_t)n] = (int64_t)h;
        }
        if ((rc = c->d_gkey.put(&c->bytes, key, c->stream)) != HQ_OK) return bail(rc);
        c->debug_halo = true;
    }

    if (variant == HQ_VARIANT_SCATTER) {
        if ((rc = c->d_force.alloc(&c->bytes, n3)) != HQ_OK || (rc = c->d_force.fill(0, c->stream)) != HQ_OK) return bail(rc);
        c->Epad = (c->E + 63) & ~63;
        for (int64_t e = 0; e < c->E && !c->etable_damped; e++)
            c->etable_damped = d->eTable[4 * e + 2] != 0.0 || d->eTable[4 * e + 3] != 0.0;
        std::vector<int32_t> soa((size_t)8 * c->Epad, 0);
        for (int64_t e = 0; e < c->E; e++)
            for (int n = 0; n < 8; n++) soa[(size_t)n * c->Epad + e] = d->lnid[8 * e + n];
        if ((rc = c->d_lnid.put(&c->bytes, soa, c->stream)) != HQ_OK ||
            (rc = c->d_c1.put(&c->bytes, prep.c1.data(), (size_t)c->E, c->stream)) != HQ_OK ||
            (rc = c->d_c2.put(&c->bytes, prep.c2.data(), (size_t)c->E, c->stream)) != HQ_OK ||
            (rc = c->d_beta.put(&c->bytes, prep.beta.data(), (size_t)c->E, c->stream)) != HQ_OK)
            return bail(rc);
        if ((rc = hq_build_schedule(c, &d->an_sched, &c->an)) != HQ_OK) return bail(rc);
        if ((rc = hq_build_schedule(c, &d->dn_sched, &c->dn)) != HQ_OK) return bail(rc);
        if (c->ldnnum) {
            std::vector<int32_t> sd;                     /* {hanging node, anchor, deps} in the reference's loop order */
            for (int32_t k = 0; k < c->ldnnum; k++)
                for (int32_t a = d->dn_ptr[k]; a < d->dn_ptr[k + 1]; a++) {
                    sd.push_back(d->dn_ldnid[k]); sd.push_back(d->dn_lanid[a]); sd.push_back(d->dn_ptr[k + 1] - d->dn_ptr[k]);
                }
            if ((rc = c->dist.build(sd, &c->bytes, c->stream)) != HQ_OK) return bail(rc);
        }
    } else {
        c->plan.ragged_default = true;
        rc = hq_patch_build(opts, &c->plan, c->E, c->N, d->lnid, d->node_xyz, prep.c1.data(), prep.c2.data(), prep.beta.data(), ntab,
                            prep.dn, prep.seed0.data(), &c->bytes, c->stream, BH.nb);
        lap("patch plan");
        if (rc == HQ_OK && sizeof(hq_real) == sizeof(double)) {   /* what hq_attenuation_set_split will need of the mesh */
            for (int64_t e = 0; e < c->E && !c->etable_damped; e++)
                c->etable_damped = d->eTable[4 * e + 2] != 0.0 || d->eTable[4 * e + 3] != 0.0;
            if (!prep.p_lnid.empty()) c->h_lnid = std::move(prep.p_lnid);
            else c->h_lnid.assign(d->lnid, d->lnid + 8 * (size_t)c->E);
            prep.desc.lnid = c->h_lnid.data();            /* (d: the description reads the context's copy from here on) */
            c->h_c1 = std::move(prep.c1); c->h_c2 = std::move(prep.c2);
            c->h_mass.resize((size_t)c->N);
#pragma omp parallel for schedule(static)
            for (int64_t n = 0; n < c->N; n++) c->h_mass[(size_t)n] = ntab[7 * n];
        }
        if (rc == HQ_OK && BH.nb > 0) rc = hq_brick_upload(&c->bricks, BH, &c->bytes, c->stream);
        c->bricks.mat = { 0.0, 0.0, d->deltaT, d->mat_bbase, d->mat_threshold_damping, d->mat_threshold_vpvs };
        lap("brick upload");
        if (rc != HQ_OK) return bail(rc);
        /* one persistent workgroup per CU, the same number on every XCD (workgroups are dealt to the XCDs round-robin) */
        c->plan.grid_cus = std::max(8, prop.multiProcessorCount & ~7);
        if ((rc = hq_build_schedule(c, &d->an_sched, &c->an)) != HQ_OK) return bail(rc);
        if ((rc = hq_build_schedule(c, &d->dn_sched, &c->dn)) != HQ_OK) return bail(rc);
        if ((rc = hq_setup_interface(c, d)) != HQ_OK) return bail(rc);
        lap("schedules, interface");
    }
    if (hipDeviceSynchronize() != hipSuccess) return bail(hq_fail(HQ_ERR_DEVICE, "upload failed%s", ""));
    c->h2d_bytes = c->d2h_bytes = 0;          /* the counters of hq_info start with the first call behind hq_create */
    *out = c;
    return HQ_OK;
}

#include "hq_plan_check.h"

extern "C" int hq_destroy(hq_ctx* c)
{
    if (!c) return HQ_OK;
    hipSetDevice(c->device);
    if (c->stream) hq_quiesce(c);
    if (c->sstream) hipStreamSynchronize(c->sstream);
    if (c->comm && g_rccl.handle) g_rccl.CommDestroy(c->comm);
    if (c->ipc) {
        hq_ipc_state* I = c->ipc;
        for (void* p : I->opened) hipIpcCloseMemHandle(p);
        if (I->arena) hipFree(I->arena);
        delete I;
        c->ipc = nullptr;
    }
    hq_outputs_drop(c->snaps);
    if (c->sstream) hipStreamDestroy(c->sstream);
    for (hq_dev_schedule* sc : { &c->an, &c->dn }) {
        for (double* hp : { sc->h_c_out, sc->h_c_in, sc->h_s_out, sc->h_s_in })
            if (hp) hipHostFree(hp);
        for (int64_t* hp : { sc->h_c_out_id, sc->h_c_in_id, sc->h_s_out_id, sc->h_s_in_id })
            if (hp) hipHostFree(hp);
    }
    if (c->ev_sent) hipEventDestroy(c->ev_sent);
    if (c->ev_output) hipEventDestroy(c->ev_output);
    if (c->cstream) { hipStreamSynchronize(c->cstream); hipStreamDestroy(c->cstream); }
    if (c->bstream) { hipStreamSynchronize(c->bstream); hipStreamDestroy(c->bstream); }
    if (c->astream) { hipStreamSynchronize(c->astream); hipStreamDestroy(c->astream); }
    if (c->ev_att_fork) hipEventDestroy(c->ev_att_fork);
    if (c->ev_att_done) hipEventDestroy(c->ev_att_done);
    for (auto& sl : c->clock) for (hipEvent_t e : sl.e) if (e) hipEventDestroy(e);
    if (c->ev_patches) hipEventDestroy(c->ev_patches);
    if (c->ev_bricks) hipEventDestroy(c->ev_bricks);
    if (c->ev_bnd) hipEventDestroy(c->ev_bnd);
    if (c->ev_shared) hipEventDestroy(c->ev_shared);
    if (c->ev_an_shared) hipEventDestroy(c->ev_an_shared);
    if (c->ev_assigned) hipEventDestroy(c->ev_assigned);
    if (c->group) {
        /* unlink: the last member to go frees the table */
        std::vector<hq_ctx*>* g = c->group;
        bool any = false;
        for (auto& m : *g) { if (m == c) m = nullptr; any |= (m != nullptr); }
        if (!any) delete g;
    }
    hq_patch_free(&c->plan);
    hq_brick_free(&c->bricks);
    for (hipEvent_t e : c->ev) hipEventDestroy(e);
    for (int k = 0; k < 2; k++) if (c->ev_span[k]) hipEventDestroy(c->ev_span[k]);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;                                        /* the device arrays go with their owners (hq_devmem.h) */
    return HQ_OK;
}

extern "C" int hq_real_bytes(void) { return (int)sizeof(hq_real); }

extern "C" int hq_abi_version(void) { return HQ_ABI_VERSION; }

extern "C" int hq_get_info_sized(hq_ctx* c, hq_info* info, uint64_t size)
{
    if (!c || !info) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    hq_info v;
    memset(&v, 0, sizeof(v));
    v.variant = c->variant;
    v.npatches = c->plan.npatches;
    v.patch_pairs = c->plan.npairs;
    v.device_bytes = c->bytes;
    v.step = c->step;
    v.nranks = c->nranks;
    v.lattice_patches = c->plan.nlattice;
    v.stencil_patches = c->plan.nstencil;
    v.ragged_patches = c->plan.nragged;
    v.brick_units = c->bricks.nunits;
    v.brick_nodes = c->bricks.nb;
    v.brick_units_pernode = c->bricks.nunits - c->bricks.nsame - c->bricks.nhet - c->bricks.nrhet;
    v.brick_units_het = c->bricks.nhet + c->bricks.nrhet;
    v.brick_units_packed = c->bricks.npacked + c->bricks.nrpacked;
    v.brick_units_ragged = c->bricks.nrag;
    v.brick_units_ragged_het = c->bricks.nrhet;
    v.pcie_h2d_bytes = c->h2d_bytes;
    v.pcie_d2h_bytes = c->d2h_bytes;
    v.transport = c->comm ? 1 : (hq_ipc_ready(c) ? (c->ipc->loopback ? 5 : 2) : (c->host_xchg ? 3 : (c->group ? 4 : 0)));
    v.ipc_arena_coarse = (c->ipc && c->ipc->coarse) ? 1 : 0;
    v.ipc_arena_kind = c->ipc ? c->ipc->arena_kind : 0;
    v.debug_halo = c->debug_halo ? 1 : 0;
    v.brick_stream = c->bstream ? 1 : 0;
    hq_clock_harvest_all(c, false);                     /* what has finished; nothing is waited for */
    v.timed_steps = c->clk_steps;
    if (c->clk_steps > 0) {
        const double n = (double)c->clk_steps;
        v.t_step_us = c->clk_us[0] / n; v.t_shell_us = c->clk_us[1] / n; v.t_interior_us = c->clk_us[2] / n;
        v.t_chain_us = c->clk_us[3] / n; v.t_chain_exposed_us = c->clk_us[4] / n;
    }
    memset(info, 0, (size_t)size);
    memcpy(info, &v, (size_t)std::min<uint64_t>(size, sizeof(v)));
    return HQ_OK;
}

/* the symbol of the rounds before hq_get_info_sized: the struct of the last header that bound it ended with brick_nodes
 * (56 bytes); never more than that is written (include/hq_solver.h) */
extern "C" int hq_get_info(hq_ctx* c, hq_info* info) { return hq_get_info_sized(c, info, 56); }

/*
 * With the exchange chain on its own stream BETWEEN GPUs the compute stream must leave it somewhere to run: stream
 * priority does not preempt resident waves, and the brick launch of a partition is one wave of workgroups that fills
 * every CU's registers until it ends (130 us on an eighth of the 64M box).  So the compute stream is re-created with a
 * CU mask (hipExtStreamCreateWithCUMask) without `reserve_cus` CUs of the device (one per XCD); pack / RCCL / interface
 * kernels on the exchange stream find them free at any time.
 */
static int hq_mask_compute_stream(hq_ctx* c)
{
    if (!c->overlap || c->reserve_cus <= 0 || c->stream_masked) return HQ_OK;
    /* opt-in (HQ_CU_MASK=1): measured on one rank of an 8-way split of the 64M box alone on the GPU
     * (profiles/r03/rank_alone_trace.txt), the chain's kernels then do run beside the brick launch, but that launch
     * -- 512 workgroups for 496 slots -- takes 164 us instead of 122: a second, nearly empty round */
    if (!hq_set(c->opts.cu_mask)) return HQ_OK;
    hipDeviceProp_t prop;
    HQ_HIP(hipGetDeviceProperties(&prop, c->device));
    const int ncu = prop.multiProcessorCount;
    if (c->reserve_cus >= ncu) return HQ_OK;
    /* which CUs: index 33 k (k = 0 .. reserve - 1): one per XCD whether the runtime numbers the CUs XCD by XCD
     * (33 k / 32 = k) or deals them round-robin (33 k mod 8 = k mod 8) */
    std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0u);
    for (int i = 0; i < ncu; i++) mask[(size_t)i / 32] |= 1u << (i % 32);
    for (int k = 0; k < c->reserve_cus; k++) {
        const int i = (33 * k) % ncu;
        mask[(size_t)i / 32] &= ~(1u << (i % 32));
    }
    hipStream_t ns = nullptr;
    if (hipExtStreamCreateWithCUMask(&ns, (uint32_t)mask.size(), mask.data()) != hipSuccess) {
        (void)hipGetLastError();
        return HQ_OK;                            /* no CU masking on this runtime: the exchange waits for free CUs as before */
    }
    HQ_HIP(hq_quiesce(c));
    hipStreamDestroy(c->stream);
    c->stream = ns;
    c->stream_masked = true;
    c->plan.grid_cus = std::max(8, (ncu - c->reserve_cus) & ~7);
    return HQ_OK;
}

extern "C" int hq_comm_unique_id(void* id128)
{
    if (!id128) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    HQ_TRY(hq_rccl_load());
    hq_nccl_id id;
    HQ_NCCL(g_rccl.GetUniqueId(&id));
    memcpy(id128, &id, sizeof id);
    return HQ_OK;
}

extern "C" int hq_comm_init(hq_ctx* c, const void* id128)
{
    if (!c || !id128) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    HQ_TRY(hq_refuse_split(c, "hq_comm_init"));
    if (hq_has_transport(c)) return hq_fail(HQ_ERR_STATE, "context already has a transport%s", "");
    HQ_TRY(hq_rccl_load());
    HQ_HIP(hipSetDevice(c->device));
    hq_nccl_id id;
    memcpy(&id, id128, sizeof id);
    HQ_NCCL(g_rccl.CommInitRank(&c->comm, c->nranks, id, c->rank));
    /* between GPUs the exchange is latency the interior patches can hide: run the chain on its own stream */
    c->overlap = c->can_overlap && c->opts.overlap != 0;
    return hq_mask_compute_stream(c);
}

extern "C" int hq_comm_selftest(hq_ctx* c, int32_t count)
{
    if (!c || count < 1) return hq_fail(HQ_ERR_ARG, "bad argument%s", "");
    if (!c->comm) return hq_fail(HQ_ERR_STATE, "hq_comm_selftest needs hq_comm_init%s", "");
    HQ_HIP(hipSetDevice(c->device));
    hipStream_t xs = c->overlap ? c->cstream : c->stream;
    std::vector<double> h((size_t)count), back((size_t)count, 0.0);
    for (int32_t i = 0; i < count; i++) h[i] = 1.0 + 0.5 * i;
    hq_dbuf<double> d_out, d_in;                     /* not counted: gone when this returns, however it returns */
    HQ_TRY(d_out.put(nullptr, h, xs));
    HQ_TRY(d_in.alloc(nullptr, (size_t)count));
    HQ_TRY(d_in.fill(0, xs));
    HQ_NCCL(g_rccl.GroupStart());
    HQ_NCCL(g_rccl.Recv(d_in, (size_t)count, HQ_NCCL_DOUBLE, c->rank, c->comm, xs));
    HQ_NCCL(g_rccl.Send(d_out, (size_t)count, HQ_NCCL_DOUBLE, c->rank, c->comm, xs));
    HQ_NCCL(g_rccl.GroupEnd());
    HQ_TRY(hq_copy_wait(back.data(), d_in, sizeof(double) * count, hipMemcpyDeviceToHost, xs));
    for (int32_t i = 0; i < count; i++)
        if (back[i] != h[i]) return hq_fail(HQ_ERR_COMM, "self send/recv through RCCL returned other data than was sent%s", "");
    return HQ_OK;
}

extern "C" int hq_comm_init_host(hq_ctx* c, hq_host_exchange_fn fn, void* user)
{
    if (!c || !fn) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    HQ_TRY(hq_refuse_split(c, "hq_comm_init_host"));
    if (hq_has_transport(c)) return hq_fail(HQ_ERR_STATE, "context already has a transport%s", "");
    c->host_xchg = fn;
    c->host_user = user;
    /* as between GPUs: the chain on its own stream, so that the host waits for the exchange stream only */
    c->overlap = c->can_overlap && c->opts.overlap != 0;
    return hq_mask_compute_stream(c);
}

/* ------------------------------------------------------------------------ */
/* IPC transport (between processes on one node; include/hq_solver.h)       */
/* ------------------------------------------------------------------------ */

static std::vector<hq_dev_messenger>& hq_ipc_list(hq_ctx* c, int x, bool sending)
{
    hq_dev_schedule* s = x < 2 ? &c->an : &c->dn;
    const bool contribution = !(x & 1);
    if (sending) return contribution ? s->c : s->s;
    return contribution ? s->s : s->c;
}

static double** hq_ipc_inbuf(hq_ctx* c, int x)
{
    hq_dev_schedule* s = x < 2 ? &c->an : &c->dn;
    return (x & 1) ? &s->d_c_in : &s->d_s_in;
}

static hq_dbuf<double>& hq_ipc_inbuf_mem(hq_ctx* c, int x)
{
    hq_dev_schedule* s = x < 2 ? &c->an : &c->dn;
    return (x & 1) ? s->c_in_mem : s->s_in_mem;
}

static int32_t hq_ipc_total(hq_ctx* c, int x, bool sending)
{
    hq_dev_schedule* s = x < 2 ? &c->an : &c->dn;
    const bool contribution = !(x & 1);
    if (sending) return contribution ? s->ctotal : s->stotal;
    return contribution ? s->stotal : s->ctotal;
}

static bool hq_ipc_ready(const hq_ctx* c) { return c->ipc && c->ipc->ready; }

/* the arena: flags, the four receive buffers (moved here from their own allocations), a dump row */
static int hq_ipc_prepare(hq_ctx* c)
{
    if (c->ipc) return HQ_OK;
    if (hq_has_transport(c)) return hq_fail(HQ_ERR_STATE, "context already has a transport%s", "");
    for (int x = 0; x < 4; x++)
        if (hq_ipc_list(c, x, false).size() > HQ_IPC_MAXNB || hq_ipc_list(c, x, true).size() > HQ_IPC_MAXNB)
            return hq_fail(HQ_ERR_ARG, "IPC transport: more than %s neighbours in one schedule", "64");
    HQ_HIP(hipSetDevice(c->device));
    HQ_HIP(hq_quiesce(c));
    hq_ipc_state* I = new (std::nothrow) hq_ipc_state();
    if (!I) return hq_fail(HQ_ERR_NOMEM, "out of host memory%s", "");
    memset(&I->mine, 0, sizeof(I->mine));
    hq_ipc_blob& B = I->mine;
    B.magic = HQ_IPC_MAGIC; B.version = HQ_ABI_VERSION;
    B.rank = c->rank; B.nranks = c->nranks; B.device = c->device; B.pid = (int32_t)getpid();
    size_t off = sizeof(unsigned long long) * 4 * HQ_IPC_MAXNB;
    B.flag_off = 0;
    for (int x = 0; x < 4; x++) {
        B.buf_off[x] = off;
        off += ((size_t)hq_ipc_total(c, x, false) * 24 + 255) / 256 * 256;
    }
    const size_t dump_off = off;
    off += 256;
    if (c->debug_halo)                               /* the check words of every received record (hq_k_pack_check) */
        for (int x = 0; x < 4; x++) {
            B.id_off[x] = off;
            off += ((size_t)hq_ipc_total(c, x, false) * 8 + 255) / 256 * 256 + 256;
        }
    I->arena_bytes = off;
    /* everything that can fail comes before the schedules' receive buffers are touched (round-4 advisor) */
    if (I->d_done.alloc(nullptr, 4) != HQ_OK || I->d_done.fill(0, c->stream) != HQ_OK) {
        delete I;
        return hq_fail(HQ_ERR_NOMEM, "hipMalloc failed%s", "");
    }
    /* fine-grained device memory: remote stores over xGMI become visible to the local consumer kernels without an L2
     * flush (what RCCL uses for its buffers); where the runtime cannot export it, coarse-grained memory -- coherent only
     * between ranks that share the device, which hq_comm_init_ipc checks */
    /* three kinds of memory, in this order: fine-grained (what RCCL uses for its buffers), uncached (MTYPE_UC: no L2
     * holds it either, so remote stores are seen as well -- for runtimes that will not export a fine-grained
     * allocation), and coarse-grained as the last resort (ranks of ONE device only).  HQ_IPC_COARSE=1 / HQ_IPC_ARENA=
     * fine | uncached | coarse pins the kind (tests). */
    const char* coarse_env = hq_opt_env_only(c->opts, "HQ_IPC_COARSE");
    bool coarse = coarse_env && atoi(coarse_env) != 0;
    int first_kind = coarse ? 2 : 0, last_kind = 2;
    if (hq_given(c->opts.ipc_arena)) first_kind = last_kind = std::min(2, c->opts.ipc_arena);
    for (int attempt = first_kind; attempt <= last_kind; attempt++) {
        hipError_t e = attempt == 0 ? hipExtMallocWithFlags(&I->arena, I->arena_bytes, hipDeviceMallocFinegrained)
                     : attempt == 1 ? hipExtMallocWithFlags(&I->arena, I->arena_bytes, hipDeviceMallocUncached)
                                    : hipMalloc(&I->arena, I->arena_bytes);
        if (e == hipSuccess) e = hipIpcGetMemHandle(&B.mem, I->arena);
        if (e == hipSuccess) { coarse = attempt == 2; I->arena_kind = attempt; break; }
        (void)hipGetLastError();
        if (I->arena) { hipFree(I->arena); I->arena = nullptr; }
        if (attempt == last_kind) {
            delete I;
            return hq_fail(HQ_ERR_DEVICE, "IPC transport: cannot allocate / export the receive arena: %s", hipGetErrorString(e));
        }
    }
    I->coarse = coarse;
    B.coarse = coarse ? 1 : 0;
    B.arena_bytes = I->arena_bytes;
    B.arena_addr = (uint64_t)(uintptr_t)I->arena;
    if (hipDeviceGetPCIBusId(B.busid, (int)sizeof(B.busid), c->device) != hipSuccess) B.busid[0] = 0;
    /* (zeroed BEFORE the blob leaves this rank: a peer raises flags in here as soon as it steps, and a hipMemset on the null
     *  stream is finished only when the device says so) */
    if (hipMemset(I->arena, 0, I->arena_bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { hipFree(I->arena); delete I; return hq_fail(HQ_ERR_DEVICE, "memset%s", ""); }
    c->bytes += (int64_t)I->arena_bytes;
    I->d_flags = (unsigned long long*)I->arena;
    for (int x = 0; x < 4; x++) {
        double** pin = hq_ipc_inbuf(c, x);           /* the receive buffer moves into the arena: its own memory goes */
        hq_ipc_inbuf_mem(c, x).reset();
        *pin = hq_ipc_total(c, x, false) ? (double*)((char*)I->arena + B.buf_off[x]) : nullptr;
        std::vector<hq_dev_messenger>& rcv = hq_ipc_list(c, x, false);
        B.nrecv[x] = (int32_t)rcv.size();
        for (size_t j = 0; j < rcv.size(); j++) {
            B.recv[x][j].procid = rcv[j].procid; B.recv[x][j].offset = rcv[j].offset; B.recv[x][j].count = rcv[j].nodecount;
            if (rcv[j].nodecount) I->wait_mask[x] |= 1ull << j;
        }
    }
    B.reserved = (int32_t)(dump_off / 8);
    if (c->debug_halo)
        for (int x = 0; x < 4; x++) I->d_in_id[x] = (int64_t*)((char*)I->arena + B.id_off[x]);
    if (hq_set(c->opts.ipc_timeout_ms)) I->timeout_ticks = (unsigned long long)(c->opts.ipc_timeout_ms * 1.0e5);
    c->ipc = I;
    return HQ_OK;
}

extern "C" int hq_comm_ipc_export(hq_ctx* c, void* blob)
{
    if (!c || !blob) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    HQ_TRY(hq_ipc_prepare(c));
    memset(blob, 0, HQ_IPC_BLOB_BYTES);
    memcpy(blob, &c->ipc->mine, sizeof(hq_ipc_blob));
    return HQ_OK;
}

/* dst / sig tables of exchange x from (peer arena base, peer blob) pairs; loopback: everything into this rank's own arena */
static int hq_ipc_connect(hq_ctx* c, const char* blobs)
{
    hq_ipc_state* I = c->ipc;
    const bool loop = blobs == nullptr;
    std::vector<void*> base((size_t)c->nranks, nullptr);
    auto peer_base = [&](int32_t r, const hq_ipc_blob** pbo) -> int {
        const hq_ipc_blob* pb = (const hq_ipc_blob*)(blobs + (size_t)r * HQ_IPC_BLOB_BYTES);
        *pbo = pb;
        if (pb->magic != HQ_IPC_MAGIC || pb->version != HQ_ABI_VERSION || pb->rank != r || pb->nranks != c->nranks)
            return hq_fail(HQ_ERR_ARG, "IPC transport: blob %s is not the export of that rank of this run", "r");
        if (base[(size_t)r]) return HQ_OK;
        if ((pb->coarse || I->coarse) && strncmp(pb->busid, I->mine.busid, sizeof(pb->busid)) != 0)
            return hq_fail(HQ_ERR_DEVICE, "IPC transport: a coarse-grained receive arena is coherent only between ranks of ONE device%s", "");
        if (pb->pid == I->mine.pid) {
            base[(size_t)r] = (void*)(uintptr_t)pb->arena_addr;         /* a context of this process: its pointer is ours */
            if (strncmp(pb->busid, I->mine.busid, sizeof(pb->busid)) != 0) {
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, c->device, pb->device) != hipSuccess || !can)
                    return hq_fail(HQ_ERR_DEVICE, "IPC transport: no peer access between the devices of two contexts%s", "");
                hipError_t e = hipDeviceEnablePeerAccess(pb->device, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return hq_fail(HQ_ERR_DEVICE, "hipDeviceEnablePeerAccess: %s", hipGetErrorString(e));
                (void)hipGetLastError();
            }
        } else {
            void* p = nullptr;
            hipError_t e = hipIpcOpenMemHandle(&p, pb->mem, hipIpcMemLazyEnablePeerAccess);
            if (e != hipSuccess) return hq_fail(HQ_ERR_DEVICE, "hipIpcOpenMemHandle: %s", hipGetErrorString(e));
            I->opened.push_back(p);
            base[(size_t)r] = p;
        }
        return HQ_OK;
    };
    for (int x = 0; x < 4; x++) {
        std::vector<hq_dev_messenger>& snd = hq_ipc_list(c, x, true);
        const int32_t total = hq_ipc_total(c, x, true);
        std::vector<double*> dst((size_t)total, nullptr);
        std::vector<int64_t*> dst_id((size_t)(c->debug_halo ? total : 0), nullptr);
        std::vector<unsigned long long*> sig;
        if (loop) {
            const int32_t in_total = hq_ipc_total(c, x, false);
            double* in = *hq_ipc_inbuf(c, x);
            double* dump = (double*)I->arena + I->mine.reserved;
            for (int32_t i = 0; i < total; i++) dst[(size_t)i] = in_total ? in + 3 * (int64_t)(i % in_total) : dump;
            if (c->debug_halo)
                for (int32_t i = 0; i < total; i++) dst_id[(size_t)i] = I->d_in_id[x] + (in_total ? i % in_total : 0);
            if (!total) I->wait_mask[x] = 0;
            for (int j = 0; j < HQ_IPC_MAXNB; j++)
                if ((I->wait_mask[x] >> j) & 1ull) sig.push_back(I->d_flags + (size_t)x * HQ_IPC_MAXNB + j);
        } else {
            for (auto& m : snd) {
                if (!m.nodecount) continue;
                if (m.procid < 0 || m.procid >= c->nranks) return hq_fail(HQ_ERR_ARG, "IPC transport: a messenger names a rank outside the run%s", "");
                const hq_ipc_blob* pb = nullptr;
                HQ_TRY(peer_base(m.procid, &pb));
                int j = -1;
                for (int q = 0; q < pb->nrecv[x] && q < HQ_IPC_MAXNB; q++) if (pb->recv[x][q].procid == c->rank) j = q;
                if (j < 0 || pb->recv[x][j].count != m.nodecount) return hq_fail(HQ_ERR_ARG, "neighbour schedules do not match%s", "");
                char* pbase = (char*)base[(size_t)m.procid];
                double* p_in = (double*)(pbase + pb->buf_off[x]);
                for (int32_t k = 0; k < m.nodecount; k++) dst[(size_t)m.offset + k] = p_in + 3 * ((int64_t)pb->recv[x][j].offset + k);
                if (c->debug_halo) {
                    if (!pb->id_off[x]) return hq_fail(HQ_ERR_STATE, "HQ_DEBUG_HALO must be set on every rank of an IPC run%s", "");
                    int64_t* p_id = (int64_t*)(pbase + pb->id_off[x]);
                    for (int32_t k = 0; k < m.nodecount; k++) dst_id[(size_t)m.offset + k] = p_id + ((int64_t)pb->recv[x][j].offset + k);
                } else if (pb->id_off[x]) {
                    return hq_fail(HQ_ERR_STATE, "HQ_DEBUG_HALO must be set on every rank of an IPC run%s", "");
                }
                sig.push_back((unsigned long long*)(pbase + pb->flag_off) + (size_t)x * HQ_IPC_MAXNB + j);
            }
        }
        I->nsig[x] = (int32_t)sig.size();
        if (total) {
            HQ_TRY(I->d_dst[x].put(&c->bytes, dst, c->stream));
            HQ_TRY(I->d_sig[x].put(&c->bytes, sig, c->stream));
            if (c->debug_halo) HQ_TRY(I->d_dst_id[x].put(&c->bytes, dst_id, c->stream));
        }
    }
    I->ready = true;
    I->loopback = loop;
    if (loop && hq_given(c->opts.loopback_delay_us)) I->delay_ticks = (unsigned long long)(c->opts.loopback_delay_us * 100.0);
    /* as between GPUs: the chain on its own stream beside the interior work */
    c->overlap = c->can_overlap && c->opts.overlap != 0;
    return hq_mask_compute_stream(c);
}

extern "C" int hq_comm_init_ipc(hq_ctx* c, const void* blobs)
{
    if (!c || !blobs) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    HQ_TRY(hq_refuse_split(c, "hq_comm_init_ipc"));
    if (!c->ipc) return hq_fail(HQ_ERR_STATE, "hq_comm_init_ipc needs the blobs of hq_comm_ipc_export (this rank's among them)%s", "");
    if (hq_has_transport(c)) return hq_fail(HQ_ERR_STATE, "context already has a transport%s", "");
    HQ_HIP(hipSetDevice(c->device));
    return hq_ipc_connect(c, (const char*)blobs);    /* (the destination / flag tables are in place when it returns) */
}

/* the same with the number of blobs the caller holds: a short all-gather is refused instead of read out of bounds */
extern "C" int hq_comm_init_ipc_n(hq_ctx* c, const void* blobs, int32_t nblobs)
{
    if (c && nblobs != c->nranks) return hq_fail(HQ_ERR_ARG, "hq_comm_init_ipc_n: one blob per rank, in rank order%s", "");
    return hq_comm_init_ipc(c, blobs);
}

extern "C" int hq_comm_init_loopback(hq_ctx* c)
{
    if (!c) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    HQ_TRY(hq_refuse_split(c, "hq_comm_init_loopback"));
    HQ_TRY(hq_ipc_prepare(c));
    if (hq_has_transport(c)) return hq_fail(HQ_ERR_STATE, "context already has a transport%s", "");
    return hq_ipc_connect(c, nullptr);
}

extern "C" int hq_group_link(hq_ctx** ctxs, int32_t n)
{
    if (!ctxs || n < 1) return hq_fail(HQ_ERR_ARG, "bad argument%s", "");
    for (int32_t i = 0; i < n; i++) {
        if (!ctxs[i] || ctxs[i]->rank != i || ctxs[i]->nranks != n)
            return hq_fail(HQ_ERR_ARG, "group member %s must be the context of rank i of n", "i");
        HQ_TRY(hq_refuse_split(ctxs[i], "hq_group_link"));
        if (hq_has_transport(ctxs[i])) return hq_fail(HQ_ERR_STATE, "context already has a transport%s", "");
        for (hq_dev_schedule* sc : { &ctxs[i]->an, &ctxs[i]->dn })
            for (auto* lst : { &sc->c, &sc->s })
                for (auto& m : *lst)
                    if (m.procid < 0 || m.procid >= n) return hq_fail(HQ_ERR_ARG, "a messenger names a rank outside the group%s", "");
    }
    /* members on DIFFERENT devices: the records travel by peer stores / peer copies, which need peer access both ways
     * (checked and enabled here, not discovered by a failing copy in the middle of a step) */
    bool one_device = true;
    for (int32_t i = 1; i < n; i++) one_device = one_device && ctxs[i]->device == ctxs[0]->device;
    if (!one_device) {
        for (int32_t i = 0; i < n; i++)
            for (int32_t j = 0; j < n; j++) {
                if (ctxs[i]->device == ctxs[j]->device) continue;
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, ctxs[i]->device, ctxs[j]->device) != hipSuccess || !can)
                    return hq_fail(HQ_ERR_DEVICE, "hq_group_link: no peer access between the devices of two members%s", "");
                HQ_HIP(hipSetDevice(ctxs[i]->device));
                hipError_t e = hipDeviceEnablePeerAccess(ctxs[j]->device, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
                    return hq_fail(HQ_ERR_DEVICE, "hipDeviceEnablePeerAccess: %s", hipGetErrorString(e));
                (void)hipGetLastError();
            }
    }
    /* Everything that can fail is built FIRST, in tables of this call; the contexts are touched only when all of it
     * exists (round-3 advisor: a failure half-way used to leave members linked to a group without its tables). */
    struct dst_table { hq_ctx* c; int which, contribution; std::vector<double*> dst; };
    std::vector<dst_table> tables;
    /* members of ONE device: the pack kernel writes where the peers read.  Across devices the records go through peer
     * COPIES (hipMemcpyAsync), whose coherence with the destination device's L2 the runtime answers for -- plain peer
     * stores into coarse-grained memory do not have it; the IPC transport with its fine-grained arena is the
     * peer-store path between devices */
    const bool direct = one_device && !hq_set(ctxs[0]->opts.group_copies);      /* the group follows its first member's options */
    if (direct) {
        for (int32_t i = 0; i < n; i++) {
            hq_ctx* c = ctxs[i];
            for (int which = 0; which < 2; which++) {
                hq_dev_schedule* s = which ? &c->dn : &c->an;
                for (int contribution = 0; contribution < 2; contribution++) {
                    std::vector<hq_dev_messenger>& snd = contribution ? s->c : s->s;
                    const int32_t total = contribution ? s->ctotal : s->stotal;
                    if (!total) continue;
                    dst_table T{ c, which, contribution, std::vector<double*>((size_t)total, nullptr) };
                    for (auto& m : snd) {
                        if (!m.nodecount) continue;
                        hq_ctx* peer = ctxs[m.procid];
                        hq_dev_schedule* ps = which ? &peer->dn : &peer->an;
                        std::vector<hq_dev_messenger>& prcv = contribution ? ps->s : ps->c;
                        double* p_in = contribution ? ps->d_s_in : ps->d_c_in;
                        const hq_dev_messenger* pm = nullptr;
                        for (auto& q : prcv) if (q.procid == c->rank) pm = &q;
                        if (!pm || pm->nodecount != m.nodecount) return hq_fail(HQ_ERR_ARG, "neighbour schedules do not match%s", "");
                        for (int32_t k = 0; k < m.nodecount; k++) T.dst[(size_t)m.offset + k] = p_in + 3 * ((int64_t)pm->offset + k);
                    }
                    tables.push_back(std::move(T));
                }
            }
        }
    }
    std::vector<hq_dbuf<double*>> uploaded(tables.size());   /* each on its member's device and compute stream, in its ledger */
    for (size_t k = 0; k < tables.size(); k++) {
        hq_ctx* tc = tables[k].c;
        hipSetDevice(tc->device);
        if (uploaded[k].put(&tc->bytes, tables[k].dst, tc->stream) != HQ_OK)
            return hq_fail(HQ_ERR_NOMEM, "hq_group_link: destination tables%s", "");
    }
    std::vector<hq_ctx*>* g = new (std::nothrow) std::vector<hq_ctx*>(ctxs, ctxs + n);
    if (!g) return hq_fail(HQ_ERR_NOMEM, "out of host memory%s", "");
    /* publish.  Partitions that share ONE GPU gain nothing from a second stream -- the other partitions' patches fill
     * the device anyway -- and pay for its events: the 64M box in 8 in-process partitions steps in 2.54 ms on one
     * stream per partition against 3.28 ms with the chain on a second one (round 2; HQ_OVERLAP=1 forces it, which is
     * how the GPU tests cover that path without a second GPU). */
    const bool ov = hq_set(ctxs[0]->opts.overlap);
    for (int32_t i = 0; i < n; i++) { ctxs[i]->group = g; ctxs[i]->overlap = ov && ctxs[i]->can_overlap; }
    for (size_t k = 0; k < tables.size(); k++) {
        hq_dev_schedule* s = tables[k].which ? &tables[k].c->dn : &tables[k].c->an;
        (tables[k].contribution ? s->d_c_dst : s->d_s_dst) = std::move(uploaded[k]);
    }
    return HQ_OK;
}

extern "C" int hq_group_run(hq_ctx** ctxs, int32_t n, int32_t nsteps)
{
    if (!ctxs || n < 1 || nsteps < 0) return hq_fail(HQ_ERR_ARG, "bad argument%s", "");
    for (int32_t i = 0; i < n; i++)
        if (!ctxs[i] || !ctxs[i]->group || (int32_t)ctxs[i]->group->size() != n || (*ctxs[i]->group)[i] != ctxs[i])
            return hq_fail(HQ_ERR_STATE, "contexts are not linked (hq_group_link)%s", "");
    /* a destroyed member leaves a hole in the group's table: its neighbours' pack kernels would write into freed receive
     * buffers, so a group steps complete or not at all */
    for (hq_ctx* m : *ctxs[0]->group)
        if (!m) return hq_fail(HQ_ERR_STATE, "a member of the group has been destroyed: the others cannot step any more%s", "");
    for (int32_t i = 0; i < n; i++) HQ_TRY(hq_output_check_room(ctxs[i], nsteps));
    for (int32_t s = 0; s < nsteps; s++)
        for (int ph = 0; ph < HQ_NPHASE; ph++)
            for (int32_t i = 0; i < n; i++) {
                HQ_HIP(hipSetDevice(ctxs[i]->device));
                HQ_TRY(hq_phase(ctxs[i], ph));
            }
    HQ_HIP(hipGetLastError());
    return HQ_OK;
}

extern "C" int hq_set_source(hq_ctx* c, int32_t nloaded, const int32_t* loaded, int32_t step0,
                             int32_t nsteps, const double* F)
{
    if (!c || nloaded < 0 || nsteps < 0 || (nloaded && nsteps && (!loaded || !F)))
        return hq_fail(HQ_ERR_ARG, "bad source description%s", "");
    HQ_HIP(hipSetDevice(c->device));
    HQ_HIP(hq_quiesce(c));
    for (int32_t i = 0; i < nloaded; i++)
        if (loaded[i] < 0 || loaded[i] >= c->N) return hq_fail(HQ_ERR_ARG, "loaded node id out of range%s", "");
    const int32_t* caller_ids = loaded;
    std::vector<int32_t> dev_ids;                        /* the loaded nodes in device numbering */
    if (!c->perm.empty() && nloaded > 0) {
        dev_ids.resize((size_t)nloaded);
        for (int32_t i = 0; i < nloaded; i++) dev_ids[(size_t)i] = c->perm[(size_t)loaded[i]];
        loaded = dev_ids.data();
    }
    /* the next window of the same loaded nodes (a host that steps window by window, or step by step as the stub of
     * INTEGRATION.md does inside the reference's loop): only the force table travels */
    const bool same_nodes = nloaded > 0 && nsteps > 0 && c->d_loaded && (int32_t)c->h_loaded.size() == nloaded &&
                            memcmp(c->h_loaded.data(), loaded, sizeof(int32_t) * (size_t)nloaded) == 0 &&
                            (size_t)nloaded * 3 * (size_t)nsteps <= c->F_capacity;
    if (same_nodes) {
        c->src_step0 = step0; c->src_nsteps = nsteps;
        HQ_TRY(c->d_F.upload(F, 3 * (size_t)nloaded * (size_t)nsteps, c->stream));
        c->h2d_bytes += 24 * (int64_t)nloaded * nsteps;
        return HQ_OK;
    }
    /* a node named twice: hq_k_source assigns F dt^2 (two threads, one slot) where the brick and patch kernels add both
     * rows, and the reference's theNodesLoadedList holds every node once -- refused before anything is reset, so the
     * context keeps the source it had.  Only here: the same-nodes path compared against a list already accepted. */
    if (nloaded > 1 && nsteps > 0) {
        std::vector<int32_t> sorted(caller_ids, caller_ids + nloaded);     /* (the renumbering is one to one) */
        std::sort(sorted.begin(), sorted.end());
        const auto twice = std::adjacent_find(sorted.begin(), sorted.end());
        if (twice != sorted.end()) {
            char n[32];
            snprintf(n, sizeof n, "%d", *twice);
            return hq_fail(HQ_ERR_ARG, "loaded node %s is named twice in one list (every node once, as theNodesLoadedList)", n);
        }
    }
    c->d_loaded.reset();
    c->d_F.reset();
    c->nloaded = 0; c->src_step0 = step0; c->src_nsteps = nsteps;   /* no source until every table is in place: a failure */
    c->h_loaded.clear(); c->F_capacity = 0;                         /* below leaves the context stepping without one      */
    if (nloaded && nsteps) {
        HQ_TRY(c->d_loaded.put(&c->bytes, loaded, (size_t)nloaded, c->stream));
        HQ_TRY(c->d_F.put(&c->bytes, F, (size_t)nloaded * 3 * (size_t)nsteps, c->stream));
        c->h2d_bytes += 4 * (int64_t)nloaded + 24 * (int64_t)nloaded * nsteps;
        c->h_loaded.assign(loaded, loaded + nloaded);
        c->F_capacity = (size_t)nloaded * 3 * (size_t)nsteps;
    }
    if (c->variant == HQ_VARIANT_PATCH) {
        HQ_TRY(hq_patch_set_source(&c->plan, (nloaded && nsteps) ? nloaded : 0, loaded, &c->bytes, c->stream));
        HQ_TRY(hq_brick_set_source(&c->bricks, (nloaded && nsteps) ? nloaded : 0, loaded, &c->bytes, c->stream));
    }
    c->nloaded = nloaded;
    return HQ_OK;
}

extern "C" int hq_run(hq_ctx* c, int32_t nsteps)
{
    if (!c || nsteps < 0) return hq_fail(HQ_ERR_ARG, "bad argument%s", "");
    if (c->group && c->group->size() > 1)
        return hq_fail(HQ_ERR_STATE, "linked contexts are stepped with hq_group_run%s", "");
    HQ_TRY(hq_output_check_room(c, nsteps));
    HQ_HIP(hipSetDevice(c->device));
    for (int32_t s = 0; s < nsteps; s++) HQ_TRY(hq_step(c));
    HQ_HIP(hipGetLastError());
    return HQ_OK;
}

extern "C" int hq_sync(hq_ctx* c)
{
    if (!c) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    HQ_HIP(hipSetDevice(c->device));
    HQ_HIP(hq_quiesce(c));
    if (c->sstream) HQ_HIP(hipStreamSynchronize(c->sstream));     /* the snapshots' copies */
    hq_clock_harvest_all(c, true);
    if (c->ipc) {
        int32_t late = 0;
        HQ_TRY(hq_copy_wait(&late, c->d_halo_err + 2, sizeof late, hipMemcpyDeviceToHost, c->stream));
        if (late) {
            char n[32];
            snprintf(n, sizeof n, "%d", late);
            HQ_HIP(hipMemsetAsync(c->d_halo_err + 2, 0, sizeof(int32_t), c->stream));
            HQ_HIP(hipStreamSynchronize(c->stream));
            return hq_fail(HQ_ERR_COMM, "IPC transport: %s waits for a neighbour's halo records timed out (HQ_IPC_TIMEOUT_MS)", n);
        }
    }
    if (c->debug_halo) {
        int32_t bad = 0;
        HQ_TRY(hq_copy_wait(&bad, c->d_halo_err, sizeof bad, hipMemcpyDeviceToHost, c->stream));
        if (bad) {
            char n[32];
            snprintf(n, sizeof n, "%d", bad);
            HQ_HIP(hipMemsetAsync(c->d_halo_err, 0, sizeof(int32_t), c->stream));      /* reported once: later syncs count afresh */
            HQ_HIP(hipStreamSynchronize(c->stream));
            return hq_fail(HQ_ERR_COMM, "HQ_DEBUG_HALO: %s halo records arrived for another node than the schedule names "
                                        "(global node ids do not match, psolve.c:5058-5069)", n);
        }
    }
    return HQ_OK;
}

/* solver_check_nan (psolve.c:3769-3782) on the device-resident fields: tm1, tm2 (and the force
 * accumulator of the scatter variant).  *nonfinite = number of NaN / infinite values; the call
 * itself fails only on runtime errors (the reference aborts; here the caller decides). */
extern "C" int hq_check_finite(hq_ctx* c, int64_t* nonfinite)
{
    if (!c || !nonfinite) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    HQ_HIP(hipSetDevice(c->device));
    HQ_HIP(hq_quiesce(c));
    HQ_HIP(hipMemsetAsync(c->d_halo_err + 1, 0, sizeof(int32_t), c->stream));
    const int64_t n3 = 3 * (int64_t)c->N;
    const hq_real* arr[2] = { c->d_u[c->now], c->d_u[c->prev] };
    for (const hq_real* a : arr)
        if (a) hq_k_count_nonfinite<<<2048, 256, 0, c->stream>>>(n3, a, c->d_halo_err + 1);
    if (c->d_force) hq_k_count_nonfinite<<<2048, 256, 0, c->stream>>>(n3, (const double*)c->d_force, c->d_halo_err + 1);
    int32_t bad = 0;
    HQ_HIP(hipMemcpyAsync(&bad, c->d_halo_err + 1, sizeof bad, hipMemcpyDeviceToHost, c->stream));
    HQ_HIP(hipStreamSynchronize(c->stream));
    *nonfinite = bad;
    return HQ_OK;
}

extern "C" int hq_run_timed(hq_ctx* c, int32_t nsteps, double* total_ms, double* kernel_ms_avg)
{
    if (!c || nsteps <= 0) return hq_fail(HQ_ERR_ARG, "bad argument%s", "");
    HQ_TRY(hq_output_check_room(c, nsteps));
    HQ_HIP(hipSetDevice(c->device));
    size_t need = 2 * (size_t)nsteps;
    while (c->ev.size() < need) {
        hipEvent_t e;
        HQ_HIP(hipEventCreate(&e));
        c->ev.push_back(e);
    }
    for (int k = 0; k < 2; k++)
        if (!c->ev_span[k]) HQ_HIP(hipEventCreate(&c->ev_span[k]));
    HQ_HIP(hq_quiesce(c));
    hq_clock_harvest_all(c, true);
    const double clk_us0 = c->clk_us[0];
    const int64_t clk_n0 = c->clk_steps;
    c->ev_used = 0;
    HQ_HIP(hipEventRecord(c->ev_span[0], c->stream));
    c->timing = true;
    int rc = HQ_OK;
    for (int32_t s = 0; s < nsteps && rc == HQ_OK; s++) rc = hq_step(c);
    c->timing = false;
    if (c->overlap) hipStreamWaitEvent(c->stream, c->ev_shared, 0);
    if (c->bstream) hipStreamWaitEvent(c->stream, c->ev_bricks, 0);
    hipEventRecord(c->ev_span[1], c->stream);
    hipError_t he = hq_quiesce(c);
    if (he == hipSuccess) hq_clock_harvest_all(c, true);
    double tot = 0, ker = 0;
    if (rc == HQ_OK && he == hipSuccess) {
        float ms = 0;
        hipEventElapsedTime(&ms, c->ev_span[0], c->ev_span[1]);
        tot = ms;
        for (size_t i = 0; i + 1 < c->ev_used; i += 2) {
            hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]);
            ker += ms;
        }
        if (c->ev_used >= 2) ker /= (double)(c->ev_used / 2);
        /* a step whose bricks ran on a stream of their own: first kernel's start -> last kernel's end, from the phase clock */
        if (c->bstream && c->clk_steps > clk_n0) ker = (c->clk_us[0] - clk_us0) / (double)(c->clk_steps - clk_n0) * 1e-3;
    }
    if (rc != HQ_OK) return rc;
    if (he != hipSuccess) return hq_fail(HQ_ERR_DEVICE, "timed run failed: %s", hipGetErrorString(he));
    if (total_ms) *total_ms = tot;
    if (kernel_ms_avg) *kernel_ms_avg = ker;
    return HQ_OK;
}

extern "C" const char* hq_dominant_kernel(hq_ctx* c)
{
    if (c && c->att.on && !c->att.split) return "hq_k_element_bkt";
    if (!c || c->variant != HQ_VARIANT_PATCH) return "hq_k_element_scatter";
    if (2 * c->bricks.nb > (int64_t)c->N) return "hq_k_brick";
    if (2 * c->plan.nstencil > c->plan.npatches) return "hq_k_patch_stencil";
    if (!hq_patch_uses_pers(&c->plan)) return "hq_k_patch_step";
    return c->plan.seeded ? "hq_k_patch_seed" : "hq_k_patch_pers";
}

static int hq_gather_impl(hq_ctx* c, int32_t n, const int32_t* lnid, hq_real* o1, hq_real* o2, hq_real* o3);

extern "C" int hq_gather(hq_ctx* c, int32_t n, const int32_t* lnid, hq_real* o1, hq_real* o2)
{
    return hq_gather_impl(c, n, lnid, o1, o2, nullptr);
}

extern "C" int hq_gather3(hq_ctx* c, int32_t n, const int32_t* lnid, hq_real* o1, hq_real* o2, hq_real* o3)
{
    if (c && o3 && c->variant != HQ_VARIANT_PATCH)
        return hq_fail(HQ_ERR_STATE, "u(t - 2 dt) is kept by the patch variant only%s", "");
    return hq_gather_impl(c, n, lnid, o1, o2, o3);
}

static int hq_gather_impl(hq_ctx* c, int32_t n, const int32_t* lnid, hq_real* o1, hq_real* o2, hq_real* o3)
{
    if (!c || n < 0 || (n && !lnid)) return hq_fail(HQ_ERR_ARG, "bad argument%s", "");
    if (n == 0) return HQ_OK;
    HQ_HIP(hipSetDevice(c->device));
    HQ_HIP(hq_quiesce(c));
    for (int32_t i = 0; i < n; i++)
        if (lnid[i] < 0 || lnid[i] >= c->N) return hq_fail(HQ_ERR_ARG, "node id out of range%s", "");
    /* scratch kept with the context: a host that prints stations every few steps (psolve.c:6679-6790) must not pay a
     * hipMalloc / hipFree pair per call */
    if (n > c->gather_cap) {
        c->gather_cap = 0;
        const int32_t cap = std::max(n, 1024);
        HQ_TRY(c->d_gather_ids.alloc(nullptr, (size_t)cap));
        HQ_TRY(c->d_gather_out.alloc(nullptr, 9 * (size_t)cap));
        c->gather_cap = cap;
    }
    int32_t* d_ids = c->d_gather_ids;
    hq_real* d_o = c->d_gather_out;
    hipError_t e;
    c->h2d_bytes += 4 * (int64_t)n;
    c->d2h_bytes += 3 * (int64_t)sizeof(hq_real) * (int64_t)n * ((o1 ? 1 : 0) + (o2 ? 1 : 0) + (o3 ? 1 : 0));
    std::vector<int32_t> dev_ids;
    if (!c->perm.empty()) {
        dev_ids.resize((size_t)n);
        for (int32_t i = 0; i < n; i++) dev_ids[(size_t)i] = c->perm[(size_t)lnid[i]];
        lnid = dev_ids.data();
    }
    hipMemcpyAsync(d_ids, lnid, sizeof(int32_t) * n, hipMemcpyHostToDevice, c->stream);
    hq_k_gather<<<hq_blocks((int64_t)n * 3, 256), 256, 0, c->stream>>>(n, d_ids, c->d_u[c->now], c->d_u[c->prev],
                                                                         d_o, d_o + 3 * (size_t)n);
    if (o1) hipMemcpyAsync(o1, d_o, sizeof(hq_real) * 3 * n, hipMemcpyDeviceToHost, c->stream);
    if (o2) hipMemcpyAsync(o2, d_o + 3 * (size_t)n, sizeof(hq_real) * 3 * n, hipMemcpyDeviceToHost, c->stream);
    if (o3) {
        hq_k_gather<<<hq_blocks((int64_t)n * 3, 256), 256, 0, c->stream>>>(n, d_ids, c->d_u[c->spare], c->d_u[c->spare],
                                                                             d_o + 6 * (size_t)n, d_o + 6 * (size_t)n);
        hipMemcpyAsync(o3, d_o + 6 * (size_t)n, sizeof(hq_real) * 3 * n, hipMemcpyDeviceToHost, c->stream);
    }
    e = hq_quiesce(c);
    if (e != hipSuccess) return hq_fail(HQ_ERR_DEVICE, "gather failed: %s", hipGetErrorString(e));
    return HQ_OK;
}

extern "C" int hq_download(hq_ctx* c, hq_real* tm1, hq_real* tm2)
{
    if (!c) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    HQ_HIP(hipSetDevice(c->device));
    HQ_HIP(hq_quiesce(c));
    if (tm1) HQ_TRY(hq_field_to_host(c, c->d_u[c->now], tm1));
    if (tm2) HQ_TRY(hq_field_to_host(c, c->d_u[c->prev], tm2));
    return HQ_OK;
}

extern "C" int hq_upload(hq_ctx* c, const hq_real* tm1, const hq_real* tm2, int32_t step)
{
    if (!c || !tm1 || !tm2) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    HQ_HIP(hipSetDevice(c->device));
    HQ_HIP(hq_quiesce(c));
    size_t bytes = sizeof(hq_real) * 3 * (size_t)c->N;
    HQ_TRY(hq_field_to_device(c, tm1, c->d_u[c->now]));
    HQ_TRY(hq_field_to_device(c, tm2, c->d_u[c->prev]));
    /* tm3 after a restart: calloc, psolve.c:3347.  ON the compute stream and waited for: a hipMemset on the null stream is
     * not ordered with this context's (non-blocking) streams -- where eight processes time-slice one GPU it could land
     * behind the first step's kernels, in the very buffer they write u(t + dt) into (round 6: one bench.py parity failure in
     * a few hundred 8-rank runs, relative error 0.37, traced to this line) */
    if (c->d_u[2]) {
        HQ_HIP(hipMemsetAsync(c->d_u[c->spare], 0, bytes, c->stream));
        HQ_HIP(hipStreamSynchronize(c->stream));
    }
    /* the memory variables after a restart: calloc, psolve.c:3322-3325 (io_checkpoint.c carries tm1 / tm2 only); an exact
     * restart follows with hq_attenuation_load */
    if (c->att.on) HQ_TRY(c->att.d_mv.fill(0, c->stream));
    /* the plastic strains after a restart: calloc, nonlinear.c:651-664; an exact restart follows with hq_nonlinear_load */
    if (c->nl.on && c->nl.nel) HQ_TRY(c->nl.d_st.fill(0, c->stream));
    c->step = step;
    return HQ_OK;
}

/* ------------------------------------------------------------------------ */
/* BKT attenuation (hq_atten.h, hq_atten_plan.h)                            */
/* ------------------------------------------------------------------------ */

/* the class doubles of a plan, refused where one is not finite */
static int hq_atten_ktab(const hq_atten_plan& P, double freq, double dt, std::vector<double>* ktab)
{
    ktab->assign((size_t)P.nclasses * HQ_ATTEN_NCOEF, 0.0);
    for (int32_t k = 0; k < P.nclasses; k++) {
        hq_atten_class_coef(P.rows.data() + HQ_ATTEN_NROW * (size_t)k, freq, dt, ktab->data() + HQ_ATTEN_NCOEF * (size_t)k);
        for (int j = 0; j < HQ_ATTEN_NCOEF; j++)
            if (!std::isfinite((*ktab)[HQ_ATTEN_NCOEF * (size_t)k + j])) return hq_fail(HQ_ERR_ARG, "attenuation: a class coefficient is not finite%s", "");
    }
    return HQ_OK;
}

/* A plan's slot state on the device and its corner table on the host, in *A beside the context's own (no ledger: the arrays
 * move, hq_ctx.bytes takes their sum at the end).  eslot: the table the device gets -- the plan's own, or a split context's
 * in the correction's element order */
static int hq_atten_slots_build(hq_atten_plan& P, const std::vector<int32_t>& eslot, const std::vector<double>& ktab, hipStream_t st,
                                hq_atten_dev* A)
{
    HQ_TRY(A->d_eslot.put(nullptr, eslot, st)); HQ_TRY(A->d_slot_node.put(nullptr, P.slot_node, st));
    HQ_TRY(A->d_slot_class.put(nullptr, P.slot_class, st)); HQ_TRY(A->d_ktab.put(nullptr, ktab, st));
    HQ_TRY(A->d_mv.alloc(nullptr, (size_t)HQ_ATTEN_NSTATE * P.nslots)); HQ_TRY(A->d_mv.fill(0, st));
    HQ_TRY(A->d_w.alloc(nullptr, (size_t)HQ_ATTEN_NW * P.nslots)); HQ_TRY(A->d_w.fill(0, st));
    A->bytes = (int64_t)(A->d_eslot.bytes() + A->d_slot_node.bytes() + A->d_slot_class.bytes() + A->d_ktab.bytes() + A->d_mv.bytes() +
                         A->d_w.bytes());
    if (A->bytes != hq_atten_bytes(P.nslots, P.Epad, P.nclasses)) return hq_fail(HQ_ERR_STATE, "attenuation: the device bytes are not the header's formula%s", "");
    A->nclasses = P.nclasses; A->nslots = P.nslots; A->Epad = (int32_t)P.Epad;
    A->h_eslot = std::move(P.eslot); A->h_slot_node = std::move(P.slot_node);
    A->on = true;
    return HQ_OK;
}

extern "C" int hq_attenuation_set(hq_ctx* c, const hq_attenuation_desc* a)
{
    if (!c || !a || !a->coef) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    if (sizeof(hq_real) != sizeof(double))
        return hq_fail(HQ_ERR_STATE, "attenuation: not in the float library (the memory variables are double state)%s", "");
    if (c->variant != HQ_VARIANT_SCATTER)
        return hq_fail(HQ_ERR_STATE, "attenuation runs in the scatter variant only: create the context with HQ_VARIANT_SCATTER%s", "");
    if (!(a->freq > 0.0) || !std::isfinite(a->freq)) return hq_fail(HQ_ERR_ARG, "attenuation: freq must be finite and > 0%s", "");
    if (c->etable_damped)
        return hq_fail(HQ_ERR_ARG, "attenuation: the eTable has c3 or c4 != 0; under BKT compute_setab yields a = b = 0 (psolve.c:5869)%s", "");
    HQ_HIP(hipSetDevice(c->device));
    HQ_HIP(hq_quiesce(c));
    std::vector<int32_t> soa((size_t)8 * c->Epad);
    HQ_TRY(hq_copy_wait(soa.data(), c->d_lnid, sizeof(int32_t) * soa.size(), hipMemcpyDeviceToHost, c->stream));
    hq_atten_plan P;
    HQ_TRY(hq_atten_plan_build(c->E, c->N, soa.data(), c->Epad, a->coef, &P));
    std::vector<double> ktab;
    HQ_TRY(hq_atten_ktab(P, a->freq, c->dt, &ktab));
    /* everything is built beside the context's own and moved in at the end: a refusal leaves the context as it was */
    hq_atten_dev A;
    HQ_TRY(hq_atten_slots_build(P, P.eslot, ktab, c->stream, &A));       /* (on a refusal A's arrays go with it) */
    hq_attenuation_clear(c);
    c->bytes += A.bytes;
    c->att = std::move(A);
    return HQ_OK;
}

/* a split context steps alone: no partition, no transport (include/hq_solver.h); a nonlinear one likewise */
static int hq_refuse_split(const hq_ctx* c, const char* what)
{
    if (c && c->att.split)
        return hq_fail(HQ_ERR_STATE, "%s: the context carries split attenuation (hq_attenuation_set_split), which steps one context alone", what);
    if (c && c->nl.on)
        return hq_fail(HQ_ERR_STATE, "%s: the context carries nonlinear soil (hq_nonlinear_set), which steps one context alone", what);
    return HQ_OK;
}

/* the stream and the two events of a correction chain's head beside the step, from the first call that needs them on */
static int hq_correction_stream(hq_ctx* c, const char* who)
{
    if (c->astream) return HQ_OK;
    hipStream_t st = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&e0, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e1, hipEventDisableTiming) != hipSuccess) {
        if (st) hipStreamDestroy(st);
        if (e0) hipEventDestroy(e0);
        return hq_fail(HQ_ERR_DEVICE, "%s: no stream or event", who);
    }
    c->astream = st; c->ev_att_fork = e0; c->ev_att_done = e1;
    return HQ_OK;
}

/* the hanging-node table in device numbering: the context's own arrays, read back */
static int hq_hanging_to_host(hq_ctx* c, std::vector<int32_t>* id, std::vector<int32_t>* ptr, std::vector<int32_t>* anchor)
{
    id->assign((size_t)c->ldnnum, 0); ptr->assign((size_t)c->ldnnum + 1, 0); anchor->clear();
    if (!c->ldnnum) return HQ_OK;
    HQ_TRY(hq_copy_wait(id->data(), c->d_dn_id, sizeof(int32_t) * id->size(), hipMemcpyDeviceToHost, c->stream));
    HQ_TRY(hq_copy_wait(ptr->data(), c->d_dn_ptr, sizeof(int32_t) * ptr->size(), hipMemcpyDeviceToHost, c->stream));
    anchor->resize((size_t)ptr->back());
    return hq_copy_wait(anchor->data(), c->d_dn_anchor, sizeof(int32_t) * anchor->size(), hipMemcpyDeviceToHost, c->stream);
}

extern "C" int hq_attenuation_set_split(hq_ctx* c, const hq_attenuation_desc* a)
{
    if (!c || !a || !a->coef) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    if (sizeof(hq_real) != sizeof(double))
        return hq_fail(HQ_ERR_STATE, "attenuation: not in the float library (the memory variables are double state)%s", "");
    if (c->variant != HQ_VARIANT_PATCH)
        return hq_fail(HQ_ERR_STATE, "split attenuation runs beside the patch variant's step: on a scatter context call hq_attenuation_set%s", "");
    if (c->nranks > 1 || hq_has_transport(c) || c->group)
        return hq_fail(HQ_ERR_STATE, "split attenuation: partitions and transports are out of scope (one context, nranks = 1)%s", "");
    if (c->nl.on)
        return hq_fail(HQ_ERR_STATE, "split attenuation: the context carries nonlinear soil (hq_nonlinear_set); the two passes do not combine%s", "");
    if (!(a->freq > 0.0) || !std::isfinite(a->freq)) return hq_fail(HQ_ERR_ARG, "attenuation: freq must be finite and > 0%s", "");
    if (c->etable_damped)
        return hq_fail(HQ_ERR_ARG, "attenuation: the eTable has c3 or c4 != 0; under BKT compute_setab yields a = b = 0 (psolve.c:5869)%s", "");
    HQ_HIP(hipSetDevice(c->device));
    HQ_HIP(hq_quiesce(c));
    const int64_t E = c->E, N = c->N;
    hq_atten_plan P;
    HQ_TRY(hq_atten_plan_build(E, N, c->h_lnid.data(), 0, a->coef, &P));
    std::vector<double> ktab;
    HQ_TRY(hq_atten_ktab(P, a->freq, c->dt, &ktab));
    std::vector<int32_t> dn_id, dn_ptr, dn_anchor;
    HQ_TRY(hq_hanging_to_host(c, &dn_id, &dn_ptr, &dn_anchor));
    hq_split_plan S;
    HQ_TRY(hq_split_plan_build(E, N, P.Epad, c->h_lnid.data(), c->ldnnum, dn_id.data(), dn_ptr.data(), dn_anchor.data(), &S));
    if (hq_atten_plan_faults(E, c->h_lnid.data(), P) != 0 ||
        hq_split_plan_faults(E, N, P.Epad, c->h_lnid.data(), c->ldnnum, dn_id.data(), dn_ptr.data(), dn_anchor.data(), S.epos.data(),
                             S.nptr.data(), S.nent.data(), S.sd.data(), (int64_t)(S.sd.size() / 3)) != 0)
        return hq_fail(HQ_ERR_STATE, "split attenuation: the plan does not pass its own check%s", "");
    HQ_TRY(hq_correction_stream(c, "split attenuation"));
    /* everything is built beside the context's own and moved in at the end: a refusal leaves the context as it was */
    hq_atten_dev A;
    std::vector<double> cc1((size_t)E), cc2((size_t)E);                 /* the device's element order (hq_split_plan.epos) */
    std::vector<int32_t> eslot_dev(P.eslot.size(), 0);
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < E; e++) {
        const size_t at = (size_t)S.epos[(size_t)e];
        cc1[at] = c->h_c1[(size_t)e]; cc2[at] = c->h_c2[(size_t)e];
        for (int i = 0; i < 8; i++) eslot_dev[(size_t)(i * P.Epad) + at] = P.eslot[(size_t)(i * P.Epad + e)];
    }
    HQ_TRY(hq_atten_slots_build(P, eslot_dev, ktab, c->stream, &A));
    HQ_TRY(A.d_c1.put(nullptr, cc1, c->stream)); HQ_TRY(A.d_c2.put(nullptr, cc2, c->stream));
    HQ_TRY(hq_correction_build(S, E, A.Epad, c->h_mass, nullptr, c->stream, &A.corr));
    if ((int64_t)(A.d_c1.bytes() + A.d_c2.bytes()) + A.corr.bytes != hq_split_bytes(E, A.Epad, N, S.nanchors, S.npairs))
        return hq_fail(HQ_ERR_STATE, "attenuation: the device bytes are not the header's formula%s", "");
    A.bytes += hq_split_bytes(E, A.Epad, N, S.nanchors, S.npairs);
    if (!c->perm.empty()) {                          /* fetch / load name nodes as the caller numbers them */
        std::vector<int32_t> inv((size_t)N);
        for (int64_t n = 0; n < N; n++) inv[(size_t)c->perm[(size_t)n]] = (int32_t)n;
        for (int32_t& n : A.h_slot_node) n = inv[(size_t)n];
    }
    A.split = true;
    hq_attenuation_clear(c);
    c->bytes += A.bytes;
    c->att = std::move(A);
    return HQ_OK;
}

extern "C" int hq_attenuation_clear(hq_ctx* c)
{
    if (!c) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    if (!c->att.on) return HQ_OK;
    HQ_HIP(hipSetDevice(c->device));
    HQ_HIP(hq_quiesce(c));
    c->bytes -= c->att.bytes;
    c->att = hq_atten_dev();
    return HQ_OK;
}

extern "C" int hq_attenuation_info(hq_ctx* c, int64_t out[4])
{
    if (!c || !out) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    out[0] = c->att.nclasses; out[1] = c->att.nslots;
    out[2] = c->att.on ? c->att.bytes : 0;
    out[3] = c->att.split ? 1 : 0;
    return HQ_OK;
}

/* the four arrays of the reference's layout, [lenum * 8][3] each (cindex = eindex * 8 + i); a NULL one is left out */
extern "C" int hq_attenuation_fetch(hq_ctx* c, double* shear1, double* shear2, double* kappa1, double* kappa2)
{
    if (!c) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    if (!c->att.on) return hq_fail(HQ_ERR_STATE, "attenuation is not set on this context%s", "");
    HQ_HIP(hipSetDevice(c->device));
    HQ_HIP(hq_quiesce(c));
    const hq_atten_dev& A = c->att;
    const int64_t ns = A.nslots;
    std::vector<double> mv((size_t)HQ_ATTEN_NSTATE * ns);
    HQ_TRY(hq_copy_wait(mv.data(), A.d_mv, sizeof(double) * mv.size(), hipMemcpyDeviceToHost, c->stream));
    c->d2h_bytes += (int64_t)(sizeof(double) * mv.size());
    double* out[HQ_ATTEN_NVAR] = { shear1, shear2, kappa1, kappa2 };
    for (int v = 0; v < HQ_ATTEN_NVAR; v++) {
        if (!out[v]) continue;
#pragma omp parallel for schedule(static)
        for (int64_t e = 0; e < c->E; e++)
            for (int i = 0; i < 8; i++) {
                const int64_t s = A.h_eslot[(size_t)(i * (int64_t)A.Epad + e)];
                for (int d = 0; d < 3; d++) out[v][3 * (8 * e + i) + d] = mv[(size_t)((3 * v + d) * ns + s)];
            }
    }
    return HQ_OK;
}

extern "C" int hq_attenuation_load(hq_ctx* c, const double* shear1, const double* shear2, const double* kappa1, const double* kappa2)
{
    if (!c || !shear1 || !shear2 || !kappa1 || !kappa2) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    if (!c->att.on) return hq_fail(HQ_ERR_STATE, "attenuation is not set on this context%s", "");
    HQ_HIP(hipSetDevice(c->device));
    HQ_HIP(hq_quiesce(c));
    const hq_atten_dev& A = c->att;
    const int64_t ns = A.nslots;
    const double* in[HQ_ATTEN_NVAR] = { shear1, shear2, kappa1, kappa2 };
    std::vector<double> mv((size_t)HQ_ATTEN_NSTATE * ns);
    std::vector<char> have((size_t)ns, 0);
    for (int64_t e = 0; e < c->E; e++)
        for (int i = 0; i < 8; i++) {
            const int64_t s = A.h_eslot[(size_t)(i * (int64_t)A.Epad + e)];
            for (int v = 0; v < HQ_ATTEN_NVAR; v++)
                for (int d = 0; d < 3; d++) {
                    const double x = in[v][3 * (8 * e + i) + d];
                    double& slot = mv[(size_t)((3 * v + d) * ns + s)];
                    if (!std::isfinite(x)) return hq_fail(HQ_ERR_ARG, "attenuation: a memory variable to load is not finite%s", "");
                    if (have[(size_t)s] && memcmp(&slot, &x, sizeof x) != 0) {
                        char node[32];
                        snprintf(node, sizeof node, "%d", (int)A.h_slot_node[(size_t)s]);
                        return hq_fail(HQ_ERR_ARG, "attenuation: corners of one class that share node %s carry different memory variables", node);
                    }
                    slot = x;
                }
            have[(size_t)s] = 1;
        }
    c->h2d_bytes += (int64_t)(sizeof(double) * mv.size());
    return c->att.d_mv.upload(mv.data(), mv.size(), c->stream);
}

extern "C" int hq_attenuation_plan_check(const hq_desc* d, const float* coef, int64_t report[4])
{
    if (!d || !coef || !report) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    hq_options opts;
    hq_options_resolve(&opts, nullptr);
    hq_prep prep;
    HQ_TRY(hq_prepare(d, opts, 0, &prep));
    hq_atten_plan P;
    HQ_TRY(hq_atten_plan_build(d->lenum, d->nharbored, d->lnid, 0, coef, &P));
    int64_t bad = hq_atten_plan_faults(d->lenum, d->lnid, P);
    std::vector<char> has((size_t)d->nharbored, 0);
    for (int32_t n : P.slot_node) has[(size_t)n] = 1;
    for (int32_t k = 0; k < d->ldnnum; k++) bad += !has[(size_t)d->dn_ldnid[k]];      /* a hanging node is a node like any other */
    report[0] = P.nclasses; report[1] = P.nslots; report[2] = hq_atten_bytes(P.nslots, P.Epad, P.nclasses); report[3] = bad;
    return HQ_OK;
}

/* the description as hq_create would number it: behind the bricks' numbering where it would build bricks (host-only: the
 * library defaults, the environment where HQ_ALLOW_ENV=1) */
static int hq_prepare_as_created(const hq_desc* d, hq_prep* prep)
{
    hq_options opts;
    hq_options_resolve(&opts, nullptr);
    return hq_prepare(d, opts, d->eTable && d->nTable && d->node_xyz ? HQ_PREP_BRICKS : 0, prep);
}

/* a plan's table into the caller's array, where there is one */
static void hq_export(int32_t* out, const std::vector<int32_t>& v)
{
    if (out && !v.empty()) memcpy(out, v.data(), sizeof(int32_t) * v.size());
}

/* ... and the split tables of it */
static int hq_split_plan_of(const hq_desc* d, hq_prep* prep, int64_t* Epad, hq_split_plan* S)
{
    HQ_TRY(hq_prepare_as_created(d, prep));
    const hq_desc& q = prep->desc;
    *Epad = ((int64_t)q.lenum + 63) & ~(int64_t)63;
    return hq_split_plan_build(q.lenum, q.nharbored, *Epad, q.lnid, q.ldnnum, q.dn_ldnid, q.dn_ptr, q.dn_lanid, S);
}

extern "C" int hq_attenuation_split_plan_check(const hq_desc* d, const float* coef, int64_t report[4])
{
    if (!d || !coef || !report) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    if (d->nranks > 1) return hq_fail(HQ_ERR_STATE, "split attenuation: partitions and transports are out of scope (one context, nranks = 1)%s", "");
    hq_prep prep;
    hq_split_plan S;
    int64_t Epad = 0;
    HQ_TRY(hq_split_plan_of(d, &prep, &Epad, &S));
    const hq_desc& q = prep.desc;
    hq_atten_plan P;
    HQ_TRY(hq_atten_plan_build(q.lenum, q.nharbored, q.lnid, 0, coef, &P));
    int64_t bad = hq_atten_plan_faults(q.lenum, q.lnid, P);
    bad += hq_split_plan_faults(q.lenum, q.nharbored, Epad, q.lnid, q.ldnnum, q.dn_ldnid, q.dn_ptr, q.dn_lanid, S.epos.data(), S.nptr.data(),
                                S.nent.data(), S.sd.data(), (int64_t)(S.sd.size() / 3));
    report[0] = P.nclasses; report[1] = P.nslots;
    report[2] = hq_atten_bytes(P.nslots, P.Epad, P.nclasses) + hq_split_bytes(q.lenum, Epad, q.nharbored, S.nanchors, S.npairs);
    report[3] = bad;
    return HQ_OK;
}

extern "C" int hq_attenuation_split_plan_tables(const hq_desc* d, int32_t* epos, int32_t* nptr, int32_t* nent, int32_t* sd, int64_t counts[3])
{
    if (!d || !counts) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    hq_prep prep;
    hq_split_plan S;
    int64_t Epad = 0;
    HQ_TRY(hq_split_plan_of(d, &prep, &Epad, &S));
    counts[0] = (int64_t)S.nptr.size(); counts[1] = (int64_t)S.nent.size(); counts[2] = (int64_t)(S.sd.size() / 3);
    hq_export(epos, S.epos); hq_export(nptr, S.nptr); hq_export(nent, S.nent); hq_export(sd, S.sd);
    return HQ_OK;
}

extern "C" int hq_attenuation_split_table_faults(const hq_desc* d, const int32_t* epos, const int32_t* nptr, const int32_t* nent, const int32_t* sd,
                                                 int64_t nsd, int64_t* faults)
{
    if (!d || !epos || !nptr || !nent || !faults || nsd < 0 || (nsd && !sd)) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    hq_prep prep;
    hq_split_plan S;
    int64_t Epad = 0;
    HQ_TRY(hq_split_plan_of(d, &prep, &Epad, &S));
    const hq_desc& q = prep.desc;
    *faults = hq_split_plan_faults(q.lenum, q.nharbored, Epad, q.lnid, q.ldnnum, q.dn_ldnid, q.dn_ptr, q.dn_lanid, epos, nptr, nent, sd, nsd);
    return HQ_OK;
}

/* ------------------------------------------------------------------------ */
/* nonlinear soil (hq_nonlin.h, hq_nonlin_dev.h)                            */
/* ------------------------------------------------------------------------ */

/* the description's own faults: model, ids, constants (include/hq_solver.h) */
static int hq_nl_validate(const hq_nonlinear_desc* a, int64_t E)
{
    if (a->model != HQ_NL_VONMISES && a->model != HQ_NL_DRUCKERPRAGER)
        return hq_fail(HQ_ERR_ARG, "nonlinear: unknown model (HQ_NL_VONMISES or HQ_NL_DRUCKERPRAGER)%s", "");
    if (a->nelems < 0 || (a->nelems > 0 && (!a->elems || !a->cons))) return hq_fail(HQ_ERR_ARG, "nonlinear: nelems < 0 or a null table%s", "");
    for (int64_t k = 0; k < a->nelems; k++) {
        if (a->elems[k] < 0 || a->elems[k] >= E) return hq_fail(HQ_ERR_ARG, "nonlinear: an element id is out of range%s", "");
        if (k && a->elems[k] <= a->elems[k - 1]) return hq_fail(HQ_ERR_ARG, "nonlinear: the element ids are not strictly ascending%s", "");
        const double* q = a->cons + HQ_NL_NCONS * k;
        for (int j = 0; j < HQ_NL_NCONS; j++)
            if (!std::isfinite(q[j])) return hq_fail(HQ_ERR_ARG, "nonlinear: a constant is not finite%s", "");
        if (!(q[0] > 0.0)) return hq_fail(HQ_ERR_ARG, "nonlinear: h must be > 0%s", "");
        if (q[1] < 0.0) return hq_fail(HQ_ERR_ARG, "nonlinear: mu must be >= 0%s", "");
        if (q[4] < 0.0) return hq_fail(HQ_ERR_ARG, "nonlinear: k must be >= 0%s", "");
        if (a->model == HQ_NL_VONMISES && q[3] != 0.0) return hq_fail(HQ_ERR_ARG, "nonlinear: alpha must be 0 under von Mises%s", "");
    }
    return HQ_OK;
}

extern "C" int hq_nonlinear_clear(hq_ctx* c)
{
    if (!c) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    if (!c->nl.on) return HQ_OK;
    HQ_HIP(hipSetDevice(c->device));
    HQ_HIP(hq_quiesce(c));
    c->bytes -= c->nl.bytes;
    c->nl = hq_nl_dev();
    return HQ_OK;
}

extern "C" int hq_nonlinear_set(hq_ctx* c, const hq_nonlinear_desc* a)
{
    if (!c || !a) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    if (sizeof(hq_real) != sizeof(double))
        return hq_fail(HQ_ERR_STATE, "nonlinear: not in the float library (the plastic strains are double state beside a double step)%s", "");
    if (c->variant != HQ_VARIANT_PATCH)
        return hq_fail(HQ_ERR_STATE, "nonlinear soil runs beside the patch variant's step: create the context with HQ_VARIANT_PATCH%s", "");
    if (c->nranks > 1 || hq_has_transport(c) || c->group)
        return hq_fail(HQ_ERR_STATE, "nonlinear: partitions and transports are out of scope (one context, nranks = 1)%s", "");
    if (c->att.on)
        return hq_fail(HQ_ERR_STATE, "nonlinear: the context carries attenuation; the two passes do not combine (hq_attenuation_clear first)%s", "");
    HQ_TRY(hq_nl_validate(a, c->E));
    HQ_HIP(hipSetDevice(c->device));
    HQ_HIP(hq_quiesce(c));
    hq_nl_dev L;                                      /* built beside the context's own: a refusal leaves the context as it was */
    L.model = a->model;
    const int64_t nel = a->nelems;
    if (nel > 0) {
        std::vector<int32_t> dn_id, dn_ptr, dn_anchor;
        HQ_TRY(hq_hanging_to_host(c, &dn_id, &dn_ptr, &dn_anchor));
        hq_nl_plan P;
        HQ_TRY(hq_nl_plan_build(nel, a->elems, c->N, c->h_lnid.data(), c->ldnnum, dn_id.data(), dn_ptr.data(), dn_anchor.data(), &P));
        if (hq_nl_plan_faults(nel, a->elems, c->N, c->h_lnid.data(), c->ldnnum, dn_id.data(), dn_ptr.data(), dn_anchor.data(), P, P.S.epos.data(),
                              P.S.nptr.data(), P.S.nent.data(), P.S.sd.data(), (int64_t)(P.S.sd.size() / 3)) != 0)
            return hq_fail(HQ_ERR_STATE, "nonlinear: the plan does not pass its own check%s", "");
        HQ_TRY(hq_correction_stream(c, "nonlinear"));
        const int64_t Ep = P.Enlpad, nt = P.nt;
        std::vector<int32_t> lnid_dev((size_t)(8 * Ep), P.tnode[0]);          /* (the padding names a node that exists) */
        std::vector<double> cons_dev((size_t)(HQ_NL_NCONS * Ep), 0.0), mass((size_t)nt);
        for (int64_t k = 0; k < nel; k++) {
            const size_t at = (size_t)P.S.epos[(size_t)k];
            for (int i = 0; i < 8; i++) lnid_dev[(size_t)(i * Ep) + at] = P.tnode[(size_t)P.lnid[(size_t)(8 * k + i)]];
            for (int j = 0; j < HQ_NL_NCONS; j++) cons_dev[(size_t)(j * Ep) + at] = a->cons[HQ_NL_NCONS * k + j];
        }
        for (int64_t t = 0; t < nt; t++) mass[(size_t)t] = c->h_mass[(size_t)P.tnode[(size_t)t]];
        HQ_TRY(L.d_st.alloc(nullptr, (size_t)(HQ_NL_NSTATE * 8 * Ep))); HQ_TRY(L.d_st.fill(0, c->stream));
        HQ_TRY(L.d_cons.put(nullptr, cons_dev, c->stream)); HQ_TRY(L.d_lnid.put(nullptr, lnid_dev, c->stream));
        HQ_TRY(hq_correction_build(P.S, nel, Ep, mass, &P.tnode, c->stream, &L.corr));
        L.bytes = (int64_t)(L.d_st.bytes() + L.d_cons.bytes() + L.d_lnid.bytes()) + L.corr.bytes;
        if (L.bytes != hq_nl_bytes(nel, Ep, nt, P.S.nanchors, P.S.npairs))
            return hq_fail(HQ_ERR_STATE, "nonlinear: the device bytes are not the header's formula%s", "");
        L.nel = (int32_t)nel; L.Enlpad = (int32_t)Ep; L.nt = (int32_t)nt;
        L.h_epos = std::move(P.S.epos);
    }
    L.on = true;
    hq_nonlinear_clear(c);
    c->bytes += L.bytes;
    c->nl = std::move(L);
    return HQ_OK;
}

extern "C" int hq_nonlinear_info(hq_ctx* c, int64_t out[4])
{
    if (!c || !out) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    out[0] = c->nl.nel; out[1] = c->nl.nt;
    out[2] = c->nl.on ? c->nl.bytes : 0;
    out[3] = 0;
    return HQ_OK;
}

/* pstrain [nelems][8][6], ep [nelems][8]: the caller's element order, the reference's quadrature and tensor order; a NULL one
 * is left out */
extern "C" int hq_nonlinear_fetch(hq_ctx* c, double* pstrain, double* ep)
{
    if (!c) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    if (!c->nl.on) return hq_fail(HQ_ERR_STATE, "nonlinear soil is not set on this context%s", "");
    HQ_HIP(hipSetDevice(c->device));
    HQ_HIP(hq_quiesce(c));
    const hq_nl_dev& L = c->nl;
    if (!L.nel) return HQ_OK;
    const int64_t Ep = L.Enlpad;
    std::vector<double> st((size_t)(HQ_NL_NSTATE * 8 * Ep));
    HQ_TRY(hq_copy_wait(st.data(), L.d_st, sizeof(double) * st.size(), hipMemcpyDeviceToHost, c->stream));
    c->d2h_bytes += (int64_t)(sizeof(double) * st.size());
    for (int64_t k = 0; k < L.nel; k++) {
        const int64_t at = L.h_epos[(size_t)k];
        for (int j = 0; j < 8; j++) {
            if (pstrain)
                for (int q = 0; q < 6; q++) pstrain[(8 * k + j) * 6 + q] = st[(size_t)((q * 8 + j) * Ep + at)];
            if (ep) ep[8 * k + j] = st[(size_t)((6 * 8 + j) * Ep + at)];
        }
    }
    return HQ_OK;
}

extern "C" int hq_nonlinear_load(hq_ctx* c, const double* pstrain, const double* ep)
{
    if (!c) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    if (!c->nl.on) return hq_fail(HQ_ERR_STATE, "nonlinear soil is not set on this context%s", "");
    const hq_nl_dev& L = c->nl;
    if (L.nel && (!pstrain || !ep)) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    HQ_HIP(hipSetDevice(c->device));
    HQ_HIP(hq_quiesce(c));
    if (!L.nel) return HQ_OK;
    const int64_t Ep = L.Enlpad;
    std::vector<double> st((size_t)(HQ_NL_NSTATE * 8 * Ep), 0.0);
    for (int64_t k = 0; k < L.nel; k++) {
        const int64_t at = L.h_epos[(size_t)k];
        for (int j = 0; j < 8; j++) {
            for (int q = 0; q < 6; q++) {
                const double x = pstrain[(8 * k + j) * 6 + q];
                if (!std::isfinite(x)) return hq_fail(HQ_ERR_ARG, "nonlinear: a plastic strain to load is not finite%s", "");
                st[(size_t)((q * 8 + j) * Ep + at)] = x;
            }
            const double x = ep[8 * k + j];
            if (!std::isfinite(x)) return hq_fail(HQ_ERR_ARG, "nonlinear: a plastic strain to load is not finite%s", "");
            st[(size_t)((6 * 8 + j) * Ep + at)] = x;
        }
    }
    c->h2d_bytes += (int64_t)(sizeof(double) * st.size());
    return c->nl.d_st.upload(st.data(), st.size(), c->stream);
}

/* the description as hq_create would number it, and the nonlinear plan of it */
static int hq_nl_plan_of(const hq_desc* d, const hq_nonlinear_desc* a, hq_prep* prep, hq_nl_plan* P)
{
    if (d->nranks > 1) return hq_fail(HQ_ERR_STATE, "nonlinear: partitions and transports are out of scope (one context, nranks = 1)%s", "");
    HQ_TRY(hq_nl_validate(a, d->lenum));
    HQ_TRY(hq_prepare_as_created(d, prep));
    const hq_desc& q = prep->desc;
    if (a->nelems == 0) { *P = hq_nl_plan(); return HQ_OK; }
    return hq_nl_plan_build(a->nelems, a->elems, q.nharbored, q.lnid, q.ldnnum, q.dn_ldnid, q.dn_ptr, q.dn_lanid, P);
}

extern "C" int hq_nonlinear_plan_check(const hq_desc* d, const hq_nonlinear_desc* a, int64_t report[4])
{
    if (!d || !a || !report) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    hq_prep prep;
    hq_nl_plan P;
    HQ_TRY(hq_nl_plan_of(d, a, &prep, &P));
    const hq_desc& q = prep.desc;
    report[0] = P.nel; report[1] = P.nt;
    report[2] = hq_nl_bytes(P.nel, P.Enlpad, P.nt, P.S.nanchors, P.S.npairs);
    report[3] = P.nel ? hq_nl_plan_faults(P.nel, a->elems, q.nharbored, q.lnid, q.ldnnum, q.dn_ldnid, q.dn_ptr, q.dn_lanid, P, P.S.epos.data(),
                                          P.S.nptr.data(), P.S.nent.data(), P.S.sd.data(), (int64_t)(P.S.sd.size() / 3)) : 0;
    return HQ_OK;
}

extern "C" int hq_nonlinear_plan_tables(const hq_desc* d, const hq_nonlinear_desc* a, int32_t* tnode, int32_t* epos, int32_t* nptr,
                                        int32_t* nent, int32_t* sd, int64_t counts[4])
{
    if (!d || !a || !counts) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    hq_prep prep;
    hq_nl_plan P;
    HQ_TRY(hq_nl_plan_of(d, a, &prep, &P));
    counts[0] = P.nt; counts[1] = (int64_t)P.S.nptr.size(); counts[2] = (int64_t)P.S.nent.size(); counts[3] = (int64_t)(P.S.sd.size() / 3);
    hq_export(tnode, P.tnode); hq_export(epos, P.S.epos); hq_export(nptr, P.S.nptr); hq_export(nent, P.S.nent); hq_export(sd, P.S.sd);
    return HQ_OK;
}

extern "C" int hq_nonlinear_table_faults(const hq_desc* d, const hq_nonlinear_desc* a, const int32_t* tnode, const int32_t* epos,
                                         const int32_t* nptr, const int32_t* nent, const int32_t* sd, int64_t nsd, int64_t* faults)
{
    if (!d || !a || !tnode || !epos || !nptr || !nent || !faults || nsd < 0 || (nsd && !sd)) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    hq_prep prep;
    hq_nl_plan P;
    HQ_TRY(hq_nl_plan_of(d, a, &prep, &P));
    if (!P.nel) return hq_fail(HQ_ERR_ARG, "nonlinear: no tables without elements%s", "");
    const hq_desc& q = prep.desc;
    P.tnode.assign(tnode, tnode + P.nt);              /* the caller's list in the plan's place: the plan's own lnid must still fit it */
    *faults = hq_nl_plan_faults(P.nel, a->elems, q.nharbored, q.lnid, q.ldnnum, q.dn_ldnid, q.dn_ptr, q.dn_lanid, P, epos, nptr, nent, sd, nsd);
    return HQ_OK;
}

extern "C" int hq_phase_force(hq_ctx* c)
{
    if (!c) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    if (c->variant != HQ_VARIANT_SCATTER) return hq_fail(HQ_ERR_STATE, "phases exist in the scatter variant only%s", "");
    HQ_HIP(hipSetDevice(c->device));
    HQ_TRY(hq_launch_source(c));
    HQ_TRY(hq_launch_element_scatter(c));
    HQ_HIP(hipGetLastError());
    return HQ_OK;
}

extern "C" int hq_phase_update(hq_ctx* c)
{
    if (!c) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    if (c->variant != HQ_VARIANT_SCATTER) return hq_fail(HQ_ERR_STATE, "phases exist in the scatter variant only%s", "");
    HQ_HIP(hipSetDevice(c->device));
    HQ_TRY(hq_launch_update(c));
    std::swap(c->now, c->prev);
    c->step++;
    HQ_HIP(hipGetLastError());
    return HQ_OK;
}

extern "C" int hq_download_force(hq_ctx* c, double* force)
{
    if (!c || !force) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    if (c->variant != HQ_VARIANT_SCATTER) return hq_fail(HQ_ERR_STATE, "no force array in the patch variant%s", "");
    HQ_HIP(hipSetDevice(c->device));
    HQ_HIP(hq_quiesce(c));
    return hq_copy_wait(force, c->d_force, sizeof(double) * 3 * (size_t)c->N, hipMemcpyDeviceToHost, c->stream);
}
