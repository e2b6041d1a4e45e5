/*
 * hq_opts.h -- where a context's settings come from: hq_options (include/hq_solver.h; the typed, per-context form, after
 * the reference's explicit Param struct psolve.c:193-284) with the HQ_* environment variables as overrides for
 * experiments where the caller allows them (hq_options.allow_env).  One resolver, run once per context at hq_create_opts
 * (hq_options_resolve): the field, overridden by the environment where allowed; else -1 = the library's default.
 *
 * Nothing else is kept here: the resolved struct lives in the context (hq_ctx.opts), planners and set-up code take it
 * as a `const hq_options&` parameter and read its fields.  g_opt_table is the only place that names a field's variable.
 */
#ifndef HQ_OPTS_H
#define HQ_OPTS_H

#include <cstddef>
#include <cstdlib>
#include <cstring>

struct hq_opt_entry { const char* env; size_t off; int kind; };     /* kind 0: int32, 1: double */

#define HQ_OPT_I(env_, field_) { env_, offsetof(hq_options, field_), 0 }
#define HQ_OPT_D(env_, field_) { env_, offsetof(hq_options, field_), 1 }
static const hq_opt_entry g_opt_table[] = {
    HQ_OPT_I("HQ_NO_BRICKS", no_bricks), HQ_OPT_I("HQ_BRICK_CZ", brick_cz), HQ_OPT_I("HQ_BRICK_MINZ", brick_minz),
    HQ_OPT_I("HQ_BRICK_MINNODES", brick_minnodes), HQ_OPT_I("HQ_BRICK_NO_HET", brick_no_het),
    HQ_OPT_I("HQ_BRICK_NO_NTSAME", brick_no_ntsame), HQ_OPT_I("HQ_BRICK_BY_COMPONENT", brick_by_component),
    HQ_OPT_I("HQ_BRICK_STREAM", brick_stream), HQ_OPT_I("HQ_BRICK_NO_FACES", brick_no_faces), HQ_OPT_I("HQ_BRICK_HALF_TILES", brick_half_tiles), HQ_OPT_I("HQ_BRICK_NO_PACK", brick_no_pack), HQ_OPT_I("HQ_PATCH_PIPE", patch_pipe), HQ_OPT_I("HQ_PATCH_THREADS", patch_threads),
    HQ_OPT_I("HQ_PATCH_PMAX", patch_pmax), HQ_OPT_I("HQ_PATCH_PMERGE", patch_pmerge), HQ_OPT_I("HQ_PATCH_PSPLIT", patch_psplit),
    HQ_OPT_I("HQ_PATCH_NLMAX", patch_nlmax), HQ_OPT_I("HQ_PATCH_VMAX", patch_vmax), HQ_OPT_I("HQ_PATCH_RAGGED", patch_ragged),
    HQ_OPT_I("HQ_PATCH_NO_LATTICE", patch_no_lattice), HQ_OPT_I("HQ_PATCH_NO_STENCIL", patch_no_stencil),
    HQ_OPT_I("HQ_PATCH_NO_UNIFORM", patch_no_uniform), HQ_OPT_I("HQ_PATCH_NO_ISO", patch_no_iso),
    HQ_OPT_I("HQ_PATCH_NO_NTSAME", patch_no_ntsame), HQ_OPT_I("HQ_PATCH_NO_DEDUP", patch_no_dedup),
    HQ_OPT_I("HQ_PATCH_WFORM", patch_wform), HQ_OPT_I("HQ_PATCH_MERGE_ROUNDS", patch_merge_rounds),
    HQ_OPT_I("HQ_OVERLAP", overlap), HQ_OPT_I("HQ_NO_OVERLAP", no_overlap), HQ_OPT_I("HQ_RESERVE_CUS", reserve_cus),
    HQ_OPT_I("HQ_CU_MASK", cu_mask), HQ_OPT_I("HQ_NO_FUSED_SHARE", no_fused_share), HQ_OPT_I("HQ_GROUP_COPIES", group_copies),
    HQ_OPT_I("HQ_DEBUG_HALO", debug_halo), HQ_OPT_I("HQ_IPC_ARENA", ipc_arena), HQ_OPT_D("HQ_IPC_TIMEOUT_MS", ipc_timeout_ms),
    HQ_OPT_D("HQ_LOOPBACK_DELAY_US", loopback_delay_us), HQ_OPT_I("HQ_PATCH_VERBOSE", verbose), HQ_OPT_I("HQ_QUIET", quiet),
    HQ_OPT_I("HQ_BRICK_RAGGED", brick_ragged), HQ_OPT_I("HQ_BRICK_RAGGED_MINFILL", brick_ragged_minfill),
    HQ_OPT_I("HQ_PHASE_TIMING", phase_timing), HQ_OPT_I("HQ_BRICK_RAGGED_HET", brick_ragged_het),
};
#undef HQ_OPT_I
#undef HQ_OPT_D

static void hq_options_defaults(hq_options* o)
{
    o->size = sizeof(hq_options);
    for (const hq_opt_entry& e : g_opt_table) {
        if (e.kind == 0) *(int32_t*)((char*)o + e.off) = -1;
        else *(double*)((char*)o + e.off) = -1.0;
    }
    o->allow_env = -1;
    o->reserved0 = -1;
}

/* the caller's struct (of its own size) into a full one */
static void hq_options_adopt(hq_options* dst, const hq_options* src)
{
    hq_options_defaults(dst);
    if (!src) return;
    const size_t n = (size_t)(src->size < sizeof(hq_options) ? src->size : sizeof(hq_options));
    if (n > sizeof(uint64_t)) memcpy((char*)dst + sizeof(uint64_t), (const char*)src + sizeof(uint64_t), n - sizeof(uint64_t));
    dst->size = sizeof(hq_options);
}

/* HQ_IPC_ARENA in the environment is a word; a switch that is set but empty (HQ_PATCH_NO_ISO=) is on */
static int hq_opt_env_int(const char* env, const char* v)
{
    if (!strcmp(env, "HQ_IPC_ARENA")) return !strcmp(v, "fine") ? 0 : (!strcmp(v, "uncached") ? 1 : (!strcmp(v, "coarse") ? 2 : atoi(v)));
    if (!*v) return 1;
    return atoi(v);
}

/*
 * hq_create_opts: the caller's options, completed, with the environment applied ONCE -- and only where the caller allows
 * it: hq_options.allow_env = 1 honours HQ_* variables, 0 ignores them, -1 (default) honours them only in a process that
 * says HQ_ALLOW_ENV=1 (experiments, the test suite, bench.py).  A host program that sets 0 (examples/psolve_hq_stub.inc)
 * cannot be steered by a stray variable.  What comes out is what the context runs with and what hq_get_options returns:
 * switches as 0 / 1 (HQ_X=0 in the environment is OFF), everything else as given; -1 = the library's default.
 */
static void hq_options_resolve(hq_options* out, const hq_options* caller)
{
    hq_options_adopt(out, caller);
    const char* master = getenv("HQ_ALLOW_ENV");
    const bool allow = out->allow_env >= 0 ? out->allow_env != 0 : (master && *master && strcmp(master, "0") != 0);
    out->allow_env = allow ? 1 : 0;
    if (!allow) return;
    for (const hq_opt_entry& e : g_opt_table) {
        const char* v = getenv(e.env);
        if (!v) continue;
        if (e.kind == 0) *(int32_t*)((char*)out + e.off) = hq_opt_env_int(e.env, v);
        else if (*v) *(double*)((char*)out + e.off) = atof(v);
    }
}

/* a resolved field: given at all (not "default")?  its value or the default?  a switch that is on (the environment's
 * HQ_X=, HQ_X=1 came in as 1, HQ_X=0 as 0)?  The same for int32_t and double fields. */
template <typename T> static inline bool hq_given(T f) { return f >= 0; }
template <typename T> static inline T hq_value_or(T f, T def) { return f >= 0 ? f : def; }
template <typename T> static inline bool hq_set(T f) { return f > 0; }

/* a setting without a field (HQ_IPC_COARSE): the environment's word where these options allow it, else null */
static inline const char* hq_opt_env_only(const hq_options& o, const char* env)
{
    return o.allow_env == 1 ? getenv(env) : nullptr;
}

#endif /* HQ_OPTS_H */
