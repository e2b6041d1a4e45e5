/* hq_prepare.h -- the host-only half of hq_create: everything that is decided about a mesh description before the first
 * device allocation.  hq_prepare() validates the description, derives the element coefficients, plans the bricks and
 * renumbers the description behind them, and builds the node sets the patch planner starts from.  It needs no device
 * and makes no HIP call: hq_create_impl (hq_engine.hip) uploads what it leaves, and the plan checks (hq_plan_check.h)
 * begin with the same call, so what they check is what hq_create runs.
 *
 * Included by hq_engine.hip (one translation unit): uses its hq_fail and the planners of hq_patch.h / hq_brick.h. */
#ifndef HQ_PREPARE_H
#define HQ_PREPARE_H

/* f(schedule, side, node id) for every node a schedule of `d` names: schedule 0 = an_sched, 1 = dn_sched; side 0 = the
 * c-lists, 1 = the s-lists; a messenger without a mapping yields -1 for each of its nodes */
template <typename F>
static void hq_for_each_sched_node(const hq_desc* d, F&& f)
{
    const hq_schedule* sched[2] = { &d->an_sched, &d->dn_sched };
    for (int s = 0; s < 2; s++)
        for (int side = 0; side < 2; side++) {
            const int32_t cnt = side ? sched[s]->s_count : sched[s]->c_count;
            const hq_messenger* list = side ? sched[s]->first_s : sched[s]->first_c;
            for (int32_t i = 0; i < cnt; i++)
                for (int32_t k = 0; k < list[i].nodecount; k++) f(s, side, list[i].mapping ? list[i].mapping[k] : -1);
        }
}

/* what a caller of hq_prepare wants beyond the validation and the node sets: c1 / c2 / beta (needs hq_desc.eTable), the
 * n_t rows as doubles (nTable), the brick plan and the renumbering behind it (both of these, and node_xyz) */
enum { HQ_PREP_COEF = 1, HQ_PREP_NT = 2, HQ_PREP_BRICKS = 4 };

struct hq_prep {
    std::vector<double> c1, c2, beta;        /* [E] element coefficients, beta = c3 / c1 (the caller's element order)      */
    const double* ntab = nullptr;            /* [N][7] n_t rows in desc's numbering: the caller's array, nt64 or p_nt      */
    std::vector<char> excl;                  /* [N] caller's numbering: nodes the bricks must leave to the patches         */
    hq_brick_host bricks;                    /* nb == 0: no bricks, desc is the caller's description as it came            */
    std::vector<int32_t> perm;               /* caller's node id -> desc's (moved out of bricks.perm); empty: the same     */
    hq_desc desc;                            /* the description in the numbering planning and the device use; tm1 / tm2
                                              * are NULL behind bricks (they are uploaded through perm)                    */
    std::vector<char> shared_dn;             /* [N] hanging nodes another rank shares (dn_sched's s-lists)                 */
    std::vector<int32_t> l_id, l_ptr, l_anc; /* the hanging nodes the patches distribute themselves: owned, not shared     */
    hq_dangling dn;                          /* ... as the planners take them (points into the three above)                */
    std::vector<char> seed0;                 /* [N] nodes whose update is finished elsewhere: hanging nodes (compute_adjust)
                                              * and the partition interface (every node a schedule names, and the anchors
                                              * of owned hanging nodes that other ranks share)                             */
    /* backing storage of ntab and desc (which point into it: an hq_prep is filled once and not copied) */
    std::vector<double> nt64, p_nt;
    std::vector<int32_t> p_lnid, p_xyz, p_dn_id, p_dn_anchor;
    std::vector<int64_t> p_gnid;
    std::vector<std::vector<int32_t>> p_maps;
    std::vector<hq_messenger> p_msg[4];
    double brick_plan_s = 0, renumber_s = 0; /* where the time went (hq_create's HQ_PATCH_VERBOSE laps)                    */
};

/* the caller's n_t rows (solver_float at the ABI) as the doubles the planners and kernels work with: the caller's own
 * array where hq_real is double, a widened copy in `store` otherwise */
static const double* hq_ntable64(const hq_desc* d, std::vector<double>& store)
{
    if (sizeof(hq_real) == sizeof(double)) return reinterpret_cast<const double*>(d->nTable);
    const size_t n = 7 * (size_t)d->nharbored;
    store.resize(n);
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < (int64_t)n; i++) store[(size_t)i] = (double)d->nTable[i];
    return store.data();
}

static int hq_prepare(const hq_desc* d, const hq_options& o, unsigned what, hq_prep* out)
{
    if (what & HQ_PREP_BRICKS) what |= HQ_PREP_COEF | HQ_PREP_NT;
    if (!d || d->lenum < 0 || d->nharbored <= 0 || d->ldnnum < 0 || (d->lenum && !d->lnid) ||
        ((what & HQ_PREP_COEF) && !d->eTable) || ((what & HQ_PREP_NT) && !d->nTable))
        return hq_fail(HQ_ERR_ARG, "inconsistent mesh description%s", "");
    const int64_t E = d->lenum, N = d->nharbored;
    const int32_t ndn = d->ldnnum;

    for (int64_t i = 0; i < E * 8; i++)
        if (d->lnid[i] < 0 || d->lnid[i] >= N) return hq_fail(HQ_ERR_ARG, "lnid out of range%s", "");
    if (ndn && (!d->dn_ldnid || !d->dn_ptr || !d->dn_lanid)) return hq_fail(HQ_ERR_ARG, "dangling-node tables missing%s", "");
    for (int32_t k = 0; k < ndn; k++) {
        if (d->dn_ldnid[k] < 0 || d->dn_ldnid[k] >= N || d->dn_ptr[k + 1] <= d->dn_ptr[k])
            return hq_fail(HQ_ERR_ARG, "bad dangling-node table%s", "");
        for (int32_t a = d->dn_ptr[k]; a < d->dn_ptr[k + 1]; a++)
            if (d->dn_lanid[a] < 0 || d->dn_lanid[a] >= N) return hq_fail(HQ_ERR_ARG, "bad anchor id%s", "");
    }
    if (ndn) {
        /* an anchor must itself be anchored (octor's 2:1 balance guarantees it): the distribution kernels read the
         * hanging nodes' rows while they add to the anchors' */
        std::vector<char> is_dn((size_t)N, 0);
        for (int32_t k = 0; k < ndn; k++) is_dn[d->dn_ldnid[k]] = 1;
        for (int32_t a = 0; a < d->dn_ptr[ndn]; a++)
            if (is_dn[d->dn_lanid[a]]) return hq_fail(HQ_ERR_ARG, "an anchor is itself a hanging node%s", "");
    }
    bool ids_ok = true;
    hq_for_each_sched_node(d, [&](int, int, int32_t n) { ids_ok = ids_ok && n >= 0 && n < N; });
    if (!ids_ok) return hq_fail(HQ_ERR_ARG, "messenger node id out of range%s", "");

    /* element coefficients: (c1, c2, beta = c3/c1).  The fused product needs c3/c1 == c4/c2 (Rayleigh:
     * both are b/dt, psolve.c:3386-3409); a table that applies different ratios to K1 and K2 is refused */
    if (what & HQ_PREP_COEF) {
        out->c1.resize((size_t)E); out->c2.resize((size_t)E); out->beta.resize((size_t)E);
        for (int64_t e = 0; e < E; e++) {
            const double* ep = d->eTable + 4 * e;
            out->c1[(size_t)e] = ep[0]; out->c2[(size_t)e] = ep[1];
            out->beta[(size_t)e] = (ep[0] != 0.0) ? ep[2] / ep[0] : ((ep[1] != 0.0) ? ep[3] / ep[1] : 0.0);
            const double lhs = ep[2] * ep[1], rhs = ep[3] * ep[0];
            if (fabs(lhs - rhs) > 1e-12 * std::max(fabs(lhs), fabs(rhs)))
                return hq_fail(HQ_ERR_ARG, "eTable is not Rayleigh-proportional (c3/c1 != c4/c2): not the table solver_init builds%s", "");
        }
    }
    auto t_last = std::chrono::steady_clock::now();
    auto lap = [&](double* s) {
        *s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_last).count();
        t_last = std::chrono::steady_clock::now();
    };
    if (what & HQ_PREP_NT) out->ntab = hq_ntable64(d, out->nt64);

    /* nodes that must stay with the patches: hanging nodes, their anchors, every node a schedule names */
    out->excl.assign((size_t)N, 0);
    for (int32_t k = 0; k < ndn; k++) {
        out->excl[d->dn_ldnid[k]] = 1;
        for (int32_t a = d->dn_ptr[k]; a < d->dn_ptr[k + 1]; a++) out->excl[d->dn_lanid[a]] = 1;
    }
    hq_for_each_sched_node(d, [&](int, int, int32_t n) { out->excl[n] = 1; });

    /*
     * Bricks (hq_brick.h): where the mesh has simple nodes in bulk -- uniformly refined, homogeneous, no dashpot, not
     * hanging, not on the partition interface -- they are stepped by the z-marching kernel on a tile-major layout.
     * That needs the nodes renumbered: out->desc is the description in DEVICE numbering (out->perm maps the caller's
     * ids); hq_set_source / hq_gather / hq_download / hq_upload translate.  Needs node_xyz.
     */
    hq_desc& dd = out->desc;
    dd = *d;
    hq_brick_host& BH = out->bricks;
    if ((what & HQ_PREP_BRICKS) && d->node_xyz && !hq_set(o.no_bricks)) {
        hq_mat_src ms;
        ms.edata = d->edata; ms.dt = d->deltaT; ms.bbase = d->mat_bbase; ms.thr_damp = d->mat_threshold_damping; ms.thr_vpvs = d->mat_threshold_vpvs;
        if (hq_brick_plan_host(o, E, N, d->lnid, d->node_xyz, out->c1.data(), out->c2.data(), out->beta.data(), out->ntab,
                               out->excl.data(), &BH, &ms) != 0)
            return hq_fail(HQ_ERR_ARG, "brick plan: %s", hq_patch_error());
        lap(&out->brick_plan_s);
    }
    if (BH.nb > 0) {
        const std::vector<int32_t>& pm = BH.perm;
        bool in_range = (int64_t)pm.size() == N;
#pragma omp parallel for schedule(static) reduction(&& : in_range)
        for (int64_t n = 0; n < (int64_t)pm.size(); n++) in_range = in_range && pm[(size_t)n] >= 0 && pm[(size_t)n] < N;
        if (!in_range) return hq_fail(HQ_ERR_STATE, "brick plan: the numbering leaves the mesh%s", "");
        out->p_lnid.resize((size_t)E * 8);
#pragma omp parallel for schedule(static)
        for (int64_t i = 0; i < E * 8; i++) out->p_lnid[(size_t)i] = pm[(size_t)d->lnid[i]];
        out->p_xyz.resize((size_t)N * 3);
        out->p_nt.resize((size_t)N * 7);
        int32_t* p_xyz = out->p_xyz.data();
        double* p_nt = out->p_nt.data();
        const double* ntab = out->ntab;
#pragma omp parallel for schedule(static)
        for (int64_t n = 0; n < N; n++) {
            const int64_t q = pm[(size_t)n];
            for (int k = 0; k < 3; k++) p_xyz[3 * q + k] = d->node_xyz[3 * n + k];
            for (int k = 0; k < 7; k++) p_nt[7 * q + k] = ntab[7 * n + k];
        }
        dd.lnid = out->p_lnid.data(); dd.node_xyz = p_xyz; dd.nTable = nullptr; out->ntab = p_nt;
        std::vector<double>().swap(out->nt64);
        if (d->node_gnid) {
            out->p_gnid.resize((size_t)N);
            for (int64_t n = 0; n < N; n++) out->p_gnid[(size_t)pm[(size_t)n]] = d->node_gnid[n];
            dd.node_gnid = out->p_gnid.data();
        }
        if (ndn) {
            const int32_t na = d->dn_ptr[ndn];
            out->p_dn_id.resize((size_t)ndn); out->p_dn_anchor.resize((size_t)na);
            for (int32_t k = 0; k < ndn; k++) out->p_dn_id[(size_t)k] = pm[(size_t)d->dn_ldnid[k]];
            for (int32_t a = 0; a < na; a++) out->p_dn_anchor[(size_t)a] = pm[(size_t)d->dn_lanid[a]];
            dd.dn_ldnid = out->p_dn_id.data(); dd.dn_lanid = out->p_dn_anchor.data();
        }
        {
            /* (the messengers keep their lists: not a walk hq_for_each_sched_node can do) */
            const hq_schedule* in[2] = { &d->an_sched, &d->dn_sched };
            hq_schedule* to[2] = { &dd.an_sched, &dd.dn_sched };
            size_t nm = 0;
            for (int s2 = 0; s2 < 2; s2++) nm += (size_t)in[s2]->c_count + (size_t)in[s2]->s_count;
            out->p_maps.reserve(nm);
            for (int s2 = 0; s2 < 2; s2++)
                for (int side = 0; side < 2; side++) {
                    const int32_t cnt = side ? in[s2]->s_count : in[s2]->c_count;
                    const hq_messenger* list = side ? in[s2]->first_s : in[s2]->first_c;
                    std::vector<hq_messenger>& v = out->p_msg[2 * s2 + side];
                    for (int32_t i = 0; i < cnt; i++) {
                        out->p_maps.emplace_back((size_t)list[i].nodecount);
                        for (int32_t k = 0; k < list[i].nodecount; k++) out->p_maps.back()[(size_t)k] = pm[(size_t)list[i].mapping[k]];
                        v.push_back({ list[i].procid, list[i].nodecount, out->p_maps.back().data() });
                    }
                    if (side) to[s2]->first_s = v.data(); else to[s2]->first_c = v.data();
                }
        }
        dd.tm1 = dd.tm2 = nullptr;
        out->perm = std::move(BH.perm);
        lap(&out->renumber_s);
    }

    /* hanging nodes the patches may distribute themselves: owned and not shared with any rank
     * (the shared ones wait for the contribution exchange, hq_setup_interface) */
    out->shared_dn.assign((size_t)N, 0);
    out->seed0.assign((size_t)N, 0);
    hq_for_each_sched_node(&dd, [&](int s, int side, int32_t n) {
        if (s == 1 && side == 1) out->shared_dn[n] = 1;
        out->seed0[n] = 1;
    });
    out->l_ptr.assign(1, 0);
    for (int32_t k = 0; k < ndn; k++) {
        out->seed0[dd.dn_ldnid[k]] = 1;
        if (out->shared_dn[dd.dn_ldnid[k]]) {
            for (int32_t a = dd.dn_ptr[k]; a < dd.dn_ptr[k + 1]; a++) out->seed0[dd.dn_lanid[a]] = 1;
            continue;
        }
        out->l_id.push_back(dd.dn_ldnid[k]);
        for (int32_t a = dd.dn_ptr[k]; a < dd.dn_ptr[k + 1]; a++) out->l_anc.push_back(dd.dn_lanid[a]);
        out->l_ptr.push_back((int32_t)out->l_anc.size());
    }
    out->dn.n = (int32_t)out->l_id.size(); out->dn.id = out->l_id.data(); out->dn.ptr = out->l_ptr.data(); out->dn.anchor = out->l_anc.data();
    return HQ_OK;
}

#endif
