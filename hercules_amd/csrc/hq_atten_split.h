/* hq_atten_split.h -- BKT attenuation beside the patch and brick step (hq_attenuation_set_split): the correction pass.
 *
 * Under BKT c3 = c4 = 0, so the patch and brick kernels apply mu K_mu + kappa K_kappa to u1 itself, and the BKT force
 * mu K_mu ws + kappa K_kappa wk with ws = u1 + ds, wk = u1 + dk (hq_atten.h) is that elastic force plus
 *     dF = mu K_mu ds + kappa K_kappa dk.
 * Everything behind the force is linear in it -- the hanging nodes' distribution, (f + m2 u1 - m u2) / n_t[0], the hanging
 * nodes' assignment -- so the attenuated step is the UNCHANGED elastic step followed by u_new += dF / n_t[0], dF distributed
 * like any force and the hanging nodes assigned again.  No step kernel, plan or launch of the elastic path changes.
 *
 *   hq_k_atten_advance_delta   one thread per (node, class) slot: the memory variables, and ds, dk into the rows w [6][nslots]
 *   hq_k_atten_corner_force    one thread per element: its 24 corner forces of (ds, dk) into ef [3][8][Epad]   (no atomics)
 *   hq_k_atten_node_sum        one thread per node: dF[n] = the sum of its (element, corner) entries IN ELEMENT ORDER through
 *                              a host-built CSR -- one summation order, the same bits on every run
 *   hq_k_distribute            (the engine's) over all hanging nodes of dF
 *   hq_k_atten_apply           un[n] += dF[n] / m[n], m = n_t[n][0] as a row of the context's own (the brick units keep
 *                              theirs packed)
 *   hq_k_adjust_assign         (the engine's) on un
 * The first three read u(t) and u(t - dt) only and run on a stream of their own beside the step; the last three follow every
 * step kernel on the compute stream.  All of it in the device's node numbering (lnid through hq_ctx.perm); the slot of every
 * corner is kept on the host in the caller's element order, so hq_attenuation_fetch / _load keep the reference's per-corner
 * layout, while the device's tables follow an element order of their own (hq_split_plan.epos, below).
 *
 * Traffic models (per element of a uniform region, one node and one slot per element; docs/LABNOTES.md has the measurements):
 *   two-pass (built)       advance 48 + 96 + 96 + 48 = 288 B per slot; corner force 32 (eslot) + 16 (c1, c2) + 192 written
 *                          + the 48 gathered doubles (384 B requested, ~48 B from HBM: neighbours share the rows); node sum 32
 *                          (entries) + 4 (ptr) + 192 read + 24 written; apply 24 + 24 + 24 + 8 = 80: 908 B per node
 *   one-pass node gather   no ef (saves 384 B) and no CSR, but every node repeats the butterflies of its eight elements: 8 x
 *                          the arithmetic and 8 x 48 gathered doubles per node, and a node on a level interface, with other
 *                          than eight elements around it, needs the same table as the two-pass form to find them
 * Included by hq_engine.hip (one translation unit): uses its hq_fail, hq_real and hq_element_force_bkt. */
#ifndef HQ_ATTEN_SPLIT_H
#define HQ_ATTEN_SPLIT_H

/* The device keeps the elements of the correction in an order of its own, epos[e] = the place of the caller's element e:
 * sorted by the element's lowest node in DEVICE numbering, so that neighbouring threads of hq_k_atten_corner_force gather
 * neighbouring slots and neighbouring nodes of hq_k_atten_node_sum read neighbouring corner forces (behind bricks the device
 * numbers the nodes tile column by tile column, and the caller's element order has nothing to do with that).
 * node -> (element, corner): entry = corner * Epad + epos[e], the index of the corner's force inside a component of ef; per
 * node in the CALLER's element order -- the one summation order.  And the distribution of ALL hanging nodes on node ids,
 * as the scatter variant has it. */
struct hq_split_plan {
    std::vector<int32_t> epos;               /* [E]     */
    std::vector<int32_t> nptr;               /* [N + 1] */
    std::vector<int32_t> nent;               /* [8 E]   */
    std::vector<int32_t> sd;                 /* {hanging node, anchor, deps} in the reference's loop order */
    int64_t nanchors = 0, npairs = 0;        /* distinct anchors, (hanging node, anchor) pairs */
};

/* the device bytes a split context adds beyond hq_atten_bytes: corner forces, c1 / c2, the node table, dF, the mass row, the
 * distribution tables (dst, ptr, src, deps; none without hanging nodes) */
static int64_t hq_split_bytes(int64_t E, int64_t Epad, int64_t N, int64_t nanchors, int64_t npairs)
{
    return 192 * Epad + 16 * E + 32 * E + 4 * (N + 1) + 24 * N + 8 * N + (npairs ? 8 * nanchors + 4 + 8 * npairs : 0);
}

/* lnid [E][8] in the numbering the device uses */
static int hq_split_plan_build(int64_t E, int64_t N, int64_t Epad, const int32_t* lnid, int32_t ndn, const int32_t* dn_id,
                               const int32_t* dn_ptr, const int32_t* dn_anchor, hq_split_plan* S)
{
    if (8 * Epad > (int64_t)0x7fffffff) return hq_fail(HQ_ERR_ARG, "attenuation: more than 2^31 - 1 element corners%s", "");
    {
        std::vector<int32_t> low((size_t)E), order((size_t)E);
#pragma omp parallel for schedule(static)
        for (int64_t e = 0; e < E; e++) {
            int32_t m = lnid[8 * e];
            for (int i = 1; i < 8; i++) m = std::min(m, lnid[8 * e + i]);
            low[(size_t)e] = m;
            order[(size_t)e] = (int32_t)e;
        }
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return low[(size_t)a] < low[(size_t)b]; });
        S->epos.resize((size_t)E);
        for (int64_t k = 0; k < E; k++) S->epos[(size_t)order[(size_t)k]] = (int32_t)k;
    }
    S->nptr.assign((size_t)N + 1, 0);
    for (int64_t i = 0; i < 8 * E; i++) S->nptr[(size_t)lnid[i] + 1]++;
    for (int64_t n = 0; n < N; n++) S->nptr[(size_t)n + 1] += S->nptr[(size_t)n];
    std::vector<int32_t> at(S->nptr.begin(), S->nptr.end() - 1);
    S->nent.resize((size_t)(8 * E));
    for (int64_t e = 0; e < E; e++)                                 /* element order, inside an element corner order */
        for (int i = 0; i < 8; i++) S->nent[(size_t)at[(size_t)lnid[8 * e + i]]++] = (int32_t)(i * Epad + S->epos[(size_t)e]);
    S->sd.clear();
    std::vector<int32_t> anchors;
    for (int32_t k = 0; k < ndn; k++)
        for (int32_t a = dn_ptr[k]; a < dn_ptr[k + 1]; a++) {
            S->sd.push_back(dn_id[k]); S->sd.push_back(dn_anchor[a]); S->sd.push_back(dn_ptr[k + 1] - dn_ptr[k]);
            anchors.push_back(dn_anchor[a]);
        }
    S->npairs = (int64_t)anchors.size();
    std::sort(anchors.begin(), anchors.end());
    S->nanchors = (int64_t)(std::unique(anchors.begin(), anchors.end()) - anchors.begin());
    return HQ_OK;
}

/*
 * What must hold of the tables, counted.  Element order: epos is a permutation of 0 .. E - 1.  Node table: ptr starts at 0,
 * ends at 8 E and never falls; an entry names an element corner of the mesh whose node is the node that lists it; inside a
 * node the entries rise in the caller's element order; every corner is listed exactly once.  Hanging-node lists ({node, anchor, deps} triples against the description's table): every (hanging
 * node, anchor) pair once, deps = the node's number of anchors, no anchor that is itself hanging.
 */
static int64_t hq_split_plan_faults(int64_t E, int64_t N, int64_t Epad, const int32_t* lnid, int32_t ndn, const int32_t* dn_id,
                                    const int32_t* dn_ptr, const int32_t* dn_anchor, const int32_t* epos, const int32_t* nptr,
                                    const int32_t* nent, const int32_t* sd, int64_t nsd)
{
    int64_t bad = 0;
    std::vector<int32_t> elem((size_t)E, -1);                       /* place -> the caller's element */
    for (int64_t e = 0; e < E; e++) {
        if (epos[e] < 0 || epos[e] >= E || elem[(size_t)epos[e]] >= 0) return 1 + 8 * E;
        elem[(size_t)epos[e]] = (int32_t)e;
    }
    if (nptr[0] != 0 || nptr[N] != 8 * E) return 1 + 8 * E;         /* (nothing below can be trusted to stay in bounds) */
    for (int64_t n = 0; n < N; n++)
        if (nptr[n + 1] < nptr[n]) return 1 + 8 * E;
    std::vector<char> seen((size_t)(8 * E), 0);
    for (int64_t n = 0; n < N; n++)
        for (int32_t q = nptr[n]; q < nptr[n + 1]; q++) {
            const int64_t x = nent[q], i = Epad > 0 ? x / Epad : -1, at = Epad > 0 ? x % Epad : -1;
            if (x < 0 || i < 0 || i > 7 || at >= E) { bad++; continue; }
            const int64_t e = elem[(size_t)at];
            if (lnid[8 * e + i] != n) bad++;
            if (seen[(size_t)(8 * e + i)]++) bad++;
            if (q > nptr[n]) {
                const int64_t y = nent[q - 1], ip = y / Epad;
                if (y >= 0 && y % Epad < E && ip >= 0 && ip <= 7) {
                    const int64_t ep = elem[(size_t)(y % Epad)];
                    if (ep > e || (ep == e && ip >= i)) bad++;
                }
            }
        }
    for (int64_t k = 0; k < 8 * E; k++) bad += !seen[(size_t)k];
    std::vector<char> hanging((size_t)N, 0);
    for (int32_t k = 0; k < ndn; k++) hanging[(size_t)dn_id[k]] = 1;
    int64_t want = 0, at = 0;
    for (int32_t k = 0; k < ndn; k++)
        for (int32_t a = dn_ptr[k]; a < dn_ptr[k + 1]; a++, want++, at++) {
            if (at >= nsd) { bad++; continue; }
            if (sd[3 * at] != dn_id[k] || sd[3 * at + 1] != dn_anchor[a] || sd[3 * at + 2] != dn_ptr[k + 1] - dn_ptr[k]) bad++;
            if (hanging[(size_t)dn_anchor[a]]) bad++;
        }
    if (nsd > want) bad += nsd - want;
    return bad;
}

/* hq_k_distribute's tables of a plan's {hanging node, anchor, deps} triples: the entries grouped by the anchor they add to,
 * inside an anchor in the triples' order (hq_build_distribution's grouping) */
static void hq_split_group_by_anchor(const std::vector<int32_t>& sd, std::vector<int32_t>* dst, std::vector<int32_t>* ptr,
                                     std::vector<int32_t>* src, std::vector<int32_t>* deps)
{
    const size_t n = sd.size() / 3;
    std::vector<int32_t> order(n);
    for (size_t i = 0; i < n; i++) order[i] = (int32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return sd[3 * (size_t)x + 1] < sd[3 * (size_t)y + 1]; });
    dst->clear(); src->clear(); deps->clear(); ptr->assign(1, 0);
    for (size_t k = 0; k < n; k++) {
        const size_t i = (size_t)order[k];
        if (dst->empty() || dst->back() != sd[3 * i + 1]) { if (!dst->empty()) ptr->push_back((int32_t)src->size()); dst->push_back(sd[3 * i + 1]); }
        src->push_back(sd[3 * i]); deps->push_back(sd[3 * i + 2]);
    }
    ptr->push_back((int32_t)src->size());
}

#if defined(__HIPCC__)
/*
 * hq_k_atten_advance in delta form (the text is hq_atten.h's hq_atten_advance_delta): one thread per slot, SoA rows.  Per
 * slot 48 B of fields, 96 B of memory variables read and written, 48 B of delta vectors written.
 */
static __device__ __forceinline__ void hq_atten_slot_delta(int32_t s, int64_t nslots, const double* __restrict__ k,
                                                           const hq_real* __restrict__ p1, const hq_real* __restrict__ p2,
                                                           double* __restrict__ mv, double* __restrict__ w)
{
#pragma unroll
    for (int d = 0; d < 3; d++) {
        double f[HQ_ATTEN_NVAR], ds, dk;
#pragma unroll
        for (int v = 0; v < HQ_ATTEN_NVAR; v++) f[v] = mv[(int64_t)(3 * v + d) * nslots + s];
        hq_atten_advance_delta((double)p1[d], (double)p2[d], k, f, 1, &ds, &dk);
#pragma unroll
        for (int v = 0; v < HQ_ATTEN_NVAR; v++) mv[(int64_t)(3 * v + d) * nslots + s] = f[v];
        w[(int64_t)d * nslots + s] = ds;
        w[(int64_t)(3 + d) * nslots + s] = dk;
    }
}

__global__ void __launch_bounds__(256)
hq_k_atten_advance_delta(int32_t nslots, const int32_t* __restrict__ slot_node, const int32_t* __restrict__ slot_class,
                         const double* __restrict__ ktab, const hq_real* __restrict__ u1, const hq_real* __restrict__ u2,
                         double* __restrict__ mv, double* __restrict__ w)
{
    const int32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nslots) return;
    const int64_t row = 3 * (int64_t)slot_node[s];
    const int32_t cls = slot_class[s];
    const int32_t cls0 = __builtin_amdgcn_readfirstlane(cls);
    if (__all(cls == cls0)) hq_atten_slot_delta(s, nslots, ktab + HQ_ATTEN_NCOEF * cls0, u1 + row, u2 + row, mv, w);
    else hq_atten_slot_delta(s, nslots, ktab + HQ_ATTEN_NCOEF * cls, u1 + row, u2 + row, mv, w);
}

/*
 * The correction force, first pass: one thread per element gathers ds, dk at its eight slots, runs the fused butterfly
 * (hq_element_force_bkt is linear in the vectors) and writes its 24 corner forces to ef [3][8][Epad]: 24 coalesced rows,
 * no atomics.  Nothing is added here, so nothing depends on the order the elements run in.
 */
__global__ void __launch_bounds__(256)
hq_k_atten_corner_force(int32_t E, int32_t Epad, int32_t nslots, const int32_t* __restrict__ eslot,
                        const double* __restrict__ c1v, const double* __restrict__ c2v, const double* __restrict__ w,
                        double* __restrict__ ef)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
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
        double* o = ef + (int64_t)n * Epad + e;
        o[0] = X[n];
        o[8 * (int64_t)Epad] = Y[n];
        o[16 * (int64_t)Epad] = Z[n];
    }
}

/* second pass: one thread per node adds its entries in the table's order (element order): dF [N][3] */
__global__ void __launch_bounds__(256)
hq_k_atten_node_sum(int32_t N, int32_t Epad, const int32_t* __restrict__ nptr, const int32_t* __restrict__ nent,
                    const double* __restrict__ ef, double* __restrict__ dF)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int32_t lo = nptr[n], hi = nptr[n + 1];
    double fx = 0.0, fy = 0.0, fz = 0.0;
    for (int32_t q = lo; q < hi; q++) {
        const double* p = ef + nent[q];
        fx += p[0];
        fy += p[8 * (int64_t)Epad];
        fz += p[16 * (int64_t)Epad];
    }
    dF[3 * (int64_t)n + 0] = fx;
    dF[3 * (int64_t)n + 1] = fy;
    dF[3 * (int64_t)n + 2] = fz;
}

/* un += dF / n_t[0]: one thread per scalar */
__global__ void __launch_bounds__(256)
hq_k_atten_apply(int64_t n3, const double* __restrict__ mass, const double* __restrict__ dF, hq_real* __restrict__ un)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n3) return;
    un[t] = (hq_real)((double)un[t] + dF[t] / mass[t / 3]);
}

/* the same over a list of nodes, dF and the mass on the list's indices: un[node[k]] += dF[k] / mass[k] (hq_nonlin_dev.h) */
__global__ void __launch_bounds__(256)
hq_k_atten_apply_at(int64_t n3, const int32_t* __restrict__ node, const double* __restrict__ mass, const double* __restrict__ dF,
                    hq_real* __restrict__ un)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n3) return;
    const int64_t k = t / 3, at = 3 * (int64_t)node[k] + (t - 3 * k);
    un[at] = (hq_real)((double)un[at] + dF[t] / mass[k]);
}
#endif /* __HIPCC__ */

#endif /* HQ_ATTEN_SPLIT_H */
