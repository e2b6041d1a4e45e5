/* hq_correction.h -- a correction pass beside the patch and brick step: what does not depend on the pass's physics.
 *
 * A pass adds a force dF to a step that stays as it is.  Everything behind the step's force is linear in it -- the hanging
 * nodes' distribution, (f + m2 u1 - m u2) / n_t[0], the hanging nodes' assignment -- so un += dF / n_t[0], dF distributed
 * like any force and the hanging nodes assigned again, gives the step of the elastic force plus dF.  A pass (split BKT
 * attenuation, hq_atten_split.h; nonlinear soil, hq_nonlin_dev.h) brings the kernels that write the corner forces of its
 * elements into ef [3][8][stride], one thread per element and no atomics; the rest is here and the same for every pass:
 *   hq_k_atten_node_sum        one thread per row: dF[r] = the sum of its (element, corner) entries IN ELEMENT ORDER through a
 *                              host-built CSR -- one summation order, the same bits on every run
 *   hq_k_distribute            (the engine's, hq_distribution) the pass's hanging nodes of dF to their anchors, on row indices
 *   hq_k_atten_apply           un[r] += dF[r] / m[r] where the rows are all nodes, m = n_t[r][0] as a row of the pass's own
 *   hq_k_atten_apply_at        un[node[r]] += dF[r] / m[r] where the rows are a list of nodes (d_tnode)
 *   hq_k_adjust_assign         (the engine's) on un, all hanging nodes
 * The pass's kernels and the node sum run on a stream of their own beside the step, the rest follows every step kernel on
 * the compute stream: hq_correction_fork, hq_correction_sum and hq_correction_join (hq_engine.hip, behind hq_ctx, whose
 * streams and events they order) are that chain, and the argument for its ordering stands over them.
 * All of it in the device's node numbering (lnid through hq_ctx.perm).
 * Included by hq_engine.hip (one translation unit): uses its hq_fail, hq_real, hq_dbuf and hq_distribution. */
#ifndef HQ_CORRECTION_H
#define HQ_CORRECTION_H

/* The device keeps the elements of the correction in an order of its own, epos[e] = the place of the caller's element e:
 * sorted by the element's lowest node in DEVICE numbering, so that neighbouring threads of the pass's element kernel gather
 * neighbouring rows and neighbouring nodes of hq_k_atten_node_sum read neighbouring corner forces (behind bricks the device
 * numbers the nodes tile column by tile column, and the caller's element order has nothing to do with that).
 * node -> (element, corner): entry = corner * Epad + epos[e], the index of the corner's force inside a component of ef; per
 * node in the CALLER's element order -- the one summation order.  And the distribution of ALL hanging nodes on node ids,
 * as the scatter variant has it.  (E, N, Epad: a pass's nelem, rows and stride.) */
struct hq_split_plan {
    std::vector<int32_t> epos;               /* [E]     */
    std::vector<int32_t> nptr;               /* [N + 1] */
    std::vector<int32_t> nent;               /* [8 E]   */
    std::vector<int32_t> sd;                 /* {hanging node, anchor, deps} in the reference's loop order */
    int64_t nanchors = 0, npairs = 0;        /* distinct anchors, (hanging node, anchor) pairs */
};

/* the device bytes of a pass's shared part: corner forces, the node table, dF and the mass per row, the node id per row where
 * the rows are a list, the distribution tables (dst, ptr, src, deps; none without hanging nodes) */
static int64_t hq_correction_bytes(int64_t nelem, int64_t stride, int64_t rows, bool listed, int64_t nanchors, int64_t npairs)
{
    return 192 * stride + 4 * (rows + 1) + 32 * nelem + (24 + 8 + (listed ? 4 : 0)) * rows + (npairs ? 8 * nanchors + 4 + 8 * npairs : 0);
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

#if defined(__HIPCC__)
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

/* the same over a list of nodes, dF and the mass on the list's indices: un[node[k]] += dF[k] / mass[k] */
__global__ void __launch_bounds__(256)
hq_k_atten_apply_at(int64_t n3, const int32_t* __restrict__ node, const double* __restrict__ mass, const double* __restrict__ dF,
                    hq_real* __restrict__ un)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n3) return;
    const int64_t k = t / 3, at = 3 * (int64_t)node[k] + (t - 3 * k);
    un[at] = (hq_real)((double)un[at] + dF[t] / mass[k]);
}

/* a pass's shared part on the device */
struct hq_correction {
    int32_t rows = 0, nelem = 0, stride = 0;  /* N or the touched nodes; the pass's elements; their padded count */
    int64_t bytes = 0;                        /* hq_correction_bytes                                             */
    hq_dbuf<double> d_ef;                     /* [3][8][stride] corner forces of this step                       */
    hq_dbuf<double> d_dF;                     /* [rows][3] their sums per row                                    */
    hq_dbuf<double> d_mass;                   /* [rows] n_t[.][0]                                                */
    hq_dbuf<int32_t> d_nptr, d_nent;          /* [rows + 1], [8 nelem] row -> (element, corner), element order   */
    hq_dbuf<int32_t> d_tnode;                 /* [rows] device node ids; none where the rows are all nodes       */
    hq_distribution dist;                     /* the plan's hanging nodes, on row indices                        */
};

/* The plan's tables, the mass row and (tnode != NULL) the node list onto the device, ef and dF zeroed, in *K beside the
 * context's own: a failure lets K go with its arrays (no ledger: the arrays move, hq_ctx.bytes takes K->bytes at the end) */
static int hq_correction_build(const hq_split_plan& S, int64_t nelem, int64_t stride, const std::vector<double>& mass,
                               const std::vector<int32_t>* tnode, hipStream_t st, hq_correction* K)
{
    const size_t rows = mass.size();
    HQ_TRY(K->d_ef.alloc(nullptr, (size_t)(24 * stride))); HQ_TRY(K->d_ef.fill(0, st));
    HQ_TRY(K->d_dF.alloc(nullptr, 3 * rows)); HQ_TRY(K->d_dF.fill(0, st));
    HQ_TRY(K->d_mass.put(nullptr, mass, st));
    HQ_TRY(K->d_nptr.put(nullptr, S.nptr, st)); HQ_TRY(K->d_nent.put(nullptr, S.nent, st));
    if (tnode) HQ_TRY(K->d_tnode.put(nullptr, *tnode, st));
    HQ_TRY(K->dist.build(S.sd, nullptr, st));
    K->bytes = (int64_t)(K->d_ef.bytes() + K->d_dF.bytes() + K->d_mass.bytes() + K->d_nptr.bytes() + K->d_nent.bytes() + K->d_tnode.bytes()) +
               K->dist.bytes();
    K->rows = (int32_t)rows; K->nelem = (int32_t)nelem; K->stride = (int32_t)stride;
    return HQ_OK;
}
#endif /* __HIPCC__ */

#endif /* HQ_CORRECTION_H */
