/* hq_plan_check.h -- the host-only diagnostics of the planners (no device needed; the -m "not gpu" tests call them).
 * Each begins with hq_prepare (hq_prepare.h), the host half of hq_create: it refuses what hq_create refuses and plans
 * on the description hq_create plans on.  Included by hq_engine.hip: the same translation unit. */
#ifndef HQ_PLAN_CHECK_H
#define HQ_PLAN_CHECK_H

/*
 * Host-only self-check of the patch planner: plans the mesh WITHOUT bricks (n0 = 0: every node is a patch node, as
 * hq_create plans with HQ_NO_BRICKS or without node_xyz) and verifies that every element row names the LDS rows
 * of its element's eight nodes, that the accumulate flags are exactly the owned nodes and the
 * hanging nodes on owned anchors, and counts the LDS passes of the gathers under the bank rule of
 * MI355X_MICROARCH.md (32-lane groups, rows distinct modulo 32).
 * report: {patches, lattice patches, (patch, element) pairs, distinct element-row blocks,
 *          gather passes, gather instructions (per 32-lane group), gather passes of the lattice patches
 *          (= 23 groups x 8 corners each when conflict-free), faults}
 */
extern "C" int hq_plan_check(const hq_desc* d, int64_t report[8])
{
    hq_options opts;                                  /* host-only diagnostic: the library defaults, the environment where HQ_ALLOW_ENV=1 */
    hq_options_resolve(&opts, nullptr);
    if (!report) return hq_fail(HQ_ERR_ARG, "inconsistent mesh description%s", "");
    hq_prep prep;
    HQ_TRY(hq_prepare(d, opts, 0, &prep));
    const int64_t E = d->lenum, N = d->nharbored;
    const hq_dangling& dn = prep.dn;
    bool want_lattice = false;
    const hq_patch_cfg cfg = hq_patch_cfg_of(opts, dn.n > 0, d->node_xyz != nullptr, &want_lattice);
    if (const char* why = hq_patch_cfg_refusal(cfg)) return hq_fail(HQ_ERR_ARG, "patch plan: %s", why);
    hq_patch_host H;
    if (hq_patch_plan_host(opts, cfg, E, N, d->lnid, d->node_xyz, dn, want_lattice, &H) != 0)
        return hq_fail(HQ_ERR_ARG, "patch plan: %s", hq_patch_error());
    const hq_lattice_tab& T = hq_lattice();
    int64_t nlat = 0, passes = 0, lpasses = 0, instr = 0, bad = 0;
    std::vector<int32_t> covered((size_t)N, 0);
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : nlat, passes, lpasses, instr, bad)
    for (int64_t p = 0; p < (int64_t)H.desc.size(); p++) {
        const hq_patch_desc& D = H.desc[(size_t)p];
        const bool lat = H.lattice[(size_t)p] != 0;
        nlat += lat;
        std::vector<int32_t> node_of_row(lat ? HQ_LAT_ROWS : (size_t)(D.nown + D.nhalo), -1);
        for (int32_t t = 0; t < D.nown + D.nhalo; t++) {
            const int32_t g = t < D.nown ? D.base + t : H.halo[(size_t)D.halo_off + (t - D.nown)];
            const int32_t r = lat ? (int32_t)T.row_of_local[t] : t;
            if (r < 0 || r >= (int32_t)node_of_row.size() || node_of_row[r] >= 0) { bad++; continue; }
            node_of_row[r] = g;
        }
        for (int32_t t = 0; t < D.nown; t++) {
#pragma omp atomic
            covered[(size_t)D.base + t]++;
        }
        const uint16_t* rows = H.pidx.data() + 8 * (size_t)D.pidx_off;
        for (int32_t q = 0; q < D.npairs; q++) {
            const int32_t* id = d->lnid + 8 * (int64_t)H.pelem[(size_t)D.pair_off + q];
            for (int c = 0; c < 8; c++) {
                const int32_t r = rows[8 * (size_t)q + c] & HQ_PIDX_ROW;
                const bool acc = (rows[8 * (size_t)q + c] & HQ_PIDX_ACC) != 0;
                if (r >= (int32_t)node_of_row.size() || node_of_row[r] != id[c]) { bad++; continue; }
                const bool owned = id[c] >= D.base && id[c] < D.base + D.nown;
                /* an accumulator: owned nodes, and (id-ordered patches) the first nacc - nown halo rows */
                const bool want = owned || (!lat && r < D.nacc);
                if (acc != want) bad++;
                if (lat && acc && r >= HQ_LAT_ACC) bad++;
            }
        }
        for (int32_t w = 0; w < D.npairs; w += 32)
            for (int c = 0; c < 8; c++) {
                int cls[32] = { 0 }, mx = 0;
                for (int32_t q = w; q < std::min(w + 32, D.npairs); q++) {
                    /* identical rows broadcast; distinct rows of one class take a pass each */
                    const int32_t r = rows[8 * (size_t)q + c] & HQ_PIDX_ROW;
                    bool dup = false;
                    for (int32_t q2 = w; q2 < q; q2++) dup |= ((rows[8 * (size_t)q2 + c] & HQ_PIDX_ROW) == r);
                    if (!dup) mx = std::max(mx, ++cls[r & 31]);
                }
                passes += mx;
                if (lat) lpasses += mx;
                instr++;
            }
    }
    for (int64_t n = 0; n < N; n++) if (covered[(size_t)n] != 1) bad++;
    if (hq_set(opts.verbose)) {                                 /* owned-node histogram of the patches */
        int64_t hist[8] = { 0 }, hp[8] = { 0 };
        for (auto& D : H.desc) {
            int b = D.nown <= 8 ? 0 : D.nown <= 64 ? 1 : D.nown <= 128 ? 2 : D.nown <= 256 ? 3 : D.nown < 512 ? 4 : D.nown == 512 ? 5 : D.nown <= 640 ? 6 : 7;
            hist[b]++; hp[b] += D.npairs;
        }
        const char* nm[8] = { "<=8", "<=64", "<=128", "<=256", "<512", "=512", "<=640", ">640" };
        for (int b = 0; b < 8; b++) fprintf(stderr, "hq plan: %8lld patches with %6s owned nodes, %10lld pairs\n", (long long)hist[b], nm[b], (long long)hp[b]);
    }
    report[0] = (int64_t)H.desc.size(); report[1] = nlat; report[2] = (int64_t)H.pelem.size();
    report[3] = H.ndistinct; report[4] = passes; report[5] = instr;
    report[6] = lpasses; report[7] = bad;
    if (bad) return hq_fail(HQ_ERR_STATE, "patch plan self-check failed%s", "");
    return HQ_OK;
}

/*
 * The sixteen numbers of the assembled 27-point stencil (hq_stencil in hq_patch.h), as hq_k_patch_stencil
 * uses them: out = {p1[6], p2[6], q1[2], q2[2]} for S = c1 S1 + c2 S2.  Host only; HQ_ERR_STATE if the
 * cube symmetry the kernel relies on does not hold for the element arithmetic (then no patch is marked).
 */
extern "C" int hq_stencil_coefficients(double out[16])
{
    if (!out) return hq_fail(HQ_ERR_ARG, "null argument%s", "");
    const hq_stencil_tab& t = hq_stencil();
    for (int i = 0; i < 6; i++) { out[i] = t.c.p1[i]; out[6 + i] = t.c.p2[i]; }
    for (int i = 0; i < 2; i++) { out[12 + i] = t.c.q1[i]; out[14 + i] = t.c.q2[i]; }
    return t.ok ? HQ_OK : hq_fail(HQ_ERR_STATE, "the assembled stencil lacks the cube symmetry%s", "");
}

/*
 * Host-only self-check of what hq_k_patch_stencil reads (needs no device).  Plans `desc` without bricks (n0 = 0, as
 * hq_plan_check does); for every
 * patch whose geometry hq_ragged_match accepts (whatever its coefficients) it checks the shape table against the
 * mesh: rows distinct and inside the image; the eight nodes of every element of the patch at row(corner 0) + the
 * lattice offsets of their corner; the element mask of every owned node = the corners it really is in the patch's
 * elements; the boundary list = the owned nodes with an incomplete mask, in order, with their index.  And once: the
 * element-matrix blocks E1, E2 of the boundary phase reproduce hq_element_force (the kernels' own arithmetic) for
 * random displacements and every subset of present octants.
 * report = {patches, patches with a table, full lattices among them, boundary nodes, element corners checked, faults}
 */
extern "C" int hq_stencil_plan_check(const hq_desc* d, int64_t report[6])
{
    hq_options opts;                                  /* host-only diagnostic: the library defaults, the environment where HQ_ALLOW_ENV=1 */
    hq_options_resolve(&opts, nullptr);
    if (!d || !report || !d->node_xyz) return hq_fail(HQ_ERR_ARG, "inconsistent mesh description (node_xyz is needed)%s", "");
    hq_prep prep;
    HQ_TRY(hq_prepare(d, opts, 0, &prep));
    const int64_t E = d->lenum, N = d->nharbored;
    const hq_dangling& dn = prep.dn;
    bool want_lattice = false;
    const hq_patch_cfg cfg = hq_patch_cfg_of(opts, dn.n > 0, true, &want_lattice);
    if (const char* why = hq_patch_cfg_refusal(cfg)) return hq_fail(HQ_ERR_ARG, "patch plan: %s", why);
    hq_patch_host H;
    if (hq_patch_plan_host(opts, cfg, E, N, d->lnid, d->node_xyz, dn, want_lattice, &H) != 0)
        return hq_fail(HQ_ERR_ARG, "patch plan: %s", hq_patch_error());
    int64_t ntab = 0, nfull = 0, nbnd_tot = 0, ncorner = 0, bad = 0;
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : ntab, nfull, nbnd_tot, ncorner, bad)
    for (int64_t p = 0; p < (int64_t)H.desc.size(); p++) {
        const hq_patch_desc& D = H.desc[(size_t)p];
        if (D.nacc != D.nown) continue;
        if (!H.ds_ptr.empty() && H.ds_ptr[(size_t)p + 1] > H.ds_ptr[(size_t)p]) continue;
        std::vector<int32_t> h(H.halo.begin() + D.halo_off, H.halo.begin() + D.halo_off + D.nhalo);
        std::vector<uint32_t> tab;
        int32_t nbnd = 0;
        if (!hq_ragged_match(D.base, D.nown, d->lnid, d->node_xyz, &H.pelem[(size_t)D.pair_off], D.npairs, h, tab, &nbnd)) continue;
        ntab++;
        nbnd_tot += nbnd;
        if (nbnd == 0 && D.nown == HQ_LAT_NOWN && D.nhalo == HQ_LAT_NHALO && D.npairs == HQ_LAT_NELEM) nfull++;
        const int32_t nloc = D.nown + D.nhalo;
        if ((int32_t)tab.size() < nloc + nbnd) { bad++; continue; }
        std::unordered_map<int32_t, int32_t> local_of;
        std::vector<char> used(HQ_ST_ROWS, 0);
        for (int32_t t = 0; t < nloc; t++) {
            local_of[t < D.nown ? D.base + t : h[(size_t)(t - D.nown)]] = t;
            const int r = HQ_RG_ROW(tab[(size_t)t]);
            if (r >= HQ_ST_ROWS || used[(size_t)r]) bad++; else used[(size_t)r] = 1;
        }
        std::vector<unsigned> want((size_t)D.nown, 0u);
        for (int32_t q = 0; q < D.npairs; q++) {
            const int32_t* id = d->lnid + 8 * (int64_t)H.pelem[(size_t)D.pair_off + q];
            auto it0 = local_of.find(id[0]);
            if (it0 == local_of.end()) { bad++; continue; }
            const int r0 = HQ_RG_ROW(tab[(size_t)it0->second]);
            for (int c = 0; c < 8; c++) {
                auto it = local_of.find(id[c]);
                if (it == local_of.end()) { bad++; continue; }
                const int r = HQ_RG_ROW(tab[(size_t)it->second]);
                if (r != r0 + HQ_ST_PX * (c & 1) + HQ_ST_PY * ((c >> 1) & 1) + HQ_ST_PZ * ((c >> 2) & 1)) bad++;
                if (it->second < D.nown) want[(size_t)it->second] |= 1u << c;
                ncorner++;
            }
        }
        int32_t nb = 0;
        for (int32_t t = 0; t < D.nown; t++) {
            const uint32_t w = tab[(size_t)t];
            if (HQ_RG_MASK(w) != want[(size_t)t]) bad++;
            if (want[(size_t)t] != 0xffu) {
                if (nb >= nbnd || HQ_RG_BIDX(w) != nb) bad++;
                else {
                    const uint32_t b = tab[(size_t)(nloc + nb)];
                    if (HQ_RG_ROW(b) != HQ_RG_ROW(w) || HQ_RG_MASK(b) != want[(size_t)t]) bad++;
                }
                nb++;
            }
        }
        if (nb != nbnd) bad++;
    }
    /* E1, E2 against the element arithmetic: a node that is corner o of its present elements */
    {
        const hq_stencil_tab& T = hq_stencil();
        if (!T.ok) bad++;
        uint64_t seed = 88172645463325252ull;
        auto rnd = [&]() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return (double)(seed >> 11) / 9007199254740992.0 - 0.5; };
        for (int trial = 0; trial < 64; trial++) {
            const double c1 = 1.0 + rnd(), c2 = 2.0 + rnd();
            const unsigned mask = (unsigned)(trial * 37 + 1) & 0xffu;
            double w[27][3];                             /* the 3x3x3 nodes around the node, index (dx+1) + 3 (dy+1) + 9 (dz+1) */
            for (auto& r : w) for (double& v : r) v = rnd();
            double ref[3] = { 0, 0, 0 }, got[3] = { 0, 0, 0 };
            for (int o = 0; o < 8; o++) {
                if (!((mask >> o) & 1)) continue;
                double X[8], Y[8], Z[8];
                for (int m = 0; m < 8; m++) {
                    const int dx = (m & 1) - (o & 1), dy = ((m >> 1) & 1) - ((o >> 1) & 1), dz = ((m >> 2) & 1) - ((o >> 2) & 1);
                    const double* q = w[(dx + 1) + 3 * (dy + 1) + 9 * (dz + 1)];
                    X[m] = q[0]; Y[m] = q[1]; Z[m] = q[2];
                    for (int a = 0; a < 3; a++)
                        for (int b = 0; b < 3; b++) {
                            const int k = ((o * 8 + m) * 3 + a) * 3 + b;
                            got[a] += (c1 * T.E1[k] + c2 * T.E2[k]) * q[b];
                        }
                }
                hq_element_force(X, Y, Z, c1, c2);
                ref[0] += X[o]; ref[1] += Y[o]; ref[2] += Z[o];
            }
            for (int a = 0; a < 3; a++)
                if (fabs(got[a] - ref[a]) > 1e-12 * (fabs(ref[a]) + 1.0)) bad++;
        }
    }
    report[0] = (int64_t)H.desc.size(); report[1] = ntab; report[2] = nfull; report[3] = nbnd_tot; report[4] = ncorner;
    report[5] = bad;
    if (bad) return hq_fail(HQ_ERR_STATE, "stencil table self-check failed%s", "");
    return HQ_OK;
}

/*
 * Host-only self-check of the brick planner (needs no device; desc->node_xyz required).  Takes hq_create's own plan
 * (hq_prepare: the bricks, and the description renumbered behind them) and verifies, against the mesh's connectivity alone (node -> elements, no coordinates): the
 * numbering is a permutation; every brick node lies in exactly one unit, is the corner of exactly eight elements
 * (one per corner) with the unit's (c1, c2, beta), has an n_t row without dashpot terms (the unit's row where the
 * unit says they are all the same), is neither hanging, an anchor, nor named in a schedule; and each of its 26
 * neighbours -- found through those eight elements -- is the node the kernel will read at that offset: a node of
 * the unit, an entry of the unit's ring table or of its first / last plane's id list.
 * report = {brick nodes, tile columns, units, units with one n_t row, levels, neighbours checked, patch nodes, faults,
 *           ragged units (HQ_BK_RAGGED), the nodes they own, ragged HET units, the nodes they own,
 *           HET units in the packed form (HQ_BK_PACKED), ragged ones included,
 *           the smallest nx, ny and np of any unit, the fewest nodes a ragged unit (of either kernel) owns in one of its
 *           planes (0: no ragged unit), units of ONE plane that carry both z faces}
 */
#define HQ_BRICK_REPORT_N 18
static int hq_brick_plan_check_impl(const hq_desc* d, int64_t report[HQ_BRICK_REPORT_N])
{
    hq_options opts;                                  /* host-only diagnostic: the library defaults, the environment where HQ_ALLOW_ENV=1 */
    hq_options_resolve(&opts, nullptr);
    for (int k = 0; k < HQ_BRICK_REPORT_N; k++) report[k] = 0;
    if (!d || !d->node_xyz || !d->eTable || !d->nTable)
        return hq_fail(HQ_ERR_ARG, "inconsistent mesh description (node_xyz is needed)%s", "");
    hq_prep prep;
    HQ_TRY(hq_prepare(d, opts, HQ_PREP_BRICKS, &prep));
    const int64_t E = d->lenum, N = d->nharbored;
    const hq_brick_host& B = prep.bricks;
    const std::vector<int32_t>& perm = prep.perm;     /* d (the caller's numbering) -> prep.desc, prep.ntab (the device's) */
    const std::vector<double>&c1 = prep.c1, &c2 = prep.c2, &beta = prep.beta;
    const std::vector<char>& excl = prep.excl;        /* (the caller's numbering) */
    int64_t bad = 0, nchecked = 0;
    report[6] = N;
    if (B.nb == 0) return HQ_OK;
    /* permutation and its inverse */
    std::vector<int32_t> inv((size_t)N, -1);
    for (int64_t n = 0; n < N; n++) {
        const int32_t q = perm[(size_t)n];
        if (q < 0 || q >= N || inv[(size_t)q] != -1) { bad++; continue; }
        inv[(size_t)q] = (int32_t)n;
    }
    /* node -> (element, corner) */
    std::vector<int64_t> aptr((size_t)N + 1, 0);
    for (int64_t i = 0; i < E * 8; i++) aptr[(size_t)d->lnid[i] + 1]++;
    for (int64_t n = 0; n < N; n++) aptr[(size_t)n + 1] += aptr[(size_t)n];
    std::vector<int64_t> adj((size_t)(E * 8));
    {
        std::vector<int64_t> fill(aptr.begin(), aptr.end() - 1);
        for (int64_t i = 0; i < E * 8; i++) adj[(size_t)fill[(size_t)d->lnid[i]]++] = i;
    }
    /* the device id the kernel reads at (x, y) of plane k of unit U, k = -1 .. np */
    auto at = [&](const hq_brick_unit& U, int x, int y, int k) -> int64_t {
        const int nx = U.nx, ny = U.ny, np = U.np, nr = 2 * (nx + 2) + 2 * ny;
        const int32_t* ring = B.tab.data() + U.tab;
        const int32_t* cap = ring + (int64_t)(np + 2) * nr;
        const bool in = x >= 0 && x < nx && y >= 0 && y < ny;
        if (in && (U.flags & HQ_BK_RAGGED)) {    /* the plane table: owned ids as they are, the others as -id - 2 */
            const int32_t v = cap[(int64_t)(k + 1) * nx * ny + y * nx + x];
            return v >= 0 ? v : (v == -1 ? -1 : -(int64_t)v - 2);
        }
        if (in) {
            if (k >= 0 && k < np) return U.base + ((int64_t)k * ny + y) * nx + x;
            return cap[(k < 0 ? 0 : nx * ny) + y * nx + x];
        }
        const int32_t* r = ring + (int64_t)(k + 1) * nr;
        if (y == -1) return r[x + 1];
        if (y == ny) return r[nx + 2 + x + 1];
        if (x == -1) return r[2 * (nx + 2) + y];
        return r[2 * (nx + 2) + ny + y];
    };
    std::vector<int32_t> covered((size_t)B.nb, 0);
    int64_t nsame = 0;
#pragma omp parallel for schedule(dynamic, 4) reduction(+ : bad, nchecked, nsame)
    for (int64_t u = 0; u < (int64_t)B.units.size(); u++) {
        const hq_brick_unit& U = B.units[(size_t)u];
        const int nx = U.nx, ny = U.ny, np = U.np, nr = 2 * (nx + 2) + 2 * ny;
        const bool het = (U.flags & HQ_BK_HET) != 0, rag = (U.flags & HQ_BK_RAGGED) != 0;
        if (nx < 1 || nx > (het ? HQ_BH_TX : HQ_BK_TX) || ny < 1 || ny > (het ? HQ_BH_TY : HQ_BK_TY) || np < 1 || U.base < 0 ||
            (!rag && U.base + (int64_t)nx * ny * np > B.nb)) { bad++; continue; }
        nsame += (U.flags & HQ_BK_NTSAME) != 0;
        if (((U.flags & HQ_BK_NTSAME) != 0) != (u < B.nsame)) bad++;
        /* the launch order: one n_t row | ragged (one row) | per-node rows | HET | HET packed | ragged HET | ragged HET packed */
        const int64_t nu = (int64_t)B.units.size();
        if ((rag && !het) != (u >= B.nsame - B.nrag && u < B.nsame) || (rag && (U.flags & (HQ_BK_TOPFACE | HQ_BK_BOTFACE)))) { bad++; continue; }
        if ((rag && het) != (u >= nu - B.nrhet)) { bad++; continue; }
        if (het != (u >= nu - B.nhet - B.nrhet)) bad++;
        if (het && ((U.flags & HQ_BK_PACKED) != 0) != (rag ? u >= nu - B.nrpacked : (u >= nu - B.nrhet - B.npacked && u < nu - B.nrhet))) bad++;
        if (het && (U.coef < 0 || U.coef + (int64_t)(np + 1) * HQ_BH_THREADS * 3 > (int64_t)B.coef.size())) { bad++; continue; }
        const int32_t* cap = B.tab.data() + U.tab + (int64_t)(np + 2) * nr;
        int64_t next = U.base;               /* a ragged unit numbers what it owns plane by plane without gaps */
        for (int k = 0; k < np; k++)
            for (int y = 0; y < ny; y++)
                for (int x = 0; x < nx; x++) {
                    int64_t q = U.base + ((int64_t)k * ny + y) * nx + x;
                    if (rag) {
                        const int32_t v = cap[(int64_t)(k + 1) * nx * ny + y * nx + x];
                        if (v < 0) continue;
                        if (v != next++ || v >= B.nb) { bad++; continue; }
                        q = v;
                    }
#pragma omp atomic
                    covered[(size_t)q]++;
                    const int32_t n = inv[(size_t)q];
                    if (n < 0) { bad++; continue; }
                    if (excl[(size_t)n]) bad++;
                    const double* t7 = prep.ntab + 7 * q;
                    if (!((t7[1] == t7[2]) && (t7[1] == t7[3]) && (t7[4] == t7[5]) && (t7[4] == t7[6]))) bad++;
                    if ((U.flags & HQ_BK_NTSAME) && (t7[0] != U.m0 || t7[1] != U.m2 || t7[4] != U.m1)) bad++;
                    int64_t el[8];
                    for (int o = 0; o < 8; o++) el[o] = -1;
                    if (aptr[(size_t)n + 1] - aptr[(size_t)n] != 8) { bad++; continue; }
                    bool ok = true;
                    for (int64_t a = aptr[(size_t)n]; a < aptr[(size_t)n + 1]; a++) {
                        const int64_t e = adj[(size_t)a] >> 3;
                        const int o = (int)(adj[(size_t)a] & 7);
                        if (el[o] != -1) ok = false;
                        el[o] = e;
                        if (het) {
                            /* the element whose corner o the node is: column (x - ox + 1, y - oy + 1) of layer k - oz + 1 */
                            const int i = x - (o & 1) + 1, j = y - ((o >> 1) & 1) + 1, l = k - ((o >> 2) & 1) + 1;
                            const double* q = B.coef.data() + U.coef + (int64_t)l * (3 * HQ_BH_THREADS) + (j * 64 + i);
                            if (c1[(size_t)e] != q[0] || c2[(size_t)e] != q[HQ_BH_CS] || beta[(size_t)e] != q[2 * HQ_BH_CS]) ok = false;
                        } else if (c1[(size_t)e] != U.c1 || c2[(size_t)e] != U.c2 || beta[(size_t)e] != U.beta) ok = false;
                    }
                    if (!ok) { bad++; continue; }
                    for (int dz = -1; dz <= 1; dz++)
                        for (int dy = -1; dy <= 1; dy++)
                            for (int dx = -1; dx <= 1; dx++) {
                                if (!dx && !dy && !dz) continue;
                                /* the neighbour is corner m of the element whose corner o the node is, m - o = d */
                                const int o = (dx < 0 ? 1 : 0) | (dy < 0 ? 2 : 0) | (dz < 0 ? 4 : 0);
                                const int m = (dx > 0 ? 1 : 0) | (dy > 0 ? 2 : 0) | (dz > 0 ? 4 : 0);
                                const int32_t nb_abi = d->lnid[8 * el[o] + m];
                                if (at(U, x + dx, y + dy, k + dz) != (int64_t)perm[(size_t)nb_abi]) bad++;
                                nchecked++;
                            }
                }
    }
    /* face planes (HQ_BK_TOPFACE / BOTFACE): every node of the plane is the corner of exactly FOUR elements, all on the
     * unit's side, with the unit's coefficients; its n_t row is the one in the unit's record; the kernel finds it in the
     * cap table and its 17 neighbours where it reads them */
#pragma omp parallel for schedule(dynamic, 4) reduction(+ : bad, nchecked)
    for (int64_t u = 0; u < (int64_t)B.units.size(); u++) {
        const hq_brick_unit& U = B.units[(size_t)u];
        const int nx = U.nx, ny = U.ny, np = U.np;
        if (!(U.flags & (HQ_BK_TOPFACE | HQ_BK_BOTFACE))) continue;
        if ((U.flags & HQ_BK_HET) || !(U.flags & HQ_BK_NTSAME)) { bad++; continue; }
        if (U.flags & HQ_BK_RAGGED) continue;            /* (a fault of the loop above: a ragged unit carries no face) */
        for (int side = 0; side < 2; side++) {
            if (!(U.flags & (side ? HQ_BK_BOTFACE : HQ_BK_TOPFACE))) continue;
            const double* row = side ? U.fb : U.ft;
            const int kf = side ? np : -1;
            for (int y = 0; y < ny; y++)
                for (int x = 0; x < nx; x++) {
                    const int64_t q = U.base + ((int64_t)(side ? np : -1) * ny + y) * nx + x;
                    if (q < 0 || q >= B.nb) { bad++; continue; }
#pragma omp atomic
                    covered[(size_t)q]++;
                    if (at(U, x, y, kf) != q) bad++;
                    const int32_t n = inv[(size_t)q];
                    if (n < 0) { bad++; continue; }
                    if (excl[(size_t)n]) bad++;
                    if (memcmp(prep.ntab + 7 * q, row, 7 * sizeof(double)) != 0) bad++;
                    int64_t el[8];
                    for (int o = 0; o < 8; o++) el[o] = -1;
                    if (aptr[(size_t)n + 1] - aptr[(size_t)n] != 4) { bad++; continue; }
                    bool ok = true;
                    for (int64_t a = aptr[(size_t)n]; a < aptr[(size_t)n + 1]; a++) {
                        const int64_t e = adj[(size_t)a] >> 3;
                        const int o = (int)(adj[(size_t)a] & 7);
                        if (((o >> 2) & 1) != side || el[o] != -1) ok = false;     /* top: the node is the elements' low-z corner */
                        el[o] = e;
                        if (c1[(size_t)e] != U.c1 || c2[(size_t)e] != U.c2 || beta[(size_t)e] != U.beta) ok = false;
                    }
                    if (!ok) { bad++; continue; }
                    for (int dz = (side ? -1 : 0); dz <= (side ? 0 : 1); dz++)
                        for (int dy = -1; dy <= 1; dy++)
                            for (int dx = -1; dx <= 1; dx++) {
                                if (!dx && !dy && !dz) continue;
                                const int o = (dx < 0 ? 1 : 0) | (dy < 0 ? 2 : 0) | (side ? 4 : 0);
                                const int m = (dx > 0 ? 1 : 0) | (dy > 0 ? 2 : 0) | ((side ? dz == 0 : dz > 0) ? 4 : 0);
                                const int32_t nb_abi = d->lnid[8 * el[o] + m];
                                if (at(U, x + dx, y + dy, kf + dz) != (int64_t)perm[(size_t)nb_abi]) bad++;
                                nchecked++;
                            }
                }
        }
    }
    for (int64_t q = 0; q < B.nb; q++) if (covered[(size_t)q] != 1) bad++;
    /* the patches behind the bricks: planned on hq_prepare's renumbered description as hq_create does it -- walking only the elements
     * of the shell (hq_patch_candidates) -- and once more walking every element: the two plans must be the same, and
     * every element around a patch node must be in its patch */
    {
        const int32_t *p_lnid = prep.desc.lnid, *p_xyz = prep.desc.node_xyz;
        const hq_dangling& dn = prep.dn;
        bool want_lattice = false;                   /* (not asked for: behind bricks the shell is planned without) */
        const hq_patch_cfg cfg = hq_patch_cfg_of(opts, dn.n > 0, true, &want_lattice);
        if (const char* why = hq_patch_cfg_refusal(cfg)) return hq_fail(HQ_ERR_ARG, "patch plan: %s", why);
        hq_patch_host Ha, Hb;
        std::vector<int32_t> all((size_t)E);
        for (int64_t e = 0; e < E; e++) all[(size_t)e] = (int32_t)e;
        if (hq_patch_plan_host(opts, cfg, E, N, p_lnid, p_xyz, dn, false, &Ha, B.nb) != 0 ||
            hq_patch_plan_host(opts, cfg, E, N, p_lnid, p_xyz, dn, false, &Hb, B.nb, &all) != 0)
            return hq_fail(HQ_ERR_ARG, "patch plan: %s", hq_patch_error());
        if (Ha.pelem != Hb.pelem || Ha.halo != Hb.halo || Ha.pidx != Hb.pidx || Ha.desc.size() != Hb.desc.size() || Ha.ds_ent != Hb.ds_ent) bad++;
        for (size_t q = 0; q < Ha.desc.size() && q < Hb.desc.size(); q++)
            if (Ha.desc[q].base != Hb.desc[q].base || Ha.desc[q].nown != Hb.desc[q].nown || Ha.desc[q].npairs != Hb.desc[q].npairs ||
                Ha.desc[q].nhalo != Hb.desc[q].nhalo || Ha.desc[q].pair_off != Hb.desc[q].pair_off) bad++;
        /* every (element, patch node) incidence is in the owner's list */
        std::vector<int32_t> patch_of((size_t)N, -1);
        for (size_t q = 0; q < Ha.desc.size(); q++)
            for (int32_t n = Ha.desc[q].base; n < Ha.desc[q].base + Ha.desc[q].nown; n++) patch_of[(size_t)n] = (int32_t)q;
        for (int64_t n = B.nb; n < N; n++) if (patch_of[(size_t)n] < 0) bad++;
        int64_t need = 0, have = 0;
        for (int64_t e = 0; e < E; e++) {
            int32_t seen[8]; int ns = 0;
            for (int c8 = 0; c8 < 8; c8++) {
                const int32_t q = patch_of[(size_t)p_lnid[8 * e + c8]];
                bool dup = q < 0;
                for (int t = 0; t < ns; t++) dup |= seen[t] == q;
                if (!dup) seen[ns++] = q;
            }
            for (int t = 0; t < ns; t++) {
                need++;
                const hq_patch_desc& D = Ha.desc[(size_t)seen[t]];
                have += std::binary_search(Ha.pelem.begin() + D.pair_off, Ha.pelem.begin() + D.pair_off + D.npairs, (int32_t)e);
            }
        }
        if (have != need) bad++;
    }
    report[0] = B.nb; report[1] = B.ncolumns; report[2] = (int64_t)B.units.size(); report[3] = nsame;
    report[4] = B.nhet + B.nrhet; report[5] = nchecked; report[6] = N - B.nb; report[7] = bad;
    report[8] = B.nrag; report[10] = B.nrhet; report[12] = B.npacked + B.nrpacked;
    report[13] = report[14] = report[15] = INT64_MAX;
    for (const hq_brick_unit& U : B.units) {
        report[13] = std::min<int64_t>(report[13], U.nx); report[14] = std::min<int64_t>(report[14], U.ny);
        report[15] = std::min<int64_t>(report[15], U.np);
        report[17] += U.np == 1 && (U.flags & HQ_BK_TOPFACE) && (U.flags & HQ_BK_BOTFACE);
        if (!(U.flags & HQ_BK_RAGGED)) continue;
        const int64_t nxy = (int64_t)U.nx * U.ny;
        const int32_t* pl = B.tab.data() + U.tab + (int64_t)(U.np + 2) * (2 * (U.nx + 2) + 2 * U.ny);
        for (int64_t k = 1; k <= U.np; k++) {            /* (planes 0 and np + 1 of the table are the caps: never owned) */
            int64_t own = 0;
            for (int64_t i = k * nxy; i < (k + 1) * nxy; i++) own += pl[i] >= 0;
            report[(U.flags & HQ_BK_HET) ? 11 : 9] += own;
            report[16] = report[16] ? std::min(report[16], own) : own;
        }
    }
    if (bad) return hq_fail(HQ_ERR_STATE, "brick plan self-check failed%s", "");
    return HQ_OK;
}

extern "C" int hq_brick_plan_check(const hq_desc* d, int64_t report[8]) { return hq_brick_plan_check_n(d, report, 8); }

/* the same with a longer report (entries 8 .. 17 above); n = entries the caller has, those past 18 are zeroed */
extern "C" int hq_brick_plan_check_n(const hq_desc* d, int64_t* report, int32_t n)
{
    int64_t r[HQ_BRICK_REPORT_N];
    if (!report || n < 8) return hq_fail(HQ_ERR_ARG, "hq_brick_plan_check_n: a report of at least 8 entries%s", "");
    const int rc = hq_brick_plan_check_impl(d, r);
    for (int k = 0; k < n; k++) report[k] = k < HQ_BRICK_REPORT_N ? r[k] : 0;
    return rc;
}

#endif
