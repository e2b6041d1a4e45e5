/* hq_nonlin_dev.h -- nonlinear soil beside the patch and brick step (hq_nonlinear_set): the plan and the pass's own kernel.
 *
 * hq_nonlin.h has the physics and why it may enter as a correction.  The pass is hq_correction.h's, over the nonlinear
 * elements and the nodes they touch ONLY -- a run with 5 % of its elements nonlinear pays for 5 %.  The pass's own:
 *   hq_k_nl_element        one thread per nonlinear element: gathers its 24 values of u(t), and for each of its eight points
 *                          reads the old plastic strain, adds the point's share to the 24 corner forces, advances the point
 *                          and writes it back; the corner forces go to ef [3][8][Enlpad]              (no atomics)
 * It reads u(t) only.  The correction's rows are the touched nodes, a list (hq_k_atten_apply_at): the nodes of the nonlinear
 * elements and the anchors of the hanging ones among them, in ascending device numbering; the tables are hq_split_plan's
 * (hq_split_plan_build, hq_split_plan_faults) over that sub-mesh: the elements renumbered 0 .. nel - 1 in the caller's
 * (ascending) order, the nodes by their place in the list.
 *
 * Traffic model per nonlinear element (docs/LABNOTES.md has the measurement): 896 B of state read and written, 192 B of
 * corner forces written and read again, 48 B of constants, 32 B of node ids, the gathered fields (192 B requested, 24 B from
 * HBM in a uniform region), the node table 32 + 4 B, and per touched node 24 B of dF written and read again, 12 + 8 + 24 +
 * 24 B of the apply: 1536 B per element where every element has a node of its own.
 * Included by hq_engine.hip (one translation unit) behind hq_correction.h: uses its hq_fail and hq_real. */
#ifndef HQ_NONLIN_DEV_H
#define HQ_NONLIN_DEV_H

#include "hq_nonlin.h"

struct hq_nl_plan {
    int64_t nel = 0, Enlpad = 0, nt = 0;
    std::vector<int32_t> tnode;              /* [nt] the touched nodes, device numbering, ascending                  */
    std::vector<int32_t> lnid;               /* [nel][8] the nonlinear elements on touched-node indices               */
    std::vector<int32_t> dn_id, dn_ptr, dn_anchor;   /* the touched hanging nodes, on touched-node indices            */
    hq_split_plan S;
};

/* the device bytes hq_nonlinear_set adds: state, constants and node ids per padded element, and the correction over the
 * nonlinear elements and the listed touched nodes */
static int64_t hq_nl_bytes(int64_t nel, int64_t Enlpad, int64_t nt, int64_t nanchors, int64_t npairs)
{
    if (nel == 0) return 0;
    return (448 + 48 + 32) * Enlpad + hq_correction_bytes(nel, Enlpad, nt, true, nanchors, npairs);
}

/* elems [nel] strictly ascending in 0 .. E - 1 (checked by the caller); lnid [E][8] and the hanging-node table in the
 * numbering the device uses */
static int hq_nl_plan_build(int64_t nel, const int32_t* elems, int64_t N, const int32_t* lnid, int32_t ndn, const int32_t* dn_id,
                            const int32_t* dn_ptr, const int32_t* dn_anchor, hq_nl_plan* P)
{
    P->nel = nel;
    P->Enlpad = (nel + 63) & ~(int64_t)63;
    std::vector<int32_t> place((size_t)N, -1);
    for (int64_t k = 0; k < nel; k++)
        for (int i = 0; i < 8; i++) place[(size_t)lnid[8 * (int64_t)elems[k] + i]] = 0;
    std::vector<int32_t> hang;                                     /* rows of the hanging-node table that are touched */
    for (int32_t k = 0; k < ndn; k++)
        if (place[(size_t)dn_id[k]] == 0) hang.push_back(k);
    for (int32_t k : hang)
        for (int32_t a = dn_ptr[k]; a < dn_ptr[k + 1]; a++) place[(size_t)dn_anchor[a]] = 0;
    P->tnode.clear();
    for (int64_t n = 0; n < N; n++)
        if (place[(size_t)n] == 0) { place[(size_t)n] = (int32_t)P->tnode.size(); P->tnode.push_back((int32_t)n); }
    P->nt = (int64_t)P->tnode.size();
    P->lnid.resize((size_t)(8 * nel));
    for (int64_t k = 0; k < nel; k++)
        for (int i = 0; i < 8; i++) P->lnid[(size_t)(8 * k + i)] = place[(size_t)lnid[8 * (int64_t)elems[k] + i]];
    P->dn_id.clear(); P->dn_anchor.clear(); P->dn_ptr.assign(1, 0);
    for (int32_t k : hang) {
        P->dn_id.push_back(place[(size_t)dn_id[k]]);
        for (int32_t a = dn_ptr[k]; a < dn_ptr[k + 1]; a++) P->dn_anchor.push_back(place[(size_t)dn_anchor[a]]);
        P->dn_ptr.push_back((int32_t)P->dn_anchor.size());
    }
    return hq_split_plan_build(nel, P->nt, P->Enlpad, P->lnid.data(), (int32_t)P->dn_id.size(), P->dn_id.data(), P->dn_ptr.data(),
                               P->dn_anchor.data(), &P->S);
}

/*
 * What must hold, counted: the touched nodes rise strictly inside 0 .. N - 1; every corner of a nonlinear element names the
 * touched node that IS its node; every touched node is a corner of a nonlinear element or an anchor of a touched hanging
 * node; the touched hanging nodes are the mesh's hanging nodes among the elements' nodes, with the mesh's anchors; and the
 * tables pass hq_split_plan_faults on the sub-mesh.
 */
static int64_t hq_nl_plan_faults(int64_t nel, const int32_t* elems, int64_t N, const int32_t* lnid, int32_t ndn, const int32_t* dn_id,
                                 const int32_t* dn_ptr, const int32_t* dn_anchor, const hq_nl_plan& P, const int32_t* epos,
                                 const int32_t* nptr, const int32_t* nent, const int32_t* sd, int64_t nsd)
{
    int64_t bad = 0;
    const int64_t nt = P.nt;
    if (P.nel != nel || (int64_t)P.tnode.size() != nt || (int64_t)P.lnid.size() != 8 * nel) return 1 + 8 * nel;
    for (int64_t t = 0; t < nt; t++)
        if (P.tnode[(size_t)t] < 0 || P.tnode[(size_t)t] >= N || (t && P.tnode[(size_t)t] <= P.tnode[(size_t)t - 1])) return 1 + 8 * nel;
    std::vector<char> used((size_t)nt, 0);
    for (int64_t k = 0; k < nel; k++)
        for (int i = 0; i < 8; i++) {
            const int32_t t = P.lnid[(size_t)(8 * k + i)];
            if (t < 0 || t >= nt) return 1 + 8 * nel;
            if (P.tnode[(size_t)t] != lnid[8 * (int64_t)elems[k] + i]) bad++;
            used[(size_t)t] = 1;
        }
    std::vector<int32_t> row((size_t)N, -1);
    for (int32_t k = 0; k < ndn; k++) row[(size_t)dn_id[k]] = k;
    int64_t want = 0;
    for (int64_t t = 0; t < nt; t++) want += used[(size_t)t] && row[(size_t)P.tnode[(size_t)t]] >= 0;
    if ((int64_t)P.dn_id.size() != want) bad++;
    for (size_t k = 0; k < P.dn_id.size(); k++) {
        const int32_t t = P.dn_id[k];
        if (t < 0 || t >= nt || !used[(size_t)t] || row[(size_t)P.tnode[(size_t)t]] < 0) { bad++; continue; }
        const int32_t r = row[(size_t)P.tnode[(size_t)t]];
        if (P.dn_ptr[k + 1] - P.dn_ptr[k] != dn_ptr[r + 1] - dn_ptr[r]) { bad++; continue; }
        for (int32_t a = 0; a < dn_ptr[r + 1] - dn_ptr[r]; a++) {
            const int32_t ta = P.dn_anchor[(size_t)(P.dn_ptr[k] + a)];
            if (ta < 0 || ta >= nt || P.tnode[(size_t)ta] != dn_anchor[dn_ptr[r] + a]) bad++;
            else used[(size_t)ta] = 1;
        }
    }
    for (int64_t t = 0; t < nt; t++) bad += !used[(size_t)t];
    if (bad) return bad;
    return hq_split_plan_faults(nel, nt, P.Enlpad, P.lnid.data(), (int32_t)P.dn_id.size(), P.dn_id.data(), P.dn_ptr.data(),
                                P.dn_anchor.data(), epos, nptr, nent, sd, nsd);
}

#if defined(__HIPCC__)
/*
 * One thread per nonlinear element, SoA rows of stride Enlpad: node ids [8], constants [6], state [7][8], corner forces
 * [3][8].  u(t) is gathered in the device's node numbering.  48 live doubles (24 values of u, 24 corner forces) plus a
 * point's temporaries: 218 registers, no scratch (docs/LABNOTES.md).
 */
__global__ void __launch_bounds__(256)
hq_k_nl_element(int32_t nel, int32_t Enlpad, const int32_t* __restrict__ lnid, const double* __restrict__ cons,
                const hq_real* __restrict__ u1, double dt2, double* __restrict__ st, double* __restrict__ ef)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nel) return;
    double u[24], f[24];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const hq_real* p = u1 + 3 * (int64_t)lnid[(int64_t)i * Enlpad + e];
        u[3 * i] = (double)p[0];
        u[3 * i + 1] = (double)p[1];
        u[3 * i + 2] = (double)p[2];
    }
    hq_nl_element(u, cons + e, Enlpad, dt2, st + e, Enlpad, f);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        double* o = ef + (int64_t)i * Enlpad + e;
        o[0] = f[3 * i];
        o[8 * (int64_t)Enlpad] = f[3 * i + 1];
        o[16 * (int64_t)Enlpad] = f[3 * i + 2];
    }
}
#endif /* __HIPCC__ */

#endif /* HQ_NONLIN_DEV_H */
