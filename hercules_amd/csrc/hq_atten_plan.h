/* hq_atten_plan.h -- the slot plan of BKT attenuation (hq_atten.h), host only: which (node, class) pairs a partition keeps
 * memory variables for and which slot every element corner reads.  No device, no HIP call: hq_attenuation_set uploads what
 * it leaves and hq_attenuation_plan_check begins with the same call, so what is checked is what runs.
 *
 *   class   one distinct row of ten floats (bitwise), numbered in the order of first appearance in the element table
 *   slot    one (harbored node, class) pair that some element corner names; sorted node-major, so consecutive slots read
 *           consecutive nodes (in a uniform region: slot == rank of the node)
 *   eslot   [8][Epad] the slot of corner i of element e, SoA like d_lnid
 * Hanging and shared nodes are nodes like any other: u is assigned / shared to them every step, so every rank advances the
 * slots of the nodes it harbors from values that are the same on every rank.
 *
 * Included by hq_engine.hip (one translation unit): uses its hq_fail. */
#ifndef HQ_ATTEN_PLAN_H
#define HQ_ATTEN_PLAN_H

#include <cmath>
#include <map>

struct hq_atten_plan {
    int32_t nclasses = 0, nslots = 0;
    int64_t Epad = 0;
    std::vector<float> rows;                 /* [nclasses][10] */
    std::vector<int32_t> eclass;             /* [E] */
    std::vector<int32_t> eslot;              /* [8][Epad] (padding: slot 0) */
    std::vector<int32_t> slot_node, slot_class;
};

/* the device bytes an attenuated context adds: 12 + 6 double rows per slot, eslot, the slots' node and class, the classes' doubles */
static int64_t hq_atten_bytes(int64_t nslots, int64_t Epad, int64_t nclasses)
{
    return 144 * nslots + 32 * Epad + 8 * nslots + 8 * HQ_ATTEN_NCOEF * nclasses;
}

/* lnid [E][8] (AoS) or, with soa_stride > 0, [8][soa_stride]; coef [E][10] */
static int hq_atten_plan_build(int64_t E, int64_t N, const int32_t* lnid, int64_t soa_stride, const float* coef, hq_atten_plan* P)
{
    if (E <= 0 || N <= 0 || !lnid || !coef) return hq_fail(HQ_ERR_ARG, "attenuation: no elements or no coefficients%s", "");
    for (int64_t i = 0; i < E * HQ_ATTEN_NROW; i++)
        if (!std::isfinite(coef[i])) return hq_fail(HQ_ERR_ARG, "attenuation: a coefficient is not finite%s", "");
    auto node_of = [&](int64_t e, int i) { return soa_stride > 0 ? lnid[(int64_t)i * soa_stride + e] : lnid[8 * e + i]; };
    struct row_t {
        uint32_t w[HQ_ATTEN_NROW];
        bool operator<(const row_t& o) const { return memcmp(w, o.w, sizeof w) < 0; }
    };
    std::map<row_t, int32_t> seen;
    P->eclass.resize((size_t)E);
    P->rows.clear();
    for (int64_t e = 0; e < E; e++) {
        row_t r;
        memcpy(r.w, coef + HQ_ATTEN_NROW * e, sizeof r.w);
        auto it = seen.find(r);
        if (it == seen.end()) {
            it = seen.emplace(r, (int32_t)seen.size()).first;
            P->rows.insert(P->rows.end(), coef + HQ_ATTEN_NROW * e, coef + HQ_ATTEN_NROW * (e + 1));
        }
        P->eclass[(size_t)e] = it->second;
    }
    const int64_t nc = (int64_t)seen.size();
    P->nclasses = (int32_t)nc;
    std::vector<int64_t> key((size_t)E * 8);
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < E; e++)
        for (int i = 0; i < 8; i++) key[(size_t)(8 * e + i)] = (int64_t)node_of(e, i) * nc + P->eclass[(size_t)e];
    std::vector<int64_t> slots(key);
    std::sort(slots.begin(), slots.end());
    slots.erase(std::unique(slots.begin(), slots.end()), slots.end());
    if (slots.size() > (size_t)0x7fffffff) return hq_fail(HQ_ERR_ARG, "attenuation: more than 2^31 - 1 (node, class) slots%s", "");
    P->nslots = (int32_t)slots.size();
    P->slot_node.resize(slots.size());
    P->slot_class.resize(slots.size());
    for (size_t s = 0; s < slots.size(); s++) {
        P->slot_node[s] = (int32_t)(slots[s] / nc);
        P->slot_class[s] = (int32_t)(slots[s] % nc);
    }
    P->Epad = (E + 63) & ~(int64_t)63;
    P->eslot.assign((size_t)(8 * P->Epad), 0);
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < E; e++)
        for (int i = 0; i < 8; i++)
            P->eslot[(size_t)(i * P->Epad + e)] =
                (int32_t)(std::lower_bound(slots.begin(), slots.end(), key[(size_t)(8 * e + i)]) - slots.begin());
    return HQ_OK;
}

/* what must hold of a plan, counted: corners whose slot is not (their node, their class), slots out of node-major order */
static int64_t hq_atten_plan_faults(int64_t E, const int32_t* lnid, const hq_atten_plan& P)
{
    int64_t bad = 0;
    for (int64_t e = 0; e < E; e++)
        for (int i = 0; i < 8; i++) {
            const int32_t s = P.eslot[(size_t)(i * P.Epad + e)];
            if (s < 0 || s >= P.nslots || P.slot_node[(size_t)s] != lnid[8 * e + i] || P.slot_class[(size_t)s] != P.eclass[(size_t)e]) bad++;
        }
    for (int32_t s = 1; s < P.nslots; s++) {
        const bool ordered = P.slot_node[(size_t)s] > P.slot_node[(size_t)s - 1] ||
                             (P.slot_node[(size_t)s] == P.slot_node[(size_t)s - 1] && P.slot_class[(size_t)s] > P.slot_class[(size_t)s - 1]);
        if (!ordered) bad++;
    }
    return bad;
}

#endif /* HQ_ATTEN_PLAN_H */
