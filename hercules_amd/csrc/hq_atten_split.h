/* hq_atten_split.h -- BKT attenuation beside the patch and brick step (hq_attenuation_set_split): the pass's own kernels.
 *
 * Under BKT c3 = c4 = 0, so the patch and brick kernels apply mu K_mu + kappa K_kappa to u1 itself, and the BKT force
 * mu K_mu ws + kappa K_kappa wk with ws = u1 + ds, wk = u1 + dk (hq_atten.h) is that elastic force plus
 *     dF = mu K_mu ds + kappa K_kappa dk,
 * which enters as a correction pass (hq_correction.h: why it may, and the chain behind the corner forces) over all elements
 * and all nodes.  No step kernel, plan or launch of the elastic path changes.  The pass's own:
 *   hq_k_atten_advance_delta   one thread per (node, class) slot: the memory variables, and ds, dk into the rows w [6][nslots]
 *   hq_k_atten_corner_force    one thread per element: its 24 corner forces of (ds, dk) into ef [3][8][Epad]   (no atomics)
 * They read u(t) and u(t - dt) only.  The slot of every corner is kept on the host in the caller's element order, so
 * hq_attenuation_fetch / _load keep the reference's per-corner layout, while the device's tables follow an element order of
 * their own (hq_split_plan.epos).
 *
 * Traffic models (per element of a uniform region, one node and one slot per element; docs/LABNOTES.md has the measurements):
 *   two-pass (built)       advance 48 + 96 + 96 + 48 = 288 B per slot; corner force 32 (eslot) + 16 (c1, c2) + 192 written
 *                          + the 48 gathered doubles (384 B requested, ~48 B from HBM: neighbours share the rows); node sum 32
 *                          (entries) + 4 (ptr) + 192 read + 24 written; apply 24 + 24 + 24 + 8 = 80: 908 B per node
 *   one-pass node gather   no ef (saves 384 B) and no CSR, but every node repeats the butterflies of its eight elements: 8 x
 *                          the arithmetic and 8 x 48 gathered doubles per node, and a node on a level interface, with other
 *                          than eight elements around it, needs the same table as the two-pass form to find them
 * Included by hq_engine.hip (one translation unit) behind hq_correction.h: uses its hq_real and hq_element_force_bkt. */
#ifndef HQ_ATTEN_SPLIT_H
#define HQ_ATTEN_SPLIT_H

/* the device bytes a split context adds beyond hq_atten_bytes: c1 / c2, and the correction over all elements and all nodes */
static int64_t hq_split_bytes(int64_t E, int64_t Epad, int64_t N, int64_t nanchors, int64_t npairs)
{
    return 16 * E + hq_correction_bytes(E, Epad, N, false, nanchors, npairs);
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

#endif /* __HIPCC__ */

#endif /* HQ_ATTEN_SPLIT_H */
