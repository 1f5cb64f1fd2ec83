// Many Lagrange-form polynomials opened in one call, each at its OWN point (bbg_open_points): for k < count, with n = 2^log2n,
// w the domain's root, f_i = F_k(w^i), z = z_k and d_i = z w^-i - 1,
//   y   = F_k(z)  = (z^n - 1)/n * sum_i f_i / d_i                       (z off the domain)
//   q_i = W(w^i)  = w^-i (y - f_i) / d_i,   W(X) = (F_k(X) - y) / (X - z)
//   proof_k = sum_i q_i LB_i                                            over the Lagrange-form string LB
// A point ON the domain, z = w^m, is answered exactly and per polynomial: y = f_m, the q_i of i != m as above, and because W has degree
// n - 2 its top coefficient n^-1 sum_i w^i q_i vanishes, which leaves
//   q_m = - w^-m sum_(i != m) (f_m - f_i) / d_i = - w^-m ( f_m S0 - S1 ),   S0 = sum_(i != m) 1 / d_i,  S1 = sum_(i != m) f_i / d_i
// -- no derivative.  tests/tools/open_points_model.py proves the identity against coefficient-form division on integers.
//
// One launch per stage over ALL polynomials of a chunk (the block index is flattened: polynomial-major), everything on one stream:
//   k_op_weights    one block per inversion group (BARY_BLK points of one polynomial): d_i from the polynomial's own z_k (device memory),
//                   block_invert, u_i = w^-i / d_i to the workspace (not for an evaluation), the group's S1 and S0 to the partials, the index
//                   of a zero d_i through atomicMin(flag + k, i).  The hit itself takes no part in the inversion and in neither sum.
//   k_op_value      one block per polynomial: z_k^n by log2n squarings, the sums of its partials; y_k = (z_k^n - 1)/n S1, or on a hit
//                   y_k = f_m and q_m from S0 and S1 (the branch is uniform over the block), both canonical.
//   k_op_quotient   q_i = (y_k - f_i) u_i in place, canonical; the hit slot takes q_m.
//   the commitments msm_run_batch over the string, BBG_MSM_BATCH_MAX polynomials per launch set, Jacobian results in the workspace; msm_join
//   k_op_normalize  the chunk's results to canonical affine, four per thread behind one inversion (aff_batch_chunk4, curve.hip.h)
// This file holds the kernels, the workspace and the chunk walk; the argument checks are poly.hip's (open_points_check).
#include "bbg_internal.h"
#include "work_layouts.h"

#include "block_invert.hip.h"
#include "curve.hip.h"
#include "ntt_consts.hip.h"

namespace bbg {

struct OpArgs {
    const Fr* evals;  // [polys][n]
    const Fr* z;      // [polys]
    unsigned log2n;
    unsigned groups;  // inversion groups per polynomial: ceil(n / BARY_BLK)
    const DomainConsts* dc;
    Fr* u;            // [polys][n]: the weights, then the quotient values; null for an evaluation
    Fr* partials;     // [polys][groups][2]: S1, S0
    Fr* hitq;         // [polys]: q_m of a polynomial with a hit
    unsigned* flag;   // [polys]: m, or BARY_NO_HIT
    Fr* y;            // [polys]: the caller's output
};

__global__ void __launch_bounds__(256) k_op_weights(OpArgs a)
{
    __shared__ Fr pre[256], suf[256];
    __shared__ Fr inv_total;
    __shared__ Fr sm[8];
    const int tid = threadIdx.x;
    const size_t n = (size_t)1 << a.log2n;
    const size_t k = blockIdx.x / a.groups;
    const size_t base = (size_t)(blockIdx.x % a.groups) * BARY_BLK;
    const Fr* __restrict__ f = a.evals + k * n;
    const Fr z = fe_reduce_once(fe_load<FrP>(a.z + k));
    Fr xe = pow_from_table(a.dc->pow2_root_inv, (uint64_t)base + tid); // w^-i of the thread's first point
    const Fr step256 = a.dc->pow2_root_inv[8];
    Fr v[BI_E], wi[BI_E];
    bool live[BI_E]; // inside the array and not the hit
#pragma unroll
    for (int e = 0; e < BI_E; e++) {
        const size_t i = base + (size_t)e * 256 + tid;
        wi[e] = xe;
        v[e] = Fr::one();
        live[e] = false;
        if (i < n) {
            const Fr d = fe_reduce_once(fe_sub(fe_mul(z, xe), Fr::one())); // z w^-i - 1, canonical
            if (d.is_zero_raw()) atomicMin(a.flag + k, (unsigned)i);       // z = w^i: answered from the values (k_op_value)
            else {
                v[e] = d;
                live[e] = true;
            }
        }
        xe = fe_mul(xe, step256);
    }
    block_invert(v, pre, suf, &inv_total);
    Fr s1 = Fr::zero(), s0 = Fr::zero();
#pragma unroll
    for (int e = 0; e < BI_E; e++) {
        const size_t i = base + (size_t)e * 256 + tid;
        if (i < n && a.u) fe_store<FrP>(a.u + k * n + i, fe_mul(wi[e], v[e])); // (the hit's slot holds w^-m: k_op_quotient replaces it)
        if (live[e]) {
            s1 = fe_add(s1, fe_mul(fe_load<FrP>(f + i), v[e]));
            s0 = fe_add(s0, v[e]);
        }
    }
    s1 = wave_sum(s1);
    s0 = wave_sum(s0);
    if ((tid & 63) == 0) {
        sm[tid >> 6] = s1;
        sm[4 + (tid >> 6)] = s0;
    }
    __syncthreads();
    if (tid < 2) {
        const Fr* p = sm + 4 * tid;
        fe_store<FrP>(a.partials + (size_t)blockIdx.x * 2 + tid, fe_add(fe_add(p[0], p[1]), fe_add(p[2], p[3])));
    }
}

__global__ void __launch_bounds__(256) k_op_value(OpArgs a)
{
    __shared__ Fr sm[8];
    const int tid = threadIdx.x;
    const size_t k = blockIdx.x;
    const size_t n = (size_t)1 << a.log2n;
    const Fr* part = a.partials + k * a.groups * 2;
    Fr s1 = Fr::zero(), s0 = Fr::zero();
    for (unsigned g = tid; g < a.groups; g += 256) {
        s1 = fe_add(s1, fe_load<FrP>(part + 2 * (size_t)g));
        s0 = fe_add(s0, fe_load<FrP>(part + 2 * (size_t)g + 1));
    }
    s1 = wave_sum(s1);
    s0 = wave_sum(s0);
    if ((tid & 63) == 0) {
        sm[tid >> 6] = s1;
        sm[4 + (tid >> 6)] = s0;
    }
    __syncthreads();
    if (tid != 0) return;
    s1 = fe_add(fe_add(sm[0], sm[1]), fe_add(sm[2], sm[3]));
    s0 = fe_add(fe_add(sm[4], sm[5]), fe_add(sm[6], sm[7]));
    const unsigned hit = a.flag[k];
    if (hit != BARY_NO_HIT) {
        const Fr fm = fe_reduce_once(fe_load<FrP>(a.evals + k * n + hit));
        const Fr w = pow_from_table(a.dc->pow2_root_inv, (uint64_t)hit);
        fe_store<FrP>(a.y + k, fm);
        fe_store<FrP>(a.hitq + k, fe_reduce_once(fe_mul(w, fe_sub(s1, fe_mul(fm, s0))))); // - w^-m (f_m S0 - S1)
        return;
    }
    Fr zn = fe_load<FrP>(a.z + k);
    for (unsigned b = 0; b < a.log2n; b++) zn = fe_sqr(zn);
    const Fr scale = fe_mul(fe_sub(zn, Fr::one()), a.dc->n_inv);
    fe_store<FrP>(a.y + k, fe_reduce_once(fe_mul(s1, scale)));
}

// u[k n + i] <- (y_k - f_i) u[k n + i], canonical, over the `total` = polys x n values of the chunk; the hit slot of polynomial k takes hitq[k]
__global__ void __launch_bounds__(256) k_op_quotient(OpArgs a, size_t total)
{
    const size_t mask = ((size_t)1 << a.log2n) - 1;
    for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < total; j += (size_t)gridDim.x * 256) {
        const size_t k = j >> a.log2n;
        const Fr y = fe_load<FrP>(a.y + k);
        Fr q = fe_reduce_once(fe_mul(fe_sub(y, fe_load<FrP>(a.evals + j)), fe_load<FrP>(a.u + j)));
        if (a.flag[k] == (unsigned)(j & mask)) q = fe_load<FrP>(a.hitq + k);
        fe_store<FrP>(a.u + j, q);
    }
}

// out[i] = the MSM's Jacobian result i as canonical affine, i < count; a thread converts four behind one inversion
__global__ void __launch_bounds__(64) k_op_normalize(const Jacobian* __restrict__ jac, size_t count, Affine* out)
{
    const size_t i0 = ((size_t)blockIdx.x * 64 + threadIdx.x) * 4;
    if (i0 >= count) return;
    const int cnt = count - i0 < 4 ? (int)(count - i0) : 4;
    aff_batch_chunk4(out + i0, cnt, [&](int e) __attribute__((always_inline)) {
        Jacobian j;
        j.x = fe_load<FqP>(&jac[i0 + e].x);
        j.y = fe_load<FqP>(&jac[i0 + e].y);
        j.z = fe_load<FqP>(&jac[i0 + e].z);
        return xyzz_from_jacobian(j);
    });
}

// the workspace of one polynomial: op_layout (work_layouts.h) at a chunk of one, which is the formula bbg.h states
size_t open_points_poly_bytes(unsigned log2n, bool proofs) { return op_layout(log2n, proofs, 1, BARY_BLK).lay.total(); }
size_t open_points_chunk(const bbg_ctx* ctx, unsigned log2n, bool proofs, size_t count)
{
    size_t c = (size_t)ctx->open_points_budget / open_points_poly_bytes(log2n, proofs);
    if (c >= BBG_MSM_BATCH_MAX) c = c / BBG_MSM_BATCH_MAX * BBG_MSM_BATCH_MAX; // whole launch sets of the MSM
    return std::min(std::max<size_t>(c, 1), count);                            // (one polynomial may be larger than the budget)
}

int open_points_run(bbg_ctx* ctx, bbg_srs* lagrange, unsigned log2n, const void* d_evals, const void* d_z, size_t count, void* d_y, void* d_proofs,
                    hipStream_t st)
{
    const size_t n = (size_t)1 << log2n, groups = (n + BARY_BLK - 1) / BARY_BLK;
    const bool proofs = d_proofs != nullptr;
    void* dc = nullptr;
    if (int rc = ntt_domain_consts(ctx, log2n, &dc)) return rc;
    const size_t chunk = open_points_chunk(ctx, log2n, proofs, count);
    const OpLayout L = op_layout(log2n, proofs, chunk, BARY_BLK);
    if (int rc = ensure_layout(ctx->open_points_work, L.lay, "bbg_open_points_device")) return rc;
    void* ws = ctx->open_points_work.p;
    OpArgs a;
    a.log2n = log2n;
    a.groups = (unsigned)groups;
    a.dc = (const DomainConsts*)dc;
    a.u = proofs ? at<Fr>(ws, L.u) : nullptr;
    a.partials = at<Fr>(ws, L.partials);
    a.hitq = at<Fr>(ws, L.hitq);
    Jacobian* jac = at<Jacobian>(ws, L.jac);
    a.flag = at<unsigned>(ws, L.flag);
    for (size_t done = 0; done < count; done += chunk) {
        const size_t c = std::min(chunk, count - done);
        a.evals = (const Fr*)d_evals + done * n;
        a.z = (const Fr*)d_z + done;
        a.y = (Fr*)d_y + done;
        {
            ProfScope ps(ctx, "open_points_weights", st);
            BBG_HIP(hipMemsetAsync(a.flag, 0xff, c * sizeof(unsigned), st)); // BARY_NO_HIT, on every call
            hipLaunchKernelGGL(k_op_weights, dim3((unsigned)(c * groups)), dim3(256), 0, st, a);
            hipLaunchKernelGGL(k_op_value, dim3((unsigned)c), dim3(256), 0, st, a);
        }
        if (!proofs) continue;
        {
            ProfScope ps(ctx, "open_points_quotient", st);
            const size_t total = c * n;
            hipLaunchKernelGGL(k_op_quotient, dim3((unsigned)std::min<size_t>((total + 255) / 256, 256 * 64)), dim3(256), 0, st, a, total);
        }
        BBG_HIP(hipGetLastError());
        for (size_t s = 0; s < c; s += BBG_MSM_BATCH_MAX) {
            const int sets = (int)std::min<size_t>(BBG_MSM_BATCH_MAX, c - s);
            const void* ptrs[BBG_MSM_BATCH_MAX];
            size_t from[BBG_MSM_BATCH_MAX], len[BBG_MSM_BATCH_MAX];
            for (int e = 0; e < sets; e++) {
                ptrs[e] = a.u + (s + e) * n;
                from[e] = 0;
                len[e] = n;
            }
            if (int rc = msm_run_batch(ctx, lagrange->s, sets, ptrs, from, len, jac + s, st)) return rc;
        }
        if (int rc = msm_join(ctx, st)) return rc;
        {
            ProfScope ps(ctx, "open_points_normalize", st);
            hipLaunchKernelGGL(k_op_normalize, dim3(grid_for((c + 3) / 4, 64)), dim3(64), 0, st, (const Jacobian*)jac, c, (Affine*)d_proofs + done);
        }
    }
    BBG_HIP(hipGetLastError());
    return BBG_OK;
}

} // namespace bbg
