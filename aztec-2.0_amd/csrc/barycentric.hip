// Lagrange-form (evaluation-basis) polynomial operations on device-resident arrays.  Reference:
//   fr::batch_invert                                   ecc/fields/field_impl.hpp:331-359
//   polynomial_arithmetic::compute_barycentric_evaluation   polynomials/polynomial_arithmetic.cpp:811-847
// With n = 2^log2n, w the domain's root, f_i = F(w^i) and d_i = z w^-i - 1:
//   F(z)   = (z^n - 1)/n * sum_i f_i / d_i                      (z^n != 1)
//   F(z w) = (z^n - 1)/n * sum_i f_{(i+1) mod n} / d_i          (the same weights, the values read one place further on)
//   W(w^i) = w^-i (F(z) - f_i) / d_i                            the values of W(X) = (F(X) - F(z)) / (X - z) on the domain
//   z = w^j: F(z) = f_j, F(z w) = f_{(j+1) mod n} exactly (d_j = 0 is detected, its index goes through one flag word)
// One block = BARY_BLK consecutive domain points = ONE inversion group (block_invert.hip.h).  The weights 1/d_i stay in registers: they never go to HBM (the opening stores w^-i / d_i, its output).
// This file holds the kernels and their launches; the host side (argument checks, scratch, z^n) is poly.hip's.
#include "bbg_internal.h"

#include "block_invert.hip.h"
#include "ntt_consts.hip.h"

namespace bbg {

// ---------------------------------------------------------------------------------------------- fr::batch_invert
// out[i] = in[i]^-1, zero stays zero.  A block reads its whole group before it writes: out may be in.
__global__ void __launch_bounds__(256) k_batch_invert(const Fr* in, Fr* out, size_t n)
{
    __shared__ Fr pre[256], suf[256];
    __shared__ Fr inv_total;
    const int tid = threadIdx.x;
    for (size_t base = (size_t)blockIdx.x * BARY_BLK; base < n; base += (size_t)gridDim.x * BARY_BLK) {
        Fr v[BI_E];
        bool zero[BI_E];
#pragma unroll
        for (int e = 0; e < BI_E; e++) {
            const size_t i = base + (size_t)e * 256 + tid;
            v[e] = Fr::one();
            zero[e] = true; // beyond the array: a one in the chain, nothing written
            if (i < n) {
                const Fr x = fe_reduce_once(fe_load<FrP>(in + i)); // [0, 2r) -> canonical: r itself is a zero
                zero[e] = x.is_zero_raw();
                if (!zero[e]) v[e] = x;
            }
        }
        block_invert(v, pre, suf, &inv_total);
#pragma unroll
        for (int e = 0; e < BI_E; e++) {
            const size_t i = base + (size_t)e * 256 + tid;
            if (i < n) fe_store<FrP>(out + i, zero[e] ? Fr::zero() : fe_reduce_once(v[e]));
        }
    }
}
int bary_batch_invert(bbg_ctx* ctx, const void* d_in, void* d_out, size_t n, hipStream_t st)
{
    if (n == 0) return BBG_OK;
    size_t grid = (n + BARY_BLK - 1) / BARY_BLK;
    if (grid > BARY_GRID_MAX) grid = BARY_GRID_MAX;
    ProfScope ps(ctx, "fr_batch_invert", st);
    hipLaunchKernelGGL(k_batch_invert, dim3((unsigned)grid), dim3(256), 0, st, (const Fr*)d_in, (Fr*)d_out, n);
    BBG_HIP(hipGetLastError());
    return BBG_OK;
}

// ---------------------------------------------------------------------------------------------- barycentric evaluation
struct BaryKernelArgs {
    const Fr* poly[BARY_MAX];
    uint32_t shifted; // bit k: polynomial k is read one place further on
    int count;
    unsigned log2n;
    Fr z, zn;         // canonical; zn = z^n
    const DomainConsts* dc;
    Fr* dest;         // the opening's w^-i / d_i, or null
    Fr* partials;     // [count][gridDim.x]
    Fr* results;      // [count]
    unsigned* flag;   // the index of a zero d_i, BARY_NO_HIT otherwise
};
// sum_i f_k[i (+1)] / d_i over the block's groups, for every polynomial k, to partials[k][block]
__global__ void __launch_bounds__(256) k_bary_partial(BaryKernelArgs a)
{
    __shared__ Fr pre[256], suf[256];
    __shared__ Fr inv_total;
    __shared__ Fr acc[BARY_MAX * 4]; // [k][wave]: running sums over the block's groups, each wave its own
    const int tid = threadIdx.x;
    const size_t n = (size_t)1 << a.log2n;
    const size_t stride = (size_t)gridDim.x * BARY_BLK;
    if (tid < a.count * 4) acc[tid] = Fr::zero(); // (count * 4 <= 128 threads)
    __syncthreads();
    // w^-i of the thread's first point, and the steps to its next values and its next group
    Fr x = pow_from_table(a.dc->pow2_root_inv, (uint64_t)blockIdx.x * BARY_BLK + tid);
    const Fr step256 = a.dc->pow2_root_inv[8];
    const Fr step_group = pow_from_table(a.dc->pow2_root_inv, (uint64_t)stride);
    for (size_t base = (size_t)blockIdx.x * BARY_BLK; base < n; base += stride) {
        Fr v[BI_E], wi[BI_E];
        Fr xe = x;
#pragma unroll
        for (int e = 0; e < BI_E; e++) {
            const size_t i = base + (size_t)e * 256 + tid;
            wi[e] = xe;
            v[e] = Fr::one();
            if (i < n) {
                const Fr d = fe_reduce_once(fe_sub(fe_mul(a.z, xe), Fr::one())); // z w^-i - 1, canonical
                if (d.is_zero_raw()) atomicMin(a.flag, (unsigned)i);             // z = w^i: answered from the values (k_bary_final)
                else v[e] = d;
            }
            xe = fe_mul(xe, step256);
        }
        block_invert(v, pre, suf, &inv_total);
        if (a.dest) {
#pragma unroll
            for (int e = 0; e < BI_E; e++) {
                const size_t i = base + (size_t)e * 256 + tid;
                if (i < n) fe_store<FrP>(a.dest + i, fe_mul(wi[e], v[e]));
            }
        }
        for (int k = 0; k < a.count; k++) {
            const size_t sh = (a.shifted >> k) & 1u;
            const Fr* __restrict__ f = a.poly[k];
            Fr s = Fr::zero();
#pragma unroll
            for (int e = 0; e < BI_E; e++) {
                const size_t i = base + (size_t)e * 256 + tid;
                if (i < n) s = fe_add(s, fe_mul(fe_load<FrP>(f + ((i + sh) & (n - 1))), v[e]));
            }
            s = wave_sum(s);
            if ((tid & 63) == 0) acc[k * 4 + (tid >> 6)] = fe_add(acc[k * 4 + (tid >> 6)], s);
        }
        x = fe_mul(x, step_group);
    }
    __syncthreads();
    if (tid < a.count) {
        const Fr s = fe_add(fe_add(acc[tid * 4], acc[tid * 4 + 1]), fe_add(acc[tid * 4 + 2], acc[tid * 4 + 3]));
        fe_store<FrP>(a.partials + (size_t)tid * gridDim.x + blockIdx.x, s);
    }
}
// results[k] = (z^n - 1)/n * sum of polynomial k's partials, or the stored value when z is on the domain; one block per polynomial
__global__ void __launch_bounds__(256) k_bary_final(BaryKernelArgs a, unsigned nparts)
{
    __shared__ Fr sm[4];
    const int tid = threadIdx.x;
    const int k = blockIdx.x;
    const size_t n = (size_t)1 << a.log2n;
    const unsigned hit = *a.flag;
    if (hit != BARY_NO_HIT) { // uniform
        if (tid == 0) {
            const size_t i = ((size_t)hit + ((a.shifted >> k) & 1u)) & (n - 1);
            fe_store<FrP>(a.results + k, fe_reduce_once(fe_load<FrP>(a.poly[k] + i)));
        }
        return;
    }
    Fr s = Fr::zero();
    for (unsigned i = tid; i < nparts; i += 256) s = fe_add(s, fe_load<FrP>(a.partials + (size_t)k * nparts + i));
    s = wave_sum(s);
    if ((tid & 63) == 0) sm[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        s = fe_add(fe_add(sm[0], sm[1]), fe_add(sm[2], sm[3]));
        const Fr scale = fe_mul(fe_sub(a.zn, Fr::one()), a.dc->n_inv);
        fe_store<FrP>(a.results + k, fe_reduce_once(fe_mul(s, scale)));
    }
}
// dest_i <- (F(z) - f_i) dest_i, canonical
__global__ void __launch_bounds__(256) k_bary_open_finish(const Fr* __restrict__ f, Fr* dest, size_t n, const Fr* fz)
{
    const Fr y = fe_load<FrP>(fz);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        fe_store<FrP>(dest + i, fe_reduce_once(fe_mul(fe_sub(y, fe_load<FrP>(f + i)), fe_load<FrP>(dest + i))));
}

int bary_evaluate(bbg_ctx* ctx, const BaryArgs& h, hipStream_t st)
{
    const size_t n = (size_t)1 << h.log2n;
    BaryKernelArgs a;
    for (int k = 0; k < BARY_MAX; k++) a.poly[k] = k < h.count ? (const Fr*)h.polys[k] : nullptr;
    a.shifted = h.shifted;
    a.count = h.count;
    a.log2n = h.log2n;
    static_assert(sizeof(Fr) == sizeof(h.z), "Fr is eight 32-bit words");
    __builtin_memcpy(&a.z, h.z, 32);
    __builtin_memcpy(&a.zn, h.zn, 32);
    a.dc = (const DomainConsts*)h.consts;
    a.dest = (Fr*)h.dest;
    a.partials = (Fr*)h.partials;
    a.results = (Fr*)h.results;
    a.flag = h.flag;
    const unsigned grid = bary_grid(n);
    ProfScope ps(ctx, "barycentric", st);
    BBG_HIP(hipMemsetAsync(h.flag, 0xff, sizeof(unsigned), st)); // BARY_NO_HIT, on every call
    hipLaunchKernelGGL(k_bary_partial, dim3(grid), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_bary_final, dim3((unsigned)h.count), dim3(256), 0, st, a, grid);
    if (h.dest) {
        size_t g2 = (n + 255) / 256;
        if (g2 > 256 * 16) g2 = 256 * 16;
        hipLaunchKernelGGL(k_bary_open_finish, dim3((unsigned)g2), dim3(256), 0, st, (const Fr*)h.polys[0], (Fr*)h.dest, n, (const Fr*)h.results);
    }
    BBG_HIP(hipGetLastError());
    return BBG_OK;
}

} // namespace bbg
