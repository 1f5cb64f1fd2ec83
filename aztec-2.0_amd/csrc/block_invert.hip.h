// One inversion group of the Lagrange-form kernels (barycentric.hip, open_points.hip): a 256-thread block inverts its BARY_BLK values behind
// ONE real inversion.  Every thread multiplies up its BARY_E values, the block scans the thread totals in LDS (inclusive prefix and exclusive
// suffix products side by side), one wave inverts the block total on the scalar unit (fe_inverse_gcd<.., true>: a binary Euclid diverges per
// lane, Montgomery's trick needs one inversion per group) and every thread walks back through its values.  Beside it the sum of an Fr over a
// wave, which the same kernels end their partial sums with.
#pragma once
#include "bbg_internal.h"

#include "field.hip.h"

namespace bbg {

constexpr int BI_E = BARY_E; // values per thread; lane-interleaved: thread t of a group takes base + e * 256 + t

// v[e] <- 1 / v[e] (coarse, < 2p) for the BI_E non-zero values of each of the block's 256 threads.  pre / suf: 256 entries each.
__device__ __forceinline__ void block_invert(Fr (&v)[BI_E], Fr* pre, Fr* suf, Fr* inv_total)
{
    const int tid = threadIdx.x;
    Fr p[BI_E]; // p[e] = v[0] .. v[e]
    p[0] = v[0];
#pragma unroll
    for (int e = 1; e < BI_E; e++) p[e] = fe_mul(p[e - 1], v[e]);
    Fr a = p[BI_E - 1], b = a; // a: inclusive prefix product of the thread totals, b: inclusive suffix product
    pre[tid] = a;
    suf[tid] = b;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        Fr xa = a, xb = b;
        if (tid >= d) xa = fe_mul(pre[tid - d], a);
        if (tid + d < 256) xb = fe_mul(b, suf[tid + d]);
        __syncthreads();
        a = xa;
        b = xb;
        pre[tid] = a;
        suf[tid] = b;
        __syncthreads();
    }
    if (__builtin_amdgcn_readfirstlane(tid) < 64) { // wave 0 alone (a scalar branch), every lane the same input: the chain runs on the scalar unit
        const Fr t = fe_inverse_gcd<FrP, true>(pre[255]);
        if (tid == 0) *inv_total = t;
    }
    __syncthreads();
    // 1 / (prefix through this thread) = (suffix after it) / total
    Fr r = *inv_total;
    if (tid + 1 < 256) r = fe_mul(r, suf[tid + 1]);
    const Fr before = tid ? pre[tid - 1] : Fr::one(); // prefix of the earlier threads
    __syncthreads();                                 // (the arrays are rewritten by the next group)
#pragma unroll
    for (int e = BI_E - 1; e >= 0; e--) {
        const Fr lead = e ? fe_mul(before, p[e - 1]) : before; // everything in front of v[e]
        const Fr inv = fe_mul(r, lead);
        r = fe_mul(r, v[e]);
        v[e] = inv;
    }
}

// the sum of s over the 64 lanes of the wave, in every lane
__device__ __forceinline__ Fr wave_sum(Fr s)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        Fr o;
#pragma unroll
        for (int w = 0; w < 8; w++) o.v[w] = (uint32_t)__shfl_xor((int)s.v[w], d, 64);
        s = fe_add(s, o);
    }
    return s;
}

} // namespace bbg
