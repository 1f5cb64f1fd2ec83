// Fq12 arithmetic spread over the lanes of ONE wave, on top of fq_tower.hip.h (pairing_wave.hip).  The element is kept in the
// w-basis, a = sum_(i<6) a_i w^i with a_i in Fq2 and w^6 = xi: against the reference's layout c0 = (a_0, a_2, a_4), c1 = (a_1, a_3, a_5).
// In LDS a value is twelve Fq, coefficient c = 2 i + h being half h (c0 / c1) of a_i.  The schoolbook product is
//     r_((i + j) mod 6) += a_i b_j, times xi where i + j >= 6,
// 36 independent Fq2 products, and a line (o, vw, vv) sits at w^0, w^3, w^4, so a sparse product is 18 of them:
//   phase 1   lane NJ i + jj forms a_i b_j (j = jj, or 0 / 3 / 4 for a line), times xi where it wraps, into prod[6 i + j]: 3 dependent fe_mul;
//   phase 2   lane c < 12 sums the NJ terms of its Fq coefficient, prod[6 ((k - j) mod 6) + j][h] with k = c / 2, h = c % 2, into the result.
// Each phase ends in a barrier, so a result may be one of the operands.  Every branch around a barrier depends on the lane index and on
// wave-uniform values only; the callers keep the control flow around a call wave-uniform.  tests/tools/pairing_wave_model.py is this
// dataflow on integers.
#pragma once
#include "fq_tower.hip.h"

namespace bbg {

constexpr int W12_LANES = 64; // a block is one wave: the lane schedules below and the callers' ballots count on it
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__GFX9__)
#error "fq12_wave.hip.h is written for the 64-lane waves of GFX9 / CDNA" // the host side checks the device's wave size as well (pairing_wave_run)
#endif

struct W12Lds {
    Fq slot[PairP::FINAL_SLOTS][12];  // the slots of PAIR_FINAL_PROGRAM; the Miller loop's accumulator is slot 0
    Fq prod[36][2];                   // the staging of one product
    Fq line[6];                       // the sparse operand: o | vw P.y | vv P.x
    Fq pt[BBG_PAIRING_MAX_PAIRS][2];  // the product's G1 points, x | y
};

// the place of a_i among the reference's six Fq2 components c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2
__device__ __forceinline__ unsigned w12_ref_component(unsigned i) { return (i & 1) ? 3 + (i >> 1) : (i >> 1); }
// the power of w a line's component jj = 0, 1, 2 (o, vw, vv) multiplies
__device__ __forceinline__ unsigned w12_line_power(unsigned jj) { return jj == 0 ? 0 : jj + 2; }

__device__ __forceinline__ void w12_set_one(W12Lds& s, unsigned lane, unsigned d)
{
    if (lane < 12) s.slot[d][lane] = lane == 0 ? Fq::one() : Fq::zero();
    __syncthreads();
}

// slot d = slot a times b: b the twelve coefficients of a slot, or with SPARSE the six of s.line
template <bool SPARSE> __device__ __forceinline__ void w12_mul(W12Lds& s, unsigned lane, unsigned d, unsigned a, const Fq* b)
{
    constexpr unsigned NJ = SPARSE ? 3 : 6;
    if (lane < 6 * NJ) {
        const unsigned i = lane / NJ, jj = lane % NJ;
        const unsigned j = SPARSE ? w12_line_power(jj) : jj;
        const Fq2 x = { s.slot[a][2 * i], s.slot[a][2 * i + 1] };
        const Fq2 y = { b[2 * jj], b[2 * jj + 1] };
        Fq2 p = f2_mul(x, y);
        if (i + j >= 6) p = f2_mul_xi(p);
        s.prod[6 * i + j][0] = p.c0;
        s.prod[6 * i + j][1] = p.c1;
    }
    __syncthreads();
    if (lane < 12) {
        const unsigned k = lane >> 1, h = lane & 1;
        Fq acc = s.prod[6 * k][h]; // j = 0: i = k
#pragma unroll
        for (unsigned jj = 1; jj < NJ; jj++) {
            const unsigned j = SPARSE ? w12_line_power(jj) : jj;
            const unsigned i = (k + 6 - j) % 6;
            acc = fe_add(acc, s.prod[6 * i + j][h]);
        }
        s.slot[d][lane] = acc;
    }
    __syncthreads();
}

// slot d = the conjugate over Fq6 of slot a: the odd powers of w change sign
__device__ __forceinline__ void w12_conj(W12Lds& s, unsigned lane, unsigned d, unsigned a)
{
    if (lane < 12) {
        const Fq t = s.slot[a][lane];
        s.slot[d][lane] = (lane & 2) ? fe_neg(t) : t;
    }
    __syncthreads();
}

// slot d = slot a to the power p^k, k = 1, 2, 3 (uniform): one constant per Fq2 coefficient, a_0 conjugated only
__device__ __forceinline__ void w12_frobenius(W12Lds& s, unsigned lane, unsigned d, unsigned a, int k)
{
    if (lane < 6) {
        const Fq2 x = { s.slot[a][2 * lane], s.slot[a][2 * lane + 1] };
        Fq2 r;
        if (lane == 0) r = (k & 1) ? f2_conj(x) : x;
        else r = f12_frob_part(x, k, (int)w12_ref_component(lane));
        s.slot[d][2 * lane] = r.c0;
        s.slot[d][2 * lane + 1] = r.c1;
    }
    __syncthreads();
}

// slot d = the inverse of slot a on lane 0, through the tower's f12_inv
__device__ __forceinline__ void w12_inv(W12Lds& s, unsigned lane, unsigned d, unsigned a)
{
    if (lane == 0) {
        const Fq* x = s.slot[a];
        Fq12 v;
        v.c0.c0 = { x[0], x[1] };
        v.c1.c0 = { x[2], x[3] };
        v.c0.c1 = { x[4], x[5] };
        v.c1.c1 = { x[6], x[7] };
        v.c0.c2 = { x[8], x[9] };
        v.c1.c2 = { x[10], x[11] };
        v = f12_inv(v);
        Fq* r = s.slot[d];
        r[0] = v.c0.c0.c0, r[1] = v.c0.c0.c1;
        r[2] = v.c1.c0.c0, r[3] = v.c1.c0.c1;
        r[4] = v.c0.c1.c0, r[5] = v.c0.c1.c1;
        r[6] = v.c1.c1.c0, r[7] = v.c1.c1.c1;
        r[8] = v.c0.c2.c0, r[9] = v.c0.c2.c1;
        r[10] = v.c1.c2.c0, r[11] = v.c1.c2.c1;
    }
    __syncthreads();
}

// Lane c < 12 writes the canonical coefficient c of slot a to its place in the reference's 384 bytes at out (may be null); returns,
// to every lane, whether the value is one.
__device__ __forceinline__ bool w12_store_is_one(const W12Lds& s, unsigned lane, unsigned a, char* out)
{
    bool mine = true;
    if (lane < 12) {
        const Fq v = fq_canon(s.slot[a][lane]);
        if (out) fe_store<FqP>(out + w12_ref_component(lane >> 1) * 64 + (lane & 1) * 32, v);
        uint32_t diff = 0;
#pragma unroll
        for (int w = 0; w < 8; w++) diff |= v.v[w] ^ (lane == 0 ? FqP::ONE[w] : 0u);
        mine = diff == 0;
    }
    return __all(mine) != 0;
}

} // namespace bbg
