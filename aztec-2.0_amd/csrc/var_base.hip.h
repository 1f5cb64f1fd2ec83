// Variable-base scalar multiplication k * P over BN254 G1 for gfx950: the bit-serial double-and-add (xyzz_mul_fr) and the windowed GLV
// form (xyzz_mul_glv) that var_base.hip, ecntt.hip and open_all.hip share.
//
// xyzz_mul_glv has the shape of the reference's element::mul_with_endomorphism (ecc/groups/element_impl.hpp:593-663): the scalar is split
// against the cube root of unity lambda, lambda (x, y) = (beta x, y), into two halves below 2^128 which walk one table of odd multiples
// side by side in signed 4-bit windows.
//
//   split    k = k1 - k2 lambda (mod r) with the lattice basis (a1, b1), (a2, b2) of { (u, v) : u + v lambda = 0 mod r }, b1 < 0:
//                c1 = floor(G2 k / 2^256),  c2 = floor(G1 k / 2^256),   G2 = floor(2^256 b2 / r),  G1 = floor(2^256 (-b1) / r)
//                k1 = k - c1 a1 - c2 a2,    k2 = c2 b2 - c1 (-b1)
//            (a1 = b2 and a1 b2 + a2 (-b1) = r).  With c1 = b2 k / r - e1, c2 = (-b1) k / r - e2 the floors give 0 <= e1 < 1.09, 0 <= e2 < 1.13
//            (1 + the fraction dropped from G times r / 2^256), and k1 = e1 a1 + e2 a2 lies in [0, 0.98 * 2^127), k2 = e1 (-b1) - e2 b2 in
//            (-1.13 b2, 0.95 * 2^127): k1 is never negative, k2 is for about one scalar in 2^63 (e1 below 2^-63).  Both are computed modulo
//            2^160 and k2 is taken as sign and magnitude, so every canonical k is split exactly (exact bounds: half_bounds() of
//            tests/tools/var_base_model.py).  Where k2 >= 0 the halves are the ones of field::split_into_endomorphism_scalars
//            (fields/field.hpp:236-282), which has the same constants and truncates a negative k2 mod r to 128 bits.
//   recode   a half h < 2^128 is made odd (skew = 1 and h + 1 for an even h: one P is taken off at the end) and written as 32 odd digits
//            h = sum_i d_i 16^i, d_i in { +-1, +-3, .. +-15 }:  d_i = (((h >> 4i) & 31) | 1) - 16 for i < 31 and d_31 = (h >> 124) | 1
//            (h_i = (h >> 4i) | 1 is what is left after i digits, d_i = h_i mod 32 - 16, and (h_i - d_i) / 16 = h_(i+1)).  A digit is five
//            bits of h: bit 4 the sign (set = positive), bits 3..1 the table index ((w >> 1) & 7 for a positive digit, 7 minus that for a
//            negative one).  The halves are shifted left four bits per round so that the window is always bits 28..24 of the top limb: no
//            runtime-indexed limb, and the loop body exists once.
//   table    T[j] = (2j + 1) P, j < 8, in XYZZ form: 1 doubling + 7 additions.  Eight XYZZ points are 1 KiB per lane: they cannot live in
//            registers (a runtime-indexed register array would go to scratch) and in LDS they would leave one wave per two SIMDs, so the
//            table is in global memory, 1 KiB per lane, and each lane gathers its own contiguous 128 bytes per addition.  The beta twin of
//            an entry is one Fq product (X -> beta X: x = X / ZZ), a negative one fe_neg(Y).
//   rounds   32 times: 4 doublings, + T[.] for the first half, - beta T[.] for the second (k = k1 - k2 lambda); then the two skew
//            corrections.  128 doublings (the first four act on infinity and return at once) + 66 additions + the table's 1 + 7, against
//            256 + ~127 of the bit-serial loop.
// Every addition is xyzz_add / xyzz_dbl of curve.hip.h, complete: an accumulator that meets +- a table entry, k = 0 (1 P - P), an infinite
// P are all handled there.
#pragma once
#include "curve.hip.h"

namespace bbg {

__device__ __forceinline__ Xyzz xyzz_neg(const Xyzz& p)
{
    Xyzz r = p;
    r.y = fe_neg(p.y);
    return r;
}

// k * P for a plain (non-Montgomery) canonical k < r < 2^254: left-to-right double-and-add.  The scalar is shifted left one bit per
// step so that the bit under test is always bit 255: no runtime-indexed limb, and the loop body exists once.
__device__ __forceinline__ Xyzz xyzz_mul_fr(const Xyzz& p, Fr k)
{
    Xyzz acc = xyzz_inf();
    for (int i = 0; i < 256; i++) {
        const bool bit = (k.v[7] >> 31) != 0;
#pragma unroll
        for (int l = 7; l > 0; l--) k.v[l] = (k.v[l] << 1) | (k.v[l - 1] >> 31);
        k.v[0] <<= 1;
        acc = xyzz_dbl(acc); // returns at once while acc is still infinity
        if (bit) acc = xyzz_add(acc, p);
    }
    return acc;
}

// ---------------------------------------------------------------------------------------------- GLV split
// Constants (32-bit limbs, little-endian) re-derived with Python integers in tests/tools/var_base_model.py, which the CPU tests pin to the
// oracle: lambda^3 = 1 mod r, beta^3 = 1 mod p, lambda G = (beta x_G, y_G).
struct GlvP {
    static constexpr uint32_t G1[5] = { 0x391eb18du, 0x7a7bd9d4u, 0xa773d2cfu, 0x4ccef014u, 0x00000002u }; // floor(2^256 (-b1) / r)
    static constexpr uint32_t G2[3] = { 0xc7e0b3d7u, 0xd91d232eu, 0x00000002u };                           // floor(2^256 b2 / r)
    static constexpr uint32_t MB1[4] = { 0x7d4f1128u, 0x8211bbebu, 0xeeb859fcu, 0x6f4d8248u };             // -b1
    static constexpr uint32_t B2[2] = { 0x94d213e3u, 0x89d32568u };                                        // b2 = a1
    static constexpr uint32_t A2[4] = { 0x1221250bu, 0x0be4e154u, 0xeeb859fdu, 0x6f4d8248u };              // a2 = (r - b2^2) / (-b1)
    // beta in Montgomery form (canonical)
    static constexpr uint32_t BETA[8] = { 0xd782e155u, 0x71930c11u, 0xffbe3323u, 0xa6bb947cu, 0xd4741444u, 0xaa303344u, 0x26594943u, 0x2c3b3f0du };
};

namespace glv {
// out[0 .. NO) = limbs [SKIP, SKIP + NO) of a * b (a: NA limbs, b: NB limbs), schoolbook by columns; every index is a constant
template <int NA, int NB, int SKIP, int NO> __device__ __forceinline__ void mul_cols(uint32_t* out, const uint32_t* a, const uint32_t* b)
{
    uint64_t lo = 0, hi = 0; // column sum = hi 2^32 + lo, hi < 2^40
#pragma unroll
    for (int c = 0; c < SKIP + NO; c++) {
#pragma unroll
        for (int i = 0; i < NA; i++) {
            const int j = c - i;
            if (j < 0 || j >= NB) continue;
            const uint64_t pr = (uint64_t)a[i] * b[j];
            lo += (uint32_t)pr;
            hi += pr >> 32;
        }
        if (c >= SKIP) out[c - SKIP] = (uint32_t)lo;
        lo = (lo >> 32) + (uint32_t)hi;
        hi >>= 32;
    }
}
// r -= s on 5 limbs (mod 2^160)
__device__ __forceinline__ void sub160(uint32_t* r, const uint32_t* s)
{
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) {
        const uint64_t d = (uint64_t)r[i] - s[i] - br;
        r[i] = (uint32_t)d;
        br = (d >> 32) & 1u;
    }
}
} // namespace glv

struct GlvHalves {
    uint32_t h1[4], h2[4]; // |k1|, |k2| made odd
    bool neg2;             // k2 < 0
    bool skew1, skew2;     // the half was even: h = |k| + 1
};

// canonical plain k < r -> halves, k = k1 - k2 lambda
__device__ __forceinline__ GlvHalves glv_split(const Fr& k)
{
    using namespace glv;
    uint32_t g1[5], g2[3], mb1[4], b2[2], a2[4];
#pragma unroll
    for (int i = 0; i < 5; i++) g1[i] = GlvP::G1[i];
#pragma unroll
    for (int i = 0; i < 3; i++) g2[i] = GlvP::G2[i];
#pragma unroll
    for (int i = 0; i < 4; i++) mb1[i] = GlvP::MB1[i], a2[i] = GlvP::A2[i];
#pragma unroll
    for (int i = 0; i < 2; i++) b2[i] = GlvP::B2[i];
    uint32_t c1[3], c2[5]; // c1 < 2^64 (limb 2 is zero), c2 < 2^128 (limb 4 is zero): G k < 2^(130 + 254)
    mul_cols<8, 3, 8, 3>(c1, k.v, g2);
    mul_cols<8, 5, 8, 5>(c2, k.v, g1);
    uint32_t k1[5], k2[5], t[5];
    // k2 = c2 b2 - c1 (-b1)   (mod 2^160)
    mul_cols<4, 2, 0, 5>(k2, c2, b2);
    mul_cols<2, 4, 0, 5>(t, c1, mb1);
    sub160(k2, t);
    // k1 = k - c1 a1 - c2 a2  (mod 2^160), a1 = b2
#pragma unroll
    for (int i = 0; i < 5; i++) k1[i] = k.v[i];
    mul_cols<2, 2, 0, 5>(t, c1, b2);
    sub160(k1, t);
    mul_cols<4, 4, 0, 5>(t, c2, a2);
    sub160(k1, t);
    GlvHalves r;
    r.neg2 = (k2[4] >> 31) != 0;
    if (r.neg2) { // |k2| = 0 - k2
        uint32_t z[5] = { 0, 0, 0, 0, 0 };
        sub160(z, k2);
#pragma unroll
        for (int i = 0; i < 5; i++) k2[i] = z[i];
    }
    r.skew1 = (k1[0] & 1u) == 0;
    r.skew2 = (k2[0] & 1u) == 0;
#pragma unroll
    for (int i = 0; i < 4; i++) r.h1[i] = k1[i], r.h2[i] = k2[i];
    r.h1[0] |= 1u; // an even half plus one
    r.h2[0] |= 1u;
    return r;
}

// The same split with the PLAIN magnitudes, for callers that recode the halves themselves (msm_points.hip): m1 = |k1| (k1 is never
// negative), m2 = |k2|, four limbs each; returns k2 < 0.  A body of its own, so that glv_split and the kernels built on it compile as
// they did; tests/tools/var_base_model.py split() is the model of both.
__device__ __forceinline__ bool glv_split_mag(const Fr& k, uint32_t* m1, uint32_t* m2)
{
    using namespace glv;
    uint32_t g1[5], g2[3], mb1[4], b2[2], a2[4];
#pragma unroll
    for (int i = 0; i < 5; i++) g1[i] = GlvP::G1[i];
#pragma unroll
    for (int i = 0; i < 3; i++) g2[i] = GlvP::G2[i];
#pragma unroll
    for (int i = 0; i < 4; i++) mb1[i] = GlvP::MB1[i], a2[i] = GlvP::A2[i];
#pragma unroll
    for (int i = 0; i < 2; i++) b2[i] = GlvP::B2[i];
    uint32_t c1[3], c2[5];
    mul_cols<8, 3, 8, 3>(c1, k.v, g2);
    mul_cols<8, 5, 8, 5>(c2, k.v, g1);
    uint32_t k1[5], k2[5], t[5];
    mul_cols<4, 2, 0, 5>(k2, c2, b2); // k2 = c2 b2 - c1 (-b1)   (mod 2^160)
    mul_cols<2, 4, 0, 5>(t, c1, mb1);
    sub160(k2, t);
#pragma unroll
    for (int i = 0; i < 5; i++) k1[i] = k.v[i]; // k1 = k - c1 a1 - c2 a2  (mod 2^160), a1 = b2
    mul_cols<2, 2, 0, 5>(t, c1, b2);
    sub160(k1, t);
    mul_cols<4, 4, 0, 5>(t, c2, a2);
    sub160(k1, t);
    const bool neg2 = (k2[4] >> 31) != 0;
    if (neg2) { // |k2| = 0 - k2
        uint32_t z[5] = { 0, 0, 0, 0, 0 };
        sub160(z, k2);
#pragma unroll
        for (int i = 0; i < 5; i++) k2[i] = z[i];
    }
#pragma unroll
    for (int i = 0; i < 4; i++) m1[i] = k1[i], m2[i] = k2[i];
    return neg2;
}

// ---------------------------------------------------------------------------------------------- table and rounds
constexpr int GLV_TABLE = 8;                                  // odd multiples P, 3P .. 15P
constexpr size_t GLV_TABLE_BYTES = GLV_TABLE * sizeof(Xyzz);  // 1 KiB per lane

// This lane's table inside its wave's block of 64 (`wave_tables`: wave-uniform, lives in scalar registers).  The address is rebuilt from
// the lane id at every use instead of being carried: with the accumulator, an entry and the addition's temporaries live the round loop has
// no vector register to spare, and a carried 64-bit address was what the register allocator spilled -- and reloaded from scratch in
// front of every gather.  The volatile statement is two instructions and cannot be hoisted into a register that would be spilled again.
// Needs blocks of exactly one wave (64 threads), lane l owning table l of the block.
__device__ __forceinline__ Xyzz* glv_lane_table(Xyzz* wave_tables)
{
    uint32_t l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return wave_tables + (size_t)l * GLV_TABLE;
}

// the table entry a five-bit window w selects, negated when the digit's sign and `flip` say so; TWIN: the entry of lambda P
template <bool TWIN> __device__ __forceinline__ Xyzz glv_entry(Xyzz* wave_tables, uint32_t w, bool flip)
{
    const Xyzz* table = glv_lane_table(wave_tables);
    const bool positive = (w & 16u) != 0;
    const uint32_t m = (w >> 1) & 7u;
    Xyzz e = xyzz_load(table + (positive ? m : 7u - m));
    if (TWIN) {
        Fq beta;
#pragma unroll
        for (int i = 0; i < 8; i++) beta.v[i] = GlvP::BETA[i];
        e.x = fe_mul(e.x, beta);
    }
    const Fq ny = fe_neg(e.y);
    const bool neg = positive == flip;
#pragma unroll
    for (int i = 0; i < 8; i++) e.y.v[i] = neg ? ny.v[i] : e.y.v[i];
    return e;
}

// k * P for a plain canonical k < r; `wave_tables`: 64 x GLV_TABLE_BYTES of global memory the calling wave owns (16-byte aligned, the same
// pointer in every lane; blocks of 64 threads).  P may be infinite.
__device__ __forceinline__ Xyzz xyzz_mul_glv(const Xyzz& p, const Fr& k, Xyzz* wave_tables)
{
    if (xyzz_is_inf(p)) return p;
    {
        const Xyzz p2 = xyzz_dbl(p);
        Xyzz e = p;
        xyzz_store(glv_lane_table(wave_tables), e);
#pragma unroll 1
        for (int j = 1; j < GLV_TABLE; j++) {
            e = xyzz_add(e, p2);
            xyzz_store(glv_lane_table(wave_tables) + j, e);
        }
    }
    GlvHalves s = glv_split(k);
    Xyzz acc = xyzz_inf();
    uint32_t w1 = 16u | (s.h1[3] >> 28), w2 = 16u | (s.h2[3] >> 28); // the top digits are positive
#pragma unroll 1
    for (int round = 0; round < 32; round++) {
#pragma unroll 1
        for (int d = 0; d < 4; d++) acc = xyzz_dbl(acc); // returns at once in round 0
        acc = xyzz_add(acc, glv_entry<false>(wave_tables, w1, false));
        acc = xyzz_add(acc, glv_entry<true>(wave_tables, w2, !s.neg2)); // - k2 lambda P
        w1 = (s.h1[3] >> 24) & 31u;
        w2 = (s.h2[3] >> 24) & 31u;
#pragma unroll
        for (int l = 3; l > 0; l--) {
            s.h1[l] = (s.h1[l] << 4) | (s.h1[l - 1] >> 28);
            s.h2[l] = (s.h2[l] << 4) | (s.h2[l - 1] >> 28);
        }
        s.h1[0] <<= 4;
        s.h2[0] <<= 4;
    }
    // skew: the odd half was one too large
    if (s.skew1) acc = xyzz_add(acc, glv_entry<false>(wave_tables, 16u, true));       // - P
    if (s.skew2) acc = xyzz_add(acc, glv_entry<true>(wave_tables, 16u, s.neg2));     // + lambda P (- for a negative k2)
    return acc;
}

} // namespace bbg
