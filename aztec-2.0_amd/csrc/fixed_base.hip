// Fixed-base batch scalar multiplication over BN254 G1 for gfx950: out[i] = s_i * B for n full-width scalars and ONE base point, and on
// top of it the structured reference string P_i = [x^i] G (bbg_srs_synth_powers).
//
// The reference has no function of this shape: where it needs many multiples of one point it loops over element::operator* on the host
// (a 254-step double-and-add each; its tests build [x^i] G that way, lagrange_base.test.cpp:25-34).  With the base fixed the doublings
// can be paid once:
//   * k_fb_table   T[w][d-1] = d * 2^(8w) * B for the 32 byte positions w of a scalar and d = 1 .. 255: 8160 canonical affine points,
//                  510 KiB, built on the device and cached in the context under the base's canonical bytes.  One block per window, one
//                  thread per entry: 8w doublings of B (the same in every thread of the block), an 8-step double-and-add by d, one
//                  inversion.  A millisecond once per base; no running sums, no second pass.
//   * k_fb_mul     one thread per FB_CH consecutive scalars.  Per scalar: out of Montgomery form, then k = sum_w d_w 2^(8w) is
//                  sum_w T[w][d_w - 1] -- at most 32 complete mixed additions (xyzz_madd) and NO doubling.  The scalar is shifted right
//                  one byte per step so that the digit is always the low byte of limb 0: no runtime-indexed limb, the loop body exists
//                  once, and the table entry of the NEXT digit is loaded before the current addition starts.  The FB_CH results are made
//                  affine behind one inversion by the batched conversion of curve.hip.h (aff_batch_*).  A result at infinity
//                  (s = 0 mod r, or an infinite base) is written as aff_inf().
//   * k_fb_powers  s_i = x^i for the structured string (each thread starts its run of FB_POW_E powers with a square-and-multiply).
// All group-law cases are handled by xyzz_madd / xyzz_add / xyzz_dbl, although with a canonical scalar k < r the accumulator
// sum_{v<w} d_v 2^(8v) B can never be +-(d_w 2^(8w) B).
#include "bbg_internal.h"
#include "curve.hip.h"

#include <cstring>

namespace bbg {

constexpr int FB_WINDOWS = 32;  // byte positions of a 256-bit scalar
constexpr int FB_DIGITS = 255;  // entries per window: d = 1 .. 255 (d = 0 adds nothing)
constexpr size_t FB_TABLE_BYTES = (size_t)FB_WINDOWS * FB_DIGITS * 64;
constexpr int FB_CH = 4;        // scalars per thread behind one inversion
constexpr int FB_POW_E = 16;    // powers per thread of k_fb_powers

// a field element / a point handed to a kernel by value (host words, little-endian 64-bit limbs)
struct FbFrArg {
    uint64_t v[4];
};
struct FbAffArg {
    uint64_t v[8];
};
template <class P> __device__ __forceinline__ Fe<P> fb_words(const uint64_t* w)
{
    Fe<P> r;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        r.v[2 * i] = (uint32_t)w[i];
        r.v[2 * i + 1] = (uint32_t)(w[i] >> 32);
    }
    return r;
}

// ---------------------------------------------------------------------------------------------- table
__global__ void __launch_bounds__(256) k_fb_table(Affine* __restrict__ table, FbAffArg base)
{
    const int w = blockIdx.x, d = threadIdx.x + 1;
    if (d > FB_DIGITS) return;
    Affine B;
    B.x = fb_words<FqP>(base.v);
    B.y = fb_words<FqP>(base.v + 4);
    Xyzz bw = aff_is_inf(B) ? xyzz_inf() : xyzz_from_affine(B);
    for (int i = 0; i < 8 * w; i++) bw = xyzz_dbl(bw); // 2^(8w) B
    Xyzz acc = xyzz_inf();
    for (int b = 7; b >= 0; b--) {
        acc = xyzz_dbl(acc);
        if ((d >> b) & 1) acc = xyzz_add(acc, bw);
    }
    aff_store(table + (size_t)w * FB_DIGITS + (d - 1), xyzz_to_affine(acc)); // aff_inf() for an infinite base
}

// ---------------------------------------------------------------------------------------------- multiplication
// k * B from the table for a plain canonical k
__device__ __forceinline__ Xyzz fb_mul_one(const Affine* __restrict__ table, Fr k)
{
    Xyzz acc = xyzz_inf();
    uint32_t d = k.v[0] & 0xffu;
    Affine nxt = aff_load(table + (d ? d - 1 : 0));
#pragma unroll 1
    for (int w = 0; w < FB_WINDOWS; w++) {
        const Affine cur = nxt;
        const uint32_t dc = d;
#pragma unroll
        for (int l = 0; l < 7; l++) k.v[l] = (k.v[l] >> 8) | (k.v[l + 1] << 24);
        k.v[7] >>= 8;
        d = k.v[0] & 0xffu;
        if (w + 1 < FB_WINDOWS) nxt = aff_load(table + (size_t)(w + 1) * FB_DIGITS + (d ? d - 1 : 0)); // in flight during the addition below
        if (dc) acc = xyzz_madd(acc, cur);
    }
    return acc;
}

// Two waves per SIMD; no scratch, no LDS.  The FB_CH results of a thread become canonical affine behind one inversion (aff_batch_chunk4,
// curve.hip.h); a result at infinity is written as aff_inf().
// Scalars arrive in Montgomery form as any 256-bit representative a: fe_from_mont returns reduce_once((a + m p) / 2^256) with m < 2^256,
// and (a + m p) / 2^256 < 1 + p, so the plain value is canonical (k < r) whatever representative came in.
static_assert(FB_CH == 4, "k_fb_mul converts its chunk with aff_batch_chunk4");
__global__ void __launch_bounds__(64, 2) k_fb_mul(const Affine* __restrict__ table, const Fr* __restrict__ scalars, size_t n, Affine* out)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t i0 = t * FB_CH;
    if (i0 >= n) return;
    const int cnt = n - i0 < (size_t)FB_CH ? (int)(n - i0) : FB_CH;
    aff_batch_chunk4(out + i0, cnt, [&](int e) __attribute__((always_inline)) { return fb_mul_one(table, fe_from_mont(fe_load<FrP>(scalars + i0 + e))); });
}

// ---------------------------------------------------------------------------------------------- powers
// out[i] = x^i, i < n (coarse Montgomery values)
__global__ void __launch_bounds__(256) k_fb_powers(Fr* __restrict__ out, size_t n, FbFrArg xa)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t i0 = t * FB_POW_E;
    if (i0 >= n) return;
    const Fr x = fb_words<FrP>(xa.v);
    Fr g = Fr::one(), sq = x;
    for (size_t e = i0; e; e >>= 1) {
        if (e & 1) g = fe_mul(g, sq);
        sq = fe_sqr(sq);
    }
    for (int e = 0; e < FB_POW_E && i0 + e < n; e++) {
        fe_store<FrP>(out + i0 + e, g);
        g = fe_mul(g, x);
    }
}

// ---------------------------------------------------------------------------------------------- host side
// Fq on the host, for the one point a call is given: Montgomery products on 4 x 64-bit limbs
namespace {
typedef unsigned __int128 u128;

struct HostFq {
    uint64_t p[4], one[4], inv; // modulus, R mod p, -p^-1 mod 2^64
    HostFq()
    {
        for (int i = 0; i < 4; i++) {
            p[i] = (uint64_t)FqP::MOD[2 * i] | ((uint64_t)FqP::MOD[2 * i + 1] << 32);
            one[i] = (uint64_t)FqP::ONE[2 * i] | ((uint64_t)FqP::ONE[2 * i + 1] << 32);
        }
        uint64_t x = 1;
        for (int i = 0; i < 6; i++) x *= 2 - p[0] * x; // Newton: p[0]^-1 mod 2^64
        inv = 0 - x;
    }
    static bool geq(const uint64_t* a, const uint64_t* b)
    {
        for (int i = 3; i >= 0; i--)
            if (a[i] != b[i]) return a[i] > b[i];
        return true;
    }
    static void sub(uint64_t* a, const uint64_t* b)
    {
        uint64_t br = 0;
        for (int i = 0; i < 4; i++) {
            const u128 d = (u128)a[i] - b[i] - br;
            a[i] = (uint64_t)d;
            br = (uint64_t)(d >> 64) & 1;
        }
    }
    // [0, 2p) -> [0, p); false when the value is 2p or more
    bool canon(uint64_t* a) const
    {
        if (geq(a, p)) sub(a, p);
        return !geq(a, p);
    }
    void add(uint64_t* r, const uint64_t* a, const uint64_t* b) const // canonical in, canonical out (2p < 2^255: no carry out)
    {
        u128 c = 0;
        for (int i = 0; i < 4; i++) {
            c += (u128)a[i] + b[i];
            r[i] = (uint64_t)c;
            c >>= 64;
        }
        if (geq(r, p)) sub(r, p);
    }
    void mul(uint64_t* r, const uint64_t* a, const uint64_t* b) const // a b / 2^256 mod p, canonical in and out
    {
        uint64_t t[6] = { 0, 0, 0, 0, 0, 0 };
        for (int i = 0; i < 4; i++) {
            u128 c = 0;
            for (int j = 0; j < 4; j++) {
                c += (u128)a[j] * b[i] + t[j];
                t[j] = (uint64_t)c;
                c >>= 64;
            }
            c += t[4];
            t[4] = (uint64_t)c;
            t[5] = (uint64_t)(c >> 64);
            const uint64_t m = t[0] * inv;
            c = ((u128)m * p[0] + t[0]) >> 64;
            for (int j = 1; j < 4; j++) {
                c += (u128)m * p[j] + t[j];
                t[j - 1] = (uint64_t)c;
                c >>= 64;
            }
            c += t[4];
            t[3] = (uint64_t)c;
            t[4] = t[5] + (uint64_t)(c >> 64);
        }
        for (int i = 0; i < 4; i++) r[i] = t[i];
        if (t[4] || geq(r, p)) sub(r, p);
    }
};

// base_affine (host, NULL = the generator) -> its canonical bytes in key[8]; BBG_E_INVALID unless it is the point at infinity in the
// reference's encoding or a point of y^2 = x^3 + 3 with both coordinates below 2p
int fb_canonical_base(const uint64_t* base_affine, uint64_t key[8])
{
    static const HostFq F;
    if (!base_affine) { // G = (1, 2)
        memcpy(key, F.one, 32);
        F.add(key + 4, F.one, F.one);
        return BBG_OK;
    }
    if (base_affine[3] >> 63) { // infinity: every multiple is infinite
        memset(key, 0, 64);
        key[3] = (uint64_t)1 << 63;
        return BBG_OK;
    }
    memcpy(key, base_affine, 64);
    if (!F.canon(key) || !F.canon(key + 4)) {
        set_error("bbg_g1_fixed_base_mul: a coordinate of the base point is not below 2p");
        return BBG_E_INVALID;
    }
    uint64_t yy[4], xx[4], rhs[4], three[4];
    F.mul(yy, key + 4, key + 4);
    F.mul(xx, key, key);
    F.mul(rhs, xx, key);
    F.add(three, F.one, F.one);
    F.add(three, three, F.one);
    F.add(rhs, rhs, three);
    if (memcmp(yy, rhs, 32) != 0) {
        set_error("bbg_g1_fixed_base_mul: the base point is not on the curve y^2 = x^3 + 3");
        return BBG_E_INVALID;
    }
    return BBG_OK;
}
} // namespace

// out[i] = scalars[i] * B on `st`.  base_affine: host, NULL = G.  Builds (or rebuilds, for another base) the context's table first.
int fixed_base_mul(bbg_ctx* ctx, const uint64_t* base_affine, const void* d_scalars, size_t n, void* d_out, hipStream_t st)
{
    uint64_t key[8];
    int rc = fb_canonical_base(base_affine, key);
    if (rc) return rc;
    if (n == 0) return BBG_OK;
    if (!ctx->fb_table.p) ctx->fb_table_valid = false;
    rc = ctx->fb_table.ensure(FB_TABLE_BYTES);
    if (rc) return rc;
    if (!ctx->fb_table_valid || memcmp(ctx->fb_table_key, key, 64) != 0) {
        ProfScope ps(ctx, "fixed_base_table", st);
        FbAffArg b;
        memcpy(b.v, key, 64);
        hipLaunchKernelGGL(k_fb_table, dim3(FB_WINDOWS), dim3(256), 0, st, (Affine*)ctx->fb_table.p, b);
        memcpy(ctx->fb_table_key, key, 64);
        ctx->fb_table_valid = true;
    }
    {
        ProfScope ps(ctx, "fixed_base_mul", st);
        hipLaunchKernelGGL(k_fb_mul, dim3(grid_for((n + FB_CH - 1) / FB_CH, 64)), dim3(64), 0, st, (const Affine*)ctx->fb_table.p, (const Fr*)d_scalars, n,
                           (Affine*)d_out);
    }
    BBG_HIP(hipGetLastError());
    return BBG_OK;
}

// d_out[i] = x^i, i < n (Montgomery Fr, coarse) on `st`; x: host words
int fixed_base_powers(const uint64_t x[4], size_t n, void* d_out, hipStream_t st)
{
    if (n == 0) return BBG_OK;
    FbFrArg xa;
    memcpy(xa.v, x, 32);
    hipLaunchKernelGGL(k_fb_powers, dim3(grid_for((n + FB_POW_E - 1) / FB_POW_E, 256)), dim3(256), 0, st, (Fr*)d_out, n, xa);
    BBG_HIP(hipGetLastError());
    return BBG_OK;
}

} // namespace bbg
