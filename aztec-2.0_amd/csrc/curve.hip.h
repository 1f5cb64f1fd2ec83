// BN254 G1 (y^2 = x^3 + 3) group arithmetic for gfx950, on top of field.hip.h.
//
// The reference works in Jacobian coordinates (ecc/groups/element_impl.hpp:70-441: self_dbl, operator+=(affine),
// operator+=(element)).  On the GPU the bucket sums use extended Jacobian "XYZZ" coordinates
// (x = X/ZZ, y = Y/ZZZ, ZZ^3 = ZZZ^2): a mixed addition is 8M + 2S instead of 7M + 4S, with no field inversion,
// and -- unlike the reference's affine trick (scalar_multiplication.cpp:305-340) -- no batch inversion pass.
// The group element computed is the same; only the boundary converts back to the reference's 96-byte Jacobian.
//
// Points at infinity: affine / Jacobian use the reference's convention, bit 63 of x.data[3] == bit 31 of x.v[7]
// (element_impl.hpp:497-516, affine_element_impl.hpp:74-93); XYZZ uses ZZ == 0.
#pragma once
#include "field.hip.h"

namespace bbg {

struct alignas(16) Affine {
    Fq x, y;
};
struct alignas(16) Jacobian {
    Fq x, y, z;
};
struct alignas(16) Xyzz {
    Fq x, y, zz, zzz;
};

__device__ __forceinline__ bool aff_is_inf(const Affine& p) { return (p.x.v[7] >> 31) != 0; }
__device__ __forceinline__ Affine aff_inf()
{
    Affine r;
    r.x = Fq::zero();
    r.y = Fq::zero();
    r.x.v[7] = 0x80000000u;
    return r;
}
// the generator G = (1, 2), Montgomery form, canonical
__device__ __forceinline__ Affine aff_generator()
{
    Affine g;
    g.x = Fq::one();
    Fq two = Fq::zero();
    two.v[0] = 2;
    g.y = fe_reduce_once(fe_to_mont(two));
    return g;
}
__device__ __forceinline__ Xyzz xyzz_inf()
{
    Xyzz r;
    r.x = Fq::zero();
    r.y = Fq::zero();
    r.zz = Fq::zero();
    r.zzz = Fq::zero();
    return r;
}
__device__ __forceinline__ bool xyzz_is_inf(const Xyzz& p) { return p.zz.is_zero_raw(); }

__device__ __forceinline__ Affine aff_load(const void* p)
{
    Affine r;
    r.x = fe_load<FqP>(p);
    r.y = fe_load<FqP>(reinterpret_cast<const char*>(p) + 32);
    return r;
}
__device__ __forceinline__ void aff_store(void* p, const Affine& a)
{
    fe_store<FqP>(p, a.x);
    fe_store<FqP>(reinterpret_cast<char*>(p) + 32, a.y);
}
__device__ __forceinline__ Xyzz xyzz_load(const void* p)
{
    const char* c = reinterpret_cast<const char*>(p);
    Xyzz r;
    r.x = fe_load<FqP>(c);
    r.y = fe_load<FqP>(c + 32);
    r.zz = fe_load<FqP>(c + 64);
    r.zzz = fe_load<FqP>(c + 96);
    return r;
}
__device__ __forceinline__ void xyzz_store(void* p, const Xyzz& a)
{
    char* c = reinterpret_cast<char*>(p);
    fe_store<FqP>(c, a.x);
    fe_store<FqP>(c + 32, a.y);
    fe_store<FqP>(c + 64, a.zz);
    fe_store<FqP>(c + 96, a.zzz);
}

__device__ __forceinline__ Xyzz xyzz_from_affine(const Affine& p)
{
    Xyzz r;
    r.x = p.x;
    r.y = p.y;
    r.zz = Fq::one();
    r.zzz = Fq::one();
    return r;
}

// 2P for an affine P (mdbl-2008-s-1).  P must not be infinity; y = 0 cannot occur on BN254 G1 (odd prime order).
__device__ __forceinline__ Xyzz xyzz_dbl_affine(const Affine& p)
{
    Fq U = fe_dbl(p.y);
    Fq V = fe_sqr(U);
    Fq W = fe_mul(U, V);
    Fq S = fe_mul(p.x, V);
    Fq xx = fe_sqr(p.x);
    Fq M = fe_add(fe_dbl(xx), xx);
    Xyzz r;
    r.x = fe_sub(fe_sqr(M), fe_dbl(S));
    r.y = fe_mul_sub2(M, fe_sub(S, r.x), W, p.y);
    r.zz = V;
    r.zzz = W;
    return r;
}
// 2P (dbl-2008-s-1), restating element::self_dbl (element_impl.hpp:70-139) in XYZZ form.
__device__ __forceinline__ Xyzz xyzz_dbl(const Xyzz& p)
{
    if (xyzz_is_inf(p)) return p;
    Fq U = fe_dbl(p.y);
    Fq V = fe_sqr(U);
    Fq W = fe_mul(U, V);
    Fq S = fe_mul(p.x, V);
    Fq xx = fe_sqr(p.x);
    Fq M = fe_add(fe_dbl(xx), xx);
    Xyzz r;
    r.x = fe_sub(fe_sqr(M), fe_dbl(S));
    r.y = fe_mul_sub2(M, fe_sub(S, r.x), W, p.y);
    r.zz = fe_mul(V, p.zz);
    r.zzz = fe_mul(W, p.zzz);
    return r;
}
// acc + P, P affine (madd-2008-s), complete: handles acc = inf, P = inf, P = +-acc like
// element::operator+=(affine_element) does (element_impl.hpp:243-330).
__device__ __forceinline__ Xyzz xyzz_madd(const Xyzz& a, const Affine& p)
{
    if (aff_is_inf(p)) return a;
    if (xyzz_is_inf(a)) return xyzz_from_affine(p);
    Fq U2 = fe_mul(p.x, a.zz);
    Fq S2 = fe_mul(p.y, a.zzz);
    Fq P = fe_sub(U2, a.x);
    Fq R = fe_sub(S2, a.y);
    if (fe_is_zero(P)) {
        if (fe_is_zero(R)) return xyzz_dbl_affine(p);
        return xyzz_inf();
    }
    Fq PP = fe_sqr(P);
    Fq PPP = fe_mul(P, PP);
    Fq Q = fe_mul(a.x, PP);
    Xyzz r;
    r.x = fe_sub(fe_sub(fe_sqr(R), PPP), fe_dbl(Q));
    r.y = fe_mul_sub2(R, fe_sub(Q, r.x), a.y, PPP);
    r.zz = fe_mul(a.zz, PP);
    r.zzz = fe_mul(a.zzz, PPP);
    return r;
}
// a + b (add-2008-s), complete like element::operator+=(element) (element_impl.hpp:354-441).
__device__ __forceinline__ Xyzz xyzz_add(const Xyzz& a, const Xyzz& b)
{
    if (xyzz_is_inf(b)) return a;
    if (xyzz_is_inf(a)) return b;
    Fq U1 = fe_mul(a.x, b.zz);
    Fq U2 = fe_mul(b.x, a.zz);
    Fq S1 = fe_mul(a.y, b.zzz);
    Fq S2 = fe_mul(b.y, a.zzz);
    Fq P = fe_sub(U2, U1);
    Fq R = fe_sub(S2, S1);
    if (fe_is_zero(P)) {
        if (fe_is_zero(R)) return xyzz_dbl(a);
        return xyzz_inf();
    }
    Fq PP = fe_sqr(P);
    Fq PPP = fe_mul(P, PP);
    Fq Q = fe_mul(U1, PP);
    Xyzz r;
    r.x = fe_sub(fe_sub(fe_sqr(R), PPP), fe_dbl(Q));
    r.y = fe_mul_sub2(R, fe_sub(Q, r.x), S1, PPP);
    r.zz = fe_mul(fe_mul(a.zz, b.zz), PP);
    r.zzz = fe_mul(fe_mul(a.zzz, b.zzz), PPP);
    return r;
}
// the sum of `v` over the 64 lanes of the wave, in every lane.  Every lane of the wave must call it.
__device__ __forceinline__ Xyzz xyzz_wave_sum(Xyzz v)
{
#pragma unroll 1
    for (int d = 32; d >= 1; d >>= 1) {
        Xyzz o;
#pragma unroll
        for (int w = 0; w < 8; w++) {
            o.x.v[w] = (uint32_t)__shfl_xor((int)v.x.v[w], d, 64);
            o.y.v[w] = (uint32_t)__shfl_xor((int)v.y.v[w], d, 64);
            o.zz.v[w] = (uint32_t)__shfl_xor((int)v.zz.v[w], d, 64);
            o.zzz.v[w] = (uint32_t)__shfl_xor((int)v.zzz.v[w], d, 64);
        }
        v = xyzz_add(v, o);
    }
    return v;
}
// y^2 = x^3 + 3 for a finite point with coordinates in [0, 2p)
__device__ __forceinline__ bool aff_on_curve(const Affine& a)
{
    const Fq three = fe_add(fe_dbl(Fq::one()), Fq::one());
    return fe_eq(fe_sqr(a.y), fe_add(fe_mul(fe_sqr(a.x), a.x), three));
}
// XYZZ -> the reference's Jacobian (X', Y', Z') with x = X'/Z'^2, y = Y'/Z'^3: take Z' = ZZ*ZZZ.
__device__ __forceinline__ Jacobian xyzz_to_jacobian(const Xyzz& p)
{
    Jacobian r;
    if (xyzz_is_inf(p)) {
        r.x = Fq::zero();
        r.y = Fq::zero();
        r.z = Fq::zero();
        r.x.v[7] = 0x80000000u;
        return r;
    }
    Fq z = fe_mul(p.zz, p.zzz);          // Z'
    Fq z2 = fe_sqr(z);                   // Z'^2 = ZZ^2 ZZZ^2
    Fq t = fe_mul(p.zz, fe_sqr(p.zzz));  // ZZ ZZZ^2
    r.x = fe_mul(p.x, t);                // x Z'^2 = X ZZ ZZZ^2
    r.y = fe_mul(fe_mul(p.y, z2), p.zz); // y Z'^3 = Y ZZ^3 ZZZ^2 = Y * Z'^2 * ZZ
    r.z = z;
    return r;
}
__device__ __forceinline__ Xyzz xyzz_from_jacobian(const Jacobian& p)
{
    Xyzz r;
    if ((p.x.v[7] >> 31) != 0) return xyzz_inf();
    r.x = p.x;
    r.y = p.y;
    r.zz = fe_sqr(p.z);
    r.zzz = fe_mul(r.zz, p.z);
    return r;
}
__device__ __forceinline__ Affine aff_neg_if(const Affine& p, bool neg)
{
    Affine r = p;
    Fq ny = fe_neg(p.y);
#pragma unroll
    for (int i = 0; i < 8; i++) r.y.v[i] = neg ? ny.v[i] : p.y.v[i];
    return r;
}

// a^(q-2) in Fq (field::invert, field_impl.hpp:323-329)
__device__ inline Fq fq_invert(const Fq& a)
{
    uint32_t e[8];
#pragma unroll
    for (int i = 0; i < 8; i++) e[i] = FqP::MOD[i];
    e[0] -= 2; // 0xd87cfd47 - 2, no borrow
    Fq acc = Fq::one();
    for (int i = 255; i >= 0; i--) {
        acc = fe_sqr(acc);
        if ((e[i >> 5] >> (i & 31)) & 1) acc = fe_mul(acc, a);
    }
    return acc;
}
// XYZZ -> canonical affine (one inversion): x = X/ZZ, y = Y/ZZZ
__device__ inline Affine xyzz_to_affine(const Xyzz& p)
{
    if (xyzz_is_inf(p)) return aff_inf();
    Fq iz = fq_invert(fe_mul(p.zz, p.zzz)); // 1/(ZZ*ZZZ)
    Affine r;
    r.x = fe_reduce_once(fe_mul(p.x, fe_mul(iz, p.zzz)));
    r.y = fe_reduce_once(fe_mul(p.y, fe_mul(iz, p.zz)));
    return r;
}

// ---------------------------------------------------------------------------------- batched XYZZ -> canonical affine
// A thread's chunk of XYZZ points q_0 .. q_(m-1) becomes canonical affine behind ONE inversion (Montgomery's trick over the
// zw_e = ZZ_e ZZZ_e), without an XYZZ working set.  Every kernel that converts more than one point per thread goes through these three:
//
//     Fq run = Fq::one();
//     for e = 0 .. m-1:    fin[e] = aff_batch_park(q_e, slot_e, zw[e], prefix[e], run);    // ascending
//     Fq inv = aff_batch_invert(run);
//     for e = m-1 .. 0:    aff_batch_finish(slot_e, fin[e], zw[e], prefix[e], inv, aff_inf());   // DEscending
//
//   * slot_e is the point's own 64-byte place in the output.  Park stores the numerators X ZZZ and Y ZZ there
//     (x = X / ZZ = X ZZZ / zw, y = Y / ZZZ = Y ZZ / zw); finish reads them back and scales them.  Only zw, the prefix product and the
//     finite flag of each point stay with the thread.  A thread touches its own slots only, and q_e is complete before slot_e is
//     written, so a slot may be the place the point was read from.
//   * Infinite members (ZZ = 0) take no part in the product: zw = 1, nothing is stored, and finish writes `inf_value` (aff_inf(), or
//     whatever the caller's output format wants) instead.  run is therefore a product of non-zero values and the inversion is defined
//     for every mix of finite and infinite members, the all-infinite chunk included (run = 1).
//   * Order: prefix[e] = zw_0 .. zw_(e-1) as park saw it.  On entry to finish for e, inv = 1 / (zw_0 .. zw_e); inv prefix[e] = 1 / zw_e,
//     and inv zw_e is what e - 1 needs.  Hence ascending parks, descending finishes, and every parked member finished.
//   * Output: both products are below 2p and go through fe_reduce_once, so the stored words are the canonical representative.
//   * The parked numerators must be RE-READ from memory by finish, not carried in registers across the 380 products of the inversion:
//     aff_batch_invert puts a compiler barrier in front of fq_invert.  It is the only way from park to finish.
__device__ __forceinline__ bool aff_batch_park(const Xyzz& q, Affine* slot, Fq& zw, Fq& prefix, Fq& run)
{
    zw = Fq::one();
    prefix = run;
    if (xyzz_is_inf(q)) return false;
    zw = fe_mul(q.zz, q.zzz);
    Affine s;
    s.x = fe_mul(q.x, q.zzz);
    s.y = fe_mul(q.y, q.zz);
    aff_store(slot, s);
    run = fe_mul(run, zw);
    return true;
}
__device__ __forceinline__ Fq aff_batch_invert(const Fq& run)
{
    asm volatile("" ::: "memory");
    return fq_invert(run);
}
__device__ __forceinline__ void aff_batch_finish(Affine* slot, bool finite, const Fq& zw, const Fq& prefix, Fq& inv, const Affine& inf_value)
{
    Affine o = inf_value;
    if (finite) {
        const Fq iz = fe_mul(inv, prefix); // 1 / zw of this point
        inv = fe_mul(inv, zw);
        const Affine s = aff_load(slot);
        o.x = fe_reduce_once(fe_mul(s.x, iz));
        o.y = fe_reduce_once(fe_mul(s.y, iz));
    }
    aff_store(slot, o);
}
// The same for a chunk of up to four points out[0 .. cnt-1], cnt >= 1, spelt out point by point so that every index is a constant and
// the four zw, the four prefix products and the flags are registers, not a runtime-indexed array.  produce(e) returns point e; it runs
// before slot e is written.
template <class Produce> __device__ __forceinline__ void aff_batch_chunk4(Affine* out, int cnt, Produce produce)
{
    Fq zw0, zw1, zw2, zw3, pf0, pf1, pf2, pf3;
    Fq run = Fq::one();
    bool f0 = false, f1 = false, f2 = false, f3 = false;
    f0 = aff_batch_park(produce(0), out, zw0, pf0, run);
    if (cnt > 1) f1 = aff_batch_park(produce(1), out + 1, zw1, pf1, run);
    if (cnt > 2) f2 = aff_batch_park(produce(2), out + 2, zw2, pf2, run);
    if (cnt > 3) f3 = aff_batch_park(produce(3), out + 3, zw3, pf3, run);
    Fq inv = aff_batch_invert(run);
    if (cnt > 3) aff_batch_finish(out + 3, f3, zw3, pf3, inv, aff_inf());
    if (cnt > 2) aff_batch_finish(out + 2, f2, zw2, pf2, inv, aff_inf());
    if (cnt > 1) aff_batch_finish(out + 1, f1, zw1, pf1, inv, aff_inf());
    aff_batch_finish(out, f0, zw0, pf0, inv, aff_inf());
}

} // namespace bbg
