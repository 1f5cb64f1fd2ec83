// The extension tower of BN254 for gfx950, on top of field.hip.h: Fq2 = Fq[u]/(u^2 + 1), Fq6 = Fq2[v]/(v^3 - xi) with xi = 9 + u,
// Fq12 = Fq6[w]/(w^2 - v) -- the reference's field2 / field6 / field12 (ecc/fields/field2.hpp, field6.hpp, field12.hpp) in its memory
// layouts: fq2 = c0 | c1 (64 B), fq6 = c0 | c1 | c2, fq12 = c0 | c1 (384 B), Montgomery form.  Every coefficient is kept coarsely reduced in
// the CLOSED interval [0, 2p] (fe_neg maps 0 to 2p) and canonicalised at the boundary (f2_canon, f12_store).  field.hip.h states fe_add and
// fe_sub for [0, 2p); both are closed on [0, 2p] too (the chains of addsub_chains.hip.h subtract 2p where a + b >= 2p and add it back on a
// borrow: 2p + 2p -> 2p, 2p - 0 -> 2p, nothing above), fe_mul of operands <= 2p is below 2p, and fe_inverse_gcd canonicalises anything below
// 4p.  What does NOT take the value 2p is a single fe_reduce_once (2p -> p) and with it fe_is_zero: zero tests here go through fq_canon, which
// reduces twice.  tests/test_gpu_tower.py holds every function below to this contract on raw operands (bbg_tower_op).  An Fq2 product is three
// Fq products (Karatsuba), an Fq6 product six Fq2 products, an Fq12 product three Fq6 products: 54 Fq products.  Constants:
// pairing_consts.hip.h, generated from the integer model.
#pragma once
#include "field.hip.h"
#include "pairing_consts.hip.h"

namespace bbg {

struct alignas(16) Fq2 {
    Fq c0, c1;
};
struct alignas(16) Fq6 {
    Fq2 c0, c1, c2;
};
struct alignas(16) Fq12 {
    Fq6 c0, c1;
};

// a generated constant (eight 32-bit limbs) as an Fq; ARR names a constexpr array, so every limb is an immediate
#define BBG_FQ_CONST(dst, ARR)                                                                                        \
    do {                                                                                                              \
        _Pragma("unroll") for (int _i = 0; _i < 8; _i++)(dst).v[_i] = ARR[_i];                                        \
    } while (0)
#define BBG_FQ2_CONST(dst, ARR)                                                                                       \
    do {                                                                                                              \
        BBG_FQ_CONST((dst).c0, ARR[0]);                                                                               \
        BBG_FQ_CONST((dst).c1, ARR[1]);                                                                               \
    } while (0)

__device__ __forceinline__ Fq fq_canon(const Fq& a) { return fe_reduce_once(fe_reduce_once(a)); } // [0, 2p] -> canonical

// ------------------------------------------------------------------------------------------------ Fq2
__device__ __forceinline__ Fq2 f2_zero() { return { Fq::zero(), Fq::zero() }; }
__device__ __forceinline__ Fq2 f2_one() { return { Fq::one(), Fq::zero() }; }
__device__ __forceinline__ Fq2 f2_add(const Fq2& a, const Fq2& b) { return { fe_add(a.c0, b.c0), fe_add(a.c1, b.c1) }; }
__device__ __forceinline__ Fq2 f2_sub(const Fq2& a, const Fq2& b) { return { fe_sub(a.c0, b.c0), fe_sub(a.c1, b.c1) }; }
__device__ __forceinline__ Fq2 f2_neg(const Fq2& a) { return { fe_neg(a.c0), fe_neg(a.c1) }; }
__device__ __forceinline__ Fq2 f2_dbl(const Fq2& a) { return { fe_dbl(a.c0), fe_dbl(a.c1) }; }
__device__ __forceinline__ Fq2 f2_conj(const Fq2& a) { return { a.c0, fe_neg(a.c1) }; } // the Frobenius map of Fq2
__device__ __forceinline__ Fq2 f2_mul(const Fq2& a, const Fq2& b)
{
    const Fq t0 = fe_mul(a.c0, b.c0), t1 = fe_mul(a.c1, b.c1);
    const Fq t2 = fe_mul(fe_add(a.c0, a.c1), fe_add(b.c0, b.c1));
    return { fe_sub(t0, t1), fe_sub(t2, fe_add(t0, t1)) };
}
__device__ __forceinline__ Fq2 f2_sqr(const Fq2& a)
{
    const Fq t = fe_mul(a.c0, a.c1);
    return { fe_mul(fe_add(a.c0, a.c1), fe_sub(a.c0, a.c1)), fe_dbl(t) };
}
__device__ __forceinline__ Fq2 f2_mul_fq(const Fq2& a, const Fq& k) { return { fe_mul(a.c0, k), fe_mul(a.c1, k) }; }
// times the non-residue xi = 9 + u: (9 a0 - a1, 9 a1 + a0)
__device__ __forceinline__ Fq2 f2_mul_xi(const Fq2& a)
{
    const Fq n0 = fe_add(fe_dbl(fe_dbl(fe_dbl(a.c0))), a.c0), n1 = fe_add(fe_dbl(fe_dbl(fe_dbl(a.c1))), a.c1);
    return { fe_sub(n0, a.c1), fe_add(n1, a.c0) };
}
// one Fq inversion (of the norm); 0 -> 0
__device__ __forceinline__ Fq2 f2_inv(const Fq2& a)
{
    const Fq t = fe_inverse_gcd<FqP>(fe_add(fe_sqr(a.c0), fe_sqr(a.c1)));
    return { fe_mul(a.c0, t), fe_neg(fe_mul(a.c1, t)) };
}
__device__ __forceinline__ Fq2 f2_canon(const Fq2& a) { return { fq_canon(a.c0), fq_canon(a.c1) }; }
__device__ __forceinline__ bool f2_is_zero(const Fq2& a) { return fq_canon(a.c0).is_zero_raw() && fq_canon(a.c1).is_zero_raw(); }
__device__ __forceinline__ bool f2_eq(const Fq2& a, const Fq2& b) { return f2_is_zero(f2_sub(a, b)); }
__device__ __forceinline__ Fq2 f2_load(const void* p)
{
    return { fe_load<FqP>(p), fe_load<FqP>(reinterpret_cast<const char*>(p) + 32) };
}
__device__ __forceinline__ void f2_store(void* p, const Fq2& a)
{
    fe_store<FqP>(p, a.c0);
    fe_store<FqP>(reinterpret_cast<char*>(p) + 32, a.c1);
}

// ------------------------------------------------------------------------------------------------ Fq6
__device__ __forceinline__ Fq6 f6_zero() { return { f2_zero(), f2_zero(), f2_zero() }; }
__device__ __forceinline__ Fq6 f6_one() { return { f2_one(), f2_zero(), f2_zero() }; }
__device__ __forceinline__ Fq6 f6_add(const Fq6& a, const Fq6& b) { return { f2_add(a.c0, b.c0), f2_add(a.c1, b.c1), f2_add(a.c2, b.c2) }; }
__device__ __forceinline__ Fq6 f6_sub(const Fq6& a, const Fq6& b) { return { f2_sub(a.c0, b.c0), f2_sub(a.c1, b.c1), f2_sub(a.c2, b.c2) }; }
__device__ __forceinline__ Fq6 f6_neg(const Fq6& a) { return { f2_neg(a.c0), f2_neg(a.c1), f2_neg(a.c2) }; }
// times v, the non-residue of Fq12 over Fq6 (field12::mul_by_non_residue)
__device__ __forceinline__ Fq6 f6_mul_v(const Fq6& a) { return { f2_mul_xi(a.c2), a.c0, a.c1 }; }
// Karatsuba (field6.hpp operator*): six Fq2 products
__device__ __forceinline__ Fq6 f6_mul(const Fq6& a, const Fq6& b)
{
    const Fq2 t0 = f2_mul(a.c0, b.c0), t1 = f2_mul(a.c1, b.c1), t2 = f2_mul(a.c2, b.c2);
    const Fq2 t3 = f2_mul(f2_add(a.c0, a.c2), f2_add(b.c0, b.c2));
    const Fq2 t4 = f2_mul(f2_add(a.c0, a.c1), f2_add(b.c0, b.c1));
    const Fq2 t5 = f2_mul(f2_add(a.c1, a.c2), f2_add(b.c1, b.c2));
    return { f2_add(t0, f2_mul_xi(f2_sub(t5, f2_add(t1, t2)))), f2_add(f2_sub(t4, f2_add(t0, t1)), f2_mul_xi(t2)), f2_sub(f2_add(t3, t1), f2_add(t0, t2)) };
}
// CH-SQR2 (field6.hpp sqr): two Fq2 products and three squarings
__device__ __forceinline__ Fq6 f6_sqr(const Fq6& a)
{
    const Fq2 s0 = f2_sqr(a.c0), s1 = f2_dbl(f2_mul(a.c0, a.c1)), s2 = f2_sqr(f2_sub(f2_add(a.c0, a.c2), a.c1));
    const Fq2 s3 = f2_dbl(f2_mul(a.c1, a.c2)), s4 = f2_sqr(a.c2);
    return { f2_add(f2_mul_xi(s3), s0), f2_add(f2_mul_xi(s4), s1), f2_sub(f2_sub(f2_add(f2_add(s1, s2), s3), s0), s4) };
}
// field6.hpp invert: one Fq2 inversion
__device__ __forceinline__ Fq6 f6_inv(const Fq6& a)
{
    const Fq2 c0 = f2_sub(f2_sqr(a.c0), f2_mul_xi(f2_mul(a.c1, a.c2)));
    const Fq2 c1 = f2_sub(f2_mul_xi(f2_sqr(a.c2)), f2_mul(a.c0, a.c1));
    const Fq2 c2 = f2_sub(f2_sqr(a.c1), f2_mul(a.c0, a.c2));
    const Fq2 t = f2_inv(f2_add(f2_mul(a.c0, c0), f2_mul_xi(f2_add(f2_mul(a.c2, c1), f2_mul(a.c1, c2)))));
    return { f2_mul(t, c0), f2_mul(t, c1), f2_mul(t, c2) };
}

// ------------------------------------------------------------------------------------------------ Fq12
__device__ __forceinline__ Fq12 f12_one() { return { f6_one(), f6_zero() }; }
__device__ __forceinline__ Fq12 f12_mul(const Fq12& a, const Fq12& b)
{
    const Fq6 t0 = f6_mul(a.c0, b.c0), t1 = f6_mul(a.c1, b.c1);
    const Fq6 t2 = f6_mul(f6_add(a.c0, a.c1), f6_add(b.c0, b.c1));
    return { f6_add(f6_mul_v(t1), t0), f6_sub(t2, f6_add(t0, t1)) };
}
__device__ __forceinline__ Fq12 f12_sqr(const Fq12& a)
{
    const Fq6 t1 = f6_mul(a.c0, a.c1);
    const Fq6 t0 = f6_mul(f6_add(a.c0, a.c1), f6_add(f6_mul_v(a.c1), a.c0));
    return { f6_sub(t0, f6_add(t1, f6_mul_v(t1))), f6_add(t1, t1) };
}
// the inverse of an element of the cyclotomic subgroup (norm one over Fq6): the conjugate (field12::unitary_inverse)
__device__ __forceinline__ Fq12 f12_conj(const Fq12& a) { return { a.c0, f6_neg(a.c1) }; }
// field12.hpp invert: ONE Fq inversion in all (Fq12 -> Fq6 -> Fq2 -> Fq); 0 -> 0
__device__ __forceinline__ Fq12 f12_inv(const Fq12& a)
{
    const Fq6 t = f6_inv(f6_sub(f6_sqr(a.c0), f6_mul_v(f6_sqr(a.c1))));
    return { f6_mul(a.c0, t), f6_neg(f6_mul(a.c1, t)) };
}
// The square of an element of the cyclotomic subgroup (what the easy part of the final exponentiation leaves) by Granger and Scott,
// "Faster squaring in the cyclotomic subgroup of sixth degree extensions": the element is three Fq4 = Fq2[s]/(s^2 - xi) pairs
// (c0.c0, c1.c1), (c1.c0, c0.c2), (c0.c1, c1.c2), each squared on its own: six Fq2 products instead of twelve.  The reference's
// cyclotomic_squared() is its plain sqr(); on the subgroup the two are the same element.
__device__ __forceinline__ void f4_sqr(const Fq2& a, const Fq2& b, Fq2& t0, Fq2& t1) // (a + b s)^2 = t0 + t1 s
{
    const Fq2 m = f2_mul(a, b);
    t0 = f2_sub(f2_mul(f2_add(a, b), f2_add(f2_mul_xi(b), a)), f2_add(m, f2_mul_xi(m)));
    t1 = f2_dbl(m);
}
__device__ __forceinline__ Fq2 f2_3t_minus_2z(const Fq2& t, const Fq2& z) { return f2_add(f2_dbl(f2_sub(t, z)), t); }
__device__ __forceinline__ Fq2 f2_3t_plus_2z(const Fq2& t, const Fq2& z) { return f2_add(f2_dbl(f2_add(t, z)), t); }
__device__ __forceinline__ Fq12 f12_cyclotomic_sqr(const Fq12& a)
{
    Fq2 t0, t1, t2, t3, t4, t5;
    f4_sqr(a.c0.c0, a.c1.c1, t0, t1);
    f4_sqr(a.c1.c0, a.c0.c2, t2, t3);
    f4_sqr(a.c0.c1, a.c1.c2, t4, t5);
    Fq12 r;
    r.c0.c0 = f2_3t_minus_2z(t0, a.c0.c0);
    r.c1.c1 = f2_3t_plus_2z(t1, a.c1.c1);
    r.c1.c0 = f2_3t_plus_2z(f2_mul_xi(t5), a.c1.c0);
    r.c0.c2 = f2_3t_minus_2z(t4, a.c0.c2);
    r.c0.c1 = f2_3t_minus_2z(t2, a.c0.c1);
    r.c1.c2 = f2_3t_plus_2z(t3, a.c1.c2);
    return r;
}
// x^(p^k), k = 1, 2, 3 (uniform): component j of the result is PAIR_FROB[k - 1][j - 1] times component j of x, conjugated for odd k
__device__ __forceinline__ Fq2 f12_frob_part(const Fq2& x, int k, int j)
{
    const Fq2 c = f2_load(&PAIR_FROB[k - 1][j - 1][0]);
    return f2_mul(c, (k & 1) ? f2_conj(x) : x);
}
__device__ __forceinline__ Fq12 f12_frobenius(const Fq12& a, int k)
{
    Fq12 r;
    r.c0.c0 = (k & 1) ? f2_conj(a.c0.c0) : a.c0.c0;
    r.c0.c1 = f12_frob_part(a.c0.c1, k, 1);
    r.c0.c2 = f12_frob_part(a.c0.c2, k, 2);
    r.c1.c0 = f12_frob_part(a.c1.c0, k, 3);
    r.c1.c1 = f12_frob_part(a.c1.c1, k, 4);
    r.c1.c2 = f12_frob_part(a.c1.c2, k, 5);
    return r;
}
// a times the sparse element (o, 0, vv) + w (0, vw, 0) that a line evaluates to: field12::self_sparse_mul, 13 Fq2 products
__device__ __forceinline__ Fq12 f12_sparse_mul(const Fq12& a, const Fq2& o, const Fq2& vw, const Fq2& vv)
{
    Fq12 r;
    const Fq2 d0 = f2_mul(a.c0.c0, o), d2 = f2_mul(a.c0.c2, vv), d4 = f2_mul(a.c1.c1, vw);
    const Fq2 t2 = f2_add(a.c0.c0, a.c1.c1), t1 = f2_add(a.c0.c0, a.c0.c2);
    const Fq2 s0 = f2_add(f2_add(a.c0.c1, a.c1.c0), a.c1.c2);
    Fq2 s1 = f2_mul(a.c0.c1, vv);
    Fq2 t3 = f2_add(s1, d4);
    r.c0.c0 = f2_add(f2_mul_xi(t3), d0);
    t3 = f2_mul(a.c1.c2, vw);
    s1 = f2_add(s1, t3);
    t3 = f2_add(t3, d2);
    Fq2 t4 = f2_mul_xi(t3);
    t3 = f2_mul(a.c0.c1, o);
    s1 = f2_add(s1, t3);
    r.c0.c1 = f2_add(t4, t3);
    t3 = f2_sub(f2_sub(f2_mul(t1, f2_add(o, vv)), d0), d2);
    t4 = f2_mul(a.c1.c0, vw);
    s1 = f2_add(s1, t4);
    r.c0.c2 = f2_add(t3, t4);
    t3 = f2_sub(f2_sub(f2_mul(f2_add(a.c0.c2, a.c1.c1), f2_add(vv, vw)), d2), d4);
    t4 = f2_mul_xi(t3);
    t3 = f2_mul(a.c1.c0, o);
    s1 = f2_add(s1, t3);
    r.c1.c0 = f2_add(t3, t4);
    t3 = f2_mul(a.c1.c2, vv);
    s1 = f2_add(s1, t3);
    t4 = f2_mul_xi(t3);
    t3 = f2_sub(f2_sub(f2_mul(f2_add(o, vw), t2), d0), d4);
    r.c1.c1 = f2_add(t3, t4);
    r.c1.c2 = f2_sub(f2_mul(s0, f2_add(f2_add(o, vv), vw)), s1);
    return r;
}
__device__ __forceinline__ bool f12_is_one(const Fq12& a)
{
    Fq one = Fq::one();
    return fe_is_zero(fe_sub(fq_canon(a.c0.c0.c0), one)) && fq_canon(a.c0.c0.c1).is_zero_raw() && f2_is_zero(a.c0.c1) && f2_is_zero(a.c0.c2) &&
           f2_is_zero(a.c1.c0) && f2_is_zero(a.c1.c1) && f2_is_zero(a.c1.c2);
}
// the reference's 384 bytes, canonical
__device__ __forceinline__ void f12_store(void* p, const Fq12& a)
{
    char* c = reinterpret_cast<char*>(p);
    f2_store(c, f2_canon(a.c0.c0));
    f2_store(c + 64, f2_canon(a.c0.c1));
    f2_store(c + 128, f2_canon(a.c0.c2));
    f2_store(c + 192, f2_canon(a.c1.c0));
    f2_store(c + 256, f2_canon(a.c1.c1));
    f2_store(c + 320, f2_canon(a.c1.c2));
}

// The working memory of the pairing kernels holds Fq12 values lane-interleaved: the twelve coefficients of product i in slot s lie at
// work[((s 12 + k) 2 + h) stride + i], 16 bytes each (k: coefficient, h: its low / high half), so a wave's loads and stores are contiguous.
__device__ __forceinline__ Fq fq_load_lanes(const uint4* w, size_t stride)
{
    const uint4 lo = w[0], hi = w[stride];
    Fq r;
    r.v[0] = lo.x; r.v[1] = lo.y; r.v[2] = lo.z; r.v[3] = lo.w;
    r.v[4] = hi.x; r.v[5] = hi.y; r.v[6] = hi.z; r.v[7] = hi.w;
    return r;
}
__device__ __forceinline__ void fq_store_lanes(uint4* w, size_t stride, const Fq& a)
{
    w[0] = make_uint4(a.v[0], a.v[1], a.v[2], a.v[3]);
    w[stride] = make_uint4(a.v[4], a.v[5], a.v[6], a.v[7]);
}
__device__ __forceinline__ Fq2 f2_load_lanes(const uint4* w, size_t stride) { return { fq_load_lanes(w, stride), fq_load_lanes(w + 2 * stride, stride) }; }
__device__ __forceinline__ void f2_store_lanes(uint4* w, size_t stride, const Fq2& a)
{
    fq_store_lanes(w, stride, a.c0);
    fq_store_lanes(w + 2 * stride, stride, a.c1);
}
__device__ __forceinline__ Fq12 f12_load_lanes(const uint4* work, size_t stride, unsigned slot, size_t i)
{
    const uint4* w = work + (size_t)slot * 24 * stride + i;
    Fq12 r;
    r.c0.c0 = f2_load_lanes(w, stride);
    r.c0.c1 = f2_load_lanes(w + 4 * stride, stride);
    r.c0.c2 = f2_load_lanes(w + 8 * stride, stride);
    r.c1.c0 = f2_load_lanes(w + 12 * stride, stride);
    r.c1.c1 = f2_load_lanes(w + 16 * stride, stride);
    r.c1.c2 = f2_load_lanes(w + 20 * stride, stride);
    return r;
}
__device__ __forceinline__ void f12_store_lanes(uint4* work, size_t stride, unsigned slot, size_t i, const Fq12& a)
{
    uint4* w = work + (size_t)slot * 24 * stride + i;
    f2_store_lanes(w, stride, a.c0.c0);
    f2_store_lanes(w + 4 * stride, stride, a.c0.c1);
    f2_store_lanes(w + 8 * stride, stride, a.c0.c2);
    f2_store_lanes(w + 12 * stride, stride, a.c1.c0);
    f2_store_lanes(w + 16 * stride, stride, a.c1.c1);
    f2_store_lanes(w + 20 * stride, stride, a.c1.c2);
}

} // namespace bbg
