// G2 of BN254 on the twist y^2 = x^3 + 3 / (9 + u) for gfx950, on top of fq_tower.hip.h: the affine and Jacobian point types, the group law of
// k_g2_mul and the line functions of the flipped Miller loop (pairing.hip).  A header of its own so that the conformance kernels
// (tower_check.hip, bbg_tower_op) run the same functions as the product.
#pragma once
#include "fq_tower.hip.h"

namespace bbg {

struct alignas(16) G2Aff {
    Fq2 x, y;
};
struct G2Jac {
    Fq2 x, y, z; // z = 0: infinity
};

// ---------------------------------------------------------------------------------------------- G2
__device__ __forceinline__ bool g2_aff_is_inf(const G2Aff& p) { return (p.x.c0.v[7] >> 31) != 0; }
__device__ __forceinline__ G2Aff g2_aff_load(const void* p) { return { f2_load(p), f2_load(reinterpret_cast<const char*>(p) + 64) }; }
// canonical; infinity in the reference's affine encoding applied to x.c0
__device__ __forceinline__ void g2_aff_store(void* p, const G2Aff& a, bool inf)
{
    G2Aff o = { f2_canon(a.x), f2_canon(a.y) };
    if (inf) {
        o.x = f2_zero();
        o.y = f2_zero();
        o.x.c0.v[7] = 0x80000000u;
    }
    f2_store(p, o.x);
    f2_store(reinterpret_cast<char*>(p) + 64, o.y);
}
__device__ __forceinline__ bool g2_on_twist(const G2Aff& a)
{
    Fq2 b;
    BBG_FQ2_CONST(b, PairP::TWIST_B);
    return f2_eq(f2_sqr(a.y), f2_add(f2_mul(f2_sqr(a.x), a.x), b));
}
__device__ __forceinline__ G2Jac g2_dbl(const G2Jac& p) // dbl-2009-l; infinity stays infinity
{
    const Fq2 a = f2_sqr(p.x), b = f2_sqr(p.y), c = f2_sqr(b);
    const Fq2 d = f2_dbl(f2_sub(f2_sub(f2_sqr(f2_add(p.x, b)), a), c));
    const Fq2 e = f2_add(f2_dbl(a), a), f = f2_sqr(e);
    G2Jac r;
    r.x = f2_sub(f, f2_dbl(d));
    r.y = f2_sub(f2_mul(e, f2_sub(d, r.x)), f2_dbl(f2_dbl(f2_dbl(c))));
    r.z = f2_dbl(f2_mul(p.y, p.z));
    return r;
}
__device__ __forceinline__ G2Jac g2_madd(const G2Jac& p, const G2Aff& q) // madd-2007-bl with every exceptional case
{
    if (f2_is_zero(p.z)) return { q.x, q.y, f2_one() };
    const Fq2 zz = f2_sqr(p.z);
    const Fq2 h = f2_sub(f2_mul(q.x, zz), p.x), rr = f2_sub(f2_mul(f2_mul(q.y, p.z), zz), p.y);
    if (f2_is_zero(h)) {
        if (f2_is_zero(rr)) return g2_dbl(p);
        return { f2_one(), f2_one(), f2_zero() };
    }
    const Fq2 hh = f2_sqr(h), i = f2_dbl(f2_dbl(hh)), j = f2_mul(h, i), r2 = f2_dbl(rr), v = f2_mul(p.x, i);
    G2Jac r;
    r.x = f2_sub(f2_sub(f2_sqr(r2), j), f2_dbl(v));
    r.y = f2_sub(f2_mul(r2, f2_sub(v, r.x)), f2_dbl(f2_mul(p.y, j)));
    r.z = f2_sub(f2_sub(f2_sqr(f2_add(p.z, h)), zz), hh);
    return r;
}

// ---------------------------------------------------------------------------------------------- lines
__device__ __forceinline__ void line_store(char* p, const Fq2& o, const Fq2& vw, const Fq2& vv)
{
    f2_store(p, f2_canon(o));
    f2_store(p + 64, f2_canon(vw));
    f2_store(p + 128, f2_canon(vv));
}
// doubling_step_for_flipped_miller_loop (pairing_impl.hpp:23-60)
__device__ __forceinline__ void line_double(G2Jac& cur, char* line)
{
    Fq two_inv;
    BBG_FQ_CONST(two_inv, PairP::TWO_INV);
    Fq2 tb;
    BBG_FQ2_CONST(tb, PairP::TWIST_B);
    const Fq2 a = f2_mul(f2_mul_fq(cur.x, two_inv), cur.y);
    const Fq2 b = f2_sqr(cur.y), c = f2_sqr(cur.z);
    const Fq2 e = f2_mul(f2_add(f2_dbl(c), c), tb);
    const Fq2 f = f2_add(f2_dbl(e), e);
    const Fq2 g = f2_mul_fq(f2_add(b, f), two_inv);
    const Fq2 h = f2_sub(f2_sqr(f2_add(cur.y, cur.z)), f2_add(b, c));
    const Fq2 i = f2_sub(e, b), j = f2_sqr(cur.x), ee = f2_sqr(e);
    cur.x = f2_mul(a, f2_sub(b, f));
    cur.y = f2_sub(f2_sqr(g), f2_add(f2_dbl(ee), ee));
    cur.z = f2_mul(b, h);
    line_store(line, f2_mul_xi(i), f2_neg(h), f2_add(f2_dbl(j), j));
}
// mixed_addition_step_for_flipped_miller_loop (:62-97)
__device__ __forceinline__ void line_add(const G2Aff& base, G2Jac& cur, char* line)
{
    const Fq2 d = f2_sub(cur.x, f2_mul(base.x, cur.z)), e = f2_sub(cur.y, f2_mul(base.y, cur.z));
    const Fq2 f = f2_sqr(d), g = f2_sqr(e), h = f2_mul(d, f), i = f2_mul(cur.x, f);
    const Fq2 j = f2_sub(f2_sub(f2_add(f2_mul(cur.z, g), h), i), i);
    cur.x = f2_mul(d, j);
    cur.y = f2_sub(f2_mul(f2_sub(i, j), e), f2_mul(cur.y, h));
    cur.z = f2_mul(cur.z, h);
    line_store(line, f2_mul_xi(f2_sub(f2_mul(e, base.x), f2_mul(d, base.y))), d, f2_neg(e));
}
__device__ __forceinline__ G2Aff g2_mul_by_q(const G2Aff& a)
{
    Fq2 cx, cy;
    BBG_FQ2_CONST(cx, PairP::TWIST_MUL_BY_Q_X);
    BBG_FQ2_CONST(cy, PairP::TWIST_MUL_BY_Q_Y);
    return { f2_mul(cx, f2_conj(a.x)), f2_mul(cy, f2_conj(a.y)) };
}

} // namespace bbg
