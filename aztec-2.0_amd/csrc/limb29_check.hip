// Conformance kernels of the 29-bit-limb arithmetic (bbg_limb29_op, a self-test entry like bbg_field_op): one device primitive of
// field29.hip.h / field29c.hip.h / curve29.hip.h / ntt29.hip.h / w29.hip.h per op, fed RAW lazily reduced operands and returning raw limbs, so
// that tests/test_gpu_limb29.py can hold the device code and the integer models (tests/test_limb29_model.py, test_ntt29_model.py,
// test_w29_model.py, tests/tools/acc29_model.py) to the same nine words at the corners of each contract.
//
// Rules: every op calls the product's own function from the product's own header; nothing is re-implemented here and no operand is adjusted
// on the device.  Preconditions are not checked: a vector outside an op's contract gives wrapped arithmetic (never a fault: a thread reads its
// own rows and writes its own rows; a table row selected past the 32 rows is a read of LDS, not of memory).  One kernel instantiation per (field, op): a switch inside one kernel would put every pair product and the
// radix-8 step into a single register allocation.
//
// Rows are 9 words.  A limb value uses all nine; an 8 x u32 Fe uses words 0..7 and word 8 is written as 0 (ignored on input).
// The op table below is the single definition of the op numbers; tests/tools/limb29_vectors.py restates it and the GPU test compares the two
// through bbg_limb29_op_shape.
#include "bbg_internal.h"
#include "curve29.hip.h"
#include "w29.hip.h"

#include <type_traits>
#include <utility>

namespace bbg {
namespace {

constexpr int L29_ROW = 9;
constexpr int L29_FR = 1, L29_FQ = 2, L29_BOTH = 3;

// X(op, operand rows, result rows, fields)
#define BBG_L29_OPS(X)                                                                                                                           \
    /* representation */                                                                                                                         \
    X(0, 1, 1, L29_BOTH)  /* f29_from_fe<P, 0>: Fe -> limbs */                                                                                    \
    X(1, 1, 1, L29_BOTH)  /* f29_from_fe<P, 5> */                                                                                                 \
    X(2, 1, 1, L29_BOTH)  /* f29_carry */                                                                                                         \
    X(3, 1, 1, L29_BOTH)  /* f29_norm */                                                                                                          \
    X(4, 1, 1, L29_BOTH)  /* f29_to_fe: limbs -> Fe */                                                                                            \
    X(5, 1, 1, L29_BOTH)  /* f29_div32_to_fe */                                                                                                   \
    X(6, 2, 1, L29_BOTH)  /* f29_add */                                                                                                           \
    X(7, 1, 1, L29_FR)    /* w29::up */                                                                                                           \
    /* products */                                                                                                                               \
    X(10, 2, 1, L29_BOTH) /* f29_mul */                                                                                                           \
    X(11, 1, 1, L29_BOTH) /* f29_sqr */                                                                                                           \
    X(12, 4, 1, L29_BOTH) /* f29_mul_sub2(a, b, c, d) */                                                                                          \
    X(13, 2, 1, L29_BOTH) /* f29_mul_ilp */                                                                                                       \
    X(14, 2, 1, L29_BOTH) /* fe_mul29: Fe, Fe -> Fe */                                                                                            \
    X(15, 2, 1, L29_BOTH) /* fe_mul29_ilp */                                                                                                      \
    X(16, 4, 2, L29_BOTH) /* f29_mul2(a1, b1, a2, b2) */                                                                                          \
    X(17, 2, 2, L29_BOTH) /* f29_sqr2(a1, a2) */                                                                                                  \
    X(18, 6, 2, L29_BOTH) /* f29_mul_sub2_mul(a, b, c, d, e, f) */                                                                                \
    X(19, 4, 2, L29_BOTH) /* f29_mul2_z(a1, b1, a2, b2) */                                                                                        \
    X(20, 6, 2, L29_BOTH) /* f29_mul2_add(a1, b1, d1, a2, b2, d2) */                                                                              \
    X(21, 4, 2, L29_BOTH) /* f29_sqr_add_mul(a, d, e, f) */                                                                                       \
    X(22, 6, 2, L29_BOTH) /* f29_mul_sub2_mul_z(a, b, c, d, e, f) */                                                                              \
    X(23, 1, 1, L29_BOTH) /* f29_sqr_z */                                                                                                         \
    /* accumulation */                                                                                                                           \
    X(30, 2, 2, L29_FQ)   /* aff29_from_table(x, y, false): Fe, Fe -> limbs, limbs */                                                             \
    X(31, 2, 2, L29_FQ)   /* aff29_from_table(x, y, true) */                                                                                      \
    X(32, 2, 4, L29_FQ)   /* xyzz29_from_affine */                                                                                                \
    X(33, 6, 4, L29_FQ)   /* xyzz29_madd(X, Y, ZZ, ZZZ; x2, y2) */                                                                                \
    X(34, 4, 5, L29_FQ)   /* xyzz29_finish: four Fe and a row whose word 0 is the returned flag */                                                \
    /* NTT */                                                                                                                                    \
    X(40, 1, 1, L29_FR)   /* ntt29_reduce */                                                                                                      \
    X(41, 1, 1, L29_FR)   /* n29_finish: limbs -> Fe */                                                                                           \
    X(42, 2, 1, L29_FR)   /* n29_finish_mul(x, Fe multiplier) */                                                                                  \
    X(43, 3, 1, L29_FR)   /* f29_mulc(x, {w, wq}) */                                                                                              \
    X(44, 6, 2, L29_FR)   /* f29_mulc2(x1, {w1, wq1}, x2, {w2, wq2}) */                                                                           \
    X(50, 18, 8, L29_FR)  /* n29_step8<0, true>: x[8], w1..w3, tw[1..7] */                                                                        \
    X(51, 11, 8, L29_FR)  /* n29_step8<0, false> */                                                                                               \
    X(52, 28, 8, L29_FR)  /* n29_step8<1, true>: x[8], {w, wq} of w1..w3, {w, wq} of tw[1..7] */                                                  \
    X(53, 14, 8, L29_FR)  /* n29_step8<1, false> */                                                                                               \
    X(54, 9, 8, L29_FR)   /* n29_step4<0>: x[8], w2 */                                                                                            \
    X(55, 10, 8, L29_FR)  /* n29_step4<1> */                                                                                                      \
    X(56, 8, 8, L29_FR)   /* n29_step2 */                                                                                                         \
    X(57, 11, 8, L29_FR)  /* n29_step8_raw<0> */                                                                                                  \
    X(58, 14, 8, L29_FR)  /* n29_step8_raw<1> */                                                                                                  \
    /* typed layer */                                                                                                                            \
    X(60, 10, 1, L29_FR)  /* w29::dot, the five-term gate of k_quotient29_turbo_fixed_base_gate: a0, b0, .., a4, b4 */

// the (M, E) pairs of f29_sub<M, E> (op 100 + i), f29_neg<M, E> (200 + i) and n29_bfly<M, E> (300 + i, Fr): every pair instantiated under csrc/.
// X(index, M, E)
#define BBG_L29_PAIRS(X)                                                                                                                         \
    X(0, 3, 30)   /* n29_bfly<N29M<0>::KP>; w29::sub of a coarse load or a product */                                                            \
    X(1, 4, 30)   /* n29_bfly<4>, <N29M<0>::KPP>, <N29M<1>::KP> */                                                                               \
    X(2, 6, 30)   /* n29_bfly<N29M<1>::KPP> */                                                                                                   \
    X(3, 7, 30)   /* n29_bfly<7> */                                                                                                              \
    X(4, 7, 31)   /* n29_bfly<7, 31> */                                                                                                          \
    X(5, 13, 30)  /* n29_bfly<13> */                                                                                                             \
    X(6, 12, 31)  /* f29_neg<12, 31> (curve29.hip.h) */                                                                                          \
    X(7, 24, 30)  /* f29_sub<24> (curve29.hip.h) */                                                                                              \
    X(8, 34, 30)  /* f29_neg<34> (curve29.hip.h) */                                                                                              \
    X(9, 64, 30)  /* f29_sub<64, 30>, f29_neg<64, 30> (field29.hip.h) */                                                                         \
    X(10, 65, 30) /* w29::sub: M = (B::vq + 63) / 64 + 1, E from B::lm -- subtrahend a class-1 load (V = 64: quad_from, the gate's dsq - 1) */      \
    X(11, 52, 30) /* w29::sub -- subtrahend dbl(e) of the logic widget's tail (quotient29.hip.h logic_part) */
// (w29::sub also instantiates (3, 30): subtrahend a class-0 load, (4, 30): a product, (7, 30): the permutation widget's neg(den))
constexpr int L29_NPAIRS = 12;

template <int I> struct L29Pair;
#define BBG_X(I, MM, EE)                                                                                                                         \
    template <> struct L29Pair<I> {                                                                                                              \
        static constexpr int M = MM, E = EE;                                                                                                     \
    };
BBG_L29_PAIRS(BBG_X)
#undef BBG_X

template <class P> __device__ __forceinline__ F29<P> l29_ld9(const uint32_t* p)
{
    F29<P> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = p[i];
    return r;
}
template <class P> __device__ __forceinline__ Fe<P> l29_ld8(const uint32_t* p)
{
    Fe<P> r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = p[i];
    return r;
}
template <class P> __device__ __forceinline__ void l29_st9(uint32_t* p, const F29<P>& a)
{
#pragma unroll
    for (int i = 0; i < 9; i++) p[i] = a.v[i];
}
template <class P> __device__ __forceinline__ void l29_st8(uint32_t* p, const Fe<P>& a)
{
#pragma unroll
    for (int i = 0; i < 8; i++) p[i] = a.v[i];
    p[8] = 0;
}
__device__ __forceinline__ C29<FrP> l29_ldc(const uint32_t* p) // {w, wq}: two rows
{
    C29<FrP> c;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        c.w[i] = p[i];
        c.q[i] = p[L29_ROW + i];
    }
    return c;
}
template <int SH> __device__ __forceinline__ typename N29M<SH>::Tw l29_ldtw(const uint32_t* p)
{
    if constexpr (SH == 0) return l29_ld9<FrP>(p);
    else return l29_ldc(p);
}

// the operand types of the widest w29::dot of quotient29.hip.h, written with the same expressions as k_quotient29_turbo_fixed_base_gate
// (types only: nothing here is evaluated)
namespace gate {
using namespace w29;
template <class T> const T& v();
using L0 = decltype(ld<0>(v<Fr>()));
using L1 = decltype(ld<1>(v<Fr>()));
using Sq = decltype(sqr(v<L1>()));                                                  // dsq, dx2, xa2
using Acc = decltype(mul(carry(sub(v<Sq>(), v<L1>())), carry(sub(v<Sq>(), v<L1>()))));
using Nw = decltype(carry(neg(v<L0>())));                                           // nw3n, nw2
using M10 = decltype(mul(v<L1>(), v<L0>()));                                        // dy, qd, i1, i2
using Xid = decltype(dot(t(v<L0>(), v<Sq>()), t(v<Nw>(), v<Sq>()), t(v<Nw>(), v<L1>()), t(v<M10>(), v<L1>())));
using Xid17 = decltype(add(v<Xid>(), v<L0>()));
using Ym = decltype(carry(sub(v<L0>(), v<M10>())));
using Yid = decltype(dot(t(v<L0>(), v<L1>()), t(v<Ym>(), v<L1>())));
using I3 = decltype(dot(t(v<L0>(), v<L1>()), t(v<Nw>(), v<L1>())));
using Init = decltype(dot(t(v<M10>(), v<L1>()), t(neg(v<M10>()), v<L1>()), t(v<I3>(), v<L1>())));
} // namespace gate

template <int OP> constexpr bool l29_needs_div32 = OP == 5 || OP == 34;
template <int OP> constexpr bool l29_needs_red = OP == 40 || OP == 41 || OP == 42 || OP == 50 || OP == 51 || OP == 52 || OP == 53;

template <int SH, bool HAVE_TW> __device__ __forceinline__ void l29_step8(const uint32_t* a, uint32_t* r, const uint32_t* red)
{
    constexpr int TW = SH == 0 ? 1 : 2; // rows per multiplier
    Fr29 x[8];
#pragma unroll
    for (int j = 0; j < 8; j++) x[j] = l29_ld9<FrP>(a + j * L29_ROW);
    const uint32_t* w = a + 8 * L29_ROW;
    const uint32_t* tw = w + 3 * TW * L29_ROW; // tw[j] at tw + (j - 1) * TW rows
    n29_step8<SH, HAVE_TW>(x, l29_ldtw<SH>(w), l29_ldtw<SH>(w + TW * L29_ROW), l29_ldtw<SH>(w + 2 * TW * L29_ROW),
                            [&](int j) { return l29_ldtw<SH>(tw + (j - 1) * TW * L29_ROW); }, red);
#pragma unroll
    for (int j = 0; j < 8; j++) l29_st9(r + j * L29_ROW, x[j]);
}
template <int SH, int KIND> __device__ __forceinline__ void l29_last_step(const uint32_t* a, uint32_t* r) // KIND 4: step4, 8: step8_raw
{
    constexpr int TW = SH == 0 ? 1 : 2;
    Fr29 x[8];
#pragma unroll
    for (int j = 0; j < 8; j++) x[j] = l29_ld9<FrP>(a + j * L29_ROW);
    const uint32_t* w = a + 8 * L29_ROW;
    if constexpr (KIND == 4) n29_step4<SH>(x, l29_ldtw<SH>(w));
    else n29_step8_raw<SH>(x, l29_ldtw<SH>(w), l29_ldtw<SH>(w + TW * L29_ROW), l29_ldtw<SH>(w + 2 * TW * L29_ROW));
#pragma unroll
    for (int j = 0; j < 8; j++) l29_st9(r + j * L29_ROW, x[j]);
}

// a: the vector's operand rows, r: its result rows, tbl: the op's LDS table (if it has one)
template <class P, int OP> __device__ __forceinline__ void l29_run(const uint32_t* a, uint32_t* r, const uint32_t* tbl)
{
    constexpr int R = L29_ROW;
    using F = F29<P>;
    if constexpr (OP == 0) l29_st9(r, f29_from_fe<P, 0>(l29_ld8<P>(a)));
    else if constexpr (OP == 1) l29_st9(r, f29_from_fe<P, 5>(l29_ld8<P>(a)));
    else if constexpr (OP == 2) l29_st9(r, f29_carry(l29_ld9<P>(a)));
    else if constexpr (OP == 3) l29_st9(r, f29_norm(l29_ld9<P>(a)));
    else if constexpr (OP == 4) l29_st8(r, f29_to_fe(l29_ld9<P>(a)));
    else if constexpr (OP == 5) l29_st8(r, f29_div32_to_fe(l29_ld9<P>(a), tbl));
    else if constexpr (OP == 6) l29_st9(r, f29_add(l29_ld9<P>(a), l29_ld9<P>(a + R)));
    else if constexpr (OP == 7) {
        // the widest class-0 type up() accepts (top limb below 2^27); the limb arithmetic does not depend on the type
        const w29::W<0, 31 * 64, 0xffffffffull> x{ l29_ld9<FrP>(a) };
        l29_st9(r, w29::up(x).f);
    } else if constexpr (OP == 10) l29_st9(r, f29_mul(l29_ld9<P>(a), l29_ld9<P>(a + R)));
    else if constexpr (OP == 11) l29_st9(r, f29_sqr(l29_ld9<P>(a)));
    else if constexpr (OP == 12) l29_st9(r, f29_mul_sub2(l29_ld9<P>(a), l29_ld9<P>(a + R), l29_ld9<P>(a + 2 * R), l29_ld9<P>(a + 3 * R)));
    else if constexpr (OP == 13) l29_st9(r, f29_mul_ilp(l29_ld9<P>(a), l29_ld9<P>(a + R)));
    else if constexpr (OP == 14) l29_st8(r, fe_mul29(l29_ld8<P>(a), l29_ld8<P>(a + R)));
    else if constexpr (OP == 15) l29_st8(r, fe_mul29_ilp(l29_ld8<P>(a), l29_ld8<P>(a + R)));
    else if constexpr (OP >= 16 && OP <= 22) {
        const F o0 = l29_ld9<P>(a), o1 = l29_ld9<P>(a + R);
        F r1, r2;
        if constexpr (OP == 17) f29_sqr2(o0, o1, r1, r2);
        else {
            const F o2 = l29_ld9<P>(a + 2 * R), o3 = l29_ld9<P>(a + 3 * R);
            if constexpr (OP == 16) f29_mul2(o0, o1, o2, o3, r1, r2);
            else if constexpr (OP == 19) f29_mul2_z(o0, o1, o2, o3, r1, r2);
            else if constexpr (OP == 21) f29_sqr_add_mul(o0, o1, o2, o3, r1, r2);
            else {
                const F o4 = l29_ld9<P>(a + 4 * R), o5 = l29_ld9<P>(a + 5 * R);
                if constexpr (OP == 18) f29_mul_sub2_mul(o0, o1, o2, o3, o4, o5, r1, r2);
                else if constexpr (OP == 20) f29_mul2_add(o0, o1, o2, o3, o4, o5, r1, r2);
                else f29_mul_sub2_mul_z(o0, o1, o2, o3, o4, o5, r1, r2);
            }
        }
        l29_st9(r, r1);
        l29_st9(r + R, r2);
    } else if constexpr (OP == 23) l29_st9(r, f29_sqr_z(l29_ld9<P>(a)));
    else if constexpr (OP == 30 || OP == 31 || OP == 32) {
        Affine p;
        p.x = l29_ld8<FqP>(a);
        p.y = l29_ld8<FqP>(a + R);
        if constexpr (OP == 32) {
            Aff29 q;
            q.x = l29_ld9<FqP>(a);
            q.y = l29_ld9<FqP>(a + R);
            const Xyzz29 s = xyzz29_from_affine(q);
            l29_st9(r, s.x), l29_st9(r + R, s.y), l29_st9(r + 2 * R, s.zz), l29_st9(r + 3 * R, s.zzz);
        } else {
            const Aff29 q = aff29_from_table(p, OP == 31);
            l29_st9(r, q.x), l29_st9(r + R, q.y);
        }
    } else if constexpr (OP == 33) {
        Xyzz29 s;
        s.x = l29_ld9<FqP>(a), s.y = l29_ld9<FqP>(a + R), s.zz = l29_ld9<FqP>(a + 2 * R), s.zzz = l29_ld9<FqP>(a + 3 * R);
        Aff29 q;
        q.x = l29_ld9<FqP>(a + 4 * R), q.y = l29_ld9<FqP>(a + 5 * R);
        const Xyzz29 o = xyzz29_madd(s, q);
        l29_st9(r, o.x), l29_st9(r + R, o.y), l29_st9(r + 2 * R, o.zz), l29_st9(r + 3 * R, o.zzz);
    } else if constexpr (OP == 34) {
        Xyzz29 s;
        s.x = l29_ld9<FqP>(a), s.y = l29_ld9<FqP>(a + R), s.zz = l29_ld9<FqP>(a + 2 * R), s.zzz = l29_ld9<FqP>(a + 3 * R);
        Xyzz o;
        const bool ok = xyzz29_finish(s, o, tbl);
        l29_st8(r, o.x), l29_st8(r + R, o.y), l29_st8(r + 2 * R, o.zz), l29_st8(r + 3 * R, o.zzz);
        r[4 * R] = ok ? 1u : 0u;
#pragma unroll
        for (int i = 1; i < 9; i++) r[4 * R + i] = 0;
    } else if constexpr (OP == 40) l29_st9(r, ntt29_reduce(l29_ld9<FrP>(a), tbl));
    else if constexpr (OP == 41) l29_st8(r, n29_finish(l29_ld9<FrP>(a), tbl));
    else if constexpr (OP == 42) l29_st8(r, n29_finish_mul(l29_ld9<FrP>(a), l29_ld8<FrP>(a + R), tbl));
    else if constexpr (OP == 43) l29_st9(r, f29_mulc(l29_ld9<FrP>(a), l29_ldc(a + R)));
    else if constexpr (OP == 44) {
        Fr29 r1, r2;
        f29_mulc2(l29_ld9<FrP>(a), l29_ldc(a + R), l29_ld9<FrP>(a + 3 * R), l29_ldc(a + 4 * R), r1, r2);
        l29_st9(r, r1), l29_st9(r + R, r2);
    } else if constexpr (OP == 50) l29_step8<0, true>(a, r, tbl);
    else if constexpr (OP == 51) l29_step8<0, false>(a, r, tbl);
    else if constexpr (OP == 52) l29_step8<1, true>(a, r, tbl);
    else if constexpr (OP == 53) l29_step8<1, false>(a, r, tbl);
    else if constexpr (OP == 54) l29_last_step<0, 4>(a, r);
    else if constexpr (OP == 55) l29_last_step<1, 4>(a, r);
    else if constexpr (OP == 56) {
        Fr29 x[8];
#pragma unroll
        for (int j = 0; j < 8; j++) x[j] = l29_ld9<FrP>(a + j * R);
        n29_step2(x);
#pragma unroll
        for (int j = 0; j < 8; j++) l29_st9(r + j * R, x[j]);
    } else if constexpr (OP == 57) l29_last_step<0, 8>(a, r);
    else if constexpr (OP == 58) l29_last_step<1, 8>(a, r);
    else if constexpr (OP == 60) {
        using namespace gate;
        const Acc a0{ l29_ld9<FrP>(a) };
        const L0 b0{ l29_ld9<FrP>(a + R) };
        const Nw a1{ l29_ld9<FrP>(a + 2 * R) };
        const L1 b1{ l29_ld9<FrP>(a + 3 * R) };
        const Xid17 a2{ l29_ld9<FrP>(a + 4 * R) };
        const L1 b2{ l29_ld9<FrP>(a + 5 * R) };
        const Yid a3{ l29_ld9<FrP>(a + 6 * R) };
        const L1 b3{ l29_ld9<FrP>(a + 7 * R) };
        const Init a4{ l29_ld9<FrP>(a + 8 * R) };
        const L1 b4{ l29_ld9<FrP>(a + 9 * R) };
        l29_st9(r, w29::dot(w29::t(a0, b0), w29::t(a1, b1), w29::t(a2, b2), w29::t(a3, b3), w29::t(a4, b4)).f);
    } else if constexpr (OP >= 100 && OP < 100 + L29_NPAIRS) {
        using Pr = L29Pair<OP - 100>;
        l29_st9(r, f29_sub<Pr::M, Pr::E>(l29_ld9<P>(a), l29_ld9<P>(a + R)));
    } else if constexpr (OP >= 200 && OP < 200 + L29_NPAIRS) {
        using Pr = L29Pair<OP - 200>;
        l29_st9(r, f29_neg<Pr::M, Pr::E>(l29_ld9<P>(a)));
    } else if constexpr (OP >= 300 && OP < 300 + L29_NPAIRS) {
        using Pr = L29Pair<OP - 300>;
        Fr29 x = l29_ld9<FrP>(a), y = l29_ld9<FrP>(a + R);
        n29_bfly<Pr::M, Pr::E>(x, y);
        l29_st9(r, x), l29_st9(r + R, y);
    }
}

// one thread per vector
template <class P, int OP, int OPERANDS, int RESULTS> __global__ void __launch_bounds__(256) k_limb29(const uint32_t* in, uint32_t* out, uint32_t n)
{
    __shared__ __attribute__((aligned(16))) uint32_t tbl[l29_needs_red<OP> ? NTT29_TABLE_WORDS : (l29_needs_div32<OP> ? 32 * DIV32_ROW : 4)];
    if constexpr (l29_needs_div32<OP>) {
        if (threadIdx.x < 32) f29_fill_div32_table<P>(tbl, threadIdx.x);
        __syncthreads();
    } else if constexpr (l29_needs_red<OP>) {
        if (threadIdx.x < NTT29_RED_ROWS) ntt29_fill_reduce_table(tbl, threadIdx.x);
        __syncthreads();
    }
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    l29_run<P, OP>(in + (size_t)i * (OPERANDS * L29_ROW), out + (size_t)i * (RESULTS * L29_ROW), tbl);
}

struct L29Shape {
    int operands, results, fields;
};
bool l29_shape(int op, L29Shape& s)
{
    switch (op) {
#define BBG_X(OP, NIN, NOUT, FIELDS)                                                                                                             \
    case OP: s = { NIN, NOUT, FIELDS }; return true;
        BBG_L29_OPS(BBG_X)
#undef BBG_X
    default: break;
    }
    if (op >= 100 && op < 100 + L29_NPAIRS) { s = { 2, 1, L29_BOTH }; return true; }
    if (op >= 200 && op < 200 + L29_NPAIRS) { s = { 1, 1, L29_BOTH }; return true; }
    if (op >= 300 && op < 300 + L29_NPAIRS) { s = { 2, 2, L29_FR }; return true; }
    return false;
}

template <class P, int OP, int NIN, int NOUT, int FIELDS> void l29_launch(const uint32_t* in, uint32_t* out, size_t n, hipStream_t st)
{
    if constexpr ((FIELDS & (std::is_same<P, FrP>::value ? L29_FR : L29_FQ)) != 0)
        hipLaunchKernelGGL((k_limb29<P, OP, NIN, NOUT>), dim3(grid_for(n, 256)), dim3(256), 0, st, in, out, (uint32_t)n);
}
template <class P> void l29_dispatch(int op, const uint32_t* in, uint32_t* out, size_t n, hipStream_t st)
{
    switch (op) {
#define BBG_X(OP, NIN, NOUT, FIELDS)                                                                                                             \
    case OP: l29_launch<P, OP, NIN, NOUT, FIELDS>(in, out, n, st); return;
        BBG_L29_OPS(BBG_X)
#undef BBG_X
#define BBG_X(I, MM, EE)                                                                                                                         \
    case 100 + I: l29_launch<P, 100 + I, 2, 1, L29_BOTH>(in, out, n, st); return;                                                                \
    case 200 + I: l29_launch<P, 200 + I, 1, 1, L29_BOTH>(in, out, n, st); return;                                                                \
    case 300 + I: l29_launch<P, 300 + I, 2, 2, L29_FR>(in, out, n, st); return;
        BBG_L29_PAIRS(BBG_X)
#undef BBG_X
    default: return;
    }
}

} // namespace

int limb29_op_shape(int which, int op, int* operands, int* results)
{
    L29Shape s;
    if ((which != 0 && which != 1) || !l29_shape(op, s) || !(s.fields & (which == 0 ? L29_FR : L29_FQ))) return BBG_E_INVALID;
    if (operands) *operands = s.operands;
    if (results) *results = s.results;
    return BBG_OK;
}

// d_in: n vectors of `operands` rows, d_out: n vectors of `results` rows (device pointers); n > 0
int limb29_op_device(int which, int op, const void* d_in, void* d_out, size_t n, hipStream_t st)
{
    int rc = limb29_op_shape(which, op, nullptr, nullptr);
    if (rc) {
        set_error("bbg_limb29_op: unknown (which, op)");
        return rc;
    }
    if (which == 0) l29_dispatch<FrP>(op, (const uint32_t*)d_in, (uint32_t*)d_out, n, st);
    else l29_dispatch<FqP>(op, (const uint32_t*)d_in, (uint32_t*)d_out, n, st);
    BBG_HIP(hipGetLastError());
    return BBG_OK;
}

} // namespace bbg
