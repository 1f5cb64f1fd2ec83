// Conformance kernels of the pairing arithmetic (bbg_tower_op, a self-test entry like bbg_limb29_op): one device function of
// fq_tower.hip.h / fq12_wave.hip.h / g2.hip.h per op, fed RAW coefficients -- a coefficient given as 2p arrives as 2p -- and returning raw
// words, so that tests/test_gpu_tower.py can hold the device code to the integer models (tests/tools/pairing_model.py,
// pairing_wave_model.py) at the corners of the tower's contract: every coefficient coarsely reduced in the CLOSED interval [0, 2p].
//
// Rules: every op calls the product's own function from the product's own header; nothing is re-implemented here and no operand is adjusted
// on the device.  Preconditions are not checked: a coefficient above 2p gives wrapped arithmetic (never a fault: a thread, or a block, reads
// its own rows and writes its own rows).  One kernel instantiation per op: a switch inside one kernel would put an Fq12 product and f12_inv
// into a single register allocation.
//
// Rows are Fq values, 8 words.  An Fq2 is two rows (c0, c1), an Fq6 six, an Fq12 twelve in the reference's order; a boolean result is one row
// whose word 0 is 0 or 1 and whose other words are 0.  The ops of fq12_wave.hip.h take and return the twelve coefficients of a slot in the
// w-basis exactly as given (the test applies the model's to_w / from_w).  The op table below is the single definition of the op numbers and
// sizes; tests/tools/tower_vectors.py restates it and the GPU test compares the two through bbg_tower_op_shape.
#include "bbg_internal.h"
#include "fq12_wave.hip.h"
#include "g2.hip.h"

namespace bbg {
namespace {

constexpr int TW_ROW = 8;
constexpr int TW_LANE = 0; // one thread per vector, blocks of 64
constexpr int TW_WAVE = 1; // one 64-lane block per vector, a W12Lds in LDS
constexpr unsigned TW_LANES_SLOT = 1; // the slot of the lane-interleaved round trip (op 42)

// X(op, operand rows, result rows, kind)
#define BBG_TOWER_OPS(X)                                                                                                                         \
    /* Fq2 */                                                                                                                                    \
    X(0, 4, 2, TW_LANE)    /* f2_add */                                                                                                           \
    X(1, 4, 2, TW_LANE)    /* f2_sub */                                                                                                           \
    X(2, 2, 2, TW_LANE)    /* f2_neg */                                                                                                           \
    X(3, 2, 2, TW_LANE)    /* f2_dbl */                                                                                                           \
    X(4, 2, 2, TW_LANE)    /* f2_conj */                                                                                                          \
    X(5, 4, 2, TW_LANE)    /* f2_mul */                                                                                                           \
    X(6, 2, 2, TW_LANE)    /* f2_sqr */                                                                                                           \
    X(7, 3, 2, TW_LANE)    /* f2_mul_fq: a, k */                                                                                                  \
    X(8, 2, 2, TW_LANE)    /* f2_mul_xi */                                                                                                        \
    X(9, 2, 2, TW_LANE)    /* f2_inv */                                                                                                           \
    X(10, 2, 2, TW_LANE)   /* f2_canon */                                                                                                         \
    X(11, 2, 1, TW_LANE)   /* f2_is_zero */                                                                                                       \
    X(12, 4, 1, TW_LANE)   /* f2_eq */                                                                                                            \
    X(13, 1, 1, TW_LANE)   /* fq_canon */                                                                                                         \
    /* Fq6 */                                                                                                                                    \
    X(20, 12, 6, TW_LANE)  /* f6_add */                                                                                                           \
    X(21, 12, 6, TW_LANE)  /* f6_sub */                                                                                                           \
    X(22, 6, 6, TW_LANE)   /* f6_neg */                                                                                                           \
    X(23, 6, 6, TW_LANE)   /* f6_mul_v */                                                                                                         \
    X(24, 12, 6, TW_LANE)  /* f6_mul */                                                                                                           \
    X(25, 6, 6, TW_LANE)   /* f6_sqr */                                                                                                           \
    X(26, 6, 6, TW_LANE)   /* f6_inv */                                                                                                           \
    /* Fq12 */                                                                                                                                   \
    X(30, 24, 12, TW_LANE) /* f12_mul */                                                                                                          \
    X(31, 12, 12, TW_LANE) /* f12_sqr */                                                                                                          \
    X(32, 12, 12, TW_LANE) /* f12_conj */                                                                                                         \
    X(33, 12, 12, TW_LANE) /* f12_inv */                                                                                                          \
    X(34, 4, 4, TW_LANE)   /* f4_sqr: a, b -> t0, t1 */                                                                                           \
    X(35, 12, 12, TW_LANE) /* f12_cyclotomic_sqr */                                                                                               \
    X(36, 12, 12, TW_LANE) /* f12_frobenius(1) */                                                                                                 \
    X(37, 12, 12, TW_LANE) /* f12_frobenius(2) */                                                                                                 \
    X(38, 12, 12, TW_LANE) /* f12_frobenius(3) */                                                                                                 \
    X(39, 18, 12, TW_LANE) /* f12_sparse_mul: a, o, vw, vv */                                                                                     \
    X(40, 12, 1, TW_LANE)  /* f12_is_one */                                                                                                       \
    X(41, 12, 12, TW_LANE) /* f12_store: canonical */                                                                                             \
    X(42, 12, 12, TW_LANE) /* f12_load_lanes(f12_store_lanes): stride = n rounded up to 64, slot 1 */                                             \
    /* one wave per element (fq12_wave.hip.h) */                                                                                                 \
    X(50, 24, 12, TW_WAVE) /* w12_mul<false>: slot 3 = slot 1 x slot 2 */                                                                         \
    X(51, 24, 12, TW_WAVE) /* w12_mul<false>(d=a): slot 1 = slot 1 x slot 2 */                                                                    \
    X(52, 18, 12, TW_WAVE) /* w12_mul<true>: slot 3 = slot 1 x the six rows of s.line */                                                          \
    X(53, 12, 12, TW_WAVE) /* w12_conj */                                                                                                         \
    X(54, 12, 12, TW_WAVE) /* w12_frobenius(1) */                                                                                                 \
    X(55, 12, 12, TW_WAVE) /* w12_frobenius(2) */                                                                                                 \
    X(56, 12, 12, TW_WAVE) /* w12_frobenius(3) */                                                                                                 \
    X(57, 12, 12, TW_WAVE) /* w12_inv */                                                                                                          \
    X(58, 12, 12, TW_WAVE) /* w12_set_one: the operand is what the slot held before */                                                            \
    X(59, 12, 13, TW_WAVE) /* w12_store_is_one: 12 canonical rows in the reference's layout, then the boolean */                                  \
    /* G2 and the lines (g2.hip.h) */                                                                                                            \
    X(60, 4, 1, TW_LANE)   /* g2_on_twist: x, y */                                                                                                \
    X(61, 6, 6, TW_LANE)   /* g2_dbl: x, y, z */                                                                                                  \
    X(62, 10, 6, TW_LANE)  /* g2_madd: P = x, y, z; Q = x, y */                                                                                   \
    X(63, 6, 12, TW_LANE)  /* line_double: cur -> cur (raw), the line (canonical) */                                                              \
    X(64, 10, 12, TW_LANE) /* line_add: base = x, y; cur -> cur (raw), the line (canonical) */                                                    \
    X(65, 4, 4, TW_LANE)   /* g2_mul_by_q */

__device__ __forceinline__ Fq tw_ld(const uint32_t* p)
{
    Fq r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = p[i];
    return r;
}
__device__ __forceinline__ void tw_st(uint32_t* p, const Fq& a)
{
#pragma unroll
    for (int i = 0; i < 8; i++) p[i] = a.v[i];
}
__device__ __forceinline__ Fq2 tw_ld2(const uint32_t* p) { return { tw_ld(p), tw_ld(p + TW_ROW) }; }
__device__ __forceinline__ Fq6 tw_ld6(const uint32_t* p) { return { tw_ld2(p), tw_ld2(p + 2 * TW_ROW), tw_ld2(p + 4 * TW_ROW) }; }
__device__ __forceinline__ Fq12 tw_ld12(const uint32_t* p) { return { tw_ld6(p), tw_ld6(p + 6 * TW_ROW) }; }
__device__ __forceinline__ void tw_st2(uint32_t* p, const Fq2& a)
{
    tw_st(p, a.c0);
    tw_st(p + TW_ROW, a.c1);
}
__device__ __forceinline__ void tw_st6(uint32_t* p, const Fq6& a)
{
    tw_st2(p, a.c0);
    tw_st2(p + 2 * TW_ROW, a.c1);
    tw_st2(p + 4 * TW_ROW, a.c2);
}
__device__ __forceinline__ void tw_st12(uint32_t* p, const Fq12& a)
{
    tw_st6(p, a.c0);
    tw_st6(p + 6 * TW_ROW, a.c1);
}
__device__ __forceinline__ void tw_st_bool(uint32_t* p, bool b)
{
    p[0] = b ? 1u : 0u;
#pragma unroll
    for (int i = 1; i < 8; i++) p[i] = 0;
}
__device__ __forceinline__ G2Jac tw_ldjac(const uint32_t* p) { return { tw_ld2(p), tw_ld2(p + 2 * TW_ROW), tw_ld2(p + 4 * TW_ROW) }; }
__device__ __forceinline__ G2Aff tw_ldaff(const uint32_t* p) { return { tw_ld2(p), tw_ld2(p + 2 * TW_ROW) }; }
__device__ __forceinline__ void tw_stjac(uint32_t* p, const G2Jac& a)
{
    tw_st2(p, a.x);
    tw_st2(p + 2 * TW_ROW, a.y);
    tw_st2(p + 4 * TW_ROW, a.z);
}

// a: the vector's operand rows, r: its result rows; i of n: the vector (op 42 only, with the lane-interleaved work memory)
template <int OP> __device__ __forceinline__ void tw_run(const uint32_t* a, uint32_t* r, uint4* work, size_t stride, size_t i)
{
    constexpr int R = TW_ROW;
    if constexpr (OP == 0) tw_st2(r, f2_add(tw_ld2(a), tw_ld2(a + 2 * R)));
    else if constexpr (OP == 1) tw_st2(r, f2_sub(tw_ld2(a), tw_ld2(a + 2 * R)));
    else if constexpr (OP == 2) tw_st2(r, f2_neg(tw_ld2(a)));
    else if constexpr (OP == 3) tw_st2(r, f2_dbl(tw_ld2(a)));
    else if constexpr (OP == 4) tw_st2(r, f2_conj(tw_ld2(a)));
    else if constexpr (OP == 5) tw_st2(r, f2_mul(tw_ld2(a), tw_ld2(a + 2 * R)));
    else if constexpr (OP == 6) tw_st2(r, f2_sqr(tw_ld2(a)));
    else if constexpr (OP == 7) tw_st2(r, f2_mul_fq(tw_ld2(a), tw_ld(a + 2 * R)));
    else if constexpr (OP == 8) tw_st2(r, f2_mul_xi(tw_ld2(a)));
    else if constexpr (OP == 9) tw_st2(r, f2_inv(tw_ld2(a)));
    else if constexpr (OP == 10) tw_st2(r, f2_canon(tw_ld2(a)));
    else if constexpr (OP == 11) tw_st_bool(r, f2_is_zero(tw_ld2(a)));
    else if constexpr (OP == 12) tw_st_bool(r, f2_eq(tw_ld2(a), tw_ld2(a + 2 * R)));
    else if constexpr (OP == 13) tw_st(r, fq_canon(tw_ld(a)));
    else if constexpr (OP == 20) tw_st6(r, f6_add(tw_ld6(a), tw_ld6(a + 6 * R)));
    else if constexpr (OP == 21) tw_st6(r, f6_sub(tw_ld6(a), tw_ld6(a + 6 * R)));
    else if constexpr (OP == 22) tw_st6(r, f6_neg(tw_ld6(a)));
    else if constexpr (OP == 23) tw_st6(r, f6_mul_v(tw_ld6(a)));
    else if constexpr (OP == 24) tw_st6(r, f6_mul(tw_ld6(a), tw_ld6(a + 6 * R)));
    else if constexpr (OP == 25) tw_st6(r, f6_sqr(tw_ld6(a)));
    else if constexpr (OP == 26) tw_st6(r, f6_inv(tw_ld6(a)));
    else if constexpr (OP == 30) tw_st12(r, f12_mul(tw_ld12(a), tw_ld12(a + 12 * R)));
    else if constexpr (OP == 31) tw_st12(r, f12_sqr(tw_ld12(a)));
    else if constexpr (OP == 32) tw_st12(r, f12_conj(tw_ld12(a)));
    else if constexpr (OP == 33) tw_st12(r, f12_inv(tw_ld12(a)));
    else if constexpr (OP == 34) {
        Fq2 t0, t1;
        f4_sqr(tw_ld2(a), tw_ld2(a + 2 * R), t0, t1);
        tw_st2(r, t0);
        tw_st2(r + 2 * R, t1);
    } else if constexpr (OP == 35) tw_st12(r, f12_cyclotomic_sqr(tw_ld12(a)));
    else if constexpr (OP == 36 || OP == 37 || OP == 38) tw_st12(r, f12_frobenius(tw_ld12(a), OP - 35));
    else if constexpr (OP == 39) tw_st12(r, f12_sparse_mul(tw_ld12(a), tw_ld2(a + 12 * R), tw_ld2(a + 14 * R), tw_ld2(a + 16 * R)));
    else if constexpr (OP == 40) tw_st_bool(r, f12_is_one(tw_ld12(a)));
    else if constexpr (OP == 41) f12_store(r, tw_ld12(a));
    else if constexpr (OP == 42) {
        f12_store_lanes(work, stride, TW_LANES_SLOT, i, tw_ld12(a));
        tw_st12(r, f12_load_lanes(work, stride, TW_LANES_SLOT, i));
    } else if constexpr (OP == 60) tw_st_bool(r, g2_on_twist(tw_ldaff(a)));
    else if constexpr (OP == 61) tw_stjac(r, g2_dbl(tw_ldjac(a)));
    else if constexpr (OP == 62) tw_stjac(r, g2_madd(tw_ldjac(a), tw_ldaff(a + 6 * R)));
    else if constexpr (OP == 63) {
        G2Jac cur = tw_ldjac(a);
        line_double(cur, reinterpret_cast<char*>(r + 6 * R));
        tw_stjac(r, cur);
    } else if constexpr (OP == 64) {
        G2Jac cur = tw_ldjac(a + 4 * R);
        line_add(tw_ldaff(a), cur, reinterpret_cast<char*>(r + 6 * R));
        tw_stjac(r, cur);
    } else if constexpr (OP == 65) {
        const G2Aff q = g2_mul_by_q(tw_ldaff(a));
        tw_st2(r, q.x);
        tw_st2(r + 2 * R, q.y);
    }
}

// one thread per vector
template <int OP, int OPERANDS, int RESULTS> __global__ void __launch_bounds__(64) k_tower(const uint32_t* in, uint32_t* out, uint32_t n, uint4* work, size_t stride)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    tw_run<OP>(in + (size_t)i * (OPERANDS * TW_ROW), out + (size_t)i * (RESULTS * TW_ROW), work, stride, i);
}

// one block of one wave per vector: the operand rows go into slot 1 (and slot 2, or s.line) as they are, the result is slot 3 (slot 1 for op 51)
template <int OP, int OPERANDS, int RESULTS> __global__ void __launch_bounds__(W12_LANES) k_tower_wave(const uint32_t* in, uint32_t* out)
{
    __shared__ W12Lds s;
    const unsigned lane = threadIdx.x;
    const uint32_t* a = in + (size_t)blockIdx.x * (OPERANDS * TW_ROW);
    uint32_t* r = out + (size_t)blockIdx.x * (RESULTS * TW_ROW);
    constexpr unsigned SA = 1, SB = 2, SD = OP == 51 ? 1 : 3;
    if (lane < 12) {
        s.slot[OP == 58 ? SD : SA][lane] = tw_ld(a + lane * TW_ROW);
        if constexpr (OP == 50 || OP == 51) s.slot[SB][lane] = tw_ld(a + (12 + lane) * TW_ROW);
    }
    if constexpr (OP == 52)
        if (lane < 6) s.line[lane] = tw_ld(a + (12 + lane) * TW_ROW);
    __syncthreads();
    if constexpr (OP == 50 || OP == 51) w12_mul<false>(s, lane, SD, SA, s.slot[SB]);
    else if constexpr (OP == 52) w12_mul<true>(s, lane, SD, SA, s.line);
    else if constexpr (OP == 53) w12_conj(s, lane, SD, SA);
    else if constexpr (OP == 54 || OP == 55 || OP == 56) w12_frobenius(s, lane, SD, SA, OP - 53);
    else if constexpr (OP == 57) w12_inv(s, lane, SD, SA);
    else if constexpr (OP == 58) w12_set_one(s, lane, SD);
    if constexpr (OP == 59) {
        const bool one = w12_store_is_one(s, lane, SA, reinterpret_cast<char*>(r));
        if (lane == 0) tw_st_bool(r + 12 * TW_ROW, one);
    } else {
        if (lane < 12) tw_st(r + lane * TW_ROW, s.slot[SD][lane]);
    }
}

template <int OP, int NIN, int NOUT, int KIND> void tw_launch(const uint32_t* in, uint32_t* out, size_t n, uint4* work, size_t stride, hipStream_t st)
{
    if constexpr (KIND == TW_WAVE) hipLaunchKernelGGL((k_tower_wave<OP, NIN, NOUT>), dim3((unsigned)n), dim3(W12_LANES), 0, st, in, out);
    else hipLaunchKernelGGL((k_tower<OP, NIN, NOUT>), dim3(grid_for(n, 64)), dim3(64), 0, st, in, out, (uint32_t)n, work, stride);
}

} // namespace

int tower_op_shape(int op, int* operands, int* results)
{
    switch (op) {
#define BBG_X(OP, NIN, NOUT, KIND)                                                                                                               \
    case OP:                                                                                                                                     \
        if (operands) *operands = NIN;                                                                                                           \
        if (results) *results = NOUT;                                                                                                            \
        return BBG_OK;
        BBG_TOWER_OPS(BBG_X)
#undef BBG_X
    default: return BBG_E_INVALID;
    }
}

// the bytes of lane-interleaved working memory op needs for n vectors (op 42: slots 0 .. TW_LANES_SLOT at a stride of n rounded up to 64)
size_t tower_op_work_bytes(int op, size_t n) { return op == 42 ? (size_t)(TW_LANES_SLOT + 1) * 24 * ((n + 63) / 64 * 64) * sizeof(uint4) : 0; }

// d_in: n vectors of `operands` rows, d_out: n vectors of `results` rows, d_work: tower_op_work_bytes(op, n) bytes (device pointers); n > 0
int tower_op_device(int op, const void* d_in, void* d_out, void* d_work, size_t n, hipStream_t st)
{
    const uint32_t* in = (const uint32_t*)d_in;
    uint32_t* out = (uint32_t*)d_out;
    const size_t stride = (n + 63) / 64 * 64;
    switch (op) {
#define BBG_X(OP, NIN, NOUT, KIND)                                                                                                               \
    case OP: tw_launch<OP, NIN, NOUT, KIND>(in, out, n, (uint4*)d_work, stride, st); break;
        BBG_TOWER_OPS(BBG_X)
#undef BBG_X
    default: set_error("bbg_tower_op: unknown op"); return BBG_E_INVALID;
    }
    BBG_HIP(hipGetLastError());
    return BBG_OK;
}

} // namespace bbg
