// G1 points and Fr scalars between their wire forms and the native form of every other entry point (bbg_wire_decode*,
// bbg_wire_encode*).  One lane per element, one launch per call, no working memory:
//   * k_wire_decode<FORM>   bytes in, 64-byte Montgomery affine (32-byte Montgomery Fr) and a status word out;
//   * k_wire_encode<FORM>   the other way.
// Every form but the compressed decode is a load, a range test, one or two products and a store.  The compressed decode recovers y as
// (x^3 + 3)^((q + 1) / 4) -- q = 3 mod 4, so that power is a square root of every residue and squares to -a for a non-residue -- through
// wire_sqrt_candidate: sliding windows of 4 bits over the 252-bit exponent, the lane's table of odd powers a, a^3 .. a^15 in LDS, 305 products
// a root (a^2, 7 for the table, 250 squarings, 47 window products).
//   Where the table lives, and how large it is (compiler figures and timings in profiles/wire.txt, the discussion in DESIGN.md 5m): as the
// lane's own array indexed by the program's digit it goes to scratch; in LDS, entry-major and lane-minor in 16-byte units, a wave's read of
// one half entry is 64 consecutive uint4 (ds_read_b128: each 16-lane group covers one 256-byte bank row, no conflict), the loop stays a loop
// and scratch is zero.  What LDS costs is occupancy, so the table holds the odd powers only: 16 KiB per 64 lanes, ten waves per CU.
//   Every lane of a wave runs the same program: it is a constant the scalar unit reads, the `product here` branch is uniform, and a lane
// whose word is malformed (or that lies past n) computes on and is masked at the store.
#include "bbg_internal.h"

#include "curve.hip.h"

namespace bbg {

constexpr size_t WIRE_MAX = (size_t)1 << 28;
constexpr int WIRE_SQRT_BLOCK = 64;   // lanes per block of the kernels that take a square root: one wave and its table
constexpr int WIRE_BLOCK = 256;       // of every other kernel
// the window width of the square-root chain: the table holds the odd powers a^1, a^3 .. a^(2^W - 1), 2^(W-1) entries of 32 bytes per lane
#ifndef BBG_WIRE_WINDOW
#define BBG_WIRE_WINDOW 4 // A/B builds only: make EXTRA=-DBBG_WIRE_WINDOW=2 .. 5
#endif
constexpr int WIRE_WINDOW = BBG_WIRE_WINDOW;
constexpr int WIRE_TAB_ENTRIES = 1 << (WIRE_WINDOW - 1);
static_assert(WIRE_WINDOW >= 2 && WIRE_WINDOW <= 5, "a table index is a 4-bit digit of the program");

constexpr bool wire_is_fr(int form) { return form == BBG_WIRE_FR || form == BBG_WIRE_FR_BYTES; }
constexpr bool wire_is_compressed(int form) { return form == BBG_WIRE_G1_COMPRESSED || form == BBG_WIRE_G1_COMPRESSED_BYTES; }
// the 32-byte words of the form are most significant byte first
constexpr bool wire_is_bytes(int form) { return form == BBG_WIRE_G1_COMPRESSED_BYTES || form == BBG_WIRE_G1_BUFFER || form == BBG_WIRE_FR_BYTES; }
constexpr int wire_decode_block(int form) { return wire_is_compressed(form) ? WIRE_SQRT_BLOCK : WIRE_BLOCK; }

// (q + 1) / 4 as eight words
struct WireExp {
    uint32_t w[8];
};
constexpr WireExp wire_sqrt_exp()
{
    WireExp e{};
    uint32_t t[8] = {};
    for (int i = 0; i < 8; i++) t[i] = FqP::MOD[i];
    t[0] += 1; // q = 3 mod 4: no carry
    for (int i = 0; i < 8; i++) e.w[i] = (t[i] >> 2) | (i < 7 ? t[i + 1] << 30 : 0u);
    return e;
}
static_assert((FqP::MOD[0] & 3u) == 3u, "the square root by one power needs q = 3 mod 4");

// The exponent as a sliding-window program, made at compile time (tests/tools/wire_model.py window_program is the same recoding).  From the
// top bit down, a set bit i opens a window i .. l, l >= i - W + 1 the lowest set bit in reach, whose odd value v is one table entry
// (v - 1) / 2: the accumulator is squared once per exponent bit, and after the squaring of bit l it takes the product with a^v.  The first
// window needs no squaring: the accumulator starts as its entry.  The exponent is a constant, so every lane of every wave runs one program.
struct WireProgram {
    uint32_t mul_at[8]; // bit l: a product follows the squaring of exponent bit l
    uint32_t entry[16]; // 4-bit digit k: the table entry of product k, in the order they run
    int first_entry;    // the accumulator's start
    int start_bit;      // the first exponent bit the loop squares for
    int products;
};
constexpr WireProgram wire_program(int window)
{
    const WireExp e = wire_sqrt_exp();
    WireProgram p{};
    int i = 255, k = -1; // k = -1: the first window
    while (!((e.w[i >> 5] >> (i & 31)) & 1u)) i--;
    while (i >= 0) {
        if (!((e.w[i >> 5] >> (i & 31)) & 1u)) {
            i--;
            continue;
        }
        int l = i - window + 1 < 0 ? 0 : i - window + 1;
        while (!((e.w[l >> 5] >> (l & 31)) & 1u)) l++;
        uint32_t v = 0;
        for (int j = i; j >= l; j--) v = v << 1 | ((e.w[j >> 5] >> (j & 31)) & 1u);
        if (k < 0) {
            p.first_entry = (int)(v - 1) / 2;
            p.start_bit = l - 1;
        } else {
            p.mul_at[l >> 5] |= 1u << (l & 31);
            p.entry[k >> 3] |= ((v - 1) / 2) << (4 * (k & 7));
        }
        k++;
        i = l - 1;
    }
    p.products = k;
    return p;
}
static_assert(wire_program(WIRE_WINDOW).products <= 128, "the entry digits of the program fit their sixteen words");
__constant__ const WireProgram WIRE_PROGRAM = wire_program(WIRE_WINDOW);

// entry e of lane t's table: two 16-byte halves, [entry][half][lane]
__device__ __forceinline__ void wire_tab_put(uint4* tab, int e, int t, const Fq& a)
{
    tab[(e * 2 + 0) * WIRE_SQRT_BLOCK + t] = make_uint4(a.v[0], a.v[1], a.v[2], a.v[3]);
    tab[(e * 2 + 1) * WIRE_SQRT_BLOCK + t] = make_uint4(a.v[4], a.v[5], a.v[6], a.v[7]);
}
__device__ __forceinline__ Fq wire_tab_get(const uint4* tab, int e, int t)
{
    const uint4 lo = tab[(e * 2 + 0) * WIRE_SQRT_BLOCK + t], hi = tab[(e * 2 + 1) * WIRE_SQRT_BLOCK + t];
    Fq r;
    r.v[0] = lo.x; r.v[1] = lo.y; r.v[2] = lo.z; r.v[3] = lo.w;
    r.v[4] = hi.x; r.v[5] = hi.y; r.v[6] = hi.z; r.v[7] = hi.w;
    return r;
}
// a^((q + 1) / 4), a in [0, 2q), result in [0, 2q).  tab: WIRE_TAB_ENTRIES x 2 x WIRE_SQRT_BLOCK uint4 of the block's LDS; a lane touches its
// own slots only, so there is no barrier.
// A/B builds only (make EXTRA=-DBBG_WIRE_TABLE_REGS): the table as the lane's own array indexed by the program's digit, which
// the compiler puts in scratch.  Results are the same.
__device__ __forceinline__ Fq wire_sqrt_candidate(const Fq& a, uint4* tab)
{
#ifdef BBG_WIRE_TABLE_REGS
    Fq own[WIRE_TAB_ENTRIES];
    auto put = [&](int e, const Fq& v) { own[e] = v; };
    auto get = [&](int e) { return own[e]; };
#else
    const int t = threadIdx.x;
    auto put = [&](int e, const Fq& v) { wire_tab_put(tab, e, t, v); };
    auto get = [&](int e) { return wire_tab_get(tab, e, t); };
#endif
    constexpr WireProgram shape = wire_program(WIRE_WINDOW); // the two scalars of the program that shape the loop
    const Fq a2 = fe_sqr(a);
    Fq p = a;
    put(0, p);
#pragma unroll 1
    for (int e = 1; e < WIRE_TAB_ENTRIES; e++) {
        p = fe_mul(p, a2);
        put(e, p);
    }
    Fq acc = get(shape.first_entry);
    int k = 0;
#pragma unroll 1
    for (int i = shape.start_bit; i >= 0; i--) {
        acc = fe_sqr(acc);
        if ((WIRE_PROGRAM.mul_at[i >> 5] >> (i & 31)) & 1u) { // uniform: scalar loads and a scalar branch
            acc = fe_mul(acc, get((int)((WIRE_PROGRAM.entry[k >> 3] >> ((k & 7) * 4)) & 15u)));
            k++;
        }
    }
    return acc;
}

// a 32-byte word as the integer it holds, eight little-endian words
template <bool BYTES, class P> __device__ __forceinline__ Fe<P> wire_load32(const void* p)
{
    Fe<P> m = fe_load<P>(p);
    if constexpr (!BYTES) return m;
    Fe<P> r;
#pragma unroll
    for (int j = 0; j < 8; j++) r.v[j] = __builtin_bswap32(m.v[7 - j]);
    return r;
}
template <bool BYTES, class P> __device__ __forceinline__ void wire_store32(void* p, const Fe<P>& a)
{
    if constexpr (!BYTES) {
        fe_store<P>(p, a);
    } else {
        Fe<P> m;
#pragma unroll
        for (int j = 0; j < 8; j++) m.v[j] = __builtin_bswap32(a.v[7 - j]);
        fe_store<P>(p, m);
    }
}
template <class P> __device__ __forceinline__ bool wire_below_modulus(const Fe<P>& a)
{
    uint32_t scratch_words[8];
    return sub_limbs<P>(scratch_words, a.v, P::MOD) != 0;
}
// q - y for canonical y (0 stays 0)
__device__ __forceinline__ Fq wire_neg_canonical(const Fq& y) { return fe_reduce_once(fe_reduce_once(fe_neg(y))); }

// the status word, and the bad ones (0, 2) counted with one atomic per wave.  Every lane of the wave comes here.
__device__ __forceinline__ void wire_report(bool live, size_t i, uint32_t st, uint32_t* status, unsigned* bad)
{
    if (live && status) status[i] = st;
    const unsigned long long m = __ballot(live && (st == 0u || st == 2u));
    if (bad && m && (threadIdx.x & 63) == 0) atomicAdd(bad, (unsigned)__popcll(m));
}

// status: 1 finite and valid, 3 infinity, 0 malformed, 2 not on the curve (include/bbg.h)
template <int FORM> __global__ void __launch_bounds__(wire_decode_block(FORM)) k_wire_decode(const char* __restrict__ wire, size_t n, char* __restrict__ native,
                                                                                             uint32_t* __restrict__ status, unsigned* bad)
{
    constexpr bool BYTES = wire_is_bytes(FORM);
    const size_t i = (size_t)blockIdx.x * wire_decode_block(FORM) + threadIdx.x;
    const bool live = i < n;
    uint32_t st = 1;
    if constexpr (wire_is_fr(FORM)) {
        if (live) {
            const Fr v = wire_load32<BYTES, FrP>(wire + i * 32);
            st = wire_below_modulus(v) ? 1u : 0u;
            fe_store<FrP>(native + i * 32, st ? fe_reduce_once(fe_to_mont(v)) : Fr::zero());
        }
    } else if constexpr (FORM == BBG_WIRE_G1_BUFFER) {
        if (live) {
            Fq y = wire_load32<BYTES, FqP>(wire + i * 64);
            const Fq x = wire_load32<BYTES, FqP>(wire + i * 64 + 32);
            Affine a = aff_inf();
            if (y.v[7] >> 31) {
                st = 3; // the flag decides, whatever lies under it
            } else if ((y.v[7] >> 30) || !wire_below_modulus(y) || !wire_below_modulus(x)) {
                st = 0;
            } else {
                Affine c;
                c.x = fe_reduce_once(fe_to_mont(x));
                c.y = fe_reduce_once(fe_to_mont(y));
                if (aff_on_curve(c)) a = c;
                else st = 2;
            }
            aff_store(native + i * 64, a);
        }
    } else {
        __shared__ uint4 tab[WIRE_TAB_ENTRIES * 2 * WIRE_SQRT_BLOCK];
        Fq x = Fq::zero();
        if (live) x = wire_load32<BYTES, FqP>(wire + i * 32);
        const uint32_t parity = x.v[7] >> 31, inf_flag = (x.v[7] >> 30) & 1u;
        x.v[7] &= 0x3fffffffu;
        if (inf_flag) st = (parity == 0 && x.is_zero_raw()) ? 3u : 0u;
        else if (!wire_below_modulus(x)) st = 0;
        // the chain, whatever the word was: x < 2^254 < 2q is inside every product's range
        const Fq xm = fe_to_mont(x);
        const Fq three = fe_add(fe_dbl(Fq::one()), Fq::one());
        const Fq rhs = fe_add(fe_mul(fe_sqr(xm), xm), three);
        Fq y = fe_reduce_once(wire_sqrt_candidate(rhs, tab));
        if (st == 1 && !fe_eq(fe_sqr(y), rhs)) st = 2;
        if ((fe_from_mont(y).v[0] & 1u) != parity) y = wire_neg_canonical(y);
        if (live) {
            Affine a = aff_inf();
            if (st == 1) {
                a.x = fe_reduce_once(xm);
                a.y = y;
            }
            aff_store(native + i * 64, a);
        }
    }
    wire_report(live, i, st, status, bad);
}

template <int FORM> __global__ void __launch_bounds__(WIRE_BLOCK) k_wire_encode(const char* __restrict__ native, size_t n, int check, char* __restrict__ wire,
                                                                                uint32_t* __restrict__ status, unsigned* bad)
{
    constexpr bool BYTES = wire_is_bytes(FORM);
    const size_t i = (size_t)blockIdx.x * WIRE_BLOCK + threadIdx.x;
    const bool live = i < n;
    uint32_t st = 1;
    if constexpr (wire_is_fr(FORM)) {
        if (live) wire_store32<BYTES, FrP>(wire + i * 32, fe_from_mont(fe_load<FrP>(native + i * 32)));
    } else {
        if (live) {
            const Affine a = aff_load(native + i * 64);
            if (aff_is_inf(a)) st = 3;
            else if (check && !aff_on_curve(a)) st = 2;
            Fq x = Fq::zero(), y = Fq::zero();
            if (st == 1) {
                x = fe_from_mont(a.x);
                y = fe_from_mont(a.y);
            }
            if constexpr (FORM == BBG_WIRE_G1_BUFFER) {
                if (st != 1) y.v[7] = 0x80000000u; // byte 0 = 0x80, 63 zero bytes
                wire_store32<BYTES, FqP>(wire + i * 64, y);
                wire_store32<BYTES, FqP>(wire + i * 64 + 32, x);
            } else {
                if (st != 1) x.v[7] = 0x40000000u; // bit 254 alone
                else x.v[7] |= (y.v[0] & 1u) << 31;
                wire_store32<BYTES, FqP>(wire + i * 32, x);
            }
        }
    }
    wire_report(live, i, st, status, bad);
}

// bbg_field_op (which = 1, op = 12): the square-root candidate alone, canonical
__global__ void __launch_bounds__(WIRE_SQRT_BLOCK) k_wire_sqrt(const Fq* __restrict__ a, Fq* __restrict__ out, size_t n)
{
    __shared__ uint4 tab[WIRE_TAB_ENTRIES * 2 * WIRE_SQRT_BLOCK];
    const size_t i = (size_t)blockIdx.x * WIRE_SQRT_BLOCK + threadIdx.x;
    Fq x = Fq::zero();
    if (i < n) x = fe_load<FqP>(a + i);
    for (int k = 0; k < 5; k++) x = fe_reduce_once(x); // any 256-bit input, as the other ops of bbg_field_op take it
    const Fq y = fe_reduce_once(wire_sqrt_candidate(x, tab));
    if (i < n) fe_store<FqP>(out + i, y);
}

// ---------------------------------------------------------------------------------------------- host side
int wire_sizes(int form, size_t* wire_bytes, size_t* native_bytes)
{
    if (form < BBG_WIRE_G1_COMPRESSED || form > BBG_WIRE_FR_BYTES) return BBG_E_INVALID;
    if (wire_bytes) *wire_bytes = form == BBG_WIRE_G1_BUFFER ? 64 : 32;
    if (native_bytes) *native_bytes = wire_is_fr(form) ? 32 : 64;
    return BBG_OK;
}

// the refusals of all four entry points: `in` and `out` with in_each / out_each bytes per element; status and bad may be null
int wire_check(const char* who, int form, int check, size_t n, const void* in, size_t in_each, const void* out, size_t out_each, const void* status,
               const void* bad)
{
    const std::string w(who);
    size_t wire_bytes = 0, native_bytes = 0;
    if (wire_sizes(form, &wire_bytes, &native_bytes)) { set_error(w + ": unknown form"); return BBG_E_INVALID; }
    if (check != 0 && check != 1) { set_error(w + ": check must be 0 or 1"); return BBG_E_INVALID; }
    if (n > WIRE_MAX) { set_error(w + ": n must be at most 2^28"); return BBG_E_INVALID; }
    if (n == 0) return BBG_OK;
    if (!in || !out) { set_error(w + ": null argument"); return BBG_E_INVALID; }
    const void* r[4] = { in, out, status, bad };
    const size_t b[4] = { n * in_each, n * out_each, n * 4, 4 };
    for (int i = 0; i < 4; i++)
        for (int j = i + 1; j < 4; j++)
            if (r[i] && r[j] && ranges_overlap(r[i], b[i], r[j], b[j])) { set_error(w + ": the input and the outputs overlap"); return BBG_E_INVALID; }
    return BBG_OK;
}
// the kernels move 16 bytes per access: device data pointers are 16-byte aligned, the status and count words 4-byte
static int wire_check_aligned(const char* who, const void* a, const void* b, const void* status, const void* bad)
{
    if (!((((uintptr_t)a | (uintptr_t)b) & 15) || (((uintptr_t)status | (uintptr_t)bad) & 3))) return BBG_OK;
    set_error(std::string(who) + ": a misaligned device pointer");
    return BBG_E_INVALID;
}

template <int FORM> static void wire_launch_decode(const void* d_wire, size_t n, void* d_native, void* d_status, void* d_bad, hipStream_t st)
{
    constexpr int block = wire_decode_block(FORM);
    hipLaunchKernelGGL(k_wire_decode<FORM>, dim3(grid_for(n, block)), dim3(block), 0, st, (const char*)d_wire, n, (char*)d_native, (uint32_t*)d_status, (unsigned*)d_bad);
}
template <int FORM> static void wire_launch_encode(const void* d_native, size_t n, int check, void* d_wire, void* d_status, void* d_bad, hipStream_t st)
{
    hipLaunchKernelGGL(k_wire_encode<FORM>, dim3(grid_for(n, WIRE_BLOCK)), dim3(WIRE_BLOCK), 0, st, (const char*)d_native, n, check, (char*)d_wire, (uint32_t*)d_status,
                       (unsigned*)d_bad);
}
// one instantiation per form
#define BBG_WIRE_DISPATCH(form, fn, ...)                                                                              \
    switch (form) {                                                                                                   \
    case BBG_WIRE_G1_COMPRESSED: fn<BBG_WIRE_G1_COMPRESSED>(__VA_ARGS__); break;                                      \
    case BBG_WIRE_G1_COMPRESSED_BYTES: fn<BBG_WIRE_G1_COMPRESSED_BYTES>(__VA_ARGS__); break;                          \
    case BBG_WIRE_G1_BUFFER: fn<BBG_WIRE_G1_BUFFER>(__VA_ARGS__); break;                                              \
    case BBG_WIRE_FR: fn<BBG_WIRE_FR>(__VA_ARGS__); break;                                                            \
    default: fn<BBG_WIRE_FR_BYTES>(__VA_ARGS__); break;                                                               \
    }

int wire_decode_run(bbg_ctx* ctx, const char* who, int form, const void* d_wire, size_t n, void* d_native, void* d_status, void* d_bad, hipStream_t st)
{
    size_t wire_bytes = 0, native_bytes = 0;
    (void)wire_sizes(form, &wire_bytes, &native_bytes);
    if (int rc = wire_check(who, form, 0, n, d_wire, wire_bytes, d_native, native_bytes, d_status, d_bad)) return rc;
    if (n) if (int rc = wire_check_aligned(who, d_wire, d_native, d_status, d_bad)) return rc;
    ProfScope ps(ctx, "wire_decode", st);
    if (d_bad) BBG_HIP(hipMemsetAsync(d_bad, 0, 4, st));
    if (n == 0) return BBG_OK;
    BBG_WIRE_DISPATCH(form, wire_launch_decode, d_wire, n, d_native, d_status, d_bad, st);
    BBG_HIP(hipGetLastError());
    return BBG_OK;
}

int wire_encode_run(bbg_ctx* ctx, const char* who, int form, const void* d_native, size_t n, int check, void* d_wire, void* d_status, void* d_bad, hipStream_t st)
{
    size_t wire_bytes = 0, native_bytes = 0;
    (void)wire_sizes(form, &wire_bytes, &native_bytes);
    if (int rc = wire_check(who, form, check, n, d_native, native_bytes, d_wire, wire_bytes, d_status, d_bad)) return rc;
    if (n) if (int rc = wire_check_aligned(who, d_wire, d_native, d_status, d_bad)) return rc;
    ProfScope ps(ctx, "wire_encode", st);
    if (d_bad) BBG_HIP(hipMemsetAsync(d_bad, 0, 4, st));
    if (n == 0) return BBG_OK;
    BBG_WIRE_DISPATCH(form, wire_launch_encode, d_native, n, check, d_wire, d_status, d_bad, st);
    BBG_HIP(hipGetLastError());
    return BBG_OK;
}

int wire_sqrt_device(const void* d_a, void* d_out, size_t n, hipStream_t st)
{
    if (n == 0) return BBG_OK;
    hipLaunchKernelGGL(k_wire_sqrt, dim3(grid_for(n, WIRE_SQRT_BLOCK)), dim3(WIRE_SQRT_BLOCK), 0, st, (const Fq*)d_a, (Fq*)d_out, n);
    BBG_HIP(hipGetLastError());
    return BBG_OK;
}

} // namespace bbg
