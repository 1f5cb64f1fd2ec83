// Batched BN254 pairing product checks over precomputed G2 lines for gfx950: for `count` independent products
//     e_i = prod_(j < pairs) e(P_ij, Q_j)
// over the SAME `pairs` G2 points, the reference's pairing::reduced_ate_pairing_batch_precomputed (ecc/curves/bn254/pairing_impl.hpp:269-282)
// once per product.  The G2 side is done once (bbg_g2_lines_prepare): the 87 line coefficients of every Q_j in the reference's
// pairing::miller_lines layout.  Every product then evaluates those lines at its own G1 points: one lane per product, the lines
// wave-uniform (every lane reads the same line at every step), the Fq12 accumulator and the G1 point per lane.
//
//   k_g2_mul       [s] B on the twist, one lane per scalar, double-and-add on Jacobian coordinates over Fq2.  Plumbing: bbg_g2_mul and the
//                  subgroup test [r] Q = infinity of bbg_g2_lines_prepare.
//   k_g2_lines     precompute_miller_lines (:23-123), one lane per G2 point.
//   k_pair_miller  miller_loop_batch (:163-205): per line index the accumulator is squared where the line opens a loop step, then multiplied
//                  by the line of every pair (field12::self_sparse_mul).  A pair whose G1 point is infinite is skipped: the factor one.
//   k_pair_final   final_exponentiation_easy_part / _tricky_part (:207-253) as a straight-line program over six Fq12 slots of working memory
//                  (PAIR_FINAL_PROGRAM, pairing_consts.hip.h): one loop whose body holds ONE inlined copy of each Fq12 operation, operands
//                  loaded from and results stored to the lane-interleaved slots, so no Fq12 is selected by a runtime index in registers.
//                  Squarings past the easy part are cyclotomic (Granger-Scott; the same element as the reference's plain sqr() there).
#include <string.h>

#include "bbg_internal.h"
#include "work_layouts.h"
#include "curve.hip.h"
#include "g2.hip.h"

namespace bbg {

constexpr size_t PAIR_MAX_COUNT = (size_t)1 << 24;
constexpr size_t PAIR_CHUNK = (size_t)1 << 16; // products per launch pair: one wave per SIMD of the chip
constexpr size_t PAIR_LINES_BYTES = (size_t)PairP::LINES * 192;
constexpr size_t G2_MUL_MAX = (size_t)1 << 16;
constexpr uint32_t G2_BASE_INF = 1u, G2_OFF_TWIST = 2u, G2_RESULT_INF = 4u;

// out[i] = [k_i] B_i, B_i = bases[i base_stride] (128 B affine), k_i = scalars[i scalar_stride]: plain 256-bit words with raw != 0, else
// Montgomery Fr in [0, 2r).  flags[i] (may be null): G2_BASE_INF | G2_OFF_TWIST | G2_RESULT_INF; out (may be null) holds infinity for a
// base off the twist.  One lane per product.
__global__ void __launch_bounds__(64) k_g2_mul(const G2Aff* __restrict__ bases, size_t base_stride, const Fr* __restrict__ scalars, size_t scalar_stride, int raw,
                                               size_t n, G2Aff* __restrict__ out, uint32_t* __restrict__ flags)
{
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const G2Aff base = g2_aff_load(bases + i * base_stride);
    uint32_t flag = 0;
    G2Jac acc = { f2_one(), f2_one(), f2_zero() };
    if (g2_aff_is_inf(base)) flag = G2_BASE_INF;
    else if (!g2_on_twist(base)) flag = G2_OFF_TWIST;
    else {
        Fr k = fe_load<FrP>(scalars + i * scalar_stride);
        if (!raw) k = fe_from_mont(k);
#pragma unroll 1
        for (int b = 0; b < 256; b++) {
            acc = g2_dbl(acc);
            const bool bit = (k.v[7] >> 31) != 0;
#pragma unroll
            for (int w = 7; w > 0; w--) k.v[w] = (k.v[w] << 1) | (k.v[w - 1] >> 31);
            k.v[0] <<= 1;
            if (bit) acc = g2_madd(acc, base);
        }
    }
    const bool inf = f2_is_zero(acc.z);
    if (inf) flag |= G2_RESULT_INF;
    if (flags) flags[i] = flag;
    if (!out) return;
    G2Aff a = { f2_zero(), f2_zero() };
    if (!inf) {
        const Fq2 zi = f2_inv(acc.z), zi2 = f2_sqr(zi);
        a.x = f2_mul(acc.x, zi2);
        a.y = f2_mul(acc.y, f2_mul(zi2, zi));
    }
    g2_aff_store(out + i, a, inf);
}

// lines[j] = precompute_miller_lines(points[j]) (:99-123): 87 x (o | vw | vv), canonical.  points[j] finite.  One lane per point.
__global__ void __launch_bounds__(64) k_g2_lines(const G2Aff* __restrict__ points, size_t n, char* __restrict__ lines)
{
    const size_t j = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (j >= n) return;
    const G2Aff q = g2_aff_load(points + j);
    G2Jac cur = { q.x, q.y, f2_one() };
    char* line = lines + j * PAIR_LINES_BYTES;
#pragma unroll 1
    for (int i = 0; i < PairP::LOOP_LENGTH; i++) {
        line_double(cur, line);
        line += 192;
        if ((PairP::LOOP_ADD >> i) & 1) {
            const bool neg = ((PairP::LOOP_NEG >> i) & 1) != 0;
            const G2Aff base = { q.x, neg ? f2_neg(q.y) : q.y };
            line_add(base, cur, line);
            line += 192;
        }
    }
    const G2Aff q1 = g2_mul_by_q(q);
    G2Aff q2 = g2_mul_by_q(q1);
    q2.y = f2_neg(q2.y);
#pragma unroll 1
    for (int s = 0; s < 2; s++) {
        const G2Aff base = s == 0 ? q1 : q2;
        line_add(base, cur, line);
        line += 192;
    }
}

// ---------------------------------------------------------------------------------------------- the pairing product
// Product i < count: slot 0 of the working memory = miller_loop_batch over the finite points among g1[i pairs + j], j < pairs, against
// lines[j]; flags[i] = 2 where a finite point is off the curve, else 0.  One lane per product; `lines` is read wave-uniformly.
__global__ void __launch_bounds__(64, 1) k_pair_miller(const char* __restrict__ lines, int pairs, const Affine* __restrict__ g1, size_t count, uint4* __restrict__ work,
                                                      size_t stride, uint32_t* __restrict__ flags)
{
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    const Affine* mine = g1 + i * (size_t)pairs;
    uint32_t live = 0, bad = 0;
#pragma unroll 1
    for (int j = 0; j < pairs; j++) {
        const Affine a = aff_load(mine + j);
        if (!aff_is_inf(a)) {
            live |= 1u << j;
            if (!aff_on_curve(a)) bad = 2;
        }
    }
    Fq12 f = f12_one();
#pragma unroll 1
    for (int it = 0; it < PairP::LINES; it++) {
        const uint32_t opens = it < 32 ? PairP::LINE_OPENS_STEP[0] >> it : it < 64 ? PairP::LINE_OPENS_STEP[1] >> (it - 32) : PairP::LINE_OPENS_STEP[2] >> (it - 64);
        if (opens & 1) f = f12_sqr(f);
#pragma unroll 1
        for (int j = 0; j < pairs; j++) {
            if (!((live >> j) & 1)) continue;
            const Affine a = aff_load(mine + j);
            const char* line = lines + (size_t)j * PAIR_LINES_BYTES + (size_t)it * 192;
            f = f12_sparse_mul(f, f2_load(line), f2_mul_fq(f2_load(line + 64), a.y), f2_mul_fq(f2_load(line + 128), a.x));
        }
    }
    f12_store_lanes(work, stride, 0, i, f);
    flags[i] = bad;
}

// Product i < count: the final exponentiation of slot 0 by PAIR_FINAL_PROGRAM, then out[i] (may be null) = the canonical Fq12 and
// status[i] (may be null) = 2 where flags[i] says so, else 1 where the value is one, else 0.  One lane per product.
__global__ void __launch_bounds__(64, 1) k_pair_final(uint4* __restrict__ work, size_t stride, size_t count, const uint32_t* __restrict__ flags, char* __restrict__ out,
                                                     uint32_t* __restrict__ status)
{
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
#pragma unroll 1
    for (int pc = 0; pc < PairP::FINAL_STEPS; pc++) {
        const uint32_t word = PAIR_FINAL_PROGRAM[pc];
        const uint32_t op = word & 255u, d = (word >> 8) & 255u, a = (word >> 16) & 255u, b = word >> 24;
        if (op == PairP::OP_END) break;
        const Fq12 x = f12_load_lanes(work, stride, a, i);
        Fq12 r;
        switch (op) {
        case PairP::OP_MUL: r = f12_mul(x, f12_load_lanes(work, stride, b, i)); break;
        case PairP::OP_CSQR: r = f12_cyclotomic_sqr(x); break;
        case PairP::OP_CONJ: r = f12_conj(x); break;
        case PairP::OP_INV: r = f12_inv(x); break;
        default: r = f12_frobenius(x, (int)op - (int)PairP::OP_FROB1 + 1); break;
        }
        f12_store_lanes(work, stride, d, i, r);
    }
    const Fq12 e = f12_load_lanes(work, stride, 0, i);
    if (out) f12_store(out + i * 384, e);
    if (status) status[i] = flags[i] ? 2u : f12_is_one(e) ? 1u : 0u;
}

// ---------------------------------------------------------------------------------------------- host side
// the products of one chunk of a call with `count` products, rounded up to whole waves: the stride of the lane-interleaved slots
static size_t pair_stride(size_t count) { return (std::min(count, PAIR_CHUNK) + 63) / 64 * 64; }

int g2_mul_host(bbg_ctx* ctx, const uint64_t* base_affine, const uint64_t* scalars, size_t n, uint64_t* out_affine)
{
    const char* who = "bbg_g2_mul";
    if (n > G2_MUL_MAX) { set_error(std::string(who) + ": n is above 2^16"); return BBG_E_INVALID; }
    if (n && (!scalars || !out_affine)) { set_error(std::string(who) + ": null argument"); return BBG_E_INVALID; }
    Staged sg(ctx, who);
    // flags: n + 1 words, the last for the base alone; scalars: the scalar 0 of the base's own check, then the caller's
    const Staged::Region r_base = sg.region(128), r_flags = sg.region(n + 1, 4), r_scalars = sg.region(n + 1, 32), r_out = sg.region(n, 128);
    if (int rc = sg.ensure()) return rc;
    hipStream_t st = ctx->stream;
    uint64_t base[16];
    if (base_affine) memcpy(base, base_affine, 128);
    else {
        for (int h = 0; h < 2; h++)
            for (int w = 0; w < 4; w++) {
                base[4 * h + w] = (uint64_t)PairP::G2_X[h][2 * w] | ((uint64_t)PairP::G2_X[h][2 * w + 1] << 32);
                base[8 + 4 * h + w] = (uint64_t)PairP::G2_Y[h][2 * w] | ((uint64_t)PairP::G2_Y[h][2 * w + 1] << 32);
            }
    }
    const G2Aff* d_base = (const G2Aff*)sg[r_base];
    Fr* d_scalars = (Fr*)sg[r_scalars];
    uint32_t* d_flags = (uint32_t*)sg[r_flags];
    if (int rc = sg.up(r_base, base, 128)) return rc;
    BBG_HIP(hipMemsetAsync(d_scalars, 0, 32, st));
    if (n) BBG_HIP(hipMemcpyAsync(d_scalars + 1, scalars, n * 32, hipMemcpyHostToDevice, st));
    // the base alone first (n = 0 validates it as well), then the products
    hipLaunchKernelGGL(k_g2_mul, dim3(1), dim3(64), 0, st, d_base, (size_t)0, (const Fr*)d_scalars, (size_t)0, 1, (size_t)1, (G2Aff*)nullptr, d_flags + n);
    if (n)
        hipLaunchKernelGGL(k_g2_mul, dim3(grid_for(n, 64)), dim3(64), 0, st, d_base, (size_t)0, (const Fr*)(d_scalars + 1), (size_t)1, 0, n, (G2Aff*)sg[r_out], d_flags);
    BBG_HIP(hipGetLastError());
    uint32_t flag = 0;
    BBG_HIP(hipMemcpyAsync(&flag, d_flags + n, 4, hipMemcpyDeviceToHost, st));
    if (int rc = sg.wait()) return rc;
    if (flag & G2_OFF_TWIST) { set_error(std::string(who) + ": the base point is not on the twist y^2 = x^3 + 3 / (9 + u)"); return BBG_E_INVALID; }
    if (n) {
        if (int rc = sg.down(out_affine, r_out, n * 128)) return rc;
        if (int rc = sg.wait()) return rc;
    }
    return BBG_OK;
}

int g2_lines_prepare(bbg_ctx* ctx, const uint64_t* g2_affine, size_t pairs, bbg_g2_lines** out)
{
    const char* who = "bbg_g2_lines_prepare";
    if (!g2_affine || !out) { set_error(std::string(who) + ": null argument"); return BBG_E_INVALID; }
    if (pairs < 1 || pairs > BBG_PAIRING_MAX_PAIRS) { set_error(std::string(who) + ": pairs must be 1 .. 8"); return BBG_E_INVALID; }
    Staged sg(ctx, who);
    const Staged::Region r_points = sg.region(pairs, 128), r_r = sg.region(32), r_flags = sg.region(pairs, 4); // points | the scalar r | flags
    if (int rc = sg.ensure()) return rc;
    hipStream_t st = ctx->stream;
    const G2Aff* d_points = (const G2Aff*)sg[r_points];
    void* d_lines = nullptr;
    BBG_HIP(hipMalloc(&d_lines, pairs * PAIR_LINES_BYTES));
    uint32_t flags[BBG_PAIRING_MAX_PAIRS];
    int rc = sg.up(r_points, g2_affine, pairs * 128);
    if (rc == BBG_OK) rc = sg.up(r_r, PairP::R_PLAIN, 32);
    if (rc == BBG_OK) {
        ProfScope ps(ctx, "g2_lines", st);
        // [r] Q per point: finite, on the twist and of order r, or the handle is refused.  A lane of k_g2_lines that meets such a point computes
        // lines nobody reads.
        hipLaunchKernelGGL(k_g2_mul, dim3(1), dim3(64), 0, st, d_points, (size_t)1, (const Fr*)sg[r_r], (size_t)0, 1, pairs, (G2Aff*)nullptr, (uint32_t*)sg[r_flags]);
        hipLaunchKernelGGL(k_g2_lines, dim3(1), dim3(64), 0, st, d_points, pairs, (char*)d_lines);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = hip_fail(e, who, __FILE__, __LINE__);
    }
    if (rc == BBG_OK) rc = sg.down(flags, r_flags, pairs * 4);
    if (rc == BBG_OK) rc = sg.wait();
    if (rc != BBG_OK) {
        (void)hipFree(d_lines);
        return rc;
    }
    for (size_t j = 0; j < pairs; j++) {
        const char* what = (flags[j] & G2_BASE_INF) ? "is the point at infinity" : (flags[j] & G2_OFF_TWIST) ? "is not on the twist y^2 = x^3 + 3 / (9 + u)"
                           : !(flags[j] & G2_RESULT_INF) ? "is not in the subgroup of order r" : nullptr;
        if (what) {
            (void)hipFree(d_lines);
            set_error(std::string(who) + ": point " + std::to_string(j) + " " + what);
            return BBG_E_INVALID;
        }
    }
    bbg_g2_lines* h = new bbg_g2_lines;
    h->device = ctx->device;
    h->pairs = pairs;
    h->d_lines = d_lines;
    *out = h;
    return BBG_OK;
}

int g2_lines_read(const bbg_g2_lines* h, size_t which, uint64_t* out)
{
    if (!h || !out || which >= h->pairs) { set_error("bbg_g2_lines_read: null argument or no such point"); return BBG_E_INVALID; }
    BBG_HIP(hipSetDevice(h->device));
    BBG_HIP(hipMemcpy(out, (const char*)h->d_lines + which * PAIR_LINES_BYTES, PAIR_LINES_BYTES, hipMemcpyDeviceToHost));
    return BBG_OK;
}

void g2_lines_release(bbg_g2_lines* h)
{
    if (!h) return;
    if (hipSetDevice(h->device) == hipSuccess) (void)hipFree(h->d_lines);
    delete h;
}

// the argument checks of both forms that need no device pointer
int pairing_product_check(const char* who, const bbg_ctx* ctx, const bbg_g2_lines* h, const void* points, size_t count, const void* out, const void* status)
{
    const char* what = !h ? "null handle" : !points ? "null points" : (!out && !status) ? "both outputs are null" : (count == 0 || count > PAIR_MAX_COUNT) ? "count must be 1 .. 2^24"
                       : h->device != ctx->device ? "the handle was made on another device" : nullptr;
    if (!what) return BBG_OK;
    set_error(std::string(who) + ": " + what);
    return BBG_E_INVALID;
}

int pairing_product_run(bbg_ctx* ctx, const bbg_g2_lines* h, const void* d_g1, size_t count, void* d_out, void* d_status, hipStream_t st)
{
    const char* who = "bbg_pairing_product_device";
    if (int rc = pairing_product_check(who, ctx, h, d_g1, count, d_out, d_status)) return rc;
    const size_t in_bytes = count * h->pairs * 64;
    if ((d_out && ranges_overlap(d_out, count * 384, d_g1, in_bytes)) || (d_status && ranges_overlap(d_status, count * 4, d_g1, in_bytes)) ||
        (d_out && d_status && ranges_overlap(d_out, count * 384, d_status, count * 4))) {
        set_error(std::string(who) + ": an output overlaps the input or the other output");
        return BBG_E_INVALID;
    }
    // the working memory: pair_layout (work_layouts.h), six lane-interleaved Fq12 slots and one flag word per product of a chunk
    const size_t stride = pair_stride(count);
    const PairLayout L = pair_layout(stride, PairP::FINAL_SLOTS);
    if (int rc = ensure_layout(ctx->pairing_work, L.lay, who)) return rc;
    uint4* work = at<uint4>(ctx->pairing_work.p, L.work);
    uint32_t* flags = at<uint32_t>(ctx->pairing_work.p, L.flags);
    for (size_t from = 0; from < count; from += PAIR_CHUNK) {
        const size_t n = std::min(count - from, PAIR_CHUNK);
        {
            ProfScope ps(ctx, "pairing_miller", st);
            hipLaunchKernelGGL(k_pair_miller, dim3(grid_for(n, 64)), dim3(64), 0, st, (const char*)h->d_lines, (int)h->pairs, (const Affine*)d_g1 + from * h->pairs, n, work,
                               stride, flags);
        }
        {
            ProfScope ps(ctx, "pairing_final", st);
            hipLaunchKernelGGL(k_pair_final, dim3(grid_for(n, 64)), dim3(64), 0, st, work, stride, n, (const uint32_t*)flags, d_out ? (char*)d_out + from * 384 : nullptr,
                               d_status ? (uint32_t*)d_status + from : nullptr);
        }
    }
    BBG_HIP(hipGetLastError());
    return BBG_OK;
}

} // namespace bbg
