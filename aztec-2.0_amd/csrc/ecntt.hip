// Lagrange-base transform of a reference string for gfx950: an inverse NTT whose elements are BN254 G1 points.
//
// Computes what lagrange_base::transform_srs computes (reference srs/lagrange_base_transformation/lagrange_base.cpp:6-46): for
// n = 2^log2n and the monomial points M_0 .. M_{n-1}
//
//     LB[k] = n^-1 * sum_j w_n^(-j k) * M_j        k = 0 .. n-1, natural order, affine
//
// with w_n = fr::get_root_of_unity(log2n), so that LB[k] = [L_k(x)] G when M_j = [x^j] G.  (The reference's recursive g1fft starts its
// running twiddle at `root`, not 1: its result[i] is the value at root^(i+1), and transform_srs rotates the indices by one to get
// back to natural order, :41-45.)
//
// The reference recurses on one thread and does n/2 log2 n + n full scalar multiplications.  Here:
//   * k_ecntt_load     copies the source points, bit-reversed, into a working set of n XYZZ points (128 B each) the call owns;
//   * k_ecntt_stage    one launch per radix-2 stage of a decimation-in-time schedule, one butterfly per thread, in place:
//                      t = w B, A' = A + t, B' = A - t.  w = w_n^(-j n/2m) is rebuilt from the domain's table of root_inv^(2^b)
//                      (at most log2 n Fr products beside 254 doublings), taken out of Montgomery form and used as a plain 254-bit
//                      integer by a left-to-right double-and-add on the complete XYZZ formulas of curve.hip.h.  Butterflies whose
//                      twiddle is 1 skip the multiplication (all of stage 0).  The LAST stage carries n^-1: its twiddles are n^-1 w
//                      and its A operands are multiplied by n^-1 (n/2 extra scalar multiplications, 1 / log2 n of the work, and no
//                      pass of its own).  By default (option "ecntt_mul" = 1) the stages run on the windowed GLV multiplication of
//                      var_base.hip.h instead (k_ecntt_stage_glv: 2.2x at 2^20, profiles/var_base.txt); 0 = this kernel, A/B;
//   * k_ecntt_normalize  batched conversion to canonical affine (aff_batch_*, curve.hip.h), one inversion per NORM_CH points;
//                      a point at infinity among the outputs raises a flag (an SRS handle never holds one) and the call fails.
// All group-law cases (equal / opposite operands, infinities inside the transform) are handled by xyzz_add / xyzz_dbl.
//
// The same three steps, each callable on its own (ecntt_load / ecntt_stages / ecntt_normalize), also make the general transform behind
// bbg_g1_ntt and the two transforms inside bbg_open_all (open_all.hip), which runs the stages on XYZZ working arrays it already holds:
//   * the stage kernels take the direction as a template parameter.  <true> is the inverse described above; <false> is the forward
//     transform out[k] = sum_j w_n^(jk) P_j: twiddles from the table of root^(2^b), and no n^-1 in the last stage;
//   * k_ecntt_normalize<true> stores a point at infinity as aff_inf() and raises no flag;
//   * ecntt_stages_blocks stops the forward stages early: many independent transforms of contiguous blocks in one pass (the cell handle
//     of open_all.hip prepares its strings that way);
//   * ecntt_stages_batch runs ALL stages of a small domain over any number of contiguous blocks, in either direction: the stage kernels
//     take the number of butterflies, not the array length (the batched calls of open_all.hip).
#include "bbg_internal.h"
#include "curve.hip.h"
#include "ecntt.hip.h" // bit_reverse
#include "ntt_consts.hip.h"
#include "var_base.hip.h" // xyzz_mul_fr, xyzz_mul_glv, xyzz_neg

namespace bbg {

// work[i] = M[bitrev(i)] in XYZZ form (the input permutation of the decimation-in-time schedule)
__global__ void __launch_bounds__(256) k_ecntt_load(const Affine* __restrict__ src, Xyzz* __restrict__ work, unsigned log2n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ((size_t)1 << log2n)) return;
    const Affine a = aff_load(src + bit_reverse(i, log2n));
    xyzz_store(work + i, aff_is_inf(a) ? xyzz_inf() : xyzz_from_affine(a));
}

// stage s (half-size m = 2^s) of the transform, in place; thread t owns the butterfly (i, i + m), i = (t / m) 2m + t % m.
// Two waves per SIMD: 246 VGPRs, no scratch, no LDS; three would cap the kernel at 168 VGPRs and spill inside the multiplication loop
// (A/B: make EXTRA=-DBBG_ECNTT_OCC=3).
#ifndef BBG_ECNTT_OCC
#define BBG_ECNTT_OCC 2
#endif
// INV: the inverse transform (twiddles w_n^-1, n^-1 folded into the last stage); the forward one ignores `last`.
// `butterflies` is n / 2 for one transform; count n / 2 walks `count` contiguous blocks of n points, each a transform of its own: i runs
// on through block after block and the twiddle depends on j alone (ecntt_stages_batch).  Registers: profiles/open_batch.txt.
template <bool INV>
__global__ void __launch_bounds__(64, BBG_ECNTT_OCC) k_ecntt_stage(Xyzz* __restrict__ work, const DomainConsts* __restrict__ dc, unsigned log2n, unsigned s, int last,
                                                                   size_t butterflies)
{
    if (!INV) last = 0;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= butterflies) return;
    const size_t m = (size_t)1 << s;
    const size_t j = t & (m - 1);
    const size_t i = ((t >> s) << (s + 1)) + j;
    Xyzz b = xyzz_load(work + i + m);
    if (last || j != 0) {
        Fr w = pow_from_table(INV ? dc->pow2_root_inv : dc->pow2_root, (uint64_t)j << (log2n - 1 - s)); // w_2m^-j = w_n^(-j n / 2m); forward: w_2m^j
        if (last) w = fe_mul(w, dc->n_inv);
        b = xyzz_mul_fr(b, fe_reduce_once(fe_from_mont(w)));
    }
    Xyzz a = xyzz_load(work + i);
    if (last) a = xyzz_mul_fr(a, fe_reduce_once(fe_from_mont(dc->n_inv)));
    xyzz_store(work + i, xyzz_add(a, b));
    xyzz_store(work + i + m, xyzz_add(a, xyzz_neg(b)));
}

// The same stage on the windowed GLV multiplication of var_base.hip.h (option "ecntt_mul" = 1, the default): a fixed number of lanes, each with its
// 1 KiB table of odd multiples in `tables`, lane t taking the butterflies t, t + lanes, ..  Bit-identical to k_ecntt_stage after the
// normalisation (the same group elements in another XYZZ representation).
template <bool INV>
__global__ void __launch_bounds__(64, BBG_ECNTT_OCC) k_ecntt_stage_glv(Xyzz* __restrict__ work, const DomainConsts* __restrict__ dc, unsigned log2n, unsigned s, int last,
                                                                       size_t butterflies, Xyzz* __restrict__ tables)
{
    if (!INV) last = 0;
    const size_t lanes = (size_t)gridDim.x * blockDim.x;
    const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    Xyzz* table = tables + (size_t)blockIdx.x * 64 * GLV_TABLE; // the wave's 64 tables (blocks of one wave): wave-uniform
    const size_t m = (size_t)1 << s;
#pragma unroll 1
    for (size_t t = lane; t < butterflies; t += lanes) {
        const size_t j = t & (m - 1);
        const size_t i = ((t >> s) << (s + 1)) + j;
        Xyzz b = xyzz_load(work + i + m);
        if (last || j != 0) {
            Fr w = pow_from_table(INV ? dc->pow2_root_inv : dc->pow2_root, (uint64_t)j << (log2n - 1 - s)); // w_2m^-j = w_n^(-j n / 2m); forward: w_2m^j
            if (last) w = fe_mul(w, dc->n_inv);
            b = xyzz_mul_glv(b, fe_reduce_once(fe_from_mont(w)), table);
        }
        Xyzz a = xyzz_load(work + i);
        if (last) a = xyzz_mul_glv(a, fe_reduce_once(fe_from_mont(dc->n_inv)), table);
        xyzz_store(work + i, xyzz_add(a, b));
        xyzz_store(work + i + m, xyzz_add(a, xyzz_neg(b)));
    }
}

// XYZZ -> canonical affine, NORM_CH consecutive points per thread behind one inversion (the batched conversion of curve.hip.h).  A
// point at infinity is reported through *inf_flag and stored as the generator, so that whatever is queued behind this kernel still
// reads valid points; the host discards the result.  INF_OK: a point at infinity is an ordinary output, stored as aff_inf(); no flag.
constexpr int NORM_CH = 8;
template <bool INF_OK>
__global__ void __launch_bounds__(128) k_ecntt_normalize(const Xyzz* __restrict__ work, Affine* __restrict__ out, size_t n, unsigned* inf_flag)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t i0 = t * NORM_CH;
    if (i0 >= n) return;
    // only the prefix products are kept per thread: ZZ ZZZ and the finite flag of a point are taken from `work` again on the way back
    Fq prefix[NORM_CH];
    Fq run = Fq::one();
    int cnt = 0;
    bool any_inf = false;
    for (int e = 0; e < NORM_CH && i0 + e < n; e++) {
        Fq zw;
        any_inf |= !aff_batch_park(xyzz_load(work + i0 + e), out + i0 + e, zw, prefix[e], run);
        cnt++;
    }
    Fq inv = aff_batch_invert(run);
    for (int e = cnt - 1; e >= 0; e--) {
        const Fq zz = fe_load<FqP>(&work[i0 + e].zz), zzz = fe_load<FqP>(&work[i0 + e].zzz);
        aff_batch_finish(out + i0 + e, !zz.is_zero_raw(), fe_mul(zz, zzz), prefix[e], inv, INF_OK ? aff_inf() : aff_generator());
    }
    if (!INF_OK && any_inf) atomicOr(inf_flag, 1u);
}

// work[i] = src[bitrev(i)] in XYZZ form on `st`: d_src = 2^log2n plain affine points (read only, aff_inf() allowed), d_work = 2^log2n x 128 B.
int ecntt_load(const void* d_src, unsigned log2n, void* d_work, hipStream_t st)
{
    const size_t n = (size_t)1 << log2n;
    hipLaunchKernelGGL(k_ecntt_load, dim3(grid_for(n, 256)), dim3(256), 0, st, (const Affine*)d_src, (Xyzz*)d_work, log2n);
    BBG_HIP(hipGetLastError());
    return BBG_OK;
}

// The first `stages` of the log2n stages on `st`, in place on d_work, over `count` contiguous blocks of n = 2^log2n points: count n / 2
// butterflies per stage.  The lanes' tables come from the context (var_base_tables) under "ecntt_mul" = 1.
static int ecntt_stages_upto(bbg_ctx* ctx, void* d_work, unsigned log2n, size_t count, int inverse, unsigned stages, hipStream_t st)
{
    if (log2n < 1 || log2n > 28) { set_error("ecntt: log2n out of range (1 .. 28)"); return BBG_E_INVALID; }
    const size_t butterflies = count << (log2n - 1);
    void* consts = nullptr;
    int rc = ntt_domain_consts(ctx, log2n, &consts); // root^(2^b), root_inv^(2^b) and n^-1 of the scalar NTT's domain
    if (rc) return rc;
    size_t lanes = 0;
    void* tables = nullptr;
    if (ctx->ecntt_mul) { // the lanes' tables of odd multiples (var_base.hip)
        rc = var_base_tables(ctx, butterflies, &lanes, &tables);
        if (rc) return rc;
    }
    auto glv = inverse ? k_ecntt_stage_glv<true> : k_ecntt_stage_glv<false>;
    auto serial = inverse ? k_ecntt_stage<true> : k_ecntt_stage<false>;
    for (unsigned s = 0; s < stages; s++) {
        const int last = s + 1 == log2n ? 1 : 0;
        if (ctx->ecntt_mul)
            hipLaunchKernelGGL(glv, dim3((unsigned)(lanes / 64)), dim3(64), 0, st, (Xyzz*)d_work, (const DomainConsts*)consts, log2n, s, last, butterflies,
                               (Xyzz*)tables);
        else
            hipLaunchKernelGGL(serial, dim3(grid_for(butterflies, 64)), dim3(64), 0, st, (Xyzz*)d_work, (const DomainConsts*)consts, log2n, s, last, butterflies);
    }
    BBG_HIP(hipGetLastError());
    return BBG_OK;
}

// The log2n stages on `st`, in place on d_work (2^log2n XYZZ points in bit-reversed order; natural order afterwards).  inverse != 0: with
// w_n^-1 and n^-1, else with w_n and no scaling.
int ecntt_stages(bbg_ctx* ctx, void* d_work, unsigned log2n, int inverse, hipStream_t st)
{
    return ecntt_stages_upto(ctx, d_work, log2n, 1, inverse, log2n, st);
}

// 2^(log2n - log2block) independent FORWARD transforms of 2^log2block points each, in place on the contiguous blocks of d_work (each
// bit-reversed within itself): the first log2block stages of the schedule over the whole array.  Stage s takes w_2m^j, m = 2^s, whatever
// the array length -- the stage kernels rebuild it from the 2^log2n domain's table as j << (log2n - 1 - s).  The inverse folds n^-1 into
// its last stage and has no such form: ecntt_stages_batch below is the one for it.
int ecntt_stages_blocks(bbg_ctx* ctx, void* d_work, unsigned log2n, unsigned log2block, hipStream_t st)
{
    if (log2block < 1 || log2block > log2n) { set_error("ecntt: block size out of range"); return BBG_E_INVALID; }
    return ecntt_stages_upto(ctx, d_work, log2n, 1, 0, log2block, st);
}

// `count` independent transforms of 2^log2block points each, any count >= 1, in EITHER direction, in place on the contiguous blocks of
// d_work (each bit-reversed within itself, natural order afterwards): ALL log2block stages of the 2^log2block domain with the butterfly
// index running to count 2^(log2block - 1).  Butterfly t has j = t mod m and i = (t / m) 2m + j: t / m runs through the pairs of one
// block and on into the next, since a block is a whole number of pairs at every stage, and the twiddle is w_2m^(+-j) whatever the block.
// The last stage is the domain's last, so the inverse's n^-1 is that of 2^log2block.  One launch per stage whatever the count.
int ecntt_stages_batch(bbg_ctx* ctx, void* d_work, unsigned log2block, size_t count, int inverse, hipStream_t st)
{
    if (count == 0 || count > ((size_t)1 << 40)) { set_error("ecntt: batch count out of range"); return BBG_E_INVALID; }
    return ecntt_stages_upto(ctx, d_work, log2block, count, inverse, log2block, st);
}

// d_out[i] = d_work[i] as canonical affine on `st`, n points.  d_inf_flag != null: a point at infinity sets *d_inf_flag (cleared by the
// caller on `st`) and is stored as the generator; null: it is stored as aff_inf().
int ecntt_normalize(bbg_ctx* ctx, const void* d_work, size_t n, void* d_out, unsigned* d_inf_flag, hipStream_t st)
{
    ProfScope ps(ctx, "ecntt_normalize", st);
    const dim3 grid(grid_for((n + NORM_CH - 1) / NORM_CH, 128));
    if (d_inf_flag)
        hipLaunchKernelGGL(k_ecntt_normalize<false>, grid, dim3(128), 0, st, (const Xyzz*)d_work, (Affine*)d_out, n, d_inf_flag);
    else
        hipLaunchKernelGGL(k_ecntt_normalize<true>, grid, dim3(128), 0, st, (const Xyzz*)d_work, (Affine*)d_out, n, (unsigned*)nullptr);
    BBG_HIP(hipGetLastError());
    return BBG_OK;
}

// Queues the whole transform on `st`: d_src = 2^log2n plain affine points (read only), d_work = 2^log2n x 128 B, d_out = 2^log2n x 64 B
// (may be d_src), d_inf_flag = one word the caller has cleared on `st`, or null (ecntt_normalize).  No host synchronisation.
int ecntt_run(bbg_ctx* ctx, const void* d_src, unsigned log2n, int inverse, void* d_work, void* d_out, unsigned* d_inf_flag, hipStream_t st)
{
    if (log2n < 1 || log2n > 28) { set_error("ecntt: log2n out of range (1 .. 28)"); return BBG_E_INVALID; }
    {
        ProfScope ps(ctx, "ecntt_stages", st);
        int rc = ecntt_load(d_src, log2n, d_work, st);
        if (rc == BBG_OK) rc = ecntt_stages(ctx, d_work, log2n, inverse, st);
        if (rc) return rc;
    }
    return ecntt_normalize(ctx, d_work, (size_t)1 << log2n, d_out, d_inf_flag, st);
}

} // namespace bbg
