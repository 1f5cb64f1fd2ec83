// Opening proofs of a polynomial on every coset of its domain for gfx950 (bbg_open_all): the Feist-Khovratovich construction.  One
// pipeline for every cell size l = 2^log2cell: bbg_open_all_prepare is l = 1 (a proof per domain point), bbg_open_all_prepare_cells l >= 2.
//
// For f = sum_i f_i X^i of degree below n = 2^log2n, the points s_0 .. s_(n-l-1) of a string, r = n / l, w = w_n and phi = w^l, proof m < r
// belongs to the coset w^m <w^r> and is the commitment to q_m in f = q_m (X^l - phi^m) + I_m, deg I_m < l (l = 1: q_m = (f - f(w^m)) /
// (X - w^m)).  q_m has the coefficients q_j = sum_(k>=1) f_(j+kl) phi^(m(k-1)), so
//
//     proof_m = sum_(u=0)^(r-2) phi^(m u) h_u,      h_u = sum_(j=0)^(n-1-(u+1)l) f_(j+(u+1)l) s_j,   h_(r-1) = infinity:
//
// the proofs are the forward G1 NTT of size r of h.  With j = l a + b, f^(b)_i = f_(l i + b) and s^(b)_a = s_(l a + b), h = sum_(b<l) h^(b)
// and h^(b)_k = sum_(i=k+1)^(r-1) f^(b)_i s^(b)_(i-1-k): a Toeplitz matrix of the f^(b)_i applied to the s^(b)_a, once per residue class b
// -- the first r entries of a cyclic convolution of length 2r:
//
//     s^(b) = (s^(b)_(r-2), .., s^(b)_0, then r+1 infinities)          c^(b) = (f^(b)_(r-1), then r+1 zeros, then f^(b)_1, .., f^(b)_(r-2))
//     h     = the first r entries of iNTT_G1,2r( sum_b NTT_Fr,2r(c^(b)) o NTT_G1,2r(s^(b)) )
//
// (entry k of convolution b is sum_i c^_(k-i) s^_i over i <= r-2: c^_0 pairs s^_k = s^(b)_(r-2-k) with f^(b)_(r-1), and c^_(2r-d), d = i - k
// in 1 .. r-2, pairs s^(b)_(r-2-i) with f^(b)_(r-d) -- f^(b)_a s^(b)_(a-1-k) for every a in k+1 .. r-1; for k = r-1 every index k - i lands on
// a zero of c^.)  f_0 .. f_(l-1) are never read.  tests/tools/open_all_model.py (l = 1) and open_cells_model.py are this on the oracle's
// group operations, checked against the quotient definition; tests/test_open_cells_cpu.py holds the l = 1 layouts of the second to the first.
//
// The handle keeps s_hat[b 2r + i] = NTT_G1,2r(s^(b))[i], 2n affine points, infinities among them where they occur.  All l transforms are
// ONE pass of the stage kernels over an array of 2n: the first log2(2r) stages of a decimation-in-time schedule over 2n points are l
// independent transforms of the contiguous blocks of 2r (ecntt_stages_blocks; all the stages for l = 1), and because
// bitrev_2n(b 2r + i) = bitrev_2r(i) l + bitrev_l(b), ecntt_load over 2n leaves every block bit-reversed within itself when
// k_open_cells_srs lays the source out as src[k l + c] = s^(bitrev_l(c))[k].  A call over c polynomials then queues, on one stream and
// without a host synchronisation (open_all_queue):
//   * k_open_cells_coeffs     c_hat[b 2r + i] = c^(b)[i], and l Fr NTTs at 2r per polynomial on the contiguous blocks (ntt.hip) -- or, in a
//                             batched call, k_open_batch_ntt_lds, which does both in LDS;
//   * k_open_batch_pointwise  over all c 2n items with log2m = log2(2n): product (b, i) = c_hat * s_hat by xyzz_mul_glv lands at
//                             work2[bitrev_2r(i) l + bitrev_l(b)] of its polynomial by the same identity -- the l products of output index i
//                             contiguous, at the position the inverse stages want, written as XYZZ: no affine normalisation and no load
//                             pass in between.  The shape of the GLV stage kernel: a fixed number of 64-thread blocks, two waves per SIMD,
//                             lane t taking the items t, t + lanes, .., each lane with its 1 KiB table of odd multiples from var_base_tables;
//   * k_open_cells_sum        sum[k] = sum_(t<l) work2[k l + t], k < 2r, by the complete addition (l >= 2 only: for l = 1 work2 is the sum);
//   * the inverse stages at 2r (ecntt_stages_batch);
//   * k_open_all_fold         the first r entries, bit-reversed, into the size-r working array, still XYZZ;
//   * the forward stages at r;
//   * one normalisation, which writes a proof at infinity as aff_inf() (f of degree below l, for one).
#include "bbg_internal.h"
#include "work_layouts.h"
#include "curve.hip.h"
#include "ecntt.hip.h" // bit_reverse
#include "ntt_consts.hip.h" // DomainConsts, pow_from_table
#include "var_base.hip.h"

namespace bbg {

// src[k l + c] = s^(b)[k] with b = bitrev_l(c), k < 2r: s_(l (r-2-k) + b) for k <= r-2, aff_inf() above.  2n entries; l = 1 gives
// s^ = (s_(n-2), .., s_0, n+1 infinities) itself.
__global__ void __launch_bounds__(256) k_open_cells_srs(const Affine* __restrict__ srs, Affine* __restrict__ src, unsigned log2n, unsigned log2cell)
{
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n = (size_t)1 << log2n, r = n >> log2cell;
    if (j >= 2 * n) return;
    const size_t k = j >> log2cell, b = bit_reverse(j & (((size_t)1 << log2cell) - 1), log2cell);
    aff_store(src + j, k + 2 <= r ? aff_load(srs + (((r - 2 - k) << log2cell) + b)) : aff_inf());
}

// c^(b)[i], i < 2r, from the n coefficients at fp: f_(l (r-1) + b) at i = 0, f_(l (i-r-1) + b) for i = r+2 .. 2r-1, zero elsewhere.  The
// words are copied as they come (any representative).
__device__ __forceinline__ Fr open_coeff_entry(const Fr* __restrict__ fp, size_t i, size_t b, size_t r, unsigned log2cell)
{
    Fr v = Fr::zero();
    if (i == 0) v = fe_load<FrP>(fp + (((r - 1) << log2cell) + b));
    else if (i >= r + 2) v = fe_load<FrP>(fp + (((i - r - 1) << log2cell) + b));
    return v;
}

// c_hat[b 2r + i] = c^(b)[i], 2n entries.  `count` polynomials at f + p n give theirs at c_hat + p 2n: item g is entry g mod 2n of
// polynomial g / 2n.
__global__ void __launch_bounds__(256) k_open_cells_coeffs(const Fr* __restrict__ f, Fr* __restrict__ c_hat, unsigned log2n, unsigned log2cell, size_t count)
{
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n = (size_t)1 << log2n, r = n >> log2cell;
    if (g >= count * 2 * n) return;
    const size_t j = g & (2 * n - 1);
    const Fr* fp = f + ((g >> (log2n + 1)) << log2n);
    fe_store<FrP>(c_hat + g, open_coeff_entry(fp, j & (2 * r - 1), j >> (log2n - log2cell + 1), r, log2cell));
}

// The products of `count` polynomials in one launch: work[p 2^log2m + bitrev(i)] = c_hat[p 2^log2m + i] * s_hat[i] for the items
// g = p 2^log2m + i < items = count 2^log2m.  s_hat is indexed by i alone; a lane's items may lie in different polynomials.  Two waves per
// SIMD, no LDS, no scratch (the register budget of k_ecntt_stage_glv, whose loop body this is without the butterfly).
__global__ void __launch_bounds__(64, 2) k_open_batch_pointwise(const Affine* __restrict__ s_hat, const Fr* __restrict__ c_hat, Xyzz* __restrict__ work, unsigned log2m,
                                                                size_t items, Xyzz* __restrict__ tables)
{
    const size_t lanes = (size_t)gridDim.x * blockDim.x;
    const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    Xyzz* table = tables + (size_t)blockIdx.x * 64 * GLV_TABLE; // the wave's 64 tables (blocks of one wave): wave-uniform
#pragma unroll 1
    for (size_t g = lane; g < items; g += lanes) {
        const size_t i = g & (((size_t)1 << log2m) - 1);
        const Affine a = aff_load(s_hat + i);
        const Xyzz p = aff_is_inf(a) ? xyzz_inf() : xyzz_from_affine(a);
        const Fr k = fe_reduce_once(fe_from_mont(fe_load<FrP>(c_hat + g)));
        xyzz_store(work + (g - i) + bit_reverse(i, log2m), xyzz_mul_glv(p, k, table));
    }
}

// dst[p n + i] = src[p 2n + bitrev(i)], i < n = 2^log2n, p < count: the first half of each polynomial's 2n results as the input of its
// size-n transform
__global__ void __launch_bounds__(256) k_open_all_fold(const Xyzz* __restrict__ src, Xyzz* __restrict__ dst, unsigned log2n, size_t count)
{
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (count << log2n)) return;
    const size_t i = g & (((size_t)1 << log2n) - 1);
    xyzz_store(dst + g, xyzz_load(src + ((g - i) << 1) + bit_reverse(i, log2n)));
}

// The Fr transforms of a batched call, one per workgroup, in LDS.  Workgroup blockIdx.x = p l + b builds block b of polynomial p's c^
// vectors as it loads it (open_coeff_entry, the scatter of k_open_cells_coeffs), bit-reversed, runs the log2(2r) radix-2 stages of the
// decimation-in-time schedule with a barrier after each, and writes c_hat[(p l + b) 2r + i] in natural order: what ntt_run(BBG_FFT) leaves there up to the representative in [0, 2r), which the products reduce away.  2r x 32 B of
// dynamic LDS as two planes of 16 B words (ds_read_b128 / ds_write_b128 on consecutive addresses); w_2m^j from the 2r domain's table of
// root^(2^b), at most log2(2r) - 1 products per butterfly.  2r >= 4; the host takes this kernel up to 2r = 2^OPEN_BATCH_LDS_LOG2.
constexpr unsigned OPEN_BATCH_LDS_LOG2 = 12; // 2^12 x 32 B = 128 KiB of a CU's 160 KiB: one workgroup per CU there, two at 2^11
__device__ __forceinline__ Fr lds_fr_load(const uint4* lo, const uint4* hi, unsigned i)
{
    const uint4 a = lo[i], b = hi[i];
    Fr r;
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
    r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
    return r;
}
__device__ __forceinline__ void lds_fr_store(uint4* lo, uint4* hi, unsigned i, const Fr& x)
{
    lo[i] = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
    hi[i] = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
}
__global__ void __launch_bounds__(256) k_open_batch_ntt_lds(const Fr* __restrict__ f, Fr* __restrict__ c_hat, const DomainConsts* __restrict__ dc, unsigned log2n,
                                                            unsigned log2cell)
{
    extern __shared__ uint4 lds[];
    const unsigned log2b = log2n - log2cell + 1;
    const unsigned len = 1u << log2b, r = len >> 1;
    uint4* lo = lds;
    uint4* hi = lds + len;
    const size_t b = blockIdx.x & ((1u << log2cell) - 1);
    const Fr* fp = f + ((size_t)(blockIdx.x >> log2cell) << log2n);
    for (unsigned i = threadIdx.x; i < len; i += blockDim.x) lds_fr_store(lo, hi, (unsigned)bit_reverse(i, log2b), open_coeff_entry(fp, i, b, r, log2cell));
    __syncthreads();
    for (unsigned s = 0; s < log2b; s++) {
        const unsigned m = 1u << s;
        for (unsigned t = threadIdx.x; t < r; t += blockDim.x) {
            const unsigned j = t & (m - 1);
            const unsigned i = ((t >> s) << (s + 1)) + j;
            const Fr a = lds_fr_load(lo, hi, i);
            Fr x = lds_fr_load(lo, hi, i + m);
            if (j != 0) x = fe_mul(x, pow_from_table(dc->pow2_root, (uint64_t)j << (log2b - 1 - s))); // w_2m^j = w_2r^(j 2r / 2m)
            lds_fr_store(lo, hi, i, fe_add(a, x));
            lds_fr_store(lo, hi, i + m, fe_sub(a, x));
        }
        __syncthreads();
    }
    Fr* out = c_hat + ((size_t)blockIdx.x << log2b);
    for (unsigned i = threadIdx.x; i < len; i += blockDim.x) fe_store<FrP>(out + i, lds_fr_load(lo, hi, i));
}

// dst[k] = sum_(t < 2^log2cell) src[k 2^log2cell + t], k < count.  One thread per output, its entries added one after the other by
// the complete addition: designed inputs make them equal, opposite and infinite.  2n additions per call beside 2n multiplications of
// about 200 group operations each.
__global__ void __launch_bounds__(64) k_open_cells_sum(const Xyzz* __restrict__ src, Xyzz* __restrict__ dst, size_t count, unsigned log2cell)
{
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const Xyzz* seg = src + (k << log2cell);
    Xyzz acc = xyzz_load(seg);
#pragma unroll 1
    for (size_t t = 1; t < ((size_t)1 << log2cell); t++) acc = xyzz_add(acc, xyzz_load(seg + t));
    xyzz_store(dst + k, acc);
}

// ---------------------------------------------------------------------------------------------- host side
// The working arrays of a call, each for `cap` polynomials and polynomial-major, in ONE allocation: oa_layout (work_layouts.h) bound to
// its base.  The handle's own workspace is this at cap = 1, the batched calls' at the reservation.
static_assert(sizeof(Xyzz) == 128 && sizeof(Fr) == 32, "the workspace is laid out in 128 B points and 32 B scalars");
struct OpenAllWork {
    Xyzz *work2, *work1, *sum;
    Fr* c_hat;
    Xyzz* inv; // the inverse transforms' arrays: sum, or work2 for l = 1
};

static OpenAllWork open_all_work(void* base, size_t cap, unsigned log2n, unsigned log2cell)
{
    const OaLayout l = oa_layout(cap, log2n, log2cell);
    OpenAllWork w;
    w.work2 = at<Xyzz>(base, l.work2);
    w.work1 = at<Xyzz>(base, l.work1);
    w.sum = at<Xyzz>(base, l.sum);
    w.c_hat = at<Fr>(base, l.c_hat);
    w.inv = log2cell ? w.sum : w.work2;
    return w;
}

// the working arrays of one polynomial: what the handle holds beside s_hat
size_t open_all_batch_poly_bytes(unsigned log2n, unsigned log2cell) { return oa_layout(1, log2n, log2cell).lay.total(); }

// what the handle holds without a reservation: s_hat (2n affine points) and the workspace of one polynomial
size_t open_all_bytes(unsigned log2n, unsigned log2cell) { return ((size_t)2 << log2n) * 64 + open_all_batch_poly_bytes(log2n, log2cell); }

void open_all_release(struct bbg_open_all* h)
{
    if (h->s_hat) (void)hipFree(h->s_hat);
    if (h->own_ws) (void)hipFree(h->own_ws);
    if (h->batch_ws) (void)hipFree(h->batch_ws);
    delete h;
}

// The handle for 0 <= log2cell <= log2n - 1.  d_srs_points: at least 2^log2n - 2^log2cell plain affine points on the context's device, read
// once.  Synchronises the stream before it returns, so the caller may free the points at once.  `who`: the entry point, for the error text.
int open_all_prepare(bbg_ctx* ctx, const char* who, const void* d_srs_points, unsigned log2n, unsigned log2cell, struct bbg_open_all** out)
{
    const size_t n = (size_t)1 << log2n;
    hipStream_t st = ctx->stream;
    struct bbg_open_all* h = new struct bbg_open_all;
    h->ctx = ctx;
    h->log2n = log2n;
    h->log2cell = log2cell;
    int rc = BBG_OK;
    hipError_t e = hipMalloc(&h->s_hat, 2 * n * 64);
    if (e == hipSuccess) e = hipMalloc(&h->own_ws, open_all_batch_poly_bytes(log2n, log2cell));
    if (e != hipSuccess) rc = hip_fail(e, (std::string(who) + ": the handle's buffers").c_str(), __FILE__, __LINE__);
    if (rc == BBG_OK) {
        Xyzz* work2 = open_all_work(h->own_ws, 1, log2n, log2cell).work2;
        ProfScope ps(ctx, "open_all_prepare", st);
        hipLaunchKernelGGL(k_open_cells_srs, dim3(grid_for(2 * n, 256)), dim3(256), 0, st, (const Affine*)d_srs_points, (Affine*)h->s_hat, log2n, log2cell);
        {
            ProfScope stages(ctx, "ecntt_stages", st);
            rc = ecntt_load(h->s_hat, log2n + 1, work2, st); // every block of 2r bit-reversed within itself
            if (rc == BBG_OK) rc = ecntt_stages_blocks(ctx, work2, log2n + 1, log2n - log2cell + 1, st);
        }
        if (rc == BBG_OK) rc = ecntt_normalize(ctx, work2, 2 * n, h->s_hat, nullptr, st); // infinite outputs are kept as such
    }
    if (rc == BBG_OK) {
        e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = hip_fail(e, who, __FILE__, __LINE__);
    }
    if (rc) {
        open_all_release(h);
        return rc;
    }
    *out = h;
    return BBG_OK;
}

// c polynomials at d_coeffs through the working arrays `w` (of at least c polynomials), c x proofs points to d_out.  Queues only.
// lds_ok: the Fr transforms may take k_open_batch_ntt_lds.  Only the batched calls pass true; a single call must keep the scatter kernel
// and ntt_run (l calls at 2r): that is its measured route and its "open_all_coeffs" scope, and the tests check the LDS kernel against the
// single call -- through the same kernel they would compare a call with itself.
static int open_all_queue(struct bbg_open_all* h, const OpenAllWork& w, const void* d_coeffs, size_t c, bool lds_ok, void* d_out, hipStream_t st)
{
    bbg_ctx* ctx = h->ctx;
    const unsigned log2n = h->log2n, log2cell = h->log2cell, log2m = log2n + 1;
    const unsigned log2p = log2n - log2cell;       // proofs per polynomial: the forward transform's size (r)
    const unsigned log2b = log2p + 1;              // the Fr transforms' and the inverse transform's size (2r)
    const size_t m = (size_t)1 << log2m, proofs = (size_t)1 << log2p;
    // the largest table set of the call first (the stages ask for at most c m / 2 lanes): the buffer does not move between the launches
    size_t lanes = 0;
    void* tables = nullptr;
    int rc = var_base_tables(ctx, c * m, &lanes, &tables);
    if (rc) return rc;
    if (lds_ok && log2b <= OPEN_BATCH_LDS_LOG2) { // c l transforms of 2r points, one workgroup each, the scatter fused into the load
        void* consts = nullptr;
        rc = ntt_domain_consts(ctx, log2b, &consts);
        if (rc) return rc;
        const size_t lds_bytes = ((size_t)1 << log2b) * 32;
        if (lds_bytes > 64 * 1024 && !h->batch_lds_attr) {
            BBG_HIP(hipFuncSetAttribute((const void*)k_open_batch_ntt_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(((size_t)1 << OPEN_BATCH_LDS_LOG2) * 32)));
            h->batch_lds_attr = true;
        }
        ProfScope ps(ctx, "ntt_pass", st);
        hipLaunchKernelGGL(k_open_batch_ntt_lds, dim3((unsigned)(c << log2cell)), dim3(256), lds_bytes, st, (const Fr*)d_coeffs, w.c_hat, (const DomainConsts*)consts, log2n,
                           log2cell);
    } else { // a single call, or 2r x 32 B does not fit a workgroup's LDS: the scatter in one launch, then the transforms block by block
        {
            ProfScope ps(ctx, "open_all_coeffs", st);
            hipLaunchKernelGGL(k_open_cells_coeffs, dim3(grid_for(c * m, 256)), dim3(256), 0, st, (const Fr*)d_coeffs, w.c_hat, log2n, log2cell, c);
        }
        for (size_t t = 0; t < (c << log2cell); t++) {
            rc = ntt_run(ctx, w.c_hat + (t << log2b), log2b, BBG_FFT, 0, nullptr, st);
            if (rc) return rc;
        }
    }
    {
        ProfScope ps(ctx, "open_all_pointwise", st);
        hipLaunchKernelGGL(k_open_batch_pointwise, dim3((unsigned)(lanes / 64)), dim3(64), 0, st, (const Affine*)h->s_hat, (const Fr*)w.c_hat, w.work2, log2m, c * m,
                           (Xyzz*)tables);
    }
    if (log2cell) {
        ProfScope ps(ctx, "open_cells_sum", st);
        hipLaunchKernelGGL(k_open_cells_sum, dim3(grid_for(c * 2 * proofs, 64)), dim3(64), 0, st, (const Xyzz*)w.work2, w.sum, c * 2 * proofs, log2cell);
    }
    {
        ProfScope ps(ctx, "ecntt_stages", st);
        rc = ecntt_stages_batch(ctx, w.inv, log2b, c, 1, st);
        if (rc) return rc;
    }
    {
        ProfScope ps(ctx, "open_all_fold", st);
        hipLaunchKernelGGL(k_open_all_fold, dim3(grid_for(c * proofs, 256)), dim3(256), 0, st, (const Xyzz*)w.inv, w.work1, log2p, c);
    }
    {
        ProfScope ps(ctx, "ecntt_stages", st);
        rc = ecntt_stages_batch(ctx, w.work1, log2p, c, 0, st);
        if (rc) return rc;
    }
    rc = ecntt_normalize(ctx, w.work1, c * proofs, d_out, nullptr, st);
    if (rc) return rc;
    BBG_HIP(hipGetLastError());
    return BBG_OK;
}

// d_coeffs: 2^log2n Montgomery Fr (read only); d_out: 2^(log2n - log2cell) x 64 B.  Queues only.
int open_all_run(struct bbg_open_all* h, const void* d_coeffs, void* d_out, hipStream_t st)
{
    return open_all_queue(h, open_all_work(h->own_ws, 1, h->log2n, h->log2cell), d_coeffs, 1, false, d_out, st);
}

// ---------------------------------------------------------------------------------------------- many polynomials per call
// A single call is latency: its G1 stages are dependent launches over 2r and r points that leave the chip idle.  A batched call runs the
// same number of launches over c polynomials each, on a workspace of its own that the handle owns beside the single call's; c is at most
// what OPEN_BATCH_BUDGET holds, and a call walks its polynomials in chunks of c.
constexpr size_t OPEN_BATCH_BUDGET = (size_t)1 << 30;

size_t open_all_batch_cap(unsigned log2n, unsigned log2cell)
{
    return std::max<size_t>(1, OPEN_BATCH_BUDGET / open_all_batch_poly_bytes(log2n, log2cell));
}

// the workspace for min(polys, the cap) polynomials; 0 releases it.  Replacing one waits for the device: queued calls may still use it.
int open_all_batch_reserve(struct bbg_open_all* h, size_t polys)
{
    polys = std::min(polys, open_all_batch_cap(h->log2n, h->log2cell));
    if (polys == h->batch_cap) return BBG_OK;
    if (h->batch_ws) {
        BBG_HIP(hipDeviceSynchronize());
        void* old = h->batch_ws;
        h->batch_ws = nullptr;
        h->batch_cap = 0;
        BBG_HIP(hipFree(old));
    }
    if (polys == 0) return BBG_OK;
    const RegionLayout lay = oa_layout(polys, h->log2n, h->log2cell).lay;
    if (!lay.ok()) { set_error("bbg_open_all_batch_reserve: size out of range"); return BBG_E_INVALID; }
    hipError_t e = hipMalloc(&h->batch_ws, lay.total());
    if (e != hipSuccess) {
        h->batch_ws = nullptr;
        (void)hipGetLastError(); // the handle stays usable: a single call ends in a hipGetLastError of its own
        return hip_fail(e, "bbg_open_all_batch_reserve: the workspace", __FILE__, __LINE__);
    }
    h->batch_cap = polys;
    return BBG_OK;
}

// d_coeffs: count x 2^log2n Montgomery Fr, polynomial-major (read only); d_out: count x proofs x 64 B.  A handle without a reservation
// reserves min(count, the cap) first.  Queues only.
int open_all_batch_run(struct bbg_open_all* h, const void* d_coeffs, size_t count, void* d_out, hipStream_t st)
{
    if (!h->batch_cap) {
        int rc = open_all_batch_reserve(h, count);
        if (rc) return rc;
    }
    const size_t n = (size_t)1 << h->log2n, proofs = n >> h->log2cell;
    const OpenAllWork w = open_all_work(h->batch_ws, h->batch_cap, h->log2n, h->log2cell);
    for (size_t done = 0; done < count; done += h->batch_cap) {
        const size_t c = std::min(h->batch_cap, count - done);
        int rc = open_all_queue(h, w, (const char*)d_coeffs + done * n * 32, c, true, (char*)d_out + done * proofs * 64, st);
        if (rc) return rc;
    }
    return BBG_OK;
}

} // namespace bbg
