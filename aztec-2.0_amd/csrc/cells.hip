// Cells of a polynomial: the values of every cell, and the polynomial back from a subset of its cells (erasure decoding).
// Notation as in open_all.hip's cell handle: n = 2^log2n, l = 2^log2cell, r = n / l, w = w_n, phi = w^l; cell m < r is the coset
// { w^(m + r t) : t < l }.  With K known cells m_0 .. m_(K-1), M the r - K missing ones and
//   Z(X) = prod_{m in M} (X^l - phi^m)
// Z depends on X only through X^l, so on the domain and on its coset g <w> it takes r values each:
//   Z(w^i)   = Zdom[i mod r],  Zdom[j] = prod_{m in M} (phi^j - phi^m)         (zero exactly on the missing cells)
//   Z(g w^i) = Zcos[i mod r],  Zcos[j] = prod_{m in M} (g^l phi^j - phi^m)     (never zero: g^n != 1)
// and the interpolant f* of degree < K l through the K l known values comes from f* Z, which has degree < n and equals (known value) *
// Zdom on the whole domain, the missing cells taken as zero:
//   A[i] = E[i] Zdom[i mod r]   ->   D = iNTT(A)   ->   B = cosetNTT(D),  B[i] /= Zcos[i mod r]   ->   f* = cosetiNTT(B).
// This file: the kernels, their launches and the argument checks; the C ABI (bbg_capi.hip) holds the context lock and stages host arrays.
#include "bbg_internal.h"
#include "work_layouts.h"

#include "ntt_consts.hip.h"

namespace bbg {

// ---------------------------------------------------------------------------------------------- the points Z is evaluated at
// roots[q] = phi^missing[q], q < nm; pts[j] = g^l phi^j, j < r; pts[r + k] = phi^ids[k], k < K.  All canonical.
__global__ void __launch_bounds__(256) k_cells_points(const DomainConsts* dc, unsigned log2cell, unsigned r, unsigned nm, unsigned K,
                                                      const uint32_t* __restrict__ missing, const uint32_t* __restrict__ ids, Fr* roots, Fr* pts)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const Fr* phi_pow2 = dc->pow2_root + log2cell; // phi^(2^b) = w^(2^(b + log2cell)); exponents stay below r, so b + log2cell < log2n <= 28
    if (i < nm) {
        fe_store<FrP>(roots + i, fe_reduce_once(pow_from_table(phi_pow2, missing[i])));
        return;
    }
    const size_t o = i - nm;
    if (o < r) {
        Fr gl = dc->gen;
        for (unsigned b = 0; b < log2cell; b++) gl = fe_sqr(gl);
        fe_store<FrP>(pts + o, fe_reduce_once(fe_mul(gl, pow_from_table(phi_pow2, o))));
    } else if (o < (size_t)r + K) {
        fe_store<FrP>(pts + o, fe_reduce_once(pow_from_table(phi_pow2, ids[o - r])));
    }
}

// ---------------------------------------------------------------------------------------------- Z at those points
// z[o] = prod_{q < nm} (pts[o] - roots[q]), o < nout.  One wave per CZ_OUT outputs: lane t takes roots t, t + 64, .. into CZ_OUT independent
// chains (one root read feeds CZ_OUT products), then the 64 partial products of each output meet in six shuffle rounds.  The block's four waves
// share the roots through LDS, CZ_CHUNK at a time.  A lane that meets no root holds one; nm = 0 gives z = 1.
constexpr int CZ_OUT = 4, CZ_CHUNK = 1024, CZ_BLOCK_OUT = 4 * CZ_OUT;
__device__ __forceinline__ Fr wave_product(Fr s)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        Fr o;
#pragma unroll
        for (int w = 0; w < 8; w++) o.v[w] = (uint32_t)__shfl_xor((int)s.v[w], d, 64);
        s = fe_mul(s, o);
    }
    return s;
}
__global__ void __launch_bounds__(256) k_cells_z(const Fr* __restrict__ roots, unsigned nm, const Fr* __restrict__ pts, Fr* z, unsigned nout)
{
    __shared__ Fr sh[CZ_CHUNK];
    const unsigned tid = threadIdx.x, lane = tid & 63;
    const size_t o0 = ((size_t)blockIdx.x * 4 + (tid >> 6)) * CZ_OUT;
    Fr x[CZ_OUT], acc[CZ_OUT];
#pragma unroll
    for (int e = 0; e < CZ_OUT; e++) {
        x[e] = o0 + e < nout ? fe_load<FrP>(pts + o0 + e) : Fr::one(); // past the end: computed like the rest (the block's barriers), not stored
        acc[e] = Fr::one();
    }
    for (unsigned c0 = 0; c0 < nm; c0 += CZ_CHUNK) {
        const unsigned lim = nm - c0 < (unsigned)CZ_CHUNK ? nm - c0 : (unsigned)CZ_CHUNK;
        __syncthreads(); // the chunk before this one has been read
        for (unsigned q = tid; q < lim; q += 256) sh[q] = fe_load<FrP>(roots + c0 + q);
        __syncthreads();
        for (unsigned q = lane; q < lim; q += 64) {
            const Fr rt = sh[q];
#pragma unroll
            for (int e = 0; e < CZ_OUT; e++) acc[e] = fe_mul(acc[e], fe_sub(x[e], rt));
        }
    }
#pragma unroll
    for (int e = 0; e < CZ_OUT; e++) {
        const Fr p = wave_product(acc[e]);
        if (lane == 0 && o0 + e < nout) fe_store<FrP>(z + o0 + e, fe_reduce_once(p));
    }
}

// ---------------------------------------------------------------------------------------------- domain order <-> cell-major
// Domain order i = m + r t is an l x r matrix (row t), cell-major m l + t its transpose: one 16 x 16 tile of 32-byte elements per block through
// LDS, 512 contiguous bytes per row on both sides.  blockIdx.y = the polynomial.
//   GATHER  (SCATTER = false): out[p n + m l + t] = in[p n + m + r t], canonical
//   SCATTER (SCATTER = true):  out[p n + m + r t] = in[(p K + slot[m]) l + t] * zdom[slot[m]], canonical; zero where slot[m] < 0
constexpr int CT = 16;
template <bool SCATTER>
__global__ void __launch_bounds__(CT * CT) k_cells_transpose(const Fr* __restrict__ in, Fr* __restrict__ out, unsigned log2r, unsigned log2l, unsigned K,
                                                             const int32_t* __restrict__ slot, const Fr* __restrict__ zdom)
{
    __shared__ Fr tile[CT][CT + 1];
    const size_t r = (size_t)1 << log2r, l = (size_t)1 << log2l, n = r * l;
    const size_t tiles_m = (r + CT - 1) / CT;
    const size_t m0 = (blockIdx.x % tiles_m) * CT, t0 = (blockIdx.x / tiles_m) * CT;
    const unsigned tx = threadIdx.x % CT, ty = threadIdx.x / CT;
    const Fr* src = in + (size_t)blockIdx.y * (SCATTER ? (size_t)K * l : n);
    Fr* dst = out + (size_t)blockIdx.y * n;
    if (SCATTER) {
        const size_t m = m0 + ty, t = t0 + tx;
        if (m < r && t < l) {
            const int32_t k = slot[m];
            tile[ty][tx] = k >= 0 ? fe_mul(fe_load<FrP>(src + (size_t)k * l + t), fe_load<FrP>(zdom + k)) : Fr::zero();
        }
    } else {
        const size_t m = m0 + tx, t = t0 + ty;
        if (m < r && t < l) tile[ty][tx] = fe_load<FrP>(src + t * r + m);
    }
    __syncthreads();
    if (SCATTER) {
        const size_t m = m0 + tx, t = t0 + ty;
        if (m < r && t < l) fe_store<FrP>(dst + t * r + m, fe_reduce_once(tile[tx][ty]));
    } else {
        const size_t m = m0 + ty, t = t0 + tx;
        if (m < r && t < l) fe_store<FrP>(dst + m * l + t, fe_reduce_once(tile[tx][ty]));
    }
}

// b[p n + i] <- b[p n + i] * inv_zcos[i mod r], canonical; with inv_zcos = null only the canonical form (the last transform leaves [0, 2r))
__global__ void __launch_bounds__(256) k_cells_divide(Fr* b, size_t n, unsigned rmask, const Fr* __restrict__ inv_zcos)
{
    Fr* a = b + (size_t)blockIdx.y * n;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        Fr v = fe_load<FrP>(a + i);
        if (inv_zcos) v = fe_mul(v, fe_load<FrP>(inv_zcos + (i & rmask)));
        fe_store<FrP>(a + i, fe_reduce_once(v));
    }
}

// ---------------------------------------------------------------------------------------------- host side
static unsigned transpose_grid(unsigned log2r, unsigned log2l)
{
    const size_t r = (size_t)1 << log2r, l = (size_t)1 << log2l;
    return (unsigned)(((r + CT - 1) / CT) * ((l + CT - 1) / CT)); // at most 2^28 / 16 blocks (l = 1)
}
static unsigned sweep_grid(size_t n) { return (unsigned)std::min<size_t>((n + 255) / 256, 256 * 16); }

int cells_check_shape(const char* who, unsigned log2n, unsigned log2cell, size_t count)
{
    if (int rc = check_log2n(who, log2n, 1, 28)) return rc;
    if (log2cell > log2n - 1) { set_error(std::string(who) + ": log2cell must be 0 .. log2n - 1"); return BBG_E_INVALID; }
    if (count < 1 || count > (size_t)BARY_MAX) { set_error(std::string(who) + ": count must be 1 .. 32"); return BBG_E_INVALID; }
    return BBG_OK;
}
int cells_check_ids(const char* who, const uint32_t* cell_ids, size_t K, unsigned log2n, unsigned log2cell)
{
    const size_t r = (size_t)1 << (log2n - log2cell);
    if (!cell_ids) { set_error(std::string(who) + ": null cell_ids"); return BBG_E_INVALID; }
    if (K < 1 || K > r) { set_error(std::string(who) + ": K must be 1 .. r = n / l"); return BBG_E_INVALID; }
    std::vector<bool> seen(r, false);
    for (size_t k = 0; k < K; k++) {
        if (cell_ids[k] >= r) { set_error(std::string(who) + ": a cell id is not below r = n / l"); return BBG_E_INVALID; }
        if (seen[cell_ids[k]]) { set_error(std::string(who) + ": a cell id appears twice"); return BBG_E_INVALID; }
        seen[cell_ids[k]] = true;
    }
    return BBG_OK;
}

// The context's pinned array with at least `bytes`, free to be written: the event says when the copy of the call before this one is
// through with it.  The caller records ctx->cells_copied behind its own copy.
int cells_pinned_ensure(bbg_ctx* ctx, size_t bytes)
{
    if (ctx->cells_pinned_bytes < bytes) {
        if (ctx->cells_pinned) {
            BBG_HIP(hipEventSynchronize(ctx->cells_copied));
            void* old = ctx->cells_pinned;
            ctx->cells_pinned = nullptr;
            ctx->cells_pinned_bytes = 0;
            BBG_HIP(hipHostFree(old));
        }
        if (!ctx->cells_copied) BBG_HIP(hipEventCreateWithFlags(&ctx->cells_copied, hipEventDisableTiming));
        BBG_HIP(hipHostMalloc(&ctx->cells_pinned, bytes, hipHostMallocDefault));
        ctx->cells_pinned_bytes = bytes;
    } else {
        BBG_HIP(hipEventSynchronize(ctx->cells_copied));
    }
    return BBG_OK;
}

int cells_values(bbg_ctx* ctx, const void* d_coeffs, unsigned log2n, unsigned log2cell, size_t count, void* d_out, hipStream_t st)
{
    if (!d_coeffs || !d_out) { set_error("bbg_cells_values_device: null argument"); return BBG_E_INVALID; }
    if (int rc = cells_check_shape("bbg_cells_values_device", log2n, log2cell, count)) return rc;
    const size_t n = (size_t)1 << log2n;
    if (ranges_overlap(d_coeffs, count * n * 32, d_out, count * n * 32)) { set_error("bbg_cells_values_device: the output overlaps the coefficients"); return BBG_E_INVALID; }
    if (int rc = ctx->cells_work.ensure(n * 32)) return rc;
    Fr* work = (Fr*)ctx->cells_work.p;
    for (size_t p = 0; p < count; p++) { // one transform at a time through the one working array: the stream orders them
        BBG_HIP(hipMemcpyAsync(work, (const Fr*)d_coeffs + p * n, n * 32, hipMemcpyDeviceToDevice, st));
        if (int rc = ntt_run(ctx, work, log2n, BBG_FFT, 0, nullptr, st)) return rc;
        ProfScope ps(ctx, "cells_gather", st);
        hipLaunchKernelGGL(k_cells_transpose<false>, dim3(transpose_grid(log2n - log2cell, log2cell)), dim3(CT * CT), 0, st, (const Fr*)work,
                           (Fr*)d_out + p * n, log2n - log2cell, log2cell, 0u, (const int32_t*)nullptr, (const Fr*)nullptr);
    }
    BBG_HIP(hipGetLastError());
    return BBG_OK;
}

int cells_recover(bbg_ctx* ctx, const uint32_t* cell_ids, size_t K, const void* d_values, unsigned log2n, unsigned log2cell, size_t count,
                  void* d_out_coeffs, hipStream_t st)
{
    const char* who = "bbg_cells_recover_device";
    if (!d_values || !d_out_coeffs) { set_error(std::string(who) + ": null argument"); return BBG_E_INVALID; }
    if (int rc = cells_check_shape(who, log2n, log2cell, count)) return rc;
    if (int rc = cells_check_ids(who, cell_ids, K, log2n, log2cell)) return rc;
    const unsigned log2r = log2n - log2cell;
    const size_t n = (size_t)1 << log2n, l = (size_t)1 << log2cell, r = (size_t)1 << log2r, nm = r - K, nout = r + K;
    if (ranges_overlap(d_values, count * K * l * 32, d_out_coeffs, count * n * 32)) { set_error(std::string(who) + ": the output overlaps the values"); return BBG_E_INVALID; }
    void* dc = nullptr;
    if (int rc = ntt_domain_consts(ctx, log2n, &dc)) return rc;
    // the call's tables: the regions of cr_layout (work_layouts.h)
    const CrLayout L = cr_layout(r);
    if (int rc = ensure_layout(ctx->cells_work, L.lay, who)) return rc;
    void* ws = ctx->cells_work.p;
    Fr *roots = at<Fr>(ws, L.roots), *pts = at<Fr>(ws, L.pts), *z = at<Fr>(ws, L.z);
    void* d_in = at<void>(ws, L.in_at);
    int32_t* slot = at<int32_t>(d_in, L.in.slot);
    uint32_t* lists = at<uint32_t>(d_in, L.in.lists);
    // slot map and id lists, built in the context's pinned array (the copy below may run after this call has returned)
    if (int rc = cells_pinned_ensure(ctx, L.in.lay.total())) return rc;
    int32_t* h_slot = at<int32_t>(ctx->cells_pinned, L.in.slot);
    uint32_t* h_lists = at<uint32_t>(ctx->cells_pinned, L.in.lists);
    for (size_t m = 0; m < r; m++) h_slot[m] = -1;
    for (size_t k = 0; k < K; k++) h_slot[cell_ids[k]] = (int32_t)k;
    size_t q = 0;
    for (size_t m = 0; m < r; m++)
        if (h_slot[m] < 0) h_lists[q++] = (uint32_t)m;
    for (size_t k = 0; k < K; k++) h_lists[nm + k] = cell_ids[k];
    BBG_HIP(hipMemcpyAsync(d_in, ctx->cells_pinned, L.in.lay.total(), hipMemcpyHostToDevice, st));
    BBG_HIP(hipEventRecord(ctx->cells_copied, st));
    {
        ProfScope ps(ctx, "cells_z", st);
        hipLaunchKernelGGL(k_cells_points, dim3(grid_for(2 * r, 256)), dim3(256), 0, st, (const DomainConsts*)dc, log2cell, (unsigned)r, (unsigned)nm,
                           (unsigned)K, (const uint32_t*)lists, (const uint32_t*)(lists + nm), roots, pts);
        hipLaunchKernelGGL(k_cells_z, dim3(grid_for(nout, CZ_BLOCK_OUT)), dim3(256), 0, st, (const Fr*)roots, (unsigned)nm, (const Fr*)pts, z, (unsigned)nout);
    }
    if (int rc = bary_batch_invert(ctx, z, z, r, st)) return rc; // Zcos -> 1 / Zcos in place; Zdom (z + r) stays
    Fr* out = (Fr*)d_out_coeffs;
    {
        ProfScope ps(ctx, "cells_scatter", st);
        hipLaunchKernelGGL(k_cells_transpose<true>, dim3(transpose_grid(log2r, log2cell), (unsigned)count), dim3(CT * CT), 0, st, (const Fr*)d_values, out,
                           log2r, log2cell, (unsigned)K, (const int32_t*)slot, (const Fr*)(z + r));
    }
    for (size_t p = 0; p < count; p++) {
        if (int rc = ntt_run(ctx, out + p * n, log2n, BBG_IFFT, 0, nullptr, st)) return rc;
        if (int rc = ntt_run(ctx, out + p * n, log2n, BBG_COSET_FFT, 0, nullptr, st)) return rc;
    }
    {
        ProfScope ps(ctx, "cells_divide", st);
        hipLaunchKernelGGL(k_cells_divide, dim3(sweep_grid(n), (unsigned)count), dim3(256), 0, st, out, n, (unsigned)(r - 1), (const Fr*)z);
    }
    for (size_t p = 0; p < count; p++)
        if (int rc = ntt_run(ctx, out + p * n, log2n, BBG_COSET_IFFT, 0, nullptr, st)) return rc;
    {
        ProfScope ps(ctx, "cells_canon", st);
        hipLaunchKernelGGL(k_cells_divide, dim3(sweep_grid(n), (unsigned)count), dim3(256), 0, st, out, n, 0u, (const Fr*)nullptr);
    }
    BBG_HIP(hipGetLastError());
    return BBG_OK;
}

} // namespace bbg
