// A batch of cell proofs reduced to the two points of one pairing check (bbg_cells_verify_reduce), and at the end of the file
// the verdict in one call (bbg_cells_verify): that reduction, [L, -R] packed, the wave pairing at count 1, one status word.
// Notation as in cells.hip: n = 2^log2n, l = 2^log2cell, r = n / l, w = w_n, phi = w^l; cell m < r is { w^(m + r t) : t < l } with the
// vanishing polynomial X^l - phi^m.  Cell k < K of the batch has a commitment index c_k < ncom, a cell index m_k < r, l values v_k[t], a
// proof pi_k; I_k is the interpolant of degree < l through its values, rho the caller's challenge, s_b the first l points of a string.
// pi_k is valid iff  x^l pi_k = C_(c_k) - [I_k(x)] + phi^(m_k) pi_k; weighted by rho^k and summed over k:
//     L = sum_k rho^k pi_k = sum_m S_m,                           S_m = sum_(k: m_k = m) rho^k pi_k
//     R = sum_c W_c C_c - sum_(b<l) A_b s_b + sum_m phi^m S_m,    W_c = sum_(k: c_k = c) rho^k,   A = coefficients of sum_k rho^k I_k
// and the caller checks e(L, [x^l]_2) = e(R, [1]_2).  A costs one transform: with E[m + r t] = sum_(k: m_k = m) rho^k v_k[t] (zero on the
// cells nobody sampled) and g = iNTT_n(E), g mod (X^l - phi^m) = sum_u phi^(m u) g_(b + l u) interpolates E on cell m, and summing over m
// leaves r g_b because sum_m phi^(m u) = r [u = 0]:   A_b = r g_b, b < l.  tests/tools/cells_verify_model.py proves it on integers.
//
// The ids are grouped on the host (a counting sort into CSR offsets by m and by c, staged through the context's pinned array as
// cells_recover stages its lists); a call then queues, on one stream and without a host synchronisation:
//   * k_fb_powers        pw[k] = rho^k (fixed_base.hip);
//   * k_cv_wsum          W_c, one wave per commitment;
//   * k_cv_fold          E, one thread per (m, t), written through the 16 x 16 LDS tile of k_cells_transpose;
//   * the Fr iNTT at n, k_cv_scale (A_b = r g_b, l values) and the MSM over s_0 .. s_(l-1);
//   * k_cv_mul           the K + ncom products rho^k pi_k (in group order) and W_c C_c by xyzz_mul_glv, the on-curve test in their loads;
//   * k_cv_segsum        S_m, one wave per group: a lane-stride walk, then six shuffle rounds of the complete addition;
//   * k_cv_phi           phi^m S_m by xyzz_mul_glv (an empty group is infinity and returns at once);
//   * k_cv_reduce        the sums over m (and c) into at most CV_PARTS partial sums each, k_cv_finish the rest and the one inversion.
#include "bbg_internal.h"
#include "work_layouts.h"

#include "curve.hip.h"
#include "ntt_consts.hip.h"
#include "var_base.hip.h"

namespace bbg {

constexpr int CV_T = 16;       // the fold's tile, as k_cells_transpose
constexpr int CV_PARTS = 256;  // partial sums per reduction: one wave on every CU
constexpr size_t CV_MAX = (size_t)1 << 30; // cells and commitments per call (the group lists are 32-bit)

// ---------------------------------------------------------------------------------------------- Fr side
// W[c] = sum of pw[k] over the cells of commitment c (coarse); an unused commitment gets zero.  One wave per commitment at a time, as
// k_cv_segsum below: lane t adds the entries t, t + 64, .. of group c, then six shuffle rounds (one blob with thousands of cells is one group).
__global__ void __launch_bounds__(64) k_cv_wsum(const Fr* __restrict__ pw, const uint32_t* __restrict__ off, const uint32_t* __restrict__ perm, Fr* __restrict__ W,
                                                size_t ncom)
{
    const unsigned lane = threadIdx.x;
#pragma unroll 1
    for (size_t c = blockIdx.x; c < ncom; c += gridDim.x) {
        const uint32_t e = off[c + 1];
        Fr acc = Fr::zero();
        for (size_t j = (size_t)off[c] + lane; j < e; j += 64) acc = fe_add(acc, fe_load<FrP>(pw + perm[j]));
#pragma unroll 1
        for (int d = 32; d >= 1; d >>= 1) {
            Fr o;
#pragma unroll
            for (int w = 0; w < 8; w++) o.v[w] = (uint32_t)__shfl_xor((int)acc.v[w], d, 64);
            acc = fe_add(acc, o);
        }
        if (lane == 0) fe_store<FrP>(W + c, acc);
    }
}

// E[m + r t] = sum_(k in group m) pw[k] v[k l + t], zero for an empty group.  The thread of (m, t) reads with t fastest (512 contiguous
// bytes per cell and tile row) and the tile is written back with m fastest.
__global__ void __launch_bounds__(CV_T * CV_T) k_cv_fold(const Fr* __restrict__ values, const Fr* __restrict__ pw, const uint32_t* __restrict__ off,
                                                        const uint32_t* __restrict__ perm, Fr* __restrict__ E, unsigned log2r, unsigned log2l)
{
    __shared__ Fr tile[CV_T][CV_T + 1];
    const size_t r = (size_t)1 << log2r, l = (size_t)1 << log2l;
    const size_t tiles_m = (r + CV_T - 1) / CV_T;
    const size_t m0 = (blockIdx.x % tiles_m) * CV_T, t0 = (blockIdx.x / tiles_m) * CV_T;
    const unsigned tx = threadIdx.x % CV_T, ty = threadIdx.x / CV_T;
    {
        const size_t m = m0 + ty, t = t0 + tx;
        if (m < r && t < l) {
            Fr acc = Fr::zero();
            for (uint32_t j = off[m]; j < off[m + 1]; j++) {
                const size_t k = perm[j];
                acc = fe_add(acc, fe_mul(fe_load<FrP>(pw + k), fe_load<FrP>(values + k * l + t)));
            }
            tile[ty][tx] = acc;
        }
    }
    __syncthreads();
    const size_t m = m0 + tx, t = t0 + ty;
    if (m < r && t < l) fe_store<FrP>(E + t * r + m, tile[tx][ty]);
}

// a[b] <- r a[b], b < l, canonical: the MSM's scalars
__global__ void __launch_bounds__(256) k_cv_scale(Fr* a, size_t l, unsigned log2r)
{
    const size_t b = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= l) return;
    Fr rr = Fr::one();
    for (unsigned i = 0; i < log2r; i++) rr = fe_dbl(rr);
    fe_store<FrP>(a + b, fe_reduce_once(fe_mul(fe_load<FrP>(a + b), rr)));
}

// ---------------------------------------------------------------------------------------------- G1 side
// Item i < K: prod[i] = pw[k] proofs[k], k = perm[i] (group order); item K + c: com_out[c] = W[c] commitments[c].  A finite point off the
// curve is counted in *bad and taken as infinity.  The shape of k_open_batch_pointwise: blocks of one wave, two waves per SIMD, lane tables.
__global__ void __launch_bounds__(64, 2) k_cv_mul(const Affine* __restrict__ proofs, const Fr* __restrict__ pw, const uint32_t* __restrict__ perm, size_t K,
                                                  const Affine* __restrict__ commitments, const Fr* __restrict__ W, size_t ncom, Xyzz* __restrict__ prod,
                                                  Xyzz* __restrict__ com_out, unsigned* bad, Xyzz* __restrict__ tables)
{
    const size_t lanes = (size_t)gridDim.x * blockDim.x;
    const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    Xyzz* table = tables + (size_t)blockIdx.x * 64 * GLV_TABLE; // the wave's 64 tables: wave-uniform
#pragma unroll 1
    for (size_t i = lane; i < K + ncom; i += lanes) {
        const bool is_proof = i < K;
        const size_t k = is_proof ? perm[i] : i - K;
        const Affine a = aff_load(is_proof ? proofs + k : commitments + k);
        const Fr s = fe_from_mont(fe_load<FrP>(is_proof ? pw + k : W + k));
        Xyzz p = xyzz_inf();
        if (!aff_is_inf(a)) {
            if (aff_on_curve(a)) p = xyzz_from_affine(a);
            else atomicAdd(bad, 1u);
        }
        xyzz_store(is_proof ? prod + i : com_out + k, xyzz_mul_glv(p, s, table));
    }
}

// S[m] = sum of prod[off[m] .. off[m + 1]), infinity for an empty group.  One wave per group at a time: lane t adds the entries t, t + 64,
// .. by the complete addition, then the 64 partial sums meet in six shuffle rounds (skipped for a group of at most one entry).
__global__ void __launch_bounds__(64) k_cv_segsum(const Xyzz* __restrict__ prod, const uint32_t* __restrict__ off, Xyzz* __restrict__ S, size_t r)
{
    const unsigned lane = threadIdx.x;
#pragma unroll 1
    for (size_t m = blockIdx.x; m < r; m += gridDim.x) {
        const uint32_t b = off[m], e = off[m + 1];
        Xyzz acc = xyzz_inf();
#pragma unroll 1
        for (size_t j = (size_t)b + lane; j < e; j += 64) acc = xyzz_add(acc, xyzz_load(prod + j));
        if (e - b > 1) acc = xyzz_wave_sum(acc);
        if (lane == 0) xyzz_store(S + m, acc);
    }
}

// Q[m] = phi^m S[m], m < r
__global__ void __launch_bounds__(64, 2) k_cv_phi(const DomainConsts* dc, unsigned log2cell, const Xyzz* __restrict__ S, Xyzz* __restrict__ Q, size_t r,
                                                  Xyzz* __restrict__ tables)
{
    const size_t lanes = (size_t)gridDim.x * blockDim.x;
    const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    Xyzz* table = tables + (size_t)blockIdx.x * 64 * GLV_TABLE;
    const Fr* phi_pow2 = dc->pow2_root + log2cell; // phi^(2^b) = w^(2^(b + log2cell)), m < r: b + log2cell < log2n <= 28
#pragma unroll 1
    for (size_t m = lane; m < r; m += lanes) {
        const Xyzz s = xyzz_load(S + m);
        const Fr e = fe_from_mont(pow_from_table(phi_pow2, m));
        xyzz_store(Q + m, xyzz_mul_glv(s, e, table));
    }
}

// parts[y CV_PARTS + block] = sum of the entries block 64 + lane, + 64 gridDim.x, .. of array y (y = 0: a0 with n0 entries, y = 1: a1, n1)
__global__ void __launch_bounds__(64) k_cv_reduce(const Xyzz* __restrict__ a0, size_t n0, const Xyzz* __restrict__ a1, size_t n1, Xyzz* __restrict__ parts)
{
    const Xyzz* a = blockIdx.y ? a1 : a0;
    const size_t n = blockIdx.y ? n1 : n0;
    Xyzz acc = xyzz_inf();
#pragma unroll 1
    for (size_t i = (size_t)blockIdx.x * 64 + threadIdx.x; i < n; i += (size_t)gridDim.x * 64) acc = xyzz_add(acc, xyzz_load(a + i));
    acc = xyzz_wave_sum(acc);
    if (threadIdx.x == 0) xyzz_store(parts + (size_t)blockIdx.y * CV_PARTS + blockIdx.x, acc);
}

// out[0] = L = the sum of the first `np` parts, out[1] = R = the sum of the next np - [A] ([A]: the MSM's Jacobian result); canonical
// affine behind one inversion.  One wave.  *off_curve (may be null) = *bad.
__global__ void __launch_bounds__(64) k_cv_finish(const Xyzz* __restrict__ parts, unsigned np, const Jacobian* __restrict__ msm_a, Affine* out, const unsigned* bad,
                                                  unsigned* off_curve)
{
    const unsigned lane = threadIdx.x;
    Xyzz L = xyzz_inf(), R = xyzz_inf();
#pragma unroll 1
    for (unsigned i = lane; i < np; i += 64) L = xyzz_add(L, xyzz_load(parts + i));
#pragma unroll 1
    for (unsigned i = lane; i < np; i += 64) R = xyzz_add(R, xyzz_load(parts + CV_PARTS + i));
    L = xyzz_wave_sum(L);
    R = xyzz_wave_sum(R);
    if (lane != 0) return;
    Jacobian j;
    j.x = fe_load<FqP>(&msm_a->x);
    j.y = fe_load<FqP>(&msm_a->y);
    j.z = fe_load<FqP>(&msm_a->z);
    R = xyzz_add(R, xyzz_neg(xyzz_from_jacobian(j)));
    aff_batch_chunk4(out, 2, [&](int e) __attribute__((always_inline)) { return e ? R : L; });
    if (off_curve) *off_curve = *bad;
}

// ---------------------------------------------------------------------------------------------- host side
int cells_verify_check(const char* who, const bbg_ctx* ctx, const bbg_srs* srs, unsigned log2n, unsigned log2cell, size_t ncom, const uint32_t* commitment_ids,
                       const uint32_t* cell_ids, size_t K, const uint64_t* rho)
{
    const std::string w(who);
    if (!srs || !commitment_ids || !cell_ids || !rho) { set_error(w + ": null argument"); return BBG_E_INVALID; }
    if (int rc = check_log2n(who, log2n, 1, 28)) return rc;
    if (log2cell > log2n - 1) { set_error(w + ": log2cell must be 0 .. log2n - 1"); return BBG_E_INVALID; }
    if (K < 1 || K > CV_MAX) { set_error(w + ": K must be 1 .. 2^30"); return BBG_E_INVALID; }
    if (ncom < 1 || ncom > CV_MAX) { set_error(w + ": ncom must be 1 .. 2^30"); return BBG_E_INVALID; }
    if (int rc = check_srs_holds(who, srs->s, log2cell, "log2cell")) return rc;
    if (int rc = check_srs_device(who, srs->s, ctx)) return rc;
    const size_t r = (size_t)1 << (log2n - log2cell);
    for (size_t k = 0; k < K; k++) {
        if (cell_ids[k] >= r) { set_error(w + ": a cell id is not below r = n / l"); return BBG_E_INVALID; }
        if (commitment_ids[k] >= ncom) { set_error(w + ": a commitment id is not below ncom"); return BBG_E_INVALID; }
    }
    return BBG_OK;
}

// off[0 .. groups], perm[0 .. K): perm lists the k < K by ids[k], each group in ascending k
static void cv_group(const uint32_t* ids, size_t K, size_t groups, uint32_t* off, uint32_t* perm)
{
    for (size_t g = 0; g <= groups; g++) off[g] = 0;
    for (size_t k = 0; k < K; k++) off[ids[k] + 1]++;
    for (size_t g = 0; g < groups; g++) off[g + 1] += off[g];
    for (size_t k = 0; k < K; k++) perm[off[ids[k]]++] = (uint32_t)k; // off[g] is now the END of group g ..
    for (size_t g = groups; g > 0; g--) off[g] = off[g - 1];          // .. which is the start of group g + 1
    off[0] = 0;
}

int cells_verify_reduce(bbg_ctx* ctx, bbg_srs* srs, unsigned log2n, unsigned log2cell, const void* d_commitments, size_t ncom, const uint32_t* commitment_ids,
                        const uint32_t* cell_ids, size_t K, const void* d_values, const void* d_proofs, const uint64_t* rho, void* d_out, void* d_off_curve,
                        hipStream_t st)
{
    const char* who = "bbg_cells_verify_reduce_device";
    if (!d_commitments || !d_values || !d_proofs || !d_out) { set_error(std::string(who) + ": null argument"); return BBG_E_INVALID; }
    if (int rc = cells_verify_check(who, ctx, srs, log2n, log2cell, ncom, commitment_ids, cell_ids, K, rho)) return rc;
    const unsigned log2r = log2n - log2cell;
    const size_t n = (size_t)1 << log2n, l = (size_t)1 << log2cell, r = (size_t)1 << log2r;
    const struct { const void* p; size_t bytes; } ins[3] = { { d_commitments, ncom * 64 }, { d_values, K * l * 32 }, { d_proofs, K * 64 } };
    for (const auto& in : ins)
        if (ranges_overlap(d_out, 128, in.p, in.bytes) || (d_off_curve && ranges_overlap(d_off_curve, 4, in.p, in.bytes))) {
            set_error(std::string(who) + ": an output overlaps an input");
            return BBG_E_INVALID;
        }
    if (d_off_curve && ranges_overlap(d_off_curve, 4, d_out, 128)) { set_error(std::string(who) + ": the two outputs overlap"); return BBG_E_INVALID; }
    void* dc = nullptr;
    if (int rc = ntt_domain_consts(ctx, log2n, &dc)) return rc;
    // working memory, all of it sized before the first launch: the lanes' tables, then the regions of cv_layout (work_layouts.h)
    size_t lanes = 0;
    void* tables = nullptr;
    if (int rc = var_base_tables(ctx, std::max(K + ncom, r), &lanes, &tables)) return rc;
    const CvLayout L = cv_layout(n, r, K, ncom, CV_PARTS);
    if (int rc = ensure_layout(ctx->cells_work, L.lay, who)) return rc;
    void* ws = ctx->cells_work.p;
    Xyzz *S = at<Xyzz>(ws, L.S), *Q = at<Xyzz>(ws, L.Q), *prod = at<Xyzz>(ws, L.prod), *parts = at<Xyzz>(ws, L.parts);
    Jacobian* msm_a = at<Jacobian>(ws, L.msm_a);
    Fr *E = at<Fr>(ws, L.E), *pw = at<Fr>(ws, L.pw), *W = at<Fr>(ws, L.W);
    unsigned* bad = at<unsigned>(ws, L.bad);
    // the group lists: built in the pinned array, one copy, read from the same places of the device block
    if (int rc = cells_pinned_ensure(ctx, L.in.lay.total())) return rc;
    void* h_lists = ctx->cells_pinned;
    cv_group(cell_ids, K, r, at<uint32_t>(h_lists, L.in.off_m), at<uint32_t>(h_lists, L.in.perm_m));
    cv_group(commitment_ids, K, ncom, at<uint32_t>(h_lists, L.in.off_c), at<uint32_t>(h_lists, L.in.perm_c));
    void* lists = at<void>(ws, L.lists);
    BBG_HIP(hipMemcpyAsync(lists, h_lists, L.in.lay.total(), hipMemcpyHostToDevice, st));
    BBG_HIP(hipEventRecord(ctx->cells_copied, st));
    BBG_HIP(hipMemsetAsync(bad, 0, 4, st));
    const uint32_t *off_m = at<uint32_t>(lists, L.in.off_m), *perm_m = at<uint32_t>(lists, L.in.perm_m), *off_c = at<uint32_t>(lists, L.in.off_c),
                   *perm_c = at<uint32_t>(lists, L.in.perm_c);
    {
        ProfScope ps(ctx, "cells_verify_powers", st);
        if (int rc = fixed_base_powers(rho, K, pw, st)) return rc;
        hipLaunchKernelGGL(k_cv_wsum, dim3((unsigned)std::min<size_t>(ncom, 8192)), dim3(64), 0, st, (const Fr*)pw, off_c, perm_c, W, ncom);
    }
    {
        ProfScope ps(ctx, "cells_verify_fold", st);
        const unsigned tiles = (unsigned)(((r + CV_T - 1) / CV_T) * ((l + CV_T - 1) / CV_T)); // at most 2^28 / 16 blocks (l = 1)
        hipLaunchKernelGGL(k_cv_fold, dim3(tiles), dim3(CV_T * CV_T), 0, st, (const Fr*)d_values, (const Fr*)pw, off_m, perm_m, E, log2r, log2cell);
    }
    if (int rc = ntt_run(ctx, E, log2n, BBG_IFFT, 0, nullptr, st)) return rc;
    {
        ProfScope ps(ctx, "cells_verify_fold", st);
        hipLaunchKernelGGL(k_cv_scale, dim3(grid_for(l, 256)), dim3(256), 0, st, E, l, log2r);
    }
    if (int rc = msm_run(ctx, srs->s, E, 0, l, msm_a, st)) return rc;
    if (int rc = msm_join(ctx, st)) return rc;
    {
        ProfScope ps(ctx, "cells_verify_mul", st);
        hipLaunchKernelGGL(k_cv_mul, dim3((unsigned)(lanes / 64)), dim3(64), 0, st, (const Affine*)d_proofs, (const Fr*)pw, perm_m, K, (const Affine*)d_commitments,
                           (const Fr*)W, ncom, prod, at<Xyzz>(ws, L.com_out), bad, (Xyzz*)tables);
    }
    {
        ProfScope ps(ctx, "cells_verify_segsum", st);
        hipLaunchKernelGGL(k_cv_segsum, dim3((unsigned)std::min<size_t>(r, 8192)), dim3(64), 0, st, (const Xyzz*)prod, off_m, S, r);
    }
    {
        ProfScope ps(ctx, "cells_verify_phi", st);
        hipLaunchKernelGGL(k_cv_phi, dim3((unsigned)(std::min(lanes, (r + 63) / 64 * 64) / 64)), dim3(64), 0, st, (const DomainConsts*)dc, log2cell, (const Xyzz*)S, Q,
                           r, (Xyzz*)tables);
    }
    {
        ProfScope ps(ctx, "cells_verify_finish", st);
        const unsigned np = (unsigned)std::min<size_t>((r + ncom + 63) / 64, CV_PARTS);
        hipLaunchKernelGGL(k_cv_reduce, dim3(np, 2), dim3(64), 0, st, (const Xyzz*)S, r, (const Xyzz*)Q, r + ncom, parts);
        hipLaunchKernelGGL(k_cv_finish, dim3(1), dim3(64), 0, st, (const Xyzz*)parts, np, (const Jacobian*)msm_a, (Affine*)d_out, (const unsigned*)bad,
                           (unsigned*)d_off_curve);
    }
    BBG_HIP(hipGetLastError());
    return BBG_OK;
}

// ---------------------------------------------------------------------------------------------- the verdict in one call (bbg_cells_verify)
// pair[0] = L, pair[1] = -R of lr = (L, R), canonical in and out: y -> p - y; infinity stays as it is, and so does y = 0.  One thread.
__global__ void __launch_bounds__(64) k_cv_pack(const Affine* __restrict__ lr, Affine* __restrict__ pair)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    Affine r = aff_load(lr + 1);
    if (!aff_is_inf(r)) r.y = fe_reduce_once(fe_reduce_once(fe_neg(r.y))); // 2p - y: p - y behind one subtraction, 0 behind two
    aff_store(pair, aff_load(lr));
    aff_store(pair + 1, r);
}
// the status word: 2 where the reduction counted a point off the curve, whatever the pairing says; else the pairing's
__global__ void __launch_bounds__(64) k_cv_verdict(const unsigned* __restrict__ off_curve, const uint32_t* __restrict__ paired, uint32_t* __restrict__ status)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *status = *off_curve ? 2u : *paired;
}

// the layout of ctx->cells_verdict
constexpr size_t CVV_LR = 0, CVV_PAIR = 128, CVV_OFF = 256, CVV_PAIRED = 260, CVV_BYTES = 512;

// The verdict's steps, shared with kzg_verify.hip: the handle's checks (`first`: what its first point is called), the buffer with the places
// of (L, R) and of the off-curve count, and the tail behind a reduction that wrote both there.
int cells_verdict_check(const char* who, const bbg_ctx* ctx, const bbg_g2_lines* lines, const char* first)
{
    const std::string w(who);
    if (lines->pairs != 2) { set_error(w + ": the lines handle must hold exactly two points, " + first + " and [1]_2"); return BBG_E_INVALID; }
    if (lines->device != ctx->device) { set_error(w + ": the handle was made on another device"); return BBG_E_INVALID; }
    return BBG_OK;
}
int cells_verdict_buffer(bbg_ctx* ctx, void** d_lr, void** d_off_curve)
{
    if (int rc = ctx->cells_verdict.ensure(CVV_BYTES)) return rc;
    *d_lr = (char*)ctx->cells_verdict.p + CVV_LR;
    *d_off_curve = (char*)ctx->cells_verdict.p + CVV_OFF;
    return BBG_OK;
}
int cells_verdict_run(bbg_ctx* ctx, const bbg_g2_lines* lines, void* d_status, hipStream_t st)
{
    char* v = (char*)ctx->cells_verdict.p;
    {
        ProfScope ps(ctx, "cells_verify_pack", st);
        hipLaunchKernelGGL(k_cv_pack, dim3(1), dim3(64), 0, st, (const Affine*)(v + CVV_LR), (Affine*)(v + CVV_PAIR));
    }
    if (int rc = pairing_wave_run(ctx, lines, v + CVV_PAIR, 1, nullptr, v + CVV_PAIRED, st)) return rc;
    {
        ProfScope ps(ctx, "cells_verify_pack", st);
        hipLaunchKernelGGL(k_cv_verdict, dim3(1), dim3(64), 0, st, (const unsigned*)(v + CVV_OFF), (const uint32_t*)(v + CVV_PAIRED), (uint32_t*)d_status);
    }
    BBG_HIP(hipGetLastError());
    return BBG_OK;
}

int cells_verify_run(bbg_ctx* ctx, bbg_srs* srs, const bbg_g2_lines* lines, unsigned log2n, unsigned log2cell, const void* d_commitments, size_t ncom,
                     const uint32_t* commitment_ids, const uint32_t* cell_ids, size_t K, const void* d_values, const void* d_proofs, const uint64_t* rho,
                     void* d_status, hipStream_t st)
{
    const std::string who("bbg_cells_verify_device");
    if (!lines || !d_status || !d_commitments || !d_values || !d_proofs) { set_error(who + ": null argument"); return BBG_E_INVALID; }
    if (int rc = cells_verdict_check(who.c_str(), ctx, lines, "[x^l]_2")) return rc;
    if (int rc = cells_verify_check(who.c_str(), ctx, srs, log2n, log2cell, ncom, commitment_ids, cell_ids, K, rho)) return rc;
    const struct { const void* p; size_t bytes; } ins[3] = { { d_commitments, ncom * 64 }, { d_values, (K * 32) << log2cell }, { d_proofs, K * 64 } };
    for (const auto& in : ins)
        if (ranges_overlap(d_status, 4, in.p, in.bytes)) { set_error(who + ": the status word overlaps an input"); return BBG_E_INVALID; }
    void *lr = nullptr, *off = nullptr;
    if (int rc = cells_verdict_buffer(ctx, &lr, &off)) return rc;
    if (int rc = cells_verify_reduce(ctx, srs, log2n, log2cell, d_commitments, ncom, commitment_ids, cell_ids, K, d_values, d_proofs, rho, lr, off, st)) return rc;
    return cells_verdict_run(ctx, lines, d_status, st);
}

} // namespace bbg
