// A batch of single-point openings (C_i, z_i, y_i, pi_i), i < N, at ARBITRARY points reduced to the two points of one pairing check
// (bbg_kzg_verify_reduce), and the verdict in one call (bbg_kzg_verify).  pi_i is valid iff x pi_i = C_i - [y_i] G + z_i pi_i;
// weighted by rho^i and summed:
//     L = sum_i rho^i pi_i
//     R = sum_i rho^i ( C_i - [y_i] G + [z_i] pi_i ) = sum_i rho^i C_i + sum_i (rho^i z_i) pi_i + [s] G,   s = - sum_i rho^i y_i
// and every opening is valid iff (with overwhelming probability over rho) e(L, [x]_2) = e(R, [1]_2).  No string is involved: G = (1, 2).
// A call queues, on one stream and without a host round trip:
//   * k_fb_powers      pw[i] = rho^i (fixed_base.hip);
//   * k_kv_prepare     the packed points [C | pi | G] (canonical, the on-curve test in their loads: a finite point off the curve is counted
//                      and taken as infinity, as k_cv_mul does) and scalars [rho^i | rho^i z_i | s], the block sums of rho^i y_i;
//     k_kv_tail        one block: s = - (the sum of the block sums), G, the off-curve count;
//   * msm_points_run   over all 2N + 1 packed terms: R;
//   * msm_points_run   over the pi with the rho^i (a window into the same arrays): L.
// The verdict form runs cells_verify.hip's tail (cells_verdict_run: [L, -R] packed, the wave pairing at count 1, the status word).
#include "bbg_internal.h"
#include "work_layouts.h"

#include "block_invert.hip.h"
#include "curve.hip.h"

namespace bbg {

constexpr size_t KV_MAX = (size_t)1 << 27;   // 2N + 1 stays inside msm_points_run's 2^28
constexpr unsigned KV_BLOCKS = 4096;         // blocks (= partial sums) of k_kv_prepare at most

// a commitment or a proof as the MSM takes it: canonical; infinity stays infinity; a finite point off the curve is counted and becomes infinity
__device__ __forceinline__ Affine kv_load_point(const Affine* p, unsigned* bad)
{
    Affine a = aff_load(p);
    if (aff_is_inf(a)) return aff_inf();
    if (!aff_on_curve(a)) {
        atomicAdd(bad, 1u);
        return aff_inf();
    }
    a.x = fe_reduce_once(a.x);
    a.y = fe_reduce_once(a.y);
    return a;
}

__global__ void __launch_bounds__(256) k_kv_prepare(const Affine* __restrict__ commitments, const Fr* __restrict__ z, const Fr* __restrict__ y,
                                                    const Affine* __restrict__ proofs, size_t N, const Fr* __restrict__ pw, Affine* __restrict__ points,
                                                    Fr* __restrict__ scalars, Fr* __restrict__ partials, unsigned* bad)
{
    __shared__ Fr sm[4];
    const int tid = threadIdx.x;
    Fr acc = Fr::zero();
    for (size_t i = (size_t)blockIdx.x * 256 + tid; i < N; i += (size_t)gridDim.x * 256) {
        aff_store(points + i, kv_load_point(commitments + i, bad));
        aff_store(points + N + i, kv_load_point(proofs + i, bad));
        const Fr p = fe_load<FrP>(pw + i);
        fe_store<FrP>(scalars + i, p);
        fe_store<FrP>(scalars + N + i, fe_mul(p, fe_load<FrP>(z + i)));
        acc = fe_add(acc, fe_mul(p, fe_load<FrP>(y + i)));
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) sm[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) fe_store<FrP>(partials + blockIdx.x, fe_add(fe_add(sm[0], sm[1]), fe_add(sm[2], sm[3])));
}

// points[2N] = G, scalars[2N] = - sum of the `np` partial sums; *off_curve (may be null) = *bad.  One block.
__global__ void __launch_bounds__(256) k_kv_tail(const Fr* __restrict__ partials, unsigned np, Affine* g_slot, Fr* s_slot, const unsigned* bad, unsigned* off_curve)
{
    __shared__ Fr sm[4];
    const int tid = threadIdx.x;
    Fr acc = Fr::zero();
    for (unsigned i = tid; i < np; i += 256) acc = fe_add(acc, fe_load<FrP>(partials + i));
    acc = wave_sum(acc);
    if ((tid & 63) == 0) sm[tid >> 6] = acc;
    __syncthreads();
    if (tid != 0) return;
    acc = fe_add(fe_add(sm[0], sm[1]), fe_add(sm[2], sm[3]));
    fe_store<FrP>(s_slot, fe_reduce_once(fe_reduce_once(fe_neg(acc)))); // 2r - acc: canonical behind one subtraction, 0 behind two
    aff_store(g_slot, aff_generator());
    if (off_curve) *off_curve = *bad;
}

// ---------------------------------------------------------------------------------------------- host side
// the argument checks shared by the four entry points (`out`: out_bytes at the caller's output, device or host)
int kzg_verify_check(const char* who, const void* commitments, const void* z, const void* y, const void* proofs, size_t N, const uint64_t* rho, const void* out)
{
    const std::string w(who);
    if (!commitments || !z || !y || !proofs || !rho || !out) { set_error(w + ": null argument"); return BBG_E_INVALID; }
    if (N < 1 || N > KV_MAX) { set_error(w + ": N must be 1 .. 2^27"); return BBG_E_INVALID; }
    return BBG_OK;
}
static bool kv_overlaps_input(const void* out, size_t bytes, const void* com, const void* z, const void* y, const void* proofs, size_t N)
{
    return ranges_overlap(out, bytes, com, N * 64) || ranges_overlap(out, bytes, z, N * 32) || ranges_overlap(out, bytes, y, N * 32) ||
           ranges_overlap(out, bytes, proofs, N * 64);
}

int kzg_verify_reduce(bbg_ctx* ctx, const void* d_commitments, const void* d_z, const void* d_y, const void* d_proofs, size_t N, const uint64_t* rho,
                      void* d_out, void* d_off_curve, hipStream_t st)
{
    const char* who = "bbg_kzg_verify_reduce_device";
    if (int rc = kzg_verify_check(who, d_commitments, d_z, d_y, d_proofs, N, rho, d_out)) return rc;
    if (kv_overlaps_input(d_out, 128, d_commitments, d_z, d_y, d_proofs, N) ||
        (d_off_curve && kv_overlaps_input(d_off_curve, 4, d_commitments, d_z, d_y, d_proofs, N))) {
        set_error(std::string(who) + ": an output overlaps an input");
        return BBG_E_INVALID;
    }
    if (d_off_curve && ranges_overlap(d_off_curve, 4, d_out, 128)) { set_error(std::string(who) + ": the two outputs overlap"); return BBG_E_INVALID; }
    // working memory, sized before the first launch: the regions of kv_layout (work_layouts.h)
    const size_t terms = 2 * N + 1;
    const KvLayout L = kv_layout(N, KV_BLOCKS);
    if (int rc = ensure_layout(ctx->kzg_work, L.lay, who)) return rc;
    void* ws = ctx->kzg_work.p;
    Affine* points = at<Affine>(ws, L.points);
    Fr *scalars = at<Fr>(ws, L.scalars), *pw = at<Fr>(ws, L.pw), *partials = at<Fr>(ws, L.partials);
    unsigned* bad = at<unsigned>(ws, L.bad);
    const unsigned blocks = (unsigned)std::min<size_t>((N + 255) / 256, KV_BLOCKS);
    {
        ProfScope ps(ctx, "kzg_verify_prepare", st);
        BBG_HIP(hipMemsetAsync(bad, 0, 4, st));
        if (int rc = fixed_base_powers(rho, N, pw, st)) return rc;
        hipLaunchKernelGGL(k_kv_prepare, dim3(blocks), dim3(256), 0, st, (const Affine*)d_commitments, (const Fr*)d_z, (const Fr*)d_y, (const Affine*)d_proofs, N,
                           (const Fr*)pw, points, scalars, partials, bad);
        hipLaunchKernelGGL(k_kv_tail, dim3(1), dim3(256), 0, st, (const Fr*)partials, blocks, points + 2 * N, scalars + 2 * N, (const unsigned*)bad,
                           (unsigned*)d_off_curve);
    }
    BBG_HIP(hipGetLastError());
    if (int rc = msm_points_run(ctx, points, scalars, terms, 0, (char*)d_out + 64, st)) return rc; // R
    return msm_points_run(ctx, points + N, scalars, N, 0, d_out, st);                                // L
}

int kzg_verify_run(bbg_ctx* ctx, const bbg_g2_lines* lines, const void* d_commitments, const void* d_z, const void* d_y, const void* d_proofs, size_t N,
                   const uint64_t* rho, void* d_status, hipStream_t st)
{
    const char* who = "bbg_kzg_verify_device";
    if (!lines) { set_error(std::string(who) + ": null argument"); return BBG_E_INVALID; }
    if (int rc = kzg_verify_check(who, d_commitments, d_z, d_y, d_proofs, N, rho, d_status)) return rc;
    if (int rc = cells_verdict_check(who, ctx, lines, "[x]_2")) return rc;
    if (kv_overlaps_input(d_status, 4, d_commitments, d_z, d_y, d_proofs, N)) { set_error(std::string(who) + ": the status word overlaps an input"); return BBG_E_INVALID; }
    void *lr = nullptr, *off = nullptr;
    if (int rc = cells_verdict_buffer(ctx, &lr, &off)) return rc;
    if (int rc = kzg_verify_reduce(ctx, d_commitments, d_z, d_y, d_proofs, N, rho, lr, off, st)) return rc;
    return cells_verdict_run(ctx, lines, d_status, st);
}

} // namespace bbg
