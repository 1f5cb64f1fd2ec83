// Variable-base batch scalar multiplication over BN254 G1 for gfx950: out[i] = s_i * P_i for n different points
// (bbg_g1_batch_mul; with one scalar for all points it is the reference's element::batch_mul_with_endomorphism,
// ecc/groups/element_impl.hpp:666-832), and on top of it the update step of a powers-of-x string, P_i <- [y^i] P_i (bbg_srs_scale_powers).
//
//   * k_vb_mul<GLV>   one lane per VB_CH consecutive points, and a FIXED number of lanes: lane t takes the chunks t, t + lanes, t + 2 lanes, ..
//                     so that the working memory -- the lanes' tables of odd multiples, 1 KiB each (var_base.hip.h) -- is bounded by the
//                     lane count (option "batch_mul_lanes", default 2^17 = two waves on every SIMD: 128 MiB), whatever n is.  Per point:
//                     the scalar out of Montgomery form, then xyzz_mul_glv (GLV = true: 128 doublings + 74 additions) or the bit-serial
//                     xyzz_mul_fr (GLV = false: 256 + ~127; option "batch_mul_glv" = 0, A/B -- it needs no table).  The VB_CH results become
//                     canonical affine behind one inversion by the batched conversion of curve.hip.h (aff_batch_*).  An infinite result
//                     is written as aff_inf().
// A lane reads point i before it writes slot i and touches no other lane's slots, so d_out may BE d_points (in place).
#include "bbg_internal.h"
#include "var_base.hip.h"

namespace bbg {

constexpr int VB_CH = 4; // points per lane behind one inversion

template <bool GLV> __device__ __forceinline__ Xyzz vb_mul_one(const Affine& p, const Fr& k, Xyzz* table)
{
    if (aff_is_inf(p)) return xyzz_inf();
    if (GLV) return xyzz_mul_glv(xyzz_from_affine(p), k, table);
    return xyzz_mul_fr(xyzz_from_affine(p), k);
}

// Two waves per SIMD.  The VB_CH results of a chunk become canonical affine behind one inversion (aff_batch_chunk4, curve.hip.h), which
// asks for point e before it writes slot e: points and out carry no __restrict__, they may be the same buffer.
// Scalars arrive in Montgomery form as any representative in [0, 2r): fe_from_mont returns the canonical plain value (fixed_base.hip).
static_assert(VB_CH == 4, "k_vb_mul converts its chunk with aff_batch_chunk4");
template <bool GLV>
__global__ void __launch_bounds__(64, 2) k_vb_mul(const Affine* points, const Fr* __restrict__ scalars, size_t n, int one_scalar, Affine* out, Xyzz* tables)
{
    const size_t lanes = (size_t)gridDim.x * blockDim.x;
    const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    Xyzz* table = GLV ? tables + (size_t)blockIdx.x * 64 * GLV_TABLE : nullptr; // the wave's 64 tables (blocks of one wave): wave-uniform
    const size_t chunks = (n + VB_CH - 1) / VB_CH;
#pragma unroll 1
    for (size_t c = lane; c < chunks; c += lanes) {
        const size_t i0 = c * VB_CH;
        const int cnt = n - i0 < (size_t)VB_CH ? (int)(n - i0) : VB_CH;
        const Fr* s0 = scalars + (one_scalar ? 0 : i0);
        const size_t ss = one_scalar ? 0 : 1;
        aff_batch_chunk4(out + i0, cnt, [&](int e) __attribute__((always_inline)) { return vb_mul_one<GLV>(aff_load(points + i0 + e), fe_from_mont(fe_load<FrP>(s0 + e * ss)), table); });
    }
}

// ---------------------------------------------------------------------------------------------- host side
// The lanes a kernel with `work` independent items runs on (a multiple of 64, at most the option "batch_mul_lanes") and their tables:
// *tables = lanes x GLV_TABLE_BYTES of the context's buffer, grown on demand, counted under `scratch`, released by bbg_memory_trim.
int var_base_tables(bbg_ctx* ctx, size_t work, size_t* lanes, void** tables)
{
    size_t l = (work + 63) / 64 * 64;
    if (l > (size_t)ctx->batch_mul_lanes) l = (size_t)ctx->batch_mul_lanes;
    if (l == 0) l = 64;
    int rc = ctx->vb_tables.ensure(l * GLV_TABLE_BYTES);
    if (rc) return rc;
    *lanes = l;
    *tables = ctx->vb_tables.p;
    return BBG_OK;
}

// d_out[i] = d_scalars[one_scalar ? 0 : i] * d_points[i] on `st`, canonical affine, aff_inf() for an infinite result.  d_out may be
// d_points; any other overlap of the two, and any overlap of d_out with the scalars, is refused.  Queues only.
int var_base_mul(bbg_ctx* ctx, const void* d_points, const void* d_scalars, size_t n, int one_scalar, void* d_out, hipStream_t st)
{
    if (n == 0) return BBG_OK;
    const char *pb = (const char*)d_points, *ob = (const char*)d_out;
    if (pb != ob && pb < ob + n * 64 && ob < pb + n * 64) {
        set_error("bbg_g1_batch_mul: the output overlaps the points without being the same buffer");
        return BBG_E_INVALID;
    }
    const char* sb = (const char*)d_scalars;
    if (sb < ob + n * 64 && ob < sb + (one_scalar ? 1 : n) * 32) { // the kernel reads scalar i after it has written slots of earlier points
        set_error("bbg_g1_batch_mul: the output overlaps the scalars");
        return BBG_E_INVALID;
    }
    const size_t chunks = (n + VB_CH - 1) / VB_CH;
    const bool glv = ctx->batch_mul_glv != 0;
    size_t lanes = (chunks + 63) / 64 * 64;
    void* tables = nullptr;
    if (glv) {
        int rc = var_base_tables(ctx, chunks, &lanes, &tables);
        if (rc) return rc;
    } else if (lanes > (size_t)ctx->batch_mul_lanes) {
        lanes = (size_t)ctx->batch_mul_lanes;
    }
    {
        ProfScope ps(ctx, "var_base_mul", st);
        if (glv)
            hipLaunchKernelGGL(k_vb_mul<true>, dim3((unsigned)(lanes / 64)), dim3(64), 0, st, (const Affine*)d_points, (const Fr*)d_scalars, n, one_scalar,
                               (Affine*)d_out, (Xyzz*)tables);
        else
            hipLaunchKernelGGL(k_vb_mul<false>, dim3((unsigned)(lanes / 64)), dim3(64), 0, st, (const Affine*)d_points, (const Fr*)d_scalars, n, one_scalar,
                               (Affine*)d_out, (Xyzz*)nullptr);
    }
    BBG_HIP(hipGetLastError());
    return BBG_OK;
}

} // namespace bbg
