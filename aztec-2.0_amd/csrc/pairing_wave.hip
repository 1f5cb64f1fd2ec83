// The wave-cooperative BN254 pairing product check for gfx950 (bbg_pairing_product_wave): the contract of pairing.hip's lane
// kernels -- the same lines handle, layouts, status words and canonical outputs -- with ONE product spread over the lanes of a wave instead
// of one product per lane.  It is the latency form: a verifier that reduced a batch of cell proofs to one two-pair check
// (bbg_cells_verify_reduce) has a single product, and the lane kernels walk its ~18 000 dependent Fq products on one lane of one wave.
//
//   k_pair_wave   block = one wave = one product, grid = count, ONE launch: the Miller loop over the 87-entry line walk
//                 (PairP::LINE_OPENS_STEP), then the final exponentiation by the same 294-step PAIR_FINAL_PROGRAM as k_pair_final.  The six
//                 Fq12 slots, the staging of a product, the scaled line and the G1 points live in LDS (W12Lds, 5.2 KiB): no global working
//                 memory.  Fq12 arithmetic: fq12_wave.hip.h -- a product or squaring is 3 dependent fe_mul, a sparse product 4 (the line is
//                 scaled by P.y and P.x on four lanes first), a Frobenius map 3, the one inversion runs on lane 0 through f12_inv.
//                 OP_CSQR runs as the product of x with itself: on the cyclotomic subgroup that is the same element, hence the same
//                 canonical output.
//                 The live-pair mask and the off-curve flag are ballots (lane j tests point j), so every branch around a barrier is
//                 wave-uniform.
#include "bbg_internal.h"
#include "curve.hip.h"
#include "fq12_wave.hip.h"

namespace bbg {

constexpr size_t PAIRW_LINES_BYTES = (size_t)PairP::LINES * 192;

__global__ void __launch_bounds__(W12_LANES) k_pair_wave(const char* __restrict__ lines, int pairs, const Affine* __restrict__ g1, char* __restrict__ out,
                                                         uint32_t* __restrict__ status)
{
    __shared__ W12Lds s;
    const unsigned lane = threadIdx.x;
    const size_t i = blockIdx.x;
    // lane j < pairs: point j into LDS, its bit of the live mask, its vote on the off-curve flag
    bool finite = false, off = false;
    if (lane < (unsigned)pairs) {
        const Affine a = aff_load(g1 + i * (size_t)pairs + lane);
        finite = !aff_is_inf(a);
        off = finite && !aff_on_curve(a);
        s.pt[lane][0] = a.x;
        s.pt[lane][1] = a.y;
    }
    const uint32_t live = (uint32_t)__ballot(finite);
    const bool bad = __any(off) != 0;
    w12_set_one(s, lane, 0); // and the points are visible
#pragma unroll 1
    for (int it = 0; it < PairP::LINES; it++) {
        const uint32_t opens = it < 32 ? PairP::LINE_OPENS_STEP[0] >> it : it < 64 ? PairP::LINE_OPENS_STEP[1] >> (it - 32) : PairP::LINE_OPENS_STEP[2] >> (it - 64);
        if (opens & 1) w12_mul<false>(s, lane, 0, 0, s.slot[0]);
#pragma unroll 1
        for (int j = 0; j < pairs; j++) {
            if (!((live >> j) & 1)) continue;
            if (lane < 6) { // o | vw P.y | vv P.x: one Fq per lane
                Fq c = fe_load<FqP>(lines + (size_t)j * PAIRW_LINES_BYTES + (size_t)it * 192 + lane * 32);
                if (lane >= 2) c = fe_mul(c, s.pt[j][lane < 4 ? 1 : 0]);
                s.line[lane] = c;
            }
            __syncthreads();
            w12_mul<true>(s, lane, 0, 0, s.line);
        }
    }
#pragma unroll 1
    for (int pc = 0; pc < PairP::FINAL_STEPS; pc++) {
        const uint32_t word = PAIR_FINAL_PROGRAM[pc];
        const uint32_t op = word & 255u, d = (word >> 8) & 255u, a = (word >> 16) & 255u, b = word >> 24;
        if (op == PairP::OP_END) break;
        switch (op) {
        case PairP::OP_MUL:
        case PairP::OP_CSQR: w12_mul<false>(s, lane, d, a, s.slot[op == PairP::OP_CSQR ? a : b]); break;
        case PairP::OP_CONJ: w12_conj(s, lane, d, a); break;
        case PairP::OP_INV: w12_inv(s, lane, d, a); break;
        default: w12_frobenius(s, lane, d, a, (int)op - (int)PairP::OP_FROB1 + 1); break;
        }
    }
    const bool one = w12_store_is_one(s, lane, 0, out ? out + i * 384 : nullptr);
    if (status && lane == 0) status[i] = bad ? 2u : one ? 1u : 0u;
}

int pairing_wave_run(bbg_ctx* ctx, const bbg_g2_lines* h, const void* d_g1, size_t count, void* d_out, void* d_status, hipStream_t st)
{
    const char* who = "bbg_pairing_product_wave_device";
    if (int rc = pairing_product_check(who, ctx, h, d_g1, count, d_out, d_status)) return rc;
    const size_t in_bytes = count * h->pairs * 64;
    if ((d_out && ranges_overlap(d_out, count * 384, d_g1, in_bytes)) || (d_status && ranges_overlap(d_status, count * 4, d_g1, in_bytes)) ||
        (d_out && d_status && ranges_overlap(d_out, count * 384, d_status, count * 4))) {
        set_error(std::string(who) + ": an output overlaps the input or the other output");
        return BBG_E_INVALID;
    }
    int wave = 0;
    BBG_HIP(hipDeviceGetAttribute(&wave, hipDeviceAttributeWarpSize, ctx->device));
    if (wave != W12_LANES) { set_error(std::string(who) + ": the device's waves do not have 64 lanes"); return BBG_E_INVALID; }
    {
        ProfScope ps(ctx, "pairing_wave", st);
        hipLaunchKernelGGL(k_pair_wave, dim3((unsigned)count), dim3(W12_LANES), 0, st, (const char*)h->d_lines, (int)h->pairs, (const Affine*)d_g1, (char*)d_out,
                           (uint32_t*)d_status);
    }
    BBG_HIP(hipGetLastError());
    return BBG_OK;
}

} // namespace bbg
