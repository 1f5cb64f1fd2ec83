// Internal declarations shared by the HIP translation units of libbbg.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/bbg.h"
#include "region_layout.h"

namespace bbg {

void set_error(const std::string& msg);
int hip_fail(hipError_t e, const char* what, const char* file, int line);
struct Srs;
// Argument checks shared by the entry points (bbg_capi.hip): BBG_OK, or BBG_E_INVALID with the error text set to "<who>: " and the sentence
int check_log2n(const char* who, unsigned log2n, unsigned lo, unsigned hi);                         // "log2n must be <lo> .. <hi>"
int check_srs_holds(const char* who, const Srs& srs, unsigned log2, const char* name = "log2n");    // "the SRS holds fewer than 2^<name> points"
int check_srs_device(const char* who, const Srs& srs, const bbg_ctx* ctx, const char* hint = "");   // "the SRS lives on another device than the context<hint>"
int check_fr_nonzero(const char* who, const uint64_t v[4], const char* what);                       // v is 0 or r, the two forms of zero in [0, 2r): <what>

#define BBG_HIP(expr)                                                                                                \
    do {                                                                                                             \
        hipError_t _e = (expr);                                                                                      \
        if (_e != hipSuccess) return ::bbg::hip_fail(_e, #expr, __FILE__, __LINE__);                                  \
    } while (0)

// blocks of `block` threads that cover n items
static inline int grid_for(size_t n, int block) { return (int)((n + block - 1) / block); }

// the byte ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte
static inline bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const char *x = (const char*)a, *y = (const char*)b;
    return x < y + b_bytes && y < x + a_bytes;
}

// A grow-only device buffer: the one owner type of a context's (and a bbg_multi's) working memory.  No destructor frees it: its owner
// is torn down explicitly (bbg_destroy, bbg_memory_trim) after hipSetDevice.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    // at least `need` bytes; growing waits for the device (queued work may still read the old block) and does NOT keep the contents
    int ensure(size_t need)
    {
        if (bytes >= need && p) return BBG_OK;
        if (p) {
            BBG_HIP(hipDeviceSynchronize());
            void* old = p;
            p = nullptr;
            bytes = 0;
            BBG_HIP(hipFree(old));
        }
        hipError_t e = hipMalloc(&p, need);
        if (e != hipSuccess) {
            p = nullptr;
            return hip_fail(e, "hipMalloc(DevBuf)", __FILE__, __LINE__);
        }
        bytes = need;
        return BBG_OK;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};
// `buf` with at least what a finished layout takes: BBG_E_INVALID with "<who>: size out of range" for one that does not fit size_t
static inline int ensure_layout(DevBuf& buf, const RegionLayout& lay, const char* who)
{
    if (!lay.ok()) { set_error(std::string(who) + ": size out of range"); return BBG_E_INVALID; }
    return buf.ensure(lay.total());
}
// the region at byte offset `off` of the buffer at `base`, as T
template <class T> static inline T* at(void* base, size_t off) { return (T*)((char*)base + off); }

// ---------------------------------------------------------------------------------------------- NTT
constexpr int NTT_MAX_PASSES = 4;
// the pass-kernel families of ntt.hip, in the order of its dispatch table: the radix-2-in-LDS kernel, then the three radix-8 ones
enum NttFamily { NTT_PASS = 0, NTT_PASS8, NTT_PASS8S, NTT_PASS29, NTT_FAMILIES };

// Per-domain-size device tables: the GPU counterpart of evaluation_domain::compute_lookup_table()
// (reference polynomials/evaluation_domain.cpp:33-55,169-175).  Built once per log2(n), cached in the context.
struct NttDomain {
    unsigned log2n = 0;
    int passes = 0;
    bool use_pass8 = false; // register-resident radix-8 pass kernel (ntt_pass8.hip.h) vs the radix-2-in-LDS one
    int tile_log8 = 11;     // its tile: 2^11 elements (256 threads) or 2^12 (512 threads: 2^21 / 2^22 in two passes)
    bool inv_scaled = false; // the inverse inter-pass twiddles of pass 0 carry n^-1: ifft needs no scaling sweep
    int logR[NTT_MAX_PASSES] = { 0, 0, 0, 0 };
    int logW[NTT_MAX_PASSES] = { 0, 0, 0, 0 };
    DevBuf consts;                                   // DomainConsts
    DevBuf tw_inter[2][NTT_MAX_PASSES];              // [inverse][pass]: omega_{N_q}^{i*lo}, N_q entries (passes 0..p-2)
    DevBuf tw_radix[2][NTT_MAX_PASSES];              // [inverse][pass]: omega_{R_q}^j, R_q entries
    DevBuf tw_radix29[2][NTT_MAX_PASSES];            // the same entries times 32 (R'-form, canonical): multipliers of the 29-bit-limb pass kernel
    uint64_t root_host[4] = { 0, 0, 0, 0 };          // host copy of the domain's root of unity (Montgomery form, canonical): poly.hip builds evaluation-point tables on the host
    DevBuf coset_fwd;                                // g^j, j < n
    DevBuf coset_inv;                                // n^-1 * g^-j, j < n
    // every device table of the domain (D: NttDomain, const or not): what ntt_free_domain releases and bbg_memory_report counts
    template <class D, class F> static void each_table(D& d, F f)
    {
        f(d.consts), f(d.coset_fwd), f(d.coset_inv);
        for (int inv = 0; inv < 2; inv++)
            for (int q = 0; q < NTT_MAX_PASSES; q++) f(d.tw_inter[inv][q]), f(d.tw_radix[inv][q]), f(d.tw_radix29[inv][q]);
    }
    size_t bytes() const
    {
        size_t sum = 0;
        each_table(*this, [&sum](const DevBuf& b) { sum += b.bytes; });
        return sum;
    }
};

// ---------------------------------------------------------------------------------------------- MSM
struct Srs {
    size_t n = 0;          // number of (plain) points
    void* points = nullptr; // device: n affine points, 64 B each, Montgomery, canonical (= window 0 of a table below)
    static constexpr int MAX_WIDTHS = 7; // BBG_MSM_TABLE_WIDTHS (msm_cfg.h)
    void* tables[MAX_WIDTHS] = {}; // window tables T[w][i] = 2^(MsmCfg<C>::table_offset(w)) P_i (balanced windows, halved weight for the narrow ones: msm_cfg.h) per compiled width C (slot = msm_width_slot(C), msm.hip); built on first use
    int home_slot = -1;    // the table built at registration: its window 0 IS `points`, so it is never released before the handle
    int device = 0;
    // tables[] may be read, built (first MSM of a width) and released (bbg_memory_trim of the owning context) from DIFFERENT contexts'
    // threads: held from the choice of a table until every kernel that reads it is queued, and by the trim around its device
    // synchronisation + free (lock order: bbg_ctx::mu -> g_srs_mu -> Srs::mu)
    std::mutex mu;
};

// Optional per-kernel timing with HIP events on the launch stream (bbg_profile_*): bench.py reads the average
// duration of the dominant kernels live from here, so the roofline numbers do not depend on an external profiler.
struct ProfEntry {
    std::vector<hipEvent_t> start, stop;
};
} // namespace bbg

struct bbg_ctx {
    bool prof_on = false;
    std::map<std::string, bbg::ProfEntry> prof;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::mutex mu;
    std::map<unsigned, bbg::NttDomain> domains;
    // Working memory, grown on demand.  Every buffer but the two MSM arenas (reported as msm_arena) is listed in BBG_CTX_SCRATCH below,
    // which is what bbg_destroy, bbg_memory_trim and bbg_memory_report walk.
    bbg::DevBuf ntt_scratch;
    bbg::DevBuf staging; // device staging for host-pointer entry points
    bbg::DevBuf msm;
    bbg::DevBuf msm_tiny; // digit bytes, sign words and per-block bucket sums of the small-circuit MSM path (msm_tiny.hip)
    uint64_t msm_tiny_layout = 0; // (n_pad, sets, slices) the buffer was last laid out for: another shape moves the double-buffered bucket sums
    bbg::DevBuf poly_scratch; // evaluate / kate partial sums, pow tables
    // MSM reduce phase may run on an auxiliary stream so that it overlaps the next MSM's sort / accumulation
    // MSM_SLOTS reduce phases may be in flight at once, each on its own auxiliary stream with its own working set, so the reduce
    // phases of consecutive MSMs (latency chains that use a sliver of the chip) overlap each other as well as the next accumulation.
    // Two, not more: with four (main + copy + 4 auxiliary streams = 6 > the runtime's 4 hardware queues) streams share queues and
    // pick up false dependencies -- measured 459 instead of 585 Mscalar-mul/s on the headline step, small proofs 10-20 % slower.
    static constexpr int MSM_SLOTS = 2;
    hipStream_t aux_stream = nullptr; // = aux_streams[0] (non-null once the streams exist)
    hipStream_t aux_streams[MSM_SLOTS] = {};
    hipEvent_t ev_acc[MSM_SLOTS] = {}, ev_done[MSM_SLOTS] = {};
    // host-buffer MSM (bbg_msm): the scalars travel in pieces on their own stream, the counting pass of a piece starts when it has landed
    static constexpr int UPLOAD_PIECES = 4;
    hipStream_t upload_stream = nullptr;
    hipEvent_t ev_upload[UPLOAD_PIECES] = {}, ev_upload_go = nullptr;
    int msm_upload_pieces = 1; // option "msm_upload_pieces": 1 = one copy in front of the MSM (default: measured FASTER, profiles/r02_host_msm_ab.txt)
    bool ev_done_valid[MSM_SLOTS] = {};
    unsigned long msm_seq = 0;
    size_t msm_layout_n = 0; // (scalars of the batch, MSMs in it, window width) of the layout the scratch arena currently holds: a change of any
    int msm_layout_sets = 0; // moves every region, so pending reduce phases are joined first (msm_run_c)
    int msm_layout_c = 0;
    void* msm_zero_buf = nullptr; // the arena whose leading zero-initialised regions (partition counters, redo flags) were cleared ...
    int msm_zero_c = 0;           // ... for this window width ...
    int msm_zero_sets = 0;        // ... and this many bucket sets (msm_layout's cap_sets)
    int msm_layout_sort = 1; // (the sort path is part of the layout: the library-sort path reserves rocPRIM's temporary storage)
    int msm_async_reduce = 0; // option "msm_async_reduce": the reduce phase runs on an auxiliary stream (see above)
    int msm_reduce_quad = 14;   // reduce stages with four lanes per EC operation (curve_quad.hip.h): bit 0 combine (a THROUGHPUT kernel over all buckets: one lane per operation is cheaper, measured), 1 row/col, 2 planes, 3 sum
    int msm_acc_waves = 0;           // option "msm_acc_waves": lane segments per SIMD lane of the accumulation (0 = automatic), A/B
    int msm_limbs29 = 1;            // option "msm_limbs29": the accumulation's field arithmetic on 9 x 29-bit limbs (0 = 8 x 32, A/B)
    int msm_accumulate_quad = 1;    // option "msm_accumulate_quad": small MSMs accumulate with four threads per lane segment (0 = one, A/B)
    int msm_reduce_low_priority = 1; // auxiliary stream created with the lowest priority (option "msm_reduce_priority" = 0 undoes it)
    std::map<uint32_t, void*> dpv_consts; // poly.hip: Z*_H division constants per (src, target, roots cut)
    std::map<uint32_t, void*> dpv_tables; // poly.hip: the Z*_H divisor per target-domain point, same key (poly_dpv_table; the prover's round 4)
    bbg::DevBuf gp_totals;  // quotient.hip: grand-product thread totals
    bbg::DevBuf quot_setup; // quotient.hip: derived challenges / constants
    int quotient_setup_plan = 1;     // option "quotient_setup_plan": the widgets' set-up blocks by the lanes of one wave side by side (quotient.hip k_quotient_setup_plan); 0 = the one-lane chain (A/B)
    int poly_limbs29 = 1;            // option "poly_limbs29": linear combinations and evaluations of coefficient arrays on 9 x 29-bit limbs, four terms per reduction (poly29.hip.h); 0 = the 32-bit kernels (A/B)
    int prover_fused_divide = 1;     // option "prover_fused_divide": round 4 divides by Z*_H inside the coset iFFT's first load (poly_dpv_table + ntt_coset_ifft_scaled) instead of a pass of its own; 0 = the separate pass (A/B)
    int prover_tail_window = 0;      // option "prover_tail_window" (A/B): window width of the commitments whose reduce phase ends a round (rounds 4 and 6: the host waits for them with the chip idle) -- fewer buckets, shorter tail, more windows; 0 = the automatic width
    int prover_ntt_batch = 1;       // option "prover_ntt_batch": the wires' iFFTs (round 1) and 4n coset forms of circuits up to 2^17 gates go through ONE launch set each (grid.y = wires) instead of one per wire (A/B)
    int prover_fail_round = 0;       // option "prover_fail_round" (tests only): the next bbg_prover_round<k> returns BBG_E_HIP once -- how the shim's fallback to the reference body is exercised
    int prover_early_cosets = -1; // -1 = from 2^18 gates (default), 0 = never, 1 = always. option "prover_early_cosets": the wires' 4n coset forms are queued behind round 1's last commitment (beside its reduce phase) instead of in front of round 3's grand product
    int prover_msm_batch = 4; // option "prover_msm_batch": commitments of a prover round per launch set (0 / 1 = one each; prover.hip commit())
    int quotient_limbs29 = 1; // option "quotient_limbs29": permutation / fixed-base / fused arithmetic + range + logic widgets on lazily reduced 29-bit limbs (quotient29.hip.h; 0 = the 32-bit kernels, A/B)
    int quotient_fuse = 1; // option "quotient_fuse": arithmetic + range + logic widgets of a chain in one pass over the wires (0 = one kernel each, A/B)
    int msm_window = 0; // 0 = automatic (msm_auto_window), or one of the compiled widths (BBG_MSM_WIDTHS)
    int msm_sort = 1; // 1 = fused recode + MSD partition sort (msm.hip), 0 = k_recode + rocPRIM radix sort + k_offsets
    int ntt_tile_log = 10; // log2(elements per LDS tile); 10/7 measured best on MI355X (profiles/r01_ntt_plan_sweep.txt)
    int ntt_max_logr = 7;
    int ntt_kernel = 2;      // 2 = k_ntt_pass8 where applicable (n >= 2^11), 1 = k_ntt_pass only
    int ntt_max_logr8 = 10;  // max log-radix per pass for k_ntt_pass8
    int ntt_big_tile = 1;    // option "ntt_big_tile": 1 = 2^21 as TWO passes over 4096-element tiles instead of three over 2048; 2 = 2^22 as well; 0 = never
    int ntt_lds_planes = 0;  // option "ntt_lds_planes": 2 = the tile stays in LDS between two steps (k_ntt_pass8), 1 = it moves one 16-byte plane at a time (k_ntt_pass8s: half the LDS, three blocks per CU), 0 = automatic (1 from 2^22)
    int ntt_limbs29 = -1;    // option "ntt_limbs29": 1 = pass arithmetic on lazily reduced 9 x 29-bit limbs (k_ntt_pass29), 0 = 8 x 32-bit (k_ntt_pass8 / 8s), -1 = automatic
    bool ntt_attr_set[bbg::NTT_FAMILIES] = {}; // dynamic-LDS attributes of a family's pass kernels set on this context's device
    // fixed_base.hip: the table T[w][d-1] = d 2^(8w) B of the base point last used (one slot: another base rebuilds it in place)
    bbg::DevBuf fb_table;
    uint64_t fb_table_key[8] = {}; // the base's canonical bytes
    bool fb_table_valid = false;
    // var_base.hip: the lanes' tables of odd multiples (1 KiB per lane) of the windowed GLV multiplication, shared by bbg_g1_batch_mul and
    // the Lagrange transform's stages under "ecntt_mul" = 1
    bbg::DevBuf vb_tables;
    // bbg_g1_ntt*: the XYZZ working set of the transform (128 B per point), grown on demand
    bbg::DevBuf ecntt_work;
    int batch_mul_glv = 1;           // option "batch_mul_glv": 1 = windowed GLV (xyzz_mul_glv), 0 = the bit-serial double-and-add (xyzz_mul_fr), A/B
    long batch_mul_lanes = 1L << 17; // option "batch_mul_lanes": lanes of the variable-base kernels = tables held (a multiple of 64; 2^17 = two waves per SIMD)
    // cells.hip: the tables of one bbg_cells_recover call (roots, points, Z, slot map) or the working array of bbg_cells_values, and the pinned
    // host array the slot map and id lists of a call are built in (cells_copied: the copy of the last call has read it); cells_verify.hip: the
    // working set of one bbg_cells_verify_reduce call, its group lists staged through the same pinned array
    bbg::DevBuf cells_work;
    void* cells_pinned = nullptr;
    size_t cells_pinned_bytes = 0;
    hipEvent_t cells_copied = nullptr;
    // msm_points.hip: the working set of one bbg_g1_msm call (buckets, group sums, partial sums, the counting sort's arrays), at most 1 GiB
    bbg::DevBuf msm_points_work;
    // pairing.hip: the working set of one bbg_pairing_product call: six lane-interleaved Fq12 slots and a flag word for at most 2^16 products
    bbg::DevBuf pairing_work;
    // cells_verify.hip: the intermediates of one bbg_cells_verify call (L, R, the packed pair [L, -R], the off-curve count, the pairing's status
    // word): 512 bytes, sized once
    bbg::DevBuf cells_verdict;
    // open_points.hip: the working set of one chunk of a bbg_open_points call (quotient values, partial sums, hit slots, the MSM's results,
    // flags), at most open_points_budget bytes unless one polynomial alone needs more
    bbg::DevBuf open_points_work;
    long open_points_budget = 1L << 30; // bbg_open_points_set_budget (bytes): what a chunk's working set may take; the tests set it to cross a chunk boundary
    // kzg_verify.hip: the working set of one bbg_kzg_verify_reduce call: the packed points and scalars, the powers of rho, the partial sums
    bbg::DevBuf kzg_work;
    int ecntt_mul = 1;               // option "ecntt_mul": 1 = the Lagrange transform's stages multiply with xyzz_mul_glv (default: measured 2.2x at 2^20, profiles/var_base.txt), 0 = with xyzz_mul_fr (A/B)
};

// every context buffer that bbg_memory_report counts under `scratch`: a new buffer is one member above plus one entry here
constexpr bbg::DevBuf bbg_ctx::* BBG_CTX_SCRATCH[] = {
    &bbg_ctx::ntt_scratch, &bbg_ctx::staging,  &bbg_ctx::poly_scratch, &bbg_ctx::gp_totals,  &bbg_ctx::quot_setup,
    &bbg_ctx::fb_table,    &bbg_ctx::vb_tables, &bbg_ctx::ecntt_work,   &bbg_ctx::cells_work, &bbg_ctx::msm_points_work,
    &bbg_ctx::pairing_work, &bbg_ctx::cells_verdict, &bbg_ctx::open_points_work, &bbg_ctx::kzg_work,
};

// bbg_open_all_prepare[_cells] (open_all.hip), l = 2^log2cell, r = n / l: the l transforms at 2r of the string's residue classes (l = 1:
// NTT_G1,2n of the reversed SRS prefix) and the working arrays of the calls, all owned by the handle.  A workspace is work2 | work1 | sum |
// c_hat for some number of polynomials, every array polynomial-major, in ONE allocation (open_all_work lays it out).
struct bbg_open_all {
    bbg_ctx* ctx = nullptr;
    unsigned log2n = 0;
    unsigned log2cell = 0;
    void* s_hat = nullptr;  // 2n x 64 B affine, infinities possible
    void* own_ws = nullptr; // the single calls' workspace: one polynomial
    // the batched calls' workspace (bbg_open_all_batch_reserve): batch_cap polynomials.  A batched call touches nothing of own_ws.
    void* batch_ws = nullptr;
    size_t batch_cap = 0;
    bool batch_lds_attr = false; // the LDS transform's dynamic-LDS limit is raised on this handle's device (hipFuncSetAttribute is per device)
};

// bbg_g2_lines_prepare (pairing.hip): the line coefficients of `pairs` G2 points, pairs x 16 704 B in the reference's pairing::miller_lines
// layout, owned by the handle
struct bbg_g2_lines {
    int device = 0;
    size_t pairs = 0;
    void* d_lines = nullptr;
};

struct bbg_srs {
    bbg::Srs s;
    bbg_ctx* ctx = nullptr;
    // owners of the handle: the creator plus every bbg_prover built on it (bbg_srs_retain); bbg_srs_free drops one and releases the device
    // memory with the last -- a cache that replaces an entry (shim/bbg_barretenberg_shim.cpp) cannot pull the SRS from under a live prover
    std::atomic<int> refs{ 1 };
};

namespace bbg {
struct ProfScope {
    bbg_ctx* ctx;
    hipStream_t st;
    hipEvent_t stop = nullptr;
    ProfScope(bbg_ctx* c, const char* name, hipStream_t s) : ctx(c), st(s)
    {
        if (!c || !c->prof_on) return;
        hipEvent_t a, b;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
        ProfEntry& e = c->prof[name];
        e.start.push_back(a);
        e.stop.push_back(b);
        (void)hipEventRecord(a, s);
        stop = b;
    }
    ~ProfScope()
    {
        if (stop) (void)hipEventRecord(stop, st);
    }
};
// One staged call of a host-array entry point: a RegionLayout (256 B regions) bound to the context's staging buffer and stream.  The entry
// point asks for its regions in order (each as large as the device call behind it may touch, slack included), ensure() sizes the buffer
// once -- a layout that does not fit size_t is "<who>: size out of range" -- and st[region] is a pointer from then on; up() and down() queue
// the copies, wait() ends the call.  Every step returns BBG_OK or the code of the HIP error with the text set.  The caller holds ctx->mu
// throughout.
class Staged {
  public:
    struct Region { size_t off; };
    Staged(bbg_ctx* c, const char* who_) : ctx(c), who(who_) {}
    Region region(size_t bytes) { return { lay.add(bytes) }; }
    Region region(size_t count, size_t each) { return { lay.add(count, each) }; }
    int ensure() { return ensure_layout(ctx->staging, lay, who); }
    char* operator[](Region r) const { return (char*)ctx->staging.p + r.off; }
    int up(Region r, const void* host, size_t bytes) { BBG_HIP(hipMemcpyAsync((*this)[r], host, bytes, hipMemcpyHostToDevice, ctx->stream)); return BBG_OK; }
    int down(void* host, Region r, size_t bytes) { BBG_HIP(hipMemcpyAsync(host, (*this)[r], bytes, hipMemcpyDeviceToHost, ctx->stream)); return BBG_OK; }
    int wait() { BBG_HIP(hipStreamSynchronize(ctx->stream)); return BBG_OK; }

  private:
    bbg_ctx* ctx;
    const char* who;
    RegionLayout lay{ STAGE_ALIGN };
};
void msm_release_aux_streams(bbg_ctx* ctx); // bbg_capi.hip: destroys the reduce streams and their events, all handles null afterwards
int ntt_run(bbg_ctx* ctx, void* d_coeffs, unsigned log2n, int op, size_t generator_size, const uint64_t* constant,
            hipStream_t stream);
int ntt_ifft_to(bbg_ctx* ctx, const void* d_in, void* d_out, unsigned log2n, hipStream_t stream);
int ntt_ifft_to_batch(bbg_ctx* ctx, int count, const void* const* d_in, void* const* d_out, unsigned log2n, hipStream_t stream);
constexpr int BBG_E_NOFUSE = -100; // internal: this domain's plan has no fused load; never returned through the C ABI
// coset iFFT of a[i] * scale[i] (scale: 2^log2n Montgomery-form values), the product taken as the first pass loads a[i]; BBG_E_NOFUSE
// when the domain's plan has no fused load (single-pass domains) -- the caller scales first and calls ntt_run
int ntt_coset_ifft_scaled(bbg_ctx* ctx, void* d_coeffs, unsigned log2n, const void* d_scale, hipStream_t stream);
int ntt_coset_extend_batch(bbg_ctx* ctx, int count, const void* const* d_in, size_t n_in, void* const* d_out, unsigned log2n, hipStream_t stream);
void ntt_free_domain(NttDomain& d);
int ntt_coset_extend(bbg_ctx* ctx, const void* d_in, size_t n_in, void* d_out, unsigned log2n, hipStream_t stream);
int ntt_coset_split(bbg_ctx* ctx, void* d_coeffs, unsigned log2n, size_t ext, hipStream_t stream);
int ntt_prepare(bbg_ctx* ctx, unsigned log2n);
int ntt_plan(bbg_ctx* ctx, unsigned log2n, int* passes, int* log_radix, int* kernel, int* tile_log);
int ntt_domain_consts(bbg_ctx* ctx, unsigned log2n, void** consts);
int ntt_domain_root_host(bbg_ctx* ctx, unsigned log2n, uint64_t out[4]);
int poly_binop(int op, const void* a, const void* b, void* r, size_t n, hipStream_t st);
int poly_evaluate(bbg_ctx* ctx, const void* d_coeffs, size_t n, const uint64_t* z, uint64_t* out, hipStream_t st);
int poly_kate_opening(bbg_ctx* ctx, const void* d_src, void* d_dest, size_t n, const uint64_t* z, uint64_t* f_out, hipStream_t st);
int poly_divide_pseudo_vanishing(bbg_ctx* ctx, void* d_evals, unsigned log2_src, unsigned log2_target, size_t roots_cut, hipStream_t st);
// barycentric.hip / poly.hip: polynomials in Lagrange form (values on the 2^log2n domain).  BARY_E values per thread, lane-interleaved;
// one 256-thread block covers BARY_BLK consecutive domain points, which is also the group of ONE inversion (Montgomery's trick)
#ifndef BBG_BARY_E
#define BBG_BARY_E 4 // A/B builds only: make EXTRA=-DBBG_BARY_E=8
#endif
constexpr int BARY_E = BBG_BARY_E, BARY_BLK = 256 * BARY_E, BARY_MAX = 32;
constexpr size_t BARY_GRID_MAX = 1024; // four blocks per CU; longer arrays go round a grid-stride loop
constexpr unsigned BARY_NO_HIT = 0xffffffffu;
static inline unsigned bary_grid(size_t n) { return (unsigned)std::min((n + BARY_BLK - 1) / BARY_BLK, BARY_GRID_MAX); }
struct BaryArgs {
    const void* polys[BARY_MAX]; // device arrays of 2^log2n values
    uint32_t shifted;            // bit k: polynomial k at z * w instead of z
    int count;
    unsigned log2n;
    uint32_t z[8], zn[8]; // canonical Montgomery words of z and z^n
    const void* consts;   // DomainConsts of the domain
    void* dest;           // opening only: 2^log2n values, else null
    void* partials;       // count x bary_grid(n) values
    void* results;        // count values
    unsigned* flag;
};
// out[i] = in[i]^-1 (zero stays zero), canonical; d_out may be d_in.  Queues only.
int bary_batch_invert(bbg_ctx* ctx, const void* d_in, void* d_out, size_t n, hipStream_t st);
// results[k] = F_k(z) or F_k(z w); with dest, dest = the values of (F_0(X) - F_0(z)) / (X - z) as well (count = 1).  Queues only.
int bary_evaluate(bbg_ctx* ctx, const BaryArgs& a, hipStream_t st);
// poly.hip: the host side.  *d_results: count canonical values on the device (context scratch), valid until the next polynomial call.
int poly_evaluate_lagrange_async(bbg_ctx* ctx, const void* const* d_evals, const int* shifted, size_t count, unsigned log2n, const uint64_t* z,
                                 void* d_dest, void** d_results, hipStream_t st);
int poly_evaluate_lagrange(bbg_ctx* ctx, const void* const* d_evals, const int* shifted, size_t count, unsigned log2n, const uint64_t* z, uint64_t* out,
                           hipStream_t st);
int poly_kate_opening_lagrange(bbg_ctx* ctx, const void* d_evals, void* d_dest, unsigned log2n, const uint64_t* z, uint64_t* f_out, hipStream_t st);
int poly_batch_invert(bbg_ctx* ctx, const void* d_in, void* d_out, size_t n, hipStream_t st);
// the divisor as a per-point table (cached per context); *table stays valid until bbg_memory_trim / bbg_destroy
int poly_dpv_table(bbg_ctx* ctx, unsigned log2_src, unsigned log2_target, size_t roots_cut, const void** table, hipStream_t st);
int ntt_scale_powers(bbg_ctx* ctx, void* d_a, size_t count, const uint64_t* start, const uint64_t* base, hipStream_t stream);
int ntt_scale_geometric(bbg_ctx* ctx, void* d_a, size_t count, unsigned log2n, int which_base, uint64_t step, uint64_t e0, int mul_inv_log2,
                        hipStream_t st);
int ntt_root_pow(bbg_ctx* ctx, unsigned log2n, uint64_t e, int inverse, uint64_t* out, hipStream_t stream);
int ntt_fr_pow(bbg_ctx* ctx, const uint64_t* base, uint64_t e, uint64_t* out, hipStream_t stream);
int ntt_cross_dft(bbg_ctx* ctx, const void* d_in, void* d_out, unsigned log2G, size_t len, unsigned log2n, int inverse, hipStream_t stream);
int field_op_device(int which, int op, const void* a, const void* b, void* out, size_t n, hipStream_t stream);
// limb29_check.hip: the conformance kernels of the 29-bit-limb arithmetic (bbg_limb29_op)
int limb29_op_shape(int which, int op, int* operands, int* results);
int limb29_op_device(int which, int op, const void* d_in, void* d_out, size_t n, hipStream_t stream);
// tower_check.hip: the conformance kernels of the pairing arithmetic (bbg_tower_op)
int tower_op_shape(int op, int* operands, int* results);
size_t tower_op_work_bytes(int op, size_t n);
int tower_op_device(int op, const void* d_in, void* d_out, void* d_work, size_t n, hipStream_t stream);
// h_scalars (optional): the n scalars are still on the HOST and d_scalars is where they belong on the device -- msm_run uploads them
// itself, piece by piece, overlapped with its first pass
int msm_run(bbg_ctx* ctx, Srs& srs, const void* d_scalars, size_t from, size_t n, void* d_out_jac,
            hipStream_t stream, const void* h_scalars = nullptr);
// `sets` MSMs over one SRS through ONE launch set (msm_cfg.h); result k at d_out_jac + 96 k
int msm_run_batch(bbg_ctx* ctx, Srs& srs, int sets, const void* const* d_scalars, const size_t* from, const size_t* n, void* d_out_jac, hipStream_t stream,
                  const void* h_scalars = nullptr);
// widest window an n-term MSM over srs (may be null) would use now (no table is built)
int msm_plan(bbg_ctx* ctx, const Srs* srs, size_t n, int* c_out);
int srs_synth_linear(bbg_ctx* ctx, uint64_t a, uint64_t s, size_t n, void* d_points, hipStream_t stream);
int msm_join(bbg_ctx* ctx, hipStream_t stream);
int srs_synth_hashed(bbg_ctx* ctx, uint64_t seed, size_t n, void* d_points, hipStream_t stream);
int g1_sum_device(bbg_ctx* ctx, const void* d_jacs, size_t n, void* d_out, hipStream_t stream);
// ecntt.hip: the NTT over G1 behind bbg_srs_lagrange, bbg_g1_ntt and bbg_open_all.  d_src: 2^log2n plain affine points (read only, aff_inf()
// allowed); d_work: 2^log2n x 128 B; d_out: 2^log2n x 64 B canonical affine, may be d_src.  inverse != 0: n^-1 sum_j w_n^(-jk) P_j, else
// sum_j w_n^(jk) P_j.  d_inf_flag != null: *d_inf_flag (cleared by the caller on `stream`) is set when an output is the point at infinity;
// null: such an output is stored as aff_inf().  Queues only, no host synchronisation.
int ecntt_run(bbg_ctx* ctx, const void* d_src, unsigned log2n, int inverse, void* d_work, void* d_out, unsigned* d_inf_flag, hipStream_t stream);
// its three steps: d_work[i] = d_src[bitrev(i)] as XYZZ; the log2n stages in place on d_work (bit-reversed in, natural out); d_work -> affine
int ecntt_load(const void* d_src, unsigned log2n, void* d_work, hipStream_t stream);
int ecntt_stages(bbg_ctx* ctx, void* d_work, unsigned log2n, int inverse, hipStream_t stream);
// the forward stages of the 2^(log2n - log2block) contiguous blocks of 2^log2block points of d_work, each block a transform of its own
int ecntt_stages_blocks(bbg_ctx* ctx, void* d_work, unsigned log2n, unsigned log2block, hipStream_t stream);
// `count` >= 1 independent transforms of 2^log2block points on the contiguous blocks of d_work (each bit-reversed within itself), all
// stages, either direction, one launch per stage
int ecntt_stages_batch(bbg_ctx* ctx, void* d_work, unsigned log2block, size_t count, int inverse, hipStream_t stream);
int ecntt_normalize(bbg_ctx* ctx, const void* d_work, size_t n, void* d_out, unsigned* d_inf_flag, hipStream_t stream);
// fixed_base.hip: d_out[i] = d_scalars[i] * B (64 B canonical affine, aff_inf() for an infinite result) from the context's table of B's
// multiples, which is built on first use and rebuilt for another base.  base_affine: HOST, NULL = the generator; BBG_E_INVALID when it is
// not on the curve.  Queues only.
int fixed_base_mul(bbg_ctx* ctx, const uint64_t* base_affine, const void* d_scalars, size_t n, void* d_out, hipStream_t stream);
// d_out[i] = x^i, i < n (Montgomery Fr, coarse); x: host words.  Queues only.
int fixed_base_powers(const uint64_t x[4], size_t n, void* d_out, hipStream_t stream);
// var_base.hip: d_out[i] = d_scalars[one_scalar ? 0 : i] * d_points[i] (64 B Montgomery affine in, canonical out, aff_inf() for an
// infinite result).  d_out may be d_points; any other overlap, and any overlap of d_out with the scalars, is BBG_E_INVALID.  Queues only.
int var_base_mul(bbg_ctx* ctx, const void* d_points, const void* d_scalars, size_t n, int one_scalar, void* d_out, hipStream_t stream);
// the lanes (a multiple of 64, at most "batch_mul_lanes") a variable-base kernel with `work` items runs on, and their tables in the
// context's buffer (1 KiB per lane, grown on demand)
int var_base_tables(bbg_ctx* ctx, size_t work, size_t* lanes, void** tables);
// msm_points.hip: *d_out = sum_i d_scalars[i] d_points[i] over plain arrays, 64 B canonical affine (aff_inf() for infinity,
// n = 0 included); window_bits 0 = automatic, else 2 .. 16.  Every argument error is BBG_E_INVALID before anything is queued.  Queues only.
int msm_points_run(bbg_ctx* ctx, const void* d_points, const void* d_scalars, size_t n, int window_bits, void* d_out, hipStream_t stream);
// what such a call runs with (any out pointer may be null); needs no device
int msm_points_plan(size_t n, int window_bits, int* c, int* windows, size_t* chunk_terms, size_t* segment_entries);
// pairing.hip.  out_affine[i] = [scalars[i]] base on the twist: HOST arrays, base_affine NULL = the generator of G2; a Staged call.
int g2_mul_host(bbg_ctx* ctx, const uint64_t* base_affine, const uint64_t* scalars, size_t n, uint64_t* out_affine);
// the lines of `pairs` finite points of the order-r subgroup of the twist (HOST, 128 B each); anything else is BBG_E_INVALID.  A Staged call.
int g2_lines_prepare(bbg_ctx* ctx, const uint64_t* g2_affine, size_t pairs, struct bbg_g2_lines** out);
int g2_lines_read(const struct bbg_g2_lines* h, size_t which, uint64_t* out);
void g2_lines_release(struct bbg_g2_lines* h);
// the argument checks of bbg_pairing_product[_device] that look at no device memory: BBG_E_INVALID with the error text set
int pairing_product_check(const char* who, const bbg_ctx* ctx, const struct bbg_g2_lines* h, const void* points, size_t count, const void* out, const void* status);
// d_out_fq12[i] (may be null) = prod_j e(d_g1[i pairs + j], Q_j), canonical; d_status[i] (may be null) = 1: the product is one, 0: it is not, 2: a
// finite point of product i is off the curve.  Queues only once ctx->pairing_work has its size.
int pairing_product_run(bbg_ctx* ctx, const struct bbg_g2_lines* h, const void* d_g1, size_t count, void* d_out_fq12, void* d_status, hipStream_t stream);
// pairing_wave.hip: the same contract with one WAVE per product (k_pair_wave) and no working memory: queues only, always
int pairing_wave_run(bbg_ctx* ctx, const struct bbg_g2_lines* h, const void* d_g1, size_t count, void* d_out_fq12, void* d_status, hipStream_t stream);
// open_all.hip: the handle for 0 <= log2cell <= log2n - 1 (`who`: the entry point, for the text of a HIP error) and a single call
int open_all_prepare(bbg_ctx* ctx, const char* who, const void* d_srs_points, unsigned log2n, unsigned log2cell, struct bbg_open_all** out);
int open_all_run(struct bbg_open_all* h, const void* d_coeffs, void* d_out, hipStream_t stream);
size_t open_all_bytes(unsigned log2n, unsigned log2cell);
// the batched calls: the workspace of one polynomial, the polynomials one workspace may hold (OPEN_BATCH_BUDGET), the
// reservation (0 releases; waits for the device when it replaces one) and the call itself, which walks `count` polynomials in chunks of
// the reservation and queues only
size_t open_all_batch_poly_bytes(unsigned log2n, unsigned log2cell);
size_t open_all_batch_cap(unsigned log2n, unsigned log2cell);
int open_all_batch_reserve(struct bbg_open_all* h, size_t polys);
int open_all_batch_run(struct bbg_open_all* h, const void* d_coeffs, size_t count, void* d_out, hipStream_t stream);
void open_all_release(struct bbg_open_all* h);
// cells.hip.  The checks return BBG_E_INVALID with the error text set; `who` names the entry point in it.
int cells_check_shape(const char* who, unsigned log2n, unsigned log2cell, size_t count);
int cells_check_ids(const char* who, const uint32_t* cell_ids, size_t K, unsigned log2n, unsigned log2cell);
// d_out[p n + m l + t] = f_p(w^(m + r t)), canonical, for `count` coefficient arrays at d_coeffs (read only, no overlap).  Queues only.
int cells_values(bbg_ctx* ctx, const void* d_coeffs, unsigned log2n, unsigned log2cell, size_t count, void* d_out, hipStream_t stream);
// d_out_coeffs[p n ..] = the interpolant of degree < K l through cells cell_ids[k] (HOST, read before the call returns) of polynomial p, whose
// values lie at d_values + ((p K + k) l) x 32 B; canonical.  d_out_coeffs is also the working array of the three transforms.  Queues only.
int cells_recover(bbg_ctx* ctx, const uint32_t* cell_ids, size_t K, const void* d_values, unsigned log2n, unsigned log2cell, size_t count,
                  void* d_out_coeffs, hipStream_t stream);
// ctx->cells_pinned with at least `bytes`, once the copy of the call before has read it; the caller records ctx->cells_copied behind its copy
int cells_pinned_ensure(bbg_ctx* ctx, size_t bytes);
// cells_verify.hip.  The argument checks that need no device pointer: BBG_E_INVALID with the error text set.
int cells_verify_check(const char* who, const bbg_ctx* ctx, const bbg_srs* srs, unsigned log2n, unsigned log2cell, size_t ncom, const uint32_t* commitment_ids,
                       const uint32_t* cell_ids, size_t K, const uint64_t* rho);
// d_out[0] = L = sum_k rho^k pi_k, d_out[1] = R (canonical affine, aff_inf() for infinity); *d_off_curve (may be null) = the finite
// commitments and proofs that are not on the curve.  The id arrays are HOST arrays, read before the call returns.  Queues only.
int cells_verify_reduce(bbg_ctx* ctx, bbg_srs* srs, unsigned log2n, unsigned log2cell, const void* d_commitments, size_t ncom, const uint32_t* commitment_ids,
                        const uint32_t* cell_ids, size_t K, const void* d_values, const void* d_proofs, const uint64_t* rho, void* d_out, void* d_off_curve,
                        hipStream_t stream);
// *d_status (uint32) = 1: every proof is valid under rho, 0: not, 2: a finite commitment or proof is off the curve.  `lines`: the handle of
// ([x^l]_2, [1]_2).  cells_verify_reduce into ctx->cells_verdict, [L, -R] packed there, the wave pairing at count 1, the status word.
// Queues only once the reduction's working memory has its size.
int cells_verify_run(bbg_ctx* ctx, bbg_srs* srs, const struct bbg_g2_lines* lines, unsigned log2n, unsigned log2cell, const void* d_commitments, size_t ncom,
                     const uint32_t* commitment_ids, const uint32_t* cell_ids, size_t K, const void* d_values, const void* d_proofs, const uint64_t* rho,
                     void* d_status, hipStream_t stream);
// the verdict's steps, shared with kzg_verify.hip: the handle's checks (BBG_E_INVALID with the error text set; `first`: what the handle's
// first point is called), ctx->cells_verdict with the places a reduction writes (L, R) and its off-curve count to, and the tail behind such a
// reduction: k_cv_pack, the wave pairing at count 1, k_cv_verdict to *d_status.  The tail queues only.
int cells_verdict_check(const char* who, const bbg_ctx* ctx, const struct bbg_g2_lines* lines, const char* first);
int cells_verdict_buffer(bbg_ctx* ctx, void** d_lr, void** d_off_curve);
int cells_verdict_run(bbg_ctx* ctx, const struct bbg_g2_lines* lines, void* d_status, hipStream_t stream);
// open_points.hip.  poly.hip's check of either form's arguments (device or host arrays; `proofs` null = evaluation only, and
// `lagrange` may then be null): BBG_E_INVALID with the error text set, nothing queued.
int open_points_check(const char* who, const bbg_ctx* ctx, const bbg_srs* lagrange, unsigned log2n, const void* evals, const void* z, size_t count, const void* y,
                      const void* proofs);
// the working set of one polynomial, and the polynomials one chunk holds under the context's budget
size_t open_points_poly_bytes(unsigned log2n, bool proofs);
size_t open_points_chunk(const bbg_ctx* ctx, unsigned log2n, bool proofs, size_t count);
// d_y[k] = F_k(d_z[k]) and, with d_proofs, d_proofs[k] = the commitment over `lagrange` to (F_k(X) - y_k) / (X - z_k); arguments already
// checked.  Queues only once the working memory has its size.
int open_points_run(bbg_ctx* ctx, bbg_srs* lagrange, unsigned log2n, const void* d_evals, const void* d_z, size_t count, void* d_y, void* d_proofs,
                    hipStream_t stream);
// kzg_verify.hip.  The argument checks that look at no overlap: BBG_E_INVALID with the error text set.
int kzg_verify_check(const char* who, const void* commitments, const void* z, const void* y, const void* proofs, size_t N, const uint64_t* rho, const void* out);
// d_out[0] = L = sum_i rho^i pi_i, d_out[1] = R = sum_i rho^i (C_i - [y_i] G + [z_i] pi_i) (canonical affine, aff_inf() for infinity);
// *d_off_curve (may be null) = the finite commitments and proofs that are not on the curve.  Queues only.
int kzg_verify_reduce(bbg_ctx* ctx, const void* d_commitments, const void* d_z, const void* d_y, const void* d_proofs, size_t N, const uint64_t* rho,
                      void* d_out, void* d_off_curve, hipStream_t stream);
// *d_status as cells_verify_run writes it; `lines`: the handle of ([x]_2, [1]_2)
int kzg_verify_run(bbg_ctx* ctx, const struct bbg_g2_lines* lines, const void* d_commitments, const void* d_z, const void* d_y, const void* d_proofs, size_t N,
                   const uint64_t* rho, void* d_status, hipStream_t stream);
// wire.hip.  The bytes per element of a form (either pointer may be null); BBG_E_INVALID for an unknown form, no error text.
int wire_sizes(int form, size_t* wire_bytes, size_t* native_bytes);
// every refusal that looks at no alignment, on host or device pointers alike: BBG_E_INVALID with the error text set
int wire_check(const char* who, int form, int check, size_t n, const void* in, size_t in_each, const void* out, size_t out_each, const void* status,
               const void* bad);
// the device calls: wire_check, the alignment of the device pointers, then the memset of *d_bad and one kernel.  Queue only.
int wire_decode_run(bbg_ctx* ctx, const char* who, int form, const void* d_wire, size_t n, void* d_native, void* d_status, void* d_bad, hipStream_t stream);
int wire_encode_run(bbg_ctx* ctx, const char* who, int form, const void* d_native, size_t n, int check, void* d_wire, void* d_status, void* d_bad,
                    hipStream_t stream);
// out[i] = a[i]^((q + 1) / 4) in Fq, canonical Montgomery (bbg_field_op, op 12)
int wire_sqrt_device(const void* d_a, void* d_out, size_t n, hipStream_t stream);
} // namespace bbg
