// C ABI of libbbg.so (declared in include/bbg.h).  Host-side plumbing only: contexts, device buffers, the SRS
// registry and the Ignition-transcript reader.  All arithmetic runs in the HIP kernels of ntt.hip / msm.hip.
//
// Most calls come as a *_device form on device pointers (the context lock, then the module) and a host-array twin, which reads: argument
// checks, regions, upload, run, download.  Its regions are those of one Staged call (bbg_internal.h): a RegionLayout (region_layout.h: offsets
// aligned to 256 B, overflow reported) over ctx->staging, sized once; no entry point computes an offset into the staging buffer by hand --
// the two of pairing.hip, whose bodies live beside their kernels, included.  The checks several entry points word alike (log2n in a range,
// an SRS too short or on another device, a zero scalar) are bbg_internal.h's check_*.
#include "bbg_internal.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <set>

namespace bbg {

static thread_local std::string g_last_error;

void set_error(const std::string& msg) { g_last_error = msg; }
int hip_fail(hipError_t e, const char* what, const char* file, int line)
{
    char buf[512];
    snprintf(buf, sizeof(buf), "HIP error %d (%s) in %s at %s:%d", (int)e, hipGetErrorString(e), what, file, line);
    g_last_error = buf;
    return e == hipErrorOutOfMemory ? BBG_E_NOMEM : BBG_E_HIP;
}
// the reduce streams and their events, whichever of them exist (a creation that failed half way leaves some): all handles null afterwards
void msm_release_aux_streams(bbg_ctx* ctx)
{
    for (int k = 0; k < bbg_ctx::MSM_SLOTS; k++) {
        if (ctx->aux_streams[k]) (void)hipStreamDestroy(ctx->aux_streams[k]);
        if (ctx->ev_acc[k]) (void)hipEventDestroy(ctx->ev_acc[k]);
        if (ctx->ev_done[k]) (void)hipEventDestroy(ctx->ev_done[k]);
        ctx->aux_streams[k] = nullptr;
        ctx->ev_acc[k] = ctx->ev_done[k] = nullptr;
        ctx->ev_done_valid[k] = false;
    }
    ctx->aux_stream = nullptr;
}
static void prof_release_events(bbg_ctx* ctx)
{
    for (auto& kv : ctx->prof) {
        for (auto e : kv.second.start) (void)hipEventDestroy(e);
        for (auto e : kv.second.stop) (void)hipEventDestroy(e);
    }
    ctx->prof.clear();
}
namespace {
// A temporary of one entry point, released when its scope ends: device memory, or pinned host memory (host = true)
struct ScopedMem {
    void* p = nullptr;
    bool host = false;
    ScopedMem() = default;
    explicit ScopedMem(bool pinned) : host(pinned) {}
    ScopedMem(const ScopedMem&) = delete;
    ScopedMem& operator=(const ScopedMem&) = delete;
    ~ScopedMem()
    {
        if (p) (void)(host ? hipHostFree(p) : hipFree(p));
    }
};

// `step` is a Staged step (bbg_internal.h) or a module's run: leave the entry point with its code unless it is BBG_OK
#define BBG_TRY(step) do { if (int _rc = (step)) return _rc; } while (0)
} // namespace

// the argument checks of bbg_internal.h
static const uint64_t R_MOD[4] = { 0x43e1f593f0000001ULL, 0x2833e84879b97091ULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL }; // the modulus of Fr
static int invalid(const char* who, const std::string& sentence) { set_error(std::string(who) + ": " + sentence); return BBG_E_INVALID; }
int check_log2n(const char* who, unsigned log2n, unsigned lo, unsigned hi)
{
    return log2n < lo || log2n > hi ? invalid(who, "log2n must be " + std::to_string(lo) + " .. " + std::to_string(hi)) : BBG_OK;
}
int check_srs_holds(const char* who, const Srs& srs, unsigned log2, const char* name)
{
    return ((size_t)1 << log2) > srs.n ? invalid(who, std::string("the SRS holds fewer than 2^") + name + " points") : BBG_OK;
}
int check_srs_device(const char* who, const Srs& srs, const bbg_ctx* ctx, const char* hint)
{
    return srs.device != ctx->device ? invalid(who, std::string("the SRS lives on another device than the context") + hint) : BBG_OK;
}
int check_fr_nonzero(const char* who, const uint64_t v[4], const char* what) // the two representatives of 0 in [0, 2r)
{
    return (v[0] | v[1] | v[2] | v[3]) == 0 || memcmp(v, R_MOD, 32) == 0 ? invalid(who, what) : BBG_OK;
}
int srs_build_tables(const void* d_points, size_t n, void* d_table, int c, hipStream_t st);
int msm_pick_window(const bbg_ctx* ctx, size_t n);
void prover_report(const bbg_ctx* ctx, size_t* bytes, unsigned* count); // prover.hip: live bbg_prover handles of a context

// every live SRS handle of the process (bbg_memory_report totals the ones of a context; a handle may outlive its context, so the
// registry is not a member of bbg_ctx)
static std::mutex g_srs_mu;
static std::set<bbg_srs*> g_live_srs;
int permutation_grand_product(bbg_ctx* ctx, const void* const* d_wires, const void* const* d_sigmas, unsigned log2n, const uint64_t* challenges,
                              void* d_z, hipStream_t st);
int poly_lincomb(bbg_ctx* ctx, const void* const* d_polys, const uint64_t* scalars, size_t count, const void* d_base, void* d_out, size_t n, hipStream_t st);
int quotient_widget(bbg_ctx* ctx, int widget, const void* const* d_polys, unsigned log2_large, const uint64_t* challenges, void* d_quotient,
                    uint64_t* alpha_out, hipStream_t st);
int msm_windows_for(int c);
int msm_width_slot(int c);
int msm_width_of_slot(int slot);
constexpr size_t DPV_CONSTS_BYTES = 4096; // poly.hip: one block of Z*_H division constants per (src, target, roots cut)
int g1_normalize_device(const void* d_jacs, size_t n, void* d_out, hipStream_t st);

static int make_srs(bbg_ctx* ctx, const void* d_plain_points, size_t n, bbg_srs** out)
{
    bbg_srs* s = new bbg_srs;
    s->ctx = ctx;
    s->s.n = n;
    s->s.device = ctx->device;
    if (n) {
        // window tables of the width a full-size MSM over this SRS will use; the other width is built on demand (msm_run)
        const int c = msm_pick_window(ctx, n);
        void* table = nullptr;
        hipError_t e = hipMalloc(&table, n * (size_t)msm_windows_for(c) * 64);
        if (e != hipSuccess) {
            delete s;
            return hip_fail(e, "hipMalloc(SRS window tables)", __FILE__, __LINE__);
        }
        int rc = srs_build_tables(d_plain_points, n, table, c, ctx->stream);
        if (rc == BBG_OK && hipStreamSynchronize(ctx->stream) != hipSuccess)
            rc = hip_fail(hipGetLastError(), "SRS table build", __FILE__, __LINE__);
        if (rc) {
            (void)hipFree(table);
            delete s;
            return rc;
        }
        s->s.points = table; // window 0 = the plain points
        s->s.tables[msm_width_slot(c)] = table;
        s->s.home_slot = msm_width_slot(c);
    }
    {
        std::lock_guard<std::mutex> lk(g_srs_mu);
        g_live_srs.insert(s);
    }
    *out = s;
    return BBG_OK;
}

// What the SRS constructors share: n plain points (64 B each) in a buffer of the call's own, filled by fill(d_plain) on the context's stream
// and then registered.  Not the staging buffer: make_srs reads the points after the fill, behind whatever the fill itself staged.
template <class Fill> static int srs_from_filled(bbg_ctx* ctx, size_t n, bbg_srs** out, Fill fill)
{
    std::lock_guard<std::mutex> lk(ctx->mu);
    ScopedMem d_plain;
    BBG_HIP(hipMalloc(&d_plain.p, n ? n * 64 : 64));
    int rc = fill(d_plain.p);
    if (rc == BBG_OK) rc = make_srs(ctx, d_plain.p, n, out); // window tables + the synchronisation
    return rc;
}
// The same for a string of powers: d_pow[i] = s^i, i < n (32 n bytes of working memory beside the points, freed before return), then
// mul(d_pow, d_plain) turns them into the points.  `what` names the working set in the text of an allocation failure.
template <class Mul> static int srs_from_powers(bbg_ctx* ctx, const char* what, const uint64_t s[4], size_t n, bbg_srs** out, Mul mul)
{
    std::lock_guard<std::mutex> lk(ctx->mu);
    ScopedMem d_plain, d_pow;
    hipError_t e = hipMalloc(&d_plain.p, n * 64);
    if (e == hipSuccess) e = hipMalloc(&d_pow.p, n * 32);
    if (e != hipSuccess) return hip_fail(e, what, __FILE__, __LINE__);
    int rc = fixed_base_powers(s, n, d_pow.p, ctx->stream);
    if (rc == BBG_OK) rc = mul(d_pow.p, d_plain.p);
    if (rc) return rc;
    return make_srs(ctx, d_plain.p, n, out); // window tables + the synchronisation
}

// ------------------------------------------------------------------------------------------------ options (bbg_set_option)
namespace {
enum : unsigned {
    OPT_SYNC = 1,         // the device is idle before the value changes
    OPT_RELAYOUT = 2,     // the MSM arena is laid out again by the next MSM
    OPT_DROP_DOMAINS = 4, // the cached NTT domains are freed after the value is stored: the next transform plans with it
};
enum OptStore { AS_VALUE, AS_BOOL, AS_LOW4 }; // (int)value, value != 0, value & 15
constexpr long ANY_LO = std::numeric_limits<long>::min(), ANY_HI = std::numeric_limits<long>::max(); // every long is accepted
struct Option {
    const char* key;
    int bbg_ctx::* field;
    long lo, hi; // accepted range, both ends included
    OptStore store;
    unsigned effects;
    // keys with a rule of their own, applied to a value inside the range before anything changes: BBG_OK, or the error with its text set
    int (*rule)(bbg_ctx* ctx, long value) = nullptr;
    long bbg_ctx::* wide = nullptr; // the one member that is a long (`field` is null then)
};

int opt_compiled_width(bbg_ctx*, long value)
{
    if (value == 0 || msm_width_slot((int)value) >= 0) return BBG_OK;
    set_error("bbg_set_option: msm_window / prover_tail_window must be 0 (automatic) or a compiled width: 13, 16, 17, 19, 20, 22");
    return BBG_E_INVALID;
}
int opt_multiple_of_64(bbg_ctx*, long value)
{
    if (value % 64 == 0) return BBG_OK;
    set_error("bbg_set_option: batch_mul_lanes must be a multiple of 64 in 64 .. 2^20");
    return BBG_E_INVALID;
}
int opt_library_sort(bbg_ctx*, long value)
{
#ifndef BBG_ROCPRIM_SORT
    if (value == 0) { set_error("msm_sort = 0 (rocPRIM radix sort, A/B only) needs a library built with `make ROCPRIM_SORT=1`"); return BBG_E_INVALID; }
#endif
    (void)value;
    return BBG_OK;
}
// fault injection is not an option of a production process: it exists only where the environment asked for test hooks when the process
// started (BBG_TEST_HOOKS=1, read once) -- a stray option string cannot make a proof fail
int opt_test_hook(bbg_ctx*, long)
{
    static const bool hooks = [] { const char* e = getenv("BBG_TEST_HOOKS"); return e && e[0] == '1' && e[1] == 0; }();
    if (hooks) return BBG_OK;
    set_error("bbg_set_option: prover_fail_round is a test hook (start the process with BBG_TEST_HOOKS=1)");
    return BBG_E_INVALID;
}
// the priority is a property of the reduce streams: they go, with their events, once the device is idle (hence no OPT_SYNC on the
// entry), and the next MSM creates them again
int opt_release_aux_streams(bbg_ctx* ctx, long)
{
    BBG_HIP(hipDeviceSynchronize());
    msm_release_aux_streams(ctx);
    return BBG_OK;
}

const Option OPTIONS[] = {
    // MSM
    { "msm_async_reduce", &bbg_ctx::msm_async_reduce, ANY_LO, ANY_HI, AS_BOOL, OPT_SYNC },       // reduce phases on the auxiliary streams (bbg_join)
    { "msm_reduce_priority", &bbg_ctx::msm_reduce_low_priority, ANY_LO, ANY_HI, AS_BOOL, 0, opt_release_aux_streams }, // 1 = low-priority reduce streams
    { "msm_reduce_quad", &bbg_ctx::msm_reduce_quad, ANY_LO, ANY_HI, AS_LOW4, OPT_SYNC },         // bit mask: reduce stages with four lanes per EC operation
    { "msm_acc_waves", &bbg_ctx::msm_acc_waves, ANY_LO, ANY_HI, AS_VALUE, OPT_SYNC | OPT_RELAYOUT }, // lane segments per SIMD lane, 0 = automatic
    { "msm_sort", &bbg_ctx::msm_sort, 0, 1, AS_VALUE, OPT_SYNC, opt_library_sort },              // 1 = partition sort, 0 = rocPRIM radix sort
    { "msm_limbs29", &bbg_ctx::msm_limbs29, ANY_LO, ANY_HI, AS_BOOL, 0 },                        // accumulation on 9 x 29-bit limbs
    { "msm_accumulate_quad", &bbg_ctx::msm_accumulate_quad, ANY_LO, ANY_HI, AS_BOOL, 0 },        // small MSMs: four threads per lane segment
    { "msm_upload_pieces", &bbg_ctx::msm_upload_pieces, 1, bbg_ctx::UPLOAD_PIECES, AS_VALUE, 0 }, // bbg_msm: pieces the host scalars travel in
    { "msm_window", &bbg_ctx::msm_window, ANY_LO, ANY_HI, AS_VALUE, 0, opt_compiled_width },     // 0 = automatic, or a compiled width
    // G1 batch multiplication and transforms
    { "batch_mul_glv", &bbg_ctx::batch_mul_glv, 0, 1, AS_VALUE, 0 },                             // 1 = windowed GLV, 0 = bit-serial double-and-add
    { "batch_mul_lanes", nullptr, 64, 1L << 20, AS_VALUE, 0, opt_multiple_of_64, &bbg_ctx::batch_mul_lanes }, // lanes = 1 KiB tables held; a launch-time choice
    { "ecntt_mul", &bbg_ctx::ecntt_mul, 0, 1, AS_VALUE, 0 },                                     // the G1 transforms' stages: 1 = windowed GLV, 0 = bit-serial
    // quotient, polynomials, prover
    { "quotient_limbs29", &bbg_ctx::quotient_limbs29, ANY_LO, ANY_HI, AS_BOOL, 0 },              // widgets on lazily reduced 29-bit limbs
    { "quotient_fuse", &bbg_ctx::quotient_fuse, ANY_LO, ANY_HI, AS_BOOL, 0 },                    // arithmetic + range + logic widgets in one pass
    { "quotient_setup_plan", &bbg_ctx::quotient_setup_plan, 0, 1, AS_VALUE, 0 },                 // set-up blocks by the lanes of one wave
    { "poly_limbs29", &bbg_ctx::poly_limbs29, 0, 1, AS_VALUE, 0 },                               // linear combinations / evaluations on 29-bit limbs
    { "prover_fused_divide", &bbg_ctx::prover_fused_divide, 0, 1, AS_VALUE, 0 },                 // round 4 divides inside the coset iFFT's first load
    { "prover_tail_window", &bbg_ctx::prover_tail_window, ANY_LO, ANY_HI, AS_VALUE, 0, opt_compiled_width }, // width of the round-ending commitments
    { "prover_ntt_batch", &bbg_ctx::prover_ntt_batch, ANY_LO, ANY_HI, AS_BOOL, 0 },              // the wires' transforms through one launch set
    { "prover_msm_batch", &bbg_ctx::prover_msm_batch, 0, BBG_MSM_BATCH_MAX, AS_VALUE, 0 },       // commitments of a round per launch set
    { "prover_early_cosets", &bbg_ctx::prover_early_cosets, -1, 1, AS_VALUE, 0 },                // -1 = automatic (from 2^18 gates)
    { "prover_fail_round", &bbg_ctx::prover_fail_round, ANY_LO, ANY_HI, AS_VALUE, 0, opt_test_hook }, // tests only: the next call of this round fails once
    // NTT: the first two are launch-time choices between kernels over the same plan and tables, the others change the plan
    { "ntt_limbs29", &bbg_ctx::ntt_limbs29, -1, 1, AS_VALUE, 0 },                                // -1 = automatic
    { "ntt_lds_planes", &bbg_ctx::ntt_lds_planes, 0, 2, AS_VALUE, 0 },                           // 0 = automatic
    { "ntt_tile_log", &bbg_ctx::ntt_tile_log, 9, 12, AS_VALUE, OPT_DROP_DOMAINS },               // log2(elements per LDS tile)
    { "ntt_kernel", &bbg_ctx::ntt_kernel, 1, 2, AS_VALUE, OPT_DROP_DOMAINS },                    // 2 = radix-8 passes in registers, 1 = radix 2 in LDS
    { "ntt_big_tile", &bbg_ctx::ntt_big_tile, 0, 3, AS_VALUE, OPT_DROP_DOMAINS },                // 4096-element tiles for 2^21 (1), 2^22 as well (2)
    { "ntt_max_logr8", &bbg_ctx::ntt_max_logr8, 6, 11, AS_VALUE, OPT_DROP_DOMAINS },             // max log-radix per radix-8 pass
    { "ntt_max_logr", &bbg_ctx::ntt_max_logr, 4, 10, AS_VALUE, OPT_DROP_DOMAINS },               // max log-radix per radix-2 pass
};
} // namespace
} // namespace bbg

using namespace bbg;

#define CHECK_CTX(ctx)                                                                                               \
    do {                                                                                                             \
        if (!(ctx)) { set_error("null bbg_ctx"); return BBG_E_INVALID; }                                             \
        hipError_t _e = hipSetDevice((ctx)->device);                                                                 \
        if (_e != hipSuccess) return hip_fail(_e, "hipSetDevice", __FILE__, __LINE__);                               \
    } while (0)

extern "C" {

const char* bbg_last_error(void) { return g_last_error.c_str(); }

int bbg_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int bbg_init(int device, bbg_ctx** out)
{
    if (!out) { set_error("bbg_init: null out"); return BBG_E_INVALID; }
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) {
        set_error("bbg_init: no HIP device visible (this library has no CPU fallback)");
        return BBG_E_NODEVICE;
    }
    if (device < 0 || device >= n) { set_error("bbg_init: device index out of range"); return BBG_E_INVALID; }
    BBG_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    BBG_HIP(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) {
        set_error(std::string("bbg_init: device is ") + prop.gcnArchName + ", this build targets gfx950 (MI355X) only");
        return BBG_E_NODEVICE;
    }
    bbg_ctx* c = new bbg_ctx;
    c->device = device;
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return hip_fail(e, "hipStreamCreate", __FILE__, __LINE__); }
    c->own_stream = true;
    *out = c;
    return BBG_OK;
}

void bbg_destroy(bbg_ctx* ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    for (auto& kv : ctx->domains) ntt_free_domain(kv.second);
    prof_release_events(ctx);
    for (auto& kv : ctx->dpv_consts) (void)hipFree(kv.second);
    for (auto& kv : ctx->dpv_tables) (void)hipFree(kv.second);
    for (auto b : BBG_CTX_SCRATCH) (ctx->*b).release();
    ctx->msm.release();
    ctx->msm_tiny.release();
    msm_release_aux_streams(ctx);
    if (ctx->cells_pinned) (void)hipHostFree(ctx->cells_pinned);
    if (ctx->cells_copied) (void)hipEventDestroy(ctx->cells_copied);
    if (ctx->upload_stream) {
        (void)hipStreamDestroy(ctx->upload_stream);
        (void)hipEventDestroy(ctx->ev_upload_go);
        for (int k = 0; k < bbg_ctx::UPLOAD_PIECES; k++) (void)hipEventDestroy(ctx->ev_upload[k]);
    }
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int bbg_sync(bbg_ctx* ctx)
{
    CHECK_CTX(ctx);
    BBG_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->aux_stream)
        for (int k = 0; k < bbg_ctx::MSM_SLOTS; k++) BBG_HIP(hipStreamSynchronize(ctx->aux_streams[k]));
    return BBG_OK;
}

int bbg_join(bbg_ctx* ctx)
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return msm_join(ctx, ctx->stream);
}

int bbg_join_lag(bbg_ctx* ctx, int lag)
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (lag <= 0) return msm_join(ctx, ctx->stream);
    // wait for every outstanding reduction except the `lag` most recent ones (slots are used round robin)
    for (int back = lag; back < bbg_ctx::MSM_SLOTS; back++) {
        if (ctx->msm_seq < (unsigned long)back + 1) break;
        const int slot = (int)((ctx->msm_seq - 1 - (unsigned long)back) % bbg_ctx::MSM_SLOTS);
        if (ctx->ev_done_valid[slot]) BBG_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_done[slot], 0));
    }
    return BBG_OK;
}

int bbg_set_stream(bbg_ctx* ctx, void* hip_stream)
{
    CHECK_CTX(ctx);
    BBG_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    ctx->stream = (hipStream_t)hip_stream;
    ctx->own_stream = false;
    return BBG_OK;
}

int bbg_set_option(bbg_ctx* ctx, const char* key, long value)
{
    CHECK_CTX(ctx);
    if (!key) { set_error("bbg_set_option: null key"); return BBG_E_INVALID; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    const Option* o = std::find_if(std::begin(OPTIONS), std::end(OPTIONS), [&](const Option& x) { return !strcmp(x.key, key); });
    if (o == std::end(OPTIONS)) { set_error(std::string("bbg_set_option: unknown key ") + key); return BBG_E_INVALID; }
    if (value < o->lo || value > o->hi) {
        set_error(std::string("bbg_set_option: ") + key + " must be in " + std::to_string(o->lo) + " .. " + std::to_string(o->hi));
        return BBG_E_INVALID;
    }
    if (o->rule) {
        int rc = o->rule(ctx, value);
        if (rc) return rc;
    }
    if (o->effects & OPT_SYNC) BBG_HIP(hipDeviceSynchronize());
    if (o->wide) ctx->*o->wide = value;
    else ctx->*o->field = o->store == AS_BOOL ? value != 0 : o->store == AS_LOW4 ? (int)value & 15 : (int)value;
    if (o->effects & OPT_RELAYOUT) ctx->msm_layout_n = 0;
    if (o->effects & OPT_DROP_DOMAINS) { // plans are per domain: drop cached domains so the new plan takes effect
        BBG_HIP(hipDeviceSynchronize());
        for (auto& kv : ctx->domains) ntt_free_domain(kv.second);
        ctx->domains.clear();
    }
    return BBG_OK;
}

// ------------------------------------------------------------------------------------------------ HBM budget
int bbg_memory_report(bbg_ctx* ctx, bbg_memory_info* out)
{
    CHECK_CTX(ctx);
    if (!out) { set_error("bbg_memory_report: null out"); return BBG_E_INVALID; }
    memset(out, 0, sizeof(*out));
    {
        std::lock_guard<std::mutex> lk(g_srs_mu);
        for (const bbg_srs* s : g_live_srs) {
            if (s->ctx != ctx) continue;
            out->live_srs++;
            std::lock_guard<std::mutex> lk2(const_cast<bbg_srs*>(s)->s.mu);
            for (int k = 0; k < Srs::MAX_WIDTHS; k++)
                if (s->s.tables[k]) out->srs_tables += s->s.n * (size_t)msm_windows_for(msm_width_of_slot(k)) * 64;
        }
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    for (const auto& kv : ctx->domains) {
        out->ntt_tables += kv.second.bytes();
        out->ntt_domains++;
    }
    for (const auto& kv : ctx->dpv_tables) out->ntt_tables += (size_t)32 << ((kv.first >> 8) & 0xff); // poly_dpv_table: one Fr per target-domain point
    out->msm_arena = ctx->msm.bytes + ctx->msm_tiny.bytes;
    out->scratch = ctx->dpv_consts.size() * (size_t)DPV_CONSTS_BYTES;
    for (auto b : BBG_CTX_SCRATCH) out->scratch += (ctx->*b).bytes;
    prover_report(ctx, &out->prover_keys, &out->live_provers);
    out->total = out->srs_points + out->srs_tables + out->ntt_tables + out->msm_arena + out->scratch + out->prover_keys;
    BBG_HIP(hipMemGetInfo(&out->device_free, &out->device_total));
    return BBG_OK;
}

int bbg_memory_trim(bbg_ctx* ctx, int tables, size_t* released)
{
    CHECK_CTX(ctx);
    bbg_memory_info before, after;
    int rc = bbg_memory_report(ctx, &before);
    if (rc) return rc;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        BBG_HIP(hipDeviceSynchronize()); // nothing queued may still read what goes away
        for (auto& kv : ctx->domains) ntt_free_domain(kv.second);
        ctx->domains.clear();
        for (auto& kv : ctx->dpv_consts) (void)hipFree(kv.second);
        ctx->dpv_consts.clear();
        for (auto& kv : ctx->dpv_tables) (void)hipFree(kv.second);
        ctx->dpv_tables.clear();
        for (auto b : BBG_CTX_SCRATCH) (ctx->*b).release();
        ctx->fb_table_valid = false; // the next fixed-base call rebuilds the table
        ctx->msm.release();
        ctx->msm_tiny.release();
        ctx->msm_tiny_layout = 0;
        ctx->msm_layout_n = 0; // the arena's counters are re-initialised with the next layout
        ctx->msm_zero_buf = nullptr;
        ctx->msm_zero_c = 0;
        ctx->msm_zero_sets = 0;
        for (int k = 0; k < bbg_ctx::MSM_SLOTS; k++) ctx->ev_done_valid[k] = false;
        if (tables) {
            std::lock_guard<std::mutex> lk2(g_srs_mu);
            for (bbg_srs* s : g_live_srs) {
                if (s->ctx != ctx) continue;
                // an MSM issued through ANOTHER context on this SRS holds Srs::mu while it picks a table and queues the kernels that read
                // it: with the lock, whatever was queued before is on the device, and the synchronisation below waits for it
                std::lock_guard<std::mutex> lk3(s->s.mu);
                BBG_HIP(hipDeviceSynchronize());
                for (int k = 0; k < Srs::MAX_WIDTHS; k++)
                    if (s->s.tables[k] && k != s->s.home_slot) { // the registration table holds the plain points: it stays
                        (void)hipFree(s->s.tables[k]);
                        s->s.tables[k] = nullptr;
                    }
            }
        }
    }
    rc = bbg_memory_report(ctx, &after);
    if (rc) return rc;
    if (released) *released = before.total > after.total ? before.total - after.total : 0; // another thread may have allocated in between
    return BBG_OK;
}

// ------------------------------------------------------------------------------------------------ kernel timing
int bbg_profile_enable(bbg_ctx* ctx, int on)
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    BBG_HIP(hipStreamSynchronize(ctx->stream));
    prof_release_events(ctx);
    ctx->prof_on = on != 0;
    return BBG_OK;
}
int bbg_profile_get(bbg_ctx* ctx, const char* name, double* total_ms, size_t* launches)
{
    CHECK_CTX(ctx);
    if (!name || !total_ms || !launches) { set_error("bbg_profile_get: null argument"); return BBG_E_INVALID; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    BBG_HIP(hipStreamSynchronize(ctx->stream));
    *total_ms = 0;
    *launches = 0;
    auto it = ctx->prof.find(name);
    if (it == ctx->prof.end()) return BBG_OK;
    for (size_t i = 0; i < it->second.start.size(); i++) {
        float ms = 0;
        BBG_HIP(hipEventElapsedTime(&ms, it->second.start[i], it->second.stop[i]));
        *total_ms += ms;
    }
    *launches = it->second.start.size();
    return BBG_OK;
}

// ------------------------------------------------------------------------------------------------ memory helpers
int bbg_dev_alloc(bbg_ctx* ctx, size_t bytes, void** d_ptr)
{
    CHECK_CTX(ctx);
    if (!d_ptr) { set_error("bbg_dev_alloc: null out"); return BBG_E_INVALID; }
    BBG_HIP(hipMalloc(d_ptr, bytes ? bytes : 1));
    return BBG_OK;
}
int bbg_dev_free(bbg_ctx* ctx, void* d_ptr)
{
    CHECK_CTX(ctx);
    BBG_HIP(hipFree(d_ptr));
    return BBG_OK;
}
int bbg_dev_upload(bbg_ctx* ctx, void* d_dst, const void* src, size_t bytes)
{
    CHECK_CTX(ctx);
    BBG_HIP(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    BBG_HIP(hipStreamSynchronize(ctx->stream));
    return BBG_OK;
}
int bbg_dev_download(bbg_ctx* ctx, void* dst, const void* d_src, size_t bytes)
{
    CHECK_CTX(ctx);
    BBG_HIP(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    BBG_HIP(hipStreamSynchronize(ctx->stream));
    return BBG_OK;
}

// ------------------------------------------------------------------------------------------------ SRS
int bbg_srs_register(bbg_ctx* ctx, const uint64_t* points, size_t n, size_t stride_bytes, bbg_srs** out)
{
    CHECK_CTX(ctx);
    if (!out || (!points && n)) { set_error("bbg_srs_register: null argument"); return BBG_E_INVALID; }
    if (stride_bytes != 64 && stride_bytes != 128) {
        set_error("bbg_srs_register: stride_bytes must be 64 (plain points) or 128 (interleaved endomorphism table)");
        return BBG_E_INVALID;
    }
    return srs_from_filled(ctx, n, out, [&](void* d_plain) {
        const hipError_t e = stride_bytes == 64 ? hipMemcpyAsync(d_plain, points, n * 64, hipMemcpyHostToDevice, ctx->stream)
                                                : hipMemcpy2DAsync(d_plain, 64, points, 128, 64, n, hipMemcpyHostToDevice, ctx->stream);
        return e == hipSuccess ? BBG_OK : hip_fail(e, "SRS upload", __FILE__, __LINE__);
    });
}

int bbg_srs_register_device(bbg_ctx* ctx, const void* d_points, size_t n, bbg_srs** out)
{
    CHECK_CTX(ctx);
    if (!out || (!d_points && n)) { set_error("bbg_srs_register_device: null argument"); return BBG_E_INVALID; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    return make_srs(ctx, d_points, n, out);
}

int bbg_srs_synth_linear(bbg_ctx* ctx, uint64_t a, uint64_t s, size_t n, bbg_srs** out)
{
    CHECK_CTX(ctx);
    if (!out) { set_error("bbg_srs_synth_linear: null out"); return BBG_E_INVALID; }
    if (s == 0 || a == 0) { set_error("bbg_srs_synth_linear: a and s must be non-zero"); return BBG_E_INVALID; }
    return srs_from_filled(ctx, n, out, [&](void* d_plain) { return srs_synth_linear(ctx, a, s, n, d_plain, ctx->stream); });
}

int bbg_srs_synth_hashed(bbg_ctx* ctx, uint64_t seed, size_t n, bbg_srs** out)
{
    CHECK_CTX(ctx);
    if (!out) { set_error("bbg_srs_synth_hashed: null out"); return BBG_E_INVALID; }
    return srs_from_filled(ctx, n, out, [&](void* d_plain) { return srs_synth_hashed(ctx, seed, n, d_plain, ctx->stream); });
}

// Structured string P_i = [x^i] G: the powers x^i on the device, then the fixed-base multiplication by the generator's table straight
// into the plain-point buffer (fixed_base.hip).
int bbg_srs_synth_powers(bbg_ctx* ctx, const uint64_t x[4], size_t n, bbg_srs** out)
{
    CHECK_CTX(ctx);
    if (!out || !x) { set_error("bbg_srs_synth_powers: null argument"); return BBG_E_INVALID; }
    if (n == 0) { set_error("bbg_srs_synth_powers: n must be at least 1"); return BBG_E_INVALID; }
    if (int rc = check_fr_nonzero("bbg_srs_synth_powers", x, "x = 0 (P_1 would be the point at infinity)")) return rc;
    return srs_from_powers(ctx, "bbg_srs_synth_powers: working set", x, n, out,
                           [&](const void* d_pow, void* d_plain) { return fixed_base_mul(ctx, nullptr, d_pow, n, d_plain, ctx->stream); });
}

// The update step of a powers-of-x string, P_i' = [y^i] P_i: the powers y^i on the device (k_fb_powers), the variable-base batch
// multiplication (var_base.hip) from the SRS's plain points into a fresh buffer, then the registration.  The lanes' tables beside it.
int bbg_srs_scale_powers(bbg_ctx* ctx, bbg_srs* srs, const uint64_t y[4], bbg_srs** out)
{
    CHECK_CTX(ctx);
    if (!srs || !y || !out) { set_error("bbg_srs_scale_powers: null argument"); return BBG_E_INVALID; }
    if (int rc = check_srs_device("bbg_srs_scale_powers", srs->s, ctx)) return rc;
    if (int rc = check_fr_nonzero("bbg_srs_scale_powers", y, "y = 0 (P_1 would become the point at infinity)")) return rc;
    const size_t n = srs->s.n;
    if (n == 0) { set_error("bbg_srs_scale_powers: the SRS is empty"); return BBG_E_INVALID; }
    return srs_from_powers(ctx, "bbg_srs_scale_powers: working set", y, n, out,
                           [&](const void* d_pow, void* d_plain) { return var_base_mul(ctx, srs->s.points, d_pow, n, 0, d_plain, ctx->stream); });
}

// pts: num_points x 8 limbs in STANDARD (non-Montgomery) form, slot 0 free: sets monomials[0] = G = (1, 2), converts to Montgomery form
// on the device and registers the SRS (the tail of read_transcript_g1 / Pippenger's constructors)
static int srs_from_plain_points(bbg_ctx* ctx, std::vector<uint64_t>& pts, size_t num_points, bbg_srs** out)
{
    for (int i = 0; i < 8; i++) pts[i] = 0;
    pts[0] = 1;
    pts[4] = 2;
    return srs_from_filled(ctx, num_points, out, [&](void* d_plain) {
        const hipError_t e = hipMemcpyAsync(d_plain, pts.data(), num_points * 64, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "transcript upload", __FILE__, __LINE__);
        return field_op_device(1, 5 /* to_montgomery */, d_plain, nullptr, d_plain, num_points * 2, ctx->stream);
    });
}

// Ignition transcript reader: restates io::read_transcript_g1 (reference srs/io.cpp:134-162): manifest of seven
// big-endian u32 (:11-19,31-45), then num_g1_points x 64 B, every 8-byte limb big-endian, limbs least-significant
// first, values NOT in Montgomery form (:47-67).  monomials[0] = G, file points follow; files transcript00.dat,
// transcript01.dat, ... are consumed until num_points are read (:123-126).  Conversion to Montgomery form runs
// on the device.
int bbg_srs_load_transcript(bbg_ctx* ctx, const char* dir, size_t num_points, bbg_srs** out)
{
    CHECK_CTX(ctx);
    if (!dir || !out || num_points == 0) { set_error("bbg_srs_load_transcript: bad argument"); return BBG_E_INVALID; }
    std::vector<uint64_t> pts(num_points * 8);
    size_t num_read = 1;
    for (size_t num = 0; num_read < num_points; num++) {
        char name[64];
        snprintf(name, sizeof(name), "/transcript%02zu.dat", num);
        std::string path = std::string(dir) + name;
        std::ifstream f(path, std::ifstream::binary);
        if (!f.good()) break;
        unsigned char m[28];
        f.read((char*)m, 28);
        if (f.gcount() != 28) { set_error("bbg_srs_load_transcript: short manifest in " + path); return BBG_E_INVALID; }
        auto be32 = [&](int k) { return ((uint32_t)m[4 * k] << 24) | ((uint32_t)m[4 * k + 1] << 16) | ((uint32_t)m[4 * k + 2] << 8) | m[4 * k + 3]; };
        const size_t num_g1 = be32(4);
        const size_t take = std::min(num_g1, num_points - num_read);
        f.read((char*)&pts[num_read * 8], (std::streamsize)(take * 64));
        if ((size_t)f.gcount() != take * 64) { set_error("bbg_srs_load_transcript: short read in " + path); return BBG_E_INVALID; }
        for (size_t i = num_read * 8; i < (num_read + take) * 8; i++) pts[i] = __builtin_bswap64(pts[i]);
        num_read += take;
    }
    if (num_read < num_points) {
        char buf[160];
        snprintf(buf, sizeof(buf), "Only read %zu points but require %zu. Is your srs large enough?", num_read, num_points);
        set_error(buf);
        return BBG_E_INVALID;
    }
    return srs_from_plain_points(ctx, pts, num_points, out);
}

// Pippenger(uint8_t const* points, size_t num_points) (pippenger.cpp:7-17; the C binding new_pippenger, c_bind.cpp:21-24): the points of a
// transcript already in memory -- (num_points - 1) x 64 bytes in the file encoding (io::read_g1_elements_from_buffer, srs/io.cpp:47-67);
// monomials[0] = G.
int bbg_srs_register_transcript_buffer(bbg_ctx* ctx, const uint8_t* points, size_t num_points, bbg_srs** out)
{
    CHECK_CTX(ctx);
    if (!out || num_points == 0 || (!points && num_points > 1)) { set_error("bbg_srs_register_transcript_buffer: bad argument"); return BBG_E_INVALID; }
    std::vector<uint64_t> pts(num_points * 8);
    if (num_points > 1) memcpy(&pts[8], points, (num_points - 1) * 64);
    for (size_t i = 8; i < num_points * 8; i++) pts[i] = __builtin_bswap64(pts[i]);
    return srs_from_plain_points(ctx, pts, num_points, out);
}

// BLAKE2b-512 (RFC 7693, unkeyed), the checksum an Ignition transcript carries after its points (srs/io.cpp:21-29 accounts for its
// 64 bytes; the reference reader skips it).  Host-side byte hashing, no field arithmetic.
namespace {
struct Blake2b {
    uint64_t h[8], t = 0;
    uint8_t buf[128];
    size_t fill = 0;
    static uint64_t rotr(uint64_t x, int r) { return (x >> r) | (x << (64 - r)); }
    Blake2b()
    {
        static const uint64_t IV[8] = { 0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
                                        0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL, 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL };
        for (int i = 0; i < 8; i++) h[i] = IV[i];
        h[0] ^= 0x01010040ULL; // digest length 64, no key, fanout 1, depth 1
    }
    void compress(const uint8_t* block, bool last)
    {
        static const uint64_t IV[8] = { 0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
                                        0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL, 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL };
        static const uint8_t SIGMA[12][16] = {
            { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15 }, { 14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3 },
            { 11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4 }, { 7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8 },
            { 9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13 }, { 2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9 },
            { 12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11 }, { 13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10 },
            { 6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5 }, { 10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0 },
            { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15 }, { 14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3 } };
        uint64_t m[16], v[16];
        memcpy(m, block, 128); // little-endian host
        for (int i = 0; i < 8; i++) { v[i] = h[i]; v[i + 8] = IV[i]; }
        v[12] ^= t;
        if (last) v[14] = ~v[14];
        auto G = [&](int a, int b, int c, int d, uint64_t x, uint64_t y) {
            v[a] = v[a] + v[b] + x; v[d] = rotr(v[d] ^ v[a], 32);
            v[c] = v[c] + v[d];     v[b] = rotr(v[b] ^ v[c], 24);
            v[a] = v[a] + v[b] + y; v[d] = rotr(v[d] ^ v[a], 16);
            v[c] = v[c] + v[d];     v[b] = rotr(v[b] ^ v[c], 63);
        };
        for (int r = 0; r < 12; r++) {
            const uint8_t* sg = SIGMA[r];
            G(0, 4, 8, 12, m[sg[0]], m[sg[1]]);   G(1, 5, 9, 13, m[sg[2]], m[sg[3]]);
            G(2, 6, 10, 14, m[sg[4]], m[sg[5]]);  G(3, 7, 11, 15, m[sg[6]], m[sg[7]]);
            G(0, 5, 10, 15, m[sg[8]], m[sg[9]]);  G(1, 6, 11, 12, m[sg[10]], m[sg[11]]);
            G(2, 7, 8, 13, m[sg[12]], m[sg[13]]); G(3, 4, 9, 14, m[sg[14]], m[sg[15]]);
        }
        for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[i + 8];
    }
    void update(const void* data, size_t len)
    {
        const uint8_t* p = (const uint8_t*)data;
        while (len) {
            if (fill == 128) { // only compress a full buffer when more input follows: the last block is flagged
                t += 128;
                compress(buf, false);
                fill = 0;
            }
            const size_t take = std::min(len, (size_t)128 - fill);
            memcpy(buf + fill, p, take);
            fill += take;
            p += take;
            len -= take;
        }
    }
    void final(uint8_t out[64])
    {
        t += fill;
        memset(buf + fill, 0, 128 - fill);
        compress(buf, true);
        memcpy(out, h, 64);
    }
};
} // namespace

// the checksum of a transcript file body (host only: usable without a GPU, e.g. to validate a downloaded transcript)
int bbg_transcript_checksum(const void* data, size_t len, uint8_t out[64])
{
    if ((!data && len) || !out) { set_error("bbg_transcript_checksum: null argument"); return BBG_E_INVALID; }
    Blake2b hash;
    hash.update(data, len);
    hash.final(out);
    return BBG_OK;
}

// Ignition transcript WRITER, the inverse of bbg_srs_load_transcript / io::read_transcript_g1 (srs/io.cpp:11-45 manifest, :47-67 point
// encoding, :123-162 file sequence): files dir/transcript00.dat, 01, ... hold points 1 .. n-1 of the SRS (point 0 is the generator,
// which every reader supplies itself, :137), points_per_file each (0 = all in one file).  Each point is x || y, every 8-byte limb
// big-endian, limbs least-significant first, values in standard (non-Montgomery) form -- the conversion runs on the device.
// g2_x_raw (may be NULL): 128 bytes appended to file 00 as its single G2 point, written as given.  The 64-byte BLAKE2b-512 checksum
// of everything before it closes each file.
int bbg_srs_write_transcript(bbg_srs* srs, const char* dir, size_t points_per_file, const uint8_t* g2_x_raw)
{
    if (!srs || !dir) { set_error("bbg_srs_write_transcript: null argument"); return BBG_E_INVALID; }
    CHECK_CTX(srs->ctx);
    const size_t n = srs->s.n;
    if (n < 2) { set_error("bbg_srs_write_transcript: nothing to write (an SRS of fewer than 2 points)"); return BBG_E_INVALID; }
    const size_t total = n - 1;
    if (points_per_file == 0 || points_per_file > total) points_per_file = total;
    const size_t files = (total + points_per_file - 1) / points_per_file;
    if (files > 100) { set_error("bbg_srs_write_transcript: more than 100 files (transcriptNN.dat)"); return BBG_E_INVALID; }
    std::vector<uint64_t> plain(total * 8);
    {
        std::lock_guard<std::mutex> lk(srs->ctx->mu);
        ScopedMem d_plain;
        BBG_HIP(hipMalloc(&d_plain.p, total * 64));
        int rc = field_op_device(1, 4 /* from_montgomery */, (const char*)srs->s.points + 64, nullptr, d_plain.p, total * 2, srs->ctx->stream);
        if (rc) return rc;
        hipError_t e = hipMemcpyAsync(plain.data(), d_plain.p, total * 64, hipMemcpyDeviceToHost, srs->ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(srs->ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "transcript download", __FILE__, __LINE__);
    }
    for (auto& limb : plain) limb = __builtin_bswap64(limb);
    auto be32 = [](uint8_t* out, uint32_t v) { out[0] = (uint8_t)(v >> 24); out[1] = (uint8_t)(v >> 16); out[2] = (uint8_t)(v >> 8); out[3] = (uint8_t)v; };
    for (size_t k = 0; k < files; k++) {
        const size_t first = k * points_per_file, count = std::min(points_per_file, total - first);
        const uint32_t num_g2 = (k == 0 && g2_x_raw) ? 1 : 0;
        uint8_t manifest[28];
        const uint32_t fields[7] = { (uint32_t)k, (uint32_t)files, (uint32_t)total, g2_x_raw ? 1u : 0u, (uint32_t)count, num_g2, (uint32_t)first };
        for (int i = 0; i < 7; i++) be32(manifest + 4 * i, fields[i]);
        Blake2b hash;
        hash.update(manifest, 28);
        hash.update(&plain[first * 8], count * 64);
        if (num_g2) hash.update(g2_x_raw, 128);
        uint8_t digest[64];
        hash.final(digest);
        char name[64];
        snprintf(name, sizeof(name), "/transcript%02zu.dat", k);
        const std::string path = std::string(dir) + name;
        std::ofstream f(path, std::ofstream::binary | std::ofstream::trunc);
        if (!f.good()) { set_error("bbg_srs_write_transcript: cannot open " + path); return BBG_E_INVALID; }
        f.write((const char*)manifest, 28);
        f.write((const char*)&plain[first * 8], (std::streamsize)(count * 64));
        if (num_g2) f.write((const char*)g2_x_raw, 128);
        f.write((const char*)digest, 64);
        if (!f.good()) { set_error("bbg_srs_write_transcript: short write to " + path); return BBG_E_INVALID; }
    }
    return BBG_OK;
}

size_t bbg_srs_num_points(const bbg_srs* srs) { return srs ? srs->s.n : 0; }

int bbg_srs_read(bbg_srs* srs, size_t from, size_t count, uint64_t* out_points)
{
    if (!srs || !out_points) { set_error("bbg_srs_read: null argument"); return BBG_E_INVALID; }
    CHECK_CTX(srs->ctx);
    if (from > srs->s.n || count > srs->s.n - from) { set_error("bbg_srs_read: range out of bounds"); return BBG_E_INVALID; }
    BBG_HIP(hipMemcpy(out_points, (const char*)srs->s.points + from * 64, count * 64, hipMemcpyDeviceToHost));
    return BBG_OK;
}

// lagrange_base::transform_srs (srs/lagrange_base_transformation/lagrange_base.cpp:31-46) on the device (ecntt.hip): the first
// 2^log2n points of `srs` become LB[k] = n^-1 sum_j w_n^(-jk) M_j, registered as an SRS of its own.  Everything is queued on the
// context's stream; the one host synchronisation is the table build's (make_srs), after which the infinity flag is read.
int bbg_srs_lagrange(bbg_ctx* ctx, bbg_srs* srs, unsigned log2n, bbg_srs** out)
{
    CHECK_CTX(ctx);
    if (!srs || !out) { set_error("bbg_srs_lagrange: null argument"); return BBG_E_INVALID; }
    if (int rc = check_log2n("bbg_srs_lagrange", log2n, 1, 28)) return rc;
    if (int rc = check_srs_holds("bbg_srs_lagrange", srs->s, log2n)) return rc;
    if (int rc = check_srs_device("bbg_srs_lagrange", srs->s, ctx)) return rc;
    const size_t n = (size_t)1 << log2n;
    std::lock_guard<std::mutex> lk(ctx->mu);
    bbg_srs* res = nullptr;
    bool inf = false;
    {
        ScopedMem d_work, d_plain, d_flag, h_flag(true); // the flag word is pinned: the copy behind the kernels stays asynchronous
        hipError_t e = hipMalloc(&d_work.p, n * 128);
        if (e == hipSuccess) e = hipMalloc(&d_plain.p, n * 64);
        if (e == hipSuccess) e = hipMalloc(&d_flag.p, sizeof(unsigned));
        if (e == hipSuccess) e = hipHostMalloc(&h_flag.p, sizeof(unsigned), hipHostMallocDefault);
        if (e == hipSuccess) {
            *(unsigned*)h_flag.p = 1; // stays set unless the copy below has run
            e = hipMemsetAsync(d_flag.p, 0, sizeof(unsigned), ctx->stream);
        }
        if (e != hipSuccess) return hip_fail(e, "bbg_srs_lagrange: working set", __FILE__, __LINE__);
        int rc = ecntt_run(ctx, srs->s.points, log2n, 1, d_work.p, d_plain.p, (unsigned*)d_flag.p, ctx->stream);
        if (rc) return rc;
        e = hipMemcpyAsync(h_flag.p, d_flag.p, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "bbg_srs_lagrange: flag copy", __FILE__, __LINE__);
        rc = make_srs(ctx, d_plain.p, n, &res); // window tables + the synchronisation
        if (rc) return rc;
        inf = *(unsigned*)h_flag.p != 0; // read before the temporaries go
    }
    if (inf) {
        bbg_srs_free(res);
        set_error("bbg_srs_lagrange: the transform has a point at infinity among its outputs (linearly dependent input points); an SRS cannot hold one");
        return BBG_E_INFINITY;
    }
    *out = res;
    return BBG_OK;
}

// The general transform on plain device arrays: the working set is the context's, the output may be the input, an infinite output is data.
int bbg_g1_ntt_device(bbg_ctx* ctx, const void* d_points_affine, unsigned log2n, int inverse, void* d_out_affine)
{
    CHECK_CTX(ctx);
    if (!d_points_affine || !d_out_affine) { set_error("bbg_g1_ntt_device: null argument"); return BBG_E_INVALID; }
    if (int rc = check_log2n("bbg_g1_ntt_device", log2n, 1, 28)) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    int rc = ctx->ecntt_work.ensure(((size_t)1 << log2n) * 128);
    if (rc) return rc;
    return ecntt_run(ctx, d_points_affine, log2n, inverse, ctx->ecntt_work.p, d_out_affine, nullptr, ctx->stream);
}

int bbg_g1_ntt(bbg_ctx* ctx, const uint64_t* points_affine, unsigned log2n, int inverse, uint64_t* out_affine)
{
    CHECK_CTX(ctx);
    if (!points_affine || !out_affine) { set_error("bbg_g1_ntt: null argument"); return BBG_E_INVALID; }
    if (int rc = check_log2n("bbg_g1_ntt", log2n, 1, 28)) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const size_t n = (size_t)1 << log2n;
    Staged st(ctx, "bbg_g1_ntt");
    const auto d_points = st.region(n, 64); // transformed in place
    BBG_TRY(st.ensure());
    BBG_TRY(ctx->ecntt_work.ensure(n * 128));
    BBG_TRY(st.up(d_points, points_affine, n * 64));
    BBG_TRY(ecntt_run(ctx, st[d_points], log2n, inverse, ctx->ecntt_work.p, st[d_points], nullptr, ctx->stream));
    BBG_TRY(st.down(out_affine, d_points, n * 64));
    return st.wait();
}

// ------------------------------------------------------------------------------------------------ all openings (open_all.hip)
int bbg_open_all_prepare(bbg_ctx* ctx, bbg_srs* srs, unsigned log2n, struct bbg_open_all** out)
{
    CHECK_CTX(ctx);
    if (!srs || !out) { set_error("bbg_open_all_prepare: null argument"); return BBG_E_INVALID; }
    if (int rc = check_log2n("bbg_open_all_prepare", log2n, 1, 27)) return rc;
    if (int rc = check_srs_holds("bbg_open_all_prepare", srs->s, log2n)) return rc;
    if (int rc = check_srs_device("bbg_open_all_prepare", srs->s, ctx)) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return open_all_prepare(ctx, "bbg_open_all_prepare", srs->s.points, log2n, 0, out);
}

int bbg_open_all_prepare_cells(bbg_ctx* ctx, bbg_srs* srs, unsigned log2n, unsigned log2cell, struct bbg_open_all** out)
{
    if (log2cell == 0) return bbg_open_all_prepare(ctx, srs, log2n, out);
    CHECK_CTX(ctx);
    if (!srs || !out) { set_error("bbg_open_all_prepare_cells: null argument"); return BBG_E_INVALID; }
    if (int rc = check_log2n("bbg_open_all_prepare_cells", log2n, 1, 27)) return rc;
    if (log2cell > log2n - 1) { set_error("bbg_open_all_prepare_cells: log2cell must be 0 .. log2n - 1"); return BBG_E_INVALID; }
    if (int rc = check_srs_holds("bbg_open_all_prepare_cells", srs->s, log2n)) return rc;
    if (int rc = check_srs_device("bbg_open_all_prepare_cells", srs->s, ctx)) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    return open_all_prepare(ctx, "bbg_open_all_prepare_cells", srs->s.points, log2n, log2cell, out);
}

int bbg_open_all_count(const struct bbg_open_all* h, size_t* proofs)
{
    if (!h || !proofs) { set_error("bbg_open_all_count: null argument"); return BBG_E_INVALID; }
    *proofs = (size_t)1 << (h->log2n - h->log2cell);
    return BBG_OK;
}

int bbg_open_all_device(struct bbg_open_all* h, const void* d_coeffs, void* d_out_affine)
{
    if (!h || !d_coeffs || !d_out_affine) { set_error("bbg_open_all_device: null argument"); return BBG_E_INVALID; }
    CHECK_CTX(h->ctx);
    std::lock_guard<std::mutex> lk(h->ctx->mu);
    return open_all_run(h, d_coeffs, d_out_affine, h->ctx->stream);
}

int bbg_open_all(struct bbg_open_all* h, const uint64_t* coeffs, uint64_t* out_affine)
{
    if (!h || !coeffs || !out_affine) { set_error("bbg_open_all: null argument"); return BBG_E_INVALID; }
    bbg_ctx* ctx = h->ctx;
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    const size_t n = (size_t)1 << h->log2n, proofs = n >> h->log2cell;
    Staged st(ctx, "bbg_open_all");
    const auto d_proofs = st.region(n, 64), d_coeffs = st.region(n, 32);
    BBG_TRY(st.ensure());
    BBG_TRY(st.up(d_coeffs, coeffs, n * 32));
    BBG_TRY(open_all_run(h, st[d_coeffs], st[d_proofs], ctx->stream));
    BBG_TRY(st.down(out_affine, d_proofs, proofs * 64));
    return st.wait();
}

int bbg_open_all_device_bytes(const struct bbg_open_all* h, size_t* bytes)
{
    if (!h || !bytes) { set_error("bbg_open_all_device_bytes: null argument"); return BBG_E_INVALID; }
    *bytes = open_all_bytes(h->log2n, h->log2cell) + h->batch_cap * open_all_batch_poly_bytes(h->log2n, h->log2cell);
    return BBG_OK;
}

int bbg_open_all_batch_reserve(struct bbg_open_all* h, size_t polys)
{
    if (!h) { set_error("bbg_open_all_batch_reserve: null argument"); return BBG_E_INVALID; }
    CHECK_CTX(h->ctx);
    std::lock_guard<std::mutex> lk(h->ctx->mu);
    return open_all_batch_reserve(h, polys);
}

int bbg_open_all_batch_device(struct bbg_open_all* h, const void* d_coeffs, size_t count, void* d_out_affine)
{
    if (!h || !d_coeffs || !d_out_affine) { set_error("bbg_open_all_batch_device: null argument"); return BBG_E_INVALID; }
    if (count == 0) { set_error("bbg_open_all_batch_device: count must be at least 1"); return BBG_E_INVALID; }
    CHECK_CTX(h->ctx);
    std::lock_guard<std::mutex> lk(h->ctx->mu);
    return open_all_batch_run(h, d_coeffs, count, d_out_affine, h->ctx->stream);
}

int bbg_open_all_batch(struct bbg_open_all* h, const uint64_t* coeffs, size_t count, uint64_t* out_affine)
{
    if (!h || !coeffs || !out_affine) { set_error("bbg_open_all_batch: null argument"); return BBG_E_INVALID; }
    if (count == 0) { set_error("bbg_open_all_batch: count must be at least 1"); return BBG_E_INVALID; }
    bbg_ctx* ctx = h->ctx;
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    const size_t n = (size_t)1 << h->log2n, proofs = n >> h->log2cell;
    if (count > ((size_t)1 << 40) / n) { set_error("bbg_open_all_batch: count x 2^log2n is out of range"); return BBG_E_INVALID; }
    Staged st(ctx, "bbg_open_all_batch");
    const auto d_proofs = st.region(count * n, 64), d_coeffs = st.region(count * n, 32);
    BBG_TRY(st.ensure());
    BBG_TRY(st.up(d_coeffs, coeffs, count * n * 32));
    BBG_TRY(open_all_batch_run(h, st[d_coeffs], count, st[d_proofs], ctx->stream));
    BBG_TRY(st.down(out_affine, d_proofs, count * proofs * 64));
    return st.wait();
}

void bbg_open_all_free(struct bbg_open_all* h)
{
    if (!h) return;
    (void)hipSetDevice(h->ctx->device);
    open_all_release(h);
}

// ------------------------------------------------------------------------------------------------ cells (cells.hip)
int bbg_cells_values_device(bbg_ctx* ctx, const void* d_coeffs, unsigned log2n, unsigned log2cell, size_t count, void* d_out)
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return cells_values(ctx, d_coeffs, log2n, log2cell, count, d_out, ctx->stream);
}

int bbg_cells_values(bbg_ctx* ctx, const uint64_t* coeffs, unsigned log2n, unsigned log2cell, size_t count, uint64_t* out)
{
    CHECK_CTX(ctx);
    if (!coeffs || !out) { set_error("bbg_cells_values: null argument"); return BBG_E_INVALID; }
    BBG_TRY(cells_check_shape("bbg_cells_values", log2n, log2cell, count));
    std::lock_guard<std::mutex> lk(ctx->mu);
    const size_t bytes = count * ((size_t)1 << log2n) * 32;
    Staged st(ctx, "bbg_cells_values");
    const auto d_coeffs = st.region(bytes), d_values = st.region(bytes);
    BBG_TRY(st.ensure());
    BBG_TRY(st.up(d_coeffs, coeffs, bytes));
    BBG_TRY(cells_values(ctx, st[d_coeffs], log2n, log2cell, count, st[d_values], ctx->stream));
    BBG_TRY(st.down(out, d_values, bytes));
    return st.wait();
}

int bbg_cells_recover_device(bbg_ctx* ctx, const uint32_t* cell_ids, size_t K, const void* d_values, unsigned log2n, unsigned log2cell, size_t count,
                             void* d_out_coeffs)
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return cells_recover(ctx, cell_ids, K, d_values, log2n, log2cell, count, d_out_coeffs, ctx->stream);
}

int bbg_cells_recover(bbg_ctx* ctx, const uint32_t* cell_ids, size_t K, const uint64_t* values, unsigned log2n, unsigned log2cell, size_t count,
                      uint64_t* out_coeffs)
{
    CHECK_CTX(ctx);
    if (!values || !out_coeffs) { set_error("bbg_cells_recover: null argument"); return BBG_E_INVALID; }
    BBG_TRY(cells_check_shape("bbg_cells_recover", log2n, log2cell, count));
    BBG_TRY(cells_check_ids("bbg_cells_recover", cell_ids, K, log2n, log2cell));
    std::lock_guard<std::mutex> lk(ctx->mu);
    const size_t in_bytes = count * K * ((size_t)32 << log2cell), out_bytes = count * ((size_t)32 << log2n);
    Staged st(ctx, "bbg_cells_recover");
    const auto d_coeffs = st.region(out_bytes), d_values = st.region(in_bytes);
    BBG_TRY(st.ensure());
    BBG_TRY(st.up(d_values, values, in_bytes));
    BBG_TRY(cells_recover(ctx, cell_ids, K, st[d_values], log2n, log2cell, count, st[d_coeffs], ctx->stream));
    BBG_TRY(st.down(out_coeffs, d_coeffs, out_bytes));
    return st.wait();
}

// ------------------------------------------------------------------------------------------------ cell proofs to one pairing check (cells_verify.hip)
int bbg_cells_verify_reduce_device(bbg_ctx* ctx, bbg_srs* srs, unsigned log2n, unsigned log2cell, const void* d_commitments, size_t ncom,
                                   const uint32_t* commitment_ids, const uint32_t* cell_ids, size_t K, const void* d_values, const void* d_proofs,
                                   const uint64_t rho[4], void* d_out, void* d_off_curve)
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return cells_verify_reduce(ctx, srs, log2n, log2cell, d_commitments, ncom, commitment_ids, cell_ids, K, d_values, d_proofs, rho, d_out, d_off_curve,
                               ctx->stream);
}

int bbg_cells_verify_reduce(bbg_ctx* ctx, bbg_srs* srs, unsigned log2n, unsigned log2cell, const uint64_t* commitments, size_t ncom,
                            const uint32_t* commitment_ids, const uint32_t* cell_ids, size_t K, const uint64_t* values, const uint64_t* proofs,
                            const uint64_t rho[4], uint64_t out[16])
{
    CHECK_CTX(ctx);
    if (!commitments || !values || !proofs || !out) { set_error("bbg_cells_verify_reduce: null argument"); return BBG_E_INVALID; }
    BBG_TRY(cells_verify_check("bbg_cells_verify_reduce", ctx, srs, log2n, log2cell, ncom, commitment_ids, cell_ids, K, rho));
    std::lock_guard<std::mutex> lk(ctx->mu);
    const size_t com_bytes = ncom * 64, proof_bytes = K * 64, value_bytes = K * ((size_t)32 << log2cell);
    Staged st(ctx, "bbg_cells_verify_reduce");
    const auto d_com = st.region(com_bytes), d_proofs = st.region(proof_bytes), d_values = st.region(value_bytes);
    const auto d_res = st.region(256); // L, R (128 B), then the off-curve count: one block, one download
    BBG_TRY(st.ensure());
    BBG_TRY(st.up(d_com, commitments, com_bytes));
    BBG_TRY(st.up(d_proofs, proofs, proof_bytes));
    BBG_TRY(st.up(d_values, values, value_bytes));
    BBG_TRY(cells_verify_reduce(ctx, srs, log2n, log2cell, st[d_com], ncom, commitment_ids, cell_ids, K, st[d_values], st[d_proofs], rho, st[d_res],
                                st[d_res] + 128, ctx->stream));
    uint64_t res[18]; // L, R, then the count in the low word of res[16]
    BBG_TRY(st.down(res, d_res, 128 + 4));
    BBG_TRY(st.wait());
    uint32_t off_curve = 0;
    memcpy(&off_curve, res + 16, 4);
    if (off_curve) {
        set_error("bbg_cells_verify_reduce: " + std::to_string(off_curve) + " of the commitments and proofs are not on the curve");
        return BBG_E_INVALID;
    }
    memcpy(out, res, 128);
    return BBG_OK;
}

int bbg_cells_verify_device(bbg_ctx* ctx, bbg_srs* srs, const bbg_g2_lines* lines, unsigned log2n, unsigned log2cell, const void* d_commitments, size_t ncom,
                            const uint32_t* commitment_ids, const uint32_t* cell_ids, size_t K, const void* d_values, const void* d_proofs,
                            const uint64_t rho[4], void* d_status)
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return cells_verify_run(ctx, srs, lines, log2n, log2cell, d_commitments, ncom, commitment_ids, cell_ids, K, d_values, d_proofs, rho, d_status, ctx->stream);
}

int bbg_cells_verify(bbg_ctx* ctx, bbg_srs* srs, const bbg_g2_lines* lines, unsigned log2n, unsigned log2cell, const uint64_t* commitments, size_t ncom,
                     const uint32_t* commitment_ids, const uint32_t* cell_ids, size_t K, const uint64_t* values, const uint64_t* proofs,
                     const uint64_t rho[4], uint32_t* status)
{
    CHECK_CTX(ctx);
    if (!lines || !commitments || !values || !proofs || !status) { set_error("bbg_cells_verify: null argument"); return BBG_E_INVALID; }
    BBG_TRY(cells_verify_check("bbg_cells_verify", ctx, srs, log2n, log2cell, ncom, commitment_ids, cell_ids, K, rho)); // before the staging buffer is sized by K
    std::lock_guard<std::mutex> lk(ctx->mu);
    const size_t com_bytes = ncom * 64, proof_bytes = K * 64, value_bytes = K * ((size_t)32 << log2cell);
    Staged st(ctx, "bbg_cells_verify");
    const auto d_com = st.region(com_bytes), d_proofs = st.region(proof_bytes), d_values = st.region(value_bytes), d_status = st.region(4);
    BBG_TRY(st.ensure());
    BBG_TRY(st.up(d_com, commitments, com_bytes));
    BBG_TRY(st.up(d_proofs, proofs, proof_bytes));
    BBG_TRY(st.up(d_values, values, value_bytes));
    BBG_TRY(cells_verify_run(ctx, srs, lines, log2n, log2cell, st[d_com], ncom, commitment_ids, cell_ids, K, st[d_values], st[d_proofs], rho, st[d_status],
                             ctx->stream));
    uint32_t word = 0;
    BBG_TRY(st.down(&word, d_status, 4));
    BBG_TRY(st.wait());
    *status = word;
    if (word == 2) {
        set_error("bbg_cells_verify: a commitment or a proof is not on the curve");
        return BBG_E_INVALID;
    }
    return BBG_OK;
}

int bbg_srs_retain(bbg_srs* srs)
{
    if (!srs) { set_error("bbg_srs_retain: null handle"); return BBG_E_INVALID; }
    srs->refs.fetch_add(1);
    return BBG_OK;
}

void bbg_srs_free(bbg_srs* srs)
{
    if (!srs) return;
    if (srs->refs.fetch_sub(1) > 1) return; // another owner (a bbg_prover, a second cache entry) still uses it
    {
        std::lock_guard<std::mutex> lk(g_srs_mu);
        g_live_srs.erase(srs);
    }
    (void)hipSetDevice(srs->s.device); // the handle's own record: the context may already be gone (bbg_destroy before bbg_srs_free)
    (void)hipDeviceSynchronize();
    for (void* t : srs->s.tables)
        if (t) (void)hipFree(t);
    delete srs;
}

// ------------------------------------------------------------------------------------------------ MSM
int bbg_msm_device(bbg_ctx* ctx, bbg_srs* srs, const void* d_scalars, size_t from, size_t n, void* d_out_jacobian)
{
    CHECK_CTX(ctx);
    if (!srs || (!d_scalars && n) || !d_out_jacobian) { set_error("bbg_msm_device: null argument"); return BBG_E_INVALID; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    return msm_run(ctx, srs->s, d_scalars, from, n, d_out_jacobian, ctx->stream);
}

int bbg_msm_batch_device(bbg_ctx* ctx, bbg_srs* srs, size_t count, const void* const* d_scalars, const size_t* from, const size_t* n,
                         void* d_out_jacobians)
{
    CHECK_CTX(ctx);
    if (!srs || !d_scalars || !n || !d_out_jacobians) { set_error("bbg_msm_batch_device: null argument"); return BBG_E_INVALID; }
    if (count < 1 || count > BBG_MSM_BATCH_MAX) { set_error("bbg_msm_batch_device: 1 .. BBG_MSM_BATCH_MAX MSMs per batch"); return BBG_E_INVALID; }
    size_t zero[BBG_MSM_BATCH_MAX] = { 0 };
    std::lock_guard<std::mutex> lk(ctx->mu);
    return msm_run_batch(ctx, srs->s, (int)count, d_scalars, from ? from : zero, n, d_out_jacobians, ctx->stream);
}

int bbg_msm_batch(bbg_ctx* ctx, bbg_srs* srs, size_t count, const uint64_t* const* scalars, const size_t* from, const size_t* n, uint64_t* out_jacobians)
{
    CHECK_CTX(ctx);
    if (!srs || !scalars || !n || !out_jacobians) { set_error("bbg_msm_batch: null argument"); return BBG_E_INVALID; }
    if (count < 1 || count > BBG_MSM_BATCH_MAX) { set_error("bbg_msm_batch: 1 .. BBG_MSM_BATCH_MAX MSMs per batch"); return BBG_E_INVALID; }
    size_t zero[BBG_MSM_BATCH_MAX] = { 0 };
    for (size_t k = 0; k < count; k++)
        if (n[k] && !scalars[k]) { set_error("bbg_msm_batch: null scalars"); return BBG_E_INVALID; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    Staged st(ctx, "bbg_msm_batch");
    const auto d_results = st.region(1024); // count x 96 B <= 768 B
    Staged::Region d_scalars[BBG_MSM_BATCH_MAX];
    for (size_t k = 0; k < count; k++) d_scalars[k] = st.region(n[k], 32);
    BBG_TRY(st.ensure());
    const void* d_ptrs[BBG_MSM_BATCH_MAX];
    for (size_t k = 0; k < count; k++) {
        d_ptrs[k] = st[d_scalars[k]];
        if (n[k]) BBG_TRY(st.up(d_scalars[k], scalars[k], n[k] * 32));
    }
    BBG_TRY(msm_run_batch(ctx, srs->s, (int)count, d_ptrs, from ? from : zero, n, st[d_results], ctx->stream));
    BBG_TRY(msm_join(ctx, ctx->stream));
    BBG_TRY(st.down(out_jacobians, d_results, count * 96));
    return st.wait();
}

int bbg_msm_plan(bbg_ctx* ctx, const bbg_srs* srs, size_t n, int* window_bits, int* windows)
{
    CHECK_CTX(ctx);
    if (!window_bits || !windows) { set_error("bbg_msm_plan: null out"); return BBG_E_INVALID; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    int c = 0;
    int rc = msm_plan(ctx, srs ? &srs->s : nullptr, n, &c);
    if (rc) return rc;
    *window_bits = c;
    *windows = msm_windows_for(c);
    return BBG_OK;
}

int bbg_msm(bbg_ctx* ctx, bbg_srs* srs, const uint64_t* scalars, size_t from, size_t n, uint64_t out_jacobian[12])
{
    CHECK_CTX(ctx);
    if (!srs || (!scalars && n) || !out_jacobian) { set_error("bbg_msm: null argument"); return BBG_E_INVALID; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    Staged st(ctx, "bbg_msm");
    const auto d_result = st.region(256), d_scalars = st.region(n, 32);
    BBG_TRY(st.ensure());
    BBG_TRY(msm_run(ctx, srs->s, st[d_scalars], from, n, st[d_result], ctx->stream, scalars)); // uploads the scalars itself, in pieces, under its first pass
    BBG_TRY(msm_join(ctx, ctx->stream));
    BBG_TRY(st.down(out_jacobian, d_result, 96));
    return st.wait();
}

int bbg_g1_sum(bbg_ctx* ctx, const uint64_t* jacobians, size_t n, uint64_t out_jacobian[12])
{
    CHECK_CTX(ctx);
    if ((!jacobians && n) || !out_jacobian) { set_error("bbg_g1_sum: null argument"); return BBG_E_INVALID; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    Staged st(ctx, "bbg_g1_sum");
    const auto d_result = st.region(256), d_terms = st.region(n, 96);
    BBG_TRY(st.ensure());
    if (n) BBG_TRY(st.up(d_terms, jacobians, n * 96));
    BBG_TRY(g1_sum_device(ctx, st[d_terms], n, st[d_result], ctx->stream));
    BBG_TRY(st.down(out_jacobian, d_result, 96));
    return st.wait();
}

int bbg_g1_sum_device(bbg_ctx* ctx, const void* d_jacobians, size_t n, void* d_out_jacobian)
{
    CHECK_CTX(ctx);
    if ((!d_jacobians && n) || !d_out_jacobian) { set_error("bbg_g1_sum_device: null argument"); return BBG_E_INVALID; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    return g1_sum_device(ctx, d_jacobians, n, d_out_jacobian, ctx->stream);
}

int bbg_g1_normalize(bbg_ctx* ctx, const uint64_t* jacobians, size_t n, uint64_t* out_affine)
{
    CHECK_CTX(ctx);
    if ((!jacobians || !out_affine) && n) { set_error("bbg_g1_normalize: null argument"); return BBG_E_INVALID; }
    if (n == 0) return BBG_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    Staged st(ctx, "bbg_g1_normalize");
    const auto d_jacs = st.region(n, 96), d_affine = st.region(n, 64);
    BBG_TRY(st.ensure());
    BBG_TRY(st.up(d_jacs, jacobians, n * 96));
    BBG_TRY(g1_normalize_device(st[d_jacs], n, st[d_affine], ctx->stream));
    BBG_TRY(st.down(out_affine, d_affine, n * 64));
    return st.wait();
}

int bbg_g1_fixed_base_mul_device(bbg_ctx* ctx, const uint64_t* base_affine, const void* d_scalars, size_t n, void* d_out_affine)
{
    CHECK_CTX(ctx);
    if ((!d_scalars || !d_out_affine) && n) { set_error("bbg_g1_fixed_base_mul_device: null argument"); return BBG_E_INVALID; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    return fixed_base_mul(ctx, base_affine, d_scalars, n, d_out_affine, ctx->stream);
}

int bbg_g1_fixed_base_mul(bbg_ctx* ctx, const uint64_t* base_affine, const uint64_t* scalars, size_t n, uint64_t* out_affine)
{
    CHECK_CTX(ctx);
    if ((!scalars || !out_affine) && n) { set_error("bbg_g1_fixed_base_mul: null argument"); return BBG_E_INVALID; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    Staged st(ctx, "bbg_g1_fixed_base_mul");
    const auto d_scalars = st.region(n, 32), d_results = st.region(n + 1, 64); // one point of slack behind the results
    BBG_TRY(st.ensure());
    if (n) BBG_TRY(st.up(d_scalars, scalars, n * 32));
    const int rc = fixed_base_mul(ctx, base_affine, st[d_scalars], n, st[d_results], ctx->stream); // validates the base for n = 0 as well
    if (rc || n == 0) return rc;
    BBG_TRY(st.down(out_affine, d_results, n * 64));
    return st.wait();
}

int bbg_g1_batch_mul_device(bbg_ctx* ctx, const void* d_points_affine, const void* d_scalars, size_t n, int one_scalar, void* d_out_affine)
{
    CHECK_CTX(ctx);
    if ((!d_points_affine || !d_scalars || !d_out_affine) && n) { set_error("bbg_g1_batch_mul_device: null argument"); return BBG_E_INVALID; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    return var_base_mul(ctx, d_points_affine, d_scalars, n, one_scalar, d_out_affine, ctx->stream);
}

int bbg_g1_batch_mul(bbg_ctx* ctx, const uint64_t* points_affine, const uint64_t* scalars, size_t n, int one_scalar, uint64_t* out_affine)
{
    CHECK_CTX(ctx);
    if ((!points_affine || !scalars || !out_affine) && n) { set_error("bbg_g1_batch_mul: null argument"); return BBG_E_INVALID; }
    if (n == 0) return BBG_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const size_t ns = one_scalar ? 1 : n;
    Staged st(ctx, "bbg_g1_batch_mul");
    const auto d_points = st.region(n, 64), d_scalars = st.region(ns, 32); // the points are multiplied in place
    BBG_TRY(st.ensure());
    BBG_TRY(st.up(d_points, points_affine, n * 64));
    BBG_TRY(st.up(d_scalars, scalars, ns * 32));
    BBG_TRY(var_base_mul(ctx, st[d_points], st[d_scalars], n, one_scalar, st[d_points], ctx->stream));
    BBG_TRY(st.down(out_affine, d_points, n * 64));
    return st.wait();
}

int bbg_g1_msm_plan(size_t n, int window_bits, int* c, int* windows, size_t* chunk_terms, size_t* segment_entries)
{
    return msm_points_plan(n, window_bits, c, windows, chunk_terms, segment_entries);
}

int bbg_g1_msm_device(bbg_ctx* ctx, const void* d_points_affine, const void* d_scalars, size_t n, int window_bits, void* d_out_affine)
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return msm_points_run(ctx, d_points_affine, d_scalars, n, window_bits, d_out_affine, ctx->stream);
}

int bbg_g1_msm(bbg_ctx* ctx, const uint64_t* points_affine, const uint64_t* scalars, size_t n, int window_bits, uint64_t out_affine[8])
{
    CHECK_CTX(ctx);
    if (!out_affine || (n && (!points_affine || !scalars))) { set_error("bbg_g1_msm: null argument"); return BBG_E_INVALID; }
    if (int rc = msm_points_plan(n, window_bits, nullptr, nullptr, nullptr, nullptr)) return rc; // before the staging buffer is sized by n
    std::lock_guard<std::mutex> lk(ctx->mu);
    Staged st(ctx, "bbg_g1_msm");
    const auto d_result = st.region(64), d_points = st.region(n, 64), d_scalars = st.region(n, 32);
    BBG_TRY(st.ensure());
    if (n) {
        BBG_TRY(st.up(d_points, points_affine, n * 64));
        BBG_TRY(st.up(d_scalars, scalars, n * 32));
    }
    BBG_TRY(msm_points_run(ctx, st[d_points], st[d_scalars], n, window_bits, st[d_result], ctx->stream));
    BBG_TRY(st.down(out_affine, d_result, 64));
    return st.wait();
}

// ------------------------------------------------------------------------------------------------ G2 and the pairing (pairing.hip)
int bbg_g2_mul(bbg_ctx* ctx, const uint64_t* base_affine, const uint64_t* scalars, size_t n, uint64_t* out_affine)
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return g2_mul_host(ctx, base_affine, scalars, n, out_affine);
}

int bbg_g2_lines_prepare(bbg_ctx* ctx, const uint64_t* g2_affine, size_t pairs, bbg_g2_lines** out)
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return g2_lines_prepare(ctx, g2_affine, pairs, out);
}

int bbg_g2_lines_pairs(const bbg_g2_lines* lines, size_t* pairs)
{
    if (!lines || !pairs) { set_error("bbg_g2_lines_pairs: null argument"); return BBG_E_INVALID; }
    *pairs = lines->pairs;
    return BBG_OK;
}

int bbg_g2_lines_read(const bbg_g2_lines* lines, size_t which, uint64_t* out) { return g2_lines_read(lines, which, out); }

void bbg_g2_lines_free(bbg_g2_lines* lines) { g2_lines_release(lines); }

int bbg_pairing_product_device(bbg_ctx* ctx, const bbg_g2_lines* lines, const void* d_g1_affine, size_t count, void* d_out_fq12, void* d_status)
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return pairing_product_run(ctx, lines, d_g1_affine, count, d_out_fq12, d_status, ctx->stream);
}

// the host form of either pairing product: `run` is the module's device call (pairing_product_run: one lane per product; pairing_wave_run: one wave)
using PairingRun = int (*)(bbg_ctx*, const bbg_g2_lines*, const void*, size_t, void*, void*, hipStream_t);
static int pairing_product_host(const char* who, PairingRun run, bbg_ctx* ctx, const bbg_g2_lines* lines, const uint64_t* g1_affine, size_t count, uint64_t* out_fq12,
                                uint32_t* status)
{
    CHECK_CTX(ctx);
    if (int rc = pairing_product_check(who, ctx, lines, g1_affine, count, out_fq12, status)) return rc; // before the staging buffer is sized by count
    std::lock_guard<std::mutex> lk(ctx->mu);
    const size_t in_bytes = count * lines->pairs * 64;
    Staged st(ctx, who);
    const auto d_values = st.region(count, 384), d_points = st.region(in_bytes), d_flags = st.region(count, 4);
    BBG_TRY(st.ensure());
    BBG_TRY(st.up(d_points, g1_affine, in_bytes));
    BBG_TRY(run(ctx, lines, st[d_points], count, st[d_values], st[d_flags], ctx->stream));
    std::vector<uint32_t> flags(count);
    BBG_TRY(st.down(flags.data(), d_flags, count * 4));
    if (out_fq12) BBG_TRY(st.down(out_fq12, d_values, count * 384));
    BBG_TRY(st.wait());
    if (status) memcpy(status, flags.data(), count * 4);
    const size_t off_curve = (size_t)std::count(flags.begin(), flags.end(), 2u);
    if (off_curve) {
        set_error(std::string(who) + ": " + std::to_string(off_curve) + " of the products have a G1 point that is not on the curve");
        return BBG_E_INVALID;
    }
    return BBG_OK;
}

int bbg_pairing_product(bbg_ctx* ctx, const bbg_g2_lines* lines, const uint64_t* g1_affine, size_t count, uint64_t* out_fq12, uint32_t* status)
{
    return pairing_product_host("bbg_pairing_product", pairing_product_run, ctx, lines, g1_affine, count, out_fq12, status);
}

int bbg_pairing_product_wave_device(bbg_ctx* ctx, const bbg_g2_lines* lines, const void* d_g1_affine, size_t count, void* d_out_fq12, void* d_status)
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return pairing_wave_run(ctx, lines, d_g1_affine, count, d_out_fq12, d_status, ctx->stream);
}

int bbg_pairing_product_wave(bbg_ctx* ctx, const bbg_g2_lines* lines, const uint64_t* g1_affine, size_t count, uint64_t* out_fq12, uint32_t* status)
{
    return pairing_product_host("bbg_pairing_product_wave", pairing_wave_run, ctx, lines, g1_affine, count, out_fq12, status);
}

// ------------------------------------------------------------------------------------------------ NTT
int bbg_ntt_prepare(bbg_ctx* ctx, unsigned log2n)
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return ntt_prepare(ctx, log2n);
}

int bbg_ntt_plan(bbg_ctx* ctx, unsigned log2n, int* passes, int log_radix[4], int* kernel, int* tile_log)
{
    CHECK_CTX(ctx);
    if (!passes || !log_radix || !kernel || !tile_log) { set_error("bbg_ntt_plan: null out"); return BBG_E_INVALID; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    return ntt_plan(ctx, log2n, passes, log_radix, kernel, tile_log);
}

int bbg_ntt_device(bbg_ctx* ctx, void* d_coeffs, unsigned log2n, int op, size_t generator_size, const uint64_t* constant)
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return ntt_run(ctx, d_coeffs, log2n, op, generator_size, constant, ctx->stream);
}

int bbg_ntt(bbg_ctx* ctx, uint64_t* coeffs, unsigned log2n, int op, size_t generator_size, const uint64_t* constant)
{
    CHECK_CTX(ctx);
    if (!coeffs) { set_error("bbg_ntt: null coeffs"); return BBG_E_INVALID; }
    if (log2n > 28) { set_error("bbg_ntt: log2n > 28 exceeds the 2-adicity of BN254 Fr (fr.hpp:27-30)"); return BBG_E_INVALID; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    const size_t bytes = ((size_t)1 << log2n) * 32;
    Staged st(ctx, "bbg_ntt");
    const auto d_coeffs = st.region(bytes); // transformed in place
    BBG_TRY(st.ensure());
    BBG_TRY(st.up(d_coeffs, coeffs, bytes));
    BBG_TRY(ntt_run(ctx, st[d_coeffs], log2n, op, generator_size, constant, ctx->stream));
    BBG_TRY(st.down(coeffs, d_coeffs, bytes));
    return st.wait();
}

int bbg_scale_powers_device(bbg_ctx* ctx, void* d_a, size_t count, const uint64_t* start, const uint64_t* base)
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return ntt_scale_powers(ctx, d_a, count, start, base, ctx->stream);
}
int bbg_fr_root_pow(bbg_ctx* ctx, unsigned log2n, uint64_t e, int inverse, uint64_t out[4])
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return ntt_root_pow(ctx, log2n, e, inverse, out, ctx->stream);
}
int bbg_fr_pow(bbg_ctx* ctx, const uint64_t base[4], uint64_t e, uint64_t out[4])
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return ntt_fr_pow(ctx, base, e, out, ctx->stream);
}
int bbg_cross_dft_device(bbg_ctx* ctx, const void* d_in, void* d_out, unsigned log2G, size_t len, unsigned log2n, int inverse)
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return ntt_cross_dft(ctx, d_in, d_out, log2G, len, log2n, inverse, ctx->stream);
}

int bbg_coset_fft_split_device(bbg_ctx* ctx, void* d_coeffs, unsigned log2n, size_t ext)
{
    CHECK_CTX(ctx);
    if (!d_coeffs) { set_error("bbg_coset_fft_split: null coeffs"); return BBG_E_INVALID; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    return ntt_coset_split(ctx, d_coeffs, log2n, ext, ctx->stream);
}

int bbg_poly_linear_combination_device(bbg_ctx* ctx, const void* const* d_polys, const uint64_t* scalars, size_t count, const void* d_base,
                                       void* d_out, size_t n)
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return poly_lincomb(ctx, d_polys, scalars, count, d_base, d_out, n, ctx->stream);
}

int bbg_permutation_grand_product_device(bbg_ctx* ctx, const void* const d_wires[4], const void* const d_sigmas[4], unsigned log2n,
                                         const uint64_t* challenges, void* d_z)
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return permutation_grand_product(ctx, d_wires, d_sigmas, log2n, challenges, d_z, ctx->stream);
}

int bbg_quotient_widget_device(bbg_ctx* ctx, int widget, const void* const d_polys[BBG_QP_COUNT], unsigned log2_large_domain,
                               const uint64_t* challenges, void* d_quotient, uint64_t* alpha_base_out)
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return quotient_widget(ctx, widget, d_polys, log2_large_domain, challenges, d_quotient, alpha_base_out, ctx->stream);
}

int bbg_coset_fft_extend(bbg_ctx* ctx, const uint64_t* coeffs, unsigned log2n, unsigned log2_domain, uint64_t* out)
{
    CHECK_CTX(ctx);
    if (!coeffs || !out) { set_error("bbg_coset_fft_extend: null argument"); return BBG_E_INVALID; }
    if (log2_domain > 28 || log2_domain < 2 || log2n > log2_domain) {
        set_error("bbg_coset_fft_extend: need log2n <= log2_domain and 2 <= log2_domain <= 28");
        return BBG_E_INVALID;
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    const size_t n = (size_t)1 << log2n, m = (size_t)1 << log2_domain;
    Staged st(ctx, "bbg_coset_fft_extend");
    const auto d_result = st.region(m, 32), d_coeffs = st.region(n, 32); // the transform reads the coefficients zero-extended and writes the result area
    BBG_TRY(st.ensure());
    BBG_TRY(st.up(d_coeffs, coeffs, n * 32));
    BBG_TRY(ntt_coset_extend(ctx, st[d_coeffs], n, st[d_result], log2_domain, ctx->stream));
    BBG_TRY(st.down(out, d_result, m * 32));
    BBG_TRY(st.wait());
    memcpy(out + m * 4, out, 4 * 32); // add_lagrange_base_coefficient(out[0..3])
    return BBG_OK;
}

int bbg_coset_fft_split(bbg_ctx* ctx, uint64_t* coeffs, unsigned log2n, size_t ext)
{
    CHECK_CTX(ctx);
    if (!coeffs) { set_error("bbg_coset_fft_split: null coeffs"); return BBG_E_INVALID; }
    if (ext == 0 || log2n > 28 || ext > ((size_t)1 << 28)) { set_error("bbg_coset_fft_split: bad size"); return BBG_E_INVALID; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    const size_t n = (size_t)1 << log2n;
    Staged st(ctx, "bbg_coset_fft_split");
    const auto d_coeffs = st.region(n * ext, 32); // n coefficients in, n * ext values out, in place
    BBG_TRY(st.ensure());
    BBG_TRY(st.up(d_coeffs, coeffs, n * 32));
    BBG_TRY(ntt_coset_split(ctx, st[d_coeffs], log2n, ext, ctx->stream));
    BBG_TRY(st.down(coeffs, d_coeffs, n * ext * 32));
    return st.wait();
}

// ------------------------------------------------------------------------------------------------ polynomial helpers
int bbg_poly_op_device(bbg_ctx* ctx, int op, const void* d_a, const void* d_b, void* d_r, size_t n)
{
    CHECK_CTX(ctx);
    if ((!d_a || !d_b || !d_r) && n) { set_error("bbg_poly_op_device: null argument"); return BBG_E_INVALID; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    return poly_binop(op, d_a, d_b, d_r, n, ctx->stream);
}
int bbg_poly_evaluate_device(bbg_ctx* ctx, const void* d_coeffs, size_t n, const uint64_t z[4], uint64_t out[4])
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return poly_evaluate(ctx, d_coeffs, n, z, out, ctx->stream);
}
int bbg_kate_opening_device(bbg_ctx* ctx, const void* d_src, void* d_dest, size_t n, const uint64_t z[4], uint64_t f_out[4])
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return poly_kate_opening(ctx, d_src, d_dest, n, z, f_out, ctx->stream);
}
int bbg_poly_evaluate(bbg_ctx* ctx, const uint64_t* coeffs, size_t n, const uint64_t z[4], uint64_t out[4])
{
    CHECK_CTX(ctx);
    if ((!coeffs && n) || !z || !out) { set_error("bbg_poly_evaluate: null argument"); return BBG_E_INVALID; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    Staged st(ctx, "bbg_poly_evaluate");
    const auto d_coeffs = st.region(n + 1, 32); // one element of slack
    BBG_TRY(st.ensure());
    if (n) BBG_TRY(st.up(d_coeffs, coeffs, n * 32));
    return poly_evaluate(ctx, st[d_coeffs], n, z, out, ctx->stream); // downloads the value and waits itself
}
int bbg_kate_opening(bbg_ctx* ctx, const uint64_t* src, uint64_t* dest, size_t n, const uint64_t z[4], uint64_t f_out[4])
{
    CHECK_CTX(ctx);
    if ((n && (!src || !dest)) || !z || !f_out) { set_error("bbg_kate_opening: null argument"); return BBG_E_INVALID; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    Staged st(ctx, "bbg_kate_opening");
    const auto d_src = st.region(n + 1, 32), d_dest = st.region(n + 1, 32); // one element of slack behind each
    BBG_TRY(st.ensure());
    if (n) BBG_TRY(st.up(d_src, src, n * 32));
    BBG_TRY(poly_kate_opening(ctx, st[d_src], st[d_dest], n, z, f_out, ctx->stream));
    if (n) BBG_TRY(st.down(dest, d_dest, n * 32));
    return st.wait();
}
int bbg_fr_batch_invert_device(bbg_ctx* ctx, const void* d_in, void* d_out, size_t n)
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return poly_batch_invert(ctx, d_in, d_out, n, ctx->stream);
}
int bbg_poly_evaluate_lagrange_device(bbg_ctx* ctx, const void* const* d_evals, const int* shifted, size_t count, unsigned log2n, const uint64_t z[4],
                                      uint64_t* out)
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return poly_evaluate_lagrange(ctx, d_evals, shifted, count, log2n, z, out, ctx->stream);
}
int bbg_poly_evaluate_lagrange(bbg_ctx* ctx, const uint64_t* evals, unsigned log2n, const uint64_t z[4], uint64_t out[4])
{
    CHECK_CTX(ctx);
    if (!evals || !z || !out || log2n == 0 || log2n > 28) { set_error("bbg_poly_evaluate_lagrange: bad argument (1 <= log2n <= 28)"); return BBG_E_INVALID; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    Staged st(ctx, "bbg_poly_evaluate_lagrange");
    const auto d_values = st.region((size_t)32 << log2n);
    BBG_TRY(st.ensure());
    BBG_TRY(st.up(d_values, evals, (size_t)32 << log2n));
    const void* d_evals = st[d_values];
    return poly_evaluate_lagrange(ctx, &d_evals, nullptr, 1, log2n, z, out, ctx->stream); // downloads the value and waits itself
}
int bbg_kate_opening_lagrange_device(bbg_ctx* ctx, const void* d_evals, void* d_dest, unsigned log2n, const uint64_t z[4], uint64_t f_out[4])
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return poly_kate_opening_lagrange(ctx, d_evals, d_dest, log2n, z, f_out, ctx->stream);
}

// ------------------------------------------------------------------------------------------------ many openings, each at its own point (open_points.hip)
int bbg_open_points_set_budget(bbg_ctx* ctx, size_t bytes)
{
    CHECK_CTX(ctx);
    if (bytes > ((size_t)1 << 36)) { set_error("bbg_open_points_set_budget: at most 2^36 bytes"); return BBG_E_INVALID; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->open_points_budget = bytes ? (long)bytes : 1L << 30;
    return BBG_OK;
}

int bbg_open_points_device(bbg_ctx* ctx, bbg_srs* lagrange, unsigned log2n, const void* d_evals, const void* d_z, size_t count, void* d_y, void* d_proofs)
{
    CHECK_CTX(ctx);
    BBG_TRY(open_points_check("bbg_open_points_device", ctx, lagrange, log2n, d_evals, d_z, count, d_y, d_proofs));
    std::lock_guard<std::mutex> lk(ctx->mu);
    return open_points_run(ctx, lagrange, log2n, d_evals, d_z, count, d_y, d_proofs, ctx->stream);
}

int bbg_open_points(bbg_ctx* ctx, bbg_srs* lagrange, unsigned log2n, const uint64_t* evals, const uint64_t* z, size_t count, uint64_t* y, uint64_t* proofs)
{
    CHECK_CTX(ctx);
    BBG_TRY(open_points_check("bbg_open_points", ctx, lagrange, log2n, evals, z, count, y, proofs)); // before the staging buffer is sized by count
    std::lock_guard<std::mutex> lk(ctx->mu);
    const size_t evals_bytes = (count * 32) << log2n;
    Staged st(ctx, "bbg_open_points");
    const auto d_evals = st.region(evals_bytes), d_z = st.region(count, 32), d_y = st.region(count, 32), d_proofs = st.region(proofs ? count : 0, 64);
    BBG_TRY(st.ensure());
    BBG_TRY(st.up(d_evals, evals, evals_bytes));
    BBG_TRY(st.up(d_z, z, count * 32));
    BBG_TRY(open_points_run(ctx, lagrange, log2n, st[d_evals], st[d_z], count, st[d_y], proofs ? st[d_proofs] : nullptr, ctx->stream));
    BBG_TRY(st.down(y, d_y, count * 32));
    if (proofs) BBG_TRY(st.down(proofs, d_proofs, count * 64));
    return st.wait();
}

// ------------------------------------------------------------------------------------------------ openings at arbitrary points to one pairing check (kzg_verify.hip)
int bbg_kzg_verify_reduce_device(bbg_ctx* ctx, const void* d_commitments, const void* d_z, const void* d_y, const void* d_proofs, size_t N, const uint64_t rho[4],
                                 void* d_out, void* d_off_curve)
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return kzg_verify_reduce(ctx, d_commitments, d_z, d_y, d_proofs, N, rho, d_out, d_off_curve, ctx->stream);
}

int bbg_kzg_verify_reduce(bbg_ctx* ctx, const uint64_t* commitments, const uint64_t* z, const uint64_t* y, const uint64_t* proofs, size_t N, const uint64_t rho[4],
                          uint64_t out[16])
{
    CHECK_CTX(ctx);
    BBG_TRY(kzg_verify_check("bbg_kzg_verify_reduce", commitments, z, y, proofs, N, rho, out)); // before the staging buffer is sized by N
    std::lock_guard<std::mutex> lk(ctx->mu);
    Staged st(ctx, "bbg_kzg_verify_reduce");
    const auto d_com = st.region(N, 64), d_proofs = st.region(N, 64), d_z = st.region(N, 32), d_y = st.region(N, 32);
    const auto d_res = st.region(256); // L, R (128 B), then the off-curve count: one block, one download
    BBG_TRY(st.ensure());
    BBG_TRY(st.up(d_com, commitments, N * 64));
    BBG_TRY(st.up(d_proofs, proofs, N * 64));
    BBG_TRY(st.up(d_z, z, N * 32));
    BBG_TRY(st.up(d_y, y, N * 32));
    BBG_TRY(kzg_verify_reduce(ctx, st[d_com], st[d_z], st[d_y], st[d_proofs], N, rho, st[d_res], st[d_res] + 128, ctx->stream));
    uint64_t res[18]; // L, R, then the count in the low word of res[16]
    BBG_TRY(st.down(res, d_res, 128 + 4));
    BBG_TRY(st.wait());
    uint32_t off_curve = 0;
    memcpy(&off_curve, res + 16, 4);
    if (off_curve) {
        set_error("bbg_kzg_verify_reduce: " + std::to_string(off_curve) + " of the commitments and proofs are not on the curve");
        return BBG_E_INVALID;
    }
    memcpy(out, res, 128);
    return BBG_OK;
}

int bbg_kzg_verify_device(bbg_ctx* ctx, const bbg_g2_lines* lines, const void* d_commitments, const void* d_z, const void* d_y, const void* d_proofs, size_t N,
                          const uint64_t rho[4], void* d_status)
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return kzg_verify_run(ctx, lines, d_commitments, d_z, d_y, d_proofs, N, rho, d_status, ctx->stream);
}

int bbg_kzg_verify(bbg_ctx* ctx, const bbg_g2_lines* lines, const uint64_t* commitments, const uint64_t* z, const uint64_t* y, const uint64_t* proofs, size_t N,
                   const uint64_t rho[4], uint32_t* status)
{
    CHECK_CTX(ctx);
    if (!lines) { set_error("bbg_kzg_verify: null argument"); return BBG_E_INVALID; }
    BBG_TRY(kzg_verify_check("bbg_kzg_verify", commitments, z, y, proofs, N, rho, status)); // before the staging buffer is sized by N
    std::lock_guard<std::mutex> lk(ctx->mu);
    Staged st(ctx, "bbg_kzg_verify");
    const auto d_com = st.region(N, 64), d_proofs = st.region(N, 64), d_z = st.region(N, 32), d_y = st.region(N, 32), d_status = st.region(4);
    BBG_TRY(st.ensure());
    BBG_TRY(st.up(d_com, commitments, N * 64));
    BBG_TRY(st.up(d_proofs, proofs, N * 64));
    BBG_TRY(st.up(d_z, z, N * 32));
    BBG_TRY(st.up(d_y, y, N * 32));
    BBG_TRY(kzg_verify_run(ctx, lines, st[d_com], st[d_z], st[d_y], st[d_proofs], N, rho, st[d_status], ctx->stream));
    uint32_t word = 0;
    BBG_TRY(st.down(&word, d_status, 4));
    BBG_TRY(st.wait());
    *status = word;
    if (word == 2) {
        set_error("bbg_kzg_verify: a commitment or a proof is not on the curve");
        return BBG_E_INVALID;
    }
    return BBG_OK;
}

// ------------------------------------------------------------------------------------------------ wire forms of G1 points and scalars (wire.hip)
int bbg_wire_sizes(int form, size_t* wire_bytes, size_t* native_bytes)
{
    const int rc = wire_sizes(form, wire_bytes, native_bytes);
    if (rc) set_error("bbg_wire_sizes: unknown form");
    return rc;
}

int bbg_wire_decode_device(bbg_ctx* ctx, int form, const void* d_wire, size_t n, void* d_native, void* d_status, void* d_bad)
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return wire_decode_run(ctx, "bbg_wire_decode_device", form, d_wire, n, d_native, d_status, d_bad, ctx->stream);
}

int bbg_wire_encode_device(bbg_ctx* ctx, int form, const void* d_native, size_t n, int check, void* d_wire, void* d_status, void* d_bad)
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return wire_encode_run(ctx, "bbg_wire_encode_device", form, d_native, n, check, d_wire, d_status, d_bad, ctx->stream);
}

// the host twin of both directions: `in` (in_each bytes per element) up, the device call, `out`, the status words and the count down
static int wire_staged(bbg_ctx* ctx, const char* who, bool encode, int form, int check, const void* in, size_t n, void* out, uint32_t* status, uint32_t* bad)
{
    size_t wire_bytes = 0, native_bytes = 0;
    (void)wire_sizes(form, &wire_bytes, &native_bytes); // an unknown form is wire_check's to report
    const size_t in_each = encode ? native_bytes : wire_bytes, out_each = encode ? wire_bytes : native_bytes;
    BBG_TRY(wire_check(who, form, check, n, in, in_each, out, out_each, status, bad)); // before the staging buffer is sized by n
    std::lock_guard<std::mutex> lk(ctx->mu);
    Staged st(ctx, who);
    const auto d_in = st.region(n, in_each), d_out = st.region(n, out_each), d_status = st.region(n, 4), d_bad = st.region(4);
    BBG_TRY(st.ensure());
    if (n) BBG_TRY(st.up(d_in, in, n * in_each));
    if (encode) BBG_TRY(wire_encode_run(ctx, who, form, st[d_in], n, check, st[d_out], st[d_status], st[d_bad], ctx->stream));
    else BBG_TRY(wire_decode_run(ctx, who, form, st[d_in], n, st[d_out], st[d_status], st[d_bad], ctx->stream));
    uint32_t count = 0;
    if (n) BBG_TRY(st.down(out, d_out, n * out_each));
    if (n && status) BBG_TRY(st.down(status, d_status, n * 4));
    BBG_TRY(st.down(&count, d_bad, 4));
    BBG_TRY(st.wait());
    if (bad) *bad = count;
    if (count) {
        set_error(std::string(who) + ": " + std::to_string(count) + " of the elements are malformed or not on the curve");
        return BBG_E_INVALID;
    }
    return BBG_OK;
}

int bbg_wire_decode(bbg_ctx* ctx, int form, const void* wire, size_t n, void* native, uint32_t* status, uint32_t* bad)
{
    CHECK_CTX(ctx);
    return wire_staged(ctx, "bbg_wire_decode", false, form, 0, wire, n, native, status, bad);
}

int bbg_wire_encode(bbg_ctx* ctx, int form, const void* native, size_t n, int check, void* wire, uint32_t* status, uint32_t* bad)
{
    CHECK_CTX(ctx);
    return wire_staged(ctx, "bbg_wire_encode", true, form, check, native, n, wire, status, bad);
}

int bbg_divide_by_pseudo_vanishing(bbg_ctx* ctx, uint64_t* evals, unsigned log2_src, unsigned log2_target, size_t num_roots_cut)
{
    CHECK_CTX(ctx);
    if (!evals) { set_error("bbg_divide_by_pseudo_vanishing: null argument"); return BBG_E_INVALID; }
    if (log2_target > 28) { set_error("bbg_divide_by_pseudo_vanishing: log2_target > 28"); return BBG_E_INVALID; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    const size_t bytes = ((size_t)1 << log2_target) * 32;
    Staged st(ctx, "bbg_divide_by_pseudo_vanishing");
    const auto d_evals = st.region(bytes); // divided in place
    BBG_TRY(st.ensure());
    BBG_TRY(st.up(d_evals, evals, bytes));
    BBG_TRY(poly_divide_pseudo_vanishing(ctx, st[d_evals], log2_src, log2_target, num_roots_cut, ctx->stream));
    BBG_TRY(st.down(evals, d_evals, bytes));
    return st.wait();
}
int bbg_divide_by_pseudo_vanishing_device(bbg_ctx* ctx, void* d_evals, unsigned log2_src, unsigned log2_target, size_t num_roots_cut)
{
    CHECK_CTX(ctx);
    std::lock_guard<std::mutex> lk(ctx->mu);
    return poly_divide_pseudo_vanishing(ctx, d_evals, log2_src, log2_target, num_roots_cut, ctx->stream);
}

int bbg_field_op(bbg_ctx* ctx, int which, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n)
{
    CHECK_CTX(ctx);
    if (!a || !out) { set_error("bbg_field_op: null argument"); return BBG_E_INVALID; }
    if (op == 12 && which != 1) { set_error("bbg_field_op: op 12 is the square root of Fq only (which = 1)"); return BBG_E_INVALID; }
    if (n == 0) return BBG_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    Staged st(ctx, "bbg_field_op");
    const auto d_a = st.region(n, 32), d_b = st.region(n, 32), d_out = st.region(n, 32);
    BBG_TRY(st.ensure());
    BBG_TRY(st.up(d_a, a, n * 32));
    if (b) BBG_TRY(st.up(d_b, b, n * 32));
    if (op == 12) BBG_TRY(wire_sqrt_device(st[d_a], st[d_out], n, ctx->stream));
    else BBG_TRY(field_op_device(which, op, st[d_a], b ? st[d_b] : nullptr, st[d_out], n, ctx->stream));
    BBG_TRY(st.down(out, d_out, n * 32));
    return st.wait();
}

int bbg_limb29_op_shape(int which, int op, int* operands, int* results)
{
    if (!operands || !results) { set_error("bbg_limb29_op_shape: null argument"); return BBG_E_INVALID; }
    const int rc = limb29_op_shape(which, op, operands, results);
    if (rc) set_error("bbg_limb29_op_shape: unknown (which, op)");
    return rc;
}
int bbg_limb29_op(bbg_ctx* ctx, int which, int op, const uint32_t* in, size_t n, uint32_t* out)
{
    CHECK_CTX(ctx);
    int operands = 0, results = 0;
    if (limb29_op_shape(which, op, &operands, &results)) { set_error("bbg_limb29_op: unknown (which, op)"); return BBG_E_INVALID; }
    if (n > ((size_t)1 << 20)) { set_error("bbg_limb29_op: n > 2^20"); return BBG_E_INVALID; }
    if (n == 0) return BBG_OK;
    if (!in || !out) { set_error("bbg_limb29_op: null argument"); return BBG_E_INVALID; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    const size_t in_bytes = n * operands * 36, out_bytes = n * results * 36; // rows of 9 words
    Staged st(ctx, "bbg_limb29_op");
    const auto d_in = st.region(in_bytes), d_out = st.region(out_bytes);
    BBG_TRY(st.ensure());
    BBG_TRY(st.up(d_in, in, in_bytes));
    BBG_TRY(limb29_op_device(which, op, st[d_in], st[d_out], n, ctx->stream));
    BBG_TRY(st.down(out, d_out, out_bytes));
    return st.wait();
}

int bbg_tower_op_shape(int op, int* operands, int* results)
{
    if (!operands || !results) { set_error("bbg_tower_op_shape: null argument"); return BBG_E_INVALID; }
    const int rc = tower_op_shape(op, operands, results);
    if (rc) set_error("bbg_tower_op_shape: unknown op");
    return rc;
}
int bbg_tower_op(bbg_ctx* ctx, int op, const uint32_t* in, size_t n, uint32_t* out)
{
    CHECK_CTX(ctx);
    int operands = 0, results = 0;
    if (tower_op_shape(op, &operands, &results)) { set_error("bbg_tower_op: unknown op"); return BBG_E_INVALID; }
    if (n > ((size_t)1 << 16)) { set_error("bbg_tower_op: n > 2^16"); return BBG_E_INVALID; }
    if (n == 0) return BBG_OK;
    if (!in || !out) { set_error("bbg_tower_op: null argument"); return BBG_E_INVALID; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    const size_t in_bytes = n * operands * 32, out_bytes = n * results * 32; // rows of 8 words
    Staged st(ctx, "bbg_tower_op");
    const auto d_in = st.region(in_bytes), d_out = st.region(out_bytes), d_work = st.region(tower_op_work_bytes(op, n));
    BBG_TRY(st.ensure());
    BBG_TRY(st.up(d_in, in, in_bytes));
    BBG_TRY(tower_op_device(op, st[d_in], st[d_out], st[d_work], n, ctx->stream));
    BBG_TRY(st.down(out, d_out, out_bytes));
    return st.wait();
}

} // extern "C"
