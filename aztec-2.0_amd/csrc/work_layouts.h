// The device working memory of the modules, one description each: a function that takes the call's shape and returns the byte offsets of
// the buffer's regions together with the RegionLayout that handed them out.  The module sizes its buffer from that layout (ensure_layout,
// bbg_internal.h) and binds every pointer to one of its offsets (at<T>), so a size and a pointer chain cannot drift apart.  The order of
// the regions and every total are part of the interface: include/bbg.h publishes several of the totals as formulas.
// Plain host C++ with no HIP in it: constants that live in a .hip file come in as arguments, and tests/tools/region_layout_check.cpp checks
// every function here over a grid of shapes (totals against the published formulas, regions inside, disjoint and aligned).
// Hand-carved buffers pack their regions (alignment 1) in descending element size: 128 B points (a Jacobian takes 96 B of a 128 B slot),
// 64 B affine points, 32 B field elements, words.
#pragma once
#include "region_layout.h"

#include <algorithm>

namespace bbg {

// ---------------------------------------------------------------------------------------------- cells_verify.hip, cells_verify_reduce
// the group lists of a call, built in the pinned host array and copied to the device in ONE copy: the same block on both sides
struct CvLists {
    size_t off_m, perm_m, off_c, perm_c; // off: groups + 1 words, perm: K words; m = by cell id (r groups), c = by commitment id (ncom)
    RegionLayout lay{ 4 };
};
static inline CvLists cv_lists(size_t r, size_t K, size_t ncom)
{
    CvLists l;
    l.off_m = l.lay.add(r + 1, 4);
    l.perm_m = l.lay.add(K, 4);
    l.off_c = l.lay.add(ncom + 1, 4);
    l.perm_c = l.lay.add(K, 4);
    return l;
}
struct CvLayout {
    size_t S;      // r points
    size_t Q;       // r + ncom points, ONE array that k_cv_reduce sums as a whole: Q (r), then ..
    size_t com_out; // .. its last ncom points, W_c C_c, which k_cv_mul writes
    size_t prod;    // K points
    size_t parts;  // 2 x `parts` partial sums
    size_t msm_a;  // [A]: a Jacobian in a 128 B slot
    size_t E;      // n values
    size_t pw;     // K values
    size_t W;      // ncom values
    size_t bad;    // the off-curve counter, 16 B
    size_t lists;  // the CvLists block
    CvLists in;
    RegionLayout lay{ 1 };
};
static inline CvLayout cv_layout(size_t n, size_t r, size_t K, size_t ncom, size_t parts /* CV_PARTS */)
{
    CvLayout l;
    l.in = cv_lists(r, K, ncom);
    l.S = l.lay.add(r, 128);
    l.Q = l.lay.add(r + ncom, 128);
    l.com_out = l.Q + r * 128;
    l.prod = l.lay.add(K, 128);
    l.parts = l.lay.add(2 * parts, 128);
    l.msm_a = l.lay.add(1, 128);
    l.E = l.lay.add(n, 32);
    l.pw = l.lay.add(K, 32);
    l.W = l.lay.add(ncom, 32);
    l.bad = l.lay.add(16);
    l.lists = l.lay.add(l.in.lay);
    return l;
}

// ---------------------------------------------------------------------------------------------- cells.hip, cells_recover
// slot map and id lists (missing ids, then the known ones), built in the pinned host array and copied in ONE copy
struct CrLists {
    size_t slot, lists; // r words each
    RegionLayout lay{ 4 };
};
struct CrLayout {
    size_t roots; // r values
    size_t pts;   // 2r values
    size_t z;     // 2r values: Zcos, then Zdom by slot
    size_t in_at; // the CrLists block
    CrLists in;
    RegionLayout lay{ 1 };
};
static inline CrLayout cr_layout(size_t r)
{
    CrLayout l;
    l.in.slot = l.in.lay.add(r, 4);
    l.in.lists = l.in.lay.add(r, 4);
    l.roots = l.lay.add(r, 32);
    l.pts = l.lay.add(2 * r, 32);
    l.z = l.lay.add(2 * r, 32);
    l.in_at = l.lay.add(l.in.lay);
    return l;
}

// ---------------------------------------------------------------------------------------------- kzg_verify.hip, kzg_verify_reduce
struct KvLayout {
    size_t points;   // 2N + 1 affine points, ONE array [C | pi | G]: the MSMs read the windows [0, 2N + 1) and [N, 2N)
    size_t scalars;  // 2N + 1 values, ONE array [rho^i | rho^i z_i | s]
    size_t pw;       // N values
    size_t partials; // `blocks` values
    size_t bad;      // the off-curve counter, 32 B
    RegionLayout lay{ 1 };
};
static inline KvLayout kv_layout(size_t N, size_t blocks /* KV_BLOCKS */)
{
    KvLayout l;
    l.points = l.lay.add(2 * N + 1, 64);
    l.scalars = l.lay.add(2 * N + 1, 32);
    l.pw = l.lay.add(N, 32);
    l.partials = l.lay.add(blocks, 32);
    l.bad = l.lay.add(32);
    return l;
}

// ---------------------------------------------------------------------------------------------- open_points.hip, one chunk of `chunk` polynomials
// include/bbg.h publishes (proofs ? 32 n : 0) + 64 ceil(n / bary_blk) + 160 bytes per polynomial, and the chunk is the budget divided by
// that figure: the five regions take 132 of the 160 bytes, the rest stays behind them as the last region
constexpr size_t OP_POLY_TAIL = 160, OP_POLY_SPARE = OP_POLY_TAIL - 32 - 96 - 4;
struct OpLayout {
    size_t u;        // proofs only: chunk x n values
    size_t partials; // chunk x groups x 2 values
    size_t hitq;     // chunk values
    size_t jac;      // chunk Jacobians, 96 B each
    size_t flag;     // chunk words
    RegionLayout lay{ 1 };
};
static inline OpLayout op_layout(unsigned log2n, bool proofs, size_t chunk, size_t bary_blk /* BARY_BLK */)
{
    const size_t n = (size_t)1 << log2n, groups = (n + bary_blk - 1) / bary_blk;
    OpLayout l;
    l.u = l.lay.add(proofs ? chunk : 0, n * 32);
    l.partials = l.lay.add(chunk, groups * 2 * 32);
    l.hitq = l.lay.add(chunk, 32);
    l.jac = l.lay.add(chunk, 96);
    l.flag = l.lay.add(chunk, 4);
    l.lay.add(chunk, OP_POLY_SPARE);
    return l;
}

// ---------------------------------------------------------------------------------------------- open_all.hip, the workspace of `cap` polynomials
// l = 2^log2cell, r = n / l; every array polynomial-major.  The inverse transforms work on `sum`, or on work2 where l = 1 and sum is empty.
struct OaLayout {
    size_t work2; // cap x 2n points: the 2n products of each polynomial
    size_t work1; // cap x r points: the forward transforms' arrays
    size_t sum;   // cap x 2r points, l >= 2 only: the summed products
    size_t c_hat; // cap x 2n values
    RegionLayout lay{ 1 };
};
static inline OaLayout oa_layout(size_t cap, unsigned log2n, unsigned log2cell)
{
    const size_t m = (size_t)2 << log2n, r = (size_t)1 << (log2n - log2cell);
    OaLayout l;
    l.work2 = l.lay.add(cap, m * 128);
    l.work1 = l.lay.add(cap, r * 128);
    l.sum = l.lay.add(log2cell ? cap : 0, 2 * r * 128);
    l.c_hat = l.lay.add(cap, m * 32);
    return l;
}

// ---------------------------------------------------------------------------------------------- pairing.hip, pairing_product_run
// stride = the products of one chunk rounded up to whole waves
struct PairLayout {
    size_t work;  // `slots` lane-interleaved Fq12 slots: stride x slots x 384 B
    size_t flags; // stride words
    RegionLayout lay{ 1 };
};
static inline PairLayout pair_layout(size_t stride, size_t slots /* PairP::FINAL_SLOTS */)
{
    PairLayout l;
    l.work = l.lay.add(stride, slots * 384);
    l.flags = l.lay.add(stride, 4);
    return l;
}

// ---------------------------------------------------------------------------------------------- msm_tiny.hip
// every region rounded up to 256 B, the last included; the per-block bucket sums once per reduce slot
template <int SLOTS> struct TinyLayout {
    size_t mags;         // sets x windows x n_pad digit bytes
    size_t signs;        // sets x n_pad sign words
    size_t parts[SLOTS]; // sets x buckets x slices points each
    RegionLayout lay{ 256 };
};
template <int SLOTS /* bbg_ctx::MSM_SLOTS */>
static inline TinyLayout<SLOTS> tiny_layout(size_t sets, size_t n_pad, size_t slices, size_t windows /* T_WINDOWS */, size_t buckets /* T_BUCKETS */)
{
    TinyLayout<SLOTS> l;
    l.mags = l.lay.add(sets * windows, n_pad);
    l.signs = l.lay.add(sets * n_pad, 4);
    for (int k = 0; k < SLOTS; k++) l.parts[k] = l.lay.add(sets * buckets * slices, 128);
    l.lay.close();
    return l;
}

// ---------------------------------------------------------------------------------------------- poly.hip, the context's polynomial scratch
struct PolyLayout {
    size_t header; // PolyHeader
    size_t part;   // partials + 2 values, 256 B aligned
    RegionLayout lay{ 256 };
};
static inline PolyLayout poly_layout(size_t header_bytes /* sizeof(PolyHeader) */, size_t partials)
{
    PolyLayout l;
    l.header = l.lay.add(header_bytes);
    l.part = l.lay.add(partials + 2, 32);
    return l;
}

// ---------------------------------------------------------------------------------------------- quotient.hip, the grand product's totals
struct GpLayout {
    size_t sd; // n values
    size_t bt; // 2 nblocks + 2 values
    RegionLayout lay{ 1 };
};
static inline GpLayout gp_layout(size_t n, size_t nblocks)
{
    GpLayout l;
    l.sd = l.lay.add(n, 32);
    l.bt = l.lay.add(2 * nblocks + 2, 32);
    return l;
}

// ---------------------------------------------------------------------------------------------- msm_points.hip: the plan of a call and one chunk's memory
constexpr int MP_C_MIN = 2, MP_C_MAX = 16;
constexpr size_t MP_MAX_N = (size_t)1 << 28;
constexpr size_t MP_BUDGET = (size_t)1 << 30;    // working memory of one call, as bbg_open_all_batch
constexpr size_t MP_CHUNK_CAP = (size_t)1 << 20; // terms per chunk at most
constexpr size_t MP_LANE_BUCKETS = 65536;        // from this many buckets a segment is one lane's, below it one wave's
constexpr size_t MP_SEG_LANE = 256, MP_SEG_WAVE = 1024;
constexpr int MP_GROUP_LOG = 5;                  // buckets per group of the reduction: 2^5 at most

struct MpPlan {
    int c = 0, windows = 0;
    size_t chunk_terms = 0, segment_entries = 0;
    bool lane = false;
    size_t buckets = 0;        // windows 2^(c-1); the dump key
    int group_log = 0;         // L = 2^group_log buckets per group
    size_t groups = 0;         // per window
    int lane_groups_log = 0;   // M = 2^lane_groups_log groups per lane of k_mp_reduce2
};

// the working memory of one chunk of T terms (bbg.h): every region rounded up to 128 B, the last included
struct MpLayout {
    size_t buckets, sg, tg, winsum, partial, counts, off, cursor, segoff, entries, sorted;
    RegionLayout lay{ 128 };
};

static inline int mp_windows(int c) { return (128 + c - 1) / c; }

// The automatic width: the fastest width of a sweep over every width at n = 2^8 .. 2^22 on an MI355X.  The cost model
// 2 n windows(c) + 4 windows(c) 2^(c-1) it replaced asked for wider windows below 2^18 terms than the fixed tail of the reduction pays for.
static inline int mp_auto_width(size_t n)
{
    if (n <= ((size_t)1 << 12)) return 4;
    if (n <= ((size_t)1 << 15)) return 8;
    if (n <= ((size_t)1 << 17)) return 9;
    return 16;
}

static inline size_t mp_max_segments(const MpPlan& p, size_t T)
{
    const size_t entries = 2 * (size_t)p.windows * T;
    return std::min(p.buckets, entries) + entries / p.segment_entries;
}

static inline MpLayout mp_layout(const MpPlan& p, size_t T)
{
    const size_t entries = 2 * (size_t)p.windows * T, bins = p.buckets + 1;
    MpLayout l;
    l.buckets = l.lay.add(p.buckets, 128);
    l.sg = l.lay.add((size_t)p.windows * p.groups, 128);
    l.tg = l.lay.add((size_t)p.windows * p.groups, 128);
    l.winsum = l.lay.add((size_t)p.windows, 128);
    l.partial = l.lay.add(mp_max_segments(p, T), 128);
    l.counts = l.lay.add(bins, 4);
    l.off = l.lay.add(bins + 1, 4);
    l.cursor = l.lay.add(bins, 4);
    l.segoff = l.lay.add(bins, 4);
    l.entries = l.lay.add(entries, 4);
    l.sorted = l.lay.add(entries, 4);
    l.lay.close();
    return l;
}

// false: window_bits is neither 0 nor a width of the range, or n is above the maximum
static inline bool mp_plan(size_t n, int window_bits, MpPlan* out)
{
    if (n > MP_MAX_N) return false;
    if (window_bits != 0 && (window_bits < MP_C_MIN || window_bits > MP_C_MAX)) return false;
    MpPlan p;
    p.c = window_bits ? window_bits : mp_auto_width(n);
    p.windows = mp_windows(p.c);
    p.buckets = (size_t)p.windows << (p.c - 1);
    p.lane = p.buckets >= MP_LANE_BUCKETS;
    p.segment_entries = p.lane ? MP_SEG_LANE : MP_SEG_WAVE;
    p.group_log = std::min(p.c - 1, MP_GROUP_LOG);
    p.groups = (size_t)1 << (p.c - 1 - p.group_log);
    p.lane_groups_log = 0;
    while (((size_t)64 << p.lane_groups_log) < p.groups) p.lane_groups_log++;
    size_t T = MP_CHUNK_CAP;
    while (mp_layout(p, T).lay.total() > MP_BUDGET) T -= T / 16; // a pure function of c: the first T of this sequence that fits
    p.chunk_terms = T;
    *out = p;
    return true;
}

} // namespace bbg
