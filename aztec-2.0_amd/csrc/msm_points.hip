// A multi-scalar multiplication over the CALLER'S points for gfx950: result = sum_i s_i P_i with no bbg_srs and no window tables
// (bbg_g1_msm).  Pippenger's bucket method without precomputation:
//
//   split     s -> (|k1|, |k2|, sign of k2), s = k1 - k2 lambda (glv_split_mag, var_base.hip.h): both halves below 2^127.
//   recode    each half into `windows` = ceil(128 / c) signed c-bit digits with carry, |d| <= 2^(c-1): v = (h >> c w) mod 2^c + carry,
//             d = v - 2^c and carry 1 where v > 2^(c-1).  h < 2^(c windows - 1) keeps the top window at most 2^(c-1) - 1, so the last carry
//             is 0.  A non-zero digit is one ENTRY: key = w 2^(c-1) + |d| - 1 (its bucket), payload = sign | twin | term index in the chunk.
//             The twin bit (second half) selects lambda P = (beta x, y): one Fq product where the point is loaded.  Both halves share the
//             buckets; the sign of a twin entry carries the minus of k1 - k2 lambda.  A zero digit, and every digit of an infinite point,
//             goes to the dump key `buckets` and is dropped by the scatter.
//   sort      a counting sort of the chunk's entries by key: histogram (k_mp_recode), one scan (k_mp_scan), scatter (k_mp_scatter).  The
//             atomics are plain vector atomicAdd on uint32_t, aggregated over equal keys of a wave (wave_agg_add).
//   buckets   a bucket's entries are cut into SEGMENTS of `segment_entries`; a segment is summed by one lane (MpPlan::lane: at least
//             MP_LANE_BUCKETS buckets, enough for every lane of the chip) or by one wave (lanes stride, then six shuffle rounds of the
//             complete addition).  The only segment of a bucket adds straight into the stored bucket, the segments of a longer bucket leave
//             partial sums which k_mp_merge adds up, one wave per such bucket: the dependent chain per lane is bounded whatever the input.
//   reduce    per window sum_b (b + 1) B_b: groups of L buckets by running sums (S_g, T_g) (k_mp_reduce1, one lane per group), then one
//             wave per window: sum_g T_g + L sum_g g S_g, the weighted sum by running sums per lane and a suffix scan across the lanes
//             (k_mp_reduce2).  The factors L and M are powers of two: c - 1 doublings per window at most, once.
//   combine   sum_w 2^(c w) W_w by Horner (one lane: about 128 doublings), canonical affine behind one inversion, one 64-byte store.
//
// Terms are walked in chunks of MpPlan::chunk_terms; the buckets persist across chunks (cleared once per call).  Everything is queued on
// one stream; the host waits only where the workspace has to grow.
#include "bbg_internal.h"
#include "work_layouts.h"
#include "var_base.hip.h"

namespace bbg {

// the plan of a call (MpPlan, mp_plan) and the working memory of one chunk (MpLayout, mp_layout) are plain host code: work_layouts.h
constexpr unsigned MP_GRID_MAX = 16384;          // blocks of one wave: 16 per SIMD
constexpr uint32_t MP_SIGN = 0x80000000u, MP_TWIN = 0x40000000u, MP_TERM = 0x3fffffffu;

// ---------------------------------------------------------------------------------------------- device side
// *(counter + key) += the lanes of the wave that hold `key`, and this lane's place among them: the value the counter had plus the lane's
// rank.  Two rounds aggregate the keys of the first lanes still waiting (all-equal scalars put a whole wave on one key, two interleaved
// values on two), the rest go one by one.  Every lane of the wave must call it; a lane with active = false takes no part.
__device__ __forceinline__ uint32_t wave_agg_add(uint32_t* counter, uint32_t key, bool active)
{
    const unsigned lane = threadIdx.x & 63u;
    uint32_t pos = 0;
    bool todo = active;
#pragma unroll 1
    for (int round = 0; round < 2; round++) {
        const unsigned long long waiting = __ballot(todo);
        if (waiting == 0) break;
        const int leader = __ffsll((long long)waiting) - 1;
        const uint32_t lk = (uint32_t)__shfl((int)key, leader, 64);
        const bool mine = todo && key == lk;
        const unsigned long long same = __ballot(mine);
        uint32_t base = 0;
        if ((int)lane == leader) base = atomicAdd(counter + lk, (uint32_t)__popcll(same));
        base = (uint32_t)__shfl((int)base, leader, 64);
        if (mine) {
            pos = base + (uint32_t)__popcll(same & (((unsigned long long)1 << lane) - 1));
            todo = false;
        }
    }
    if (todo) pos = atomicAdd(counter + key, 1u);
    return pos;
}

// Term t < T of the chunk: entries[(2 w + half) T + t] = key | sign, and the histogram of the keys.  One thread per term.
__global__ void __launch_bounds__(256) k_mp_recode(const Affine* __restrict__ points, const Fr* __restrict__ scalars, size_t T, int c, int windows,
                                                   uint32_t* __restrict__ entries, uint32_t* counts)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool active = t < T;
    const uint32_t dump = (uint32_t)windows << (c - 1);
    uint32_t m[2][4] = { { 0, 0, 0, 0 }, { 0, 0, 0, 0 } };
    bool neg2 = false, inf = true;
    if (active) {
        inf = (reinterpret_cast<const uint32_t*>(points + t)[7] >> 31) != 0;
        neg2 = glv_split_mag(fe_from_mont(fe_load<FrP>(scalars + t)), m[0], m[1]);
    }
    const uint32_t mask = (1u << c) - 1, half_range = 1u << (c - 1);
#pragma unroll
    for (int half = 0; half < 2; half++) {
        uint64_t lo = ((uint64_t)m[half][1] << 32) | m[half][0], hi = ((uint64_t)m[half][3] << 32) | m[half][2];
        const bool flip = half == 1 && !neg2; // - k2 lambda P
        uint32_t carry = 0;
#pragma unroll 1
        for (int w = 0; w < windows; w++) {
            const uint32_t v = ((uint32_t)lo & mask) + carry;
            lo = (lo >> c) | (hi << (64 - c));
            hi >>= c;
            carry = v > half_range ? 1u : 0u;
            const uint32_t mag = carry ? (1u << c) - v : v;
            const uint32_t key = (mag == 0 || inf) ? dump : ((uint32_t)w << (c - 1)) + mag - 1;
            const bool negative = (carry != 0) != flip;
            if (active) entries[((size_t)(2 * w + half)) * T + t] = key | (negative ? MP_SIGN : 0u);
            (void)wave_agg_add(counts, key, active && key != dump); // the dump key is not counted: the scatter drops its entries
        }
    }
}

// off = the exclusive scan of counts over the bins (off[bins] = all entries), cursor = off, segoff = the exclusive scan of the segments
// ceil(count / seg) of the buckets (segoff[buckets] = all segments).  One block: thread i takes `per` consecutive bins.
__global__ void __launch_bounds__(1024) k_mp_scan(const uint32_t* __restrict__ counts, uint32_t bins, uint32_t seg, uint32_t* __restrict__ off,
                                                  uint32_t* __restrict__ cursor, uint32_t* __restrict__ segoff)
{
    __shared__ uint32_t sh_e[1024], sh_s[1024];
    const uint32_t buckets = bins - 1, per = (bins + 1023) / 1024;
    const uint32_t b0 = threadIdx.x * per, b1 = min(b0 + per, bins);
    uint32_t e = 0, s = 0;
    for (uint32_t b = b0; b < b1; b++) {
        const uint32_t n = counts[b];
        e += n;
        if (b < buckets) s += (n + seg - 1) / seg;
    }
    sh_e[threadIdx.x] = e;
    sh_s[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        uint32_t ae = 0, as = 0;
        if (threadIdx.x >= d) ae = sh_e[threadIdx.x - d], as = sh_s[threadIdx.x - d];
        __syncthreads();
        sh_e[threadIdx.x] += ae;
        sh_s[threadIdx.x] += as;
        __syncthreads();
    }
    e = sh_e[threadIdx.x] - e; // exclusive
    s = sh_s[threadIdx.x] - s;
    for (uint32_t b = b0; b < b1; b++) {
        const uint32_t n = counts[b];
        off[b] = e;
        cursor[b] = e;
        segoff[b] = s; // b = buckets: all segments
        e += n;
        if (b < buckets) s += (n + seg - 1) / seg;
    }
    if (threadIdx.x == 1023) off[bins] = sh_e[1023];
}

// sorted[place] = sign | twin | term for every entry that is not on the dump key, the places of a key handed out from its cursor
__global__ void __launch_bounds__(256) k_mp_scatter(const uint32_t* __restrict__ entries, size_t T, size_t count, uint32_t dump, uint32_t* cursor,
                                                    uint32_t* __restrict__ sorted)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t v = dump;
    if (e < count) v = entries[e];
    const uint32_t key = v & ~MP_SIGN;
    const bool active = key != dump;
    const uint32_t place = wave_agg_add(cursor, key, active);
    if (active) sorted[place] = (v & MP_SIGN) | (((e / T) & 1) ? MP_TWIN : 0u) | (uint32_t)(e % T);
}

// the point an entry adds: P, lambda P = (beta x, y) for a twin, negated under the sign
__device__ __forceinline__ Affine mp_entry_point(const Affine* points, uint32_t payload)
{
    Affine a = aff_load(points + (payload & MP_TERM));
    if (payload & MP_TWIN) {
        Fq beta;
#pragma unroll
        for (int i = 0; i < 8; i++) beta.v[i] = GlvP::BETA[i];
        a.x = fe_mul(a.x, beta);
    }
    return aff_neg_if(a, (payload & MP_SIGN) != 0);
}

// the bucket of segment s: the largest b with segoff[b] <= s (segoff[buckets] = all segments > s)
__device__ __forceinline__ uint32_t mp_segment_bucket(const uint32_t* segoff, uint32_t buckets, uint32_t s)
{
    uint32_t lo = 0, hi = buckets;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (segoff[mid] <= s) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Segment s of the chunk: the sum of its entries' points, added into the stored bucket where it is the bucket's only segment and left in
// partial[s] otherwise.  LANE: one lane per segment; else one wave per segment, lanes stride and meet in six shuffle rounds.
template <bool LANE>
__global__ void __launch_bounds__(64) k_mp_accumulate(const Affine* __restrict__ points, const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ off,
                                                      const uint32_t* __restrict__ segoff, uint32_t buckets, uint32_t seg, Xyzz* bucket_sums, Xyzz* __restrict__ partial)
{
    const uint32_t segments = segoff[buckets];
    const uint32_t step = LANE ? gridDim.x * 64u : gridDim.x;
#pragma unroll 1
    for (uint32_t s = LANE ? blockIdx.x * 64u + threadIdx.x : blockIdx.x; s < segments; s += step) {
        const uint32_t b = mp_segment_bucket(segoff, buckets, s);
        const uint32_t first = segoff[b], of_bucket = segoff[b + 1] - first;
        const uint32_t beg = off[b] + (s - first) * seg, end = min(beg + seg, off[b + 1]);
        Xyzz acc = xyzz_inf();
#pragma unroll 1
        for (uint32_t e = beg + (LANE ? 0u : threadIdx.x); e < end; e += LANE ? 1u : 64u) acc = xyzz_madd(acc, mp_entry_point(points, sorted[e]));
        if (!LANE && end - beg > 1) acc = xyzz_wave_sum(acc);
        if (LANE || threadIdx.x == 0) {
            if (of_bucket == 1) xyzz_store(bucket_sums + b, xyzz_add(xyzz_load(bucket_sums + b), acc));
            else xyzz_store(partial + s, acc);
        }
    }
}

// a bucket of more than one segment: the stored bucket += its partial sums.  One wave per bucket at a time.
__global__ void __launch_bounds__(64) k_mp_merge(const uint32_t* __restrict__ segoff, uint32_t buckets, Xyzz* bucket_sums, const Xyzz* __restrict__ partial)
{
#pragma unroll 1
    for (uint32_t b = blockIdx.x; b < buckets; b += gridDim.x) {
        const uint32_t first = segoff[b], last = segoff[b + 1];
        if (last - first < 2) continue;
        Xyzz acc = xyzz_inf();
#pragma unroll 1
        for (uint32_t s = first + threadIdx.x; s < last; s += 64) acc = xyzz_add(acc, xyzz_load(partial + s));
        acc = xyzz_wave_sum(acc);
        if (threadIdx.x == 0) xyzz_store(bucket_sums + b, xyzz_add(xyzz_load(bucket_sums + b), acc));
    }
}

// Group i = w groups + g: S = sum_j B[j], T = sum_j (j + 1) B[j] over the L = 2^group_log buckets B[j] = bucket (w groups + g) L + j, by
// running sums from the top.  One lane per group.
__global__ void __launch_bounds__(64) k_mp_reduce1(const Xyzz* __restrict__ bucket_sums, size_t all_groups, int group_log, Xyzz* __restrict__ sg, Xyzz* __restrict__ tg)
{
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= all_groups) return;
    const Xyzz* B = bucket_sums + (i << group_log);
    Xyzz s = xyzz_inf(), t = xyzz_inf();
#pragma unroll 1
    for (int j = (1 << group_log) - 1; j >= 0; j--) {
        s = xyzz_add(s, xyzz_load(B + j));
        t = xyzz_add(t, s);
    }
    xyzz_store(sg + i, s);
    xyzz_store(tg + i, t);
}

// Window w (one wave): winsum[w] = sum_g T_g + L sum_g g S_g.  Lane l takes the M = 2^m_log groups l M .. l M + M - 1 (none beyond
// `groups`): tt = sum T_g, s = sum S_g, t = sum (g - l M) S_g by running sums.  Then sum_g g S_g = sum_l t_l + M sum_l l s_l, and
// sum_l l s_l = sum_(j >= 1) suffix_j with suffix_j = sum_(l >= j) s_l: an inclusive suffix scan in six shuffle rounds.
__global__ void __launch_bounds__(64) k_mp_reduce2(const Xyzz* __restrict__ sg, const Xyzz* __restrict__ tg, uint32_t groups, int m_log, int group_log,
                                                   Xyzz* __restrict__ winsum)
{
    const unsigned lane = threadIdx.x;
    const Xyzz* S = sg + (size_t)blockIdx.x * groups;
    const Xyzz* Tg = tg + (size_t)blockIdx.x * groups;
    const uint32_t g0 = lane << m_log;
    Xyzz s = xyzz_inf(), t = xyzz_inf(), tt = xyzz_inf();
    if (g0 < groups) {
#pragma unroll 1
        for (int g = (1 << m_log) - 1; g >= 0; g--) {
            t = xyzz_add(t, s);
            s = xyzz_add(s, xyzz_load(S + g0 + g));
            tt = xyzz_add(tt, xyzz_load(Tg + g0 + g));
        }
    }
    tt = xyzz_wave_sum(tt);
    Xyzz acc = xyzz_wave_sum(t);
#pragma unroll 1
    for (int d = 1; d < 64; d <<= 1) { // s becomes the suffix sum
        Xyzz o;
#pragma unroll
        for (int w = 0; w < 8; w++) {
            o.x.v[w] = (uint32_t)__shfl_down((int)s.x.v[w], d, 64);
            o.y.v[w] = (uint32_t)__shfl_down((int)s.y.v[w], d, 64);
            o.zz.v[w] = (uint32_t)__shfl_down((int)s.zz.v[w], d, 64);
            o.zzz.v[w] = (uint32_t)__shfl_down((int)s.zzz.v[w], d, 64);
        }
        if (lane + d >= 64) o = xyzz_inf();
        s = xyzz_add(s, o);
    }
    if (lane == 0) s = xyzz_inf();
    s = xyzz_wave_sum(s); // sum_l l s_l
#pragma unroll 1
    for (int i = 0; i < m_log; i++) s = xyzz_dbl(s);
    acc = xyzz_add(acc, s); // sum_g g S_g
#pragma unroll 1
    for (int i = 0; i < group_log; i++) acc = xyzz_dbl(acc);
    acc = xyzz_add(acc, tt);
    if (lane == 0) xyzz_store(winsum + blockIdx.x, acc);
}

// out = sum_w 2^(c w) winsum[w] by Horner, canonical affine (aff_inf() for infinity).  One lane: a chain of c (windows - 1) doublings.
__global__ void __launch_bounds__(64) k_mp_combine(const Xyzz* __restrict__ winsum, int windows, int c, Affine* out)
{
    if (threadIdx.x != 0) return;
    Xyzz acc = xyzz_load(winsum + windows - 1);
#pragma unroll 1
    for (int w = windows - 2; w >= 0; w--) {
#pragma unroll 1
        for (int i = 0; i < c; i++) acc = xyzz_dbl(acc);
        acc = xyzz_add(acc, xyzz_load(winsum + w));
    }
    aff_batch_chunk4(out, 1, [&](int) __attribute__((always_inline)) { return acc; });
}

// ---------------------------------------------------------------------------------------------- host side
int msm_points_plan(size_t n, int window_bits, int* c, int* windows, size_t* chunk_terms, size_t* segment_entries)
{
    MpPlan p;
    if (!mp_plan(n, window_bits, &p)) {
        set_error("bbg_g1_msm_plan: window_bits must be 0 or 2 .. 16 and n at most 2^28");
        return BBG_E_INVALID;
    }
    if (c) *c = p.c;
    if (windows) *windows = p.windows;
    if (chunk_terms) *chunk_terms = p.chunk_terms;
    if (segment_entries) *segment_entries = p.segment_entries;
    return BBG_OK;
}

// d_out = sum_i d_scalars[i] d_points[i] on `st`: 64 B canonical affine, aff_inf() for infinity (n = 0 included).  Queues only.
int msm_points_run(bbg_ctx* ctx, const void* d_points, const void* d_scalars, size_t n, int window_bits, void* d_out, hipStream_t st)
{
    const char* who = "bbg_g1_msm_device";
    MpPlan p;
    if (!mp_plan(n, window_bits, &p)) { set_error(std::string(who) + ": window_bits must be 0 or 2 .. 16 and n at most 2^28"); return BBG_E_INVALID; }
    if (!d_out || (n && (!d_points || !d_scalars))) { set_error(std::string(who) + ": null argument"); return BBG_E_INVALID; }
    if (n && (ranges_overlap(d_out, 64, d_points, n * 64) || ranges_overlap(d_out, 64, d_scalars, n * 32))) {
        set_error(std::string(who) + ": the output overlaps an input");
        return BBG_E_INVALID;
    }
    const size_t T = std::max<size_t>(std::min(n, p.chunk_terms), 1);
    const MpLayout l = mp_layout(p, T);
    if (int rc = ensure_layout(ctx->msm_points_work, l.lay, who)) return rc;
    char* ws = (char*)ctx->msm_points_work.p;
    Xyzz *bucket_sums = (Xyzz*)(ws + l.buckets), *sg = (Xyzz*)(ws + l.sg), *tg = (Xyzz*)(ws + l.tg), *winsum = (Xyzz*)(ws + l.winsum), *partial = (Xyzz*)(ws + l.partial);
    uint32_t *counts = (uint32_t*)(ws + l.counts), *off = (uint32_t*)(ws + l.off), *cursor = (uint32_t*)(ws + l.cursor), *segoff = (uint32_t*)(ws + l.segoff);
    uint32_t *entries = (uint32_t*)(ws + l.entries), *sorted = (uint32_t*)(ws + l.sorted);
    const uint32_t buckets = (uint32_t)p.buckets, bins = buckets + 1;
    BBG_HIP(hipMemsetAsync(bucket_sums, 0, p.buckets * 128, st)); // xyzz_inf() is all zero words
    for (size_t from = 0; from < n; from += p.chunk_terms) {
        const size_t t = std::min(n - from, p.chunk_terms), count = 2 * (size_t)p.windows * t;
        const Affine* pts = (const Affine*)d_points + from;
        {
            ProfScope ps(ctx, "msm_points_sort", st);
            BBG_HIP(hipMemsetAsync(counts, 0, (size_t)bins * 4, st));
            hipLaunchKernelGGL(k_mp_recode, dim3(grid_for(t, 256)), dim3(256), 0, st, pts, (const Fr*)d_scalars + from, t, p.c, p.windows, entries, counts);
            hipLaunchKernelGGL(k_mp_scan, dim3(1), dim3(1024), 0, st, (const uint32_t*)counts, bins, (uint32_t)p.segment_entries, off, cursor, segoff);
            hipLaunchKernelGGL(k_mp_scatter, dim3(grid_for(count, 256)), dim3(256), 0, st, (const uint32_t*)entries, t, count, buckets, cursor, sorted);
        }
        {
            ProfScope ps(ctx, "msm_points_accumulate", st);
            const size_t segs = std::max<size_t>(mp_max_segments(p, t), 1);
            if (p.lane)
                hipLaunchKernelGGL(k_mp_accumulate<true>, dim3((unsigned)std::min<size_t>((segs + 63) / 64, MP_GRID_MAX)), dim3(64), 0, st, pts, (const uint32_t*)sorted,
                                   (const uint32_t*)off, (const uint32_t*)segoff, buckets, (uint32_t)p.segment_entries, bucket_sums, partial);
            else
                hipLaunchKernelGGL(k_mp_accumulate<false>, dim3((unsigned)std::min<size_t>(segs, MP_GRID_MAX)), dim3(64), 0, st, pts, (const uint32_t*)sorted,
                                   (const uint32_t*)off, (const uint32_t*)segoff, buckets, (uint32_t)p.segment_entries, bucket_sums, partial);
            hipLaunchKernelGGL(k_mp_merge, dim3((unsigned)std::min<size_t>(p.buckets, 4096)), dim3(64), 0, st, (const uint32_t*)segoff, buckets, bucket_sums,
                               (const Xyzz*)partial);
        }
    }
    {
        ProfScope ps(ctx, "msm_points_reduce", st);
        const size_t all_groups = (size_t)p.windows * p.groups;
        hipLaunchKernelGGL(k_mp_reduce1, dim3(grid_for(all_groups, 64)), dim3(64), 0, st, (const Xyzz*)bucket_sums, all_groups, p.group_log, sg, tg);
        hipLaunchKernelGGL(k_mp_reduce2, dim3((unsigned)p.windows), dim3(64), 0, st, (const Xyzz*)sg, (const Xyzz*)tg, (uint32_t)p.groups, p.lane_groups_log, p.group_log,
                           winsum);
    }
    {
        ProfScope ps(ctx, "msm_points_combine", st);
        hipLaunchKernelGGL(k_mp_combine, dim3(1), dim3(64), 0, st, (const Xyzz*)winsum, p.windows, p.c, (Affine*)d_out);
    }
    BBG_HIP(hipGetLastError());
    return BBG_OK;
}

} // namespace bbg
