"""Python-integer model of the table-free MSM over the caller's points (csrc/msm_points.hip, bbg_g1_msm), shared by
tests/test_msm_points_cpu.py and tests/test_gpu_msm_points.py.  The group is the integers: a "point" is any integer a, the result is
sum s_i a_i mod r, which is what the device computes for P_i = [a_i] G.

* plan             the automatic width, windows(c), chunk_terms, segment_entries and the workspace formula of include/bbg.h, as the C side has
                   them (the CPU test pins this copy to bbg_g1_msm_plan).
* recode           a half h -> `windows` signed c-bit digits, least significant first, and the carry left over.
* entry / unpack   the key and payload words of one digit.
* weighted_sum     sum_b (b + 1) B_b by the dataflow of k_mp_reduce1 / k_mp_reduce2: groups of L buckets by running sums, lanes of M groups
                   by running sums, a Hillis-Steele suffix scan over 64 lanes.
* route            split, recode, bucket, weighted sum per window, Horner over the windows: the whole call on integers.
* designed_scalars for a width c, a list of 300 scalars (representatives in [0, 2r)) that holds the recoding's edges; edges() names them.
"""
import var_base_model as vb

R_MOD = vb.R_MOD
C_MIN, C_MAX = 2, 16
MAX_N = 1 << 28
BUDGET = 1 << 30
CHUNK_CAP = 1 << 20
LANE_BUCKETS = 65536
SEG_LANE, SEG_WAVE = 256, 1024
GROUP_LOG = 5
SIGN, TWIN, TERM = 1 << 31, 1 << 30, (1 << 30) - 1


def windows(c):
    """The smallest count of c-bit signed digits that takes every half: a half is below 2^127 (var_base_model.half_bounds), and
    h < 2^(c W - 1) leaves the top window at most 2^(c-1) - 1, which absorbs a carry.  One window less cannot hold the bounds: the CPU test
    recodes them with W - 1 windows and finds a carry left."""
    return -(-128 // c)


def auto_width(n):
    """The measured table of csrc/msm_points.hip (profiles/msm_points.txt)"""
    return 4 if n <= 1 << 12 else 8 if n <= 1 << 15 else 9 if n <= 1 << 17 else 16


def shape(c):
    """(buckets, lane layout, segment_entries, L = buckets per group, G = groups per window, M = groups per lane of the window's wave)"""
    w = windows(c)
    buckets = w << (c - 1)
    lane = buckets >= LANE_BUCKETS
    group_log = min(c - 1, GROUP_LOG)
    groups = 1 << (c - 1 - group_log)
    m = 1
    while 64 * m < groups:
        m *= 2
    return buckets, lane, SEG_LANE if lane else SEG_WAVE, 1 << group_log, groups, m


def workspace_bytes(c, terms):
    """The formula of include/bbg.h with its alignment: every region rounded up to 128 bytes."""
    w = windows(c)
    buckets, _, seg, _, groups, _ = shape(c)
    entries = 2 * w * terms
    bins = buckets + 1
    regions = [buckets * 128, w * groups * 128, w * groups * 128, w * 128, (min(buckets, entries) + entries // seg) * 128,
               bins * 4, (bins + 1) * 4, bins * 4, bins * 4, entries * 4, entries * 4]
    return sum(-(-x // 128) * 128 for x in regions)


def chunk_terms(c):
    t = CHUNK_CAP
    while workspace_bytes(c, t) > BUDGET:
        t -= t // 16
    return t


def plan(n, window_bits=0):
    """(c, windows, chunk_terms, segment_entries), or None where the call is refused"""
    if n > MAX_N or (window_bits != 0 and not C_MIN <= window_bits <= C_MAX):
        return None
    c = window_bits or auto_width(n)
    return c, windows(c), chunk_terms(c), shape(c)[2]


def recode(h, c, count=None):
    """(digits, carry): h = sum_w d_w 2^(c w) + carry 2^(c count), |d_w| <= 2^(c-1)"""
    count = windows(c) if count is None else count
    digits, carry = [], 0
    for w in range(count):
        v = ((h >> (c * w)) & ((1 << c) - 1)) + carry
        carry = 1 if v > 1 << (c - 1) else 0
        digits.append(v - (carry << c))
    return digits, carry


def entry(w, d, c, negate, twin, term):
    """(key, payload) of digit d != 0 of window w; negate: the half's own sign (the minus of - k2 lambda, undone by a negative k2)"""
    assert d != 0 and 0 <= term <= TERM
    key = (w << (c - 1)) + abs(d) - 1
    return key, (SIGN if (d < 0) != negate else 0) | (TWIN if twin else 0) | term


def unpack(key, payload, c):
    """(window, |d|, negative, twin, term)"""
    return key >> (c - 1), (key & ((1 << (c - 1)) - 1)) + 1, bool(payload & SIGN), bool(payload & TWIN), payload & TERM


def weighted_sum(B, c):
    """sum_b (b + 1) B[b] over the 2^(c-1) buckets of one window, by the device's dataflow"""
    _, _, _, L, G, M = shape(c)
    assert len(B) == L * G
    sg, tg = [], []
    for g in range(G):  # k_mp_reduce1: one lane per group
        s = t = 0
        for j in range(L - 1, -1, -1):
            s += B[g * L + j]
            t += s
        sg.append(s)
        tg.append(t)
    s_l, t_l, tt_l = [0] * 64, [0] * 64, [0] * 64
    for lane in range(64):  # k_mp_reduce2: one wave per window
        g0 = lane * M
        if g0 < G:
            for g in range(M - 1, -1, -1):
                t_l[lane] += s_l[lane]
                s_l[lane] += sg[g0 + g]
                tt_l[lane] += tg[g0 + g]
    d = 1
    while d < 64:
        s_l = [s_l[i] + (s_l[i + d] if i + d < 64 else 0) for i in range(64)]
        d *= 2
    return sum(tt_l) + L * (sum(t_l) + M * sum(s_l[1:]))


def route(scalars, values, c):
    """sum s_i a_i mod r as the device takes it; scalars: any representatives in [0, 2r)"""
    w_count = windows(c)
    buckets = [0] * (w_count << (c - 1))
    for term, (s, a) in enumerate(zip(scalars, values)):
        k1, k2 = vb.split(s % R_MOD)
        for twin, (h, negate) in enumerate(((k1, False), (abs(k2), k2 >= 0))):
            digits, carry = recode(h, c)
            assert carry == 0
            for w, d in enumerate(digits):
                if d == 0:
                    continue
                key, payload = entry(w, d, c, negate, twin, term & TERM)
                _, _, negative, is_twin, _ = unpack(key, payload, c)
                point = a * vb.LAMBDA % R_MOD if is_twin else a
                buckets[key] += -point if negative else point
    acc = 0
    for w in range(w_count - 1, -1, -1):
        acc = (acc << c) + weighted_sum(buckets[w << (c - 1):(w + 1) << (c - 1)], c)
    return acc % R_MOD


def edges(k, c):
    """The edges of the width-c recoding that scalar k reaches, as a set of names"""
    k1, k2 = vb.split(k % R_MOD)
    found = set()
    if k1 == 0:
        found.add("k1 = 0")
    if k2 == 0:
        found.add("k2 = 0")
    if k2 < 0:
        found.add("k2 negative")
    for h in (k1, abs(k2)):
        digits, carry = recode(h, c)
        assert carry == 0
        if any(abs(d) == 1 << (c - 1) for d in digits):
            found.add("digit of magnitude 2^(c-1)")
        if h and digits[-1] == 0:
            found.add("zero top digit")
        run, carry_in = 0, 0
        for w in range(len(digits)):
            v = ((h >> (c * w)) & ((1 << c) - 1)) + carry_in
            carry_in = 1 if v > 1 << (c - 1) else 0
            run = run + 1 if carry_in else 0
            if run >= 3:
                found.add("carry through three windows")
    return found


EDGES = ("digit of magnitude 2^(c-1)", "carry through three windows", "zero top digit", "k2 = 0", "k1 = 0", "k2 negative")


def designed_scalars(c):
    """300 scalars for width c: the constructed edge cases, the list of var_base_model.gpu_scalars() and r, r + 1, 2r - 1 as
    representatives in [r, 2r).  A scalar below 2^64 is its own first half with k2 = 0 (c1 = c2 = 0 in the split), so:
      2^(c-1)          digit 0 has v = 2^(c-1), not above the half range: d = +2^(c-1), the largest magnitude;
      2^(3c) - 1       windows 0 .. 2 read 2^c - 1, 2^c, 2^c: three carries in a row, digits -1, 0, 0, then +1;
      both             have zero top digits and k2 = 0;  0 has k1 = 0;  negative_half_scalar() has k2 < 0."""
    built = [1 << (c - 1), (1 << (3 * c)) - 1, 0, vb.negative_half_scalar(), (1 << (c - 1)) + (1 << (2 * c - 1))]
    _, ks = vb.gpu_scalars()
    tail = [R_MOD, R_MOD + 1, 2 * R_MOD - 1]
    return built + ks[:300 - len(built) - len(tail)] + tail
