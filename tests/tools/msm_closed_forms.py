"""MSM input families with exact expectations that stay cheap at 2^18 .. 2^22 terms, and a restatement of how the bucket MSM's launch
shape follows n (test tooling for tests/test_gpu_msm_scale.py).

oracle.msm_naive is far too slow above 2^16 and oracle.pippenger costs seconds at 2^20, so every family below is built so that its result
has a closed form: a scalar sum times one point, sums of point classes, or a pippenger over at most n terms of distinct points.
tests/test_msm_closed_forms_cpu.py checks each closed form against oracle.msm_naive at small n and shows that it rejects near misses.

Scalars are Montgomery words as the ABI takes them; point arrays are (n, 8) affine Montgomery words; a point at infinity has bit 63 of x's
top limb set (the reference's convention).  Expectations are affine (8,) words, or None for the point at infinity.
"""
import collections

import numpy as np

import coarse_inputs as ci

R_MOD = ci.R_MOD
FQ_ONE = ci.to_words([ci.MONT_R % ci.Q_MOD])[0]  # Montgomery 1 in Fq: the Z of an affine point in Jacobian form
FAMILIES = ("A", "B_cancel", "B_mixed", "C", "D", "AD", "E", "F", "G64", "G8", "H", "I")
# which point array a family's terms run over (one registered SRS per kind and size on the GPU)
SRS_KIND = {"A": "equal", "AD": "equal", "B_cancel": "pairs", "B_mixed": "pairs", "C": "twice", "I": "holes",
            "D": "hashed", "E": "hashed", "F": "hashed", "G64": "hashed", "G8": "hashed", "H": "hashed"}
SPARSE_TERMS = 1 << 12  # nonzero scalars of family F
HOLE_STRIDE = 11        # family I: every 11th point is the point at infinity

Case = collections.namedtuple("Case", "family scalars want")


# ---------------------------------------------------------------------------------------------- restatement of the launch shape
CHIP_LANES = 65536      # msm_kernels.hip.h msm_seg_len: 256 CUs x 4 SIMDs x 64
MSM_SEG_MIN, MSM_SEG_DEFAULT = 8, 64  # msm_kernels.hip.h, the constants of the same names
MSM_LONG_SPAN = 48      # msm_kernels.hip.h MSM_LONG_SPAN: buckets spanning more lanes go to k_combine_long (bucket_classify)
MSM_TINY_WIDTH = 8


def msm_auto_window(n):
    """msm.hip msm_auto_window (MSM_SMALL_WINDOW_MAX_LOG2N = 14, MSM_TINY_MAX_LOG2N = 13)."""
    if n >= 1 << 23:
        return 22
    if n >= 1 << 21:
        return 20
    if n >= 1 << 20:
        return 19
    if n > (1 << 14) + 1024:
        return 16
    if n <= (1 << 13) + 1024:
        return MSM_TINY_WIDTH
    return 13


def msm_windows(c):
    """msm_cfg.h MsmCfg<C>::windows."""
    return (254 + c) // c


def msm_buckets(c):
    return 1 << (c - 1)


def msm_seg_len(entries, buckets, waves_override=0):
    """msm_kernels.hip.h msm_seg_len: entries per accumulation lane segment (buckets = sets x 2^(C-1))."""
    max_waves = waves_override if waves_override > 0 else 6
    if entries <= MSM_SEG_MIN * 4 * CHIP_LANES:
        return MSM_SEG_MIN
    if entries <= MSM_SEG_DEFAULT * max_waves * CHIP_LANES:
        k = max(4, -(-entries // (MSM_SEG_DEFAULT * CHIP_LANES)))
        if waves_override > 0:
            k = waves_override
        seg = -(-entries // (k * CHIP_LANES))
    else:
        per_round = MSM_SEG_DEFAULT * max_waves * CHIP_LANES
        rounds = max(1, (entries + per_round // 2) // per_round)
        seg = -(-entries // (rounds * max_waves * CHIP_LANES))
    while entries // seg > buckets * 32 and entries // seg > 1048576:
        seg *= 2
    return seg


def msm_shape(n, c=None, waves=0, sets=1, total_n=None):
    """What an n-term MSM (or a batch of `sets` of total_n terms) runs with: window, windows, seg, lanes and the default one-lane combine
    kernel (msm_kernels.hip.h msm_run_c, `groups`: k_combine_lanes when lanes > 2 x buckets, else k_combine; the four-thread forms of
    msm_reduce_quad bit 0, k_combine_lanes<C, EcQuad> and k_combine_q, are chosen by the same test).  Only used to pick option values and to document what a case reaches, never to compute a result."""
    c = c or msm_auto_window(n)
    total_n = n if total_n is None else total_n
    entries = total_n * msm_windows(c)
    nb = sets * msm_buckets(c)
    seg = msm_seg_len(entries, nb, waves)
    lanes = -(-entries // seg)
    return {"c": c, "windows": msm_windows(c), "entries": entries, "seg": seg, "lanes": lanes,
            "combine": "k_combine_lanes" if lanes > 2 * nb else "k_combine",
            "count": "k_sortA_count<STRIDE>" if -(-n // 1024) > 2048 else "k_sortA_count"}


# (log2 n, msm_acc_waves) -> (seg, combine kernel) the GPU module runs; pinned against the restatement by the CPU test
SCALE_CASES = {
    (18, 0): (16, "k_combine_lanes"),
    (18, 1): (64, "k_combine"),
    (18, 8): (8, "k_combine_lanes"),
    (20, 0): (56, "k_combine"),
    (20, 3): (75, "k_combine"),
    (20, 12): (19, "k_combine_lanes"),
    (20, 32): (7, "k_combine_lanes"),
    (22, 0): (70, "k_combine"),
    (22, 16): (52, "k_combine"),
}


# ---------------------------------------------------------------------------------------------- group helpers
def is_inf(p):
    return p is None or bool(int(p[3]) >> 63)


def as_result(p):
    """Oracle affine output -> (8,) words, or None for the point at infinity."""
    return None if is_inf(p) else np.ascontiguousarray(p, dtype=np.uint64)


def add(oracle, a, b):
    if is_inf(a):
        return as_result(b)
    if is_inf(b):
        return as_result(a)
    return as_result(oracle.g1_add(a, b))


def mul(oracle, p, k):
    """k * p for an integer k (the plain scalar value): oracle.g1_mul takes a Montgomery scalar."""
    k %= R_MOD
    if k == 0 or is_inf(p):
        return None
    return as_result(oracle.g1_mul(p, ci.to_words([ci.to_mont(k, 0)])[0]))


def point_sum(oracle, pts):
    """Sum of the affine points (infinities skipped), or None."""
    pts = np.ascontiguousarray(pts, dtype=np.uint64).reshape(-1, 8)
    pts = pts[(pts[:, 3] >> np.uint64(63)) == 0]
    if pts.shape[0] == 0:
        return None
    jac = np.empty((pts.shape[0], 12), dtype=np.uint64)
    jac[:, :8] = pts
    jac[:, 8:] = FQ_ONE
    return as_result(oracle.g1_sum(jac))


def mont_sum(words):
    """(sum of the scalars' plain values) mod r, from their Montgomery words: Montgomery form is linear, so the sum of the words is the
    Montgomery form of the sum; summed by 32-bit halves so that 2^22 rows cannot overflow."""
    w = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, 4)
    total = 0
    for k in range(4):
        total += int((w[:, k] & np.uint64(0xFFFFFFFF)).sum(dtype=np.uint64)) << (64 * k)
        total += int((w[:, k] >> np.uint64(32)).sum(dtype=np.uint64)) << (64 * k + 32)
    return ci.from_mont(total % R_MOD, 0)


def plain(word):
    """Plain value of one Montgomery scalar (4,) words."""
    return ci.from_mont(ci.to_ints(word)[0] % R_MOD, 0)


def negate(oracle, pts):
    out = np.array(pts, dtype=np.uint64, copy=True).reshape(-1, 8)
    out[:, 4:] = oracle.fe_sub(1, np.zeros((out.shape[0], 4), dtype=np.uint64), out[:, 4:])
    return out


def mont_words(vals):
    return ci.to_words([ci.to_mont(v % R_MOD, 0) for v in vals])


def class_form(oracle, pts, values, classes):
    """sum_j values[j] * (sum of the points i with classes[i] == j); values are plain integers."""
    order = np.argsort(classes, kind="stable")
    bounds = np.searchsorted(classes[order], np.arange(len(values) + 1))
    want = None
    for j, v in enumerate(values):
        if v % R_MOD:
            want = add(oracle, want, mul(oracle, point_sum(oracle, pts[order[bounds[j]:bounds[j + 1]]]), v))
    return want


# ---------------------------------------------------------------------------------------------- point arrays
def srs_points(oracle, kind, base):
    """The (n, 8) point array of a family kind over a hashed base of n distinct points."""
    n = base.shape[0]
    if kind == "hashed":
        return base
    if kind == "equal":
        return np.repeat(base[:1], n, axis=0)
    if kind == "pairs":  # P_0, -P_0, P_2, -P_2, ...
        out = np.array(base, copy=True)
        out[1::2] = negate(oracle, base[0::2][: n // 2])
        return out
    if kind == "twice":  # P_0, P_0, P_1, P_1, ...
        return np.repeat(base[: n // 2], 2, axis=0)
    if kind == "holes":
        out = np.array(base, copy=True)
        out[::HOLE_STRIDE] = 0
        out[::HOLE_STRIDE, 3] = np.uint64(1) << np.uint64(63)
        return out
    raise ValueError(kind)


def digit_edge_scalars():
    """family H's scalar classes: every digit pattern of every compiled width (coarse_inputs.msm_digit_patterns), each as the canonical
    Montgomery word and as that word + r.  Returns (plain values, (k, 4) words)."""
    ks = [k for c in ci.MSM_WINDOWS for _, k, _ in ci.msm_digit_patterns(c)]
    # a pattern k is the value the recoding sees, i.e. the plain scalar: its Montgomery word is to_mont(k)
    words = mont_words(ks)
    return ks + ks, np.concatenate([words, ci.add_int(words, R_MOD)])


# ---------------------------------------------------------------------------------------------- families
def family_case(oracle, pkg, family, pts, base, seed):
    """Case(family, scalars, want) over the point array `pts` (= srs_points(SRS_KIND[family], base)).  pkg supplies synthetic_scalars.
    Cost: at most one oracle.pippenger over n terms of distinct points."""
    n = pts.shape[0]
    rnd = pkg.synthetic_scalars
    if family == "A":  # (sum s_i) * P
        sc = rnd(seed, n)
        return Case(family, sc, mul(oracle, pts[0], mont_sum(sc)))
    if family == "AD":  # n doublings in one bucket of every window: (n s) * P
        sc = np.repeat(rnd(seed, 1), n, axis=0)
        return Case(family, sc, mul(oracle, pts[0], n * plain(sc[0])))
    if family == "B_cancel":  # P with s, -P with s: infinity
        sc = np.repeat(rnd(seed, n // 2), 2, axis=0)
        return Case(family, sc, None)
    if family == "B_mixed":  # every other pair cancels; the rest leave (s_2i - s_2i+1) P_2i
        sc = rnd(seed, n)
        sc[1::4] = sc[0::4]
        diff = oracle.fe_sub(0, sc[0::2], sc[1::2])
        return Case(family, sc, as_result(oracle.pippenger(diff, pts[0::2])))
    if family == "C":  # each point twice, its scalar split s = a + b over the copies
        s = rnd(seed, n // 2)
        a = rnd(seed + 1, n // 2)
        sc = np.empty((n, 4), dtype=np.uint64)
        sc[0::2] = a
        sc[1::2] = oracle.fe_sub(0, s, a)
        return Case(family, sc, as_result(oracle.pippenger(s, pts[0::2])))
    if family == "D":  # all scalars equal: s * sum P
        sc = np.repeat(rnd(seed, 1), n, axis=0)
        return Case(family, sc, mul(oracle, point_sum(oracle, pts), plain(sc[0])))
    if family == "E":  # three scalars by residue class mod 3
        v = rnd(seed, 3)
        cls = np.arange(n) % 3
        return Case(family, v[cls], class_form(oracle, pts, [plain(x) for x in v], cls))
    if family == "F":  # 2^12 nonzero scalars at random indices
        idx = np.sort(np.random.default_rng(seed).choice(n, size=min(SPARSE_TERMS, n), replace=False))
        sc = np.zeros((n, 4), dtype=np.uint64)
        sc[idx] = rnd(seed, idx.shape[0])
        return Case(family, sc, as_result(oracle.pippenger(sc[idx], pts[idx])))
    if family == "G64":  # plain values below 2^64: the top windows are empty
        p_ = np.zeros((n, 4), dtype=np.uint64)
        p_[:, 0] = rnd(seed, n)[:, 0]
        sc = oracle.to_mont(0, p_)
        return Case(family, sc, as_result(oracle.pippenger(sc, pts)))
    if family == "G8":  # plain values 0 .. 7: one window holds every digit, zero digits dropped
        v = np.random.default_rng(seed).integers(0, 8, size=n)
        p_ = np.zeros((n, 4), dtype=np.uint64)
        p_[:, 0] = v.astype(np.uint64)
        return Case(family, oracle.to_mont(0, p_), class_form(oracle, pts, list(range(8)), v))
    if family == "H":  # the recoding's digit edges of every width, as canonical words and + r, by residue class
        vals, words = digit_edge_scalars()
        cls = np.arange(n) % len(vals)
        return Case(family, words[cls], class_form(oracle, pts, vals, cls))
    if family == "I":  # points at infinity every 11th index
        sc = rnd(seed, n)
        keep = (pts[:, 3] >> np.uint64(63)) == 0
        return Case(family, sc, as_result(oracle.pippenger(sc[keep], pts[keep])))
    raise ValueError(family)
