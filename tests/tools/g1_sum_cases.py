"""Inputs and expectations of tests/test_gpu_g1_helpers.py (bbg_g1_sum, bbg_g1_sum_device, bbg_g1_normalize) and the designed points of
tests/test_gpu_multi_group.py, built on the CPU alone: Python integers mod r and one oracle.g1_mul per point.  Nothing here touches the
GPU or the library, so tests/test_g1_sum_cases_cpu.py holds every case to a second route before any GPU time is spent.

Every point is [k] G for a plain integer k.  Its affine value comes from oracle.g1_mul; it is handed over as the Jacobian
(x l^2, y l^3, l) with a non-zero l of its own (l = 1 at index 0 of every case).  The expectation of a sum is the closed form
[sum k_i mod r] G, or the point at infinity when that sum is 0 -- never a result of the library.

The designs follow the reduction order of k_g1_sum (csrc/msm.hip), which `replay` restates on the integers: 256 threads, thread t adds
the inputs t, t + 256, t + 512, .. one after the other (the serial steps), then a tree over the `tree_width(n)` lowest threads, thread
t < stride adding thread t + stride for stride = width / 2, .., 1.  Each step is one xyzz_add(a, b) (csrc/curve.hip.h), which compares
its operands only when both are finite; `replay` lists exactly those steps, so a design can be checked for the branch it is after:

    generic          distinct random k: no step meets equal or opposite operands
    all_equal        one k under n different l: the result is [n k] G; for n a power of two up to 512 EVERY step is a doubling
    level1_*         the serial sums S_t of the two halves of the tree satisfy S_(t + w / 2) = +-S_t (for n <= 256, k_(t + w / 2) =
                     +-k_t): the first tree level doubles, or gives infinity, at every pair; `_free` leaves the pair of slot
                     w / 2 - 1 (whose partner is absent when n = w - 1) generic, so that the opposite variant has a finite result
    level2_*         all k distinct and no coincidence at the first level, but S_t + S_(t + w / 2) = +-(S_(t + w / 4) + S_(t + 3 w / 4))
    serial_*         n > 256 and k_(i + 256) = +-k_i: the serial steps double or cancel
    lifted_twin      equal elements under the SAME l, one twin canonical and the other with X, Y or Z lifted by q (below 2 q, so the
                     infinity bit stays clear): tree twins (k_(t + w / 2) = k_t) up to 256 points, serial twins (k_(i + 256) = k_i, i < 256) above
    inf_*            inputs flagged as infinity (bit 63 of word 3 of x) in a pattern; `_dirty`: the flag set and every other word arbitrary
"""
import random

import numpy as np

import coarse_inputs as ci
import fixed_base_model as fb

R, Q = ci.R_MOD, ci.Q_MOD
SEED = 0xBB254 + 0x6153
THREADS = 256
FLAG = 1 << 63  # in word 3 of x

SIZES = (0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1000)
FAMILY_SIZES = (2, 4, 16, 256, 257, 600)
FREE_SIZES = (3, 4, 15, 16, 255, 256, 257, 600)  # n = w - 1: the free slot's partner is absent, one point stays unpaired
LEVEL2_SIZES = (4, 16, 256, 257, 600)            # needs a tree of two levels
SERIAL_SIZES = (257, 511, 512, 513, 600)
INF_PATTERNS = ("all", "every_other", "every_other_dirty", "only_first", "all_but_last", "lower_half", "upper_half")
NORMALIZE_SIZES = (0, 1, 2, 127, 128, 129, 1000)
POOL = 1024

FAMILIES = (
    [("generic", n) for n in SIZES]
    + [("all_equal", n) for n in FAMILY_SIZES + (512,)]
    + [(f, n) for f in ("level1_equal", "level1_opposite") for n in FAMILY_SIZES]
    + [(f, n) for f in ("level1_equal_free", "level1_opposite_free") for n in FREE_SIZES]
    + [(f, n) for f in ("level2_equal", "level2_opposite") for n in LEVEL2_SIZES]
    + [(f, n) for f in ("serial_equal", "serial_opposite") for n in SERIAL_SIZES]
    + [("lifted_twin", n) for n in FAMILY_SIZES]
    + [("inf_" + p, n) for p in INF_PATTERNS for n in FAMILY_SIZES]
)
NAMES = tuple(f"{f}-{n}" for f, n in FAMILIES)
DEVICE_SIZES = (0, 1, 257, 600)  # the cases that also go through bbg_g1_sum_device
DEVICE_NAMES = tuple(f"{f}-{n}" for f, n in FAMILIES if n in DEVICE_SIZES)

_made = {}
_points = {}


def once(key, make):
    if key not in _made:
        _made[key] = make()
    return _made[key]


# ------------------------------------------------------------------------------------------------ the reduction order on integers
def tree_width(n):
    """k_g1_sum: the smallest power of two >= n, at most 256 (1 for n = 0)."""
    w = THREADS
    while w > 1 and (w >> 1) >= n:
        w >>= 1
    return w


def slot_sum(ks, t):
    """S_t: what thread t holds after its serial steps."""
    return sum(ks[t::THREADS]) % R


def replay(ks):
    """(total, steps) of k_g1_sum on the integers ks (0 = an input at infinity): steps = [(("serial", j) or ("tree", level), a, b)] for
    every xyzz_add(a, b) whose operands are both finite, in the order of the kernel."""
    n = len(ks)
    acc, steps = [0] * THREADS, []
    for t in range(min(n, THREADS)):
        for j, i in enumerate(range(t, n, THREADS)):
            a, b = acc[t], ks[i] % R
            if a and b:
                steps.append((("serial", j), a, b))
            acc[t] = (a + b) % R
    stride, level = tree_width(n) >> 1, 1
    while stride >= 1:
        for t in range(stride):
            a, b = acc[t], acc[t + stride]
            if a and b:
                steps.append((("tree", level), a, b))
            acc[t] = (a + b) % R
        stride >>= 1
        level += 1
    return acc[0], steps


def kind(a, b):
    return "equal" if a == b else "opposite" if (a + b) % R == 0 else "generic"


# ------------------------------------------------------------------------------------------------ points
def _rng(*tag):
    return random.Random(":".join(str(v) for v in (SEED,) + tag))


def pool_scalars():
    """POOL distinct random scalars: the cases that need no designed value draw from them, so their points are computed once."""
    def make():
        rng = _rng("pool")
        ks = [rng.randrange(1, R) for _ in range(POOL)]
        assert len({min(k, R - k) for k in ks}) == POOL
        return tuple(ks)
    return once("pool", make)


def point(oracle, k):
    """(x, y) of [k] G as canonical Montgomery residues, k != 0 mod r: oracle.g1_mul on the generator, -P from a known P."""
    k %= R
    assert k
    if k not in _points:
        if R - k in _points:
            x, y = _points[R - k]
            _points[k] = (x, Q - y)  # y = 0 cannot occur in a group of odd order
        else:
            w = oracle.g1_mul(oracle.g1_generator(), ci.to_words([ci.to_mont(k, 0)])[0])
            x, y = ci.to_ints(w.reshape(2, 4))
            assert x >> 255 == 0
            _points[k] = (x % Q, y % Q)
    return _points[k]


def affine_words(oracle, k):
    """[k] G as 8 canonical Montgomery words; the affine infinity of include/bbg.h for k = 0 mod r."""
    if k % R == 0:
        return fb.aff_infinity()
    return ci.to_words(point(oracle, k)).reshape(8)


def affine_points(oracle, ks):
    return np.stack([affine_words(oracle, k) for k in ks]) if len(ks) else np.zeros((0, 8), dtype=np.uint64)


def jacobian_ints(oracle, k, lam):
    """(X, Y, Z) = (x l^2, y l^3, l) of [k] G as canonical Montgomery residues (l a plain integer: x l^2 keeps x's Montgomery factor)."""
    x, y = point(oracle, k)
    lam %= Q
    assert lam
    return [x * lam * lam % Q, y * pow(lam, 3, Q) % Q, ci.to_mont(lam, 1)]


def clean_infinity():
    j = np.zeros(12, dtype=np.uint64)
    j[3] = np.uint64(FLAG)
    return j


def dirty_infinity(rng):
    """The flag set, every other bit arbitrary."""
    j = np.array([rng.getrandbits(64) for _ in range(12)], dtype=np.uint64)
    j[3] |= np.uint64(FLAG)
    return j


def jacobians(oracle, ks, lams, lifts=None, flags=None, tag=""):
    """(n, 12) words: entry i is [ks[i]] G under lams[i]; lifts = {i: 0 | 1 | 2} adds q to X, Y or Z of entry i; flags = {i: dirty}
    replaces entry i by an infinity."""
    lifts, flags = lifts or {}, flags or {}
    rng = _rng("dirty", tag)
    out = np.zeros((len(ks), 12), dtype=np.uint64)
    for i, (k, lam) in enumerate(zip(ks, lams)):
        if i in flags:
            out[i] = dirty_infinity(rng) if flags[i] else clean_infinity()
            continue
        c = jacobian_ints(oracle, k, lam)
        if i in lifts:
            c[lifts[i]] += Q
            assert c[lifts[i]] < 2 * Q < 1 << 255
        out[i] = ci.to_words(c).reshape(12)
    return out


# ------------------------------------------------------------------------------------------------ the designs (integers only)
class Spec:
    """ks: the scalar of every entry; lams: its l; lifts / flags as `jacobians` takes them; eff: the scalars as the sum sees them (0 where
    flagged); total = sum eff mod r."""

    def __init__(self, name, ks, lams, lifts=None, flags=None):
        self.name, self.n = name, len(ks)
        self.ks, self.lams, self.lifts, self.flags = list(ks), list(lams), dict(lifts or {}), dict(flags or {})
        self.eff = [0 if i in self.flags else k % R for i, k in enumerate(self.ks)]
        self.total = sum(self.eff) % R
        assert all(k % R for k in self.ks) and all(lam % Q for lam in self.lams)


def _lams(rng, n):
    """Distinct non-zero l, l = 1 first."""
    out = [1] + [rng.randrange(2, Q) for _ in range(max(n - 1, 0))]
    assert len(set(out)) == len(out)
    return out[:n]


def _solve(ks, u, target):
    """Sets the first input of slot u so that S_u = target."""
    ks[u] = (target - sum(ks[u + THREADS::THREADS])) % R
    assert ks[u] != 0


def _level1(ks, sign, free):
    w = tree_width(len(ks))
    h = w >> 1
    for t in range(h):
        if t + h >= len(ks) or (free and t == h - 1):
            continue
        _solve(ks, t + h, sign * slot_sum(ks, t))


def _level2(ks, sign):
    n, w = len(ks), tree_width(len(ks))
    h, q = w >> 1, w >> 2
    assert q >= 1
    for t in range(q):
        s = lambda u: slot_sum(ks, u) if u < n else 0  # noqa: E731
        _solve(ks, t + q, sign * (s(t) + s(t + h)) - s(t + h + q))


def _flagged(pattern, n):
    h = tree_width(n) >> 1
    return {"all": lambda i: True, "every_other": lambda i: i % 2 == 0, "only_first": lambda i: i == 0, "all_but_last": lambda i: i != n - 1,
            "lower_half": lambda i: i % THREADS < h, "upper_half": lambda i: i % THREADS >= h}[pattern]


def spec(name):
    """The design `name` = "<family>-<n>" on integers."""
    def make():
        family, n = name.rsplit("-", 1)
        n = int(n)
        rng = _rng(name)
        ks = rng.sample(pool_scalars(), n)
        lams = _lams(rng, n)
        lifts, flags = {}, {}
        if family == "all_equal":
            ks = [ks[0]] * n
        elif family.startswith("level1_"):
            _level1(ks, 1 if "equal" in family else -1, family.endswith("_free"))
        elif family.startswith("level2_"):
            _level2(ks, 1 if "equal" in family else -1)
        elif family.startswith("serial_"):
            assert n > THREADS
            for i in range(THREADS, n):
                ks[i] = ks[i - THREADS] if "equal" in family else R - ks[i - THREADS]
        elif family == "lifted_twin":
            h = tree_width(n) >> 1
            twins = [(i - THREADS, i) for i in range(THREADS, min(n, 2 * THREADS))] if n > THREADS else [(t, t + h) for t in range(h) if t + h < n]
            for p, (a, b) in enumerate(twins):
                ks[b], lams[b] = ks[a], lams[a]
                lifts[b if p // 3 % 2 == 0 else a] = p % 3  # X, Y, Z in turn; the later twin lifted, then the earlier one
        elif family.startswith("inf_"):
            pattern = family[4:]
            dirty = pattern.endswith("_dirty")
            hit = _flagged(pattern[:-6] if dirty else pattern, n)
            flags = {i: dirty for i in range(n) if hit(i)}
        else:
            assert family == "generic", family
        return Spec(name, ks, lams, lifts, flags)
    return once(("spec", name), make)


# ------------------------------------------------------------------------------------------------ the cases
class Case:
    pass


def case(oracle, name):
    """name, n, spec, jac ((n, 12) words, read-only), want (8 words: [total] G canonical, or the affine infinity)."""
    def make():
        s = spec(name)
        c = Case()
        c.name, c.n, c.spec = name, s.n, s
        c.jac = jacobians(oracle, s.ks, s.lams, s.lifts, s.flags, tag=name)
        c.want = affine_words(oracle, s.total)
        c.jac.setflags(write=False)
        c.want.setflags(write=False)
        return c
    return once(("case", name), make)


def normalize_case(oracle, n):
    """(jac (n, 12), want (n, 8), kinds) for bbg_g1_normalize over the same material, mixed by index: rescaled (a random l), plain (l = 1),
    lifted (X, Y or Z plus q, under a random l) and flagged (clean and dirty in turn).  want[i] = [k_i] G canonical, or the affine
    infinity for a flagged entry."""
    def make():
        rng = _rng("normalize", n)
        pool = pool_scalars()
        ks = [pool[rng.randrange(POOL)] for _ in range(n)]
        kinds = [("rescaled", "lifted", "flagged", "plain")[i % 4] for i in range(n)]
        lams = [1 if kd == "plain" else rng.randrange(2, Q) for kd in kinds]
        lifts = {i: i // 4 % 3 for i, kd in enumerate(kinds) if kd == "lifted"}
        flags = {i: i // 4 % 2 == 1 for i, kd in enumerate(kinds) if kd == "flagged"}
        jac = jacobians(oracle, ks, lams, lifts, flags, tag=f"normalize-{n}")
        want = affine_points(oracle, [0 if i in flags else k for i, k in enumerate(ks)])
        jac.setflags(write=False)
        want.setflags(write=False)
        return jac, want, tuple(kinds)
    return once(("normalize", n), make)


def mont_scalars(vals):
    """Plain integers -> (n, 4) canonical Montgomery words of Fr."""
    return ci.to_words([ci.to_mont(v % R, 0) for v in vals])
