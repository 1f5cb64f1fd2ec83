"""The multi-context group (bbg_multi_* in csrc/multi.hip) on its edges: MSMs over designed strings whose per-context partials are equal,
opposite or at infinity, strings shorter than the group, (from, range) on and beside the shard boundaries; the sharded NTT at its
smallest legal shapes, on coarse inputs, and in resident calls queued back to back with no synchronisation between them.

MSM.  The strings are registered with bbg_multi_srs_register from points [k_i] G with known k_i (tests/tools/g1_sum_cases.py), so every
expectation is [sum s_i k_i mod r] G by Python integers, with oracle.msm_naive over the same words as a second route.  The G partials
meet in k_g1_sum (through bbg_g1_sum, or through the all-gather and g1_sum_device under exchange = 1): equal partials double at every
level of its tree, opposite ones cancel there.  ceil(n / G) sharding leaves the trailing contexts of a short string without points.

NTT.  Against oracle.ntt, bit-exact on canonical words.  The back-to-back sections queue several group calls with NO bbg_multi_sync and no
download between them and synchronise once at the very end: the cross-context waits of multi_ntt_core (ev_sent, ev_done) exist only for
that.  The last section shows completion behind bbg_multi_sync alone, with the discipline of tests/test_gpu_stream_order.py: a first
pass and a full synchronisation take out first-use work; in the checked pass the shards are poisoned, the inputs copied into place on
the device, the resident call queued, bbg_multi_sync called, and `shard.clone()` taken on a fresh stream per device that was created
before the call and is the only thing synchronised afterwards.  Nothing asserts the negative ("stale without the sync"): that is a race.

Each group is created once per module (`group`) and shared; the sections that need a fresh group (buffer growth in flight) make their own.
All contexts share device 0 on a one-GPU box and spread over the GPUs of a node (_spread), as in tests/test_gpu_parity.py."""
import ctypes
import random

import numpy as np
import pytest

import coarse_inputs as ci
import g1_sum_cases as gc
from stream_order import POISON
from test_gpu_parity import COSET_FFT, COSET_IFFT, FFT, IFFT, _distinct, _gather_shards, _Multi, _shards_to_devices, _spread

pytestmark = pytest.mark.gpu

R = gc.R
OPS = (FFT, IFFT, COSET_FFT, COSET_IFFT)
GROUPS = (2, 4, 8)
PER = 6  # points per context in the designed strings: even, so that a shard can consist of P / -P pairs


# ------------------------------------------------------------------------------------------------ groups, shared
@pytest.fixture(scope="module")
def group(pkg, bbg):
    """group(G): the module's one group of G contexts (_spread), made on first use."""
    made = {}

    def get(G):
        if G not in made:
            made[G] = (_Multi(pkg, _spread(pkg, G)), _spread(pkg, G))
        return made[G]
    yield get
    for M, _ in made.values():
        M.close()


@pytest.fixture(scope="module")
def distinct_group(pkg, bbg):
    devs = _distinct(pkg)
    M = _Multi(pkg, devs)
    yield M, devs
    M.close()


# ------------------------------------------------------------------------------------------------ MSM helpers
def rng_for(*tag):
    return random.Random(":".join(str(v) for v in ("multi group",) + tag))


def fresh_scalars(rng, n):
    """Scalars of every size class: full width, 1, r - 1, one word."""
    edge = [1, R - 1, rng.getrandbits(64) | 1]
    return [edge[i % 7] if i % 7 < 3 else rng.randrange(1, R) for i in range(n)]


def register(M, oracle, ks, stride=64):
    pts = gc.affine_points(oracle, ks)
    src = oracle.point_table(pts) if stride == 128 and len(ks) else pts  # (2 n, 8): each point followed by its endomorphism image
    src = np.ascontiguousarray(src)
    M.ck(M.lib.bbg_multi_srs_register(M.h, src.ctypes.data, len(ks), stride))
    assert M.lib.bbg_multi_srs_num_points(M.h) == len(ks)
    return pts


def run_msm(M, words, start=0):
    out = np.zeros(12, dtype=np.uint64)
    s = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, 4)
    M.ck(M.lib.bbg_multi_msm(M.h, s.ctypes.data, start, s.shape[0], out.ctypes.data))
    return out


def check_msm(M, oracle, pts, ks, ss, start=0, what=""):
    """bbg_multi_msm of the scalars ss over points [start, start + len(ss)) against [sum s_i k_i] G, itself held to oracle.msm_naive."""
    n = len(ss)
    total = sum(s * k for s, k in zip(ss, ks[start:start + n])) % R
    want = gc.affine_words(oracle, total)
    words = gc.mont_scalars(ss)
    if n:
        assert np.array_equal(oracle.msm_naive(words, pts[start:start + n]), want), ("second route", what)
    got = run_msm(M, words, start)
    assert (int(got[3]) >> 63 == 1) == (total == 0), (what, "infinity flag")
    if total:
        ci.assert_coarse_jacobian(got, str(what))
    assert np.array_equal(oracle.jac_to_affine(got), want), what
    return total


def material(rng, count):
    return rng.sample(gc.pool_scalars(), count)


def equal_partials(G, rng):
    """Every shard holds the same (point, scalar) pairs, rotated by its index: G equal partials, summed in G different orders."""
    ks, ss = material(rng, PER), fresh_scalars(rng, PER)
    rot = lambda v, g: v[g % PER:] + v[:g % PER]  # noqa: E731
    return sum((rot(ks, g) for g in range(G)), []), sum((rot(ss, g) for g in range(G)), [])


def opposite_partials(G, rng, pattern):
    """Shards of P and -P material under the same scalars.  alternating: + - + - ..; halves: + .. + - .. -; surplus: + - + .. over the
    first G - 1 shards and other material in the last one, so that the total is finite."""
    ks, ss = material(rng, PER), fresh_scalars(rng, PER)
    sign = {"alternating": lambda g: g % 2 == 0, "halves": lambda g: g < (G + 1) // 2, "surplus": lambda g: g % 2 == 0}[pattern]
    out_k = sum(([k if sign(g) else R - k for k in ks] for g in range(G)), [])
    out_s = ss * G
    if pattern == "surplus":
        out_k[-PER:], out_s[-PER:] = material(rng, PER), fresh_scalars(rng, PER)
    return out_k, out_s


def infinite_partial(G, rng, g0, mode):
    """Generic shards, except that the partial of shard g0 is the point at infinity: all its scalars zero (`zeros`), or P / -P pairs under
    pairwise equal scalars inside it (`pairs`)."""
    ks, ss = material(rng, G * PER), fresh_scalars(rng, G * PER)
    lo = g0 * PER
    if mode == "zeros":
        ss[lo:lo + PER] = [0] * PER
    else:
        for j in range(0, PER, 2):
            ks[lo + j + 1], ss[lo + j + 1] = R - ks[lo + j], ss[lo + j]
    assert sum(s * k for s, k in zip(ss[lo:lo + PER], ks[lo:lo + PER])) % R == 0
    return ks, ss


# ------------------------------------------------------------------------------------------------ MSM
@pytest.mark.parametrize("G", GROUPS)
def test_msm_equal_partials_double_at_every_level(group, oracle, G):
    M, _ = group(G)
    ks, ss = equal_partials(G, rng_for("equal", G))
    pts = register(M, oracle, ks)
    total = check_msm(M, oracle, pts, ks, ss, what=("equal partials", G))
    assert total == G * sum(s * k for s, k in zip(ss[:PER], ks[:PER])) % R != 0


@pytest.mark.parametrize("pattern", ["alternating", "halves", "surplus"])
@pytest.mark.parametrize("G", GROUPS)
def test_msm_opposite_partials_cancel(group, oracle, G, pattern):
    M, _ = group(G)
    ks, ss = opposite_partials(G, rng_for("opposite", G, pattern), pattern)
    pts = register(M, oracle, ks)
    total = check_msm(M, oracle, pts, ks, ss, what=(pattern, G))
    assert (total == 0) == (pattern != "surplus")


@pytest.mark.parametrize("mode", ["zeros", "pairs"])
@pytest.mark.parametrize("G", GROUPS)
def test_msm_one_partial_at_infinity(group, oracle, G, mode):
    M, _ = group(G)
    for g0 in (0, G - 1):
        ks, ss = infinite_partial(G, rng_for("infinite", G, mode, g0), g0, mode)
        pts = register(M, oracle, ks)
        assert check_msm(M, oracle, pts, ks, ss, what=(mode, G, g0)) != 0
        # that shard alone: the whole result is the point at infinity
        assert check_msm(M, oracle, pts, ks, ss[g0 * PER:(g0 + 1) * PER], start=g0 * PER, what=(mode, G, g0, "alone")) == 0


@pytest.mark.parametrize("stride", [64, 128])
@pytest.mark.parametrize("G", GROUPS)
def test_msm_strings_shorter_than_the_group(group, oracle, G, stride):
    """ceil(n / G) points per context: G = 8, n = 9 gives shards of 2, 2, 2, 2, 1, 0, 0, 0 points -- trailing contexts own nothing, and
    for n < G so do most.  include/bbg.h excludes no n, so every such string registers and sums like any other."""
    M, _ = group(G)
    for n in sorted({1, 3, G - 1, G, G + 1, 2 * G + 1}):
        rng = rng_for("short", G, n)
        ks, ss = material(rng, n), fresh_scalars(rng, n)
        pts = register(M, oracle, ks, stride)
        assert check_msm(M, oracle, pts, ks, ss, what=("short", G, stride, n)) != 0
        for start in (0, n):
            assert check_msm(M, oracle, pts, ks, [], start=start, what=("no terms", G, stride, n, start)) == 0
        assert M.lib.bbg_multi_srs_num_points(M.h) == n


@pytest.mark.parametrize("G", GROUPS)
def test_msm_ranges_on_and_beside_shard_boundaries(group, pkg, oracle, G):
    M, _ = group(G)
    n = G * PER
    rng = rng_for("ranges", G)
    ks = material(rng, n)
    pts = register(M, oracle, ks)
    ranges = [(PER, PER),          # one whole shard: both ends on boundaries
              (0, PER + 1),        # the end one past a boundary
              (1, PER),            # both ends one past a boundary
              (PER - 1, 2),        # one point on each side
              (PER + 1, 3),        # wholly inside shard 1
              (n - PER, PER),      # the last shard
              (n - 1, 1), (0, n),
              (n, 0), (PER, 0)]    # no terms: at the end of the string and on a boundary
    for start, count in ranges:
        total = check_msm(M, oracle, pts, ks, fresh_scalars(rng, count), start=start, what=("range", G, start, count))
        assert (total == 0) == (count == 0)
    with pytest.raises(pkg.BbgError):
        run_msm(M, gc.mont_scalars([1, 2]), start=n - 1)


def test_msm_partials_through_the_rccl_exchange(distinct_group, oracle):
    """exchange = 1 on the largest group of distinct devices: one context on a one-GPU box, which still goes through the all-gather and
    g1_sum_device; 2, 4 or 8 on a node, where the designed partials meet in the tree."""
    M, devs = distinct_group
    G = len(devs)
    M.ck(M.lib.bbg_multi_set_option(M.h, b"exchange", 1))
    try:
        designs = [("equal", equal_partials(G, rng_for("rccl equal", G)))]
        designs += [(p, opposite_partials(G, rng_for("rccl", p, G), p)) for p in ("alternating", "halves")]
        designs += [(m, infinite_partial(G, rng_for("rccl", m, G), G - 1, m)) for m in ("zeros", "pairs")]
        for what, (ks, ss) in designs:
            pts = register(M, oracle, ks)
            total = check_msm(M, oracle, pts, ks, ss, what=("rccl", what, G))
            if what in ("alternating", "halves") and G > 1:
                assert total == 0
            if what in ("zeros", "pairs"):
                assert (total == 0) == (G == 1)
                assert check_msm(M, oracle, pts, ks, ss[-PER:], start=(G - 1) * PER, what=("rccl", what, G, "alone")) == 0
    finally:
        M.ck(M.lib.bbg_multi_set_option(M.h, b"exchange", 0))


# ------------------------------------------------------------------------------------------------ NTT helpers
def resident(M, shards, lg, op):
    ptrs = (ctypes.c_void_p * len(shards))(*[t.data_ptr() for t in shards])
    M.ck(M.lib.bbg_multi_ntt_device(M.h, ptrs, lg, op))


def host_form(M, a, lg, op):
    buf = np.ascontiguousarray(a, dtype=np.uint64).copy()
    M.ck(M.lib.bbg_multi_ntt(M.h, buf.ctypes.data, lg, op))
    return buf


def gathered(oracle, shards, lg):
    """Canonical natural-order words of resident shards (a blocking download: only after the section's one synchronisation)."""
    return oracle.canon(0, _gather_shards(shards, 1 << lg, len(shards)))


@pytest.fixture(scope="module")
def wanted(pkg, oracle):
    """wanted(seed, lg, op) -> (input, oracle.ntt of it), computed once per module and left unchanged."""
    made = {}

    def get(seed, lg, op):
        if (seed, lg) not in made:
            a = pkg.synthetic_scalars(seed, 1 << lg)
            a.setflags(write=False)
            made[(seed, lg)] = {"a": a}
        d = made[(seed, lg)]
        if op not in d:
            d[op] = oracle.ntt(d["a"], op)
            d[op].setflags(write=False)
        return d["a"], d[op]
    return get


# ------------------------------------------------------------------------------------------------ NTT: shapes and inputs
@pytest.mark.parametrize("G,lg", [(2, 2), (2, 3), (4, 4), (4, 5), (8, 6), (8, 7)])
def test_ntt_smallest_shapes(group, wanted, oracle, G, lg):
    """log2n = 2 log2(G) is the smallest legal size: one element per chunk of the all-to-all (len = 1).  That and the size above it."""
    M, devs = group(G)
    for op in OPS:
        a, want = wanted(0x4100 + G, lg, op)
        assert np.array_equal(oracle.canon(0, host_form(M, a, lg, op)), want), (G, lg, op, "host form")
        shards = _shards_to_devices(a, devs)
        resident(M, shards, lg, op)
        M.ck(M.lib.bbg_multi_sync(M.h))
        assert np.array_equal(gathered(oracle, shards, lg), want), (G, lg, op, "resident form")


@pytest.mark.parametrize("G,lg", [(2, 1), (4, 3), (8, 5), (2, 29), (4, 29), (8, 29)])
def test_ntt_sizes_outside_the_range_are_refused(group, pkg, G, lg):
    """Below 2 log2(G) and above 2^28 both forms refuse before they touch the data (the buffers here are far smaller than 2^29)."""
    M, devs = group(G)
    a = pkg.synthetic_scalars(7, 64)
    shards = _shards_to_devices(a, devs)
    for op in OPS:
        with pytest.raises(pkg.BbgError):
            host_form(M, a, lg, op)
        with pytest.raises(pkg.BbgError):
            resident(M, shards, lg, op)
    M.ck(M.lib.bbg_multi_sync(M.h))
    assert np.array_equal(_gather_shards(shards, 64, G), _gather_shards(_shards_to_devices(a, devs), 64, G)), "a refused call changed its input"


@pytest.mark.parametrize("G,lg", [(4, 6), (8, 8)])
def test_ntt_coarse_inputs(group, wanted, oracle, G, lg):
    """Every input lifted into [r, 2 r): the results are the canonical ones' and every stored word stays below 2 r."""
    M, devs = group(G)
    for op in OPS:
        a, want = wanted(0x4200 + G, lg, op)
        lifted = ci.add_int(a, R)
        assert ci.below(lifted, 2 * R).all() and not ci.below(lifted, R).any()
        got = host_form(M, lifted, lg, op)
        ci.assert_coarse(got, 0, f"host form {G} {lg} {op}")
        assert np.array_equal(oracle.canon(0, got), want), (G, lg, op, "host form")
        shards = _shards_to_devices(lifted, devs)
        resident(M, shards, lg, op)
        M.ck(M.lib.bbg_multi_sync(M.h))
        raw = _gather_shards(shards, 1 << lg, G)
        ci.assert_coarse(raw, 0, f"resident form {G} {lg} {op}")
        assert np.array_equal(oracle.canon(0, raw), want), (G, lg, op, "resident form")


# ------------------------------------------------------------------------------------------------ NTT: back to back, one synchronisation
LG = 8  # 2^8: chunks of 16 (G = 4) and 4 (G = 8) elements


def left_in_shards(spectrum, G):
    """The sequence a resident call leaves behind, read as the residue classes the NEXT call takes its shards for: shard r holds the runs
    A[t m + r len ..) for t < G (include/bbg.h), so element i of shard r is element r + G i of the returned sequence."""
    n = spectrum.shape[0]
    m, length = n // G, n // G // G
    out = np.empty_like(spectrum)
    for r in range(G):
        out[r::G] = np.concatenate([spectrum[t * m + r * length: t * m + (r + 1) * length] for t in range(G)])
    return out


def composed(oracle, a, G, ops):
    """What the resident calls `ops`, queued one after the other on the same shards, leave in them (natural order), by the oracle."""
    v = a
    for k, op in enumerate(ops):
        v = oracle.ntt(left_in_shards(v, G) if k else v, op)
    return v


@pytest.mark.parametrize("forward,back", [(FFT, IFFT), (COSET_FFT, COSET_IFFT)])
@pytest.mark.parametrize("G", [4, 8])
def test_transform_and_inverse_queued_on_the_same_shards(group, wanted, oracle, G, forward, back):
    """The inverse reads what the forward call wrote into the same shards, with nothing but the contexts' streams and the group's events
    between them.  A resident call leaves runs of the natural order in a shard, not its residue class, so the pair is not the identity
    on the shards: the inverse transforms the sequence `left_in_shards` names, and the expectation is the oracle's for exactly that.
    The round trip itself -- the inverse of the spectrum is the input -- is asserted on the oracle's side of the same data."""
    M, devs = group(G)
    a, spectrum = wanted(0x4300 + G, LG, forward)
    assert np.array_equal(oracle.ntt(spectrum, back), oracle.canon(0, a)), "the oracle's round trip"
    shards = _shards_to_devices(a, devs)
    resident(M, shards, LG, forward)
    resident(M, shards, LG, back)
    M.ck(M.lib.bbg_multi_sync(M.h))
    assert np.array_equal(gathered(oracle, shards, LG), composed(oracle, a, G, (forward, back))), (G, forward, back)


@pytest.mark.parametrize("G", [4, 8])
def test_two_shard_sets_interleaved(group, wanted, oracle, G):
    """A, B, A, B (fft, fft, ifft, ifft) with no synchronisation: each call fills the group's receive buffers again while the other set's
    copies are in flight, and each inverse reads what the forward call left in its own set (see the test above for the expectation)."""
    M, devs = group(G)
    a, _ = wanted(0x4400 + G, LG, FFT)
    b, _ = wanted(0x4500 + G, LG, FFT)
    sa, sb = _shards_to_devices(a, devs), _shards_to_devices(b, devs)
    for shards, op in ((sa, FFT), (sb, FFT), (sa, IFFT), (sb, IFFT)):
        resident(M, shards, LG, op)
    M.ck(M.lib.bbg_multi_sync(M.h))
    assert np.array_equal(gathered(oracle, sa, LG), composed(oracle, a, G, (FFT, IFFT))), (G, "set A")
    assert np.array_equal(gathered(oracle, sb, LG), composed(oracle, b, G, (FFT, IFFT))), (G, "set B")


@pytest.mark.parametrize("G", [4, 8])
def test_buffer_growth_between_queued_calls(pkg, wanted, oracle, G):
    """2^6, 2^10, 2^6 queued in a row on a FRESH group: the second call grows the group's buffers while the first is in flight."""
    devs = _spread(pkg, G)
    M = _Multi(pkg, devs)
    try:
        runs = []
        for seed, lg, op in ((0x4600, 6, FFT), (0x4601, 10, COSET_FFT), (0x4602, 6, IFFT)):
            a, want = wanted(seed + G, lg, op)
            shards = _shards_to_devices(a, devs)
            runs.append((shards, lg, op, want))
        for shards, lg, op, _ in runs:
            resident(M, shards, lg, op)
        M.ck(M.lib.bbg_multi_sync(M.h))
        for shards, lg, op, want in runs:
            assert np.array_equal(gathered(oracle, shards, lg), want), (G, lg, op)
    finally:
        M.close()


@pytest.mark.parametrize("G", [4, 8])
def test_host_form_behind_an_unsynchronised_resident_call(group, wanted, oracle, G):
    M, devs = group(G)
    a, fa = wanted(0x4700 + G, LG, COSET_FFT)
    b, fb_ = wanted(0x4701 + G, LG, FFT)
    shards = _shards_to_devices(a, devs)
    resident(M, shards, LG, COSET_FFT)
    got = host_form(M, b, LG, FFT)
    M.ck(M.lib.bbg_multi_sync(M.h))
    assert np.array_equal(oracle.canon(0, got), fb_), (G, "host form")
    assert np.array_equal(gathered(oracle, shards, LG), fa), (G, "resident form")


@pytest.mark.parametrize("G", [4, 8])
def test_msm_between_two_resident_calls(group, wanted, oracle, G):
    M, devs = group(G)
    rng = rng_for("between", G)
    n = 2 * G + 1
    ks, ss = material(rng, n), fresh_scalars(rng, n)
    pts = register(M, oracle, ks)
    a, fa = wanted(0x4800 + G, LG, FFT)
    b, fb_ = wanted(0x4801 + G, LG, COSET_IFFT)
    sa, sb = _shards_to_devices(a, devs), _shards_to_devices(b, devs)
    resident(M, sa, LG, FFT)
    assert check_msm(M, oracle, pts, ks, ss, what=("between resident calls", G)) != 0
    resident(M, sb, LG, COSET_IFFT)
    M.ck(M.lib.bbg_multi_sync(M.h))
    assert np.array_equal(gathered(oracle, sa, LG), fa), (G, "before the MSM")
    assert np.array_equal(gathered(oracle, sb, LG), fb_), (G, "behind the MSM")


@pytest.mark.parametrize("G", [4, 8])
def test_single_context_transform_between_two_resident_calls(group, pkg, wanted, oracle, G):
    """bbg_ntt_device at the shard size n / G on bbg_multi_ctx(m, g), on a buffer of the test's own: it shares that context's stream,
    domain tables and scratch with the group calls around it."""
    import torch
    M, devs = group(G)
    lgm = LG - (G.bit_length() - 1)
    a, fa = wanted(0x4900 + G, LG, FFT)
    b, fb_ = wanted(0x4901 + G, LG, IFFT)
    sa, sb = _shards_to_devices(a, devs), _shards_to_devices(b, devs)
    own = {}
    for g in (0, G - 1):
        x, fx = wanted(0x4910 + G + g, lgm, FFT)
        t = torch.from_numpy(np.array(x).view(np.int64).reshape(-1)).to(f"cuda:{devs[g]}")
        torch.cuda.synchronize(devs[g])
        own[g] = (t, fx)
    resident(M, sa, LG, FFT)
    for g, (t, _) in own.items():
        ctx = M.lib.bbg_multi_ctx(M.h, g)
        assert ctx
        M.ck(M.lib.bbg_ntt_device(ctx, ctypes.c_void_p(t.data_ptr()), lgm, FFT, 0, None))
    resident(M, sb, LG, IFFT)
    M.ck(M.lib.bbg_multi_sync(M.h))
    assert np.array_equal(gathered(oracle, sa, LG), fa), (G, "before")
    assert np.array_equal(gathered(oracle, sb, LG), fb_), (G, "behind")
    for g, (t, fx) in own.items():
        assert np.array_equal(oracle.canon(0, t.cpu().numpy().view(np.uint64).reshape(-1, 4)), fx), (G, g, "the context's own transform")


# ------------------------------------------------------------------------------------------------ NTT: completion behind bbg_multi_sync
@pytest.mark.parametrize("op", [FFT, COSET_IFFT])
@pytest.mark.parametrize("G", [4, 8])
def test_multi_sync_alone_completes_a_resident_call(group, wanted, oracle, G, op):
    import torch
    M, devs = group(G)
    lg = 12
    a, want = wanted(0x4A00 + G, lg, op)
    masters = _shards_to_devices(a, devs)
    # first pass: first-use work (domain tables, the group's buffers and their growth, which synchronises the devices)
    resident(M, [m.clone() for m in masters], lg, op)
    M.ck(M.lib.bbg_multi_sync(M.h))
    for d in set(devs):
        torch.cuda.synchronize(d)
    # checked pass
    side = [torch.cuda.Stream(device=d) for d in devs]
    assert all(s.cuda_stream != 0 for s in side)
    shards = [torch.full_like(m, POISON * 0x0101010101010101) for m in masters]
    for t, m in zip(shards, masters):
        t.copy_(m)  # the transform is in place: the inputs are copied into place on the device
    for d in set(devs):
        torch.cuda.synchronize(d)  # the library runs on the contexts' own streams: torch's fills are complete before anything is queued
    resident(M, shards, lg, op)
    M.ck(M.lib.bbg_multi_sync(M.h))
    snaps = []
    for t, s in zip(shards, side):
        with torch.cuda.stream(s):
            snaps.append(t.clone())
    for s in side:
        s.synchronize()
    assert np.array_equal(gathered(oracle, snaps, lg), want), (G, op)
