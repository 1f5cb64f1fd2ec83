"""The batched calls of bbg_open_all on the MI355X (bbg_open_all_batch_reserve / _batch_device / _batch, csrc/open_all.hip):
the proofs of many polynomials over one string per call, on the all-points handle and on the cell handle.

Every comparison is bit-exact on canonical Montgomery affine words.  Expected values come from single calls through the same handle, from
the host models' DEFINITION routes on the oracle (tests/tools/open_all_model.py, open_cells_model.py), and over a powers string from the
closed forms through bbg_g1_fixed_base_mul.  A batch mixes, in this order, a random polynomial written in [r, 2r), the zero polynomial, a
repeat of the first (canonical this time) and further random ones; a batch of k takes the first k."""
import contextlib
import ctypes
import statistics
import time

import numpy as np
import pytest

import coarse_inputs as ci
import open_all_model as oa
import open_batch_model as ob
import open_cells_model as oc

pytestmark = pytest.mark.gpu

R = oa.R_MOD
SEED = 0xBB254 + 0xBA7C
X_INT = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
SHAPES = [(2, 1), (3, 1), (3, 2), (4, 2), (6, 3), (7, 6), (1, 0), (2, 0), (3, 0), (6, 0)]
COUNTS = (1, 2, 3, 5)
LANES64 = ("batch_mul_lanes", 64, 1 << 17)
SERIAL = ("ecntt_mul", 0, 1)


@contextlib.contextmanager
def option(bbg, key, value, default):
    bbg.set_option(key, value)
    try:
        yield
    finally:
        bbg.set_option(key, default)


def mont(vals):
    return ci.to_words([ci.to_mont(v % R, 0) for v in vals])


def coefficients(seed, n):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(32), "little") % R for _ in range(n)]


def infinities(n):
    return np.tile(oa.aff_infinity(), (n, 1))


def check(got, want, what):
    assert np.asarray(got).shape == np.asarray(want).shape, f"{what}: {np.asarray(got).shape} proofs, expected {np.asarray(want).shape}"
    bad = np.flatnonzero((np.asarray(got) != np.asarray(want)).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(want)} proofs differ, first at {bad[:8]}"


def fixed(bbg, scalars):
    """[k] G for plain integers k by bbg_g1_fixed_base_mul."""
    return bbg.g1_fixed_base_mul(mont(scalars))


def mixed_batch(seed, n):
    """(integers, words) of the five polynomials of a batch: random (written in [r, 2r)), zero, the first again (canonical), random, random."""
    a, d, e = (coefficients(seed + k, n) for k in range(3))
    ints = [a, [0] * n, a, d, e]
    words = np.stack([mont(f) for f in ints])
    words[0] = ci.add_int(words[0], R)
    assert ci.below(words[0], 2 * R).all() and not ci.below(words[0], R).any()
    return ints, words


def definition(oracle, pts, f, lc):
    return oc.open_cells_definition(oracle, pts, f, lc) if lc else oa.open_all_definition(oracle, pts, f)


def prepared(bbg, srs, lg, lc):
    h = bbg.open_all_prepare(srs, lg, lc)
    srs.free()
    return h


@pytest.fixture(scope="module")
def hashed(bbg):
    """{(lg, lc): (points, handle)} over hashed strings, made on first use and kept for the module."""
    made = {}

    def get(lg, lc):
        if (lg, lc) not in made:
            srs = bbg.srs_synth_hashed(SEED + 16 * lg + lc, 1 << lg)
            pts = srs.read()
            made[(lg, lc)] = (pts, prepared(bbg, srs, lg, lc))
        return made[(lg, lc)]
    yield get
    for _, h in made.values():
        h.free()


@pytest.fixture(scope="module")
def over_powers(bbg):
    """{(lg, lc): handle} over the powers string of X_INT."""
    made = {}

    def get(lg, lc):
        if (lg, lc) not in made:
            made[(lg, lc)] = prepared(bbg, bbg.srs_synth_powers(mont([X_INT])[0], 1 << lg), lg, lc)
        return made[(lg, lc)]
    yield get
    for h in made.values():
        h.free()


@pytest.fixture(scope="module")
def reference(bbg, oracle, hashed):
    """{(lg, lc): (words, expected)}: the mixed batch of a shape and its proofs by the definition on the oracle, (5, proofs, 8), computed once
    and never written."""
    made = {}

    def get(lg, lc):
        if (lg, lc) not in made:
            pts, _ = hashed(lg, lc)
            ints, words = mixed_batch(SEED + 100 + 16 * lg + lc, 1 << lg)
            by_poly = {}
            for f in ints:
                if tuple(f) not in by_poly:
                    by_poly[tuple(f)] = definition(oracle, pts, f, lc)
            want = np.stack([by_poly[tuple(f)] for f in ints])
            words.setflags(write=False)
            want.setflags(write=False)
            made[(lg, lc)] = (words, want)
        return made[(lg, lc)]
    return get


def check_batch(h, words, want, what, singles=True):
    """open_batch on `words` against `want`, and against single calls through the same handle."""
    got = h.open_batch(words)
    assert got.shape == (len(words), h.count, 8)
    for p in range(len(words)):
        check(got[p], want[p], f"{what}, polynomial {p} of {len(words)}")
        if singles:
            check(got[p], h.open(words[p]), f"{what}, polynomial {p} of {len(words)} against the single call")
    return got


# 1 ------------------------------------------------------------------------------------------------ against single calls and the definition
@pytest.mark.parametrize("lg,lc", SHAPES)
def test_against_single_calls_and_the_definition(bbg, hashed, reference, lg, lc):
    n, proofs = 1 << lg, 1 << (lg - lc)
    _, h = hashed(lg, lc)
    words, want = reference(lg, lc)
    check(want[1], infinities(proofs), "the zero polynomial by the definition")
    check(want[2], want[0], "the repeated polynomial by the definition")
    for count in COUNTS:
        check_batch(h, words[:count], want, f"({lg}, {lc})")
    # the device entry: the coefficients are left as they were, nothing is written past count x proofs
    count = 5
    d_c, d_o = bbg.dev_alloc(count * n * 32), bbg.dev_alloc((count * proofs + 1) * 64)
    try:
        bbg.dev_upload(d_c, words.reshape(-1, 4))
        guard = np.full((count * proofs + 1, 8), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        bbg.dev_upload(d_o, guard)
        h.open_batch_device(d_c, count, d_o)
        got = bbg.dev_download(d_o, (count * proofs + 1, 8))
        check(got[:-1], want.reshape(-1, 8), f"({lg}, {lc}), device entry")
        assert np.array_equal(got[-1], guard[-1]), "the device entry wrote past its count x proofs points"
        assert np.array_equal(bbg.dev_download(d_c, (count * n, 4)), words.reshape(-1, 4)), "the coefficients were written"
    finally:
        bbg.dev_free(d_c)
        bbg.dev_free(d_o)
        h.reserve_batch(0)


# 2 ------------------------------------------------------------------------------------------------ chunking and the reservation
@pytest.mark.parametrize("lg,lc", [(6, 3), (6, 0)])
def test_chunks_and_the_reservation(bbg, hashed, reference, lg, lc):
    words, want = reference(lg, lc)
    srs = bbg.srs_synth_hashed(SEED + 16 * lg + lc, 1 << lg)  # the string of `hashed`, a handle of this test's own
    h = prepared(bbg, srs, lg, lc)
    try:
        bare = ob.handle_bytes(lg, lc)
        assert h.device_bytes() == bare, "a handle that never reserved reports more than its own buffers"
        first = h.open(words[3])
        check(first, want[3], "a single call before any batch")
        h.reserve_batch(2)
        assert h.device_bytes() == bare + 2 * ob.poly_bytes(lg, lc)
        check_batch(h, words, want, f"({lg}, {lc}), chunks 2 2 1", singles=False)
        assert h.device_bytes() == bare + 2 * ob.poly_bytes(lg, lc), "a batched call changed the reservation"
        check(h.open(words[3]), first, "a single call after a batched one")
        h.reserve_batch(1)
        assert h.device_bytes() == bare + ob.poly_bytes(lg, lc)
        check_batch(h, words[:3], want, f"({lg}, {lc}), chunks 1 1 1", singles=False)
        h.reserve_batch(0)
        assert h.device_bytes() == bare
        check_batch(h, words, want, f"({lg}, {lc}), reserved by the call", singles=False)  # a batched call after a single one, no reservation
        assert h.device_bytes() == bare + 5 * ob.poly_bytes(lg, lc)
        h.reserve_batch(1 << 40)  # above the cap: the cap
        assert h.device_bytes() == bare + ob.batch_cap(lg, lc) * ob.poly_bytes(lg, lc) <= bare + ob.BUDGET
        check_batch(h, words, want, f"({lg}, {lc}), the cap reserved", singles=False)
        h.reserve_batch(0)
        assert h.device_bytes() == bare
    finally:
        h.free()


# 3 ------------------------------------------------------------------------------------------------ launch shapes
@pytest.mark.parametrize("lg,lc,count", [(6, 3, 5), (8, 4, 3)])
@pytest.mark.parametrize("opt", [LANES64, SERIAL], ids=["lanes64", "ecntt_mul0"])
def test_launch_shapes(bbg, hashed, reference, lg, lc, count, opt):
    """64 lanes: every lane loops over products and butterflies and its items cross polynomial borders.  ecntt_mul = 0: the bit-serial
    stage kernel over the blocks."""
    _, h = hashed(lg, lc)
    words, want = reference(lg, lc)
    single = [h.open(words[p]) for p in range(count)]
    try:
        with option(bbg, *opt):
            got = check_batch(h, words[:count], want, f"({lg}, {lc}) x {count}, {opt[0]} = {opt[1]}", singles=False)
        for p in range(count):
            check(got[p], single[p], f"({lg}, {lc}) x {count}, {opt[0]} = {opt[1]}, polynomial {p} against the single call")
    finally:
        h.reserve_batch(0)


# 4 ------------------------------------------------------------------------------------------------ the LDS transform's edges
@pytest.mark.parametrize("lg,lc", [(5, 4), (ob.LDS_LOG2, 1), (ob.LDS_LOG2 + 1, 1), (ob.LDS_LOG2 - 1, 0)],
                         ids=["2r=4", "2r=largest-in-LDS", "2r=first-fallback", "2n=largest-in-LDS"])
def test_lds_transform_edges(bbg, lg, lc):
    """2r = 4 is the smallest block there is; 2r = 2^12 the largest the LDS kernel takes (128 KiB), 2^13 the first that goes through the
    single call's transforms block by block; (11, 0) is the all-points handle at the kernel's largest 2n.  Two polynomials each, against
    single calls."""
    n = 1 << lg
    h = prepared(bbg, bbg.srs_synth_hashed(SEED + 400 + lg, n), lg, lc)
    try:
        words = np.stack([mont(coefficients(SEED + 410 + lg + k, n)) for k in range(2)])
        got = h.open_batch(words)
        for p in range(2):
            check(got[p], h.open(words[p]), f"({lg}, {lc}), polynomial {p}")
    finally:
        h.free()


# 5 ------------------------------------------------------------------------------------------------ closed form at size
@pytest.mark.parametrize("lg,lc,count", [(12, 6, 16), (12, 0, 4)], ids=["12-6-x16", "12-0-x4"])
def test_closed_form_over_a_powers_string(bbg, over_powers, lg, lc, count):
    n, proofs = 1 << lg, 1 << (lg - lc)
    h = over_powers(lg, lc)
    fs = [coefficients(SEED + 500 + 16 * lg + lc + k, n) for k in range(count)]
    if lc:
        ks = [oc.cell_closed_form_scalars(f, X_INT, lc) for f in fs]
    else:
        ks = [oa.closed_form_scalars(f, X_INT, ci.root_of_unity(lg)) for f in fs]
    want = fixed(bbg, [k for row in ks for k in row]).reshape(count, proofs, 8)
    try:
        got = h.open_batch(np.stack([mont(f) for f in fs]))
        for p in range(count):
            check(got[p], want[p], f"({lg}, {lc}) x {count}, polynomial {p} against [k_m] G")
    finally:
        h.reserve_batch(0)


# 6 ------------------------------------------------------------------------------------------------ degenerate sums across a batch
def signs(kind, l, seed):
    rng = np.random.default_rng(seed)
    if kind == "plus":
        return [1] * l
    if kind == "alternating":
        return [1, -1] * (l // 2)
    e = [1] * (l // 2) + [-1] * (l // 2) if kind == "balanced" else [1] * (l // 2 + 1) + [-1] * (l // 2 - 1)
    rng.shuffle(e)
    return [int(v) for v in e]


def test_segment_sums_of_equal_opposite_and_infinite_points_across_a_batch(bbg, over_powers):
    """One polynomial per kind of sign pattern in ONE batch: segments of equal points beside segments that cancel pairwise and segments
    that end at infinity, in neighbouring polynomials of one launch."""
    lg, lc = 8, 4
    n, l = 1 << lg, 1 << lc
    r = n // l
    h = over_powers(lg, lc)
    g = coefficients(SEED + 600, r)
    C, S = oc.designed_factors(g, X_INT, lc)
    assert sum(1 for c, s in zip(C, S) if c * s % R) == 2 * r  # every segment adds l finite points
    kinds = ("plus", "alternating", "balanced", "unbalanced")
    fs = [oc.designed_coeffs(g, X_INT, signs(kind, l, SEED + 610), lc) for kind in kinds]
    ks = [oc.cell_closed_form_scalars(f, X_INT, lc) for f in fs]
    assert all(ks[0]) and not any(ks[1]) and not any(ks[2]) and all(ks[3])
    try:
        got = h.open_batch(np.stack([mont(f) for f in fs]))
        for p, kind in enumerate(kinds):
            check(got[p], fixed(bbg, ks[p]), f"eps = {kind}")
            check(got[p], h.open(mont(fs[p])), f"eps = {kind}, against the single call")
    finally:
        h.reserve_batch(0)


# 7 ------------------------------------------------------------------------------------------------ errors
def test_errors(bbg, hashed):
    lg, lc = 4, 2
    n, proofs = 1 << lg, 1 << (lg - lc)
    _, h = hashed(lg, lc)
    lib = bbg.lib
    words = np.stack([mont(coefficients(SEED + 700 + k, n)) for k in range(2)])
    out = np.full((2, proofs, 8), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    untouched = out.copy()
    d_c, d_o = bbg.dev_alloc(2 * n * 32), bbg.dev_alloc(2 * proofs * 64)
    try:
        bbg.dev_upload(d_c, words.reshape(-1, 4))
        bbg.dev_upload(d_o, out.reshape(-1, 8))
        vp = ctypes.c_void_p
        for args in ((None, words.ctypes.data, 2, out.ctypes.data), (h.handle, None, 2, out.ctypes.data), (h.handle, words.ctypes.data, 2, None),
                     (h.handle, words.ctypes.data, 0, out.ctypes.data)):
            assert lib.bbg_open_all_batch(args[0], vp(args[1]), args[2], vp(args[3])) == -1 and lib.bbg_last_error()
        assert np.array_equal(out, untouched), "the output was written on an error path"
        for args in ((None, d_c, 2, d_o), (h.handle, None, 2, d_o), (h.handle, d_c, 2, None), (h.handle, d_c, 0, d_o)):
            assert lib.bbg_open_all_batch_device(args[0], vp(args[1]), args[2], vp(args[3])) == -1 and lib.bbg_last_error()
        bbg.sync()
        assert np.array_equal(bbg.dev_download(d_o, (2 * proofs, 8)), untouched.reshape(-1, 8)), "the device output was written on an error path"
        assert lib.bbg_open_all_batch_reserve(None, 2) == -1 and lib.bbg_last_error()
        with pytest.raises(ValueError):
            h.open_batch(np.zeros((2, n - 1, 4), dtype=np.uint64))
        with pytest.raises(ValueError):
            h.open_batch(np.zeros((n, 4), dtype=np.uint64))
        got = h.open_batch(words)  # and the handle works afterwards
        for p in range(2):
            check(got[p], h.open(words[p]), f"after the errors, polynomial {p}")
    finally:
        bbg.dev_free(d_c)
        bbg.dev_free(d_o)
        h.reserve_batch(0)


# 8 ------------------------------------------------------------------------------------------------ one relative time bound
def test_a_batch_of_8_is_no_slower_than_8_single_calls_at_12_6(bbg):
    """At (12, 6) a single call is 13 dependent G1 stages over 128 and 64 points; the batched call runs the same 13 launches over 8 times
    the points.  The median of 9 batched device calls of 8 polynomials may not exceed the median of 9 times 8 single device calls, one
    handle, one process, one warm-up each, on the host clock up to a synchronisation.  1.0 x, no margin: a batched call that loses to the
    loop it replaces has no reason to exist."""
    lg, lc, count = 12, 6, 8
    n, proofs = 1 << lg, 1 << (lg - lc)
    srs = bbg.srs_synth_hashed(SEED + 800, n)
    h = d_c = d_o = None
    try:
        h = bbg.open_all_prepare(srs, lg, lc)
        h.reserve_batch(count)
        d_c, d_o = bbg.dev_alloc(count * n * 32), bbg.dev_alloc(count * proofs * 64)
        bbg.dev_upload(d_c, np.concatenate([mont(coefficients(SEED + 801 + k, n)) for k in range(count)]))

        def batched():
            h.open_batch_device(d_c, count, d_o)

        def looped():
            for p in range(count):
                h.open_device(d_c + p * n * 32, d_o + p * proofs * 64)

        def median(call):
            call()  # warm-up
            bbg.sync()
            ts = []
            for _ in range(9):
                t0 = time.perf_counter()
                call()
                bbg.sync()
                ts.append(time.perf_counter() - t0)
            return statistics.median(ts)

        loop = median(looped)
        want = bbg.dev_download(d_o, (count * proofs, 8))
        mine = median(batched)
        check(bbg.dev_download(d_o, (count * proofs, 8)), want, "the timed calls")
        print(f"open batch (12, 6) x 8: {mine * 1e3:.2f} ms; 8 single calls: {loop * 1e3:.2f} ms; ratio {mine / loop:.3f}")
        assert mine <= loop, f"the batched call of 8 at (12, 6) took {mine * 1e3:.2f} ms, 8 single calls {loop * 1e3:.2f} ms"
    finally:
        if h is not None:
            h.free()
        for d in (d_c, d_o):
            if d is not None:
                bbg.dev_free(d)
        srs.free()
