"""The cell handle of bbg_open_all on the MI355X (bbg_open_all_prepare_cells, csrc/open_all.hip): one KZG proof per coset of l = 2^log2cell
domain points, r = n / l proofs per call.

Every comparison is bit-exact on canonical Montgomery affine words.  Expected values come from the host model's DEFINITION route
(tests/tools/open_cells_model.py: the quotient by X^l - phi^m, then oracle.msm_naive), from the closed form over a powers string through
bbg_g1_fixed_base_mul and oracle.g1_mul, or from the existing route, the same quotient through bbg_msm.  The SRS is freed between prepare
and the first call wherever the test does not need it afterwards: the handle keeps nothing of it.

Section 5 feeds k_open_cells_sum what hashed or random inputs never give it.  Over s_j = [x^j] G and with f_(l i + b) = eps_b x^(-b) g_i the
l products it adds at one output index are [eps_b C_i S_i] G (tests/test_open_cells_cpu.py proves that from the integers): with every eps_b
= +1 all l entries of a segment are the SAME point, so every pairing is a doubling in whatever order a kernel adds; with alternating signs
each second addition cancels to infinity and the next one starts from infinity; a balanced pattern ends at infinity in all 2r segments."""
import contextlib
import ctypes
import statistics
import time

import numpy as np
import pytest

import coarse_inputs as ci
import lagrange_model as lm
import open_all_model as oa
import open_cells_model as oc

pytestmark = pytest.mark.gpu

R = oa.R_MOD
SEED = 0xBB254 + 0xCE11
X_INT = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
SHAPES = [(2, 1), (3, 1), (3, 2), (4, 2), (6, 3), (7, 6)]
LANES64 = ("batch_mul_lanes", 64, 1 << 17)
SERIAL = ("ecntt_mul", 0, 1)


@contextlib.contextmanager
def option(bbg, key, value, default):
    bbg.set_option(key, value)
    try:
        yield
    finally:
        bbg.set_option(key, default)


def optional(bbg, opt):
    return option(bbg, *opt) if opt else contextlib.nullcontext()


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
    """[k] G for plain integers k by bbg_g1_fixed_base_mul; k = 0 comes back as the affine encoding of infinity."""
    out = bbg.g1_fixed_base_mul(mont(scalars))
    for i, k in enumerate(scalars):
        assert np.array_equal(out[i], oa.aff_infinity()) == (k % R == 0)
    return out


def prepared(bbg, srs, lg, lc):
    """The handle over `srs`, which is freed before the handle is used."""
    h = bbg.open_all_prepare(srs, lg, lc)
    srs.free()
    return h


def powers(bbg, x, n):
    return bbg.srs_synth_powers(mont([x])[0], n)


@pytest.fixture(scope="module")
def hashed(bbg):
    """{(lg, lc): (points, handle)} over hashed strings (no structure), made on first use and kept for the module."""
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
    """{(lg, lc): handle} over the powers string of X_INT, made on first use and kept for the module."""
    made = {}

    def get(lg, lc):
        if (lg, lc) not in made:
            made[(lg, lc)] = prepared(bbg, powers(bbg, X_INT, 1 << lg), lg, lc)
        return made[(lg, lc)]
    yield get
    for h in made.values():
        h.free()


# 1 ------------------------------------------------------------------------------------------------ against the definition
@pytest.mark.parametrize("lg,lc", SHAPES)
def test_against_the_definition(bbg, oracle, hashed, lg, lc):
    n, r = 1 << lg, 1 << (lg - lc)
    pts, h = hashed(lg, lc)
    assert h.count == r
    f = coefficients(SEED + 100 + 16 * lg + lc, n)
    want = oc.open_cells_definition(oracle, pts, f, lc)
    words = mont(f)
    check(h.open(words), want, f"({lg}, {lc}), canonical coefficients")
    lifted = ci.add_int(words, R)
    assert ci.below(lifted, 2 * R).all() and not ci.below(lifted, R).any()
    check(h.open(lifted), want, f"({lg}, {lc}), coefficients in [r, 2r)")
    # the device entry, coefficients left untouched, nothing written past the r proofs
    d_c, d_o = bbg.dev_alloc(n * 32), bbg.dev_alloc((r + 1) * 64)
    try:
        bbg.dev_upload(d_c, lifted)
        guard = np.full((r + 1, 8), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        bbg.dev_upload(d_o, guard)
        h.open_device(d_c, d_o)
        got = bbg.dev_download(d_o, (r + 1, 8))
        check(got[:r], want, f"({lg}, {lc}), device entry")
        assert np.array_equal(got[r], guard[r]), "the device entry wrote past its r proofs"
        assert np.array_equal(bbg.dev_download(d_c, (n, 4)), lifted), "the coefficients were written"
    finally:
        bbg.dev_free(d_c)
        bbg.dev_free(d_o)


# 2 ------------------------------------------------------------------------------------------------ closed form at size
@pytest.fixture(scope="module")
def closed_form(bbg):
    """{(lg, lc): (coefficient words, scalars k_m, [k_m] G by bbg_g1_fixed_base_mul)} over the powers string of X_INT, computed once."""
    made = {}

    def get(lg, lc):
        if (lg, lc) not in made:
            f = coefficients(SEED + 200 + 16 * lg + lc, 1 << lg)
            ks = oc.cell_closed_form_scalars(f, X_INT, lc)
            made[(lg, lc)] = (mont(f), ks, bbg.g1_fixed_base_mul(mont(ks)))
        return made[(lg, lc)]
    return get


@pytest.mark.parametrize("lg,lc,opt", [(12, 6, None), (16, 6, None), (12, 1, None), (10, 9, None), (12, 6, LANES64), (12, 6, SERIAL)],
                         ids=["12-6", "16-6", "12-1", "10-9", "12-6-lanes64", "12-6-ecntt_mul0"])
def test_closed_form_over_a_powers_string(bbg, oracle, closed_form, lg, lc, opt):
    """(10, 9) has r = 2: four segments of 512 entries each."""
    n, r = 1 << lg, 1 << (lg - lc)
    assert lm.root(oracle, lg) == ci.root_of_unity(lg)
    words, ks, want = closed_form(lg, lc)
    with optional(bbg, opt):
        h = prepared(bbg, powers(bbg, X_INT, n), lg, lc)
        try:
            assert h.count == r
            got = h.open(words)
        finally:
            h.free()
    check(got, want, f"({lg}, {lc}), {opt}")
    if opt is None:
        G = oracle.g1_generator()
        rng = np.random.default_rng(SEED + lg)
        for m in list(dict.fromkeys([0, r - 1] + [int(v) for v in rng.integers(0, r, 14)])):
            assert np.array_equal(got[m], oa.canon_points(oracle, oracle.g1_mul(G, mont([ks[m]])[0]))[0]), f"({lg}, {lc}): proof {m} != [k_m] G"


# 3 ------------------------------------------------------------------------------------------------ the existing route
def test_agrees_with_quotient_and_msm(bbg):
    lg, lc = 12, 6
    n, l = 1 << lg, 1 << lc
    r = n // l
    srs = bbg.srs_synth_hashed(SEED + 300, n)
    try:
        h = bbg.open_all_prepare(srs, lg, lc)
        try:
            f = coefficients(SEED + 301, n)
            got = h.open(mont(f))
        finally:
            h.free()
        phi = pow(ci.root_of_unity(lg), l, R)
        rng = np.random.default_rng(SEED + 302)
        for m in [0, r - 1] + [int(v) for v in rng.integers(1, r - 1, 6)]:
            q = oc.cell_quotient_coeffs(f, l, pow(phi, m, R))
            want = bbg.g1_normalize(bbg.msm(srs, mont(q + [0] * l)))[0]
            assert np.array_equal(got[m], want), f"proof {m} differs from the quotient by X^l - phi^m through bbg_msm"
    finally:
        srs.free()


# 4 ------------------------------------------------------------------------------------------------ log2cell = 0
def test_log2cell_zero_is_bbg_open_all_prepare(bbg, pkg):
    lg = 6
    n = 1 << lg
    srs = bbg.srs_synth_hashed(SEED + 400, n)
    a = b = None
    try:
        a = bbg.open_all_prepare(srs, lg)
        raw = ctypes.c_void_p()
        assert bbg.lib.bbg_open_all_prepare_cells(bbg.ctx, srs.handle, lg, 0, ctypes.byref(raw)) == 0
        b = pkg.binding.OpenAll(bbg, raw, lg)
        srs.free()
        assert a.count == b.count == n
        assert a.device_bytes() == b.device_bytes() == 576 * n
        for seed in (401, 402):
            words = mont(coefficients(SEED + seed, n))
            check(b.open(words), a.open(words), "log2cell = 0 against bbg_open_all_prepare")
    finally:
        for h in (a, b):
            if h is not None:
                h.free()
        srs.free()


# 5 ------------------------------------------------------------------------------------------------ the segment sum's special cases
def signs(kind, l, seed):
    rng = np.random.default_rng(seed)
    if kind == "plus":
        return [1] * l
    if kind == "alternating":
        return [1, -1] * (l // 2)
    if kind == "halves":
        return [1] * (l // 2) + [-1] * (l // 2)
    e = [1] * (l // 2) + [-1] * (l // 2) if kind == "balanced" else [1] * (l // 2 + 1) + [-1] * (l // 2 - 1)
    rng.shuffle(e)
    return [int(v) for v in e]


@pytest.mark.parametrize("lg,lc", [(8, 4), (9, 6)])
def test_segment_sums_of_equal_opposite_and_infinite_points(bbg, over_powers, lg, lc):
    n, l = 1 << lg, 1 << lc
    r = n // l
    h = over_powers(lg, lc)
    g = coefficients(SEED + 500 + lg, r)
    C, S = oc.designed_factors(g, X_INT, lc)
    assert sum(1 for c, s in zip(C, S) if c * s % R) == 2 * r  # every segment adds l finite points
    for kind in ("plus", "alternating", "halves", "balanced", "unbalanced"):
        eps = signs(kind, l, SEED + 510 + lg)
        f = oc.designed_coeffs(g, X_INT, eps, lc)
        ks = oc.cell_closed_form_scalars(f, X_INT, lc)
        if kind in ("alternating", "halves", "balanced"):
            assert sum(eps) == 0 and not any(ks)
        else:
            assert all(ks)
        check(h.open(mont(f)), fixed(bbg, ks), f"({lg}, {lc}), eps = {kind}")
    check(h.open(mont([0] * n)), infinities(r), f"({lg}, {lc}), f = 0")
    check(h.open(ci.to_words([R] * n)), infinities(r), f"({lg}, {lc}), f = 0 written as r")
    low = coefficients(SEED + 520 + lg, l) + [0] * (n - l)
    check(h.open(mont(low)), infinities(r), f"({lg}, {lc}), only f_0 .. f_(l-1) non-zero")
    c = coefficients(SEED + 530 + lg, 1)[0]
    check(h.open(mont([0] * l + [c] + [0] * (n - l - 1))), np.tile(fixed(bbg, [c]), (r, 1)), f"({lg}, {lc}), f = c X^l: every proof is [c] s_0")


# 6 ------------------------------------------------------------------------------------------------ degenerate strings
def test_degenerate_powers_strings(bbg, oracle):
    """x on the domains the transforms run over: the closed form's denominator vanishes for some, ŝ_hat has infinite entries, and
    butterflies meet equal and opposite points in both sets of stages.  Held to the definition on the oracle and to the integers."""
    lg, lc = 6, 3
    n, l = 1 << lg, 1 << lc
    r = n // l
    w = ci.root_of_unity(lg)
    bases = {"1": 1, "-1": R - 1, "w_n": w, "w_n^-1": pow(w, R - 2, R), "w_2n": ci.root_of_unity(lg + 1), "w_2r": ci.root_of_unity(lg - lc + 1)}
    fs = {"ones": [1] * n, "alternating": [1, R - 1] * (n // 2), "random": coefficients(SEED + 600, n)}
    phi = pow(w, l, R)
    for name, x in bases.items():
        srs = powers(bbg, x, n)
        pts = srs.read()
        h = prepared(bbg, srs, lg, lc)
        try:
            got = {p: h.open(mont(f)) for p, f in fs.items()}
        finally:
            h.free()
        for p, f in fs.items():
            check(got[p], oc.open_cells_definition(oracle, pts, f, lc), f"x = {name}, f = {p}, against the definition")
            ks = [oc.horner(oc.cell_quotient_coeffs(f, l, pow(phi, m, R)), x) for m in range(r)]
            check(got[p], fixed(bbg, ks), f"x = {name}, f = {p}, against [q_m(x)] G")


# 7 ------------------------------------------------------------------------------------------------ one handle, degenerate calls between
def test_reuse_after_degenerate_calls(bbg, over_powers):
    lg, lc = 8, 4
    n, l = 1 << lg, 1 << lc
    r = n // l
    h = over_powers(lg, lc)
    f1 = coefficients(SEED + 700, n)
    f2 = oc.designed_coeffs(coefficients(SEED + 701, r), X_INT, signs("balanced", l, SEED + 702), lc)
    first = h.open(mont(f1))
    check(first, fixed(bbg, oc.cell_closed_form_scalars(f1, X_INT, lc)), "a random f")
    check(h.open(mont(f2)), infinities(r), "a designed f behind it: every segment cancels")
    check(h.open(mont([0] * n)), infinities(r), "f = 0 behind that")
    check(h.open(mont(f1)), first, "the first f again")


# 8 ------------------------------------------------------------------------------------------------ errors
def test_errors(bbg, pkg):
    srs = bbg.srs_synth_hashed(SEED + 800, 16)
    other = None
    try:
        sentinel = 0x5E17117E1
        prepare = bbg.lib.bbg_open_all_prepare_cells
        # log2cell = log2n, log2cell > log2n (twice), log2n out of range, 32 > the 16 points the string holds
        for lg, lc in ((4, 4), (4, 5), (3, 31), (0, 1), (28, 2), (5, 2)):
            out = ctypes.c_void_p(sentinel)
            assert prepare(bbg.ctx, srs.handle, lg, lc, ctypes.byref(out)) == -1 and bbg.lib.bbg_last_error()
            assert out.value == sentinel, "*out was written on the error path"
            with pytest.raises(pkg.BbgError):
                bbg.open_all_prepare(srs, lg, lc)
        out = ctypes.c_void_p(sentinel)
        assert prepare(bbg.ctx, None, 4, 2, ctypes.byref(out)) == -1 and out.value == sentinel
        assert prepare(bbg.ctx, srs.handle, 4, 2, None) == -1
        assert prepare(None, srs.handle, 4, 2, ctypes.byref(out)) == -1 and out.value == sentinel
        if bbg.lib.bbg_device_count() > 1:  # a string on another device
            other = pkg.Bbg(1)
            far = other.srs_synth_hashed(SEED + 801, 16)
            try:
                assert prepare(bbg.ctx, far.handle, 4, 2, ctypes.byref(out)) == -1 and out.value == sentinel
            finally:
                far.free()
        count = ctypes.c_size_t(7)
        assert bbg.lib.bbg_open_all_count(None, ctypes.byref(count)) == -1 and count.value == 7
        h = bbg.open_all_prepare(srs, 4, 3)  # n = num_points exactly and two cells are legal
        try:
            assert bbg.lib.bbg_open_all_count(h.handle, None) == -1
            assert h.count == 2 and h.device_bytes() == 2 * 16 * 64 + 2 * 16 * 128 + 2 * 16 * 32 + 4 * 128 + 2 * 128
            with pytest.raises(ValueError):
                h.open(np.zeros((8, 4), dtype=np.uint64))
        finally:
            h.free()
    finally:
        srs.free()
        if other is not None:
            other.close()


# 9 ------------------------------------------------------------------------------------------------ one relative time bound
def test_cells_are_no_slower_than_all_points_at_2_12(bbg):
    """A cell call at (12, 6) runs 7 + 6 dependent G1 stages where the all-points call at 2^12 runs 13 + 12, the same 2^13 products, plus 64
    Fr transforms of 128 points and the segment sums: the median of 9 cell calls may not exceed the median of 9 all-points calls, both
    handles alive in one process.  1.0 x, no margin: a cell call that is slower has no reason to exist at this size."""
    lg, lc = 12, 6
    n = 1 << lg
    srs = bbg.srs_synth_hashed(SEED + 900, n)
    cells = points = d_c = d_o = None
    try:
        cells = bbg.open_all_prepare(srs, lg, lc)
        points = bbg.open_all_prepare(srs, lg)
        d_c, d_o = bbg.dev_alloc(n * 32), bbg.dev_alloc(n * 64)
        bbg.dev_upload(d_c, mont(coefficients(SEED + 901, n)))

        def median(h):
            h.open_device(d_c, d_o)  # warm-up
            bbg.sync()
            ts = []
            for _ in range(9):
                t0 = time.perf_counter()
                h.open_device(d_c, d_o)
                bbg.sync()
                ts.append(time.perf_counter() - t0)
            return statistics.median(ts)

        all_points = median(points)
        mine = median(cells)
        print(f"open cells (12, 6): {mine * 1e3:.2f} ms; open all 2^12: {all_points * 1e3:.2f} ms; ratio {mine / all_points:.3f}")
        assert mine <= all_points, f"the cell call at (12, 6) took {mine * 1e3:.2f} ms, the all-points call at 2^12 {all_points * 1e3:.2f} ms"
    finally:
        for h in (cells, points):
            if h is not None:
                h.free()
        for d in (d_c, d_o):
            if d is not None:
                bbg.dev_free(d)
        srs.free()
