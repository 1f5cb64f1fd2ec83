"""The cells of a polynomial as data on the MI355X (bbg_cells_values, bbg_cells_recover, csrc/cells.hip): the values of every cell, and the
polynomial back from a subset of its cells.

Every comparison is bit-exact on canonical Montgomery words.  Expected cell values come from the host model (tests/tools/cells_model.py: the
oracle's transform read cell by cell); a recovery is held to the coefficients the values were made from, which have degree exactly K l - 1,
so that the top kept coefficient is non-zero and everything above it must come back as zero words."""
import statistics
import time

import numpy as np
import pytest

import cells_model as cm
import coarse_inputs as ci

pytestmark = pytest.mark.gpu

R = cm.R_MOD
SEED = 0xBB254 + 0xCE115
X_INT = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
VALUE_SHAPES = [(2, 1), (3, 1), (3, 2), (4, 2), (6, 3), (7, 6), (9, 1), (13, 6)]
GUARD = 0xA5A5A5A5A5A5A5A5


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape}, expected {want.shape}"
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(want)} words differ, first at {bad[:8]}"


def lifted(words):
    out = ci.add_int(words, R)
    assert ci.below(out, 2 * R).all() and not ci.below(out, R).any()
    return out


def low_degree(seed, lg, deg_bound):
    """n integers: a random polynomial of degree exactly deg_bound - 1."""
    f = cm.random_ints(seed, deg_bound)
    f[-1] = f[-1] or 1
    return f + [0] * ((1 << lg) - deg_bound)


def shuffled(ids, seed):
    return [int(v) for v in np.random.default_rng(seed).permutation(np.asarray(ids))]


@pytest.fixture(scope="module")
def polys(oracle):
    """{(lg, lc, K, seed): (f, coefficient words, cell-major values)} of low-degree polynomials, made on first use and shared."""
    made = {}

    def get(lg, lc, K, seed=0):
        key = (lg, lc, K, seed)
        if key not in made:
            f = low_degree(SEED + 1000 * lg + 10 * lc + K + seed, lg, K << lc)
            made[key] = (f, cm.mont(f), cm.cell_values(oracle, f, lc))
        return made[key]
    return get


def recovers(bbg, polys, lg, lc, ids, what):
    K = len(ids)
    f, words, values = polys(lg, lc, K)
    got = bbg.cells_recover(ids, cm.mont(cm.known_values(values, ids, lc)), lg, lc)
    same(got, words, f"({lg}, {lc}) {what}, K = {K}")
    assert not got[K << lc:].any(), f"({lg}, {lc}) {what}: the words from K l up must be zero"


# 1 ------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("lg,lc", VALUE_SHAPES)
def test_values_against_the_model(bbg, oracle, lg, lc):
    n = 1 << lg
    fs = [cm.random_ints(SEED + 16 * lg + lc + 100 * p, n) for p in range(3)]
    want = [cm.mont(cm.cell_values(oracle, f, lc)) for f in fs]
    words = [cm.mont(f) for f in fs]
    same(bbg.cells_values(words[0], lg, lc), want[0], f"({lg}, {lc}), count 1")
    same(bbg.cells_values(np.concatenate(words), lg, lc), np.concatenate(want), f"({lg}, {lc}), count 3")
    same(bbg.cells_values(lifted(words[1]), lg, lc), want[1], f"({lg}, {lc}), coefficients in [r, 2r)")
    # the device entry: coefficients left as they are, nothing written past count x n values
    up = np.concatenate([lifted(words[0]), words[1], lifted(words[2])])
    d_c, d_o = bbg.dev_alloc(3 * n * 32), bbg.dev_alloc((3 * n + 1) * 32)
    try:
        bbg.dev_upload(d_c, up)
        bbg.dev_upload(d_o, np.full((3 * n + 1, 4), GUARD, dtype=np.uint64))
        bbg.cells_values_device(d_c, lg, lc, 3, d_o)
        got = bbg.dev_download(d_o, (3 * n + 1, 4))
        same(got[:3 * n], np.concatenate(want), f"({lg}, {lc}), device entry")
        assert (got[3 * n] == GUARD).all(), "the device entry wrote past its values"
        assert np.array_equal(bbg.dev_download(d_c, (3 * n, 4)), up), "the coefficients were written"
    finally:
        bbg.dev_free(d_c)
        bbg.dev_free(d_o)


# 2 ------------------------------------------------------------------------------------------------ recovery of a low-degree polynomial
def test_recover_smallest_shapes(bbg, polys):
    recovers(bbg, polys, 3, 1, [2], "K = 1")
    recovers(bbg, polys, 3, 1, [0, 1, 2, 3], "K = r: Z = 1")
    recovers(bbg, polys, 3, 1, [3, 0, 2, 1], "K = r, shuffled")
    for m in range(8):
        recovers(bbg, polys, 6, 3, [m], f"the single cell {m}")
    for m in range(2):
        recovers(bbg, polys, 7, 6, [m], f"the single cell {m} of two")


def missing_sets_9_1():
    r = 256
    rng = np.random.default_rng(SEED + 91)
    sets = {f"{c} missing": sorted(int(v) for v in rng.permutation(r)[:c]) for c in (1, 63, 64, 65, 130, 255)}
    sets["first half missing"] = list(range(r // 2))
    sets["second half missing"] = list(range(r // 2, r))
    sets["even cells missing"] = list(range(0, r, 2))
    sets["a random set missing"] = sorted(int(v) for v in rng.permutation(r)[:int(rng.integers(2, r - 1))])
    return sets


@pytest.mark.parametrize("name", list(missing_sets_9_1()))
def test_recover_256_cells(bbg, polys, name):
    """r = 256 cells of two points: 1 .. 255 missing cells take the lane-stride loop of k_cells_z past its first round (> 64 roots), leave
    waves partly filled (63, 65, 130) and need more than one block of outputs (r + K > 16)."""
    missing = set(missing_sets_9_1()[name])
    ids = [m for m in range(256) if m not in missing]
    recovers(bbg, polys, 9, 1, ids, name + ", sorted ids")
    recovers(bbg, polys, 9, 1, shuffled(ids, SEED + len(ids)), name + ", shuffled ids")


@pytest.mark.parametrize("lg,lc,K", [(12, 6, 32), (13, 6, 64), (10, 0, 512)], ids=["12-6", "13-6", "10-0"])
def test_recover_a_random_half(bbg, polys, lg, lc, K):
    r = 1 << (lg - lc)
    ids = shuffled(range(r), SEED + lg)[:K]
    recovers(bbg, polys, lg, lc, sorted(ids), "a random half, sorted ids")
    recovers(bbg, polys, lg, lc, ids, "a random half, shuffled ids")


# 3 ------------------------------------------------------------------------------------------------ values of no low-degree polynomial
@pytest.mark.parametrize("lg,lc", [(6, 3), (9, 4)])
def test_inconsistent_values_give_the_interpolant(bbg, lg, lc):
    n, l, r = cm.shape(lg, lc)
    K = r // 2
    ids = shuffled(range(r), SEED + 30 + lg)[:K]
    known = cm.mont(cm.random_ints(SEED + 31 + lg, K * l))
    got = bbg.cells_recover(ids, known, lg, lc)
    assert got[:K * l].any() and not got[K * l:].any(), "the top n - K l coefficients must be zero words"
    back = bbg.cells_values(got, lg, lc).reshape(r, l, 4)
    same(np.concatenate([back[m] for m in ids]), known, f"({lg}, {lc}): the interpolant on the known cells")


# 4 ------------------------------------------------------------------------------------------------ count, lifted values
def test_count_and_lifted_values(bbg, polys):
    lg, lc = 9, 4
    n, l, r = cm.shape(lg, lc)
    K = 20
    ids = shuffled(range(r), SEED + 40)[:K]
    each = [polys(lg, lc, K, seed) for seed in range(8)]
    known = [cm.mont(cm.known_values(values, ids, lc)) for _, _, values in each]
    single = [bbg.cells_recover(ids, k, lg, lc) for k in known]
    for p in range(8):
        same(single[p], each[p][1], f"polynomial {p} alone")
    for count in (3, 8):
        same(bbg.cells_recover(ids, np.concatenate(known[:count]), lg, lc), np.concatenate(single[:count]), f"count = {count}")
    same(bbg.cells_recover(ids, lifted(known[0]), lg, lc), single[0], "values in [r, 2r)")
    mixed = np.concatenate([lifted(known[0]), known[1], lifted(known[2])])
    same(bbg.cells_recover(ids, mixed, lg, lc), np.concatenate(single[:3]), "count = 3, two of them lifted")


# 5 ------------------------------------------------------------------------------------------------ one context, set after set
def test_reuse_across_sets_and_a_trim(bbg, polys):
    lg, lc = 9, 4
    n, l, r = cm.shape(lg, lc)
    a, b = shuffled(range(r), SEED + 50)[:9], shuffled(range(r), SEED + 51)[:27]
    fa, fb = polys(lg, lc, len(a)), polys(lg, lc, len(b))
    d_a, d_b, d_oa, d_ob = (bbg.dev_alloc(n * 32) for _ in range(4))
    try:
        bbg.dev_upload(d_a, cm.mont(cm.known_values(fa[2], a, lc)))
        bbg.dev_upload(d_b, cm.mont(cm.known_values(fb[2], b, lc)))
        for round_ in range(2):
            bbg.cells_recover_device(a, d_a, lg, lc, 1, d_oa)  # back to back: the second call rebuilds the tables the first one's kernels read
            bbg.cells_recover_device(b, d_b, lg, lc, 1, d_ob)
            same(bbg.dev_download(d_oa, (n, 4)), fa[1], f"round {round_}: the first set")
            same(bbg.dev_download(d_ob, (n, 4)), fb[1], f"round {round_}: the second set")
            before = bbg.memory_report()["scratch"]
            assert bbg.memory_trim() > 0 and bbg.memory_report()["scratch"] < before
    finally:
        for d in (d_a, d_b, d_oa, d_ob):
            bbg.dev_free(d)


# 6 ------------------------------------------------------------------------------------------------ end to end with the cell handle
def test_proofs_of_the_recovered_polynomial(bbg, polys):
    lg, lc = 8, 4
    n, l, r = cm.shape(lg, lc)
    K = r // 2
    f, words, values = polys(lg, lc, K)
    ids = shuffled(range(r), SEED + 60)[:K]
    srs = bbg.srs_synth_powers(cm.mont([X_INT])[0], n)
    h = d_v = d_c = d_o = None
    try:
        h = bbg.open_all_prepare(srs, lg, lc)
        want = h.open(words)
        d_v, d_c, d_o = bbg.dev_alloc(K * l * 32), bbg.dev_alloc(n * 32), bbg.dev_alloc(r * 64)
        bbg.dev_upload(d_v, cm.mont(cm.known_values(values, ids, lc)))
        bbg.cells_recover_device(ids, d_v, lg, lc, 1, d_c)
        h.open_device(d_c, d_o)
        got = bbg.dev_download(d_o, (r, 8))
        assert np.array_equal(got, want), "the cell proofs of the recovered coefficients differ from those of the original"
        # and the missing cells' values come back from the recovered coefficients
        same(bbg.cells_values(bbg.dev_download(d_c, (n, 4)), lg, lc), cm.mont(values), "every cell of the recovered polynomial")
    finally:
        if h is not None:
            h.free()
        for d in (d_v, d_c, d_o):
            if d is not None:
                bbg.dev_free(d)
        srs.free()


# 7 ------------------------------------------------------------------------------------------------ errors
def test_errors_leave_the_output_untouched(bbg, pkg):
    lg, lc = 6, 3
    n, l, r = cm.shape(lg, lc)
    lib = bbg.lib
    guard = np.full((33 * n, 4), GUARD, dtype=np.uint64)
    d_in, d_out = bbg.dev_alloc(33 * n * 32), bbg.dev_alloc(33 * n * 32)

    def u32(ids):
        return np.ascontiguousarray(ids, dtype=np.uint32)

    def untouched(what):
        bbg.sync()
        assert np.array_equal(bbg.dev_download(d_out, guard.shape), guard), f"{what}: the output was written"

    try:
        bbg.dev_upload(d_in, np.zeros_like(guard))
        bbg.dev_upload(d_out, guard)
        good = u32([1, 5, 6])
        # (ids, K, log2n, log2cell, count)
        bad = {"K = 0": (good, 0, lg, lc, 1), "K > r": (u32(list(range(r)) + [0]), r + 1, lg, lc, 1), "a duplicate id": (u32([1, 5, 1]), 3, lg, lc, 1),
               "an id = r": (u32([1, r, 2]), 3, lg, lc, 1), "log2cell = log2n": (u32([0]), 1, lg, lg, 1), "count = 0": (good, 3, lg, lc, 0),
               "count = 33": (good, 3, lg, lc, 33), "log2n = 0": (u32([0]), 1, 0, 0, 1), "log2n = 29": (good, 3, 29, lc, 1)}
        for what, (ids, K, a, b, count) in bad.items():
            assert lib.bbg_cells_recover_device(bbg.ctx, ids.ctypes.data, K, d_in, a, b, count, d_out) == -1 and lib.bbg_last_error(), what
            untouched(what)
            host = guard[:n].copy()
            assert lib.bbg_cells_recover(bbg.ctx, ids.ctypes.data, K, guard.ctypes.data, a, b, count, host.ctypes.data) == -1, what + " (host entry)"
            assert np.array_equal(host, guard[:n]), what + ": the host output was written"
        with pytest.raises(pkg.BbgError):
            bbg.cells_recover([1, 5, 1], np.zeros((3 * l, 4), dtype=np.uint64), lg, lc)
        # overlapping buffers, null pointers
        assert lib.bbg_cells_recover_device(bbg.ctx, good.ctypes.data, 3, d_out, lg, lc, 1, d_out) == -1
        assert lib.bbg_cells_recover_device(bbg.ctx, good.ctypes.data, 3, d_out + (n - 1) * 32, lg, lc, 1, d_out) == -1
        assert lib.bbg_cells_recover_device(bbg.ctx, good.ctypes.data, 3, d_out, lg, lc, 1, d_out + (3 * l - 1) * 32) == -1
        assert lib.bbg_cells_recover_device(bbg.ctx, None, 3, d_in, lg, lc, 1, d_out) == -1
        assert lib.bbg_cells_recover_device(bbg.ctx, good.ctypes.data, 3, None, lg, lc, 1, d_out) == -1
        assert lib.bbg_cells_recover_device(bbg.ctx, good.ctypes.data, 3, d_in, lg, lc, 1, None) == -1
        assert lib.bbg_cells_recover_device(None, good.ctypes.data, 3, d_in, lg, lc, 1, d_out) == -1
        untouched("overlaps and null pointers")
        for what, (a, b, count) in {"log2cell = log2n": (lg, lg, 1), "count = 0": (lg, lc, 0), "count = 33": (lg, lc, 33), "log2n = 0": (0, 0, 1)}.items():
            assert lib.bbg_cells_values_device(bbg.ctx, d_in, a, b, count, d_out) == -1, what
        assert lib.bbg_cells_values_device(bbg.ctx, d_out, lg, lc, 1, d_out) == -1
        assert lib.bbg_cells_values_device(bbg.ctx, d_out + (n - 1) * 32, lg, lc, 1, d_out) == -1
        assert lib.bbg_cells_values_device(bbg.ctx, None, lg, lc, 1, d_out) == -1
        assert lib.bbg_cells_values_device(bbg.ctx, d_in, lg, lc, 1, None) == -1
        untouched("bbg_cells_values_device")
        # the neighbours of the limits are legal: K = r, count = 32, two buffers that touch
        assert lib.bbg_cells_recover_device(bbg.ctx, u32(range(r)).ctypes.data, r, d_in, lg, lc, 32, d_out) == 0
        assert lib.bbg_cells_values_device(bbg.ctx, d_out, lg, lc, 1, d_out + n * 32) == 0
        bbg.sync()
        assert (bbg.dev_download(d_out + 32 * n * 32, (n, 4)) == GUARD).all(), "count = 32 wrote past 32 polynomials"
    finally:
        bbg.dev_free(d_in)
        bbg.dev_free(d_out)


# 8 ------------------------------------------------------------------------------------------------ one relative time bound
BOUND = 1.9


def test_recovery_at_2_12_against_three_transforms_and_an_inversion(bbg, pkg):
    """bbg_cells_recover_device at (12, 6), K = r / 2, count = 1 against the yardstick at 2^12 -- bbg_ntt_device three times (inverse, coset,
    inverse coset) and bbg_fr_batch_invert_device of n values, queued together -- both up to a synchronisation, interleaved, medians of 9 in
    this one process.  profiles/cells_recover.txt (tests/tools/cells_time.py, one MI355X) has the ratio at 1.205: 0.267 against 0.222 ms.  The
    bound is 1.5 x that, rounded up to one decimal: the margin covers launch-latency noise at a quarter of a millisecond and the ~3 % spread
    between boxes.  The call does what the yardstick does (its one inversion is over r values, not n, but costs the same 81 us: one block's
    scalar-unit inversion) plus the Z products and three pointwise passes."""
    lg, lc = 12, 6
    n, l, r = cm.shape(lg, lc)
    K = r // 2
    ids = sorted(shuffled(range(r), SEED + 80)[:K])
    d_v, d_o, d_y = bbg.dev_alloc(K * l * 32), bbg.dev_alloc(n * 32), bbg.dev_alloc(n * 32)
    try:
        bbg.dev_upload(d_v, ci.coarse_scalars(SEED + 81, K * l, 0))
        bbg.dev_upload(d_y, ci.coarse_scalars(SEED + 82, n, 0))

        def recover():
            bbg.cells_recover_device(ids, d_v, lg, lc, 1, d_o)

        def yardstick():
            for op in (pkg.binding.IFFT, pkg.binding.COSET_FFT, pkg.binding.COSET_IFFT):
                bbg.ntt_device(d_y, lg, op)
            bbg.fr_batch_invert_device(d_y, d_y, n)

        def timed(fn):
            bbg.sync()
            t0 = time.perf_counter()
            fn()
            bbg.sync()
            return time.perf_counter() - t0

        recover()  # warm-up: the domain, the working memory
        yardstick()
        mine, yard = [], []
        for _ in range(9):
            mine.append(timed(recover))
            yard.append(timed(yardstick))
        mine, yard = statistics.median(mine), statistics.median(yard)
        print(f"cells_recover (12, 6): {mine * 1e3:.3f} ms; 3 transforms + batch inversion at 2^12: {yard * 1e3:.3f} ms; ratio {mine / yard:.3f}")
        assert mine <= BOUND * yard, f"the call took {mine * 1e3:.3f} ms, {mine / yard:.2f} x the yardstick's {yard * 1e3:.3f} ms (bound {BOUND} x)"
    finally:
        for d in (d_v, d_o, d_y):
            bbg.dev_free(d)
