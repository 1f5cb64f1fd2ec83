"""Many Lagrange-form polynomials opened in one call, each at its own point, on the MI355X (bbg_open_points*, csrc/open_points.hip).

The string is [x^i] G for a known x and its Lagrange form, so every expected proof is one scalar multiplication of the integer model
(tests/tools/open_points_cases.py): [(F(x) - F(z)) / (x - z)] G, with F(x) and F(z) from Horner on integers.  Shapes are the smallest at
which each mechanism can fail: 2^4 (less than one inversion group), 2^10 (exactly one), 2^11 (two: partial sums across blocks), 2^12 (the
blob size); 1, 8, 9 (a second launch set of the batched MSM) and 33 polynomials (more than the 32 of bbg_poly_evaluate_lagrange)."""
import numpy as np
import pytest

import open_points_cases as oc
import pairing_model as pm

pytestmark = pytest.mark.gpu

R = oc.R
SEED = 0xBB254 + 0x09E0
LOGS = [4, 10, 11, 12]
COUNTS = [1, 8, 9, 33]
GUARD = 0xA5
INF = pm.G1_INFINITY_WORDS


class Shape:
    """One domain size: the string, its Lagrange form and a batch of 33 generic polynomials whose prefixes are the smaller batches."""

    def __init__(self, bbg, oracle, lg):
        self.lg, self.n = lg, 1 << lg
        self.srs = bbg.srs_synth_powers(oc.X_WORDS, self.n)
        self.lag = self.srs.lagrange(lg)
        self.batch = oc.Batch(oracle, lg, 33, SEED + lg)

    def free(self):
        self.lag.free()
        self.srs.free()


@pytest.fixture(scope="module")
def shapes(bbg, oracle):
    made = {}

    def get(lg):
        if lg not in made:
            made[lg] = Shape(bbg, oracle, lg)
        return made[lg]
    yield get
    for s in made.values():
        s.free()


def check(bbg, lag, b, count=None, what=""):
    count = b.count if count is None else count
    y, proofs = bbg.open_points(lag, b.evals[:count], b.z_words[:count])
    assert np.array_equal(y, b.y_words[:count]), what + ": y"
    assert np.array_equal(proofs, b.proofs[:count]), what + ": proofs"


# 1 ------------------------------------------------------------------------------------------------ every shape, bit for bit
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("lg", LOGS)
def test_values_and_proofs(bbg, shapes, lg, count):
    s = shapes(lg)
    check(bbg, s.lag, s.batch, count)


# 2 ------------------------------------------------------------------------------------------------ the route it replaces
@pytest.mark.parametrize("lg", LOGS)
def test_one_polynomial_agrees_with_the_single_call_route(bbg, shapes, lg):
    s = shapes(lg)
    b = s.batch
    d_evals, d_dest = bbg.dev_alloc(s.n * 32), bbg.dev_alloc(s.n * 32)
    try:
        bbg.dev_upload(d_evals, b.evals[0])
        y_old = bbg.kate_opening_lagrange_device(d_evals, d_dest, lg, b.z_words[0])
        proof_old = bbg.g1_normalize(bbg.msm(s.lag, bbg.dev_download(d_dest, (s.n, 4))))[0]
    finally:
        bbg.dev_free(d_evals)
        bbg.dev_free(d_dest)
    y, proofs = bbg.open_points(s.lag, b.evals[:1], b.z_words[:1])
    assert np.array_equal(y[0], y_old) and np.array_equal(proofs[0], proof_old)


# 3, 4 --------------------------------------------------------------------------------------------- points on the domain
@pytest.mark.parametrize("lg", LOGS)
def test_points_on_the_domain(bbg, oracle, shapes, lg):
    s = shapes(lg)
    ms = [0, 1, s.n - 1] + ([1024 + 5] if lg >= 11 else [])  # 1029: a hit in the second inversion group
    b = oc.Batch(oracle, lg, len(ms), SEED + 100 + lg, on_domain=dict(enumerate(ms)))
    y, proofs = bbg.open_points(s.lag, b.evals, b.z_words)
    for k, m in enumerate(ms):
        assert np.array_equal(y[k], b.evals[k, m]), f"y = f_m exactly, m = {m}"
    assert np.array_equal(y, b.y_words)
    assert np.array_equal(proofs, b.proofs), "the proof is the closed form [(F(x) - f_m) / (x - w^m)] G"


def test_batch_mixing_points_on_and_off_the_domain(bbg, oracle, shapes):
    """Polynomials 0, 4 and 8 of nine sit on the domain, each at its own m; a flag or a point shared between polynomials fails this."""
    s = shapes(11)
    b = oc.Batch(oracle, 11, 9, SEED + 200, on_domain={0: 3, 4: 1024 + 5, 8: 2047})
    check(bbg, s.lag, b, what="mixed")
    assert np.array_equal(b.y_words[4], b.evals[4, 1029])


# 5 ------------------------------------------------------------------------------------------------ edge polynomials
def test_zero_constant_and_top_degree_polynomials_in_a_batch(bbg, oracle, shapes):
    s = shapes(10)
    n = s.n
    b = oc.Batch(oracle, 10, 8, SEED + 300, coeffs={1: [0], 3: [12345], 5: [0] * (n - 1) + [1], 6: [0]}, on_domain={6: 17})
    y, proofs = bbg.open_points(s.lag, b.evals, b.z_words)
    assert np.array_equal(y, b.y_words) and np.array_equal(proofs, b.proofs)
    assert not y[1].any() and np.array_equal(proofs[1], INF), "the zero polynomial: y = 0 and a proof at infinity"
    assert np.array_equal(proofs[3], INF), "a constant: a proof at infinity"
    assert not y[6].any() and np.array_equal(proofs[6], INF), "the zero polynomial at a domain point"
    assert not np.array_equal(proofs[5], INF)


# 6 ------------------------------------------------------------------------------------------------ the second representatives
def test_inputs_in_r_to_2r(bbg, shapes):
    s = shapes(11)
    b = s.batch
    y, proofs = bbg.open_points(s.lag, oc.lifted(b.evals[:9]), oc.lifted(b.z_words[:9]))
    assert np.array_equal(y, b.y_words[:9]) and np.array_equal(proofs, b.proofs[:9])


def test_on_domain_point_in_r_to_2r(bbg, oracle, shapes):
    s = shapes(10)
    b = oc.Batch(oracle, 10, 2, SEED + 400, on_domain={0: 5, 1: 1023})
    y, proofs = bbg.open_points(s.lag, oc.lifted(b.evals), oc.lifted(b.z_words))
    assert np.array_equal(y, b.y_words) and np.array_equal(proofs, b.proofs)


# 7 ------------------------------------------------------------------------------------------------ evaluation only
def test_evaluation_only_needs_no_string(bbg, shapes):
    s = shapes(11)
    b, count = s.batch, 33
    y, proofs = bbg.open_points(None, b.evals, b.z_words, proofs=False)
    assert proofs is None and np.array_equal(y, b.y_words)
    d_evals, d_z, d_out = bbg.dev_alloc(count * s.n * 32), bbg.dev_alloc(count * 32), bbg.dev_alloc(count * 32 + 128)
    try:
        bbg.dev_upload(d_evals, b.evals)
        bbg.dev_upload(d_z, b.z_words)
        bbg.dev_upload(d_out, np.full(count * 32 + 128, GUARD, dtype=np.uint8))
        bbg.open_points_device(None, 11, d_evals, d_z, count, d_out + 64, None)
        bbg.sync()
        got = bbg.dev_download(d_out, (count * 32 + 128,), dtype=np.uint8)
        assert (got[:64] == GUARD).all() and (got[-64:] == GUARD).all(), "the guard around y"
        assert np.array_equal(got[64:-64].view(np.uint64).reshape(count, 4), b.y_words)
    finally:
        for d in (d_evals, d_z, d_out):
            bbg.dev_free(d)


# 8 ------------------------------------------------------------------------------------------------ a chunk boundary
def test_chunks_of_the_workspace(bbg, shapes):
    """33 polynomials at 2^10 under a budget of 16 polynomials' working memory (the formula of include/bbg.h): chunks of 16, 16 and 1."""
    s = shapes(10)
    per = 32 * s.n + 64 * ((s.n + 1023) // 1024) + 160
    bbg.open_points_set_budget(16 * per + per // 2)
    try:
        bbg.profile_enable(True)
        _, before = bbg.profile_get("open_points_weights")
        check(bbg, s.lag, s.batch, 33, "three chunks")
        _, after = bbg.profile_get("open_points_weights")
        assert after - before == 3, "one weights stage per chunk"
        bbg.open_points_set_budget(per)  # less than one launch set of the MSM: one polynomial per chunk
        check(bbg, s.lag, s.batch, 3, "one polynomial per chunk")
    finally:
        bbg.profile_enable(False)
        bbg.open_points_set_budget(0)
    assert bbg.memory_report()["scratch"] >= 16 * per, "the workspace is counted under scratch"
    check(bbg, s.lag, s.batch, 33, "the default budget again")


# 9 ------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(bbg, shapes):
    s, short = shapes(10), shapes(4)
    b, count, n = s.batch, 4, s.n
    lib = bbg.lib
    d_evals, d_z, d_y, d_p = bbg.dev_alloc(count * n * 32), bbg.dev_alloc(count * 32), bbg.dev_alloc(count * 32), bbg.dev_alloc(count * 64)
    try:
        bbg.dev_upload(d_evals, b.evals[:count])
        bbg.dev_upload(d_z, b.z_words[:count])
        bbg.dev_upload(d_y, np.full(count * 32, GUARD, dtype=np.uint8))
        bbg.dev_upload(d_p, np.full(count * 64, GUARD, dtype=np.uint8))

        def device(lag=s.lag.handle, lg=10, ev=d_evals, z=d_z, cnt=count, y=d_y, p=d_p):
            return lib.bbg_open_points_device(bbg.ctx, lag, lg, ev, z, cnt, y, p)
        refused = {"a string shorter than n": dict(lag=short.lag.handle), "a null string with proofs": dict(lag=None), "null values": dict(ev=None),
                   "null points": dict(z=None), "a null y": dict(y=None), "count = 0": dict(cnt=0), "count above 2^20": dict(cnt=(1 << 20) + 1),
                   "log2n = 0": dict(lg=0), "log2n = 29": dict(lg=29), "y on the values": dict(y=d_evals + 64), "y on the points": dict(y=d_z),
                   "the proofs on the values": dict(p=d_evals), "the proofs on the points": dict(p=d_z), "the proofs on y": dict(p=d_y)}
        for what, kw in refused.items():
            assert device(**kw) == -1 and lib.bbg_last_error(), what
        y_host, p_host = np.full((count, 4), 7, dtype=np.uint64), np.full((count, 8), 7, dtype=np.uint64)
        ev_host, z_host = np.ascontiguousarray(b.evals[:count]), np.ascontiguousarray(b.z_words[:count])
        for what, (lag, cnt, yy) in {"a string shorter than n": (short.lag.handle, count, y_host.ctypes.data), "count = 0": (s.lag.handle, 0, y_host.ctypes.data),
                                     "a null y": (s.lag.handle, count, None)}.items():
            assert lib.bbg_open_points(bbg.ctx, lag, 10, ev_host.ctypes.data, z_host.ctypes.data, cnt, yy, p_host.ctypes.data) == -1, what
        assert (y_host == 7).all() and (p_host == 7).all()
        bbg.sync()
        assert (bbg.dev_download(d_y, (count * 32,), dtype=np.uint8) == GUARD).all(), "a refused call wrote y"
        assert (bbg.dev_download(d_p, (count * 64,), dtype=np.uint8) == GUARD).all(), "a refused call wrote the proofs"
        assert np.array_equal(bbg.dev_download(d_evals, (count, n, 4)), b.evals[:count]), "a refused call wrote an input"
        assert device() == 0, "the legal call right after"
        bbg.sync()
        assert np.array_equal(bbg.dev_download(d_y, (count, 4)), b.y_words[:count])
        assert np.array_equal(bbg.dev_download(d_p, (count, 8)), b.proofs[:count])
    finally:
        for d in (d_evals, d_z, d_y, d_p):
            bbg.dev_free(d)
