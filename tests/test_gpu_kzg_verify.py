"""A batch of openings at arbitrary points reduced to one pairing check on the MI355X (bbg_kzg_verify*, csrc/kzg_verify.hip).

Openings are those of tests/tools/open_points_cases.py at 2^6 values over the string [x^i] G: the proofs are made by bbg_open_points (and
held to the integer expectation), the commitments are [F(x)] G.  L and R of the reduce form are compared bit for bit with the integer closed
form L = [sum rho^i w_i] G, R = [sum rho^i (c_i - y_i + z_i w_i)] G; N = 63, 64, 65 straddle a wave, 200 fills more than one."""
import ctypes

import numpy as np
import pytest

import coarse_inputs as ci
import open_points_cases as oc
import open_points_model as om
import pairing_model as pm

pytestmark = pytest.mark.gpu

R, P = pm.R, pm.P
SEED = 0xBB254 + 0x0C26
LG = 6
NS = [1, 2, 63, 64, 65, 200]
GUARD32 = 0xA5A5A5A5
INF = pm.G1_INFINITY_WORDS


def negated(point):
    p = pm.g1_from_words(point)
    return pm.g1_words(None if p is None else (p[0], -p[1] % P))


class World:
    """The string, its Lagrange form, the lines of ([x]_2, [1]_2) and 200 honest openings, made once."""

    def __init__(self, bbg, oracle):
        self.bbg = bbg
        self.srs = bbg.srs_synth_powers(oc.X_WORDS, 1 << LG)
        self.lag = self.srs.lagrange(LG)
        self.lines = bbg.g2_lines_prepare(np.stack([bbg.g2_mul(pm.fr_words([oc.X_INT]))[0], pm.g2_words(pm.G2)]))
        rng = np.random.default_rng(SEED)
        self.rho_int = oc.rand_fr(rng)
        self.rho = pm.fr_words([self.rho_int])[0]
        self.b = oc.Batch(oracle, LG, 200, SEED + 1, coeffs={7: [0]})  # opening 7: the zero polynomial, commitment and proof at infinity
        y, proofs = bbg.open_points(self.lag, self.b.evals, self.b.z_words)
        assert np.array_equal(y, self.b.y_words) and np.array_equal(proofs, self.b.proofs), "bbg_open_points made the proofs"
        self.proofs = proofs
        assert np.array_equal(self.b.commitments[7], INF) and np.array_equal(proofs[7], INF)

    def opening(self, N):
        b = self.b
        return b.commitments[:N].copy(), b.z_words[:N].copy(), b.y_words[:N].copy(), self.proofs[:N].copy()

    def status(self, o, rho=None):
        """(return code, status word) of the host form."""
        com, z, y, prf = (np.ascontiguousarray(a) for a in o)
        rho = self.rho if rho is None else rho
        word = ctypes.c_uint32(GUARD32)
        rc = self.bbg.lib.bbg_kzg_verify(self.bbg.ctx, self.lines.handle, com.ctypes.data, z.ctypes.data, y.ctypes.data, prf.ctypes.data, com.shape[0],
                                         rho.ctypes.data, ctypes.byref(word))
        return rc, word.value

    def free(self):
        self.lines.free()
        self.lag.free()
        self.srs.free()


@pytest.fixture(scope="module")
def world(bbg, oracle):
    w = World(bbg, oracle)
    yield w
    w.free()


def expected_lr(c, z, y, w, rho):
    l, r = om.kzg_closed_form(c, z, y, w, rho)
    return np.stack([oc.g1(l), oc.g1(r)])


# 1 ------------------------------------------------------------------------------------------------ the status word
@pytest.mark.parametrize("N", NS)
def test_status(world, pkg, N):
    bbg = world.bbg
    o = world.opening(N)
    assert world.status(o) == (0, 1), "the honest batch"
    assert bbg.kzg_verify(world.lines, *o, world.rho) == 1
    k = N - 1
    wrong = {}
    y2 = o[2].copy()
    y2[k] = pm.fr_words([12345])[0]
    wrong["one y changed"] = (o[0], o[1], y2, o[3])
    z2 = o[1].copy()
    z2[k] = pm.fr_words([54321])[0]
    wrong["one z changed"] = (o[0], z2, o[2], o[3])
    if N > 1:
        p2 = o[3].copy()
        p2[[0, 1]] = p2[[1, 0]]
        wrong["two proofs swapped"] = (o[0], o[1], o[2], p2)
        c2 = o[0].copy()
        c2[k] = c2[0]
        wrong["one commitment replaced by another"] = (c2, o[1], o[2], o[3])
    for what, bad in wrong.items():
        assert world.status(bad) == (0, 0), what
    for which, what in ((0, "a commitment off the curve"), (3, "a proof off the curve")):
        bad = [a.copy() for a in o]
        j = 0 if N <= 7 else 5  # (a finite point: opening 7 is the zero polynomial)
        bad[which][j, 4:] = ci.add_int(bad[which][j, 4:], 1)[0]  # y + 1
        assert world.status(bad) == (-1, 2), what
        assert b"not on the curve" in bbg.lib.bbg_last_error()
        with pytest.raises(pkg.BbgError):
            bbg.kzg_verify_reduce(*bad, world.rho)
        d = [bbg.dev_alloc(a.nbytes) for a in bad] + [bbg.dev_alloc(256)]
        try:
            for p, a in zip(d, bad):
                bbg.dev_upload(p, a)
            bbg.dev_upload(d[4], np.full(64, GUARD32, dtype=np.uint32))
            bbg.kzg_verify_reduce_device(d[0], d[1], d[2], d[3], N, world.rho, d[4], d[4] + 128)
            got = bbg.dev_download(d[4], (64,), dtype=np.uint32)
            assert int(got[32]) == 1, what + ": a count of exactly 1"
            assert (got[33:] == GUARD32).all()
        finally:
            for p in d:
                bbg.dev_free(p)
    assert world.status(o) == (0, 1), "the honest batch again, behind the others"


# 2 ------------------------------------------------------------------------------------------------ L and R against the integer closed form
@pytest.mark.parametrize("N", NS)
def test_reduction_is_the_closed_form(world, N):
    bbg, b = world.bbg, world.b
    o = world.opening(N)
    got = bbg.kzg_verify_reduce(*o, world.rho)
    assert np.array_equal(got, expected_lr(b.c[:N], b.z[:N], b.y[:N], b.w[:N], world.rho_int))
    # inputs in [r, 2r) and coordinates in [p, 2p): the same canonical L and R
    lifted = (np.concatenate([ci.add_int(o[0][:, :4], P), ci.add_int(o[0][:, 4:], P)], axis=1) if N < 8 else o[0], oc.lifted(o[1]), oc.lifted(o[2]), o[3])
    assert np.array_equal(bbg.kzg_verify_reduce(*lifted, oc.lifted(world.rho)), got)
    # a reduction is a function of its inputs, valid or not
    y2 = o[2].copy()
    y2[0] = pm.fr_words([999])[0]
    assert np.array_equal(bbg.kzg_verify_reduce(o[0], o[1], y2, o[3], world.rho), expected_lr(b.c[:N], b.z[:N], [999] + b.y[1:N], b.w[:N], world.rho_int))


@pytest.mark.parametrize("N", [1, 65])
def test_rho_zero(world, N):
    b = world.b
    zero = pm.fr_words([0])[0]
    got = world.bbg.kzg_verify_reduce(*world.opening(N), zero)
    assert np.array_equal(got, expected_lr(b.c[:N], b.z[:N], b.y[:N], b.w[:N], 0)), "rho^0 = 1 also for rho = 0"
    assert np.array_equal(got[0], world.proofs[0])
    assert world.status(world.opening(N), zero) == (0, 1)


def test_one_polynomial_at_many_points(world, oracle):
    bbg, N = world.bbg, 65
    rng = np.random.default_rng(SEED + 2)
    f = [oc.rand_fr(rng) for _ in range(1 << LG)]
    b = oc.Batch(oracle, LG, N, SEED + 3, coeffs={k: f for k in range(N)}, on_domain={3: 9, 4: 9})  # a repeated point as well
    y, proofs = bbg.open_points(world.lag, b.evals, b.z_words)
    assert np.array_equal(proofs, b.proofs)
    got = bbg.kzg_verify_reduce(b.commitments, b.z_words, y, proofs, world.rho)
    assert np.array_equal(got, expected_lr(b.c, b.z, b.y, b.w, world.rho_int))
    assert bbg.kzg_verify(world.lines, b.commitments, b.z_words, y, proofs, world.rho) == 1


def test_only_the_zero_polynomial(world):
    o = tuple(a[7:8] for a in world.opening(8))
    got = world.bbg.kzg_verify_reduce(*o, world.rho)
    assert np.array_equal(got[0], INF) and np.array_equal(got[1], INF), "infinite commitment and proof, y = 0: L = R = infinity"
    assert world.status(o) == (0, 1)


# 3 ------------------------------------------------------------------------------------------------ the existing verifier
def test_agrees_with_cells_verify_at_single_points(world):
    """Openings at domain points, values from bbg_ntt: L and R are what bbg_cells_verify_reduce writes at log2cell = 0 for the same cells in
    the same order, and the verdict is that of the two-step route (reduce, negate on the host, bbg_pairing_product)."""
    bbg, b = world.bbg, world.b
    n = 1 << LG
    npoly = 3
    values = np.stack([bbg.ntt(pm.fr_words(b.polys[c])) for c in range(npoly)])  # (3, n, 4)
    cells = [(c, m) for m in (0, 1, 5, 31, n - 1) for c in range(npoly)] + [(1, 5)]  # a duplicate as well
    cids, mids = [c for c, _ in cells], [m for _, m in cells]
    w = om.root(LG)
    z = pm.fr_words([pow(w, m, R) for m in mids])
    evals = np.stack([values[c] for c in cids])
    y, proofs = bbg.open_points(world.lag, evals, z)
    assert np.array_equal(y, np.stack([b.evals[c, m] for c, m in cells])), "y = f_m, canonical"
    want = bbg.cells_verify_reduce(world.srs, LG, 0, b.commitments[:npoly], cids, mids, y, proofs, world.rho)
    got = bbg.kzg_verify_reduce(b.commitments[cids], z, y, proofs, world.rho)
    assert np.array_equal(got, want)
    _, two_step = bbg.pairing_product(world.lines, np.stack([got[0], negated(got[1])]), want_values=False)
    assert int(two_step[0]) == 1 and bbg.kzg_verify(world.lines, b.commitments[cids], z, y, proofs, world.rho) == 1
    y2 = y.copy()
    y2[2] = pm.fr_words([4242])[0]
    got2 = bbg.kzg_verify_reduce(b.commitments[cids], z, y2, proofs, world.rho)
    assert np.array_equal(got2, bbg.cells_verify_reduce(world.srs, LG, 0, b.commitments[:npoly], cids, mids, y2, proofs, world.rho))
    _, two_step = bbg.pairing_product(world.lines, np.stack([got2[0], negated(got2[1])]), want_values=False)
    assert int(two_step[0]) == 0 and bbg.kzg_verify(world.lines, b.commitments[cids], z, y2, proofs, world.rho) == 0


# 4 ------------------------------------------------------------------------------------------------ refusals and back-to-back calls
def test_refusals_write_nothing(world):
    bbg, N = world.bbg, 8
    lib = bbg.lib
    o = world.opening(N)
    d = [bbg.dev_alloc(a.nbytes) for a in o]
    d_out, d_st = bbg.dev_alloc(256), bbg.dev_alloc(4)
    one = bbg.g2_lines_prepare(pm.g2_words(pm.G2).reshape(1, 16))
    try:
        for p, a in zip(d, o):
            bbg.dev_upload(p, a)
        bbg.dev_upload(d_out, np.full(64, GUARD32, dtype=np.uint32))
        bbg.dev_upload(d_st, np.full(1, GUARD32, dtype=np.uint32))

        def reduce(com=d[0], z=d[1], y=d[2], prf=d[3], n=N, rho=world.rho.ctypes.data, out=d_out, off=d_out + 128):
            return lib.bbg_kzg_verify_reduce_device(bbg.ctx, com, z, y, prf, n, rho, out, off)

        def verdict(lines=world.lines.handle, com=d[0], n=N, st=d_st):
            return lib.bbg_kzg_verify_device(bbg.ctx, lines, com, d[1], d[2], d[3], n, world.rho.ctypes.data, st)
        for what, kw in {"null commitments": dict(com=None), "null points": dict(z=None), "null values": dict(y=None), "null proofs": dict(prf=None),
                         "a null rho": dict(rho=None), "a null output": dict(out=None), "N = 0": dict(n=0), "N above 2^27": dict(n=(1 << 27) + 1),
                         "the output on the proofs": dict(out=d[3]), "the count on the values": dict(off=d[2] + 4), "the count on the output": dict(off=d_out + 64)}.items():
            assert reduce(**kw) == -1 and lib.bbg_last_error(), what
        for what, kw in {"a null handle": dict(lines=None), "a one-pair handle": dict(lines=one.handle), "N = 0": dict(n=0), "a null status": dict(st=None),
                         "null commitments": dict(com=None), "the status on the points": dict(st=d[1] + 8)}.items():
            assert verdict(**kw) == -1 and lib.bbg_last_error(), what
        assert verdict(lines=one.handle) == -1 and b"exactly two points" in lib.bbg_last_error()
        bbg.sync()
        assert (bbg.dev_download(d_out, (64,), dtype=np.uint32) == GUARD32).all(), "a refused call wrote an output"
        assert int(bbg.dev_download(d_st, (1,), dtype=np.uint32)[0]) == GUARD32
        for p, a in zip(d, o):
            assert np.array_equal(bbg.dev_download(p, a.shape), a), "a refused call wrote an input"
        assert verdict() == 0 and int(bbg.dev_download(d_st, (1,), dtype=np.uint32)[0]) == 1, "the legal call right after"
    finally:
        one.free()
        for p in d + [d_out, d_st]:
            bbg.dev_free(p)


def test_back_to_back_calls_keep_their_own_status(world):
    """Three calls with alternating valid and invalid inputs and ONE synchronisation: they share the packed arrays, the MSM's working memory
    and the context's 512 bytes, and each word must hold its own call's verdict."""
    bbg, N = world.bbg, 65
    o = world.opening(N)
    wrong = o[2].copy()
    wrong[N - 1] = pm.fr_words([777])[0]
    d = [bbg.dev_alloc(a.nbytes) for a in o]
    d_wrong, d_st = bbg.dev_alloc(wrong.nbytes), bbg.dev_alloc(16)
    try:
        for p, a in zip(d + [d_wrong, d_st], list(o) + [wrong, np.full(4, GUARD32, dtype=np.uint32)]):
            bbg.dev_upload(p, a)
        bbg.sync()
        for k, d_y in enumerate((d[2], d_wrong, d[2])):
            bbg.kzg_verify_device(world.lines, d[0], d[1], d_y, d[3], N, world.rho, d_st + 4 * k)
        bbg.sync()
        assert list(bbg.dev_download(d_st, (4,), dtype=np.uint32)) == [1, 0, 1, GUARD32]
    finally:
        for p in d + [d_wrong, d_st]:
            bbg.dev_free(p)
