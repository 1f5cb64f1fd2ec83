"""The resident prover's own entry points (csrc/prover.hip) against a model, with no reference-prover binary: the commitment identity of
every round, rounds 5a (bbg_prover_evaluate), 5b (bbg_prover_linearise) and 6 (bbg_prover_round6) against tests/tools/prover_rounds_model.py,
and all of it again under every batching option and every path of round 4's widget chain.

What is held to what.  The handle's polynomials are read back with bbg_prover_read_poly; every commitment must be the MSM of the coefficients
it claims to commit to (oracle.pippenger at 2^6; from 2^11 bbg_msm, which is pinned to the oracle elsewhere and shares no code with commit()'s
chunking), and every evaluation, r(X), r(zeta), W_zeta and W_zeta_omega must be what the model makes of the same read-back coefficients.
Rounds 1 and 3 are pinned by tests/test_gpu_ntt_dispatch.py and tests/test_gpu_parity.py and are not modelled again.  All comparisons are
bit-exact on canonical words.  An option row runs one whole proof and must reproduce the default row's commitments, evaluations and (canonical)
read-back polynomials exactly, so the model's side is computed once per shape, from the default row, and reused.

Shapes: 2^6 (one evaluation block everywhere); 2^11 at width 4 (n is one 4096-coefficient block, 4n two: one multi-evaluation launch mixes block
counts); 2^12 at width 3 and the MiMC flavour (T_3 and F have 4097 coefficients: a second block of exactly one)."""
import contextlib
import ctypes

import numpy as np
import pytest

import barycentric_model as bm
import coarse_inputs as ci
import prover_rounds_model as prm
from test_gpu_barycentric import make_prover

pytestmark = pytest.mark.gpu

P = ci.R_MOD
E_INVALID = -1
COEFF = 0  # BBG_FORM_COEFF
# enum bbg_quotient_poly / bbg_prover_poly (include/bbg.h)
W_1, Z, SIGMA_1, Q_1, Q_LOGIC = 0, 4, 5, 9, 19
QUOTIENT, T_1, T_3, T_4, LINEAR, OPENING, SHIFTED_OPENING, Q_MIMC_COEFFICIENT, Q_MIMC_SELECTOR = 21, 22, 24, 25, 26, 27, 28, 29, 30
FLAVOUR_MIMC = 2
SENTINEL = 0x5A5A5A5A5A5A5A5A
DEFAULTS = {"prover_msm_batch": 4, "prover_tail_window": 0, "msm_window": 0, "poly_limbs29": 1, "prover_ntt_batch": 1, "prover_early_cosets": -1,
            "quotient_limbs29": 1, "quotient_fuse": 1, "quotient_setup_plan": 1}
SHAPES = {"6w3": (6, 3, False), "6w4": (6, 4, False), "11w4": (11, 4, False), "12w3": (12, 3, False), "12mimc": (12, 3, True)}
ROUND6_DEFAULT = (14, 5)  # the term counts of a TurboPLONK proof (bench.py prover_shaped)


def word(v):
    return ci.to_words([v])[0]


def splice_edges(a, seed):
    """p - 1 and coarse representatives x + p (below 2p) at a few seeded places of a synthetic array."""
    a = a.copy()
    n = len(a)
    a[seed % n] = word(P - 1)
    for i in ((3 * seed + 1) % n, (5 * seed + 2) % n, n - 1 - seed % 3):
        a[i] = word(ci.to_ints(a[i])[0] % P + P)
    return a


@contextlib.contextmanager
def options(bbg, **values):
    try:
        for key, value in values.items():
            bbg.set_option(key, value)
        yield
    finally:
        for key in values:
            bbg.set_option(key, DEFAULTS[key])


def make_mimc_prover(pkg, bbg, srs, lg):
    """make_prover's key under the MiMC flavour: width 3 and the two selectors only its widget reads."""
    lib, n = bbg.lib, 1 << lg
    gens = np.stack([bbg.field_op(0, 5, np.array([[k, 0, 0, 0]], dtype=np.uint64))[0] for k in (5, 5, 6, 7)])
    h = ctypes.c_void_p()
    assert lib.bbg_prover_create_flavour(bbg.ctx, srs.handle, lg, FLAVOUR_MIMC, gens.ctypes.data, ctypes.byref(h)) == 0, lib.bbg_last_error()
    for pid in [p for p in range(5, 20) if p != 8] + [Q_MIMC_COEFFICIENT, Q_MIMC_SELECTOR]:
        assert lib.bbg_prover_set_key_poly(h, pid, COEFF, pkg.synthetic_scalars(500 + pid, n).ctypes.data) == 0, lib.bbg_last_error()
    assert lib.bbg_prover_finalize_key(h) == 0, lib.bbg_last_error()
    return h


class Shape:
    """One proving key on the device, its inputs, and the id lists of rounds 5 and 6."""

    def __init__(self, pkg, bbg, name):
        self.name = name
        self.lg, self.width, self.mimc = SHAPES[name]
        self.pkg, self.bbg, self.lib = pkg, bbg, bbg.lib
        lg, width = self.lg, self.width
        n = self.n = 1 << lg
        self.srs = bbg.srs_synth_hashed(5, n + 1)
        self.h = make_mimc_prover(pkg, bbg, self.srs, lg) if self.mimc else make_prover(pkg, bbg, self.srs, lg, width)
        for pid in (SIGMA_1, Q_1 + 2, Q_1 + 5):  # sigma_1, q_3, q_m with edge entries (re-registering replaces every form at the next finalize)
            edged = splice_edges(pkg.synthetic_scalars(500 + pid, n), pid)
            assert self.lib.bbg_prover_set_key_poly(self.h, pid, COEFF, edged.ctypes.data) == 0, self.lib.bbg_last_error()
        assert self.lib.bbg_prover_finalize_key(self.h) == 0, self.lib.bbg_last_error()
        self.wires = [splice_edges(pkg.synthetic_scalars(600 + k, n), 7 + k) for k in range(4)]
        self.ch = pkg.synthetic_scalars(700, 8)
        sigmas = [SIGMA_1 + k for k in range(width)]
        wires = [W_1 + k for k in range(width)]
        selectors = list(range(Q_1, Q_LOGIC + 1)) + ([Q_MIMC_COEFFICIENT, Q_MIMC_SELECTOR] if self.mimc else [])
        self.key_ids = sigmas + selectors
        self.len_of = {QUOTIENT: 4 * n, T_3: n + 1 if width == 3 else n}
        # round 5a: 32 ids -- t (4n), every T_k (T_3 has n + 1 at width 3), wires, z, sigmas, selectors; about every third one shifted
        pool = [QUOTIENT, T_1, T_1 + 1, T_3, T_4] + wires + [Z] + sigmas + selectors
        self.eval_ids = [pool[k % len(pool)] for k in range(32)]
        self.eval_shifted = [1 if k % 3 == 1 else 0 for k in range(32)]
        self.fill_shifted = [k % 2 for k in range(32)]
        # rounds 5b and 6 read n coefficients of each id
        lin_pool = [Z] + sigmas + selectors + wires + [T_1 + 1]
        self.lin_ids = [lin_pool[k % len(lin_pool)] for k in range(32)]
        zeta_pool = wires + selectors[6:9] + sigmas[:-1] + [LINEAR, T_1 + 1, T_3, T_4] + selectors[:6] + [Z]
        self.zeta_ids = [zeta_pool[k % len(zeta_pool)] for k in range(32)]
        omega_pool = wires + [Z] + sigmas + selectors
        self.omega_ids = [omega_pool[k % len(omega_pool)] for k in range(32)]
        self.lin_scalars = self.scalars(710)
        self.nu_zeta, self.nu_omega = self.scalars(711), self.scalars(712)
        generic = bm.mont_words(bm.Z_INTS[:1])[0]
        self.zeta = generic
        self.zeta_omega = prm.times_root(generic, lg)
        self.top_scalar = pkg.synthetic_scalars(713, 1)[0] if width == 3 else None
        root5 = ci.to_mont(pow(ci.root_of_unity(lg), 5, P), 0)
        self.points = {"generic": generic, "zero": word(0), "one": word(ci.to_mont(1, 0)), "domain": word(root5),
                       "coarse": bm.second_representative(generic)[0]}
        self.baseline = None  # the default row's proof
        self.want = None      # what the model and the reference MSM make of the baseline's read-back polynomials

    def scalars(self, seed):
        """32 scalars: a coarse value, 0, 1, p - 1 and the raw word 1 first, synthetic ones after."""
        s = self.pkg.synthetic_scalars(seed, 32)
        for k, v in enumerate((ci.to_ints(s[0])[0] % P + P, 0, ci.to_mont(1, 0), P - 1, 1)):
            s[k] = word(v)
        return s

    def close(self):
        self.lib.bbg_prover_destroy(self.h)
        self.srs.free()

    # ---- device side
    def read(self, pid, count=None):
        out = np.zeros((count or self.len_of.get(pid, self.n), 4), dtype=np.uint64)
        assert self.lib.bbg_prover_read_poly(self.h, pid, COEFF, out.ctypes.data, len(out)) == 0, (pid, self.lib.bbg_last_error())
        return out

    def rounds_1_3_4(self):
        """Rounds 1, 3 and 4 on the shape's wires and challenges: W_1 .. W_w, Z, T_1 .. T_w as canonical affine points."""
        lib, h, ch, w = self.lib, self.h, self.ch, self.width
        wp = (ctypes.c_void_p * 4)(*[a.ctypes.data for a in self.wires])
        com = np.zeros((2 * w + 1, 12), dtype=np.uint64)
        assert lib.bbg_prover_round1(h, wp, com.ctypes.data) == 0, lib.bbg_last_error()
        assert lib.bbg_prover_round3(h, ch[0].ctypes.data, ch[1].ctypes.data, ch[2:5].ctypes.data, com[w:].ctypes.data) == 0, lib.bbg_last_error()
        assert lib.bbg_prover_round4(h, ch[5].ctypes.data, ch[6].ctypes.data, com[w + 1:].ctypes.data) == 0, lib.bbg_last_error()
        return self.bbg.g1_normalize(com)

    def evaluate(self, ids, shifted, zeta):
        out = np.full((len(ids), 4), SENTINEL, dtype=np.uint64)
        idv = (ctypes.c_int * len(ids))(*ids)
        shv = (ctypes.c_int * len(ids))(*shifted) if shifted is not None else None
        assert self.lib.bbg_prover_evaluate(self.h, len(ids), idv, shv, zeta.ctypes.data, out.ctypes.data) == 0, self.lib.bbg_last_error()
        return out

    def linearise(self, count):
        out = np.full(4, SENTINEL, dtype=np.uint64)
        idv = (ctypes.c_int * count)(*self.lin_ids[:count])
        sc = np.ascontiguousarray(self.lin_scalars[:count])
        assert self.lib.bbg_prover_linearise(self.h, count, idv, sc.ctypes.data, self.zeta.ctypes.data, out.ctypes.data) == 0, self.lib.bbg_last_error()
        return out

    def round6(self, count_zeta, count_omega):
        """PI_Z and PI_Z_OMEGA as canonical affine points."""
        pi = np.full((2, 12), SENTINEL, dtype=np.uint64)
        iz, io = (ctypes.c_int * 32)(*self.zeta_ids), (ctypes.c_int * 32)(*self.omega_ids)
        top = self.top_scalar.ctypes.data if self.top_scalar is not None else None
        rc = self.lib.bbg_prover_round6(self.h, count_zeta, iz, self.nu_zeta.ctypes.data, count_omega, io, self.nu_omega.ctypes.data,
                                        self.zeta.ctypes.data, self.zeta_omega.ctypes.data, top, pi[0].ctypes.data, pi[1].ctypes.data)
        assert rc == 0, self.lib.bbg_last_error()
        return self.bbg.g1_normalize(pi)

    def prove(self, counts=ROUND6_DEFAULT, full=True):
        """One proof, rounds 1 to 6.  full: with the reads and calls of assertions (a) to (d); else only what round 6 needs."""
        out = {"com": self.rounds_1_3_4(), "polys": {}, "evals": {}, "lin": {}}
        if full:
            for pid in [W_1 + k for k in range(self.width)] + [Z, QUOTIENT] + [T_1 + k for k in range(4)]:
                out["polys"][pid] = self.read(pid)
            for name, z in self.points.items():
                # first a call in which every polynomial fills every block: none of its partial sums may show in the mixed-length call after it
                out["evals"][name] = (self.evaluate([QUOTIENT] * 32, self.fill_shifted, z), self.evaluate(self.eval_ids, self.eval_shifted, z),
                                      self.evaluate([QUOTIENT], [1], z))
        for count in (1, 5, 32) if full else (32,):  # the last one leaves the r(X) round 6 opens
            r_eval = self.linearise(count)
            out["lin"][count] = (r_eval, self.read(LINEAR))
        out["pi"] = self.round6(*counts)
        out["openings"] = (self.read(OPENING), self.read(SHIFTED_OPENING))
        return out

    # ---- model side
    def commit(self, coeffs):
        """The commitment to `coeffs` over the shape's SRS by a route that shares nothing with commit(): canonical affine words."""
        if self.lg <= 6:
            return prm.oracle().pippenger(prm.canon(coeffs), self.srs.read(0, len(coeffs)))
        return self.bbg.g1_normalize(self.bbg.msm(self.srs, coeffs))[0]

    def coefficient_arrays(self, polys):
        """id -> read-back coefficients, for every id rounds 5 and 6 name (the key's polynomials are read here, once)."""
        arrays = dict(polys)
        for pid in self.key_ids:
            arrays[pid] = self.read(pid)
        return arrays

    def expected_openings(self, counts):
        cz, co = counts
        a, n = self.want["arrays"], self.n
        top = (self.top_scalar, a[QUOTIENT][3 * n]) if self.width == 3 else None
        return prm.openings(a[QUOTIENT][:n], [a[i][:n] for i in self.zeta_ids[:cz]], self.nu_zeta[:cz], [a[i][:n] for i in self.omega_ids[:co]],
                            self.nu_omega[:co], self.zeta, self.zeta_omega, top)

    def expectations(self, proof):
        n, w = self.n, self.width
        a = self.coefficient_arrays(proof["polys"])
        want = self.want = {"arrays": a}
        want["com"] = np.stack([self.commit(a[W_1 + k]) for k in range(w)] + [self.commit(a[Z])] + [self.commit(a[T_1 + k]) for k in range(w)])
        want["evals"] = {}
        for name, z in self.points.items():
            t_at = prm.evaluations([a[QUOTIENT]] * 2, [0, 1], z, self.lg)
            want["evals"][name] = (t_at[self.fill_shifted], prm.evaluations([a[i] for i in self.eval_ids], self.eval_shifted, z, self.lg), t_at[1:])
        want["lin"] = {c: prm.linearisation([a[i][:n] for i in self.lin_ids[:c]], self.lin_scalars[:c], self.zeta) for c in (1, 5, 32)}
        a[LINEAR] = want["lin"][32][0]
        want["openings"] = {ROUND6_DEFAULT: self.expected_openings(ROUND6_DEFAULT)}
        want["pi"] = {ROUND6_DEFAULT: np.stack([self.commit(o) for o in want["openings"][ROUND6_DEFAULT]])}
        return want

    def round6_expected(self, counts):
        if counts not in self.want["openings"]:
            self.want["openings"][counts] = self.expected_openings(counts)
            self.want["pi"][counts] = np.stack([self.commit(o) for o in self.want["openings"][counts]])
        return self.want["openings"][counts], self.want["pi"][counts]

    # ---- assertions (a) to (d) on one proof
    def check(self, proof, what, counts=ROUND6_DEFAULT):
        want, n, w = self.want, self.n, self.width
        polys = proof["polys"]
        # (a) commitment identity, and t(X) as the concatenation of its slices
        assert np.array_equal(proof["com"], want["com"]), f"{what}: W_k / Z / T_k are not the commitments to the read-back coefficients"
        for k in range(4):
            m = len(polys[T_1 + k])
            assert m == (n + 1 if (w == 3 and k == 2) else n)
            assert np.array_equal(polys[T_1 + k], polys[QUOTIENT][k * n:k * n + m]), f"{what}: T_{k + 1} is not its slice of t(X)"
        # (b) round 5a
        for name in self.points:
            for got, expect, call in zip(proof["evals"][name], want["evals"][name], ("32 x t", "32 ids", "one id")):
                assert ci.below(got, P).all(), f"{what}: evaluations at {name} ({call}) not below p"
                assert np.array_equal(got, expect), f"{what}: evaluations at {name} ({call}): ids {np.flatnonzero((got != expect).any(axis=1)).tolist()}"
        # (c) round 5b
        for count, (r_eval, r) in proof["lin"].items():
            expect_r, expect_eval = want["lin"][count]
            assert np.array_equal(prm.canon(r), expect_r), f"{what}: r(X) of {count} terms"
            assert np.array_equal(prm.canon(r_eval), expect_eval), f"{what}: r(zeta) of {count} terms"
        self.check_round6(proof, what, counts)

    def check_round6(self, proof, what, counts):
        # (d) round 6: both opening polynomials, and their commitments as in (a)
        expect_w, expect_pi = self.round6_expected(counts)
        for got, expect, label in zip(proof["openings"], expect_w, ("W_zeta", "W_zeta_omega")):
            assert np.array_equal(prm.canon(got), expect), f"{what}: {label} for counts {counts}"
        assert np.array_equal(proof["pi"], expect_pi), f"{what}: PI_Z / PI_Z_OMEGA for counts {counts}"

    def check_same_as_baseline(self, proof, what):
        """What reaches the host -- commitments, evaluations, r(zeta) -- word for word; resident polynomials on canonical words: a device array may
        hold any representative below 2p, and the 32-bit and the 29-bit kernels of option poly_limbs29 leave different ones of the same values."""
        base = self.baseline
        assert np.array_equal(proof["com"], base["com"]) and np.array_equal(proof["pi"], base["pi"]), f"{what}: commitments differ from the default row's"
        for pid, a in base["polys"].items():
            assert np.array_equal(prm.canon(proof["polys"][pid]), prm.canon(a)), f"{what}: polynomial {pid} differs from the default row's"
        for count, (r_eval, r) in base["lin"].items():
            assert np.array_equal(proof["lin"][count][0], r_eval), f"{what}: r(zeta) of {count} terms differs from the default row's"
            assert np.array_equal(prm.canon(proof["lin"][count][1]), prm.canon(r)), f"{what}: r(X) of {count} terms differs from the default row's"
        for got, a in zip(proof["openings"], base["openings"]):
            assert np.array_equal(prm.canon(got), prm.canon(a)), f"{what}: an opening polynomial differs from the default row's"
        for name, pair in base["evals"].items():
            assert all(np.array_equal(g, b) for g, b in zip(proof["evals"][name], pair)), f"{what}: evaluations at {name}"


_SHAPES = {}


@pytest.fixture(scope="module")
def shapes(pkg, bbg):
    """name -> Shape with its default-row proof checked and its expectations computed: once per shape, on first use."""
    def get(name):
        if name not in _SHAPES:
            s = _SHAPES[name] = Shape(pkg, bbg, name)
            s.baseline = s.prove()
            s.expectations(s.baseline)
        return _SHAPES[name]
    yield get
    for s in _SHAPES.values():
        s.close()
    _SHAPES.clear()


def option_row(s, bbg, what, **values):
    with options(bbg, **values):
        proof = s.prove()
    s.check(proof, what)
    s.check_same_as_baseline(proof, what)


# (a) - (d) ---------------------------------------------------------------------------------------- library defaults
@pytest.mark.parametrize("name", list(SHAPES))
def test_default_proof_against_the_model(shapes, name):
    s = shapes(name)
    s.check(s.baseline, f"{name} defaults")
    again = s.prove()  # a second proof on the handle: nothing of the first one is left over
    s.check_same_as_baseline(again, f"{name} second proof")


@pytest.mark.parametrize("name", list(SHAPES))
def test_round6_every_term_count(shapes, name):
    s = shapes(name)
    for count_zeta in (0, 1, 14, 32):
        for count_omega in (1, 5, 32):
            proof = s.prove((count_zeta, count_omega), full=False)
            assert np.array_equal(proof["com"], s.baseline["com"])
            assert np.array_equal(proof["lin"][32][1], s.baseline["lin"][32][1])
            s.check_round6(proof, name, (count_zeta, count_omega))


# (e) ---------------------------------------------------------------------------------------------- call order and refusals
@pytest.mark.parametrize("name", ["6w3", "6w4"])
def test_call_order_and_refusals(shapes, name):
    s = shapes(name)
    lib, h = s.lib, s.h
    ids = (ctypes.c_int * 33)(*([Z] * 33))
    sc = np.ascontiguousarray(np.concatenate([s.lin_scalars, s.lin_scalars[:1]]))
    r_eval = np.full(4, SENTINEL, dtype=np.uint64)
    ev = np.full((33, 4), SENTINEL, dtype=np.uint64)
    pi = np.full((2, 12), SENTINEL, dtype=np.uint64)
    zeta, zo = s.zeta.ctypes.data, s.zeta_omega.ctypes.data
    top = s.top_scalar.ctypes.data if s.width == 3 else None

    def linearise(count, idp, scp, zp, outp):
        return lib.bbg_prover_linearise(h, count, idp, scp, zp, outp)

    def round6(cz, iz, sz, co, io, so, zp, zop, topp, a, b):
        return lib.bbg_prover_round6(h, cz, iz, sz, co, io, so, zp, zop, topp, a, b)

    def untouched():
        return (r_eval == SENTINEL).all() and (ev == SENTINEL).all() and (pi == SENTINEL).all()

    # a proof that has ended with round 6 leaves stage 0 until a new one has passed round 4
    s.prove(full=False)
    assert lib.bbg_prover_evaluate(h, 1, ids, None, zeta, ev.ctypes.data) == E_INVALID and b"round 4" in lib.bbg_last_error()
    assert linearise(1, ids, sc.ctypes.data, zeta, r_eval.ctypes.data) == E_INVALID and b"round 4" in lib.bbg_last_error()
    assert round6(1, ids, sc.ctypes.data, 1, ids, sc.ctypes.data, zeta, zo, top, pi[0].ctypes.data, pi[1].ctypes.data) == E_INVALID
    assert b"round 4" in lib.bbg_last_error()
    wp = (ctypes.c_void_p * 4)(*[a.ctypes.data for a in s.wires])
    com = np.zeros((4, 12), dtype=np.uint64)
    assert lib.bbg_prover_round1(h, wp, com.ctypes.data) == 0
    assert lib.bbg_prover_evaluate(h, 1, ids, None, zeta, ev.ctypes.data) == E_INVALID, "round 1 alone does not open round 5"
    assert linearise(1, ids, sc.ctypes.data, zeta, r_eval.ctypes.data) == E_INVALID
    assert untouched(), "a refused call wrote"
    assert np.array_equal(s.rounds_1_3_4(), s.baseline["com"])

    # bad arguments
    unknown = (ctypes.c_int * 2)(Z, 99)
    negative = (ctypes.c_int * 2)(Z, -1)
    wrong_width = [(ctypes.c_int * 2)(Z, W_1 + 3), (ctypes.c_int * 2)(Z, SIGMA_1 + 3)] if s.width == 3 else []
    mimc_only = (ctypes.c_int * 2)(Z, Q_MIMC_SELECTOR)  # never registered under these flavours
    for count in (0, 33):
        assert linearise(count, ids, sc.ctypes.data, zeta, r_eval.ctypes.data) == E_INVALID, count
    assert linearise(1, None, sc.ctypes.data, zeta, r_eval.ctypes.data) == E_INVALID
    assert linearise(1, ids, None, zeta, r_eval.ctypes.data) == E_INVALID
    assert linearise(1, ids, sc.ctypes.data, None, r_eval.ctypes.data) == E_INVALID
    assert linearise(1, ids, sc.ctypes.data, zeta, None) == E_INVALID
    for bad in [unknown, negative, mimc_only] + wrong_width:
        assert linearise(2, bad, sc.ctypes.data, zeta, r_eval.ctypes.data) == E_INVALID, list(bad)
    a, b = pi[0].ctypes.data, pi[1].ctypes.data
    scp = sc.ctypes.data
    assert round6(33, ids, scp, 1, ids, scp, zeta, zo, top, a, b) == E_INVALID
    assert round6(1, ids, scp, 33, ids, scp, zeta, zo, top, a, b) == E_INVALID
    assert round6(1, ids, scp, 0, ids, scp, zeta, zo, top, a, b) == E_INVALID, "count_omega = 0"
    for hole in (1, 2, 4, 5, 6, 7, 9, 10):  # every pointer but the top scalar, which has its own case below
        args = [1, ids, scp, 1, ids, scp, zeta, zo, top, a, b]
        args[hole] = None
        assert round6(*args) == E_INVALID, f"null argument {hole}"
    for bad in [unknown, negative, mimc_only] + wrong_width:
        assert round6(2, bad, scp, 1, ids, scp, zeta, zo, top, a, b) == E_INVALID, list(bad)
        assert round6(1, ids, scp, 2, bad, scp, zeta, zo, top, a, b) == E_INVALID, list(bad)
    if s.width == 3:
        assert round6(1, ids, scp, 1, ids, scp, zeta, zo, None, a, b) == E_INVALID and b"StandardPLONK" in lib.bbg_last_error()
    assert untouched(), "a refused call wrote"

    # the proof goes on as if nothing had been refused
    for count in (1, 5, 32):
        got = s.linearise(count)
        assert np.array_equal(prm.canon(got), s.want["lin"][count][1]), count
    assert np.array_equal(s.evaluate(s.eval_ids, s.eval_shifted, s.zeta), s.want["evals"]["generic"][1])
    points = s.round6(*ROUND6_DEFAULT)
    proof = {"pi": points, "openings": (s.read(OPENING), s.read(SHIFTED_OPENING))}
    s.check_round6(proof, f"{name} after the refusals", ROUND6_DEFAULT)
    assert lib.bbg_prover_evaluate(h, 1, ids, None, zeta, ev.ctypes.data) == E_INVALID, "round 6 closes the proof"
    assert linearise(1, ids, sc.ctypes.data, zeta, r_eval.ctypes.data) == E_INVALID
    assert untouched()


# option matrix ------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [0, 1, 2, 3, 4, 8])
@pytest.mark.parametrize("name", ["6w3", "6w4", "12w3"])
def test_option_prover_msm_batch(shapes, bbg, name, batch):
    """2 and 3 split the commitments of rounds 1 and 4 into uneven chunks (the second iteration of commit()'s loop, a last group of round 1
    shorter than the others); below 2 round 6 commits through two separate MSMs."""
    option_row(shapes(name), bbg, f"{name} prover_msm_batch={batch}", prover_msm_batch=batch)


@pytest.mark.parametrize("batch", [1, 4])
@pytest.mark.parametrize("window", [0, 13, 20])
def test_option_prover_tail_window(shapes, bbg, window, batch):
    s = shapes("11w4")
    before = bbg.msm_plan(s.n)
    assert before[0] == 8, "library default: 8-bit windows up to 2^13 terms (include/bbg.h, msm_window)"
    option_row(s, bbg, f"prover_tail_window={window} prover_msm_batch={batch}", prover_tail_window=window, prover_msm_batch=batch)
    assert bbg.msm_plan(s.n) == before, "the tail window outlived the commitments it was set for"
    with options(bbg, prover_tail_window=window, prover_msm_batch=batch):
        s.rounds_1_3_4()
        assert bbg.msm_plan(s.n) == before, "the tail window is still in place after round 4"
        s.linearise(32)
        s.round6(*ROUND6_DEFAULT)
        assert bbg.msm_plan(s.n) == before, "the tail window is still in place after round 6"


def test_tail_window_does_not_override_msm_window(shapes, bbg):
    s = shapes("11w4")
    with options(bbg, msm_window=16, prover_tail_window=13):
        assert bbg.msm_plan(s.n)[0] == 16
        proof = s.prove()
        assert bbg.msm_plan(s.n)[0] == 16, "an explicit msm_window was replaced by the tail window"
    s.check(proof, "msm_window=16 prover_tail_window=13")
    s.check_same_as_baseline(proof, "msm_window=16 prover_tail_window=13")


@pytest.mark.parametrize("limbs29", [1, 0])
@pytest.mark.parametrize("name", ["11w4", "12w3"])
def test_option_poly_limbs29(shapes, bbg, name, limbs29):
    """0 = the evaluations, r(X) and both opening sums on the 32-bit kernels (k_multi_eval_partial, k_poly_lincomb, k_eval_partial)."""
    option_row(shapes(name), bbg, f"{name} poly_limbs29={limbs29}", poly_limbs29=limbs29)


@pytest.mark.parametrize("limbs29,fuse,plan", [(1, 0, 1), (0, 1, 1), (0, 0, 1), (1, 1, 0), (0, 0, 0)])
@pytest.mark.parametrize("name", ["6w4", "6w3", "11w4", "12mimc"])
def test_option_quotient_paths(shapes, bbg, name, limbs29, fuse, plan):
    """Round 4's widget chain (csrc/quotient.hip) by every path: 29-bit or 32-bit limbs, arithmetic + range + logic fused or a kernel each, the
    set-up blocks by a wave's lanes or by one lane's chain -- blocks 1 to 4 of a chain start from what the block before handed on, which the
    one-widget tests never reach.  6w4: 4n = 256, one block exactly, the shifted rows wrap inside it; 6w3: the chain 5, 6, nothing to fuse;
    11w4: 32 blocks, the wrap from the last to the first; 12mimc: the chain 5, 7, 6."""
    what = f"{name} quotient_limbs29={limbs29} quotient_fuse={fuse} quotient_setup_plan={plan}"
    option_row(shapes(name), bbg, what, quotient_limbs29=limbs29, quotient_fuse=fuse, quotient_setup_plan=plan)


def test_option_unbatched_transforms_and_early_cosets(shapes, bbg):
    option_row(shapes("11w4"), bbg, "prover_ntt_batch=0 prover_early_cosets=1", prover_ntt_batch=0, prover_early_cosets=1)
