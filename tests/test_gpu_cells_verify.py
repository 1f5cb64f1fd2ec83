"""A batch of cell proofs reduced to the two points of one pairing check on the MI355X (bbg_cells_verify_reduce, csrc/cells_verify.hip).

Every comparison is bit-exact on canonical Montgomery words against the host model's device route (tests/tools/cells_verify_model.py), and
every result is also put to the pairing check itself in the form it takes for a known x: [x^l] L = R holds for an honest batch and fails
after any single corruption.  Honest proofs are the closed-form scalars times G over the powers string of X_INT; no FK20 run is needed but
in the last test, which verifies the proofs bbg_open_all makes."""
import ctypes

import numpy as np
import pytest

import cells_model as cm
import cells_verify_model as vm
import coarse_inputs as ci
import open_all_model as oa

pytestmark = pytest.mark.gpu

R = cm.R_MOD
Q = ci.Q_MOD
SEED = 0xBB254 + 0x7E81F
X_INT = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
SHAPES = [(1, 0), (2, 1), (3, 1), (4, 2), (6, 3), (7, 6), (9, 1), (13, 6)]
SRS_POINTS = 128  # l <= 64 in every test: the string is longer than any call reads
GUARD = 0xA5A5A5A5A5A5A5A5
RHO = 0x1F2E3D4C5B6A79880796A5B4C3D2E1F00F1E2D3C4B5A69788796A5B4C3D2E1F0 % R


@pytest.fixture(scope="module")
def string(bbg):
    srs = bbg.srs_synth_powers(cm.mont([X_INT])[0], SRS_POINTS)
    yield srs, srs.read()
    srs.free()


@pytest.fixture(scope="module")
def polys():
    """{(lg, c): coefficients} of random polynomials, made on first use and shared."""
    made = {}

    def get(lg, c):
        if (lg, c) not in made:
            made[(lg, c)] = cm.random_ints(SEED + 1000 * lg + c, 1 << lg)
        return made[(lg, c)]
    return get


@pytest.fixture(scope="module")
def honest(oracle, polys):
    """(lg, lc, ncom, cells) -> the honest batch (commitments, commitment ids, cell ids, values, proofs) of polynomials 0 .. ncom - 1."""
    def get(lg, lc, ncom, cells):
        return vm.honest_batch(oracle, [polys(lg, c) for c in range(ncom)], X_INT, lc, cells)
    return get


def device(bbg, srs, lg, lc, batch, rho):
    com, cids, mids, values, proofs = batch
    return bbg.cells_verify_reduce(srs, lg, lc, com, cids, mids, cm.mont(values), proofs, cm.mont([rho])[0])


def check(bbg, oracle, string, lg, lc, batch, rho, what, valid=True):
    srs, pts = string
    got = device(bbg, srs, lg, lc, batch, rho)
    L, R_ = vm.reduce_route(oracle, pts, lg, lc, *batch, rho)
    assert np.array_equal(got[0], L), f"({lg}, {lc}) {what}: L differs from the model"
    assert np.array_equal(got[1], R_), f"({lg}, {lc}) {what}: R differs from the model"
    assert vm.holds(oracle, got[0], got[1], X_INT, lc) == valid, f"({lg}, {lc}) {what}: [x^l] L = R must {'hold' if valid else 'fail'}"
    return got


def random_cells(seed, r, ncom, K):
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(0, ncom)), int(rng.integers(0, r))) for _ in range(K)]


def lifted_scalars(words):
    out = ci.add_int(words, R)
    assert ci.below(out, 2 * R).all() and not ci.below(out, R).any()
    return out


def lifted_points(points):
    """Both coordinates of every finite point moved into [p, 2p)."""
    p = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8).copy()
    finite = np.array([not oa.is_infinity(row) for row in p])
    p[finite] = ci.add_int(p[finite].reshape(-1, 4), Q).reshape(-1, 8)
    return p


# 1 ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("lg,lc", SHAPES)
def test_shapes(bbg, oracle, string, honest, lg, lc):
    n, l, r = cm.shape(lg, lc)
    check(bbg, oracle, string, lg, lc, honest(lg, lc, 2, random_cells(SEED + 16 * lg + lc, r, 2, 5)), RHO, "ncom = 2, K = 5")
    check(bbg, oracle, string, lg, lc, honest(lg, lc, 1, [(0, r - 1)]), RHO, "one cell, the last")


# 2 ------------------------------------------------------------------------------------------------ batch sizes
@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 257])
def test_batch_sizes(bbg, oracle, string, honest, K):
    lg, lc = 9, 1  # r = 256: K = 257 repeats a cell
    check(bbg, oracle, string, lg, lc, honest(lg, lc, 3, random_cells(SEED + K, 256, 3, K)), RHO, f"K = {K}")


def test_full_grid_13_6(bbg, oracle, string, honest):
    lg, lc, ncom = 13, 6, 8
    n, l, r = cm.shape(lg, lc)
    cells = [(c, m) for m in range(r) for c in range(ncom)]
    check(bbg, oracle, string, lg, lc, honest(lg, lc, ncom, cells), RHO, "every cell of 8 polynomials")


# 3 ------------------------------------------------------------------------------------------------ grouping
def grouping_cases():
    r = 256
    rng = np.random.default_rng(SEED + 33)
    long_groups = [(k % 3, 5) for k in range(300)] + [(k % 3, 9) for k in range(70)] + [(0, 200), (1, 201), (2, 255)]
    return {"all cells in one group": [(c, 17) for c in range(6)],
            "every group of size one": [(m % 3, m) for m in range(r)],
            "every group of size one, shuffled": [(m % 3, int(m)) for m in rng.permutation(r)],
            "groups of 300 and 70 beside single cells": long_groups,
            "the same, shuffled": [long_groups[i] for i in rng.permutation(len(long_groups))]}


@pytest.mark.parametrize("name", list(grouping_cases()))
def test_grouping(bbg, oracle, string, honest, name):
    cells = grouping_cases()[name]
    check(bbg, oracle, string, 9, 1, honest(9, 1, max(c for c, _ in cells) + 1, cells), RHO, name)


# 4 ------------------------------------------------------------------------------------------------ commitments
def test_commitment_counts(bbg, oracle, string, honest):
    lg, lc = 6, 3
    check(bbg, oracle, string, lg, lc, honest(lg, lc, 1, [(0, 1), (0, 6), (0, 3)]), RHO, "ncom = 1")
    check(bbg, oracle, string, lg, lc, honest(lg, lc, 5, [(c, (3 * c) % 8) for c in range(5)]), RHO, "ncom = K")
    check(bbg, oracle, string, lg, lc, honest(lg, lc, 3, [(0, 1), (2, 6), (2, 3), (0, 0)]), RHO, "commitment 1 is referred to by nobody")


# 5 ------------------------------------------------------------------------------------------------ duplicates, cancellation, special rho
def test_duplicates_and_special_challenges(bbg, oracle, string, honest):
    lg, lc = 6, 3
    srs, pts = string
    check(bbg, oracle, string, lg, lc, honest(lg, lc, 2, [(1, 4), (0, 2), (1, 4)]), RHO, "the same cell twice")
    got = check(bbg, oracle, string, lg, lc, honest(lg, lc, 1, [(0, 5), (0, 5)]), R - 1, "the same cell twice, rho = -1")
    assert np.array_equal(got, np.stack([oa.aff_infinity()] * 2)), "L = R = infinity in the documented encoding"
    cells = [(0, 5), (1, 2), (1, 7)]
    zero = check(bbg, oracle, string, lg, lc, honest(lg, lc, 2, cells), 0, "rho = 0")
    alone = device(bbg, srs, lg, lc, honest(lg, lc, 2, cells[:1]), RHO)
    assert np.array_equal(zero, alone), "with rho = 0 only cell 0 counts"
    check(bbg, oracle, string, lg, lc, honest(lg, lc, 2, cells), 1, "rho = 1")


# 6 ------------------------------------------------------------------------------------------------ infinities as data
def test_infinite_proofs_and_commitments(bbg, oracle, string, polys):
    lg, lc = 6, 3
    n, l, r = cm.shape(lg, lc)
    low = cm.random_ints(SEED + 60, l) + [0] * (n - l)  # degree < l: every proof is infinity
    fs = [low, [0] * n, polys(lg, 0)]                   # the zero polynomial: its commitment is infinity too
    b = vm.honest_batch(oracle, fs, X_INT, lc, [(0, 1), (0, 6)])
    assert all(oa.is_infinity(p) for p in b[4]) and not oa.is_infinity(b[0][0]) and oa.is_infinity(b[0][1])
    got = check(bbg, oracle, string, lg, lc, b, RHO, "a polynomial of degree < l")
    assert np.array_equal(got, np.stack([oa.aff_infinity()] * 2))
    check(bbg, oracle, string, lg, lc, vm.honest_batch(oracle, fs, X_INT, lc, [(1, 3), (1, 0)]), RHO, "the zero polynomial")
    check(bbg, oracle, string, lg, lc, vm.honest_batch(oracle, fs, X_INT, lc, [(2, 3), (0, 3), (1, 3), (2, 0), (1, 5), (0, 0)]), RHO, "a mixed batch")


# 7 ------------------------------------------------------------------------------------------------ non-canonical inputs
def test_lifted_inputs(bbg, oracle, string, honest):
    lg, lc = 6, 3
    srs, pts = string
    com, cids, mids, values, proofs = honest(lg, lc, 2, [(1, 4), (0, 2), (1, 7), (0, 4)])
    want = check(bbg, oracle, string, lg, lc, (com, cids, mids, values, proofs), RHO, "canonical inputs")
    v, rho = cm.mont(values), cm.mont([RHO])
    assert np.array_equal(bbg.cells_verify_reduce(srs, lg, lc, com, cids, mids, lifted_scalars(v), proofs, lifted_scalars(rho)[0]), want), "values, rho in [r, 2r)"
    assert np.array_equal(bbg.cells_verify_reduce(srs, lg, lc, lifted_points(com), cids, mids, v, lifted_points(proofs), rho[0]), want), "coordinates in [p, 2p)"


# 8 ------------------------------------------------------------------------------------------------ soundness
def test_single_corruptions(bbg, oracle, string, honest):
    lg, lc = 6, 3
    n, l, r = cm.shape(lg, lc)
    com, cids, mids, values, proofs = honest(lg, lc, 2, [(1, 4), (0, 2), (1, 7), (0, 4)])
    other = vm.scalar_times_generator(oracle, [12345])[0]
    v2 = list(values)
    v2[l + 3] = (v2[l + 3] + 1) % R
    p2, c2 = proofs.copy(), com.copy()
    p2[1], c2[1] = other, other
    m2, i2 = list(mids), list(cids)
    m2[2], i2[1] = (m2[2] + 1) % r, 1 - i2[1]
    cases = {"one value": (com, cids, mids, v2, proofs), "one proof": (com, cids, mids, values, p2), "one commitment": (c2, cids, mids, values, proofs),
             "one cell id": (com, cids, m2, values, proofs), "one commitment id": (com, i2, mids, values, proofs)}
    for what, batch in cases.items():
        check(bbg, oracle, string, lg, lc, batch, RHO, what + " changed", valid=False)


# 9 ------------------------------------------------------------------------------------------------ points off the curve
def test_off_curve_points(bbg, pkg, oracle, string, honest):
    lg, lc = 6, 3
    n, l, r = cm.shape(lg, lc)
    srs, pts = string
    com, cids, mids, values, proofs = honest(lg, lc, 2, [(1, 4), (0, 2), (1, 7), (0, 4)])
    bad_p, bad_c = proofs.copy(), com.copy()
    bad_p[2, 4:] = ci.add_int(bad_p[2, 4:], 1)[0]  # y + 1
    bad_c[0, 4:] = ci.add_int(bad_c[0, 4:], 1)[0]
    assert not oracle.g1_on_curve(bad_p[2]) and not oracle.g1_on_curve(bad_c[0])
    v, rho = cm.mont(values), cm.mont([RHO])[0]
    K = len(mids)
    bufs = [bbg.dev_alloc(b) for b in (2 * 64, K * l * 32, K * 64, 128, 4)]
    d_com, d_val, d_prf, d_out, d_cnt = bufs
    try:
        bbg.dev_upload(d_val, v)
        for c, p, want in ((bad_c, bad_p, 2), (com, bad_p, 1), (bad_c, proofs, 1), (com, proofs, 0)):  # the last call is honest and follows three bad ones
            bbg.dev_upload(d_com, c)
            bbg.dev_upload(d_prf, p)
            bbg.dev_upload(d_cnt, np.full(1, 0xFFFFFFFF, dtype=np.uint32))
            bbg.cells_verify_reduce_device(srs, lg, lc, d_com, 2, cids, mids, d_val, d_prf, rho, d_out, d_cnt)
            assert int(bbg.dev_download(d_cnt, (1,), dtype=np.uint32)[0]) == want
        L, R_ = vm.reduce_route(oracle, pts, lg, lc, com, cids, mids, values, proofs, RHO)
        assert np.array_equal(bbg.dev_download(d_out, (2, 8)), np.stack([L, R_])), "the honest call after the bad ones"
    finally:
        for d in bufs:
            bbg.dev_free(d)
    # the host form: BBG_E_INVALID, out untouched
    out = np.full((2, 8), GUARD, dtype=np.uint64)
    ids_c, ids_m = np.ascontiguousarray(cids, dtype=np.uint32), np.ascontiguousarray(mids, dtype=np.uint32)
    rc = bbg.lib.bbg_cells_verify_reduce(bbg.ctx, srs.handle, lg, lc, com.ctypes.data, 2, ids_c.ctypes.data, ids_m.ctypes.data, K, v.ctypes.data,
                                         bad_p.ctypes.data, rho.ctypes.data, out.ctypes.data)
    assert rc == -1 and b"not on the curve" in bbg.lib.bbg_last_error() and (out == GUARD).all()
    with pytest.raises(pkg.BbgError):
        bbg.cells_verify_reduce(srs, lg, lc, bad_c, cids, mids, v, proofs, rho)


# 10 ----------------------------------------------------------------------------------------------- the device entry
def test_device_entry_and_argument_errors(bbg, oracle, string, honest):
    lg, lc = 6, 3
    n, l, r = cm.shape(lg, lc)
    srs, pts = string
    com, cids, mids, values, proofs = honest(lg, lc, 2, [(1, 4), (0, 2), (1, 7), (0, 4)])
    K = len(mids)
    v, rho = cm.mont(values), cm.mont([RHO])[0]
    L, R_ = vm.reduce_route(oracle, pts, lg, lc, com, cids, mids, values, proofs, RHO)
    ins = np.concatenate([com.reshape(-1), v.reshape(-1), proofs.reshape(-1)])  # one input buffer: commitments | values | proofs
    d_in, d_out = bbg.dev_alloc(ins.nbytes), bbg.dev_alloc(128 + 64)
    d_com, d_val, d_prf = d_in, d_in + com.nbytes, d_in + com.nbytes + v.nbytes
    guard = np.full(24, GUARD, dtype=np.uint64)
    c32, m32 = np.ascontiguousarray(cids, dtype=np.uint32), np.ascontiguousarray(mids, dtype=np.uint32)
    lib = bbg.lib
    short = bbg.srs_synth_powers(cm.mont([X_INT])[0], l - 1)

    def call(srs_h=srs.handle, a=lg, b=lc, dc=d_com, ncom=2, ci_=c32.ctypes.data, mi=m32.ctypes.data, k=K, dv=d_val, dp=d_prf, rh=rho.ctypes.data, do=d_out,
             dn=None, ctx=None):
        return lib.bbg_cells_verify_reduce_device(bbg.ctx if ctx is None else ctx, srs_h, a, b, dc, ncom, ci_, mi, k, dv, dp, rh, do, dn)

    try:
        bbg.dev_upload(d_in, ins)
        bbg.dev_upload(d_out, guard)
        assert call() == 0  # d_off_curve = NULL
        got = bbg.dev_download(d_out, (24,))
        assert np.array_equal(got[:16].reshape(2, 8), np.stack([L, R_])) and (got[16:] == GUARD).all(), "L, R, then the guard words"
        assert np.array_equal(bbg.dev_download(d_in, ins.shape), ins), "the inputs were written"
        bbg.dev_upload(d_out, guard)
        bad_c, bad_m = c32.copy(), m32.copy()
        bad_c[3], bad_m[0] = 2, r
        errors = {"null srs": dict(srs_h=None), "null commitments": dict(dc=None), "null commitment ids": dict(ci_=None), "null cell ids": dict(mi=None),
                  "null values": dict(dv=None), "null proofs": dict(dp=None), "null rho": dict(rh=None), "null output": dict(do=None), "K = 0": dict(k=0),
                  "ncom = 0": dict(ncom=0), "a commitment id = ncom": dict(ci_=bad_c.ctypes.data), "a cell id = r": dict(mi=bad_m.ctypes.data),
                  "log2n = 0": dict(a=0, b=0), "log2n = 29": dict(a=29), "log2cell = log2n": dict(b=lg), "l above the SRS length": dict(srs_h=short.handle),
                  "the output on the commitments": dict(do=d_com), "the output on the last value": dict(do=d_val + v.nbytes - 32),
                  "the output on the last proof": dict(do=d_prf + proofs.nbytes - 64), "the count on a proof": dict(dn=d_prf + 8),
                  "the count on the output": dict(dn=d_out + 124)}
        for what, kw in errors.items():
            assert call(**kw) == -1 and lib.bbg_last_error(), what
        host = np.full((2, 8), GUARD, dtype=np.uint64)
        assert lib.bbg_cells_verify_reduce(bbg.ctx, srs.handle, lg, lc, com.ctypes.data, 2, c32.ctypes.data, bad_m.ctypes.data, K, v.ctypes.data,
                                           proofs.ctypes.data, rho.ctypes.data, host.ctypes.data) == -1 and (host == GUARD).all()
        assert lib.bbg_cells_verify_reduce(bbg.ctx, srs.handle, lg, lc, None, 2, c32.ctypes.data, m32.ctypes.data, K, v.ctypes.data,
                                           proofs.ctypes.data, rho.ctypes.data, host.ctypes.data) == -1 and (host == GUARD).all()
        bbg.sync()
        assert (bbg.dev_download(d_out, (24,)) == GUARD).all(), "an argument error wrote the output"
        assert np.array_equal(bbg.dev_download(d_in, ins.shape), ins), "an argument error wrote an input"
        # the neighbours are legal: the count right behind the output, the working memory back after a trim
        assert call(dn=d_out + 128) == 0
        assert bbg.memory_trim() > 0
        assert call(dn=d_out + 128) == 0
        got = bbg.dev_download(d_out, (24,))
        assert np.array_equal(got[:16].reshape(2, 8), np.stack([L, R_])) and int(got[16]) == (GUARD >> 32) << 32
    finally:
        short.free()
        bbg.dev_free(d_in)
        bbg.dev_free(d_out)


# 11 ----------------------------------------------------------------------------------------------- single-point openings: bbg_open_all's proofs
def test_log2cell_0_verifies_open_all(bbg, oracle, string):
    lg = 6
    n = 1 << lg
    srs, pts = string
    f = cm.random_ints(SEED + 110, n)
    words = cm.mont(f)
    h = bbg.open_all_prepare(srs, lg)
    try:
        proofs = h.open(words)
    finally:
        h.free()
    values = bbg.ntt(words)  # f(w^m) at index m: with l = 1 cell m is the point w^m
    commitment = oa.canon_points(oracle, oracle.jac_to_affine(bbg.msm(srs, words)))
    ids = [int(m) for m in np.random.default_rng(SEED + 111).permutation(n)]
    got = bbg.cells_verify_reduce(srs, lg, 0, commitment, [0] * n, ids, values[ids], proofs[ids], cm.mont([RHO])[0])
    assert not oa.is_infinity(got[0]) and vm.holds(oracle, got[0], got[1], X_INT, 0), "[x] L = R for the proofs of bbg_open_all"
    wrong = values[ids].copy()
    wrong[7] = values[ids[8]]
    got = bbg.cells_verify_reduce(srs, lg, 0, commitment, [0] * n, ids, wrong, proofs[ids], cm.mont([RHO])[0])
    assert not vm.holds(oracle, got[0], got[1], X_INT, 0), "a wrong value must fail"
