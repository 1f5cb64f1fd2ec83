"""GPU tests over the whole coarse input range [0, 2p) (run with -m gpu on an MI355X).

include/bbg.h accepts any representative in [0, 2p) and every device array is meant to hold one, in and out; the 29-bit-limb kernels rely
on those bounds (tests/test_ntt29_model.py, tests/test_w29_model.py).  The rest of the GPU suite draws inputs below 2^252 (the bottom sixth
of [0, 2r)) and compares outputs after canonicalising them, so an input near 2p or an output in [2p, 2^256) would pass unnoticed.  Here the
kernels get the whole range and its edges (tests/tools/coarse_inputs.py) and every result is checked twice: its canonical value against
the oracle, a big-integer reference or a digest recorded from the compiled reference, and its raw words against 2p on all 256 bits.
The MSM gets scalars whose signed-digit recoding hits the top bucket, carry-made zero digits and carry chains on every term, and point
tables with coordinates in [q, 2q)."""
import functools

import numpy as np
import pytest

import coarse_inputs as ci
from conftest import sha, unhex

pytestmark = pytest.mark.gpu

FFT, IFFT, COSET_FFT, COSET_IFFT = 0, 1, 2, 3
MSM_WINDOWS = ci.MSM_WINDOWS
ACCUMULATORS = ((1, 1), (0, 1), (0, 0))  # (msm_accumulate_quad, msm_limbs29): four-lane kernel, 29-bit limbs, 32-bit limbs


@functools.lru_cache(maxsize=None)
def _coarse(seed, n, which=0):
    w = ci.coarse_scalars(seed, n, which)
    w.setflags(write=False)
    return w


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).reshape(-1).copy()).cuda()


def _host(bbg, t, n):
    bbg.sync()
    return t.cpu().numpy().view(np.uint64).reshape(n, 4)


def _check(oracle, got, want, what, which=0):
    """The device's words are below 2p and canonically equal to the reference's."""
    ci.assert_coarse(got, which, what)
    assert np.array_equal(oracle.canon(which, got), oracle.canon(which, np.reshape(want, (-1, 4)))), what


def _coarse_constant(golden):
    """The NTT's golden constant and its representative in [p, 2p)."""
    kc = unhex(golden["ntt_constant"])[0]
    return kc, ci.add_int(kc, ci.R_MOD)[0]


# ---------------------------------------------------------------------------------------------- fields
@pytest.mark.parametrize("which", [0, 1])
def test_field_ops_on_the_catalogue(oracle, bbg, which):
    """bbg_field_op ops 0-5 and 8-11 on every pair of edge values of [0, 2p) against Python integers."""
    cat = ci.catalogue(which)
    a_int = [x for x in cat for _ in cat]
    b_int = [y for _ in cat for y in cat]
    a, b = ci.to_words(a_int), ci.to_words(b_int)
    p = ci.MODULI[which]
    mul = [ci.mont_mul(x, y, which) for x, y in zip(a_int, b_int)]
    want = {0: mul, 3: mul,
            1: [ci.mont_add(x, y, which) for x, y in zip(a_int, b_int)],
            2: [ci.mont_sub(x, y, which) for x, y in zip(a_int, b_int)],
            8: [(ci.mont_mul(x, x, which) - ci.mont_mul(y, y, which)) % p for x, y in zip(a_int, b_int)],
            9: [2 * m % p for m in mul]}
    for op, w in want.items():
        _check(oracle, bbg.field_op(which, op, a, b), ci.to_words(w), (which, op), which)
    c = ci.to_words(cat)
    for op, fn in ((4, ci.from_mont), (5, ci.to_mont), (10, ci.mont_inv), (11, ci.mont_inv)):
        _check(oracle, bbg.field_op(which, op, c), ci.to_words([fn(v, which) for v in cat]), (which, op), which)


@pytest.mark.parametrize("which", [0, 1])
def test_raw_montgomery_products(oracle, bbg, which):
    """Ops 6 / 7: fe_mul and fe_mul_cios with no pre-reduction, on operands in [0, 2p) and on a < 4p with b < p (field.hip.h: the result
    is then still < 2p)."""
    p = ci.MODULI[which]
    cat = ci.catalogue(which)
    a_int = [x for x in cat for _ in cat] + ci.coarse_ints(60 + which, 4000, which)
    b_int = [y for _ in cat for y in cat] + ci.coarse_ints(61 + which, 4000, which)
    for op in (6, 7):
        got = bbg.field_op(which, op, ci.to_words(a_int), ci.to_words(b_int))
        _check(oracle, got, ci.to_words([ci.mont_mul(x, y, which) for x, y in zip(a_int, b_int)]), (which, op, "2p"), which)
    a4 = [x + 2 * p for x in ci.coarse_ints(62 + which, 2000, which)] + [4 * p - 1, 2 * p, 3 * p]
    b1 = [y % p for y in ci.coarse_ints(63 + which, 2000, which)] + [p - 1, p - 1, 1]
    for op in (6, 7):
        got = bbg.field_op(which, op, ci.to_words(a4), ci.to_words(b1))
        _check(oracle, got, ci.to_words([ci.mont_mul(x, y, which) for x, y in zip(a4, b1)]), (which, op, "4p x p"), which)


# ---------------------------------------------------------------------------------------------- NTT, small sizes
@pytest.mark.parametrize("lg", [0, 1, 2, 3, 4, 5, 7, 9, 10, 11, 12, 13, 14, 15, 16])
def test_ntt_all_ops_coarse(oracle, bbg, golden, lg):
    """bbg_ntt ops 0-7 on inputs spread over [0, 2r), with and without generator_size = n / 4, with the constant in [0, r) and in [r, 2r);
    against the oracle, and for n <= 2^10 against an O(n^2) big-integer DFT too."""
    n = 1 << lg
    c = _coarse(0xC0A + lg, n)
    kc, kc2 = _coarse_constant(golden)
    for op in range(8):
        for k in ((kc, kc2) if op >= 4 else (None,)):
            _check(oracle, bbg.ntt(c, op, 0, k), oracle.ntt(c, op, 0, k), (lg, op))
    if lg >= 2:
        for op in (2, 5, 6):
            for k in ((kc, kc2) if op >= 4 else (None,)):
                _check(oracle, bbg.ntt(c, op, n // 4, k), oracle.ntt(c, op, n // 4, k), (lg, op, "gs"))
    if lg <= 10:
        vals = ci.to_ints(c)
        for op in ((0, 1, 2, 3) if lg <= 8 else (0, 3)):
            got = bbg.ntt(c, op)
            ci.assert_coarse(got, 0, (lg, op, "dft"))
            assert ci.to_ints(oracle.canon(0, got)) == ci.dft(vals, op), (lg, op, "dft")


# ---------------------------------------------------------------------------------------------- NTT, every plan
def _plan_cases(oracle, bbg, lgs, what, coset_gs=True):
    for lg in lgs:
        n = 1 << lg
        c = _coarse(0xC1A + lg, n)
        _check(oracle, bbg.ntt(c, FFT), oracle.ntt(c, 0), (what, lg, "fft"))
        _check(oracle, bbg.ntt(c, COSET_IFFT), oracle.ntt(c, 3), (what, lg, "coset_ifft"))
        if coset_gs and lg >= 2:  # the zero-extended input: fused into the first pass's load where the plan can (ntt.hip can_fuse)
            _check(oracle, bbg.ntt(c, COSET_FFT, n // 4), oracle.ntt(c, 2, n // 4), (what, lg, "coset_fft gs"))
            _check(oracle, bbg.ntt(c, COSET_FFT), oracle.ntt(c, 2), (what, lg, "coset_fft"))


@pytest.mark.parametrize("tile,maxr", [(12, 9), (11, 8), (10, 6), (9, 5)])
def test_ntt_pass_plans_coarse(oracle, bbg, tile, maxr):
    bbg.set_option("ntt_tile_log", tile)
    bbg.set_option("ntt_max_logr", maxr)
    try:
        _plan_cases(oracle, bbg, (12, 14, 17), ("tile", tile, maxr))
    finally:
        bbg.set_option("ntt_tile_log", 10)
        bbg.set_option("ntt_max_logr", 7)


@pytest.mark.parametrize("planes", [2, 1, 29])
def test_ntt_pass8_plans_coarse(oracle, bbg, planes):
    """k_ntt_pass8 / k_ntt_pass8s / k_ntt_pass29 under every per-pass radix limit; single-pass plans take the unfused coset load."""
    bbg.set_option("ntt_kernel", 2)
    bbg.set_option("ntt_lds_planes", planes if planes != 29 else 0)
    bbg.set_option("ntt_limbs29", 1 if planes == 29 else 0)
    try:
        for maxr8 in (6, 7, 8, 9, 10, 11):
            bbg.set_option("ntt_max_logr8", maxr8)
            _plan_cases(oracle, bbg, (9, 11, 13, 16) if maxr8 in (6, 10) else (12, 17), ("pass8", planes, maxr8))
    finally:
        bbg.set_option("ntt_max_logr8", 10)
        bbg.set_option("ntt_lds_planes", 0)
        bbg.set_option("ntt_limbs29", -1)


def test_ntt_kernel_v1_coarse(oracle, bbg):
    bbg.set_option("ntt_kernel", 1)
    try:
        _plan_cases(oracle, bbg, (11, 14, 18), "kernel 1")
    finally:
        bbg.set_option("ntt_kernel", 2)


# ---------------------------------------------------------------------------------------------- NTT, full size, tied to the reference
def _full_size_records(golden, lg):
    import json
    import os
    if lg in (18, 20):
        return [r for r in golden["ntt"] if r["log2n"] == lg and r["op"] < 4 and r["generator_size"] == 0]
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ntt_large.json")) as f:
        return [r for r in json.load(f)["ntt"] if r["log2n"] == lg]


def _powers(oracle, t, n):
    """t^0 .. t^(n-1) (Montgomery) by log-depth doubling: log2(n) vectorised oracle products."""
    pw = oracle.to_mont(0, np.array([[1, 0, 0, 0]], dtype=np.uint64))
    step = np.ascontiguousarray(t, dtype=np.uint64).reshape(1, 4)
    while pw.shape[0] < n:
        pw = np.concatenate([pw, oracle.fe_mul(0, pw, np.repeat(step, pw.shape[0], axis=0))])
        step = oracle.fe_mul(0, step, step)
    return pw[:n]


@pytest.mark.parametrize("lg", [20, 22, 24])
def test_ntt_full_size_high_range_vs_reference_digests(pkg, oracle, bbg, golden, lg):
    """x + r (x the recorded seed's scalars, so x + r lies in [r, r + 2^252) within [0, 2r)) through every op and pass kernel: the canonical
    output hashes to the REFERENCE's digest of x's transform, and the raw output stays below 2r.  Then the middle of the range through
    linearity with a closed form: v_j = c w^(-jk) gives fft(x + v) = fft(x) + n c delta_k, with x + v in [0, r + 2^252).  Round trips
    take the inverse and coset ops over the same coarse vectors."""
    import torch
    n = 1 << lg
    recs = _full_size_records(golden, lg)
    assert sorted(r["op"] for r in recs) == [0, 1, 2, 3]
    seed = recs[0]["seed"]
    assert all(r["seed"] == seed for r in recs)
    x = pkg.synthetic_scalars(seed, n)
    xp = _dev(ci.add_int(x, ci.R_MOD))

    def run(op, src):
        work = src.clone()
        bbg.ntt_device(work.data_ptr(), lg, op)
        return _host(bbg, work, n)

    configs = {20: [(1, 2), (1, 1), (1, 29)], 22: [(0, 2), (2, 1), (0, 29), (2, 29)], 24: [(1, 0), (1, 29)]}[lg]  # (big tile, planes)
    fx = None
    try:
        for big, planes in configs:
            bbg.set_option("ntt_big_tile", big)
            bbg.set_option("ntt_lds_planes", planes if planes not in (0, 29) else 0)
            bbg.set_option("ntt_limbs29", 1 if planes == 29 else (-1 if planes == 0 else 0))
            for rec in recs:
                out = run(rec["op"], xp)
                ci.assert_coarse(out, 0, (lg, rec["op"], big, planes))
                canon = oracle.canon(0, out)
                assert sha(canon) == rec["sha256"], (lg, rec["op"], big, planes)
                if rec["op"] == FFT:
                    fx = canon
    finally:
        bbg.set_option("ntt_big_tile", 1)
        bbg.set_option("ntt_lds_planes", 0)
        bbg.set_option("ntt_limbs29", -1)
    # linearity with a closed form: the middle of the range
    k = 3 + (n >> 1) // 3
    c = oracle.canon(0, _coarse(0xC2A, 1)[0:1])
    w_inv_k = oracle.fe_inv(0, _powers(oracle, oracle.root_of_unity(lg), k + 1)[k:k + 1])
    v = oracle.canon(0, oracle.fe_mul(0, _powers(oracle, w_inv_k, n), np.repeat(c, n, axis=0)))
    xv = ci.add_words(x, v)
    assert ci.below(xv, ci.R_MOD + (1 << 252)).all()
    got = run(FFT, _dev(xv))
    ci.assert_coarse(got, 0, (lg, "x + v"))
    want = fx.copy()
    nc = oracle.fe_mul(0, c, oracle.to_mont(0, np.array([[n, 0, 0, 0]], dtype=np.uint64)))
    want[k] = oracle.fe_add(0, want[k:k + 1], nc)[0]
    assert np.array_equal(oracle.canon(0, got), want), (lg, "fft(x + v) = fft(x) + n c delta_k")
    del got, want, v
    # round trips on the coarse vectors
    for fwd, inv in ((FFT, IFFT), (COSET_FFT, COSET_IFFT)):
        for src, ref in ((xp, x), (_dev(xv), xv)):
            work = src.clone()
            bbg.ntt_device(work.data_ptr(), lg, fwd)
            bbg.ntt_device(work.data_ptr(), lg, inv)
            back = _host(bbg, work, n)
            ci.assert_coarse(back, 0, (lg, fwd, "round trip"))
            assert np.array_equal(oracle.canon(0, back), oracle.canon(0, ref)), (lg, fwd, "round trip")
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------- other Fr kernels
def test_coset_fft_split_and_extend_coarse(oracle, bbg):
    for lg, ext in ((10, 4), (12, 8), (11, 2)):
        c = _coarse(0xC3A + lg, 1 << lg)
        _check(oracle, bbg.coset_fft_split(c, ext), oracle.coset_fft_split(c, ext), ("split", lg, ext))
    for lg, dom in ((10, 12), (12, 14), (3, 5)):
        c = _coarse(0xC3B + lg, 1 << lg)
        pad = np.zeros((1 << dom, 4), dtype=np.uint64)
        pad[: 1 << lg] = c
        want = oracle.ntt(pad, 2, 1 << lg)
        _check(oracle, bbg.coset_fft_extend(c, dom), np.concatenate([want, want[:4]]), ("extend", lg, dom))


@pytest.mark.parametrize("G,lg,inverse,coset", [(2, 12, False, False), (4, 12, False, True), (8, 13, False, False), (8, 12, True, False),
                                                 (4, 14, True, True)])
def test_sharded_ntt_device_blocks_coarse(pkg, oracle, bbg, G, lg, inverse, coset):
    """scale_powers_device / the local NTT / cross_dft_device composed as in tests/test_gpu_parity.py::test_sharded_ntt_device_blocks, on
    coarse inputs and with the scale bases and starts handed in as representatives in [r, 2r); every intermediate stays below 2r."""
    import importlib
    import torch
    par = importlib.import_module("aztec_amd.parallel")
    ops = par.BbgNttOps(bbg)
    n = 1 << lg
    m, lenq, log2g = n // G, n // G // G, G.bit_length() - 1
    a = _coarse(0xC4A + lg + G, n)
    five = oracle.to_mont(0, np.array([[5, 0, 0, 0]], dtype=np.uint64))[0]

    def hi(w):  # the [r, 2r) representative of a canonical value
        return ci.add_int(oracle.canon(0, np.reshape(w, (1, 4))), ci.R_MOD)[0]
    want = oracle.ntt(a, (3 if coset else 1) if inverse else (2 if coset else 0))
    Z = []
    for g in range(G):
        x = _dev(a[g::G])
        if coset and not inverse:
            ops.scale_powers(x, m, hi(ops.fr_pow(five, G)), hi(ops.fr_pow(five, g)))
            ci.assert_coarse(_host(bbg, x, m), 0, "scale_powers")
        ops.ntt(x, lg - log2g, 1 if inverse else 0)
        start = hi(par._mont_limbs(pow(G, -1, par._R_MOD))) if inverse else None
        ops.scale_powers(x, m, hi(ops.root_pow(lg, g, inverse)), start)
        ci.assert_coarse(_host(bbg, x, m), 0, "scale_powers")
        Z.append(x)
    bbg.sync()
    got = np.zeros((n, 4), dtype=np.uint64)
    for r in range(G):
        recv = torch.cat([Z[s][4 * r * lenq: 4 * (r + 1) * lenq] for s in range(G)])
        out = torch.empty_like(recv)
        ops.cross_dft(recv, out, log2g, lenq, lg, inverse)
        o = _host(bbg, out, G * lenq)
        ci.assert_coarse(o, 0, "cross_dft")
        o = o.reshape(G, lenq, 4)
        for t in range(G):
            got[r * lenq + m * t: r * lenq + m * t + lenq] = o[t]
    got = oracle.canon(0, got)
    if inverse and coset:
        got = oracle.fe_mul(0, got, _powers(oracle, oracle.fe_inv(0, five.reshape(1, 4)), n))
    assert np.array_equal(oracle.canon(0, got), want)


def test_poly_helpers_coarse(oracle, bbg, golden):
    """poly_op_device (add / sub / mul), poly_evaluate(_device), kate_opening(_device) (also in place) and
    divide_by_pseudo_vanishing(_device) on coarse coefficients and points z in [0, r) and [r, 2r), at ragged sizes."""
    import torch
    kc, kc2 = _coarse_constant(golden)
    for n in (1, 17, 4096, 4097, 70001):
        a_np, b_np = _coarse(0xC5A + n, n), _coarse(0xC5B + n, n)
        a, b = _dev(a_np), _dev(b_np)
        for op in (0, 1, 2):
            r = torch.empty_like(a)
            bbg.poly_op_device(op, a.data_ptr(), b.data_ptr(), r.data_ptr(), n)
            _check(oracle, _host(bbg, r, n), oracle.poly_binop(op, a_np, b_np), ("poly_op", op, n))
        for z in (kc, kc2):
            want = oracle.poly_eval(a_np, z)
            for got in (bbg.poly_evaluate_device(a.data_ptr(), n, z), bbg.poly_evaluate(a_np, z)):
                _check(oracle, got, want, ("evaluate", n))
            want_d, want_f = oracle.kate_opening(a_np, z)
            d = torch.zeros_like(a)
            f = bbg.kate_opening_device(a.data_ptr(), d.data_ptr(), n, z)
            _check(oracle, f, want_f, ("kate f", n))
            _check(oracle, _host(bbg, d, n), want_d, ("kate", n))
            for in_place in (False, True):
                d2, f2 = bbg.kate_opening(a_np, z, in_place=in_place)
                _check(oracle, f2, want_f, ("kate f host", n, in_place))
                _check(oracle, d2, want_d, ("kate host", n, in_place))
        if n == 4097:  # Horner on big integers for one size
            assert ci.to_ints(oracle.canon(0, bbg.poly_evaluate(a_np, kc2).reshape(1, 4)))[0] == ci.horner(ci.to_ints(a_np), ci.to_ints(kc2)[0])
    for log2_src, log2_target, cut in ((10, 12, 4), (12, 14, 4), (5, 7, 4), (11, 13, 0)):
        e = _coarse(0xC5C + log2_target, 1 << log2_target)
        want = oracle.divide_by_pseudo_vanishing(e, log2_src, cut)
        _check(oracle, bbg.divide_by_pseudo_vanishing(e, log2_src, cut), want, ("dpv host", log2_src, log2_target))
        d = _dev(e)
        bbg.divide_by_pseudo_vanishing_device(d.data_ptr(), log2_src, log2_target, cut)
        _check(oracle, _host(bbg, d, 1 << log2_target), want, ("dpv", log2_src, log2_target))


@pytest.mark.parametrize("log2n", [0, 1, 3, 5, 9, 12])
def test_permutation_grand_product_coarse(oracle, bbg, log2n):
    import torch
    n = 1 << log2n
    wires = np.stack([_coarse(0xC6A + k, n) for k in range(4)])
    sigmas = np.stack([_coarse(0xC6E + k, n) for k in range(4)])
    ch = _coarse(0xC70, 5)
    dw, ds = [_dev(wires[k]) for k in range(4)], [_dev(sigmas[k]) for k in range(4)]
    z = torch.zeros(n * 4, dtype=torch.int64, device="cuda")
    bbg.permutation_grand_product_device([t.data_ptr() for t in dw], [t.data_ptr() for t in ds], log2n, ch[0], ch[1], ch[2:5], z.data_ptr())
    _check(oracle, _host(bbg, z, n), oracle.permutation_z(wires, sigmas, ch[0], ch[1], ch[2:5]), ("grand product", log2n))


# ---------------------------------------------------------------------------------------------- MSM scalars
@pytest.fixture(scope="module")
def srs16c(bbg):
    s = bbg.srs_synth_hashed(0xBB254, 1 << 16)
    yield s
    s.free()


def _mont_scalars(ks):
    return ci.to_words([ci.to_mont(k, 0) for k in ks])


def _representatives(s):
    """s (canonical Montgomery words), s + r and s + 3r: every one below 2^256, the wider claim of recode_digits' comment."""
    return [s, ci.add_int(s, ci.R_MOD), ci.add_int(s, 3 * ci.R_MOD)]


def _jac_of_affine(pts):
    one = ci.to_words([ci.MONT_R % ci.Q_MOD])[0]
    j = np.zeros((pts.shape[0], 12), dtype=np.uint64)
    j[:, :8] = pts
    j[:, 8:] = one
    return j


def _affine(oracle, jac):
    ci.assert_coarse_jacobian(jac)
    return None if int(jac[3]) >> 63 else oracle.jac_to_affine(jac)


def _msm_options(bbg, window, quad, limbs29):
    bbg.set_option("msm_window", window)
    bbg.set_option("msm_accumulate_quad", quad)
    bbg.set_option("msm_limbs29", limbs29)


def _msm_reset(bbg):
    _msm_options(bbg, 0, 1, 1)


def test_msm_digit_patterns_mixed(oracle, bbg, srs16c):
    """Every window width with msm_window forced, through the three accumulation kernels: the digit patterns of that width (and of
    every other width) in one set, each as s, s + r and s + 3r, plus 2^256 - 1 -- against oracle.pippenger (a different recoding)."""
    ks = [k for c in MSM_WINDOWS for _, k, _ in ci.msm_digit_patterns(c)]
    s = _mont_scalars(ks)
    sc = np.concatenate(_representatives(s) + [ci.to_words([(1 << 256) - 1])])
    canon = oracle.canon(0, sc)
    pts = srs16c.read(0, sc.shape[0])
    want = oracle.pippenger(canon, pts)
    try:
        for window in MSM_WINDOWS:
            for quad, limbs29 in ACCUMULATORS:
                _msm_options(bbg, window, quad, limbs29)
                assert np.array_equal(_affine(oracle, bbg.msm(srs16c, sc)), want), (window, quad, limbs29)
    finally:
        _msm_reset(bbg)


def test_msm_digit_patterns_all_equal(oracle, bbg, srs16c):
    """n terms with one pattern's scalar k each: k * sum P_i (oracle).  Every pattern of the width in force, 512 terms, as s / s + r /
    s + 3r in turn; the widths' top-bucket, carry and chain patterns through all three accumulation kernels."""
    n = 512
    pts = srs16c.read(0, n)
    total = oracle.g1_sum(_jac_of_affine(pts))
    try:
        for window in MSM_WINDOWS:
            L = ci.MsmLayout(window)
            every_kernel = ("top_bucket_all", "neg_carry_all", f"ones_{L.offset(L.windows - 1)}")
            for idx, (name, k, _) in enumerate(ci.msm_digit_patterns(window)):
                s = _mont_scalars([k])
                want = oracle.pippenger(s, total.reshape(1, 8))
                rep = _representatives(s)[idx % 3]
                for quad, limbs29 in (ACCUMULATORS if name in every_kernel else ((1, 1),)):
                    _msm_options(bbg, window, quad, limbs29)
                    got = _affine(oracle, bbg.msm(srs16c, np.repeat(rep, n, axis=0)))
                    assert np.array_equal(got, want), (window, name, quad, limbs29)
    finally:
        _msm_reset(bbg)


def test_msm_every_term_in_the_top_bucket(oracle, bbg, srs16c):
    """All n terms in bucket 2^(C-1) of every window but the top one (the lone extra partition of the sort): n = 2^16 through the sort
    path at C = 13 / 16 / 17, n = 2^12 through the small path (C = 8), and a mixed batch at C = 8 and C = 13."""
    def case(window, n):
        pts = srs16c.read(0, n)
        total = oracle.g1_sum(_jac_of_affine(pts))
        k = dict((p[0], p[1]) for p in ci.msm_digit_patterns(window))["top_bucket_all"]
        s = _mont_scalars([k])
        return np.repeat(s, n, axis=0), oracle.pippenger(s, total.reshape(1, 8))
    try:
        for window, n in ((13, 1 << 16), (16, 1 << 16), (17, 1 << 16), (8, 1 << 12)):
            sc, want = case(window, n)
            for quad, limbs29 in (ACCUMULATORS if window == 8 else ((0, 1), (0, 0))):
                _msm_options(bbg, window, quad, limbs29)
                assert np.array_equal(_affine(oracle, bbg.msm(srs16c, sc)), want), (window, n, quad, limbs29)
        pts = srs16c.read(0, 3000)
        for window in (8, 13):
            top, want_top = case(window, 2048)
            pats = _mont_scalars([p[1] for p in ci.msm_digit_patterns(window)])
            mixed = np.concatenate([pats, ci.add_int(pats, ci.R_MOD)])
            sets = [(top, 0), (mixed, 100), (ci.coarse_scalars(0xC7A, 1000), 2000)]
            _msm_options(bbg, window, 1, 1)
            got = bbg.msm_batch(srs16c, [s for s, _ in sets], [f for _, f in sets])
            assert np.array_equal(_affine(oracle, got[0]), want_top), (window, "batch top")
            for j in (1, 2):
                sc, f = sets[j]
                want = oracle.pippenger(oracle.canon(0, sc), pts[f:f + sc.shape[0]])
                assert np.array_equal(_affine(oracle, got[j]), want), (window, "batch", j)
    finally:
        _msm_reset(bbg)


# ---------------------------------------------------------------------------------------------- coarse points
def _coarse_points(pts, seed):
    """(x + q, y + q) on a seeded third of the points (both stay below 2q)."""
    out = pts.copy()
    sel = np.random.default_rng(seed).random(pts.shape[0]) < 0.34
    sel[:2] = True
    out[sel, :4] = ci.add_int(pts[sel, :4], ci.Q_MOD)
    out[sel, 4:] = ci.add_int(pts[sel, 4:], ci.Q_MOD)
    return out, sel


def test_msm_over_coarse_point_tables(oracle, bbg, srs16c, tmp_path):
    """An SRS whose coordinates are (x + q, y + q) on a seeded subset, registered with stride 64, with stride 128 (the reference's
    interleaved point table) and from device memory: srs.read canon-equals the input below 2q, MSMs at every width equal the canonical
    SRS's, and the transcript writer emits the canonical SRS's bytes."""
    n = 3000
    pts = srs16c.read(0, n)
    cpts, sel = _coarse_points(pts, 0xC8A)
    assert sel.sum() > n // 4 and not ci.below(cpts[sel, :4], ci.Q_MOD).any()
    table = oracle.point_table(pts).reshape(n, 16)  # P_i || endo(P_i): the library reads the first half
    table[:, :8] = cpts
    table[sel, 8:12] = ci.add_int(table[sel, 8:12], ci.Q_MOD)
    table[sel, 12:16] = ci.add_int(table[sel, 12:16], ci.Q_MOD)
    dpts = _dev(cpts.reshape(-1, 4))
    srss = {"stride64": bbg.srs_register(cpts), "stride128": bbg.srs_register(table, stride_bytes=128),
            "device": bbg.srs_register_device(dpts.data_ptr(), n)}
    canon_srs = bbg.srs_register(pts)
    try:
        for name, s in srss.items():
            back = s.read()
            ci.assert_coarse(back.reshape(-1, 4), 1, name)
            assert np.array_equal(oracle.canon(1, back.reshape(-1, 4)), pts.reshape(-1, 4)), name
        pats = _mont_scalars([p[1] for p in ci.msm_digit_patterns(16)])
        sc = np.concatenate([ci.coarse_scalars(0xC8B, n - pats.shape[0]), pats])
        want = oracle.pippenger(oracle.canon(0, sc), pts[:sc.shape[0]])
        for window in MSM_WINDOWS:
            _msm_options(bbg, window, 1, 1)
            for name, s in srss.items():
                for m in (n, 1000):
                    w = want if m == n else oracle.pippenger(oracle.canon(0, sc[:m]), pts[:m])
                    assert np.array_equal(_affine(oracle, bbg.msm(s, sc[:m])), w), (name, window, m)
        _msm_reset(bbg)
        (tmp_path / "canon").mkdir()
        (tmp_path / "coarse").mkdir()
        canon_srs.write_transcript(tmp_path / "canon")
        srss["stride64"].write_transcript(tmp_path / "coarse")
        files = sorted(p.name for p in (tmp_path / "canon").iterdir())
        assert files and files == sorted(p.name for p in (tmp_path / "coarse").iterdir())
        for f in files:
            assert (tmp_path / "canon" / f).read_bytes() == (tmp_path / "coarse" / f).read_bytes(), f
    finally:
        _msm_reset(bbg)
        for s in list(srss.values()) + [canon_srs]:
            s.free()


def test_g1_sum_and_normalize_coarse_jacobians(oracle, bbg, srs16c):
    """bbg_g1_sum / bbg_g1_normalize on Jacobian inputs whose X, Y, Z are representatives in [q, 2q) where that fits, with points at
    infinity among them: the sum equals the oracle's, normalised outputs are canonical (below q)."""
    sc = ci.coarse_scalars(0xC9A, 600)
    parts = np.stack([bbg.msm(srs16c, sc[i * 100:(i + 1) * 100], start=i * 100) for i in range(6)])
    zero = bbg.msm(srs16c, np.zeros((10, 4), dtype=np.uint64))
    assert int(zero[3]) >> 63 == 1
    jac = np.concatenate([parts, zero.reshape(1, 12), parts[:2]])
    coarse = jac.copy()
    for i in range(coarse.shape[0]):
        if int(coarse[i, 3]) >> 63:
            continue
        for c in range(3):
            v = ci.to_ints(coarse[i, 4 * c:4 * c + 4])[0]
            if v < ci.Q_MOD and (i + c) % 2 == 0:
                coarse[i, 4 * c:4 * c + 4] = ci.to_words([v + ci.Q_MOD])[0]
    assert not ci.below(coarse[:, :4], ci.Q_MOD).all()
    want = oracle.g1_sum(jac)
    got = bbg.g1_sum(coarse)
    assert np.array_equal(_affine(oracle, got), want)
    norm = bbg.g1_normalize(coarse)
    for i in range(coarse.shape[0]):
        if int(jac[i, 3]) >> 63:
            assert int(norm[i, 3]) >> 63 == 1, i
            continue
        ci.assert_canonical(norm[i].reshape(2, 4), 1, ("normalize", i))
        assert np.array_equal(norm[i], oracle.jac_to_affine(jac[i])), i
