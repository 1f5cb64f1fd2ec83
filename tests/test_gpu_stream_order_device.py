"""Stream ordering of the G1, opening, cell and polynomial *_device entry points on a caller's own non-blocking stream: the second half of
tests/test_gpu_stream_order.py, under the discipline of that file's docstring (poison with 0x5A on the stream, queue, `snap = out.clone()`
on the stream, synchronise the stream once, compare the SNAPSHOT; two passes per section, the first one into scratch buffers; no bbg_sync,
no torch.cuda.synchronize, no host-pointer entry point and no synchronising option between the first queued call and that synchronisation;
no negative assertion).  That docstring also lists which case covers which entry point.

  A  one call, one snapshot                 (test_a_*)
  B  the call's device inputs are zeroed on the stream right behind it: the snapshot is the result of the ORIGINAL inputs (test_b_*,
     each beside the test_a_* of the same call)
  C  back-to-back calls that share context state: the pinned id array and the cells working memory, the MSM arena under
     msm_async_reduce = 1, the single fixed-base table slot, the lanes' GLV tables, a handle across a stream switch (test_c_*)

Expectations come from tests/tools/stream_order_cases.py: the C oracle and the integer models, bit for bit; the G1 cases run over the powers
string of a known x, where every expected point is one oracle.g1_mul.  The string is the library's (bbg_srs_synth_powers), read back once
in the fixture and held to the oracle's; no other output of the library serves as an expectation.  Handles, batch reservations, the string
and the 2^20 NTT tables are made in the fixture, before any section.

The first pass of a section leaves the context's working memory holding the very intermediates the checked pass computes.  Where a call
reads such an intermediate across streams -- bbg_cells_verify_reduce_device reads [A], the result of its inner MSM, which under
msm_async_reduce = 1 an auxiliary stream writes into the cells working memory -- a wait the library failed to queue would hand it the
RIGHT value, left over from the first pass.  So every section with a reduction runs, between its two passes, the same batch under another
challenge rho (reduction_under_another_challenge): E, [A], the products and the sums then differ from what the checked call must compute,
and a value read too early is a wrong one.

bbg_kate_opening_device and bbg_kate_opening_lagrange_device return a scalar to the host and so synchronise by themselves; their quotient
array is snapshotted on the stream all the same.  bbg_quotient_widget_device is called with alpha_base_out = NULL, the form that does not
synchronise, through ctypes; bbg_coset_fft_split_device has no binding method and is called through ctypes too."""
import ctypes

import numpy as np
import pytest

import open_all_model as oa
import stream_order_cases as sc
from stream_order import Env, affine, env, options, poisoned, to_device, unsynchronised, words  # noqa: F401 (env: a fixture)

pytestmark = pytest.mark.gpu

LG, LC = sc.LG, sc.LC
N, L, R_CELLS = 1 << LG, 1 << LC, 1 << (LG - LC)
RAGGED = sc.RAGGED


@pytest.fixture(scope="module")
def dev(env):
    """The powers string on the stream-order context, an all-points handle at 2^8 (batch reservation 3) and a cell handle at (10, 4)
    (reservation 2: five polynomials walk chunks of 2, 2, 1), the tables of the 2^20 transform."""
    d = Env()
    ctx = env.ctx
    d.string = ctx.srs_synth_powers(sc.x_mont(), sc.N_POINTS)
    d.pts = sc.string_points(env.oracle)
    assert np.array_equal(d.string.read(), d.pts), "bbg_srs_synth_powers differs from the oracle's string"
    d.h8 = ctx.open_all_prepare(d.string, 8)  # prepared while the context is on env.s
    d.h8.reserve_batch(3)
    d.hc = ctx.open_all_prepare(d.string, LG, LC)
    d.hc.reserve_batch(2)
    assert d.h8.count == 256 and d.hc.count == R_CELLS
    ctx.ntt_prepare(20)
    ctx.sync()
    yield d
    ctx.sync()
    d.h8.free()
    d.hc.free()
    d.string.free()


def up(env, a):
    """A device copy on the stream; the cases' arrays are read-only, so the host side of the upload is a writable copy."""
    return to_device(env, np.array(a, dtype=np.uint64))


def one_call(env, masters, out_bytes, call, consume=False, between=None):
    """One unsynchronised section around call(inputs, outs) -> the tensors to snapshot (None: outs).  consume: every input tensor is zeroed
    on the stream right behind the call, and the zeroed inputs are snapshotted too, to show that the overwrite happened."""
    def body(inputs, outs):
        watched = call(inputs, outs)
        watched = outs if watched is None else watched
        assert not consume or all(all(w is not i for i in inputs) for w in watched), "a consumed input cannot be the output"
        if consume:
            for t in inputs:
                t.zero_()
        return [w.clone() for w in watched] + ([t.clone() for t in inputs] if consume else [])

    got = unsynchronised(env, masters, out_bytes, body, between=between)
    if not consume:
        return got
    keep = len(got) - len(masters)
    for k, z in enumerate(got[keep:]):
        assert not z.any(), f"input {k} was not overwritten"
    return got[:keep]


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape}, expected {want.shape}"
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(want)} rows differ from the expectation, first at {bad[:8]}"


def canon(env, snap):
    return env.oracle.canon(0, words(snap, 4))


# ---- the calls, shared by A, B and C
def g1_ntt_call(env, inverse):
    return lambda inputs, outs: env.ctx.g1_ntt_device(inputs[0].data_ptr(), LG, outs[0].data_ptr(), inverse)


def open_call(handle):
    return lambda inputs, outs: handle.open_device(inputs[0].data_ptr(), outs[0].data_ptr())


def batch_call(handle, polys):
    return lambda inputs, outs: handle.open_batch_device(inputs[0].data_ptr(), polys, outs[0].data_ptr())


def recover_call(env, ids, count, k_in=0, k_out=0):
    return lambda inputs, outs: env.ctx.cells_recover_device(ids, inputs[k_in].data_ptr(), LG, LC, count, outs[k_out].data_ptr())


def verify_call(env, dev, case, k_in=0, k_out=0):
    """inputs[k_in .. k_in + 2]: commitments, values, proofs; outs[k_out], outs[k_out + 1]: L and R, the off-curve count."""
    com, cids, mids, _, _, rho, _ = case
    return lambda inputs, outs: env.ctx.cells_verify_reduce_device(dev.string, LG, LC, inputs[k_in].data_ptr(), com.shape[0], cids, mids,
                                                                   inputs[k_in + 1].data_ptr(), inputs[k_in + 2].data_ptr(), rho,
                                                                   outs[k_out].data_ptr(), outs[k_out + 1].data_ptr())


def verify_masters(env, case):
    com, _, _, values, proofs, _, _ = case
    return [up(env, com), up(env, values), up(env, proofs)]


def check_verify(snap_lr, snap_count, case, what):
    same(words(snap_lr, 8), case[6], f"{what}: L, R")
    assert int(np.ascontiguousarray(snap_count).view(np.uint32)[0]) == 0, f"{what}: the off-curve count"


def reduction_under_another_challenge(env, dev):
    """A between() for unsynchronised(): behind the first pass and its synchronisation, the batch of sc.verify_case under RHO_OTHER, run to
    its end (bbg_sync also waits for the auxiliary streams) and held to the model.  What it leaves in the context's working memory -- the
    folded values, [A], the products, S, Q -- is what no checked call may compute (tests/test_stream_order_cases_cpu.py: [A], L and R
    differ between the two challenges), see the module docstring."""
    other = sc.verify_case(env.oracle, rho=sc.RHO_OTHER)

    def between():
        masters, outs = verify_masters(env, other), [poisoned(env, 128), poisoned(env, 4)]
        verify_call(env, dev, other)(masters, outs)
        env.ctx.sync()
        env.torch.cuda.synchronize()
        check_verify(outs[0].cpu().numpy(), outs[1].cpu().numpy(), other, "the reduction under the other challenge, between the passes")
    return between


# A, B 1 ----------------------------------------------------------------------------------------------------- G1 transform
@pytest.mark.parametrize("ecntt_mul", [1, 0])
@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_a_g1_ntt(env, dev, inverse, ecntt_mul):
    with options(env, ecntt_mul=ecntt_mul):
        snap, = one_call(env, [up(env, dev.pts)], [N * 64], g1_ntt_call(env, inverse))
    same(words(snap, 8), sc.g1_ntt_want(env.oracle, inverse), f"g1_ntt 2^{LG}, inverse = {inverse}, ecntt_mul = {ecntt_mul}")


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_b_g1_ntt_consumes_its_points_in_stream_order(env, dev, inverse):
    snap, = one_call(env, [up(env, dev.pts)], [N * 64], g1_ntt_call(env, inverse), consume=True)
    same(words(snap, 8), sc.g1_ntt_want(env.oracle, inverse), f"g1_ntt 2^{LG}, inverse = {inverse}, points zeroed behind the call")


# A 2, A, B 3 ------------------------------------------------------------------------------------------------ one polynomial's proofs
def test_a_open_all_every_point(env, dev):
    coeffs, want = sc.open_case(env.oracle, 8, 0, [1])
    snap, = one_call(env, [up(env, coeffs)], [256 * 64], open_call(dev.h8))
    same(words(snap, 8), want, "open_all 2^8")


def open_all_cells(env, dev, consume):
    coeffs, want = sc.open_case(env.oracle, LG, LC, [2])
    snap, = one_call(env, [up(env, coeffs)], [R_CELLS * 64], open_call(dev.hc), consume=consume)
    same(words(snap, 8), want, f"open_all ({LG}, {LC}), coefficients zeroed behind the call = {consume}")


def test_a_open_all_cells(env, dev):
    open_all_cells(env, dev, False)


def test_b_open_all_cells_consumes_its_coefficients_in_stream_order(env, dev):
    open_all_cells(env, dev, True)


# A, B 4 ----------------------------------------------------------------------------------------------------- batched FK20
BATCH_SHAPES = ["10-4-five-in-chunks-of-two", "8-0-three-in-one-chunk"]


def open_all_batch(env, dev, shape, consume):
    lg, lc, handle, tags = (LG, LC, dev.hc, [3, 4, 5, 6, 7]) if shape.startswith("10") else (8, 0, dev.h8, [8, 9, 10])
    coeffs, want = sc.open_case(env.oracle, lg, lc, tags)
    snap, = one_call(env, [up(env, coeffs)], [want.shape[0] * 64], batch_call(handle, len(tags)), consume=consume)
    same(words(snap, 8), want, f"open_all_batch {shape}, coefficients zeroed behind the call = {consume}")


@pytest.mark.parametrize("shape", BATCH_SHAPES)
def test_a_open_all_batch(env, dev, shape):
    open_all_batch(env, dev, shape, False)


@pytest.mark.parametrize("shape", BATCH_SHAPES)
def test_b_open_all_batch_consumes_its_coefficients_in_stream_order(env, dev, shape):
    open_all_batch(env, dev, shape, True)


# A 5, A, B 6 ------------------------------------------------------------------------------------------------ cells as data
def test_a_cells_values(env, dev):
    coeffs, want = sc.values_case(env.oracle, 3)
    snap, = one_call(env, [up(env, coeffs)], [3 * N * 32],
                     lambda inputs, outs: env.ctx.cells_values_device(inputs[0].data_ptr(), LG, LC, 3, outs[0].data_ptr()))
    same(words(snap, 4), want, "cells_values, count 3")


def cells_recover(env, consume):
    ids, known, want = sc.recover_case(env.oracle, 0, 2)
    snap, = one_call(env, [up(env, known)], [2 * N * 32], recover_call(env, ids, 2), consume=consume)
    same(words(snap, 4), want, f"cells_recover, K = r / 2, count 2, values zeroed behind the call = {consume}")


def test_a_cells_recover(env, dev):
    cells_recover(env, False)


def test_b_cells_recover_consumes_its_values_in_stream_order(env, dev):
    cells_recover(env, True)


# A, B 7 ----------------------------------------------------------------------------------------------------- pairing-check reduction
def cells_verify_reduce(env, dev, async_reduce, consume):
    case = sc.verify_case(env.oracle)
    with options(env, msm_async_reduce=async_reduce):
        lr, count = one_call(env, verify_masters(env, case), [128, 4], verify_call(env, dev, case), consume=consume,
                             between=reduction_under_another_challenge(env, dev))
    check_verify(lr, count, case, f"cells_verify_reduce, msm_async_reduce = {async_reduce}, inputs zeroed behind the call = {consume}")


@pytest.mark.parametrize("async_reduce", [0, 1])
def test_a_cells_verify_reduce(env, dev, async_reduce):
    """The MSM inside runs under msm_async_reduce = 1 on an auxiliary stream and writes [A] into the context's working memory; the call
    joins it by itself.  Between the passes that memory is left with the [A] of another challenge."""
    cells_verify_reduce(env, dev, async_reduce, False)


@pytest.mark.parametrize("async_reduce", [0, 1])
def test_b_cells_verify_reduce_consumes_its_inputs_in_stream_order(env, dev, async_reduce):
    cells_verify_reduce(env, dev, async_reduce, True)


# A 8 -------------------------------------------------------------------------------------------------------- Fr helpers
def test_a_fr_batch_invert(env):
    a, want = sc.invert_case(env.pkg)
    snap, = one_call(env, [up(env, a)], [RAGGED * 32],
                     lambda inputs, outs: env.ctx.fr_batch_invert_device(inputs[0].data_ptr(), outs[0].data_ptr(), RAGGED))
    same(words(snap, 4), want, f"fr_batch_invert, n = {RAGGED}")


# A 9 -------------------------------------------------------------------------------------------------------- the two openings
def test_a_kate_opening(env):
    n = 1 << 12
    a, z = env.pkg.synthetic_scalars(sc.SEED + 400, n), env.pkg.synthetic_scalars(sc.SEED + 401, 1)[0]
    want_d, want_f = env.oracle.kate_opening(a, z)
    fs = []

    def call(inputs, outs):
        fs.append(env.ctx.kate_opening_device(inputs[0].data_ptr(), outs[0].data_ptr(), n, z))

    snap, = one_call(env, [up(env, a)], [n * 32], call)
    assert np.array_equal(fs[-1], want_f), "F(z)"
    same(canon(env, snap), want_d, "kate_opening 2^12: the quotient's coefficients")


def test_a_kate_opening_lagrange(env):
    lg = 12
    evals, z, want_d, want_f = sc.lagrange_opening_case(env.pkg, lg)
    fs = []

    def call(inputs, outs):
        fs.append(env.ctx.kate_opening_lagrange_device(inputs[0].data_ptr(), outs[0].data_ptr(), lg, z))

    snap, = one_call(env, [up(env, evals)], [32 << lg], call)
    assert np.array_equal(fs[-1], want_f), "F(z)"
    same(words(snap, 4), want_d, "kate_opening_lagrange 2^12: the quotient's values")


# A 10 ------------------------------------------------------------------------------------------------------- linear combination
@pytest.mark.parametrize("limbs29", [1, 0])
def test_a_poly_linear_combination(env, limbs29):
    oracle, n, terms = env.oracle, RAGGED, 5
    polys = [env.pkg.synthetic_scalars(sc.SEED + 500 + k, n) for k in range(terms)]
    scal, base = env.pkg.synthetic_scalars(sc.SEED + 510, terms), env.pkg.synthetic_scalars(sc.SEED + 511, n)
    want = oracle.canon(0, base)
    for k in range(terms):
        want = oracle.fe_add(0, want, oracle.fe_mul(0, polys[k], np.tile(scal[k], (n, 1))))

    def call(inputs, outs):
        env.ctx.poly_linear_combination_device([t.data_ptr() for t in inputs[:terms]], scal, inputs[terms].data_ptr(), outs[0].data_ptr(), n)

    with options(env, poly_limbs29=limbs29):
        snap, = one_call(env, [up(env, p) for p in polys + [base]], [n * 32], call)
    same(canon(env, snap), oracle.canon(0, want), f"poly_linear_combination, 5 terms and a base, n = {n}, poly_limbs29 = {limbs29}")


# A 11 ------------------------------------------------------------------------------------------------------- grand product
def test_a_permutation_grand_product(env):
    lg = 10
    n = 1 << lg
    wires = np.stack([env.pkg.synthetic_scalars(sc.SEED + 600 + k, n) for k in range(4)])
    sigmas = np.stack([env.pkg.synthetic_scalars(sc.SEED + 610 + k, n) for k in range(4)])
    ch = env.pkg.synthetic_scalars(sc.SEED + 620, 5)

    def call(inputs, outs):
        env.ctx.permutation_grand_product_device([t.data_ptr() for t in inputs[:4]], [t.data_ptr() for t in inputs[4:]], lg, ch[0], ch[1], ch[2:5],
                                                 outs[0].data_ptr())

    snap, = one_call(env, [up(env, a) for a in list(wires) + list(sigmas)], [n * 32], call)
    same(canon(env, snap), env.oracle.permutation_z(wires, sigmas, ch[0], ch[1], ch[2:5]), "permutation_grand_product 2^10")


# A 12 ------------------------------------------------------------------------------------------------------- one quotient widget
def test_a_quotient_widget(env):
    """The permutation widget (it ASSIGNS the quotient, so the poison is gone from every row) over a 2^12 domain, inputs as
    tests/test_gpu_parity.py::test_quotient_widgets_vs_oracle makes them; alpha_base_out = NULL: with it the call would synchronise."""
    lg = 12
    m = 1 << lg
    polys = [env.pkg.synthetic_scalars(5000 + 31 * lg + k, m) for k in range(23)]
    ch9 = env.pkg.synthetic_scalars(6000 + lg, 9)
    want = np.zeros((m, 4), dtype=np.uint64)
    env.oracle.quotient_widget(0, polys, lg, ch9, want)
    rcs = []

    def call(inputs, outs):
        arr = (ctypes.c_void_p * 23)(*[ctypes.c_void_p(t.data_ptr()) for t in inputs])
        rcs.append(env.ctx.lib.bbg_quotient_widget_device(env.ctx.ctx, 0, arr, lg, ch9.ctypes.data, ctypes.c_void_p(outs[0].data_ptr()), None))

    snap, = one_call(env, [up(env, p) for p in polys], [m * 32], call)
    assert rcs == [0, 0]
    same(canon(env, snap), env.oracle.canon(0, want), "quotient_widget: permutation, 2^12")


# A 13 - 16 -------------------------------------------------------------------------------------------------- in place on one array
def test_a_divide_by_pseudo_vanishing(env):
    e = env.pkg.synthetic_scalars(sc.SEED + 700, 1 << 12)

    def call(inputs, outs):
        env.ctx.divide_by_pseudo_vanishing_device(inputs[0].data_ptr(), 10, 12, 4)
        return [inputs[0]]

    snap, = one_call(env, [up(env, e)], [], call)
    same(canon(env, snap), env.oracle.canon(0, env.oracle.divide_by_pseudo_vanishing(e, 10, 4)), "divide_by_pseudo_vanishing 2^10 -> 2^12")


def test_a_cross_dft(env):
    a, want = sc.cross_dft_case(env.pkg, 1, 1 << 9, 10)
    snap, = one_call(env, [up(env, a)], [a.shape[0] * 32],
                     lambda inputs, outs: env.ctx.cross_dft_device(inputs[0].data_ptr(), outs[0].data_ptr(), 1, 1 << 9, 10))
    same(canon(env, snap), want, "cross_dft, G = 2, len = 2^9, n = 2^10")


def test_a_scale_powers(env):
    a, start, base, want = sc.scale_powers_case(env.pkg)

    def call(inputs, outs):
        env.ctx.scale_powers_device(inputs[0].data_ptr(), RAGGED, base, start)
        return [inputs[0]]

    snap, = one_call(env, [up(env, a)], [], call)
    same(canon(env, snap), want, f"scale_powers, n = {RAGGED}")


def test_a_coset_fft_split(env):
    """No binding method: bbg.lib through ctypes.  The buffer holds ext x n elements, the coefficients in the first n."""
    lg, ext = 10, 4
    c = env.oracle.canon(0, env.pkg.synthetic_scalars(1200 + lg, 1 << lg))
    buf = np.zeros((ext << lg, 4), dtype=np.uint64)
    buf[:1 << lg] = c
    rcs = []

    def call(inputs, outs):
        rcs.append(env.ctx.lib.bbg_coset_fft_split_device(env.ctx.ctx, ctypes.c_void_p(inputs[0].data_ptr()), lg, ext))
        return [inputs[0]]

    snap, = one_call(env, [up(env, buf)], [], call)
    assert rcs == [0, 0]
    same(canon(env, snap), env.oracle.canon(0, env.oracle.coset_fft_split(c, ext)), "coset_fft_split 2^10, ext 4")


# C 1 -------------------------------------------------------------------------------------------------------- the pinned array
FILLER_LOG2, FILLER_RUNS = 20, 4


def test_c_pinned_id_array_is_not_reused_before_its_copy(env, dev):
    """Four 2^20 transforms keep the stream busy; behind them, with nothing in between, two recoveries over different id sets of the same K
    and one reduction: three calls, two entry points, ONE pinned host array that each fills with its lists and uploads asynchronously
    (cells_pinned_ensure in csrc/cells.hip), and one working memory on the device.  The host may block inside the second and third call:
    that is the guard.  All three results must be those of their own lists."""
    oracle = env.oracle
    x, y, v = sc.recover_case(oracle, 0, 2), sc.recover_case(oracle, 1, 2), sc.verify_case(oracle)
    assert x[0] != y[0] and len(x[0]) == len(y[0])
    filler = env.pkg.synthetic_scalars(sc.SEED + 800, 1 << FILLER_LOG2)
    recover_x, recover_y, verify = recover_call(env, x[0], 2, 1, 0), recover_call(env, y[0], 2, 2, 1), verify_call(env, dev, v, 3, 2)

    def body(inputs, outs):
        for _ in range(FILLER_RUNS):
            env.ctx.ntt_device(inputs[0].data_ptr(), FILLER_LOG2, env.pkg.binding.FFT)
        recover_x(inputs, outs)
        recover_y(inputs, outs)
        verify(inputs, outs)
        return [o.clone() for o in outs]

    masters = [up(env, filler), up(env, x[1]), up(env, y[1])] + verify_masters(env, v)
    got_x, got_y, lr, count = unsynchronised(env, masters, [2 * N * 32, 2 * N * 32, 128, 4], body, between=reduction_under_another_challenge(env, dev))
    same(words(got_x, 4), x[2], "the first recovery (id set X)")
    same(words(got_y, 4), y[2], "the second recovery (id set Y)")
    check_verify(lr, count, v, "the reduction behind the two recoveries")


# C 2 -------------------------------------------------------------------------------------------------------- the MSM arena
def test_c_reduction_shares_the_arena_with_an_msm_in_flight(env, dev):
    """msm_async_reduce = 1: a 2^16 MSM at window 20 (2^19 buckets reducing on an auxiliary stream, no join), then the reduction, whose own
    MSM takes the other slot of the same arena, then join().  Between the passes the working memory is left with another challenge's [A]."""
    n = 1 << 16
    k = env.pkg.synthetic_scalars(sc.SEED + 900, n)
    want = env.oracle.pippenger(k, env.pts[:n])
    v = sc.verify_case(env.oracle)
    verify = verify_call(env, dev, v, 1, 1)

    def body(inputs, outs):
        env.ctx.msm_device(env.srs, inputs[0].data_ptr(), n, outs[0].data_ptr())
        verify(inputs, outs)
        env.ctx.join()
        return [o.clone() for o in outs]

    with options(env, msm_async_reduce=1, msm_window=20):
        msm, lr, count = unsynchronised(env, [up(env, k)] + verify_masters(env, v), [96, 128, 4], body,
                                        between=reduction_under_another_challenge(env, dev))
    assert np.array_equal(affine(env, msm)[0], want), "the MSM in flight"
    check_verify(lr, count, v, "the reduction behind an MSM in flight")


# C 3 -------------------------------------------------------------------------------------------------------- the fixed-base table slot
def test_c_fixed_base_table_is_rebuilt_in_stream_order(env):
    """Generator, another base, generator again: each change of base rebuilds the ONE table slot in place (csrc/fixed_base.hip) while the
    products of the call before may still be reading it."""
    n, oracle = 300, env.oracle
    ks = [env.pkg.synthetic_scalars(sc.SEED + 1000 + j, n) for j in range(3)]
    other = env.pts[7]
    bases = [None, other, None]

    def body(inputs, outs):
        for d_k, base, out in zip(inputs, bases, outs):
            env.ctx.g1_fixed_base_mul_device(d_k.data_ptr(), n, out.data_ptr(), base)
        return [o.clone() for o in outs]

    snaps = unsynchronised(env, [up(env, k) for k in ks], [64 * n] * 3, body)
    for j, (snap, k, base) in enumerate(zip(snaps, ks, bases)):
        b = oracle.g1_generator() if base is None else base
        want = oa.canon_points(oracle, np.stack([oracle.g1_mul(b, w) for w in k]))
        same(words(snap, 8), want, f"call {j}: {'the generator' if base is None else 'the second base'}")


# C 4 -------------------------------------------------------------------------------------------------------- the lanes' GLV tables
def test_c_g1_kernels_share_their_tables_in_stream_order(env, dev):
    """Variable-base products, a G1 transform and a cell opening back to back: all three build per-lane multiples in the context's one
    table buffer."""
    n, oracle = 300, env.oracle
    k = env.pkg.synthetic_scalars(sc.SEED + 1100, n)
    p = env.pts[1000:1000 + n]
    coeffs, want_open = sc.open_case(oracle, LG, LC, [2])

    def body(inputs, outs):
        env.ctx.g1_batch_mul_device(inputs[0].data_ptr(), inputs[1].data_ptr(), n, outs[0].data_ptr())
        env.ctx.g1_ntt_device(inputs[2].data_ptr(), LG, outs[1].data_ptr(), False)
        dev.hc.open_device(inputs[3].data_ptr(), outs[2].data_ptr())
        return [o.clone() for o in outs]

    masters = [up(env, p), up(env, k), up(env, dev.pts), up(env, coeffs)]
    mul, ntt, opened = unsynchronised(env, masters, [64 * n, 64 * N, 64 * R_CELLS], body)
    same(words(mul, 8), oa.canon_points(oracle, np.stack([oracle.g1_mul(pt, w) for pt, w in zip(p, k)])), "g1_batch_mul")
    same(words(ntt, 8), sc.g1_ntt_want(oracle, False), "g1_ntt behind g1_batch_mul")
    same(words(opened, 8), want_open, "open_all behind g1_ntt")


# C 5 -------------------------------------------------------------------------------------------------------- a handle across a stream switch
def test_c_handle_follows_a_stream_switch(env, dev):
    """The handle was prepared while the context was on `s`; after bbg_set_stream(s2) its call must run on s2."""
    torch, ctx = env.torch, env.ctx
    s2 = torch.cuda.Stream()
    coeffs, want = sc.open_case(env.oracle, 8, 0, [1])

    def body(inputs, outs):
        ctx.set_stream(s2.cuda_stream)
        dev.h8.open_device(inputs[0].data_ptr(), outs[0].data_ptr())
        # inputs and outs belong to `s` for torch's caching allocator and no record_stream tells it about s2: using them on s2 is safe only
        # because the tensors outlive s2.synchronize() (unsynchronised() keeps them until its snapshots are on the host) -- keep that order
        with torch.cuda.stream(s2):
            return [outs[0].clone()]

    def back_to_the_first_stream():  # behind the first pass and its synchronisation: the checked pass starts on `s` again
        ctx.set_stream(env.s.cuda_stream)

    try:
        snap, = unsynchronised(env, [up(env, coeffs)], [256 * 64], body, between=back_to_the_first_stream, final_stream=s2)
    finally:
        ctx.set_stream(env.s.cuda_stream)
    same(words(snap, 8), want, "open_all 2^8 behind a stream switch")
