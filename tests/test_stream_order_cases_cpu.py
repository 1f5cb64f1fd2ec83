"""The expectations of tests/test_gpu_stream_order_device.py (tests/tools/stream_order_cases.py) held to a second route on the CPU, at the
shapes the GPU cases use: closed forms over the powers string against the models' definition routes on the oracle, the integer
restatements against the oracle's field operations."""
import numpy as np

import cells_model as cm
import cells_verify_model as vm
import coarse_inputs as ci
import lagrange_model as lm
import open_all_model as oa
import open_cells_model as oc
import stream_order_cases as sc

R = sc.R
LG, LC = sc.LG, sc.LC


def test_the_string_is_the_powers_of_x(oracle):
    pts = sc.string_points(oracle)
    assert pts.shape == (1 << LG, 8)
    assert np.array_equal(pts[[0, 1, 1023]], vm.scalar_times_generator(oracle, [1, sc.X_INT, pow(sc.X_INT, 1023, R)]))


def test_g1_transform_by_its_definition_at_a_few_outputs(oracle):
    n, pts = 1 << LG, sc.string_points(oracle)
    w = lm.root(oracle, LG)
    assert w == ci.root_of_unity(LG)
    for inverse in (False, True):
        want = sc.g1_ntt_want(oracle, inverse)
        assert want.shape == (n, 8)
        base, scale = (pow(w, R - 2, R), pow(n, R - 2, R)) if inverse else (w, 1)
        for k in (0, 1, 517, n - 1):
            row = lm.ints_to_mont(oracle, [scale * pow(base, (j * k) % n, R) for j in range(n)])
            assert np.array_equal(oa.canon_points(oracle, oracle.msm_naive(row, pts))[0], want[k]), (inverse, k)


def test_proofs_by_their_definition_at_a_few_indices(oracle):
    pts = sc.string_points(oracle)
    _, want = sc.open_case(oracle, 8, 0, [1])
    ms = [0, 5, 255]
    assert np.array_equal(oa.open_all_definition(oracle, pts, list(sc.poly(1, 256)), ms), want[ms])
    coeffs, want = sc.open_case(oracle, LG, LC, [3, 4, 5, 6, 7])
    assert coeffs.shape == (5 << LG, 4) and want.shape == (5 * 64, 8)
    ms = [0, 17, 63]
    for p, tag in ((0, 3), (4, 7)):
        assert np.array_equal(oc.open_cells_definition(oracle, pts, list(sc.poly(tag, 1 << LG)), LC, ms), want[[64 * p + m for m in ms]]), tag
    assert len({want[64 * p].tobytes() for p in range(5)}) == 5, "five different polynomials"


def test_cell_values_and_recovery(oracle):
    n, l, r = cm.shape(LG, LC)
    coeffs, values = sc.values_case(oracle, 3)
    w = ci.root_of_unity(LG)
    for p, m, t in ((0, 0, 0), (1, 63, 15), (2, 20, 7)):
        f = sc.poly(100 + p, n)
        assert np.array_equal(values[p * n + m * l + t], cm.mont([oc.horner(f, pow(w, m + r * t, R))])[0]), (p, m, t)
    x, y = sc.recover_case(oracle, 0, 2), sc.recover_case(oracle, 1, 2)
    assert len(x[0]) == len(y[0]) == r // 2 and set(x[0]) != set(y[0]) and x[0] != sorted(x[0])
    for ids, known, want in (x, y):
        K = len(ids)
        for p in range(2):
            route = cm.recover_route(oracle, ids, cm.unmont(known[p * K * l:(p + 1) * K * l]), LG, LC)
            assert np.array_equal(cm.mont(route), want[p * n:(p + 1) * n]), p
            assert want[p * n + K * l - 1].any() and not want[p * n + K * l:(p + 1) * n].any()


def test_the_reduction_holds_and_agrees_with_its_definition(oracle):
    com, cids, mids, values, proofs, rho, want = sc.verify_case(oracle)
    assert com.shape == (2, 8) and len(mids) == 16 and set(cids) == {0, 1}
    assert not oa.is_infinity(want[0]) and not oa.is_infinity(want[1])
    assert vm.holds(oracle, want[0], want[1], sc.X_INT, LC), "[x^l] L = R for the honest batch"
    L, R_ = vm.reduce_definition(oracle, sc.string_points(oracle), LG, LC, com, cids, mids, cm.unmont(values), proofs, sc.RHO)
    assert np.array_equal(np.stack([L, R_]), want)
    # the batch under the other challenge, which the GPU cases run in front of every checked reduction: it holds too, and what it leaves
    # behind -- [A], the result of the MSM inside the call, and L and R -- differs from what the checked call must compute
    other = sc.verify_case(oracle, rho=sc.RHO_OTHER)
    assert all(np.array_equal(a, b) for a, b in zip(other[:5], (com, cids, mids, values, proofs))) and not np.array_equal(other[5], rho)
    assert vm.holds(oracle, other[6][0], other[6][1], sc.X_INT, LC)
    assert not np.array_equal(other[6][0], want[0]) and not np.array_equal(other[6][1], want[1])
    a_checked, a_other = sc.interpolant_commitment(oracle, sc.RHO), sc.interpolant_commitment(oracle, sc.RHO_OTHER)
    assert not oa.is_infinity(a_checked) and not oa.is_infinity(a_other) and not np.array_equal(a_checked, a_other)


def test_fr_restatements_against_the_oracles_field_operations(pkg, oracle):
    one = oracle.to_mont(0, np.array([[1, 0, 0, 0]], dtype=np.uint64))[0]
    a, inv = sc.invert_case(pkg)
    zero = ~a.any(axis=1)
    assert zero.sum() == 4 and not inv[zero].any()
    prod = oracle.canon(0, oracle.fe_mul(0, a, inv))
    assert (prod[~zero] == one).all()
    a, start, base, want = sc.scale_powers_case(pkg)
    f, rows = start.copy(), {}
    for j in range(2050):  # the running factor by the oracle's own products
        rows[j] = oracle.fe_mul(0, a[j], f)[0]
        f = oracle.fe_mul(0, f, base)[0]
    for j in (0, 1, 255, 256, 2049):
        assert np.array_equal(oracle.canon(0, rows[j].reshape(1, 4))[0], want[j]), j
    b_int, s_int = (ci.from_mont(v, 0) for v in ci.to_ints(np.stack([base, start])))
    last = sc.RAGGED - 1
    fl = cm.mont([s_int * pow(b_int, last, R)])[0]
    assert np.array_equal(oracle.canon(0, oracle.fe_mul(0, a[last], fl))[0], want[last])
    a, want = sc.cross_dft_case(pkg, 1, 1 << 9, 10)
    lo, hi = a[:512], a[512:]
    assert np.array_equal(oracle.canon(0, oracle.fe_add(0, lo, hi)), want[:512]) and np.array_equal(oracle.canon(0, oracle.fe_sub(0, lo, hi)), want[512:])


def test_lagrange_opening_is_the_coefficient_opening_transformed(pkg, oracle):
    evals, z, dest, fz = sc.lagrange_opening_case(pkg, 12)
    coeffs = oracle.ntt(evals, 1)
    want_d, want_f = oracle.kate_opening(coeffs, z)
    assert np.array_equal(fz, want_f)
    assert np.array_equal(oracle.canon(0, oracle.ntt(dest, 1)), oracle.canon(0, want_d))
