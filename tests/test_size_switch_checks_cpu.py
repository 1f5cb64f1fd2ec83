"""CPU tests of tests/tools/size_switch_checks.py, the O(n) grand-product check the size-switch GPU tests (tests/test_gpu_size_switches.py)
rely on above 2^18 rows: it agrees with the oracle's serial restatement, rejects a z that is wrong in any of the ways a broken scan would
make it, and its closing inputs really close."""
import numpy as np
import pytest

import coarse_inputs as ci
import size_switch_checks as sc

LOG2N = 10


@pytest.fixture(scope="module")
def case(oracle):
    rng = np.random.default_rng(0x5C)
    n = 1 << LOG2N
    wires = np.stack([sc.random_scalars(rng, n) for _ in range(4)])
    sigmas = np.stack([sc.random_scalars(rng, n) for _ in range(4)])
    ch = sc.random_scalars(rng, 5)
    return wires, sigmas, ch


def test_powers_match_big_integers(oracle):
    x = sc.random_scalars(np.random.default_rng(1), 1)[0]
    got = ci.to_ints(sc.powers(oracle, x, 37))
    xs = ci.to_ints(x)[0]
    acc = ci.to_mont(1, 0)
    for j in range(37):
        assert got[j] == acc, j
        acc = ci.mont_mul(acc, xs, 0)
    w = ci.to_ints(sc.omega_powers(oracle, 5))
    wr = ci.root_of_unity(5)
    assert [ci.from_mont(v, 0) for v in w] == [pow(wr, j, ci.R_MOD) for j in range(32)]


@pytest.mark.parametrize("width", [4, 3])
def test_check_agrees_with_the_oracle(oracle, case, width):
    wires, sigmas, ch = case
    sigmas = sigmas.copy()
    if width == 3:  # the oracle is width 4 only: sigma_4 = K_3 w^j makes the fourth column's factors cancel
        sigmas[3] = sc.identity_tags(oracle, LOG2N, ch[2:5], 4)[3]
    z = oracle.permutation_z(wires, sigmas, ch[0], ch[1], ch[2:5])
    N, D = sc.row_terms(oracle, wires, sigmas, ch[0], ch[1], ch[2:5], width)
    sc.check_grand_product(oracle, z, N, D)
    # and coarse representatives of the inputs and of z give the same terms and pass the same check
    N2, D2 = sc.row_terms(oracle, sc.plus_p(wires), sc.plus_p(sigmas), ch[0], ch[1], ch[2:5], width)
    assert np.array_equal(N2, N) and np.array_equal(D2, D)
    sc.check_grand_product(oracle, sc.plus_p(z), N, D)
    # the other width's terms are different ones: a width mix-up cannot pass
    No, Do = sc.row_terms(oracle, wires, sigmas, ch[0], ch[1], ch[2:5], 7 - width)
    if width == 4:
        with pytest.raises(AssertionError):
            sc.check_grand_product(oracle, z, No, Do)
    else:  # the fourth column cancels row by row, in N / D, not in N and D apiece
        assert not np.array_equal(No, N) and not np.array_equal(Do, D)


def _mutants(oracle, z):
    n = z.shape[0]
    one_row = z.copy()
    one_row[n // 2] = oracle.fe_add(0, one_row[n // 2:n // 2 + 1], sc.mont_one(oracle).reshape(1, 4))[0]
    last_changed = z.copy()
    last_changed[n - 1] = z[n - 2]
    swapped = z.copy()
    swapped[[300, 301]] = z[[301, 300]]
    scaled = oracle.fe_mul(0, z, sc._bcast(oracle.to_mont(0, np.array([[3, 0, 0, 0]], dtype=np.uint64)), n))
    return {
        "one row": one_row,
        "last row changed to its neighbour": last_changed,
        "shifted down (z[0] kept)": np.concatenate([z[:1], z[:-1]]),
        "shifted up": np.concatenate([z[1:], z[-1:]]),
        "rolled": np.roll(z, 1, axis=0),
        "scaled by 3": scaled,
        "two adjacent rows swapped": swapped,
        "last row dropped": z[:-1],
        "last row duplicated": np.concatenate([z, z[-1:]]),
    }


def test_check_rejects_wrong_grand_products(oracle, case):
    wires, sigmas, ch = case
    z = oracle.permutation_z(wires, sigmas, ch[0], ch[1], ch[2:5])
    N, D = sc.row_terms(oracle, wires, sigmas, ch[0], ch[1], ch[2:5], 4)
    sc.check_grand_product(oracle, z, N, D)
    for name, bad in _mutants(oracle, z).items():
        with pytest.raises(AssertionError):
            sc.check_grand_product(oracle, bad, N, D, what=name)
    # a z of the wrong challenges, and a z that does not close where the input does
    z_other = oracle.permutation_z(wires, sigmas, ch[1], ch[0], ch[2:5])
    with pytest.raises(AssertionError):
        sc.check_grand_product(oracle, z_other, N, D)
    with pytest.raises(AssertionError):
        sc.check_grand_product(oracle, z, N, D, closing=True)


@pytest.mark.parametrize("width", [4, 3])
def test_closing_inputs_close(oracle, width):
    ks = sc.random_scalars(np.random.default_rng(7), 3)
    beta, gamma = sc.random_scalars(np.random.default_rng(8), 2)
    wires, sigmas = sc.closing_inputs(oracle, LOG2N, ks, width, seed=9)
    n = 1 << LOG2N
    assert wires.shape == sigmas.shape == (width, n, 4)
    ids = sc.identity_tags(oracle, LOG2N, ks, width).reshape(-1, 4)
    flat = sigmas.reshape(-1, 4)
    # sigma is a permutation of the identity tags, not the identity, and the wires agree along it
    key = lambda a: np.lexsort(a.T[::-1])  # noqa: E731
    assert np.array_equal(flat[key(flat)], ids[key(ids)])
    moved = (flat != ids).any(axis=1)
    assert moved.sum() > n
    tag_pos = {tuple(t): i for i, t in enumerate(ids.tolist())}
    w = wires.reshape(-1, 4)
    dest = np.array([tag_pos[tuple(t)] for t in flat.tolist()])
    assert np.array_equal(w, w[dest])
    N, D = sc.row_terms(oracle, wires, sigmas, beta, gamma, ks, width)
    prod_n, prod_d = ci.to_mont(1, 0), ci.to_mont(1, 0)
    for a, b in zip(ci.to_ints(N), ci.to_ints(D)):
        prod_n, prod_d = ci.mont_mul(prod_n, a, 0), ci.mont_mul(prod_d, b, 0)
    assert prod_n == prod_d
    if width == 4:  # the oracle's z closes: z[n-1] N_{n-1} = D_{n-1}
        z = oracle.permutation_z(wires, sigmas, beta, gamma, ks)
        sc.check_grand_product(oracle, z, N, D, closing=True)
        # and a random sigma does not
        rs = sc.random_scalars(np.random.default_rng(10), 4 * n).reshape(4, n, 4)
        N2, D2 = sc.row_terms(oracle, wires, rs, beta, gamma, ks, 4)
        with pytest.raises(AssertionError):
            sc.check_grand_product(oracle, oracle.permutation_z(wires, rs, beta, gamma, ks), N2, D2, closing=True)
