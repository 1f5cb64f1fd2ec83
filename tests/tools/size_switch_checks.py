"""An O(n) check of the permutation grand product and inputs for it at the sizes where the kernels change shape (test tooling).

oracle.permutation_z restates the grand product row by row with one inversion per row: fine up to 2^18 rows, too slow above.  The
check here needs no inversion.  With N_j = prod_k (w_k[j] + gamma + beta K_k w^j) and D_j = prod_k (w_k[j] + gamma + beta sigma_k[j])
(K_0 = 1, K_1..3 = ks, w the 2^log2n-th root of unity), z is the grand product exactly when

    z[0] = 1   and   z[j+1] D_j = z[j] N_j  for every j < n - 1,

as long as no D_j is zero (probability ~n 2^-250 for random inputs).  Every product comes from the oracle's vectorised field ops.  A
*closing* input (a real copy permutation: sigma permutes the identity tags K_k w^j and the wires are constant on its cycles) has
prod_j N_j / D_j = 1 over all n rows, so there also z[n-1] N_{n-1} = D_{n-1}.  tests/test_gpu_size_switches.py runs the check on
the device's z; tests/test_size_switch_checks_cpu.py checks the check.
"""
import numpy as np

import coarse_inputs as ci


def mont_one(oracle):
    return oracle.to_mont(0, np.array([[1, 0, 0, 0]], dtype=np.uint64))[0]


def _bcast(v, n):
    return np.ascontiguousarray(np.broadcast_to(np.reshape(v, (1, 4)), (n, 4)))


def powers(oracle, x, n):
    """x^0 .. x^(n-1) (Montgomery) by doubling: each step multiplies the powers so far by x^len."""
    out = mont_one(oracle).reshape(1, 4).copy()
    x = np.reshape(x, (1, 4))
    while out.shape[0] < n:
        step = oracle.fe_mul(0, out[-1:], x)  # x^len
        k = min(out.shape[0], n - out.shape[0])
        out = np.concatenate([out, oracle.fe_mul(0, out[:k], _bcast(step, k))])
    return out


def omega_powers(oracle, log2n):
    return powers(oracle, oracle.root_of_unity(log2n), 1 << log2n)


def identity_tags(oracle, log2n, ks, width):
    """(width, n, 4): K_k w^j, the values sigma_k[j] takes where position (k, j) is copied to itself."""
    wj = omega_powers(oracle, log2n)
    n = wj.shape[0]
    K = [mont_one(oracle)] + [np.reshape(ks, (3, 4))[k] for k in range(3)]
    tags = np.stack([wj if k == 0 else oracle.fe_mul(0, wj, _bcast(K[k], n)) for k in range(width)])
    return oracle.canon(0, tags.reshape(-1, 4)).reshape(width, n, 4)


def row_terms(oracle, wires, sigmas, beta, gamma, ks, width):
    """(N, D), each (n, 4) canonical Montgomery: the numerator and denominator of every row over the first `width` columns.  Inputs
    may be any representatives in [0, 2p)."""
    n = np.shape(wires)[1]
    log2n = n.bit_length() - 1
    assert n == 1 << log2n
    g, b = _bcast(gamma, n), _bcast(beta, n)
    ids = identity_tags(oracle, log2n, ks, width)
    N = D = None
    for k in range(width):
        wpg = oracle.fe_add(0, oracle.canon(0, wires[k]), g)
        nk = oracle.fe_add(0, wpg, oracle.fe_mul(0, ids[k], b))
        dk = oracle.fe_add(0, wpg, oracle.fe_mul(0, oracle.canon(0, sigmas[k]), b))
        N = nk if N is None else oracle.fe_mul(0, N, nk)
        D = dk if D is None else oracle.fe_mul(0, D, dk)
    return oracle.canon(0, N), oracle.canon(0, D)


def check_grand_product(oracle, z, N, D, closing=False, what=""):
    """Raises AssertionError unless z (any representatives below 2^256 that canonicalise) is the grand product of N / D."""
    n = N.shape[0]
    z = np.ascontiguousarray(z, dtype=np.uint64).reshape(-1, 4)
    assert z.shape[0] == n, f"{what}: z has {z.shape[0]} rows, expected {n}"
    assert not (D == 0).all(axis=1).any(), f"{what}: a zero denominator: the recurrence does not fix z"
    zc = oracle.canon(0, z)
    assert np.array_equal(zc[0], mont_one(oracle)), f"{what}: z[0] != 1"
    lhs = oracle.canon(0, oracle.fe_mul(0, zc[1:], D[:-1]))
    rhs = oracle.canon(0, oracle.fe_mul(0, zc[:-1], N[:-1]))
    bad = np.flatnonzero((lhs != rhs).any(axis=1))
    assert bad.size == 0, f"{what}: z[j+1] D_j != z[j] N_j at {bad.size} row(s), first j = {int(bad[0]) if bad.size else -1}"
    if closing:
        last = oracle.canon(0, oracle.fe_mul(0, zc[-1:], N[-1:]))
        assert np.array_equal(last, D[-1:]), f"{what}: z[n-1] N_(n-1) != D_(n-1): the permutation does not close"


def random_scalars(rng, n):
    """n random values below 2^252 (< r), read as Montgomery residues."""
    a = rng.integers(0, np.iinfo(np.uint64).max, size=(n, 4), dtype=np.uint64, endpoint=True)
    a[:, 3] &= np.uint64((1 << 60) - 1)
    return a


def closing_inputs(oracle, log2n, ks, width, seed):
    """(wires, sigmas), each (width, n, 4): a random copy permutation of the width * n positions (every position joins one of ~n random
    groups; a group's positions form one cycle) and wires that take one random value per group.  sigma_k[j] is the identity tag of the
    position (k, j) is copied to, so the multisets {w + beta id} and {w + beta sigma} agree and prod_j N_j / D_j = 1."""
    n = 1 << log2n
    rng = np.random.default_rng(seed)
    total = width * n
    groups = rng.integers(0, n, size=total)
    order = np.argsort(groups, kind="stable")  # positions, group by group
    gs = groups[order]
    start = np.ones(total, dtype=bool)
    start[1:] = gs[1:] != gs[:-1]
    first = np.maximum.accumulate(np.where(start, np.arange(total), 0))  # each sorted slot's group start
    nxt = np.arange(1, total + 1)
    end = np.ones(total, dtype=bool)
    end[:-1] = start[1:]
    nxt[end] = first[end]  # the last position of a group is copied to its first
    perm = np.empty(total, dtype=np.int64)
    perm[order] = order[nxt]  # position -> the position it is copied to
    vals = random_scalars(rng, n)
    wires = vals[groups].reshape(width, n, 4)
    ids = identity_tags(oracle, log2n, ks, width).reshape(total, 4)
    sigmas = ids[perm].reshape(width, n, 4)
    return np.ascontiguousarray(wires), np.ascontiguousarray(sigmas)


def plus_p(words):
    """The [p, 2p) representative of canonical Fr values."""
    return ci.add_int(words, ci.R_MOD).reshape(np.shape(words))
