"""CPU model of the Lagrange-base SRS transform, built only from the C oracle (oracle/bn254_oracle.c) and Python integers:

    LB[k] = n^-1 * sum_j w_n^(-j k) * M_j,   w_n = fr::get_root_of_unity(log2n)

what lagrange_base::transform_srs returns (srs/lagrange_base_transformation/lagrange_base.cpp) and bbg_srs_lagrange computes.
Shared by tests/test_lagrange_srs_cpu.py, tests/test_gpu_lagrange_srs.py and tests/golden/gen_golden_lagrange_srs.py."""
import numpy as np

R_MOD = 21888242871839275222246405745257275088548364400416034343698204186575808495617  # BN254 Fr


def limbs_to_int(a):
    return sum(int(x) << (64 * i) for i, x in enumerate(np.asarray(a, dtype=np.uint64).reshape(4)))


def ints_to_limbs(vals):
    out = np.empty((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        for l in range(4):
            out[i, l] = (v >> (64 * l)) & 0xFFFFFFFFFFFFFFFF
    return out


def ints_to_mont(oracle, vals):
    """Plain integers mod r -> Montgomery-form Fr limbs, the form every scalar crosses the C ABI in."""
    return oracle.to_mont(0, ints_to_limbs([v % R_MOD for v in vals]))


def root(oracle, log2n):
    """w_n as a plain integer."""
    w = limbs_to_int(oracle.from_mont(0, oracle.canon(0, oracle.root_of_unity(log2n).reshape(1, 4)))[0])
    assert pow(w, 1 << log2n, R_MOD) == 1 and (log2n == 0 or pow(w, 1 << (log2n - 1), R_MOD) == R_MOD - 1)
    return w


def canon_points(oracle, pts):
    """(n, 8) Montgomery affine points with both coordinates reduced below p."""
    p = np.ascontiguousarray(pts, dtype=np.uint64).reshape(-1, 8)
    return oracle.canon(1, p.reshape(-1, 4)).reshape(-1, 8)


def lagrange_scalars(oracle, log2n, k):
    """[n^-1 w_n^(-j k)]_j as Montgomery Fr: the row of the inverse DFT matrix that makes LB[k]."""
    n = 1 << log2n
    w_inv, n_inv = pow(root(oracle, log2n), R_MOD - 2, R_MOD), pow(n, R_MOD - 2, R_MOD)
    return ints_to_mont(oracle, [n_inv * pow(w_inv, (j * k) % n, R_MOD) for j in range(n)])


def lagrange_point(oracle, points, log2n, k):
    """LB[k] of the first 2^log2n points, canonical."""
    n = 1 << log2n
    return canon_points(oracle, oracle.msm_naive(lagrange_scalars(oracle, log2n, k), np.ascontiguousarray(points[:n])))[0]


def lagrange_srs(oracle, points, log2n):
    """The whole table by the model: n naive MSMs of n terms (small n only)."""
    return np.stack([lagrange_point(oracle, points, log2n, k) for k in range(1 << log2n)])

