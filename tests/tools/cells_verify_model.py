"""CPU model of bbg_cells_verify_reduce (csrc/cells_verify.hip): a batch of cell proofs reduced to the two points of one
pairing check, on Python integers for Fr and the C oracle's group operations.

With n = 2^log2n, l = 2^log2cell, r = n / l, w = w_n and phi = w^l, cell m < r is { w^(m + r t) : t < l }.  A batch is ncom commitments and K
cells; cell k has a commitment index c_k, a cell index m_k, l values v_k[t] (cell-major order, as bbg_cells_values writes them) and a proof
pi_k.  With I_k the interpolant of degree < l through cell k's values and s_b the first l points of a string,

    L = sum_k rho^k pi_k
    R = sum_k rho^k (C_(c_k) - [I_k] + phi^(m_k) pi_k),      [I_k] = sum_(b<l) I_k,b s_b.

Scalars are plain integers here, points (8,) uint64 Montgomery affine words; mont() of cells_model.py makes the scalar words of the C ABI.

    interpolant_sum_definition   A = the coefficients of sum_k rho^k I_k, each I_k by Lagrange's formula on integers.
    interpolant_sum_route        the same by the device's route: E[m + r t] = sum_(k: m_k = m) rho^k v_k[t], g = iNTT_n(E), A_b = r g_b.
    reduce_definition            (L, R) from the definition: one weighted sum per output, every cell on its own.
    reduce_route                 (L, R) by the device's route: the groups by m and by c, S_m, W_c, sum_m phi^m S_m, A by the transform.
    holds                        over s_j = [x^j] G an honest batch satisfies [x^l] L = R: the pairing check for a known x.
    honest_batch                 commitments [f_c(x)] G, values and proofs [(f(x) - I_m(x)) / (x^l - phi^m)] G for a list of (c, m)."""
import numpy as np

import cells_model as cm
import coarse_inputs as ci
import lagrange_model as lm
import open_all_model as oa
import open_cells_model as oc

R_MOD = cm.R_MOD


# ------------------------------------------------------------------------------------------------ group helpers
def weighted_sum(oracle, scalars, points):
    """sum_i scalars[i] points[i], canonical; infinite points and an empty list are handled here, not by the oracle."""
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
    assert len(scalars) == pts.shape[0]
    live = [i for i in range(len(scalars)) if not oa.is_infinity(pts[i]) and scalars[i] % R_MOD]
    if not live:
        return oa.aff_infinity()
    words = lm.ints_to_mont(oracle, [scalars[i] for i in live])
    return oa.canon_points(oracle, oracle.msm_naive(words, np.ascontiguousarray(pts[live])))[0]


def scalar_times_generator(oracle, scalars):
    """[k] G for every k, canonical, infinity for k = 0."""
    g = oracle.g1_generator()
    out = [oa.aff_infinity() if k % R_MOD == 0 else oracle.g1_mul(g, lm.ints_to_mont(oracle, [k])[0]) for k in scalars]
    return oa.canon_points(oracle, np.stack(out))


def powers(rho, K):
    out, run = [], 1  # rho^0 = 1, also for rho = 0
    for _ in range(K):
        out.append(run)
        run = run * rho % R_MOD
    return out


# ------------------------------------------------------------------------------------------------ A = the coefficients of sum_k rho^k I_k
def interpolant_sum_definition(log2n, log2cell, cell_ids, values, rho):
    """Each I_k by Lagrange interpolation through its l points (l <= 64), then the weighted sum."""
    n, l, r = cm.shape(log2n, log2cell)
    K = len(cell_ids)
    assert len(values) == K * l
    A = [0] * l
    for k, (m, pk) in enumerate(zip(cell_ids, powers(rho, K))):
        I_k = cm.interpolate_definition(cm.cell_points(log2n, log2cell, [m]), values[k * l:(k + 1) * l])
        A = [(a + pk * c) % R_MOD for a, c in zip(A, I_k)]
    return A


def folded_values(log2n, log2cell, cell_ids, values, rho):
    """E in domain order: E[m + r t] = sum_(k: m_k = m) rho^k v_k[t], zero on the cells nobody sampled."""
    n, l, r = cm.shape(log2n, log2cell)
    E = [0] * n
    for k, (m, pk) in enumerate(zip(cell_ids, powers(rho, len(cell_ids)))):
        assert 0 <= m < r
        for t in range(l):
            E[m + r * t] = (E[m + r * t] + pk * values[k * l + t]) % R_MOD
    return E


def inverse_transform(vals, log2n):
    """iNTT_n on Python integers alone."""
    n = 1 << log2n
    w_inv = pow(ci.root_of_unity(log2n), R_MOD - 2, R_MOD)
    n_inv = pow(n, R_MOD - 2, R_MOD)
    return [v * n_inv % R_MOD for v in oa.fr_fft([v % R_MOD for v in vals], w_inv)]


def interpolant_sum_route(log2n, log2cell, cell_ids, values, rho):
    """A_b = r g_b, b < l, g = iNTT_n(E).  Also returns g, so that a test can look at the blocks the sum over m kills."""
    n, l, r = cm.shape(log2n, log2cell)
    g = inverse_transform(folded_values(log2n, log2cell, cell_ids, values, rho), log2n)
    return [r * c % R_MOD for c in g[:l]], g


def cell_interpolant_from_blocks(g, log2n, log2cell, m):
    """g mod (X^l - phi^m): coefficient b is sum_u phi^(m u) g_(b + l u) -- the interpolant of E on cell m."""
    n, l, r = cm.shape(log2n, log2cell)
    phi_m = pow(ci.root_of_unity(log2n), l * m, R_MOD)
    return [sum(pow(phi_m, u, R_MOD) * g[b + l * u] for u in range(r)) % R_MOD for b in range(l)]


# ------------------------------------------------------------------------------------------------ (L, R)
def reduce_definition(oracle, srs_points, log2n, log2cell, commitments, commitment_ids, cell_ids, values, proofs, rho):
    n, l, r = cm.shape(log2n, log2cell)
    K = len(cell_ids)
    com = np.ascontiguousarray(commitments, dtype=np.uint64).reshape(-1, 8)
    prf = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 8)
    s = np.ascontiguousarray(srs_points, dtype=np.uint64).reshape(-1, 8)[:l]
    assert prf.shape[0] == K and len(commitment_ids) == K and len(values) == K * l and s.shape[0] == l
    phi = pow(ci.root_of_unity(log2n), l, R_MOD)
    pw = powers(rho, K)
    L = weighted_sum(oracle, pw, prf)
    terms = []
    for k in range(K):  # rho^k (C - [I_k] + phi^m pi_k), cell by cell
        I_k = cm.interpolate_definition(cm.cell_points(log2n, log2cell, [cell_ids[k]]), values[k * l:(k + 1) * l])
        scalars = [pw[k]] + [-pw[k] * c % R_MOD for c in I_k] + [pw[k] * pow(phi, cell_ids[k], R_MOD) % R_MOD]
        terms.append(weighted_sum(oracle, scalars, np.concatenate([com[commitment_ids[k]][None], s, prf[k][None]])))
    return L, weighted_sum(oracle, [1] * K, np.stack(terms))


def groups(ids, count):
    out = [[] for _ in range(count)]
    for k, g in enumerate(ids):
        out[g].append(k)
    return out


def reduce_route(oracle, srs_points, log2n, log2cell, commitments, commitment_ids, cell_ids, values, proofs, rho):
    n, l, r = cm.shape(log2n, log2cell)
    K = len(cell_ids)
    com = np.ascontiguousarray(commitments, dtype=np.uint64).reshape(-1, 8)
    prf = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 8)
    s = np.ascontiguousarray(srs_points, dtype=np.uint64).reshape(-1, 8)[:l]
    phi = pow(ci.root_of_unity(log2n), l, R_MOD)
    pw = powers(rho, K)
    by_m, by_c = groups(cell_ids, r), groups(commitment_ids, com.shape[0])
    S = np.stack([weighted_sum(oracle, [pw[k] for k in grp], prf[grp]) for grp in by_m])
    W = [sum(pw[k] for k in grp) % R_MOD for grp in by_c]
    A, _ = interpolant_sum_route(log2n, log2cell, cell_ids, values, rho)
    L = weighted_sum(oracle, [1] * r, S)
    parts = np.stack([weighted_sum(oracle, W, com), weighted_sum(oracle, [-a % R_MOD for a in A], s),
                      weighted_sum(oracle, [pow(phi, m, R_MOD) for m in range(r)], S)])
    return L, weighted_sum(oracle, [1, 1, 1], parts)


def holds(oracle, L, R, x, log2cell):
    """[x^l] L = R: what e(L, [x^l]_2) = e(R, [1]_2) says over a powers string of a known x."""
    return np.array_equal(weighted_sum(oracle, [pow(x, 1 << log2cell, R_MOD)], np.asarray(L, dtype=np.uint64)[None]),
                          oa.canon_points(oracle, R)[0])


# ------------------------------------------------------------------------------------------------ honest batches over s_j = [x^j] G
def honest_batch(oracle, polys, x, log2cell, cells):
    """polys: coefficient lists of one length n; cells: (c, m) pairs.  Returns (commitments (ncom, 8), commitment_ids, cell_ids, values
    (K l integers), proofs (K, 8))."""
    n = len(polys[0])
    lg, l, r = oc.shape(n, log2cell)
    commitments = scalar_times_generator(oracle, [oc.horner(f, x) for f in polys])
    on_domain = [oa.fr_fft([c % R_MOD for c in f], ci.root_of_unity(lg)) for f in polys]
    proof_scalars = [oc.cell_closed_form_scalars(f, x, log2cell) for f in polys]
    used = sorted(set(cells))
    point = dict(zip(used, scalar_times_generator(oracle, [proof_scalars[c][m] for c, m in used])))
    values = [on_domain[c][m + r * t] for c, m in cells for t in range(l)]
    return commitments, [c for c, _ in cells], [m for _, m in cells], values, np.stack([point[cm_] for cm_ in cells])
