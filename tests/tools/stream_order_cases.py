"""Inputs and expectations of tests/test_gpu_stream_order_device.py, built on the CPU alone: the C oracle and the integer models
(open_all_model, open_cells_model, cells_model, cells_verify_model, barycentric_model).  Nothing here touches the GPU or the library, so
tests/test_stream_order_cases_cpu.py holds the models to each other at these very shapes before any GPU time is spent.

Every G1 case runs over the powers string s_j = [x^j] G of X_INT, 2^10 points: over it a G1 transform, an opening proof and a commitment
are each a known scalar times G, so an expectation costs one oracle.g1_mul per point.  Each builder computes once per process (`once`) and
hands out read-only arrays."""
import numpy as np

import barycentric_model as bm
import cells_model as cm
import cells_verify_model as vm
import coarse_inputs as ci
import open_all_model as oa
import open_cells_model as oc

R = cm.R_MOD
SEED = 0xBB254 + 0x57DE
X_INT = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
RHO = 0x1F2E3D4C5B6A79880796A5B4C3D2E1F00F1E2D3C4B5A69788796A5B4C3D2E1F0 % R
LG, LC = 10, 4  # the cell shape of every cell case: n = 1024, l = 16, r = 64
N_POINTS = 1 << LG
RAGGED = 70001  # no multiple of a 256-thread block, of 1024 (the inversion groups) or of 4096

_made = {}


def once(key, make):
    if key not in _made:
        _made[key] = freeze(make())
    return _made[key]


def freeze(v):
    if isinstance(v, np.ndarray):
        v.setflags(write=False)
    elif isinstance(v, (tuple, list)):
        for x in v:
            freeze(x)
    return v


def x_mont():
    return cm.mont([X_INT])[0]


def string_points(oracle):
    """The 2^10 points of the powers string by the oracle, canonical."""
    return once("string", lambda: oa.canon_points(oracle, oracle.srs_powers(x_mont(), N_POINTS)))


def times_g(oracle, scalars):
    return vm.scalar_times_generator(oracle, scalars)


# ------------------------------------------------------------------------------------------------ G1 transform
def g1_ntt_want(oracle, inverse):
    """The transform of the string's 2^10 points: out[k] = [sum_j w^(+-jk) x^j (/ n)] G."""
    def make():
        n = N_POINTS
        w = ci.root_of_unity(LG)
        xs = [pow(X_INT, j, R) for j in range(n)]
        if not inverse:
            return times_g(oracle, oa.fr_fft(xs, w))
        n_inv = pow(n, R - 2, R)
        return times_g(oracle, [v * n_inv % R for v in oa.fr_fft(xs, pow(w, R - 2, R))])
    return once(("g1_ntt", bool(inverse)), make)


# ------------------------------------------------------------------------------------------------ openings
def poly(tag, n):
    return once(("poly", tag, n), lambda: tuple(cm.random_ints(SEED + 7919 * tag + n, n)))


def open_want(oracle, f, log2cell):
    """The proofs of f over the string: closed-form scalars times G."""
    lg = len(f).bit_length() - 1
    if log2cell == 0:
        return times_g(oracle, oa.closed_form_scalars(list(f), X_INT, ci.root_of_unity(lg)))
    return times_g(oracle, oc.cell_closed_form_scalars(list(f), X_INT, log2cell))


def open_case(oracle, lg, log2cell, tags):
    """(coefficient words (polys * n, 4), proofs (polys * count, 8)) of the polynomials `tags`, one after the other."""
    def make():
        fs = [poly(t, 1 << lg) for t in tags]
        return np.concatenate([cm.mont(f) for f in fs]), np.concatenate([open_want(oracle, f, log2cell) for f in fs])
    return once(("open", lg, log2cell, tuple(tags)), make)


# ------------------------------------------------------------------------------------------------ cells as data
def values_case(oracle, count=3):
    def make():
        fs = [poly(100 + p, N_POINTS) for p in range(count)]
        return np.concatenate([cm.mont(f) for f in fs]), np.concatenate([cm.mont(cm.cell_values(oracle, list(f), LC)) for f in fs])
    return once(("values", count), make)


def recover_case(oracle, which, count=2):
    """(ids, known values (count * K * l, 4), coefficients (count * n, 4)): K = r / 2 shuffled cells of `count` polynomials of degree K l - 1.
    which: 0 and 1 are two id sets of the same K over different polynomials."""
    def make():
        n, l, r = cm.shape(LG, LC)
        K = r // 2
        ids = [int(v) for v in np.random.default_rng(SEED + 31 + which).permutation(r)[:K]]
        known, coeffs = [], []
        for p in range(count):
            f = cm.random_ints(SEED + 1000 * which + 40 + p, K * l)
            f[-1] = f[-1] or 1
            f += [0] * (n - K * l)
            kv = cm.known_values(cm.cell_values(oracle, f, LC), ids, LC)
            known.append(cm.mont(kv))
            coeffs.append(cm.mont(f))
        return ids, np.concatenate(known), np.concatenate(coeffs)
    return once(("recover", which, count), make)


# ------------------------------------------------------------------------------------------------ the pairing-check reduction
RHO_OTHER = (RHO + 1) % R


def verify_case(oracle, ncom=2, K=16, rho=RHO):
    """An honest batch over the string and its (L, R) by the model's device route: (commitments, commitment ids, cell ids, value words,
    proofs, rho words, want (2, 8)).  rho = RHO_OTHER is the same batch under another challenge: every intermediate of the reduction that
    depends on rho -- the folded values E, their commitment [A], the products -- differs, and so do L and R."""
    def batch():
        n, l, r = cm.shape(LG, LC)
        rng = np.random.default_rng(SEED + 77)
        cells = [(int(rng.integers(0, ncom)), int(rng.integers(0, r))) for _ in range(K)]
        return vm.honest_batch(oracle, [list(poly(200 + c, n)) for c in range(ncom)], X_INT, LC, cells)

    def make():
        com, cids, mids, values, proofs = once(("verify batch", ncom, K), batch)
        L, R_ = vm.reduce_route(oracle, string_points(oracle), LG, LC, com, cids, mids, list(values), proofs, rho)
        return com, tuple(cids), tuple(mids), cm.mont(values), proofs, cm.mont([rho])[0], np.stack([L, R_])
    return once(("verify", ncom, K, rho), make)


def interpolant_commitment(oracle, case_rho, ncom=2, K=16):
    """[A] = sum_b A_b s_b of the batch under `case_rho`: what the MSM inside the reduction computes."""
    _, cids, mids, values, _, _, _ = verify_case(oracle, ncom, K, case_rho)
    A, _ = vm.interpolant_sum_route(LG, LC, list(mids), cm.unmont(values), case_rho)
    return vm.weighted_sum(oracle, A, string_points(oracle)[:1 << LC])


# ------------------------------------------------------------------------------------------------ Fr cases on plain integers
def invert_case(pkg):
    def make():
        a = pkg.synthetic_scalars(SEED + 300, RAGGED)
        a[[0, 1023, 1024, RAGGED - 1]] = 0  # zero stays zero: the ends of the array and both sides of a group boundary
        return a, bm.batch_invert(a)
    return once("invert", make)


def scale_powers_case(pkg):
    """a[j] * start * base^j on the Montgomery residues (a plain factor keeps a residue in Montgomery form)."""
    def make():
        a = pkg.synthetic_scalars(SEED + 310, RAGGED)
        start, base = pkg.synthetic_scalars(SEED + 311, 2)
        s, b = (ci.from_mont(v, 0) for v in ci.to_ints(np.stack([start, base])))
        out, f = [], s
        for v in ci.to_ints(a):
            out.append(v * f % R)
            f = f * b % R
        return a, start, base, ci.to_words(out)
    return once("scale_powers", make)


def cross_dft_case(pkg, log2g=1, length=1 << 9, log2n=10):
    """out[t len + q] = sum_s w_G^(s t) in[s len + q], w_G = w_n^(n / G)."""
    def make():
        G = 1 << log2g
        a = pkg.synthetic_scalars(SEED + 320, G * length)
        v = ci.to_ints(a)
        wg = pow(ci.root_of_unity(log2n), (1 << log2n) >> log2g, R)
        out = [sum(pow(wg, s * t, R) * v[s * length + q] for s in range(G)) % R for t in range(G) for q in range(length)]
        return a, ci.to_words(out)
    return once(("cross_dft", log2g, length, log2n), make)


def lagrange_opening_case(pkg, lg=12):
    def make():
        evals = pkg.synthetic_scalars(SEED + 330, 1 << lg)
        z = bm.mont_words([bm.Z_INTS[0]])[0]
        dest, fz = bm.opening(evals, lg, z)
        return evals, z, dest, fz
    return once(("lagrange_opening", lg), make)
