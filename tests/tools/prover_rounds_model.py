"""Model of the resident prover's rounds 5a, 5b and 6 (csrc/prover.hip: bbg_prover_evaluate, bbg_prover_linearise, bbg_prover_round6) on
coefficient arrays: Montgomery words in (any representative below 2p), canonical Montgomery words out.  No device calls; every step is one
of the C oracle's field operations (fe_mul, fe_add, canon, poly_eval, kate_opening, root_of_unity), which tests/test_oracle_golden.py
pins to the reference.  tests/test_prover_rounds_model_cpu.py holds the functions below against Python integers.

With n = 2^lg and w_n the domain's root:
  evaluations     P_k(zeta), or P_k(zeta w_n) where shifted[k] is set; each array has its own length (n, n + 1, 4n)
  linearisation   r = sum_k scalars[k] P_k over the arrays' common length, and r(zeta)
  openings        F = t_low + sum_k nu_k P_k (F = t_low for no terms), extended by F[n] = top_scalar * t[3n] for StandardPLONK, whose t_high has
                  n + 1 coefficients; F' = sum_k nu'_k P'_k;  W_zeta = the first n coefficients of (F - F(zeta)) / (X - zeta) -- the quotient of
                  an (n + 1)-coefficient F has n, its last word is the zero of an exact division --, W_zeta_omega = (F' - F'(zeta w_n)) / (X - zeta w_n)
The opening points must not be zero: kate_opening runs the reference's recurrence, which divides by the point."""
import numpy as np

_ORACLE = None


def oracle():
    """The C oracle, loaded on first use."""
    global _ORACLE
    if _ORACLE is None:
        from oracle.oracle import Oracle
        _ORACLE = Oracle()
    return _ORACLE


def canon(words):
    """Canonical representatives, in the shape given."""
    return oracle().canon(0, words).reshape(np.shape(words))


def times_root(zeta, lg):
    """zeta * w_n, canonical."""
    o = oracle()
    return canon(o.fe_mul(0, canon(zeta).reshape(1, 4), o.root_of_unity(lg).reshape(1, 4))[0])


def evaluations(coeff_arrays, shifted, zeta, lg):
    """(count, 4): array k at zeta, or at zeta * w_n where shifted[k] is set (shifted may be None)."""
    o = oracle()
    z, zw = canon(zeta), times_root(zeta, lg)
    flags = shifted if shifted is not None else [0] * len(coeff_arrays)
    return np.stack([canon(o.poly_eval(canon(c), zw if s else z)) for c, s in zip(coeff_arrays, flags)])


def combination(base, coeff_arrays, scalars, length):
    """base + sum_k scalars[k] * coeff_arrays[k] over `length` coefficients (base may be None = 0), canonical."""
    o = oracle()
    acc = canon(base[:length]) if base is not None else np.zeros((length, 4), dtype=np.uint64)
    for c, s in zip(coeff_arrays, scalars):
        assert len(c) >= length
        acc = o.fe_add(0, acc, o.fe_mul(0, canon(c[:length]), np.tile(canon(s), (length, 1))))
    return canon(acc)


def linearisation(coeff_arrays, scalars, zeta):
    """(r, r(zeta)) with r = sum_k scalars[k] * P_k; the arrays share one length."""
    length = len(coeff_arrays[0])
    assert all(len(c) == length for c in coeff_arrays) and len(coeff_arrays) == len(scalars)
    r = combination(None, coeff_arrays, scalars, length)
    return r, canon(oracle().poly_eval(r, canon(zeta)))


def opened_polynomials(t_low, arrays_zeta, nu_zeta, arrays_omega, nu_omega, top=None):
    """(F, F'): the polynomials round 6 opens.  top = (top_scalar, t[3n]) appends F[n] = top_scalar * t[3n]."""
    n = len(t_low)
    f = combination(t_low, arrays_zeta, nu_zeta, n)
    if top is not None:
        o = oracle()
        extra = o.fe_mul(0, canon(top[0]).reshape(1, 4), canon(top[1]).reshape(1, 4))
        f = np.concatenate([f, canon(extra)])
    assert len(arrays_omega) >= 1
    return f, combination(None, arrays_omega, nu_omega, n)


def openings(t_low, arrays_zeta, nu_zeta, arrays_omega, nu_omega, zeta, zeta_omega, top=None):
    """(W_zeta, W_zeta_omega), n canonical coefficients each."""
    o = oracle()
    n = len(t_low)
    f, f_shifted = opened_polynomials(t_low, arrays_zeta, nu_zeta, arrays_omega, nu_omega, top)
    assert canon(zeta).any() and canon(zeta_omega).any(), "kate_opening divides by the opening point"
    w, _ = o.kate_opening(f, canon(zeta))
    w = canon(w)
    assert not w[n:].any() and len(w) - n in (0, 1), "the quotient of n + 1 coefficients has n"
    w_shifted, _ = o.kate_opening(f_shifted, canon(zeta_omega))
    return w[:n], canon(w_shifted)
