"""Inputs with designed discrete logarithms for bbg_g1_ntt and bbg_open_all: Python integers mod r only, the conventions of
open_all_model.py.

Every point of a designed input is [a] G for a known scalar a, and the a are chosen by solving a small linear system mod r so that the
kernels of csrc/ecntt.hip and csrc/open_all.hip meet what hashed or random inputs never give them:

    design_ntt      in every stage of the transform a butterfly with A = t (xyzz_add's doubling branch) and one with A = -t (its
                    result at infinity), from stage 1 on under a twiddle other than 1 and between operands that are sums themselves;
    design_string   a string whose prepared transform s_hat = NTT_G1,2n(s^) is the point at infinity at chosen indices;
    design_coeffs   coefficients whose c_hat = NTT_Fr,2n(c^) is zero at chosen indices.

Every expected output is then [y] G for an integer y computed here (dit_model, proof_scalars).  tests/test_g1_design_cpu.py holds the
designs to what they claim; tests/test_gpu_g1_ntt.py and tests/test_gpu_open_all.py run them on the device."""
import functools
import random

import coarse_inputs as ci
import open_all_model as oa

R_MOD = oa.R_MOD


def bit_reverse(i, lg):
    return int(format(i, f"0{lg}b")[::-1], 2) if lg else 0


def dit_model(vals, lg, inverse):
    """The butterflies of ecntt_stages on scalars: work[i] = vals[bitrev(i)], then stage s = 0 .. lg-1 with m = 2^s, butterfly b on
    (i, i + m), i = (b / m) 2m + j, j = b mod m, t = w^(j n / 2m) B, A' = A + t, B' = A - t.  The inverse takes w^-1, and in its last
    stage t = n^-1 w^.. B and A = n^-1 A, as the kernels do.  Returns (outputs, pairs): pairs[s][b] = (A, t) as xyzz_add meets them."""
    n = 1 << lg
    assert len(vals) == n and lg >= 1
    w = ci.root_of_unity(lg)
    if inverse:
        w = pow(w, R_MOD - 2, R_MOD)
    n_inv = pow(n, R_MOD - 2, R_MOD)
    wp = [1] * n
    for e in range(1, n):
        wp[e] = wp[e - 1] * w % R_MOD
    work = [vals[bit_reverse(i, lg)] % R_MOD for i in range(n)]
    pairs = []
    for s in range(lg):
        m = 1 << s
        last = inverse and s + 1 == lg
        stage = []
        for b in range(n // 2):
            j = b & (m - 1)
            i = ((b >> s) << (s + 1)) + j
            A, t = work[i], wp[j << (lg - 1 - s)] * work[i + m] % R_MOD
            if last:
                A, t = A * n_inv % R_MOD, t * n_inv % R_MOD
            stage.append((A, t))
            work[i], work[i + m] = (A + t) % R_MOD, (A - t) % R_MOD
        pairs.append(stage)
    return work, pairs


@functools.lru_cache(maxsize=None)
def stage_functionals(lg, inverse):
    """(minus, plus): minus[s][b] is the row of n coefficients of the linear functional "A - t at butterfly b of stage s" of the inputs,
    plus[s][b] the one of "A + t", from dit_model on the unit vectors."""
    n = 1 << lg
    minus = [[[0] * n for _ in range(n // 2)] for _ in range(lg)]
    plus = [[[0] * n for _ in range(n // 2)] for _ in range(lg)]
    for k in range(n):
        _, pairs = dit_model([int(i == k) for i in range(n)], lg, inverse)
        for s in range(lg):
            for b, (A, t) in enumerate(pairs[s]):
                minus[s][b][k] = (A - t) % R_MOD
                plus[s][b][k] = (A + t) % R_MOD
    return minus, plus


def solve(constraints, n, seed, may_repeat=0):
    """n scalars x with sum_k row[k] x[k] = 0 for every row of `constraints`: the rows are brought to reduced echelon form mod r, the
    n - t inputs without a pivot are fixed at seeded random values and the t pivot inputs follow.  Asserts that the rows are independent
    and that all inputs come out non-zero and pairwise distinct (`may_repeat`: how many of them may equal an earlier one -- A = t in
    stage 0, where the twiddle is 1, IS the equality of two inputs)."""
    rows = [[c % R_MOD for c in row] for row in constraints]
    assert all(len(row) == n for row in rows)
    rng = random.Random(seed)
    order = list(range(n))
    rng.shuffle(order)  # the pivots are looked for in a seeded order, so that they do not pile up at the low indices
    pivots = []
    for r in range(len(rows)):
        col = next((c for c in order if c not in pivots and rows[r][c]), None)
        assert col is not None, f"constraint {r} depends on the ones before it"
        inv = pow(rows[r][col], R_MOD - 2, R_MOD)
        rows[r] = [v * inv % R_MOD for v in rows[r]]
        for q in range(len(rows)):
            if q != r and rows[q][col]:
                f = rows[q][col]
                rows[q] = [(v - f * u) % R_MOD for v, u in zip(rows[q], rows[r])]
        pivots.append(col)
    x = [0 if c in pivots else rng.randrange(1, R_MOD) for c in range(n)]
    for r, col in enumerate(pivots):
        x[col] = -sum(v * xv for v, xv in zip(rows[r], x)) % R_MOD  # row[col] = 1 and x[col] = 0 so far
    assert all(x) and len(set(x)) == n - may_repeat, "a designed input is zero or repeats"
    for row in constraints:
        assert sum(v * xv for v, xv in zip(row, x)) % R_MOD == 0
    return x


def chosen_butterflies(lg, seed):
    """{stage: (butterfly with A = t, butterfly with A = -t)}, seeded.  A = t leaves infinity at the butterfly's upper place i + m and
    A = -t at its lower place i, so the butterflies of the NEXT stage that read such a place are left out: with an infinite operand
    xyzz_add returns before it compares.  Among the rest: j != 0 from stage 1 on where two such butterflies are left (always from 2^4
    on; at 2^3 the two butterflies of stage 1 with j != 0 read all four upper places of stage 0, so one of them meets the infinity of
    stage 0 and the second coincidence of stage 1 falls on j = 0); no index twice where the stage allows it; from 2^8 on the second
    butterfly of every stage has an index >= 64."""
    n = 1 << lg
    rng = random.Random(seed)
    used, out, zeroed = set(), {}, set()
    for s in range(lg):
        m = 1 << s
        place = lambda b: ((b >> s) << (s + 1)) + (b & (m - 1))
        clean = [b for b in range(n // 2) if place(b) not in zeroed and place(b) + m not in zeroed]
        pick = []
        for want_high in (False, lg >= 8):
            pool = [b for b in clean if b not in pick and (not want_high or b >= 64)]
            for keep in (lambda b: b & (m - 1) or s == 0, lambda b: b not in used):  # each preference only while it leaves a choice
                pool = [b for b in pool if keep(b)] or pool
            pick.append(rng.choice(pool))
        used.update(pick)
        out[s] = tuple(pick)
        zeroed = {place(pick[0]) + m, place(pick[1])}
    return out


def coincidences(pairs, lg):
    """{stage: (count A = t, count A = -t, of those with j != 0)} of a dit_model run, finite operands only (A = t = 0 is no coincidence
    of the group law: xyzz_add returns before it compares)."""
    report = {}
    for s in range(lg):
        m = 1 << s
        eq = [b for b, (A, t) in enumerate(pairs[s]) if A and A == t]
        op = [b for b, (A, t) in enumerate(pairs[s]) if A and (A + t) % R_MOD == 0]
        report[s] = (len(eq), len(op), sum(1 for b in eq + op if b & (m - 1)))
    return report


def design_ntt(lg, inverse, seed):
    """(inputs, expected outputs, report): n = 2^lg scalars for which every stage has a butterfly with A = t and one with A = -t
    (chosen_butterflies), what dit_model makes of them, and the coincidences the model itself meets on the way."""
    n = 1 << lg
    minus, plus = stage_functionals(lg, bool(inverse))
    chosen = chosen_butterflies(lg, seed)
    rows = []
    for s in range(lg):
        rows.append(minus[s][chosen[s][0]])
        rows.append(plus[s][chosen[s][1]])
    a = solve(rows, n, seed, may_repeat=1)
    out, pairs = dit_model(a, lg, inverse)
    return a, out, coincidences(pairs, lg)


def string_transform(a):
    """The integer s_hat of the string [a_j] G: NTT_Fr,2n of s^ = (a_(n-2), .., a_0, n + 1 zeros)."""
    n = len(a)
    lg = n.bit_length() - 1
    return oa.fr_fft([a[n - 2 - i] for i in range(n - 1)] + [0] * (n + 1), ci.root_of_unity(lg + 1))


def coeff_transform(f):
    """The integer c_hat of the coefficients f: NTT_Fr,2n of open_all_model.embedding's c^."""
    n = len(f)
    lg = n.bit_length() - 1
    c = [f[n - 1]] + [0] * (n + 1) + [f[i] for i in range(1, n - 1)]
    return oa.fr_fft([v % R_MOD for v in c], ci.root_of_unity(lg + 1))


def design_string(lg, inf_at, seed):
    """(a, s_hat): scalars a_0 .. a_(n-1) of a string [a_j] G whose s_hat is zero -- the point at infinity -- at exactly the indices
    inf_at of 0 .. 2n-1.  a_(n-1) is random and unused by bbg_open_all."""
    n = 1 << lg
    w = ci.root_of_unity(lg + 1)
    rows = [[pow(w, (n - 2 - j) * k % (2 * n), R_MOD) for j in range(n - 1)] for k in sorted(inf_at)]  # s^_i = a_(n-2-i)
    a = solve(rows, n - 1, seed) + [random.Random(seed + 1).randrange(1, R_MOD)]
    s_hat = string_transform(a)
    assert [k for k in range(2 * n) if s_hat[k] == 0] == sorted(inf_at)
    return a, s_hat


def design_coeffs(lg, zero_at, seed):
    """(f, c_hat): n = 2^lg coefficients whose c_hat is zero at exactly the indices zero_at of 0 .. 2n-1.  f_0 is free (random)."""
    n = 1 << lg
    w = ci.root_of_unity(lg + 1)
    # the variables are f_1 .. f_(n-1): c^_0 = f_(n-1), c^_(n+1+i) = f_i for i = 1 .. n-2
    rows = [[pow(w, (n + 1 + i) * k % (2 * n), R_MOD) for i in range(1, n - 1)] + [1] for k in sorted(zero_at)]
    f = [random.Random(seed + 1).randrange(1, R_MOD)] + solve(rows, n - 1, seed)
    c_hat = coeff_transform(f)
    assert [k for k in range(2 * n) if c_hat[k] == 0] == sorted(zero_at)
    return f, c_hat


def proof_scalars(f, a):
    """[sum_j q^(m)_j a_j for m < n], q^(m) = open_all_model.quotient_coeffs(f, w^m): the discrete logarithm of proof m over the string
    [a_j] G -- any string, also one of powers of an x ON the domain, where closed_form_scalars has no value."""
    n = len(f)
    lg = n.bit_length() - 1
    assert 1 << lg == n and len(a) >= n - 1
    w = ci.root_of_unity(lg)
    out, z = [], 1
    for _ in range(n):
        out.append(sum(q * aj for q, aj in zip(oa.quotient_coeffs(f, z), a)) % R_MOD)
        z = z * w % R_MOD
    return out
