"""The dataflow of the wave-cooperative pairing kernel (csrc/pairing_wave.hip, csrc/fq12_wave.hip.h) on Python integers: the
w-basis, the lane schedule of the full and the sparse product (which lane forms which a_i b_j, which lane sums what), the line at
w^0 / w^3 / w^4, conjugation and Frobenius per coefficient, the cyclotomic squaring run as the product of x with itself, the one inversion
through the tower.  It is driven by the kernel's own tables: LINE_OPENS_STEP and PAIR_FINAL_PROGRAM are read out of
csrc/pairing_consts.hip.h, which tests/test_pairing_cpu.py holds to its generator.  Values are plain residues mod p, not Montgomery words."""
import importlib.util
import os
import re

import pairing_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CONSTS = os.path.join(ROOT, "aztec-2.0_amd", "csrc", "pairing_consts.hip.h")
P = pm.P
LANES = 64
SLOTS = 6
OP_END, OP_MUL, OP_CSQR, OP_CONJ, OP_FROB1, OP_FROB2, OP_FROB3, OP_INV = range(8)


def _generator():
    spec = importlib.util.spec_from_file_location("gen_pairing_consts", os.path.join(ROOT, "scripts", "gen_pairing_consts.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _header_words(name):
    text = open(CONSTS).read()
    body = re.search(name + r"\[[^\]]*\]\s*=\s*\{(.*?)\};", text, flags=re.S).group(1)
    return [int(w, 16) for w in re.findall(r"0x([0-9a-fA-F]+)u", body)]


LINE_OPENS_STEP = _header_words("LINE_OPENS_STEP")
FINAL_PROGRAM = _header_words("PAIR_FINAL_PROGRAM")
FROB = _generator().frobenius_table()  # [k - 1][j - 1]: the constant of reference component j = 1 .. 5


# ------------------------------------------------------------------------------------------------ the w-basis
def ref_component(i):
    """The place of a_i among the reference's components c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2: c0 = (a0, a2, a4), c1 = (a1, a3, a5)."""
    return 3 + (i >> 1) if i & 1 else i >> 1


def line_power(jj):
    """The power of w that component jj of a line (o, vw, vv) multiplies."""
    return 0 if jj == 0 else jj + 2


def to_w(a):
    """A reference fq12 as the twelve coefficients of a slot: c = 2 i + h is half h of a_i."""
    six = list(a[0]) + list(a[1])
    return [six[ref_component(c >> 1)][c & 1] for c in range(12)]


def from_w(x):
    six = [None] * 6
    for i in range(6):
        six[ref_component(i)] = (x[2 * i] % P, x[2 * i + 1] % P)
    return (tuple(six[:3]), tuple(six[3:]))


# ------------------------------------------------------------------------------------------------ the lane schedule
def product_lane(lane, sparse):
    """Phase 1: (i, jj, j) -- the lane forms a_i times component jj of the second operand, which multiplies w^j -- or None for an idle lane."""
    nj = 3 if sparse else 6
    if lane >= 6 * nj:
        return None
    i, jj = divmod(lane, nj)
    return i, jj, line_power(jj) if sparse else jj


def sum_terms(c, sparse):
    """Phase 2: the staging entries (index, half) that lane c < 12 adds up for coefficient c of the result."""
    k, h = c >> 1, c & 1
    powers = [line_power(jj) for jj in range(3)] if sparse else list(range(6))
    return [(6 * ((k + 6 - j) % 6) + j, h) for j in powers]


class Wave:
    """The LDS of one block: six slots of twelve coefficients, the staging of one product, the scaled line, the G1 points."""

    def __init__(self):
        self.slot = [[None] * 12 for _ in range(SLOTS)]
        self.prod = [[None, None] for _ in range(36)]
        self.line = [None] * 6
        self.pt = []

    def set_one(self, d):
        self.slot[d] = [1] + [0] * 11

    def mul(self, d, a, b, sparse):
        """slot d = slot a times b (twelve coefficients, or the six of a line)."""
        self.prod = [[None, None] for _ in range(36)]  # a term that phase 2 reads and this phase 1 did not write is a TypeError
        for lane in range(LANES):
            t = product_lane(lane, sparse)
            if t is None:
                continue
            i, jj, j = t
            p = pm.f2_mul((self.slot[a][2 * i], self.slot[a][2 * i + 1]), (b[2 * jj], b[2 * jj + 1]))
            if i + j >= 6:
                p = pm.f2_mul_xi(p)
            self.prod[6 * i + j] = list(p)
        self.slot[d] = [sum(self.prod[e][h] for e, h in sum_terms(c, sparse)) % P for c in range(12)]

    def conj(self, d, a):
        self.slot[d] = [-v % P if c & 2 else v for c, v in enumerate(self.slot[a])]

    def frobenius(self, d, a, k):
        out = []
        for i in range(6):
            x = (self.slot[a][2 * i], self.slot[a][2 * i + 1])
            if k & 1:
                x = pm.f2_conj(x)
            out += list(x if i == 0 else pm.f2_mul(FROB[k - 1][ref_component(i) - 1], x))
        self.slot[d] = out

    def inv(self, d, a):
        self.slot[d] = to_w(pm.f12_inv(from_w(self.slot[a])))

    def scale_line(self, line, j):
        """Lanes 0 .. 5: o | vw P.y | vv P.x of pair j."""
        o, vw, vv = line
        px, py = self.pt[j]
        self.line = [o[0], o[1], vw[0] * py % P, vw[1] * py % P, vv[0] * px % P, vv[1] * px % P]


def pairing_product(points, tables):
    """(value, status) of one product as k_pair_wave computes it: points[j] = (x, y) or None for infinity, tables[j] the 87 lines of Q_j."""
    w = Wave()
    w.pt = [p if p is not None else (0, 0) for p in points]
    live = [p is not None for p in points]
    bad = any(p is not None and (p[1] * p[1] - p[0] ** 3 - 3) % P for p in points)
    w.set_one(0)
    for it in range(pm.LINES):
        if (LINE_OPENS_STEP[it // 32] >> (it % 32)) & 1:
            w.mul(0, 0, w.slot[0], False)
        for j in range(len(points)):
            if not live[j]:
                continue
            w.scale_line(tables[j][it], j)
            w.mul(0, 0, w.line, True)
    for word in FINAL_PROGRAM:
        op, d, a, b = word & 255, (word >> 8) & 255, (word >> 16) & 255, word >> 24
        if op == OP_END:
            break
        if op in (OP_MUL, OP_CSQR):
            w.mul(d, a, w.slot[a if op == OP_CSQR else b], False)
        elif op == OP_CONJ:
            w.conj(d, a)
        elif op == OP_INV:
            w.inv(d, a)
        else:
            w.frobenius(d, a, op - OP_FROB1 + 1)
    value = from_w(w.slot[0])
    return value, 2 if bad else int(value == pm.F12_ONE)
