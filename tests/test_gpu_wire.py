"""G1 points and scalars between their wire forms and the native form on the MI355X (bbg_wire_decode*, bbg_wire_encode*, csrc/wire.hip),
held to tests/tools/wire_model.py: every native array, status word and count bit for bit.  The compressed decode runs one wave per block
(64 lanes, its window table in LDS), every other kernel 256 lanes per block; no grid is capped, so the counts straddle a wave and a block of
either size.  bbg_field_op's op 12 checks the square-root chain apart from the packing."""
import ctypes
import random

import numpy as np
import pytest

import open_points_cases as oc
import pairing_model as pm
import wire_model as wm

pytestmark = pytest.mark.gpu

Q, R = wm.Q, wm.R
GUARD = 0xA5
GUARD32 = 0xA5A5A5A5
COUNTS = [0, 1, 63, 64, 65, 200, 257]  # 65: just over the compressed decode's block, 257: just over every other kernel's
INVALID = -1


@pytest.fixture(scope="module")
def points():
    return wm.multiples_of_g(max(COUNTS))


class Dev:
    """Device buffers of one test: every output is allocated with a guard behind it, and freed at the end."""

    def __init__(self, bbg):
        self.bbg, self.ptrs = bbg, []

    def put(self, data):
        a = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        p = self.bbg.dev_alloc(a.size + 64)
        self.ptrs.append(p)
        if a.size:
            self.bbg.dev_upload(p, a)
        return p

    def out(self, nbytes):
        return self.put(np.full(nbytes + 64, GUARD, dtype=np.uint8))

    def get(self, p, nbytes):
        """The first nbytes, after checking the 64 guard bytes behind them."""
        raw = self.bbg.dev_download(p, (nbytes + 64,), dtype=np.uint8)
        assert (raw[nbytes:] == GUARD).all(), "a write past the end of an output"
        return raw[:nbytes]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.bbg.dev_free(p)


def dev_decode(bbg, form, wire, n=None):
    """(native words, status, bad) of the device form."""
    wb, nb = wm.sizes(form)
    n = len(wire) // wb if n is None else n
    with Dev(bbg) as d:
        d_wire, d_native, d_status, d_bad = d.put(wire), d.out(n * nb), d.out(n * 4), d.out(4)
        bbg.wire_decode_device(form, d_wire, n, d_native, d_status, d_bad)
        bbg.sync()
        return (d.get(d_native, n * nb).view(np.uint64).reshape(n, nb // 8), d.get(d_status, n * 4).view(np.uint32), int(d.get(d_bad, 4).view(np.uint32)[0]))


def dev_encode(bbg, form, native, check=1):
    """(wire bytes, status, bad) of the device form."""
    wb, nb = wm.sizes(form)
    native = np.ascontiguousarray(native, dtype=np.uint64).reshape(-1, nb // 8)
    n = native.shape[0]
    with Dev(bbg) as d:
        d_native, d_wire, d_status, d_bad = d.put(native), d.out(n * wb), d.out(n * 4), d.out(4)
        bbg.wire_encode_device(form, d_native, n, check, d_wire, d_status, d_bad)
        bbg.sync()
        return d.get(d_wire, n * wb).tobytes(), d.get(d_status, n * 4).view(np.uint32), int(d.get(d_bad, 4).view(np.uint32)[0])


def same(got, want):
    """(array, status, bad) triples, bit for bit."""
    a, b = got[0], want[0]
    assert (a == b if isinstance(a, bytes) else np.array_equal(a, b)), "the data"
    assert np.array_equal(got[1], want[1]), (got[1], want[1])
    assert got[2] == want[2], (got[2], want[2])


def mont_words(values, modulus, lift=0):
    """(n, 4) Montgomery words of integers, the representative in [lift * modulus, (lift + 1) * modulus)."""
    out = np.zeros((len(values), 4), dtype=np.uint64)
    for i, v in enumerate(values):
        m = v % modulus * wm.MONT % modulus + lift * modulus
        out[i] = [(m >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]
    return out


def compressed_wire(form, words):
    return b"".join(wm.word_to_bytes(form, w) for w in words)


# 1 ------------------------------------------------------------------------------------------------ counts
@pytest.mark.parametrize("n", COUNTS)
def test_counts(bbg, points, n):
    pts = points[:n]
    for form in wm.G1_FORMS:
        wire = b"".join(wm.encode(form, p)[1] for p in pts)
        want = wm.decode_batch(form, wire)
        assert want[2] == 0 and (want[1] == 1).all() and np.array_equal(want[0], wm.native_words(form, pts))
        got = dev_decode(bbg, form, wire)
        same(got, want)
        same(dev_encode(bbg, form, got[0]), (wire, want[1], 0))
    if n >= 63:
        assert {p[1] & 1 for p in pts} == {0, 1}, "both parities occur"


# 2 ------------------------------------------------------------------------------------------------ edge x
def test_edge_x(bbg):
    two = pm.fq_words([1, 2, 1, Q - 2]).reshape(2, 8)
    for form in (wm.G1_COMPRESSED, wm.G1_COMPRESSED_BYTES):
        got = dev_decode(bbg, form, compressed_wire(form, [1, 1 | 1 << 255]))
        same(got, (two, np.array([1, 1], dtype=np.uint32), 0))  # x = 1: the generator (1, 2) and its negative
        words = [x | b << 255 for x in (2, 3, Q - 2, Q - 1) for b in (0, 1)]
        got = dev_decode(bbg, form, compressed_wire(form, words))
        assert (got[1] == 1).all() and got[2] == 0
        for w, p in zip(words, wm.native_values(form, got[0])):
            assert wm.is_decoding_of(w, p), hex(w)  # the definition, no root taken
        same(got, wm.decode_batch(form, compressed_wire(form, words)))
        same(dev_decode(bbg, form, compressed_wire(form, [0, 1 << 255])), (np.stack([pm.G1_INFINITY_WORDS] * 2), np.array([2, 2], dtype=np.uint32), 2))
    random.seed(1)
    xs = [random.randrange(Q) for _ in range(256)]
    non_residue = [wm.is_non_residue(wm.rhs(x)) for x in xs]  # Euler's criterion
    assert sum(non_residue) == 129
    words = [x | (i & 1) << 255 for i, x in enumerate(xs)]
    for form in (wm.G1_COMPRESSED, wm.G1_COMPRESSED_BYTES):
        native, status, bad = dev_decode(bbg, form, compressed_wire(form, words))
        assert list(status) == [2 if nr else 1 for nr in non_residue]
        assert bad == 129
        for i, p in enumerate(wm.native_values(form, native)):
            if non_residue[i]:
                assert np.array_equal(native[i], pm.G1_INFINITY_WORDS)
            else:
                assert wm.is_decoding_of(words[i], p), i  # the valid neighbours of every bad element are untouched
        same((native, status, bad), wm.decode_batch(form, compressed_wire(form, words)))


# 3 ------------------------------------------------------------------------------------------------ malformed words
def test_malformed(bbg, points):
    n, at = 130, (0, 31, 63, 64)
    pts = points[:n]
    for form in (wm.G1_COMPRESSED, wm.G1_COMPRESSED_BYTES):
        words = [wm.compress(p) for p in pts]
        for pos, w in zip(at, (Q, Q + 1, wm.INF_WORD | 1 << 100, wm.INF_WORD)):
            words[pos] = w
        words[100] = wm.INF_WORD | 1 << 255
        words[101] = Q | 1 << 255
        native, status, bad = got = dev_decode(bbg, form, compressed_wire(form, words))
        assert [int(status[p]) for p in at] == [0, 0, 0, 3] and int(status[100]) == 0 and int(status[101]) == 0 and bad == 5
        assert all(np.array_equal(native[p], pm.G1_INFINITY_WORDS) for p in at + (100, 101))
        assert (np.delete(status, at + (100, 101)) == 1).all()
        same(got, wm.decode_batch(form, compressed_wire(form, words)))
    x, y = pts[5]
    buf = [wm.encode(wm.G1_BUFFER, p)[1] for p in pts]
    b = lambda yy, xx: yy.to_bytes(32, "big") + xx.to_bytes(32, "big")
    buf[0] = b(y + Q, x)                                   # y >= q
    buf[31] = b(y | 1 << 254, x)                           # bit 6 of byte 0
    buf[63] = bytes([0x80 | 0x2A]) + bytes(range(1, 64))   # the flag over junk: infinity
    buf[64] = b(y + 1, x)                                  # off the curve
    buf[99] = b(y, Q)                                      # x >= q
    native, status, bad = got = dev_decode(bbg, wm.G1_BUFFER, b"".join(buf))
    assert [int(status[p]) for p in (0, 31, 63, 64, 99)] == [0, 0, 3, 2, 0] and bad == 4
    assert (np.delete(status, (0, 31, 63, 64, 99)) == 1).all()
    same(got, wm.decode_batch(wm.G1_BUFFER, b"".join(buf)))


# 4 ------------------------------------------------------------------------------------------------ encode
def test_encode(bbg, points):
    pts = points[:70]
    lifted = np.concatenate([mont_words([p[0] for p in pts], Q, 1), mont_words([p[1] for p in pts], Q, 1)], axis=1)  # x + q, y + q
    x, y = pts[9]
    off = pm.g1_words((x, (y + 1) % Q))
    for form in wm.G1_FORMS:
        want = b"".join(wm.encode(form, p)[1] for p in pts)
        for check in (0, 1):
            same(dev_encode(bbg, form, lifted, check), (want, np.ones(70, dtype=np.uint32), 0))
        inf = wm.encode(form, None)[1]
        assert inf == (wm.INF_BUFFER if form == wm.G1_BUFFER else wm.word_to_bytes(form, 1 << 254))
        native = np.stack([pm.g1_words(pts[0]), pm.G1_INFINITY_WORDS, off, pm.g1_words(pts[1])])
        edges = [wm.encode(form, pts[0])[1], inf, None, wm.encode(form, pts[1])[1]]
        edges[2] = inf
        same(dev_encode(bbg, form, native, 1), (b"".join(edges), np.array([1, 3, 2, 1], dtype=np.uint32), 1))
        edges[2] = wm.encode(form, (x, (y + 1) % Q), check=0)[1]  # x and the parity of the y it was given
        same(dev_encode(bbg, form, native, 0), (b"".join(edges), np.array([1, 3, 1, 1], dtype=np.uint32), 0))
        same(dev_encode(bbg, form, native, 0), wm.encode_batch(form, native, 0))
    assert wm.word_from_bytes(0, wm.encode(0, (x, (y + 1) % Q), check=0)[1]) == x | ((y + 1) % Q & 1) << 255


# 5 ------------------------------------------------------------------------------------------------ the fr forms
def test_fr_forms(bbg):
    rng = random.Random(0xF5)
    vals = [0, 1, R - 1, R, (1 << 256) - 1] + [rng.randrange(R) for _ in range(64)]
    good = [v for v in vals if v < R]
    for form in (wm.FR, wm.FR_BYTES):
        wire = b"".join(wm.word_to_bytes(form, v) for v in vals)
        native, status, bad = got = dev_decode(bbg, form, wire)
        assert list(status[:5]) == [1, 1, 1, 0, 0] and (status[5:] == 1).all() and bad == 2
        assert np.array_equal(native, pm.fr_words([v if v < R else 0 for v in vals]))
        same(got, wm.decode_batch(form, wire))
        want = b"".join(wm.word_to_bytes(form, v) for v in good)
        for lift in (0, 1):  # canonical, and the representatives in [r, 2r)
            for check in (0, 1):
                same(dev_encode(bbg, form, pm.fr_words(good, lift=lift), check), (want, np.ones(len(good), dtype=np.uint32), 0))


# 6 ------------------------------------------------------------------------------------------------ the square-root candidate alone
def test_field_op_sqrt_candidate(bbg):
    rng = random.Random(12)
    residues, others = [], []
    while len(residues) < 64 or len(others) < 64:
        a = rng.randrange(1, Q)
        (others if wm.is_non_residue(a) else residues).append(a)
    vals = residues[:64] + others[:64]
    a = np.concatenate([mont_words(vals[i::2], Q, i) for i in (0, 1)])  # half of the inputs in [q, 2q)
    vals = vals[0::2] + vals[1::2]
    out = bbg.field_op(1, 12, a)
    roots = pm.fq_ints(out)
    assert roots == [wm.sqrt_candidate(v) for v in vals] == [wm.window_pow(v) for v in vals]
    assert np.array_equal(out, mont_words(roots, Q)), "canonical"
    for v, y in zip(vals, roots):
        assert y * y % Q == (Q - v if wm.is_non_residue(v) else v)
    assert pm.fq_ints(bbg.field_op(1, 12, mont_words([0, 1, 4], Q))) == [0, 1, wm.sqrt_candidate(4)]
    one = mont_words([4], R)
    res = np.full((1, 4), GUARD32, dtype=np.uint64)
    assert bbg.lib.bbg_field_op(bbg.ctx, 0, 12, one.ctypes.data, None, res.ctypes.data, 1) == INVALID  # r = 1 mod 4: no single power is a root
    assert (res == GUARD32).all()


# 7 ------------------------------------------------------------------------------------------------ from bytes to the verdict
def test_bytes_to_verdict_on_one_stream(bbg, oracle):
    import torch
    N, LG = 8, 6
    b = oc.Batch(oracle, LG, N, 0xBB254 + 0x0C26 + 1)
    lines = bbg.g2_lines_prepare(np.stack([bbg.g2_mul(pm.fr_words([oc.X_INT]))[0], pm.g2_words(pm.G2)]))
    rho = pm.fr_words([oc.rand_fr(np.random.default_rng(77))])[0]
    form = wm.G1_COMPRESSED
    com_wire, st, bad = bbg.wire_encode(form, b.commitments)
    assert bad == 0 and (st == 1).all()
    prf_wire, st, bad = bbg.wire_encode(form, b.proofs)
    assert bad == 0 and (st == 1).all()
    assert com_wire.tobytes() == b"".join(wm.encode(form, p)[1] for p in wm.native_values(form, b.commitments))

    def verdict(proof_wire):
        with Dev(bbg) as d:
            d_cw, d_pw, d_z, d_y = d.put(com_wire), d.put(proof_wire), d.put(b.z_words), d.put(b.y_words)
            d_c, d_p, d_status, d_bad = d.out(N * 64), d.out(N * 64), d.out(4), d.out(8)
            stream = torch.cuda.Stream()
            bbg.set_stream(stream.cuda_stream)
            try:
                bbg.wire_decode_device(form, d_cw, N, d_c, None, d_bad)
                bbg.wire_decode_device(form, d_pw, N, d_p, None, d_bad + 4)
                bbg.kzg_verify_device(lines, d_c, d_z, d_y, d_p, N, rho, d_status)
                stream.synchronize()  # the one synchronisation
            finally:
                bbg.set_stream(torch.cuda.current_stream().cuda_stream)
            bads = d.get(d_bad, 8).view(np.uint32)
            return int(d.get(d_status, 4).view(np.uint32)[0]), int(bads[0]), int(bads[1])

    try:
        assert verdict(prf_wire) == (1, 0, 0)
        flipped = prf_wire.copy()
        flipped[3, 31] ^= 0x80  # the parity bit of proof 3: bit 255 of the little-endian word
        assert verdict(flipped) == (0, 0, 0)
        broken = prf_wire.copy()
        broken[5] = 0  # x = 0: x^3 + 3 = 3 is a non-residue
        assert verdict(broken)[1:] == (0, 1)
    finally:
        lines.free()


# 8 ------------------------------------------------------------------------------------------------ refusals
def test_refusals(bbg, points):
    lib, ctx = bbg.lib, bbg.ctx
    n = 8
    wire = b"".join(wm.encode(0, p)[1] for p in points[:n])
    vp = ctypes.c_void_p
    with Dev(bbg) as d:
        d_in, d_out, d_status, d_bad = d.put(wire + bytes(n * 32)), d.out(n * 64), d.out(n * 4), d.out(4)
        outs = ((d_out, n * 64), (d_status, n * 4), (d_bad, 4))

        def refused(rc, what):
            assert rc == INVALID, what
            for p, nbytes in outs:
                assert (d.get(p, nbytes) == GUARD).all(), what + ": an output was written"

        dec = lambda c, form, w, k, nat, s, bd: lib.bbg_wire_decode_device(c, form, vp(w), k, vp(nat), vp(s), vp(bd))
        enc = lambda c, form, nat, k, check, w, s, bd: lib.bbg_wire_encode_device(c, form, vp(nat), k, check, vp(w), vp(s), vp(bd))
        refused(dec(None, 0, d_in, n, d_out, d_status, d_bad), "a null context")
        refused(dec(ctx, 0, None, n, d_out, d_status, d_bad), "a null input")
        refused(dec(ctx, 0, d_in, n, None, d_status, d_bad), "a null output")
        refused(enc(ctx, 0, None, n, 1, d_out, d_status, d_bad), "a null input (encode)")
        for form in (-1, 5, 99):
            refused(dec(ctx, form, d_in, n, d_out, d_status, d_bad), "an unknown form")
            refused(enc(ctx, form, d_in, n, 1, d_out, d_status, d_bad), "an unknown form (encode)")
        for check in (2, -1):
            refused(enc(ctx, 0, d_in, n, check, d_out, d_status, d_bad), "check outside 0, 1")
            refused(enc(ctx, wm.FR, d_in, n, check, d_out, d_status, d_bad), "check outside 0, 1 (fr)")
        big = (1 << 28) + 1
        refused(dec(ctx, 0, 0x10000, big, 0x7F0000000000, None, None), "n above 2^28")  # pointers never dereferenced
        refused(enc(ctx, 2, 0x10000, big, 0, 0x7F0000000000, None, None), "n above 2^28 (encode)")
        # overlaps: the outputs named in each call are what the call would write
        refused(dec(ctx, 0, d_in, n, d_in, d_status, d_bad), "output = input")
        refused(dec(ctx, 0, d_in, n, d_in + n * 32 - 16, d_status, d_bad), "output over the input's tail")
        refused(dec(ctx, 0, d_in, n, d_out, d_in + 16, d_bad), "status over the input")
        refused(dec(ctx, 0, d_in, n, d_out, d_status, d_in + n * 32 - 4), "count over the input")
        refused(dec(ctx, 0, d_in, n, d_out, d_out + 64, d_bad), "status over the output")
        refused(dec(ctx, 0, d_in, n, d_out, d_status, d_out + n * 64 - 4), "count over the output")
        refused(dec(ctx, 0, d_in, n, d_out, d_status, d_status + 4), "count over the status words")
        refused(enc(ctx, 0, d_in, n // 2, 1, d_in + 32, d_status, d_bad), "output over the input (encode)")
        refused(dec(ctx, 0, d_in + 8, n, d_out, d_status, d_bad), "a misaligned input")
        refused(dec(ctx, 0, d_in, n, d_out + 4, d_status, d_bad), "a misaligned output")
        refused(dec(ctx, 0, d_in, n, d_out, d_status + 2, d_bad), "a misaligned status pointer")
        assert b"bbg_wire_decode_device" in lib.bbg_last_error()
        # the host forms refuse the same things
        h_in, h_out = np.frombuffer(wire, dtype=np.uint8).copy(), np.full(n * 64, GUARD, dtype=np.uint8)
        h_status, h_bad = np.full(n, GUARD32, dtype=np.uint32), ctypes.c_uint32(GUARD32)
        hd = lambda c, form, w, k, nat: lib.bbg_wire_decode(c, form, w, k, nat, h_status.ctypes.data, ctypes.byref(h_bad))
        for rc in (hd(None, 0, h_in.ctypes.data, n, h_out.ctypes.data), hd(ctx, 0, None, n, h_out.ctypes.data), hd(ctx, 0, h_in.ctypes.data, n, None),
                   hd(ctx, 7, h_in.ctypes.data, n, h_out.ctypes.data), hd(ctx, 0, h_in.ctypes.data, big, h_out.ctypes.data),
                   hd(ctx, 0, h_in.ctypes.data, n // 2, h_in.ctypes.data + 64),
                   lib.bbg_wire_encode(ctx, 0, h_in.ctypes.data, n // 2, 2, h_out.ctypes.data, h_status.ctypes.data, ctypes.byref(h_bad))):
            assert rc == INVALID
        assert (h_out == GUARD).all() and (h_status == GUARD32).all() and h_bad.value == GUARD32
        # and the sizes
        wb, nb = ctypes.c_size_t(0), ctypes.c_size_t(0)
        for form in wm.FORMS:
            assert lib.bbg_wire_sizes(form, ctypes.byref(wb), ctypes.byref(nb)) == 0 and (wb.value, nb.value) == wm.sizes(form)
        assert lib.bbg_wire_sizes(5, ctypes.byref(wb), ctypes.byref(nb)) == INVALID and lib.bbg_wire_sizes(0, None, None) == 0
        # n = 0: legal, the count is written, nothing else
        assert dec(ctx, 0, None, 0, None, None, d_bad) == 0
        bbg.sync()
        assert int(d.get(d_bad, 4).view(np.uint32)[0]) == 0 and (d.get(d_out, n * 64) == GUARD).all() and (d.get(d_status, n * 4) == GUARD).all()


# 9 ------------------------------------------------------------------------------------------------ host forms
def test_host_forms(bbg, pkg, points):
    pts = points[:70]
    x, y = pts[2]
    for form in wm.G1_FORMS:
        elems = [wm.encode(form, p)[1] for p in pts] + [wm.encode(form, None)[1]]
        wire = b"".join(elems)
        got = bbg.wire_decode(form, wire)
        same(got, dev_decode(bbg, form, wire))
        same(got, wm.decode_batch(form, wire))
        back = bbg.wire_encode(form, got[0])
        same((back[0].tobytes(), back[1], back[2]), (wire, got[1], 0))
        # something bad: BBG_E_INVALID behind the outputs
        elems[7] = wm.word_to_bytes(form, Q) if form != wm.G1_BUFFER else (y + 1).to_bytes(32, "big") + x.to_bytes(32, "big")
        wire = b"".join(elems)
        with pytest.raises(pkg.BbgError):
            bbg.wire_decode(form, wire)
        assert b"malformed or not on the curve" in bbg.lib.bbg_last_error()
        got = bbg.wire_decode(form, wire, strict=False)
        assert got[2] == 1 and int(got[1][7]) == (2 if form == wm.G1_BUFFER else 0)
        same(got, dev_decode(bbg, form, wire))
        same(got, wm.decode_batch(form, wire))
        native = got[0].copy()
        native[3] = pm.g1_words((x, (y + 1) % Q))
        with pytest.raises(pkg.BbgError):
            bbg.wire_encode(form, native, check=1)
        back = bbg.wire_encode(form, native, check=1, strict=False)
        assert back[2] == 1 and int(back[1][3]) == 2
        same((back[0].tobytes(), back[1], back[2]), dev_encode(bbg, form, native, 1))
        same((back[0].tobytes(), back[1], back[2]), wm.encode_batch(form, native, 1))
    for form in (wm.FR, wm.FR_BYTES):
        wire = b"".join(wm.word_to_bytes(form, v) for v in (5, R - 1, R, 0))
        got = bbg.wire_decode(form, wire, strict=False)
        same(got, wm.decode_batch(form, wire))
        same(got, dev_decode(bbg, form, wire))
        back = bbg.wire_encode(form, got[0])
        assert back[0].tobytes() == b"".join(wm.word_to_bytes(form, v) for v in (5, R - 1, 0, 0)) and back[2] == 0
    # no status array, no count, no elements
    n = 4
    wire = np.frombuffer(b"".join(wm.encode(0, p)[1] for p in pts[:n]), dtype=np.uint8).copy()
    out = np.zeros((n, 8), dtype=np.uint64)
    assert bbg.lib.bbg_wire_decode(bbg.ctx, 0, wire.ctypes.data, n, out.ctypes.data, None, None) == 0
    assert np.array_equal(out, wm.native_words(0, pts[:n]))
    bad = ctypes.c_uint32(GUARD32)
    assert bbg.lib.bbg_wire_decode(bbg.ctx, 0, None, 0, None, None, ctypes.byref(bad)) == 0 and bad.value == 0
