"""The wire forms of G1 points and scalars without a GPU: tests/tools/wire_model.py against the definition of every form, against the
reference's own compressed words (tests/golden/g1_wire.json, made from the reference's headers by tests/golden/gen_golden_g1_wire.py) and,
where the compiled reference runs, against its serialize_to_buffer, on_curve and Montgomery conversions."""
import json
import os
import random

import numpy as np
import pytest

import pairing_model as pm
import wire_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q, R = wm.Q, wm.R


@pytest.fixture(scope="module")
def points():
    return wm.multiples_of_g(65)


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "g1_wire.json")) as f:
        return json.load(f)["points"]


# ------------------------------------------------------------------------------------------------ the square root and the kernel's program
def test_window_program_recomposes_the_exponent():
    assert wm.SQRT_EXP.bit_length() == 252 and bin(wm.SQRT_EXP).count("1") == 109
    src = open(os.path.join(ROOT, "aztec-2.0_amd", "csrc", "wire.hip")).read()
    assert f"#define BBG_WIRE_WINDOW {wm.WINDOW} " in src, "the model's window width is the kernel's default"
    rng = random.Random(7)
    for window in (2, 3, 4, 5):
        first, start, steps = wm.window_program(window)
        windows = [(start + 1, first)] + steps
        assert sum(v << l for l, v in windows) == wm.SQRT_EXP                      # the program recomposes to (q + 1) / 4
        assert all(v & 1 and v < 1 << window for _, v in windows)                  # odd values the table holds
        assert [l for l, _ in windows] == sorted({l for l, _ in windows}, reverse=True) and windows[-1][0] >= 0
        assert len(steps) <= 128                                                   # the sixteen words of entry digits
        counts = {}
        for a in [0, 1, 2, 3, Q - 1, Q - 3] + [rng.randrange(Q) for _ in range(10)]:
            assert wm.window_pow(a, window, counts) == wm.sqrt_candidate(a)
        assert counts == {"table": 1 << (window - 1), "squarings": start + 1, "products": len(steps)}
    counts = {}
    wm.window_pow(5, counts=counts)
    assert counts == {"table": 8, "squarings": 250, "products": 47}, counts  # with a^2 and the 7 table products: 305 products a root


def test_candidate_is_a_root_exactly_for_residues():
    rng = random.Random(11)
    for a in [rng.randrange(1, Q) for _ in range(100)]:
        y = wm.sqrt_candidate(a)
        if wm.is_non_residue(a):
            assert y * y % Q == Q - a
        else:
            assert y * y % Q == a
    assert wm.is_non_residue(3) and wm.decode_word(0)[0] == wm.OFF_CURVE  # x = 0: y^2 = 3 has no solution
    for x in (1, 2, 3, Q - 2, Q - 1):
        assert not wm.is_non_residue(wm.rhs(x)), x
    random.seed(1)
    xs = [random.randrange(Q) for _ in range(256)]
    assert sum(1 for x in xs if wm.is_non_residue(wm.rhs(x))) == 129  # the split tests/test_gpu_wire.py asserts on the device


# ------------------------------------------------------------------------------------------------ model against definition
def test_decode_is_the_definition_and_encode_inverts_it(points):
    for form in (wm.G1_COMPRESSED, wm.G1_COMPRESSED_BYTES):
        for p in points + [None]:
            st, data = wm.encode(form, p)
            assert st == (wm.INFINITY if p is None else wm.VALID) and len(data) == 32
            w = wm.word_from_bytes(form, data)
            st2, back = wm.decode(form, data)
            assert back == p and st2 == st
            if p is not None:
                assert wm.is_decoding_of(w, back) and w == p[0] | (p[1] & 1) << 255
            assert wm.encode(form, back)[1] == data
    assert {p[1] & 1 for p in points} == {0, 1}
    # every valid word round-trips; the other parity is the negated point
    rng = random.Random(3)
    seen = 0
    while seen < 40:
        w = rng.randrange(Q) | rng.randrange(2) << 255
        st, p = wm.decode_word(w)
        if st == wm.VALID:
            seen += 1
            assert wm.is_decoding_of(w, p) and wm.compress(p) == w
            assert wm.decode_word(w ^ 1 << 255) == (wm.VALID, (p[0], Q - p[1]))
        else:
            assert st == wm.OFF_CURVE and wm.is_non_residue(wm.rhs(w & (wm.INF_WORD - 1)))


def test_malformed_words_and_buffers(points):
    assert wm.decode_word(wm.INF_WORD) == (wm.INFINITY, None)
    for w in (Q, Q + 1, (1 << 254) - 1, wm.INF_WORD | 1, wm.INF_WORD | 1 << 255, (1 << 256) - 1, Q | 1 << 255):
        assert wm.decode_word(w) == (wm.MALFORMED, None), hex(w)
    assert wm.decode_word(Q - 1)[0] == wm.VALID
    x, y = points[4]
    buf = lambda yy, xx: yy.to_bytes(32, "big") + xx.to_bytes(32, "big")
    assert wm.decode(wm.G1_BUFFER, buf(y, x)) == (wm.VALID, (x, y))
    assert wm.decode(wm.G1_BUFFER, buf(y + 1, x)) == (wm.OFF_CURVE, None)
    assert wm.decode(wm.G1_BUFFER, buf(y + Q, x)) == (wm.MALFORMED, None)          # y >= q
    assert wm.decode(wm.G1_BUFFER, buf(y, Q)) == (wm.MALFORMED, None)
    assert wm.decode(wm.G1_BUFFER, buf(y | 1 << 254, x)) == (wm.MALFORMED, None)   # bit 6 of byte 0
    assert wm.decode(wm.G1_BUFFER, bytes([0x80 | 0x55]) + bytes(range(63))) == (wm.INFINITY, None)  # the flag over junk
    assert wm.encode(wm.G1_BUFFER, None) == (wm.INFINITY, wm.INF_BUFFER)
    for form in wm.G1_FORMS:
        assert wm.encode(form, (x, y + 1), check=1) == (wm.OFF_CURVE, wm.encode(form, None)[1])
        st, data = wm.encode(form, (x, y + 1), check=0)
        assert st == wm.VALID and data != wm.encode(form, (x, y))[1]
        assert wm.encode(form, (x + Q, y + Q)) == wm.encode(form, (x, y))
    for form in (wm.FR, wm.FR_BYTES):
        for v in (0, 1, R - 1):
            assert wm.decode(form, wm.word_to_bytes(form, v)) == (wm.VALID, v)
            assert wm.encode(form, v + R) == (wm.VALID, wm.word_to_bytes(form, v))
        for v in (R, (1 << 256) - 1):
            assert wm.decode(form, wm.word_to_bytes(form, v)) == (wm.MALFORMED, 0)
    assert wm.word_to_bytes(wm.FR, 1)[0] == 1 and wm.word_to_bytes(wm.FR_BYTES, 1)[31] == 1


def test_batches_are_the_elements(points):
    for form in wm.G1_FORMS:
        vals = points[:5] + [None]
        wire = b"".join(wm.encode(form, p)[1] for p in vals)
        native, status, bad = wm.decode_batch(form, wire)
        assert bad == 0 and list(status) == [1] * 5 + [3] and np.array_equal(native[5], pm.G1_INFINITY_WORDS)
        assert wm.native_values(form, native) == vals
        again, status, bad = wm.encode_batch(form, native)
        assert again == wire and bad == 0 and list(status) == [1] * 5 + [3]
    native, status, bad = wm.decode_batch(wm.FR, wm.word_to_bytes(wm.FR, 5) + wm.word_to_bytes(wm.FR, R))
    assert bad == 1 and list(status) == [1, 0] and wm.native_values(wm.FR, native) == [5, 0]


# ------------------------------------------------------------------------------------------------ the reference's own compressed words
def test_compressed_form_is_the_references(fixture, points):
    assert [e["k"] for e in fixture] == list(range(1, 33))
    for e, mine in zip(fixture, points):
        p = (int(e["x"], 16), int(e["y"], 16))
        assert p == mine and e["negated"] == (e["k"] % 3 == 0) and e["on_curve"] and e["roundtrip_equal"]
        w = int(e["word"], 16)
        assert wm.compress(p) == w
        assert wm.encode(wm.G1_COMPRESSED, p) == (wm.VALID, w.to_bytes(32, "little"))
        assert wm.encode(wm.G1_COMPRESSED_BYTES, p) == (wm.VALID, bytes.fromhex(e["word_bytes"]))
        assert wm.encode(wm.G1_BUFFER, p) == (wm.VALID, bytes.fromhex(e["buffer"]))
        assert wm.decode_word(w) == (wm.VALID, (int(e["roundtrip_x"], 16), int(e["roundtrip_y"], 16)))
        assert wm.decode(wm.G1_COMPRESSED_BYTES, bytes.fromhex(e["word_bytes"])) == (wm.VALID, p)


# ------------------------------------------------------------------------------------------------ the compiled reference, where it runs
def test_buffer_form_and_curve_test_against_the_compiled_reference(ref, points):
    x, y = points[6]
    for p in points[:20]:
        assert ref.g1_to_buffer(pm.g1_words(p)) == wm.encode(wm.G1_BUFFER, p)[1]
    assert ref.g1_to_buffer(pm.G1_INFINITY_WORDS)[0] & 0x80 and wm.encode(wm.G1_BUFFER, None)[1][0] & 0x80  # only the flag is specified
    for p in points[:8] + [(x, y + 1), (x + 1, y), (1, 3)]:
        on = ref.g1_on_curve(pm.g1_words(p))
        assert on == wm.on_curve(p)
        assert (wm.encode(wm.G1_BUFFER, p, check=1)[0] == wm.OFF_CURVE) == (not on)
        data = p[1].to_bytes(32, "big") + p[0].to_bytes(32, "big")
        assert (wm.decode(wm.G1_BUFFER, data)[0] == wm.OFF_CURVE) == (not on)


def test_fr_forms_against_the_compiled_reference(ref):
    rng = random.Random(5)
    vals = [0, 1, R - 1] + [rng.randrange(R) for _ in range(29)]
    plain = np.array([[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64)
    to_int = lambda rows: [sum(int(r[k]) << (64 * k) for k in range(4)) % R for r in rows]
    mont = ref.fe_op(0, 4, plain)  # to_montgomery_form
    native, status, bad = wm.decode_batch(wm.FR, plain.tobytes())
    assert bad == 0 and (status == 1).all() and to_int(mont) == to_int(native)
    back = ref.fe_op(0, 5, native)  # from_montgomery_form
    assert to_int(back) == vals
    wire, _, _ = wm.encode_batch(wm.FR, native)
    assert wire == plain.tobytes()
    wire_be, _, _ = wm.encode_batch(wm.FR_BYTES, native)
    assert [int.from_bytes(wire_be[i:i + 32], "big") for i in range(0, len(wire_be), 32)] == vals
