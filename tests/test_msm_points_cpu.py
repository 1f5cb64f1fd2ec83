"""CPU side of the table-free MSM over the caller's points (bbg_g1_msm, csrc/msm_points.hip): the ABI surface, the Python-integer model
of the recoding and of the whole route (tests/tools/msm_points_model.py), and the model's plan pinned to bbg_g1_msm_plan, which needs no
device.  Python integers only."""
import ctypes
import os
import random
import re

import pytest

import msm_points_model as mp
import var_base_model as vb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("bbg_g1_msm", "bbg_g1_msm_device", "bbg_g1_msm_plan")
R = vb.R_MOD
WIDTHS = range(mp.C_MIN, mp.C_MAX + 1)


def test_header_and_binding_declare_the_entry_points(pkg):
    header = open(os.path.join(ROOT, "include", "bbg.h")).read()
    declared = set(re.findall(r"\b(bbg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    for sym in NEW_SYMBOLS:
        assert sym in declared, f"{sym} is not declared in include/bbg.h"
        assert sym in pkg.binding.EXPORTED_SYMBOLS, f"{sym} is missing from binding.EXPORTED_SYMBOLS"
    for method in ("g1_msm", "g1_msm_device", "g1_msm_plan"):
        assert callable(getattr(pkg.Bbg, method, None)), f"Bbg.{method} is missing"
    for name in ('"msm_points_sort"', '"msm_points_accumulate"', '"msm_points_reduce"', '"msm_points_combine"'):
        assert name in header, f"{name} is not listed in include/bbg.h"


def half_cases():
    k1_max, k2_max = vb.half_bounds()
    rng = random.Random(0x5CA1AB1E + 40)
    # half_bounds() gives the exact upper bounds as RATIONALS that no half reaches (e1, e2 are strict bounds): the largest integer a half
    # can be is below each, so the floors stand for "at the exact upper bounds"; 2^127 - 1 is above both floors and is the last value the
    # proof of windows(c) covers, so the recoding is also held there
    return [0, 1, int(k1_max), int(k2_max), (1 << 127) - 1] + [rng.randrange(1 << 127) for _ in range(200)]


@pytest.mark.parametrize("c", WIDTHS)
def test_recoding_recombines_with_no_carry_left(c):
    w = mp.windows(c)
    for h in half_cases():
        digits, carry = mp.recode(h, c)
        assert len(digits) == w and carry == 0, f"c = {c}, h = {h:#x}: carry left"
        assert all(abs(d) <= 1 << (c - 1) for d in digits)
        assert sum(d << (c * i) for i, d in enumerate(digits)) == h
    # windows(c) is the smallest count: with one window less the bounds do not fit
    for bound in vb.half_bounds():
        digits, carry = mp.recode(int(bound), c, w - 1)
        assert carry == 1 or int(bound) >> (c * (w - 1)), f"c = {c}: {w - 1} windows would do for a bound"


@pytest.mark.parametrize("c", WIDTHS)
def test_key_and_payload_round_trip(c):
    rng = random.Random(c)
    w = mp.windows(c)
    for _ in range(200):
        win, mag = rng.randrange(w), rng.randrange(1, (1 << (c - 1)) + 1)
        d = mag if rng.random() < 0.5 else -mag
        negate, twin, term = rng.random() < 0.5, rng.random() < 0.5, rng.choice([0, 1, mp.TERM, rng.randrange(mp.TERM)])
        key, payload = mp.entry(win, d, c, negate, twin, term)
        assert key < w << (c - 1) and payload < 1 << 32  # below the dump key, one 32-bit word
        assert mp.unpack(key, payload, c) == (win, mag, (d < 0) != negate, twin, term)


@pytest.mark.parametrize("c", WIDTHS)
def test_reduction_dataflow_is_the_weighted_bucket_sum(c):
    rng = random.Random(100 + c)
    nb = 1 << (c - 1)
    for fill in (lambda: rng.randrange(-10**9, 10**9), lambda: 1, lambda: rng.choice([0, 0, 0, 5])):
        B = [fill() for _ in range(nb)]
        assert mp.weighted_sum(B, c) == sum((b + 1) * B[b] for b in range(nb))


@pytest.mark.parametrize("c", WIDTHS)
def test_whole_route_on_integers(c):
    _, ks = vb.gpu_scalars()
    if c < 6:
        ks = ks[:60]  # the edge values and constructed halves; hundreds of windows per scalar otherwise
    ks = ks + [R, R + 1, 2 * R - 1]
    rng = random.Random(200 + c)
    values = [rng.randrange(R) for _ in ks]
    assert mp.route(ks, values, c) == sum(k * a for k, a in zip(ks, values)) % R


@pytest.mark.parametrize("c", WIDTHS)
def test_designed_scalars_hold_every_edge(c):
    ks = mp.designed_scalars(c)
    assert len(ks) == 300 and all(0 <= k < 2 * R for k in ks)
    found = set()
    for k in ks:
        found |= mp.edges(k, c)
    for edge in mp.EDGES:
        assert edge in found, f"c = {c}: no designed scalar reaches '{edge}'"
    assert "digit of magnitude 2^(c-1)" in mp.edges(1 << (c - 1), c)
    assert "carry through three windows" in mp.edges((1 << (3 * c)) - 1, c)
    rng = random.Random(300 + c)
    values = [rng.randrange(R) for _ in ks]
    assert mp.route(ks[:40] + ks[-3:], values[:40] + values[-3:], c) == sum(k * a for k, a in zip(ks[:40] + ks[-3:], values[:40] + values[-3:])) % R


def c_plan(lib, n, window_bits):
    c, w, chunk, seg = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = lib.bbg_g1_msm_plan(n, window_bits, ctypes.byref(c), ctypes.byref(w), ctypes.byref(chunk), ctypes.byref(seg))
    return rc, (c.value, w.value, chunk.value, seg.value)


def test_plan_is_the_models_and_stays_in_budget(pkg):
    lib = pkg.load_library()
    sizes = {0, 1, 2, 3}
    for e in range(1, 29):
        sizes |= {(1 << e) - 1, 1 << e, (1 << e) + 1}
    sizes = sorted(s for s in sizes if s <= mp.MAX_N)
    assert mp.MAX_N >= 1 << 24 and sizes[-1] == mp.MAX_N
    for n in sizes:
        for wb in (0, mp.C_MIN, 13, mp.C_MAX):
            rc, got = c_plan(lib, n, wb)
            assert rc == 0 and got == mp.plan(n, wb), f"n = {n}, window_bits = {wb}: the C plan {got} is not the model's {mp.plan(n, wb)}"
            c, w, chunk, seg = got
            assert mp.C_MIN <= c <= mp.C_MAX and (wb == 0 or c == wb) and w == mp.windows(c)
            assert chunk >= 1 and seg >= 1
            assert mp.workspace_bytes(c, max(min(n, chunk), 1)) <= mp.BUDGET
    for c in WIDTHS:  # every width at the size that needs the most memory
        rc, got = c_plan(lib, mp.MAX_N, c)
        assert rc == 0 and got == mp.plan(mp.MAX_N, c) and mp.workspace_bytes(c, got[2]) <= mp.BUDGET
    assert pkg.Bbg.g1_msm_plan(1000) == mp.plan(1000)
    # refusals: out values untouched
    for n, wb in ((mp.MAX_N + 1, 0), (10, 1), (10, mp.C_MAX + 1), (10, -1)):
        rc, got = c_plan(lib, n, wb)
        assert rc == -1 and got == (-1, -1, 0, 0) and mp.plan(n, wb) is None
        with pytest.raises(pkg.BbgError):
            pkg.Bbg.g1_msm_plan(n, wb)
    assert lib.bbg_g1_msm_plan(5, 0, None, None, None, None) == 0
