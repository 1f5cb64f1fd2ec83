"""The batched calls of bbg_open_all (bbg_open_all_batch*) without a GPU: the schedules and indices of csrc/open_all.hip and
csrc/ecntt.hip on Python integers mod r (tests/tools/open_batch_model.py), and the new symbols in the header, the library and the binding.
Nothing here calls the library beyond loading it."""
import ctypes
import os
import random
import re

import pytest

import open_batch_model as ob
import open_cells_model as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = ob.R_MOD
NEW_SYMBOLS = ("bbg_open_all_batch_reserve", "bbg_open_all_batch_device", "bbg_open_all_batch")


def values(seed, n):
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(n)]


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("count", [1, 3, 5])
def test_batched_stages_are_independent_transforms(count, inverse):
    """One pass per stage over count 2^(log2block - 1) butterflies transforms every contiguous block on its own, in both directions, with
    n^-1 folded into the last inverse stage: blocks of 2 .. 64."""
    for log2block in range(1, 7):
        n = 1 << log2block
        natural = values(0xB47C + 100 * log2block + count, count * n)
        got = ob.batched_stages(ob.bit_reversed_blocks(natural, log2block), log2block, count, inverse)
        for p in range(count):
            assert got[p * n:(p + 1) * n] == ob.transform(natural[p * n:(p + 1) * n], inverse), (log2block, count, p)


def test_inverse_of_forward_is_the_identity_across_blocks():
    log2block, count = 4, 3
    natural = values(0xB47C + 7, count << log2block)
    there = ob.batched_stages(ob.bit_reversed_blocks(natural, log2block), log2block, count)
    assert ob.batched_stages(ob.bit_reversed_blocks(there, log2block), log2block, count, True) == natural


@pytest.mark.parametrize("log2b", [2, 3, 6])
def test_lds_transform_is_the_transform(log2b):
    v = values(0xB47C + 20 + log2b, 1 << log2b)
    assert ob.lds_transform(v) == ob.transform(v)


@pytest.mark.parametrize("lg,lc", [(2, 1), (3, 1), (3, 2), (4, 2), (6, 3), (7, 6), (3, 0), (6, 0)])
def test_product_destination_is_the_single_layout_within_the_polynomial(lg, lc):
    """Product (p, b, i) lands at p 2n + bitrev_2r(i) l + bitrev_l(b): open_cells_model's layout, shifted to polynomial p's array; every
    destination is hit once."""
    l, r2 = 1 << lc, 1 << (lg - lc + 1)
    seen = set()
    for p in range(3):
        for b in range(l):
            for i in range(r2):
                d = ob.product_destination(p, b, i, lg, lc)
                assert d == (p << (lg + 1)) + oc.bit_reverse(i, lg - lc + 1) * l + oc.bit_reverse(b, lc)
                seen.add(d)
    assert seen == set(range(3 << (lg + 1)))


def test_fold_reads_the_first_half_of_each_polynomial():
    for log2p in (1, 3, 5):
        n = 1 << log2p
        for p in range(3):
            src = [ob.fold_source(p, i, log2p) for i in range(n)]
            assert src == [2 * n * p + oc.bit_reverse(i, log2p) for i in range(n)]
            assert all(2 * n * p <= s < 2 * n * p + n for s in src)


def test_chunk_walk_visits_every_polynomial_once_and_in_order():
    for count in range(1, 10):
        for cap in range(1, 5):
            chunks = ob.chunk_walk(count, cap)
            assert [p for first, c in chunks for p in range(first, first + c)] == list(range(count))
            assert all(1 <= c <= cap for _, c in chunks) and all(c == cap for _, c in chunks[:-1])


def test_cap_keeps_the_workspace_within_the_budget():
    for lg, lc in ((12, 6), (16, 6), (12, 0), (20, 6), (27, 0)):
        cap = ob.batch_cap(lg, lc)
        assert cap >= 1 and (cap == 1 or cap * ob.poly_bytes(lg, lc) <= ob.BUDGET < (cap + 1) * ob.poly_bytes(lg, lc))
    assert ob.handle_bytes(6, 0) == 576 * 64 and ob.poly_bytes(6, 0) == 448 * 64
    assert ob.batch_cap(27, 0) == 1
    src = open(os.path.join(ROOT, "aztec-2.0_amd", "csrc", "open_all.hip")).read()
    assert re.search(r"OPEN_BATCH_BUDGET = \(size_t\)1 << 30;", src) and re.search(r"OPEN_BATCH_LDS_LOG2 = %d;" % ob.LDS_LOG2, src)
    assert (1 << ob.LDS_LOG2) * 32 <= 160 * 1024 < (2 << ob.LDS_LOG2) * 32  # the largest power of two whose 32 B elements fit a CU's LDS


def test_new_symbols_are_declared_exported_and_bound(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bbg.h")).read(), flags=re.S)
    lib = pkg.load_library()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint %s\s*\(struct bbg_open_all\* h," % sym, text), f"{sym} is not declared in include/bbg.h"
        assert hasattr(lib, sym), f"{sym} is not exported by libbbg.so"
        assert sym in pkg.binding.EXPORTED_SYMBOLS
        assert getattr(lib, sym).restype is ctypes.c_int
    for method in ("reserve_batch", "open_batch", "open_batch_device"):
        assert callable(getattr(pkg.binding.OpenAll, method))
