"""The host-array entry points of the C ABI against their *_device twins, bit for bit.

A host-array entry point stages its arrays through ONE device buffer of the context (csrc/bbg_capi.hip on csrc/region_layout.h): it lays the
buffer out in regions, uploads, runs the module's device call on the regions, downloads and waits.  Its twin takes device pointers and
does the arithmetic alone, so the two must agree in every word whatever the inputs are; a wrong region offset, a region too small, a
missing upload or download shows as a difference.  (The two MSMs over an SRS are compared in canonical affine form, every word of it:
their Jacobian coordinates differ between two runs of the same call, see affine().)  The twins themselves are pinned against the oracle
and the models elsewhere (tests/test_gpu_parity.py, test_gpu_open_all.py, test_gpu_cells.py, test_gpu_cells_verify.py, test_gpu_msm_points.py, test_gpu_pairing.py,
test_gpu_var_base.py, test_gpu_fixed_base.py, test_gpu_barycentric.py, test_gpu_g1_helpers.py).

  * the smallest shapes at which an offset can go wrong: element counts 1, 3 and 65, transforms of 2^1 and 2^5, cells at (4, 1) with one
    and two polynomials, a batch of MSMs of 0, 1 and 65 terms, 1 and 3 products of 2 pairs, both one_scalar forms, every n = 0 the ABI takes
  * large, small, large behind bbg_memory_trim: the staging buffer is allocated, reused while larger than needed, and grown
  * one invalid call per entry point with its return code and the exact text of bbg_last_error()

The five entry points without a twin are held to the oracle by tests/test_gpu_g1_helpers.py::test_g1_normalize_mixed_entries
(bbg_g1_normalize), tests/test_gpu_parity.py::test_field_ops (bbg_field_op), tests/test_gpu_limb29.py::test_device_primitive_against_its_model
(bbg_limb29_op), tests/test_gpu_tower.py::test_device_function_against_the_model (bbg_tower_op, against the integer models) and
tests/test_gpu_coarse_range.py::test_coset_fft_split_and_extend_coarse (bbg_coset_fft_extend); here they run through the
large, small, large sequence against themselves (the same input gives the same output whatever the buffer held before) and the table."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x57A6ED
P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47  # BN254 Fq
N_POINTS = 1 << 12
INVALID = -1


class World:
    pass


@pytest.fixture(scope="module")
def world(pkg, bbg, oracle):
    """Points, scalars and handles shared by every case; nothing here is an expectation."""
    w = World()
    w.pkg, w.bbg, w.oracle = pkg, bbg, oracle
    w.srs = bbg.srs_synth_hashed(SEED, N_POINTS)
    w.pts = w.srs.read()
    one = np.array([(pow(2, 256, P) >> (64 * k)) & (2**64 - 1) for k in range(4)], dtype=np.uint64)  # Montgomery form of 1
    w.jac = np.concatenate([w.pts, np.tile(one, (N_POINTS, 1))], axis=1)
    w.handles = {}
    w.lines = bbg.g2_lines_prepare(bbg.g2_mul(pkg.synthetic_scalars(SEED + 1, 2)))
    yield w
    bbg.sync()
    for h in w.handles.values():
        h.free()
    w.lines.free()
    w.srs.free()


def scalars(w, tag, n):
    return w.pkg.synthetic_scalars(SEED + 100 + tag, n)


def handle(w, lg, lc):
    if (lg, lc) not in w.handles:
        w.handles[(lg, lc)] = w.bbg.open_all_prepare(w.srs, lg, lc)
    return w.handles[(lg, lc)]


class Device:
    """Device arrays of one twin call, freed on the way out."""

    def __init__(self, bbg):
        self.bbg, self.ptrs = bbg, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.bbg.sync()
        for p in self.ptrs:
            self.bbg.dev_free(p)

    def alloc(self, nbytes):
        self.ptrs.append(self.bbg.dev_alloc(max(nbytes, 1)))
        return self.ptrs[-1]

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        if a.nbytes:
            self.bbg.dev_upload(p, a)
        return p

    def down(self, p, shape, dtype=np.uint64):
        return self.bbg.dev_download(p, shape, dtype)


# ---- one function per entry point: shape -> (what the host form returns, what the twin computes), as tuples of arrays
def g1_ntt(w, lg):
    n, inverse = 1 << lg, bool(lg & 1)
    with Device(w.bbg) as d:
        d_out = d.alloc(n * 64)
        w.bbg.g1_ntt_device(d.up(w.pts[:n]), lg, d_out, inverse)
        return (w.bbg.g1_ntt(w.pts[:n], inverse),), (d.down(d_out, (n, 8)),)


def open_all(w, shape):
    lg, lc = shape
    h, c = handle(w, lg, lc), scalars(w, 1, 1 << lg)
    with Device(w.bbg) as d:
        d_out = d.alloc(h.count * 64)
        h.open_device(d.up(c), d_out)
        return (h.open(c),), (d.down(d_out, (h.count, 8)),)


def open_all_batch(w, shape):
    lg, lc, polys = shape
    h, c = handle(w, lg, lc), scalars(w, 2, polys << lg).reshape(polys, 1 << lg, 4)
    with Device(w.bbg) as d:
        d_out = d.alloc(polys * h.count * 64)
        h.open_batch_device(d.up(c), polys, d_out)
        return (h.open_batch(c),), (d.down(d_out, (polys, h.count, 8)),)


def cells_values(w, shape):
    lg, lc, polys = shape
    c = scalars(w, 3, polys << lg)
    with Device(w.bbg) as d:
        d_out = d.alloc(c.nbytes)
        w.bbg.cells_values_device(d.up(c), lg, lc, polys, d_out)
        return (w.bbg.cells_values(c, lg, lc),), (d.down(d_out, c.shape),)


def cells_recover(w, shape):
    lg, lc, polys = shape
    r = 1 << (lg - lc)
    ids = [(3 * k + 1) % r for k in range(r // 2 + 1)]  # K = r / 2 + 1 cells, not in ascending order
    v = scalars(w, 4, polys * len(ids) << lc)
    with Device(w.bbg) as d:
        d_out = d.alloc(polys * 32 << lg)
        w.bbg.cells_recover_device(ids, d.up(v), lg, lc, polys, d_out)
        return (w.bbg.cells_recover(ids, v, lg, lc),), (d.down(d_out, (polys << lg, 4)),)


def cells_verify_reduce(w, shape):
    lg, lc, ncom, K = shape
    r = 1 << (lg - lc)
    cids, mids = [(5 * k + 2) % ncom for k in range(K)], [(7 * k + 3) % r for k in range(K)]
    com, proofs, values, rho = w.pts[100:100 + ncom], w.pts[200:200 + K], scalars(w, 5, K << lc), scalars(w, 6, 1)[0]
    with Device(w.bbg) as d:
        d_out, d_bad = d.alloc(128), d.alloc(4)
        w.bbg.cells_verify_reduce_device(w.srs, lg, lc, d.up(com), ncom, cids, mids, d.up(values), d.up(proofs), rho, d_out, d_bad)
        got = d.down(d_out, (2, 8))
        assert int(d.down(d_bad, (1,), np.uint32)[0]) == 0
        return (w.bbg.cells_verify_reduce(w.srs, lg, lc, com, cids, mids, values, proofs, rho),), (got,)


def affine(w, jacs):
    """The canonical affine form of MSM results.  An MSM's Jacobian coordinates are one representative of its point: which one depends on
    the order the partition sort's atomics happen to leave the bucket entries in, so two runs of the SAME call differ in them."""
    return np.stack([w.oracle.jac_to_affine(j) for j in np.asarray(jacs).reshape(-1, 12)])


def msm(w, n):
    k = scalars(w, 7, n)
    with Device(w.bbg) as d:
        d_out = d.alloc(96)
        w.bbg.msm_device(w.srs, d.up(k), n, d_out, start=3)
        w.bbg.join()
        return (affine(w, w.bbg.msm(w.srs, k, start=3)),), (affine(w, d.down(d_out, (12,))),)


def msm_batch(w, lens):
    ks = [scalars(w, 8 + j, n) for j, n in enumerate(lens)]
    starts = list(range(len(lens)))
    with Device(w.bbg) as d:
        d_out = d.alloc(96 * len(lens))
        w.bbg.msm_batch_device(w.srs, [d.up(k) for k in ks], lens, d_out, starts)
        w.bbg.join()
        return (affine(w, w.bbg.msm_batch(w.srs, ks, starts)),), (affine(w, d.down(d_out, (len(lens), 12))),)


def g1_msm(w, n):
    k = scalars(w, 20, n)
    with Device(w.bbg) as d:
        d_out = d.alloc(64)
        w.bbg.g1_msm_device(d.up(w.pts[:n]), d.up(k), n, d_out)
        return (w.bbg.g1_msm(w.pts[:n], k),), (d.down(d_out, (8,)),)


def g1_sum(w, n):
    with Device(w.bbg) as d:
        d_out = d.alloc(96)
        w.bbg.g1_sum_device(d.up(w.jac[:n]), n, d_out)
        return (w.bbg.g1_sum(w.jac[:n]),), (d.down(d_out, (12,)),)


def g1_fixed_base_mul(w, n):
    k, base = scalars(w, 21, n), (w.pts[9] if n & 1 else None)
    with Device(w.bbg) as d:
        d_out = d.alloc(n * 64)
        w.bbg.g1_fixed_base_mul_device(d.up(k), n, d_out, base)
        return (w.bbg.g1_fixed_base_mul(k, base),), (d.down(d_out, (n, 8)),)


def g1_batch_mul(w, shape):
    n, one_scalar = shape
    k = scalars(w, 22, 1 if one_scalar else n)
    with Device(w.bbg) as d:
        d_out = d.alloc(n * 64)
        w.bbg.g1_batch_mul_device(d.up(w.pts[:n]), d.up(k), n, d_out, one_scalar)
        return (w.bbg.g1_batch_mul(w.pts[:n], k, one_scalar),), (d.down(d_out, (n, 8)),)


def pairing_product(w, count):
    g1 = w.pts[300:300 + 2 * count].copy()
    with Device(w.bbg) as d:
        d_out, d_status = d.alloc(count * 384), d.alloc(count * 4)
        w.bbg.pairing_product_device(w.lines, d.up(g1), count, d_out, d_status)
        return w.bbg.pairing_product(w.lines, g1), (d.down(d_out, (count, 48)), d.down(d_status, (count,), np.uint32))


def ntt(w, lg):
    a, op = scalars(w, 23, 1 << lg), (w.pkg.binding.COSET_FFT if lg & 1 else w.pkg.binding.FFT)
    with Device(w.bbg) as d:
        d_a = d.up(a)
        w.bbg.ntt_device(d_a, lg, op)
        return (w.bbg.ntt(a, op),), (d.down(d_a, a.shape),)


def coset_fft_split(w, shape):
    lg, ext = shape
    a = scalars(w, 24, 1 << lg)
    buf = np.zeros((ext << lg, 4), dtype=np.uint64)
    buf[:1 << lg] = a
    with Device(w.bbg) as d:
        d_a = d.up(buf)
        w.bbg._ck(w.bbg.lib.bbg_coset_fft_split_device(w.bbg.ctx, ctypes.c_void_p(d_a), lg, ext))
        return (w.bbg.coset_fft_split(a, ext),), (d.down(d_a, buf.shape),)


def poly_evaluate(w, n):
    a, z = scalars(w, 25, n), scalars(w, 26, 1)[0]
    with Device(w.bbg) as d:
        return (w.bbg.poly_evaluate(a, z),), (w.bbg.poly_evaluate_device(d.up(a), n, z),)


def kate_opening(w, n):
    a, z = scalars(w, 27, n), scalars(w, 28, 1)[0]
    with Device(w.bbg) as d:
        d_dest = d.alloc(n * 32)
        f = w.bbg.kate_opening_device(d.up(a), d_dest, n, z)
        return w.bbg.kate_opening(a, z), (d.down(d_dest, (n, 4)), f)


def poly_evaluate_lagrange(w, lg):
    a, z = scalars(w, 29, 1 << lg), scalars(w, 30, 1)[0]
    with Device(w.bbg) as d:
        return (w.bbg.poly_evaluate_lagrange(a, z),), (w.bbg.poly_evaluate_lagrange_device([d.up(a)], lg, z)[0],)


def divide_by_pseudo_vanishing(w, shape):
    lg_src, lg_target = shape
    a = scalars(w, 31, 1 << lg_target)
    with Device(w.bbg) as d:
        d_a = d.up(a)
        w.bbg.divide_by_pseudo_vanishing_device(d_a, lg_src, lg_target, 1)
        return (w.bbg.divide_by_pseudo_vanishing(a, lg_src, 1),), (d.down(d_a, a.shape),)


# entry point -> (the pair above, the smallest shapes, large / small / large)
TWINS = {
    "bbg_g1_ntt": (g1_ntt, [1, 5], [10, 1, 11]),
    "bbg_open_all": (open_all, [(1, 0), (5, 0), (4, 1)], [(9, 0), (1, 0), (10, 0)]),
    "bbg_open_all_batch": (open_all_batch, [(4, 1, 1), (4, 1, 2), (1, 0, 3), (5, 0, 2)], [(9, 0, 2), (1, 0, 1), (9, 0, 5)]),
    "bbg_cells_values": (cells_values, [(4, 1, 1), (4, 1, 2)], [(10, 3, 2), (4, 1, 1), (11, 3, 3)]),
    "bbg_cells_recover": (cells_recover, [(4, 1, 1), (4, 1, 2)], [(10, 3, 2), (4, 1, 1), (11, 3, 3)]),
    "bbg_cells_verify_reduce": (cells_verify_reduce, [(4, 1, 1, 1), (4, 1, 2, 3), (4, 1, 3, 65)], [(10, 3, 40, 500), (4, 1, 1, 1), (10, 3, 90, 1200)]),
    "bbg_msm": (msm, [1, 3, 65, 0], [3000, 1, 4000]),
    "bbg_msm_batch": (msm_batch, [[0, 1, 65], [3], [65, 0]], [[1500, 1000], [1, 0, 65], [2000, 1500, 500]]),
    "bbg_g1_msm": (g1_msm, [1, 3, 65, 0], [3000, 1, 4000]),
    "bbg_g1_sum": (g1_sum, [1, 3, 65, 0], [3000, 1, 4000]),
    "bbg_g1_fixed_base_mul": (g1_fixed_base_mul, [1, 3, 65], [3000, 1, 4000]),
    "bbg_g1_batch_mul": (g1_batch_mul, [(1, False), (3, False), (65, False), (1, True), (3, True), (65, True)], [(3000, False), (1, True), (4000, True)]),
    "bbg_pairing_product": (pairing_product, [1, 3], [40, 1, 70]),
    "bbg_ntt": (ntt, [1, 5], [10, 1, 11]),
    "bbg_coset_fft_split": (coset_fft_split, [(1, 4), (5, 4), (5, 1)], [(10, 4), (1, 2), (11, 4)]),
    "bbg_poly_evaluate": (poly_evaluate, [1, 3, 65, 0], [3000, 1, 4000]),
    "bbg_kate_opening": (kate_opening, [1, 3, 65], [3000, 1, 4000]),
    "bbg_poly_evaluate_lagrange": (poly_evaluate_lagrange, [1, 5], [10, 1, 11]),
    "bbg_divide_by_pseudo_vanishing": (divide_by_pseudo_vanishing, [(1, 1), (3, 5)], [(8, 10), (1, 1), (9, 11)]),
}


def agree(name, shape, host, twin):
    assert len(host) == len(twin)
    for k, (h, t) in enumerate(zip(host, twin)):
        h, t = np.asarray(h), np.asarray(t)
        assert h.shape == t.shape and h.dtype == t.dtype, f"{name} {shape}: output {k} is {h.dtype}{h.shape}, the twin's {t.dtype}{t.shape}"
        assert np.array_equal(h, t), f"{name} {shape}: output {k} differs from the _device twin's in {int((h != t).sum())} of {h.size} words"


@pytest.mark.parametrize("name", list(TWINS))
def test_host_form_equals_device_twin_on_the_smallest_shapes(world, name):
    pair, shapes, _ = TWINS[name]
    for shape in shapes:
        agree(name, shape, *pair(world, shape))


@pytest.mark.parametrize("name", list(TWINS))
def test_host_form_equals_device_twin_large_small_large(world, name):
    """bbg_memory_trim releases the staging buffer: the first call allocates it, the second runs in a buffer far larger than it needs, the
    third makes it grow."""
    pair, _, shapes = TWINS[name]
    world.bbg.memory_trim()
    for shape in shapes:
        agree(name, shape, *pair(world, shape))


# ---- the entry points without a twin: the same input gives the same output whatever the staging buffer held and however large it was
def g1_normalize(w, n):
    return w.bbg.g1_normalize(w.jac[:n])


def field_op(w, n):
    return np.stack([w.bbg.field_op(1, 0, scalars(w, 40, n), scalars(w, 41, n)), w.bbg.field_op(0, 4, scalars(w, 40, n))])


def limb29_op(w, n):
    operands, results = w.bbg.limb29_op_shape(0, 6)  # f29_add: two rows in, one out
    assert (operands, results) == (2, 1)
    rows = (w.pkg.splitmix64_limbs(SEED + 50, n * operands * 9) & np.uint64((1 << 29) - 1)).astype(np.uint32).reshape(n, operands, 9)
    return w.bbg.limb29_op(0, 6, rows)


def tower_op(w, n):
    operands, results = w.bbg.tower_op_shape(0)  # f2_add: four rows in, two out
    assert (operands, results) == (4, 2)
    rows = (w.pkg.splitmix64_limbs(SEED + 51, n * operands * 8) & np.uint64((1 << 28) - 1)).astype(np.uint32).reshape(n, operands, 8)
    return w.bbg.tower_op(0, rows)


def coset_fft_extend(w, shape):
    lg, dom = shape
    return w.bbg.coset_fft_extend(scalars(w, 42, 1 << lg), dom)


NO_TWIN = {
    "bbg_g1_normalize": (g1_normalize, [3000, 1, 4000]),
    "bbg_field_op": (field_op, [3000, 1, 4000]),
    "bbg_limb29_op": (limb29_op, [3000, 1, 4000]),
    "bbg_tower_op": (tower_op, [3000, 1, 4000]),
    "bbg_coset_fft_extend": (coset_fft_extend, [(8, 10), (1, 2), (9, 11)]),
}


@pytest.mark.parametrize("name", list(NO_TWIN))
def test_entry_without_twin_large_small_large(world, name):
    call, shapes = NO_TWIN[name]
    world.bbg.memory_trim()
    first = [call(world, s) for s in shapes]               # allocate, reuse, grow
    again = [call(world, s) for s in reversed(shapes)]     # every shape once more, in a buffer that held something else
    for s, a, b in zip(shapes, first, reversed(again)):
        assert np.array_equal(a, b), f"{name} {s}: the result depends on the staging buffer's history"
    if name == "bbg_coset_fft_extend":
        for s, a in zip(shapes, first):
            assert np.array_equal(a[-4:], a[:4]), f"{name} {s}: the four wrapped values"


# ---- n = 0
def test_zero_length_forms(world):
    w, bbg, lib = world, world.bbg, world.bbg.lib
    inf = bbg.g1_msm(np.zeros((0, 8), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64))
    for name in ("bbg_msm", "bbg_g1_msm", "bbg_g1_sum", "bbg_poly_evaluate"):   # run with zero terms, and agree with the twin (the table above)
        assert 0 in TWINS[name][1]
    assert np.array_equal(bbg.g1_normalize(bbg.msm(w.srs, np.zeros((0, 4), dtype=np.uint64)).reshape(1, 12))[0], inf), "an empty MSM is the point at infinity"
    assert np.array_equal(bbg.g1_normalize(bbg.g1_sum(np.zeros((0, 12), dtype=np.uint64)).reshape(1, 12))[0], inf), "an empty sum is the point at infinity"
    assert not bbg.poly_evaluate(np.zeros((0, 4), dtype=np.uint64), scalars(w, 60, 1)[0]).any(), "the empty polynomial evaluates to zero"
    # NULL arrays are legal with n = 0, and nothing is written
    out = np.full(12, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    keep = out.copy()
    assert lib.bbg_g1_normalize(bbg.ctx, None, 0, None) == 0
    assert lib.bbg_g1_batch_mul(bbg.ctx, None, None, 0, 0, None) == 0 and lib.bbg_g1_batch_mul(bbg.ctx, None, None, 0, 1, None) == 0
    assert lib.bbg_g1_fixed_base_mul(bbg.ctx, None, None, 0, None) == 0
    a = scalars(w, 61, 1)
    assert lib.bbg_field_op(bbg.ctx, 0, 0, a.ctypes.data, None, out.ctypes.data, 0) == 0
    assert lib.bbg_limb29_op(bbg.ctx, 0, 0, None, 0, None) == 0
    assert lib.bbg_tower_op(bbg.ctx, 0, None, 0, None) == 0
    assert np.array_equal(out, keep)
    assert lib.bbg_msm(bbg.ctx, w.srs.handle, None, 0, 0, out.ctypes.data) == 0 and lib.bbg_g1_sum(bbg.ctx, None, 0, out.ctypes.data) == 0
    assert lib.bbg_g1_msm(bbg.ctx, None, None, 0, 0, out.ctypes.data) == 0 and np.array_equal(out[:8], inf)
    # the base of a fixed-base call is validated for n = 0 as well
    off = w.pts[9].copy()
    off[0] ^= np.uint64(1)
    assert lib.bbg_g1_fixed_base_mul(bbg.ctx, w.pts[9].ctypes.data, None, 0, None) == 0
    assert lib.bbg_g1_fixed_base_mul(bbg.ctx, off.ctypes.data, None, 0, None) == INVALID


# ---- one invalid call per entry point: the return code and the exact text
def test_invalid_calls_keep_their_code_and_text(world, pkg):
    w, bbg, lib, ctx = world, world.bbg, world.bbg.lib, world.bbg.ctx
    buf = np.zeros((64, 12), dtype=np.uint64)
    p = buf.ctypes.data
    ids = np.zeros(4, dtype=np.uint32)
    ptrs = (ctypes.c_void_p * 8)()
    ns = (ctypes.c_size_t * 8)(*([1] * 8))
    h41 = handle(w, 4, 1).handle
    short = bbg.srs_synth_hashed(SEED + 2, 3)  # fewer than 2^2 points
    out_h = ctypes.c_void_p()
    srs = w.srs.handle
    rows = [
        (lambda: lib.bbg_g1_ntt(ctx, p, 0, 0, p), "bbg_g1_ntt: log2n must be 1 .. 28"),
        (lambda: lib.bbg_g1_ntt(ctx, None, 4, 0, p), "bbg_g1_ntt: null argument"),
        (lambda: lib.bbg_open_all(h41, None, p), "bbg_open_all: null argument"),
        (lambda: lib.bbg_open_all_batch(h41, p, 0, p), "bbg_open_all_batch: count must be at least 1"),
        (lambda: lib.bbg_open_all_batch(h41, p, 1 << 37, p), "bbg_open_all_batch: count x 2^log2n is out of range"),
        (lambda: lib.bbg_cells_values(ctx, p, 4, 4, 1, p), "bbg_cells_values: log2cell must be 0 .. log2n - 1"),
        (lambda: lib.bbg_cells_values(ctx, p, 29, 1, 1, p), "bbg_cells_values: log2n must be 1 .. 28"),
        (lambda: lib.bbg_cells_recover(ctx, ids.ctypes.data, 2, p, 4, 1, 1, p), "bbg_cells_recover: a cell id appears twice"),
        (lambda: lib.bbg_cells_recover(ctx, ids.ctypes.data, 1, p, 4, 1, 33, p), "bbg_cells_recover: count must be 1 .. 32"),
        (lambda: lib.bbg_cells_verify_reduce(ctx, srs, 4, 1, p, 0, ids.ctypes.data, ids.ctypes.data, 1, p, p, p, p), "bbg_cells_verify_reduce: ncom must be 1 .. 2^30"),
        (lambda: lib.bbg_cells_verify_reduce(ctx, srs, 0, 0, p, 1, ids.ctypes.data, ids.ctypes.data, 1, p, p, p, p), "bbg_cells_verify_reduce: log2n must be 1 .. 28"),
        (lambda: lib.bbg_cells_verify_reduce(ctx, short.handle, 4, 2, p, 1, ids.ctypes.data, ids.ctypes.data, 1, p, p, p, p),
         "bbg_cells_verify_reduce: the SRS holds fewer than 2^log2cell points"),
        (lambda: lib.bbg_msm(ctx, srs, None, 0, 4, p), "bbg_msm: null argument"),
        (lambda: lib.bbg_msm_batch(ctx, srs, 9, ptrs, None, ns, p), "bbg_msm_batch: 1 .. BBG_MSM_BATCH_MAX MSMs per batch"),
        (lambda: lib.bbg_msm_batch(ctx, srs, 2, ptrs, None, ns, p), "bbg_msm_batch: null scalars"),
        (lambda: lib.bbg_g1_msm(ctx, p, p, 4, 17, p), "bbg_g1_msm_plan: window_bits must be 0 or 2 .. 16 and n at most 2^28"),
        (lambda: lib.bbg_g1_msm(ctx, p, None, 4, 0, p), "bbg_g1_msm: null argument"),
        (lambda: lib.bbg_g1_sum(ctx, None, 4, p), "bbg_g1_sum: null argument"),
        (lambda: lib.bbg_g1_normalize(ctx, p, 4, None), "bbg_g1_normalize: null argument"),
        (lambda: lib.bbg_g1_fixed_base_mul(ctx, None, None, 4, p), "bbg_g1_fixed_base_mul: null argument"),
        (lambda: lib.bbg_g1_batch_mul(ctx, p, None, 4, 0, p), "bbg_g1_batch_mul: null argument"),
        (lambda: lib.bbg_pairing_product(ctx, w.lines.handle, p, 0, p, p), "bbg_pairing_product: count must be 1 .. 2^24"),
        (lambda: lib.bbg_pairing_product(ctx, w.lines.handle, p, 1, None, None), "bbg_pairing_product: both outputs are null"),
        (lambda: lib.bbg_ntt(ctx, p, 29, 0, 0, None), "bbg_ntt: log2n > 28 exceeds the 2-adicity of BN254 Fr (fr.hpp:27-30)"),
        (lambda: lib.bbg_ntt(ctx, None, 4, 0, 0, None), "bbg_ntt: null coeffs"),
        (lambda: lib.bbg_coset_fft_extend(ctx, p, 3, 1, p), "bbg_coset_fft_extend: need log2n <= log2_domain and 2 <= log2_domain <= 28"),
        (lambda: lib.bbg_coset_fft_split(ctx, p, 4, 0), "bbg_coset_fft_split: bad size"),
        (lambda: lib.bbg_coset_fft_split(ctx, p, 2, 3), "bbg_coset_fft_split: ext must be a power of two with n*ext <= 2^28"),
        (lambda: lib.bbg_poly_evaluate(ctx, None, 4, p, p), "bbg_poly_evaluate: null argument"),
        (lambda: lib.bbg_kate_opening(ctx, p, None, 4, p, p), "bbg_kate_opening: null argument"),
        (lambda: lib.bbg_kate_opening(ctx, None, None, 0, p, p), "bbg_kate_opening: bad argument"),
        (lambda: lib.bbg_poly_evaluate_lagrange(ctx, p, 0, p, p), "bbg_poly_evaluate_lagrange: bad argument (1 <= log2n <= 28)"),
        (lambda: lib.bbg_divide_by_pseudo_vanishing(ctx, p, 2, 29, 4), "bbg_divide_by_pseudo_vanishing: log2_target > 28"),
        (lambda: lib.bbg_divide_by_pseudo_vanishing(ctx, p, 5, 4, 4), "bbg_divide_by_pseudo_vanishing: need src <= target <= 2^28, target/src <= 16, roots_cut <= 8"),
        (lambda: lib.bbg_field_op(ctx, 0, 0, None, None, p, 4), "bbg_field_op: null argument"),
        (lambda: lib.bbg_limb29_op(ctx, 0, 0, p, (1 << 20) + 1, p), "bbg_limb29_op: n > 2^20"),
        (lambda: lib.bbg_limb29_op(ctx, 0, 0, None, 4, p), "bbg_limb29_op: null argument"),
        (lambda: lib.bbg_tower_op(ctx, 0, p, (1 << 16) + 1, p), "bbg_tower_op: n > 2^16"),
        (lambda: lib.bbg_tower_op(ctx, 0, None, 4, p), "bbg_tower_op: null argument"),
        # the argument checks the constructors and handles share
        (lambda: lib.bbg_open_all_prepare(ctx, short.handle, 2, ctypes.byref(out_h)), "bbg_open_all_prepare: the SRS holds fewer than 2^log2n points"),
        (lambda: lib.bbg_open_all_prepare_cells(ctx, short.handle, 2, 1, ctypes.byref(out_h)), "bbg_open_all_prepare_cells: the SRS holds fewer than 2^log2n points"),
        (lambda: lib.bbg_open_all_prepare(ctx, srs, 28, ctypes.byref(out_h)), "bbg_open_all_prepare: log2n must be 1 .. 27"),
        (lambda: lib.bbg_open_all_prepare_cells(ctx, srs, 0, 1, ctypes.byref(out_h)), "bbg_open_all_prepare_cells: log2n must be 1 .. 27"),
        (lambda: lib.bbg_srs_lagrange(ctx, srs, 29, ctypes.byref(out_h)), "bbg_srs_lagrange: log2n must be 1 .. 28"),
        (lambda: lib.bbg_srs_lagrange(ctx, short.handle, 2, ctypes.byref(out_h)), "bbg_srs_lagrange: the SRS holds fewer than 2^log2n points"),
        (lambda: lib.bbg_g1_ntt_device(ctx, p, 29, 0, p), "bbg_g1_ntt_device: log2n must be 1 .. 28"),
        (lambda: lib.bbg_srs_synth_powers(ctx, p, 4, ctypes.byref(out_h)), "bbg_srs_synth_powers: x = 0 (P_1 would be the point at infinity)"),
        (lambda: lib.bbg_srs_scale_powers(ctx, srs, R_WORDS.ctypes.data, ctypes.byref(out_h)), "bbg_srs_scale_powers: y = 0 (P_1 would become the point at infinity)"),
    ]
    try:
        for k, (call, text) in enumerate(rows):
            rc = call()
            assert rc == INVALID and lib.bbg_last_error().decode() == text, f"row {k}: returned {rc} with {lib.bbg_last_error().decode()!r}, expected {INVALID} with {text!r}"
        assert not out_h.value, "a refused constructor wrote its handle"
    finally:
        short.free()


R_WORDS = np.array([0x43e1f593f0000001, 0x2833e84879b97091, 0xb85045b68181585d, 0x30644e72e131a029], dtype=np.uint64)  # r: zero in [0, 2r)
