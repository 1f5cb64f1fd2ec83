#!/usr/bin/env python3
"""Timings of the Lagrange-form entry points against the coefficient route (csrc/barycentric.hip) -- the table in profiles/barycentric.txt.

Per size (default 2^12, 2^16, 2^20), in ONE process, one warm-up call of every variant and then REPS rounds that interleave them:
  * bbg_fr_batch_invert_device: the whole call ending in a synchronisation, and the "fr_batch_invert" kernel time from bbg_profile_get;
  * bbg_poly_evaluate_lagrange_device for count = 1, 8 and 32 (half of them shifted), whole call and the "barycentric" time;
  * the route without it: count x (bbg_ntt_device(IFFT) + bbg_poly_evaluate_device);
  * bbg_kate_opening_lagrange_device, and the route without it: iFFT + bbg_kate_opening_device + FFT.
The library under test is BBG_LIB_PATH when set (A/B builds with another group shape, make EXTRA=-DBBG_BARY_E=...).  Medians and minima are printed."""
import hashlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import __graft_entry__ as ge  # noqa: E402
import barycentric_model as bm  # noqa: E402

REPS = 5
SEED = 0xBA2C
FFT, IFFT = 0, 1


def med_min(v):
    return f"{statistics.median(v):9.3f} {min(v):9.3f}"


def main():
    pkg = ge.load_package()
    bbg = pkg.Bbg(0)
    sizes = [int(a) for a in sys.argv[1:]] or [12, 16, 20]
    z = bm.mont_words(bm.Z_INTS[:1])[0]
    with open(pkg.binding.LIB_PATH, "rb") as f:
        print(f"# build: {os.path.relpath(pkg.binding.LIB_PATH, ROOT)} sha256 {hashlib.sha256(f.read()).hexdigest()}  (one MI355X)")
    print(f"# one process; per size one warm-up of every variant, then {REPS} rounds interleaving the variants; every pair of columns is")
    print("# median and minimum in ms.  wall = the whole call on a host clock (ends in a synchronisation); kernel = bbg_profile_get")
    print('# ("fr_batch_invert" / "barycentric", HIP events on the stream; 0 for the coefficient route, which has no single scope)')
    print("log2n  variant                     wall_ms(med min)     kernel_ms(med min)")
    for lg in sizes:
        n = 1 << lg
        assert bm.off_domain(bm.Z_INTS[0], lg)
        src = [bbg.dev_alloc(n * 32) for _ in range(32)]
        for k, p in enumerate(src):
            bbg.dev_upload(p, pkg.synthetic_scalars(SEED + 64 * lg + k, n))
        dest = bbg.dev_alloc(n * 32)
        res = {}

        def timed(name, prof, fn):
            bbg.profile_enable(True)
            t0 = time.perf_counter()
            fn()
            bbg.sync()
            w = time.perf_counter() - t0
            ms, _ = bbg.profile_get(prof) if prof else (0.0, 1)
            bbg.profile_enable(False)
            res.setdefault(name, ([], []))
            res[name][0].append(1e3 * w)
            res[name][1].append(ms)

        # the coefficient route transforms in place: the arrays hold other (equally arbitrary) values afterwards, the work is the same
        def coeff_eval(count):
            for k in range(count):
                bbg.ntt_device(src[k], lg, IFFT)
                bbg.poly_evaluate_device(src[k], n, z)

        def coeff_open():
            bbg.ntt_device(src[0], lg, IFFT)
            bbg.kate_opening_device(src[0], dest, n, z)
            bbg.ntt_device(dest, lg, FFT)

        variants = [("batch_invert", "fr_batch_invert", lambda: bbg.fr_batch_invert_device(src[31], dest, n))]
        for count in (1, 8, 32):
            sh = [k % 2 for k in range(count)]
            variants.append((f"evaluate_lagrange x{count}", "barycentric", lambda c=count, s=sh: bbg.poly_evaluate_lagrange_device(src[:c], lg, z, s)))
            variants.append((f"ifft + evaluate x{count}", None, lambda c=count: coeff_eval(c)))
        variants.append(("opening_lagrange", "barycentric", lambda: bbg.kate_opening_lagrange_device(src[0], dest, lg, z)))
        variants.append(("ifft + opening + fft", None, coeff_open))
        for _, _, fn in variants:  # warm-up
            fn()
        bbg.sync()
        for _ in range(REPS):
            for name, prof, fn in variants:
                timed(name, prof, fn)
        for name, _, _ in variants:
            print(f"{lg:5d}  {name:26s} {med_min(res[name][0])}   {med_min(res[name][1])}", flush=True)
        for p in src + [dest]:
            bbg.dev_free(p)
    bbg.close()


if __name__ == "__main__":
    main()
