#!/usr/bin/env python3
"""Timings of the fixed-base multiplication and the powers-of-x SRS (csrc/fixed_base.hip) -- the table in profiles/fixed_base.txt.

Per size (default 2^12, 2^16, 2^20), one warm-up call and then the median of 5:
  * bbg_g1_fixed_base_mul_device on device-resident scalars: the whole call (host clock, ends in a stream synchronisation) and the
    "fixed_base_mul" kernel time from bbg_profile_get (HIP events on the stream);
  * "fixed_base_table": the table build, forced by alternating between two base points;
  * bbg_srs_synth_powers(x, n) and bbg_srs_synth_hashed(seed, n), whole calls in the same process (both end in the same window-table build).
Then the host time of oracle.srs_powers(x, 2^16) on this machine's cores, and the library's sha256.

--one LOG2N: a single bbg_g1_fixed_base_mul_device call of 2^LOG2N scalars after a warm-up of 64 (for a counter run under rocprofv3 --pmc)."""
import hashlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import __graft_entry__ as ge  # noqa: E402
import coarse_inputs as ci  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402

REPS = 5
X_INT = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % ci.R_MOD
SEED = 0xBB254


def wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def main():
    pkg = ge.load_package()
    oracle = Oracle()
    bbg = pkg.Bbg(0)
    x_mont = ci.to_words([ci.to_mont(X_INT, 0)])[0]
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        n = 1 << int(sys.argv[2])
        d_s, d_o = bbg.dev_alloc(n * 32), bbg.dev_alloc(n * 64)
        bbg.dev_upload(d_s, ci.coarse_scalars(SEED, n, 0))
        bbg.g1_fixed_base_mul_device(d_s, 64, d_o)
        bbg.sync()
        bbg.g1_fixed_base_mul_device(d_s, n, d_o)
        bbg.sync()
        print(f"one bbg_g1_fixed_base_mul_device call, n = {n}")
        bbg.close()
        return
    sizes = [int(a) for a in sys.argv[1:]] or [12, 16, 20]
    with open(pkg.LIB_PATH, "rb") as f:
        print(f"# build: libbbg.so sha256 {hashlib.sha256(f.read()).hexdigest()}  (one MI355X)")
    print(f"# one warm-up call, then {REPS} calls; wall = the whole call on a host clock (ends in a stream synchronisation); mul_kernel / table =")
    print('# bbg_profile_get("fixed_base_mul" / "fixed_base_table") per launch (HIP events on the stream); scalars spread over [0, 2r)')
    G = oracle.g1_generator()
    B = oracle.canon(1, oracle.g1_mul(G, ci.to_words([ci.to_mont(0xFEDCBA987654321, 0)])[0]).reshape(-1, 4)).reshape(8)
    print("log2n  mul_device_wall_ms  mul_kernel_ms  table_ms  Mscalar/s(kernel)  synth_powers_wall_s  synth_hashed_wall_s  powers/hashed")
    for lg in sizes:
        n = 1 << lg
        d_s, d_o = bbg.dev_alloc(n * 32), bbg.dev_alloc(n * 64)
        bbg.dev_upload(d_s, ci.coarse_scalars(SEED + lg, n, 0))

        def mul(base=None):
            bbg.g1_fixed_base_mul_device(d_s, n, d_o, base)
            bbg.sync()

        mul()
        bbg.profile_enable(True)
        walls = [wall(mul)[0] for _ in range(REPS)]
        bbg.sync()
        k_ms, k_cnt = bbg.profile_get("fixed_base_mul")
        for r in range(REPS):  # every call here changes the base: REPS table builds
            mul(B if r % 2 == 0 else None)
        mul(None)
        t_ms, t_cnt = bbg.profile_get("fixed_base_table")
        bbg.profile_enable(False)
        bbg.dev_free(d_s)
        bbg.dev_free(d_o)
        assert k_cnt == REPS and t_cnt >= REPS, (k_cnt, t_cnt)

        def powers():
            bbg.srs_synth_powers(x_mont, n).free()

        def hashed():
            bbg.srs_synth_hashed(SEED, n).free()

        powers()
        hashed()
        pw, hs = [], []
        for _ in range(REPS):  # alternating
            t0 = time.perf_counter()
            s = bbg.srs_synth_powers(x_mont, n)
            pw.append(time.perf_counter() - t0)
            s.free()
            t0 = time.perf_counter()
            s = bbg.srs_synth_hashed(SEED, n)
            hs.append(time.perf_counter() - t0)
            s.free()
        mp, mh = statistics.median(pw), statistics.median(hs)
        print(f"{lg:5d}  {1e3 * statistics.median(walls):18.3f}  {k_ms / k_cnt:13.3f}  {t_ms / t_cnt:8.3f}  {n / (k_ms / k_cnt) / 1e3:17.1f}  "
              f"{mp:19.4f}  {mh:19.4f}  {mp / mh:13.2f}", flush=True)
        print(f"#      powers wall_s of the {REPS} calls: {' '.join(f'{v:.4f}' for v in pw)}   hashed: {' '.join(f'{v:.4f}' for v in hs)}", flush=True)
    dt, _ = wall(lambda: oracle.srs_powers(x_mont, 1 << 16))
    print(f"# oracle.srs_powers(x, 2^16) on this host ({oracle.num_threads()} oracle threads): {dt:.2f} s", flush=True)
    bbg.close()


if __name__ == "__main__":
    main()
