#!/usr/bin/env python3
"""Timings of the variable-base batch multiplication, the SRS power update and the Lagrange transform's "ecntt_mul" A/B
(csrc/var_base.hip, csrc/ecntt.hip) -- the table in profiles/var_base.txt.

Per size (default 2^12, 2^16, 2^20), in ONE process, one warm-up call and then REPS rounds that interleave the variants:
  * bbg_g1_batch_mul_device on device-resident points of a hashed string and scalars spread over [0, 2r), for "batch_mul_glv" = 1 and 0:
    the whole call (host clock, ends in a stream synchronisation) and the "var_base_mul" kernel time from bbg_profile_get;
  * bbg_srs_scale_powers(srs, y), whole call (window-table build included);
  * bbg_srs_lagrange for "ecntt_mul" = 0 and 1: whole call and the "ecntt_stages" time.
Medians and minima are printed."""
import hashlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import __graft_entry__ as ge  # noqa: E402
import coarse_inputs as ci  # noqa: E402

REPS = 5
Y_INT = 0x3243F6A8885A308D313198A2E03707344A4093822299F31D0082EFA98EC4E6C8 % ci.R_MOD
SEED = 0xBB254


def med_min(v):
    return f"{statistics.median(v):9.3f} {min(v):9.3f}"


def main():
    pkg = ge.load_package()
    bbg = pkg.Bbg(0)
    sizes = [int(a) for a in sys.argv[1:]] or [12, 16, 20]
    y_mont = ci.to_words([ci.to_mont(Y_INT, 0)])[0]
    with open(pkg.LIB_PATH, "rb") as f:
        print(f"# build: libbbg.so sha256 {hashlib.sha256(f.read()).hexdigest()}  (one MI355X)")
    print(f"# one process; per size one warm-up of every variant, then {REPS} rounds interleaving the variants; every pair of columns is")
    print("# median and minimum in ms.  wall = the whole call on a host clock (ends in a synchronisation); kernel / stages = bbg_profile_get")
    print('# ("var_base_mul" / "ecntt_stages", HIP events on the stream).  points: bbg_srs_synth_hashed; scalars spread over [0, 2r)')
    print("log2n  variant                 wall_ms(med min)     kernel_ms(med min)")
    for lg in sizes:
        n = 1 << lg
        srs = bbg.srs_synth_hashed(SEED + lg, n)
        d_p, d_s, d_o = bbg.dev_alloc(n * 64), bbg.dev_alloc(n * 32), bbg.dev_alloc(n * 64)
        bbg.dev_upload(d_p, srs.read())
        bbg.dev_upload(d_s, ci.coarse_scalars(SEED + lg, n, 0))
        res = {}

        def timed(name, prof, fn):
            bbg.profile_enable(True)
            t0 = time.perf_counter()
            fn()
            bbg.sync()
            w = time.perf_counter() - t0
            ms, cnt = bbg.profile_get(prof) if prof else (0.0, 1)
            bbg.profile_enable(False)
            res.setdefault(name, ([], []))
            res[name][0].append(1e3 * w)
            res[name][1].append(ms)

        def mul(glv):
            bbg.set_option("batch_mul_glv", glv)
            bbg.g1_batch_mul_device(d_p, d_s, n, d_o)

        def scale():
            bbg.set_option("batch_mul_glv", 1)
            srs.scale_powers(y_mont).free()

        def lagrange(v):
            bbg.set_option("ecntt_mul", v)
            srs.lagrange(lg).free()

        variants = [("batch_mul glv=1", "var_base_mul", lambda: mul(1)), ("batch_mul glv=0", "var_base_mul", lambda: mul(0)),
                    ("srs_scale_powers", "var_base_mul", lambda: scale()),
                    ("lagrange ecntt_mul=0", "ecntt_stages", lambda: lagrange(0)), ("lagrange ecntt_mul=1", "ecntt_stages", lambda: lagrange(1))]
        for _, _, fn in variants:  # warm-up
            fn()
        bbg.sync()
        for _ in range(REPS):
            for name, prof, fn in variants:
                timed(name, prof, fn)
        for name, _, _ in variants:
            print(f"{lg:5d}  {name:22s} {med_min(res[name][0])}   {med_min(res[name][1])}", flush=True)
        bbg.dev_free(d_p)
        bbg.dev_free(d_s)
        bbg.dev_free(d_o)
        srs.free()
    bbg.close()


if __name__ == "__main__":
    main()
