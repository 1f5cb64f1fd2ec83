#!/usr/bin/env python3
"""Timings of the table-free MSM over the caller's points (bbg_g1_msm_device, csrc/msm_points.hip) -- the table in profiles/msm_points.txt.

    python tests/tools/msm_points_time.py [OUT [log2n ...]]      (OUT defaults to profiles/msm_points.txt)

Per size (default 2^10, 2^12 .. 2^22), in ONE process on one MI355X, device-resident points of a hashed string and scalars spread over
[0, 2r); one warm-up of every variant, then REPS = 9 rounds that interleave the variants, each sample the whole call on a host clock
(it ends in a stream synchronisation):
  * msm c      bbg_g1_msm_device at the automatic width c and at its two neighbours (where the range has them), and from 2^18 also
               at c = 13, the width the cost model expects there (the neighbour 15 has a top window of 7 bits and is no fair rival);
  * (a)        bbg_g1_batch_mul_device over the same n: a lower bound of the multiply-then-sum route;
  * (b)        bbg_srs_register_device + bbg_msm_device + bbg_srs_free over the same points.
Then, for every width timed, REPS calls with the timers on: the phases "msm_points_sort" (recode + counting sort),
"msm_points_accumulate", "msm_points_reduce", "msm_points_combine" from bbg_profile_get, medians.  At 2^20 one more row: all scalars equal.
Every row gives median, minimum and maximum; `wins` under a size says whether EVERY sample of the call at the automatic width is faster
than EVERY sample of (a) and of (b)."""
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

REPS = 9
SEED = 0xBB254
MODEL_WIDTH = 13  # the width the cost model 2 n windows(c) + reduction expects at 2^20: timed from 2^18 beside the automatic one
PHASES = ("msm_points_sort", "msm_points_accumulate", "msm_points_reduce", "msm_points_combine")


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "msm_points.txt")
    sizes = [int(a) for a in sys.argv[2:]] or [10, 12, 14, 16, 18, 20, 22]
    pkg = ge.load_package()
    bbg = pkg.Bbg(0)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        with open(out_path, "w") as f:  # rewritten row by row: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")

    with open(pkg.LIB_PATH, "rb") as f:
        emit(f"# build: libbbg.so sha256 {hashlib.sha256(f.read()).hexdigest()}  (one MI355X)")
    emit(f"# tests/tools/msm_points_time.py: one process; per size one warm-up of every variant, then {REPS} rounds interleaving the variants;")
    emit("# a sample is the whole call on a host clock, ending in a stream synchronisation; ms.  points: bbg_srs_synth_hashed, device-resident;")
    emit("# scalars spread over [0, 2r).  (a) = bbg_g1_batch_mul_device, (b) = bbg_srs_register_device + bbg_msm_device + bbg_srs_free.")
    emit("# phases: bbg_profile_get medians over further calls at each width timed (HIP events on the stream).")
    emit("log2n  variant                     median       min       max")
    for lg in sizes:
        n = 1 << lg
        srs = bbg.srs_synth_hashed(SEED + lg, n)
        pts = srs.read()
        srs.free()
        d_p, d_s, d_o, d_j = bbg.dev_alloc(n * 64), bbg.dev_alloc(n * 32), bbg.dev_alloc(n * 64), bbg.dev_alloc(96)
        bbg.dev_upload(d_p, pts)
        scalars = ci.coarse_scalars(SEED + lg, n, 0)
        bbg.dev_upload(d_s, scalars)
        c_auto = bbg.g1_msm_plan(n)[0]
        widths = [c for c in (c_auto - 1, c_auto, c_auto + 1) if 2 <= c <= 16]
        if lg >= 18 and MODEL_WIDTH not in widths:
            widths.insert(0, MODEL_WIDTH)

        def registered():
            s = bbg.srs_register_device(d_p, n)
            bbg.msm_device(s, d_s, n, d_j)
            bbg.sync()
            s.free()

        variants = [(f"msm c = {c}" + (" (auto)" if c == c_auto else ""), (lambda c=c: bbg.g1_msm_device(d_p, d_s, n, d_o, c))) for c in widths]
        variants += [("(a) batch_mul", lambda: bbg.g1_batch_mul_device(d_p, d_s, n, d_o)), ("(b) register + msm + free", registered)]
        if lg == 20:
            d_e = bbg.dev_alloc(n * 32)
            bbg.dev_upload(d_e, np.tile(scalars[:1], (n, 1)))
            variants.append(("msm auto, all scalars equal", lambda: bbg.g1_msm_device(d_p, d_e, n, d_o, 0)))
        res = {name: [] for name, _ in variants}
        for _, fn in variants:  # warm-up
            fn()
            bbg.sync()
        for _ in range(REPS):
            for name, fn in variants:
                t0 = time.perf_counter()
                fn()
                bbg.sync()
                res[name].append(1e3 * (time.perf_counter() - t0))
        for name, _ in variants:
            v = res[name]
            emit(f"{lg:5d}  {name:26s} {statistics.median(v):9.3f} {min(v):9.3f} {max(v):9.3f}")
        auto = res[f"msm c = {c_auto} (auto)"]
        wins = max(auto) < min(res["(a) batch_mul"]) and max(auto) < min(res["(b) register + msm + free"])
        emit(f"{lg:5d}  wins: every sample at the automatic width below every sample of (a) and (b): {'yes' if wins else 'NO'}")
        for c in widths:
            phase = {p: [] for p in PHASES}
            for _ in range(REPS):
                bbg.profile_enable(True)
                bbg.g1_msm_device(d_p, d_s, n, d_o, c)
                bbg.sync()
                for p in PHASES:
                    phase[p].append(bbg.profile_get(p)[0])
                bbg.profile_enable(False)
            emit(f"{lg:5d}  phases at c = {c:2d}:  " + "  ".join(f"{p[11:]} {statistics.median(phase[p]):.3f}" for p in PHASES))
        for d in (d_p, d_s, d_o, d_j) + ((d_e,) if lg == 20 else ()):
            bbg.dev_free(d)
    bbg.close()


if __name__ == "__main__":
    main()
