#!/usr/bin/env python3
"""Timings of bbg_open_all (csrc/open_all.hip) -- the table in profiles/open_all.txt, which this script writes (--out PATH for another
place; the lines are printed as well).

Per size (default 2^12, 2^16, 2^20), in ONE process:
  * bbg_open_all_prepare over a hashed string: the whole call on a host clock (it ends in a synchronisation), REPS times;
  * bbg_open_all_device on device-resident coefficients: one warm-up, then REPS calls, each the whole call up to a stream synchronisation
    on a host clock, with the profile scopes of that call from bbg_profile_get (HIP events on the stream);
  * for comparison, SINGLES single openings by the existing route, bbg_kate_opening_device + bbg_msm_device at the same n, on a host
    clock; their mean times n is what all n proofs would cost that way.  That figure is EXTRAPOLATED, not measured, and labelled so.
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
SINGLES = 16
SEED = 0xBB254
SCOPES = ("open_all_coeffs", "ntt_pass", "open_all_pointwise", "ecntt_stages", "open_all_fold", "ecntt_normalize")


def med_min(v):
    return f"{statistics.median(v):10.3f} {min(v):10.3f}"


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "open_all.txt")
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    sizes = [int(a) for a in args] or [12, 16, 20]
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    pkg = ge.load_package()
    bbg = pkg.Bbg(0)
    with open(pkg.LIB_PATH, "rb") as f:
        emit(f"# build: libbbg.so sha256 {hashlib.sha256(f.read()).hexdigest()}  (one MI355X)")
    emit(f"# one process; per size {REPS} prepares, one warm-up call and {REPS} timed calls, {SINGLES} single openings; every pair of columns is median")
    emit("# and minimum in ms.  prepare / call = the whole call on a host clock, up to a synchronisation; the scopes are bbg_profile_get's (HIP")
    emit("# events on the stream) for the same calls.  points: bbg_srs_synth_hashed; coefficients spread over [0, 2r)")
    emit(f"# single = one bbg_kate_opening_device + bbg_msm_device at the same n (mean of {SINGLES}); all-by-singles = that mean times n: EXTRAPOLATED")
    emit("log2n  what                          ms(med min)")
    for lg in sizes:
        n = 1 << lg
        srs = bbg.srs_synth_hashed(SEED + lg, n)
        d_c, d_q, d_o, d_j = bbg.dev_alloc(n * 32), bbg.dev_alloc(n * 32), bbg.dev_alloc(n * 64), bbg.dev_alloc(96)
        bbg.dev_upload(d_c, ci.coarse_scalars(SEED + lg, n, 0))
        prep = []
        h = None
        for _ in range(REPS + 1):  # the first one builds the domains and grows the context's buffers: not counted
            if h is not None:
                h.free()
            bbg.sync()
            t0 = time.perf_counter()
            h = bbg.open_all_prepare(srs, lg)
            prep.append(1e3 * (time.perf_counter() - t0))
        prep = prep[1:]
        h.open_device(d_c, d_o)  # warm-up
        bbg.sync()
        wall, scopes = [], {k: [] for k in SCOPES}
        for _ in range(REPS):
            bbg.profile_enable(True)
            t0 = time.perf_counter()
            h.open_device(d_c, d_o)
            bbg.sync()
            wall.append(1e3 * (time.perf_counter() - t0))
            for k in SCOPES:
                scopes[k].append(bbg.profile_get(k)[0])
            bbg.profile_enable(False)
        emit(f"{lg:5d}  {'prepare':28s} {med_min(prep)}")
        emit(f"{lg:5d}  {'call':28s} {med_min(wall)}")
        for k in SCOPES:
            emit(f"{lg:5d}  {'  ' + k:28s} {med_min(scopes[k])}")
        emit(f"{lg:5d}  {'handle bytes':28s} {h.device_bytes():10d}")
        # the existing route, one opening at a time
        w = ci.root_of_unity(lg)
        zs = ci.to_words([ci.to_mont(pow(w, 1 + 7 * i, ci.R_MOD), 0) for i in range(SINGLES + 1)])
        single = []
        for i in range(SINGLES + 1):  # the first is the warm-up
            t0 = time.perf_counter()
            bbg.kate_opening_device(d_c, d_q, n, zs[i])
            bbg.msm_device(srs, d_q, n, d_j)
            bbg.sync()
            single.append(1e3 * (time.perf_counter() - t0))
        single = single[1:]
        mean = statistics.mean(single)
        emit(f"{lg:5d}  {'single (kate + msm)':28s} {med_min(single)}")
        emit(f"{lg:5d}  {'all-by-singles EXTRAPOLATED':28s} {mean * n:10.1f}   (= {mean:.3f} ms x {n}; open_all call is {mean * n / statistics.median(wall):.0f}x faster)")
        h.free()
        for d in (d_c, d_q, d_o, d_j):
            bbg.dev_free(d)
        srs.free()
    bbg.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
