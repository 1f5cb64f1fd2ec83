#!/usr/bin/env python3
"""Timings of the batched calls of bbg_open_all (bbg_open_all_batch_device, csrc/open_all.hip) -- the table in profiles/open_batch.txt,
which this script writes (--out PATH for another place; the lines are printed as well).

Per shape (log2n, log2cell) in (12, 6), (16, 6), (12, 0) and per count in 1, 4, 16, 64, in ONE process and through ONE handle over a hashed
string, on device-resident coefficients:
  * one batched call of `count` polynomials (the workspace reserved for all of them beforehand): one warm-up, then REPS calls, each the
    whole call up to a stream synchronisation on a host clock, with the profile scopes of that call from bbg_profile_get;
  * beside it `count` single calls of bbg_open_all_device through the same handle, timed the same way as one unit, and the ratio of the
    two medians;
  * the handle's bytes with the reservation.
Medians (of REPS = 9) and minima are printed.  Shapes as LOG2N:LOG2CELL arguments and --counts A,B,.. replace the defaults."""
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

REPS = 9
SEED = 0xBB254
SCOPES = ("open_all_coeffs", "ntt_pass", "open_all_pointwise", "open_cells_sum", "ecntt_stages", "open_all_fold", "ecntt_normalize")


def med_min(v):
    return f"{statistics.median(v):10.3f} {min(v):10.3f}"


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "open_batch.txt")
    counts = [1, 4, 16, 64]
    for flag in ("--out", "--counts"):
        if flag in args:
            i = args.index(flag)
            if flag == "--out":
                out_path = args[i + 1]
            else:
                counts = [int(c) for c in args[i + 1].split(",")]
            del args[i:i + 2]
    shapes = [tuple(int(v) for v in a.split(":")) for a in args] or [(12, 6), (16, 6), (12, 0)]
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    pkg = ge.load_package()
    bbg = pkg.Bbg(0)
    with open(pkg.LIB_PATH, "rb") as f:
        emit(f"# build: libbbg.so sha256 {hashlib.sha256(f.read()).hexdigest()}  (one MI355X)")
    emit(f"# one process, one handle per shape; per count one warm-up and {REPS} timed units of each kind, interleaved: a unit is ONE batched call of")
    emit("# `count` polynomials, or `count` single calls.  every pair of columns is median and minimum in ms.  call = the whole unit on a host")
    emit("# clock, up to a synchronisation; the scopes are bbg_profile_get's (HIP events on the stream) summed over the unit.  points:")
    emit("# bbg_srs_synth_hashed; coefficients spread over [0, 2r)")
    emit("shape     count  what                             batched ms(med min)    single x count ms(med min)")
    for lg, lc in shapes:
        n, proofs = 1 << lg, 1 << (lg - lc)
        top = max(counts)
        srs = bbg.srs_synth_hashed(SEED + lg, n)
        h = bbg.open_all_prepare(srs, lg, lc)
        srs.free()
        d_c, d_o = bbg.dev_alloc(top * n * 32), bbg.dev_alloc(top * proofs * 64)
        bbg.dev_upload(d_c, ci.coarse_scalars(SEED + lg, top * n, 0))
        # (12, 6) x 8 is the condition of tests/test_gpu_open_batch.py: its ratio belongs in the table
        for count in sorted(set(counts) | ({8} if (lg, lc) == (12, 6) and top >= 8 else set())):
            h.reserve_batch(count)

            def batched():
                h.open_batch_device(d_c, count, d_o)

            def looped():
                for p in range(count):
                    h.open_device(d_c + p * n * 32, d_o + p * proofs * 64)

            units = {"batched": batched, "single": looped}
            wall = {k: [] for k in units}
            scopes = {k: {s: [] for s in SCOPES} for k in units}
            for call in units.values():  # warm-up
                call()
            bbg.sync()
            for _ in range(REPS):
                for name, call in units.items():
                    bbg.profile_enable(True)
                    t0 = time.perf_counter()
                    call()
                    bbg.sync()
                    wall[name].append(1e3 * (time.perf_counter() - t0))
                    for s in SCOPES:
                        scopes[name][s].append(bbg.profile_get(s)[0])
                    bbg.profile_enable(False)
            tag = f"({lg:2d},{lc:2d}) {count:6d}"
            emit(f"{tag}  {'call':32s} {med_min(wall['batched'])}   {med_min(wall['single'])}")
            for s in SCOPES:
                emit(f"{tag}  {'  ' + s:32s} {med_min(scopes['batched'][s])}   {med_min(scopes['single'][s])}")
            emit(f"{tag}  {'handle bytes':32s} {h.device_bytes():21d}")
            emit(f"{tag}  {'call, batched / single x count':32s} {statistics.median(wall['batched']) / statistics.median(wall['single']):21.3f}")
        h.free()
        for d in (d_c, d_o):
            bbg.dev_free(d)
    bbg.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
