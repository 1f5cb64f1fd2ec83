#!/usr/bin/env python3
"""Timings of bbg_open_points_device and bbg_kzg_verify_device (csrc/open_points.hip, csrc/kzg_verify.hip) beside the routes
they replace -- the tables in profiles/open_points.txt, which this script writes (--out PATH for another place; the lines are printed as well).

ONE process, one context on a stream of its own; every figure is the time between two events recorded on that stream around the queued
work, one warm-up and then REPS = 9 samples per line, the median first and every sample after it, in ms.

  A  bbg_open_points_device at 2^12, 2^16 and 2^20 values with 1, 8 and 64 polynomials (1 and 8 at 2^20), its scopes from bbg_profile_get over
     further calls, and beside it, interleaved, the route it replaces: per polynomial bbg_kate_opening_lagrange_device (which hands F(z) to
     the host and so synchronises) and bbg_msm_device, then one bbg_g1_normalize over all results (host arrays: download, upload, download).
  B  the same call with d_proofs = NULL beside bbg_poly_evaluate_lagrange_device, the NEAREST existing call and not an equal: that one takes
     at most 32 polynomials and ONE point shared by all of them, so 64 polynomials are two calls of 32.
  C  bbg_kzg_verify_device at N = 1, 64, 2^10, 2^14, 2^17 beside bbg_cells_verify_device at log2cell = 0 over the same number of openings
     placed on the points of a domain of max(2^6, N) points: the only existing verifier.  Commitments and proofs are points on the curve
     (a hashed string: either reduction costs the same for valid and invalid proofs), values, points and the challenge arbitrary field elements.

`--quick` leaves the 2^20 rows and N = 2^17 out."""
import hashlib
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import __graft_entry__ as ge  # noqa: E402
import coarse_inputs as ci  # noqa: E402

REPS = 9
SEED = 0xBB254 + 0x09E7
OPEN_SCOPES = ("open_points_weights", "open_points_quotient", "msm_recode", "msm_sort", "msm_offsets", "msm_accumulate", "msm_reduce", "open_points_normalize")
VERIFY_SCOPES = ("kzg_verify_prepare", "msm_points_sort", "msm_points_accumulate", "msm_points_reduce", "msm_points_combine", "cells_verify_pack", "pairing_wave")


def main():
    import torch
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "open_points.txt")
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    quick = "--quick" in args
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    pkg = ge.load_package()
    bbg = pkg.Bbg(0)
    stream = torch.cuda.Stream()
    bbg.set_stream(stream.cuda_stream)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        bbg.sync()
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    def row(tag, what, samples):
        emit(f"{tag}{what:44s} {statistics.median(samples):10.3f}   " + " ".join(f"{v:.3f}" for v in samples))

    def side_by_side(new, old):
        for fn in (new, old):
            fn()
        bbg.sync()
        t_new, t_old = [], []
        for _ in range(REPS):
            t_new.append(timed(new))
            t_old.append(timed(old))
        return t_new, t_old

    def scopes_of(fn, names):
        got = {s: [] for s in names}
        for _ in range(REPS):
            bbg.profile_enable(True)
            fn()
            bbg.sync()
            for s in names:
                got[s].append(bbg.profile_get(s)[0])
            bbg.profile_enable(False)
        return got

    def verdict(new, old):
        m_new, m_old = statistics.median(new), statistics.median(old)
        if max(new) < min(old):
            return f"ahead: median {m_old / m_new:.2f}x, sample lists disjoint"
        if min(new) > max(old):
            return f"behind: median {m_new / m_old:.2f}x slower, sample lists disjoint"
        return f"draws: medians {m_new:.3f} against {m_old:.3f}, sample lists overlap"

    with open(pkg.LIB_PATH, "rb") as f:
        emit(f"# build: libbbg.so sha256 {hashlib.sha256(f.read()).hexdigest()}  (one MI355X)")
    emit(f"# one process; events on the context's stream; one warm-up, then {REPS} samples per line, the two routes of a case interleaved;")
    emit("# columns: the median, then every sample, in ms.  Scope rows: bbg_profile_get totals over further calls.")

    # ---- A, B: opening and evaluating
    emit("")
    emit("# A / B  bbg_open_points_device beside count x (bbg_kate_opening_lagrange_device + bbg_msm_device) + bbg_g1_normalize, and its")
    emit("#        evaluation-only form beside bbg_poly_evaluate_lagrange_device (at most 32 polynomials, ONE shared point: nearest, not equal)")
    emit("log2n count  what                                         ms(median)   samples")
    open_cases = [(lg, c) for lg in (12, 16) for c in (1, 8, 64)] + ([] if quick else [(20, 1), (20, 8)])
    lags = {}
    for lg, count in open_cases:
        n = 1 << lg
        if lg not in lags:
            srs = bbg.srs_synth_hashed(SEED + lg, n)  # any string will do for the time: the call cannot tell a Lagrange form from another
            lags[lg] = srs
        lag = lags[lg]
        d_evals, d_z, d_y, d_p = bbg.dev_alloc(count * n * 32), bbg.dev_alloc(count * 32), bbg.dev_alloc(count * 32), bbg.dev_alloc(count * 64)
        d_dest, d_jac = bbg.dev_alloc(n * 32), bbg.dev_alloc(count * 96)
        z = pkg.synthetic_scalars(SEED + 1, count)
        for k in range(count):
            bbg.dev_upload(d_evals + k * n * 32, pkg.synthetic_scalars(SEED + 2 + k, n))
        bbg.dev_upload(d_z, z)

        def new():
            bbg.open_points_device(lag, lg, d_evals, d_z, count, d_y, d_p)

        def old():
            for k in range(count):
                bbg.kate_opening_lagrange_device(d_evals + k * n * 32, d_dest, lg, z[k])
                bbg.msm_device(lag, d_dest, n, d_jac + 96 * k)
            bbg.join()
            bbg.g1_normalize(bbg.dev_download(d_jac, (count, 12)))

        def new_eval():
            bbg.open_points_device(None, lg, d_evals, d_z, count, d_y, None)

        def old_eval():
            for first in range(0, count, 32):
                bbg.poly_evaluate_lagrange_device([d_evals + k * n * 32 for k in range(first, min(first + 32, count))], lg, z[0])
        tag = f"{lg:5d} {count:5d}  "
        t_new, t_old = side_by_side(new, old)
        row(tag, "bbg_open_points_device", t_new)
        for s, v in scopes_of(new, OPEN_SCOPES).items():
            row(tag, "  " + s, v)
        row(tag, "count x (kate_lagrange + msm) + normalize", t_old)
        emit(f"{tag}{'-> ' + verdict(t_new, t_old)}")
        t_new, t_old = side_by_side(new_eval, old_eval)
        row(tag, "bbg_open_points_device, values only", t_new)
        row(tag, "bbg_poly_evaluate_lagrange_device (shared z)", t_old)
        emit(f"{tag}{'-> ' + verdict(t_new, t_old)}")
        for d in (d_evals, d_z, d_y, d_p, d_dest, d_jac):
            bbg.dev_free(d)
    for srs in lags.values():
        srs.free()

    # ---- C: verifying
    emit("")
    emit("# C  bbg_kzg_verify_device beside bbg_cells_verify_device at log2cell = 0 over the same number of openings on domain points")
    emit("log2n     N  what                                         ms(median)   samples")
    ns = [1, 64, 1 << 10, 1 << 14] + ([] if quick else [1 << 17])
    pool = bbg.srs_synth_hashed(SEED + 100, 2 * max(ns))
    points = pool.read()
    pool.free()
    string = bbg.srs_synth_hashed(SEED + 101, 64)
    g2 = bbg.g2_mul(ci.to_words([3, 5]))  # two finite points of the subgroup: the time does not depend on them
    g2_lines = bbg.g2_lines_prepare(g2)
    rho = ci.coarse_scalars(SEED + 103, 1, 0)[0]
    for N in ns:
        lg = max(6, (N - 1).bit_length())
        rng = np.random.default_rng(SEED + N)
        mids = rng.permutation(1 << lg)[:N].astype(np.uint32)
        cids = np.arange(N, dtype=np.uint32)
        d_com, d_prf, d_z, d_yv, d_st = bbg.dev_alloc(N * 64), bbg.dev_alloc(N * 64), bbg.dev_alloc(N * 32), bbg.dev_alloc(N * 32), bbg.dev_alloc(8)
        bbg.dev_upload(d_com, points[:N])
        bbg.dev_upload(d_prf, points[max(ns):max(ns) + N])
        bbg.dev_upload(d_z, ci.coarse_scalars(SEED + 104, N, 0))
        bbg.dev_upload(d_yv, ci.coarse_scalars(SEED + 105, N, 0))

        def new():
            bbg.kzg_verify_device(g2_lines, d_com, d_z, d_yv, d_prf, N, rho, d_st)

        def old():
            bbg.cells_verify_device(string, g2_lines, lg, 0, d_com, N, cids, mids, d_yv, d_prf, rho, d_st + 4)
        tag = f"{lg:5d} {N:6d} "
        t_new, t_old = side_by_side(new, old)
        row(tag, "bbg_kzg_verify_device", t_new)
        for s, v in scopes_of(new, VERIFY_SCOPES).items():
            row(tag, "  " + s, v)
        row(tag, "bbg_cells_verify_device, log2cell = 0", t_old)
        emit(f"{tag}{'-> ' + verdict(t_new, t_old)}")
        for d in (d_com, d_prf, d_z, d_yv, d_st):
            bbg.dev_free(d)
    g2_lines.free()
    string.free()
    bbg.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
