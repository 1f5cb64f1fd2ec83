#!/usr/bin/env python3
"""Timings of the wave-cooperative pairing product (bbg_pairing_product_wave_device, csrc/pairing_wave.hip) beside the lane form
(bbg_pairing_product_device, csrc/pairing.hip), and of bbg_cells_verify_device beside the two-step route it replaces -- the table in
profiles/pairing_wave.txt.

    python tests/tools/pairing_wave_time.py [OUT [RESOURCES]]      (OUT defaults to profiles/pairing_wave.txt)

RESOURCES: a text file with what `make -C aztec-2.0_amd/csrc pairing_wave.o EXTRA=-Rpass-analysis=kernel-resource-usage` printed; its lines
for k_pair_wave (VGPRs, scratch, LDS, occupancy) are copied into the table.

In ONE process on one MI355X.  Pairing: for pairs = 2 and 4 and count = 1, 16, 256, 2^10, 2^12, 2^14, 2^16, device-resident G1 points made
by bbg_g1_fixed_base_mul_device over scalars spread over [0, 2r); per row and form one warm-up, then REPS = 9 calls, the two forms
interleaved, each sample the whole call on a host clock ending in a stream synchronisation; every sample is listed.  The outputs of the
two forms are compared word for word.  Verdict: 1 024 cells of 8 blobs of 2^13 coefficients with 64-point cells (the shape of
profiles/cells_verify.txt), proofs and commitments points of a hashed string (the cost does not depend on validity), all inputs resident;
    one call       bbg_cells_verify_device, then the download of the status word;
    two steps      bbg_cells_verify_reduce_device, the download of L and R, the negation of R on the host, the upload of the pair,
                   bbg_pairing_product_device (the lane form), the download of the status word -- what a caller had to do before;
    device only    bbg_cells_verify_reduce_device and the lane pairing on (L, R) as they lie, no negation and no round trip: a lower bound
                   on any two-step route, not a verifier."""
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
import pairing_model as pm  # noqa: E402

REPS = 9
SEED = 0xBB254 + 0x3A7E
COUNTS = (1, 16, 256, 1 << 10, 1 << 12, 1 << 14, 1 << 16)
PAIRS = (2, 4)
VERDICT_SHAPE = (13, 6, 8, 1024)  # log2n, log2cell, blobs, cells


def fmt(samples):
    return f"{statistics.median(samples):9.3f}  [" + " ".join(f"{s:.3f}" for s in samples) + "]"


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pairing_wave.txt")
    pkg = ge.load_package()
    bbg = pkg.Bbg(0)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        with open(out_path, "w") as f:  # rewritten row by row: a run that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")

    def timed(fn):
        bbg.sync()
        t0 = time.perf_counter()
        fn()
        bbg.sync()
        return 1e3 * (time.perf_counter() - t0)

    with open(pkg.LIB_PATH, "rb") as f:
        emit(f"# build: libbbg.so sha256 {hashlib.sha256(f.read()).hexdigest()}  (one MI355X)")
    emit(f"# tests/tools/pairing_wave_time.py: one process; per row one warm-up of each form, then {REPS} calls of each, interleaved; a sample is the")
    emit("# whole call on a host clock ending in a stream synchronisation; ms, median [every sample].")
    if len(sys.argv) > 2:
        emit("# -Rpass-analysis=kernel-resource-usage for csrc/pairing_wave.hip:")
        keep = ("Function Name", "VGPRs:", "AGPRs", "ScratchSize", "Occupancy", "LDS Size")
        for row in open(sys.argv[2]):
            if any(k in row for k in keep):
                emit("#   " + row.split("remark:")[-1].replace("[-Rpass-analysis=kernel-resource-usage]", "").strip())
    b = [int.from_bytes(hashlib.sha256(b"pairing_time %d" % j).digest(), "little") % pm.R for j in range(max(PAIRS))]
    q_words = bbg.g2_mul(pm.fr_words(b))
    ahead = {}
    for pairs in PAIRS:
        h = bbg.g2_lines_prepare(q_words[:pairs])
        ahead[pairs] = None
        for count in COUNTS:
            n = count * pairs
            d_s, d_p = bbg.dev_alloc(n * 32), bbg.dev_alloc(n * 64)
            d_o = [bbg.dev_alloc(count * 384) for _ in range(2)]
            d_st = [bbg.dev_alloc(count * 4) for _ in range(2)]
            bbg.dev_upload(d_s, ci.coarse_scalars(SEED + count + pairs, n, 0))
            bbg.g1_fixed_base_mul_device(d_s, n, d_p)
            forms = {"wave": lambda: bbg.pairing_product_wave_device(h, d_p, count, d_o[0], d_st[0]),
                     "lane": lambda: bbg.pairing_product_device(h, d_p, count, d_o[1], d_st[1])}
            samples = {k: [] for k in forms}
            for rep in range(REPS + 1):
                for k, fn in forms.items():
                    samples[k].append(timed(fn))
            same = np.array_equal(bbg.dev_download(d_o[0], (count, 48)), bbg.dev_download(d_o[1], (count, 48))) and \
                np.array_equal(bbg.dev_download(d_st[0], (count,), dtype=np.uint32), bbg.dev_download(d_st[1], (count,), dtype=np.uint32))
            assert same, "the two forms differ"
            wave, lane = samples["wave"][1:], samples["lane"][1:]
            emit(f"pairs {pairs} count {count:6d}  wave {fmt(wave)}")
            emit(f"pairs {pairs} count {count:6d}  lane {fmt(lane)}")
            every = max(wave) < min(lane)
            emit(f"pairs {pairs} count {count:6d}  lane / wave (medians) {statistics.median(lane) / statistics.median(wave):7.2f}   every wave sample below every lane sample: {'yes' if every else 'no'}")
            if statistics.median(wave) < statistics.median(lane):
                ahead[pairs] = count
            for d in [d_s, d_p] + d_o + d_st:
                bbg.dev_free(d)
        h.free()
    for pairs in PAIRS:
        emit(f"# pairs {pairs}: the largest measured count at which the wave form's median is ahead: {ahead[pairs]}")

    lg, lc, ncom, K = VERDICT_SHAPE
    l = 1 << lc
    string = bbg.srs_synth_hashed(SEED, l)
    pool = bbg.srs_synth_hashed(SEED + 1, K + ncom)
    points = pool.read()
    pool.free()
    rho = ci.coarse_scalars(SEED + 2, 1, 0)[0]
    rng = np.random.default_rng(SEED + 3)
    cids, mids = rng.integers(0, ncom, K).astype(np.uint32), rng.integers(0, 1 << (lg - lc), K).astype(np.uint32)
    verdict_lines = bbg.g2_lines_prepare(q_words[:2])
    d_com, d_prf, d_val = bbg.dev_alloc(ncom * 64), bbg.dev_alloc(K * 64), bbg.dev_alloc(K * l * 32)
    d_lr, d_pair, d_st = bbg.dev_alloc(128), bbg.dev_alloc(128), bbg.dev_alloc(4)
    bbg.dev_upload(d_prf, points[:K])
    bbg.dev_upload(d_com, points[K:])
    bbg.dev_upload(d_val, ci.coarse_scalars(SEED + 4, K * l, 0))
    got = {}

    def one_call():
        bbg.cells_verify_device(string, verdict_lines, lg, lc, d_com, ncom, cids, mids, d_val, d_prf, rho, d_st)
        got["one call"] = int(bbg.dev_download(d_st, (1,), dtype=np.uint32)[0])

    def two_steps():
        bbg.cells_verify_reduce_device(string, lg, lc, d_com, ncom, cids, mids, d_val, d_prf, rho, d_lr)
        lr = bbg.dev_download(d_lr, (2, 8))
        r = pm.g1_from_words(lr[1])
        bbg.dev_upload(d_pair, np.stack([lr[0], pm.g1_words(None if r is None else (r[0], -r[1] % pm.P))]))
        bbg.pairing_product_device(verdict_lines, d_pair, 1, None, d_st)
        got["two steps"] = int(bbg.dev_download(d_st, (1,), dtype=np.uint32)[0])

    def device_only():
        bbg.cells_verify_reduce_device(string, lg, lc, d_com, ncom, cids, mids, d_val, d_prf, rho, d_lr)
        bbg.pairing_product_device(verdict_lines, d_lr, 1, None, d_st)

    routes = {"one call": one_call, "two steps": two_steps, "device only": device_only}
    samples = {k: [] for k in routes}
    for rep in range(REPS + 1):
        for k, fn in routes.items():
            samples[k].append(timed(fn))
    assert got["one call"] == got["two steps"], "the two routes disagree"
    emit(f"# verdict: log2n {lg}, log2cell {lc}, {ncom} blobs, {K} cells, device-resident inputs; status {got['one call']} by both routes")
    for k in routes:
        emit(f"verdict  {k:12s} {fmt(samples[k][1:])}")
    for d in (d_com, d_prf, d_val, d_lr, d_pair, d_st):
        bbg.dev_free(d)
    verdict_lines.free()
    string.free()
    bbg.close()


if __name__ == "__main__":
    main()
