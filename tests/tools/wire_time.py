#!/usr/bin/env python3
"""Timings of bbg_wire_decode_device and bbg_wire_encode_device (csrc/wire.hip) -- the tables in profiles/wire.txt, which this
script writes (--out PATH for another place; the lines are printed as well).

ONE process, one context on a stream of its own; every figure is the time between two events recorded on that stream around the queued
work, one warm-up and then REPS = 9 samples per line, the median first and every sample after it, in ms.

  A  decode of 2^12, 2^16 and 2^20 compressed points beside the DERIVED ceiling of the chain (335 products x 160 multiply-adds per point
     over 33.8 T multiply-adds per second: not a measurement) and beside the buffer-form decode of the same count, the same traffic per
     output without the chain; encode at the same sizes, both forms.  The points are a hashed string, every one on the curve.
  B  bbg_kzg_verify_device at N = 2^10 and 2^14 from compressed commitments and proofs (two decodes queued ahead of it) beside the same call
     on native inputs, interleaved.
  C  the compiler's resource figures of every kernel of csrc/wire.hip (hipcc -Rpass-analysis=kernel-resource-usage), and of the compressed
     decode with the window table as a register array (-DBBG_WIRE_TABLE_REGS), the placement DESIGN.md 5m compares.  No GPU is needed for
     this part: `--resources-only` makes it alone and APPENDS it to the file, `--no-resources` leaves it out of a GPU run.

`--quick` leaves the 2^20 rows out."""
import hashlib
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import __graft_entry__ as ge  # noqa: E402

REPS = 9
SEED = 0xBB254 + 0x31BE
PRODUCTS, MADS_PER_PRODUCT, MADS_PER_SECOND = 335, 160, 33.8e12
COMPRESSED, BUFFER = 0, 2


def resources(emit, extra=()):
    """One line per kernel of csrc/wire.hip from the compiler's remarks."""
    csrc = os.path.join(ROOT, "aztec-2.0_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I/opt/rocm/include", *extra,
                            "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "wire.hip"), "-o", os.path.join(d, "wire.o")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        emit("  hipcc failed: " + r.stdout.decode()[-300:])
        return
    text = r.stdout.decode()
    kernel, row = None, {}

    def name_of(mangled):  # _ZN3bbg13k_wire_decodeILi0EEEvPKcmPcPjS4_ -> k_wire_decode<0>
        m = re.search(r"(k_wire_[a-z]+)(?:ILi(\d+)E)?", mangled)
        return mangled if not m else m.group(1) + (f"<{m.group(2)}>" if m.group(2) else "")
    emit("  kernel                                   VGPRs  SGPRs  scratch B/lane  LDS B/block  waves/SIMD")

    def flush():
        if kernel:
            emit(f"  {kernel:40s} {row.get('VGPRs', '?'):>5s}  {row.get('TotalSGPRs', '?'):>5s}  {row.get('ScratchSize [bytes/lane]', '?'):>14s}  "
                 f"{row.get('LDS Size [bytes/block]', '?'):>11s}  {row.get('Occupancy [waves/SIMD]', '?'):>10s}")
    for line in text.splitlines():
        m = re.search(r"remark:\s+Function Name: (.*?) \[-Rpass", line)
        if m:
            flush()
            kernel, row = name_of(m.group(1)), {}
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if m:
            row[m.group(1).strip()] = m.group(2)
    flush()


def main():
    args = sys.argv[1:]
    out_path = os.path.join(ROOT, "profiles", "wire.txt")
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    quick = "--quick" in args
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def section_c():
        emit("")
        emit("# C  hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage on csrc/wire.hip as built")
        resources(emit)
        emit("#    the same with -DBBG_WIRE_TABLE_REGS: the window table as a register array indexed by the digit")
        resources(emit, ("-DBBG_WIRE_TABLE_REGS",))

    if "--resources-only" in args:
        section_c()
        with open(out_path, "a") as f:
            f.write("\n".join(lines) + "\n")
        return
    import torch
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
        emit(f"{tag}{what:52s} {statistics.median(samples):10.4f}   " + " ".join(f"{v:.4f}" for v in samples))

    def sampled(*fns):
        """One warm-up each, then REPS samples of each, interleaved."""
        for fn in fns:
            fn()
        bbg.sync()
        out = [[] for _ in fns]
        for _ in range(REPS):
            for t, fn in zip(out, fns):
                t.append(timed(fn))
        return out

    with open(pkg.LIB_PATH, "rb") as f:
        emit(f"# build: libbbg.so sha256 {hashlib.sha256(f.read()).hexdigest()}  (one MI355X)")
    emit(f"# one process; events on the context's stream; one warm-up, then {REPS} samples per line, the calls of a case interleaved;")
    emit("# columns: the median, then every sample, in ms.")

    sizes = [12, 16] + ([] if quick else [20])
    nmax = 1 << max(sizes + [14])
    srs = bbg.srs_synth_hashed(SEED, 2 * nmax)  # points on the curve: commitments from the first half, proofs from the second
    d_points = bbg.dev_alloc(2 * nmax * 64)
    bbg.dev_upload(d_points, srs.read())
    srs.free()
    d_wire, d_native, d_status, d_bad = bbg.dev_alloc(2 * nmax * 64), bbg.dev_alloc(2 * nmax * 64), bbg.dev_alloc(2 * nmax * 4), bbg.dev_alloc(16)

    emit("")
    emit("# A  one call over n points, status words and the count written")
    emit("log2n  what                                                 ms(median)   samples")
    for lg in sizes:
        n = 1 << lg
        tag = f"{lg:5d}  "
        for form, name in ((COMPRESSED, "compressed"), (BUFFER, "buffer")):
            bbg.wire_encode_device(form, d_points, n, 1, d_wire, d_status, d_bad)
            bbg.sync()
            assert int(bbg.dev_download(d_bad, (1,), dtype="uint32")[0]) == 0
            dec, enc0, enc1 = sampled(lambda: bbg.wire_decode_device(form, d_wire, n, d_native, d_status, d_bad),
                                      lambda: bbg.wire_encode_device(form, d_native, n, 0, d_wire, d_status, d_bad),
                                      lambda: bbg.wire_encode_device(form, d_native, n, 1, d_wire, d_status, d_bad))
            assert int(bbg.dev_download(d_bad, (1,), dtype="uint32")[0]) == 0
            row(tag, f"bbg_wire_decode_device, {name}", dec)
            if form == COMPRESSED:
                emit(f"{tag}{'  derived ceiling of the chain (not measured)':52s} {PRODUCTS * MADS_PER_PRODUCT * n / MADS_PER_SECOND * 1e3:10.4f}")
            row(tag, f"bbg_wire_encode_device, {name}, check = 0", enc0)
            row(tag, f"bbg_wire_encode_device, {name}, check = 1", enc1)

    emit("")
    emit("# B  bbg_kzg_verify_device: two bbg_wire_decode_device (compressed) queued ahead of it, beside the call on native inputs")
    emit("    N  what                                                 ms(median)   samples")
    import coarse_inputs as ci
    g2_lines = bbg.g2_lines_prepare(bbg.g2_mul(ci.to_words([3, 5])))  # two finite points of the subgroup: the time does not depend on them
    rho = ci.coarse_scalars(SEED + 3, 1, 0)[0]
    for N in (1 << 10, 1 << 14):
        d_com, d_prf = d_points, d_points + nmax * 64
        d_cw, d_pw = d_wire, d_wire + nmax * 64
        d_c, d_p = d_native, d_native + nmax * 64
        d_z, d_y = bbg.dev_alloc(N * 32), bbg.dev_alloc(N * 32)
        bbg.dev_upload(d_z, ci.coarse_scalars(SEED + 4, N, 0))
        bbg.dev_upload(d_y, ci.coarse_scalars(SEED + 5, N, 0))
        bbg.wire_encode_device(COMPRESSED, d_com, N, 1, d_cw)
        bbg.wire_encode_device(COMPRESSED, d_prf, N, 1, d_pw)

        def from_bytes():
            bbg.wire_decode_device(COMPRESSED, d_cw, N, d_c, None, d_bad)
            bbg.wire_decode_device(COMPRESSED, d_pw, N, d_p, None, d_bad + 4)
            bbg.kzg_verify_device(g2_lines, d_c, d_z, d_y, d_p, N, rho, d_bad + 8)

        def native():
            bbg.kzg_verify_device(g2_lines, d_com, d_z, d_y, d_prf, N, rho, d_bad + 12)
        t_bytes, t_native = sampled(from_bytes, native)
        words = bbg.dev_download(d_bad, (4,), dtype="uint32")
        assert int(words[0]) == 0 and int(words[1]) == 0 and int(words[2]) == int(words[3]), words
        tag = f"{N:5d}  "
        row(tag, "2 x bbg_wire_decode_device + bbg_kzg_verify_device", t_bytes)
        row(tag, "bbg_kzg_verify_device on native inputs", t_native)
        bbg.dev_free(d_z)
        bbg.dev_free(d_y)
    g2_lines.free()
    for d in (d_points, d_wire, d_native, d_status, d_bad):
        bbg.dev_free(d)
    bbg.close()
    if "--no-resources" not in args:
        section_c()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
