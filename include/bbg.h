/*
 * bbg.h -- C ABI of libbbg.so: the MI355X (gfx950) implementation of barretenberg's PLONK-prover
 * hot path -- Pippenger MSM over BN254 G1 and the radix-2 NTT family over BN254 Fr.
 *
 * This is the drop-in boundary.  Every entry point takes plain pointers and sizes in the
 * REFERENCE'S OWN MEMORY LAYOUT (paths relative to barretenberg/src/aztec/):
 *   fr / fq           32 B, 4 x u64 little-endian limbs, Montgomery form R = 2^256, any representative
 *                     in [0, 2p) accepted                        (ecc/fields/field.hpp:24,86)
 *   g1::affine_element 64 B  x || y                               (ecc/groups/affine_element.hpp:70-71)
 *   g1::element        96 B  x || y || z Jacobian, infinity = bit 63 of x.data[3]
 *                                                                 (ecc/groups/element.hpp:88-90, element_impl.hpp:497-516)
 * so a barretenberg build binds them with no marshalling (see INTEGRATION.md for the C++ shim that
 * re-exports scalar_multiplication::pippenger*() and polynomial_arithmetic::fft*() on top of this).
 *
 * All functions return 0 on success and a negative BBG_E* code on failure; bbg_last_error() gives a
 * thread-local message.  The reference has no status codes (throw_or_abort, common/throw_or_abort.hpp:5-13);
 * the C++ shim turns a non-zero return into std::runtime_error.
 *
 * There is no CPU fallback anywhere behind this ABI: without a HIP device bbg_init() fails.
 */
#ifndef BBG_H
#define BBG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BBG_OK 0
#define BBG_E_INVALID (-1)  /* bad argument (null pointer, size out of range, n not a power of two ...) */
#define BBG_E_HIP (-2)      /* a HIP runtime call failed; see bbg_last_error() */
#define BBG_E_NODEVICE (-3) /* no gfx950 device visible */
#define BBG_E_NOMEM (-4)
#define BBG_E_INFINITY (-5) /* a result that must be a finite point is the point at infinity (bbg_srs_lagrange) */

typedef struct bbg_ctx bbg_ctx; /* one per GPU / per process rank */
typedef struct bbg_srs bbg_srs; /* device-resident SRS (the Pippenger point table) */

/* ---- context ---------------------------------------------------------------------------------------- */
int bbg_device_count(void);
/* Binds `device` (hipSetDevice), creates the context and its stream. */
int bbg_init(int device, bbg_ctx** out);
void bbg_destroy(bbg_ctx* ctx);
const char* bbg_last_error(void);
/* Blocks until everything queued on the context's stream has finished. */
int bbg_sync(bbg_ctx* ctx);
/* With the option "msm_async_reduce" = 1 the last phase of bbg_msm_device (bucket reduction) is queued on an auxiliary
 * stream so that it overlaps the next call's sort / accumulation (the prover issues several independent MSMs per round,
 * prover.cpp:66-73).  The result buffer is then complete after bbg_sync(), or, for stream-ordered consumers, after
 * bbg_join(): it makes the context stream wait (on the device, no host sync) for all outstanding reductions. */
int bbg_join(bbg_ctx* ctx);
/* Like bbg_join but leaves the `lag` most recent reductions outstanding (lag = 1: wait for everything except the
 * MSM issued last) -- lets a caller consume result i-1 while MSM i is still reducing.  At most two reductions are ever
 * outstanding (the reduce slots; a third MSM waits for the slot it reuses), so lag >= 2 waits for nothing and returns BBG_OK. */
int bbg_join_lag(bbg_ctx* ctx, int lag);
/* Use a caller-owned HIP stream (hipStream_t passed as void*; e.g. torch.cuda.current_stream().cuda_stream).  Every *_device
 * entry point enqueues on the context stream and returns; a caller that fills or reads those device buffers on ANOTHER stream
 * (a framework's memset, a copy) must order the two itself -- sharing one stream through this call is the simple way. */
int bbg_set_stream(bbg_ctx* ctx, void* hip_stream);

/* ---- SRS: replaces scalar_multiplication::Pippenger (ecc/curves/bn254/scalar_multiplication/pippenger.hpp:35-52,
 *      pippenger.cpp:7-37) and the C binding new_pippenger/delete_pippenger (.../c_bind.cpp:17-29). --------------
 * points: n affine points in Montgomery form.  stride_bytes = 64 for a plain array P_0..P_{n-1} (what
 * io::read_transcript_g1 yields, srs/io.cpp:134-162) or 128 for the reference's interleaved endomorphism table
 * [P_i, (beta*x_i, -y_i)] (generate_pippenger_point_table, scalar_multiplication.cpp:104-112), whose odd entries
 * are ignored: the (beta*x, -y) twin is one Fq multiplication on chip.  The table is uploaded to HBM once. */
int bbg_srs_register(bbg_ctx* ctx, const uint64_t* points, size_t n, size_t stride_bytes, bbg_srs** out);
/* Same, from a device buffer of n plain 64-byte points (copied). */
int bbg_srs_register_device(bbg_ctx* ctx, const void* d_points, size_t n, bbg_srs** out);
/* Synthetic SRS P_i = (a + i*s)*G generated on the GPU (the Ignition transcript is absent from the
 * reference snapshot).  a, s: plain 64-bit scalars, s != 0. */
int bbg_srs_synth_linear(bbg_ctx* ctx, uint64_t a, uint64_t s, size_t n, bbg_srs** out);
/* Synthetic SRS P_i = k_i*G, k_i = mix64(seed + i) | 1 (splitmix64 finaliser): no small linear relations between
 * the bases, which pippenger_unsafe requires of its inputs (scalar_multiplication.cpp:908-921). */
int bbg_srs_synth_hashed(bbg_ctx* ctx, uint64_t seed, size_t n, bbg_srs** out);
/* Structured SRS P_i = [x^i] G, i < n (P_0 = G): what a powers-of-tau ceremony outputs for a KNOWN x, i.e. a test / benchmark
 * string.  x: Montgomery Fr on the host, [0, 2r).  x = 0 mod r -> BBG_E_INVALID (P_1 would be infinite), *out untouched.  n need not be
 * a power of two.  The powers are made on the device and multiplied into G by bbg_g1_fixed_base_mul's kernels (32 n bytes of working
 * memory beside the result, freed before return). */
int bbg_srs_synth_powers(bbg_ctx* ctx, const uint64_t x[4], size_t n, bbg_srs** out);
/* The update step of a powers-of-x string: *out is a new SRS of the same length with P_i' = [y^i] P_i (P_0' = P_0), so that a string for x
 * becomes the string for x y -- what a ceremony participant, or a test harness, does to an EXISTING string whose x nobody knows.  y:
 * Montgomery Fr on the host, [0, 2r).  y = 0 mod r -> BBG_E_INVALID, *out untouched.  `srs` is only read and must live on the context's
 * device.  The powers y^i are made on the device and multiplied into the points by bbg_g1_batch_mul_device's kernel (32 n bytes of working
 * memory beside the result, freed before return, and the tables described there). */
int bbg_srs_scale_powers(bbg_ctx* ctx, bbg_srs* srs, const uint64_t y[4], bbg_srs** out);
/* Reads an Ignition-format transcript file (manifest + big-endian points; srs/io.cpp:11-162): result is
 * monomials[0] = G followed by the file's points, num_points in total -- exactly read_transcript_g1. */
int bbg_srs_load_transcript(bbg_ctx* ctx, const char* path, size_t num_points, bbg_srs** out);
/* The same from memory: Pippenger(uint8_t const* points, size_t num_points) (pippenger.cpp:7-17, the C binding new_pippenger): `points` =
 * (num_points - 1) x 64 bytes in the transcript encoding (srs/io.cpp:47-67); monomials[0] = G. */
int bbg_srs_register_transcript_buffer(bbg_ctx* ctx, const uint8_t* points, size_t num_points, bbg_srs** out);
/* The inverse: writes the SRS as Ignition-format files dir/transcript00.dat, 01, ... holding points 1 .. n-1 (point 0 is the
 * generator every reader supplies itself, srs/io.cpp:137), points_per_file per file (0 = one file); manifest and point encoding of
 * srs/io.cpp:11-67.  g2_x_raw (may be NULL): 128 bytes stored as file 00's single G2 point, as given.  Each file ends with the
 * BLAKE2b-512 checksum of what precedes it. */
int bbg_srs_write_transcript(bbg_srs* srs, const char* dir, size_t points_per_file, const uint8_t* g2_x_raw);
/* BLAKE2b-512 (RFC 7693) of a byte string: the checksum that closes a transcript file.  Host only, needs no GPU. */
int bbg_transcript_checksum(const void* data, size_t len, uint8_t out[64]);
size_t bbg_srs_num_points(const bbg_srs* srs);
/* Copies points [from, from+count) back to the host (64-byte Montgomery affine each). */
int bbg_srs_read(bbg_srs* srs, size_t from, size_t count, uint64_t* out_points);
/* The Lagrange-base form of a reference string: lagrange_base::transform_srs (srs/lagrange_base_transformation/lagrange_base.cpp:31-46)
 * as an inverse NTT over G1 on the device.  With n = 2^log2n (1 <= log2n <= 28, n <= bbg_srs_num_points(srs)) and M_j the first n points of `srs`,
 * *out is a new SRS of n points LB[k] = n^-1 * sum_j w_n^(-j k) M_j (w_n = fr::get_root_of_unity(log2n), natural order): for a monomial string
 * M_j = [x^j] G that is [L_k(x)] G, so bbg_msm over a polynomial's EVALUATIONS and *out equals bbg_msm over its coefficients and `srs`.
 * `srs` is only read and must live on the context's device; *out has its own lifetime and is an ordinary SRS for every entry point.
 * Points at infinity inside the transform are handled; one among the OUTPUTS (linearly dependent inputs) fails with BBG_E_INFINITY and
 * leaves *out untouched.  Timed under "ecntt_stages" / "ecntt_normalize" (bbg_profile_get). */
int bbg_srs_lagrange(bbg_ctx* ctx, bbg_srs* srs, unsigned log2n, bbg_srs** out);
/* Shared ownership: bbg_srs_retain adds an owner, bbg_srs_free drops one; the device memory goes with the last owner.  bbg_prover_create
 * retains the SRS it is given (and bbg_prover_destroy releases it), so freeing or replacing a cached SRS never invalidates a live prover. */
int bbg_srs_retain(bbg_srs* srs);
void bbg_srs_free(bbg_srs* srs);

/* ---- MSM: replaces scalar_multiplication::pippenger / pippenger_unsafe
 *      (scalar_multiplication.cpp:853-929) and Pippenger::pippenger_unsafe(scalars, from, range) (pippenger.cpp:27-31),
 *      C binding pippenger_unsafe (c_bind.cpp:31-37). -------------------------------------------------------------
 * result = sum_{i<n} scalars[i] * P_{from+i}.  scalars: n x 4 limbs, Montgomery Fr.  out_jacobian: 12 limbs
 * (g1::element).  Exceptional cases (equal / opposite points, zero scalars, n = 0 -> infinity) are always handled,
 * i.e. the behaviour of handle_edge_cases = true; the "unsafe" entry of the shim maps here too. */
int bbg_msm(bbg_ctx* ctx, bbg_srs* srs, const uint64_t* scalars, size_t from, size_t n, uint64_t out_jacobian[12]);
/* Device-resident variant: d_scalars and d_out_jacobian (96 B) are device pointers; asynchronous on the context stream. */
int bbg_msm_device(bbg_ctx* ctx, bbg_srs* srs, const void* d_scalars, size_t from, size_t n, void* d_out_jacobian);
/* A round's independent commitments as ONE unit of work -- what the reference queues and processes together (the four wire commitments of
 * round 1, prover.cpp:66-74; the quotient parts of round 4, :120-135; work_queue.hpp:208-282): `count` (<= BBG_MSM_BATCH_MAX) MSMs over the SAME
 * SRS go through ONE sort / accumulate / reduce launch set, MSM k's entries filed under bucket set k (count x 2^(C-1) buckets), instead of
 * `count` latency chains.  out_jacobians[k] = sum_{i<n[k]} scalars[k][i] * P_{from[k]+i}; from == NULL means all zero; the n[k] may differ
 * (StandardPLONK's t_high has n + 1 coefficients).  Each result is the same group element bbg_msm gives for that MSM alone. */
#define BBG_MSM_BATCH_MAX 8
int bbg_msm_batch(bbg_ctx* ctx, bbg_srs* srs, size_t count, const uint64_t* const* scalars, const size_t* from, const size_t* n,
                  uint64_t* out_jacobians /* count x 12 limbs */);
/* Device-resident variant: d_scalars[k] are device pointers, d_out_jacobians holds count x 96 B; asynchronous on the context stream. */
int bbg_msm_batch_device(bbg_ctx* ctx, bbg_srs* srs, size_t count, const void* const* d_scalars, const size_t* from, const size_t* n,
                         void* d_out_jacobians);
/* The configuration an n-term MSM over `srs` (may be NULL: a fresh SRS of n points) would run with now: *window_bits = the widest bucket
 * window C (buckets = 2^(C-1)), *windows = the number of windows, i.e. table gathers and mixed additions per scalar.  Follows the option
 * "msm_window" and the resident-table rule for short MSMs over long SRSs. */
int bbg_msm_plan(bbg_ctx* ctx, const bbg_srs* srs, size_t n, int* window_bits, int* windows);
/* g1_sum (c_bind.cpp:39-46): sum of n Jacobian points (host arrays, 96 B each). */
int bbg_g1_sum(bbg_ctx* ctx, const uint64_t* jacobians, size_t n, uint64_t out_jacobian[12]);
/* Same on device buffers, asynchronous on the context stream (the multi-GPU combine after an all-gather of partials). */
int bbg_g1_sum_device(bbg_ctx* ctx, const void* d_jacobians, size_t n, void* d_out_jacobian);
/* g1::affine_element(result) (element_impl.hpp:51-68) for n points; output canonical Montgomery affine (64 B each). */
int bbg_g1_normalize(bbg_ctx* ctx, const uint64_t* jacobians, size_t n, uint64_t* out_affine);
/* Fixed-base batch scalar multiplication (no counterpart in the reference, which loops over element::operator* on the host):
 * out_affine[i] = scalars[i] * B for i < n.  base_affine: one 64-byte Montgomery affine point on the HOST (any
 * representative in [0, 2p) per coordinate), NULL = the generator (1, 2).  scalars: Montgomery Fr, any representative in
 * [0, 2r).  out: 64-byte canonical Montgomery affine points; a result that is the point at infinity (s = 0 mod r, or an
 * infinite base) is written in the reference's affine encoding of infinity, exactly what aff_inf() in csrc/curve.hip.h
 * writes (bit 63 of x.data[3] set, every other bit zero).  n = 0 is legal and does nothing.  A base that is not on the curve is
 * BBG_E_INVALID.  A table of B's multiples d * 2^(8w) * B (510 KiB, counted under `scratch` in bbg_memory_report, released by
 * bbg_memory_trim) is built on the first call and rebuilt when the base changes; each scalar then costs at most 32 mixed additions.
 * Timed under "fixed_base_table" / "fixed_base_mul" (bbg_profile_get). */
int bbg_g1_fixed_base_mul(bbg_ctx* ctx, const uint64_t* base_affine, const uint64_t* scalars, size_t n, uint64_t* out_affine);
/* Device-resident: d_scalars and d_out_affine are device pointers, asynchronous on the context stream. */
int bbg_g1_fixed_base_mul_device(bbg_ctx* ctx, const uint64_t* base_affine, const void* d_scalars, size_t n, void* d_out_affine);

/* Variable-base batch scalar multiplication: out_affine[i] = scalars[i] * points_affine[i] for i < n, n different points.  With
 * one_scalar != 0 only scalars[0] is read and out_affine[i] = scalars[0] * points_affine[i]: element::batch_mul_with_endomorphism(points,
 * exponent) (ecc/groups/element_impl.hpp:666-832).  points: 64-byte Montgomery affine, any representative in [0, 2p) per coordinate; the
 * affine encoding of infinity is accepted and gives infinity.  Points are NOT checked to be on the curve: for a point off it the result is
 * unspecified (but nothing else is affected).  scalars: Montgomery Fr, any representative in [0, 2r).  out: canonical Montgomery affine;
 * a result at infinity is written exactly as bbg_g1_fixed_base_mul writes it.  n = 0 is legal and does nothing; null pointers with n > 0
 * are BBG_E_INVALID.  Each product is a GLV multiplication on signed 4-bit windows (csrc/var_base.hip.h: the scalar split against the
 * cube root of unity into two halves below 2^128, a table of the point's odd multiples P .. 15P, 32 rounds of 4 doublings + 2 additions)
 * on the complete addition formulas, so every scalar and every point is handled.  Working memory: 1 KiB of table per lane for at most
 * "batch_mul_lanes" lanes (default 2^17: 128 MiB, whatever n is), counted under `scratch` in bbg_memory_report and released by
 * bbg_memory_trim.  Timed under "var_base_mul" (bbg_profile_get). */
int bbg_g1_batch_mul(bbg_ctx* ctx, const uint64_t* points_affine, const uint64_t* scalars, size_t n, int one_scalar, uint64_t* out_affine);
/* Device-resident: device pointers, asynchronous on the context stream.  d_out_affine may BE d_points_affine (the points are multiplied
 * in place); an output that overlaps the points in any other way, or overlaps the scalars, is refused with BBG_E_INVALID. */
int bbg_g1_batch_mul_device(bbg_ctx* ctx, const void* d_points_affine, const void* d_scalars, size_t n, int one_scalar, void* d_out_affine);

/* A multi-scalar multiplication over the CALLER'S points: out_affine = sum_(i<n) scalars[i] * points_affine[i], with no bbg_srs and no
 * window tables (csrc/msm_points.hip; bbg_msm* needs a registered string and its precomputed tables).  points: 64-byte
 * Montgomery affine, any representative in [0, 2p) per coordinate; the affine encoding of infinity is accepted as data and contributes
 * nothing.  Points are NOT checked to be on the curve: for a point off it the result is unspecified (but nothing else is affected).
 * scalars: Montgomery Fr, any representative in [0, 2r).  out: ONE canonical Montgomery affine point of 64 bytes; a result at infinity is
 * written exactly as bbg_g1_fixed_base_mul writes it (bit 63 of x.data[3] set, every other bit zero).  n = 0 is legal and writes infinity.
 * The output being canonical, the order of the additions does not show: the result is a function of the inputs alone.
 *   window_bits   0 = automatic (a function of n alone, as measured on an MI355X: 4 up to 2^12 terms, 8 up to 2^15, 9 up to 2^17, 16
 *                 above), or a width c in 2 .. 16; anything else is BBG_E_INVALID.  windows(c) = ceil(128 / c) signed c-bit digits per
 *                 half scalar.  A forced width is taken as given and is not tuned for small n: from 14 bits (65536 buckets and
 *                 more) a bucket's run is summed by one lane, below by one whole wave, whatever n is, so a wide forced width over a few
 *                 hundred terms spends a wave and a search on every one-entry bucket.
 *   n             at most 2^28; more is BBG_E_INVALID.
 * Null pointers with n > 0 (and a null out always) are BBG_E_INVALID.  Each scalar is split against the cube root of unity into two
 * halves below 2^127 and recoded into signed digits; the 2 n windows(c) non-zero digits are grouped by bucket with a counting sort, the
 * buckets summed by mixed additions (a bucket longer than segment_entries is cut into segments summed by different lanes or waves, so
 * no input makes one lane's chain longer), and reduced per window by running sums.  Terms are walked in chunks of chunk_terms.  Working
 * memory: at most 1 GiB, 128 (2 B + 2 windows G + windows + E / segment_entries) + 16 (B + 1) + 8 E bytes (B = windows 2^(c-1) buckets,
 * G = 2^(c-1) / min(2^(c-1), 32) groups per window, E = 2 windows min(n, chunk_terms) entries) plus less than 2 KiB of alignment, counted
 * under `scratch` in bbg_memory_report and released by bbg_memory_trim.  Timed under "msm_points_sort", "msm_points_accumulate",
 * "msm_points_reduce", "msm_points_combine" (bbg_profile_get). */
int bbg_g1_msm(bbg_ctx* ctx, const uint64_t* points_affine, const uint64_t* scalars, size_t n, int window_bits, uint64_t out_affine[8]);
/* Device-resident: device pointers, asynchronous on the context stream, no host synchronisation once the working memory has its size.
 * That size depends on BOTH window_bits and n (the formula above): the buffer only grows, and a call that needs more than any call
 * before it -- a larger n, or another width, forced or automatic -- waits for the device once while the buffer is replaced; calls that
 * fit what is there only queue.  The inputs are left untouched.  An output that overlaps the points or the scalars is BBG_E_INVALID; every argument error is decided
 * before anything is queued. */
int bbg_g1_msm_device(bbg_ctx* ctx, const void* d_points_affine, const void* d_scalars, size_t n, int window_bits, void* d_out_affine);
/* What a call with these arguments would run with; a pure host function that needs no device and no context.  *c: the width used,
 * *windows: digits per half scalar, *chunk_terms: terms per chunk (a function of the width alone: 2^20, less where 1 GiB asks for it),
 * *segment_entries: the longest run of one bucket's entries that one lane (256, from 65536 buckets) or one wave (1024) sums.  Any out
 * pointer may be NULL.  BBG_E_INVALID for a window_bits or an n that the call would refuse. */
int bbg_g1_msm_plan(size_t n, int window_bits, int* c, int* windows, size_t* chunk_terms, size_t* segment_entries);

/* ---- G2 and batched pairing product checks over precomputed lines (csrc/pairing.hip, csrc/fq_tower.hip.h): for `count`
 *      independent products over the SAME `pairs` G2 points Q_j,
 *          e_i = prod_(j < pairs) e(P_ij, Q_j),        status_i = (e_i == 1),
 *      what pairing::reduced_ate_pairing_batch_precomputed (ecc/curves/bn254/pairing_impl.hpp:269-282) computes once per product.  In KZG
 *      verification the G2 points are fixed ([1]_2 and [x]_2 or [x^l]_2), so their line coefficients are computed once per handle and
 *      every product evaluates the same lines at its own G1 points: e(L, [x^l]_2) e(-R, [1]_2) = 1 is the check bbg_cells_verify_reduce
 *      leaves.  Layouts are the reference's, Montgomery form: fq2 = c0 | c1 (64 B), fq6 = c0 | c1 | c2, fq12 = c0 | c1 (384 B),
 *      g2::affine_element = x | y (128 B), pairing::miller_lines = 87 x (o | vw | vv) (16 704 B).  Fq inputs: any representative in
 *      [0, 2p) per Fq limb group; every output is canonical. ---- */
#define BBG_PAIRING_MAX_PAIRS 8
typedef struct bbg_g2_lines bbg_g2_lines;
/* out_affine[i] = [scalars[i]] B on the twist y^2 = x^3 + 3 / (9 + u), i < n: double-and-add, one lane per scalar (plumbing, not a hot
 * path: it makes [x^l]_2 and runs the subgroup test of bbg_g2_lines_prepare).  base_affine: one 128-byte point on the HOST, NULL =
 * g2::one, the generator; the affine encoding of infinity (below) is accepted and gives infinity.  A finite base that is not on the twist
 * is BBG_E_INVALID (n = 0 included) with out_affine untouched; it need not be in the order-r subgroup.  scalars: Montgomery Fr, any
 * representative in [0, 2r).  out: canonical 128-byte points; a result at infinity (scalar = 0 mod the point's order, or an infinite base)
 * is written in the reference's affine infinity encoding applied to x.c0: bit 63 of the top limb of x.c0 (word 3 of the 16) set, every
 * other bit of the 128 bytes zero.  All arrays are HOST arrays; the call is synchronous.  n is at most 2^16: more is BBG_E_INVALID.
 * n = 0 is legal; null scalars or out with n > 0 are BBG_E_INVALID. */
int bbg_g2_mul(bbg_ctx* ctx, const uint64_t* base_affine, const uint64_t* scalars, size_t n, uint64_t* out_affine);
/* The 87 line coefficients (precompute_miller_lines, pairing_impl.hpp:23-123) of `pairs` (1 .. BBG_PAIRING_MAX_PAIRS) G2 points, 128 bytes
 * each on the HOST, as a handle.  Every point must be finite, on the twist, and in the subgroup of order r: the subgroup test is [r] Q =
 * infinity, once per point (G2 has a cofactor, and a pairing check against a point outside the subgroup proves nothing).  A violation,
 * like a null argument or a bad `pairs`, is BBG_E_INVALID and leaves *out untouched.  The call synchronises.  The handle owns its
 * pairs x 16 704 bytes of device memory and keeps nothing of the caller's; it belongs to the context's device and may be used by any
 * context on that device.  Timed under "g2_lines" (bbg_profile_get). */
int bbg_g2_lines_prepare(bbg_ctx* ctx, const uint64_t* g2_affine, size_t pairs, bbg_g2_lines** out);
int bbg_g2_lines_pairs(const bbg_g2_lines* lines, size_t* pairs);
/* out (HOST, 16 704 bytes) = the lines of point `which` < pairs, bit for bit the canonical pairing::miller_lines that
 * precompute_miller_lines makes of it; synchronous. */
int bbg_g2_lines_read(const bbg_g2_lines* lines, size_t which, uint64_t* out);
void bbg_g2_lines_free(bbg_g2_lines* lines);
/* d_g1_affine: count x pairs Montgomery affine G1 points of 64 bytes, product i pairing point (i, j) at index i pairs + j with the
 * handle's point j.  The affine encoding of infinity is accepted as data: such a pair contributes the factor one and its lines are
 * skipped (L and R of bbg_cells_verify_reduce are both infinite when every polynomial has degree below l); a product whose pairs are all
 * infinite is one.  d_out_fq12 (may be NULL): count x 384 bytes, for finite inputs bit for bit the canonical form of
 * reduced_ate_pairing_batch_precomputed(P_i, lines, pairs).  d_status (may be NULL): count uint32 words,
 *     1   the product is one in Fq12
 *     0   it is not
 *     2   some finite G1 point of this product is not on y^2 = x^3 + 3; the Fq12 written for that product is unspecified and nothing
 *         else is affected.
 * BBG_E_INVALID with nothing queued: a null context, handle or d_g1_affine; both outputs null; count = 0 or above 2^24; a handle made on
 * another device; an output overlapping the input or the other output.
 * Queued on the context stream with no host synchronisation once the working memory has its size: 2308 bytes (six Fq12 values and one
 * flag word) per product for min(count, 2^16) products rounded up to a multiple of 64 -- at most 145 MiB; longer batches are walked in
 * chunks of 2^16.  The buffer only grows: a call that needs more than any call before waits for the device once.  It is counted under
 * `scratch` in bbg_memory_report and released by bbg_memory_trim.  Timed under "pairing_miller" (the Miller loop: 64 Fq12 squarings and
 * 87 sparse products per pair, one lane per product) and "pairing_final" (the final exponentiation) (bbg_profile_get). */
int bbg_pairing_product_device(bbg_ctx* ctx, const bbg_g2_lines* lines, const void* d_g1_affine, size_t count, void* d_out_fq12, void* d_status);
/* The same on HOST arrays (out_fq12: count x 48 words, status: count words; either may be NULL, not both); synchronous.  A status 2
 * anywhere returns BBG_E_INVALID after both outputs have been written, so the caller can see which product it was; every other error
 * leaves them untouched. */
int bbg_pairing_product(bbg_ctx* ctx, const bbg_g2_lines* lines, const uint64_t* g1_affine, size_t count, uint64_t* out_fq12, uint32_t* status);
/* The wave-cooperative form (csrc/pairing_wave.hip, csrc/fq12_wave.hip.h): exactly the contract of bbg_pairing_product_device -- the same
 * arguments, layouts, status words 1 / 0 / 2, infinity accepted as data, an all-infinite product is one, the same refusals and the same
 * count limit 1 .. 2^24 -- with ONE WAVE per product instead of one lane.  Every output is canonical, so the results are bit for bit those
 * of the lane form, whatever formulas run inside.  One launch (grid = count blocks of 64 threads) does the Miller loop and the final
 * exponentiation; the Fq12 lives in LDS in the w-basis, a product is 36 Fq2 products on 36 lanes, a sparse product 18, and no Fq12
 * operation but the one inversion has more than four dependent Fq products on its critical path.  It takes NO working memory: nothing is
 * grown, ctx's pairing buffer is not touched, and the call never synchronises the host.  Timed under "pairing_wave" (bbg_profile_get).
 *   Which form to call (profiles/pairing_wave.txt, one MI355X, pairs = 2): the wave form is the latency form, the lane form the
 * throughput form.  One check takes 1.85 ms here against 17.5 ms there (every wave sample below every lane sample); 1 024 checks 2.04
 * against 15.1 ms (one wave on every SIMD of the chip: the time is flat up to there), 4 096 checks 7.5 against 15.1 ms, and from 16 384
 * (28.7 against 15.2 ms; 2^16: 113 against 17.1 ms) the lane form is ahead, because the wave form spends about six times the instructions
 * per check and the lane form only fills the chip at 2^16.  4 096 is the largest measured count at which the wave form's median is
 * ahead, at four pairs as well (9.97 against 20.6 ms): call the wave form up to about 4 096 products and the lane form above.
 * Neither entry point dispatches to the other. */
int bbg_pairing_product_wave_device(bbg_ctx* ctx, const bbg_g2_lines* lines, const void* d_g1_affine, size_t count, void* d_out_fq12, void* d_status);
/* The same on HOST arrays, as bbg_pairing_product: synchronous, a status 2 anywhere returns BBG_E_INVALID after both outputs are written. */
int bbg_pairing_product_wave(bbg_ctx* ctx, const bbg_g2_lines* lines, const uint64_t* g1_affine, size_t count, uint64_t* out_fq12, uint32_t* status);

/* The NTT over G1 on plain arrays of points (no counterpart in the reference beyond the recursion inside transform_srs): with n = 2^log2n,
 * 1 <= log2n <= 28, and w_n = fr::get_root_of_unity(log2n), natural order in and out,
 *     out[k] = sum_j w_n^(j k) P_j            (inverse == 0)
 *     out[k] = n^-1 sum_j w_n^(-j k) P_j      (inverse != 0; what bbg_srs_lagrange computes, bit for bit).
 * points: 64-byte Montgomery affine, any representative in [0, 2p) per coordinate; the affine encoding of infinity is accepted.  Points are
 * not checked to be on the curve.  out: canonical Montgomery affine, and an output at infinity is DATA here, written exactly as
 * bbg_g1_fixed_base_mul writes it (bit 63 of x.data[3] set, every other bit zero) -- bbg_srs_lagrange, whose result must be an SRS, keeps
 * failing with BBG_E_INFINITY.  The working set, 128 bytes per point, is the context's (counted under `scratch` in bbg_memory_report,
 * released by bbg_memory_trim), as are the lanes' tables of bbg_g1_batch_mul under "ecntt_mul" = 1.  Null pointers and log2n outside
 * 1 .. 28 are BBG_E_INVALID.  Timed under "ecntt_stages" / "ecntt_normalize" (bbg_profile_get). */
int bbg_g1_ntt(bbg_ctx* ctx, const uint64_t* points_affine, unsigned log2n, int inverse, uint64_t* out_affine);
/* Device-resident: device pointers, asynchronous on the context stream, no host synchronisation once the working set has its size.
 * d_out_affine may BE d_points_affine. */
int bbg_g1_ntt_device(bbg_ctx* ctx, const void* d_points_affine, unsigned log2n, int inverse, void* d_out_affine);

/* ---- All openings at once: the KZG proofs of one polynomial at every point of its domain (Feist-Khovratovich, csrc/open_all.hip; no
 *      counterpart in the reference, whose compute_kate_opening_coefficients + pippenger gives one).  With n = 2^log2n, s_j the first n - 1
 *      points of an SRS and f = sum_(i<n) f_i X^i:
 *          out[m] = commitment over the s_j to (f(X) - f(w_n^m)) / (X - w_n^m),   m = 0 .. n-1
 *                 = sum_k w_n^(m k) h_k,   h_k = sum_(i=k+1)^(n-1) f_i s_(i-1-k)  (k <= n-2),  h_(n-1) = infinity.
 *      h is a Toeplitz product, taken as a cyclic convolution of length 2n: one Fr NTT, 2n point-scalar products, one inverse G1 NTT at
 *      2n, one forward G1 NTT at n -- instead of n calls of bbg_kate_opening_device + bbg_msm. ---- */
struct bbg_open_all; /* the handle; no typedef, because bbg_open_all is also the name of the host entry point below */
/* Prepares openings of polynomials of n = 2^log2n coefficients, 1 <= log2n <= 27, n <= bbg_srs_num_points(srs): reads the first n - 1
 * points of `srs` once, transforms them (a forward G1 NTT at 2n) and synchronises.  The handle keeps the context and NOTHING of the SRS:
 * freeing `srs` afterwards is legal.  It owns its device memory -- 2n x 64 B of transformed points, 2n x 128 B + n x 128 B of XYZZ
 * working arrays, 2n x 32 B of scalars: 576 n bytes, bbg_open_all_device_bytes -- which bbg_memory_report does not count and
 * bbg_memory_trim does not touch.  Null pointers, log2n outside 1 .. 27 and n above the SRS length are BBG_E_INVALID.  The SRS is NOT
 * required to be a powers string: the definition above holds for any points. */
int bbg_open_all_prepare(bbg_ctx* ctx, bbg_srs* srs, unsigned log2n, struct bbg_open_all** out);
/* Cells: one proof per coset of l = 2^log2cell domain points instead of one per point (the multi-proof half of Feist-Khovratovich; the
 * unit data-availability sampling opens).  With r = n / l and phi = w_n^l, cell m (m < r) is the coset w_n^m <w_n^r> = { w_n^(m + r t) :
 * t < l }, whose vanishing polynomial is X^l - phi^m, and with f = q_m (X^l - phi^m) + I_m, deg I_m < l,
 *     out[m] = commitment over the s_j to q_m = sum_(u=0)^(r-2) phi^(m u) h_u,   h_u = sum_(j=0)^(n-1-(u+1)l) f_(j+(u+1)l) s_j,
 * r proofs in natural order of m.  Over a powers string s_j = [x^j] G that is [(f(x) - I_m(x)) / (x^l - phi^m)] G.  The checks are those
 * of bbg_open_all_prepare, plus log2cell <= log2n - 1 (at least two cells); a violation is BBG_E_INVALID and leaves *out as it was.
 * log2cell = 0 IS bbg_open_all_prepare.  For log2cell >= 1 the points s_0 .. s_(n-l-1) are read, once, and the call synchronises: `srs`
 * may be freed at once.  The handle holds l G1 transforms at 2r of the string's residue classes, and a call then runs G1 transforms at 2r
 * and r instead of 2n and n.  Its memory: 2n x 64 B of transformed points, 2n x 128 B of products, 2n x 32 B of scalars, 2r x 128 B +
 * r x 128 B of working arrays (bbg_open_all_device_bytes), outside bbg_memory_report like the all-points handle's.
 *   The VALUES of cell m are f(w_n^(m + r t)), t < l: bbg_ntt(BBG_FFT) of the n coefficients, read at index m with stride r.
 * bbg_cells_values writes them cell by cell, and bbg_cells_recover gives the coefficients back from any K of the r cells (below).
 * Verification: bbg_cells_verify_reduce (below) reduces any batch of cell proofs to two G1 points L, R with e(L, [x^l]_2) = e(R, [1]_2)
 * iff every proof is valid.  The caller still owes that one two-pair pairing against [x^l]_2 (bbg_g2_mul makes the point, bbg_pairing_product the check), and
 * the choice of the challenge rho. */
int bbg_open_all_prepare_cells(bbg_ctx* ctx, bbg_srs* srs, unsigned log2n, unsigned log2cell, struct bbg_open_all** out);
/* The number of proofs a call writes: n >> log2cell (n for a handle of bbg_open_all_prepare). */
int bbg_open_all_count(const struct bbg_open_all* h, size_t* proofs);
/* d_coeffs: n Montgomery Fr coefficients on the device (any representative in [0, 2r)), read only; f_0 is never read.  d_out_affine:
 * n x 64 B canonical Montgomery affine; a proof at infinity (every one of a constant f) is written as bbg_g1_ntt writes it.  Asynchronous
 * on the context stream, no host synchronisation; calls through one handle are ordered by that stream and share its working arrays.
 * Timed under "open_all_coeffs", "ntt_pass", "open_all_pointwise", "ecntt_stages", "open_all_fold", "ecntt_normalize".
 * A cell handle writes bbg_open_all_count proofs, (n >> log2cell) x 64 B, never reads f_0 .. f_(l-1) (every proof of a polynomial of
 * degree below l is the point at infinity), and is also timed under "open_cells_sum". */
int bbg_open_all_device(struct bbg_open_all* h, const void* d_coeffs, void* d_out_affine);
/* Host arrays; returns when the proofs are in out_affine. */
int bbg_open_all(struct bbg_open_all* h, const uint64_t* coeffs, uint64_t* out_affine);
/* Many polynomials per call, on either kind of handle.  One call of bbg_open_all_device is a chain of dependent G1 stages over few points
 * (13 launches at (log2n, log2cell) = (12, 6)) and leaves the device idle; the batched call runs the same chain once over `count`
 * polynomials.  out[p] is, bit for bit, what bbg_open_all writes for polynomial p alone.
 * bbg_open_all_batch_reserve: the handle's batch workspace for `polys` polynomials at a time -- `polys` copies of the single call's working
 * arrays (bbg_open_all_device_bytes less the 2n x 64 B of transformed points, each), owned by the handle beside the buffers of the single
 * calls, which keep theirs.  `polys` above the cap -- the largest number whose workspace stays within 1 GiB, at least 1 -- reserves the
 * cap; 0 releases the workspace.  Replacing or releasing a reservation waits for the device.  BBG_E_NOMEM when the allocation fails: the
 * handle then has no reservation and still serves single calls.
 * bbg_open_all_batch_device: d_coeffs = count x 2^log2n Montgomery Fr (any representative in [0, 2r)), polynomial p at p * 2^log2n, read
 * only; d_out_affine = count x proofs x 64 B canonical Montgomery affine, polynomial-major, proofs = bbg_open_all_count.  The call walks
 * its polynomials in chunks of the reservation; on a handle without one it first reserves min(count, the cap).  Asynchronous on the
 * context stream, no host synchronisation (but for that first reservation's allocation).  Timed under the names of bbg_open_all_device;
 * "ntt_pass" covers the batched Fr transforms.  A null pointer or count = 0 is BBG_E_INVALID. */
int bbg_open_all_batch_reserve(struct bbg_open_all* h, size_t polys);
int bbg_open_all_batch_device(struct bbg_open_all* h, const void* d_coeffs, size_t count, void* d_out_affine);
/* Host arrays; returns when the count x proofs proofs are in out_affine. */
int bbg_open_all_batch(struct bbg_open_all* h, const uint64_t* coeffs, size_t count, uint64_t* out_affine);

/* ---- cells as data: the values of every cell of a polynomial, and the polynomial back from a subset of its cells (erasure decoding; the
 *      consumer side of the cell handle above, pure Fr work).  n = 2^log2n, l = 2^log2cell, r = n / l, cell m < r = { w_n^(m + r t) : t < l }.
 *      Shared by all four: Montgomery Fr, every input any representative in [0, 2r_mod), every output canonical; 1 <= log2n <= 28,
 *      0 <= log2cell <= log2n - 1, 1 <= count <= 32 polynomials per call, laid out one after the other.  A null pointer, a value out of
 *      range or an overlap of input and output is BBG_E_INVALID: nothing is queued and the output stays untouched.  The device entries
 *      queue on the context stream and do not synchronise the host once the working memory (`scratch` in bbg_memory_report, released by
 *      bbg_memory_trim) and the domain's tables have their size.  Timed under "cells_gather" (values), "cells_z", "cells_scatter",
 *      "cells_divide", "cells_canon" (recovery), beside "ntt_pass" and "fr_batch_invert". ---- */
/* d_out[p n + m l + t] = f_p(w_n^(m + r t)): cell-major, cell m contiguous.  d_coeffs: count x n coefficients, read only; d_out: count x n
 * values, no overlap with d_coeffs.  One forward transform per polynomial, then a transposition. */
int bbg_cells_values_device(bbg_ctx* ctx, const void* d_coeffs, unsigned log2n, unsigned log2cell, size_t count, void* d_out);
/* Host-buffer form: upload, compute, download; synchronous. */
int bbg_cells_values(bbg_ctx* ctx, const uint64_t* coeffs, unsigned log2n, unsigned log2cell, size_t count, uint64_t* out);
/* The unique polynomial of degree < K l through K cells.  cell_ids: HOST array of K distinct cell indices below r, 1 <= K <= r, in any
 * order, read before the call returns; every polynomial of the call has the same cells.  d_values: count x K x l values, cell k of
 * polynomial p at (p K + k) l in bbg_cells_values' order within the cell.  d_out_coeffs: count x n coefficients, no overlap with d_values;
 * coefficients K l .. n - 1 are exactly zero.  There is no 50 % rule: a caller whose polynomial has degree < n / 2 passes any K >= r / 2
 * cells and gets it back; values that lie on no polynomial of the caller's degree bound show as non-zero coefficients above that bound.
 * Cost: three Fr transforms at n per polynomial and, once per call, 2 r products of r - K factors (log2cell = 0, interpolation from
 * single points, is legal and quadratic in the number of missing points). */
int bbg_cells_recover_device(bbg_ctx* ctx, const uint32_t* cell_ids, size_t K, const void* d_values, unsigned log2n, unsigned log2cell, size_t count,
                             void* d_out_coeffs);
/* Host-buffer form: upload, compute, download; synchronous. */
int bbg_cells_recover(bbg_ctx* ctx, const uint32_t* cell_ids, size_t K, const uint64_t* values, unsigned log2n, unsigned log2cell, size_t count,
                      uint64_t* out_coeffs);
/* ---- a batch of cell proofs reduced to ONE pairing check (csrc/cells_verify.hip): everything a verifier of cell proofs computes in G1 and
 *      Fr, up to the pairing, which is bbg_pairing_product's (above).  A batch has ncom commitments C_c and K cells; cell k < K carries a commitment index
 *      commitment_ids[k] < ncom, a cell index cell_ids[k] < r, the l values of that cell at values[k l .. k l + l) in bbg_cells_values'
 *      order within the cell, and a proof pi_k (what bbg_open_all_device writes for that cell).  With I_k the interpolant of degree < l
 *      through the values, s_b the first l points of `srs` and rho the caller's challenge, the call writes
 *          L = sum_k rho^k pi_k
 *          R = sum_k rho^k ( C_(c_k) - sum_(b<l) I_k,b s_b + phi^(m_k) pi_k )
 *      and over a powers string every proof is valid iff (with overwhelming probability over rho) e(L, [x^l]_2) = e(R, [1]_2): one
 *      two-pair pairing whatever K is.  rho must be unpredictable to whoever made the proofs (Fiat-Shamir over the whole batch is the
 *      caller's business); rho^0 = 1 also for rho = 0.  log2cell = 0 is batched verification of single-point openings (bbg_open_all's
 *      proofs, the values those of bbg_ntt).  The coefficients of sum_k rho^k I_k cost ONE inverse transform at n, not one per cell: they
 *      are r times the first l coefficients of iNTT_n of the rho-weighted values laid out in domain order.
 *        Conventions: Fr inputs (values, rho) Montgomery, any representative in [0, 2r_mod); points 64-byte Montgomery affine, any
 *      representative in [0, 2p) per coordinate, the affine encoding of infinity accepted as data (every proof of a polynomial of degree
 *      < l, the commitment of the zero polynomial).  out: L then R, canonical affine; an output at infinity is written exactly as bbg_g1_ntt
 *      writes it.  Duplicate (commitment, cell) pairs are legal, and so are commitments no cell refers to.  The reduction is a function of
 *      its inputs, valid or not.
 *        Curve check: every finite commitment and proof is tested against y^2 = x^3 + 3 as it is loaded (a verifier that accepts points off
 *      the curve is unsound).  The device form writes the number that fail to *d_off_curve (uint32) when that is not NULL; L and R are
 *      then unspecified, but nothing else is affected.  The host form returns BBG_E_INVALID for a non-zero count and leaves `out` untouched.
 *        BBG_E_INVALID with nothing queued and the outputs untouched: a null pointer (d_off_curve excepted), K = 0, ncom = 0, K or ncom
 *      above 2^30, an id out of range, log2n outside 1 .. 28, log2cell > log2n - 1, l above the SRS length, an SRS on another device, an
 *      output that overlaps an input or the other output.  The id arrays are HOST arrays, read before the call returns.  The device form
 *      queues on the context stream and does not synchronise the host once the working memory has its size: 32 n + 256 r + 160 (K + ncom)
 *      bytes and the group lists in the cells buffer, the lanes' tables of bbg_g1_batch_mul (both `scratch` in bbg_memory_report, released
 *      by bbg_memory_trim), the domain's tables and the MSM's arena.  Timed under "cells_verify_powers", "cells_verify_fold",
 *      "cells_verify_mul", "cells_verify_segsum", "cells_verify_phi", "cells_verify_finish", beside "ntt_pass" and the MSM's names. ---- */
int bbg_cells_verify_reduce_device(bbg_ctx* ctx, bbg_srs* srs, unsigned log2n, unsigned log2cell, const void* d_commitments, size_t ncom,
                                   const uint32_t* commitment_ids, const uint32_t* cell_ids, size_t K, const void* d_values, const void* d_proofs,
                                   const uint64_t rho[4], void* d_out, void* d_off_curve);
/* Host-buffer form: upload, compute, download; synchronous. */
int bbg_cells_verify_reduce(bbg_ctx* ctx, bbg_srs* srs, unsigned log2n, unsigned log2cell, const uint64_t* commitments, size_t ncom,
                            const uint32_t* commitment_ids, const uint32_t* cell_ids, size_t K, const uint64_t* values, const uint64_t* proofs,
                            const uint64_t rho[4], uint64_t out[16]);
/* The verdict in one call: the reduction above, then e(L, [x^l]_2) e(-R, [1]_2) = 1, with no host round trip in between.  `lines` is a
 * bbg_g2_lines handle of exactly two points, ([x^l]_2, [1]_2) in that order (bbg_g2_mul makes [x^l]_2); every other argument is
 * bbg_cells_verify_reduce_device's.  *d_status (one uint32 on the device) becomes
 *     1   every proof is valid under this rho
 *     0   not
 *     2   the reduction counted a finite commitment or proof off the curve, whatever the pairing then says.
 * The call queues four steps on the context stream -- the reduction, a pack kernel that writes [L, -R] (the negation canonical: p - y;
 * infinity stays as it is and so does y = 0), bbg_pairing_product_wave_device at count 1, the status word -- and does not synchronise the
 * host once the reduction's working memory has its size.  L, R, the packed pair, the off-curve count and the pairing's own status word
 * live in 512 bytes of the context (`scratch` in bbg_memory_report, released by bbg_memory_trim), which every call on the context shares:
 * calls are ordered on the context stream, each writes its verdict to its OWN d_status as its last step, and so any number of calls may be
 * queued back to back and read after one synchronisation.
 *   BBG_E_INVALID with nothing queued and *d_status untouched: a null pointer, a handle with another pair count than two or made on
 * another device, a status word that overlaps an input, and every refusal of bbg_cells_verify_reduce_device.  Timed under the
 * reduction's names, "cells_verify_pack" (the pack kernel and the status word) and "pairing_wave". */
int bbg_cells_verify_device(bbg_ctx* ctx, bbg_srs* srs, const bbg_g2_lines* lines, unsigned log2n, unsigned log2cell, const void* d_commitments, size_t ncom,
                            const uint32_t* commitment_ids, const uint32_t* cell_ids, size_t K, const void* d_values, const void* d_proofs,
                            const uint64_t rho[4], void* d_status);
/* Host-buffer form: upload, the device form, download; synchronous.  Status 2 returns BBG_E_INVALID with *status written; every other
 * error leaves it untouched. */
int bbg_cells_verify(bbg_ctx* ctx, bbg_srs* srs, const bbg_g2_lines* lines, unsigned log2n, unsigned log2cell, const uint64_t* commitments, size_t ncom,
                     const uint32_t* commitment_ids, const uint32_t* cell_ids, size_t K, const uint64_t* values, const uint64_t* proofs,
                     const uint64_t rho[4], uint32_t* status);
/* The handle's device memory: its own buffers plus the batch workspace it holds at the moment (none before the first reservation or
 * batched call, and none after bbg_open_all_batch_reserve(h, 0)). */
int bbg_open_all_device_bytes(const struct bbg_open_all* h, size_t* bytes);
/* Releases the handle and its device memory (a device synchronisation); must precede bbg_destroy of its context. */
void bbg_open_all_free(struct bbg_open_all* h);

/* ---- NTT family: replaces polynomial_arithmetic::fft/ifft/coset_fft/coset_ifft/... on fr* coeffs
 *      (polynomials/polynomial_arithmetic.cpp:374-484) and the C bindings coset_fft_with_generator_shift / ifft
 *      (plonk/proof_system/prover/c_bind.cpp:59-76). ----------------------------------------------------------- */
enum {
    BBG_FFT = 0,                             /* fft                            :374 */
    BBG_IFFT = 1,                            /* ifft                           :379 */
    BBG_COSET_FFT = 2,                       /* coset_fft(coeffs, domain)      :395 */
    BBG_COSET_IFFT = 3,                      /* coset_ifft                     :480 */
    BBG_FFT_WITH_CONSTANT = 4,               /* fft_with_constant              :387 */
    BBG_COSET_FFT_WITH_CONSTANT = 5,         /* coset_fft_with_constant        :458 */
    BBG_COSET_FFT_WITH_GENERATOR_SHIFT = 6,  /* coset_fft_with_generator_shift :465 */
    BBG_IFFT_WITH_CONSTANT = 7               /* ifft_with_constant             :471 */
};
/* In place on coeffs[2^log2n] (Montgomery Fr, natural order in and out).  generator_size = evaluation_domain::
 * generator_size (0 = whole domain): coset_fft scales only the first generator_size coefficients by g^j
 * (polynomial_arithmetic.cpp:397, proving_key.cpp:21-22).  constant: Montgomery Fr for ops 4-7, else NULL.
 * The per-size twiddle tables (evaluation_domain::compute_lookup_table) are built on first use and cached.
 * log2n <= 28, the 2-adicity of BN254 Fr (fr.hpp:27-30); every size up to 2^28 is checked against the reference's digests
 * (tests/golden/ntt_large.json: 2^25 .. 2^28 in round 6; the tables of a 2^28 domain take 5 x 32 n bytes = 40 GiB of HBM). */
int bbg_ntt(bbg_ctx* ctx, uint64_t* coeffs, unsigned log2n, int op, size_t generator_size, const uint64_t* constant);
int bbg_ntt_device(bbg_ctx* ctx, void* d_coeffs, unsigned log2n, int op, size_t generator_size, const uint64_t* constant);
/* Pre-builds the tables for a domain size (outside any timed region, like compute_lookup_table()). */
int bbg_ntt_prepare(bbg_ctx* ctx, unsigned log2n);
/* How a 2^log2n transform runs NOW (options included), without building anything: *passes = kernel launches per transform, log_radix[q] =
 * log2 of pass q's radix (0 beyond the last pass), *tile_log = log2 elements per tile, *kernel = the pass kernel: 0 k_ntt_pass (radix 2 in LDS,
 * n < 2^11), 8 k_ntt_pass8, 81 k_ntt_pass8s (one-plane exchange), 29 k_ntt_pass29 (9 x 29-bit limbs).  What bench.py labels its NTT roofline with. */
int bbg_ntt_plan(bbg_ctx* ctx, unsigned log2n, int* passes, int log_radix[4], int* kernel, int* tile_log);
/* coset_fft(coeffs, small_domain, large_domain, ext) (:401-456): coeffs holds 2^log2n coefficients in a buffer of
 * ext * 2^log2n elements; result interleaves ext size-n coset FFTs at index ext*i + k. */
int bbg_coset_fft_split(bbg_ctx* ctx, uint64_t* coeffs, unsigned log2n, size_t ext);
int bbg_coset_fft_split_device(bbg_ctx* ctx, void* d_coeffs, unsigned log2n, size_t ext);
/* The prover's FFT work item as ONE call (work_queue.hpp:252-264, WorkType::FFT): copy the 2^log2n coefficients of a wire
 * into a zeroed domain of 2^log2_domain elements, coset_fft over that domain with generator_size = 2^log2n, and append
 * the first four results (polynomial::add_lagrange_base_coefficient x4).  coeffs: 2^log2n elements (read only);
 * out: 2^log2_domain + 4 elements.  Uploads n elements instead of 4n and spares the host the 4n copy / zero fill. */
int bbg_coset_fft_extend(bbg_ctx* ctx, const uint64_t* coeffs, unsigned log2n, unsigned log2_domain, uint64_t* out);

/* ---- building blocks of an NTT sharded across GPUs by residue class (aztec-2.0_amd/parallel.py::ntt_sharded; the
 *      reference's precedent is the 4-way coset split, work_queue.hpp:166-199, polynomial_arithmetic.cpp:401-456) ---- */
/* a[j] *= start * base^j, j < count (start may be NULL = 1); base/start Montgomery Fr on the host. */
int bbg_scale_powers_device(bbg_ctx* ctx, void* d_a, size_t count, const uint64_t* start, const uint64_t* base);
/* out = w_n^e for the 2^log2n domain (inverse != 0: w_n^-e); out = base^e. */
int bbg_fr_root_pow(bbg_ctx* ctx, unsigned log2n, uint64_t e, int inverse, uint64_t out[4]);
int bbg_fr_pow(bbg_ctx* ctx, const uint64_t base[4], uint64_t e, uint64_t out[4]);
/* out[t*len + q] = sum_{s<G} w_G^(s*t) in[s*len + q], G = 2^log2G <= 8, w_G = w_n^(n/G): the cross-rank DFT after the
 * all-to-all exchange. */
int bbg_cross_dft_device(bbg_ctx* ctx, const void* d_in, void* d_out, unsigned log2G, size_t len, unsigned log2n, int inverse);

/* ---- polynomial helpers between the NTTs and the MSMs, on device-resident Montgomery Fr arrays ----
 * polynomial_arithmetic::add / sub / mul (polynomials/polynomial_arithmetic.cpp:486-505): r[i] = a[i] (op) b[i], op = 0 add,
 * 1 sub, 2 mul; r may alias a or b. */
int bbg_poly_op_device(bbg_ctx* ctx, int op, const void* d_a, const void* d_b, void* d_r, size_t n);
/* out[i] = base[i] + sum_k polys[k][i] * scalars[k], k < count <= 32 (base may be NULL = 0; out may alias base): the
 * accumulation of the opening polynomials in KateCommitmentScheme::batch_open (kate_commitment_scheme.cpp:216-226).
 * d_polys: host array of device addresses; scalars: count Montgomery Fr on the host. */
int bbg_poly_linear_combination_device(bbg_ctx* ctx, const void* const* d_polys, const uint64_t* scalars, size_t count, const void* d_base,
                                       void* d_out, size_t n);
/* polynomial_arithmetic::evaluate (:507-538): out = sum_i coeffs[i] z^i (canonical Montgomery).  Synchronous. */
int bbg_poly_evaluate_device(bbg_ctx* ctx, const void* d_coeffs, size_t n, const uint64_t z[4], uint64_t out[4]);
/* polynomial_arithmetic::compute_kate_opening_coefficients (:727-750): dest = coefficients of (F(X) - F(z)) / (X - z),
 * f_out = F(z).  dest must not alias src.  Synchronous. */
int bbg_kate_opening_device(bbg_ctx* ctx, const void* d_src, void* d_dest, size_t n, const uint64_t z[4], uint64_t f_out[4]);
/* polynomial_arithmetic::divide_by_pseudo_vanishing_polynomial (:628-725): in place on the 2^log2_target coset evaluations;
 * src domain 2^log2_src, num_roots_cut roots cut out of the vanishing polynomial (the reference default is 4). */
int bbg_divide_by_pseudo_vanishing_device(bbg_ctx* ctx, void* d_evals, unsigned log2_src, unsigned log2_target, size_t num_roots_cut);

/* Host-buffer forms of the three helpers above (what the C++ shim binds polynomial_arithmetic::evaluate,
 * compute_kate_opening_coefficients and divide_by_pseudo_vanishing_polynomial to): upload, compute, download; synchronous.
 * bbg_kate_opening: dest may alias src, as the prover calls it (kate_commitment_scheme.cpp:231-235). */
int bbg_poly_evaluate(bbg_ctx* ctx, const uint64_t* coeffs, size_t n, const uint64_t z[4], uint64_t out[4]);
int bbg_kate_opening(bbg_ctx* ctx, const uint64_t* src, uint64_t* dest, size_t n, const uint64_t z[4], uint64_t f_out[4]);
int bbg_divide_by_pseudo_vanishing(bbg_ctx* ctx, uint64_t* evals, unsigned log2_src, unsigned log2_target, size_t num_roots_cut);

/* ---- polynomials in LAGRANGE form: n = 2^log2n values f_i = F(w^i) on the domain, w = fr::get_root_of_unity(log2n) = bbg_fr_root_pow(log2n, 1),
 *      natural order -- the form bbg_srs_lagrange commits to.  These evaluate and open such a polynomial where it lies, without an iFFT.
 *      Shared by all: Montgomery Fr, every input any representative in [0, 2r) (r itself is a zero), every output canonical;
 *      1 <= log2n <= 28, 1 <= count <= 32; a null pointer, or a count or log2n out of range, is BBG_E_INVALID and nothing is written.
 *      Timed under "fr_batch_invert" / "barycentric" (bbg_profile_get); the partial sums live in the evaluation scratch (`scratch` in
 *      bbg_memory_report, released by bbg_memory_trim). ---- */
/* fr::batch_invert (ecc/fields/field_impl.hpp:331-359): out[i] = in[i]^-1, zero stays zero.  d_out may BE d_in; any other overlap of the two
 * is BBG_E_INVALID.  n = 0 does nothing.  One real inversion per 1024 elements (Montgomery's trick).  Asynchronous on the context stream. */
int bbg_fr_batch_invert_device(bbg_ctx* ctx, const void* d_in, void* d_out, size_t n);
/* polynomial_arithmetic::compute_barycentric_evaluation (polynomials/polynomial_arithmetic.cpp:811-847) for `count` polynomials in one pass:
 * out[k] = F_k(z), or F_k(z * w) where shifted[k] != 0 (shifted may be NULL), from F(z) = (z^n - 1)/n * sum_i f_i / (z w^-i - 1); the shifted
 * form uses the same weights and reads the values one place further on.  d_evals: host array of `count` device addresses.
 * Two deliberate differences from the reference: (1) the shifted value is the mathematical F(z * w) -- the reference's Lagrange branch passes
 * zeta where it means the shifted point (kate_commitment_scheme.cpp:429), its coefficient branch two lines below computes F(z * w), which is
 * what a verifier needs; (2) z ON the domain, z = w^j, is answered exactly, F(z) = f_j and F(z w) = f_{(j+1) mod n} -- the reference's
 * batch_invert skips the zero denominator and returns a wrong sum.  Synchronous: one host synchronisation, like bbg_poly_evaluate_device. */
int bbg_poly_evaluate_lagrange_device(bbg_ctx* ctx, const void* const* d_evals, const int* shifted, size_t count, unsigned log2n,
                                      const uint64_t z[4], uint64_t* out /* count x 4 limbs */);
/* Host-buffer form for ONE polynomial (what a shim would bind compute_barycentric_evaluation to): upload, evaluate at z, synchronous. */
int bbg_poly_evaluate_lagrange(bbg_ctx* ctx, const uint64_t* evals, unsigned log2n, const uint64_t z[4], uint64_t out[4]);
/* The Kate opening quotient in evaluation form: d_dest[i] = W(w^i) = w^-i (F(z) - f_i) / (z w^-i - 1) for W(X) = (F(X) - F(z)) / (X - z), f_out = F(z);
 * the inverse NTT of d_dest is what bbg_kate_opening_device gives for F's coefficients (top coefficient zero).  d_dest holds n values and must
 * not overlap d_evals (BBG_E_INVALID).  For z on the domain (z^n = 1) W(w^j) would need a derivative: BBG_E_INVALID, decided on the host before
 * anything is queued, d_dest untouched.  Synchronous. */
int bbg_kate_opening_lagrange_device(bbg_ctx* ctx, const void* d_evals, void* d_dest, unsigned log2n, const uint64_t z[4], uint64_t f_out[4]);

/* ---- many Lagrange-form polynomials opened in ONE call, each at its OWN point (csrc/open_points.hip): the
 *      compute_blob_kzg_proof of a blob library for a whole batch, and the last step of a PLONK prover.  d_evals holds `count` polynomials of
 *      n = 2^log2n values each, contiguous and polynomial-major; d_z holds `count` points ON THE DEVICE (a Fiat-Shamir point computed there
 *      never visits the host; z_k^n is log2n squarings in a kernel).  For every k < count
 *          y[k]      = F_k(z_k)
 *          proofs[k] = [ (F_k(X) - y_k) / (X - z_k) ]  committed over `lagrange`
 *      `lagrange` must be a string in LAGRANGE form, which is what bbg_srs_lagrange returns; the call cannot tell whether it is, and over
 *      any other string the proofs are commitments to something else.  Conventions of the Lagrange-form calls above: Montgomery Fr, every
 *      input any representative in [0, 2r), y canonical; the proofs canonical affine, a proof at infinity (a constant polynomial) written
 *      exactly as bbg_g1_ntt writes it.  d_proofs == NULL asks for the values only: `lagrange` may then be NULL, and no quotient and no MSM
 *      is queued -- the y_k = F_k(z_k) step of a batch verifier.
 *        A point ON the domain, z_k = w^m, is answered exactly, per polynomial (a batch may mix such polynomials with others): y_k = f_m, and
 *      the quotient's value at w^m follows from the vanishing top coefficient of the quotient, q_m = - w^-m sum_(i != m) (f_m - f_i) /
 *      (z w^-i - 1); no derivative is taken.  (bbg_kate_opening_lagrange_device keeps its documented refusal.)
 *        1 <= log2n <= 28, 1 <= count <= 2^20.  BBG_E_INVALID with nothing queued and the outputs untouched: a null pointer other than the
 *      two optional ones, log2n or count out of range, a string shorter than n or on another device than the context, an output that
 *      overlaps an input or the other output.  The device form queues on the context stream only and does not synchronise the host once
 *      the working memory has its size.  One launch per stage covers ALL polynomials of a chunk; the commitments go through the batched MSM,
 *      BBG_MSM_BATCH_MAX polynomials per launch set.
 *        Working memory: a chunk of c polynomials takes c (32 n + 64 ceil(n / 1024) + 160) bytes with proofs -- the quotient values, two
 *      partial sums per inversion group of 1024 points, a slot for q_m, the MSM's Jacobian result, a flag -- and c (64 ceil(n / 1024) + 160)
 *      without; it is counted under `scratch` in bbg_memory_report, released by bbg_memory_trim, and only grows.  c is what fits the budget
 *      (1 GiB; bbg_open_points_set_budget), rounded down to a multiple of BBG_MSM_BATCH_MAX (at least one polynomial), and at most count;
 *      a call with more polynomials walks them in chunks of c.  Beside it: the domain's constants and the MSM's arena.
 *      Timed under "open_points_weights" (weights, partial sums, values), "open_points_quotient", "open_points_normalize" and the MSM's
 *      names. ---- */
int bbg_open_points_device(bbg_ctx* ctx, bbg_srs* lagrange, unsigned log2n, const void* d_evals /* count x n Fr */, const void* d_z /* count Fr, DEVICE */,
                           size_t count, void* d_y /* count Fr */, void* d_proofs /* count x 64 B, or NULL */);
/* Host-buffer form: upload, compute, download; synchronous.  proofs may be NULL (and `lagrange` then too). */
int bbg_open_points(bbg_ctx* ctx, bbg_srs* lagrange, unsigned log2n, const uint64_t* evals, const uint64_t* z, size_t count, uint64_t* y, uint64_t* proofs);
/* The bytes a chunk's working memory may take from the next call on (0 = the default, 1 GiB; at most 2^36).  A smaller budget means more,
 * smaller chunks and the same results; memory already held is kept until bbg_memory_trim. */
int bbg_open_points_set_budget(bbg_ctx* ctx, size_t bytes);

/* ---- a batch of openings at ARBITRARY points reduced to ONE pairing check (csrc/kzg_verify.hip): the
 *      verify_blob_kzg_proof_batch of a blob library, the last step of a batch of PLONK verifiers.  Opening i < N is a commitment C_i, a
 *      point z_i, a claimed value y_i and a proof pi_i (what bbg_open_points writes).  With rho the caller's challenge and G = (1, 2)
 *          L = sum_i rho^i pi_i
 *          R = sum_i rho^i ( C_i - [y_i] G + [z_i] pi_i )
 *      and over a powers string every opening is valid iff (with overwhelming probability over rho) e(L, [x]_2) = e(R, [1]_2).  No SRS takes
 *      part.  One commitment per opening: repeating a commitment (one polynomial at several points) is legal, and so is repeating a point.
 *      rho must be unpredictable to whoever made the proofs; rho^0 = 1 also for rho = 0.
 *        Conventions, the curve check, the meaning of *d_off_curve and of the status word, and infinity as data are bbg_cells_verify_reduce's
 *      and bbg_cells_verify's (above): Montgomery Fr in [0, 2r), points 64-byte Montgomery affine in [0, 2p) per coordinate, L then R
 *      canonical affine with infinity as bbg_g1_ntt writes it; every finite commitment and proof is tested against y^2 = x^3 + 3 as it is
 *      loaded, the number that fail goes to *d_off_curve (uint32, may be NULL), and L and R are then unspecified.  The host form returns
 *      BBG_E_INVALID for a non-zero count and leaves `out` untouched.
 *        1 <= N <= 2^27.  BBG_E_INVALID with nothing queued and the outputs untouched: a null pointer (d_off_curve excepted), N out of
 *      range, an output that overlaps an input or the other output.  The device form queues on the context stream -- the powers of rho, one
 *      kernel that packs the points [C | pi | G] and the scalars [rho^i | rho^i z_i | - sum rho^i y_i], and bbg_g1_msm_device's steps twice:
 *      over the 2 N + 1 packed terms for R, over the proofs for L -- and does not synchronise the host once the working memory has its
 *      size: 96 (2 N + 1) + 32 N + 128 KiB bytes of its own and the working memory of bbg_g1_msm (both `scratch` in bbg_memory_report,
 *      released by bbg_memory_trim).  Timed under "kzg_verify_prepare" and bbg_g1_msm's names. ---- */
int bbg_kzg_verify_reduce_device(bbg_ctx* ctx, const void* d_commitments /* N x 64 B */, const void* d_z, const void* d_y, const void* d_proofs, size_t N,
                                 const uint64_t rho[4], void* d_out /* L, R */, void* d_off_curve /* uint32 or NULL */);
/* Host-buffer form: upload, compute, download; synchronous. */
int bbg_kzg_verify_reduce(bbg_ctx* ctx, const uint64_t* commitments, const uint64_t* z, const uint64_t* y, const uint64_t* proofs, size_t N,
                          const uint64_t rho[4], uint64_t out[16]);
/* The verdict in one call: the reduction above into the context's 512 bytes, then bbg_cells_verify_device's own last three steps ([L, -R]
 * packed, bbg_pairing_product_wave_device at count 1, the status word), with no host round trip.  `lines`: a handle of exactly two points,
 * ([x]_2, [1]_2) in that order.  *d_status (uint32): 1 every opening is valid under this rho, 0 not, 2 a finite commitment or proof is off
 * the curve.  Calls may be queued back to back and read after one synchronisation, each writes its OWN d_status as its last step.
 * BBG_E_INVALID with nothing queued and *d_status untouched: a null pointer, a handle with another pair count than two or made on another
 * device, a status word that overlaps an input, and every refusal of the reduction.  Timed under the reduction's names, "cells_verify_pack"
 * and "pairing_wave". */
int bbg_kzg_verify_device(bbg_ctx* ctx, const bbg_g2_lines* lines, const void* d_commitments, const void* d_z, const void* d_y, const void* d_proofs, size_t N,
                          const uint64_t rho[4], void* d_status);
/* Host-buffer form: upload, the device form, download; synchronous.  Status 2 returns BBG_E_INVALID with *status written; every other
 * error leaves it untouched. */
int bbg_kzg_verify(bbg_ctx* ctx, const bbg_g2_lines* lines, const uint64_t* commitments, const uint64_t* z, const uint64_t* y, const uint64_t* proofs, size_t N,
                   const uint64_t rho[4], uint32_t* status);

/* ---- wire forms: G1 points and scalars as they cross a network or sit in a proof, decoded to and encoded from the native form of every
 *      other entry point, on the device (csrc/wire.hip).  Paths relative to barretenberg/src/aztec/.  q is the modulus of Fq,
 *      r that of Fr.
 *        Native side: exactly what the other calls take and give.  G1: 64-byte Montgomery affine x || y.  Decode writes canonical
 *      coordinates and writes infinity as bbg_g1_ntt does (bit 63 of x.data[3] set, every other bit zero); encode accepts any representative in
 *      [0, 2q) per coordinate and that infinity encoding as data.  Fr: 32-byte Montgomery; decode writes it canonical, encode accepts [0, 2r).
 *        Compressed forms (32 B): for a finite point the word is, bit for bit, the reference's uint256_t(P) (affine_element::operator uint256_t,
 *      ecc/groups/affine_element_impl.hpp:24-40, 58-65): canonical non-Montgomery x in bits 0 .. 253, bit 0 of canonical y in bit 255.  The
 *      reference cannot express infinity in this form; here it is bit 254 set and every other bit zero (q < 2^254, so no finite word sets bit
 *      254).  A word with bit 254 and any other bit set is malformed, and so is one whose x is not below q.  This is STRICTER than the
 *      reference, whose constructor reduces x silently and returns a point that is not on the curve when x^3 + 3 is a non-residue: here the
 *      first is status 0 and the second status 2.  y is recovered as (x^3 + 3)^((q + 1) / 4) and accepted iff its square is x^3 + 3.
 *        Buffer form (64 B): y, then x, 32 bytes each, most significant byte first, canonical.  Decode: bit 7 of byte 0 set is the point at
 *      infinity whatever the other 511 bits hold, as the reference reads it; otherwise bit 6 of byte 0 and both coordinates are range-checked
 *      and the point is tested against y^2 = x^3 + 3.  Encode writes infinity as 0x80 followed by 63 zero bytes (the reference writes
 *      unspecified bytes under the flag, and its reader ignores them).
 *        Status word per element (d_status: n uint32, may be NULL); *d_bad (uint32, may be NULL) counts the statuses 0 and 2, is written by
 *      every call and is 0 for n = 0:
 *          1   finite and valid
 *          3   the point at infinity (G1 forms only; valid)
 *          0   malformed: a coordinate or scalar not below its modulus, or an undefined flag bit
 *          2   well-formed but not on the curve: x^3 + 3 a non-residue (compressed forms), y^2 != x^3 + 3 (buffer form, encode with check)
 *      An element with status 0 or 2 writes the infinity encoding (of the native side, or of the form) for G1 and zero for Fr, so calls
 *      downstream see a defined value and nothing else is affected.
 *        Encode: check = 1 tests every finite point against the curve (status 2, counted, the form's infinity written); check = 0 writes x
 *      and the parity of whatever y it is given, status 1 or 3.  For the Fr forms check is ignored (but must be 0 or 1) and every status is 1.
 *        n is at most 2^28; n = 0 is legal.  BBG_E_INVALID with nothing queued and every output untouched: a null context, a null data
 *      pointer with n > 0, an unknown form, check other than 0 or 1, n out of range, any overlap between the input and the outputs or between
 *      two outputs, and -- the device forms only, whose kernels move 16 bytes per access -- a data pointer that is not 16-byte aligned or a
 *      status or count pointer that is not 4-byte aligned.  The device forms queue on the context stream only (a memset of *d_bad and one
 *      kernel, one lane per element), use no working memory and never synchronise the host.  Timed under "wire_decode" and "wire_encode"
 *      (bbg_profile_get). ---- */
#define BBG_WIRE_G1_COMPRESSED       0  /* 32 B: the reference's in-memory uint256_t, 4 x u64 little-endian limbs */
#define BBG_WIRE_G1_COMPRESSED_BYTES 1  /* the same word as 32 bytes, most significant first (write(buf, uint256_t), numeric/uint256/uint256.hpp:188-195) */
#define BBG_WIRE_G1_BUFFER           2  /* 64 B: affine_element::serialize_to_buffer (ecc/groups/affine_element.hpp:38-56) */
#define BBG_WIRE_FR                  3  /* 32 B: the canonical integer as 4 x u64 little-endian limbs (uint256_t(fr)) */
#define BBG_WIRE_FR_BYTES            4  /* 32 B big-endian canonical: fr::serialize_to_buffer (ecc/fields/field.hpp:189-191) */
/* Bytes per element on either side of a form (either pointer may be NULL); a pure host function that needs no device and no context.
 * BBG_E_INVALID for an unknown form. */
int bbg_wire_sizes(int form, size_t* wire_bytes, size_t* native_bytes);
int bbg_wire_decode_device(bbg_ctx* ctx, int form, const void* d_wire, size_t n, void* d_native, void* d_status /* n uint32 or NULL */,
                           void* d_bad /* uint32 or NULL */);
int bbg_wire_encode_device(bbg_ctx* ctx, int form, const void* d_native, size_t n, int check, void* d_wire, void* d_status, void* d_bad);
/* Host-buffer forms: upload, the device form, download; synchronous; no alignment is asked of host pointers.  A non-zero count of bad
 * elements returns BBG_E_INVALID AFTER the outputs, the status words and *bad have been written, so the caller can see which elements
 * they were (as bbg_pairing_product does for status 2); every other error leaves them untouched. */
int bbg_wire_decode(bbg_ctx* ctx, int form, const void* wire, size_t n, void* native, uint32_t* status, uint32_t* bad);
int bbg_wire_encode(bbg_ctx* ctx, int form, const void* native, size_t n, int check, void* wire, uint32_t* status, uint32_t* bad);

/* ---- device memory helpers for hosts that do not link HIP (bbmalloc/bbfree analogue, c_bind.cpp:11-15) ---- */
int bbg_dev_alloc(bbg_ctx* ctx, size_t bytes, void** d_ptr);
int bbg_dev_free(bbg_ctx* ctx, void* d_ptr);
int bbg_dev_upload(bbg_ctx* ctx, void* d_dst, const void* src, size_t bytes);
int bbg_dev_download(bbg_ctx* ctx, void* dst, const void* d_src, size_t bytes);

/* ---- quotient-polynomial pointwise kernels on the 4n coset domain: the widgets' compute_quotient_contribution of
 *      ProverBase::execute_fourth_round (prover.cpp:304-319).  Device-resident: every polynomial is an array of
 *      2^log2_large_domain (+4) Fr values on the device, as left behind by the coset FFTs ("*_fft" arrays of the proving key). ---- */
enum bbg_quotient_poly { /* index into d_polys[]; entries a widget does not read may be NULL */
    BBG_QP_W_1 = 0, BBG_QP_W_2, BBG_QP_W_3, BBG_QP_W_4, BBG_QP_Z,
    BBG_QP_SIGMA_1, BBG_QP_SIGMA_2, BBG_QP_SIGMA_3, BBG_QP_SIGMA_4,
    BBG_QP_Q_1, BBG_QP_Q_2, BBG_QP_Q_3, BBG_QP_Q_4, BBG_QP_Q_5, BBG_QP_Q_M, BBG_QP_Q_C,
    BBG_QP_Q_ARITH, BBG_QP_Q_FIXED_BASE, BBG_QP_Q_RANGE, BBG_QP_Q_LOGIC, BBG_QP_LAGRANGE_1,
    BBG_QP_COUNT,
    /* extension read only by BBG_WIDGET_MIMC: d_polys then has BBG_QP_EXT_COUNT entries (the first BBG_QP_COUNT as above) */
    BBG_QP_EXT_Q_MIMC_COEFFICIENT = BBG_QP_COUNT, BBG_QP_EXT_Q_MIMC_SELECTOR,
    BBG_QP_EXT_COUNT
};
enum bbg_quotient_widget {
    BBG_WIDGET_PERMUTATION = 0,      /* ProverPermutationWidget<4,false> (permutation_widget_impl.hpp:316-420): ASSIGNS the quotient */
    BBG_WIDGET_TURBO_ARITHMETIC = 1, /* TurboArithmeticKernel (turbo_arithmetic_widget.hpp): the transition widgets ACCUMULATE */
    BBG_WIDGET_TURBO_FIXED_BASE = 2, /* TurboFixedBaseKernel */
    BBG_WIDGET_TURBO_RANGE = 3,      /* TurboRangeKernel */
    BBG_WIDGET_TURBO_LOGIC = 4,      /* TurboLogicKernel */
    BBG_WIDGET_PERMUTATION_3 = 5,    /* StandardPLONK: ProverPermutationWidget<3,false> (w_4 / sigma_4 not read): ASSIGNS */
    BBG_WIDGET_ARITHMETIC = 6,       /* StandardPLONK: ArithmeticKernel (arithmetic_widget.hpp): accumulates */
    BBG_WIDGET_MIMC = 7              /* MiMCComposer: MiMCKernel (mimc_widget.hpp:17-52) over w_1..w_3 and the two BBG_QP_EXT selectors: accumulates */
};
/* challenges: 9 Montgomery Fr (4 limbs each) on the host -- alpha_base (this widget's starting power of alpha), alpha,
 * beta, gamma, public_input_delta, g (the small domain's coset generator), k1, k2, k3 (fr::coset_generator(0..2)).
 * alpha_base_out (may be NULL) receives the alpha_base for the next widget, as compute_quotient_contribution returns it. */
int bbg_quotient_widget_device(bbg_ctx* ctx, int widget, const void* const d_polys[BBG_QP_COUNT], unsigned log2_large_domain,
                               const uint64_t* challenges, void* d_quotient, uint64_t* alpha_base_out);

/* The permutation grand product z of ProverPermutationWidget<4,false>::compute_round_commitments
 * (permutation_widget_impl.hpp:48-268, before the blinding of the last rows and the ifft): d_z[0] = 1,
 * d_z[j+1] = prod_{i<=j} prod_k (w_k[i] + gamma + beta K_k w^i) / (w_k[i] + gamma + beta sigma_k[i]).  d_wires / d_sigmas: 4 device
 * arrays of 2^log2n Lagrange-base values each; challenges: 5 Montgomery Fr on the host -- beta, gamma, k1, k2, k3; d_z: 2^log2n
 * values.  Asynchronous on the context stream. */
int bbg_permutation_grand_product_device(bbg_ctx* ctx, const void* const d_wires[4], const void* const d_sigmas[4], unsigned log2n,
                                         const uint64_t* challenges, void* d_z);

/* ---- resident prover rounds (SURVEY 8f-1 with 8f-2 / 8f-4 inside): the native, handle-based form of a PLONK prover's O(n) work.
 *      The host keeps the transcript (Fiat-Shamir hashing) and the O(1) challenge algebra -- in a barretenberg build that is
 *      shim/bbg_resident_prover.hpp, which drives these entry points from ProverBase's own public members in place of
 *      ProverBase::construct_proof (prover.cpp:420-436) and work_queue::process_queue (work_queue.hpp:208-282).
 *      One handle per proving key; selector / permutation polynomials are registered ONCE (explicit lifetime, no content
 *      fingerprints), wires go up per proof, 11 commitments and the opening evaluations come down.  All values Montgomery Fr; commitments
 *      leave as g1::element (Jacobian, 96 bytes = 12 limbs, what pippenger_unsafe returns) and the caller normalises them the way
 *      work_queue::process_queue does (g1::affine_element(result), work_queue.hpp:233-239).  Rounds must be called in order; each
 *      returns after ONE host sync. ---- */
typedef struct bbg_prover bbg_prover;
enum bbg_poly_form {
    BBG_FORM_COEFF = 0,    /* n coefficients (monomial form)                                   */
    BBG_FORM_LAGRANGE = 1, /* n values on the small domain                                     */
    BBG_FORM_COSET = 2     /* 4n values on the coset g * <w_4n> (the key's "*_fft" arrays)      */
};
enum bbg_prover_poly { /* continues enum bbg_quotient_poly: the polynomials a proof creates */
    BBG_PP_QUOTIENT = BBG_QP_COUNT, /* all 4n coefficients of t(X)                                                      */
    BBG_PP_T_1, BBG_PP_T_2, BBG_PP_T_3, BBG_PP_T_4, /* t_low, t_mid, t_high, t_higher: slices of n coefficients of t(X) */
    BBG_PP_LINEAR,                  /* r(X), the linearisation polynomial                                               */
    BBG_PP_OPENING, BBG_PP_SHIFTED_OPENING, /* W_zeta(X), W_zeta_omega(X)                                               */
    BBG_PP_Q_MIMC_COEFFICIENT, BBG_PP_Q_MIMC_SELECTOR, /* key polynomials of the MiMC flavour (set_key_poly / evaluate / linearise / round 6 ids) */
    BBG_PP_COUNT
};
enum bbg_prover_flavour { /* the widget list of round 4, in the prover's order */
    BBG_FLAVOUR_TURBO = 0,    /* width 4: permutation<4>, turbo arithmetic, fixed base, range, logic (turbo_composer.cpp:735-752) */
    BBG_FLAVOUR_STANDARD = 1, /* width 3: permutation<3>, arithmetic (standard_composer.cpp:562-582)                             */
    BBG_FLAVOUR_MIMC = 2      /* width 3: permutation<3>, MiMC, arithmetic (MiMCComposer::preprocess, mimc_composer.cpp:277-302)  */
};
/* program_width: 4 = TurboPLONK (ProverPermutationWidget<4> + turbo arithmetic / fixed base / range / logic widgets,
 * turbo_composer.cpp:735-752), 3 = StandardPLONK (ProverPermutationWidget<3> + arithmetic widget, standard_composer.cpp:562-582).
 * generators: 4 Montgomery Fr -- the small domain's coset generator g and fr::coset_generator(0..2) = k1, k2, k3.
 * srs must hold n points (n + 1 for StandardPLONK).  The srs and the context must outlive the handle. */
int bbg_prover_create(bbg_ctx* ctx, bbg_srs* srs, unsigned log2n, int program_width, const uint64_t* generators, bbg_prover** out);
/* The same with the flavour named (bbg_prover_create(4) = TURBO, (3) = STANDARD). */
int bbg_prover_create_flavour(bbg_ctx* ctx, bbg_srs* srs, unsigned log2n, int flavour, const uint64_t* generators, bbg_prover** out);
void bbg_prover_destroy(bbg_prover* p);
/* Per proving key.  id: BBG_QP_SIGMA_1 .. BBG_QP_LAGRANGE_1, BBG_PP_Q_MIMC_*.  form BBG_FORM_COEFF (n values; what proving_key::constraint_selectors /
 * permutation_selectors hold) is sufficient: bbg_prover_finalize_key derives sigma's Lagrange form, every 4n-coset form and L_1 on the
 * device.  A caller may instead hand over its own BBG_FORM_LAGRANGE (sigma) / BBG_FORM_COSET arrays.  The array is copied before
 * the call returns.  Re-registering a polynomial replaces it (call finalize again). */
int bbg_prover_set_key_poly(bbg_prover* p, int id, int form, const uint64_t* values);
int bbg_prover_finalize_key(bbg_prover* p);
/* Preamble + round 1 (prover.cpp:139-190, :66-84): wires_lagrange[k], k < program_width: the n values of wire k INCLUDING the blinding
 * rows n-4 .. n-2 the host has drawn.  Uploads them (kept for round 3), iffts to coefficient form (resident), commits.
 * commitments: program_width x 12 limbs, W_1 .. W_w as g1::element. */
int bbg_prover_round1(bbg_prover* p, const uint64_t* const* wires_lagrange, uint64_t* commitments);
/* Round 3 (permutation_widget_impl.hpp:48-312, prover.cpp:239-268): grand product z over the resident wires and sigmas, rows
 * n-3 .. n-1 <- blind[3][4], ifft, commitment Z, and the 4n-coset forms of z and the wires (resident, for round 4). */
int bbg_prover_round3(bbg_prover* p, const uint64_t beta[4], const uint64_t gamma[4], const uint64_t* blind, uint64_t z_commitment[12]);
/* Round 4 (prover.cpp:275-363): the flavour's widgets in the prover's order, division by Z*_H, coset_ifft(4n) -> t(X) resident;
 * commitments T_1 .. T_w, 12 limbs each (the last one over n + 1 coefficients for StandardPLONK, prover.cpp:117-137). */
int bbg_prover_round4(bbg_prover* p, const uint64_t alpha[4], const uint64_t public_input_delta[4], uint64_t* t_commitments);
/* Round 5a (add_opening_evaluations_to_transcript, kate_commitment_scheme.cpp:362-420; quotient_large.evaluate, prover.cpp:397):
 * out[k] = P_ids[k](zeta), or P(zeta * w_n) where shifted[k] != 0 (shifted may be NULL); ids from bbg_quotient_poly /
 * bbg_prover_poly (coefficient forms; BBG_PP_QUOTIENT evaluates all 4n coefficients).  count <= 32. */
int bbg_prover_evaluate(bbg_prover* p, size_t count, const int* ids, const int* shifted, const uint64_t zeta[4], uint64_t* out);
/* The same evaluations from the handle's LAGRANGE-form arrays, where they lie (bbg_poly_evaluate_lagrange_device's contract and formula): ids
 * BBG_QP_W_1 .. W_width and BBG_QP_SIGMA_1 .. SIGMA_width -- the arrays bbg_prover_read_poly(..., BBG_FORM_LAGRANGE, ...) returns; any other id is
 * BBG_E_INVALID.  Needs a finalised key and round 1 of the current proof; reads only (no round uses those arrays as scratch), so a proof in
 * progress is not disturbed and its stage does not change.  count <= 32; returns after one host synchronisation. */
int bbg_prover_evaluate_lagrange(bbg_prover* p, size_t count, const int* ids, const int* shifted, const uint64_t zeta[4], uint64_t* out);
/* Round 5b (compute_linear_contribution of every widget, prover.cpp:399-407): r(X) = sum_k scalars[k] * P_ids[k](X) (resident as
 * BBG_PP_LINEAR), r_eval = r(zeta). */
int bbg_prover_linearise(bbg_prover* p, size_t count, const int* ids, const uint64_t* scalars, const uint64_t zeta[4], uint64_t r_eval[4]);
/* Round 6 (KateCommitmentScheme::batch_open, kate_commitment_scheme.cpp:133-236): F = t_low + sum scalars_zeta[k] P_ids_zeta[k],
 * F' = sum scalars_omega[k] P_ids_omega[k]; W_zeta = (F - F(zeta)) / (X - zeta), W_zeta_omega likewise at zeta_omega; commitments
 * PI_Z and PI_Z_OMEGA.  t_high_top_scalar: StandardPLONK only (else NULL) -- the scalar zeta^(2n) of t's (3n+1)-th coefficient, which
 * enters F as its coefficient n (:196-205). */
int bbg_prover_round6(bbg_prover* p, size_t count_zeta, const int* ids_zeta, const uint64_t* scalars_zeta, size_t count_omega,
                      const int* ids_omega, const uint64_t* scalars_omega, const uint64_t zeta[4], const uint64_t zeta_omega[4],
                      const uint64_t* t_high_top_scalar, uint64_t pi_z[12], uint64_t pi_z_omega[12]);
/* Copies a resident polynomial back (tests; a host that wants the reference's post-proof state): id / form as above. */
int bbg_prover_read_poly(bbg_prover* p, int id, int form, uint64_t* out, size_t count);
/* Device bytes this handle owns (key polynomials in every form + the per-proof working set); what a key cache budgets with. */
int bbg_prover_device_bytes(const bbg_prover* p, size_t* bytes);

/* ---- several GPUs in one process: one MSM / one (coset) NTT spread over a group of contexts, one per device of the node
 *      (device indices may repeat: several contexts on one GPU, which is how the split is tested on a single-GPU box).
 *      MSM: point-range shards as in Pippenger::pippenger_unsafe(scalars, from, range) + g1_sum (pippenger.cpp:27-31, c_bind.cpp:31-46);
 *      only G x 96 bytes cross between GPUs.  NTT: residue classes + ONE all-to-all over peer copies (xGMI) + size-G DFTs.
 *      The process-per-GPU form of the same split (torch.distributed / RCCL) is aztec-2.0_amd/parallel.py. ---- */
typedef struct bbg_multi bbg_multi;
int bbg_multi_create(const int* devices, int count, bbg_multi** out);
void bbg_multi_destroy(bbg_multi* m);
int bbg_multi_count(const bbg_multi* m);
bbg_ctx* bbg_multi_ctx(bbg_multi* m, int k); /* context k of the group (for the *_device entry points on its GPU) */
int bbg_multi_sync(bbg_multi* m);
/* key "exchange": 0 = peer copies ordered with events (default), 1 = RCCL from C++ -- one communicator per context (ncclCommInitAll over
 * the group's devices, which must be distinct), ncclAllGather of the 96-byte MSM partials + the group sum, the NTT's all-to-all as grouped
 * ncclSend / ncclRecv on the contexts' streams.  librccl.so is loaded on first use.  Both back ends give identical results. */
int bbg_multi_set_option(bbg_multi* m, const char* key, long value);
/* Shards the SRS by point range: context g keeps points [g*ceil(n/G), (g+1)*ceil(n/G)) with their window tables resident.
 * points / stride_bytes as bbg_srs_register.  Replaces a previously registered SRS. */
int bbg_multi_srs_register(bbg_multi* m, const uint64_t* points, size_t n, size_t stride_bytes);
/* The hashed synthetic SRS of bbg_srs_synth_hashed(seed, n), every shard generated on its own GPU. */
int bbg_multi_srs_synth_hashed(bbg_multi* m, uint64_t seed, size_t n);
size_t bbg_multi_srs_num_points(const bbg_multi* m);
/* result = sum_{i<n} scalars[i] * P_{from+i}: every context runs the bucket MSM over its part of the range (scalars uploaded in
 * parallel, one host thread per GPU), the 96-byte partials are summed on context 0.  Same contract as bbg_msm. */
int bbg_multi_msm(bbg_multi* m, const uint64_t* scalars, size_t from, size_t n, uint64_t out_jacobian[12]);
/* op: BBG_FFT, BBG_IFFT, BBG_COSET_FFT or BBG_COSET_IFFT over the whole 2^log2n domain; G = 1, 2, 4 or 8 contexts.
 * Device-resident, asynchronous: d_shards[g] (on context g's GPU) holds the residue class a_{g + G j}, j < m = n / G; on return (after
 * bbg_multi_sync) shard r holds A[t*m + r*len + q] at index t*len + q (t < G, q < len = m / G), i.e. G contiguous runs of the
 * natural-order result.  One all-to-all of (G-1)/G^2 of the data per GPU, no host synchronisation between the phases. */
int bbg_multi_ntt_device(bbg_multi* m, void* const* d_shards, unsigned log2n, int op);
/* Host-buffer form, in place on coeffs[2^log2n] in natural order (residue classes gathered on the host by one thread per GPU; bound by
 * that gather and PCIe, not by the GPUs -- the resident form above is the one to build a multi-GPU prover on). */
int bbg_multi_ntt(bbg_multi* m, uint64_t* coeffs, unsigned log2n, int op);

/* ---- HBM budget: what a context holds on its device, by purpose.  Everything here is allocated on first use and then kept (the
 *      pippenger_runtime_state / evaluation_domain analogue: runtime_states.cpp:14-66, evaluation_domain.cpp:57-76); this call is how a
 *      host sees and bounds the total.  bbg_memory_trim releases what can be rebuilt on demand. ---- */
typedef struct bbg_memory_info {
    size_t srs_points;     /* plain SRS points not part of a window table (none today: window 0 of a table IS the plain points) */
    size_t srs_tables;     /* window tables of every live SRS of this context, all widths */
    size_t ntt_tables;     /* per-domain twiddle / coset tables (5 x 32n bytes per prepared size) */
    size_t msm_arena;      /* the MSM scratch arena (entries, sorted values, per-slot bucket sets) */
    size_t scratch;        /* NTT ping-pong buffer, host-entry staging, evaluation partials, widget constants, the fixed-base table, the
                              variable-base lanes' tables, the working set of bbg_g1_ntt, the tables of bbg_cells_recover,
                              the working set of bbg_cells_verify_reduce, the working memory of bbg_g1_msm and of bbg_pairing_product,
                              the 512 bytes of bbg_cells_verify (and bbg_kzg_verify), the working sets of bbg_open_points and of
                              bbg_kzg_verify_reduce */
    size_t prover_keys;    /* every live bbg_prover handle of this context (bbg_prover_device_bytes) */
    size_t total;          /* sum of the above */
    size_t device_total;   /* hipMemGetInfo: the device's memory ... */
    size_t device_free;    /* ... and what is free right now (other processes and the runtime included) */
    unsigned live_srs, live_provers, ntt_domains;
} bbg_memory_info;
int bbg_memory_report(bbg_ctx* ctx, bbg_memory_info* out);
/* Frees the rebuildable part after a device synchronisation: NTT tables of every size, the MSM arena, scratch and staging buffers, and --
 * with tables != 0 -- every window table except the one each SRS was registered with.  Returns the bytes released in *released (may be NULL). */
int bbg_memory_trim(bbg_ctx* ctx, int tables, size_t* released);

/* ---- tuning / introspection ---- */
/* key: "ntt_tile_log" (log2 elements per LDS tile, 9..12), "ntt_max_logr" (max radix per pass, 4..10),
 * "msm_async_reduce" (0/1, see bbg_join), "msm_window" (widest bucket window: 0 = automatic [8 bits up to 2^13 terms -- the small-circuit path: three launches, no sort --, 13 up to 2^14, 16 below 2^20, 19 at 2^20, 20 from 2^21, 22 from 2^23 -- bbg_msm_plan reports it],
 * or a compiled width 8 / 13 / 16 / 17 / 19 / 20 / 22; windows are BALANCED -- 255 bits split as evenly as the window count allows --; a width's window tables
 * are built the first time it is used on an SRS), "msm_sort" (1 = fused recode + two-level partition sort, default; 0 = recode + rocPRIM radix sort, only
 * in builds made with `make ROCPRIM_SORT=1`),
 * "msm_reduce_quad" (bit mask 0..15, default 14: reduce-phase stages with four lanes per EC operation -- bit 0 combine, 1 row/column sums, 2 bit
 * planes, 3 plane sum; 0 = the one-lane kernels), "msm_accumulate_quad" (1 = small MSMs accumulate with four threads per lane segment, default),
 * "msm_limbs29" (1 = the bucket accumulation's field arithmetic on 9 x 29-bit limbs, default; 0 = on 8 x 32-bit limbs, A/B),
 * "msm_acc_waves" (0 = automatic; N > 0 = lane segments per SIMD lane of the bucket accumulation, A/B), "msm_reduce_priority" (1 = low-priority reduce streams, default), "msm_upload_pieces" (1..4, default 1: pieces the host scalars of bbg_msm travel in),
 * "quotient_fuse" (1 = arithmetic + range + logic widgets of a chain in one pass, default),
 * "quotient_setup_plan" (1 = the challenge powers of a widget chain's set-up blocks are computed by the lanes of one wave side by side, default; 0 = one
 * lane's chain of products, A/B),
 * "poly_limbs29" (1 = bbg_poly_linear_combination*, bbg_poly_evaluate* and the prover's evaluations / linearisation / opening sums on 9 x 29-bit limbs
 * with four terms per reduction, default; 0 = on 8 x 32-bit limbs, A/B),
 * "prover_fused_divide" (1 = a bbg_prover's round 4 divides the quotient by Z*_H inside the coset iFFT's first load, from a per-point divisor table
 * kept per context -- 32 bytes per point of the 4n domain, counted under ntt_tables -- default; 0 = a pass of its own, A/B),
 * "prover_tail_window" (A/B: window width of the commitments that end prover rounds 4 and 6, 0 = automatic, default; measured: no width beats it),
 * "prover_ntt_batch" (1 = the wires' iFFTs of round 1 and their 4n coset forms go through ONE launch set each -- grid.y = wires -- for circuits up to
 * 2^17 gates, where a single transform has at most 128 tiles for 256 CUs, default; 0 = one launch set per wire, A/B),
 * "prover_early_cosets" (1 = a bbg_prover queues the wires' 4n coset forms behind round 1's last commitment, beside its reduce phase; 0 = in
 * front of round 3's grand product; -1 = the first from 2^18 gates, the second below, default),
 * "quotient_limbs29" (1 = the quotient widgets on lazily reduced 9 x 29-bit limbs with sums of products sharing one reduction, default; 0 = on 8 x 32-bit limbs, A/B),
 * "ntt_kernel" (2 = register-resident radix-8 passes, default; 1 = radix-2 in LDS),
 * "ntt_max_logr8" (6..11, max log-radix per radix-8 pass, default 10), "ntt_big_tile" (0 / 1 / 2: 4096-element tiles for 2^21 [default] / also 2^22),
 * "ntt_lds_planes" (2 = a pass keeps its tile in LDS between two radix-8 steps, 1 = the tile moves one 16-byte plane at a time through half the LDS with
 * three waves per SIMD, 0 = automatic [default]: 1 from 2^22), "ntt_limbs29" (1 = the radix-8 passes compute on lazily reduced 9 x 29-bit limbs,
 * 0 = on 8 x 32-bit limbs, -1 = automatic, default), "prover_msm_batch" (0 .. BBG_MSM_BATCH_MAX, default 4: commitments of a bbg_prover round per
 * launch set; 0 / 1 = one launch set each),
 * "batch_mul_glv" (1 = bbg_g1_batch_mul* multiplies with the windowed GLV form, default; 0 = with the bit-serial double-and-add, A/B),
 * "batch_mul_lanes" (a multiple of 64 in 64 .. 2^20, default 2^17: lanes of the variable-base kernels, each holding a 1 KiB table and walking
 * the points with that stride), "ecntt_mul" (1 = the stages of the G1 transforms -- bbg_srs_lagrange, bbg_g1_ntt, bbg_open_all -- multiply with the
 * windowed GLV form, default; 0 = bit-serially, A/B).
 * "prover_fail_round" is a test hook, not a tuning option: the next bbg_prover_round<value> fails once as a device error would.  It is refused
 * with BBG_E_INVALID unless the process was started with BBG_TEST_HOOKS=1.
 * A null or unknown key and a value outside a key's range return BBG_E_INVALID and leave the context unchanged.
 * Every value of every option gives bit-identical results; they exist for A/B measurements. */
int bbg_set_option(bbg_ctx* ctx, const char* key, long value);
/* Per-kernel timing with HIP events recorded on the launch stream.  Names: "msm_recode", "msm_sort", "msm_offsets",
 * "msm_accumulate", "msm_reduce", "ntt_pass", "quotient_widget", "ecntt_stages", "ecntt_normalize", "fixed_base_table", "fixed_base_mul", "var_base_mul",
 * "fr_batch_invert", "barycentric", "open_all_prepare", "open_all_coeffs", "open_all_pointwise", "open_all_fold", "open_cells_sum",
 * "cells_gather", "cells_z", "cells_scatter", "cells_divide", "cells_canon", "cells_verify_powers", "cells_verify_fold", "cells_verify_mul",
 * "cells_verify_segsum", "cells_verify_phi", "cells_verify_finish", "msm_points_sort", "msm_points_accumulate", "msm_points_reduce",
 * "msm_points_combine", "g2_lines", "pairing_miller", "pairing_final", "wire_decode", "wire_encode".  enable(…, 1) clears previous samples. */
int bbg_profile_enable(bbg_ctx* ctx, int on);
int bbg_profile_get(bbg_ctx* ctx, const char* name, double* total_ms, size_t* launches);
/* Field-level self test entry used by tests: out[i] = a[i] (op) b[i] computed by the device field code.
 * which: 0 Fr, 1 Fq.  op: 0 mul, 1 add, 2 sub, 3 mul via the CIOS cross-check path, 4 from_montgomery, 5 to_montgomery,
 * 6/7 mul / CIOS mul without pre-reduction, 8 a*a - b*b and 9 (-a)(-b) - a(-b) through the fused two-product multiplier,
 * 10 / 11 the inverse of a (0 -> 0) by the binary extended Euclid of the set-up kernels, per lane / on the scalar unit (one wave per element),
 * 12 (which = 1 only) a^((q + 1) / 4), the square-root candidate of bbg_wire_decode's compressed forms alone: a root of a when a is a
 * residue, and a value that squares to -a when it is not; which = 0 is BBG_E_INVALID, because r = 1 mod 4 and no single power is a root. */
int bbg_field_op(bbg_ctx* ctx, int which, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
/* Self test entry of the 29-bit-limb arithmetic, used by tests (like bbg_field_op, but on RAW operands: nothing is pre-reduced, so a lazily
 * reduced value -- limbs above 29 bits, a value of many p -- reaches the device primitive as it is, and the raw result limbs come back).
 * which: 0 Fr, 1 Fq.  in: n vectors of `operands` rows, out: n vectors of `results` rows (bbg_limb29_op_shape gives both counts, without
 * device work).  A row is 9 uint32_t: a limb value uses all nine; an 8 x u32 field element uses words 0..7 and word 8 is written as 0.
 * op: one primitive of csrc/field29.hip.h, field29c.hip.h, curve29.hip.h, ntt29.hip.h or w29.hip.h each; the numbers are listed in
 * csrc/limb29_check.hip (BBG_L29_OPS; 100 + i / 200 + i / 300 + i: f29_sub / f29_neg / n29_bfly with the i-th (M, E) pair of BBG_L29_PAIRS).
 * The device checks no precondition: a vector outside an op's contract gives wrapped arithmetic.
 * BBG_E_INVALID (out untouched) for an unknown (which, op), a null pointer with n > 0, or n > 2^20; n = 0 is BBG_OK. */
int bbg_limb29_op(bbg_ctx* ctx, int which, int op, const uint32_t* in, size_t n, uint32_t* out);
int bbg_limb29_op_shape(int which, int op, int* operands, int* results);
/* Self test entry of the pairing arithmetic, used by tests (like bbg_limb29_op: RAW operands, nothing is pre-reduced): one device function of
 * csrc/fq_tower.hip.h, fq12_wave.hip.h or g2.hip.h per op, on coefficients anywhere in the tower's coarse range [0, 2p] -- a coefficient given
 * as 2p arrives as 2p -- with the raw result words coming back.  in: n vectors of `operands` rows, out: n vectors of `results` rows
 * (bbg_tower_op_shape gives both counts, without device work).  A row is one Fq value, 8 uint32_t, Montgomery form; an Fq2 is two rows
 * (c0, c1), an Fq12 twelve in the reference's order; the ops of fq12_wave.hip.h take and return the twelve coefficients of a slot in the
 * w-basis.  A boolean result is one row whose word 0 is 0 or 1 and whose other words are 0.  The op numbers are listed in
 * csrc/tower_check.hip (BBG_TOWER_OPS).  The device checks no precondition: a coefficient above 2p gives wrapped arithmetic.
 * BBG_E_INVALID (out untouched) for an unknown op, a null pointer with n > 0, or n > 2^16; n = 0 is BBG_OK. */
int bbg_tower_op(bbg_ctx* ctx, int op, const uint32_t* in, size_t n, uint32_t* out);
int bbg_tower_op_shape(int op, int* operands, int* results);

#ifdef __cplusplus
}
#endif
#endif /* BBG_H */
