// lagrange_check.cpp -- link-compatibility + parity proof for the shim's lagrange_base::transform_srs (test infrastructure; built only
// where the reference tree exists, the prebuilt binary oracle/_ref/lagrange_check travels to the GPU box).
//
// Written against barretenberg's OWN public API and linked against barretenberg's OWN translation units, unmodified, among them
// srs/lagrange_base_transformation/lagrange_base.cpp.  The final link wraps transform_srs (-Wl,--wrap=..., shim/wrap_flags.txt), so the
// plain call lands in shim/bbg_barretenberg_shim.cpp -> bbg_srs_lagrange -> MI355X while __real_* reaches the reference's recursive CPU
// g1fft in the same process.
//
//   lagrange_check                       degrees 4, 64 and 2^10: GPU table == CPU table (g1::affine_element equality), then the reference's
//                                        own test (lagrange_base.test.cpp: the commitment to a random polynomial over the monomial table
//                                        equals the commitment to its fft over the Lagrange table, both by the reference's CPU pippenger)
//                                        on the GPU-made table; `--also LOG2N` compares and times one more size (2^12: the CPU side takes seconds)
//   lagrange_check --dump IN OUT LOG2N   CPU only, never touches a GPU: IN = 2^LOG2N points (64 B each, Montgomery), OUT = the reference's
//                                        transform_srs of them (how tests/golden/lagrange_srs.json is made)
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <ecc/curves/bn254/scalar_multiplication/scalar_multiplication.hpp>
#include <polynomials/evaluation_domain.hpp>
#include <polynomials/polynomial_arithmetic.hpp>
#include <srs/lagrange_base_transformation/lagrange_base.hpp>

using namespace barretenberg;

#define REAL(m) asm("__real_" m)
namespace real {
void transform_srs(g1::affine_element*, g1::affine_element*, const size_t)
    REAL("_ZN12barretenberg13lagrange_base13transform_srsEPNS_14group_elements14affine_elementINS_5fieldINS_13Bn254FqParamsEEENS3_INS_13Bn254FrParamsEEENS_13Bn254G1ParamsEEESA_m");
g1::element pippenger(fr*, g1::affine_element*, const size_t, scalar_multiplication::pippenger_runtime_state&, bool)
    REAL("_ZN12barretenberg21scalar_multiplication9pippengerEPNS_5fieldINS_13Bn254FrParamsEEEPNS_14group_elements14affine_elementINS1_INS_13Bn254FqParamsEEES3_NS_13Bn254G1ParamsEEEmRNS0_23pippenger_runtime_stateEb");
void fft(fr*, const evaluation_domain&) REAL("_ZN12barretenberg21polynomial_arithmetic3fftEPNS_5fieldINS_13Bn254FrParamsEEERKNS_17evaluation_domainE");
} // namespace real

static uint64_t sm_state = 0xBB254;
static uint64_t splitmix()
{
    uint64_t z = (sm_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
static fr rand_fr()
{
    fr r{ splitmix(), splitmix(), splitmix(), splitmix() & 0x0FFFFFFFFFFFFFFFULL };
    return r;
}
static int failures = 0;
static void expect(bool ok, const std::string& what)
{
    std::printf("%s %s\n", ok ? "ok  " : "FAIL", what.c_str());
    if (!ok) failures++;
}
static double seconds_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
// monomials[i] = [x^i] G, as the reference's test builds them (lagrange_base.test.cpp:25-34)
static std::vector<g1::affine_element> monomial_srs(size_t degree)
{
    const fr x = rand_fr();
    std::vector<g1::affine_element> m(degree);
    fr power = fr::one();
    for (size_t i = 0; i < degree; i++) {
        m[i] = g1::affine_element(g1::element(g1::affine_one) * power);
        power *= x;
    }
    return m;
}

static int dump(const char* in_path, const char* out_path, unsigned log2n)
{
    const size_t n = (size_t)1 << log2n;
    std::vector<g1::affine_element> in(n), out(n);
    FILE* f = std::fopen(in_path, "rb");
    if (!f || std::fread((void*)in.data(), sizeof(g1::affine_element), n, f) != n) {
        std::fprintf(stderr, "lagrange_check --dump: cannot read %zu points from %s\n", n, in_path);
        return 2;
    }
    std::fclose(f);
    const auto t0 = std::chrono::steady_clock::now();
    real::transform_srs(in.data(), out.data(), n);
    std::printf("reference transform_srs 2^%u: %.3f s\n", log2n, seconds_since(t0));
    f = std::fopen(out_path, "wb");
    if (!f || std::fwrite((const void*)out.data(), sizeof(g1::affine_element), n, f) != n) {
        std::fprintf(stderr, "lagrange_check --dump: cannot write %s\n", out_path);
        return 2;
    }
    std::fclose(f);
    return 0;
}

static void check_degree(size_t degree)
{
    const std::string tag = "degree " + std::to_string(degree);
    std::vector<g1::affine_element> monomials = monomial_srs(degree);
    std::vector<g1::affine_element> gpu(2 * degree), cpu(2 * degree); // room for the endomorphism tables below

    auto t0 = std::chrono::steady_clock::now();
    lagrange_base::transform_srs(monomials.data(), gpu.data(), degree); // wrapped: the GPU
    const double first = seconds_since(t0);
    t0 = std::chrono::steady_clock::now();
    lagrange_base::transform_srs(monomials.data(), gpu.data(), degree); // again: the domain tables exist, the kernels are loaded
    const double t_gpu = seconds_since(t0);
    t0 = std::chrono::steady_clock::now();
    real::transform_srs(monomials.data(), cpu.data(), degree);
    const double t_cpu = seconds_since(t0);
    std::printf("transform_srs %s: shim first call %.4f s, second call %.4f s (upload + transform + window tables + download), reference %.4f s\n",
                tag.c_str(), first, t_gpu, t_cpu);

    bool same = true, on_curve = true;
    for (size_t i = 0; i < degree; i++) {
        same = same && gpu[i] == cpu[i];
        on_curve = on_curve && gpu[i].on_curve();
    }
    expect(on_curve, tag + ": every point of the shim's table is on the curve");
    expect(same, tag + ": shim transform_srs == reference transform_srs, point by point");

    // the reference's own test on the shim's table: commit(coefficients, monomial) == commit(evaluations, Lagrange), all on the CPU
    evaluation_domain domain(degree);
    domain.compute_lookup_table();
    std::vector<fr> coeffs(degree), evals;
    for (auto& c : coeffs) c = rand_fr();
    evals = coeffs;
    real::fft(evals.data(), domain);
    std::vector<g1::affine_element> mono_table(2 * degree);
    std::memcpy((void*)mono_table.data(), (const void*)monomials.data(), degree * sizeof(g1::affine_element));
    scalar_multiplication::generate_pippenger_point_table(mono_table.data(), mono_table.data(), degree);
    scalar_multiplication::generate_pippenger_point_table(gpu.data(), gpu.data(), degree);
    scalar_multiplication::pippenger_runtime_state state(degree);
    g1::element expected = real::pippenger(coeffs.data(), mono_table.data(), degree, state, true);
    g1::element result = real::pippenger(evals.data(), gpu.data(), degree, state, true);
    expect(g1::affine_element(expected) == g1::affine_element(result), tag + ": commitment from evaluations over the shim's table == commitment from coefficients");
}

int main(int argc, char** argv)
{
    if (argc == 5 && std::strcmp(argv[1], "--dump") == 0) return dump(argv[2], argv[3], (unsigned)std::atoi(argv[4]));
    for (size_t degree : { (size_t)4, (size_t)64, (size_t)1024 }) check_degree(degree);
    if (argc == 3 && std::strcmp(argv[1], "--also") == 0) {
        const size_t degree = (size_t)1 << std::atoi(argv[2]);
        std::vector<g1::affine_element> monomials = monomial_srs(degree), gpu(degree), cpu(degree);
        auto t0 = std::chrono::steady_clock::now();
        lagrange_base::transform_srs(monomials.data(), gpu.data(), degree);
        t0 = std::chrono::steady_clock::now();
        lagrange_base::transform_srs(monomials.data(), gpu.data(), degree);
        const double t_gpu = seconds_since(t0);
        t0 = std::chrono::steady_clock::now();
        real::transform_srs(monomials.data(), cpu.data(), degree);
        const double t_cpu = seconds_since(t0);
        std::printf("transform_srs degree %zu: shim second call %.4f s, reference %.4f s\n", degree, t_gpu, t_cpu);
        bool same = true;
        for (size_t i = 0; i < degree; i++) same = same && gpu[i] == cpu[i];
        expect(same, "degree " + std::to_string(degree) + ": shim transform_srs == reference transform_srs, point by point");
    }
    if (failures) {
        std::printf("lagrange_check FAILED (%d)\n", failures);
        return 1;
    }
    std::printf("lagrange_check PASS\n");
    return 0;
}
