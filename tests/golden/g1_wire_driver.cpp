// Prints the JSON body of tests/golden/g1_wire.json: the compressed words of [k] G, k = 1 .. 32 (every third one negated), as the reference's
// own affine_element::operator uint256_t makes them, the same word through write(buf, uint256_t), the 64-byte serialize_to_buffer form, and
// the uint256_t round trip affine_element(uint256_t(P)).  Built by gen_golden_g1_wire.py against the reference's headers alone; no part of
// the reference is linked.
#include <cstdint>
#include <cstdio>
#include <vector>

#include <ecc/curves/bn254/g1.hpp>

using namespace barretenberg;

static void hex_be(const char* name, const uint8_t* p, size_t n, const char* tail)
{
    printf("\"%s\": \"", name);
    for (size_t i = 0; i < n; i++) printf("%02x", p[i]);
    printf("\"%s", tail);
}
// a 256-bit integer, most significant digit first
static void hex_int(const char* name, const uint256_t& v, const char* tail)
{
    printf("\"%s\": \"%016lx%016lx%016lx%016lx\"%s", name, (unsigned long)v.data[3], (unsigned long)v.data[2], (unsigned long)v.data[1], (unsigned long)v.data[0],
           tail);
}

int main()
{
    printf("[\n");
    for (uint64_t k = 1; k <= 32; k++) {
        g1::affine_element p(g1::element(g1::affine_one) * fr(k));
        const bool negated = k % 3 == 0;
        if (negated) p = -p;
        const uint256_t word(p);
        std::vector<uint8_t> word_bytes;
        write(word_bytes, word);
        uint8_t buffer[64];
        g1::affine_element::serialize_to_buffer(p, buffer);
        const g1::affine_element back(word);
        printf(" {\"k\": %lu, \"negated\": %s, ", (unsigned long)k, negated ? "true" : "false");
        hex_int("x", uint256_t(p.x), ", ");
        hex_int("y", uint256_t(p.y), ", ");
        hex_int("word", word, ", ");
        hex_be("word_bytes", word_bytes.data(), word_bytes.size(), ", ");
        hex_be("buffer", buffer, 64, ", ");
        hex_int("roundtrip_x", uint256_t(back.x), ", ");
        hex_int("roundtrip_y", uint256_t(back.y), ", ");
        printf("\"roundtrip_equal\": %s, \"on_curve\": %s}%s\n", back == p ? "true" : "false", p.on_curve() ? "true" : "false", k < 32 ? "," : "");
    }
    printf("]\n");
    return 0;
}
