// Stand-alone check of csrc/stage_layout.h, the region arithmetic behind every host-array entry point of the C ABI (bbg_capi.hip).
// Built and run by tests/test_abi_cpu.py::test_stage_layout_host_logic with g++ -fsanitize=address,undefined; needs the header alone.
#include "../../aztec-2.0_amd/csrc/stage_layout.h"

#include <cstdio>
#include <vector>

using bbg::STAGE_ALIGN;
using bbg::StageLayout;

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);            \
            failures++;                                                       \
        }                                                                     \
    } while (0)

// the properties every layout must have: offsets ascending and aligned, regions disjoint and as large as asked, total = end of the last one
static void check_sequence(const std::vector<size_t>& sizes)
{
    StageLayout lay;
    std::vector<size_t> off;
    for (size_t s : sizes) off.push_back(lay.add(s));
    EXPECT(lay.ok());
    size_t end = 0;
    for (size_t k = 0; k < sizes.size(); k++) {
        EXPECT(off[k] % STAGE_ALIGN == 0);
        EXPECT(off[k] >= end);                     // disjoint from, and not below, everything before it
        EXPECT(off[k] - end < STAGE_ALIGN);        // the padding is alignment and nothing else
        if (k) EXPECT(off[k] >= off[k - 1]);
        end = off[k] + sizes[k];                   // the region holds what was asked for
    }
    EXPECT(lay.total() == end);
}

int main()
{
    EXPECT(StageLayout().ok() && StageLayout().total() == 0);
    check_sequence({ 1 });
    check_sequence({ 256, 256, 256 });
    check_sequence({ 1, 2, 3, 255, 257, 4096, 31 });
    check_sequence({ 96, 65 * 32 });                        // a result block in front of 65 scalars
    check_sequence({ 0, 64, 0, 0, 32, 0 });                 // zero-byte regions, first, in the middle and last
    check_sequence({ 0 });
    check_sequence({ (size_t)1 << 40, 1, (size_t)1 << 40 });
    check_sequence({ SIZE_MAX - 1024, 3 });                 // close to the limit and still representable
    {
        StageLayout lay; // the element-count form is the byte form of the product
        EXPECT(lay.add(3, 96) == 0 && lay.add(65, 32) == 512 && lay.add(0, 64) == 2816 && lay.add(7, 0) == 2816);
        EXPECT(lay.ok() && lay.total() == 2816);
    }
    {
        StageLayout lay; // one request that is too large on its own
        EXPECT(lay.add(16) == 0);
        lay.add(SIZE_MAX);
        EXPECT(!lay.ok() && lay.total() == 0);
        EXPECT(lay.add(16) == 0 && !lay.ok()); // it stays that way
    }
    {
        StageLayout lay; // a sum that crosses SIZE_MAX, every term representable
        lay.add(SIZE_MAX / 2 + 1);
        EXPECT(lay.ok());
        lay.add(SIZE_MAX / 2 + 1);
        EXPECT(!lay.ok() && lay.total() == 0);
    }
    {
        StageLayout lay; // the sum fits, its alignment padding does not
        lay.add(SIZE_MAX - 100);
        EXPECT(lay.ok());
        lay.add(1);
        EXPECT(!lay.ok());
    }
    {
        StageLayout lay; // count x size wraps to something small
        lay.add(((size_t)1 << 62) + 1, 4);
        EXPECT(!lay.ok());
        StageLayout lay2;
        lay2.add(SIZE_MAX, SIZE_MAX);
        EXPECT(!lay2.ok());
        StageLayout lay3; // the largest product that fits
        EXPECT(lay3.add(SIZE_MAX / 32, 32) == 0 && lay3.ok() && lay3.total() == SIZE_MAX / 32 * 32);
    }
    if (failures) return 1;
    printf("stage_layout_check PASS\n");
    return 0;
}
