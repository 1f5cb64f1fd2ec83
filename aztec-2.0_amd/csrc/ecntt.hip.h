// Index helper shared by the kernels around the G1 transform (ecntt.hip, open_all.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace bbg {

// the `bits` low bits of i in reverse order: the input permutation of the decimation-in-time schedule.  bits = 0 gives 0 (a shift by 64
// has no defined result): the layout kernel of open_all.hip reverses within cells of one point.
__device__ __forceinline__ size_t bit_reverse(size_t i, unsigned bits)
{
    return bits ? (size_t)(__brevll((unsigned long long)i) >> (64 - bits)) : 0;
}

} // namespace bbg
