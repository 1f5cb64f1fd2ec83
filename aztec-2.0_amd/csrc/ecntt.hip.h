// Index helper shared by the kernels around the G1 transform (ecntt.hip, open_all.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace bbg {

// the `bits` low bits of i in reverse order: the input permutation of the decimation-in-time schedule
__device__ __forceinline__ size_t bit_reverse(size_t i, unsigned bits)
{
    return (size_t)(__brevll((unsigned long long)i) >> (64 - bits));
}

} // namespace bbg
