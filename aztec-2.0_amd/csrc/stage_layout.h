// The layout of one staged call: the device regions a host-array entry point of the C ABI needs (its inputs, its outputs, a kernel's slack),
// carved out of ONE buffer.  The caller asks for the regions in order, each by its byte count, and gets their offsets, each a multiple of
// STAGE_ALIGN; total() is the end of the last region, which is what the buffer must hold.  A request that does not fit size_t -- a single
// one or the sum -- is remembered instead of wrapping: ok() turns false and stays false, and the offsets handed out from then on are 0.
// Plain host C++ with no HIP in it: bbg_capi.hip binds it to the context's staging buffer, tests/tools/stage_layout_check.cpp checks it alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bbg {

constexpr size_t STAGE_ALIGN = 256;

class StageLayout {
  public:
    // the offset of a new region of `bytes` bytes (zero bytes are a region too: it shares its offset with the next one)
    size_t add(size_t bytes)
    {
        const size_t pad = (STAGE_ALIGN - end_ % STAGE_ALIGN) % STAGE_ALIGN;
        if (!ok_ || pad > SIZE_MAX - end_ || bytes > SIZE_MAX - end_ - pad) {
            ok_ = false;
            return 0;
        }
        const size_t at = end_ + pad;
        end_ = at + bytes;
        return at;
    }
    // a region of `count` elements of `each` bytes
    size_t add(size_t count, size_t each)
    {
        if (each && count > SIZE_MAX / each) {
            ok_ = false;
            return 0;
        }
        return add(count * each);
    }
    size_t total() const { return ok_ ? end_ : 0; }
    bool ok() const { return ok_; }

  private:
    size_t end_ = 0;
    bool ok_ = true;
};

} // namespace bbg
