// The layout of one buffer: the regions a call needs -- a host-array entry point's staged inputs and outputs (bbg_capi.hip), a module's
// device working memory (work_layouts.h, msm_layout in msm_kernels.hip.h) -- carved out of ONE allocation.  The caller asks for the regions
// in order, each by its byte count, and gets their offsets, each a multiple of the layout's alignment; total() is the end of the last
// region, which is what the buffer must hold, and close() first pads that end to the alignment for the layouts whose size includes the pad.
// An alignment of 1 packs the regions: a module that orders them by descending element size keeps every element naturally aligned.
// A request that does not fit size_t -- a single one or the sum -- is remembered instead of wrapping: ok() turns false and stays false,
// and the offsets handed out from then on are 0.
// Plain host C++ with no HIP in it: bbg_internal.h binds a finished layout to a DevBuf (ensure_layout), tests/tools/region_layout_check.cpp
// checks it alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bbg {

constexpr size_t STAGE_ALIGN = 256; // the staging buffer's regions (bbg_capi.hip)

class RegionLayout {
  public:
    explicit RegionLayout(size_t align) : align_(align) {} // align >= 1
    // the offset of a new region of `bytes` bytes (zero bytes are a region too: it shares its offset with the next one)
    size_t add(size_t bytes)
    {
        const size_t pad = (align_ - end_ % align_) % align_;
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
    // a region that holds a whole finished layout: a block that is described once and placed in two buffers.  Its failure becomes this one's.
    size_t add(const RegionLayout& block)
    {
        if (!block.ok_) ok_ = false;
        return add(block.end_);
    }
    // the end padded to the alignment: the total of a layout that rounds every region up, the last one included
    size_t close() { return add(0); }
    size_t total() const { return ok_ ? end_ : 0; }
    bool ok() const { return ok_; }

  private:
    size_t align_;
    size_t end_ = 0;
    bool ok_ = true;
};

} // namespace bbg
