// offset32_host.hpp -- when the BC1 / BC3 / BC4 / BC5 kernels may walk a surface with 32-bit byte offsets (bc1_bc3.hip bc13_kernel<SMALL>,
// bc4_bc5.hip bc45_kernel<WHOLE>) instead of forming a 64-bit address per row.  One definition of the rule for the three launchers.  Plain
// C++, so that a host-only program can replay the walk against it under a sanitizer (tools/offset32_host_check.cpp).
//
// The walk: a lane holds `off`, the byte offset of its block's first texel from the surface's base, as a uint32_t.  It starts at
// yy * 4 * stride + xx * block_row_bytes, advances by workgroup-uniform steps (off_step, and off_wrap when the column passes the end of a
// block row), is replaced by the last block's offset for lanes past the end, and each of the block's four rows is loaded from
// base + (uint32_t)(off + y * stride), y = 0 .. 3.  The additions are modulo 2^32, so `off` is the true offset whenever the true offset of
// every row the walk loads is below 2^32 -- sums that pass 2^32 on the way (off_step before off_wrap, an off_wrap that is "negative" under
// overlapping rows) cancel.  The largest row offset is that of the last row's last block, below (rows - 1) * stride + row_bytes, which for
// rows that overlap (0 < stride < row_bytes; the ABI tolerates them for device surfaces) is NOT bounded by height * stride.
#pragma once
#include <cstdint>

namespace itw {

// width, height: of the surface, in texels; block_row_bytes: the bytes of four texels of one row (16 for RGBA8); out_bytes: the size of the
// block stream where the kernel offsets its stores with 32 bits too, 0 where it does not.
// True only if no byte offset of the walk reaches 2^31 (so none wraps, and none is negative as an int32_t either):
//   height * stride < 2^31                        the rule as it always was: which surfaces walk is a performance contract
//   (rows - 1) * stride + row_bytes <= 2^31 - 1   the column term; implied by the first for rows that do not overlap
//   out_bytes < 2^32                              the last store starts below out_bytes
inline bool walk_fits_32(int64_t stride, int width, int height, int block_row_bytes, int64_t out_bytes)
{
    const int64_t blocks_x = width / 4, blocks_y = height / 4;          // the walk covers whole blocks only
    if (stride <= 0 || blocks_x <= 0 || blocks_y <= 0 || block_row_bytes <= 0) return false;
    const int64_t lim31 = (int64_t)1 << 31;
    if (stride >= lim31 || (int64_t)height * stride >= lim31) return false;
    const int64_t row_bytes = blocks_x * block_row_bytes;               // below 2^29 * block_row_bytes: no overflow
    if ((blocks_y * 4 - 1) * stride + row_bytes >= lim31) return false;
    return out_bytes >= 0 && out_bytes < ((int64_t)1 << 32);
}

} // namespace itw
