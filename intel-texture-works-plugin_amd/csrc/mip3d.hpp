// mip3d.hpp -- what mipgen.hip's entry points hand a call with ITW_MIP_VOLUME to (mip3d.hip; include/itw_dispatch.h, "Mip chains: volumes").
// `who` names the entry point in every message; `flags` come without the ITW_MIP_VOLUME bit.
#pragma once
#include <cstdint>
#include "../../include/itw_dispatch.h"

namespace itw {

int mip_levels_3d(int width, int height, int depth);                                  // 1 + floor(log2(max(w, h, d))); 0 for a size below 1
int mip_slices_3d(int depth, int levels);                                             // sum over l < levels of max(1, depth >> l); -1 on bad arguments
int64_t mip_chain_layout_3d(int width, int height, int depth, int levels, int pixel_size, uint8_t* storage, rgba_surface* out);
int generate_mip_chain_3d(const char* who, const rgba_surface* slices, int depth, int levels, int pixel_size, uint32_t flags);
bool compress_volume_mipped(const char* who, const rgba_surface* base_slices, int depth, int levels, uint32_t mip_flags, uint8_t* target, int dxgi_format,
                            const void* settings, ItwProgressFunc* progress, void* user);

} // namespace itw
