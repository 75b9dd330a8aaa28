// image_list_host.hpp -- what the texel stages (mipgen.hip, mip_alpha.hip, normal_prep.hip) and the chain entry points ask of a list of
// rgba_surface images before any device work, and where a list of host images is staged in a thread's device buffer.  One definition of
// each rule; the HIP-side half (messages, pointer kinds, the copies) is host_rt.hpp's.  Plain C++, so that a host-only program can run it
// under a sanitizer (tools/image_list_host_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../include/ispc_texcomp.h"

namespace itw {

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// A quad is four consecutive texels of one row, a lane's share in the stream kernels: ceil(width / 4) * height of them per image, and a
// launch of 256-lane workgroups covers a list while its workgroup count stays an int32.
inline int64_t texel_quads(int width, int height) { return (int64_t)((width + 3) >> 2) * height; }
inline bool quads_fit_one_launch(int64_t quads) { return (quads + 255) / 256 <= (int64_t)0x7fffffff; }

// The first thing wrong with an image, in this order.  ALIGN: the pointer, or the row step of an image of more than one row, is no multiple
// of the alignment asked for.
enum ImageFaultKind { IMAGE_OK = 0, IMAGE_NULL_TEXELS, IMAGE_SIZE, IMAGE_STRIDE, IMAGE_ALIGN };
struct ImageFault {
    ImageFaultKind kind = IMAGE_OK;
    int index = -1;                                 // of the image in its list
    explicit operator bool() const { return kind != IMAGE_OK; }
};

// `align`: a power of two, or 0 for texels that may sit anywhere
inline ImageFaultKind image_fault(const rgba_surface& s, int texel_bytes, int align)
{
    if (!s.ptr) return IMAGE_NULL_TEXELS;
    if (s.width < 1 || s.height < 1) return IMAGE_SIZE;
    if ((int64_t)s.stride < (int64_t)s.width * texel_bytes) return IMAGE_STRIDE;
    const uintptr_t row_step = s.height > 1 ? (uintptr_t)(uint32_t)s.stride : 0;
    if (align && (((uintptr_t)s.ptr | row_step) & (uintptr_t)(align - 1))) return IMAGE_ALIGN;
    return IMAGE_OK;
}

// the first faulty image of a list and what is wrong with it
inline ImageFault image_list_fault(const rgba_surface* images, int count, int texel_bytes, int align)
{
    for (int i = 0; i < count; i++) {
        const ImageFaultKind k = image_fault(images[i], texel_bytes, align);
        if (k != IMAGE_OK) return ImageFault{k, i};
    }
    return ImageFault{};
}

// Where the images of a list are on the device's side of a call whose buffer starts with `head` bytes of the caller's own (a table, a work
// area, an earlier plan).  Device images stay where they are, rows at the caller's stride.  Host images are staged behind the head: rows of
// a 16-byte multiple (a row quad that starts at a 16-byte address is one vector access), each image at a 256-byte multiple.  `bytes`: the
// end of the last image, the head rounded up to 256 when nothing is staged.  Offsets only: the buffer's address joins them in ptr(), so
// that a plan sizes the buffer it is then bound to.
struct StagingPlan {
    const rgba_surface* images = nullptr;
    int count = 0, texel_bytes = 0;
    bool dev = true;
    size_t bytes = 0;
    struct Staged { size_t offset; int64_t stride; };
    std::vector<Staged> at;                         // per image; empty for device images

    StagingPlan(const rgba_surface* list, int n, int texel, bool device, size_t head)
        : images(list), count(n), texel_bytes(texel), dev(device), bytes(up256(head))
    {
        if (dev) return;
        at.resize((size_t)count);
        for (int i = 0; i < count; i++) {
            at[(size_t)i].offset = bytes;
            at[(size_t)i].stride = (int64_t)((row_bytes(i) + 15) & ~(size_t)15);
            bytes += up256((size_t)at[(size_t)i].stride * (size_t)images[i].height);
        }
    }
    size_t row_bytes(int i) const { return (size_t)images[i].width * (size_t)texel_bytes; }
    int64_t stride(int i) const { return dev ? (int64_t)images[i].stride : at[(size_t)i].stride; }
    uint8_t* ptr(int i, uint8_t* base) const { return dev ? images[i].ptr : base + at[(size_t)i].offset; }
};

} // namespace itw
