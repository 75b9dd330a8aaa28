// texel_rows.hpp -- what the kernels that compare a block with its source share (measure.hip, refine.hip): a block's source rows as
// row-wide vector loads, and the wave64 reductions their sums and maxima end in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace itw {

// a dword from a source whose alignment is whatever the caller's pointer and stride make it
__device__ __forceinline__ uint32_t measure_load_u32(const uint8_t* p)
{
    if (((uintptr_t)p & 3) == 0) return *reinterpret_cast<const uint32_t*>(p);
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// the DW dwords (4 texels) of one source row of a block; texels at and beyond column nx are not read (they come back as 0 and are not compared)
template <int DW>
__device__ __forceinline__ void measure_load_row(const uint8_t* p, int nx, uint32_t (&v)[DW])
{
    constexpr int PER = DW / 4;                                 // dwords per texel
    if (nx == 4 && ((uintptr_t)p & 15) == 0) {
#pragma unroll
        for (int q = 0; q < DW / 4; q++) {
            const uint4 t = reinterpret_cast<const uint4*>(p)[q];
            v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 4; c++)
#pragma unroll
            for (int q = 0; q < PER; q++) v[c * PER + q] = c < nx ? measure_load_u32(p + (c * PER + q) * 4) : 0u;
    }
}

template <class T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
template <class T>
__device__ __forceinline__ T wave_max(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const T u = __shfl_xor(v, o); v = u > v ? u : v; }
    return v;
}

} // namespace itw
