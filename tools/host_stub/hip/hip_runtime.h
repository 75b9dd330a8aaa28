// A stand-in for <hip/hip_runtime.h> for host-only programs that compile the library's device-side decoder text with a plain C++ compiler
// (tools/bc6hs_host_check.cpp: g++ -Itools/host_stub ...): the qualifiers vanish, and the handful of vector types and functions that
// csrc/decode_core.hpp uses exist as ordinary C++.  Not used by any build of the library.
#pragma once
#include <algorithm>
#include <cstdint>

#define __device__
#define __host__
#define __forceinline__ inline
#define __restrict__

struct uint2 { uint32_t x, y; };
struct alignas(16) uint4 { uint32_t x, y, z, w; };
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
using std::max;
using std::min;
