// bc6hs_host_check.cpp -- the BC6H decoder's own text (csrc/decode_core.hpp: decode_block<BCN_BC6HS> and, for comparison, <BCN_BC6H>) run on
// the host, block after block.  tests/test_bc6hs_cpu.py compares what it writes with the reference's recorded D3DXDecodeBC6HS output, so
// the kernels' decoder is checked where there is no GPU.  decode_core.hpp is included as it is; tools/host_stub/hip/hip_runtime.h stands in
// for the HIP header.  A stand-alone program: it can be built with -fsanitize=address,undefined as well.
//   g++ -std=c++17 -O2 -Itools/host_stub tools/bc6hs_host_check.cpp -o /tmp/bc6hs_host_check
//   /tmp/bc6hs_host_check blocks.bin texels.bin modes.bin <signed: 1 | 0>
// blocks.bin: n blocks of 16 bytes; texels.bin: n x 16 RGBA16F texels (8 bytes each, raster order inside the block); modes.bin: n int32.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../intel-texture-works-plugin_amd/csrc/decode_core.hpp"

int main(int argc, char** argv)
{
    if (argc != 5) { std::fprintf(stderr, "usage: %s blocks.bin texels.bin modes.bin signed\n", argv[0]); return 2; }
    const bool is_signed = std::atoi(argv[4]) != 0;
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::perror(argv[1]); return 1; }
    std::vector<uint4> blocks;
    uint4 w;
    while (std::fread(&w, 16, 1, in) == 1) blocks.push_back(w);
    std::fclose(in);
    std::vector<uint32_t> texels(blocks.size() * 32);
    std::vector<int32_t> modes(blocks.size());
    for (size_t b = 0; b < blocks.size(); b++) {
        uint32_t lo[16], hi[16];
        modes[b] = is_signed ? itw::decode_block<itw::BCN_BC6HS>(blocks[b], lo, hi) : itw::decode_block<itw::BCN_BC6H>(blocks[b], lo, hi);
        for (int k = 0; k < 16; k++) { texels[b * 32 + 2 * k] = lo[k]; texels[b * 32 + 2 * k + 1] = hi[k]; }
    }
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out || std::fwrite(texels.data(), 4, texels.size(), out) != texels.size()) { std::perror(argv[2]); return 1; }
    std::fclose(out);
    out = std::fopen(argv[3], "wb");
    if (!out || std::fwrite(modes.data(), 4, modes.size(), out) != modes.size()) { std::perror(argv[3]); return 1; }
    std::fclose(out);
    return 0;
}
