// encode_dds -- a C++ host above the C ABI, the way the plugin's save path uses it (IntelPlugin.cpp:186-261, 816-884):
// raw texels -> pad to multiples of 4 -> CompressImageMT through the slice loop -> .DDS file.  Only include/*.h is used;
// the program links libispc_texcomp.so like the plugin links ispc_texcomp.lib.
//
//   encode_dds [--measure] [--refine <profile> <max_block_sse> | --refine-share <profile> <percent> | --refine-psnr <profile> <dB>]
//              [--normal flipx,flipy,normalize | --signed-normal int8|half|float[,flipx,flipy,normalize]] [--cube-cross] [--mips [levels] [--srgb-mips]]
//              [--height r|g|b|a|lum[,mirroru,mirrorv,invert,occlusion] [--height-amplitude <A>]]
//              [--alpha-weight] [--alpha-coverage <ref>] [--bc-dither rgb|a|rgb,a] [--bc-uniform]
//              <format> <width> <height> <in.raw> <out.dds> [slice_pixels]
//     format : bc1 | bc1a[:<alpha_ref>] | bc2 | bc3 | bc3_dxtex | bc4 | bc5 | bc4_snorm | bc5_snorm | bc7_<profile> | bc6h_<profile> | etc1_slow      (profiles: the GetProfile_* names)
//              bc1a: BC1 with 1-bit alpha by DirectXTex's encoder (ITW_FORMAT_BC1A_UNORM, itw_dispatch.h): a texel whose alpha is below <alpha_ref>
//              (a float, default 0.5) is transparent; --bc-dither and --bc-uniform are its flags (ITW_BC_DITHER_RGB / _A, ITW_BC_UNIFORM).  The file
//              is a BC1 file (DXGI 71).  It has no trampoline: the slices go through itwCompressImageSlicedEx; goes with --mips, --alpha-weight,
//              --alpha-coverage (pass alpha_ref = ref / 255), --cube-cross, --measure; --refine* and --normal are refused
//              bc2: BC2 (DXT3: 4 bits of explicit alpha per texel) by DirectXTex's encoder (ITW_FORMAT_BC2_UNORM, itw_dispatch.h); --bc-dither and
//              --bc-uniform are its flags too; the file is a DXT3 file (DX10 with 74 for an array).  Like bc1a it goes through
//              itwCompressImageSlicedEx, with --mips, --alpha-weight, --alpha-coverage, --cube-cross, --measure; --refine* and --normal are refused
//              bc3_dxtex: BC3 by DirectXTex's encoder, D3DXEncodeBC3 (ITW_FORMAT_BC3_DXTEX, itw_dispatch.h) -- the bytes of `texconv -f DXT5`; bc3 stays
//              kernel.ispc's encoder.  --bc-dither (a: the alpha indices; rgb: the colour half) and --bc-uniform are its flags too; the file is a
//              DXT5 file (DX10 with 77 for an array), which --decode reads like any other.  Like bc2 it goes through itwCompressImageSlicedEx, with
//              --mips, --resize, --alpha-weight, --alpha-coverage, --cube-cross, --measure; --refine* and --normal are refused
//              etc1_slow: DDS has no code for ETC1, so the output is a KTX 1.1 file (itwKtx*, itw_dds.h); the slices go through itwCompressImageSlicedEx
//              (ETC1 has no trampoline); --refine* is refused: ETC1 has one preset
//     in.raw : width*height tightly packed RGBA8 texels (RGBA16F bit patterns for bc6h_*; RGBA8_SNORM, int8 codes, for bc4_snorm / bc5_snorm)
//     --measure : after encoding, one line on stdout per image: what the stream costs against the source (itwMeasureBlocks)
//     --refine  : bc7_* / bc6h_* only: encode to an error budget (itwCompressImageRefined) -- <format>'s preset everywhere, then <profile>
//                 (a preset of the same format: `slow`, `alpha_slow`, ...) on the blocks whose error is above <max_block_sse>, kept where
//                 it is strictly better; one line on stdout with the call's statistics.  The slice loop is not used.
//     --refine-share : the same with the budget chosen on the device (itwCompressImageRefinedTo): <profile> on at most <percent> % of
//                 the blocks, the worst ones, in one round
//     --refine-psnr  : bc7_* only: <profile> on as many of the worst blocks as it takes to reach <dB> over the format's own channels
//                 (itwPsnrToTotalSse gives the target), in up to five rounds
//     --normal flipx,flipy,normalize : the input is a normal map; the named stages of the plugin's save path (FlipXYChannelNormalMap,
//                 NormalizeNormalMapChain) are applied as the texels are encoded -- bc5 through itwCompressNormalMapBC5 (one kernel), any
//                 other format through itwCompressNormalMapChain.  The slice loop is not used; not with --refine*.
//     --signed-normal int8|half|float[,flipx,flipy,normalize] : bc4_snorm / bc5_snorm only: the raw file is a SIGNED normal source of the
//                 named texel kind (RGBA8_SNORM codes, RGBA16F halfs or RGBA32F floats; itw_dispatch.h, "signed normal sources") and the
//                 stages have their signed meaning: negate x / y, normalise in fp32, quantise with round to nearest even.  bc5_snorm goes
//                 through itwCompressNormalMapBC5S (one kernel), bc4_snorm through itwCompressSignedNormalMapChain with one image; with
//                 --cube-cross the six faces through that chain call, with --mips everything through itwCompressSignedNormalMapMipped.
//                 Not with --normal (whose biased 8-bit behaviour stays), --refine* or --measure; the slice loop is not used.
//     --height r|g|b|a|lum[,mirroru,mirrorv,invert,occlusion], --height-amplitude <A> : with --normal or --signed-normal: the input is a
//                 HEIGHT map (bump, displacement), and DirectXTex's ComputeNormalMap (Texconv's -nmap / -nmapamp) makes the normal map from the
//                 named channel first: ITW_NORMAL_FROM_HEIGHT in the calls' `ops` word (itw_dispatch.h, "height maps").  An axis wraps unless
//                 mirrored; occlusion puts the occlusion term into alpha; A (default 1) is rounded to a half.  With --mips the one-call saves take
//                 the word themselves (the stage writes level 0); without, the stage runs first over the image or each cross face --
//                 itwPrepareNormalMapChain in place for --normal, itwQuantizeNormalMapChain into an int8 map for --signed-normal -- with the
//                 flips and the normalise, and the encoders then see a finished map.
//     --cube-cross : the input is a horizontal (4 x 3 faces) or vertical (3 x 4) cube cross; its six faces (itwCubeCrossFaces: views, no
//                 copy) are encoded by one chain call into a cube-map DDS.  Goes with --normal; not with --refine*, --measure or etc1_slow.
//     --mips [levels] : a mipped file from the base image (or the six cross faces) in one call, itwCompressImageMipped: the save path's
//                 order -- the flips of --normal on level 0, DirectXTex's box / linear mip filter, the normalise on every level, every image
//                 encoded.  levels: how many, the base included (default: the full chain).  Every format; goes with --normal and
//                 --cube-cross; not with --refine* or --measure.  The header carries the image's own size: level l is max(1, w >> l) wide.
//     --srgb-mips : with --mips: the texels' R, G, B are sRGB coded and every level is filtered in linear light (itwCompressImageMippedEx with
//                 ITW_MIP_SRGB; alpha stays linear).  RGBA8 colour formats only: not with bc6h_*, the SNORM pair or --normal.
//     --alpha-weight, --alpha-coverage <ref> : with --mips: the rules for cut-out textures (itwCompressImageMippedAlpha; itw_dispatch.h,
//                 "Mip chains of cut-out textures") -- colour weighted by alpha, so what alpha 0 hides stays out of the levels, and the
//                 share of texels passing `alpha >= ref` (1 .. 255) kept at every level.  With --alpha-coverage one line on stdout per
//                 image: texels, the count passing before and after, the threshold chosen (itwGenerateMipChainAlpha's report).  RGBA8
//                 colour formats only, as --srgb-mips; not with --normal.
//     --mip-filter cubic|triangle, --mip-wrap u|v|uv : with --mips: DirectXTex's cubic or triangle filter on every level in place of the
//                 default's box / linear (ITW_MIP_CUBIC / ITW_MIP_TRIANGLE), and wrap addressing along x, y or both for a tiling texture
//                 (ITW_MIP_WRAP_U / _V; it changes nothing under the default filter).  Every format; go with --srgb-mips,
//                 --alpha-coverage, --normal and --cube-cross; not with --alpha-weight or --signed-normal.
//     --resize WxH | --fit pow2, --resize-filter point|linear|cubic|triangle : the first stage of a texture pipeline, texconv's -w / -h /
//                 -pow2: the image is fitted to W x H, or to the power-of-two size nearest its own (the longer axis down to a power of
//                 two, the other to the one that keeps the aspect best), before everything else -- the normal stages, --mips, the
//                 encode.  DirectX::Resize on the device (itwGenerateMipChain with ITW_MIP_RESIZE over two levels); without
//                 --resize-filter the reference's default, box at exactly 2:1 and linear otherwise.  --srgb-mips and --mip-wrap hold
//                 for this stage too (the linear filter refuses wrap on an axis that grows).  Not with --cube-cross or --signed-normal.
//     --volume <depth> : a volume texture (3D LUT, fog or cloud density, 3D noise).  in.raw holds <depth> slices of width x height, one
//                 after another, and the output is a volume DDS (ITW_DDS_VOLUME, itw_dds.h: slices level-major) from one call,
//                 itwCompressImageMippedEx with ITW_MIP_VOLUME.  --mips [levels] builds the 3D chain by DirectXTex's default, box for power-of-two sizes and
//                 triangle otherwise; --mip-filter point|linear|cubic|triangle names the filter (point and linear are the volume's alone) and
//                 --mip-wrap takes the letters u, v, w in that order (w is the volume's alone); --srgb-mips as for an image.  --measure prints
//                 one line per slice of every level (itwMeasureChain over the generated chain).  Not with --normal, --signed-normal,
//                 --height, --cube-cross, --refine*, --alpha-weight, --alpha-coverage, --resize, --fit, etc1_slow or a slice size.
//
//   encode_dds --decode <in.dds | in.ktx> <out.raw>
//     (.dds or .ktx: told apart by the file's first bytes; a KTX file's images come in ITS order, level then face)
//     the load path (IntelPlugin.cpp:2461-2561): header -> every image of the file through ONE itwDecodeChain -> texels.  out.raw holds
//     every image's texels one after another in file order, tightly packed (RGBA8; RGBA16F bit patterns for BC6H; int8 codes for the
//     SNORM pair); one line on stdout per image: index, width, height, min alpha (the smallest decoded alpha code: IsAlphaAllOpaque).
//     A BC6H_SF16 file (DX10 format 96) is decoded and previewed by the signed reading, ITW_FORMAT_BC6H_SIGNED: as a GPU shows it.
//     A volume DDS is read in its own order, level-major; its lines end in the slice's level and number.
//
//   encode_dds --preview <in.dds | in.ktx> <image index> <out.ppm> <w> <h> <x> <y> <zoom> [channels] [exposure] [matte]
//     the preview path (IntelPlugin::FetchPreviewRGB): a w x h viewport of ONE image of the file (itwDdsImage / itwKtxImage's index), decoded
//     only where the viewport looks (itwPreviewBlocks), written as a binary PPM.  x, y: the viewport's offset in its own pixels; zoom: source
//     texels per viewport pixel (the caller divides by 1 << mip level to show a mip at the base image's scale); channels: letters of rgba
//     (default rgb); exposure: BC6H only (default 1); matte: 0xBBGGRR outside the image (default 0).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../include/ispc_texcomp.h"
#include "../include/itw_amd.h"
#include "../include/itw_bc45.h"
#include "../include/itw_dds.h"
#include "../include/itw_decode.h"
#include "../include/itw_dispatch.h"

namespace {

struct Format { const char* name; CompressionFunc* fn; int dxgi; int texel_bytes; bool pad; unsigned own_channels; };   // own_channels: bit 0 = R .. bit 3 = A

const Format kFormats[] = {
    {"bc1", CompressImageBC1, ITW_DXGI_FORMAT_BC1_UNORM, 4, true, 7},
    {"bc1a", nullptr, ITW_FORMAT_BC1A_UNORM, 4, false, 15},                     // no trampoline: itwCompressImageSlicedEx; a DirectXTex format, written as 71
    {"bc2", nullptr, ITW_FORMAT_BC2_UNORM, 4, false, 15},                       // no trampoline either; a DirectXTex format, written as DXT3 / 74
    {"bc3", CompressImageBC3, ITW_DXGI_FORMAT_BC3_UNORM, 4, true, 15},
    {"bc3_dxtex", nullptr, ITW_FORMAT_BC3_DXTEX, 4, false, 15},                 // no trampoline either; DirectXTex's BC3 encoder, written as DXT5 / 77
    {"bc4", CompressImageBC4, ITW_DXGI_FORMAT_BC4_UNORM, 4, false, 1},      // DirectXTex formats keep partial blocks
    {"bc5", CompressImageBC5, ITW_DXGI_FORMAT_BC5_UNORM, 4, false, 3},
    {"bc4_snorm", CompressImageBC4S, ITW_DXGI_FORMAT_BC4_SNORM, 4, false, 1},   // the raw file's bytes are int8 codes (normal maps)
    {"bc5_snorm", CompressImageBC5S, ITW_DXGI_FORMAT_BC5_SNORM, 4, false, 3},
    {"bc7_ultrafast", CompressImageBC7_ultrafast, ITW_DXGI_FORMAT_BC7_UNORM, 4, true, 7},
    {"bc7_veryfast", CompressImageBC7_veryfast, ITW_DXGI_FORMAT_BC7_UNORM, 4, true, 7},
    {"bc7_fast", CompressImageBC7_fast, ITW_DXGI_FORMAT_BC7_UNORM, 4, true, 7},
    {"bc7_basic", CompressImageBC7_basic, ITW_DXGI_FORMAT_BC7_UNORM, 4, true, 7},
    {"bc7_slow", CompressImageBC7_slow, ITW_DXGI_FORMAT_BC7_UNORM, 4, true, 7},
    {"bc7_alpha_ultrafast", CompressImageBC7_alpha_ultrafast, ITW_DXGI_FORMAT_BC7_UNORM, 4, true, 15},
    {"bc7_alpha_veryfast", CompressImageBC7_alpha_veryfast, ITW_DXGI_FORMAT_BC7_UNORM, 4, true, 15},
    {"bc7_alpha_fast", CompressImageBC7_alpha_fast, ITW_DXGI_FORMAT_BC7_UNORM, 4, true, 15},
    {"bc7_alpha_basic", CompressImageBC7_alpha_basic, ITW_DXGI_FORMAT_BC7_UNORM, 4, true, 15},
    {"bc7_alpha_slow", CompressImageBC7_alpha_slow, ITW_DXGI_FORMAT_BC7_UNORM, 4, true, 15},
    {"bc6h_veryfast", CompressImageBC6H_veryfast, ITW_DXGI_FORMAT_BC6H_UF16, 8, true, 7},
    {"bc6h_fast", CompressImageBC6H_fast, ITW_DXGI_FORMAT_BC6H_UF16, 8, true, 7},
    {"bc6h_basic", CompressImageBC6H_basic, ITW_DXGI_FORMAT_BC6H_UF16, 8, true, 7},
    {"bc6h_slow", CompressImageBC6H_slow, ITW_DXGI_FORMAT_BC6H_UF16, 8, true, 7},
    {"bc6h_veryslow", CompressImageBC6H_veryslow, ITW_DXGI_FORMAT_BC6H_UF16, 8, true, 7},
    {"etc1_slow", nullptr, ITW_FORMAT_ETC1_RGB8, 4, true, 7},                  // no trampoline: itwCompressImageSlicedEx; written as .ktx
};

// GetProfile_<name> / GetProfile_bc6h_<name> into `settings` (room for either struct); false: no such preset
bool profile_by_name(bool bc6h, const char* name, void* settings)
{
    struct P7 { const char* name; void (*get)(bc7_enc_settings*); };
    struct P6 { const char* name; void (*get)(bc6h_enc_settings*); };
    static const P7 k7[] = {{"ultrafast", GetProfile_ultrafast}, {"veryfast", GetProfile_veryfast}, {"fast", GetProfile_fast}, {"basic", GetProfile_basic},
                            {"slow", GetProfile_slow}, {"alpha_ultrafast", GetProfile_alpha_ultrafast}, {"alpha_veryfast", GetProfile_alpha_veryfast},
                            {"alpha_fast", GetProfile_alpha_fast}, {"alpha_basic", GetProfile_alpha_basic}, {"alpha_slow", GetProfile_alpha_slow}};
    static const P6 k6[] = {{"veryfast", GetProfile_bc6h_veryfast}, {"fast", GetProfile_bc6h_fast}, {"basic", GetProfile_bc6h_basic},
                            {"slow", GetProfile_bc6h_slow}, {"veryslow", GetProfile_bc6h_veryslow}};
    if (bc6h) { for (const P6& p : k6) if (std::strcmp(p.name, name) == 0) { p.get(static_cast<bc6h_enc_settings*>(settings)); return true; } }
    else      { for (const P7& p : k7) if (std::strcmp(p.name, name) == 0) { p.get(static_cast<bc7_enc_settings*>(settings)); return true; } }
    return false;
}

itw_bc1a_settings g_bc1a = { (uint32_t)sizeof(itw_bc1a_settings), 0.5f, 0, 0 };      // bc1a[:<alpha_ref>], bc2 and bc3_dxtex, --bc-dither, --bc-uniform
bool takes_bc_settings(int dxgi) { return dxgi == ITW_FORMAT_BC1A_UNORM || dxgi == ITW_FORMAT_BC2_UNORM || dxgi == ITW_FORMAT_BC3_DXTEX; }

bool on_progress(int done, int total, void*)
{
    std::fprintf(stderr, "\rslice %d / %d", done, total);
    return true;                                                   // false would abort like the plugin's cancel button
}

// encode_dds --normal / --cube-cross: `source` (or its six cross faces) through ONE call that pads, prepares and encodes
int encode_normal_or_cross(const Format& f, const rgba_surface& source, uint32_t ops, bool cube_cross, bool measure, const char* out_path)
{
    const bool bc7 = std::strncmp(f.name, "bc7_", 4) == 0, bc6h = std::strncmp(f.name, "bc6h_", 5) == 0, etc1 = f.dxgi == ITW_FORMAT_ETC1_RGB8;
    union { bc7_enc_settings s7; bc6h_enc_settings s6; etc_enc_settings se; } settings;
    if (etc1) itwGetProfile_etc_slow(&settings.se);
    else if ((bc7 || bc6h) && !profile_by_name(bc6h, f.name + (bc7 ? 4 : 5), &settings)) return 2;
    rgba_surface images[6] = {source};
    int count = 1;
    if (cube_cross) {
        if (itwCubeCrossFaces(&source, f.texel_bytes, images) != 0) { std::fprintf(stderr, "%d x %d is too small for a cube cross\n", source.width, source.height); return 2; }
        count = 6;
    }
    const int64_t bytes = itwChainBytes(images, count, f.dxgi);
    if (bytes <= 0) { std::fprintf(stderr, "bad size\n"); return 2; }
    std::vector<uint8_t> blocks((size_t)bytes);
    itwSetErrorMode(ITW_ON_ERROR_RETURN);
    bool ok;
    if (f.dxgi == ITW_DXGI_FORMAT_BC5_UNORM && !cube_cross) {      // the plugin's normal-map format: the stages run inside the encoder
        itwCompressNormalMapBC5(&source, blocks.data(), ops);
        ok = itwLastError() == nullptr;
    } else {
        ok = (takes_bc_settings(f.dxgi) && !ops) ? itwCompressImageChainEx(images, count, blocks.data(), f.dxgi, &g_bc1a, nullptr, nullptr)
                                                       : itwCompressNormalMapChain(images, count, blocks.data(), f.dxgi, &settings, ops, nullptr, nullptr);
    }
    if (!ok) { std::fprintf(stderr, "%s\n", itwLastError() ? itwLastError() : "compression failed"); return 1; }
    if (measure) {
        // against the PREPARED texels: what the stream was encoded from
        std::vector<uint8_t> prepared((size_t)source.stride * source.height);
        std::memcpy(prepared.data(), source.ptr, prepared.size());
        rgba_surface p = source;
        p.ptr = prepared.data();
        itw_error_stats st;
        if (itwPrepareNormalMapChain(&p, 1, f.texel_bytes, ops) != 0 || itwMeasureBlocks(f.dxgi, blocks.data(), &p, &st, sizeof st, nullptr) != 0) {
            std::fprintf(stderr, "measurement failed\n");
            return 1;
        }
        std::printf("image 0: %dx%d %s", st.width, st.height, f.name);
        if (f.texel_bytes == 4) std::printf(" psnr %.4f dB", itwStatsPsnr(&st, f.own_channels));
        std::printf(" sse [%llu, %llu, %llu, %llu] max_abs [%u, %u, %u, %u]\n", (unsigned long long)st.sse[0], (unsigned long long)st.sse[1],
                    (unsigned long long)st.sse[2], (unsigned long long)st.sse[3], st.max_abs[0], st.max_abs[1], st.max_abs[2], st.max_abs[3]);
    }
    // formats that pad store the padded size, as the save path does; the DirectXTex formats keep the image's own
    const uint32_t w = f.pad ? (uint32_t)((images[0].width + 3) & ~3) : (uint32_t)images[0].width, h = f.pad ? (uint32_t)((images[0].height + 3) & ~3) : (uint32_t)images[0].height;
    ItwDdsDesc desc = { w, h, 1, (uint32_t)f.dxgi, cube_cross ? 1u : 0u, 1 };
    ItwKtxDesc kdesc = { w, h, 1, ITW_FORMAT_ETC1_RGB8, 0, 0 };
    std::vector<uint8_t> file(etc1 ? itwKtxFileBytes(&kdesc) : itwDdsFileBytes(&desc));
    const uint8_t* levels[6];
    for (int i = 0; i < count; i++) levels[i] = blocks.data() + (size_t)i * (blocks.size() / (size_t)count);      // the faces are equal
    if ((etc1 ? itwKtxWriteFile(&kdesc, levels, 1, file.data(), file.size()) : itwDdsWriteFile(&desc, levels, (size_t)count, file.data(), file.size())) != file.size()
        || file.empty()) {
        std::fprintf(stderr, "%s assembly failed\n", etc1 ? "KTX" : "DDS");
        return 1;
    }
    FILE* out = std::fopen(out_path, "wb");
    if (!out || std::fwrite(file.data(), 1, file.size(), out) != file.size()) { std::fprintf(stderr, "cannot write %s\n", out_path); return 1; }
    std::fclose(out);
    DestroyThreads();
    std::fprintf(stderr, "%s: %ux%u%s -> %zu bytes (%s, normal ops %u)\n", out_path, w, h, cube_cross ? " x 6 faces" : "", file.size(), f.name, ops);
    return 0;
}

// encode_dds --mips: the base image (or its six cross faces) to a mipped DDS / KTX in one call; levels == 0: the full chain
int encode_mipped(const Format& f, const rgba_surface& source, uint32_t ops, uint32_t mip_flags, const itw_mip_alpha* alpha, bool cube_cross, int levels,
                  const char* out_path)
{
    const bool bc7 = std::strncmp(f.name, "bc7_", 4) == 0, bc6h = std::strncmp(f.name, "bc6h_", 5) == 0, etc1 = f.dxgi == ITW_FORMAT_ETC1_RGB8;
    union { bc7_enc_settings s7; bc6h_enc_settings s6; etc_enc_settings se; } settings;
    if (etc1) itwGetProfile_etc_slow(&settings.se);
    else if ((bc7 || bc6h) && !profile_by_name(bc6h, f.name + (bc7 ? 4 : 5), &settings)) return 2;
    rgba_surface bases[6] = {source};
    int items = 1;
    if (cube_cross) {
        if (itwCubeCrossFaces(&source, f.texel_bytes, bases) != 0) { std::fprintf(stderr, "%d x %d is too small for a cube cross\n", source.width, source.height); return 2; }
        items = 6;
    }
    const int w = bases[0].width, h = bases[0].height, full = itwMipLevels(w, h);
    if (levels < 0 || levels > full) { std::fprintf(stderr, "--mips %d: a full chain of %d x %d has %d levels\n", levels, w, h, full); return 2; }
    if (levels == 0) levels = full;
    std::vector<rgba_surface> chain((size_t)items * levels);
    if (itwMipChainLayout(w, h, items, levels, f.texel_bytes, nullptr, chain.data()) < 0) { std::fprintf(stderr, "bad size\n"); return 2; }
    const int64_t bytes = itwChainBytes(chain.data(), items * levels, f.dxgi);      // (sizes only: the layout's pointers are offsets)
    if (bytes <= 0) { std::fprintf(stderr, "bad size\n"); return 2; }
    std::vector<uint8_t> blocks((size_t)bytes);
    itwSetErrorMode(ITW_ON_ERROR_RETURN);
    const void* sp = takes_bc_settings(f.dxgi) ? (const void*)&g_bc1a : (const void*)&settings;
    const bool done = alpha ? itwCompressImageMippedAlpha(bases, items, levels, mip_flags, alpha, blocks.data(), f.dxgi, sp, nullptr, nullptr)
                            : itwCompressImageMippedEx(bases, items, levels, ops, mip_flags, blocks.data(), f.dxgi, sp, nullptr, nullptr);
    if (!done) {
        std::fprintf(stderr, "%s\n", itwLastError() ? itwLastError() : "compression failed");
        return 1;
    }
    if (alpha && alpha->coverage_ref) {                              // the report: the same chain once more, in host memory
        std::vector<uint8_t> texels((size_t)itwMipChainLayout(w, h, items, levels, 4, nullptr, nullptr));
        std::vector<itw_mip_coverage> rows((size_t)items * levels);
        itwMipChainLayout(w, h, items, levels, 4, texels.data(), chain.data());
        for (int i = 0; i < items; i++)
            for (int y = 0; y < h; y++) std::memcpy(chain[(size_t)i * levels].ptr + (size_t)y * w * 4, bases[i].ptr + (size_t)y * bases[i].stride, (size_t)w * 4);
        if (itwGenerateMipChainAlpha(chain.data(), items, levels, mip_flags, alpha, rows.data()) != 0) {
            std::fprintf(stderr, "%s\n", itwLastError() ? itwLastError() : "the report failed");
            return 1;
        }
        for (size_t i = 0; i < rows.size(); i++)
            std::printf("coverage item %zu level %zu texels %llu before %llu after %llu threshold %u\n", i / levels, i % levels, (unsigned long long)rows[i].texels,
                        (unsigned long long)rows[i].covered_plain, (unsigned long long)rows[i].covered, rows[i].threshold);
    }
    ItwDdsDesc desc = { (uint32_t)w, (uint32_t)h, (uint32_t)levels, (uint32_t)f.dxgi, cube_cross ? 1u : 0u, 1 };
    ItwKtxDesc kdesc = { (uint32_t)w, (uint32_t)h, (uint32_t)levels, ITW_FORMAT_ETC1_RGB8, 0, 0 };
    std::vector<uint8_t> file(etc1 ? itwKtxFileBytes(&kdesc) : itwDdsFileBytes(&desc));
    std::vector<const uint8_t*> images((size_t)items * levels);      // DDS: face-major, then level -- the call's order; KTX here: one face
    size_t at = 0;
    for (size_t i = 0; i < images.size(); i++) {
        images[i] = blocks.data() + at;
        at += etc1 ? itwKtxImage(&kdesc, (uint32_t)i, nullptr, nullptr, nullptr) : itwDdsImage(&desc, (uint32_t)i, nullptr, nullptr, nullptr);
    }
    if (at != blocks.size() || file.empty()
        || (etc1 ? itwKtxWriteFile(&kdesc, images.data(), images.size(), file.data(), file.size())
                 : itwDdsWriteFile(&desc, images.data(), images.size(), file.data(), file.size())) != file.size()) {
        std::fprintf(stderr, "%s assembly failed\n", etc1 ? "KTX" : "DDS");
        return 1;
    }
    FILE* out = std::fopen(out_path, "wb");
    if (!out || std::fwrite(file.data(), 1, file.size(), out) != file.size()) { std::fprintf(stderr, "cannot write %s\n", out_path); return 1; }
    std::fclose(out);
    DestroyThreads();
    std::fprintf(stderr, "%s: %dx%d%s, %d levels -> %zu bytes (%s, normal ops %u)\n", out_path, w, h, cube_cross ? " x 6 faces" : "", levels, file.size(), f.name, ops);
    return 0;
}

// encode_dds --volume: `depth` slices of width x height to a volume DDS in one call; levels == 0: the full chain, 1: no mips
int encode_volume(const Format& f, uint8_t* texels, int w, int h, int depth, int levels, uint32_t mip_flags, bool measure, const char* out_path)
{
    const bool bc7 = std::strncmp(f.name, "bc7_", 4) == 0, bc6h = std::strncmp(f.name, "bc6h_", 5) == 0;
    union { bc7_enc_settings s7; bc6h_enc_settings s6; } settings;
    if ((bc7 || bc6h) && !profile_by_name(bc6h, f.name + (bc7 ? 4 : 5), &settings)) return 2;
    const int full = itwMipLevels(w > h ? w : h, depth);            // 1 + floor(log2(max(w, h, d)))
    if (levels < 0 || levels > full) { std::fprintf(stderr, "--mips %d: a full chain of %d x %d x %d has %d levels\n", levels, w, h, depth, full); return 2; }
    if (levels == 0) levels = full;
    // the slice list, level-major, packed with tight rows; `storage` null: sizes and offsets only
    std::vector<rgba_surface> chain;
    auto layout = [&](uint8_t* storage) {
        size_t at = 0;
        chain.clear();
        for (int l = 0; l < levels; l++) {
            const int lw = (w >> l) ? (w >> l) : 1, lh = (h >> l) ? (h >> l) : 1, ld = (depth >> l) ? (depth >> l) : 1;
            for (int z = 0; z < ld; z++) {
                chain.push_back(rgba_surface{storage ? storage + at : nullptr, lw, lh, lw * f.texel_bytes});
                at += (size_t)lw * lh * f.texel_bytes;
            }
        }
        return at;
    };
    const size_t texel_bytes = layout(nullptr);
    const int count = (int)chain.size();
    const int64_t bytes = itwChainBytes(chain.data(), count, f.dxgi);
    if (bytes <= 0) { std::fprintf(stderr, "bad size\n"); return 2; }
    std::vector<rgba_surface> bases((size_t)depth);
    for (int z = 0; z < depth; z++) bases[(size_t)z] = rgba_surface{texels + (size_t)z * w * h * f.texel_bytes, w, h, w * f.texel_bytes};
    std::vector<uint8_t> blocks((size_t)bytes);
    itwSetErrorMode(ITW_ON_ERROR_RETURN);
    const void* sp = takes_bc_settings(f.dxgi) ? (const void*)&g_bc1a : (const void*)&settings;
    if (!itwCompressImageMippedEx(bases.data(), depth, levels, 0, mip_flags | ITW_MIP_VOLUME, blocks.data(), f.dxgi, sp, nullptr, nullptr)) {
        std::fprintf(stderr, "%s\n", itwLastError() ? itwLastError() : "compression failed");
        return 1;
    }
    if (measure) {                                                  // the same chain once more, in host memory, and the stream against it
        std::vector<uint8_t> levels_texels(texel_bytes);
        layout(levels_texels.data());
        std::memcpy(levels_texels.data(), texels, (size_t)depth * w * h * f.texel_bytes);
        std::vector<itw_error_stats> st((size_t)count);
        if (itwGenerateMipChain(chain.data(), depth, levels, f.texel_bytes, mip_flags | ITW_MIP_VOLUME) != 0
            || itwMeasureChain(chain.data(), count, blocks.data(), f.dxgi, st.data(), sizeof(itw_error_stats)) != 0) {
            std::fprintf(stderr, "%s\n", itwLastError() ? itwLastError() : "measurement failed");
            return 1;
        }
        for (int i = 0; i < count; i++) {
            std::printf("image %d: %dx%d %s", i, st[(size_t)i].width, st[(size_t)i].height, f.name);
            if (f.texel_bytes == 4) std::printf(" psnr %.4f dB", itwStatsPsnr(&st[(size_t)i], f.own_channels));
            std::printf(" sse [%llu, %llu, %llu, %llu] max_abs [%u, %u, %u, %u]\n", (unsigned long long)st[(size_t)i].sse[0], (unsigned long long)st[(size_t)i].sse[1],
                        (unsigned long long)st[(size_t)i].sse[2], (unsigned long long)st[(size_t)i].sse[3], st[(size_t)i].max_abs[0], st[(size_t)i].max_abs[1],
                        st[(size_t)i].max_abs[2], st[(size_t)i].max_abs[3]);
        }
    }
    ItwDdsDesc desc = { (uint32_t)w, (uint32_t)h, (uint32_t)levels, (uint32_t)f.dxgi, ITW_DDS_VOLUME, (uint32_t)depth };
    std::vector<uint8_t> file(itwDdsFileBytes(&desc));
    std::vector<const uint8_t*> slices((size_t)count);              // level-major: the call's order
    size_t at = 0;
    for (size_t i = 0; i < slices.size(); i++) {
        slices[i] = blocks.data() + at;
        at += itwDdsImage(&desc, (uint32_t)i, nullptr, nullptr, nullptr);
    }
    if (at != blocks.size() || file.empty() || itwDdsWriteFile(&desc, slices.data(), slices.size(), file.data(), file.size()) != file.size()) {
        std::fprintf(stderr, "DDS assembly failed\n");
        return 1;
    }
    FILE* out = std::fopen(out_path, "wb");
    if (!out || std::fwrite(file.data(), 1, file.size(), out) != file.size()) { std::fprintf(stderr, "cannot write %s\n", out_path); return 1; }
    std::fclose(out);
    DestroyThreads();
    std::fprintf(stderr, "%s: %dx%dx%d, %d levels, %d slices -> %zu bytes (%s)\n", out_path, w, h, depth, levels, count, file.size(), f.name);
    return 0;
}

// --height-amplitude: a float as the bits of the nearest IEEE half (ties to even; overflow gives 0x7C00, which the caller refuses)
uint32_t half_bits_of(float v)
{
    uint32_t x;
    std::memcpy(&x, &v, sizeof x);
    if ((x >> 31) || x > 0x7f800000u) return 0;                 // negative or NaN: refused as 0 is
    if (x >= 0x477ff000u) return 0x7c00u;
    if (x < 0x33000001u) return 0;
    const bool tiny = x < 0x38800000u;
    const uint32_t m = tiny ? ((x & 0x7fffffu) | 0x800000u) : x - 0x38000000u, shift = tiny ? 126u - (x >> 23) : 13u;
    uint32_t r = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1u), halfway = 1u << (shift - 1u);
    if (rem > halfway || (rem == halfway && (r & 1u))) r++;
    return r;
}

// encode_dds --signed-normal: a signed normal source of `tb`-byte texels (or its six cross faces) to BC4_SNORM / BC5_SNORM, mipped or not
int encode_signed_normal(const Format& f, const rgba_surface& source, int tb, uint32_t ops, bool cube_cross, bool mips, int levels, const char* out_path)
{
    rgba_surface bases[6] = {source};
    int items = 1;
    if (cube_cross) {
        if (itwCubeCrossFaces(&source, tb, bases) != 0) { std::fprintf(stderr, "%d x %d is too small for a cube cross\n", source.width, source.height); return 2; }
        items = 6;
    }
    const int w = bases[0].width, h = bases[0].height, full = itwMipLevels(w, h);
    if (!mips) levels = 1;
    else if (levels < 0 || levels > full) { std::fprintf(stderr, "--mips %d: a full chain of %d x %d has %d levels\n", levels, w, h, full); return 2; }
    else if (levels == 0) levels = full;
    ItwDdsDesc desc = { (uint32_t)w, (uint32_t)h, (uint32_t)levels, (uint32_t)f.dxgi, cube_cross ? 1u : 0u, 1 };
    std::vector<const uint8_t*> images((size_t)items * levels);      // face-major, then level: the calls' order
    size_t bytes = 0;
    for (size_t i = 0; i < images.size(); i++) bytes += itwDdsImage(&desc, (uint32_t)i, nullptr, nullptr, nullptr);
    std::vector<uint8_t> blocks(bytes);
    itwSetErrorMode(ITW_ON_ERROR_RETURN);
    bool ok;
    if (mips) ok = itwCompressSignedNormalMapMipped(bases, items, levels, tb, ops, blocks.data(), f.dxgi, nullptr, nullptr);
    else if (f.dxgi == ITW_DXGI_FORMAT_BC5_SNORM && !cube_cross) {
        itwCompressNormalMapBC5S(&source, tb, blocks.data(), ops);   // the stages run inside the encoder
        ok = itwLastError() == nullptr;
    } else ok = itwCompressSignedNormalMapChain(bases, items, tb, blocks.data(), f.dxgi, ops, nullptr, nullptr);
    if (!ok) { std::fprintf(stderr, "%s\n", itwLastError() ? itwLastError() : "compression failed"); return 1; }
    size_t at = 0;
    for (size_t i = 0; i < images.size(); i++) { images[i] = blocks.data() + at; at += itwDdsImage(&desc, (uint32_t)i, nullptr, nullptr, nullptr); }
    std::vector<uint8_t> file(itwDdsFileBytes(&desc));
    if (file.empty() || itwDdsWriteFile(&desc, images.data(), images.size(), file.data(), file.size()) != file.size()) { std::fprintf(stderr, "DDS assembly failed\n"); return 1; }
    FILE* out = std::fopen(out_path, "wb");
    if (!out || std::fwrite(file.data(), 1, file.size(), out) != file.size()) { std::fprintf(stderr, "cannot write %s\n", out_path); return 1; }
    std::fclose(out);
    DestroyThreads();
    std::fprintf(stderr, "%s: %dx%d%s, %d levels -> %zu bytes (%s, signed source of %d-byte texels, ops %u)\n", out_path, w, h, cube_cross ? " x 6 faces" : "", levels,
                 file.size(), f.name, tb, ops);
    return 0;
}

// encode_dds --decode: the whole file through one call
int decode_file(const char* in_path, const char* out_path)
{
    FILE* in = std::fopen(in_path, "rb");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", in_path); return 1; }
    std::vector<uint8_t> file;
    uint8_t buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, in)) > 0;) file.insert(file.end(), buf, buf + n);
    std::fclose(in);
    static const uint8_t ktx_id[12] = {0xAB, 0x4B, 0x54, 0x58, 0x20, 0x31, 0x31, 0xBB, 0x0D, 0x0A, 0x1A, 0x0A};
    const bool ktx = file.size() >= 12 && std::memcmp(file.data(), ktx_id, 12) == 0;
    ItwDdsDesc desc = {};
    ItwKtxDesc kdesc = {};
    bool volume = false;                                           // a volume DDS: slices level-major, the depth in array_size
    std::vector<uint32_t> level_of, slice_of;
    size_t first = 0;
    std::vector<uint8_t> packed;                                   // KTX: the images behind one another (a size word sits in front of each level)
    if (ktx) {
        if (!itwKtxReadHeader(file.data(), file.size(), &kdesc)) { std::fprintf(stderr, "%s: not an ETC1 KTX 1.1 file this library reads\n", in_path); return 1; }
        desc.dxgi_format = kdesc.gl_internal_format;
    } else {
        first = itwDdsReadHeader(file.data(), file.size(), &desc);
        volume = first && desc.is_cubemap == ITW_DDS_VOLUME;
        if (!first) { std::fprintf(stderr, "%s: not a BCn DDS file this library reads\n", in_path); return 1; }
    }
    // a file labelled BC6H_SF16 is read as a GPU reads it: the signed reading has a code of its own (itw_dispatch.h), 96 is the header's word
    const int stream_format = desc.dxgi_format == ITW_DXGI_FORMAT_BC6H_SF16 ? (int)ITW_FORMAT_BC6H_SIGNED : (int)desc.dxgi_format;
    const int texel_bytes = desc.dxgi_format == ITW_DXGI_FORMAT_BC6H_UF16 || desc.dxgi_format == ITW_DXGI_FORMAT_BC6H_SF16 ? 8 : 4;
    std::vector<rgba_surface> outs;
    size_t texels_bytes = 0, end = first;
    for (uint32_t i = 0;; i++) {                                   // the payload, image by image
        uint32_t w = 0, h = 0; size_t off = 0;
        const size_t n = ktx ? itwKtxImage(&kdesc, i, &w, &h, &off) : itwDdsImage(&desc, i, &w, &h, &off);
        if (!n) break;
        if (volume) {                                              // index i is slice i - (slices of the levels before) of its level
            uint32_t lv = 0, before = 0;
            for (uint32_t ld = desc.array_size; i - before >= ld; lv++, ld = ld > 1 ? ld / 2 : 1) before += ld;
            level_of.push_back(lv); slice_of.push_back(i - before);
        }
        outs.push_back(rgba_surface{nullptr, (int32_t)w, (int32_t)h, (int32_t)w * texel_bytes});
        texels_bytes += (size_t)w * h * texel_bytes;
        end = off + n;
        if (ktx) packed.insert(packed.end(), file.begin() + (ptrdiff_t)off, file.begin() + (ptrdiff_t)(off + n));      // (itwKtxReadHeader has checked the file's length)
    }
    if (outs.empty() || file.size() < end) { std::fprintf(stderr, "%s: truncated: %zu bytes, the header describes %zu\n", in_path, file.size(), end); return 1; }
    std::vector<uint8_t> texels(texels_bytes);
    size_t at = 0;
    for (rgba_surface& s : outs) { s.ptr = texels.data() + at; at += (size_t)s.stride * s.height; }
    std::vector<uint32_t> min_alpha(outs.size());
    itwSetErrorMode(ITW_ON_ERROR_RETURN);
    if (itwDecodeChain(stream_format, ktx ? packed.data() : file.data() + first, outs.data(), (int)outs.size(), nullptr, min_alpha.data()) != 0) {
        std::fprintf(stderr, "%s\n", itwLastError() ? itwLastError() : "itwDecodeChain refused the file");
        return 1;
    }
    for (size_t i = 0; i < outs.size(); i++) {
        std::printf("image %zu: %d %d min_alpha %u", i, outs[i].width, outs[i].height, min_alpha[i]);
        if (volume) std::printf(" level %u slice %u", level_of[i], slice_of[i]);
        std::printf("\n");
    }
    FILE* out = std::fopen(out_path, "wb");
    if (!out || std::fwrite(texels.data(), 1, texels.size(), out) != texels.size()) { std::fprintf(stderr, "cannot write %s\n", out_path); return 1; }
    std::fclose(out);
    std::fprintf(stderr, "%s: %zu images -> %zu bytes\n", out_path, outs.size(), texels.size());
    return 0;
}

// encode_dds --preview: one image of the file, the part of it a viewport shows; args: index, out.ppm, w, h, x, y, zoom [channels exposure matte]
int preview_file(const char* in_path, int argc, char** args)
{
    FILE* in = std::fopen(in_path, "rb");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", in_path); return 1; }
    std::vector<uint8_t> file;
    uint8_t buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, in)) > 0;) file.insert(file.end(), buf, buf + n);
    std::fclose(in);
    static const uint8_t ktx_id[12] = {0xAB, 0x4B, 0x54, 0x58, 0x20, 0x31, 0x31, 0xBB, 0x0D, 0x0A, 0x1A, 0x0A};
    const bool ktx = file.size() >= 12 && std::memcmp(file.data(), ktx_id, 12) == 0;
    ItwDdsDesc desc = {};
    ItwKtxDesc kdesc = {};
    if (ktx ? !itwKtxReadHeader(file.data(), file.size(), &kdesc) : !itwDdsReadHeader(file.data(), file.size(), &desc)) {
        std::fprintf(stderr, "%s: not a DDS / KTX file this library reads\n", in_path);
        return 1;
    }
    const int format = ktx ? (int)kdesc.gl_internal_format
                     : desc.dxgi_format == ITW_DXGI_FORMAT_BC6H_SF16 ? (int)ITW_FORMAT_BC6H_SIGNED : (int)desc.dxgi_format;      // (as --decode)
    uint32_t w = 0, h = 0; size_t off = 0;
    const uint32_t index = (uint32_t)std::strtoul(args[0], nullptr, 10);
    const size_t n = ktx ? itwKtxImage(&kdesc, index, &w, &h, &off) : itwDdsImage(&desc, index, &w, &h, &off);
    if (!n) { std::fprintf(stderr, "%s has no image %u\n", in_path, index); return 1; }
    if (file.size() < off + n) { std::fprintf(stderr, "%s: truncated: %zu bytes, image %u ends at %zu\n", in_path, file.size(), index, off + n); return 1; }
    itw_preview_view view = {};
    view.width = std::atoi(args[2]); view.height = std::atoi(args[3]);
    view.x_offset = std::atoi(args[4]); view.y_offset = std::atoi(args[5]);
    view.zoom = std::atof(args[6]);
    for (const char* c = argc > 7 ? args[7] : "rgb"; *c; c++)
        view.options |= *c == 'r' ? ITW_PREVIEW_CHANNEL_RED : *c == 'g' ? ITW_PREVIEW_CHANNEL_GREEN : *c == 'b' ? ITW_PREVIEW_CHANNEL_BLUE : *c == 'a' ? ITW_PREVIEW_CHANNEL_ALPHA : 0u;
    view.exposure = argc > 8 ? (float)std::atof(args[8]) : 1.0f;
    view.matte_color = argc > 9 ? (uint32_t)std::strtoul(args[9], nullptr, 0) : 0u;
    if (view.width < 1 || view.width > 16384 || view.height < 1 || view.height > 16384) { std::fprintf(stderr, "a viewport is 1 .. 16384 pixels each way\n"); return 2; }
    std::vector<uint8_t> rgb((size_t)view.width * view.height * 3);
    itwSetErrorMode(ITW_ON_ERROR_RETURN);
    if (itwPreviewBlocks(format, file.data() + off, (int)w, (int)h, &view, sizeof view, rgb.data(), (int64_t)view.width * 3) != 0) {
        std::fprintf(stderr, "%s\n", itwLastError() ? itwLastError() : "itwPreviewBlocks refused the call (a format that is not previewed, an offset or zoom out of range)");
        return 1;
    }
    FILE* out = std::fopen(args[1], "wb");
    if (!out || std::fprintf(out, "P6\n%d %d\n255\n", view.width, view.height) < 0 || std::fwrite(rgb.data(), 1, rgb.size(), out) != rgb.size()) {
        std::fprintf(stderr, "cannot write %s\n", args[1]);
        return 1;
    }
    std::fclose(out);
    std::fprintf(stderr, "%s: image %u (%ux%u) -> %dx%d viewport at (%d, %d), zoom %g\n", args[1], index, w, h, view.width, view.height, view.x_offset, view.y_offset, view.zoom);
    return 0;
}

} // namespace

// --fit pow2, texconv's rule for -pow2 with its default size cap restated: the longer axis becomes the largest of 16384, 8192, ... that
// is <= itself; the other axis the one of them whose ratio to it is nearest the source's aspect in fp32, the larger on a tie
static void fit_power_of_two(int w, int h, int* tw, int* th)
{
    const int cap = 16384;
    const float aspect = (float)w / (float)h;
    int longer = cap;
    while (longer > 1 && longer > (w > h ? w : h)) longer >>= 1;
    int other = cap;
    float best = INFINITY;
    for (int v = cap; v > 0; v >>= 1) {
        const float score = std::fabs((w > h ? (float)longer / (float)v : (float)v / (float)longer) - aspect);
        if (score < best) { best = score; other = v; }
    }
    *tw = w > h ? longer : other;
    *th = w > h ? other : longer;
}

int main(int argc, char** argv)
{
    if (argc == 4 && std::strcmp(argv[1], "--decode") == 0) return decode_file(argv[2], argv[3]);
    if (argc >= 10 && argc <= 13 && std::strcmp(argv[1], "--preview") == 0) return preview_file(argv[2], argc - 3, argv + 3);
    bool measure = false;
    const char* refine_profile = nullptr;
    unsigned long long max_block_sse = 0;
    int refine_to = 0;                                          // 1: --refine-share, 2: --refine-psnr
    double refine_value = 0.0;                                  // percent / dB
    bool normal_given = false, cube_cross = false;
    uint32_t normal_ops = 0;                                    // ITW_NORMAL_*
    bool mips = false, srgb_mips = false, alpha_given = false, filter_given = false;
    uint32_t filter_flags = 0;                                  // ITW_MIP_CUBIC / _TRIANGLE / _WRAP_U / _WRAP_V
    int resize_w = 0, resize_h = 0;                             // --resize WxH
    bool fit_pow2 = false, resize_filter_given = false;         // --fit pow2, --resize-filter
    uint32_t resize_filter = 0;                                 // ITW_MIP_POINT / _LINEAR / _CUBIC / _TRIANGLE
    itw_mip_alpha alpha = { (uint32_t)sizeof(itw_mip_alpha), 0, 0, 0 };
    int mip_levels = 0;                                         // 0: the full chain
    int signed_tb = 0;                                          // --signed-normal: texel bytes of the signed source (4, 8 or 16)
    int volume_depth = 0;                                       // --volume <depth>
    bool volume_given = false, volume_filter = false, volume_wrap = false;      // --mip-filter point|linear, --mip-wrap with w: the volume's alone
    uint32_t height_ops = 0, height_amplitude = 0x3C00;         // --height: ITW_NORMAL_FROM_HEIGHT and its fields; the amplitude as half bits (1.0)
    for (int i = 1; i < argc; i++)
        if (std::strcmp(argv[i], "--measure") == 0) {
            measure = true;
            for (int k = i; k + 1 < argc; k++) argv[k] = argv[k + 1];
            argc--; i--;
        } else if (std::strcmp(argv[i], "--refine") == 0 && i + 2 < argc) {
            refine_profile = argv[i + 1];
            max_block_sse = std::strtoull(argv[i + 2], nullptr, 10);
            for (int k = i; k + 3 < argc; k++) argv[k] = argv[k + 3];
            argc -= 3; i--;
        } else if ((std::strcmp(argv[i], "--refine-share") == 0 || std::strcmp(argv[i], "--refine-psnr") == 0) && i + 2 < argc) {
            refine_to = std::strcmp(argv[i], "--refine-share") == 0 ? 1 : 2;
            refine_profile = argv[i + 1];
            refine_value = std::atof(argv[i + 2]);
            for (int k = i; k + 3 < argc; k++) argv[k] = argv[k + 3];
            argc -= 3; i--;
        } else if (std::strcmp(argv[i], "--normal") == 0 && i + 1 < argc) {
            normal_given = true;
            for (const char* p = argv[i + 1]; *p;) {
                const size_t n = std::strcspn(p, ",");
                if (n == 5 && std::strncmp(p, "flipx", 5) == 0) normal_ops |= ITW_NORMAL_FLIP_X;
                else if (n == 5 && std::strncmp(p, "flipy", 5) == 0) normal_ops |= ITW_NORMAL_FLIP_Y;
                else if (n == 9 && std::strncmp(p, "normalize", 9) == 0) normal_ops |= ITW_NORMAL_NORMALIZE;
                else { std::fprintf(stderr, "--normal takes a list of flipx, flipy, normalize\n"); return 2; }
                p += n + (p[n] == ',' ? 1 : 0);
            }
            for (int k = i; k + 2 < argc; k++) argv[k] = argv[k + 2];
            argc -= 2; i--;
        } else if (std::strcmp(argv[i], "--signed-normal") == 0 && i + 1 < argc) {
            for (const char* p = argv[i + 1]; *p;) {
                const size_t n = std::strcspn(p, ",");
                if (p == argv[i + 1] && n == 4 && std::strncmp(p, "int8", 4) == 0) signed_tb = 4;
                else if (p == argv[i + 1] && n == 4 && std::strncmp(p, "half", 4) == 0) signed_tb = 8;
                else if (p == argv[i + 1] && n == 5 && std::strncmp(p, "float", 5) == 0) signed_tb = 16;
                else if (signed_tb && n == 5 && std::strncmp(p, "flipx", 5) == 0) normal_ops |= ITW_NORMAL_FLIP_X;
                else if (signed_tb && n == 5 && std::strncmp(p, "flipy", 5) == 0) normal_ops |= ITW_NORMAL_FLIP_Y;
                else if (signed_tb && n == 9 && std::strncmp(p, "normalize", 9) == 0) normal_ops |= ITW_NORMAL_NORMALIZE;
                else { std::fprintf(stderr, "--signed-normal takes int8, half or float, then a list of flipx, flipy, normalize\n"); return 2; }
                p += n + (p[n] == ',' ? 1 : 0);
            }
            for (int k = i; k + 2 < argc; k++) argv[k] = argv[k + 2];
            argc -= 2; i--;
        } else if (std::strcmp(argv[i], "--height") == 0 && i + 1 < argc) {
            height_ops |= ITW_NORMAL_FROM_HEIGHT;
            for (const char* p = argv[i + 1]; *p;) {
                const size_t n = std::strcspn(p, ",");
                const bool first = p == argv[i + 1];
                if (first && n == 1 && std::strchr("rgba", *p)) height_ops |= ITW_HEIGHT_CHANNEL(1 + (std::strchr("rgba", *p) - "rgba"));
                else if (first && n == 3 && std::strncmp(p, "lum", 3) == 0) height_ops |= ITW_HEIGHT_CHANNEL(5);
                else if (!first && n == 7 && std::strncmp(p, "mirroru", 7) == 0) height_ops |= ITW_HEIGHT_MIRROR_U;
                else if (!first && n == 7 && std::strncmp(p, "mirrorv", 7) == 0) height_ops |= ITW_HEIGHT_MIRROR_V;
                else if (!first && n == 6 && std::strncmp(p, "invert", 6) == 0) height_ops |= ITW_HEIGHT_INVERT_SIGN;
                else if (!first && n == 9 && std::strncmp(p, "occlusion", 9) == 0) height_ops |= ITW_HEIGHT_OCCLUSION;
                else { std::fprintf(stderr, "--height takes r, g, b, a or lum, then a list of mirroru, mirrorv, invert, occlusion\n"); return 2; }
                p += n + (p[n] == ',' ? 1 : 0);
            }
            for (int k = i; k + 2 < argc; k++) argv[k] = argv[k + 2];
            argc -= 2; i--;
        } else if (std::strcmp(argv[i], "--height-amplitude") == 0 && i + 1 < argc) {
            height_amplitude = half_bits_of((float)std::atof(argv[i + 1]));
            if (height_amplitude == 0 || height_amplitude >= 0x7C00) { std::fprintf(stderr, "--height-amplitude: finite and above 0 once rounded to a half\n"); return 2; }
            for (int k = i; k + 2 < argc; k++) argv[k] = argv[k + 2];
            argc -= 2; i--;
        } else if (std::strcmp(argv[i], "--cube-cross") == 0) {
            cube_cross = true;
            for (int k = i; k + 1 < argc; k++) argv[k] = argv[k + 1];
            argc--; i--;
        } else if (std::strcmp(argv[i], "--mips") == 0) {
            mips = true;
            const bool count = i + 1 < argc && argv[i + 1][0] != '\0' && std::strspn(argv[i + 1], "0123456789") == std::strlen(argv[i + 1]);
            if (count) mip_levels = std::atoi(argv[i + 1]);
            const int used = count ? 2 : 1;
            for (int k = i; k + used < argc; k++) argv[k] = argv[k + used];
            argc -= used; i--;
        } else if (std::strcmp(argv[i], "--srgb-mips") == 0) {
            srgb_mips = true;
            for (int k = i; k + 1 < argc; k++) argv[k] = argv[k + 1];
            argc--; i--;
        } else if (std::strcmp(argv[i], "--mip-filter") == 0 && i + 1 < argc) {
            filter_given = true;
            if (std::strcmp(argv[i + 1], "cubic") == 0) filter_flags |= ITW_MIP_CUBIC;
            else if (std::strcmp(argv[i + 1], "triangle") == 0) filter_flags |= ITW_MIP_TRIANGLE;
            else if (std::strcmp(argv[i + 1], "point") == 0) { filter_flags |= ITW_MIP_POINT; volume_filter = true; }
            else if (std::strcmp(argv[i + 1], "linear") == 0) { filter_flags |= ITW_MIP_LINEAR; volume_filter = true; }
            else { std::fprintf(stderr, "--mip-filter takes cubic or triangle\n"); return 2; }
            for (int k = i; k + 2 < argc; k++) argv[k] = argv[k + 2];
            argc -= 2; i--;
        } else if (std::strcmp(argv[i], "--mip-wrap") == 0 && i + 1 < argc) {
            filter_given = true;
            if (std::strcmp(argv[i + 1], "u") == 0) filter_flags |= ITW_MIP_WRAP_U;
            else if (std::strcmp(argv[i + 1], "v") == 0) filter_flags |= ITW_MIP_WRAP_V;
            else if (std::strcmp(argv[i + 1], "uv") == 0) filter_flags |= ITW_MIP_WRAP_U | ITW_MIP_WRAP_V;
            else if (std::strcmp(argv[i + 1], "w") == 0 || std::strcmp(argv[i + 1], "uw") == 0 || std::strcmp(argv[i + 1], "vw") == 0 || std::strcmp(argv[i + 1], "uvw") == 0) {
                volume_wrap = true;
                filter_flags |= ITW_MIP_WRAP_W | (std::strchr(argv[i + 1], 'u') ? (uint32_t)ITW_MIP_WRAP_U : 0u) | (std::strchr(argv[i + 1], 'v') ? (uint32_t)ITW_MIP_WRAP_V : 0u);
            }
            else { std::fprintf(stderr, "--mip-wrap takes u, v or uv\n"); return 2; }
            for (int k = i; k + 2 < argc; k++) argv[k] = argv[k + 2];
            argc -= 2; i--;
        } else if (std::strcmp(argv[i], "--volume") == 0 && i + 1 < argc) {
            volume_given = true;
            volume_depth = std::atoi(argv[i + 1]);
            if (volume_depth < 1) { std::fprintf(stderr, "--volume takes a depth of at least 1\n"); return 2; }
            for (int k = i; k + 2 < argc; k++) argv[k] = argv[k + 2];
            argc -= 2; i--;
        } else if (std::strcmp(argv[i], "--resize") == 0 && i + 1 < argc) {
            if (std::sscanf(argv[i + 1], "%dx%d", &resize_w, &resize_h) != 2 || resize_w < 1 || resize_h < 1) { std::fprintf(stderr, "--resize takes WxH\n"); return 2; }
            for (int k = i; k + 2 < argc; k++) argv[k] = argv[k + 2];
            argc -= 2; i--;
        } else if (std::strcmp(argv[i], "--fit") == 0 && i + 1 < argc) {
            if (std::strcmp(argv[i + 1], "pow2") != 0) { std::fprintf(stderr, "--fit takes pow2\n"); return 2; }
            fit_pow2 = true;
            for (int k = i; k + 2 < argc; k++) argv[k] = argv[k + 2];
            argc -= 2; i--;
        } else if (std::strcmp(argv[i], "--resize-filter") == 0 && i + 1 < argc) {
            resize_filter_given = true;
            if (std::strcmp(argv[i + 1], "point") == 0) resize_filter = ITW_MIP_POINT;
            else if (std::strcmp(argv[i + 1], "linear") == 0) resize_filter = ITW_MIP_LINEAR;
            else if (std::strcmp(argv[i + 1], "cubic") == 0) resize_filter = ITW_MIP_CUBIC;
            else if (std::strcmp(argv[i + 1], "triangle") == 0) resize_filter = ITW_MIP_TRIANGLE;
            else { std::fprintf(stderr, "--resize-filter takes point, linear, cubic or triangle\n"); return 2; }
            for (int k = i; k + 2 < argc; k++) argv[k] = argv[k + 2];
            argc -= 2; i--;
        } else if (std::strcmp(argv[i], "--bc-dither") == 0 && i + 1 < argc) {
            if (std::strcmp(argv[i + 1], "rgb") == 0) g_bc1a.flags |= ITW_BC_DITHER_RGB;
            else if (std::strcmp(argv[i + 1], "a") == 0) g_bc1a.flags |= ITW_BC_DITHER_A;
            else if (std::strcmp(argv[i + 1], "rgb,a") == 0 || std::strcmp(argv[i + 1], "a,rgb") == 0) g_bc1a.flags |= ITW_BC_DITHER_RGB | ITW_BC_DITHER_A;
            else { std::fprintf(stderr, "--bc-dither takes rgb, a or rgb,a\n"); return 2; }
            for (int k = i; k + 2 < argc; k++) argv[k] = argv[k + 2];
            argc -= 2; i--;
        } else if (std::strcmp(argv[i], "--bc-uniform") == 0) {
            g_bc1a.flags |= ITW_BC_UNIFORM;
            for (int k = i; k + 1 < argc; k++) argv[k] = argv[k + 1];
            argc--; i--;
        } else if (std::strcmp(argv[i], "--alpha-weight") == 0) {
            alpha_given = true; alpha.weight_colour = 1;
            for (int k = i; k + 1 < argc; k++) argv[k] = argv[k + 1];
            argc--; i--;
        } else if (std::strcmp(argv[i], "--alpha-coverage") == 0 && i + 1 < argc) {
            alpha_given = true; alpha.coverage_ref = (uint32_t)std::atoi(argv[i + 1]);      // (the call refuses what is not 0 .. 255)
            for (int k = i; k + 2 < argc; k++) argv[k] = argv[k + 2];
            argc -= 2; i--;
        }
    if (argc < 6) {
        std::fprintf(stderr, "usage: %s [--measure] [--refine <profile> <max_block_sse> | --refine-share <profile> <percent> | --refine-psnr <profile> <dB>]\n"
                             "          [--normal flipx,flipy,normalize | --signed-normal int8|half|float[,flipx,flipy,normalize]] [--cube-cross] [--mips [levels] [--srgb-mips]]\n"
                             "          [--height r|g|b|a|lum[,mirroru,mirrorv,invert,occlusion] [--height-amplitude <A>]]\n"
                             "          [--alpha-weight] [--alpha-coverage <ref>] [--mip-filter cubic|triangle] [--mip-wrap u|v|uv] [--bc-dither rgb|a|rgb,a] [--bc-uniform]\n"
                             "          [--resize WxH | --fit pow2] [--resize-filter point|linear|cubic|triangle]\n"
                             "          [--volume <depth> [--mips [levels]] [--mip-filter point|linear|cubic|triangle] [--mip-wrap u|v|w|uv|uw|vw|uvw] [--srgb-mips] [--measure]]\n"
                             "          <format> <width> <height> <in.raw> <out.dds> [slice_pixels]\n"
                             "       %s --decode <in.dds | in.ktx> <out.raw>\n"
                             "       %s --preview <in.dds | in.ktx> <image index> <out.ppm> <w> <h> <x> <y> <zoom> [channels] [exposure] [matte]\n", argv[0], argv[0], argv[0]);
        return 2;
    }
    const Format* f = nullptr;
    const bool bc1a = std::strcmp(argv[1], "bc1a") == 0 || std::strncmp(argv[1], "bc1a:", 5) == 0 || std::strcmp(argv[1], "bc2") == 0 || std::strcmp(argv[1], "bc3_dxtex") == 0;      // (takes g_bc1a)
    if (bc1a && argv[1][3] == 'a' && argv[1][4] == ':') { g_bc1a.alpha_ref = (float)std::atof(argv[1] + 5); argv[1][4] = '\0'; }
    for (const Format& k : kFormats) if (std::strcmp(k.name, argv[1]) == 0) f = &k;
    int width = std::atoi(argv[2]), height = std::atoi(argv[3]);
    if (!f || width < 1 || height < 1) { std::fprintf(stderr, "unknown format or bad size\n"); return 2; }
    const long long slice_pixels = argc > 6 ? std::atoll(argv[6]) : 0;

    if (!volume_given && volume_filter) { std::fprintf(stderr, "--mip-filter takes cubic or triangle\n"); return 2; }      // (point and linear are --volume's)
    if (!volume_given && volume_wrap) { std::fprintf(stderr, "--mip-wrap takes u, v or uv\n"); return 2; }
    if (g_bc1a.flags && !bc1a) { std::fprintf(stderr, "--bc-dither and --bc-uniform are bc1a's flags (and bc2's), and bc3_dxtex's\n"); return 2; }
    if (bc1a && (normal_given || refine_profile)) { std::fprintf(stderr, "%s holds colour and has one encoder: not with --normal or --refine*\n", argv[1]); return 2; }
    if (signed_tb && (normal_given || refine_profile || measure || (f->dxgi != ITW_DXGI_FORMAT_BC4_SNORM && f->dxgi != ITW_DXGI_FORMAT_BC5_SNORM))) {
        std::fprintf(stderr, "--signed-normal is for bc4_snorm / bc5_snorm and does not go with --normal, --refine* or --measure\n");
        return 2;
    }
    if (srgb_mips && (!mips || signed_tb)) { std::fprintf(stderr, "--srgb-mips goes with --mips, and not with --signed-normal\n"); return 2; }
    if (alpha_given && (!mips || signed_tb || normal_given)) {
        std::fprintf(stderr, "--alpha-weight and --alpha-coverage go with --mips, and not with --normal or --signed-normal\n");
        return 2;
    }
    if (filter_given && (!mips || signed_tb)) { std::fprintf(stderr, "--mip-filter and --mip-wrap go with --mips, and not with --signed-normal\n"); return 2; }
    if (volume_given) {
        if (normal_given || signed_tb || height_ops || cube_cross || refine_profile || alpha_given || resize_w || fit_pow2 || resize_filter_given || argc > 6
            || f->dxgi == ITW_FORMAT_ETC1_RGB8) {
            std::fprintf(stderr, "--volume does not go with --normal, --signed-normal, --height, --cube-cross, --refine*, --alpha-weight, --alpha-coverage, --resize, --fit, "
                                 "etc1_slow or a slice size: a volume has mips, a filter, wrap addressing and sRGB colour\n");
            return 2;
        }
        if ((srgb_mips || filter_given) && !mips) { std::fprintf(stderr, "--srgb-mips, --mip-filter and --mip-wrap go with --mips\n"); return 2; }
        std::vector<uint8_t> slices((size_t)width * height * volume_depth * f->texel_bytes);
        FILE* vin = std::fopen(argv[4], "rb");
        if (!vin || std::fread(slices.data(), 1, slices.size(), vin) != slices.size()) { std::fprintf(stderr, "cannot read %s\n", argv[4]); return 1; }
        std::fclose(vin);
        return encode_volume(*f, slices.data(), width, height, volume_depth, mips ? mip_levels : 1, (srgb_mips ? (uint32_t)ITW_MIP_SRGB : 0u) | filter_flags, measure, argv[5]);
    }
    const int texel_bytes = signed_tb ? signed_tb : f->texel_bytes;
    std::vector<uint8_t> texels((size_t)width * height * texel_bytes);
    FILE* in = std::fopen(argv[4], "rb");
    if (!in || std::fread(texels.data(), 1, texels.size(), in) != texels.size()) { std::fprintf(stderr, "cannot read %s\n", argv[4]); return 1; }
    std::fclose(in);

    rgba_surface source = { texels.data(), width, height, width * texel_bytes };
    std::vector<uint8_t> resized;                               // --resize / --fit: the image everything after this sees
    if (resize_w || fit_pow2 || resize_filter_given) {
        if ((resize_w != 0) == fit_pow2) { std::fprintf(stderr, "--resize-filter goes with --resize WxH or --fit pow2, one of the two\n"); return 2; }
        if (signed_tb || cube_cross) { std::fprintf(stderr, "--resize and --fit do not go with --signed-normal or --cube-cross\n"); return 2; }
        if (fit_pow2) fit_power_of_two(width, height, &resize_w, &resize_h);
        resized.resize((size_t)resize_w * resize_h * texel_bytes);
        const rgba_surface pair[2] = { source, { resized.data(), resize_w, resize_h, resize_w * texel_bytes } };
        const uint32_t flags = ITW_MIP_RESIZE | resize_filter | (srgb_mips ? (uint32_t)ITW_MIP_SRGB : 0u) | (filter_flags & (uint32_t)(ITW_MIP_WRAP_U | ITW_MIP_WRAP_V));
        itwSetErrorMode(ITW_ON_ERROR_RETURN);
        if (itwGenerateMipChain(pair, 1, 2, texel_bytes, flags) != 0) { std::fprintf(stderr, "%s\n", itwLastError() ? itwLastError() : "the resize refused the call"); return 1; }
        itwSetErrorMode(ITW_ON_ERROR_ABORT);
        source = pair[1]; width = resize_w; height = resize_h;
    }
    std::vector<uint8_t> quantised;                             // --height with --signed-normal and no --mips: the RGBA8_SNORM map
    if (height_ops) {
        // the input is a height map.  The one-call saves take the bit themselves; the other routes see one texel or one block at a time, so
        // the stage runs first, over the image or each face of its cross: in place (itwPrepareNormalMapChain) or into an int8 copy
        // (itwQuantizeNormalMapChain), with the flips and the normalise, which then are done
        if (!normal_given && !signed_tb) { std::fprintf(stderr, "--height goes with --normal or --signed-normal\n"); return 2; }
        normal_ops |= height_ops | ITW_HEIGHT_AMPLITUDE(height_amplitude);
        if (!mips) {
            rgba_surface faces[6] = {source}, targets[6];
            const int items = cube_cross ? 6 : 1;
            if (cube_cross && itwCubeCrossFaces(&source, texel_bytes, faces) != 0) { std::fprintf(stderr, "%d x %d is too small for a cube cross\n", width, height); return 2; }
            itwSetErrorMode(ITW_ON_ERROR_RETURN);
            int rc;
            if (signed_tb) {
                quantised.resize((size_t)width * height * 4);
                const rgba_surface map = { quantised.data(), width, height, width * 4 };
                targets[0] = map;
                if (cube_cross) itwCubeCrossFaces(&map, 4, targets);
                rc = itwQuantizeNormalMapChain(faces, signed_tb, targets, items, normal_ops);
                source = map; signed_tb = 4;
            } else rc = itwPrepareNormalMapChain(faces, items, texel_bytes, normal_ops);
            if (rc != 0) { std::fprintf(stderr, "%s\n", itwLastError() ? itwLastError() : "the height stage refused the call"); return 1; }
            normal_ops = 0;
        }
    }
    if (signed_tb) return encode_signed_normal(*f, source, signed_tb, normal_ops, cube_cross, mips, mip_levels, argv[5]);
    if (mips) {
        if (refine_profile || measure || (cube_cross && f->dxgi == ITW_FORMAT_ETC1_RGB8)) {
            std::fprintf(stderr, "--mips does not go with --refine* or --measure; --cube-cross not with etc1_slow\n");
            return 2;
        }
        return encode_mipped(*f, source, normal_ops, (srgb_mips ? (uint32_t)ITW_MIP_SRGB : 0u) | filter_flags, alpha_given ? &alpha : nullptr, cube_cross, mip_levels, argv[5]);
    }
    if (normal_given || cube_cross) {
        // the normal-map and cube-cross stages of the save path (IntelPlugin.cpp:2075-2106, 2149-2152): one call over the image or its six faces
        if (refine_profile || (cube_cross && (measure || f->dxgi == ITW_FORMAT_ETC1_RGB8))) {
            std::fprintf(stderr, "--normal / --cube-cross do not go with --refine*; --cube-cross not with --measure or etc1_slow\n");
            return 2;
        }
        return encode_normal_or_cross(*f, source, normal_ops, cube_cross, measure, argv[5]);
    }
    rgba_surface padded = source;
    if (f->pad && ((width | height) & 3)) padded = itwPadToMultipleOf4(&source, f->texel_bytes);     // IntelPlugin.cpp:893-928

    const bool etc1 = f->dxgi == ITW_FORMAT_ETC1_RGB8;
    if (etc1 && refine_profile) { std::fprintf(stderr, "--refine* is for bc7_* and bc6h_*: ETC1 has one preset, there is nothing to refine with\n"); return 2; }
    ItwDdsDesc desc = { (uint32_t)padded.width, (uint32_t)padded.height, 1, (uint32_t)f->dxgi, 0, 1 };
    ItwKtxDesc kdesc = { (uint32_t)padded.width, (uint32_t)padded.height, 1, ITW_FORMAT_ETC1_RGB8, 0, 0 };
    std::vector<uint8_t> blocks(etc1 ? (size_t)(padded.width / 4) * (padded.height / 4) * 8 : itwDdsLevelBytes(desc.dxgi_format, desc.width, desc.height));
    const int64_t pitch = (int64_t)((padded.width + 3) / 4) * GetBytesPerBlock(f->dxgi);
    bool ok;
    if (refine_profile) {
        const bool bc7 = std::strncmp(f->name, "bc7_", 4) == 0, bc6h = std::strncmp(f->name, "bc6h_", 5) == 0;
        union { bc7_enc_settings s7; bc6h_enc_settings s6; } first, second;
        if ((!bc7 && !bc6h) || !profile_by_name(bc6h, f->name + (bc7 ? 4 : 5), &first) || !profile_by_name(bc6h, refine_profile, &second)) {
            std::fprintf(stderr, "--refine needs a bc7_* or bc6h_* format and a preset of the same format\n");
            return 2;
        }
        itw_refine_stats rs;
        itwSetErrorMode(ITW_ON_ERROR_RETURN);
        if (refine_to) {
            const unsigned long long nb = (unsigned long long)(padded.width / 4) * (unsigned long long)(padded.height / 4);
            itw_refine_policy pol = { UINT64_MAX, UINT64_MAX };
            if (refine_to == 1) {
                if (!(refine_value >= 0.0 && refine_value <= 100.0)) { std::fprintf(stderr, "--refine-share: a percentage, 0..100\n"); return 2; }
                pol.max_listed = (uint64_t)(refine_value / 100.0 * (double)nb);
            } else {
                pol.target_total_sse = itwPsnrToTotalSse(f->dxgi, width, height, f->own_channels, refine_value);
                if (pol.target_total_sse == UINT64_MAX) { std::fprintf(stderr, "--refine-psnr needs a bc7_* format and a finite dB\n"); return 2; }
            }
            itw_refine_target_stats ts;
            ok = itwCompressImageRefinedTo(&padded, blocks.data(), f->dxgi, &first, &second, f->own_channels, &pol, sizeof pol, &ts, sizeof ts, nullptr, nullptr);
            rs = ts.total;
            if (!ok) std::fprintf(stderr, "%s\n", itwLastError() ? itwLastError() : "itwCompressImageRefinedTo failed");
            else {
                std::printf("refined: %s -> %s %s %g rounds %u met %u budgets [%llu, %llu, %llu, %llu, %llu] blocks %llu listed %llu replaced %llu sse %llu -> %llu "
                            "worst %llu -> %llu\n", f->name, refine_profile, refine_to == 1 ? "share" : "psnr", refine_value, ts.rounds, ts.target_met,
                            (unsigned long long)ts.budget[0], (unsigned long long)ts.budget[1], (unsigned long long)ts.budget[2], (unsigned long long)ts.budget[3],
                            (unsigned long long)ts.budget[4], (unsigned long long)rs.blocks, (unsigned long long)rs.listed, (unsigned long long)rs.replaced,
                            (unsigned long long)rs.sse_first, (unsigned long long)rs.sse_final, (unsigned long long)rs.worst_first, (unsigned long long)rs.worst_final);
            }
        } else {
            ok = itwCompressImageRefined(&padded, blocks.data(), f->dxgi, &first, &second, f->own_channels, max_block_sse, &rs, sizeof rs, nullptr, nullptr);
            if (!ok) std::fprintf(stderr, "%s\n", itwLastError() ? itwLastError() : "itwCompressImageRefined failed");
            else std::printf("refined: %s -> %s budget %llu blocks %llu listed %llu replaced %llu sse %llu -> %llu worst %llu -> %llu\n", f->name, refine_profile,
                             max_block_sse, (unsigned long long)rs.blocks, (unsigned long long)rs.listed, (unsigned long long)rs.replaced,
                             (unsigned long long)rs.sse_first, (unsigned long long)rs.sse_final, (unsigned long long)rs.worst_first, (unsigned long long)rs.worst_final);
        }
    } else if (bc1a) {
        ok = itwCompressImageSlicedEx(&padded, blocks.data(), pitch, f->dxgi, &g_bc1a, slice_pixels, slice_pixels ? on_progress : nullptr, nullptr);
    } else if (etc1) {
        etc_enc_settings se;
        itwGetProfile_etc_slow(&se);
        ok = itwCompressImageSlicedEx(&padded, blocks.data(), pitch, f->dxgi, &se, slice_pixels, slice_pixels ? on_progress : nullptr, nullptr);
    } else {
        ok = itwCompressImageSliced(&padded, blocks.data(), pitch, f->fn, f->dxgi, /*multithreaded*/ true,
                                    slice_pixels, slice_pixels ? on_progress : nullptr, nullptr);
    }
    if (padded.ptr != source.ptr) itwFreeSurface(&padded);
    if (!ok) { std::fprintf(stderr, "\ncompression aborted\n"); return 1; }
    if (measure) {
        // the stream against the texels as they were read: the pad's texels are not part of the image and are not compared
        itw_error_stats st;
        if (itwMeasureBlocks(f->dxgi, blocks.data(), &source, &st, sizeof st, nullptr) != 0) { std::fprintf(stderr, "\nmeasurement failed\n"); return 1; }
        std::printf("image 0: %dx%d %s", st.width, st.height, f->name);
        if (f->texel_bytes == 4) std::printf(" psnr %.4f dB", itwStatsPsnr(&st, f->own_channels));      // (no PSNR of half-float codes)
        std::printf(" sse [%llu, %llu, %llu, %llu] max_abs [%u, %u, %u, %u]\n", (unsigned long long)st.sse[0], (unsigned long long)st.sse[1],
                    (unsigned long long)st.sse[2], (unsigned long long)st.sse[3], st.max_abs[0], st.max_abs[1], st.max_abs[2], st.max_abs[3]);
    }

    std::vector<uint8_t> file(etc1 ? itwKtxFileBytes(&kdesc) : itwDdsFileBytes(&desc));
    const uint8_t* levels[1] = { blocks.data() };
    if ((etc1 ? itwKtxWriteFile(&kdesc, levels, 1, file.data(), file.size()) : itwDdsWriteFile(&desc, levels, 1, file.data(), file.size())) != file.size() || file.empty()) {
        std::fprintf(stderr, "%s assembly failed\n", etc1 ? "KTX" : "DDS");
        return 1;
    }
    FILE* out = std::fopen(argv[5], "wb");
    if (!out || std::fwrite(file.data(), 1, file.size(), out) != file.size()) { std::fprintf(stderr, "cannot write %s\n", argv[5]); return 1; }
    std::fclose(out);
    DestroyThreads();
    std::fprintf(stderr, "%s%s: %dx%d -> %zu bytes (%s)\n", slice_pixels ? "\n" : "", argv[5], desc.width, desc.height, file.size(), f->name);
    return 0;
}
