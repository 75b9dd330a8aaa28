"""itw_amd -- thin host binding of libispc_texcomp.so (the MI355X-native BCn encoder).

The product is the C-ABI shared library built from ../csrc (extern "C"
CompressBlocksBC1/BC3/BC7/BC6H + GetProfile_*, the reference's own entry points,
/root/reference/3rdParty/Intel/Source/ispc_texcomp.h:67-107).  This package only
binds it with ctypes for tests and benchmarks and offers torch-tensor
conveniences (device memory, streams, torch.distributed are plumbing here).

There is no CPU implementation in this package: if the library is missing or no
GPU is present, calls raise / the library aborts.  Nothing here imports oracle/.
"""
from .abi import (  # noqa: F401
    lib, test_lib, TEST_HOOK_SYMBOLS, BC7_ROUTE_COUNTERS, lib_path, RgbaSurface, Bc7Settings, Bc6hSettings, EtcSettings, Bc1aSettings, BC_DITHER_RGB, BC_DITHER_A, BC_UNIFORM, BC7_PROFILES, BC6H_PROFILES,
    bc7_profile, bc6h_profile, etc_profile, compress, compress_numpy, band_for_part, version, device_info,
    BYTES_PER_BLOCK, EXPORTED_SYMBOLS, DXGI_FORMAT, DdsDesc, image_func, compress_image, PROGRESS_FUNC, pad_to_multiple_of_4, dds_file, decode, block_count, KEEPS_PARTIAL_BLOCKS, SIGNED_FORMATS,
    available, set_error_mode, last_error, ON_ERROR_ABORT, ON_ERROR_RETURN, set_bc7_path, set_bc7_pilot, compress_image_multigpu, multigpu_sub_bands, MultiGpuStats, source_sha256, bc7_two_subset_bounds, bc7_rotation_bounds, bc7_f02_scan,
    chain_bytes, compress_chain, mip_chain, decode_chain, decode_image, load_dds, dds_images,
    KtxDesc, ktx_file, ktx_images, load_ktx,
    PreviewView, PREVIEW_CHANNEL, PREVIEW_CHANNEL_MASK, PREVIEW_TILE_MAX_ZOOM, preview_view, preview, preview_surface,
    ErrorStats, OWN_CHANNELS, measure, measure_async, measure_chain, stats_from_tensor,
    RefineStats, compress_refined, RefinePolicy, RefineTargetStats, compress_refined_to, psnr_to_total_sse,
    compress_chain_refined, compress_chain_refined_to, chain_psnr_to_total_sse,
    NORMAL_FLIP_X, NORMAL_FLIP_Y, NORMAL_NORMALIZE, normal_ops, prepare_normal_map, compress_normal_map, quantize_normal_map, compress_normal_map_snorm, compress_chain_normal_snorm, compress_mipped_normal_snorm, cube_cross_faces,
    NORMAL_FROM_HEIGHT, HEIGHT_CHANNEL, HEIGHT_MIRROR_U, HEIGHT_MIRROR_V, HEIGHT_INVERT_SIGN, HEIGHT_OCCLUSION, height_ops, height_amplitude, height_to_normal,
    MIP_PER_LEVEL, MIP_SRGB, MIP_CUBIC, MIP_TRIANGLE, MIP_WRAP_U, MIP_WRAP_V, MIP_RESIZE, MIP_POINT, MIP_LINEAR, MIP_MIRROR_U, MIP_MIRROR_V, mip_filter_flags,
    resize_flags, fit_size, resize, resize_chain_into, mip_levels, mip_chain_layout, generate_mips, generate_mips_into, compress_mipped,
    srgb_to_linear, linear_to_srgb, srgb_encode_device,
    MipAlpha, MipCoverage, alpha_coverage,
    MIP_WRAP_W, MIP_VOLUME, DDS_VOLUME, mip_filter_flags_3d, mip_levels_3d, mip_slices_3d, mip_chain_layout_3d, generate_mips_3d, generate_mips_3d_into, compress_volume,
    DdsVolumeDesc, dds_volume_file, dds_volume_images, load_dds_volume,
)
