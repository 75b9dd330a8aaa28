"""ctypes binding of the drop-in C ABI (include/ispc_texcomp.h, include/itw_amd.h)."""
import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.normpath(os.path.join(_PKG, "..", "lib", "libispc_texcomp.so"))
_TEST_LIB = os.path.normpath(os.path.join(_PKG, "..", "lib", "libispc_texcomp_test.so"))

BYTES_PER_BLOCK = {"bc1": 8, "bc3": 16, "bc7": 16, "bc6h": 16, "bc4": 8, "bc5": 16, "bc4_snorm": 8, "bc5_snorm": 16, "etc1": 8, "bc1a": 8, "bc1a_srgb": 8, "bc2": 16, "bc2_srgb": 16, "bc3_dxtex": 16, "bc3_dxtex_srgb": 16}
KEEPS_PARTIAL_BLOCKS = ("bc4", "bc5", "bc4_snorm", "bc5_snorm", "bc1a", "bc1a_srgb", "bc2", "bc2_srgb", "bc3_dxtex", "bc3_dxtex_srgb")     # DirectXTex formats: ceil(w/4) x ceil(h/4) blocks (include/itw_bc45.h)
SIGNED_FORMATS = ("bc4_snorm", "bc5_snorm")     # RGBA8_SNORM sources: int8 arrays / tensors, never uint8 (include/itw_bc45.h)
BC7_PROFILES = ("ultrafast", "veryfast", "fast", "basic", "slow",
                "alpha_ultrafast", "alpha_veryfast", "alpha_fast", "alpha_basic", "alpha_slow")
BC6H_PROFILES = ("veryfast", "fast", "basic", "slow", "veryslow")

# every symbol include/*.h declares
EXPORTED_SYMBOLS = tuple(
    ["CompressBlocksBC1", "CompressBlocksBC3", "CompressBlocksBC6H", "CompressBlocksBC7"]
    + ["GetProfile_" + p for p in BC7_PROFILES] + ["GetProfile_bc6h_" + p for p in BC6H_PROFILES]
    + ["itwSetStream", "itwGetStream", "itwAvailable", "itwSetErrorMode", "itwLastError", "itwClearError", "itwSetBc7Path", "itwSetBc7Pilot",
       "itwDeviceInfo", "itwVersion", "itwBandForPart", "itwBandForPartEx", "itwGetProfile_etc_slow", "itwCompressBlocksETC1"]
    # include/itw_dispatch.h: the reference's dispatch layer (win32Threads.h), slice loop, pad pre-pass
    + ["GetProcessorCount", "InitWin32Threads", "DestroyThreads", "GetBytesPerBlock", "CompressImageMT", "CompressImageST",
       "CompressImageBC1", "CompressImageBC3", "CompressImageBC4", "CompressImageBC5", "CompressImageBC4S", "CompressImageBC5S"]
    + ["CompressImageBC7_" + p for p in BC7_PROFILES] + ["CompressImageBC6H_" + p for p in BC6H_PROFILES]
    + ["itwCompressImageSliced", "itwCompressImageSlicedEx", "itwChainBytes", "itwCompressImageChain", "itwCompressImageChainEx", "itwCompressImageRefined", "itwCompressImageRefinedTo", "itwPsnrToTotalSse", "itwCompressImageChainRefined", "itwCompressImageChainRefinedTo", "itwChainPsnrToTotalSse", "itwSetSliceWindow", "itwSliceWindow", "itwSliceWindowFor", "itwPadToMultipleOf4", "itwFreeSurface", "itwPadToMultipleOf4Device",
       "itwConvertToRGBA8Device", "itwConvertToRGBA16FDevice",
       "itwPrepareNormalMapChain", "itwCompressNormalMapChain", "itwQuantizeNormalMapChain", "itwCompressSignedNormalMapChain", "itwCompressSignedNormalMapMipped", "itwCubeCrossFaces",
       "itwMipLevels", "itwMipChainLayout", "itwGenerateMipChain", "itwCompressImageMipped", "itwCompressImageMippedEx", "itwSrgbToLinear", "itwLinearToSrgb",
       "itwGenerateMipChainAlpha", "itwCompressImageMippedAlpha", "itwAlphaCoverage"]
    # include/itw_multigpu.h: one surface over all GPUs, one process
    + ["itwMultiGpuRanks", "itwMultiGpuTransport", "itwMultiGpuPeerLinks", "itwCompressImageMultiGPU", "itwCompressImageMultiGPUEx", "itwCompressImageMultiGPUBands",
       "itwMultiGpuSetInterleave", "itwMultiGpuPieces"]
    # include/itw_bc45.h: the DirectXTex formats of the plugin
    + ["CompressBlocksBC4", "CompressBlocksBC5", "itwWarmupBC45", "CompressBlocksBC4S", "CompressBlocksBC5S", "itwWarmupBC45S", "itwCompressNormalMapBC5", "itwCompressNormalMapBC5S"]
    # include/itw_decode.h: device decoders
    + ["itwDecodeBlocks", "itwDecodeChain", "itwDecodeImage", "itwMeasureBlocks", "itwMeasureChain", "itwStatsPsnr", "itwPreviewBlocks", "itwPreviewSurface"]
    # include/itw_dds.h: DDS container
    + ["itwDdsLevelBytes", "itwDdsHeaderBytes", "itwDdsFileBytes", "itwDdsWriteHeader", "itwDdsReadHeader", "itwDdsWriteFile", "itwDdsImage"]
    # include/itw_dds.h, second part: KTX 1.1 container (ETC1)
    + ["itwKtxHeaderBytes", "itwKtxFileBytes", "itwKtxWriteHeader", "itwKtxReadHeader", "itwKtxWriteFile", "itwKtxImage"])
# include/itw_test_hooks.h: exported by libispc_texcomp_test.so only (the same sources built with -DITW_TEST_HOOKS), never by the product
TEST_HOOK_SYMBOLS = ("itwTestRcp", "itwTestRsqrt", "itwTestF2I", "itwTestBc7TwoSubsetBounds", "itwTestBc7RotationBounds", "itwTestBc7F02Scan", "itwTestBc45IndexTable", "itwTestBc45ClosestS",
                     "itwMultiGpuTestInjectFailure", "itwTestCombinerHold", "itwTestCombinerCounters", "itwTestBc7RouteCounters", "itwTestBc7RouteCountersReset",
                     "itwTestBc7CallCountersArm", "itwTestBc7CallCounters", "itwTestSrgbEncode", "itwTestAlphaHistVariant", "itwTestMipCubicVariant",
                     "itwTestMipFilterTable", "itwTestResizeTable", "itwTestWalks32")
# enum itw_test_bc7_call_counter (include/itw_test_hooks.h): what itwTestBc7CallCounters fills; the per-band ones are band 0 then band 1
BC7_CALL_COUNTERS = ("pilot_listed", "pilot_sampled", "pilot_flag", "rot00", "rot01", "rot02", "rot10", "rot11", "rot12", "listed0", "listed1",
                     "pairs0", "pairs1", "overflow0", "overflow1", "redo0", "redo1")
# enum itw_test_bc7_route (include/itw_test_hooks.h), in its order: what itwTestBc7RouteCounters fills
BC7_ROUTE_COUNTERS = ("WIDE", "PER_FAMILY", "ALPHA_FIRST_BOUNDED7", "ALPHA_FIRST_BOUNDED", "ALPHA_FIRST_PLAIN", "RGB_BOUNDED", "REFERENCE_ORDER", "PROBE_IGNORED",
                      "TWO_BANDS", "PILOT", "PAIRS", "ROT_TASKS", "COMPACT", "HOST_VERDICT", "PROBE",
                      "SHAPE_WHOLE", "SHAPE_STAGED", "SHAPE_BAND", "SHAPE_VERDICT_BAND", "SHAPE_PROBE")




class RgbaSurface(C.Structure):
    """struct rgba_surface (ispc_texcomp.h:19-25): 24 bytes."""
    _fields_ = [("ptr", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32)]


class Bc7Settings(C.Structure):
    """struct bc7_enc_settings (ispc_texcomp.h:27-41): 64 bytes."""
    _fields_ = [("mode_selection", C.c_bool * 4), ("refineIterations", C.c_int * 8),
                ("skip_mode2", C.c_bool), ("fastSkipTreshold_mode1", C.c_int),
                ("fastSkipTreshold_mode3", C.c_int), ("fastSkipTreshold_mode7", C.c_int),
                ("mode45_channel0", C.c_int), ("refineIterations_channel", C.c_int),
                ("channels", C.c_int)]


class Bc6hSettings(C.Structure):
    """struct bc6h_enc_settings (ispc_texcomp.h:43-50): 16 bytes."""
    _fields_ = [("slow_mode", C.c_bool), ("fast_mode", C.c_bool), ("refineIterations_1p", C.c_int),
                ("refineIterations_2p", C.c_int), ("fastSkipTreshold", C.c_int)]


class EtcSettings(C.Structure):
    """struct etc_enc_settings (ispc_texcomp.h:52-55): 4 bytes."""
    _fields_ = [("fastSkipTreshold", C.c_int)]


BC_DITHER_RGB, BC_DITHER_A, BC_UNIFORM = 0x10000, 0x20000, 0x40000      # ITW_BC_* (itw_dispatch.h): DirectXTex's BC_FLAGS_* values


class Bc1aSettings(C.Structure):
    """struct itw_bc1a_settings (itw_dispatch.h), 16 bytes: the settings of "bc1a" / "bc1a_srgb", BC1 with 1-bit alpha by DirectXTex's encoder.
    A texel is transparent when its alpha (code * (1/255) in fp32) < alpha_ref; a caller who kept coverage with alpha_coverage=r passes
    alpha_ref=Bc1aSettings.ref_of(r).  None where settings are taken means Bc1aSettings().
    "bc2" / "bc2_srgb" take the same struct: BC2 has no colour key, so alpha_ref is checked (finite) but ignored; dither_a diffuses the error
    of the 4-bit alpha, dither_rgb and uniform mean what they mean for "bc1a".
    "bc3_dxtex" / "bc3_dxtex_srgb" take it too, alpha_ref ignored likewise: dither_a diffuses the error of the 3-bit alpha indices."""
    _fields_ = [("struct_size", C.c_uint32), ("alpha_ref", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]

    def __init__(self, alpha_ref=0.5, dither_rgb=False, dither_a=False, uniform=False):
        super().__init__(16, alpha_ref, (BC_DITHER_RGB if dither_rgb else 0) | (BC_DITHER_A if dither_a else 0) | (BC_UNIFORM if uniform else 0), 0)

    @staticmethod
    def ref_of(code):
        """(float)code * (1.0f / 255.0f): the texel conversion's own expression, so that a < alpha_ref is a < code on the integer codes."""
        import numpy as np
        return float(np.float32(code) * (np.float32(1.0) / np.float32(255.0)))


assert C.sizeof(RgbaSurface) == 24 and C.sizeof(Bc7Settings) == 64 and C.sizeof(Bc6hSettings) == 16 and C.sizeof(EtcSettings) == 4 and C.sizeof(Bc1aSettings) == 16

# "etc1": ITW_FORMAT_ETC1_RGB8, the GL enum (ETC1 has no DXGI code); decode, measure, the slice pipeline and the chain calls take it (with an
# EtcSettings); the refined calls, the multi-GPU calls and DDS refuse it -- its container is KTX (KtxDesc, ktx_file, load_ktx)
# "bc1a" / "bc1a_srgb": ITW_FORMAT_BC1A_UNORM[_SRGB], GL enums likewise (DXGI has no code for BC1 with alpha): the slice pipeline, the chain and
# the mipped calls encode them (with a Bc1aSettings or None); decode, measure, preview and DDS take them as synonyms of "bc1" / "bc1_srgb"
# "bc2" / "bc2_srgb": ITW_FORMAT_BC2_UNORM[_SRGB], GL enums too -- DXGI's 74 / 75 stay refused codes at the entry points and live in DDS files only;
# encoded where "bc1a" is (same Bc1aSettings), decoded, measured and previewed under the same two codes, stored by dds_file as DXT3 / DX10 74 / 75
# "bc6h_signed": ITW_FORMAT_BC6H_SIGNED, the GL enum of the SIGNED reading of a BC6H stream (what a GPU shows for a BC6H_SF16 texture): a decode key
# only -- decode, decode_chain, decode_image, measure, measure_chain and preview take it (uint16 half bit patterns, like "bc6h"), load_dds decodes
# a file labelled 96 under it, and every compress* raises ValueError: there is no signed BC6H encoder ("bc6h_sf16" still encodes the
# reference's unsigned-coded blocks, and decode("bc6h_sf16") is not offered)
# "bc3_dxtex" / "bc3_dxtex_srgb": ITW_FORMAT_BC3_DXTEX[_SRGB], BC3 by DirectXTex's D3DXEncodeBC3 ("bc3" stays kernel.ispc's encoder): encoded where
# "bc1a" is (same Bc1aSettings); decode, measure, preview and DDS take them as synonyms of "bc3" / "bc3_srgb" (load_dds reports 77 / 78)
DXGI_FORMAT = {"bc3_dxtex": 0x83F3, "bc3_dxtex_srgb": 0x8C4F, "bc6h_signed": 0x8E8E, "bc2": 0x83F2, "bc2_srgb": 0x8C4E, "bc1a": 0x83F1, "bc1a_srgb": 0x8C4D, "etc1": 0x8D64, "bc1": 71, "bc1_srgb": 72, "bc3": 77, "bc3_srgb": 78, "bc4": 80, "bc4_snorm": 81, "bc5": 83, "bc5_snorm": 84, "bc6h": 95, "bc6h_sf16": 96, "bc7": 98, "bc7_srgb": 99}


class DdsDesc(C.Structure):
    """struct ItwDdsDesc (itw_dds.h)."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("mip_levels", C.c_uint32), ("dxgi_format", C.c_uint32),
                ("is_cubemap", C.c_uint32), ("array_size", C.c_uint32)]


DDS_VOLUME = 2        # ITW_DDS_VOLUME (itw_dds.h): DdsDesc.is_cubemap of a volume texture, whose array_size is the depth of level 0


def DdsVolumeDesc(width, height, depth, mip_levels, dxgi_format):
    """The DdsDesc of a volume texture: is_cubemap = ITW_DDS_VOLUME, array_size = depth; slices level-major."""
    return DdsDesc(width, height, mip_levels, dxgi_format, DDS_VOLUME, depth)


class KtxDesc(C.Structure):
    """struct ItwKtxDesc (itw_dds.h)."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("mip_levels", C.c_uint32), ("gl_internal_format", C.c_uint32),
                ("is_cubemap", C.c_uint32), ("key_value_bytes", C.c_uint32)]


class MultiGpuRankStats(C.Structure):
    """struct itw_multigpu_rank_stats (itw_multigpu.h)."""
    _fields_ = [("rank", C.c_int32), ("device", C.c_int32), ("block_row0", C.c_int32), ("block_rows", C.c_int32),
                ("upload_ms", C.c_float), ("encode_ms", C.c_float), ("gather_ms", C.c_float), ("span_ms", C.c_float)]


class MultiGpuStats(C.Structure):
    """struct itw_multigpu_stats (itw_multigpu.h)."""
    _fields_ = [("ranks", C.c_int32), ("devices", C.c_int32), ("peer_links", C.c_int32), ("rccl_ranks", C.c_int32),
                ("watchdog_fired", C.c_int32), ("resident_bands", C.c_int32), ("wall_ms", C.c_float), ("posted_ms", C.c_float),
                ("transport", C.c_char * 8), ("transport_note", C.c_char * 96), ("rank", MultiGpuRankStats * 64),
                ("interleave", C.c_int32)]          # appended after round 4: the offsets above never move

    def as_dict(self):
        n = max(0, min(int(self.ranks), 64))
        return {"ranks": int(self.ranks), "devices": int(self.devices), "peer_links": int(self.peer_links), "rccl_ranks": int(self.rccl_ranks),
                "watchdog_fired": bool(self.watchdog_fired), "resident_bands": bool(self.resident_bands), "interleave": int(self.interleave),
                "wall_ms": round(float(self.wall_ms), 4), "posted_ms": round(float(self.posted_ms), 4),
                "transport": self.transport.decode(), "transport_note": self.transport_note.decode(),
                "per_rank": [{"rank": int(r.rank), "device": int(r.device), "block_row0": int(r.block_row0), "block_rows": int(r.block_rows),
                              "upload_ms": round(float(r.upload_ms), 4), "encode_ms": round(float(r.encode_ms), 4),
                              "gather_ms": round(float(r.gather_ms), 4), "span_ms": round(float(r.span_ms), 4)} for r in self.rank[:n]]}


# the channels of a decoded texel that carry a format's own data (the others are fill values: itw_decode.h)
OWN_CHANNELS = {"bc1": "rgb", "bc3": "rgba", "bc4": "r", "bc5": "rg", "bc4_snorm": "r", "bc5_snorm": "rg", "bc6h": "rgb", "bc7": "rgba", "etc1": "rgb", "bc1a": "rgba", "bc1a_srgb": "rgba", "bc2": "rgba", "bc2_srgb": "rgba", "bc3_dxtex": "rgba", "bc3_dxtex_srgb": "rgba"}
_DXGI_BASE = {71: "bc1", 72: "bc1", 77: "bc3", 78: "bc3", 80: "bc4", 81: "bc4_snorm", 83: "bc5", 84: "bc5_snorm", 95: "bc6h", 96: "bc6h",
              98: "bc7", 99: "bc7", 0x8D64: "etc1", 0x83F2: "bc2", 0x8C4E: "bc2", 0x8E8E: "bc6h"}


def _encodes(fn):
    """Decorator of every compress*: "bc6h_signed" names a reading of a stream, not an encoder."""
    import functools

    @functools.wraps(fn)
    def checked(fmt, *args, **kwargs):
        if fmt == "bc6h_signed":
            raise ValueError(f"{fn.__name__}: 'bc6h_signed' is a decode format: there is no signed BC6H encoder")
        return fn(fmt, *args, **kwargs)
    return checked


def _base(fmt):
    """Key of BYTES_PER_BLOCK for a key of DXGI_FORMAT: 'bc7_srgb' -> 'bc7'; the signed formats and 'bc3_dxtex' are their own base."""
    return fmt if fmt in SIGNED_FORMATS else "bc3_dxtex" if fmt.startswith("bc3_dxtex") else fmt.split("_")[0]


def _check_texel_type(fmt, img):
    """The signed formats take int8 texels and nothing else: a uint8 array reinterpreted as int8 would encode 200 as -56 without a word."""
    if fmt in SIGNED_FORMATS and not str(img.dtype).endswith(".int8") and str(img.dtype) != "int8":     # numpy "int8", torch "torch.int8"
        raise TypeError(f"{fmt} encodes RGBA8_SNORM: pass an int8 array / tensor, not {img.dtype} "
                        "(view uint8 bytes as int8 if they are two's complement codes)")


def _channel_mask(channels):
    """Bit mask (bit 0 = R .. bit 3 = A) of `channels`: a string of the letters r, g, b, a or an iterable of indices 0..3."""
    mask = 0
    for c in channels:
        mask |= 1 << ("rgba".index(c.lower()) if isinstance(c, str) else int(c))
    assert 0 <= mask < 16
    return mask


PREVIEW_CHANNEL = {"r": 0x04, "g": 0x08, "b": 0x10, "a": 0x20}     # ITW_PREVIEW_CHANNEL_* (itw_decode.h)
PREVIEW_CHANNEL_MASK = 0x3C
PREVIEW_TILE_MAX_ZOOM = 2.0                                        # ITW_PREVIEW_TILE_MAX_ZOOM: zoom <= this takes the kernel's tile route


class PreviewView(C.Structure):
    """struct itw_preview_view (itw_decode.h): the viewport of itwPreviewBlocks / itwPreviewSurface, 40 bytes."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("x_offset", C.c_int32), ("y_offset", C.c_int32), ("zoom", C.c_double),
                ("options", C.c_uint32), ("matte_color", C.c_uint32), ("exposure", C.c_float), ("_pad", C.c_uint32)]


class ErrorStats(C.Structure):
    """struct itw_error_stats (itw_decode.h): what itwMeasureBlocks reports, all integers."""
    _fields_ = [("dxgi_format", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("reserved_blocks", C.c_uint32),
                ("blocks", C.c_uint64), ("sse", C.c_uint64 * 4), ("max_abs", C.c_uint32 * 4), ("worst_block_sse", C.c_uint64),
                ("worst_block", C.c_uint32), ("_pad", C.c_uint32), ("mode_hist", C.c_uint64 * 16)]

    def _mask(self, channels):
        return _channel_mask(OWN_CHANNELS[_DXGI_BASE[int(self.dxgi_format)]] if channels is None else channels)

    def mse(self, channels=None):
        """Mean squared code difference over `channels` ('rgb', 'a', (0, 1), ...; default: the format's own channels)."""
        mask = self._mask(channels)
        picked = [c for c in range(4) if mask >> c & 1]
        return sum(int(self.sse[c]) for c in picked) / float(int(self.width) * int(self.height) * len(picked))

    def psnr(self, channels=None):
        """itwStatsPsnr over `channels`; ValueError for BC6H, whose codes are half-float bit patterns."""
        if _DXGI_BASE.get(int(self.dxgi_format)) == "bc6h":
            raise ValueError("PSNR is not defined for BC6H code differences; use sse / max_abs")
        return float(lib().itwStatsPsnr(C.byref(self), self._mask(channels)))

    def as_dict(self):
        return {"dxgi_format": int(self.dxgi_format), "width": int(self.width), "height": int(self.height),
                "reserved_blocks": int(self.reserved_blocks), "blocks": int(self.blocks), "sse": [int(v) for v in self.sse],
                "max_abs": [int(v) for v in self.max_abs], "worst_block_sse": int(self.worst_block_sse), "worst_block": int(self.worst_block),
                "mode_hist": [int(v) for v in self.mode_hist]}

    def __eq__(self, other):
        return isinstance(other, ErrorStats) and bytes(self) == bytes(other)

    __hash__ = None


assert C.sizeof(ErrorStats) == 216


class RefineStats(C.Structure):
    """struct itw_refine_stats (itw_dispatch.h): what itwCompressImageRefined reports, all integers."""
    _fields_ = [("blocks", C.c_uint64), ("listed", C.c_uint64), ("replaced", C.c_uint64), ("sse_first", C.c_uint64), ("sse_final", C.c_uint64),
                ("worst_first", C.c_uint64), ("worst_final", C.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


assert C.sizeof(RefineStats) == 56


class RefinePolicy(C.Structure):
    """struct itw_refine_policy (itw_dispatch.h): what itwCompressImageRefinedTo may spend and has to reach."""
    _fields_ = [("max_listed", C.c_uint64), ("target_total_sse", C.c_uint64)]


class RefineTargetStats(C.Structure):
    """struct itw_refine_target_stats (itw_dispatch.h): itw_refine_stats over the whole call, then what each round chose and listed."""
    _fields_ = [("total", RefineStats), ("rounds", C.c_uint32), ("target_met", C.c_uint32), ("budget", C.c_uint64 * 5), ("listed", C.c_uint64 * 5)]

    def as_dict(self):
        d = self.total.as_dict()
        d.update(rounds=int(self.rounds), target_met=int(self.target_met), budget=[int(v) for v in self.budget],
                 listed_per_round=[int(v) for v in self.listed])
        return d


assert C.sizeof(RefinePolicy) == 16 and C.sizeof(RefineTargetStats) == 144
UINT64_MAX = 2 ** 64 - 1

COMPRESSION_FUNC = C.CFUNCTYPE(None, C.POINTER(RgbaSurface), C.c_void_p)
PROGRESS_FUNC = C.CFUNCTYPE(C.c_bool, C.c_int, C.c_int, C.c_void_p)

_lib = None
_test_lib = None


def lib_path():
    return _LIB


def lib():
    """Load libispc_texcomp.so (the product); raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        _lib = _load(_LIB, hooks=False)
    return _lib


def test_lib():
    """Load libispc_texcomp_test.so: the product's sources built with -DITW_TEST_HOOKS, which adds the entry points of
    include/itw_test_hooks.h.  A second, independent instance of the library in the process; tests/ use it for the hook calls only."""
    global _test_lib
    if _test_lib is None:
        _test_lib = _load(_TEST_LIB, hooks=True)
    return _test_lib


def _load(path, hooks):
    if True:
        if not os.path.exists(path):
            raise RuntimeError(
                f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C intel-texture-works-plugin_amd/csrc`.  There is no CPU fallback.")
        L = C.CDLL(path, mode=C.RTLD_LOCAL if hooks else C.RTLD_GLOBAL)
        L.CompressBlocksBC1.argtypes = [C.POINTER(RgbaSurface), C.c_void_p]
        L.CompressBlocksBC4.argtypes = [C.POINTER(RgbaSurface), C.c_void_p]
        L.CompressBlocksBC5.argtypes = [C.POINTER(RgbaSurface), C.c_void_p]
        L.CompressBlocksBC4.restype = None
        L.itwWarmupBC45.restype = None
        for n in ("CompressBlocksBC4S", "CompressBlocksBC5S", "CompressImageBC4S", "CompressImageBC5S"):
            getattr(L, n).argtypes = [C.POINTER(RgbaSurface), C.c_void_p]
            getattr(L, n).restype = None
        L.itwWarmupBC45S.restype = None
        L.CompressBlocksBC5.restype = None
        L.CompressBlocksBC3.argtypes = [C.POINTER(RgbaSurface), C.c_void_p]
        L.CompressBlocksBC7.argtypes = [C.POINTER(RgbaSurface), C.c_void_p, C.POINTER(Bc7Settings)]
        L.CompressBlocksBC6H.argtypes = [C.POINTER(RgbaSurface), C.c_void_p, C.POINTER(Bc6hSettings)]
        for n in ("CompressBlocksBC1", "CompressBlocksBC3", "CompressBlocksBC7", "CompressBlocksBC6H"):
            getattr(L, n).restype = None
        L.itwGetProfile_etc_slow.argtypes = [C.POINTER(EtcSettings)]
        L.itwGetProfile_etc_slow.restype = None
        L.itwCompressBlocksETC1.argtypes = [C.POINTER(RgbaSurface), C.c_void_p, C.POINTER(EtcSettings)]
        L.itwCompressBlocksETC1.restype = None
        L.itwSetStream.argtypes = [C.c_void_p]
        L.itwSetStream.restype = None
        L.itwGetStream.restype = C.c_void_p
        L.itwDeviceInfo.restype = C.c_char_p
        L.itwAvailable.restype = C.c_int
        L.itwSetErrorMode.argtypes = [C.c_int]
        L.itwSetErrorMode.restype = None
        L.itwLastError.restype = C.c_char_p
        L.itwClearError.restype = None
        L.itwSetBc7Path.argtypes = [C.c_int]
        L.itwSetBc7Path.restype = None
        L.itwSetBc7Pilot.argtypes = [C.c_int]
        L.itwSetBc7Pilot.restype = None
        L.itwVersion.restype = C.c_char_p
        L.itwBandForPart.argtypes = [C.c_int32] * 5 + [C.POINTER(C.c_int32)] * 2
        L.itwBandForPart.restype = C.c_int64
        L.itwBandForPartEx.argtypes = [C.c_int32] * 6 + [C.POINTER(C.c_int32)] * 2
        L.itwBandForPartEx.restype = C.c_int64
        if hooks:
            for n in ("itwTestRcp", "itwTestRsqrt", "itwTestF2I"):
                getattr(L, n).argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
                getattr(L, n).restype = None
            L.itwTestBc7TwoSubsetBounds.argtypes = [C.POINTER(RgbaSurface), C.c_void_p]
            L.itwTestBc7TwoSubsetBounds.restype = None
            L.itwTestBc7RotationBounds.argtypes = [C.POINTER(RgbaSurface), C.c_void_p]
            L.itwTestBc7RotationBounds.restype = None
            L.itwTestBc7F02Scan.argtypes = [C.POINTER(RgbaSurface), C.c_void_p]
            L.itwTestBc7F02Scan.restype = None
            L.itwTestBc45IndexTable.argtypes = [C.c_void_p]
            L.itwTestBc45IndexTable.restype = C.c_int
            L.itwTestBc45ClosestS.argtypes = [C.c_void_p]
            L.itwTestBc45ClosestS.restype = C.c_int
            L.itwMultiGpuTestInjectFailure.argtypes = [C.c_int, C.c_int, C.c_int]
            L.itwMultiGpuTestInjectFailure.restype = None
            L.itwTestCombinerHold.argtypes = [C.c_int, C.c_int]
            L.itwTestCombinerHold.restype = None
            L.itwTestCombinerCounters.argtypes = [C.POINTER(C.c_int64)]
            L.itwTestCombinerCounters.restype = None
            L.itwTestBc7RouteCounters.argtypes = [C.POINTER(C.c_int64), C.c_int]
            L.itwTestBc7RouteCounters.restype = None
            L.itwTestBc7RouteCountersReset.argtypes = []
            L.itwTestBc7RouteCountersReset.restype = None
            L.itwTestBc7CallCountersArm.argtypes = [C.c_int]
            L.itwTestBc7CallCountersArm.restype = None
            L.itwTestBc7CallCounters.argtypes = [C.POINTER(C.c_int32), C.c_int]
            L.itwTestBc7CallCounters.restype = None
            L.itwTestSrgbEncode.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
            L.itwTestSrgbEncode.restype = None
            L.itwTestAlphaHistVariant.argtypes = [C.c_int]
            L.itwTestAlphaHistVariant.restype = None
            L.itwTestMipCubicVariant.argtypes = [C.c_int]
            L.itwTestMipCubicVariant.restype = None
            L.itwTestMipFilterTable.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]
            L.itwTestMipFilterTable.restype = C.c_int64
            L.itwTestResizeTable.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]
            L.itwTestResizeTable.restype = C.c_int64
            L.itwTestWalks32.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int]
            L.itwTestWalks32.restype = C.c_int
        # dispatch layer (itw_dispatch.h)
        L.GetProcessorCount.restype = C.c_int
        L.GetBytesPerBlock.argtypes = [C.c_int]
        L.GetBytesPerBlock.restype = C.c_int
        for n in ("CompressImageMT", "CompressImageST"):
            getattr(L, n).argtypes = [C.POINTER(RgbaSurface), C.c_void_p, C.c_void_p, C.c_int]
            getattr(L, n).restype = C.c_bool
        for n in ["CompressImageBC1", "CompressImageBC3"] + ["CompressImageBC7_" + p for p in BC7_PROFILES] \
                + ["CompressImageBC6H_" + p for p in BC6H_PROFILES]:
            getattr(L, n).argtypes = [C.POINTER(RgbaSurface), C.c_void_p]
            getattr(L, n).restype = None
        L.itwCompressImageSliced.argtypes = [C.POINTER(RgbaSurface), C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_bool,
                                             C.c_int64, C.c_void_p, C.c_void_p]
        L.itwCompressImageSliced.restype = C.c_bool
        L.itwCompressImageSlicedEx.argtypes = [C.POINTER(RgbaSurface), C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.itwCompressImageSlicedEx.restype = C.c_bool
        L.itwChainBytes.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.itwChainBytes.restype = C.c_int64
        L.itwCompressImageChain.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.itwCompressImageChain.restype = C.c_bool
        L.itwCompressImageChainEx.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.itwCompressImageChainEx.restype = C.c_bool
        L.itwCompressImageRefined.argtypes = [C.POINTER(RgbaSurface), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64,
                                              C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.itwCompressImageRefined.restype = C.c_bool
        L.itwCompressImageRefinedTo.argtypes = [C.POINTER(RgbaSurface), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t,
                                                C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.itwCompressImageRefinedTo.restype = C.c_bool
        L.itwPsnrToTotalSse.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_double]
        L.itwPsnrToTotalSse.restype = C.c_uint64
        L.itwCompressImageChainRefined.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64,
                                                   C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.itwCompressImageChainRefined.restype = C.c_bool
        L.itwCompressImageChainRefinedTo.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t,
                                                     C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.itwCompressImageChainRefinedTo.restype = C.c_bool
        L.itwChainPsnrToTotalSse.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_double]
        L.itwChainPsnrToTotalSse.restype = C.c_uint64
        L.itwSetSliceWindow.argtypes = [C.c_int]
        L.itwSetSliceWindow.restype = None
        L.itwSliceWindow.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64]
        L.itwSliceWindow.restype = C.c_int
        L.itwSliceWindowFor.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int64]
        L.itwSliceWindowFor.restype = C.c_int
        L.itwMultiGpuRanks.restype = C.c_int
        L.itwMultiGpuSetInterleave.argtypes = [C.c_int]
        L.itwMultiGpuSetInterleave.restype = None
        L.itwMultiGpuPieces.argtypes = [C.c_int32, C.c_int, C.c_int]
        L.itwMultiGpuPieces.restype = C.c_int
        L.itwMultiGpuTransport.restype = C.c_char_p
        L.itwMultiGpuPeerLinks.restype = C.c_int
        L.itwCompressImageMultiGPU.argtypes = [C.POINTER(RgbaSurface), C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.itwCompressImageMultiGPU.restype = C.c_bool
        L.itwCompressImageMultiGPUEx.argtypes = [C.POINTER(RgbaSurface), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(RgbaSurface),
                                                 C.POINTER(MultiGpuStats)]
        L.itwCompressImageMultiGPUEx.restype = C.c_bool
        L.itwCompressImageMultiGPUBands.argtypes = [C.POINTER(RgbaSurface), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(RgbaSurface), C.c_int,
                                                    C.POINTER(MultiGpuStats)]
        L.itwCompressImageMultiGPUBands.restype = C.c_bool
        L.itwPadToMultipleOf4.argtypes = [C.POINTER(RgbaSurface), C.c_int]
        L.itwPadToMultipleOf4.restype = RgbaSurface
        L.itwFreeSurface.argtypes = [C.POINTER(RgbaSurface)]
        L.itwFreeSurface.restype = None
        L.itwPadToMultipleOf4Device.argtypes = [C.POINTER(RgbaSurface), C.c_int, C.c_void_p]
        L.itwPadToMultipleOf4Device.restype = None
        L.itwConvertToRGBA8Device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.itwConvertToRGBA8Device.restype = C.c_int
        L.itwConvertToRGBA16FDevice.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.itwConvertToRGBA16FDevice.restype = C.c_int
        L.itwPrepareNormalMapChain.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32]
        L.itwPrepareNormalMapChain.restype = C.c_int
        L.itwCompressNormalMapChain.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.itwCompressNormalMapChain.restype = C.c_bool
        L.itwCompressNormalMapBC5.argtypes = [C.POINTER(RgbaSurface), C.c_void_p, C.c_uint32]
        L.itwCompressNormalMapBC5.restype = None
        L.itwQuantizeNormalMapChain.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_uint32]
        L.itwQuantizeNormalMapChain.restype = C.c_int
        L.itwCompressSignedNormalMapChain.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
        L.itwCompressSignedNormalMapChain.restype = C.c_bool
        L.itwCompressSignedNormalMapMipped.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.itwCompressSignedNormalMapMipped.restype = C.c_bool
        L.itwCompressNormalMapBC5S.argtypes = [C.POINTER(RgbaSurface), C.c_int, C.c_void_p, C.c_uint32]
        L.itwCompressNormalMapBC5S.restype = None
        L.itwCubeCrossFaces.argtypes = [C.POINTER(RgbaSurface), C.c_int, C.POINTER(RgbaSurface)]
        L.itwCubeCrossFaces.restype = C.c_int
        L.itwMipLevels.argtypes = [C.c_int, C.c_int]
        L.itwMipLevels.restype = C.c_int
        L.itwMipChainLayout.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.itwMipChainLayout.restype = C.c_int64
        L.itwGenerateMipChain.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32]
        L.itwGenerateMipChain.restype = C.c_int
        L.itwCompressImageMipped.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.itwCompressImageMipped.restype = C.c_bool
        L.itwCompressImageMippedEx.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.itwCompressImageMippedEx.restype = C.c_bool
        L.itwGenerateMipChainAlpha.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
        L.itwGenerateMipChainAlpha.restype = C.c_int
        L.itwCompressImageMippedAlpha.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.itwCompressImageMippedAlpha.restype = C.c_bool
        L.itwAlphaCoverage.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.itwAlphaCoverage.restype = C.c_int
        L.itwSrgbToLinear.argtypes = [C.c_uint8]
        L.itwSrgbToLinear.restype = C.c_float
        L.itwLinearToSrgb.argtypes = [C.c_float]
        L.itwLinearToSrgb.restype = C.c_uint8
        L.itwDecodeBlocks.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
        L.itwDecodeBlocks.restype = C.c_int
        L.itwDecodeChain.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.itwDecodeChain.restype = C.c_int
        L.itwDecodeImage.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.itwDecodeImage.restype = C.c_int
        L.itwMeasureBlocks.argtypes = [C.c_int, C.c_void_p, C.POINTER(RgbaSurface), C.c_void_p, C.c_size_t, C.c_void_p]
        L.itwMeasureBlocks.restype = C.c_int
        L.itwMeasureChain.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        L.itwMeasureChain.restype = C.c_int
        L.itwStatsPsnr.argtypes = [C.POINTER(ErrorStats), C.c_uint32]
        L.itwStatsPsnr.restype = C.c_double
        L.itwPreviewBlocks.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(PreviewView), C.c_size_t, C.c_void_p, C.c_int64]
        L.itwPreviewBlocks.restype = C.c_int
        L.itwPreviewSurface.argtypes = [C.POINTER(RgbaSurface), C.c_int, C.POINTER(PreviewView), C.c_size_t, C.c_void_p, C.c_int64]
        L.itwPreviewSurface.restype = C.c_int
        # DDS container (itw_dds.h)
        L.itwDdsLevelBytes.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
        L.itwDdsLevelBytes.restype = C.c_size_t
        for n in ("itwDdsHeaderBytes", "itwDdsFileBytes"):
            getattr(L, n).argtypes = [C.POINTER(DdsDesc)]
            getattr(L, n).restype = C.c_size_t
        L.itwDdsWriteHeader.argtypes = [C.POINTER(DdsDesc), C.c_void_p, C.c_size_t]
        L.itwDdsWriteHeader.restype = C.c_size_t
        L.itwDdsReadHeader.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(DdsDesc)]
        L.itwDdsReadHeader.restype = C.c_size_t
        L.itwDdsWriteFile.argtypes = [C.POINTER(DdsDesc), C.POINTER(C.c_void_p), C.c_size_t, C.c_void_p, C.c_size_t]
        L.itwDdsWriteFile.restype = C.c_size_t
        L.itwDdsImage.argtypes = [C.POINTER(DdsDesc), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_size_t)]
        L.itwDdsImage.restype = C.c_size_t
        # KTX 1.1 container (itw_dds.h)
        for n in ("itwKtxHeaderBytes", "itwKtxFileBytes"):
            getattr(L, n).argtypes = [C.POINTER(KtxDesc)]
            getattr(L, n).restype = C.c_size_t
        L.itwKtxWriteHeader.argtypes = [C.POINTER(KtxDesc), C.c_void_p, C.c_size_t]
        L.itwKtxWriteHeader.restype = C.c_size_t
        L.itwKtxReadHeader.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(KtxDesc)]
        L.itwKtxReadHeader.restype = C.c_size_t
        L.itwKtxWriteFile.argtypes = [C.POINTER(KtxDesc), C.POINTER(C.c_void_p), C.c_size_t, C.c_void_p, C.c_size_t]
        L.itwKtxWriteFile.restype = C.c_size_t
        L.itwKtxImage.argtypes = [C.POINTER(KtxDesc), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_size_t)]
        L.itwKtxImage.restype = C.c_size_t
    return L


def version():
    return lib().itwVersion().decode()


def source_sha256():
    """SHA-256 over the kernel sources (csrc/*.hip, *.hpp, *.h, Makefile: names and bytes, sorted).  Profiles taken on the GPU box
    carry it (tools/profile_gpu.sh) and bench.py quotes committed counter values only when it equals the tree it runs from."""
    import hashlib
    d = os.path.normpath(os.path.join(_PKG, "..", "csrc"))
    h = hashlib.sha256()
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".hpp", ".h")) or name == "Makefile":
            h.update(name.encode() + b"\0")
            with open(os.path.join(d, name), "rb") as f:
                h.update(f.read())
    return h.hexdigest()


ON_ERROR_ABORT, ON_ERROR_RETURN = 0, 1
BC7_PATH = {"auto": 0, "deep": 1, "wide": 2}


def set_bc7_pilot(percent):
    """itwSetBc7Pilot: threshold of the bounded mode order's pilot in percent (0 = reference order for the rest of the surface, 100 = bounded,
    -1 = no pilot, None = back to the library's preset: ITW_BC7_PILOT_THR or 90); same bytes whatever the value."""
    lib().itwSetBc7Pilot(-2 if percent is None else int(percent))


def set_bc7_path(name):
    """itwSetBc7Path: 'auto' | 'deep' | 'wide' (same bytes either way; tests and probes)."""
    lib().itwSetBc7Path(BC7_PATH[name])


def available():
    """itwAvailable(): True if the current HIP device is a gfx950 this library can run on.  Never aborts."""
    return bool(lib().itwAvailable())


def set_error_mode(mode):
    lib().itwSetErrorMode(mode)


def last_error():
    """Message of the last failed ABI call on this host thread, or None."""
    e = lib().itwLastError()
    return e.decode() if e else None


def device_info():
    return lib().itwDeviceInfo().decode()


def bc7_profile(name):
    """GetProfile_<name> (ispc_texcomp.h:67-79) into a zero-initialised struct."""
    if name not in BC7_PROFILES:
        raise KeyError(name)
    s = Bc7Settings()
    getattr(lib(), "GetProfile_" + name)(C.byref(s))
    return s


def bc6h_profile(name):
    """GetProfile_bc6h_<name> (ispc_texcomp.h:81-85)."""
    if name not in BC6H_PROFILES:
        raise KeyError(name)
    s = Bc6hSettings()
    getattr(lib(), "GetProfile_bc6h_" + name)(C.byref(s))
    return s


def etc_profile(name="slow"):
    """itwGetProfile_etc_<name>: the reference has the one preset, `slow` (fastSkipTreshold 6)."""
    if name != "slow":
        raise KeyError(name)
    s = EtcSettings()
    lib().itwGetProfile_etc_slow(C.byref(s))
    return s


def band_for_part(width, height, fmt, part, parts):
    """(first_texel_row, texel_rows, output_byte_offset) of `part` among `parts` (itwBandForPart)."""
    y0, n = C.c_int32(), C.c_int32()
    off = lib().itwBandForPartEx(width, height, BYTES_PER_BLOCK[fmt], part, parts, 1 if fmt in KEEPS_PARTIAL_BLOCKS else 0, C.byref(y0), C.byref(n))
    if off < 0:
        raise ValueError((part, parts))
    return y0.value, n.value, off


def _call(fmt, surf, dst_ptr, settings):
    L = lib()
    if fmt == "bc1":
        L.CompressBlocksBC1(C.byref(surf), dst_ptr)
    elif fmt == "bc3":
        L.CompressBlocksBC3(C.byref(surf), dst_ptr)
    elif fmt == "bc4":
        L.CompressBlocksBC4(C.byref(surf), dst_ptr)
    elif fmt == "bc5":
        L.CompressBlocksBC5(C.byref(surf), dst_ptr)
    elif fmt == "bc4_snorm":
        L.CompressBlocksBC4S(C.byref(surf), dst_ptr)
    elif fmt == "bc5_snorm":
        L.CompressBlocksBC5S(C.byref(surf), dst_ptr)
    elif fmt == "bc7":
        st = settings if isinstance(settings, Bc7Settings) else bc7_profile(settings or "slow")
        L.CompressBlocksBC7(C.byref(surf), dst_ptr, C.byref(st))
    elif fmt == "bc6h":
        st = settings if isinstance(settings, Bc6hSettings) else bc6h_profile(settings or "slow")
        L.CompressBlocksBC6H(C.byref(surf), dst_ptr, C.byref(st))
    elif fmt == "etc1":
        st = settings if isinstance(settings, EtcSettings) else etc_profile(settings or "slow")
        L.itwCompressBlocksETC1(C.byref(surf), dst_ptr, C.byref(st))
    elif fmt in ("bc1a", "bc1a_srgb", "bc2", "bc2_srgb", "bc3_dxtex", "bc3_dxtex_srgb"):
        # no block-level entry point: the single image is the slice call with one slice (synchronous)
        assert settings is None or isinstance(settings, Bc1aSettings)
        pitch = ((surf.width + 3) // 4) * BYTES_PER_BLOCK[fmt]
        if not L.itwCompressImageSlicedEx(C.byref(surf), dst_ptr, pitch, DXGI_FORMAT[fmt], C.cast(C.byref(settings), C.c_void_p) if settings is not None else None,
                                          1 << 62, None, None) and L.itwLastError():
            raise RuntimeError(L.itwLastError().decode())
    else:
        raise ValueError(fmt)


def block_count(fmt, width, height):
    """Blocks a width x height surface encodes to: the ISPC formats drop partial blocks, the DirectXTex ones keep them."""
    if fmt in KEEPS_PARTIAL_BLOCKS:
        return ((width + 3) // 4) * ((height + 3) // 4)
    return (width // 4) * (height // 4)


@_encodes
def compress_numpy(fmt, img, settings=None):
    """Host-pointer path (what the Photoshop plugin does): img (H, W, 4) uint8, or uint16 half bits for bc6h, or int8 for the
    signed formats (TypeError for uint8).  Synchronous; returns a uint8 numpy array of packed blocks."""
    import numpy as np
    _check_texel_type(fmt, img)
    assert img.ndim == 3 and img.shape[2] == 4 and img.strides[2] == img.itemsize and img.strides[1] == 4 * img.itemsize
    assert img.dtype == (np.uint16 if fmt == "bc6h" else np.int8 if fmt in SIGNED_FORMATS else np.uint8)
    h, w = img.shape[:2]
    out = np.empty(block_count(fmt, w, h) * BYTES_PER_BLOCK[fmt], dtype=np.uint8)
    surf = RgbaSurface(img.ctypes.data, w, h, img.strides[0])
    _call(fmt, surf, out.ctypes.data, settings)
    return out


@_encodes
def compress(fmt, img, settings=None, out=None):
    """Device-resident path: img is a CUDA(HIP) torch tensor (H, W, 4) uint8, or int16/uint16/float16 for bc6h, or int8 for the
    signed formats (TypeError for uint8); rows may be strided.  Launches asynchronously on torch's current stream and returns a uint8
    CUDA tensor."""
    import torch
    _check_texel_type(fmt, img)
    assert img.is_cuda and img.dim() == 3 and img.shape[2] == 4
    es = img.element_size()
    assert es == (2 if fmt == "bc6h" else 1), "texel type does not match the format"
    assert img.stride(2) == 1 and img.stride(1) == 4
    h, w = img.shape[:2]
    nbytes = block_count(fmt, w, h) * BYTES_PER_BLOCK[fmt]
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=img.device)
    assert out.is_cuda and out.numel() >= nbytes and out.is_contiguous()
    L = lib()
    with torch.cuda.device(img.device):
        L.itwSetStream(torch.cuda.current_stream(img.device).cuda_stream)
        surf = RgbaSurface(img.data_ptr(), w, h, img.stride(0) * es)
        _call(fmt, surf, out.data_ptr(), settings)
    return out


def bc7_two_subset_bounds(img):
    """Test hook: the bounded BC7 mode order's lower bound of each two-subset shape (itwTestBc7TwoSubsetBounds).
    img: CUDA tensor (H, W, 4) uint8 -> float32 CUDA tensor (blocks, 64), raster block order."""
    import torch
    assert img.is_cuda and img.dim() == 3 and img.shape[2] == 4 and img.element_size() == 1
    assert img.stride(2) == 1 and img.stride(1) == 4
    h, w = img.shape[:2]
    out = torch.empty(((h // 4) * (w // 4), 64), dtype=torch.float32, device=img.device)
    L = test_lib()
    with torch.cuda.device(img.device):
        L.itwSetStream(torch.cuda.current_stream(img.device).cuda_stream)
        surf = RgbaSurface(img.data_ptr(), w, h, img.stride(0))
        L.itwTestBc7TwoSubsetBounds(C.byref(surf), out.data_ptr())
    e = L.itwLastError()
    if e:
        raise RuntimeError(e.decode())
    return out


def bc7_rotation_bounds(img):
    """Test hook: the lower bound of modes 4/5's candidates of each rotation under an RGB profile (itwTestBc7RotationBounds).
    img: CUDA tensor (H, W, 4) uint8 -> float32 CUDA tensor (blocks, 3), raster block order."""
    import torch
    assert img.is_cuda and img.dim() == 3 and img.shape[2] == 4 and img.element_size() == 1
    assert img.stride(2) == 1 and img.stride(1) == 4
    h, w = img.shape[:2]
    out = torch.empty(((h // 4) * (w // 4), 3), dtype=torch.float32, device=img.device)
    L = test_lib()
    with torch.cuda.device(img.device):
        L.itwSetStream(torch.cuda.current_stream(img.device).cuda_stream)
        surf = RgbaSurface(img.data_ptr(), w, h, img.stride(0))
        L.itwTestBc7RotationBounds(C.byref(surf), out.data_ptr())
    e = L.itwLastError()
    if e:
        raise RuntimeError(e.decode())
    return out


def bc7_f02_scan(img):
    """Test hook: the modes 0/2 scan of every block in the scheduled, cached order and in table order with nothing cached (itwTestBc7F02Scan).
    img: CUDA tensor (H, W, 4) uint8 -> int32 CUDA tensor (blocks, 2, 84), raster block order; [:, 0] scheduled, [:, 1] table order;
    [..., 0:4] mode 0's winner (error, shape) and mode 2's, [..., 4:20] mode 0's per-shape errors, [..., 20:84] mode 2's."""
    import torch
    assert img.is_cuda and img.dim() == 3 and img.shape[2] == 4 and img.element_size() == 1
    assert img.stride(2) == 1 and img.stride(1) == 4
    h, w = img.shape[:2]
    out = torch.full(((h // 4) * (w // 4), 2, 84), -1, dtype=torch.int32, device=img.device)
    L = test_lib()
    with torch.cuda.device(img.device):
        L.itwSetStream(torch.cuda.current_stream(img.device).cuda_stream)
        surf = RgbaSurface(img.data_ptr(), w, h, img.stride(0))
        L.itwTestBc7F02Scan(C.byref(surf), out.data_ptr())
    e = L.itwLastError()
    if e:
        raise RuntimeError(e.decode())
    return out


def image_func(fmt, profile=None, L=None):
    """Address of the CompressImage* trampoline (win32Threads.h:58-80) for a format / profile, as a void* (L: the library instance, default the product)."""
    name = {"bc1": "CompressImageBC1", "bc3": "CompressImageBC3", "bc4": "CompressImageBC4", "bc5": "CompressImageBC5",
            "bc4_snorm": "CompressImageBC4S", "bc5_snorm": "CompressImageBC5S"}.get(fmt) or \
        ("CompressImageBC7_" if fmt == "bc7" else "CompressImageBC6H_") + (profile or "slow")
    return C.cast(getattr(L or lib(), name), C.c_void_p)


@_encodes
def compress_image(fmt, img, profile=None, multithreaded=True, slice_pixels=0, progress=None, out=None, settings=None):
    """The plugin's save path below the pixel conversion (IntelPlugin.cpp:816-884): slice loop -> CompressImageMT/ST ->
    trampoline -> CompressBlocks* (itwCompressImageSliced; with `settings` -- a Bc7Settings / Bc6hSettings / EtcSettings -- through
    itwCompressImageSlicedEx; "etc1" has no trampoline and always goes that way, by default with etc_profile("slow")).  img: host numpy (H, W, 4) uint8 / uint16 half bits, or a CUDA torch tensor of that shape
    (then `out` is a CUDA uint8 tensor too unless given).  Returns (ok, blocks)."""
    import numpy as np
    _check_texel_type(fmt, img)
    h, w = img.shape[:2]
    nbytes = block_count(fmt, w, h) * BYTES_PER_BLOCK[fmt]
    on_device = hasattr(img, "data_ptr")
    if on_device:
        import torch
        if out is None:
            out = torch.zeros(nbytes, dtype=torch.uint8, device=img.device)
        surf = RgbaSurface(img.data_ptr(), w, h, img.stride(0) * img.element_size())
        lib().itwSetStream(torch.cuda.current_stream(img.device).cuda_stream)
    else:
        if out is None:
            out = np.zeros(nbytes, dtype=np.uint8)
        surf = RgbaSurface(img.ctypes.data, w, h, img.strides[0])
    dst = out.data_ptr() if hasattr(out, "data_ptr") else out.ctypes.data
    cb = PROGRESS_FUNC(progress) if progress else None
    pitch = block_count(fmt, w, 4) * BYTES_PER_BLOCK[fmt]
    if fmt == "etc1" and settings is None:
        settings = etc_profile(profile or "slow")
    if settings is not None or _base(fmt) in ("bc1a", "bc2", "bc3_dxtex"):           # ("bc1a", "bc2", "bc3_dxtex": no trampoline either; None is Bc1aSettings())
        ok = lib().itwCompressImageSlicedEx(C.byref(surf), dst, pitch, DXGI_FORMAT[fmt], C.cast(C.byref(settings), C.c_void_p) if settings is not None else None, slice_pixels,
                                            C.cast(cb, C.c_void_p) if cb else None, None)
    else:
        ok = lib().itwCompressImageSliced(C.byref(surf), dst, pitch, image_func(fmt, profile),
                                          DXGI_FORMAT[fmt], multithreaded, slice_pixels, C.cast(cb, C.c_void_p) if cb else None, None)
    return bool(ok), out


def _surfaces(images):
    """ctypes array of rgba_surface for a list of host numpy arrays / CUDA torch tensors (H, W, 4), rows may be strided."""
    surfs = []
    for img in images:
        if hasattr(img, "data_ptr"):
            assert img.dim() == 3 and img.shape[2] == 4 and img.stride(2) == 1 and img.stride(1) == 4
            surfs.append(RgbaSurface(img.data_ptr(), img.shape[1], img.shape[0], img.stride(0) * img.element_size()))
        else:
            assert img.ndim == 3 and img.shape[2] == 4 and img.strides[2] == img.itemsize and img.strides[1] == 4 * img.itemsize
            surfs.append(RgbaSurface(img.ctypes.data, img.shape[1], img.shape[0], img.strides[0]))
    return (RgbaSurface * max(1, len(surfs)))(*surfs)


def chain_bytes(fmt, images):
    """itwChainBytes: bytes a chain of images (arrays / tensors, or (height, width) tuples) encodes to; -1 on bad arguments."""
    arr = (RgbaSurface * max(1, len(images)))(*[RgbaSurface(None, s[1], s[0], 0) if isinstance(s, tuple) else _surfaces([s])[0] for s in images])
    return int(lib().itwChainBytes(C.cast(arr, C.c_void_p), len(images), DXGI_FORMAT[fmt]))


@_encodes
def compress_chain(fmt, images, profile=None, settings=None, progress=None, out=None, cmp_func=None, normal_ops=None):
    """A whole mip chain / cube map / array in one call (itwCompressImageChainEx; with `cmp_func` -- a CompressionFunc address, e.g.
    image_func(fmt, profile) -- itwCompressImageChain; with `normal_ops` -- a bit set of NORMAL_FLIP_X / NORMAL_FLIP_Y / NORMAL_NORMALIZE,
    see normal_ops() -- itwCompressNormalMapChain: the normal-map stages applied to every texel as it is gathered, sources untouched).  images: list of host numpy arrays or CUDA torch tensors (H, W, 4), uint8 or
    uint16 half bits for bc6h, all of one kind, any size >= 1; "etc1" takes settings=EtcSettings (default etc_profile("slow")).  `out` (optional): numpy array or CUDA uint8 tensor of chain_bytes() bytes;
    by default the images' kind.  Returns (ok, blocks): the images' blocks one after another, tightly packed (a DDS payload)."""
    import numpy as np
    fmt_key = fmt
    base = _base(fmt)
    for img in images:
        _check_texel_type(fmt, img)
    nbytes = sum(((img.shape[1] + 3) // 4) * ((img.shape[0] + 3) // 4) for img in images) * BYTES_PER_BLOCK[base]
    on_device = bool(images) and hasattr(images[0], "data_ptr")
    if out is None:
        if on_device:
            import torch
            out = torch.zeros(nbytes, dtype=torch.uint8, device=images[0].device)
        else:
            out = np.zeros(nbytes, dtype=np.uint8)
    if on_device or hasattr(out, "data_ptr"):
        import torch
        dev = images[0].device if on_device else out.device
        lib().itwSetStream(torch.cuda.current_stream(dev).cuda_stream)
    dst = out.data_ptr() if hasattr(out, "data_ptr") else out.ctypes.data
    arr = _surfaces(images)
    cb = PROGRESS_FUNC(progress) if progress else None
    cbp = C.cast(cb, C.c_void_p) if cb else None
    if cmp_func is not None:
        ok = lib().itwCompressImageChain(C.cast(arr, C.c_void_p), len(images), dst, cmp_func, DXGI_FORMAT[fmt_key], cbp, None)
    else:
        if settings is None and base == "bc7":
            settings = bc7_profile(profile or "slow")
        elif settings is None and base == "bc6h":
            settings = bc6h_profile(profile or "slow")
        elif settings is None and base == "etc1":
            settings = etc_profile(profile or "slow")
        sp = C.cast(C.byref(settings), C.c_void_p) if settings is not None else None
        if normal_ops is not None:
            ok = lib().itwCompressNormalMapChain(C.cast(arr, C.c_void_p), len(images), dst, DXGI_FORMAT[fmt_key], sp, int(normal_ops), cbp, None)
        else:
            ok = lib().itwCompressImageChainEx(C.cast(arr, C.c_void_p), len(images), dst, DXGI_FORMAT[fmt_key], sp, cbp, None)
    return bool(ok), out


NORMAL_FLIP_X, NORMAL_FLIP_Y, NORMAL_NORMALIZE = 1, 2, 4     # ITW_NORMAL_* (include/itw_dispatch.h)


def normal_ops(flip_x=False, flip_y=False, normalize=False):
    """The `ops` bit set of the normal-map calls: the flips apply first, then the normalise (IntelPlugin.cpp:2103-2106, 2149-2152)."""
    return (NORMAL_FLIP_X if flip_x else 0) | (NORMAL_FLIP_Y if flip_y else 0) | (NORMAL_NORMALIZE if normalize else 0)


# ITW_NORMAL_FROM_HEIGHT and ITW_HEIGHT_* (include/itw_dispatch.h, "height maps"): the further fields of the `ops` word
NORMAL_FROM_HEIGHT = 0x20
HEIGHT_CHANNEL = {"r": 1, "g": 2, "b": 3, "a": 4, "lum": 5}      # ITW_HEIGHT_CHANNEL(c) = c << 8; 0 is red too
HEIGHT_MIRROR_U, HEIGHT_MIRROR_V, HEIGHT_INVERT_SIGN, HEIGHT_OCCLUSION = 0x1000, 0x2000, 0x4000, 0x8000


def height_ops(channel="r", mirror="", invert=False, occlusion=False, amplitude=1.0, flip_x=False, flip_y=False, normalize=False):
    """The `ops` word that makes a normal-map call take height maps (DirectXTex's ComputeNormalMap first, then the flips and the normalise
    with their usual meaning).  channel: "r", "g", "b", "a" or "lum"; mirror: "", "u", "v" or "uv" (an axis not named wraps); amplitude: the
    bump strength, rounded to an IEEE half -- ValueError unless that half is finite and above 0.  height_amplitude() gives it back."""
    import numpy as np
    if channel not in HEIGHT_CHANNEL:
        raise ValueError(f"height channel {channel!r}: one of {sorted(HEIGHT_CHANNEL)}")
    if any(c not in "uv" for c in mirror):
        raise ValueError(f"mirror {mirror!r}: '', 'u', 'v' or 'uv'")
    with np.errstate(over="ignore"):
        bits = int(np.array(amplitude, dtype=np.float64).astype(np.float16).view(np.uint16))
    if not 0 < bits < 0x7C00:
        raise ValueError(f"amplitude {amplitude!r}: as an IEEE half it must be finite and above 0")
    return (normal_ops(flip_x, flip_y, normalize) | NORMAL_FROM_HEIGHT | (HEIGHT_CHANNEL[channel] << 8) | (HEIGHT_MIRROR_U if "u" in mirror else 0)
            | (HEIGHT_MIRROR_V if "v" in mirror else 0) | (HEIGHT_INVERT_SIGN if invert else 0) | (HEIGHT_OCCLUSION if occlusion else 0) | (bits << 16))


def height_amplitude(ops):
    """The amplitude an `ops` word of height_ops() carries, as a float."""
    import numpy as np
    return float(np.array((int(ops) >> 16) & 0x7FFF, dtype=np.uint16).view(np.float16))


def height_to_normal(images, ops, kind="biased", out=None):
    """Height maps to normal maps; `ops` is a word of height_ops().  images: one (H, W, 4) host numpy array / CUDA torch tensor or a list of
    them, all of one dtype.  kind "biased": itwPrepareNormalMapChain IN PLACE, uint8 (RGBA8 heights become a biased RGBA8 map) or 2-byte
    elements (RGBA16F half bits become an RGBA16F map); returns the images.  kind "snorm": itwQuantizeNormalMapChain, int8, float16 / half
    bits or float32 heights into RGBA8_SNORM targets (`out`, default new ones, never the sources); returns the targets."""
    if not int(ops) & NORMAL_FROM_HEIGHT:
        raise ValueError("height_to_normal: ops without NORMAL_FROM_HEIGHT (see height_ops())")
    if kind == "biased":
        return prepare_normal_map(images, ops=ops)
    if kind == "snorm":
        return quantize_normal_map(images, ops=ops, out=out)
    raise ValueError(f"kind {kind!r}: 'biased' or 'snorm'")


def prepare_normal_map(images, flip_x=False, flip_y=False, normalize=False, ops=None):
    """itwPrepareNormalMapChain: the plugin's normal-map flip / normalise IN PLACE over one image or a list of them (a mip chain), host numpy
    arrays or CUDA torch tensors (H, W, 4), all of one kind: uint8 (RGBA8) or 2-byte elements (RGBA16F half bits).  Device tensors: one
    launch, asynchronous on torch's current stream; numpy arrays: synchronous.  Returns the images."""
    single = hasattr(images, "shape")
    imgs = [images] if single else list(images)
    ops = normal_ops(flip_x, flip_y, normalize) if ops is None else int(ops)
    if imgs:
        es = imgs[0].element_size() if hasattr(imgs[0], "data_ptr") else imgs[0].itemsize
        assert es in (1, 2) and all((i.element_size() if hasattr(i, "data_ptr") else i.itemsize) == es for i in imgs), "uint8 or half texels, one kind per call"
        if hasattr(imgs[0], "data_ptr"):
            import torch
            lib().itwSetStream(torch.cuda.current_stream(imgs[0].device).cuda_stream)
        if lib().itwPrepareNormalMapChain(C.cast(_surfaces(imgs), C.c_void_p), len(imgs), 4 * es, ops) != 0:
            raise ValueError("itwPrepareNormalMapChain refused the call: " + (last_error() or "bad arguments"))
    return images


def compress_normal_map(img, flip_x=False, flip_y=False, normalize=False, ops=None, out=None):
    """itwCompressNormalMapBC5: BC5 of a normal map with the plugin's flip / normalise applied in the encoder's load (one kernel; `img` is
    not modified).  img: CUDA torch tensor (H, W, 4) uint8 (asynchronous on torch's current stream, returns a CUDA uint8 tensor) or a host
    numpy array (synchronous, returns a numpy array).  Same bytes as compress("bc5", prepared copy)."""
    ops = normal_ops(flip_x, flip_y, normalize) if ops is None else int(ops)
    h, w = img.shape[:2]
    nbytes = block_count("bc5", w, h) * 16
    if hasattr(img, "data_ptr"):
        import torch
        assert img.is_cuda and img.dim() == 3 and img.shape[2] == 4 and img.element_size() == 1 and img.stride(2) == 1 and img.stride(1) == 4
        if out is None:
            out = torch.empty(nbytes, dtype=torch.uint8, device=img.device)
        assert out.is_cuda and out.numel() >= nbytes and out.is_contiguous()
        with torch.cuda.device(img.device):
            lib().itwSetStream(torch.cuda.current_stream(img.device).cuda_stream)
            lib().itwCompressNormalMapBC5(C.byref(RgbaSurface(img.data_ptr(), w, h, img.stride(0))), out.data_ptr(), ops)
        return out
    import numpy as np
    assert img.ndim == 3 and img.shape[2] == 4 and img.dtype == np.uint8 and img.strides[2] == 1 and img.strides[1] == 4
    if out is None:
        out = np.empty(nbytes, dtype=np.uint8)
    lib().itwCompressNormalMapBC5(C.byref(RgbaSurface(img.ctypes.data, w, h, img.strides[0])), out.ctypes.data, ops)
    return out


def _signed_texel_bytes(img):
    """The texel kind of a signed normal source (include/itw_dispatch.h) from its dtype: int8 -> 4 (RGBA8_SNORM), float16 or any 2-byte
    element -> 8 (RGBA16F), float32 -> 16 (RGBA32F)."""
    name = str(img.dtype).replace("torch.", "")
    es = img.element_size() if hasattr(img, "data_ptr") else img.itemsize
    if name == "int8":
        return 4
    if es == 2:
        return 8
    if name == "float32":
        return 16
    raise TypeError(f"a signed normal source is int8, float16 (or 2-byte half bits) or float32, not {name}")


def _signed_surface(img):
    """RgbaSurface of an (H, W, 4) numpy array or torch tensor of any element size, texels contiguous."""
    if hasattr(img, "data_ptr"):
        assert img.dim() == 3 and img.shape[2] == 4 and img.stride(2) == 1 and img.stride(1) == 4
        return RgbaSurface(img.data_ptr(), img.shape[1], img.shape[0], img.stride(0) * img.element_size())
    assert img.ndim == 3 and img.shape[2] == 4 and img.strides[2] == img.itemsize and img.strides[1] == 4 * img.itemsize
    return RgbaSurface(img.ctypes.data, img.shape[1], img.shape[0], img.strides[0])


def quantize_normal_map(images, flip_x=False, flip_y=False, normalize=False, ops=None, out=None):
    """itwQuantizeNormalMapChain: one signed normal source or a list of them (a mip chain) -- (H, W, 4) numpy arrays or CUDA torch tensors of
    one dtype: int8, float16 / 2-byte half bits, or float32 -- to RGBA8_SNORM images (int8) of the same sizes: the flips, the normalise in
    fp32, and the quantisation with round to nearest even.  `out`: the targets (default: new ones; an int8 source may be its own target).
    Device tensors: one launch, asynchronous on torch's current stream; numpy arrays: synchronous.  Returns the target(s)."""
    single = hasattr(images, "shape")
    imgs = [images] if single else list(images)
    ops = normal_ops(flip_x, flip_y, normalize) if ops is None else int(ops)
    if not imgs:
        return []
    tb = _signed_texel_bytes(imgs[0])
    assert all(_signed_texel_bytes(i) == tb for i in imgs), "one texel kind per call"
    on_device = hasattr(imgs[0], "data_ptr")
    if out is None:
        if on_device:
            import torch
            outs = [torch.empty(tuple(i.shape), dtype=torch.int8, device=i.device) for i in imgs]
        else:
            import numpy as np
            outs = [np.empty(i.shape, dtype=np.int8) for i in imgs]
    else:
        outs = [out] if hasattr(out, "shape") else list(out)
    assert len(outs) == len(imgs)
    if on_device:
        import torch
        lib().itwSetStream(torch.cuda.current_stream(imgs[0].device).cuda_stream)
    src = (RgbaSurface * len(imgs))(*[_signed_surface(i) for i in imgs])
    dst = (RgbaSurface * len(outs))(*[_signed_surface(o) for o in outs])
    if lib().itwQuantizeNormalMapChain(C.cast(src, C.c_void_p), tb, C.cast(dst, C.c_void_p), len(imgs), ops) != 0:
        raise ValueError("itwQuantizeNormalMapChain refused the call: " + (last_error() or "bad arguments"))
    return outs[0] if single else outs


def compress_normal_map_snorm(img, flip_x=False, flip_y=False, normalize=False, ops=None, out=None):
    """itwCompressNormalMapBC5S: BC5_SNORM of a signed normal source -- (H, W, 4) int8, float16 / 2-byte half bits, or float32 -- with the
    flips, the fp32 normalise and the quantisation applied in the encoder's load (one kernel; `img` is not modified).  CUDA torch tensor:
    asynchronous on torch's current stream, returns a CUDA uint8 tensor; host numpy array: synchronous, returns a numpy array.  Same bytes
    as compress("bc5_snorm", quantize_normal_map(img, ...))."""
    ops = normal_ops(flip_x, flip_y, normalize) if ops is None else int(ops)
    tb = _signed_texel_bytes(img)
    h, w = img.shape[:2]
    nbytes = block_count("bc5", w, h) * 16
    surface = _signed_surface(img)
    if hasattr(img, "data_ptr"):
        import torch
        assert img.is_cuda
        if out is None:
            out = torch.empty(nbytes, dtype=torch.uint8, device=img.device)
        assert out.is_cuda and out.numel() >= nbytes and out.is_contiguous()
        with torch.cuda.device(img.device):
            lib().itwSetStream(torch.cuda.current_stream(img.device).cuda_stream)
            lib().itwCompressNormalMapBC5S(C.byref(surface), tb, out.data_ptr(), ops)
        return out
    import numpy as np
    if out is None:
        out = np.empty(nbytes, dtype=np.uint8)
    lib().itwCompressNormalMapBC5S(C.byref(surface), tb, out.ctypes.data, ops)
    return out


@_encodes
def compress_chain_normal_snorm(fmt, images, flip_x=False, flip_y=False, normalize=False, ops=None, progress=None, out=None):
    """itwCompressSignedNormalMapChain: a whole mip chain / cube map of signed normal sources -- (H, W, 4) numpy arrays or CUDA torch tensors
    of one dtype: int8, float16 / 2-byte half bits, or float32 -- to "bc4_snorm" or "bc5_snorm" in one call, every texel quantised as the
    chain's gather copies it.  Returns (ok, blocks) as compress_chain: same bytes as compress_chain(fmt, quantize_normal_map(images, ...))."""
    assert fmt in SIGNED_FORMATS, fmt
    images = list(images)
    ops = normal_ops(flip_x, flip_y, normalize) if ops is None else int(ops)
    tb = _signed_texel_bytes(images[0])
    assert all(_signed_texel_bytes(i) == tb for i in images), "one texel kind per call"
    nbytes = sum(block_count(fmt, i.shape[1], i.shape[0]) for i in images) * BYTES_PER_BLOCK[fmt]
    on_device = hasattr(images[0], "data_ptr")
    if out is None:
        if on_device:
            import torch
            out = torch.zeros(nbytes, dtype=torch.uint8, device=images[0].device)
        else:
            import numpy as np
            out = np.zeros(nbytes, dtype=np.uint8)
    if on_device or hasattr(out, "data_ptr"):
        import torch
        lib().itwSetStream(torch.cuda.current_stream(images[0].device if on_device else out.device).cuda_stream)
    dst = out.data_ptr() if hasattr(out, "data_ptr") else out.ctypes.data
    arr = (RgbaSurface * len(images))(*[_signed_surface(i) for i in images])
    cb = PROGRESS_FUNC(progress) if progress else None
    ok = lib().itwCompressSignedNormalMapChain(C.cast(arr, C.c_void_p), len(images), tb, dst, DXGI_FORMAT[fmt], ops, C.cast(cb, C.c_void_p) if cb else None, None)
    return bool(ok), out


@_encodes
def compress_mipped_normal_snorm(fmt, base_or_bases, levels=0, flip_x=False, flip_y=False, normalize=False, ops=None, progress=None, out=None):
    """itwCompressSignedNormalMapMipped: the signed normal-map save path from base images in one call -- one signed normal source or a list of
    equally sized ones (int8, float16 / 2-byte half bits, or float32) widened to RGBA16F with the flips, the mip chain, then
    compress_chain_normal_snorm with the normalise in fp32 on every level.  fmt "bc4_snorm" or "bc5_snorm"; levels == 0: the full chain.
    Returns (ok, blocks): the DDS payload, item-major then level."""
    assert fmt in SIGNED_FORMATS, fmt
    single = hasattr(base_or_bases, "shape")
    bases = [base_or_bases] if single else list(base_or_bases)
    ops = normal_ops(flip_x, flip_y, normalize) if ops is None else int(ops)
    tb = _signed_texel_bytes(bases[0])
    assert all(_signed_texel_bytes(b) == tb for b in bases), "one texel kind per call"
    h, w = bases[0].shape[:2]
    n = levels or mip_levels(w, h)
    nbytes = len(bases) * sum(block_count(fmt, max(1, w >> l), max(1, h >> l)) for l in range(n)) * BYTES_PER_BLOCK[fmt]
    on_device = hasattr(bases[0], "data_ptr")
    if out is None:
        if on_device:
            import torch
            out = torch.zeros(nbytes, dtype=torch.uint8, device=bases[0].device)
        else:
            import numpy as np
            out = np.zeros(nbytes, dtype=np.uint8)
    if on_device or hasattr(out, "data_ptr"):
        import torch
        lib().itwSetStream(torch.cuda.current_stream(bases[0].device if on_device else out.device).cuda_stream)
    dst = out.data_ptr() if hasattr(out, "data_ptr") else out.ctypes.data
    arr = (RgbaSurface * len(bases))(*[_signed_surface(b) for b in bases])
    cb = PROGRESS_FUNC(progress) if progress else None
    ok = lib().itwCompressSignedNormalMapMipped(C.cast(arr, C.c_void_p), len(bases), levels, tb, ops, dst, DXGI_FORMAT[fmt],
                                                C.cast(cb, C.c_void_p) if cb else None, None)
    return bool(ok), out


def cube_cross_faces(img):
    """itwCubeCrossFaces: the six faces (+X -X +Y -Y +Z -Z) of a horizontal (4 x 3 cells) or vertical (3 x 4, width < height) cube cross as
    VIEWS into `img` (numpy array or torch tensor (H, W, 4), uint8 or 2-byte half texels): no copy, no rotation.  The views feed
    compress_chain directly."""
    es = img.element_size() if hasattr(img, "data_ptr") else img.itemsize
    row = (img.stride(0) * es) if hasattr(img, "data_ptr") else img.strides[0]
    base = img.data_ptr() if hasattr(img, "data_ptr") else img.ctypes.data
    faces = (RgbaSurface * 6)()
    if lib().itwCubeCrossFaces(C.byref(RgbaSurface(base, img.shape[1], img.shape[0], row)), 4 * es, faces) != 0:
        raise ValueError(f"not a cube cross: {img.shape[1]} x {img.shape[0]}")
    views = []
    for f in faces:
        y, x = divmod(f.ptr - base, row)
        x //= 4 * es
        views.append(img[y:y + f.height, x:x + f.width])
    return views


MIP_PER_LEVEL = 1     # ITW_MIP_PER_LEVEL (include/itw_dispatch.h)
MIP_SRGB = 4          # ITW_MIP_SRGB: R, G, B of RGBA8 texels are sRGB coded and filtered in linear light
MIP_CUBIC = 0x10      # ITW_MIP_CUBIC: DirectXTex's cubic filter on every level
MIP_TRIANGLE = 0x20   # ITW_MIP_TRIANGLE: DirectXTex's triangle filter on every level
MIP_WRAP_U = 0x40     # ITW_MIP_WRAP_U / _V: the cubic and triangle filters address the source as a tiling texture along x / y
MIP_WRAP_V = 0x80


def mip_filter_flags(filter=None, wrap=""):
    """The ITW_MIP_* bits of filter=None | "cubic" | "triangle" and wrap="" | "u" | "v" | "uv"."""
    if filter not in (None, "cubic", "triangle"):
        raise ValueError(f"filter {filter!r} (None, 'cubic' or 'triangle')")
    if wrap not in ("", "u", "v", "uv"):
        raise ValueError(f"wrap {wrap!r} ('', 'u', 'v' or 'uv')")
    return {None: 0, "cubic": MIP_CUBIC, "triangle": MIP_TRIANGLE}[filter] | (MIP_WRAP_U if "u" in wrap else 0) | (MIP_WRAP_V if "v" in wrap else 0)


class MipAlpha(C.Structure):
    """struct itw_mip_alpha (include/itw_dispatch.h): the two rules for cut-out textures, both off by default.  16 bytes."""
    _fields_ = [("struct_size", C.c_uint32), ("weight_colour", C.c_uint32), ("coverage_ref", C.c_uint32), ("reserved", C.c_uint32)]

    def __init__(self, weight_colour=0, coverage_ref=0, struct_size=16, reserved=0):
        super().__init__(struct_size, int(weight_colour), int(coverage_ref), reserved)


class MipCoverage(C.Structure):
    """struct itw_mip_coverage: one report row per image of a chain, DDS order.  32 bytes."""
    _fields_ = [("texels", C.c_uint64), ("covered_plain", C.c_uint64), ("covered", C.c_uint64), ("threshold", C.c_uint32), ("reserved", C.c_uint32)]


def alpha_coverage(images, ref):
    """itwAlphaCoverage: the number of texels with alpha >= ref in each RGBA8 image of a list (numpy arrays or CUDA torch tensors (H, W, 4)
    uint8, any sizes, rows may be strided): a list of ints.  One image gives one int."""
    single = hasattr(images, "shape")
    imgs = [images] if single else list(images)
    if imgs and hasattr(imgs[0], "data_ptr"):
        import torch
        lib().itwSetStream(torch.cuda.current_stream(imgs[0].device).cuda_stream)
    out = (C.c_uint64 * max(1, len(imgs)))()
    if lib().itwAlphaCoverage(C.cast(_surfaces(imgs), C.c_void_p), len(imgs), int(ref), C.cast(out, C.c_void_p)) != 0:
        raise ValueError("itwAlphaCoverage refused the call: " + (last_error() or "bad arguments"))
    got = [int(out[i]) for i in range(len(imgs))]
    return got[0] if single else got


def srgb_to_linear(code):
    """itwSrgbToLinear: D[code] of the sRGB mip filter (include/itw_dispatch.h), the fp32 nearest to the linear light of sRGB code 0..255."""
    assert 0 <= int(code) <= 255
    return float(lib().itwSrgbToLinear(int(code)))


def linear_to_srgb(v):
    """itwLinearToSrgb: E(v) of the sRGB mip filter, the nearest sRGB code of the fp32 value v (host arithmetic, the kernels' definition)."""
    return int(lib().itwLinearToSrgb(float(v)))


def srgb_encode_device(values):
    """Test hook (itwTestSrgbEncode): the mip kernels' own E over a float32 CUDA tensor -> uint8 CUDA tensor of the same shape."""
    import torch
    assert values.is_cuda and values.dtype == torch.float32 and values.is_contiguous()
    out = torch.empty(values.shape, dtype=torch.uint8, device=values.device)
    L = test_lib()
    with torch.cuda.device(values.device):
        L.itwSetStream(torch.cuda.current_stream(values.device).cuda_stream)
        L.itwTestSrgbEncode(values.data_ptr(), out.data_ptr(), values.numel())
    e = L.itwLastError()
    if e:
        raise RuntimeError(e.decode())
    return out


def mip_levels(width, height):
    """itwMipLevels: the length of a full mip chain, 1 + floor(log2(max(width, height))); 0 for a size below 1."""
    return int(lib().itwMipLevels(width, height))


def mip_chain_layout(width, height, items=1, levels=0, pixel_size=4):
    """itwMipChainLayout without storage: (bytes, [(offset, width, height, stride)] in DDS order -- item-major, then level; levels == 0: the
    full chain).  Raises ValueError where the call returns -1."""
    n = int(lib().itwMipChainLayout(width, height, items, levels, pixel_size, None, None))
    if n < 0:
        raise ValueError(f"itwMipChainLayout refused {width} x {height}, {items} items, {levels} levels, pixel_size {pixel_size}")
    count = items * (levels or mip_levels(width, height))
    out = (RgbaSurface * max(1, count))()
    lib().itwMipChainLayout(width, height, items, levels, pixel_size, None, C.cast(out, C.c_void_p))
    return n, [(int(out[i].ptr or 0), out[i].width, out[i].height, out[i].stride) for i in range(count)]


def generate_mips(base_or_bases, levels=0, per_level=False, srgb=False, alpha_weight=False, alpha_coverage=0, report=False, filter=None, wrap=""):
    """itwGenerateMipChain: the mip levels of one base image or a list of equally sized ones (cube faces, array items): host numpy arrays or
    CUDA torch tensors (H, W, 4), uint8 (RGBA8) or 2-byte elements (RGBA16F half bits), all of one kind.  DirectXTex's box filter when width
    and height are powers of two, else its linear filter (include/itw_dispatch.h).  levels == 0: the full chain.  per_level forces one
    launch per level; srgb (uint8 only) filters R, G, B as sRGB codes in linear light (ITW_MIP_SRGB).  Returns the list of levels [base, level 1, ...] for one base, a list of such lists for a list; the bases themselves
    are level 0 and are not copied.  Device tensors: asynchronous on torch's current stream.  alpha_weight / alpha_coverage (uint8 only) are
    the rules of itwGenerateMipChainAlpha; with report=True the result is (levels, rows), rows the MipCoverage list in DDS order.
    filter="cubic" | "triangle" runs that DirectXTex filter on every level whatever the size (ITW_MIP_CUBIC / ITW_MIP_TRIANGLE), and
    wrap="u" | "v" | "uv" lets it address the source as a tiling texture; wrap changes nothing under the default filter."""
    single = hasattr(base_or_bases, "shape")
    bases = [base_or_bases] if single else list(base_or_bases)
    assert bases, "no base image"
    h, w = bases[0].shape[:2]
    n = levels or mip_levels(w, h)
    on_device = hasattr(bases[0], "data_ptr")
    es = bases[0].element_size() if on_device else bases[0].itemsize
    assert es in (1, 2), "uint8 or half texels"
    chains = []
    for b in bases:
        if on_device:
            import torch
            chains.append([b] + [torch.empty((max(1, h >> l), max(1, w >> l), 4), dtype=b.dtype, device=b.device) for l in range(1, n)])
        else:
            import numpy as np
            chains.append([b] + [np.empty((max(1, h >> l), max(1, w >> l), 4), dtype=b.dtype) for l in range(1, n)])
    rows = generate_mips_into(chains, per_level=per_level, srgb=srgb, alpha_weight=alpha_weight, alpha_coverage=alpha_coverage, report=report, filter=filter, wrap=wrap)
    if report:
        return (chains[0] if single else chains), rows[1]
    return chains[0] if single else chains


def generate_mips_into(chains, per_level=False, srgb=False, alpha_weight=False, alpha_coverage=0, report=False, filter=None, wrap=""):
    """itwGenerateMipChain over caller-made levels: `chains` is a list of items, each the list of its levels (level 0 filled in), which may
    be strided views of larger arrays / tensors.  Raises ValueError where the call returns -1.  alpha_weight, alpha_coverage or report make
    it itwGenerateMipChainAlpha (RGBA8); with report=True it returns (chains, [MipCoverage] in DDS order) and is synchronous.  filter and
    wrap as generate_mips takes them."""
    flat = [lv for ch in chains for lv in ch]
    on_device = hasattr(flat[0], "data_ptr")
    es = flat[0].element_size() if on_device else flat[0].itemsize
    if on_device:
        import torch
        lib().itwSetStream(torch.cuda.current_stream(flat[0].device).cuda_stream)
    flags = (MIP_PER_LEVEL if per_level else 0) | (MIP_SRGB if srgb else 0) | mip_filter_flags(filter, wrap)
    if alpha_weight or alpha_coverage or report:
        assert es == 1, "the alpha rules are for RGBA8 texels"
        opts = MipAlpha(1 if alpha_weight else 0, alpha_coverage)
        rows = (MipCoverage * len(flat))() if report else None
        if lib().itwGenerateMipChainAlpha(C.cast(_surfaces(flat), C.c_void_p), len(chains), len(chains[0]), flags, C.cast(C.byref(opts), C.c_void_p),
                                          C.cast(rows, C.c_void_p) if report else None) != 0:
            raise ValueError("itwGenerateMipChainAlpha refused the call: " + (last_error() or "bad arguments"))
        return (chains, list(rows)) if report else chains
    if lib().itwGenerateMipChain(C.cast(_surfaces(flat), C.c_void_p), len(chains), len(chains[0]), 4 * es, flags) != 0:
        raise ValueError("itwGenerateMipChain refused the call: " + (last_error() or "bad arguments"))
    return chains


MIP_RESIZE = 0x200    # ITW_MIP_RESIZE: the chain's level sizes are the caller's ("Mip chains: free sizes"); itwGenerateMipChain only
MIP_POINT = 0x400     # ITW_MIP_POINT / ITW_MIP_LINEAR: DirectX::Resize's point and linear filters by name (with ITW_MIP_RESIZE)
MIP_LINEAR = 0x800
MIP_MIRROR_U = 0x1000  # ITW_MIP_MIRROR_U / _V: the cubic filter mirrors the source about its edges along x / y (with ITW_MIP_RESIZE)
MIP_MIRROR_V = 0x2000


def resize_flags(filter=None, wrap="", mirror="", srgb=False):
    """The ITW_MIP_* bits of a free-size chain: ITW_MIP_RESIZE, filter=None | "point" | "linear" | "cubic" | "triangle", wrap and mirror
    each "" | "u" | "v" | "uv", and ITW_MIP_SRGB."""
    kinds = {None: 0, "point": MIP_POINT, "linear": MIP_LINEAR, "cubic": MIP_CUBIC, "triangle": MIP_TRIANGLE}
    if filter not in kinds:
        raise ValueError(f"filter {filter!r} (None, 'point', 'linear', 'cubic' or 'triangle')")
    for name, axes in (("wrap", wrap), ("mirror", mirror)):
        if axes not in ("", "u", "v", "uv"):
            raise ValueError(f"{name} {axes!r} ('', 'u', 'v' or 'uv')")
    return (MIP_RESIZE | kinds[filter] | (MIP_WRAP_U if "u" in wrap else 0) | (MIP_WRAP_V if "v" in wrap else 0)
            | (MIP_MIRROR_U if "u" in mirror else 0) | (MIP_MIRROR_V if "v" in mirror else 0) | (MIP_SRGB if srgb else 0))


def fit_size(w, h, rule, max_size=16384):
    """The size a w x h source is fitted to before its chain is made; host arithmetic only.  rule "pow2": texconv's FitPowerOf2 restated --
    the longer axis becomes the largest of max_size, max_size / 2, ... that is <= itself, the other the one of them whose ratio to it is
    nearest the source's aspect in fp32, the larger on a tie; "pow2_up": the next power of two per axis; "multiple4": each axis rounded up
    to a multiple of 4.  The last two are capped at max_size."""
    w, h = int(w), int(h)
    if w < 1 or h < 1 or max_size < 1:
        raise ValueError(f"fit_size: {w} x {h}, max_size {max_size}")
    if rule == "pow2_up":
        return tuple(min(max_size, 1 << (v - 1).bit_length()) for v in (w, h))
    if rule == "multiple4":
        return tuple(min(max_size, (v + 3) // 4 * 4) for v in (w, h))
    if rule != "pow2":
        raise ValueError(f"fit rule {rule!r} ('pow2', 'pow2_up' or 'multiple4')")
    import numpy as np
    f32 = np.float32
    aspect = f32(w) / f32(h)

    def below(v):                                    # max_size halved until it is <= v (1 at the least)
        x = max_size
        while x > 1 and x > v:
            x >>= 1
        return x

    def other(score_of):                             # max_size halved down to 1: the first strictly best score wins, so the larger on a tie
        best, best_score, x = None, None, max_size
        while x > 0:
            s = abs(score_of(x) - aspect)
            if best_score is None or s < best_score:
                best, best_score = x, s
            x >>= 1
        return best

    if w > h:
        nw = below(w)
        return nw, other(lambda y: f32(nw) / f32(y))
    nh = below(h)
    return other(lambda x: f32(x) / f32(nh)), nh


def _like(img, h, w):
    if hasattr(img, "data_ptr"):
        import torch
        return torch.empty((h, w, 4), dtype=img.dtype, device=img.device)
    import numpy as np
    return np.empty((h, w, 4), dtype=img.dtype)


def resize(image_or_images, size=None, fit=None, filter=None, wrap="", mirror="", srgb=False, out=None):
    """DirectX::Resize on the device (itwGenerateMipChain with ITW_MIP_RESIZE, a chain of two levels): one image or a list of equally sized
    ones -- host numpy arrays or CUDA torch tensors (H, W, 4), uint8 (RGBA8) or 2-byte elements (RGBA16F half bits), as generate_mips takes
    them -- to size=(w, h), or to fit_size(w, h, fit) with fit="pow2" | "pow2_up" | "multiple4".  filter=None is the reference's default (box
    at exactly 2:1, else linear); "point", "linear", "cubic", "triangle" name one.  wrap / mirror: "" | "u" | "v" | "uv"; mirror is read by
    the cubic filter, and linear with wrap on a growing axis is refused (include/itw_dispatch.h, "Mip chains: free sizes").  srgb (uint8
    only) filters R, G, B in linear light.  out: the target or list of targets, which may be strided views.  Returns the resized image, or
    the list of them.  Device tensors: asynchronous on torch's current stream."""
    single = hasattr(image_or_images, "shape")
    imgs = [image_or_images] if single else list(image_or_images)
    assert imgs, "no image"
    h, w = imgs[0].shape[:2]
    if (size is None) == (fit is None):
        raise ValueError("resize: give size=(w, h) or fit=, one of them")
    tw, th = fit_size(w, h, fit) if size is None else (int(size[0]), int(size[1]))
    outs = [_like(img, th, tw) for img in imgs] if out is None else ([out] if hasattr(out, "shape") else list(out))
    resize_chain_into([[img, o] for img, o in zip(imgs, outs)], filter=filter, wrap=wrap, mirror=mirror, srgb=srgb)
    return outs[0] if single else outs


_resize_images = resize       # (compress_mipped has a parameter of that name)


def resize_chain_into(chains, filter=None, wrap="", mirror="", srgb=False):
    """itwGenerateMipChain with ITW_MIP_RESIZE over caller-made levels: `chains` is a list of items, each the list of its 2 .. 32 levels
    (level 0 filled in), of any sizes -- level l alike across the items -- which may be strided views of larger arrays / tensors.  Level l
    is filtered from level l-1 as stored.  Raises ValueError where the call returns -1.  Options as resize takes them."""
    flat = [lv for ch in chains for lv in ch]
    on_device = hasattr(flat[0], "data_ptr")
    es = flat[0].element_size() if on_device else flat[0].itemsize
    assert es in (1, 2), "uint8 or half texels"
    if on_device:
        import torch
        lib().itwSetStream(torch.cuda.current_stream(flat[0].device).cuda_stream)
    if lib().itwGenerateMipChain(C.cast(_surfaces(flat), C.c_void_p), len(chains), len(chains[0]), 4 * es, resize_flags(filter, wrap, mirror, srgb)) != 0:
        raise ValueError("itwGenerateMipChain refused the call: " + (last_error() or "bad arguments"))
    return chains


@_encodes
def compress_mipped(fmt, base_or_bases, levels=0, profile=None, settings=None, normal_ops=0, progress=None, out=None, srgb=False,
                    alpha_weight=False, alpha_coverage=0, filter=None, wrap="", report=False, resize=None, resize_filter=None):
    """itwCompressImageMipped: the save path from base images in one call -- flips of `normal_ops` on level 0, the mip chain, the normalise on
    every level, then the chain encoder.  One base or a list of equally sized ones (numpy arrays or CUDA torch tensors, as compress_chain
    takes them); levels == 0: the full chain.  srgb: the chain's colour is filtered in linear light (itwCompressImageMippedEx with
    ITW_MIP_SRGB; the format name is not read as a request).  alpha_weight / alpha_coverage: the rules for cut-out textures
    (itwCompressImageMippedAlpha; no normal_ops with them).  filter / wrap: the chain's filter, as generate_mips takes them
    (itwCompressImageMippedEx with ITW_MIP_CUBIC / _TRIANGLE / _WRAP_*).  Returns (ok, blocks): the DDS payload, item-major then level.
    report=True (with the alpha rules): (ok, blocks, rows), rows the MipCoverage list of the same chain in DDS order -- the encode call has no
    report of its own, so the chain is generated once more for it (generate_mips with the same options, which is deterministic).
    resize=(w, h) | "pow2" | "pow2_up" | "multiple4" first fits every base to that size with resize(..., filter=resize_filter, wrap=wrap,
    srgb=srgb) and hands the result on.  The two stages are not fused: from host arrays the resized bases come back to the host and go up
    again with the save call, a second transfer; pass CUDA tensors to keep both stages resident."""
    import numpy as np
    single = hasattr(base_or_bases, "shape")
    bases = [base_or_bases] if single else list(base_or_bases)
    if resize is not None:
        bases = _resize_images(bases, fit=resize, filter=resize_filter, wrap=wrap, srgb=srgb) if isinstance(resize, str) \
            else _resize_images(bases, size=resize, filter=resize_filter, wrap=wrap, srgb=srgb)
    base = _base(fmt)
    for img in bases:
        _check_texel_type(fmt, img)
    h, w = bases[0].shape[:2]
    n = levels or mip_levels(w, h)
    nbytes = len(bases) * sum(((max(1, w >> l) + 3) // 4) * ((max(1, h >> l) + 3) // 4) for l in range(n)) * BYTES_PER_BLOCK[base]
    on_device = hasattr(bases[0], "data_ptr")
    if out is None:
        if on_device:
            import torch
            out = torch.zeros(nbytes, dtype=torch.uint8, device=bases[0].device)
        else:
            out = np.zeros(nbytes, dtype=np.uint8)
    if on_device or hasattr(out, "data_ptr"):
        import torch
        dev = bases[0].device if on_device else out.device
        lib().itwSetStream(torch.cuda.current_stream(dev).cuda_stream)
    dst = out.data_ptr() if hasattr(out, "data_ptr") else out.ctypes.data
    if settings is None and base == "bc7":
        settings = bc7_profile(profile or "slow")
    elif settings is None and base == "bc6h":
        settings = bc6h_profile(profile or "slow")
    elif settings is None and base == "etc1":
        settings = etc_profile(profile or "slow")
    sp = C.cast(C.byref(settings), C.c_void_p) if settings is not None else None
    cb = PROGRESS_FUNC(progress) if progress else None
    mip_flags = (MIP_SRGB if srgb else 0) | mip_filter_flags(filter, wrap)
    if alpha_weight or alpha_coverage:
        assert not normal_ops, "the alpha rules are for colour, not normal maps"
        opts = MipAlpha(1 if alpha_weight else 0, alpha_coverage)
        ok = lib().itwCompressImageMippedAlpha(C.cast(_surfaces(bases), C.c_void_p), len(bases), levels, mip_flags,
                                               C.cast(C.byref(opts), C.c_void_p), dst, DXGI_FORMAT[fmt], sp, C.cast(cb, C.c_void_p) if cb else None, None)
    elif mip_flags:
        ok = lib().itwCompressImageMippedEx(C.cast(_surfaces(bases), C.c_void_p), len(bases), levels, int(normal_ops), mip_flags, dst, DXGI_FORMAT[fmt],
                                            sp, C.cast(cb, C.c_void_p) if cb else None, None)
    else:
        ok = lib().itwCompressImageMipped(C.cast(_surfaces(bases), C.c_void_p), len(bases), levels, int(normal_ops), dst, DXGI_FORMAT[fmt],
                                          sp, C.cast(cb, C.c_void_p) if cb else None, None)
    if report:
        assert alpha_weight or alpha_coverage, "the report is the alpha rules'"
        rows = generate_mips(bases, levels=levels, srgb=srgb, alpha_weight=alpha_weight, alpha_coverage=alpha_coverage, report=True, filter=filter, wrap=wrap)[1]
        return bool(ok), out, rows
    return bool(ok), out


MIP_WRAP_W = 0x100    # ITW_MIP_WRAP_W: a volume's third wrap axis (beside MIP_VOLUME only)
MIP_VOLUME = 0x8000   # ITW_MIP_VOLUME: itwGenerateMipChain / itwCompressImageMippedEx take the image list as a volume's slices, `items` as its depth


def mip_filter_flags_3d(filter=None, wrap="", srgb=False, per_level=False):
    """The ITW_MIP_* bits of a volume call: filter=None | "point" | "linear" | "cubic" | "triangle", wrap a string of the letters u, v, w."""
    if filter not in (None, "point", "linear", "cubic", "triangle"):
        raise ValueError(f"filter {filter!r} (None, 'point', 'linear', 'cubic' or 'triangle')")
    if any(c not in "uvw" for c in wrap):
        raise ValueError(f"wrap {wrap!r} (letters of 'uvw')")
    return {None: 0, "point": MIP_POINT, "linear": MIP_LINEAR, "cubic": MIP_CUBIC, "triangle": MIP_TRIANGLE}[filter] \
        | (MIP_WRAP_U if "u" in wrap else 0) | (MIP_WRAP_V if "v" in wrap else 0) | (MIP_WRAP_W if "w" in wrap else 0) \
        | (MIP_SRGB if srgb else 0) | (MIP_PER_LEVEL if per_level else 0)


def mip_levels_3d(width, height, depth):
    """The length of a volume's full mip chain, 1 + floor(log2(max(width, height, depth))): itwMipLevels(max(width, height), depth); 0 for a
    size below 1."""
    return int(lib().itwMipLevels(max(width, height), depth)) if min(width, height, depth) >= 1 else 0


def mip_slices_3d(depth, levels):
    """The slices of a volume chain's first `levels` levels: the sum over l < levels of max(1, depth >> l)."""
    return sum(max(1, depth >> l) for l in range(levels))


def mip_chain_layout_3d(width, height, depth, levels=0, pixel_size=4):
    """A packed volume chain: (bytes, [(offset, width, height, stride)] of every slice in volume order -- level-major, tight rows, the slices
    one after another; levels == 0: the full chain).  Host arithmetic, as include/itw_dispatch.h ("Mip chains: volumes") states it.  Raises
    ValueError for a size below 1, levels above the full chain, a pixel_size other than 4 or 8 or a row above 2^31 - 1 bytes."""
    full = mip_levels_3d(width, height, depth)
    if full == 0 or levels < 0 or levels > full or pixel_size not in (4, 8) or width * pixel_size > 0x7fffffff:
        raise ValueError(f"no volume chain of {width} x {height} x {depth}, {levels} levels, pixel_size {pixel_size}")
    out, at = [], 0
    for l in range(levels or full):
        w, h = max(1, width >> l), max(1, height >> l)
        for _ in range(max(1, depth >> l)):
            out.append((at, w, h, w * pixel_size))
            at += w * h * pixel_size
    return at, out


def generate_mips_3d(volume, levels=0, filter=None, wrap="", srgb=False, per_level=False):
    """itwGenerateMipChain with ITW_MIP_VOLUME: the mip levels of a volume, a (D, H, W, 4) numpy array or CUDA torch tensor, uint8 (RGBA8) or 2-byte elements
    (RGBA16F half bits).  filter None: DirectXTex's 3D default, box when all three sizes are powers of two, else TRIANGLE (the 2D call's
    default is linear there); or "point", "linear", "cubic", "triangle".  wrap: letters of "uvw", read by cubic and triangle.  srgb (uint8
    only): ITW_MIP_SRGB.  levels == 0: the full chain.  Returns [volume, level 1, ...], each (d, h, w, 4); the volume itself is level 0 and
    is not copied.  Device tensors: asynchronous on torch's current stream."""
    d, h, w = volume.shape[:3]
    n = levels or mip_levels_3d(w, h, d)
    out = [volume]
    for l in range(1, n):
        shape = (max(1, d >> l), max(1, h >> l), max(1, w >> l), 4)
        if hasattr(volume, "data_ptr"):
            import torch
            out.append(torch.empty(shape, dtype=volume.dtype, device=volume.device))
        else:
            import numpy as np
            out.append(np.empty(shape, dtype=volume.dtype))
    return generate_mips_3d_into(out, filter=filter, wrap=wrap, srgb=srgb, per_level=per_level)


def generate_mips_3d_into(levels, filter=None, wrap="", srgb=False, per_level=False, flags=None):
    """itwGenerateMipChain with ITW_MIP_VOLUME over caller-made levels: `levels` is the list of a chain's levels, each a (d, h, w, 4) array / tensor or a
    list of d (h, w, 4) slices, which may be strided views of larger arrays / tensors; level 0 filled in.  `flags`: the raw bit set in
    place of the named options.  Raises ValueError where the call returns -1."""
    flat = [lv[z] for lv in levels for z in range(len(lv))]
    on_device = hasattr(flat[0], "data_ptr")
    es = flat[0].element_size() if on_device else flat[0].itemsize
    if on_device:
        import torch
        lib().itwSetStream(torch.cuda.current_stream(flat[0].device).cuda_stream)
    if flags is None:
        flags = mip_filter_flags_3d(filter, wrap, srgb, per_level)
    if lib().itwGenerateMipChain(C.cast(_surfaces(flat), C.c_void_p), len(levels[0]), len(levels), 4 * es, flags | MIP_VOLUME) != 0:
        raise ValueError("itwGenerateMipChain refused the volume: " + (last_error() or "bad arguments"))
    return levels


def compress_volume(fmt, volume, levels=0, profile=None, settings=None, filter=None, wrap="", srgb=False, progress=None, out=None):
    """itwCompressImageMippedEx with ITW_MIP_VOLUME: the volume save path in one call -- the base slices into level 0 of a device-side chain, the 3D mip chain
    (filter / wrap / srgb as generate_mips_3d takes them), then the chain encoder over the slice list.  volume: a (D, H, W, 4) numpy array
    or CUDA torch tensor, or a list of D (H, W, 4) slices.  Returns (ok, blocks): a volume .dds file's payload, level-major."""
    import numpy as np
    base = _base(fmt)
    slices = [volume[z] for z in range(len(volume))]
    for img in slices:
        _check_texel_type(fmt, img)
    d, (h, w) = len(slices), slices[0].shape[:2]
    n = levels or mip_levels_3d(w, h, d)
    nbytes = sum(max(1, d >> l) * ((max(1, w >> l) + 3) // 4) * ((max(1, h >> l) + 3) // 4) for l in range(n)) * BYTES_PER_BLOCK[base]
    on_device = hasattr(slices[0], "data_ptr")
    if out is None:
        if on_device:
            import torch
            out = torch.zeros(nbytes, dtype=torch.uint8, device=slices[0].device)
        else:
            out = np.zeros(nbytes, dtype=np.uint8)
    if on_device or hasattr(out, "data_ptr"):
        import torch
        dev = slices[0].device if on_device else out.device
        lib().itwSetStream(torch.cuda.current_stream(dev).cuda_stream)
    dst = out.data_ptr() if hasattr(out, "data_ptr") else out.ctypes.data
    if settings is None and base == "bc7":
        settings = bc7_profile(profile or "slow")
    elif settings is None and base == "bc6h":
        settings = bc6h_profile(profile or "slow")
    elif settings is None and base == "etc1":
        settings = etc_profile(profile or "slow")
    sp = C.cast(C.byref(settings), C.c_void_p) if settings is not None else None
    cb = PROGRESS_FUNC(progress) if progress else None
    ok = lib().itwCompressImageMippedEx(C.cast(_surfaces(slices), C.c_void_p), d, levels, 0, mip_filter_flags_3d(filter, wrap, srgb) | MIP_VOLUME, dst,
                                        DXGI_FORMAT[fmt], sp, C.cast(cb, C.c_void_p) if cb else None, None)
    return bool(ok), out


def mip_chain(img):
    """Test / tool content: the level list of a full mip chain of `img` (numpy (H, W, 4)), level l+1 of max(1, w >> 1) x max(1, h >> 1)
    from level l by a plain 2x2 mean (an odd last row / column is repeated).  uint8 levels average as integers, uint16 half bits as float16.
    Not a reproduction of any particular filter: GPU or DirectXTex mip generation is not part of this package."""
    import numpy as np
    levels = [np.ascontiguousarray(img)]
    half = img.dtype == np.uint16
    while levels[-1].shape[0] > 1 or levels[-1].shape[1] > 1:
        a = levels[-1]
        f = a.view(np.float16).astype(np.float32) if half else a.astype(np.float32)
        h, w = a.shape[:2]
        nh, nw = max(1, h >> 1), max(1, w >> 1)
        f = np.pad(f, ((0, 2 * nh - h if 2 * nh > h else 0), (0, 2 * nw - w if 2 * nw > w else 0), (0, 0)), mode="edge")[:2 * nh, :2 * nw]
        m = 0.25 * (f[0::2, 0::2] + f[1::2, 0::2] + f[0::2, 1::2] + f[1::2, 1::2])
        levels.append(np.ascontiguousarray(m.astype(np.float16).view(np.uint16) if half else np.floor(m + 0.5).astype(np.uint8)))
    return levels


def multigpu_sub_bands(fmt, width, height, ranks, L=None):
    """The partition a multi-GPU call uses (itw_multigpu.h): [(j, rank, first_texel_row, texel_rows, output_byte_offset)] for the
    K * ranks sub-bands, K = itwMultiGpuPieces(height, ranks); sub-band j belongs to rank j % ranks."""
    k = (L or lib()).itwMultiGpuPieces(height, ranks, 1 if fmt in KEEPS_PARTIAL_BLOCKS else 0)
    out = []
    for j in range(k * ranks):
        y0, rows, off = band_for_part(width, height, fmt, j, k * ranks)
        out.append((j, j % ranks, y0, rows, off))
    return out


@_encodes
def compress_image_multigpu(fmt, img, profile=None, ranks=0, out=None, bands=None, stats=None, L=None, interleave=None):
    """itwCompressImageMultiGPU[Ex]: img is a host numpy array or a CUDA torch tensor (H, W, 4); the block stream comes back in
    the same kind of container (or in `out`, which may be the other kind).  Synchronous.
    bands: optional list of CUDA tensors, K * ranks of them (K = 1..8, stated by the list's length): sub-band j = block rows
    itwBandForPart(j, K * ranks), resident on the device of rank j % ranks (multigpu_sub_bands() cuts a surface the way a call WITHOUT
    resident bands would); no scatter; `img` may then be a (height, width) tuple; goes through itwCompressImageMultiGPUBands, or -- K = 1 --
    through itwCompressImageMultiGPUEx.  interleave: sets K of calls without resident bands for the process first (1 = the reference's
    contiguous bands).  stats: an optional MultiGpuStats to fill (stats.as_dict()).  L: the library instance (default: the product;
    the failure-injection tests pass test_lib(), whose hook arms that instance)."""
    import numpy as np
    L = L or lib()
    if interleave is not None:
        L.itwMultiGpuSetInterleave(int(interleave))      # process-wide (itw_multigpu.h): K sub-bands per rank
    if bands is not None:
        import torch
        h, w = (img if isinstance(img, tuple) else img.shape[:2])
        if not ranks:
            ranks = len(bands)                           # (K = 1: one surface per rank)
        assert len(bands) % ranks == 0, f"{len(bands)} resident surfaces for {ranks} ranks"
        for b in bands:
            assert b.is_cuda and b.dim() == 3 and b.shape[2] == 4 and b.stride(2) == 1 and b.stride(1) == 4 and b.shape[1] == w
            torch.cuda.synchronize(b.device)
        arr = (RgbaSurface * len(bands))(*[RgbaSurface(b.data_ptr(), w, b.shape[0], b.stride(0) * b.element_size()) for b in bands])
        on_gpu, src_ptr, stride = True, None, w * 4 * bands[0].element_size()
        first_dev = bands[0].device
    else:
        h, w = img.shape[:2]
        arr = None
        on_gpu = not isinstance(img, np.ndarray)
        src_ptr, stride = (img.data_ptr(), img.stride(0) * img.element_size()) if on_gpu else (img.ctypes.data, img.strides[0])
        first_dev = img.device if on_gpu else None
    nbytes = block_count(fmt, w, h) * BYTES_PER_BLOCK[fmt]
    if out is None:
        if on_gpu:
            import torch
            out = torch.empty(nbytes, dtype=torch.uint8, device=first_dev)
        else:
            out = np.empty(nbytes, dtype=np.uint8)
    dst_ptr = out.ctypes.data if isinstance(out, np.ndarray) else out.data_ptr()
    if on_gpu and bands is None:
        import torch
        torch.cuda.synchronize(img.device)            # the rank threads read the texels on their own streams
    surf = RgbaSurface(src_ptr, w, h, stride)
    if bands is None and stats is None:
        ok = L.itwCompressImageMultiGPU(C.byref(surf), dst_ptr, image_func(fmt, profile, L), DXGI_FORMAT[fmt], ranks)
    elif bands is not None and len(bands) != ranks:
        ok = L.itwCompressImageMultiGPUBands(C.byref(surf), dst_ptr, image_func(fmt, profile, L), DXGI_FORMAT[fmt], ranks, arr, len(bands),
                                             C.byref(stats) if stats is not None else None)
    else:
        ok = L.itwCompressImageMultiGPUEx(C.byref(surf), dst_ptr, image_func(fmt, profile, L), DXGI_FORMAT[fmt], ranks, arr,
                                          C.byref(stats) if stats is not None else None)
    if not ok:
        e = L.itwLastError()
        raise RuntimeError((e.decode() if e else None) or "itwCompressImageMultiGPU failed")
    return out


def pad_to_multiple_of_4(img):
    """Host pre-pass (IntelPlugin.cpp:893-928) through the library; returns a new numpy array."""
    import numpy as np
    h, w = img.shape[:2]
    ps = 4 * img.itemsize
    surf = RgbaSurface(img.ctypes.data, w, h, img.strides[0])
    out = lib().itwPadToMultipleOf4(C.byref(surf), ps)
    n = out.height * out.stride
    arr = np.ctypeslib.as_array(C.cast(out.ptr, C.POINTER(C.c_uint8)), shape=(n,)).copy()
    lib().itwFreeSurface(C.byref(out))
    return arr.view(img.dtype).reshape(out.height, out.width, 4)


def dds_file(fmt_key, width, height, levels, mip_levels=1, cubemap=False, array_size=1):
    """DDS file bytes for block arrays `levels` (file order).  fmt_key: a key of DXGI_FORMAT."""
    import numpy as np
    d = DdsDesc(width, height, mip_levels, DXGI_FORMAT[fmt_key], 1 if cubemap else 0, array_size)
    total = lib().itwDdsFileBytes(C.byref(d))
    if not total:
        raise ValueError("unsupported DDS description")
    out = np.empty(total, dtype=np.uint8)
    keep = [np.ascontiguousarray(np.asarray(l, dtype=np.uint8)) for l in levels]
    ptrs = (C.c_void_p * len(keep))(*[k.ctypes.data for k in keep])
    n = lib().itwDdsWriteFile(C.byref(d), ptrs, len(keep), out.ctypes.data, out.size)
    if n != total:
        raise ValueError("itwDdsWriteFile failed (level count / sizes)")
    return out


def decode(fmt, blocks, width, height, want_modes=False):
    """GPU decode (itwDecodeBlocks).  blocks: uint8 numpy array or CUDA torch tensor of packed blocks.  Returns texels as
    (H, W, 4) uint8 -- uint16 half bit patterns for bc6h and bc6h_signed, int8 for the signed formats -- in the same kind of container, plus the per-block modes
    (int32) when asked."""
    import numpy as np
    key = {"bc1": 71, "bc3": 77, "bc7": 98, "bc6h": 95, "bc4": 80, "bc5": 83, "bc4_snorm": 81, "bc5_snorm": 84, "etc1": 0x8D64, "bc1a": 0x83F1, "bc1a_srgb": 0x8C4D, "bc2": 0x83F2, "bc2_srgb": 0x8C4E, "bc3_dxtex": 0x83F3, "bc3_dxtex_srgb": 0x8C4F, "bc6h_signed": 0x8E8E}[fmt]
    signed = fmt in SIGNED_FORMATS                      # RGBA8_SNORM texels: int8
    nb = block_count(fmt, width, height)
    half = _base(fmt) == "bc6h"                         # "bc6h", "bc6h_signed": RGBA16F bit patterns
    es = 2 if half else 1
    if isinstance(blocks, np.ndarray):
        blk = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1)
        out = np.empty((height, width, 4), dtype=np.uint16 if half else np.int8 if signed else np.uint8)
        modes = np.empty(nb, dtype=np.int32) if want_modes else None
        rc = lib().itwDecodeBlocks(key, blk.ctypes.data, width, height, out.ctypes.data, width * 4 * es,
                                   modes.ctypes.data if want_modes else None)
    else:
        import torch
        assert blocks.is_cuda and blocks.dtype == torch.uint8 and blocks.is_contiguous()
        out = torch.empty((height, width, 4), dtype=torch.int16 if half else torch.int8 if signed else torch.uint8, device=blocks.device)
        modes = torch.empty(nb, dtype=torch.int32, device=blocks.device) if want_modes else None
        with torch.cuda.device(blocks.device):
            lib().itwSetStream(torch.cuda.current_stream(blocks.device).cuda_stream)
            rc = lib().itwDecodeBlocks(key, blocks.data_ptr(), width, height, out.data_ptr(), width * 4 * es,
                                       modes.data_ptr() if want_modes else None)
    if rc != 0:
        raise ValueError("itwDecodeBlocks: unsupported format or size")
    return (out, modes) if want_modes else out


def _texel_dtype(fmt, torch_mod=None):
    """Element type of a decoded (H, W, 4) array / tensor: uint16 (torch: int16) half bits for bc6h, int8 for the signed formats, else uint8."""
    import numpy as np
    base = _base(fmt)
    if torch_mod is not None:
        return torch_mod.int16 if base == "bc6h" else torch_mod.int8 if fmt in SIGNED_FORMATS else torch_mod.uint8
    return np.uint16 if base == "bc6h" else np.int8 if fmt in SIGNED_FORMATS else np.uint8


def decode_chain(fmt, blocks, sizes_or_outs, want_modes=False, want_min_alpha=False):
    """itwDecodeChain: every image of the packed stream `blocks` (compress_chain's layout, a DDS payload) in one call, any size >= 1.
    blocks: uint8 numpy array (host pointers) or CUDA uint8 tensor (device pointers, torch's current stream, asynchronous).
    sizes_or_outs: a list of (h, w) to allocate, or a list of preallocated (H, W, 4) arrays / tensors of blocks' kind to fill; rows may
    be strided views into a larger allocation.  fmt: a key of DXGI_FORMAT.  Returns the list of texel arrays -- uint8, uint16 (torch:
    int16) half bits for bc6h, int8 for the signed formats -- followed by the modes (int32, one per block of the whole stream) and the
    per-image minimum alpha codes (uint32 numpy array, or a CUDA int32 tensor holding the same bits) when asked for."""
    import numpy as np
    base = _base(fmt)
    on_device = hasattr(blocks, "data_ptr")
    if on_device:
        import torch
        assert blocks.is_cuda and blocks.dtype == torch.uint8 and blocks.is_contiguous()
    else:
        blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1)
    outs = []
    for s in sizes_or_outs:
        if isinstance(s, tuple):
            h, w = s
            if on_device:
                outs.append(torch.empty((h, w, 4), dtype=_texel_dtype(fmt, torch), device=blocks.device))
            else:
                outs.append(np.empty((h, w, 4), dtype=_texel_dtype(fmt)))
        else:
            assert hasattr(s, "data_ptr") == on_device, "outputs and blocks must be of one kind"
            assert (s.element_size() if on_device else s.itemsize) == (2 if base == "bc6h" else 1), "texel type does not match the format"
            outs.append(s)
    n = len(outs)
    total = sum(((o.shape[1] + 3) // 4) * ((o.shape[0] + 3) // 4) for o in outs)
    assert (blocks.numel() if on_device else blocks.size) >= total * BYTES_PER_BLOCK[base]
    arr = _surfaces(outs)
    if on_device:
        modes = torch.empty(total, dtype=torch.int32, device=blocks.device) if want_modes else None
        amin = torch.empty(max(1, n), dtype=torch.int32, device=blocks.device) if want_min_alpha else None
        with torch.cuda.device(blocks.device):
            lib().itwSetStream(torch.cuda.current_stream(blocks.device).cuda_stream)
            rc = lib().itwDecodeChain(DXGI_FORMAT[fmt], blocks.data_ptr(), C.cast(arr, C.c_void_p), n,
                                      modes.data_ptr() if want_modes else None, amin.data_ptr() if want_min_alpha else None)
        if want_min_alpha:
            amin = amin[:n]
    else:
        modes = np.empty(total, dtype=np.int32) if want_modes else None
        amin = np.empty(n, dtype=np.uint32) if want_min_alpha else None
        rc = lib().itwDecodeChain(DXGI_FORMAT[fmt], blocks.ctypes.data, C.cast(arr, C.c_void_p), n,
                                  modes.ctypes.data if want_modes else None, amin.ctypes.data if want_min_alpha else None)
    if rc != 0:
        raise ValueError("itwDecodeChain: " + (last_error() or "bad arguments"))
    res = (outs,) + ((modes,) if want_modes else ()) + ((amin,) if want_min_alpha else ())
    return res[0] if len(res) == 1 else res


def decode_image(fmt, blocks, size_or_out, want_modes=False, want_min_alpha=False):
    """itwDecodeImage: decode_chain for one image of any size; size_or_out is (h, w) or a preallocated array / tensor.  Returns the
    texels, then modes and the image's minimum alpha code (an int for numpy, a one-element tensor on the device) when asked for."""
    import numpy as np
    base = _base(fmt)
    on_device = hasattr(blocks, "data_ptr")
    if isinstance(size_or_out, tuple):
        h, w = size_or_out
        if on_device:
            import torch
            out = torch.empty((h, w, 4), dtype=_texel_dtype(fmt, torch), device=blocks.device)
        else:
            out = np.empty((h, w, 4), dtype=_texel_dtype(fmt))
    else:
        out = size_or_out
        assert hasattr(out, "data_ptr") == on_device, "output and blocks must be of one kind"
    total = ((out.shape[1] + 3) // 4) * ((out.shape[0] + 3) // 4)
    surf = _surfaces([out])
    if on_device:
        import torch
        assert blocks.is_cuda and blocks.dtype == torch.uint8 and blocks.is_contiguous() and blocks.numel() >= total * BYTES_PER_BLOCK[base]
        modes = torch.empty(total, dtype=torch.int32, device=blocks.device) if want_modes else None
        amin = torch.empty(1, dtype=torch.int32, device=blocks.device) if want_min_alpha else None
        with torch.cuda.device(blocks.device):
            lib().itwSetStream(torch.cuda.current_stream(blocks.device).cuda_stream)
            rc = lib().itwDecodeImage(DXGI_FORMAT[fmt], blocks.data_ptr(), C.cast(surf, C.c_void_p),
                                      modes.data_ptr() if want_modes else None, amin.data_ptr() if want_min_alpha else None)
    else:
        blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1)
        assert blocks.size >= total * BYTES_PER_BLOCK[base]
        modes = np.empty(total, dtype=np.int32) if want_modes else None
        word = np.empty(1, dtype=np.uint32) if want_min_alpha else None
        rc = lib().itwDecodeImage(DXGI_FORMAT[fmt], blocks.ctypes.data, C.cast(surf, C.c_void_p),
                                  modes.ctypes.data if want_modes else None, word.ctypes.data if want_min_alpha else None)
        amin = int(word[0]) if want_min_alpha else None
    if rc != 0:
        raise ValueError("itwDecodeImage: " + (last_error() or "bad arguments"))
    res = (out,) + ((modes,) if want_modes else ()) + ((amin,) if want_min_alpha else ())
    return res[0] if len(res) == 1 else res


def preview_view(view_w, view_h, x=0, y=0, zoom=1.0, channels="rgb", matte=0, exposure=1.0):
    """A PreviewView.  channels: a string of the letters r, g, b, a (empty: RGB), or the option bits themselves."""
    options = channels if isinstance(channels, int) else sum({PREVIEW_CHANNEL[c.lower()] for c in channels})
    return PreviewView(view_w, view_h, x, y, zoom, options, matte, exposure, 0)


def _preview_call(call, source, view, out):
    """Runs call(view pointer, sizeof, out pointer, out stride) into `out` or a new (view_h, view_w, 3) uint8 array of `source`'s kind."""
    import numpy as np
    on_device = hasattr(source, "data_ptr")
    shape = (view.height, view.width, 3)
    if out is None:
        if on_device:
            import torch
            out = torch.empty(shape, dtype=torch.uint8, device=source.device)
        else:
            out = np.empty(shape, dtype=np.uint8)
    assert hasattr(out, "data_ptr") == on_device and tuple(out.shape) == shape, "the viewport is of the source's kind, (view_h, view_w, 3) uint8"
    if on_device:
        import torch
        assert out.dtype == torch.uint8 and out.stride(2) == 1 and out.stride(1) == 3
        with torch.cuda.device(source.device):
            lib().itwSetStream(torch.cuda.current_stream(source.device).cuda_stream)
            rc = call(C.byref(view), C.sizeof(view), out.data_ptr(), out.stride(0))
    else:
        assert out.dtype == np.uint8 and out.strides[2] == 1 and out.strides[1] == 3
        rc = call(C.byref(view), C.sizeof(view), out.ctypes.data, out.strides[0])
    return rc, out


def preview(fmt, blocks, width, height, view_w, view_h, x=0, y=0, zoom=1.0, channels="rgb", matte=0, exposure=1.0, out=None):
    """itwPreviewBlocks: a view_w x view_h RGB8 viewport of the width x height image whose blocks are `blocks` (uint8 numpy array: host
    pointers; CUDA uint8 tensor: device pointers, torch's current stream, asynchronous), decoded only where the viewport looks.  x, y: the
    viewport's offset in viewport pixels; zoom: source texels per viewport pixel; channels: letters of "rgba"; matte: 0x00BBGGRR; exposure:
    bc6h only.  The definition is in include/itw_decode.h.  Returns a (view_h, view_w, 3) uint8 array of blocks' kind (`out`, if given; its
    rows may be strided)."""
    import numpy as np
    base = _base(fmt)
    if hasattr(blocks, "data_ptr"):
        import torch
        assert blocks.is_cuda and blocks.dtype == torch.uint8 and blocks.is_contiguous()
        ptr, have = blocks.data_ptr(), blocks.numel()
    else:
        blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1)
        ptr, have = blocks.ctypes.data, blocks.size
    assert have >= ((width + 3) // 4) * ((height + 3) // 4) * BYTES_PER_BLOCK[base]
    view = preview_view(view_w, view_h, x, y, zoom, channels, matte, exposure)
    rc, out = _preview_call(lambda v, n, o, s: lib().itwPreviewBlocks(DXGI_FORMAT[fmt], ptr, width, height, v, n, o, s), blocks, view, out)
    if rc != 0:
        raise ValueError("itwPreviewBlocks: " + (last_error() or "bad arguments"))
    return out


def preview_surface(img, view_w, view_h, x=0, y=0, zoom=1.0, channels="rgb", matte=0, exposure=1.0, out=None):
    """itwPreviewSurface: preview() of an (H, W, 4) surface of texels -- uint8 RGBA8, or uint16 (torch: int16) RGBA16F bit patterns, to which
    `exposure` applies; numpy or CUDA tensor, rows may be strided."""
    assert img.ndim == 3 and img.shape[2] == 4
    texel = 4 * (img.element_size() if hasattr(img, "data_ptr") else img.itemsize)
    assert texel in (4, 8), "RGBA8 or RGBA16F"
    surf = _surfaces([img])
    view = preview_view(view_w, view_h, x, y, zoom, channels, matte, exposure)
    rc, out = _preview_call(lambda v, n, o, s: lib().itwPreviewSurface(surf, texel, v, n, o, s), img, view, out)
    if rc != 0:
        raise ValueError("itwPreviewSurface: " + (last_error() or "bad arguments"))
    return out


def dds_images(desc):
    """itwDdsImage over a DdsDesc: [(height, width, offset, bytes)] of every image in file order (array item, face, mip)."""
    out = []
    w, h, off = C.c_uint32(), C.c_uint32(), C.c_size_t()
    i = 0
    while True:
        n = lib().itwDdsImage(C.byref(desc), i, C.byref(w), C.byref(h), C.byref(off))
        if not n:
            return out
        out.append((int(h.value), int(w.value), int(off.value), int(n)))
        i += 1


def load_dds(data, device=None):
    """The load path: a .dds file's bytes (bytes / uint8 numpy array) -> (DdsDesc, [texel arrays in file order], [min alpha per image]).
    itwDdsReadHeader + itwDdsImage + one itwDecodeChain over the payload.  device None: numpy arrays through host pointers; a torch
    device: the payload is uploaded and the texels are CUDA tensors.  A BC6H_SF16 file (DXGI 96) is decoded by the signed reading, "bc6h_signed",
    whoever wrote it; the descriptor returned still says 96.  Raises ValueError for a header this library does not read and a file shorter
    than its header describes."""
    import numpy as np
    raw = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    desc = DdsDesc()
    first = lib().itwDdsReadHeader(raw.ctypes.data, raw.size, C.byref(desc))
    if not first:
        raise ValueError("not a BCn DDS file this library reads")
    if desc.is_cubemap == DDS_VOLUME:
        raise ValueError("a volume DDS file: its slices are level-major, load_dds_volume reads it")
    fmt = {v: k for k, v in DXGI_FORMAT.items()}[int(desc.dxgi_format)]
    if fmt == "bc6h_sf16":
        fmt = "bc6h_signed"                               # a file's label 96 is a descriptor code; the entry points read it under 0x8E8E
    images = dds_images(desc)
    end = images[-1][2] + images[-1][3] if images else 0
    if not images or images[0][2] != first or raw.size < end:
        raise ValueError(f"truncated DDS file: {raw.size} bytes, the header describes {end}")
    payload = raw[first:end]
    sizes = [(h, w) for h, w, _, _ in images]
    if device is None:
        texels, amin = decode_chain(fmt, payload, sizes, want_min_alpha=True)
        return desc, texels, [int(v) for v in amin]
    import torch
    texels, amin = decode_chain(fmt, torch.from_numpy(payload.copy()).to(device), sizes, want_min_alpha=True)
    return desc, texels, [int(v) & 0xFFFFFFFF for v in amin.cpu().tolist()]


def dds_volume_file(fmt_key, width, height, depth, slices, mip_levels=1):
    """Volume DDS file bytes for the block arrays `slices` in file order (level-major).  fmt_key: a key of DXGI_FORMAT."""
    import numpy as np
    d = DdsVolumeDesc(width, height, depth, mip_levels, DXGI_FORMAT[fmt_key])
    total = lib().itwDdsFileBytes(C.byref(d))
    if not total:
        raise ValueError("unsupported volume DDS description")
    out = np.empty(total, dtype=np.uint8)
    keep = [np.ascontiguousarray(np.asarray(s, dtype=np.uint8)) for s in slices]
    ptrs = (C.c_void_p * max(1, len(keep)))(*[k.ctypes.data for k in keep])
    n = lib().itwDdsWriteFile(C.byref(d), ptrs, len(keep), out.ctypes.data, out.size)
    if n != total:
        raise ValueError("itwDdsWriteFile failed (slice count / sizes)")
    return out


def dds_volume_images(desc):
    """itwDdsImage over a volume's DdsDesc: [(height, width, level, slice, offset, bytes)] of every slice in file order (level-major)."""
    assert desc.is_cubemap == DDS_VOLUME
    out, level, first = [], 0, 0
    for h, w, off, n in dds_images(desc):
        while len(out) - first >= max(1, desc.array_size >> level):
            first += max(1, desc.array_size >> level)
            level += 1
        out.append((h, w, level, len(out) - first, off, n))
    return out


def load_dds_volume(data, device=None):
    """The load path of a volume: a .dds file's bytes -> (DdsDesc, [texels per level as (d, h, w, 4)], [min alpha per slice]).
    itwDdsReadHeader + itwDdsImage + one itwDecodeChain over the payload, every level decoded into one array / tensor; the descriptor
    says is_cubemap = ITW_DDS_VOLUME and holds the depth in array_size.  device as load_dds takes it.  Raises ValueError for a header that
    is no volume this library reads and for a truncated file."""
    import numpy as np
    raw = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    desc = DdsDesc()
    first = lib().itwDdsReadHeader(raw.ctypes.data, raw.size, C.byref(desc))
    if not first or desc.is_cubemap != DDS_VOLUME:
        raise ValueError("not a BCn volume DDS file this library reads")
    fmt = {v: k for k, v in DXGI_FORMAT.items()}[int(desc.dxgi_format)]
    if fmt == "bc6h_sf16":
        fmt = "bc6h_signed"
    images = dds_volume_images(desc)
    end = images[-1][4] + images[-1][5] if images else 0
    if not images or images[0][4] != first or raw.size < end:
        raise ValueError(f"truncated DDS file: {raw.size} bytes, the header describes {end}")
    payload = raw[first:end]
    depth = desc.array_size
    if device is None:
        blocks = payload
        levels = [np.empty((max(1, depth >> l), max(1, desc.height >> l), max(1, desc.width >> l), 4), dtype=_texel_dtype(fmt)) for l in range(desc.mip_levels)]
    else:
        import torch
        blocks = torch.from_numpy(payload.copy()).to(device)
        levels = [torch.empty((max(1, depth >> l), max(1, desc.height >> l), max(1, desc.width >> l), 4), dtype=_texel_dtype(fmt, torch), device=device)
                  for l in range(desc.mip_levels)]
    _, amin = decode_chain(fmt, blocks, [levels[lv][sl] for _, _, lv, sl, _, _ in images], want_min_alpha=True)
    if device is None:
        return desc, levels, [int(v) for v in amin]
    return desc, levels, [int(v) & 0xFFFFFFFF for v in amin.cpu().tolist()]


def ktx_file(width, height, levels, mip_levels=1, cubemap=False):
    """KTX 1.1 file bytes for the ETC1 block arrays `levels` in KTX order: level major, then face (a DDS-ordered chain is face major)."""
    import numpy as np
    d = KtxDesc(width, height, mip_levels, DXGI_FORMAT["etc1"], 1 if cubemap else 0, 0)
    total = lib().itwKtxFileBytes(C.byref(d))
    if not total:
        raise ValueError("unsupported KTX description")
    out = np.empty(total, dtype=np.uint8)
    keep = [np.ascontiguousarray(np.asarray(l, dtype=np.uint8)) for l in levels]
    ptrs = (C.c_void_p * max(1, len(keep)))(*[k.ctypes.data for k in keep])
    sizes = [n for _, _, _, n in ktx_images(d)]
    if len(keep) != len(sizes) or any(k.size != n for k, n in zip(keep, sizes)):
        raise ValueError("ktx_file: level count / sizes do not match the description")
    n = lib().itwKtxWriteFile(C.byref(d), ptrs, len(keep), out.ctypes.data, out.size)
    if n != total:
        raise ValueError("itwKtxWriteFile failed")
    return out


def ktx_images(desc):
    """itwKtxImage over a KtxDesc: [(height, width, offset, bytes)] of every image in file order (level, then face)."""
    out = []
    w, h, off = C.c_uint32(), C.c_uint32(), C.c_size_t()
    i = 0
    while True:
        n = lib().itwKtxImage(C.byref(desc), i, C.byref(w), C.byref(h), C.byref(off))
        if not n:
            return out
        out.append((int(h.value), int(w.value), int(off.value), int(n)))
        i += 1


def load_ktx(data, device=None):
    """load_dds for a .ktx file's bytes: (KtxDesc, [texel arrays in file order: level, then face], [min alpha per image]).
    itwKtxReadHeader + itwKtxImage; the images are copied into one packed stream on the host (a size word sits in front of each level),
    then one itwDecodeChain.  device None: numpy arrays through host pointers; a torch device: CUDA tensors.  Raises ValueError for a
    file this library does not read (itw_dds.h), a truncated one included."""
    import numpy as np
    raw = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    desc = KtxDesc()
    if not lib().itwKtxReadHeader(raw.ctypes.data, raw.size, C.byref(desc)):
        raise ValueError("not an ETC1 KTX 1.1 file this library reads")
    images = ktx_images(desc)
    payload = np.concatenate([raw[off:off + n] for _, _, off, n in images])
    sizes = [(h, w) for h, w, _, _ in images]
    if device is None:
        texels, amin = decode_chain("etc1", payload, sizes, want_min_alpha=True)
        return desc, texels, [int(v) for v in amin]
    import torch
    texels, amin = decode_chain("etc1", torch.from_numpy(payload).to(device), sizes, want_min_alpha=True)
    return desc, texels, [int(v) & 0xFFFFFFFF for v in amin.cpu().tolist()]


def measure_async(fmt, blocks, img, stats_out, block_map=None):
    """The all-device form of itwMeasureBlocks: asynchronous on torch's current stream, nothing allocated, capturable into a graph.
    blocks: CUDA uint8 tensor; img: CUDA tensor (H, W, 4), rows may be strided; stats_out: CUDA uint8 tensor of sizeof(ErrorStats) bytes
    (read it back with stats_from_tensor); block_map (optional): CUDA int64 tensor, one element per block."""
    import torch
    _check_texel_type(fmt, img)
    assert blocks.is_cuda and blocks.dtype == torch.uint8 and blocks.is_contiguous()
    assert img.is_cuda and img.dim() == 3 and img.shape[2] == 4 and img.stride(2) == 1 and img.stride(1) == 4
    assert img.element_size() == (2 if fmt.split("_")[0] == "bc6h" else 1), "texel type does not match the format"
    assert stats_out.is_cuda and stats_out.dtype == torch.uint8 and stats_out.is_contiguous() and stats_out.numel() == C.sizeof(ErrorStats)
    h, w = img.shape[:2]
    nb = ((w + 3) // 4) * ((h + 3) // 4)
    assert blocks.numel() >= nb * BYTES_PER_BLOCK[_base(fmt)]
    assert block_map is None or (block_map.is_cuda and block_map.dtype == torch.int64 and block_map.is_contiguous() and block_map.numel() >= nb)
    with torch.cuda.device(img.device):
        lib().itwSetStream(torch.cuda.current_stream(img.device).cuda_stream)
        surf = RgbaSurface(img.data_ptr(), w, h, img.stride(0) * img.element_size())
        rc = lib().itwMeasureBlocks(DXGI_FORMAT[fmt], blocks.data_ptr(), C.byref(surf), stats_out.data_ptr(), C.sizeof(ErrorStats),
                                    block_map.data_ptr() if block_map is not None else None)
    if rc != 0:
        raise ValueError("itwMeasureBlocks: " + (last_error() or "bad arguments"))


def stats_from_tensor(t):
    """ErrorStats (or a list of them) from the bytes a device-side measurement wrote; synchronises with the tensor's stream through the copy."""
    raw = t.cpu().numpy().tobytes()
    n = C.sizeof(ErrorStats)
    out = [ErrorStats.from_buffer_copy(raw[i:i + n]) for i in range(0, len(raw), n)]
    return out[0] if len(out) == 1 and t.dim() == 1 else out


def measure(fmt, blocks, img, want_block_map=False):
    """itwMeasureBlocks: the integer error statistics of the stream `blocks` against its source `img`, decoded and compared on the GPU in
    one kernel.  numpy arrays (host pointers) or CUDA tensors (device pointers), as for decode(); img is (H, W, 4) uint8, or uint16 /
    int16 / float16 half bit patterns for bc6h, int8 for the signed formats, any H, W >= 1, and blocks holds ceil(W/4)*ceil(H/4) blocks.  fmt: a key of DXGI_FORMAT.
    Returns an ErrorStats; with want_block_map also the per-block sums (uint64 numpy array, or int64 CUDA tensor)."""
    import numpy as np
    base = _base(fmt)
    _check_texel_type(fmt, img)
    h, w = img.shape[:2]
    nb = ((w + 3) // 4) * ((h + 3) // 4)
    if isinstance(blocks, np.ndarray):
        assert isinstance(img, np.ndarray) and img.ndim == 3 and img.shape[2] == 4 and img.strides[2] == img.itemsize and img.strides[1] == 4 * img.itemsize
        assert img.itemsize == (2 if base == "bc6h" else 1), "texel type does not match the format"
        blk = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1)
        assert blk.size >= nb * BYTES_PER_BLOCK[base]
        st = ErrorStats()
        bmap = np.empty(nb, dtype=np.uint64) if want_block_map else None
        surf = RgbaSurface(img.ctypes.data, w, h, img.strides[0])
        rc = lib().itwMeasureBlocks(DXGI_FORMAT[fmt], blk.ctypes.data, C.byref(surf), C.addressof(st), C.sizeof(ErrorStats),
                                    bmap.ctypes.data if want_block_map else None)
        if rc != 0:
            raise ValueError("itwMeasureBlocks: " + (last_error() or "bad arguments"))
    else:
        import torch
        raw = torch.empty(C.sizeof(ErrorStats), dtype=torch.uint8, device=blocks.device)
        bmap = torch.empty(nb, dtype=torch.int64, device=blocks.device) if want_block_map else None
        measure_async(fmt, blocks, img, raw, bmap)
        st = stats_from_tensor(raw)
    return (st, bmap) if want_block_map else st


def measure_chain(fmt, blocks, levels):
    """itwMeasureChain: one ErrorStats per image of a chain encoded by compress_chain(fmt, levels): `blocks` is its packed stream.
    levels and blocks: numpy arrays, or CUDA tensors (then the call runs on torch's current stream and the result is copied back)."""
    import numpy as np
    base = _base(fmt)
    for lv in levels:
        _check_texel_type(fmt, lv)
    total = sum(((lv.shape[1] + 3) // 4) * ((lv.shape[0] + 3) // 4) for lv in levels) * BYTES_PER_BLOCK[base]
    arr = _surfaces(levels)
    n = len(levels)
    if isinstance(blocks, np.ndarray):
        blk = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1)
        assert blk.size >= total
        out = (ErrorStats * max(1, n))()
        rc = lib().itwMeasureChain(C.cast(arr, C.c_void_p), n, blk.ctypes.data, DXGI_FORMAT[fmt], C.addressof(out), C.sizeof(ErrorStats))
        res = [ErrorStats.from_buffer_copy(bytes(out[i])) for i in range(n)]
    else:
        import torch
        assert blocks.is_cuda and blocks.dtype == torch.uint8 and blocks.is_contiguous() and blocks.numel() >= total
        raw = torch.empty((max(1, n), C.sizeof(ErrorStats)), dtype=torch.uint8, device=blocks.device)
        with torch.cuda.device(blocks.device):
            lib().itwSetStream(torch.cuda.current_stream(blocks.device).cuda_stream)
            rc = lib().itwMeasureChain(C.cast(arr, C.c_void_p), n, blocks.data_ptr(), DXGI_FORMAT[fmt], raw.data_ptr(), C.sizeof(ErrorStats))
        res = stats_from_tensor(raw)[:n] if rc == 0 else None
    if rc != 0:
        raise ValueError("itwMeasureChain: " + (last_error() or "bad arguments"))
    return res


@_encodes
def compress_refined(fmt, img, first, refine, max_block_sse, channels=None, want_block_map=False, want_tier_map=False):
    """itwCompressImageRefined: encode `img` with the preset `first`, then encode with `refine` only the blocks whose error is above
    max_block_sse, keeping a second encoding only where it is strictly better (include/itw_dispatch.h).  fmt: 'bc7' / 'bc6h' (or another
    key of DXGI_FORMAT for them); first, refine: profile names or Bc7Settings / Bc6hSettings; img: numpy (H, W, 4) uint8 -- uint16 half
    bits for bc6h -- or a CUDA torch tensor of that shape (rows may be strided), H and W multiples of 4; channels: the channels the block
    error sums ('rgb', 'rgba', (0, 1), ...; default 'rgb': right for BC6H and for the BC7 RGB presets -- pass 'rgba' with the alpha presets).
    Synchronous.  Returns (blocks, RefineStats[, block_sse][, tier_map]) in the source's kind of container: uint8 / uint64 / uint8 numpy
    arrays, or uint8 / int64 / uint8 CUDA tensors."""
    import numpy as np
    base = fmt.split("_")[0]
    if base not in ("bc7", "bc6h"):
        raise ValueError(f"{fmt}: only bc7 and bc6h have presets to refine with")
    profile, settings_type = (bc7_profile, Bc7Settings) if base == "bc7" else (bc6h_profile, Bc6hSettings)
    s1 = first if isinstance(first, settings_type) else profile(first)
    s2 = refine if isinstance(refine, settings_type) else profile(refine)
    mask = _channel_mask("rgb" if channels is None else channels)
    h, w = img.shape[:2]
    nb = (w // 4) * (h // 4)
    st = RefineStats()
    L = lib()
    if isinstance(img, np.ndarray):
        assert img.ndim == 3 and img.shape[2] == 4 and img.strides[2] == img.itemsize and img.strides[1] == 4 * img.itemsize
        assert img.itemsize == (2 if base == "bc6h" else 1), "texel type does not match the format"
        out = np.empty(nb * 16, dtype=np.uint8)
        bmap = np.empty(nb, dtype=np.uint64) if want_block_map else None
        tmap = np.empty(nb, dtype=np.uint8) if want_tier_map else None
        surf = RgbaSurface(img.ctypes.data, w, h, img.strides[0])
        ptr = lambda a: a.ctypes.data if a is not None else None
        ok = L.itwCompressImageRefined(C.byref(surf), ptr(out), DXGI_FORMAT[fmt], C.addressof(s1), C.addressof(s2), mask, int(max_block_sse),
                                       C.addressof(st), C.sizeof(RefineStats), ptr(bmap), ptr(tmap))
    else:
        import torch
        assert img.is_cuda and img.dim() == 3 and img.shape[2] == 4 and img.stride(2) == 1 and img.stride(1) == 4
        assert img.element_size() == (2 if base == "bc6h" else 1), "texel type does not match the format"
        out = torch.empty(nb * 16, dtype=torch.uint8, device=img.device)
        bmap = torch.empty(nb, dtype=torch.int64, device=img.device) if want_block_map else None
        tmap = torch.empty(nb, dtype=torch.uint8, device=img.device) if want_tier_map else None
        ptr = lambda t: t.data_ptr() if t is not None else None
        with torch.cuda.device(img.device):
            L.itwSetStream(torch.cuda.current_stream(img.device).cuda_stream)
            surf = RgbaSurface(img.data_ptr(), w, h, img.stride(0) * img.element_size())
            ok = L.itwCompressImageRefined(C.byref(surf), ptr(out), DXGI_FORMAT[fmt], C.addressof(s1), C.addressof(s2), mask, int(max_block_sse),
                                           C.addressof(st), C.sizeof(RefineStats), ptr(bmap), ptr(tmap))
    if not ok:
        raise ValueError("itwCompressImageRefined: " + (last_error() or "failed"))
    return (out, st) + ((bmap,) if want_block_map else ()) + ((tmap,) if want_tier_map else ())


def psnr_to_total_sse(fmt, width, height, psnr_db, channels=None):
    """itwPsnrToTotalSse: the largest summed error at which a width x height image still has psnr_db over `channels` (default 'rgb');
    UINT64_MAX where itwStatsPsnr has no answer (bc6h, a non-finite psnr_db)."""
    return int(lib().itwPsnrToTotalSse(DXGI_FORMAT[fmt], int(width), int(height), _channel_mask("rgb" if channels is None else channels), float(psnr_db)))


@_encodes
def compress_refined_to(fmt, img, first, refine, max_listed=None, share=None, target_sse=None, target_psnr=None, channels=None,
                        want_block_map=False, want_tier_map=False):
    """itwCompressImageRefinedTo: compress_refined with the budget chosen on the device (include/itw_dispatch.h).  What to spend: max_listed,
    the most blocks the refine tier may encode, or share (0..1), which becomes max_listed = floor(share * blocks); neither: no cap.  What to
    reach: target_sse, the stream's summed block error, or target_psnr in dB over `channels` (bc7 only), which becomes
    itwPsnrToTotalSse's target; neither: one round that lists the max_listed worst blocks (policy A).  Everything else as compress_refined.
    Returns (blocks, RefineTargetStats[, block_sse][, tier_map])."""
    import numpy as np
    base = fmt.split("_")[0]
    if base not in ("bc7", "bc6h"):
        raise ValueError(f"{fmt}: only bc7 and bc6h have presets to refine with")
    if max_listed is not None and share is not None:
        raise ValueError("max_listed and share are two ways to say one thing: pass one")
    if target_sse is not None and target_psnr is not None:
        raise ValueError("target_sse and target_psnr are two ways to say one thing: pass one")
    profile, settings_type = (bc7_profile, Bc7Settings) if base == "bc7" else (bc6h_profile, Bc6hSettings)
    s1 = first if isinstance(first, settings_type) else profile(first)
    s2 = refine if isinstance(refine, settings_type) else profile(refine)
    mask = _channel_mask("rgb" if channels is None else channels)
    h, w = img.shape[:2]
    nb = (w // 4) * (h // 4)
    if share is not None:
        if not 0.0 <= share <= 1.0:
            raise ValueError(f"share {share}: a fraction of the blocks, 0..1")
        max_listed = int(share * nb)
    if target_psnr is not None:
        if base == "bc6h":
            raise ValueError("bc6h: no PSNR of half-float codes; pass target_sse")
        target_sse = psnr_to_total_sse(fmt, w, h, target_psnr, "rgb" if channels is None else channels)
    pol = RefinePolicy(UINT64_MAX if max_listed is None else int(max_listed), UINT64_MAX if target_sse is None else int(target_sse))
    st = RefineTargetStats()
    L = lib()
    if isinstance(img, np.ndarray):
        assert img.ndim == 3 and img.shape[2] == 4 and img.strides[2] == img.itemsize and img.strides[1] == 4 * img.itemsize
        assert img.itemsize == (2 if base == "bc6h" else 1), "texel type does not match the format"
        out = np.empty(nb * 16, dtype=np.uint8)
        bmap = np.empty(nb, dtype=np.uint64) if want_block_map else None
        tmap = np.empty(nb, dtype=np.uint8) if want_tier_map else None
        surf = RgbaSurface(img.ctypes.data, w, h, img.strides[0])
        ptr = lambda a: a.ctypes.data if a is not None else None
        ok = L.itwCompressImageRefinedTo(C.byref(surf), ptr(out), DXGI_FORMAT[fmt], C.addressof(s1), C.addressof(s2), mask, C.addressof(pol),
                                         C.sizeof(RefinePolicy), C.addressof(st), C.sizeof(RefineTargetStats), ptr(bmap), ptr(tmap))
    else:
        import torch
        assert img.is_cuda and img.dim() == 3 and img.shape[2] == 4 and img.stride(2) == 1 and img.stride(1) == 4
        assert img.element_size() == (2 if base == "bc6h" else 1), "texel type does not match the format"
        out = torch.empty(nb * 16, dtype=torch.uint8, device=img.device)
        bmap = torch.empty(nb, dtype=torch.int64, device=img.device) if want_block_map else None
        tmap = torch.empty(nb, dtype=torch.uint8, device=img.device) if want_tier_map else None
        ptr = lambda t: t.data_ptr() if t is not None else None
        with torch.cuda.device(img.device):
            L.itwSetStream(torch.cuda.current_stream(img.device).cuda_stream)
            surf = RgbaSurface(img.data_ptr(), w, h, img.stride(0) * img.element_size())
            ok = L.itwCompressImageRefinedTo(C.byref(surf), ptr(out), DXGI_FORMAT[fmt], C.addressof(s1), C.addressof(s2), mask, C.addressof(pol),
                                             C.sizeof(RefinePolicy), C.addressof(st), C.sizeof(RefineTargetStats), ptr(bmap), ptr(tmap))
    if not ok:
        raise ValueError("itwCompressImageRefinedTo: " + (last_error() or "failed"))
    return (out, st) + ((bmap,) if want_block_map else ()) + ((tmap,) if want_tier_map else ())


def chain_psnr_to_total_sse(fmt, images, psnr_db, channels=None):
    """itwChainPsnrToTotalSse: psnr_to_total_sse over all texels of a chain (arrays / tensors, or (height, width) tuples)."""
    arr = (RgbaSurface * max(1, len(images)))(*[RgbaSurface(None, s[1], s[0], 0) if isinstance(s, tuple) else _surfaces([s])[0] for s in images])
    return int(lib().itwChainPsnrToTotalSse(C.cast(arr, C.c_void_p), len(images), DXGI_FORMAT[fmt], _channel_mask("rgb" if channels is None else channels),
                                            float(psnr_db)))


def _chain_refined(name, fmt, images, first, refine, channels, want_block_map, want_tier_map, want_image_stats, stats, middle):
    """The two chain calls: `middle(L)` gives the arguments between channel_mask and stats."""
    import numpy as np
    base = fmt.split("_")[0]
    profile, settings_type = (bc7_profile, Bc7Settings) if base == "bc7" else (bc6h_profile, Bc6hSettings)
    s1 = first if isinstance(first, settings_type) else profile(first)
    s2 = refine if isinstance(refine, settings_type) else profile(refine)
    mask = _channel_mask("rgb" if channels is None else channels)
    for img in images:
        _check_texel_type(fmt, img)
    n = len(images)
    nb = sum(((img.shape[1] + 3) // 4) * ((img.shape[0] + 3) // 4) for img in images)
    arr = _surfaces(images)
    L = lib()
    call = getattr(L, name)
    if not (images and hasattr(images[0], "data_ptr")):
        out = np.empty(nb * 16, dtype=np.uint8)
        bmap = np.empty(nb, dtype=np.uint64) if want_block_map else None
        tmap = np.empty(nb, dtype=np.uint8) if want_tier_map else None
        per = (RefineStats * max(1, n))() if want_image_stats else None
        ptr = lambda a: a.ctypes.data if a is not None else None
        ok = call(C.cast(arr, C.c_void_p), n, ptr(out), DXGI_FORMAT[fmt], C.addressof(s1), C.addressof(s2), mask, *middle,
                  C.addressof(stats), C.sizeof(stats), C.addressof(per) if per is not None else None, ptr(bmap), ptr(tmap))
        per = [RefineStats.from_buffer_copy(bytes(per[i])) for i in range(n)] if want_image_stats else None
    else:
        import torch
        dev = images[0].device
        out = torch.empty(nb * 16, dtype=torch.uint8, device=dev)
        bmap = torch.empty(nb, dtype=torch.int64, device=dev) if want_block_map else None
        tmap = torch.empty(nb, dtype=torch.uint8, device=dev) if want_tier_map else None
        raw = torch.empty((max(1, n), C.sizeof(RefineStats) // 8), dtype=torch.int64, device=dev) if want_image_stats else None
        ptr = lambda t: t.data_ptr() if t is not None else None
        with torch.cuda.device(dev):
            L.itwSetStream(torch.cuda.current_stream(dev).cuda_stream)
            ok = call(C.cast(arr, C.c_void_p), n, ptr(out), DXGI_FORMAT[fmt], C.addressof(s1), C.addressof(s2), mask, *middle,
                      C.addressof(stats), C.sizeof(stats), ptr(raw), ptr(bmap), ptr(tmap))
        per = None
        if want_image_stats and ok:
            host = raw.cpu().numpy()
            per = [RefineStats.from_buffer_copy(host[i].tobytes()) for i in range(n)]
    if not ok:
        raise ValueError(name + ": " + (last_error() or "failed"))
    return (out, stats) + ((bmap,) if want_block_map else ()) + ((tmap,) if want_tier_map else ()) + ((per,) if want_image_stats else ())


@_encodes
def compress_chain_refined(fmt, images, first, refine, max_block_sse, channels=None, want_block_map=False, want_tier_map=False,
                           want_image_stats=False):
    """itwCompressImageChainRefined: compress_refined over a whole chain as one population of blocks (include/itw_dispatch.h).  images: list
    of numpy arrays or of CUDA tensors (H, W, 4), any size >= 1, as compress_chain takes them; the block error leaves the padding of
    partial blocks out.  Returns (blocks, RefineStats[, block_sse][, tier_map][, image_stats]): blocks, block_sse and tier_map over the
    chain's concatenated block list (compress_chain's layout), image_stats a list of one RefineStats per image."""
    base = fmt.split("_")[0]
    if base not in ("bc7", "bc6h"):
        raise ValueError(f"{fmt}: only bc7 and bc6h have presets to refine with")
    return _chain_refined("itwCompressImageChainRefined", fmt, images, first, refine, channels, want_block_map, want_tier_map, want_image_stats,
                          RefineStats(), (int(max_block_sse),))


@_encodes
def compress_chain_refined_to(fmt, images, first, refine, max_listed=None, share=None, target_sse=None, target_psnr=None, channels=None,
                              want_block_map=False, want_tier_map=False, want_image_stats=False):
    """itwCompressImageChainRefinedTo: compress_refined_to over a whole chain as one population: share is of the chain's blocks, target_psnr
    (bc7 only) goes through itwChainPsnrToTotalSse.  Returns (blocks, RefineTargetStats[, block_sse][, tier_map][, image_stats])."""
    base = fmt.split("_")[0]
    if base not in ("bc7", "bc6h"):
        raise ValueError(f"{fmt}: only bc7 and bc6h have presets to refine with")
    if max_listed is not None and share is not None:
        raise ValueError("max_listed and share are two ways to say one thing: pass one")
    if target_sse is not None and target_psnr is not None:
        raise ValueError("target_sse and target_psnr are two ways to say one thing: pass one")
    if share is not None:
        if not 0.0 <= share <= 1.0:
            raise ValueError(f"share {share}: a fraction of the blocks, 0..1")
        max_listed = int(share * sum(((img.shape[1] + 3) // 4) * ((img.shape[0] + 3) // 4) for img in images))
    if target_psnr is not None:
        if base == "bc6h":
            raise ValueError("bc6h: no PSNR of half-float codes; pass target_sse")
        target_sse = chain_psnr_to_total_sse(fmt, [(img.shape[0], img.shape[1]) for img in images], target_psnr, "rgb" if channels is None else channels)
    pol = RefinePolicy(UINT64_MAX if max_listed is None else int(max_listed), UINT64_MAX if target_sse is None else int(target_sse))
    return _chain_refined("itwCompressImageChainRefinedTo", fmt, images, first, refine, channels, want_block_map, want_tier_map, want_image_stats,
                          RefineTargetStats(), (C.addressof(pol), C.sizeof(RefinePolicy)))
