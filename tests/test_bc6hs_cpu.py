"""CPU, the signed reading of BC6H (ITW_FORMAT_BC6H_SIGNED, include/itw_dispatch.h / itw_decode.h): the numpy model (tests/_dxtex_bc6hs.py)
and the decoder's own text run on the host (tools/bc6hs_host_check.cpp over csrc/decode_core.hpp) against the reference's recorded
D3DXDecodeBC6HS output (tests/golden/bc6hs_ref.npz), bit for bit; what the recording contains; where the signed and the unsigned reading
must agree; what the entry points refuse before any device work; the symbol list; the load path's truncation error; and the built kernels'
resources."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import _dxtex_bc6hs as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "intel-texture-works-plugin_amd", "csrc", "build")


@pytest.fixture(scope="module")
def sets():
    return H.recorded_sets()


@pytest.fixture(scope="module")
def models(sets):
    return {name: H.model(blocks) for name, blocks, _ in sets}


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("bc6hs_host_check")
    exe = os.path.join(str(d), "bc6hs_host_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "tools", "host_stub"), os.path.join(ROOT, "tools", "bc6hs_host_check.cpp"), "-o", exe],
                   check=True, capture_output=True)
    return exe, str(d)


def run_host_check(host_check, blocks, signed=True):
    exe, d = host_check
    np.ascontiguousarray(blocks, dtype=np.uint8).tofile(os.path.join(d, "blocks.bin"))
    subprocess.run([exe, os.path.join(d, "blocks.bin"), os.path.join(d, "texels.bin"), os.path.join(d, "modes.bin"), "1" if signed else "0"], check=True)
    return np.fromfile(os.path.join(d, "texels.bin"), dtype=np.uint16).reshape(-1, 16, 4), np.fromfile(os.path.join(d, "modes.bin"), dtype=np.int32)


def test_the_recording_holds_the_four_sets(sets):
    assert [name for name, _, _ in sets] == ["sweep", "constructed", "random", "encoded"]
    assert [blocks.size // 16 for _, blocks, _ in sets] == [8192, 14 * 36 * 3, 4096, 256]
    for name, blocks, rgb in sets:
        assert rgb.dtype == np.uint16 and rgb.shape == (blocks.size // 16, 16, 3), name
    g = H.golden()
    assert np.array_equal(g["constructed_blocks"], H.constructed_blocks()) and np.array_equal(g["random_blocks"], H.random_blocks())
    assert os.path.getsize(H.GOLDEN) < 1 << 20


def test_model_equals_every_recorded_texel(sets, models):
    for name, blocks, rgb in sets:
        got = models[name]["texels"]
        bad = np.nonzero((got[..., :3] != rgb).any(axis=(1, 2)))[0]
        assert bad.size == 0, (name, bad[:8], got[bad[:1]], rgb[bad[:1]])
        assert (got[..., 3] == 0x3C00).all()


def test_the_reference_still_gives_the_recording(sets):
    for name, blocks, rgb in sets:
        got = H.reference_decode(blocks)                        # (skips where the reference library is absent and cannot be built)
        assert np.array_equal(got[..., :3], rgb) and (got[..., 3] == 0x3C00).all(), name


def test_census_of_the_recording(sets, models):
    """The comparisons cannot pass by never entering a case: every mode and every reserved prefix, both signs in every channel, endpoints
    that saturate, transforms that wrap, and -Inf -- which the 16-bit mode produces from an endpoint of -32768 -- all occur; +Inf and NaN
    patterns never do."""
    rgb = np.concatenate([r for _, _, r in sets])
    modes = np.concatenate([models[n]["modes"] for n, _, _ in sets])
    flag = {k: np.concatenate([models[n][k] for n, _, _ in sets]) for k in ("saturated", "wrapped", "negative", "neg_inf")}
    print({k: int(v.sum()) for k, v in flag.items()}, np.bincount(modes + 1))
    assert set(np.unique(modes)) == set(range(-1, 14))
    sweep = sets[0][1].reshape(-1, 16)
    reserved = sweep[models["sweep"]["modes"] == -1, 0] & 31
    assert set(reserved) == {0x13, 0x17, 0x1B, 0x1F}
    assert (rgb[models_reserved(models, sets)] == 0).all()
    for ch in range(3):
        c = rgb[..., ch]
        assert ((c & 0x8000) != 0).any() and (((c & 0x8000) == 0) & (c != 0)).any(), ch
    assert flag["saturated"].any() and flag["wrapped"].any() and flag["negative"].any()
    # saturation reaches the texels: an endpoint of +-0x7FFF finishes as (0x7FFF * 31) >> 5 = 0x7BFF under either sign
    assert (rgb == 0x7BFF).any() and (rgb == 0xFBFF).any()
    assert int((rgb == 0xFC00).sum()) >= 1 and flag["neg_inf"].any()
    assert (modes[flag["neg_inf"]] == 13).all()                 # only the 16-bit mode has an endpoint of -32768
    assert not (rgb == 0x7C00).any() and not ((rgb & 0x7FFF) > 0x7C00).any()
    assert not (rgb == 0x8000).any()                            # zero is never -0


def models_reserved(models, sets):
    return np.concatenate([models[n]["modes"] for n, _, _ in sets]) == -1


def test_the_kernels_text_on_the_host_equals_the_recording(sets, models, host_check):
    for name, blocks, rgb in sets:
        texels, modes = run_host_check(host_check, blocks)
        bad = np.nonzero((texels[..., :3] != rgb).any(axis=(1, 2)))[0]
        assert bad.size == 0, (name, bad[:8])
        assert (texels[..., 3] == 0x3C00).all() and np.array_equal(modes, models[name]["modes"]), name


def test_where_the_two_readings_agree(sets, models, host_check, oracle):
    """The exact relation.  For an endpoint c with 0 < c < (1 << (bits - 1)) - 1 the signed ((c << 15) + 0x4000) >> (bits - 1) and the
    unsigned ((c << 16) + 0x8000) >> bits are the same integer, 0 stays 0, and a sign-extension of a field whose top bit is clear changes
    nothing; so on a block all of whose endpoints are non-negative and unsaturated (after the transform) both readings interpolate the
    same x, and finish it as (x * 31) >> 5 and (x * 31) >> 6: unsigned == signed >> 1, texel for texel (the unsigned clamp at 0x7BFF is
    out of reach: x < 0x8000).  Everywhere else nothing is promised."""
    total = 0
    for name, blocks, rgb in sets:
        m = models[name]
        plain = ~m["negative"] & ~m["saturated"] & (m["modes"] >= 0)
        nb = blocks.size // 16
        unsigned, umodes = oracle.decode("bc6h", blocks, 4 * nb, 4)      # the from-spec C decoder, one row of blocks
        unsigned = H.blocks_of(unsigned)
        assert np.array_equal(unsigned[plain], rgb[plain] >> 1), name
        assert np.array_equal(umodes, m["modes"])
        ours, _ = run_host_check(host_check, blocks, signed=False)            # the unsigned instantiation of the same text did not move
        assert np.array_equal(ours[..., :3], unsigned), name
        total += int(plain.sum())
        if name == "sweep":                                                # and the readings do differ where a sign bit is set
            differs = (unsigned != rgb).any(axis=(1, 2))
            assert differs[m["negative"]].mean() > 0.9 and not differs[plain & (rgb == 0).all(axis=(1, 2))].any()
    print("plain blocks", total)
    assert total >= 1000


def test_format_table_facts(itw):
    L = itw.lib()
    assert itw.DXGI_FORMAT["bc6h_signed"] == H.FORMAT == 0x8E8E and itw.DXGI_FORMAT["bc6h_sf16"] == 96
    assert L.GetBytesPerBlock(H.FORMAT) == 16
    assert itw.abi._texel_dtype("bc6h_signed") == np.uint16 and itw.abi._base("bc6h_signed") == "bc6h"
    # not a descriptor code
    d = itw.DdsDesc(16, 16, 1, H.FORMAT, 0, 1)
    assert L.itwDdsFileBytes(C.byref(d)) == 0 and L.itwDdsHeaderBytes(C.byref(d)) == 0
    w, h, off = C.c_uint32(), C.c_uint32(), C.c_size_t()
    assert L.itwDdsImage(C.byref(d), 0, C.byref(w), C.byref(h), C.byref(off)) == 0
    buf = np.zeros(256, dtype=np.uint8)
    assert L.itwDdsWriteHeader(C.byref(d), buf.ctypes.data, buf.size) == 0 and not buf.any()
    d96 = itw.DdsDesc(16, 16, 1, 96, 0, 1)
    assert L.itwDdsFileBytes(C.byref(d96)) == 128 + 20 + 256               # 96 stays a descriptor code
    es = itw.ErrorStats()
    es.dxgi_format, es.width, es.height = H.FORMAT, 4, 4
    es.sse[0] = 5
    assert np.isnan(L.itwStatsPsnr(C.byref(es), 1))
    with pytest.raises(ValueError):
        es.psnr()


def test_every_python_compress_refuses_the_key(itw):
    img = np.zeros((8, 8, 4), dtype=np.uint16)
    calls = {"compress_numpy": lambda: itw.compress_numpy("bc6h_signed", img), "compress": lambda: itw.compress("bc6h_signed", img),
             "compress_image": lambda: itw.compress_image("bc6h_signed", img, "fast"), "compress_chain": lambda: itw.compress_chain("bc6h_signed", [img], "fast"),
             "compress_mipped": lambda: itw.compress_mipped("bc6h_signed", img), "compress_image_multigpu": lambda: itw.compress_image_multigpu("bc6h_signed", img),
             "compress_refined": lambda: itw.compress_refined("bc6h_signed", img, "fast", "slow", 0),
             "compress_refined_to": lambda: itw.compress_refined_to("bc6h_signed", img, "fast", "slow", max_listed=1),
             "compress_chain_refined": lambda: itw.compress_chain_refined("bc6h_signed", [img], "fast", "slow", 0),
             "compress_chain_refined_to": lambda: itw.compress_chain_refined_to("bc6h_signed", [img], "fast", "slow", max_listed=1)}
    for name, call in calls.items():
        with pytest.raises(ValueError, match="no signed BC6H encoder"):
            call()


def test_the_product_library_still_lists_its_132_names(itw):
    out = subprocess.run(["nm", "-D", "--defined-only", itw.lib_path()], check=True, capture_output=True, text=True).stdout
    names = sorted(l.split()[2] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T")
    assert names == sorted(itw.EXPORTED_SYMBOLS) and len(names) == 132


def test_bad_calls_return_before_any_device_use():
    """Every entry point that encodes refuses 0x8E8E with a message that says there is no signed encoder, and writes nothing; the decode
    calls keep for it the size and stride rules they have for 95; 96 keeps its refusals.  Run in a fresh interpreter: the error mode is
    process-wide."""
    code = r"""
import ctypes as C, sys, numpy as np
sys.path.insert(0, %r)
import itw_amd
L = itw_amd.lib()
itw_amd.set_error_mode(itw_amd.ON_ERROR_RETURN)
S = 0x8E8E
img = np.zeros((8, 8, 4), dtype=np.uint16)
out = np.full(4096, 0xA5, dtype=np.uint8)
def arr(*s):
    return C.cast((itw_amd.RgbaSurface * len(s))(*s), C.c_void_p)
good = itw_amd.RgbaSurface(img.ctypes.data, 8, 8, 64)
s6 = itw_amd.bc6h_profile("fast")
sp = C.cast(C.byref(s6), C.c_void_p)
rs, ts = itw_amd.RefineStats(), itw_amd.RefineTargetStats()
pol = itw_amd.RefinePolicy(1, 2 ** 64 - 1)
called = []
fn = itw_amd.abi.COMPRESSION_FUNC(lambda s, o: called.append(1))
fp = C.cast(fn, C.c_void_p)
a = itw_amd.MipAlpha(0, 128)
calls = {
    "sliced_ex": lambda: L.itwCompressImageSlicedEx(C.byref(good), out.ctypes.data, 32, S, sp, 0, None, None),
    "sliced": lambda: L.itwCompressImageSliced(C.byref(good), out.ctypes.data, 32, fp, S, False, 0, None, None),
    "sliced_mt": lambda: L.itwCompressImageSliced(C.byref(good), out.ctypes.data, 32, fp, S, True, 0, None, None),
    "image_st": lambda: L.CompressImageST(C.byref(good), out.ctypes.data, fp, S),
    "image_mt": lambda: L.CompressImageMT(C.byref(good), out.ctypes.data, fp, S),
    "chain_ex": lambda: L.itwCompressImageChainEx(arr(good), 1, out.ctypes.data, S, sp, None, None),
    "chain": lambda: L.itwCompressImageChain(arr(good), 1, out.ctypes.data, fp, S, None, None),
    "mipped": lambda: L.itwCompressImageMipped(arr(good), 1, 0, 0, out.ctypes.data, S, sp, None, None),
    "mipped_ex": lambda: L.itwCompressImageMippedEx(arr(good), 1, 0, 0, 0, out.ctypes.data, S, sp, None, None),
    "mipped_alpha": lambda: L.itwCompressImageMippedAlpha(arr(good), 1, 0, 0, C.cast(C.byref(a), C.c_void_p), out.ctypes.data, S, sp, None, None),
    "refined": lambda: L.itwCompressImageRefined(C.byref(good), out.ctypes.data, S, sp, sp, 7, 0, C.addressof(rs), C.sizeof(rs), None, None),
    "refined_to": lambda: L.itwCompressImageRefinedTo(C.byref(good), out.ctypes.data, S, sp, sp, 7, C.addressof(pol), C.sizeof(pol), C.addressof(ts), C.sizeof(ts), None, None),
    "chain_refined": lambda: L.itwCompressImageChainRefined(arr(good), 1, out.ctypes.data, S, sp, sp, 7, 0, C.addressof(rs), C.sizeof(rs), None, None, None),
    "chain_refined_to": lambda: L.itwCompressImageChainRefinedTo(arr(good), 1, out.ctypes.data, S, sp, sp, 7, C.addressof(pol), C.sizeof(pol), C.addressof(ts), C.sizeof(ts), None, None, None),
    "normal_chain": lambda: L.itwCompressNormalMapChain(arr(good), 1, out.ctypes.data, S, sp, 4, None, None),
    "normal_chain_0": lambda: L.itwCompressNormalMapChain(arr(good), 1, out.ctypes.data, S, sp, 0, None, None),
    "signed_normal_chain": lambda: L.itwCompressSignedNormalMapChain(arr(good), 1, 8, out.ctypes.data, S, 0, None, None),
    "signed_normal_mipped": lambda: L.itwCompressSignedNormalMapMipped(arr(good), 1, 0, 8, 0, out.ctypes.data, S, None, None),
    "multigpu": lambda: L.itwCompressImageMultiGPU(C.byref(good), out.ctypes.data, fp, S, 1),
}
n = 0
for name, call in calls.items():
    L.itwClearError()
    ok = call()
    err = itw_amd.last_error()
    assert ok is False and err, (name, ok, err)
    if not name.startswith("signed_normal"):                 # (those two take 81 / 84 and say so)
        assert "no signed BC6H encoder" in err, (name, err)
    n += 1
assert not called and (out == 0xA5).all()
assert L.itwChainBytes(arr(good), 1, S) == -1 and L.itwChainBytes(arr(good), 1, 96) == 4 * 16
assert L.itwSliceWindow(S, 4096, 4096, 0x40000) == 0 and L.itwSliceWindowFor(S, sp, 4096, 4096, 0x40000) == 0
assert L.itwSliceWindow(96, 4096, 4096, 0x40000) == L.itwSliceWindow(95, 4096, 4096, 0x40000) > 0
kd = itw_amd.KtxDesc(8, 8, 1, S, 0, 0)
assert L.itwKtxFileBytes(C.byref(kd)) == 0 and L.itwKtxHeaderBytes(C.byref(kd)) == 0
# the decode calls: the rules of 95
blocks = np.zeros(16 * 16, dtype=np.uint8)
tex = np.full((16, 16, 4), 0xA5A5, dtype=np.uint16)
def surf(w, h, stride, ptr=tex.ctypes.data):
    return itw_amd.RgbaSurface(ptr, w, h, stride)
for code_ in (S, 95):
    for w, h, stride in ((6, 8, 64), (8, 7, 64), (0, 8, 64), (8, 8, 60), (8, 8, 66), (8, 8, 2 ** 31)):
        assert L.itwDecodeBlocks(code_, blocks.ctypes.data, w, h, tex.ctypes.data, stride, None) == -1, (code_, w, h, stride)
    for s in (surf(0, 8, 64), surf(8, 0, 64), surf(8, 8, 56), surf(7, 5, 58), surf(8, 8, 64, None)):
        assert L.itwDecodeImage(code_, blocks.ctypes.data, C.byref(s), None, None) == -1
        assert L.itwDecodeChain(code_, blocks.ctypes.data, arr(surf(8, 8, 64), s), 2, None, None) == -1
    assert L.itwDecodeChain(code_, blocks.ctypes.data, arr(surf(8, 8, 64)), -1, None, None) == -1
    assert L.itwDecodeChain(code_, blocks.ctypes.data, arr(surf(8, 8, 64)), 0, None, None) == 0
    assert L.itwDecodeChain(code_, None, arr(surf(8, 8, 64)), 1, None, None) == -1
    es = itw_amd.ErrorStats()
    assert L.itwMeasureBlocks(code_, blocks.ctypes.data, C.byref(surf(8, 8, 56)), C.byref(es), C.sizeof(es), None) == -1
    assert L.itwMeasureBlocks(code_, blocks.ctypes.data, C.byref(surf(8, 8, 64)), C.byref(es), C.sizeof(es) - 8, None) == -1
    v = itw_amd.preview_view(4, 4)
    rgb = np.full(48, 0xA5, dtype=np.uint8)
    assert L.itwPreviewBlocks(code_, blocks.ctypes.data, 0, 8, C.byref(v), C.sizeof(v), rgb.ctypes.data, 12) == -1
    assert L.itwPreviewBlocks(code_, blocks.ctypes.data, 8, 8, C.byref(v), C.sizeof(v), rgb.ctypes.data, 11) == -1
    assert (rgb == 0xA5).all()
# 96 keeps its refusals
s = surf(8, 8, 64)
assert L.itwDecodeImage(96, blocks.ctypes.data, C.byref(s), None, None) == -1 and L.itwDecodeChain(96, blocks.ctypes.data, arr(s), 1, None, None) == -1
v = itw_amd.preview_view(4, 4)
rgb = np.full(48, 0xA5, dtype=np.uint8)
assert L.itwPreviewBlocks(96, blocks.ctypes.data, 8, 8, C.byref(v), C.sizeof(v), rgb.ctypes.data, 12) == -1
assert (tex == 0xA5A5).all()
print("rejected", n)
""" % os.path.join(ROOT, "intel-texture-works-plugin_amd")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip() == "rejected 19"


def dx10_header(width, height, dxgi, mips=1, cube=False):
    """A DDS header with the DX10 extension, field by field (DDS.h): 4 + 124 + 20 bytes."""
    linear = ((width + 3) // 4) * ((height + 3) // 4) * 16
    flags = 0x1 | 0x2 | 0x4 | 0x1000 | 0x80000 | (0x20000 if mips > 1 else 0)
    caps = 0x1000 | (0x400008 if mips > 1 else 0) | (0x8 if cube else 0)
    pf = struct.pack("<II4sIIIII", 32, 0x4, b"DX10", 0, 0, 0, 0, 0)
    head = struct.pack("<4sIIIIIII44s", b"DDS ", 124, flags, height, width, linear, 0, mips, b"\0" * 44) + pf + \
        struct.pack("<IIIII", caps, 0xFE00 if cube else 0, 0, 0, 0)
    return head + struct.pack("<IIIII", dxgi, 3, 0x4 if cube else 0, 1, 0)


def test_load_dds_on_a_truncated_sf16_file_raises_the_truncation_error(itw):
    head = dx10_header(16, 12, 96)
    assert len(head) == 148
    d = itw.DdsDesc()
    raw = np.frombuffer(head + bytes(12 * 16), dtype=np.uint8)
    assert itw.lib().itwDdsReadHeader(raw.ctypes.data, raw.size, C.byref(d)) == 148 and d.dxgi_format == 96      # the header keeps saying 96
    with pytest.raises(ValueError, match="truncated DDS file") as e:
        itw.load_dds(head + bytes(12 * 16 - 1))
    assert "not decoded" not in str(e.value)
    assert "not decoded" not in itw.load_dds.__doc__ and "bc6h_signed" in itw.load_dds.__doc__


# What the build gave (gfx950, -O3): name -> (VGPRs, LDS bytes); scratch and spills are 0 in all of them.  DESIGN.md 3.16 records the
# same figures beside the unsigned instantiations' from the same build (80 / 89, 95, 123 / 90).
RESOURCES = {"decode_chain.o": {"decode_chain_kernel<22, true>": (79, 0), "decode_chain_kernel<22, false>": (88, 0)},
             "measure.o": {"measure_kernel<22>": (103, 304)},
             "preview.o": {"preview_bc6hs_kernel<true>": (120, 33 * 9 * 96), "preview_bc6hs_kernel<false>": (94, 0)}}


def test_resources_of_the_new_instantiations():
    for obj, want in RESOURCES.items():
        path = os.path.join(BUILD, obj)
        if not os.path.exists(path):
            pytest.skip("csrc/build/ is not populated: run __graft_entry__.build() first")
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), path], check=True, capture_output=True, text=True).stdout
        seen = {}
        for line in out.splitlines():
            m = re.match(r"(?:void )?itw::(\S+<[^>]*>)\s+vgpr\s+(\d+) agpr\s+(\d+) .*?scratch\s+(\d+) B\s+lds\s+(\d+) B\s+spills v(\d+) s(\d+)", line)
            if m:
                seen[m.group(1)] = tuple(int(m.group(i)) for i in range(2, 8))
        for name, (regs, lds_want) in want.items():
            assert name in seen, (obj, name, sorted(seen))
            vgpr, agpr, scratch, lds, vspill, sspill = seen[name]
            print(name, seen[name], "waves per SIMD", 512 // (-(-(vgpr + agpr) // 8) * 8))
            assert (scratch, vspill, sspill) == (0, 0, 0), (name, seen[name])
            assert lds == lds_want and vgpr + agpr == regs, (name, seen[name])
