"""BC4_SNORM / BC5_SNORM without a GPU: the model the GPU tests use is pinned to the reference's own decoder (tests/_dxtex_snorm.py binds
D3DXDecodeBC4S of oracle/_ref/libdxtex_bc_ref.so), the assumption the encoder's index escape rests on is counted, and the host-only
layers -- DDS headers, argument checks, the binding's dtype rule -- are exercised for the two formats (DXGI 81 / 84)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _dxtex_snorm as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def levels():
    return ref.levels()


@pytest.fixture(scope="module")
def closest(levels):
    return ref.closest_table(levels)


def test_numpy_levels_are_the_reference_decoders(levels):
    """All 65 536 endpoint pairs x 8 indices, bit for bit: -128 read as -127, the raw bytes choosing the form, levels 6 / 7 = -1 / 1."""
    assert np.array_equal(ref.model_levels().view(np.uint32), levels.view(np.uint32))


def test_integer_decode_rule_is_the_rounded_reference(levels):
    want = np.rint(127.0 * levels.astype(np.float64)).astype(np.int32)
    rule = ref.integer_levels()
    assert np.array_equal(rule, want)
    assert np.abs(127.0 * levels.astype(np.float64) - rule).max() < 0.43       # no value near a tie: the rounding is not in doubt
    assert rule.min() == -127 and rule.max() == 127                            # never -128


def test_index_function_has_more_than_eight_runs_for_thirty_equal_endpoint_pairs_only(closest, levels):
    """What the kernel's run table with its escape assumes (csrc/bc4_bc5.hip).  F is the first strict minimum over the reference's levels."""
    t = ref.to_float(np.arange(256).astype(np.uint8).view(np.int8))
    rng = np.random.default_rng(81)
    for r0, r1, v in rng.integers(0, 256, size=(2000, 3)):                     # F itself, case by case, as FindClosestSNORM is written
        best, delta = 0, np.float32(100000.0)
        for k in range(8):
            d = np.abs(levels[r0, r1, k] - t[v])
            if d < delta:
                best, delta = k, d
        assert closest[r0, r1, v] == best
    runs = ref.run_counts(closest)
    many = np.argwhere(runs > 8)
    assert len(many) == 30 and (runs <= 8).sum() == 65506
    assert all(a == b for a, b in many)
    assert runs[runs > 8].min() == 12 and runs.max() == 19
    ends = sorted(int(np.uint8(a).view(np.int8)) for a, _ in many)
    half = [7, 13, 14, 26, 27, 28, 29, 52, 53, 54, 55, 56, 57, 58, 59]
    assert ends == sorted([-e for e in half] + half)


# ---- DDS ----------------------------------------------------------------------------------------------------------------------------

def _hdr(itw, key, w, h, mips=1, cube=False, arr=1):
    d = itw.DdsDesc(w, h, mips, itw.DXGI_FORMAT[key], 1 if cube else 0, arr)
    n = itw.lib().itwDdsHeaderBytes(C.byref(d))
    buf = np.zeros(n, dtype=np.uint8)
    assert itw.lib().itwDdsWriteHeader(C.byref(d), buf.ctypes.data, buf.size) == n
    return d, buf


@pytest.mark.parametrize("key,cc,bpb", [("bc4_snorm", b"BC4S", 8), ("bc5_snorm", b"BC5S", 16)])
@pytest.mark.parametrize("w,h,mips,cube", [(256, 128, 1, False), (64, 64, 7, True), (215, 217, 1, False)])
def test_dds_headers_round_trip(itw, key, cc, bpb, w, h, mips, cube):
    d, buf = _hdr(itw, key, w, h, mips=mips, cube=cube)
    assert buf.size == 128 and buf[84:88].tobytes() == cc                      # legacy FourCC, no DX10 extension (DirectXTexDDS.cpp:481-483)
    back = itw.DdsDesc()
    assert itw.lib().itwDdsReadHeader(buf.ctypes.data, buf.size, C.byref(back)) == 128
    assert (back.width, back.height, back.mip_levels, back.dxgi_format, back.is_cubemap) == (w, h, mips, itw.DXGI_FORMAT[key], 1 if cube else 0)
    # sizes by the pitch rule: ceil(w/4) * ceil(h/4) blocks per level, levels halved down
    chain, lw, lh = 0, w, h
    for _ in range(mips):
        assert itw.lib().itwDdsLevelBytes(itw.DXGI_FORMAT[key], lw, lh) == ((lw + 3) // 4) * ((lh + 3) // 4) * bpb
        chain += ((lw + 3) // 4) * ((lh + 3) // 4) * bpb
        lw, lh = max(1, lw // 2), max(1, lh // 2)
    assert itw.lib().itwDdsFileBytes(C.byref(d)) == 128 + chain * (6 if cube else 1)
    assert int.from_bytes(buf[20:24].tobytes(), "little") == ((w + 3) // 4) * ((h + 3) // 4) * bpb     # dwPitchOrLinearSize


def test_dds_ati_spellings_stay_unorm_and_dds_file_carries_the_blocks(itw):
    blocks = np.arange(2 * 3 * 16, dtype=np.uint8)
    f = itw.dds_file("bc5_snorm", 10, 6, [blocks])
    assert f.size == 128 + blocks.size and np.array_equal(f[128:], blocks)
    d = itw.DdsDesc()
    for cc, fmt in ((b"ATI1", 80), (b"ATI2", 83), (b"BC4S", 81), (b"BC5S", 84), (b"BC5U", 83)):
        alt = f.copy()
        alt[84:88] = np.frombuffer(cc, dtype=np.uint8)
        assert itw.lib().itwDdsReadHeader(alt.ctypes.data, alt.size, C.byref(d)) == 128 and d.dxgi_format == fmt


@pytest.mark.parametrize("key,unorm,mips,cube", [("bc4_snorm", "bc4", 1, False), ("bc5_snorm", "bc5", 1, False), ("bc5_snorm", "bc5", 9, True),
                                                 ("bc4_snorm", "bc4", 4, True)])
def test_headers_read_back_through_the_references_own_dds_definitions(itw, tmp_path, key, unorm, mips, cube):
    """oracle/_ref/ref_dds_check (DirectXTex/DDS.h compiled unmodified) knows the pixel formats DXT1, DXT5, BC4U, BC5U and DX10 by name, not
    the signed pair.  So the check is in two parts that together cover every byte: the 32-byte DDS_PIXELFORMAT equals DDSPF_BC4_SNORM /
    DDSPF_BC5_SNORM as DDS.h:86-93 define them -- { 32, DDS_FOURCC, 'BC4S' / 'BC5S', 0, 0, 0, 0, 0 } --, and with the FourCC's last letter put
    back to 'U' the header equals the UNORM format's byte for byte.  The tool is then run on that patched header; since it is the UNORM header,
    the run adds nothing beyond the byte comparison and what tests/test_dds_container.py proves for BC4U / BC5U -- it is kept so that this
    test follows the other formats' and starts checking more the day the tool learns the signed names.  The signed check proper is the
    comparison with DDS.h's definition above."""
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_dds_check")
    if not os.path.exists(exe):
        if not os.path.exists("/root/reference/3rdParty/DirectXTex/DirectXTex/DDS.h"):
            pytest.skip("oracle/_ref/ref_dds_check not prebuilt and /root/reference absent")
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle", "ref_build")], check=True)
    _, buf = _hdr(itw, key, 256, 128, mips=mips, cube=cube)
    cc = {"bc4_snorm": b"BC4S", "bc5_snorm": b"BC5S"}[key]
    ddspf = np.array([32, 0x4, int.from_bytes(cc, "little"), 0, 0, 0, 0, 0], dtype="<u4")
    assert buf[4 + 72:4 + 104].tobytes() == ddspf.tobytes()
    _, ubuf = _hdr(itw, unorm, 256, 128, mips=mips, cube=cube)
    patched = buf.copy()
    patched[87] = ord("U")
    assert np.array_equal(patched, ubuf)
    path = tmp_path / "h.dds"
    patched.tofile(path)
    r = subprocess.run([exe, str(path), cc[:3].decode() + "U", str(itw.DXGI_FORMAT[unorm]), "256", "128", str(mips), "1" if cube else "0", "1"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr


# ---- argument checks that need no device ------------------------------------------------------------------------------------------------

def test_bytes_per_block_and_format_tables(itw):
    L = itw.lib()
    assert L.GetBytesPerBlock(81) == 8 and L.GetBytesPerBlock(84) == 16
    assert itw.DXGI_FORMAT["bc4_snorm"] == 81 and itw.DXGI_FORMAT["bc5_snorm"] == 84
    assert itw.BYTES_PER_BLOCK["bc4_snorm"] == 8 and itw.BYTES_PER_BLOCK["bc5_snorm"] == 16
    assert "bc4_snorm" in itw.KEEPS_PARTIAL_BLOCKS and "bc5_snorm" in itw.KEEPS_PARTIAL_BLOCKS
    assert itw.OWN_CHANNELS["bc4_snorm"] == "r" and itw.OWN_CHANNELS["bc5_snorm"] == "rg"
    assert itw.block_count("bc5_snorm", 9, 263) == 3 * 66
    for name in ("CompressBlocksBC4S", "CompressBlocksBC5S", "itwWarmupBC45S", "CompressImageBC4S", "CompressImageBC5S"):
        assert name in itw.EXPORTED_SYMBOLS and hasattr(L, name)
    assert "itwTestBc45ClosestS" in itw.TEST_HOOK_SYMBOLS and not hasattr(L, "itwTestBc45ClosestS")
    assert itw.chain_bytes("bc4_snorm", [(10, 6), (5, 3), (1, 1)]) == (3 * 2 + 2 * 1 + 1) * 8
    assert itw.chain_bytes("bc5_snorm", [(10, 6), (5, 3), (1, 1)]) == (3 * 2 + 2 * 1 + 1) * 16
    assert itw.chain_bytes("bc5_snorm", [(10, 0)]) == -1


def test_stats_psnr_uses_the_code_range_254(itw):
    s = itw.ErrorStats()
    for fmt in (81, 84):
        s.dxgi_format, s.width, s.height = fmt, 10, 6
        s.sse[0], s.sse[1] = 120, 60
        want = 10.0 * np.log10(254.0 * 254.0 * (10 * 6 * 2) / 180.0)
        assert abs(itw.lib().itwStatsPsnr(C.byref(s), 3) - want) <= 1e-9
        assert abs(s.psnr() - (want if fmt == 84 else 10.0 * np.log10(254.0 * 254.0 * 60 / 120.0))) <= 1e-9


def test_bad_calls_with_the_signed_formats_return_before_any_device_use():
    """itwMeasureBlocks / itwMeasureChain / itwDecodeBlocks / itwCompressImageChainEx: each bad argument is refused as for the other formats.
    A fresh interpreter, so that nothing in it has touched a device."""
    code = r"""
import ctypes as C, sys, numpy as np
sys.path.insert(0, %r)
import itw_amd
L = itw_amd.lib()
itw_amd.set_error_mode(itw_amd.ON_ERROR_RETURN)
S = itw_amd.RgbaSurface
n = C.sizeof(itw_amd.ErrorStats)
img = np.zeros((8, 8, 4), dtype=np.int8)
blk = np.zeros(4096, dtype=np.uint8)
out = np.zeros(4096, dtype=np.uint8)
st = (itw_amd.ErrorStats * 4)()
stp = C.addressof(st)
good = S(img.ctypes.data, 8, 8, 32)
count = 0
for fmt in (81, 84):
    cases = {
        "null blocks": (fmt, None, good, stp, n, None),
        "null source": (fmt, blk.ctypes.data, None, stp, n, None),
        "null texels": (fmt, blk.ctypes.data, S(None, 8, 8, 32), stp, n, None),
        "null stats": (fmt, blk.ctypes.data, good, None, n, None),
        "width 0": (fmt, blk.ctypes.data, S(img.ctypes.data, 0, 8, 32), stp, n, None),
        "height 0": (fmt, blk.ctypes.data, S(img.ctypes.data, 8, 0, 32), stp, n, None),
        "stride below the row": (fmt, blk.ctypes.data, S(img.ctypes.data, 8, 8, 31), stp, n, None),
        "stats_bytes short": (fmt, blk.ctypes.data, good, stp, n - 8, None),
        "misaligned stats": (fmt, blk.ctypes.data, good, stp + 4, n, None),
        "too many blocks": (fmt, blk.ctypes.data, S(img.ctypes.data, 32768, 16388, 32768 * 4), stp, n, None),
    }
    for name, (f, b, s, stats, nbytes, m) in cases.items():
        L.itwClearError()
        rc = L.itwMeasureBlocks(f, b, C.byref(s) if s is not None else None, stats, nbytes, m)
        assert rc == -1 and itw_amd.last_error() is None, (fmt, name, rc, itw_amd.last_error())
        count += 1
    def arr(*s):
        return C.cast((S * len(s))(*s), C.c_void_p)
    chain = {
        "count 0": (arr(good), 0, blk.ctypes.data, fmt, stp, n),
        "null images": (None, 1, blk.ctypes.data, fmt, stp, n),
        "second image 0 wide": (arr(good, S(img.ctypes.data, 0, 8, 32)), 2, blk.ctypes.data, fmt, stp, n),
        "stats_bytes": (arr(good), 1, blk.ctypes.data, fmt, stp, n + 1),
    }
    for name, a in chain.items():
        L.itwClearError()
        assert L.itwMeasureChain(*a) == -1 and itw_amd.last_error() is None, (fmt, "chain", name)
        count += 1
    dec = {
        "width 0": (fmt, blk.ctypes.data, 0, 8, out.ctypes.data, 32, None),
        "height 0": (fmt, blk.ctypes.data, 8, 0, out.ctypes.data, 32, None),
        "stride below the row": (fmt, blk.ctypes.data, 8, 8, out.ctypes.data, 28, None),
        "stride not a multiple of 4": (fmt, blk.ctypes.data, 8, 8, out.ctypes.data, 34, None),
    }
    for name, a in dec.items():
        assert L.itwDecodeBlocks(*a) == -1, (fmt, "decode", name)
        count += 1
    # the chain: sizes first, then the call's own checks (itw_dispatch.h) through the error mode, before any device use
    assert L.itwChainBytes(arr(S(None, 10, 6, 0), S(None, 5, 3, 0)), 2, fmt) == (6 + 2) * (8 if fmt == 81 else 16)
    assert L.itwChainBytes(arr(S(None, 10, -1, 0)), 1, fmt) == -1
    assert L.itwChainBytes(None, 1, fmt) == -1
    for name, a in {"count 0": (arr(good), 0, out.ctypes.data, fmt, None, None, None),
                    "null target": (arr(good), 1, None, fmt, None, None, None),
                    "null images": (None, 1, out.ctypes.data, fmt, None, None, None),
                    "null texels": (arr(S(None, 8, 8, 32)), 1, out.ctypes.data, fmt, None, None, None),
                    "height 0": (arr(S(img.ctypes.data, 8, 0, 32)), 1, out.ctypes.data, fmt, None, None, None)}.items():
        L.itwClearError()
        assert L.itwCompressImageChainEx(*a) is False and itw_amd.last_error(), (fmt, "chain ex", name)
        count += 1
print("rejected", count)
""" % os.path.join(ROOT, "intel-texture-works-plugin_amd")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip() == "rejected 46"


def test_binding_rejects_uint8_for_the_signed_formats(itw):
    """A uint8 array handed to a signed format would be reinterpreted without a word (200 -> -56): TypeError, before any library call."""
    img = np.zeros((8, 8, 4), dtype=np.uint8)
    blocks = np.zeros(4 * 16, dtype=np.uint8)
    for fmt in ("bc4_snorm", "bc5_snorm"):
        with pytest.raises(TypeError):
            itw.compress_numpy(fmt, img)
        with pytest.raises(TypeError):
            itw.compress_image(fmt, img)
        with pytest.raises(TypeError):
            itw.compress_chain(fmt, [img.view(np.int8), img])
        with pytest.raises(TypeError):
            itw.measure(fmt, blocks, img)
        with pytest.raises(TypeError):
            itw.measure_chain(fmt, blocks, [img])
        with pytest.raises(TypeError):
            itw.compress_numpy(fmt, img.astype(np.int16))


def test_snorm_normal_map_is_seeded_unit_length_and_int8():
    from itw_amd import surfaces
    a = surfaces.snorm_normal_map(53, 101)
    assert a.dtype == np.int8 and a.shape == (53, 101, 4) and np.array_equal(a, surfaces.snorm_normal_map(53, 101))
    assert not np.array_equal(a, surfaces.snorm_normal_map(53, 101, seed=3))
    assert (a[..., 3] == 127).all() and a.min() >= -127 and (a[..., 2] > 0).all()
    n = np.sqrt((a[..., :3].astype(np.float64) ** 2).sum(axis=-1)) / 127.0
    assert np.abs(n - 1.0).max() < 0.02
    assert surfaces.snorm_normal_map(1, 1).shape == (1, 1, 4)
