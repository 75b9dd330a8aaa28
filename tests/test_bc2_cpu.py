"""BC2 (ITW_FORMAT_BC2_UNORM[_SRGB], include/itw_dispatch.h) without a GPU: the numpy model of tests/_dxtex_bc2.py and the kernel's own text
run on the host (tools/bc2_host_check.cpp over csrc/bc2_core.hpp) against the reference's D3DXEncodeBC2 and its recorded streams
(tests/golden/bc2_ref.npz), byte for byte; what the dither does over the content the GPU tests encode; the format table's facts; what the
entry points refuse before any device work (DXGI 74 / 75 among it); the symbol list; and the built kernels' resources."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _dxtex_bc2 as B2
from _dxtex_snorm import block_texels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "intel-texture-works-plugin_amd", "csrc", "build")
BC2, BC2_SRGB = 0x83F2, 0x8C4E


@pytest.fixture(scope="module")
def texels():
    return {name: block_texels(img) for name, img in B2.content().items()}


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("bc2_host_check")
    return B2.build_host_check(d), d


def test_content_and_golden_file(texels):
    assert texels["boundary"].shape == (1024, 16, 4) and texels["strip"].shape == (256, 16, 4) and texels["alpha"].shape == (64, 16, 4)
    g = B2.golden()
    assert len(g) == 3 * len(B2.FLAG_SETS) + len(B2.SIZES) * len(B2.SIZE_FLAGS) + 2
    for name, tx in texels.items():
        for flags in B2.FLAG_SETS:
            assert g[B2.golden_key(name, flags)].size == tx.shape[0] * 16
    assert np.array_equal(g["decode.blocks"], B2.decode_test_blocks()) and g["decode.ref"].shape == (64, 16, 4)


@pytest.mark.parametrize("flags", B2.FLAG_SETS, ids=lambda f: "flags_%05x" % f)
def test_model_equals_golden(texels, flags):
    g = B2.golden()
    for name, tx in texels.items():
        want = g[B2.golden_key(name, flags)].reshape(-1, 16)
        got = B2.model(tx, flags)[0]
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (name, hex(flags), bad[:8], got[bad[:2]], want[bad[:2]])


@pytest.mark.parametrize("flags", B2.FLAG_SETS, ids=lambda f: "flags_%05x" % f)
def test_reference_equals_golden(texels, flags):
    g = B2.golden()
    for name, tx in texels.items():
        assert np.array_equal(B2.encode_blocks(tx, flags), g[B2.golden_key(name, flags)].reshape(-1, 16)), (name, hex(flags))


def test_odd_sizes_take_the_directxtex_fill():
    """Golden == model for the partial-block cases the GPU tests encode: ceil(w/4) x ceil(h/4) blocks, texels beyond the edge
    replicated by the {0, 0, 0, 1} rule."""
    g = B2.golden()
    for h, w in B2.SIZES:
        img = B2.size_image(h, w)
        for flags in B2.SIZE_FLAGS:
            want = g[B2.size_key(h, w, flags)]
            assert want.size == ((h + 3) // 4) * ((w + 3) // 4) * 16
            assert np.array_equal(B2.model(block_texels(img), flags)[0].reshape(-1), want), (h, w, hex(flags))


def test_odd_sizes_reference_equals_golden():
    g = B2.golden()
    for h, w in B2.SIZES:
        for flags in B2.SIZE_FLAGS:
            assert np.array_equal(B2.encode(B2.size_image(h, w), flags), g[B2.size_key(h, w, flags)]), (h, w, hex(flags))


def test_references_decode_equals_its_recording():
    g = B2.golden()
    assert np.array_equal(B2.decode(g["decode.blocks"]), g["decode.ref"])


@pytest.mark.parametrize("flags", B2.FLAG_SETS, ids=lambda f: "flags_%05x" % f)
def test_the_kernels_text_on_the_host_equals_golden(texels, host_check, flags):
    exe, d = host_check
    g = B2.golden()
    for name, tx in texels.items():
        got = B2.host_check_encode(exe, d, tx, flags)
        want = g[B2.golden_key(name, flags)].reshape(-1, 16)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (name, hex(flags), bad[:8])


def test_the_colour_half_is_the_bc1a_stream_with_no_key(texels):
    """D3DXEncodeBC2 calls EncodeBC1(bColorKey = false, 0.f, flags): bytes 8..15 of every block are D3DXEncodeBC1's with alpha_ref 0 and
    without DITHER_A, which tests/golden/bc1a_ref.npz holds for the shared content."""
    import _dxtex_bc1 as B
    g, g1 = B2.golden(), B.golden()
    for name in ("boundary", "strip"):
        for flags in B2.FLAG_SETS:
            got = g[B2.golden_key(name, flags)].reshape(-1, 16)[:, 8:]
            assert np.array_equal(got, g1[B.golden_key(name, 0.0, flags & ~B.DITHER_A)].reshape(-1, 8)), (name, hex(flags))


def test_coverage_what_the_dither_does_over_the_shared_content(texels):
    """The GPU comparison cannot pass by never entering a case: under DITHER_A the content holds a nibble the diffusion raises, one it
    lowers, a texel whose fAlph is above 1 and one below 0 -- in the model AND in the reference's own bytes (its DITHER_A stream differs from
    its plain one in exactly the blocks the model names); without the flag all 256 alpha codes occur.  No texel's u exceeds 15."""
    tx = np.concatenate(list(texels.values()))
    g = B2.golden()
    for flags in (B2.DITHER_A, B2.DITHER_A | B2.DITHER_RGB | B2.UNIFORM):
        c = {k: int(v.sum()) for k, v in B2.alpha_model(tx, flags)[1].items()}
        print(hex(flags), c)
        assert c["raised"] >= 1 and c["lowered"] >= 1 and c["above_one"] >= 1 and c["below_zero"] >= 1 and c["spill"] == 0, c
    for name, t in texels.items():
        paths = B2.alpha_model(t, B2.DITHER_A)[1]
        plain = g[B2.golden_key(name, 0)].reshape(-1, 16)[:, :8].copy().view("<u4")
        dith = g[B2.golden_key(name, B2.DITHER_A)].reshape(-1, 16)[:, :8].copy().view("<u4")
        nib = lambda w: np.stack([(w[:, i >> 3] >> (4 * (i & 7))) & 15 for i in range(16)], axis=1).astype(np.int64)      # noqa: E731
        assert np.array_equal((nib(dith) > nib(plain)).any(axis=1), paths["raised"]), name
        assert np.array_equal((nib(dith) < nib(plain)).any(axis=1), paths["lowered"]), name
    c = {k: int(v.sum()) for k, v in B2.alpha_model(tx, 0)[1].items()}
    assert not any(c.values()), c                                                       # without the flag nothing of this happens
    assert set(np.unique(tx[..., 3]).tolist()) == set(range(256))
    # without the flag a nibble is the rounded alpha: floor(a / 17 + 0.5) on the integer codes
    plain = B2.alpha_model(tx, 0)[0].view("<u4")
    for i in range(16):
        assert np.array_equal((plain[:, i >> 3] >> (4 * (i & 7))) & 15, (tx[:, i, 3].astype(np.int64) * 2 + 17) // 34), i


def test_table_facts(itw):
    L = itw.lib()
    for key, code in (("bc2", BC2), ("bc2_srgb", BC2_SRGB)):
        assert itw.DXGI_FORMAT[key] == code and itw.BYTES_PER_BLOCK[key] == 16 and key in itw.KEEPS_PARTIAL_BLOCKS and itw.OWN_CHANNELS[key] == "rgba"
        assert L.GetBytesPerBlock(code) == 16
        assert itw.block_count(key, 61, 75) == 16 * 19                       # partial blocks kept: ceil, like BC4 / BC5
        sizes = [(1, 1), (3, 5), (61, 75), (64, 64)]
        assert itw.chain_bytes(key, sizes) == 16 * sum(((h + 3) // 4) * ((w + 3) // 4) for h, w in sizes) == itw.chain_bytes("bc5", sizes)
        # the window of the transfer-bound formats: 262 144 blocks = 16 slices of 4096^2's 64
        assert L.itwSliceWindow(code, 4096, 4096, 0x40000) == 16 == L.itwSliceWindow(83, 4096, 4096, 0x40000)
        assert L.itwSliceWindowFor(code, None, 4096, 4096, 0x40000) == 16
        assert itw.band_for_part(61, 75, key, 1, 2) == itw.band_for_part(61, 75, "bc5", 1, 2)
    # DXGI's own codes for BC2 stay what they were: codes the library does not know (GetBytesPerBlock: the reference's default, 8)
    for code in (74, 75):
        assert L.GetBytesPerBlock(code) == 8
    assert "ignored" in itw.Bc1aSettings.__doc__ and "bc2" in itw.Bc1aSettings.__doc__


def test_the_product_library_still_lists_its_132_names(itw):
    out = subprocess.run(["nm", "-D", "--defined-only", itw.lib_path()], check=True, capture_output=True, text=True).stdout
    names = sorted(l.split()[2] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T")
    assert names == sorted(itw.EXPORTED_SYMBOLS) and len(names) == 132


def test_bad_bc2_calls_return_false_before_any_device_use():
    """The settings rules and the entry points that refuse the format, each with its message and nothing written; 74 / 75 stay refused at
    the encode, decode and preview entry points.  Run in a fresh interpreter: the error mode is process-wide."""
    code = r"""
import ctypes as C, sys, numpy as np
sys.path.insert(0, %r)
import itw_amd
L = itw_amd.lib()
itw_amd.set_error_mode(itw_amd.ON_ERROR_RETURN)
BC2 = 0x83F2
img = np.zeros((8, 8, 4), dtype=np.uint8)
out = np.full(4096, 0xA5, dtype=np.uint8)
def arr(*s):
    return C.cast((itw_amd.RgbaSurface * len(s))(*s), C.c_void_p)
good = itw_amd.RgbaSurface(img.ctypes.data, 8, 8, 32)
def st(**kw):
    s = itw_amd.Bc1aSettings()
    for k, v in kw.items():
        setattr(s, k, v)
    return s
bad = {"struct_size 12": (st(struct_size=12), "struct_size"), "struct_size 0": (st(struct_size=0), "struct_size"), "reserved": (st(reserved=1), "reserved"),
       "flag 0x80000": (st(flags=0x80000), "flag"), "flag 1": (st(flags=0x10001), "flag"), "nan": (st(alpha_ref=float("nan")), "finite"),
       "inf": (st(alpha_ref=float("inf")), "finite"), "-inf": (st(alpha_ref=float("-inf")), "finite")}
n = 0
for code_ in (BC2, 0x8C4E):
    for name, (s, word) in bad.items():
        sp = C.cast(C.byref(s), C.c_void_p)
        for call in ("sliced", "chain", "mipped", "mipped_ex", "mipped_alpha"):
            L.itwClearError()
            if call == "sliced":
                ok = L.itwCompressImageSlicedEx(C.byref(good), out.ctypes.data, 32, code_, sp, 0, None, None)
            elif call == "chain":
                ok = L.itwCompressImageChainEx(arr(good), 1, out.ctypes.data, code_, sp, None, None)
            elif call == "mipped":
                ok = L.itwCompressImageMipped(arr(good), 1, 0, 0, out.ctypes.data, code_, sp, None, None)
            elif call == "mipped_ex":
                ok = L.itwCompressImageMippedEx(arr(good), 1, 0, 0, itw_amd.MIP_SRGB, out.ctypes.data, code_, sp, None, None)
            else:
                a = itw_amd.MipAlpha(0, 128)
                ok = L.itwCompressImageMippedAlpha(arr(good), 1, 0, 0, C.cast(C.byref(a), C.c_void_p), out.ctypes.data, code_, sp, None, None)
            err = itw_amd.last_error()
            assert ok is False and err and word in err and err.startswith("BC2:"), (name, call, ok, err)
            n += 1
# the chain's and the slice call's own argument rules still hold with good settings
ok_s = itw_amd.Bc1aSettings()
okp = C.cast(C.byref(ok_s), C.c_void_p)
for images, count in ((arr(good), 0), (None, 1), (arr(itw_amd.RgbaSurface(None, 8, 8, 32)), 1), (arr(itw_amd.RgbaSurface(img.ctypes.data, 8, 8, 31)), 1)):
    L.itwClearError()
    assert L.itwCompressImageChainEx(images, count, out.ctypes.data, BC2, okp, None, None) is False and itw_amd.last_error()
L.itwClearError()
assert L.itwCompressImageSlicedEx(C.byref(good), out.ctypes.data, 16, BC2, None, 0, None, None) is False and "block_row_pitch" in itw_amd.last_error()
# refused: the refined calls, the multi-GPU calls, the normal-map chain calls, normal ops
rs = itw_amd.RefineStats()
L.itwClearError()
assert L.itwCompressImageRefined(C.byref(good), out.ctypes.data, BC2, okp, okp, 15, 0, C.addressof(rs), C.sizeof(rs), None, None) is False
assert "one encoder" in itw_amd.last_error()
L.itwClearError()
assert L.itwCompressImageChainRefined(arr(good), 1, out.ctypes.data, BC2, okp, okp, 15, 0, C.addressof(rs), C.sizeof(rs), None, None, None) is False
assert "one encoder" in itw_amd.last_error()
called = []
fn = itw_amd.abi.COMPRESSION_FUNC(lambda s, o: called.append(1))
L.itwClearError()
assert L.itwCompressImageMultiGPU(C.byref(good), out.ctypes.data, C.cast(fn, C.c_void_p), BC2, 1) is False
assert "(BC2) has no block-level function" in itw_amd.last_error()
assert not called
for ops in (4, 1):
    L.itwClearError()
    assert L.itwCompressNormalMapChain(arr(good), 1, out.ctypes.data, BC2, None, ops, None, None) is False and "(BC2) holds colour, not normals" in itw_amd.last_error()
L.itwClearError()
assert L.itwCompressNormalMapChain(arr(good), 1, out.ctypes.data, BC2, None, 0, None, None) is False and "not normals" in itw_amd.last_error()
L.itwClearError()
assert L.itwCompressImageMipped(arr(good), 1, 0, 4, out.ctypes.data, BC2, None, None, None) is False and "(BC2), which holds colour" in itw_amd.last_error()
# KTX carries ETC1 and nothing else
kd = itw_amd.KtxDesc(8, 8, 1, BC2, 0, 0)
assert L.itwKtxFileBytes(C.byref(kd)) == 0
# 74 / 75 stay codes the library does not encode, decode or preview
for code_ in (74, 75):
    L.itwClearError()
    assert L.itwCompressImageSlicedEx(C.byref(good), out.ctypes.data, 32, code_, None, 0, None, None) is False and "not one this library encodes" in itw_amd.last_error()
    L.itwClearError()
    assert L.itwCompressImageChainEx(arr(good), 1, out.ctypes.data, code_, None, None, None) is False and itw_amd.last_error()
    assert L.itwChainBytes(arr(good), 1, code_) == -1
    blocks = np.zeros(64, dtype=np.uint8)
    tex = np.full((8, 8, 4), 0xA5, dtype=np.uint8)
    ts = itw_amd.RgbaSurface(tex.ctypes.data, 8, 8, 32)
    assert L.itwDecodeBlocks(code_, blocks.ctypes.data, 8, 8, tex.ctypes.data, 32, None) == -1
    assert L.itwDecodeImage(code_, blocks.ctypes.data, C.byref(ts), None, None) == -1
    assert L.itwDecodeChain(code_, blocks.ctypes.data, arr(ts), 1, None, None) == -1
    v = itw_amd.preview_view(4, 4)
    rgb = np.full(48, 0xA5, dtype=np.uint8)
    assert L.itwPreviewBlocks(code_, blocks.ctypes.data, 8, 8, C.byref(v), C.sizeof(v), rgb.ctypes.data, 12) == -1
    es = itw_amd.ErrorStats()
    assert L.itwMeasureBlocks(code_, blocks.ctypes.data, C.byref(good), C.byref(es), C.sizeof(es), None) == -1
    assert (tex == 0xA5).all() and (rgb == 0xA5).all()
assert (out == 0xA5).all()
print("rejected", n)
""" % os.path.join(ROOT, "intel-texture-works-plugin_amd")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip() == "rejected 80"


def test_every_kernel_variant_uses_no_scratch_and_no_lds():
    """Scratch and LDS are 0 B for every variant (2 dither bits x 2 load paths): every array of bc2_core.hpp and bc1a_core.hpp is indexed by
    unrolled loop counters, and the alpha pass's error array is dead before the colour half starts."""
    path = os.path.join(BUILD, "bc2.o")
    if not os.path.exists(path):
        pytest.skip("csrc/build/ is not populated: run __graft_entry__.build() first")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), path, "bc2_kernel"], check=True, capture_output=True, text=True).stdout
    seen = {}
    for line in out.splitlines():
        m = re.match(r"(?:void )?itw::(bc2_kernel<\S+, \S+>)\s+vgpr\s+(\d+) agpr\s+(\d+) .*?scratch\s+(\d+) B\s+lds\s+(\d+) B", line)
        if m:
            seen[m.group(1)] = (int(m.group(2)) + int(m.group(3)), int(m.group(4)), int(m.group(5)))
    want = {"bc2_kernel<%du, %s>" % (d, v) for d in range(4) for v in ("true", "false")}
    assert set(seen) == want, sorted(seen)
    for name, (regs, scratch, lds) in seen.items():
        assert scratch == 0 and lds == 0, (name, regs, scratch, lds)
        assert 512 // (-(-regs // 8) * 8) >= 2, (name, regs)              # two waves per SIMD, as DESIGN.md 3.15 records


def test_the_decode_side_kernels_of_bc2_use_no_scratch():
    """The BC2 instantiations in decode_chain.o, measure.o and preview.o: 0 B of scratch, no spills; the preview pair (named
    preview_bc2_kernel: tests/test_preview_cpu.py pins the set of preview_kernel instantiations as it was) has the tile route's LDS of
    33 x 9 blocks and none on the per-pixel route, and leaves at least 4 waves per SIMD like the other preview kernels."""
    want = {"decode_chain.o": ("decode_chain_kernel<2, true>", "decode_chain_kernel<2, false>"), "measure.o": ("measure_kernel<2>",),
            "preview.o": ("preview_bc2_kernel<true>", "preview_bc2_kernel<false>")}
    for obj, names in want.items():
        path = os.path.join(BUILD, obj)
        if not os.path.exists(path):
            pytest.skip("csrc/build/ is not populated: run __graft_entry__.build() first")
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), path], check=True, capture_output=True, text=True).stdout
        seen = {}
        for line in out.splitlines():
            m = re.match(r"(?:void )?itw::(\S+<[^>]*>)\s+vgpr\s+(\d+) agpr\s+(\d+) .*?scratch\s+(\d+) B\s+lds\s+(\d+) B\s+spills v(\d+) s(\d+)", line)
            if m:
                seen[m.group(1)] = tuple(int(m.group(i)) for i in range(2, 8))
        for name in names:
            assert name in seen, (obj, name, sorted(seen))
            vgpr, agpr, scratch, lds, vspill, sspill = seen[name]
            assert (scratch, vspill, sspill) == (0, 0, 0), (name, seen[name])
            if obj == "preview.o":
                assert lds == (33 * 9 * 64 if name.endswith("<true>") else 0), (name, lds)
                assert min(512 // (-(-(vgpr + agpr) // 8) * 8), (160 * 1024) // lds if lds else 8) >= 4, (name, seen[name])
