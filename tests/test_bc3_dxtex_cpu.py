"""BC3 by DirectXTex's encoder (ITW_FORMAT_BC3_DXTEX[_SRGB], include/itw_dispatch.h) without a GPU: the numpy model of tests/_dxtex_bc3.py and
the kernel's own text run on the host (tools/bc3_host_check.cpp over csrc/bc3_core.hpp) against the reference's D3DXEncodeBC3 and its recorded
streams (tests/golden/bc3_dxtex_ref.npz), byte for byte; the branches of the alpha half the shared content takes; the format table's facts;
what the entry points refuse before any device work; the symbol list; the built kernels' resources; and that the three encoders whose text
the new one borrows or sits beside compile to the code objects they had."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _dxtex_bc3 as B3
from _dxtex_snorm import block_texels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "intel-texture-works-plugin_amd", "csrc", "build")
BC3DX, BC3DX_SRGB = 0x83F3, 0x8C4F


@pytest.fixture(scope="module")
def texels():
    return {name: block_texels(img) for name, img in B3.content().items()}


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("bc3_host_check")
    return B3.build_host_check(d), d


def test_content_and_golden_file(texels):
    assert texels["boundary"].shape == (1024, 16, 4) and texels["strip"].shape == (256, 16, 4) and texels["alpha"].shape == (128, 16, 4)
    g = B3.golden()
    assert len(g) == 3 * len(B3.FLAG_SETS) + len(B3.SIZES) * len(B3.SIZE_FLAGS)
    for name, tx in texels.items():
        for flags in B3.FLAG_SETS:
            assert g[B3.golden_key(name, flags)].size == tx.shape[0] * 16
    assert os.path.getsize(B3.GOLDEN) < 1 << 20


@pytest.mark.parametrize("flags", B3.FLAG_SETS, ids=lambda f: "flags_%05x" % f)
def test_model_equals_golden(texels, flags):
    g = B3.golden()
    for name, tx in texels.items():
        want = g[B3.golden_key(name, flags)].reshape(-1, 16)
        got = B3.model(tx, flags)[0]
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (name, hex(flags), bad[:8], got[bad[:2]], want[bad[:2]])


@pytest.mark.parametrize("flags", B3.FLAG_SETS, ids=lambda f: "flags_%05x" % f)
def test_reference_equals_golden(texels, flags):
    g = B3.golden()
    for name, tx in texels.items():
        assert np.array_equal(B3.encode_blocks(tx, flags), g[B3.golden_key(name, flags)].reshape(-1, 16)), (name, hex(flags))


def test_odd_sizes_take_the_directxtex_fill():
    """Golden == model for the partial-block cases the GPU tests encode: ceil(w/4) x ceil(h/4) blocks, texels beyond the edge
    replicated by the {0, 0, 0, 1} rule."""
    g = B3.golden()
    for h, w in B3.SIZES:
        img = B3.size_image(h, w)
        for flags in B3.SIZE_FLAGS:
            want = g[B3.size_key(h, w, flags)]
            assert want.size == ((h + 3) // 4) * ((w + 3) // 4) * 16
            assert np.array_equal(B3.model(block_texels(img), flags)[0].reshape(-1), want), (h, w, hex(flags))


def test_odd_sizes_reference_equals_golden():
    g = B3.golden()
    for h, w in B3.SIZES:
        for flags in B3.SIZE_FLAGS:
            assert np.array_equal(B3.encode(B3.size_image(h, w), flags), g[B3.size_key(h, w, flags)]), (h, w, hex(flags))


@pytest.mark.parametrize("flags", B3.FLAG_SETS, ids=lambda f: "flags_%05x" % f)
def test_the_kernels_text_on_the_host_equals_golden(texels, host_check, flags):
    exe, d = host_check
    g = B3.golden()
    for name, tx in texels.items():
        got = B3.host_check_encode(exe, d, tx, flags)
        want = g[B3.golden_key(name, flags)].reshape(-1, 16)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (name, hex(flags), bad[:8])
    for h, w in B3.SIZES:
        if flags in B3.SIZE_FLAGS:
            got = B3.host_check_encode(exe, d, block_texels(B3.size_image(h, w)), flags)
            assert np.array_equal(got.reshape(-1), g[B3.size_key(h, w, flags)]), (h, w, hex(flags))


def test_the_colour_half_is_the_bc1a_stream_with_no_key():
    """D3DXEncodeBC3 calls EncodeBC1(bColorKey = false, 0.f, flags): bytes 8..15 of every block are D3DXEncodeBC1's with alpha_ref 0 and
    without DITHER_A, which tests/golden/bc1a_ref.npz holds for the shared content."""
    import _dxtex_bc1 as B
    g, g1 = B3.golden(), B.golden()
    for name in ("boundary", "strip"):
        for flags in B3.FLAG_SETS:
            got = g[B3.golden_key(name, flags)].reshape(-1, 16)[:, 8:]
            assert np.array_equal(got, g1[B.golden_key(name, 0.0, flags & ~B.DITHER_A)].reshape(-1, 8)), (name, hex(flags))


def test_every_named_branch_is_taken_by_the_recorded_streams(texels):
    """The GPU comparison cannot pass by never entering a case.  The model equals the reference's recorded stream for every flag set
    (test_model_equals_golden), so the branches the model names are the branches the reference's stream took: each is taken by the shared
    content, except those no RGBA8 block is known to take (_dxtex_bc3.UNREACHED_BRANCHES, with the reasons), which the
    content is asserted NOT to take, so that a block which does take one would show here."""
    g = B3.golden()
    tx = np.concatenate(list(texels.values()))
    want = np.concatenate([g[B3.golden_key(name, 0)].reshape(-1, 16) for name in texels])
    want_a = np.concatenate([g[B3.golden_key(name, B3.DITHER_A)].reshape(-1, 16) for name in texels])
    for flags, stream in ((0, want), (B3.DITHER_A, want_a)):
        alpha, branches = B3.alpha_model(tx, flags)
        assert np.array_equal(alpha, stream[:, :8])
        c = B3.census(branches)
        print(hex(flags), c)
        for k in B3.BRANCHES + (B3.DITHER_A_BRANCHES if flags else ()):
            if k in B3.UNREACHED_BRANCHES:
                assert c[k] == 0, (hex(flags), k, c[k])
            else:
                assert c[k] >= 1, (hex(flags), k)
    # the stream says the same where it can: the early outs leave a zero bitmap, the 6-step blocks store alpha[0] <= alpha[1] or FF 00
    _, br = B3.alpha_model(tx, 0)
    assert (want[br["all_opaque"], :8] == np.array([255, 255, 0, 0, 0, 0, 0, 0], dtype=np.uint8)).all()
    eq = br["eight_equal_endpoints"]
    assert (want[eq, 0] == want[eq, 1]).all() and not want[eq, 2:8].any()
    assert (want[br["eight"] & ~eq, 0] > want[br["eight"] & ~eq, 1]).all()
    # DITHER_A changes indices and nothing else of the alpha half: an RGBA8 source leaves the pre-pass nothing to diffuse
    assert B3.prepass_is_identity()
    assert np.array_equal(want[:, :2], want_a[:, :2]) and (want[:, 2:8] != want_a[:, 2:8]).any()
    assert set(np.unique(tx[..., 3]).tolist()) == set(range(256))


def test_table_facts(itw):
    L = itw.lib()
    for key, code, stream in (("bc3_dxtex", BC3DX, "bc3"), ("bc3_dxtex_srgb", BC3DX_SRGB, "bc3_srgb")):
        assert itw.DXGI_FORMAT[key] == code and itw.BYTES_PER_BLOCK[key] == 16 and key in itw.KEEPS_PARTIAL_BLOCKS and itw.OWN_CHANNELS[key] == "rgba"
        assert L.GetBytesPerBlock(code) == 16
        assert itw.block_count(key, 61, 75) == 16 * 19                       # partial blocks kept: ceil, like BC2
        sizes = [(1, 1), (3, 5), (61, 75), (64, 64)]
        assert itw.chain_bytes(key, sizes) == 16 * sum(((h + 3) // 4) * ((w + 3) // 4) for h, w in sizes) == itw.chain_bytes("bc2", sizes)
        for w, h, px in ((4096, 4096, 0x40000), (61, 75, 0), (1028, 4, 16)):
            assert L.itwSliceWindow(code, w, h, px) == L.itwSliceWindow(0x83F2, w, h, px)
            assert L.itwSliceWindowFor(code, None, w, h, px) == L.itwSliceWindowFor(0x83F2, None, w, h, px)
        assert L.itwSliceWindow(code, 4096, 4096, 0x40000) == 16
        assert itw.band_for_part(61, 75, key, 1, 2) == itw.band_for_part(61, 75, "bc2", 1, 2)
    # 77 / 78 keep their geometry: kernel.ispc's encoder drops partial blocks
    assert itw.block_count("bc3", 61, 75) == 15 * 18 and L.GetBytesPerBlock(77) == 16
    assert "bc3_dxtex" in itw.Bc1aSettings.__doc__


def test_the_product_library_still_lists_its_132_names(itw):
    out = subprocess.run(["nm", "-D", "--defined-only", itw.lib_path()], check=True, capture_output=True, text=True).stdout
    names = sorted(l.split()[2] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T")
    assert names == sorted(itw.EXPORTED_SYMBOLS) and len(names) == 132


def test_bad_bc3_dxtex_calls_return_false_before_any_device_use():
    """The settings rules and the entry points that refuse the codes, each with its message and nothing written.  Run in a fresh
    interpreter: the error mode is process-wide."""
    code = r"""
import ctypes as C, sys, numpy as np
sys.path.insert(0, %r)
import itw_amd
L = itw_amd.lib()
itw_amd.set_error_mode(itw_amd.ON_ERROR_RETURN)
BC3DX = 0x83F3
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
for code_ in (BC3DX, 0x8C4F):
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
            assert ok is False and err and word in err and err.startswith("BC3 (DirectXTex):"), (name, call, ok, err)
            n += 1
# the chain's and the slice call's own argument rules still hold with good settings
ok_s = itw_amd.Bc1aSettings()
okp = C.cast(C.byref(ok_s), C.c_void_p)
for images, count in ((arr(good), 0), (None, 1), (arr(itw_amd.RgbaSurface(None, 8, 8, 32)), 1), (arr(itw_amd.RgbaSurface(img.ctypes.data, 8, 8, 31)), 1)):
    L.itwClearError()
    assert L.itwCompressImageChainEx(images, count, out.ctypes.data, BC3DX, okp, None, None) is False and itw_amd.last_error()
L.itwClearError()
assert L.itwCompressImageSlicedEx(C.byref(good), out.ctypes.data, 16, BC3DX, None, 0, None, None) is False and "block_row_pitch" in itw_amd.last_error()
# refused: the refined calls, the multi-GPU calls, the normal-map chain calls, normal ops
for code_ in (BC3DX, 0x8C4F):
    rs = itw_amd.RefineStats()
    L.itwClearError()
    assert L.itwCompressImageRefined(C.byref(good), out.ctypes.data, code_, okp, okp, 15, 0, C.addressof(rs), C.sizeof(rs), None, None) is False
    assert "one encoder" in itw_amd.last_error()
    L.itwClearError()
    assert L.itwCompressImageChainRefined(arr(good), 1, out.ctypes.data, code_, okp, okp, 15, 0, C.addressof(rs), C.sizeof(rs), None, None, None) is False
    assert "one encoder" in itw_amd.last_error()
    called = []
    fn = itw_amd.abi.COMPRESSION_FUNC(lambda s, o: called.append(1))
    L.itwClearError()
    assert L.itwCompressImageMultiGPU(C.byref(good), out.ctypes.data, C.cast(fn, C.c_void_p), code_, 1) is False
    assert "(BC3 by DirectXTex's encoder) has no block-level function" in itw_amd.last_error()
    assert not called
    for ops in (4, 1):
        L.itwClearError()
        assert L.itwCompressNormalMapChain(arr(good), 1, out.ctypes.data, code_, None, ops, None, None) is False and "(BC3 by DirectXTex's encoder) holds colour, not normals" in itw_amd.last_error()
    L.itwClearError()
    assert L.itwCompressNormalMapChain(arr(good), 1, out.ctypes.data, code_, None, 0, None, None) is False and "not normals" in itw_amd.last_error()
    L.itwClearError()
    assert L.itwCompressImageMipped(arr(good), 1, 0, 4, out.ctypes.data, code_, None, None, None) is False and "(BC3 by DirectXTex's encoder), which holds colour" in itw_amd.last_error()
    # KTX carries ETC1 and nothing else
    kd = itw_amd.KtxDesc(8, 8, 1, code_, 0, 0)
    assert L.itwKtxFileBytes(C.byref(kd)) == 0
# the neighbouring values stay codes the library does not know
for code_ in (0x83F0, 0x83F4, 0x8C4C, 0x8C50):
    L.itwClearError()
    assert L.itwCompressImageSlicedEx(C.byref(good), out.ctypes.data, 32, code_, None, 0, None, None) is False and "not one this library encodes" in itw_amd.last_error()
    assert L.itwChainBytes(arr(good), 1, code_) == -1 and L.GetBytesPerBlock(code_) == 8
assert (out == 0xA5).all()
print("rejected", n)
""" % os.path.join(ROOT, "intel-texture-works-plugin_amd")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip() == "rejected 80"


def test_every_kernel_variant_uses_no_scratch_and_no_lds():
    """Scratch and LDS are 0 B, no VGPR spills and at most 256 VGPRs (two waves per SIMD, bc2_kernel's figure) for every variant (2 dither
    bits x 2 load paths): every array of bc3_core.hpp and bc1a_core.hpp is indexed by unrolled loop counters, a value picked by a run-time
    step comes through selects, and the alpha pass's arrays are dead before the colour half starts."""
    path = os.path.join(BUILD, "bc3_dxtex.o")
    if not os.path.exists(path):
        pytest.skip("csrc/build/ is not populated: run __graft_entry__.build() first")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), path, "bc3_dxtex_kernel"], check=True, capture_output=True, text=True).stdout
    seen = {}
    for line in out.splitlines():
        m = re.match(r"(?:void )?itw::(bc3_dxtex_kernel<\S+, \S+>)\s+vgpr\s+(\d+) agpr\s+(\d+) .*?scratch\s+(\d+) B\s+lds\s+(\d+) B\s+spills v(\d+)", line)
        if m:
            seen[m.group(1)] = (int(m.group(2)) + int(m.group(3)), int(m.group(4)), int(m.group(5)), int(m.group(6)))
    want = {"bc3_dxtex_kernel<%du, %s>" % (d, v) for d in range(4) for v in ("true", "false")}
    assert set(seen) == want, sorted(seen)
    for name, (regs, scratch, lds, vspill) in seen.items():
        print(name, regs, scratch, lds, vspill)
        assert scratch == 0 and lds == 0 and vspill == 0, (name, regs, scratch, lds, vspill)
        assert regs <= 256 and 512 // (-(-regs // 8) * 8) >= 2, (name, regs)


def _code_digests(obj):
    """kernel or device function -> SHA-256 of its instructions as tools/code_object_diff.py compares them (pc-relative literals masked)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import tempfile
    import code_object_diff as D
    from kernel_resources import unbundle
    with tempfile.TemporaryDirectory() as d:
        dis = D.disassembly_by_symbol(unbundle(obj, d), False)
    return {name: hashlib.sha256("\n".join(ins).encode()).hexdigest() for name, ins in dis.items()}


@pytest.mark.parametrize("obj", ("bc4_bc5", "bc1a", "bc2"))
def test_the_neighbouring_encoders_compile_to_the_code_they_had(obj):
    """bc4_bc5.o (whose Newton loop bc3_core.hpp restates instead of sharing), bc1a.o and bc2.o (whose text the new kernel includes) hold,
    kernel for kernel, the instructions they held before this format was added: the digests of tests/golden/bc3_dxtex_parent_code.json were
    taken from a build of the parent commit with the comparison of tools/code_object_diff.py."""
    path = os.path.join(BUILD, obj + ".o")
    if not os.path.exists(path):
        pytest.skip("csrc/build/ is not populated: run __graft_entry__.build() first")
    with open(os.path.join(ROOT, "tests", "golden", "bc3_dxtex_parent_code.json")) as f:
        want = json.load(f)[obj]
    got = _code_digests(path)
    assert sorted(got) == sorted(want), (sorted(set(got) ^ set(want)))
    assert [k for k in want if got[k] != want[k]] == []
