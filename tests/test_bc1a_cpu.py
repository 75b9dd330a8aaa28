"""BC1 with 1-bit alpha (ITW_FORMAT_BC1A_UNORM[_SRGB], include/itw_dispatch.h) without a GPU: the numpy model of tests/_dxtex_bc1.py and the
kernel's own text run on the host (tools/bc1a_host_check.cpp over csrc/bc1a_core.hpp) against the reference's D3DXEncodeBC1 and its recorded
streams (tests/golden/bc1a_ref.npz), byte for byte; the model's census of the source's branches over the content the GPU tests encode; what the
entry points refuse before any device work; the format table's facts; the DDS header; and the built kernels' resources."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _dxtex_bc1 as B
from _dxtex_snorm import block_texels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "intel-texture-works-plugin_amd", "csrc", "build")
BC1A, BC1A_SRGB = 0x83F1, 0x8C4D


@pytest.fixture(scope="module")
def texels():
    return {name: block_texels(img) for name, img in B.content().items()}


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("bc1a_host_check")
    return B.build_host_check(d), d


def test_content_is_what_the_issue_measured(texels):
    assert texels["boundary"].shape == (1024, 16, 4) and texels["strip"].shape == (256, 16, 4)
    g = B.golden()
    assert len(g) == 2 * len(B.FLAG_SETS) * len(B.ALPHA_REFS)
    plain = g[B.golden_key("boundary", 0.5, 0)].reshape(-1, 8)
    assert int((plain == np.array([0, 0, 255, 255, 255, 255, 255, 255], np.uint8)).all(axis=1).sum()) == 162       # all transparent
    assert int(((plain[:, :2].view("<u2") == plain[:, 2:4].view("<u2")).ravel() & (plain[:, 4:] == 0).all(axis=1)).sum()) == 83   # solid 4-step
    dith = g[B.golden_key("boundary", 0.5, B.DITHER_A)].reshape(-1, 8)
    assert int((dith == np.array([0, 0, 255, 255, 255, 255, 255, 255], np.uint8)).all(axis=1).sum()) == 29


@pytest.mark.parametrize("flags", B.FLAG_SETS, ids=lambda f: "flags_%05x" % f)
def test_model_equals_reference_and_golden(texels, flags):
    g = B.golden()
    for name, tx in texels.items():
        for ref in B.ALPHA_REFS:
            want = g[B.golden_key(name, ref, flags)].reshape(-1, 8)
            got, _ = B.model(tx, ref, flags)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, (name, float(ref), hex(flags), bad[:8], got[bad[:2]], want[bad[:2]])


@pytest.mark.parametrize("flags", B.FLAG_SETS, ids=lambda f: "flags_%05x" % f)
def test_reference_equals_golden(texels, flags):
    g = B.golden()
    for name, tx in texels.items():
        for ref in B.ALPHA_REFS:
            assert np.array_equal(B.encode_blocks(tx, ref, flags), g[B.golden_key(name, ref, flags)].reshape(-1, 8)), (name, float(ref), hex(flags))


@pytest.mark.parametrize("flags", B.FLAG_SETS, ids=lambda f: "flags_%05x" % f)
def test_the_kernels_text_on_the_host_equals_golden(texels, host_check, flags):
    exe, d = host_check
    g = B.golden()
    for name, tx in texels.items():
        for ref in B.ALPHA_REFS:
            got = B.host_check_encode(exe, d, tx, ref, flags)
            want = g[B.golden_key(name, ref, flags)].reshape(-1, 8)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, (name, float(ref), hex(flags), bad[:8])


def test_census_every_branch_of_the_source_is_taken_by_the_shared_content(texels):
    """The GPU comparison cannot pass by never entering a branch: over the content it encodes, flags 0 take every path id, and each dither bit
    takes every branch its dithering adds (alpha_ref 0.5 and the coverage rule's 128/255)."""
    tx = np.concatenate([texels["boundary"], texels["strip"]])
    for ref in (B.ALPHA_REFS[1], B.ALPHA_REFS[2]):
        c = B.census(B.model(tx, ref, 0)[1])
        print("flags 0, alpha_ref", float(ref), c)
        assert set(c) == set(B.PATHS)
        assert all(c[p] >= 1 for p in B.PATHS), c
    c = B.census(B.model(tx, 0.5, B.DITHER_A)[1])
    print("DITHER_A", c)
    assert all(c[p] >= 1 for p in B.DITHER_A_PATHS), c
    c = B.census(B.model(tx, 0.5, B.DITHER_RGB)[1])
    print("DITHER_RGB", c)
    assert all(c[p] >= 1 for p in B.DITHER_RGB_PATHS), c
    c = B.census(B.model(tx, 0.5, B.DITHER_RGB | B.DITHER_A | B.UNIFORM)[1])
    assert all(c[p] >= 1 for p in B.DITHER_A_PATHS + B.DITHER_RGB_PATHS), c


def test_extreme_alpha_refs(texels):
    tx = texels["boundary"]
    assert (B.model(tx, 1.5, 0)[0] == np.array([0, 0, 255, 255, 255, 255, 255, 255], np.uint8)).all()         # > 1: every block transparent
    m, paths = B.model(tx, 0.0, 0)
    assert not paths["steps3"].any() and not paths["all_transparent"].any()                                     # <= 0: no texel transparent
    assert np.array_equal(m, B.model(tx, -3.0, 0)[0])


def test_table_facts(itw):
    L = itw.lib()
    assert C.sizeof(itw.Bc1aSettings) == 16
    s = itw.Bc1aSettings()
    assert (s.struct_size, s.alpha_ref, s.flags, s.reserved) == (16, 0.5, 0, 0)
    assert itw.Bc1aSettings(0.25, True, True, True).flags == 0x70000
    assert np.float32(itw.Bc1aSettings.ref_of(128)) == B.ALPHA_REFS[2]
    for key, code in (("bc1a", BC1A), ("bc1a_srgb", BC1A_SRGB)):
        assert itw.DXGI_FORMAT[key] == code and itw.BYTES_PER_BLOCK[key] == 8 and key in itw.KEEPS_PARTIAL_BLOCKS and itw.OWN_CHANNELS[key] == "rgba"
        assert L.GetBytesPerBlock(code) == 8
        # partial blocks kept: ceil, like BC4
        assert itw.block_count(key, 61, 75) == 16 * 19
        sizes = [(1, 1), (3, 5), (61, 75), (64, 64)]
        assert itw.chain_bytes(key, sizes) == 8 * sum(((h + 3) // 4) * ((w + 3) // 4) for h, w in sizes) == itw.chain_bytes("bc4", sizes)
        # the window of the transfer-bound formats: 262 144 blocks = 16 slices of 4096^2's 64
        assert L.itwSliceWindow(code, 4096, 4096, 0x40000) == 16 == L.itwSliceWindow(80, 4096, 4096, 0x40000)
        assert L.itwSliceWindowFor(code, None, 4096, 4096, 0x40000) == 16
        y0, n, off = itw.band_for_part(61, 75, key, 1, 2)
        assert (y0, n, off) == itw.band_for_part(61, 75, "bc4", 1, 2)


def test_dds_headers_are_those_of_71_and_72(itw):
    rng = np.random.default_rng(3)
    for w, h, mips, cube in ((64, 64, 1, False), (61, 75, 7, False), (16, 16, 5, True)):
        faces = 6 if cube else 1
        levels = [rng.integers(0, 256, ((max(1, w >> l) + 3) // 4) * ((max(1, h >> l) + 3) // 4) * 8, dtype=np.uint8) for _ in range(faces) for l in range(mips)]
        for new, old in (("bc1a", "bc1"), ("bc1a_srgb", "bc1_srgb")):
            a = itw.dds_file(new, w, h, levels, mip_levels=mips, cubemap=cube)
            b = itw.dds_file(old, w, h, levels, mip_levels=mips, cubemap=cube)
            assert np.array_equal(a, b), (new, w, h)
            desc = itw.DdsDesc()
            assert itw.lib().itwDdsReadHeader(a.ctypes.data, a.size, C.byref(desc)) and desc.dxgi_format == itw.DXGI_FORMAT[old]   # read back: 71 / 72
            assert len(itw.dds_images(desc)) == faces * mips


def test_bad_bc1a_calls_return_false_before_any_device_use():
    """The settings rules and the entry points that refuse the format, with nothing written.  Run in a fresh interpreter: the error mode is
    process-wide."""
    code = r"""
import ctypes as C, sys, numpy as np
sys.path.insert(0, %r)
import itw_amd
L = itw_amd.lib()
itw_amd.set_error_mode(itw_amd.ON_ERROR_RETURN)
BC1A = 0x83F1
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
for code_ in (BC1A, 0x8C4D):
    for name, (s, word) in bad.items():
        sp = C.cast(C.byref(s), C.c_void_p)
        for call in ("sliced", "chain", "mipped", "mipped_alpha"):
            L.itwClearError()
            if call == "sliced":
                ok = L.itwCompressImageSlicedEx(C.byref(good), out.ctypes.data, 16, code_, sp, 0, None, None)
            elif call == "chain":
                ok = L.itwCompressImageChainEx(arr(good), 1, out.ctypes.data, code_, sp, None, None)
            elif call == "mipped":
                ok = L.itwCompressImageMipped(arr(good), 1, 0, 0, out.ctypes.data, code_, sp, None, None)
            else:
                a = itw_amd.MipAlpha(0, 128)
                ok = L.itwCompressImageMippedAlpha(arr(good), 1, 0, 0, C.cast(C.byref(a), C.c_void_p), out.ctypes.data, code_, sp, None, None)
            err = itw_amd.last_error()
            assert ok is False and err and word in err, (name, call, ok, err)
            n += 1
# the chain's and the slice call's own argument rules still hold with good settings
ok_s = itw_amd.Bc1aSettings()
okp = C.cast(C.byref(ok_s), C.c_void_p)
for images, count in ((arr(good), 0), (None, 1), (arr(itw_amd.RgbaSurface(None, 8, 8, 32)), 1), (arr(itw_amd.RgbaSurface(img.ctypes.data, 8, 8, 31)), 1)):
    L.itwClearError()
    assert L.itwCompressImageChainEx(images, count, out.ctypes.data, BC1A, okp, None, None) is False and itw_amd.last_error()
L.itwClearError()
assert L.itwCompressImageSlicedEx(C.byref(good), out.ctypes.data, 32, BC1A, None, 0, None, None) is False and "block_row_pitch" in itw_amd.last_error()
# refused: the refined calls, the multi-GPU calls, the normal-map chain calls
rs = itw_amd.RefineStats()
L.itwClearError()
assert L.itwCompressImageRefined(C.byref(good), out.ctypes.data, BC1A, okp, okp, 15, 0, C.addressof(rs), C.sizeof(rs), None, None) is False
assert "one encoder" in itw_amd.last_error()
L.itwClearError()
assert L.itwCompressImageChainRefined(arr(good), 1, out.ctypes.data, BC1A, okp, okp, 15, 0, C.addressof(rs), C.sizeof(rs), None, None, None) is False
assert "one encoder" in itw_amd.last_error()
called = []
fn = itw_amd.abi.COMPRESSION_FUNC(lambda s, o: called.append(1))
L.itwClearError()
assert L.itwCompressImageMultiGPU(C.byref(good), out.ctypes.data, C.cast(fn, C.c_void_p), BC1A, 1) is False and "BC1 with 1-bit alpha" in itw_amd.last_error()
assert not called
L.itwClearError()
assert L.itwCompressNormalMapChain(arr(good), 1, out.ctypes.data, BC1A, None, 4, None, None) is False and "normals" in itw_amd.last_error()
L.itwClearError()
assert L.itwCompressImageMipped(arr(good), 1, 0, 4, out.ctypes.data, BC1A, None, None, None) is False and itw_amd.last_error()
# 74 (BC2) stays a code the library does not encode
L.itwClearError()
assert L.itwCompressImageSlicedEx(C.byref(good), out.ctypes.data, 32, 74, None, 0, None, None) is False and "not one this library encodes" in itw_amd.last_error()
assert (out == 0xA5).all()
print("rejected", n)
""" % os.path.join(ROOT, "intel-texture-works-plugin_amd")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip() == "rejected 64"


def test_every_kernel_variant_uses_no_scratch():
    """Scratch is 0 B for every variant (2 dither bits x 2 load paths): every array of bc1a_core.hpp is indexed by unrolled loop counters."""
    path = os.path.join(BUILD, "bc1a.o")
    if not os.path.exists(path):
        pytest.skip("csrc/build/ is not populated: run __graft_entry__.build() first")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), path, "bc1a_kernel"], check=True, capture_output=True, text=True).stdout
    seen = {}
    for line in out.splitlines():
        import re
        m = re.match(r"(?:void )?itw::(bc1a_kernel<\S+, \S+>)\s+vgpr\s+(\d+) agpr\s+(\d+) .*?scratch\s+(\d+) B\s+lds\s+(\d+) B", line)
        if m:
            seen[m.group(1)] = (int(m.group(2)) + int(m.group(3)), int(m.group(4)), int(m.group(5)))
    want = {"bc1a_kernel<%du, %s>" % (d, v) for d in range(4) for v in ("true", "false")}
    assert set(seen) == want, sorted(seen)
    for name, (regs, scratch, lds) in seen.items():
        assert scratch == 0 and lds == 0, (name, regs, scratch, lds)
        assert 512 // (-(-regs // 8) * 8) >= 2, (name, regs)              # two waves per SIMD, as DESIGN.md 3.13 records
