"""The encode host layer's format and geometry facts as seen from outside the library (no GPU needed): the slice window of the pipelined
slice loop, and the three entry points that restate "bytes per block" and "this format keeps partial blocks".  Every figure below is a
restatement of the rule in Python, never something read back from the library."""
import ctypes as C
import os

import pytest

# every format code the library encodes: BC1 / BC1_SRGB, BC3 / BC3_SRGB, BC4 U/S, BC5 U/S, BC6H UF16/SF16, BC7 / BC7_SRGB, ETC1 (its GL enum)
CODES = (71, 72, 77, 78, 80, 81, 83, 84, 95, 96, 98, 99, 0x8D64)
KEEP_PARTIAL = (80, 81, 83, 84)                        # the DirectXTex formats: blocks round up
COMPUTE_BOUND = (95, 96, 98, 99, 0x8D64)               # windows of 131 072 blocks; the others (PCIe-bound) 262 144
SIXTEEN_BYTES = (77, 78, 83, 84, 95, 96, 98, 99)       # bytes per block: 16; the others 8
SIZES = ((64, 64), (255, 257), (1024, 1024), (2048, 2050), (4096, 4096), (16384, 16384))
SLICE_PIXELS = (0, 4096, 0x40000, 1 << 20)
SCAN_EVERY_SHAPE = ("slow", "alpha_slow")              # the BC7 profiles whose modes 1/3 scan all 64 shapes (fastSkipTreshold 64)


def _window(code, heavy, w, h, slice_pixels):
    sp = slice_pixels if slice_pixels > 0 else 0x40000
    slices = min(max(1, (w * h) // sp), 1 << 24)
    blocks = ((w + 3) // 4) * ((h + 3) // 4) if code in KEEP_PARTIAL else (w // 4) * (h // 4)
    target = 131072 if (code in COMPUTE_BOUND and not heavy) else 262144
    per = max(1, blocks // slices)
    return min(max((target + per // 2) // per, 1), slices)


def test_slice_window_for_every_format_size_and_slice_size(itw):
    if "ITW_SLICE_WINDOW" in os.environ or os.environ.get("ITW_SLICED_PIPELINE") == "0":
        pytest.skip("the environment presets the window")
    L = itw.lib()
    etc = itw.etc_profile("slow")
    cases = []                                          # (code, settings object or None, heavy, label)
    for code in CODES:
        cases.append((code, None, False, "null"))
        if code in (98, 99):
            cases += [(code, itw.bc7_profile(p), p in SCAN_EVERY_SHAPE, p) for p in itw.BC7_PROFILES]
        if code == 0x8D64:
            cases.append((code, etc, False, "etc settings"))
    assert len(itw.BC7_PROFILES) == 10
    for code, st, heavy, label in cases:
        sp_arg = C.cast(C.byref(st), C.c_void_p) if st is not None else None
        for w, h in SIZES:
            for sp in SLICE_PIXELS:
                got = L.itwSliceWindowFor(code, sp_arg, w, h, sp)
                assert got == _window(code, heavy, w, h, sp), (code, label, w, h, sp, got)
                if st is None:
                    assert L.itwSliceWindow(code, w, h, sp) == got, (code, w, h, sp)


THRESHOLDS = (0, 1, 16, 17, 63, 64, 70)               # off, ranked (short, 16, long, longest), every shape, beyond


def test_slice_window_follows_the_scans_every_shape_rule_for_any_bc7_settings(itw):
    """the one BC7 route predicate reachable without a device: a BC7 call is `heavy` -- its window half as many slices' worth -- exactly when
    modes 0/2 are on, modes 1/3 are on with a positive list length, and neither list is a proper prefix of the ranking (1..63)"""
    if "ITW_SLICE_WINDOW" in os.environ or os.environ.get("ITW_SLICED_PIPELINE") == "0" or os.environ.get("ITW_BC7_BOUND", "1")[:1] == "0":
        pytest.skip("the environment presets the window or the mode order")
    L = itw.lib()
    ranked = lambda t: 1 <= t <= 63
    seen = set()
    for bits in range(16):
        for channels in (3, 4):
            for t1 in THRESHOLDS:
                for t3 in THRESHOLDS:
                    for t7 in THRESHOLDS:
                        s = itw.bc7_profile("slow")
                        for i in range(4):
                            s.mode_selection[i] = bool(bits >> i & 1)
                        s.fastSkipTreshold_mode1, s.fastSkipTreshold_mode3, s.fastSkipTreshold_mode7, s.channels = t1, t3, t7, channels
                        heavy = bool(bits & 1) and bool(bits & 2) and (t1 > 0 or t3 > 0) and not ranked(t1) and not ranked(t3)
                        seen.add(heavy)
                        for code, w, h, sp in ((98, 4096, 4096, 4096), (99, 2048, 2050, 0)):
                            got = L.itwSliceWindowFor(code, C.cast(C.byref(s), C.c_void_p), w, h, sp)
                            assert got == _window(code, heavy, w, h, sp), (bits, channels, t1, t3, t7, code, got)
    assert seen == {False, True}
    assert _window(98, True, 4096, 4096, 4096) != _window(98, False, 4096, 4096, 4096)      # the sweep's sizes tell the two apart
    assert _window(99, True, 2048, 2050, 0) != _window(99, False, 2048, 2050, 0)


def test_bytes_per_block_chain_bytes_and_bands_agree_with_the_table(itw):
    L = itw.lib()
    for code in CODES:
        bpb = 16 if code in SIXTEEN_BYTES else 8
        keep = code in KEEP_PARTIAL
        assert L.GetBytesPerBlock(code) == bpb, code
        for w in range(1, 10):
            for h in range(1, 10):
                surf = (itw.RgbaSurface * 1)(itw.RgbaSurface(None, w, h, 0))
                # a chain pads every image to whole blocks, whatever the format
                assert L.itwChainBytes(C.cast(surf, C.c_void_p), 1, code) == ((w + 3) // 4) * ((h + 3) // 4) * bpb, (code, w, h)
                # the whole surface as the last of two bands: offset = the first band's block rows, rows = the rest, partial rows kept or dropped
                bx, rows = ((w + 3) // 4, (h + 3) // 4) if keep else (w // 4, h // 4)
                y0, n = C.c_int32(-1), C.c_int32(-1)
                off = L.itwBandForPartEx(w, h, L.GetBytesPerBlock(code), 1, 2, 1 if keep else 0, C.byref(y0), C.byref(n))
                r0 = rows // 2
                assert off == r0 * bx * bpb and y0.value == r0 * 4, (code, w, h, off, y0.value)
                assert n.value == ((min(rows * 4, h) - r0 * 4) if keep else (rows - r0) * 4), (code, w, h, n.value)
                # one band = the surface: nothing before it, every kept row
                assert L.itwBandForPartEx(w, h, bpb, 0, 1, 1 if keep else 0, C.byref(y0), C.byref(n)) == 0
                assert (y0.value, n.value) == (0, h if keep else rows * 4), (code, w, h)
    assert L.GetBytesPerBlock(0) == 8 and L.GetBytesPerBlock(12345) == 8          # the reference's "unknown -> 8"
    surf = (itw.RgbaSurface * 1)(itw.RgbaSurface(None, 4, 4, 0))
    assert L.itwChainBytes(C.cast(surf, C.c_void_p), 1, 12345) == -1
