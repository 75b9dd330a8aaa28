"""ETC1 without a GPU: the two entry points exist where include/itw_amd.h says, the preset and the refusals work before any device is
touched, the golden file is what the reference library produces today, and the numpy decoder the GPU tests compare against (tests/_etc1.py)
decodes hand-worked blocks and the golden streams as the format's definition says."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _etc1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return _etc1.load_golden()


# ---- the boundary ---------------------------------------------------------------------------------------------------------------------------
def test_both_symbols_are_exported_declared_and_listed(itw):
    header = open(os.path.join(ROOT, "include", "itw_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("itwGetProfile_etc_slow", "itwCompressBlocksETC1"):
        assert hasattr(itw.lib(), name), name
        assert name in itw.EXPORTED_SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert "struct etc_enc_settings" in open(os.path.join(ROOT, "include", "ispc_texcomp.h")).read()


def test_settings_struct_is_four_bytes(itw):
    assert C.sizeof(itw.EtcSettings) == 4
    assert itw.EtcSettings.fastSkipTreshold.offset == 0
    assert itw.BYTES_PER_BLOCK["etc1"] == 8 and itw.DXGI_FORMAT["etc1"] == _etc1.ETC1 == 0x8D64


def test_profile_writes_what_the_reference_writes(itw):
    ref = _etc1.live_reference()
    ours = (C.c_uint8 * 16)(*([0xA5] * 16))
    theirs = (C.c_uint8 * 16)(*([0xA5] * 16))
    itw.lib().itwGetProfile_etc_slow(C.cast(ours, C.POINTER(itw.EtcSettings)))
    ref.GetProfile_etc_slow(C.cast(theirs, C.c_void_p))
    assert bytes(ours) == bytes(theirs)
    assert bytes(ours)[4:] == b"\xa5" * 12                      # four bytes written, no more


def test_slow_profile_is_six(itw):
    assert itw.etc_profile("slow").fastSkipTreshold == 6
    with pytest.raises(KeyError):
        itw.etc_profile("fast")


@pytest.fixture
def return_mode(itw):
    itw.set_error_mode(itw.ON_ERROR_RETURN)
    yield
    itw.lib().itwClearError()
    itw.set_error_mode(itw.ON_ERROR_ABORT)


@pytest.mark.parametrize("case", ["threshold 0", "threshold -1", "null settings", "null surface", "null texels", "null destination"])
def test_bad_calls_return_with_a_message_and_leave_the_output_alone(itw, return_mode, case):
    img = _etc1.ramp()[:8, :8].copy()
    out = np.full(4 * 8 + 16, 0x5A, dtype=np.uint8)
    surf = itw.RgbaSurface(img.ctypes.data, 8, 8, 32)
    st = itw.EtcSettings(6)
    args = [C.byref(surf), out.ctypes.data, C.byref(st)]
    if case.startswith("threshold"):
        st.fastSkipTreshold = int(case.split()[1])
    elif case == "null settings":
        args[2] = None
    elif case == "null surface":
        args[0] = None
    elif case == "null texels":
        surf.ptr = None
    else:
        args[1] = None
    itw.lib().itwCompressBlocksETC1(*args)
    assert itw.last_error(), case
    assert (out == 0x5A).all(), case


# ---- the golden file ------------------------------------------------------------------------------------------------------------------------
def test_golden_file_holds_the_inputs_and_eight_streams(golden):
    """The ramp itself, the noise input as its SHA-256 (16 KiB of random bytes: _etc1.load_golden regenerates and checks it), eight streams."""
    raw = dict(np.load(_etc1.GOLDEN))
    assert np.array_equal(raw["ramp"], _etc1.ramp()) and "noise" not in raw
    assert str(raw["noise.sha256"]) == _etc1.sha256(_etc1.noise()) and np.array_equal(golden["noise"], _etc1.noise())
    for name in ("noise", "ramp"):
        for t in _etc1.GOLDEN_THRESHOLDS:
            assert golden[f"{name}.t{t}"].shape == (2048,) and golden[f"{name}.t{t}"].dtype == np.uint8
    assert os.path.getsize(_etc1.GOLDEN) < 40 * 1000


def test_live_reference_reproduces_the_golden_file(golden):
    _etc1.live_reference()
    for name in ("noise", "ramp"):
        for t in _etc1.GOLDEN_THRESHOLDS:
            assert np.array_equal(_etc1.ref_stream(name, t), golden[f"{name}.t{t}"]), (name, t)


def test_reference_is_deterministic_and_ignores_alpha():
    _etc1.live_reference()
    img = _etc1.ramp().copy()
    img[..., 3] = _etc1.noise()[..., 3]
    assert np.array_equal(_etc1.ref_encode(img, 6), _etc1.ref_stream("ramp", 6))


def test_golden_streams_cover_every_path(golden):
    """What the parity tests rely on: both flips x both base encodings, every table in both halves, and second halves clamped at -4 / +3."""
    both = _etc1.coverage([golden["noise.t6"], golden["ramp.t6"]])
    assert both["pairs"] == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert both["table0"] == set(range(8)) and both["table1"] == set(range(8))
    r = _etc1.coverage([golden["ramp.t6"]])
    assert (r["differential"], r["clamped"]) == (168, 72), r         # exact: seeded inputs, pinned reference (the issue's own draw: 63 of 168)


def test_numpy_decoder_reproduces_the_inputs_at_the_stored_psnr(golden):
    for name in ("noise", "ramp"):
        last = 0.0
        for t in _etc1.GOLDEN_THRESHOLDS:
            texels, modes = _etc1.decode_np(golden[f"{name}.t{t}"], 64, 64)
            assert (modes >= 0).all() and (texels[..., 3] == 255).all()
            got = _etc1.psnr_rgb(texels, golden[name])
            assert abs(got - float(golden[f"{name}.t{t}.psnr"])) < 0.01, (name, t, got)
            assert got >= last - 0.01                           # more candidates never hurt by more than the quantised tie-breaks
            last = got


# ---- the kernel's arithmetic, on the host -----------------------------------------------------------------------------------------------------
def test_kernel_arithmetic_on_the_host_matches_the_reference(tmp_path):
    """csrc/etc1_core.hpp -- the text the kernel is built from -- walked lane after lane by tools/etc1_host_check.cpp against the reference
    library: 3 584 blocks of four kinds of content at thresholds 1, 2, 6 and 32.  What no GPU is needed for: division sites, clamps,
    tie-breaks, bit packing."""
    import subprocess
    _etc1.live_reference()
    exe = str(tmp_path / "etc1_host_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle"),
                    os.path.join(ROOT, "tools", "etc1_host_check.cpp"), "-ldl", "-o", exe], check=True)
    run = subprocess.run([exe, _etc1.ref_path(), "16"], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("ok"), (run.stdout[-400:], run.stderr[-400:])
    assert run.stdout.count(": 0 of 256 blocks differ") == 14


# ---- the numpy decoder against blocks worked by hand --------------------------------------------------------------------------------------
def _block(b0, b1, b2, table0, table1, diff, flip, msb, lsb):
    return np.array([b0, b1, b2, (table0 << 5) | (table1 << 2) | (diff << 1) | flip, msb >> 8, msb & 255, lsb >> 8, lsb & 255], dtype=np.uint8)


def test_decoder_individual_flip0():
    # bases (1, 2, 3) x 17 left, (14, 13, 12) x 17 right; table 0 (2, 8) left, table 7 (47, 183) right; every selector 0 = +small
    t, m = _etc1.decode_np(_block(0x1E, 0x2D, 0x3C, 0, 7, 0, 0, 0, 0), 4, 4)
    assert m.tolist() == [0]
    assert (t[:, :2, :3] == [17 + 2, 34 + 2, 51 + 2]).all()
    assert (t[:, 2:, :3] == [238 + 47 - 30, 221 + 47 - 13, 204 + 47]).all() and (t[:, 2:, 0] == 255).all()     # 285, 268 clamp to 255
    assert (t[..., 3] == 255).all()


def test_decoder_individual_flip1_and_every_selector():
    # texel (x, y) is bit x * 4 + y: (0,0) +small, (0,1) +large, (0,2) -small, (0,3) -large with msb 0b1100, lsb 0b1010
    t, m = _etc1.decode_np(_block(0x88, 0x88, 0x88, 2, 3, 0, 1, 0b1100, 0b1010), 4, 4)
    assert m.tolist() == [0]
    assert t[0, 0, :3].tolist() == [136 + 9] * 3 and t[1, 0, :3].tolist() == [136 + 29] * 3      # rows 0-1: table 2 (9, 29)
    assert t[2, 0, :3].tolist() == [136 - 13] * 3 and t[3, 0, :3].tolist() == [136 - 42] * 3     # rows 2-3: table 3 (13, 42)
    assert (t[:2, 1:, :3] == 136 + 9).all() and (t[2:, 1:, :3] == 136 + 13).all()


def test_decoder_differential_with_negative_delta_and_clamp_at_zero():
    # R: base 2, delta -2 -> 0; G: base 31, delta 0; B: base 16, delta +3 -> 19.  Table 7, every selector 3 = -large (-183)
    t, m = _etc1.decode_np(_block((2 << 3) | 6, (31 << 3) | 0, (16 << 3) | 3, 7, 7, 1, 0, 0xFFFF, 0xFFFF), 4, 4)
    assert m.tolist() == [1]
    assert (t[:, :2, :3] == [0, 255 - 183, 0]).all()            # (16, 255, 132) - 183
    assert (t[:, 2:, :3] == [0, 255 - 183, 0]).all()            # (0, 255, 156) - 183
    t, m = _etc1.decode_np(_block((2 << 3) | 6, (31 << 3) | 0, (16 << 3) | 3, 0, 0, 1, 1, 0, 0), 4, 4)      # flip 1, +2
    assert (t[:2, :, :3] == [16 + 2, 255, 132 + 2]).all() and (t[2:, :, :3] == [0 + 2, 255, 156 + 2]).all()


def test_decoder_overflowing_differential_block_is_mode_minus_one():
    # R: base 30, delta +3 -> 33 = 1 modulo 32; G: base 1, delta -4 -> -3 = 29 modulo 32; B in range
    t, m = _etc1.decode_np(_block((30 << 3) | 3, (1 << 3) | 4, (10 << 3) | 0, 0, 0, 1, 0, 0, 0), 4, 4)
    assert m.tolist() == [-1]
    assert (t[:, :2, :3] == [247 + 2, 8 + 2, 82 + 2]).all()
    assert (t[:, 2:, :3] == [8 + 2, 239 + 2, 82 + 2]).all()     # 1 -> 8, 29 -> 239


def test_decoder_block_order_is_raster():
    a = _block(0x00, 0x00, 0x00, 0, 0, 0, 0, 0, 0)
    b = _block(0xFF, 0xFF, 0xFF, 0, 0, 0, 0, 0xFFFF, 0)          # every selector 2 = -small
    t, _ = _etc1.decode_np(np.concatenate([a, b, b, a]), 8, 8)
    assert (t[:4, :4, :3] == 2).all() and (t[:4, 4:, :3] == 253).all() and (t[4:, :4, :3] == 253).all() and (t[4:, 4:, :3] == 2).all()
