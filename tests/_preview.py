"""The preview viewport (include/itw_decode.h: itwPreviewBlocks, itwPreviewSurface) restated in numpy, one operation per line: what
IntelPlugin::FetchPreviewRGB (IntelPlugin.cpp:487-739) computes for an RGBA8 or an RGBA16F image.  Integer and IEEE arithmetic only, so
every comparison against it is ==.  tests/test_preview_cpu.py checks this module against literals typed in from the reference's text."""
import numpy as np

RED, GREEN, BLUE, ALPHA, MASK = 0x04, 0x08, 0x10, 0x20, 0x3C      # PREVIEW_CHANNEL_*, IntelPlugin.h:248-261
NONE = -1


def channel_table(options):
    """([channel of byte 0, of byte 1, of byte 2], alpha alone): 0 .. 3, or NONE for a byte that shows 0 (:585-624 with planes = 4)."""
    m = options & MASK
    if m == 0:
        m = RED | GREEN | BLUE
    if m == RED:
        return [0, 0, 0], False
    if m == GREEN:
        return [1, 1, 1], False
    if m == BLUE:
        return [2, 2, 2], False
    if m == ALPHA:
        return [3, 3, 3], True
    ch = [NONE, NONE, NONE]
    if m & RED:
        ch[0] = 0
    if m & GREEN:
        ch[1] = 1
    if m & BLUE:
        ch[2] = 2
    if m & ALPHA:
        ch[2] = 3                                                # channelIndex[2] = 3, whether or not blue is set (:610-611)
    return ch, False


def coords(n_view, offset, zoom, n_source):
    """(inside, x) for viewport coordinates 0 .. n_view - 1: x = int((t + offset) * zoom), outside when the product is <= -1 or >= n_source."""
    t = np.arange(n_view, dtype=np.int64) + np.int64(offset)
    f = t.astype(np.float64) * np.float64(zoom)                  # one double multiply
    inside = (f > -1.0) & (f < np.float64(n_source))             # compared before the conversion
    x = np.trunc(np.where(inside, f, 0.0)).astype(np.int64)      # toward zero: -1 < f < 0 gives 0
    return inside, x


def float_to_byte(half_bits, exposure):
    """FloatToByte(F16toF32(h) * exposure) (IntelPlugin.h:41-48, IntelPlugin.cpp:676-678) for uint16 half patterns."""
    with np.errstate(all="ignore"):
        v = np.asarray(half_bits, dtype=np.uint16).view(np.float16).astype(np.float32) * np.float32(exposure)      # one fp32 multiply
        d = v.astype(np.float64)
        scaled = d * np.float64(255.0)                           # the product in double: exact, v has 24 significant bits
        middle = np.trunc(np.where((d >= 0.0) & (d <= 1.0), scaled, 0.0)).astype(np.uint8)
        out = np.where(d > 1.0, np.uint8(255), middle)
        out = np.where(d < 0.0, np.uint8(0), out)
        return np.where(np.isnan(d), np.uint8(0), out).astype(np.uint8)


def viewport(image, view_w, view_h, x_offset=0, y_offset=0, zoom=1.0, options=0, matte=0, exposure=1.0):
    """The (view_h, view_w, 3) uint8 viewport of `image`: (H, W, 4) uint8 RGBA8 codes, or (H, W, 4) uint16 RGBA16F bit patterns."""
    H, W = image.shape[:2]
    in_y, y = coords(view_h, y_offset, zoom, H)
    in_x, x = coords(view_w, x_offset, zoom, W)
    inside = in_y[:, None] & in_x[None, :]
    texels = image[y[:, None], x[None, :]]                       # (view_h, view_w, 4); outside pixels read texel (0, 0) and are overwritten
    ch, alpha_alone = channel_table(options)
    if alpha_alone:
        exposure = 1.0
    out = np.zeros((view_h, view_w, 3), dtype=np.uint8)
    for b in range(3):
        if ch[b] == NONE:
            continue
        code = texels[..., ch[b]]
        out[..., b] = code if image.dtype == np.uint8 else float_to_byte(code, exposure)
    matte_bytes = np.array([matte & 0xFF, (matte >> 8) & 0xFF, (matte >> 16) & 0xFF], dtype=np.uint8)
    out[~inside] = matte_bytes
    return out
