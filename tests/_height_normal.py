"""The checker of the height-map stage (include/itw_dispatch.h, "height maps": ITW_NORMAL_FROM_HEIGHT): a plain numpy restatement of the
per-texel definition, DirectXTex's ComputeNormalMap (DirectXTexNormalMaps.cpp:22-244).  float32 arrays, one operation per line, so every
operation is rounded on its own; numpy's float32 -> float16 rounds to nearest even.  The flips and the normalise of bits 0..2 come from the
checkers the normal-map stages already have (_normal_prep, _normal_snorm).  Not a test module: tests import it."""
import os

import numpy as np

import _normal_prep as P
import _normal_snorm as S

f32 = np.float32
FROM_HEIGHT, MIRROR_U, MIRROR_V, INVERT_SIGN, OCCLUSION = 0x20, 0x1000, 0x2000, 0x4000, 0x8000
CHANNELS = {"r": 1, "g": 2, "b": 3, "a": 4, "lum": 5}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heightmap_ref.npz")
GOLDEN_SHA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heightmap_ref_sha256.json")


def ops_word(channel=1, mirror_u=False, mirror_v=False, invert=False, occlusion=False, amplitude=1.0, low=0):
    """The `ops` word from its fields, without the binding: channel a number 0..15, amplitude a float that is a half."""
    bits = int(np.array(amplitude, dtype=np.float16).view(np.uint16))
    assert float(np.array(bits, dtype=np.uint16).view(np.float16)) == float(amplitude), "the amplitude must be a half"
    return (low | FROM_HEIGHT | (channel << 8) | (MIRROR_U if mirror_u else 0) | (MIRROR_V if mirror_v else 0) | (INVERT_SIGN if invert else 0)
            | (OCCLUSION if occlusion else 0) | (bits << 16))


def amplitude_of(ops):
    return f32(np.array((ops >> 16) & 0x7FFF, dtype=np.uint16).view(np.float16))


def load(img):
    """(H, W, 4) uint8 codes, int8 codes, float16 / uint16 half bits or float32 -> the float32 components, by the kind's load rule."""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        v = img.astype(f32)
        return v * (f32(1.0) / f32(255.0))
    return S.load(img)


def heights(img, channel):
    """_EvaluateColor over the image: (H, W) float32."""
    v = load(img)
    if channel == 5:
        with np.errstate(all="ignore"):
            r = v[..., 0] * f32(0.2125)
            g = v[..., 1] * f32(0.7154)
            b = v[..., 2] * f32(0.0721)
            s = r + g
            s = s + b
        assert s.dtype == np.float32
        return s
    assert 0 <= channel <= 4
    return np.array(v[..., 0 if channel < 2 else channel - 1], dtype=f32, copy=True)


def _padded(h, mirror_u, mirror_v):
    """The heights with one column and one row more on every side: the opposite edge (wrap) or the edge itself (mirror)."""
    left, right = (h[:, :1], h[:, -1:]) if mirror_u else (h[:, -1:], h[:, :1])
    h = np.concatenate([left, h, right], axis=1)
    top, bottom = (h[:1], h[-1:]) if mirror_v else (h[-1:], h[:1])
    return np.concatenate([top, h, bottom], axis=0)


def normal(img, ops, biased):
    """What the reference hands to its scanline store: (H, W, 4) float32, the encoded normal and alpha.  biased: a UNORM target."""
    amp = amplitude_of(ops)
    p = _padded(heights(img, (ops >> 8) & 15), bool(ops & MIRROR_U), bool(ops & MIRROR_V))
    H, W = p.shape[0] - 2, p.shape[1] - 2
    v = [[p[r:r + H, c:c + W] for c in range(3)] for r in range(3)]        # v[row][column]: rows y - 1, y, y + 1; columns x - 1, x, x + 1
    with np.errstate(all="ignore"):
        a = v[0][0] - v[0][2]
        b = v[1][0] - v[1][2]
        c = v[2][0] - v[2][2]
        t = a + b
        t = t + c
        t = t * amp
        dzx = t / f32(6.0)
        a = v[0][0] - v[2][0]
        b = v[0][1] - v[2][1]
        c = v[0][2] - v[2][2]
        t = a + b
        t = t + c
        t = t * amp
        dzy = t / f32(6.0)
        # cross((-1, 0, dzx), (0, -1, dzy)): six products, three differences
        zero, mone = f32(0.0), f32(-1.0)
        p1 = zero * dzy
        p2 = dzx * mone
        cx = p1 - p2
        p1 = dzx * zero
        p2 = mone * dzy
        cy = p1 - p2
        cz = np.full_like(dzx, mone * mone - zero * zero)
        xx = cx * cx
        yy = cy * cy
        zz = cz * cz
        s = xx + yy
        s = s + zz
        m = np.sqrt(s)
        nx = cx / m
        ny = cy / m
        nz = cz / m
        bad = np.isinf(m)
        nx = np.where(bad, f32(np.nan), nx)
        ny = np.where(bad, f32(np.nan), ny)
        nz = np.where(bad, f32(np.nan), nz)
        alpha = np.ones_like(dzx)
        if ops & OCCLUSION:
            centre = v[1][1]
            delta = np.zeros_like(dzx)
            for r, col in ((0, 0), (0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1), (2, 2)):
                d = v[r][col] - centre
                delta = np.where(d > 0, delta + d, delta)
            k = f32(0.125) * amp
            delta = delta * k
            dd = delta * delta
            dd = f32(1.0) + dd
            root = np.sqrt(dd)
            num = root - delta
            occ = num / root
            alpha = np.where(delta > 0, occ, alpha)
        if biased:
            k = f32(-0.5) if ops & INVERT_SIGN else f32(0.5)
            nx = k * nx
            ny = k * ny
            nz = k * nz
            nx = nx + f32(0.5)
            ny = ny + f32(0.5)
            nz = nz + f32(0.5)
        elif ops & INVERT_SIGN:
            nx, ny, nz = -nx, -ny, -nz
    out = np.stack([nx, ny, nz, alpha], axis=-1)
    assert out.dtype == np.float32
    return out


def store_half(v):
    """float32 -> half bits: NaN -> 0x7E00, clamp to +-65504, round to nearest even."""
    v = np.asarray(v, dtype=f32)
    nan = np.isnan(v)
    c = np.minimum(np.maximum(np.where(nan, f32(0.0), v), f32(-65504.0)), f32(65504.0))
    return np.where(nan, np.uint16(0x7E00), c.astype(np.float16).view(np.uint16)).astype(np.uint16)


def store_unorm8(v):
    """float32 -> biased 8-bit codes: NaN -> 0, clamp to [0, 1], * 255, + 0.5, truncate."""
    v = np.asarray(v, dtype=f32)
    c = np.minimum(np.maximum(np.where(np.isnan(v), f32(0.0), v), f32(0.0)), f32(1.0))
    p = c * f32(255.0)
    p = p + f32(0.5)
    assert p.dtype == np.float32
    return p.astype(np.int32).astype(np.uint8)


def canonical_nan(v):
    """float32 bits with every NaN as 0x7FC00000: which NaN comes out of a divide is the machine's choice."""
    v = np.array(v, dtype=f32, copy=True)
    v[np.isnan(v)] = np.uint32(0x7FC00000).view(f32)
    return v.view(np.uint32)


def to_rgba8(img, ops):
    """itwPrepareNormalMapChain, pixel_size 4: RGBA8 heights -> the biased RGBA8 map, then the flips and the normalise of the convention."""
    return P.prepare_rgba8(store_unorm8(normal(img, ops, True)), ops & 7)


def to_rgba16f(img, ops):
    """itwPrepareNormalMapChain, pixel_size 8: half heights -> half bits."""
    return P.prepare_rgba16f(store_half(normal(img, ops, False)), ops & 7)


def to_snorm(img, ops):
    """itwQuantizeNormalMapChain: int8, half or float heights -> RGBA8_SNORM codes (int8), the signed flips and normalise in fp32."""
    return S.quantize_values(S.apply_ops(normal(img, ops, False), ops & 7))


def to_rgba16f_signed(img, ops):
    """Level 0 of itwCompressSignedNormalMapMipped: the normal in RGBA16F with the flips as negations."""
    v = normal(img, ops, False)
    if ops & 1:
        v[..., 0] = -v[..., 0]
    if ops & 2:
        v[..., 1] = -v[..., 1]
    return store_half(v)


# ---- the recorded reference cases (tools/make_heightmap_golden.py writes them; the tests read them) ------------------------------------------
GOLDEN_SIZES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 5), (7, 5), (16, 16), (65, 17), (130, 33)]           # (width, height)
GOLDEN_AMPLITUDES = [1.0, 0.5, 2.0, 8.0, 100.0, 0.0999755859375]
GOLDEN_CONTENTS = ("noise", "flat", "ramp", "checker", "naninf")
GOLDEN_STORED = 600          # texels up to which a case's arrays are in the npz; above, their SHA-256 only


def golden_input(kind, what, h, w, seed):
    """(h, w, 4) heights of kind "half" (uint16 bits) or "float": seeded noise in [0, 1), a flat image, a ramp, a 0 / 1 checkerboard, or the
    noise with a NaN, a +Inf and a -Inf height (as far as the image has texels for them)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if what == "flat":
        v = np.broadcast_to(np.array([0.5, 0.25, 0.75, 1.0], f32), (h, w, 4))
    elif what == "ramp":
        v = np.stack([(xx * (k + 1) + yy * 2) / f32(8.0) for k in range(4)], axis=-1)
    elif what == "checker":
        v = np.stack([((xx + yy + k) & 1) for k in range(4)], axis=-1)
    else:
        v = rng.random((h, w, 4), dtype=f32)
    v = np.array(v, dtype=f32, copy=True)
    if what == "naninf":
        flat = v.reshape(-1, 4)
        for i, bad in zip(rng.permutation(h * w)[:3], (np.nan, np.inf, -np.inf)):
            flat[i, :] = bad
    return np.ascontiguousarray(v.astype(np.float16).view(np.uint16) if kind == "half" else v)


def golden_cases():
    """Every recorded case as a dict: src "half" / "float", content, width, height, seed, ops.  Every size under both source kinds and the
    four mirror combinations with the other fields rotating; all six channel values; all amplitudes; every content."""
    cases, n = [], 0

    def add(src, what, w, h, **fields):
        nonlocal n
        n += 1
        cases.append({"src": src, "content": what, "width": w, "height": h, "seed": 700 + len(cases), "ops": ops_word(**fields)})

    for w, h in GOLDEN_SIZES:
        for src in ("float", "half"):
            for m in range(4):
                add(src, "noise", w, h, channel=n % 6, mirror_u=bool(m & 1), mirror_v=bool(m & 2), invert=n % 3 == 0, occlusion=n % 2 == 0,
                    amplitude=GOLDEN_AMPLITUDES[n % 6])
    for w, h in ((7, 5), (16, 16)):
        for src in ("float", "half") if w == 7 else ("float",):
            for channel in range(6):
                add(src, "noise", w, h, channel=channel)
            for what in GOLDEN_CONTENTS[1:]:
                add(src, what, w, h, channel=5 if what == "naninf" else 2, occlusion=True, invert=what == "checker", mirror_u=what == "ramp")
                add(src, what, w, h, channel=1, amplitude=8.0, mirror_v=what == "ramp")
    for src in ("float", "half"):
        for amplitude in GOLDEN_AMPLITUDES:
            add(src, "noise", 7, 5, channel=3, occlusion=True, amplitude=amplitude)
            add(src, "noise", 7, 5, channel=4, invert=True, amplitude=amplitude)
    return cases


def golden_name(c):
    return f"{c['src']}_{c['content']}_{c['width']}x{c['height']}_s{c['seed']}_{c['ops']:08x}"


def golden_skips_row0(c):
    """The stated divergence: under MIRROR_V the reference's row above row 0 is a partial copy for a source narrower than RGBA32F, so
    row 0 of such a case is compared with the model alone."""
    return c["src"] == "half" and bool(c["ops"] & MIRROR_V)


# ---- seeded content the tests share --------------------------------------------------------------------------------------------------------
_content = {}


def content(kind, h, w, seed):
    """(h, w, 4) heights of the kind "uint8", "int8", "half" or "float": smooth bumps plus noise, every channel different."""
    key = (kind, h, w, seed)
    if key not in _content:
        rng = np.random.default_rng(seed)
        yy, xx = np.mgrid[0:h, 0:w].astype(f32)
        base = np.stack([np.sin(xx * f32(0.7) + k) * np.cos(yy * f32(0.45) - k) for k in range(4)], axis=-1).astype(f32)
        v = (base * f32(0.4) + rng.normal(0, 0.15, (h, w, 4)).astype(f32)).astype(f32)
        if kind == "uint8":
            a = np.clip(np.rint((v * f32(0.5) + f32(0.5)) * 255), 0, 255).astype(np.uint8)
        elif kind == "int8":
            a = np.clip(np.rint(v * 127), -128, 127).astype(np.int8)
        elif kind == "half":
            a = v.astype(np.float16).view(np.uint16)
        else:
            a = v
        _content[key] = np.ascontiguousarray(a)
    return _content[key]
