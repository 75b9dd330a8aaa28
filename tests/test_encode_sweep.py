"""tests/_encode_sweep.py on the CPU: the sources do what they are for.  Counted on the ORACLE's streams, never the device's: under `alpha_slow`
the BC7 source makes every one of the 285 (mode, partition / rotation + index selector) combinations win blocks, under `slow` and `veryslow` the
BC6H source every one of the 324 (mode, partition) pairs; the combinations the earlier content never emitted are listed and found.  The number of
combinations per preset and per settings struct, and a SHA-256 of each source, are pinned in tests/golden/encode_sweep_counts.json (written by
`python tests/test_encode_sweep.py --write`, read back with `==`): a change of seed, construction or decoder shows as a diff there, not as
silently different coverage in tests/test_gpu_encode_sweep.py, which asserts the same counts before it compares."""
import collections
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import _encode_sweep as es

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINS = os.path.join(ROOT, "tests", "golden", "encode_sweep_counts.json")
BC7_PRESETS = ["ultrafast", "veryfast", "fast", "basic", "slow", "alpha_ultrafast", "alpha_veryfast", "alpha_fast", "alpha_basic", "alpha_slow"]
BC6H_PRESETS = ["veryfast", "fast", "basic", "slow", "veryslow"]
COMBINATION = {"bc7": es.bc7_combination, "bc6h": es.bc6h_combination}
_streams = {}


def pins():
    with open(PINS) as f:
        return json.load(f)


def source(fmt):
    return es.bc7_source() if fmt == "bc7" else es.bc6h_source()


def settings_of(module, fmt, name):
    """A preset's name as it is, or the struct of a variant of _encode_sweep, from `module` (the oracle or the product: same interface)."""
    variants = es.BC7_VARIANTS if fmt == "bc7" else es.BC6H_VARIANTS
    if name not in variants:
        return name
    base, tweak = variants[name]
    return es.apply(getattr(module, fmt + "_profile")(base), tweak)


def oracle_stream(oracle, fmt, name):
    """The oracle's blocks of the format's source under a preset or a variant: encoded once per process, read-only."""
    if (fmt, name) not in _streams:
        blocks = oracle.encode_mt(fmt, source(fmt), settings_of(oracle, fmt, name))
        blocks.setflags(write=False)
        _streams[(fmt, name)] = blocks
    return _streams[(fmt, name)]


def emitted(oracle, fmt, name):
    """Counter of the combinations in oracle_stream()."""
    return collections.Counter(COMBINATION[fmt](oracle_stream(oracle, fmt, name)))


def sha256(img):
    return hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest()


def measured(oracle):
    """Everything the JSON pins, recomputed."""
    out = {"sha256": {"bc7": sha256(es.bc7_source()), "bc6h": sha256(es.bc6h_source())}, "shape": {}, "combinations": {}, "golden_streams": {}}
    out["sha256"].update({fmt: sha256(img) for fmt, img in es.small_sources().items()})
    out["shape"] = {"bc7": list(es.bc7_source().shape), "bc6h": list(es.bc6h_source().shape)}
    for fmt, names in (("bc7", BC7_PRESETS + list(es.BC7_VARIANTS)), ("bc6h", BC6H_PRESETS + list(es.BC6H_VARIANTS))):
        out["combinations"][fmt] = {name: len(emitted(oracle, fmt, name)) for name in names}
    gold = dict(np.load(os.path.join(ROOT, "tests", "golden", "golden_blocks.npz")))
    for fmt in ("bc7", "bc6h"):
        out["golden_streams"][fmt] = len(golden_combinations(gold, fmt))
    return out


def golden_combinations(golden_blocks, fmt):
    """What the committed encoder streams of the format hold, every image and preset together."""
    seen = set()
    for key, blocks in golden_blocks.items():
        if f".{fmt}." in key:
            seen |= set(COMBINATION[fmt](blocks))
    return seen


# ---- the conditions --------------------------------------------------------------------------------------------------------------------

def test_sources_have_the_stated_geometry():
    s7, s6 = es.bc7_source(), es.bc6h_source()
    assert s7.dtype == np.uint8 and s7.shape == (288, 256, 4) and s7.flags["C_CONTIGUOUS"]      # 4 608 blocks, 285 x 16 of them drawn
    assert s6.dtype == np.uint16 and s6.shape == (772, 256, 4) and s6.flags["C_CONTIGUOUS"]     # 12 352 = 324 x 16 + 28 x 32 x 8
    assert (s6[..., 3] == 0x3C00).all() and int(s6[..., :3].max()) <= 0x7BFF
    assert len(es.bc7_words()) == es.BC7_COMBINATIONS * es.PAYLOADS and len(es.bc6h_words()) == es.BC6H_COMBINATIONS * es.PAYLOADS + 28 * 32 * 8
    assert len({w for _, _, w in es.bc7_words()}) == len(es.bc7_words())                        # all different
    small = es.small_sources()
    assert {k: v.shape for k, v in small.items()} == {"bc1": (500, 500, 4), "bc3": (500, 500, 4), "bc4": (1024, 1024, 4), "bc5": (1024, 1024, 4)}


def test_combination_readers_read_what_the_construction_wrote():
    """the words the sources were decoded from carry their (mode, field) by construction; the readers find it from the bytes"""
    import _block_sweep as sweep
    words = es.bc7_words()
    assert es.bc7_combination(sweep._pack([w for _, _, w in words])) == [(m, v) for m, v, _ in words]
    assert set(es.bc7_combination(sweep._pack([w for _, _, w in words]))) == es.all_bc7_combinations() and len(es.all_bc7_combinations()) == 285
    words = es.bc6h_words()
    assert es.bc6h_combination(sweep._pack([w for _, _, w in words])) == [(m, p) for m, p, _ in words]
    assert {(m, p) for m, p, _ in words} == es.all_bc6h_combinations() and len(es.all_bc6h_combinations()) == 324
    assert es.bc7_combination(np.zeros(16, np.uint8)) == [(-1, 0)] and es.bc6h_combination(np.full(16, 0x13, np.uint8)) == [(-1, 0)]


def test_bc7_alpha_slow_emits_all_285_combinations_at_least_four_times(oracle):
    got = emitted(oracle, "bc7", "alpha_slow")
    print("bc7 alpha_slow:", len(got), "of 285, fewest blocks per combination:", min(got.values()))
    assert set(got) == es.all_bc7_combinations() and len(got) == 285
    assert min(got.values()) >= 4, [k for k, n in got.items() if n < 4]


@pytest.mark.parametrize("prof", ["slow", "veryslow"])
def test_bc6h_slow_emits_all_324_combinations(oracle, prof):
    got = emitted(oracle, "bc6h", prof)
    print("bc6h", prof + ":", len(got), "of 324, fewest blocks per combination:", min(got.values()))
    assert set(got) == es.all_bc6h_combinations() and len(got) == 324


def test_counts_and_hashes_are_the_pinned_ones(oracle):
    want, got = pins(), measured(oracle)
    for section in got:
        assert got[section] == want[section], section
    assert set(want) == set(got) | {"synthetic_surfaces"}
    c7, c6 = want["combinations"]["bc7"], want["combinations"]["bc6h"]
    assert c7["alpha_slow"] == 285 and c6["slow"] == c6["veryslow"] == 324


def test_the_combinations_earlier_content_never_emitted_are_emitted_now(oracle, golden_blocks):
    """the committed encoder streams (every preset of monkey, baboon, edge_cases; the HDR images) -- what the parity tests compare against --
    hold 269 of 285 and 242 of 324; each missing combination wins blocks of the sweep"""
    for fmt, every, prof, held in (("bc7", es.all_bc7_combinations(), "alpha_slow", 269), ("bc6h", es.all_bc6h_combinations(), "slow", 242)):
        old = golden_combinations(golden_blocks, fmt) & every
        never = sorted(every - old)
        per_mode = collections.Counter(m for m, _ in never)
        print(fmt, "golden streams:", len(old), "of", len(every), "; never emitted:", never, "; per mode:", dict(sorted(per_mode.items())))
        assert len(old) == held
        now = emitted(oracle, fmt, prof)
        assert all(now[c] >= 1 for c in never), [c for c in never if not now[c]]


def test_synthetic_surfaces_of_the_parity_tests_leave_combinations_out(oracle):
    """the other content of the GPU parity tests, for the record in DESIGN.md section 5: smooth fields and random bits at 256 x 256"""
    got = synthetic_surface_counts(oracle)
    print("ldr_smooth 256^2, slow + alpha_slow + basic:", got["bc7"], "of 285; hdr_smooth + hdr_random_bits 256^2, slow:", got["bc6h"], "of 324")
    assert got == pins()["synthetic_surfaces"]
    assert got["bc7"] < 285 and got["bc6h"] < 324


def synthetic_surface_counts(oracle):
    from itw_amd import surfaces
    ldr = surfaces.ldr_smooth(256, 256)
    seen7, seen6 = set(), set()
    for prof in ("slow", "alpha_slow", "basic"):
        seen7 |= set(es.bc7_combination(oracle.encode_mt("bc7", ldr, prof)))
    for gen in (surfaces.hdr_smooth, surfaces.hdr_random_bits):
        seen6 |= set(es.bc6h_combination(oracle.encode_mt("bc6h", gen(256, 256), "slow")))
    return {"bc7": len(seen7 & es.all_bc7_combinations()), "bc6h": len(seen6 & es.all_bc6h_combinations())}


def write_pins():
    from oracle import pyoracle
    pyoracle.build()
    out = measured(pyoracle)
    out["synthetic_surfaces"] = synthetic_surface_counts(pyoracle)
    with open(PINS, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "intel-texture-works-plugin_amd")):
        sys.path.insert(0, p)
    if sys.argv[1:] == ["--write"]:
        write_pins()
