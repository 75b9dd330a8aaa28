"""No entry point goes without a stream-order case: every symbol lib/libispc_texcomp.so exports is either named by a case of
tests/_stream_order.py (run by tests/test_gpu_stream_order.py) or listed in EXEMPT with the reason it has no stream order to keep.  A new
entry point fails this test until someone decides which it is."""
import os
import subprocess

import _stream_order as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "intel-texture-works-plugin_amd", "lib", "libispc_texcomp.so")

HOST_ONLY = "host arithmetic or host memory only: no device work"
SETTING = "reads or sets a setting of the thread or the process: no device work"
PROFILE = "fills a settings struct on the host"
TRAMPOLINE = "a CompressionFunc trampoline: CompressBlocks* of its preset, which has cases; as a function pointer it names the preset of a sliced / chain call"

EXEMPT = {
    # stream and settings
    "itwSetStream": "the setter the whole module stands on: every case calls it through the binding",
    "itwGetStream": SETTING, "itwAvailable": SETTING, "itwSetErrorMode": SETTING, "itwLastError": SETTING, "itwClearError": SETTING,
    "itwSetBc7Pilot": SETTING, "itwDeviceInfo": SETTING, "itwVersion": HOST_ONLY, "itwSliceWindow": HOST_ONLY, "itwSliceWindowFor": HOST_ONLY,
    "itwBandForPart": HOST_ONLY, "itwBandForPartEx": HOST_ONLY, "GetProcessorCount": SETTING, "InitWin32Threads": "starts the host thread pool",
    "DestroyThreads": "ends the host thread pool", "GetBytesPerBlock": HOST_ONLY, "itwChainBytes": HOST_ONLY, "itwPsnrToTotalSse": HOST_ONLY,
    "itwChainPsnrToTotalSse": HOST_ONLY, "itwStatsPsnr": HOST_ONLY, "itwPadToMultipleOf4": HOST_ONLY, "itwFreeSurface": HOST_ONLY,
    "itwCubeCrossFaces": HOST_ONLY, "itwMipLevels": HOST_ONLY, "itwMipChainLayout": HOST_ONLY, "itwSrgbToLinear": HOST_ONLY, "itwLinearToSrgb": HOST_ONLY,
    "itwWarmupBC45": "builds the BC4 / BC5 index table ahead of the first call; synchronous, no caller buffer",
    "itwWarmupBC45S": "builds the signed index table ahead of the first call; synchronous, no caller buffer",
    # multi-GPU: synchronous, host pointers, needs two GPUs
    "itwMultiGpuRanks": SETTING, "itwMultiGpuTransport": SETTING, "itwMultiGpuPeerLinks": SETTING, "itwMultiGpuSetInterleave": SETTING, "itwMultiGpuPieces": HOST_ONLY,
    "itwCompressImageMultiGPU": "synchronous, streams of its own per GPU, needs two GPUs (tests/test_gpu_multigpu_cpp.py)",
    "itwCompressImageMultiGPUEx": "synchronous, streams of its own per GPU, needs two GPUs (tests/test_gpu_multigpu_cpp.py)",
    "itwCompressImageMultiGPUBands": "synchronous, streams of its own per GPU, needs two GPUs (tests/test_gpu_multigpu_cpp.py)",
    # containers
    "itwDdsLevelBytes": HOST_ONLY, "itwDdsHeaderBytes": HOST_ONLY, "itwDdsFileBytes": HOST_ONLY, "itwDdsWriteHeader": HOST_ONLY, "itwDdsReadHeader": HOST_ONLY,
    "itwDdsWriteFile": HOST_ONLY, "itwDdsImage": HOST_ONLY, "itwKtxHeaderBytes": HOST_ONLY, "itwKtxFileBytes": HOST_ONLY, "itwKtxWriteHeader": HOST_ONLY,
    "itwKtxReadHeader": HOST_ONLY, "itwKtxWriteFile": HOST_ONLY, "itwKtxImage": HOST_ONLY,
}
for _p in ("ultrafast", "veryfast", "fast", "basic", "slow"):
    EXEMPT.setdefault("GetProfile_" + _p, PROFILE)
    EXEMPT.setdefault("GetProfile_alpha_" + _p, PROFILE)
    EXEMPT["CompressImageBC7_" + _p] = EXEMPT["CompressImageBC7_alpha_" + _p] = TRAMPOLINE
for _p in ("veryfast", "fast", "basic", "slow", "veryslow"):
    EXEMPT.setdefault("GetProfile_bc6h_" + _p, PROFILE)
    EXEMPT["CompressImageBC6H_" + _p] = TRAMPOLINE
for _n in ("CompressImageBC4", "CompressImageBC5", "CompressImageBC4S", "CompressImageBC5S"):
    EXEMPT[_n] = TRAMPOLINE
EXEMPT["itwGetProfile_etc_slow"] = PROFILE


def _exported():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    rows = [ln.split() for ln in out.splitlines()]
    return {r[2] for r in rows if len(r) == 3 and r[1] == "T" and not r[2].startswith("_")}       # the C entry points (weak C++ template instances are no ABI)


def test_every_exported_symbol_has_a_case_or_a_reason():
    import itw_amd
    names = _exported()
    assert names >= set(itw_amd.EXPORTED_SYMBOLS), sorted(set(itw_amd.EXPORTED_SYMBOLS) - names)      # nm found the library's table
    covered = so.covered_symbols()
    unlisted = sorted(n for n in names if n not in covered and n not in EXEMPT)
    assert not unlisted, f"{unlisted}: add a case to tests/_stream_order.py or an entry, with its reason, to EXEMPT"
    gone = sorted(n for n in covered | set(EXEMPT) if n not in names)
    assert not gone, f"{gone}: named here, exported nowhere"
    assert all(EXEMPT.values())


def test_every_scheme_has_cases_and_every_case_names_an_entry_point():
    assert {c.scheme for c in so.CASES} == {"A", "B", "D"}
    for c in so.CASES:
        assert c.symbols and callable(c.build), c.id
    # the asynchronous, capturable calls are all in sequence A
    assert all(c.scheme == "A" for c in so.CASES if c.capturable)
