"""The rule that sends a BC1 / BC3 / BC4 / BC5 call to the 32-bit offset walk or to the 64-bit loaders, without a GPU:
csrc/offset32_host.hpp is plain C++, and tools/offset32_host_check.cpp replays the kernels' offset recurrence in uint32_t and in int64_t
over a few thousand (stride, width, height) triples as a stand-alone program.  Built with AddressSanitizer and UBSan where the compiler has
their runtimes (an empty program links with the flags), without them elsewhere.  The second test asks the launchers' own functions, through
the hooks build, on both sides of the switch."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_the_32_bit_walk_agrees_with_64_bit_offsets_wherever_the_rule_allows_it(tmp_path):
    empty = tmp_path / "empty.cpp"
    empty.write_text("int main() { return 0; }\n")
    probe = subprocess.run(["g++", *SANITIZE, str(empty), "-o", str(tmp_path / "empty")], capture_output=True, text=True)
    flags = SANITIZE if probe.returncode == 0 else []
    exe = str(tmp_path / "offset32_host_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", *flags, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "offset32_host_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print("sanitizers:", "on" if flags else "no runtime installed, built without", "|", run.stdout.strip())
    assert run.returncode == 0 and run.stdout.startswith("ok "), (run.stdout[-400:], run.stderr[-2000:])
    assert int(run.stdout.split()[1]) > 1000


def test_the_launchers_switch_loaders_at_two_gib():
    """itwTestWalks32 (libispc_texcomp_test.so only) is the function launch_bc1 / launch_bc3 / launch_bc45 branch on.  Eight rows
    2^28 - 16 bytes apart end 128 bytes below 2^31: the last surface of the 32-bit walk; at 2^28 bytes apart they end at 2^31: the first
    one on the 64-bit loaders."""
    import itw_amd as itw
    assert "itwTestWalks32" in itw.TEST_HOOK_SYMBOLS and not hasattr(itw.lib(), "itwTestWalks32")
    T = itw.test_lib()
    for kind in (1, 3, 4, 8, 16):
        assert T.itwTestWalks32(kind, (1 << 28) - 16, 1028, 8) == 1, kind
        assert T.itwTestWalks32(kind, 1 << 28, 1028, 8) == 0, kind
        assert T.itwTestWalks32(kind, 0x30000000, 1028, 8) == 0, kind
        assert T.itwTestWalks32(kind, -4112, 1028, 8) == 0 and T.itwTestWalks32(kind, 0, 1028, 8) == 0, kind
        assert T.itwTestWalks32(kind, 4 * 16384, 16384, 16384) == 1, kind                      # 16384^2 RGBA8, 1 GiB: the fast path
        assert T.itwTestWalks32(kind, 16, (1 << 30) + 4, 4) == 0, kind                         # overlapping rows: the column term alone passes 2^32
    assert T.itwTestWalks32(1, 4100, 1025, 9) == 1 and T.itwTestWalks32(4, 4100, 1025, 8) == 0  # BC4 / BC5 walk whole-block surfaces only
    assert T.itwTestWalks32(4, 4112, 1028, 7) == 0 and T.itwTestWalks32(2, 4112, 1028, 8) == -1
