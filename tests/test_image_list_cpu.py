"""The per-image argument check and the staging plan of the texel stages without a GPU: csrc/image_list_host.hpp is plain C++, and
tools/image_list_host_check.cpp asserts its rules over a few hundred small lists, and the plan against the sums the stages used to make
inline, as a stand-alone program.  Built with AddressSanitizer and UBSan where the compiler has their runtimes (an empty program links with
the flags), without them elsewhere."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_image_checks_and_staging_plan_on_the_host(tmp_path):
    empty = tmp_path / "empty.cpp"
    empty.write_text("int main() { return 0; }\n")
    probe = subprocess.run(["g++", *SANITIZE, str(empty), "-o", str(tmp_path / "empty")], capture_output=True, text=True)
    flags = SANITIZE if probe.returncode == 0 else []
    exe = str(tmp_path / "image_list_host_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", *flags, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "image_list_host_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print("sanitizers:", "on" if flags else "no runtime installed, built without", "|", run.stdout.strip())
    assert run.returncode == 0 and run.stdout.startswith("ok "), (run.stdout[-400:], run.stderr[-2000:])
    assert int(run.stdout.split()[1]) > 1000
