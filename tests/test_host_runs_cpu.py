"""The run cuts and the band workspace layout of a host-pointer call without a GPU: csrc/host_runs.hpp is plain C++, and
tools/host_runs_check.cpp asserts the rules of ITW_HOST_CHUNKS, ITW_HOST_RUNS and the default splits on it as a stand-alone program.  Built
with AddressSanitizer and UBSan where the compiler has their runtimes (an empty program links with the flags), without them elsewhere."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_run_cuts_and_band_workspace_on_the_host(tmp_path):
    empty = tmp_path / "empty.cpp"
    empty.write_text("int main() { return 0; }\n")
    probe = subprocess.run(["g++", *SANITIZE, str(empty), "-o", str(tmp_path / "empty")], capture_output=True, text=True)
    flags = SANITIZE if probe.returncode == 0 else []
    exe = str(tmp_path / "host_runs_check")
    subprocess.run(["g++", "-std=c++17", "-g", *flags, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "host_runs_check.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print("sanitizers:", "on" if flags else "no runtime installed, built without", "|", run.stdout.strip())
    assert run.returncode == 0 and run.stdout.startswith("ok "), (run.stdout[-400:], run.stderr[-2000:])
    assert int(run.stdout.split()[1]) > 1000
