"""aimet_amd/csrc/scratch.hpp: the owner of a temporary device block, on the host alone. The program
tests/cpp/test_scratch_handle.cpp replaces the three raw calls behind the owner with recording fakes
and checks when, how often and on which stream a block is released -- at scope exit, under an
exception, after a move, on move-assignment, after reset(), for an empty handle, for the two-stream
upload and with a release that throws. Built here as plain C++ (the header needs neither device code
nor common.hpp) with ASan + UBSan; the program stands alone, so it runs as it is."""
import os
import subprocess

from conftest import REPO

SRC = os.path.join(REPO, "tests", "cpp", "test_scratch_handle.cpp")


def test_scratch_handle_life_cycle(tmp_path):
    exe = str(tmp_path / "test_scratch_handle")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-x", "c++", "-O1", "-g", "-Wall", "-Werror",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(REPO, "aimet_amd", "csrc"),
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "OK"
