"""The owners of the context's device memory (blok_amd/csrc/hip/device_buffer.h) on the host, under ASan + UBSan:
tests/host_harness/device_buffer_main.cpp, a program of its own that defines the HIP entry points the header calls as fakes over malloc
and links no HIP library.  It checks that a reserve within capacity makes no call, that growth is wait, free, allocate with the wait the
caller named, that a failed allocation leaves the owner empty with the sticky error consumed, that "replaced" is true exactly on first
allocation and growth, that moves and fresh values free exactly once, and that a struct of owners frees everything when it is assigned
{} or erased from a map; the same for pinned arrays and events.  No GPU."""
import os
import subprocess
from pathlib import Path

from blok_amd import build

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_harness" / "device_buffer_main.cpp"


def test_device_buffer_under_address_and_ub_sanitizers(tmp_path):
    rocm_include = Path(build.hipcc()).resolve().parent.parent / "include"
    exe = tmp_path / "device_buffer_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", f"-I{rocm_include}", f"-I{ROOT / 'blok_amd/csrc/hip'}",
                    "-o", os.fspath(exe), os.fspath(SRC)], check=True)
    run = subprocess.run([os.fspath(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == "", run.stderr
    assert int(run.stdout) == 132
