"""The keyed brick index of the resident volume (blok_amd/csrc/hip/volume_device.h: cell_key / key_cell) on the host, under ASan + UBSan:
tests/host_harness/cell_key_main.cpp, a program of its own, checks the round trip, the digit order and that the keys of a cube are a
permutation, for every cell of 4^d per axis, d = 1..3.  No GPU."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_harness" / "cell_key_main.cpp"


def test_cell_key_round_trip_under_address_and_ub_sanitizers(tmp_path):
    exe = tmp_path / "cell_key_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", f"-I{ROOT / 'blok_amd/csrc/hip'}", "-o", os.fspath(exe), os.fspath(SRC)], check=True)
    run = subprocess.run([os.fspath(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == "", run.stderr
    assert int(run.stdout) == 4 ** 3 + 16 ** 3 + 64 ** 3
