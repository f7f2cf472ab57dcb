"""The resident volume's edit log (blok_amd/csrc/hip/edit_log.h) on the host, under ASan + UBSan: tests/host_harness/edit_log_main.cpp, a
program of its own, checks that a fresh log takes as nothing, that boxes join per axis and the fill bit is the OR of the notes, that a
note empty on one axis changes nothing (its bit included), that take resets, the world conversion at a negative origin and at world
32768, and that "whole" means exactly [0, dims).  No GPU."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "host_harness" / "edit_log_main.cpp"


def test_edit_log_under_address_and_ub_sanitizers(tmp_path):
    exe = tmp_path / "edit_log_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", f"-I{ROOT / 'blok_amd/csrc/hip'}", "-o", os.fspath(exe), os.fspath(SRC)], check=True)
    run = subprocess.run([os.fspath(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == "", run.stderr
    assert int(run.stdout) == 28
