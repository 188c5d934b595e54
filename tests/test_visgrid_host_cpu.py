"""The kernel of csrc/visgrid.hip compiled for the host (tests/host/visgrid_host.cpp: a launch becomes a serial loop over
the grid) as a stand-alone program under AddressSanitizer and UBSan: index arithmetic, bounds, the vector and scalar forms,
the aligned and unaligned loads and stores and the byte conversion at every threshold against a plain loop, byte for byte,
on exact-size heap buffers; plus the sizes the launcher must refuse. It says nothing about the GPU build's code generation;
tests/test_visgrid_gpu.py covers that."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def _compiler():
    hipcc = Path(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    for c in (hipcc.parent.parent / "llvm" / "bin" / "clang++", shutil.which("clang++"), shutil.which("g++")):
        if c and Path(c).is_file():
            return str(c)
    pytest.fail("no C++ compiler found")


def test_host_build_of_the_kernel_matches_the_plain_loop(tmp_path):
    src = (ROOT / "ganslate_amd" / "csrc" / "visgrid.hip").read_text()
    assert src.count('#include "common.hpp"') == 1
    (tmp_path / "visgrid_body.inc").write_text(src.replace('#include "common.hpp"', ""))
    exe = tmp_path / "visgrid_host"
    r = subprocess.run([_compiler(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", str(tmp_path), str(ROOT / "tests" / "host" / "visgrid_host.cpp"),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ALL OK" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
    assert r.stdout.count(": grid=") >= 14 and r.stdout.count(": rejected") == 7
