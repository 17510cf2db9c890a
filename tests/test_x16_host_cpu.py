"""The staged 16-bit hand-off's host-side launch arithmetic (csrc/x16.h: strides, item counts,
LDS sizes, shape gates) under AddressSanitizer + UBSan, through the stand-alone program
tools/x16_host_check.cpp — host code only, no GPU and nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_x16_host_arithmetic_under_sanitizers(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "x16_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "vae-teb_amd", "csrc"), os.path.join(ROOT, "tools", "x16_host_check.cpp"),
                    "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert out.stdout.startswith("ok"), out.stdout + out.stderr
