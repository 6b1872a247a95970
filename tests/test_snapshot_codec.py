"""The snapshot codec (csrc/snapshot.h) without a GPU.

tests/snapshot_codec_main.cpp is compiled together with csrc/snapshot.cpp as a
host-only program under AddressSanitizer and UBSan, and run as a child process:
round trips of every section kind and of versions 5, 6 and 7, every proper
prefix of the bytes, every count field at its edge values, the refusals with
their messages, the key-index mapping, and hand-assembled version 2 - 4 bytes.
Exit status 0 means every check passed and the sanitizers saw nothing.
"""
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "flink-siddhi_amd"


def _compiler():
    """The Makefile's HIPCC (as a plain C++ compiler: -x c++, no offload arch), else the host's c++."""
    hipcc = os.environ.get("HIPCC")
    if not hipcc:
        m = re.search(r"^HIPCC\s*\?=\s*(\S+)", (PKG / "Makefile").read_text(), re.M)
        hipcc = m.group(1) if m else None
    if hipcc and (Path(hipcc).exists() or shutil.which(hipcc)):
        return [hipcc, "-x", "c++"]
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no C++ compiler found (HIPCC, g++, c++)")
    return [cxx]


def test_snapshot_codec_under_sanitizers(tmp_path):
    exe = tmp_path / "snapshot_codec"
    cmd = _compiler() + [
        "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
        "-I", str(PKG / "csrc"),
        str(PKG / "csrc" / "snapshot.cpp"), str(ROOT / "tests" / "snapshot_codec_main.cpp"),
        "-o", str(exe),
    ]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, "build failed:\n%s\n%s" % (" ".join(cmd), build.stderr[-4000:])
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, "exit status %d\n%s" % (run.returncode, run.stderr[-4000:])
