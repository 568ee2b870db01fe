"""The workspace carver of csrc/xsec/xsec_ws.h, on the CPU: tests/host/xs_ws_check.cpp includes that header alone, is built with the
host compiler under AddressSanitizer and UBSan, and run directly.  It checks the carver's rules -- 256-byte starts, spans in taking
order and pairwise disjoint inside a block of exactly the measured size, zero counts that move nothing, a wrapping size refused --
for double / int32 / uint16 / byte spans of 0, 1, 31, 32, 33 and 2^20 elements, and writes every byte of every span."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_carver_rules_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/host/xs_ws_check.cpp")
    exe = tmp_path / "xs_ws_check"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", str(ROOT / "polars_quant_amd" / "csrc" / "xsec"),
                            str(ROOT / "tests" / "host" / "xs_ws_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "xs_ws_check OK" in run.stdout, run.stdout[-4000:] + run.stderr[-4000:]


def test_header_needs_no_hip():
    """the header includes <cstddef> and <cstdint> only, so that the host compiler builds it alone"""
    text = (ROOT / "polars_quant_amd" / "csrc" / "xsec" / "xsec_ws.h").read_text()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<cstddef>", "<cstdint>"], includes
