"""The all-patterns kernel runs beside two 192-VGPR job waves on every SIMD of a suite step: each of its
instantiations must fit the 128 registers that leaves, without scratch.  CPU only: reads the figures the Makefile writes when it
compiles pattern.hip (csrc/pattern.resources.txt)."""
import re
from pathlib import Path

import pytest

RES = Path(__file__).resolve().parent.parent / "polars_quant_amd" / "csrc" / "pattern.resources.txt"


def test_cdl_all_kernel_fits_beside_two_job_waves_without_scratch():
    if not RES.exists():
        pytest.skip("pattern.resources.txt is written when pattern.hip is compiled")
    blocks = re.split(r"(?=Function Name:)", RES.read_text())
    seen = {}
    for b in blocks:
        m = re.match(r"Function Name: (\S*cdl_all_kernel\S*)", b)
        if not m:
            continue
        vgprs = int(re.search(r"^\s*VGPRs: (\d+)", b, re.M).group(1))
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        seen[m.group(1)] = (vgprs, scratch)
    assert len(seen) == 4, f"expected the four cdl_all_kernel<ALL, VEC> instantiations, found {sorted(seen)}"
    for fn, (vgprs, scratch) in seen.items():
        assert scratch == 0, f"{fn}: {scratch} bytes of scratch per lane"
        assert vgprs <= 128, f"{fn}: {vgprs} VGPRs"
