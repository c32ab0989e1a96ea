"""Occupancy guard for the relay kernels (CPU: reads the built library's AMDGPU metadata, as
tests/test_occupancy.py).  DESIGN.md section 4 "Relay" records what the line-staged kernel is shipped
with: 3 waves per SIMD (at most 168 VGPRs, no AGPRs) and 72 bytes of scratch per lane -- the emitter's
held line-0 words, stored once before the block loop and reloaded once after it."""
import os
import re
import subprocess
import tempfile

import pytest

from test_occupancy import waves_per_simd

LINES = r"k_relay_uniformILi1E"     # k_relay_uniform<ST_LINES>
RECORDED_WAVES = 3                  # DESIGN.md section 4 "Relay"
RECORDED_SCRATCH = 72               # bytes per lane, DESIGN.md section 4 "Relay"


def _metadata(lib):
    """{mangled name: (vgprs, agprs, private segment bytes)} of every kernel of the library"""
    from jeromq_amd import build
    out = {}
    for co in build.device_code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            notes = subprocess.run([os.path.join(build.LLVM_BIN, "llvm-readelf"), "--notes", f.name],
                                   check=True, capture_output=True, text=True).stdout
        for blk in notes.split("  - .agpr_count:")[1:]:
            name = re.search(r"^\s+\.name:\s+(\S+)", blk, re.M)
            vg = re.search(r"^\s+\.vgpr_count:\s+(\d+)", blk, re.M)
            pv = re.search(r"^\s+\.private_segment_fixed_size:\s+(\d+)", blk, re.M)
            ag = re.match(r"\s*(\d+)", blk)
            if name and vg and pv and ag:
                out[name.group(1)] = (int(vg.group(1)), int(ag.group(1)), int(pv.group(1)))
    return out


@pytest.fixture(scope="module")
def kernels():
    from jeromq_amd import build
    build.build_library()
    ks = _metadata(build.PRODUCT_LIB)
    assert ks, "no kernel metadata found"
    return ks


def test_relay_kernels_are_in_the_library(kernels):
    for pat in (LINES, r"k_relay_uniformILi0E", r"k_relay_desc"):
        assert [n for n in kernels if re.search(pat, n)], pat


def test_line_staged_relay_keeps_its_recorded_occupancy(kernels):
    (name, (vg, ag, _pv)), = [(n, v) for n, v in kernels.items() if re.search(LINES, n)]
    got = waves_per_simd(vg, ag)
    assert RECORDED_WAVES >= 2
    assert got >= RECORDED_WAVES, f"{name}: {vg} VGPRs + {ag} AGPRs = {got} waves per SIMD, DESIGN.md records {RECORDED_WAVES}"


def test_line_staged_relay_has_no_scratch_beyond_what_design_states(kernels):
    (name, (_vg, _ag, pv)), = [(n, v) for n, v in kernels.items() if re.search(LINES, n)]
    assert pv <= RECORDED_SCRATCH, f"{name}: {pv} bytes of scratch per lane, DESIGN.md states {RECORDED_SCRATCH}"


def test_design_records_these_figures():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "DESIGN.md")).read()
    sec = text[text.index("### Relay"):]
    assert f"{RECORDED_WAVES} waves per SIMD" in sec and f"{RECORDED_SCRATCH} bytes of scratch" in sec
