"""Occupancy guard for the segmented relay kernels (CPU: reads the built library's AMDGPU metadata, as
tests/test_relay_occupancy.py).  DESIGN.md section 4 "Segmented relay" records what k_relay_segments is
shipped with: 2 waves per SIMD (at most 256 VGPRs, no AGPRs) and 0 bytes of scratch per lane -- two keys,
two keystream blocks and two Poly1305 chains per lane, as k_relay_desc, and no scratch access in the
block loop."""
import os
import re

import pytest

from test_occupancy import waves_per_simd
from test_relay_occupancy import _metadata

SEGMENTS = r"k_relay_segments"
COMBINE = r"k_relay_combine"
RECORDED_WAVES = 2                  # DESIGN.md section 4 "Segmented relay"
RECORDED_SCRATCH = 0                # bytes per lane, DESIGN.md section 4 "Segmented relay"


@pytest.fixture(scope="module")
def kernels():
    from jeromq_amd import build
    build.build_library()
    ks = _metadata(build.PRODUCT_LIB)
    assert ks, "no kernel metadata found"
    return ks


def test_segmented_relay_kernels_are_in_the_library(kernels):
    for pat in (SEGMENTS, COMBINE):
        assert len([n for n in kernels if re.search(pat, n)]) == 1, pat


def test_segments_kernel_keeps_its_recorded_occupancy(kernels):
    (name, (vg, ag, _pv)), = [(n, v) for n, v in kernels.items() if re.search(SEGMENTS, n)]
    got = waves_per_simd(vg, ag)
    assert RECORDED_WAVES >= 2
    assert got >= RECORDED_WAVES, f"{name}: {vg} VGPRs + {ag} AGPRs = {got} waves per SIMD, DESIGN.md records {RECORDED_WAVES}"


def test_segments_kernel_has_no_scratch_beyond_what_design_states(kernels):
    (name, (_vg, _ag, pv)), = [(n, v) for n, v in kernels.items() if re.search(SEGMENTS, n)]
    assert pv <= RECORDED_SCRATCH, f"{name}: {pv} bytes of scratch per lane, DESIGN.md states {RECORDED_SCRATCH}"


def test_design_records_these_figures():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "DESIGN.md")).read()
    sec = text[text.index("### Segmented relay"):]
    assert f"{RECORDED_WAVES} waves per SIMD" in sec and f"{RECORDED_SCRATCH} bytes of scratch" in sec
