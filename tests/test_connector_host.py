"""CPU: the batched connector (jeromq_amd/csrc/cz_connector.cpp, cz_connect_kernels.h) without a device --
it cannot be created without the GPU (no CPU fallback); its kernels' AMDGPU metadata, read as
tests/test_acceptor_host.py reads it: no scratch and no spills in any of them, the two X25519 kernels
still at 3 waves per SIMD; and the host-only parsers it shares with cz_hs (cz_hs_parse.cpp), run in a
stand-alone program under the address and undefined-behaviour sanitizers (tools/con_parse_fuzz.cpp)."""
import ctypes
import os
import re
import subprocess

import pytest

from test_acceptor_host import kernel_notes

NEW_KERNELS = ["k_con_hello", "k_con_welcome", "k_con_initiate", "k_con_ready"]


@pytest.fixture(scope="module")
def product():
    from jeromq_amd import build
    build.build_library()
    return build


def test_new_kernels_use_no_scratch_and_ladders_keep_occupancy(product):
    from test_occupancy import waves_per_simd
    notes = kernel_notes(product)
    for k in NEW_KERNELS:
        hits = [(n, f) for n, f in notes.items() if re.search(r"\d+" + k + r"E", n)]
        assert len(hits) == 1, f"{k}: {[n for n, _ in hits]}"
        name, f = hits[0]
        assert f["private_segment_fixed_size"] == 0, f"{name} uses {f['private_segment_fixed_size']} bytes of scratch"
        assert f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, name
    for k in ("k_x25519_jobs", "k_x25519"):
        (f,) = [f for n, f in notes.items() if re.search(r"\d+" + k + r"E", n)]
        got = waves_per_simd(f["vgpr_count"], f["agpr_count"])
        assert f["private_segment_fixed_size"] == 0 and got >= 3, f"{k}: {f['vgpr_count']} VGPRs, {got} waves per SIMD"


def test_create_validates_before_touching_the_device(product):
    from jeromq_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    pub, sec = bytes(32), bytes(32)
    assert L.cz_connector_create(None, pub, sec, 0, None, 0, 4, 0) == _lib.CZ_EINVAL
    assert L.cz_connector_create(ctypes.byref(h), None, sec, 0, None, 0, 4, 0) == _lib.CZ_EINVAL
    assert L.cz_connector_create(ctypes.byref(h), pub, None, 0, None, 0, 4, 0) == _lib.CZ_EINVAL
    assert L.cz_connector_create(ctypes.byref(h), pub, sec, 5, None, 3, 4, 0) == _lib.CZ_EINVAL     # identity_len, no identity
    assert L.cz_connector_create(ctypes.byref(h), pub, sec, 21, None, 0, 4, 0) == _lib.CZ_EINVAL    # no such socket type
    assert L.cz_connector_create(ctypes.byref(h), pub, sec, 0, None, 0, 0, 0) == _lib.CZ_EINVAL     # max_pending 0
    # DEALER metadata is 35 + identity bytes: 221 is the largest identity that fits 256
    assert L.cz_zmtp_metadata(5, bytes(221), 221, None, 0) == 256
    assert L.cz_connector_create(ctypes.byref(h), pub, sec, 5, bytes(222), 222, 4, 0) == _lib.CZ_EMSGSIZE
    assert not h.value
    assert L.cz_connector_pending(None) == 0
    assert L.cz_connector_release(None, 0) == _lib.CZ_EINVAL
    assert L.cz_connector_error_status(None, 0) == 0
    assert L.cz_connector_hello(None, 1, None, None, 200, None, None) == _lib.CZ_EINVAL


@pytest.mark.skipif(os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK), reason="GPU present")
def test_connector_needs_the_gpu(product):
    from jeromq_amd import _lib, connector
    h = ctypes.c_void_p()
    assert _lib.lib().cz_connector_create(ctypes.byref(h), bytes(32), bytes(32), 0, None, 0, 16, 0) == _lib.CZ_EHIP
    assert not h.value and "no HIP device" in _lib.last_error()
    # the largest identity passes the argument checks and reaches the device check
    assert _lib.lib().cz_connector_create(ctypes.byref(h), bytes(32), bytes(32), 5, bytes(221), 221, 16,
                                          0) == _lib.CZ_EHIP
    with pytest.raises(_lib.CzError):
        connector.CurveConnector(bytes(32), bytes(32))


def test_host_parsers_under_the_sanitizers(product, tmp_path):
    """tools/con_parse_fuzz.cpp with cz_hs_parse.cpp, built for the CPU with -fsanitize=address,undefined and
    run as a child process: 10^5 mutated commands per parser, exit status 0, no sanitizer report.  The
    sanitizer runtimes are linked statically: the program does not depend on what else the loader brings in."""
    exe = tmp_path / "con_parse_fuzz"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(product.ROOT, "include"),
                           os.path.join(product.ROOT, "tools", "con_parse_fuzz.cpp"),
                           os.path.join(product.CSRC, "cz_hs_parse.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), "100000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    m = re.match(r"con_parse_fuzz: dispatch (\d+), error (\d+), metadata (\d+) \+ (\d+), 0 failed checks", r.stdout)
    assert m and all(int(x) >= 100000 for x in m.groups()), r.stdout
