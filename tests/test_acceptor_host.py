"""CPU: the batched acceptor (jeromq_amd/csrc/cz_acceptor.cpp, cz_accept_kernels.h) without a device -- it
cannot be created without the GPU (no CPU fallback), and its kernels' AMDGPU metadata, read as
tests/test_occupancy.py reads it: no scratch in any of them, and the per-lane-job X25519 kernel at
k_x25519's 3 waves per SIMD (the ladder is VALU-bound; DESIGN.md section 4, "Batched server handshake")."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest

NEW_KERNELS = ["k_x25519_jobs", "k_acc_welcome", "k_acc_initiate", "k_acc_ready"]


@pytest.fixture(scope="module")
def product():
    from jeromq_amd import build
    build.build_library()
    return build


def kernel_notes(build):
    """name -> {field: int} for every kernel of the product library's gfx950 code objects"""
    out = {}
    for co in build.device_code_objects(build.PRODUCT_LIB):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            notes = subprocess.run([os.path.join(build.LLVM_BIN, "llvm-readelf"), "--notes", f.name],
                                   check=True, capture_output=True, text=True).stdout
        for blk in notes.split("  - .agpr_count:")[1:]:
            name = re.search(r"^\s+\.name:\s+(\S+)", blk, re.M)
            if not name:
                continue
            fields = {k: int(v) for k, v in re.findall(r"^\s+\.(\w+):\s+(\d+)\s*$", blk, re.M)}
            fields["agpr_count"] = int(re.match(r"\s*(\d+)", blk).group(1))
            out[name.group(1)] = fields
    return out


def test_new_kernels_use_no_scratch_and_keep_occupancy(product):
    from test_occupancy import waves_per_simd
    notes = kernel_notes(product)
    for k in NEW_KERNELS:
        hits = [(n, f) for n, f in notes.items() if re.search(r"\d+" + k + r"E", n)]
        assert len(hits) == 1, f"{k}: {[n for n, _ in hits]}"
        name, f = hits[0]
        assert f["private_segment_fixed_size"] == 0, f"{name} uses {f['private_segment_fixed_size']} bytes of scratch"
        assert f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, name
        if k == "k_x25519_jobs":
            got = waves_per_simd(f["vgpr_count"], f["agpr_count"])
            assert got >= 3, f"{name}: {f['vgpr_count']} VGPRs + {f['agpr_count']} AGPRs = {got} waves per SIMD"
    # k_x25519 itself is unchanged by sharing its field arithmetic
    (kx,) = [f for n, f in notes.items() if re.search(r"\d+k_x25519E", n)]
    assert kx["private_segment_fixed_size"] == 0 and waves_per_simd(kx["vgpr_count"], kx["agpr_count"]) >= 3


def test_result_layout_matches_c(product, tmp_path):
    from jeromq_amd._lib import cz_accept_result
    c = tmp_path / "layout.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "curvezmq_mi355x.h"\n'
                 'int main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(cz_accept_result),'
                 'offsetof(cz_accept_result,rc),offsetof(cz_accept_result,event),offsetof(cz_accept_result,slot),'
                 'offsetof(cz_accept_result,reply_len));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(product.ROOT, "include"), str(c),
                           "-o", str(exe)])
    vals = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    assert vals == [ctypes.sizeof(cz_accept_result)] + [getattr(cz_accept_result, k).offset
                                                        for k in ("rc", "event", "slot", "reply_len")]


def test_create_validates_before_touching_the_device(product):
    from jeromq_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.cz_acceptor_create(None, bytes(32), 0, None, 0, 4, 0) == _lib.CZ_EINVAL
    assert L.cz_acceptor_create(ctypes.byref(h), None, 0, None, 0, 4, 0) == _lib.CZ_EINVAL
    assert L.cz_acceptor_create(ctypes.byref(h), bytes(32), 21, None, 0, 4, 0) == _lib.CZ_EINVAL   # no such socket type
    assert L.cz_acceptor_create(ctypes.byref(h), bytes(32), 0, None, 0, 0, 0) == _lib.CZ_EINVAL    # max_pending 0
    assert L.cz_acceptor_create(ctypes.byref(h), bytes(32), 6, bytes(222), 222, 4, 0) == _lib.CZ_EMSGSIZE  # ROUTER identity
    assert not h.value
    assert L.cz_acceptor_pending(None) == 0
    assert L.cz_acceptor_release(None, 0) == _lib.CZ_EINVAL


@pytest.mark.skipif(os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK), reason="GPU present")
def test_acceptor_needs_the_gpu(product):
    from jeromq_amd import _lib, acceptor
    h = ctypes.c_void_p()
    assert _lib.lib().cz_acceptor_create(ctypes.byref(h), bytes(32), 0, None, 0, 16, 0) == _lib.CZ_EHIP
    assert not h.value and "no HIP device" in _lib.last_error()
    with pytest.raises(_lib.CzError):
        acceptor.CurveAcceptor(bytes(32))
