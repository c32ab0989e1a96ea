"""CPU: the PUB fan-out seal (cz_seal_fanout, k_seal_fanout) and cz_engine_publish without a device --
the subscriber record's layout against the C header, the argument checks that run before the device
is touched, no CPU fallback, and the kernel's AMDGPU metadata read as tests/test_acceptor_host.py
reads it: no scratch, at least 3 waves per SIMD, and still four code objects in the library."""
import ctypes
import os
import re
import subprocess

import pytest

from cz_testlib import ROOT

HEADER = os.path.join(ROOT, "include", "curvezmq_mi355x.h")


@pytest.fixture(scope="module")
def product():
    from jeromq_amd import build
    build.build_library()
    return build


@pytest.fixture(scope="module")
def lib(product):
    from jeromq_amd import _lib
    return _lib.lib()


def test_sub_layout_matches_c(tmp_path):
    c = tmp_path / "layout.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "curvezmq_mi355x.h"\n'
                 'int main(void){printf("%zu %zu %zu %zu\\n", sizeof(cz_fanout_sub),'
                 'offsetof(cz_fanout_sub,counter),offsetof(cz_fanout_sub,key_idx),'
                 'offsetof(cz_fanout_sub,reserved));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(c), "-o",
                           str(exe)])
    assert list(map(int, subprocess.check_output([str(exe)], text=True).split())) == [16, 0, 8, 12]
    from jeromq_amd import _lib, batch
    assert ctypes.sizeof(_lib.cz_fanout_sub) == 16
    assert [getattr(_lib.cz_fanout_sub, f).offset for f in ("counter", "key_idx", "reserved")] == [0, 8, 12]
    assert batch.FANOUT_SUB_DTYPE.itemsize == 16
    assert [batch.FANOUT_SUB_DTYPE.fields[f][1] for f in ("counter", "key_idx", "reserved")] == [0, 8, 12]


def test_arguments_are_checked_before_the_device(lib):
    from jeromq_amd import _lib
    f = lib.cz_seal_fanout
    p = 4096  # any non-null address: a rejected call never reads it
    assert f(4, 100, None, 0, p, p, p, 256, None) == _lib.CZ_EINVAL
    assert f(4, 100, p, 0, None, p, p, 256, None) == _lib.CZ_EINVAL
    assert f(4, 100, p, 0, p, None, p, 256, None) == _lib.CZ_EINVAL
    assert f(4, 100, p, 0, p, p, None, 256, None) == _lib.CZ_EINVAL
    assert f(4, 100, p, 0, p, p, p, 132, None) == _lib.CZ_EINVAL           # out_stride < len + 33
    assert f(1, 100, p, 0, p, p, p, 132, None) == _lib.CZ_EINVAL           # ... for one subscriber too
    assert f(4, _lib.CZ_MESSAGE_MAX + 1, p, 0, p, p, p, 1 << 32, None) == _lib.CZ_EMSGSIZE
    assert f(0, 100, None, 0, None, None, None, 0, None) == _lib.CZ_OK     # nothing to do, nothing launched


@pytest.mark.skipif(os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK), reason="GPU present")
def test_no_cpu_fallback(lib):
    from jeromq_amd import _lib
    pay = ctypes.create_string_buffer(128)
    subs = (_lib.cz_fanout_sub * 4)()
    keys = ctypes.create_string_buffer(32)
    out = ctypes.create_string_buffer(4 * 256)
    adr = ctypes.addressof
    assert lib.cz_seal_fanout(4, 100, adr(pay), 0, adr(subs), adr(keys), adr(out), 256, None) == _lib.CZ_EHIP
    assert out.raw == bytes(4 * 256)


def test_engine_publish_validates(lib):
    from jeromq_amd import _lib
    ids = (ctypes.c_int * 2)(0, 1)
    q = ctypes.c_uint32(7)
    assert lib.cz_engine_publish(None, ids, 2, b"x", 1, 0, ctypes.byref(q)) == _lib.CZ_EINVAL
    assert q.value == 0
    # a null list with a count, and a null payload with a length: refused before the engine is read
    # (no engine exists without a device, so the handle is a stand-in that must never be touched)
    standin = ctypes.create_string_buffer(64)
    assert lib.cz_engine_publish(ctypes.addressof(standin), None, 2, b"x", 1, 0, ctypes.byref(q)) == _lib.CZ_EINVAL
    assert lib.cz_engine_publish(ctypes.addressof(standin), ids, 2, None, 1, 0, None) == _lib.CZ_EINVAL
    assert standin.raw == bytes(64)


def test_kernel_metadata(product):
    from test_acceptor_host import kernel_notes
    from test_occupancy import waves_per_simd
    assert len(product.device_code_objects(product.PRODUCT_LIB)) == 4
    hits = [(n, f) for n, f in kernel_notes(product).items() if re.search(r"\d+k_seal_fanoutI", n)]
    assert len(hits) == 3, [n for n, _ in hits]  # ST_LINES, ST_REGION, ST_DIRECT
    for name, f in hits:
        assert f["private_segment_fixed_size"] == 0, f"{name} uses {f['private_segment_fixed_size']} bytes of scratch"
        assert f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, name
        got = waves_per_simd(f["vgpr_count"], f["agpr_count"])
        assert got >= 3, f"{name}: {f['vgpr_count']} VGPRs + {f['agpr_count']} AGPRs = {got} waves per SIMD"
