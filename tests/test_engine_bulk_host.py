"""CPU: the bulk session hand-over (section 13 of the header: cz_engine_add_conns, cz_engine_add_accepted_batch,
cz_engine_add_connected_batch, cz_engine_remove_conns, cz_acceptor_release_batch, cz_connector_release_batch)
without a device -- the symbols are exported and bound, null handles and null arrays are refused before the
device is touched, there is no CPU fallback, and the two new kernels' AMDGPU metadata, read as
tests/test_fanout_host.py reads it: no scratch, no spills, no LDS, and still four code objects."""
import ctypes
import os
import re

import pytest

from cz_testlib import ROOT

HEADER = os.path.join(ROOT, "include", "curvezmq_mi355x.h")
BULK = ("cz_engine_add_conns", "cz_engine_add_accepted_batch", "cz_engine_add_connected_batch",
        "cz_engine_remove_conns", "cz_acceptor_release_batch", "cz_connector_release_batch")


@pytest.fixture(scope="module")
def product():
    from jeromq_amd import build
    build.build_library()
    return build


@pytest.fixture(scope="module")
def lib(product):
    from jeromq_amd import _lib
    return _lib.lib()


def test_symbols_exported_bound_and_declared(lib):
    from jeromq_amd import _lib
    header = open(HEADER).read()
    for name in BULK:
        assert name in _lib.SIGNATURES, name
        f = getattr(lib, name)                       # AttributeError: not exported
        assert f.restype is ctypes.c_int and f.argtypes == _lib.SIGNATURES[name][1]
        assert re.search(r"\bint %s\(" % name, header), name
    from jeromq_amd.acceptor import CurveAcceptor
    from jeromq_amd.connector import CurveConnector
    from jeromq_amd.engine import CurveBatchEngine
    for cls, methods in ((CurveBatchEngine, ("add_connections", "add_accepted_many", "add_connected_many",
                                             "remove_connections")),
                         (CurveAcceptor, ("release_many",)), (CurveConnector, ("release_many",))):
        for m in methods:
            assert callable(getattr(cls, m)), f"{cls.__name__}.{m}"


def test_null_arguments_are_refused_before_the_device(lib):
    """No engine or handshake exists without a device, so the handles are stand-ins that a refused call
    must never read or write; output arrays that are given hold only negative entries afterwards."""
    from jeromq_amd import _lib
    E = _lib.CZ_EINVAL
    standin = ctypes.create_string_buffer(256)
    h = ctypes.addressof(standin)
    keys = ctypes.create_string_buffer(2 * 32)
    roles = (ctypes.c_uint8 * 2)(1, 0)
    n64 = (ctypes.c_uint64 * 2)(2, 3)
    ids = (ctypes.c_int32 * 2)(7, 7)
    slots = (ctypes.c_int32 * 2)(0, 1)
    conns = (ctypes.c_int * 2)(0, 1)
    adr = ctypes.addressof
    f = lib.cz_engine_add_conns
    assert f(None, 2, adr(roles), adr(keys), adr(n64), adr(n64), adr(ids)) == E
    assert list(ids) == [7, 7]                                   # no handle: nothing is written
    assert f(h, 2, adr(roles), None, adr(n64), adr(n64), adr(ids)) == E and list(ids) == [E, E]
    assert f(h, 2, None, adr(keys), None, adr(n64), adr(ids)) == E
    assert f(h, 2, None, adr(keys), adr(n64), None, adr(ids)) == E
    assert f(h, 2, adr(roles), adr(keys), adr(n64), adr(n64), None) == E
    assert f(h, 0, None, None, None, None, None) == _lib.CZ_OK   # nothing to do, nothing launched
    for g in (lib.cz_engine_add_accepted_batch, lib.cz_engine_add_connected_batch):
        ids[0] = ids[1] = 7
        assert g(None, h, 2, adr(slots), adr(ids)) == E and g(h, None, 2, adr(slots), adr(ids)) == E
        assert list(ids) == [7, 7]
        assert g(h, h, 2, None, adr(ids)) == E and list(ids) == [E, E]
        assert g(h, h, 2, adr(slots), None) == E
        assert g(h, h, 0, None, None) == _lib.CZ_OK
    rcs = (ctypes.c_int32 * 2)(7, 7)
    f = lib.cz_engine_remove_conns
    assert f(None, 2, adr(conns), adr(rcs)) == E and f(h, 2, None, adr(rcs)) == E and f(h, 2, adr(conns), None) == E
    assert f(h, 0, None, None) == _lib.CZ_OK
    for g in (lib.cz_acceptor_release_batch, lib.cz_connector_release_batch):
        assert g(None, 2, adr(slots)) == E and g(h, 2, None) == E
        assert g(h, 0, None) == _lib.CZ_OK
    assert standin.raw == bytes(256)


@pytest.mark.skipif(os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK), reason="GPU present")
def test_no_cpu_fallback():
    """without a device there is no engine and no handshake to hand sessions over from or to: the
    constructors raise, and nothing computes subkeys on the host instead"""
    from jeromq_amd import _lib
    from jeromq_amd.acceptor import CurveAcceptor
    from jeromq_amd.connector import CurveConnector
    from jeromq_amd.engine import CurveBatchEngine
    for make in (lambda: CurveBatchEngine(arena_bytes=4096), lambda: CurveAcceptor(bytes(range(32))),
                 lambda: CurveConnector(bytes(range(32)), bytes(range(32)))):
        with pytest.raises(_lib.CzError, match=r"\(-5\)"):
            make()


def test_kernel_metadata(product):
    from test_acceptor_host import kernel_notes
    assert len(product.device_code_objects(product.PRODUCT_LIB)) == 4
    notes = kernel_notes(product)
    for kernel in ("k_session_subkeys", "k_scatter_wipe"):
        hits = [(n, f) for n, f in notes.items() if re.search(r"\d+%sE" % kernel, n)]
        assert len(hits) == 1, (kernel, [n for n, _ in hits])
        name, f = hits[0]
        assert f["private_segment_fixed_size"] == 0, f"{name} uses {f['private_segment_fixed_size']} bytes of scratch"
        assert f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, name
        assert f["group_segment_fixed_size"] == 0, f"{name} uses LDS"
