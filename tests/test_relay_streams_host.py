"""CPU side of the stream relay (header section 3j) and the engine's forward routes: the boundary, the argument
checks without a device, the Python bounds checks, the route table's rules in a stand-alone program (no engine
exists without a device), the two new kernels' metadata, and the model the GPU tests stand on
(tests/relay_streams_model.py) against the one receive model of tests/rx_model.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import rx_model as rx
from cz_testlib import ROOT
from relay_streams_model import engine_expect, stream_expect

from jeromq_amd import batch
from jeromq_amd.engine import CurveBatchEngine

# the Python face of the feature: every test of this file stands on it
CALLS = (batch.relay_streams, CurveBatchEngine.forward, CurveBatchEngine.flush_forward, CurveBatchEngine.forward_out,
         CurveBatchEngine.forward_frames)

HEADER = os.path.join(ROOT, "include", "curvezmq_mi355x.h")
CSRC = os.path.join(ROOT, "jeromq_amd", "csrc")
NEW = ("cz_relay_streams", "cz_engine_forward", "cz_engine_flush_forward", "cz_engine_forward_out",
       "cz_engine_forward_frames")


@pytest.fixture(scope="module")
def product():
    from jeromq_amd import build
    build.build_library()
    return build


@pytest.fixture(scope="module")
def lib(product):
    from jeromq_amd import _lib
    return _lib.lib()


def _prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b(int|uint64_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in the header"
    return m.group(1), [" ".join(a.split()) for a in m.group(2).split(",")]


def _ctype(arg):
    if arg.count("*") == 2:
        return ctypes.POINTER(ctypes.c_void_p)
    if arg.startswith("uint64_t *"):
        return ctypes.POINTER(ctypes.c_uint64)
    if "*" in arg:
        return ctypes.c_void_p
    return {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int64_t": ctypes.c_int64,
            "int": ctypes.c_int}[arg.split()[0]]


@pytest.mark.parametrize("name", NEW)
def test_header_declares_and_lib_binds_the_declared_signature(lib, name):
    from jeromq_amd import _lib
    ret, args = _prototype(name)
    res, argtypes = _lib.SIGNATURES[name]
    assert res is {"int": ctypes.c_int, "uint64_t": ctypes.c_uint64}[ret]
    want = [_ctype(a) for a in args]
    if name == "cz_relay_streams":
        want[12] = ctypes.c_void_p          # uint64_t *d_nonces is a device pointer
    assert list(argtypes) == want, args
    assert hasattr(lib, name) and getattr(lib, name).argtypes == list(argtypes)


def test_record_layout_matches_c(tmp_path):
    c = tmp_path / "layout.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "curvezmq_mi355x.h"\n'
                 '#define O(f) offsetof(cz_relay_stream_result, f)\n'
                 'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(cz_relay_stream_result), O(ok_bytes),'
                 'O(whole_bytes), O(peer_nonce), O(ok_frames), O(fail_status), O(reserved));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(c), "-o", str(exe)])
    vals = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    dt = batch.RELAY_STREAM_RESULT_DTYPE
    assert vals[0] == dt.itemsize == 32
    assert vals[1:] == [dt.fields[k][1] for k in ("ok_bytes", "whole_bytes", "peer_nonce", "ok_frames", "fail_status",
                                                  "reserved")]
    from jeromq_amd._lib import cz_relay_stream_result
    assert ctypes.sizeof(cz_relay_stream_result) == 32


def test_header_section_cites_the_reference_path():
    src = open(HEADER).read()
    sec = src[src.index("---- 3j. stream relay"):src.index("int cz_relay_streams(")]
    for cite in ("Proxy.java:140-160", "V2Decoder.java:37-105", "Decoder.java:76-98", "CurveServerMechanism.java:165-225",
                 "CurveClientMechanism.java:165-224", ":126-163"):
        assert cite in sec, cite
    assert "NOTHING BEHIND THEM" in sec
    eng = src[src.index("int cz_engine_forward(") - 1200:src.index("int cz_engine_forward(")]
    assert "Proxy.java:140-160" in eng


def test_null_pointers_and_empty_calls_without_a_device(lib):
    from jeromq_amd import _lib
    p = 4096        # never dereferenced: the checks come before the device is touched
    tot = _lib.cz_v2_totals(7, 7)
    t = ctypes.addressof(tot)
    #       streams to count wire out max scan desc to_frames cap subkeys status nonces results totals stream
    full = [p, p, 3, p, p, -1, p, p, p, 8, p, p, p, p, t, None]
    for k in (0, 1, 3, 4, 6, 7, 8, 10, 11, 12, 13, 14):
        a = list(full)
        a[k] = None
        assert lib.cz_relay_streams(*a) == _lib.CZ_EINVAL, k
        assert "null pointer" in _lib.last_error()
    empty = list(full)
    empty[2] = 0
    assert lib.cz_relay_streams(*empty) == _lib.CZ_OK and (tot.nframes, tot.slot_bytes) == (0, 0)
    # the engine calls: no engine exists without a device, and a null one is refused
    w, n = ctypes.c_void_p(), ctypes.c_uint64()
    assert lib.cz_engine_forward(None, 0, 1) == _lib.CZ_EINVAL
    assert lib.cz_engine_flush_forward(None) == _lib.CZ_EINVAL
    assert lib.cz_engine_forward_out(None, 0, ctypes.byref(w), ctypes.byref(n)) == _lib.CZ_EINVAL
    standin = ctypes.create_string_buffer(64)
    assert lib.cz_engine_forward_out(ctypes.addressof(standin), 0, None, ctypes.byref(n)) == _lib.CZ_EINVAL
    assert lib.cz_engine_forward_out(ctypes.addressof(standin), 0, ctypes.byref(w), None) == _lib.CZ_EINVAL
    assert lib.cz_engine_forward_frames(None) == 0 and standin.raw == bytes(64)


@pytest.mark.skipif(os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK), reason="GPU present")
def test_no_cpu_fallback_without_gpu(lib):
    from jeromq_amd import _lib
    assert lib.cz_device_ok() == 0
    buf = ctypes.create_string_buffer(8192)
    p = ctypes.addressof(buf)
    tot = _lib.cz_v2_totals()
    assert lib.cz_relay_streams(p, p, 1, p, p, -1, p, p, p, 8, p, p, p, p, ctypes.byref(tot), None) == _lib.CZ_EHIP
    assert not any(buf.raw)         # nothing was computed on the host


def test_python_bounds_checks():
    from jeromq_amd.wire import V2_STREAM_DTYPE
    st = np.zeros(3, dtype=V2_STREAM_DTYPE)
    st["off"], st["len"], st["key_idx"] = (5, 100, 300), (80, 150, 84), (0, 1, 0)
    to = np.zeros(3, dtype=batch.FANOUT_SUB_DTYPE)
    to["key_idx"] = (1, 0, 1)
    ok = dict(count=3, nto=3, nscan=3, nresults=3, desc_cap=9, ndesc=9, nto_frames=9, nstatus=9, nnonces=9,
              wire_bytes=400, out_bytes=400, streams_np=st, to_np=to, nkeys=2)
    batch._check_relay_streams_bounds(**ok)
    batch._check_relay_streams_bounds(**dict(ok, streams_np=None, to_np=None, out_bytes=401))
    for bad in (dict(nto=2), dict(nscan=2), dict(nresults=2), dict(ndesc=8), dict(nto_frames=8), dict(nstatus=8),
                dict(nnonces=8), dict(out_bytes=399), dict(wire_bytes=399, out_bytes=399), dict(nkeys=1), dict(count=4)):
        with pytest.raises(ValueError):
            batch._check_relay_streams_bounds(**dict(ok, **bad))
    t2 = to.copy()
    t2["key_idx"][2] = 2
    with pytest.raises(ValueError):
        batch._check_relay_streams_bounds(**dict(ok, to_np=t2))

    class T:            # a stand-in for a tensor: the checks run before any device call
        is_cuda = False
    with pytest.raises(ValueError):
        batch.relay_streams(T(), T(), T(), T(), T(), T(), T(), T(), T(), T(), T())


# ---- the route table, as a stand-alone program --------------------------------------------------------
ROUTES_MAIN = r"""
#include <stdio.h>
#include <vector>
#include "cz_routes.h"
#define CHECK(x) do { if (!(x)) { printf("line %d: %s\n", __LINE__, #x); return 1; } } while (0)
int main()
{
    std::vector<bool> removed(6, false);
    auto live = [&](int id) { return id >= 0 && id < (int)removed.size() && !removed[(size_t)id]; };
    czi::RouteTable r;
    CHECK(r.dest(0) == -1 && r.source(0) == -1 && r.dest(-1) == -1 && r.dest(99) == -1);
    CHECK(r.set(0, 1, live) && r.dest(0) == 1 && r.source(1) == 0);
    CHECK(r.set(1, 0, live) && r.dest(1) == 0);               // A -> B with B -> A: the normal proxy
    CHECK(!r.set(2, 1, live) && r.dest(2) == -1);             // a shared destination
    CHECK(!r.set(2, 2, live));                                // from == to
    CHECK(!r.set(2, 6, live) && !r.set(6, 2, live) && !r.set(-1, 2, live) && !r.set(2, -2, live));   // unknown ids
    CHECK(r.set(0, 1, live));                                 // the same route again
    CHECK(r.set(0, 3, live) && r.dest(0) == 3 && r.source(1) == -1 && r.source(3) == 0);   // re-routed: 1 is free
    CHECK(r.set(2, 1, live));
    CHECK(r.set(0, -1, live) && r.dest(0) == -1 && r.source(3) == -1);    // cleared
    CHECK(r.set(0, -1, live));                                // clearing nothing is fine
    removed[4] = true;
    CHECK(!r.set(4, 5, live) && !r.set(5, 4, live) && !r.set(4, -1, live));   // a removed id
    // removing either end clears the route
    CHECK(r.set(3, 5, live) && r.set(5, 3, live));
    r.drop(5);
    CHECK(r.dest(3) == -1 && r.dest(5) == -1 && r.source(3) == -1 && r.source(5) == -1);
    CHECK(r.dest(2) == 1 && r.dest(1) == 0);                  // the others stand
    r.drop(0);                                                // the destination of 1 -> 0
    CHECK(r.dest(1) == -1 && r.source(0) == -1 && r.dest(2) == 1);
    r.drop(99);
    r.drop(-1);
    CHECK(r.set(3, 0, live));                                 // a freed destination takes a new source
    puts("ok");
    return 0;
}
"""


def test_route_table_rules(tmp_path):
    """what cz_engine_forward answers CZ_EINVAL to -- a shared destination, from == to, an unknown or removed id
    -- and what cz_engine_remove_conn clears: the engine keeps its routes in this table"""
    src = tmp_path / "routes_main.cpp"
    src.write_text(ROUTES_MAIN)
    exe = tmp_path / "routes_main"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src),
                           "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    eng = open(os.path.join(CSRC, "cz_engine.cpp")).read()
    assert "routes.set(from, to, live)" in eng and eng.count("routes.drop(") == 2      # both removal paths


def test_kernel_metadata(product):
    from test_acceptor_host import kernel_notes
    notes = kernel_notes(product)
    for kernel in ("k_v2_emit_relay", "k_relay_cut"):
        hits = [(n, f) for n, f in notes.items() if re.search(r"\d+%sE" % kernel, n)]
        assert len(hits) == 1, (kernel, [n for n, _ in hits])
        name, f = hits[0]
        assert f["private_segment_fixed_size"] == 0, f"{name} uses {f['private_segment_fixed_size']} bytes of scratch"
        assert f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, name
        assert f["group_segment_fixed_size"] == 0, f"{name} uses LDS"


# ---- the model the GPU tests stand on, against the one receive model -----------------------------------
@pytest.mark.parametrize("role", rx.ROLES)
def test_model_agrees_with_the_stream_model(role):
    """for every scenario of the table: the frames that leave, cnPeerNonce and the failure event of the source are
    those of the same bytes delivered through V2Decoder and the mechanism"""
    bad = []
    other = rx.from_server(role) ^ 1
    for sc in rx.scenarios():
        wire = sc.wire(role)
        want = rx.stream_model(role, sc.floor, [(wire, True)])[0]
        exp = stream_expect(wire, sc.floor, rx.from_server(role), rx.PRECOM, 1 << 40, other, rx.PRECOM)
        got = engine_expect(exp, role)
        if got != (len(want["delivered"]), want["peer_nonce"], want["error"]):
            bad.append(f"{sc.name}: model {got}, stream_model {(len(want['delivered']), want['peer_nonce'], want['error'])}")
            continue
        # what leaves opens, in the oracle, to what was delivered, under the outbound counters
        nd = len(want["delivered"])
        for k in sorted({0, 1, 2, nd - 2, nd - 1} & set(range(nd))):
            payload, fl = want["delivered"][k]
            _h, off, size = exp.frames[k]
            rc, p, f, n = rx.or_curve_decode(exp.out[off:off + size], other, rx.PRECOM)
            if (rc, p, f, n) != (0, payload, fl, (1 << 40) + k):
                bad.append(f"{sc.name} frame {k}: the re-sealed body does not open to what was delivered")
        if exp.ok_bytes != (exp.frames[exp.ok_frames - 1][1] + exp.frames[exp.ok_frames - 1][2] if exp.ok_frames else 0):
            bad.append(f"{sc.name}: ok_bytes {exp.ok_bytes}")
        if not exp.whole_bytes <= exp.ok_bytes <= exp.consumed <= len(wire):
            bad.append(f"{sc.name}: {exp.whole_bytes} / {exp.ok_bytes} / {exp.consumed}")
    assert not bad, "\n".join(bad[:20])


def test_model_framing_errors_and_partial_frames():
    from cz_testlib import or_curve_encode, v2_encode
    b = [or_curve_encode(bytes([k]) * (10 + k), k & 1, 5 + k, 0, rx.PRECOM) for k in range(3)]
    good = b"".join(v2_encode(x, 1 if k == 0 else 0) for k, x in enumerate(b))
    for tail, rc in ((b"", 0), (b"\x00", 0), (b"\x02\x00\x00\x00", 0), (b"\x00\x28" + bytes(10), 0),
                     (b"\x02" + bytes(8), rx.CZ_EPROTO), (b"\x02\xff" + bytes(7), rx.CZ_EPROTO)):
        exp = stream_expect(good + tail, 4, 0, rx.PRECOM, 100, 1, rx.PRECOM)
        assert (len(exp.frames), exp.consumed, exp.rc, exp.ok_frames, exp.ok_bytes) == (3, len(good), rc, 3, len(good))
        assert exp.whole_bytes == len(good) and exp.peer_nonce == 7 and len(exp.out) == len(good)
        assert engine_expect(exp, rx.SERVER) == (3, 7, (rc, 0))
    exp = stream_expect(b"", 4, 0, rx.PRECOM, 100, 1, rx.PRECOM)
    assert (exp.frames, exp.consumed, exp.ok_bytes, exp.peer_nonce, exp.fail_status) == ([], 0, 0, 4, 0)
