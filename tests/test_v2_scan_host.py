"""CPU: the device V2 scan's boundary (include/curvezmq_mi355x.h section 7b) without a device: record layouts
against a gcc-compiled probe, argument validation before any device call, no CPU fallback, the scan_in knob,
and the new kernels' code-object metadata."""
import ctypes
import os
import re
import subprocess

import pytest

from cz_testlib import ROOT

HEADER = os.path.join(ROOT, "include", "curvezmq_mi355x.h")
STREAM_FIELDS = ("off", "len", "floor", "key_idx", "reserved")
RESULT_FIELDS = ("consumed", "slot_off", "first", "nframes", "rc", "reserved")
TOTALS_FIELDS = ("nframes", "slot_bytes")
NEW_KERNELS = ("k_v2_scan", "k_v2_place", "k_v2_emit")


@pytest.fixture(scope="module")
def product():
    from jeromq_amd import build
    build.build_library()
    return build


@pytest.fixture(scope="module")
def lib(product):
    from jeromq_amd import _lib
    return _lib.lib()


def test_layouts_and_prototypes_match_c(tmp_path):
    c = tmp_path / "layout.c"
    offs = ",".join(["sizeof(cz_v2_stream)"] + [f"offsetof(cz_v2_stream,{f})" for f in STREAM_FIELDS] +
                    ["sizeof(cz_v2_stream_result)"] + [f"offsetof(cz_v2_stream_result,{f})" for f in RESULT_FIELDS] +
                    ["sizeof(cz_v2_totals)"] + [f"offsetof(cz_v2_totals,{f})" for f in TOTALS_FIELDS])
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "curvezmq_mi355x.h"\n'
                 'int main(void){size_t v[] = {' + offs + '};'
                 'for (unsigned i = 0; i < sizeof v / sizeof *v; i++) printf("%zu ", v[i]);return 0;}\n')
    exe = tmp_path / "layout"
    gcc = ["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER)]
    subprocess.check_call(gcc + [str(c), "-o", str(exe)])
    # (compiled, not linked: the prototypes are checked by the initialisers)
    p = tmp_path / "proto.c"
    p.write_text('#include "curvezmq_mi355x.h"\n'
                 'int (*scan)(const cz_v2_stream *, uint32_t, const void *, int64_t, uint32_t, cz_v2_stream_result *, '
                 'cz_v2_totals *, void *) = cz_v2_scan;\n'
                 'int (*emit)(const cz_v2_stream *, const cz_v2_stream_result *, uint32_t, const void *, uint32_t, '
                 'cz_v2_frame *, cz_frame_desc *, void *) = cz_v2_scan_emit;\n'
                 'int (*open)(const cz_v2_stream *, uint32_t, const void *, int64_t, uint32_t, cz_v2_stream_result *, '
                 'cz_frame_desc *, uint64_t, void *, uint64_t, const void *, uint16_t *, uint64_t *, cz_v2_totals *, '
                 'void *) = cz_open_streams;\n'
                 'uint64_t (*frames)(const cz_engine *) = cz_engine_scan_frames;\n')
    subprocess.check_call(gcc + ["-c", str(p), "-o", str(tmp_path / "proto.o")])
    want = [32, 0, 8, 16, 24, 28, 32, 0, 8, 16, 20, 24, 28, 16, 0, 8]
    assert list(map(int, subprocess.check_output([str(exe)], text=True).split())) == want
    from jeromq_amd import _lib, wire
    for cls, fields, dtype, w in ((_lib.cz_v2_stream, STREAM_FIELDS, wire.V2_STREAM_DTYPE, want[0:6]),
                                  (_lib.cz_v2_stream_result, RESULT_FIELDS, wire.V2_STREAM_RESULT_DTYPE, want[6:13]),
                                  (_lib.cz_v2_totals, TOTALS_FIELDS, wire.V2_TOTALS_DTYPE, want[13:16])):
        assert ctypes.sizeof(cls) == dtype.itemsize == w[0]
        assert [getattr(cls, f).offset for f in fields] == [dtype.fields[f][1] for f in fields] == w[1:]
    assert wire.V2_STREAM_RESULT_DTYPE.fields["rc"][0].kind == "i"


def test_symbols_exported_bound_and_cited(lib):
    from jeromq_amd import _lib, batch, wire
    from jeromq_amd.engine import CurveBatchEngine
    header = open(HEADER).read()
    for name in ("cz_v2_scan", "cz_v2_scan_emit", "cz_open_streams", "cz_engine_scan_frames"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    # each export of section 7b cites the decoder it restates, as section 7 does
    sec = header[header.index("---- 7b."):header.index("---- 8.")]
    for name in ("cz_v2_scan", "cz_v2_scan_emit", "cz_open_streams"):
        proto = sec.index("int %s(" % name)
        comment = sec[sec.rindex("/*", 0, proto):proto]
        assert "V2Decoder.java:37-105" in comment and "Decoder.java:76-98" in comment, name
    assert callable(wire.scan) and callable(wire.scan_emit) and callable(batch.open_streams)
    assert isinstance(CurveBatchEngine.scan_frames, property)


def _bufs():
    streams = (_lib_mod().cz_v2_stream * 2)()
    streams[0].len = 4
    streams[1].off, streams[1].len = 4, 4
    wire = ctypes.create_string_buffer(bytes([0, 2, 1, 2, 0, 2, 3, 4]), 8)
    results = ctypes.create_string_buffer(b"\x5a" * 64, 64)
    totals = ctypes.create_string_buffer(b"\x5a" * 16, 16)
    return streams, wire, results, totals


def _lib_mod():
    from jeromq_amd import _lib
    return _lib


def test_null_pointers_and_bad_slot_align_are_einval(lib):
    """checked before any device call: the same answers with and without a device, nothing written"""
    L, adr = _lib_mod(), ctypes.addressof
    s, w, r, t = _bufs()
    desc = ctypes.create_string_buffer(b"\x5a" * 80, 80)
    frames = ctypes.create_string_buffer(b"\x5a" * 32, 32)
    out = ctypes.create_string_buffer(256)
    keys = ctypes.create_string_buffer(32)
    status = (ctypes.c_uint16 * 2)(0x5a5a, 0x5a5a)
    tot = L.cz_v2_totals(7, 7)
    S, W, R, T, D, F, O, K, ST, HT = adr(s), adr(w), adr(r), adr(t), adr(desc), adr(frames), adr(out), adr(keys), \
        adr(status), ctypes.byref(tot)
    for args in ((None, 2, W, -1, 128, R, T, None), (S, 2, None, -1, 128, R, T, None), (S, 2, W, -1, 128, None, T, None),
                 (S, 2, W, -1, 128, R, None, None), (S, 0, W, -1, 128, R, None, None)):
        assert lib.cz_v2_scan(*args) == L.CZ_EINVAL, args
    for args in ((None, R, 2, W, 128, F, D, None), (S, None, 2, W, 128, F, D, None), (S, R, 2, None, 128, F, D, None)):
        assert lib.cz_v2_scan_emit(*args) == L.CZ_EINVAL, args
    good = [S, 2, W, -1, 128, R, D, 2, O, 256, K, ST, None, HT, None]
    for i in (0, 2, 5, 6, 8, 10, 11, 13):
        args = list(good)
        args[i] = None
        assert lib.cz_open_streams(*args) == L.CZ_EINVAL, i
    for align in (0, 3, 24, 100, 8192, 1 << 31):
        assert lib.cz_v2_scan(S, 2, W, -1, align, R, T, None) == L.CZ_EINVAL, align
        assert lib.cz_v2_scan_emit(S, R, 2, W, align, F, D, None) == L.CZ_EINVAL, align
        assert lib.cz_open_streams(*(good[:4] + [align] + good[5:])) == L.CZ_EINVAL, align
    assert "slot_align" in L.last_error()
    assert r.raw == b"\x5a" * 64 and t.raw == b"\x5a" * 16 and desc.raw == b"\x5a" * 80 and frames.raw == b"\x5a" * 32
    assert list(status) == [0x5a5a, 0x5a5a]
    # count == 0 with nothing to read is fine for the calls that take no totals from the device
    assert lib.cz_v2_scan_emit(None, None, 0, None, 128, None, None, None) == L.CZ_OK
    assert lib.cz_open_streams(None, 0, None, -1, 128, None, D, 2, O, 256, K, ST, None, HT, None) == L.CZ_OK
    assert (tot.nframes, tot.slot_bytes) == (0, 0)


@pytest.mark.skipif(os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK), reason="GPU present")
def test_no_cpu_fallback(lib):
    L, adr = _lib_mod(), ctypes.addressof
    s, w, r, t = _bufs()
    desc = ctypes.create_string_buffer(b"\x5a" * 80, 80)
    frames = ctypes.create_string_buffer(b"\x5a" * 32, 32)
    out = ctypes.create_string_buffer(b"\x5a" * 256, 256)
    keys = ctypes.create_string_buffer(32)
    status = (ctypes.c_uint16 * 2)(0x5a5a, 0x5a5a)
    tot = L.cz_v2_totals()
    assert lib.cz_v2_scan(adr(s), 2, adr(w), -1, 128, adr(r), adr(t), None) == L.CZ_EHIP
    assert lib.cz_v2_scan_emit(adr(s), adr(r), 2, adr(w), 128, adr(frames), adr(desc), None) == L.CZ_EHIP
    assert lib.cz_open_streams(adr(s), 2, adr(w), -1, 128, adr(r), adr(desc), 2, adr(out), 256, adr(keys), adr(status),
                               None, ctypes.byref(tot), None) == L.CZ_EHIP
    assert r.raw == b"\x5a" * 64 and t.raw == b"\x5a" * 16 and desc.raw == b"\x5a" * 80 and out.raw == b"\x5a" * 256
    assert frames.raw == b"\x5a" * 32 and list(status) == [0x5a5a, 0x5a5a]


def test_scan_in_knob(lib):
    """off by default unless the measured default says otherwise (DESIGN.md section 4 "Device V2 scan"); set / get"""
    src = open(os.path.join(ROOT, "jeromq_amd", "csrc", "cz_host.cpp")).read()
    default = int(re.search(r"g_scan_in\{(\d+)\}", src).group(1))
    # ... which is what the rule gives on the committed measurement: the largest measured per-connection byte count
    # with the scanned flush not slower at every measured shape at or below it
    import json
    prof = json.load(open(os.path.join(ROOT, "profiles", "scan", "scan.json")))
    best = 0
    for e in sorted(prof["engine"], key=lambda e: e["bytes_per_connection"]):
        if e["scanned_flush_ms"] > e["unscanned_flush_ms"]:
            break
        best = e["bytes_per_connection"]
    assert len(prof["engine"]) == 5 and best == prof["scan_in_rule"] == default == 0
    old = lib.cz_tune(b"scan_in", 65536)
    try:
        assert old == default
        assert lib.cz_tune(b"scan_in", 100) == 65536
        assert lib.cz_tune(b"scan_in", -5) == 100        # clamped to 0
        assert lib.cz_tune(b"scan_in", 0) == 0
    finally:
        lib.cz_tune(b"scan_in", old)
    assert lib.cz_tune(b"scan_in", old) == old


def test_kernel_metadata(product):
    """one code object entry each, no scratch, no spills, and a walk small enough for full occupancy"""
    from test_acceptor_host import kernel_notes
    from test_occupancy import waves_per_simd
    notes = kernel_notes(product)
    for k in NEW_KERNELS:
        hits = [(n, f) for n, f in notes.items() if re.search(r"\d+" + k + r"(E|P|I)", n) and k + "_" not in n]
        assert len(hits) == 1, f"{k}: {[n for n, _ in hits]}"
        name, f = hits[0]
        assert f["private_segment_fixed_size"] == 0, f"{name} uses {f['private_segment_fixed_size']} bytes of scratch"
        assert f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, name
        assert waves_per_simd(f["vgpr_count"], f["agpr_count"]) >= 8, f"{name}: {f['vgpr_count']} VGPRs"
    (place,) = [f for n, f in notes.items() if "k_v2_place" in n]
    assert place["group_segment_fixed_size"] == 2 * 256 * 8      # the two LDS scan rows
