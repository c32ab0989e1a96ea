"""CPU side of the segmented CURVE relay (header section 3i): the boundary, the argument checks without a
device, the Python bounds and workspace checks, SegmentPlan's two-plane workspace, and the launcher's
grid through the launch-printing shim."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from cz_testlib import DESC_DTYPE, ROOT

from jeromq_amd import batch

sys.path.insert(0, os.path.join(ROOT, "tools"))
import dispatch_record  # noqa: E402

RELAY_SEGMENTS = batch.relay_segments       # the Python face of the feature: every test of this file stands on it

HEADER = os.path.join(ROOT, "include", "curvezmq_mi355x.h")
NAME = "cz_relay_segments"
needs_hipcc = pytest.mark.skipif(not os.path.exists(dispatch_record.HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def lib():
    from jeromq_amd import _lib
    from jeromq_amd.build import build_library
    build_library()
    return _lib.lib()


def _prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in the header"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _ctype(arg):
    if "*" in arg:
        return ctypes.c_void_p
    return {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int}[arg.split()[0]]


def test_header_declares_and_lib_binds_the_declared_signature(lib):
    from jeromq_amd import _lib
    args = _prototype(NAME)
    assert [a.split()[-1].lstrip("*") for a in args] == [
        "d_desc", "d_to", "d_seg", "nseg", "d_comb", "ncomb", "npart", "d_in", "d_out", "d_subkeys", "d_work", "d_status",
        "d_nonces", "stream"]
    res, argtypes = _lib.SIGNATURES[NAME]
    assert res is ctypes.c_int and list(argtypes) == [_ctype(a) for a in args], args
    assert hasattr(lib, NAME) and getattr(lib, NAME).argtypes == list(argtypes)


def test_header_section_follows_3h_and_states_the_contract():
    src = open(HEADER).read()
    assert src.index("---- 3h. relay") < src.index("int cz_relay_uniform(") < src.index("---- 3i. segmented relay")
    sec = src[src.index("---- 3i. segmented relay"):src.index("int cz_relay_segments(")]
    for cite in ("Proxy.java:140-160", "CurveServerMechanism.java:165-225", "CurveClientMechanism.java:165-224", ":126-163"):
        assert cite in sec, cite
    for said in ("128 bytes per part", "NO IN PLACE", "must not overlap", "open = 1", "block 2 or later", "CZ_EHIP",
                 "at most two launches"):
        assert said in sec, said


#            desc to seg nseg comb ncomb npart in out keys work status nonces stream
def _args(p, **kw):
    a = dict(desc=p, to=p, seg=p, nseg=4, comb=p, ncomb=1, npart=2, inp=p, out=p, keys=p, work=p, status=p, nonces=None,
             stream=None)
    a.update(kw)
    return list(a.values())


def test_null_pointers_and_empty_plans_without_a_device(lib):
    from jeromq_amd import _lib
    p = 4096        # never dereferenced: the checks come before the device is touched
    assert lib.cz_relay_segments(*([None] * 3 + [0] + [None, 0, 0] + [None] * 7)) == _lib.CZ_OK
    assert lib.cz_relay_segments(*_args(p, nseg=0)) == _lib.CZ_OK                # nothing launched, no device needed
    for k in ("desc", "to", "seg", "inp", "out", "keys", "status"):
        assert lib.cz_relay_segments(*_args(p, **{k: None})) == _lib.CZ_EINVAL, k
        assert "null pointer" in _lib.last_error()
    for k in ("comb", "work"):          # needed only with split frames
        assert lib.cz_relay_segments(*_args(p, **{k: None})) == _lib.CZ_EINVAL, k
        assert "combine list / workspace" in _lib.last_error()


@pytest.mark.skipif(os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK), reason="GPU present")
def test_no_cpu_fallback_without_gpu(lib):
    from jeromq_amd import _lib
    assert lib.cz_device_ok() == 0
    buf = ctypes.create_string_buffer(8192)
    p = ctypes.addressof(buf)
    assert lib.cz_relay_segments(*_args(p, nseg=1, ncomb=0, comb=None, work=None)) == _lib.CZ_EHIP
    assert lib.cz_relay_segments(*_args(p, nseg=2, ncomb=1)) == _lib.CZ_EHIP
    assert not any(buf.raw)         # nothing was computed on the host


class _T:
    """a stand-in for a device tensor: the checks under test run before any device call"""
    is_cuda = True

    def __init__(self, nbytes, rows=None):
        import torch
        self.dtype, self._n, self.shape = torch.uint8, nbytes, (rows if rows is not None else nbytes,)

    def numel(self):
        return self._n

    def element_size(self):
        return 1

    def data_ptr(self):
        raise AssertionError("the library was reached")


def _plan_stub(desc, seg_blocks, work_bytes):
    plan = batch.SegmentPlan(desc, open_=True, seg_blocks=seg_blocks)
    plan.d_seg, plan.d_comb, plan.d_work = _T(16 * plan.nseg), _T(16 * max(plan.ncomb, 1)), _T(work_bytes)
    return plan


def test_python_bounds_and_workspace_checks(lib):
    d = np.zeros(3, dtype=DESC_DTYPE)
    d["in_off"], d["out_off"], d["len"], d["key_idx"], d["prev"] = (0, 1040, 1200), (8, 1048, 1208), (1025, 133, 400), (0, 1, 2), (-1, 0, 1)
    to = np.zeros(3, dtype=batch.FANOUT_SUB_DTYPE)
    to["key_idx"] = (3, 3, 0)
    nparts = batch.SegmentPlan(d, open_=True, seg_blocks=2).npart
    assert nparts >= 2

    def call(desc_np=d, to_np=to, in_bytes=1600, out_bytes=1608, nkeys=4, nstatus=3, nnonces=3, work=128 * nparts, ndesc=3, nto=3):
        batch.relay_segments(_T(40 * ndesc), _T(16 * nto), _plan_stub(d, 2, work), _T(in_bytes), _T(out_bytes),
                             _T(32 * nkeys, rows=nkeys), _T(nstatus), nonces=None if nnonces is None else _T(nnonces),
                             stream=0, desc_np=desc_np, to_np=to_np)

    # every check passes: the call goes on to the library (the stand-ins refuse to give a pointer)
    with pytest.raises(AssertionError, match="the library was reached"):
        call()
    for bad in (dict(in_bytes=1599), dict(out_bytes=1607), dict(nkeys=3), dict(nstatus=2), dict(nnonces=2), dict(nto=2),
                dict(ndesc=2)):
        with pytest.raises(ValueError):
            call(**bad)
    d2 = d.copy()
    d2["key_idx"][2] = 4                    # the inbound key index against the table
    with pytest.raises(ValueError):
        call(desc_np=d2)
    d2 = d.copy()
    d2["prev"][0] = 3
    with pytest.raises(ValueError):
        call(desc_np=d2)
    t2 = to.copy()
    t2["key_idx"][1] = 4                    # the outbound one
    with pytest.raises(ValueError):
        call(to_np=t2)
    # the workspace: 128 bytes per part, not the open's 64
    with pytest.raises(ValueError, match="128 bytes per part"):
        call(work=64 * nparts)
    with pytest.raises(ValueError, match="128 bytes per part"):
        call(work=128 * nparts - 1)

    class Host:
        is_cuda = False
    with pytest.raises(ValueError):
        batch.relay_segments(Host(), Host(), _plan_stub(d, 2, 128 * nparts), Host(), Host(), Host(), Host())


def test_segment_plan_workspace_planes():
    """to(device, records=2) allocates two planes of npart 64-byte records; the default is the open's one"""
    import torch
    d = np.zeros(2, dtype=DESC_DTYPE)
    d["len"], d["out_off"] = (2000, 100), (0, 2048)
    plan = batch.SegmentPlan(d, open_=True, seg_blocks=4)
    assert plan.npart == 8 and plan.ncomb == 1
    dev = torch.device("cpu")
    assert plan.to(dev).d_work.numel() == 64 * plan.npart
    assert plan.to(dev, records=1).d_work.numel() == 64 * plan.npart
    assert plan.to(dev, records=2).d_work.numel() == 128 * plan.npart
    assert plan.d_seg.numel() == 16 * plan.nseg and plan.d_comb.numel() == 16 * plan.ncomb
    with pytest.raises(ValueError):
        plan.to(dev, records=3)
    empty = batch.SegmentPlan(d[1:], open_=True, seg_blocks=4)      # no split frame: one record still allocated
    assert empty.npart == 0 and empty.to(dev, records=2).d_work.numel() == 128


# ---- the grid, through the launch-printing shim -------------------------------------------------------
SHIFT_ROWS_LDS = 4 * 64 * 208       # WAVES x SHIFT_LDS_BYTES: the segment emitters' rows, 4 waves
MODE_LINES, MODE_SHIFT16 = 1, 8     # SEGMODE_LINES, SEGMODE_SHIFT16


@needs_hipcc
def test_grid_names_exactly_the_two_kernels():
    text = dispatch_record.record(relay_segments=True)
    knob, cases, cur = None, [], None
    for ln in text.splitlines():
        m = re.fullmatch(r"relay_segments nseg=(\d+) ncomb=(\d+) npart=(\d+)", ln)
        if m:
            cur = (knob, tuple(map(int, m.groups())), [])
            cases.append(cur)
        elif ln.startswith("  ") and " g=" in ln:
            k, rest = ln[2:].split(" g=", 1)
            g, b, l, args = re.fullmatch(r"(\d+) b=(\d+) l=(\d+) :(.*)", rest).groups()
            assert b == "256"
            cur[2].append((k, int(g), int(l), tuple(int(a) if a.isdigit() else a for a in args.split())))
        else:
            assert ln.startswith("knob "), ln
            knob = ln[5:]
    assert len(cases) >= 200 and {k for k, *_ in cases} >= {"default=0", "seglines=0", "shift16=0"}
    for knob, (nseg, ncomb, npart), got in cases:
        lines, shift16 = knob != "seglines=0", knob != "shift16=0"
        mode = (MODE_LINES if lines else 0) | (MODE_SHIFT16 if shift16 else 0)
        want = []
        if nseg:
            want.append(("k_relay_segments", (nseg + 255) // 256, SHIFT_ROWS_LDS if lines else 0,
                         ("A+0", "A+800", "A+1000", nseg, "I+0", "O+0", "K+0", "A+3000", npart, "A+4000", "A+5000", mode)))
            if ncomb:
                want.append(("k_relay_combine", (ncomb + 255) // 256, 0,
                             ("A+0", "A+2000", ncomb, "I+0", "O+0", "A+3000", npart, "A+4000")))
        assert got == want, (knob, nseg, ncomb, got, want)
    assert dispatch_record.signatures(text) == {"k_relay_segments", "k_relay_combine"}
    assert {255, 256, 257} <= {c[1][0] for c in cases} and {0, 1, 256, 257} <= {c[1][1] for c in cases}


@needs_hipcc
def test_other_records_hold_no_relay_segments_case():
    """the new grid is behind its own argument: the default grid still records the parent's text
    (tests/test_dispatch_record.py compares it) and the relay grid its own kernels only"""
    assert "relay" not in open(os.path.join(ROOT, "tests", "golden", "dispatch_parent.txt")).read()
    src = open(os.path.join(ROOT, "tools", "dispatch_record", "driver.cpp")).read()
    main = src[src.index("int main("):]
    assert main.index("relay_segments_cases()") < main.index("seal_cases()")
    assert main[main.index("relay_segments_cases()"):main.index("seal_cases()")].count("return 0;") == 1
    relay = dispatch_record.record(relay=True)
    assert "relay_segments" not in relay
    assert dispatch_record.signatures(relay) == {"k_relay_uniform<1>", "k_relay_uniform<0>"}
    with pytest.raises(ValueError):
        dispatch_record.record(relay=True, relay_segments=True)
