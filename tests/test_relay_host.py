"""CPU side of the CURVE relay (header section 3h): the boundary, the argument checks without a device,
the Python bounds checks, the launcher's pure plan through the launch-printing shim, and the CPU model
of decode -> Msg -> encode pinned against what libzmq sealed and accepted."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

from cz_testlib import DESC_DTYPE, ROOT, or_curve_decode, splitmix_bytes
from relay_model import relay_expect

from jeromq_amd import batch

sys.path.insert(0, os.path.join(ROOT, "tools"))
import dispatch_record  # noqa: E402

# the Python face of the feature: every test of this file stands on it (the model tests pin what it must compute)
RELAY_CALLS = (batch.relay_batch, batch.relay_uniform)

HEADER = os.path.join(ROOT, "include", "curvezmq_mi355x.h")
RELAY = ("cz_relay_batch", "cz_relay_uniform")
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


@pytest.mark.parametrize("name", RELAY)
def test_header_declares_and_lib_binds_the_declared_signature(lib, name):
    from jeromq_amd import _lib
    args = _prototype(name)
    res, argtypes = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and list(argtypes) == [_ctype(a) for a in args], args
    assert hasattr(lib, name) and getattr(lib, name).argtypes == list(argtypes)


def test_header_section_cites_the_reference_path():
    src = open(HEADER).read()
    sec = src[src.index("---- 3h. relay"):src.index("int cz_relay_uniform(")]
    for cite in ("Proxy.java:140-160", "CurveServerMechanism.java:165-225", "CurveClientMechanism.java:165-224", ":126-163"):
        assert sec.count(cite) >= 2, cite       # once per export


def test_null_pointers_and_empty_batches_without_a_device(lib):
    from jeromq_amd import _lib
    p = 4096        # never dereferenced: the checks come before the device is touched
    assert lib.cz_relay_batch(None, None, None, 0, None, None, None, None, None, None) == _lib.CZ_OK
    assert lib.cz_relay_uniform(0, 4129, None, 0, None, 0, None, 0, 1, None, 0, None, None) == _lib.CZ_OK
    full = [p, p, None, 4, p, p, p, p, None, None]      # d_order and d_nonces are optional
    for k in (0, 1, 4, 5, 6, 7):
        a = list(full)
        a[k] = None
        assert lib.cz_relay_batch(*a) == _lib.CZ_EINVAL, k
        assert "null pointer" in _lib.last_error()
    full = [4, 100, p, 112, p, 128, p, 0, 1, p, 0, p, None]
    for k in (2, 4, 6, 9, 11):
        a = list(full)
        a[k] = None
        assert lib.cz_relay_uniform(*a) == _lib.CZ_EINVAL, k
    assert lib.cz_relay_uniform(4, 100, p, 99, p, 128, p, 0, 1, p, 0, p, None) == _lib.CZ_EINVAL     # in_stride < size
    assert lib.cz_relay_uniform(4, 100, p, 112, p, 99, p, 0, 1, p, 0, p, None) == _lib.CZ_EINVAL     # out_stride < size
    assert lib.cz_relay_uniform(1 << 31, 100, p, 1 << 62, p, 128, p, 0, 1, p, 0, p, None) == _lib.CZ_EINVAL


@pytest.mark.skipif(os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK), reason="GPU present")
def test_no_cpu_fallback_without_gpu(lib):
    from jeromq_amd import _lib
    assert lib.cz_device_ok() == 0
    buf = ctypes.create_string_buffer(8192)
    p = ctypes.addressof(buf)
    assert lib.cz_relay_batch(p, p, None, 1, p, p, p, p, None, None) == _lib.CZ_EHIP
    assert lib.cz_relay_uniform(1, 100, p, 112, p, 128, p, 0, 1, p, 0, p, None) == _lib.CZ_EHIP
    assert not any(buf.raw)         # nothing was computed on the host


def test_python_bounds_checks():
    from jeromq_amd import batch
    d = np.zeros(3, dtype=DESC_DTYPE)
    d["in_off"], d["out_off"], d["len"], d["key_idx"], d["prev"] = (0, 200, 400), (8, 208, 408), 133, (0, 1, 2), (-1, 0, 1)
    to = np.zeros(3, dtype=batch.FANOUT_SUB_DTYPE)
    to["key_idx"] = (3, 3, 0)
    ok = dict(desc_np=d, to_np=to, count=3, in_bytes=533, out_bytes=541, nkeys=4, nstatus=3, nnonces=3)
    batch._check_relay_bounds(**ok)
    batch._check_relay_bounds(**dict(ok, nnonces=None, desc_np=None, to_np=None))
    for bad in (dict(in_bytes=532), dict(out_bytes=540), dict(nkeys=3), dict(nstatus=2), dict(nnonces=2), dict(count=4)):
        with pytest.raises(ValueError):
            batch._check_relay_bounds(**dict(ok, **bad))
    d2 = d.copy()
    d2["key_idx"][2] = 4                    # the inbound key index against the table
    with pytest.raises(ValueError):
        batch._check_relay_bounds(**dict(ok, desc_np=d2))
    d2 = d.copy()
    d2["prev"][0] = 3
    with pytest.raises(ValueError):
        batch._check_relay_bounds(**dict(ok, desc_np=d2))
    t2 = to.copy()
    t2["key_idx"][1] = 4                    # the outbound one
    with pytest.raises(ValueError):
        batch._check_relay_bounds(**dict(ok, to_np=t2))

    u = batch._check_relay_uniform_bounds   # (in_bytes, in_stride, out_bytes, out_stride, count, size, nstatus)
    u(3 * 4144, 4144, 3 * 4224, 4224, 3, 4129, 3)
    u(2 * 4144 + 4129, 4144, 2 * 4129 + 4129, 4129, 3, 4129, 3)     # a stride that owns nothing: bodies only
    u(0, 0, 0, 0, 0, 4129, 0)
    for a in ((3 * 4144 - 16, 4144, 3 * 4224, 4224, 3, 4129, 3), (3 * 4144, 4144, 3 * 4224 - 1, 4224, 3, 4129, 3),
              (3 * 4144, 4144, 3 * 4129 - 1, 4129, 3, 4129, 3), (3 * 4144, 4144, 3 * 4224, 4224, 3, 4129, 2),
              (3 * 4144, 4128, 3 * 4224, 4224, 3, 4129, 3), (3 * 4144, 4144, 3 * 4224, 4128, 3, 4129, 3)):
        with pytest.raises(ValueError):
            u(*a)

    class T:            # stand-ins for tensors: the checks run before any device call
        is_cuda = False
    with pytest.raises(ValueError):
        batch.relay_uniform(T(), 16, T(), 16, 1, 16, T(), 0, T(), 0, T())
    with pytest.raises(ValueError):
        batch.relay_batch(T(), T(), 1, T(), T(), T(), T())


# ---- the plan, through the launch-printing shim -------------------------------------------------------
LINES_LDS = 4 * (64 * 128 + 64 * 64)       # the seal's line emitter: a line and block 1 of every frame, 4 waves


def _expected_launches(ib, ist, ob, ost, n, size):
    """the issue's rule, restated: the line path for full waves when d_in, in_stride, d_out and out_stride
    are all 16-byte aligned, out_stride % 128 == 0 and below LINES_STRIDE_MAX, and size >= LINES_BYTES_MIN;
    everything else lane-wise, including the last partial wave"""
    args = lambda first, cnt, tail: (f"I+{ib + first * ist:x}", ist, f"O+{ob + first * ost:x}", ost, cnt, size, "K+0",  # noqa: E731
                                     5, 1, "K+20", 9 + first, f"A+{2 * first:x}", tail)
    lines = (ib | ist | ob | ost) % 16 == 0 and ost % 128 == 0 and ost < (1 << 25) and size >= 256
    full = n & ~63
    if lines and full:
        out = [("k_relay_uniform<1>", (full + 255) // 256, LINES_LDS, args(0, full, 0))]
        if n - full:
            out.append(("k_relay_uniform<0>", 1, 0, args(full, n - full, 1)))
        return out
    return [("k_relay_uniform<0>", (n + 255) // 256, 0, args(0, n, 0))]


@needs_hipcc
def test_plan_chooses_exactly_the_named_instantiations():
    text = dispatch_record.record(relay=True)
    cases, cur = [], None
    for ln in text.splitlines():
        m = re.fullmatch(r"relay (\d+)/(\d+) (\d+)/(\d+) n=(\d+) len=(\d+)", ln)
        if m:
            cur = (tuple(map(int, m.groups())), [])
            cases.append(cur)
        elif ln.startswith("  ") and cur:
            k, rest = ln[2:].split(" g=", 1)
            g, b, l, args = re.fullmatch(r"(\d+) b=(\d+) l=(\d+) :(.*)", rest).groups()
            assert b == "256"
            cur[1].append((k, int(g), int(l), tuple(int(a) if a.isdigit() else a for a in args.split())))
        else:
            assert ln.startswith("knob "), ln
            cur = None
    assert len(cases) > 250
    seen = set()
    for key, got in cases:
        want = _expected_launches(*key)
        assert got == want, (key, got, want)
        seen |= {k for k, *_ in got}
    assert seen == {"k_relay_uniform<1>", "k_relay_uniform<0>"} == dispatch_record.signatures(text)
    # both sides of every limit were visited
    keys = [k for k, _ in cases]
    assert any(k[5] == 255 and k[3] % 128 == 0 for k in keys) and any(k[5] == 256 and k[3] % 128 == 0 for k in keys)
    assert any(k[3] == (1 << 25) - 128 for k in keys) and any(k[3] == 1 << 25 for k in keys)
    assert {63, 64, 65, 127, 128, 129} <= {k[4] for k in keys}
    assert any(k[0] % 16 for k in keys) and any(k[2] % 16 for k in keys) and any(k[1] % 16 for k in keys)


@needs_hipcc
def test_default_record_holds_no_relay_case():
    """the relay's grid is behind its own flag: the default grid still records the parent's text
    (tests/test_dispatch_record.py compares it)"""
    assert "relay" not in open(os.path.join(ROOT, "tests", "golden", "dispatch_parent.txt")).read()
    src = open(os.path.join(ROOT, "tools", "dispatch_record", "driver.cpp")).read()
    main = src[src.index("int main("):]
    assert main.index("relay_cases()") < main.index("return 0;") < main.index("seal_cases()")


# ---- the CPU model against libzmq ----------------------------------------------------------------------
S = json.load(open(os.path.join(ROOT, "tests", "golden", "libzmq_session.json")))
PRECOM = bytes.fromhex(S["precom"])


def test_model_relays_what_libzmq_sealed():
    """bodies libzmq sealed (server to client) relayed under the session key in the other direction open in
    the oracle to the recorded payloads, flags & 3 and the outbound counter"""
    floor = 0
    for j, m in enumerate(S["s2c"]):
        body = bytes.fromhex(m["body"])
        counter = (1 << 40) + 3 * j
        st, nonce, out = relay_expect(body, floor, True, 1, PRECOM, counter, 0, PRECOM)
        assert st == (m["flags"] << 8) and nonce == m["nonce"] and len(out) == len(body)
        rc, payload, flags, n = or_curve_decode(out, 0, PRECOM)
        assert rc == 0 and payload == splitmix_bytes(m["n"], m["seed"]) and flags == m["flags"] & 3 and n == counter
        floor = nonce
        # a replay of it, and one damaged byte, leave zeros
        assert relay_expect(body, floor, True, 1, PRECOM, counter, 0, PRECOM) == (4, nonce, bytes(len(body)))
        bad = bytearray(body)
        bad[-1] ^= 1
        assert relay_expect(bytes(bad), floor - 1, True, 1, PRECOM, counter, 0, PRECOM) == (1, nonce, bytes(len(body)))


def test_model_is_the_identity_on_what_libzmq_accepted():
    """a body libzmq accepted, relayed under the same key and nonce, is that body again"""
    for m in S["c2s"]:
        body = bytes.fromhex(m["body"])
        st, nonce, out = relay_expect(body, m["nonce"] - 1, True, 0, PRECOM, m["nonce"], 0, PRECOM)
        assert st == (m["flags"] << 8) and nonce == m["nonce"]
        assert out == body or (m["flags"] & ~3)
