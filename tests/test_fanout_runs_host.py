"""CPU: the grouped PUB fan-out (cz_plan_fanout, cz_seal_fanout_runs, k_seal_fanout_runs) without a device --
the run and wave records' layouts against the C header, every refusal of the planner with its outputs
untouched, the capacity protocol, the wave table (padding to whole waves, the class of every wave against
pick_staging's rule restated here, longest first inside a class, every (run, subscriber) covered once), the
launch's argument checks before the device, no CPU fallback, and the kernels' AMDGPU metadata read as
tests/test_fanout_host.py reads it."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from cz_testlib import ROOT

HEADER = os.path.join(ROOT, "include", "curvezmq_mi355x.h")
RUN_FIELDS = ("payload_off", "out_off", "out_stride", "len", "flags", "first_sub", "count")
LINES, REGION, DIRECT = 0, 1, 2
SENT = 0xDEADBEEF


@pytest.fixture(scope="module")
def product():
    from jeromq_amd import build
    build.build_library()
    return build


@pytest.fixture(scope="module")
def lib(product):
    from jeromq_amd import _lib
    return _lib.lib()


def test_layouts_match_c(tmp_path):
    c = tmp_path / "layout.c"
    offs = ",".join(f"offsetof(cz_fanout_run,{f})" for f in RUN_FIELDS)
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "curvezmq_mi355x.h"\n'
                 'int main(void){size_t v[] = {sizeof(cz_fanout_run),' + offs + ',sizeof(cz_fanout_wave),'
                 'offsetof(cz_fanout_wave,run),offsetof(cz_fanout_wave,first),CZ_FANOUT_LINES,CZ_FANOUT_REGION,'
                 'CZ_FANOUT_DIRECT};for (unsigned i = 0; i < sizeof v / sizeof *v; i++) printf("%zu ", v[i]);return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(c), "-o",
                           str(exe)])
    want = [40, 0, 8, 16, 24, 28, 32, 36, 8, 0, 4, LINES, REGION, DIRECT]
    assert list(map(int, subprocess.check_output([str(exe)], text=True).split())) == want
    from jeromq_amd import _lib, batch
    assert ctypes.sizeof(_lib.cz_fanout_run) == 40 and ctypes.sizeof(_lib.cz_fanout_wave) == 8
    assert [getattr(_lib.cz_fanout_run, f).offset for f in RUN_FIELDS] == want[1:8]
    assert [getattr(_lib.cz_fanout_wave, f).offset for f in ("run", "first")] == [0, 4]
    assert batch.FANOUT_RUN_DTYPE.itemsize == 40 and batch.FANOUT_WAVE_DTYPE.itemsize == 8
    assert [batch.FANOUT_RUN_DTYPE.fields[f][1] for f in RUN_FIELDS] == want[1:8]
    assert [batch.FANOUT_WAVE_DTYPE.fields[f][1] for f in ("run", "first")] == [0, 4]
    assert (_lib.CZ_FANOUT_LINES, _lib.CZ_FANOUT_REGION, _lib.CZ_FANOUT_DIRECT) == (LINES, REGION, DIRECT)


def make_runs(rows):
    from jeromq_amd import batch
    r = np.zeros(len(rows), dtype=batch.FANOUT_RUN_DTYPE)
    for k, row in enumerate(rows):
        for f, v in row.items():
            r[f][k] = v
    return r


class Outputs:
    """the planner's outputs, pre-filled so that a refused call can be shown to have written nothing"""

    def __init__(self, cap):
        from jeromq_amd import batch
        self.waves = np.full(max(cap, 1), SENT, dtype=np.uint64).view(batch.FANOUT_WAVE_DTYPE)
        self.cap = cap
        self.nwaves, self.region = ctypes.c_uint32(SENT), ctypes.c_uint32(SENT)
        self.cc = (ctypes.c_uint32 * 3)(SENT, SENT, SENT)

    def call(self, lib, runs, d_in=4096, d_out=8192, nruns=None):
        return lib.cz_plan_fanout(runs.ctypes.data if runs is not None else None, len(runs) if nruns is None else nruns,
                                  d_in, d_out, self.waves.ctypes.data, self.cap, ctypes.byref(self.nwaves), self.cc,
                                  ctypes.byref(self.region))

    def untouched(self, nwaves_too=True):
        return (np.all(self.waves.view(np.uint64) == SENT) and list(self.cc) == [SENT] * 3 and self.region.value == SENT
                and (not nwaves_too or self.nwaves.value == SENT))


GOOD = dict(payload_off=0, out_off=0, out_stride=256, len=100, flags=1, first_sub=0, count=130)


def test_plan_refusals_leave_the_outputs_untouched(lib):
    from jeromq_amd import _lib
    bad = [
        (dict(GOOD, len=_lib.CZ_MESSAGE_MAX + 1, out_stride=1 << 32), _lib.CZ_EMSGSIZE),
        (dict(GOOD, out_stride=132), _lib.CZ_EINVAL),                               # out_stride < len + 33
        (dict(GOOD, out_stride=132, count=0), _lib.CZ_EINVAL),                      # ... in an empty run too
        (dict(GOOD, first_sub=(1 << 32) - 100), _lib.CZ_EINVAL),                    # first_sub + count overflows
        (dict(GOOD, out_off=(1 << 64) - 256 * 100), _lib.CZ_EINVAL),                # out_off + count * stride wraps
        (dict(GOOD, out_stride=1 << 62, count=8), _lib.CZ_EINVAL),                  # count * stride wraps
        (dict(GOOD, out_stride=1 << 46, count=3), _lib.CZ_EINVAL),                  # ... or leaves the address space
    ]
    for row, rc in bad:
        # the bad run last, behind two good ones: nothing may be planned before every run is checked
        runs = make_runs([GOOD, dict(GOOD, out_off=1 << 20), row])
        o = Outputs(64)
        assert o.call(lib, runs) == rc, row
        assert o.untouched(), row
    runs = make_runs([GOOD])
    o = Outputs(64)
    assert o.call(lib, None, nruns=1) == _lib.CZ_EINVAL and o.untouched()
    assert o.call(lib, runs, d_in=None) == _lib.CZ_EINVAL and o.untouched()
    assert o.call(lib, runs, d_out=None) == _lib.CZ_EINVAL and o.untouched()
    w, cc, n, rs = o.waves.ctypes.data, o.cc, ctypes.byref(o.nwaves), ctypes.byref(o.region)
    assert lib.cz_plan_fanout(runs.ctypes.data, 1, 4096, 8192, w, 64, None, cc, rs) == _lib.CZ_EINVAL
    assert lib.cz_plan_fanout(runs.ctypes.data, 1, 4096, 8192, w, 64, n, None, rs) == _lib.CZ_EINVAL
    assert lib.cz_plan_fanout(runs.ctypes.data, 1, 4096, 8192, w, 64, n, cc, None) == _lib.CZ_EINVAL
    assert o.untouched()


def test_plan_capacity_protocol(lib):
    from jeromq_amd import _lib
    runs = make_runs([GOOD, dict(GOOD, out_off=1 << 20, count=64), dict(GOOD, out_off=2 << 20, count=1)])
    need = 3 + 1 + 1
    for cap in (0, need - 1):
        o = Outputs(cap)
        assert o.call(lib, runs) == _lib.CZ_EINVAL
        assert o.nwaves.value == need and o.untouched(nwaves_too=False)
    o = Outputs(need)
    assert lib.cz_plan_fanout(runs.ctypes.data, 3, 4096, 8192, None, need, ctypes.byref(o.nwaves), o.cc,
                              ctypes.byref(o.region)) == _lib.CZ_EINVAL      # a null table with waves to write
    assert o.nwaves.value == need and o.untouched(nwaves_too=False)
    o = Outputs(need + 2)
    assert o.call(lib, runs) == _lib.CZ_OK
    assert o.nwaves.value == need and sum(o.cc) == need
    assert np.all(o.waves.view(np.uint64)[need:] == SENT)                    # nothing past the table's end
    # no runs, and runs without subscribers: an empty table, CZ_OK
    o = Outputs(0)
    assert lib.cz_plan_fanout(None, 0, None, None, None, 0, ctypes.byref(o.nwaves), o.cc, ctypes.byref(o.region)) == _lib.CZ_OK
    assert o.nwaves.value == 0 and list(o.cc) == [0, 0, 0] and o.region.value == 0
    o = Outputs(0)
    assert o.call(lib, make_runs([dict(GOOD, count=0), dict(GOOD, count=0, len=5000, out_stride=5120)])) == _lib.CZ_OK
    assert o.nwaves.value == 0 and list(o.cc) == [0, 0, 0]


def staging(stride, length, count, aligned):
    """pick_staging's rule as czk_seal_fanout applies it to one run (restated, not imported)"""
    mlen = length + 33
    if count < 64 or not aligned:
        return DIRECT
    if stride % 128 == 0 and mlen >= 256 and stride < (1 << 25):
        return LINES
    if stride % 16 == 0 and 64 * stride <= 16384:
        return REGION
    return DIRECT


def round_up(v, a):
    return (v + a - 1) // a * a


def mixed_runs(rng, n):
    rows, off = [], 0
    for k in range(n):
        length = int(rng.choice([0, 31, 47, 100, 222, 223, 224, 1000, 4097]))
        mlen = length + 33
        stride = [round_up(mlen, 128), round_up(mlen, 128) + 128, round_up(mlen, 16), mlen, mlen + 7][k % 5]
        count = int(rng.choice([0, 1, 63, 64, 65, 128, 130, 257]))
        out_off = off + [0, 0, 16, 8, 1][(k // 5) % 5]
        rows.append(dict(payload_off=int(rng.integers(0, 64)) * [16, 16, 8, 1][k % 4], out_off=out_off,
                         out_stride=stride, len=length, flags=k % 4, first_sub=int(rng.integers(0, 1000)), count=count))
        off = round_up(out_off + count * stride + 64, 128)
    return make_runs(rows)


@pytest.mark.parametrize("d_in,d_out", [(1 << 20, 1 << 30), ((1 << 20) + 8, 1 << 30), (1 << 20, (1 << 30) + 1),
                                        ((1 << 20) + 16, (1 << 30) + 48)])
def test_plan_wave_table(lib, d_in, d_out):
    from jeromq_amd import _lib
    rng = np.random.default_rng(d_in ^ d_out)
    runs = mixed_runs(rng, 60)
    total = int(sum((int(c) + 63) // 64 for c in runs["count"]))
    o = Outputs(total)
    assert o.call(lib, runs, d_in=d_in, d_out=d_out) == _lib.CZ_OK
    assert o.nwaves.value == total                       # every run padded to whole waves
    assert sum(o.cc) == total
    waves = o.waves[:total]
    # the class of every wave: its run's staging choice for a full wave, lane-wise for a partial one
    cls, region = [], 0
    for w in waves:
        r = runs[int(w["run"])]
        al = ((d_in + int(r["payload_off"])) | (d_out + int(r["out_off"])) | int(r["out_stride"])) % 16 == 0
        st = staging(int(r["out_stride"]), int(r["len"]), int(r["count"]), al)
        assert int(w["first"]) % 64 == 0 and int(w["first"]) < int(r["count"])
        full = int(w["first"]) + 64 <= int(r["count"])
        cls.append(st if full else DIRECT)
        if st == REGION:
            region = max(region, int(r["out_stride"]))
    assert cls == [LINES] * o.cc[LINES] + [REGION] * o.cc[REGION] + [DIRECT] * o.cc[DIRECT]
    assert o.region.value == region
    if d_in % 16 == 0 and d_out % 16 == 0:
        assert o.cc[LINES] and o.cc[REGION] and o.cc[DIRECT]          # the traffic reaches every class
    # longest payload first inside a class
    at = 0
    for c in (LINES, REGION, DIRECT):
        lens = [int(runs["len"][int(w["run"])]) for w in waves[at:at + o.cc[c]]]
        assert lens == sorted(lens, reverse=True), c
        at += o.cc[c]
    # every (run, subscriber) exactly once
    got = sorted((int(w["run"]), int(w["first"])) for w in waves)
    want = sorted((k, f) for k, c in enumerate(runs["count"]) for f in range(0, int(c), 64))
    assert got == want


def test_plan_unaligned_base_means_lane_wise(lib):
    """an output base at byte phase 1 leaves no run 16-byte aligned (offsets here are multiples of 8): every
    wave is lane-wise and the region stride is 0"""
    from jeromq_amd import _lib
    runs = make_runs([dict(GOOD, count=256), dict(GOOD, out_off=1 << 20, len=1000, out_stride=1152, count=128)])
    o = Outputs(6)
    assert o.call(lib, runs, d_out=8193) == _lib.CZ_OK
    assert list(o.cc) == [0, 0, 6] and o.region.value == 0
    o = Outputs(6)
    assert o.call(lib, runs) == _lib.CZ_OK
    assert list(o.cc) == [2, 4, 0] and o.region.value == 256
    assert [int(r) for r in o.waves["run"][:6]] == [1, 1, 0, 0, 0, 0]


def test_python_plan(lib):
    from jeromq_amd import batch
    runs = make_runs([GOOD, dict(GOOD, out_off=1 << 20, len=1000, out_stride=1152, count=65)])
    p = batch.plan_fanout(runs, 4096, 8192)
    assert (p.nruns, p.nwaves, p.class_count, p.region_stride) == (2, 5, [1, 2, 2], 256)
    assert p.waves.dtype == batch.FANOUT_WAVE_DTYPE and len(p.waves) == 5
    assert batch.plan_fanout(runs[:0], 4096, 8192).nwaves == 0


def test_launch_arguments_are_checked_before_the_device(lib):
    from jeromq_amd import _lib
    f = lib.cz_seal_fanout_runs
    p = 4096  # any non-null address: a rejected call never reads it
    cc = (ctypes.c_uint32 * 3)(1, 1, 1)
    for k in (0, 2, 5, 6, 7, 8):
        a = [p, 2, p, cc, 256, p, p, p, p, None]
        a[k] = None
        assert f(*a) == _lib.CZ_EINVAL, k
    assert f(p, 2, p, None, 256, p, p, p, p, None) == _lib.CZ_EINVAL
    # nothing to do, nothing launched, nothing read
    assert f(None, 0, None, cc, 0, None, None, None, None, None) == _lib.CZ_OK
    assert f(None, 3, None, (ctypes.c_uint32 * 3)(0, 0, 0), 0, None, None, None, None, None) == _lib.CZ_OK


@pytest.mark.skipif(os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK), reason="GPU present")
def test_no_cpu_fallback(lib):
    from jeromq_amd import _lib
    runs = make_runs([dict(GOOD, count=4)])
    o = Outputs(1)
    assert o.call(lib, runs) == _lib.CZ_OK
    pay = ctypes.create_string_buffer(128)
    subs = (_lib.cz_fanout_sub * 4)()
    keys = ctypes.create_string_buffer(32)
    out = ctypes.create_string_buffer(4 * 256)
    adr = ctypes.addressof
    assert lib.cz_seal_fanout_runs(runs.ctypes.data, 1, o.waves.ctypes.data, o.cc, o.region.value, adr(pay), adr(subs),
                                   adr(keys), adr(out), None) == _lib.CZ_EHIP
    assert out.raw == bytes(4 * 256)


def test_tune_fanout_short(lib):
    """the knob's protocol as the other knobs: the previous value comes back, negative values clamp to 0"""
    old = lib.cz_tune(b"fanout_short", 4096)
    try:
        assert lib.cz_tune(b"fanout_short", -5) == 4096
        assert lib.cz_tune(b"fanout_short", 100) == 0
        assert lib.cz_tune(b"fanout_short", 100) == 100
    finally:
        lib.cz_tune(b"fanout_short", old)
    assert lib.cz_tune(b"fanout_short", old) == old


def test_kernel_metadata(product):
    from test_acceptor_host import kernel_notes
    from test_occupancy import waves_per_simd
    assert len(product.device_code_objects(product.PRODUCT_LIB)) == 4
    notes = kernel_notes(product)
    runs = [(n, f) for n, f in notes.items() if re.search(r"\d+k_seal_fanout_runsI", n)]
    assert len(runs) == 3, [n for n, _ in runs]  # ST_LINES, ST_REGION, ST_DIRECT
    for name, f in runs:
        assert f["private_segment_fixed_size"] == 0, f"{name} uses {f['private_segment_fixed_size']} bytes of scratch"
        assert f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, name
        got = waves_per_simd(f["vgpr_count"], f["agpr_count"])
        assert got >= 3, f"{name}: {f['vgpr_count']} VGPRs + {f['agpr_count']} AGPRs = {got} waves per SIMD"
        assert f["group_segment_fixed_size"] == 0, name   # dynamic LDS only: the launch sizes each class's own
    assert len([n for n in notes if re.search(r"\d+k_seal_fanoutI", n)]) == 3
