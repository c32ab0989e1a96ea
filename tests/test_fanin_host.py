"""CPU: the fan-in open (cz_plan_fanin, cz_open_fanin_runs, k_open_fanin_runs) without a device -- the
record layouts against the C header, every refusal of the planner with its outputs untouched, the capacity
protocol, the wave table (padding to whole waves, the class of every wave against pick_staging's rule
restated here, longest first inside a class, every (run, body) covered once), the launch's argument checks
before the device, no CPU fallback, the engine knob and accessor, and the kernels' AMDGPU metadata."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from cz_testlib import ROOT

HEADER = os.path.join(ROOT, "include", "curvezmq_mi355x.h")
RUN_FIELDS = ("in_off", "in_stride", "out_off", "out_stride", "size", "first_sub", "count", "reserved")
SUB_FIELDS = ("floor", "key_idx", "flags")
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
    offs = ",".join([f"offsetof(cz_fanin_run,{f})" for f in RUN_FIELDS] + [f"offsetof(cz_fanin_sub,{f})" for f in SUB_FIELDS])
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "curvezmq_mi355x.h"\n'
                 'int main(void){size_t v[] = {sizeof(cz_fanin_run),sizeof(cz_fanin_sub),' + offs + ',CZ_FANIN_CHECK_NONCE,'
                 'CZ_FANIN_FLOOR_IS_BODY};for (unsigned i = 0; i < sizeof v / sizeof *v; i++) printf("%zu ", v[i]);return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(c), "-o", str(exe)])
    want = [48, 16, 0, 8, 16, 24, 32, 36, 40, 44, 0, 8, 12, 1, 2]
    assert list(map(int, subprocess.check_output([str(exe)], text=True).split())) == want
    from jeromq_amd import _lib, batch
    assert ctypes.sizeof(_lib.cz_fanin_run) == 48 and ctypes.sizeof(_lib.cz_fanin_sub) == 16
    assert [getattr(_lib.cz_fanin_run, f).offset for f in RUN_FIELDS] == want[2:10]
    assert [getattr(_lib.cz_fanin_sub, f).offset for f in SUB_FIELDS] == want[10:13]
    assert batch.FANIN_RUN_DTYPE.itemsize == 48 and batch.FANIN_SUB_DTYPE.itemsize == 16
    assert [batch.FANIN_RUN_DTYPE.fields[f][1] for f in RUN_FIELDS] == want[2:10]
    assert [batch.FANIN_SUB_DTYPE.fields[f][1] for f in SUB_FIELDS] == want[10:13]
    assert (_lib.CZ_FANIN_CHECK_NONCE, _lib.CZ_FANIN_FLOOR_IS_BODY) == (1, 2)
    assert (batch.FANIN_CHECK_NONCE, batch.FANIN_FLOOR_IS_BODY) == (1, 2)


def make_runs(rows):
    from jeromq_amd import batch
    r = np.zeros(len(rows), dtype=batch.FANIN_RUN_DTYPE)
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
        return lib.cz_plan_fanin(runs.ctypes.data if runs is not None else None, len(runs) if nruns is None else nruns,
                                 d_in, d_out, self.waves.ctypes.data, self.cap, ctypes.byref(self.nwaves), self.cc,
                                 ctypes.byref(self.region))

    def untouched(self, nwaves_too=True):
        return (np.all(self.waves.view(np.uint64) == SENT) and list(self.cc) == [SENT] * 3 and self.region.value == SENT
                and (not nwaves_too or self.nwaves.value == SENT))


GOOD = dict(in_off=0, in_stride=256, out_off=0, out_stride=128, size=133, first_sub=0, count=130)


def test_plan_refusals_leave_the_outputs_untouched(lib):
    from jeromq_amd import _lib
    bad = [
        dict(GOOD, out_stride=99),                               # out_stride < nout with count > 1
        dict(GOOD, in_stride=132),                               # in_stride < size with count > 1
        dict(GOOD, size=0x80000000, in_stride=1 << 32, out_stride=1 << 32),   # size above 0x7fffffff
        dict(GOOD, first_sub=(1 << 32) - 100),                   # first_sub + count past 2^32
        dict(GOOD, out_off=(1 << 64) - 128 * 100),               # out_off + count * stride wraps
        dict(GOOD, in_off=(1 << 64) - 256 * 100),                # in_off + ... wraps
        dict(GOOD, out_stride=1 << 62, count=8),                 # count * stride wraps
        dict(GOOD, in_stride=1 << 62, count=8),
        dict(GOOD, out_stride=1 << 46, count=3),                 # ... or leaves the address space
        dict(GOOD, in_stride=1 << 46, count=4),
        dict(GOOD, count=1, in_off=1 << 47),                     # one body past the address space
    ]
    for row in bad:
        # the bad run last, behind two good ones: nothing may be planned before every run is checked
        runs = make_runs([GOOD, dict(GOOD, out_off=1 << 20, in_off=1 << 20), row])
        o = Outputs(64)
        assert o.call(lib, runs) == _lib.CZ_EINVAL, row
        assert o.untouched(), row
    # one frame needs no stride: the same strides pass with count 1
    o = Outputs(64)
    assert o.call(lib, make_runs([dict(GOOD, out_stride=99, in_stride=1, count=1)])) == _lib.CZ_OK
    runs = make_runs([GOOD])
    o = Outputs(64)
    assert o.call(lib, None, nruns=1) == _lib.CZ_EINVAL and o.untouched()
    assert o.call(lib, runs, d_in=None) == _lib.CZ_EINVAL and o.untouched()
    assert o.call(lib, runs, d_out=None) == _lib.CZ_EINVAL and o.untouched()
    w, cc, n, rs = o.waves.ctypes.data, o.cc, ctypes.byref(o.nwaves), ctypes.byref(o.region)
    assert lib.cz_plan_fanin(runs.ctypes.data, 1, 4096, 8192, w, 64, None, cc, rs) == _lib.CZ_EINVAL
    assert lib.cz_plan_fanin(runs.ctypes.data, 1, 4096, 8192, w, 64, n, None, rs) == _lib.CZ_EINVAL
    assert lib.cz_plan_fanin(runs.ctypes.data, 1, 4096, 8192, w, 64, n, cc, None) == _lib.CZ_EINVAL
    assert o.untouched()


def test_plan_capacity_protocol(lib):
    from jeromq_amd import _lib
    runs = make_runs([GOOD, dict(GOOD, out_off=1 << 20, in_off=1 << 20, count=64),
                      dict(GOOD, out_off=2 << 20, in_off=2 << 20, count=1)])
    need = 3 + 1 + 1
    for cap in (0, need - 1):
        o = Outputs(cap)
        assert o.call(lib, runs) == _lib.CZ_EINVAL
        assert o.nwaves.value == need and o.untouched(nwaves_too=False)
    o = Outputs(need)
    assert lib.cz_plan_fanin(runs.ctypes.data, 3, 4096, 8192, None, need, ctypes.byref(o.nwaves), o.cc,
                             ctypes.byref(o.region)) == _lib.CZ_EINVAL      # a null table with waves to write
    assert o.nwaves.value == need and o.untouched(nwaves_too=False)
    o = Outputs(need + 2)
    assert o.call(lib, runs) == _lib.CZ_OK
    assert o.nwaves.value == need and sum(o.cc) == need
    assert np.all(o.waves.view(np.uint64)[need:] == SENT)                    # nothing past the table's end
    # no runs, and runs without bodies: an empty table, CZ_OK
    o = Outputs(0)
    assert lib.cz_plan_fanin(None, 0, None, None, None, 0, ctypes.byref(o.nwaves), o.cc, ctypes.byref(o.region)) == _lib.CZ_OK
    assert o.nwaves.value == 0 and list(o.cc) == [0, 0, 0] and o.region.value == 0
    o = Outputs(0)
    assert o.call(lib, make_runs([dict(GOOD, count=0), dict(GOOD, count=0, size=5000, out_stride=5120)])) == _lib.CZ_OK
    assert o.nwaves.value == 0 and list(o.cc) == [0, 0, 0]


def staging(stride, size, count, aligned):
    """pick_staging's rule for the plaintext slots of one run (restated, not imported)"""
    nout = size - 33 if size >= 33 else 0
    if count < 64 or not aligned:
        return DIRECT
    if stride % 128 == 0 and nout >= 256 and stride < (1 << 25):
        return LINES
    if stride % 16 == 0 and 64 * stride <= 16384:
        return REGION
    return DIRECT


def round_up(v, a):
    return (v + a - 1) // a * a


def mixed_runs(rng, n):
    rows, off, ioff = [], 0, 0
    for k in range(n):
        size = int(rng.choice([0, 20, 33, 34, 133, 288, 289, 1033, 4129]))      # nout 255 / 256: the line-class edge
        nout = max(size - 33, 0)
        stride = [round_up(nout, 128), round_up(nout, 128) + 128, round_up(nout, 16), nout, nout + 7][k % 5]
        in_stride = [round_up(size, 128), size, round_up(size, 16), size + 8][(k // 2) % 4]
        count = int(rng.choice([0, 1, 63, 64, 65, 128, 130, 257]))
        out_off = off + [0, 0, 16, 8, 1][(k // 5) % 5]
        in_off = ioff + [0, 16, 8, 1][(k // 3) % 4]
        rows.append(dict(in_off=in_off, in_stride=in_stride, out_off=out_off, out_stride=stride, size=size,
                         first_sub=int(rng.integers(0, 1000)), count=count))
        off = round_up(out_off + count * stride + 64, 128)
        ioff = round_up(in_off + count * in_stride + 64, 128)
    return make_runs(rows)


@pytest.mark.parametrize("d_in,d_out", [(1 << 20, 1 << 30), ((1 << 20) + 8, 1 << 30), (1 << 20, (1 << 30) + 1),
                                        ((1 << 20) + 16, (1 << 30) + 48)])
def test_plan_wave_table(lib, d_in, d_out):
    from jeromq_amd import _lib
    rng = np.random.default_rng(d_in ^ d_out)
    runs = mixed_runs(rng, 120)
    total = int(sum((int(c) + 63) // 64 for c in runs["count"]))
    o = Outputs(total)
    assert o.call(lib, runs, d_in=d_in, d_out=d_out) == _lib.CZ_OK
    assert o.nwaves.value == total                       # every run padded to whole waves; count 0 gives none
    assert sum(o.cc) == total
    waves = o.waves[:total]
    cls, region = [], 0
    for w in waves:
        r = runs[int(w["run"])]
        al = ((d_in + int(r["in_off"])) | int(r["in_stride"]) | (d_out + int(r["out_off"])) | int(r["out_stride"])) % 16 == 0
        st = staging(int(r["out_stride"]), int(r["size"]), int(r["count"]), al)
        assert int(w["first"]) % 64 == 0 and int(w["first"]) < int(r["count"])
        full = int(w["first"]) + 64 <= int(r["count"])
        cls.append(st if full else DIRECT)               # partial waves are lane-wise
        if st == REGION:
            region = max(region, int(r["out_stride"]))
    assert cls == [LINES] * o.cc[LINES] + [REGION] * o.cc[REGION] + [DIRECT] * o.cc[DIRECT]
    assert o.region.value == region
    if d_in % 16 == 0 and d_out % 16 == 0:
        assert o.cc[LINES] and o.cc[REGION] and o.cc[DIRECT]
    at = 0
    for c in (LINES, REGION, DIRECT):                    # longest size first inside a class
        sizes = [int(runs["size"][int(w["run"])]) for w in waves[at:at + o.cc[c]]]
        assert sizes == sorted(sizes, reverse=True), c
        at += o.cc[c]
    got = sorted((int(w["run"]), int(w["first"])) for w in waves)
    want = sorted((k, f) for k, c in enumerate(runs["count"]) for f in range(0, int(c), 64))
    assert got == want


def test_plan_line_class_edge_and_alignment(lib):
    """nout 255 stays with the region class at a 256-byte stride, nout 256 is the first line-class payload;
    any of the four alignments off 16 bytes makes the run lane-wise"""
    from jeromq_amd import _lib
    a = dict(in_off=0, in_stride=384, out_off=0, out_stride=256, size=288, first_sub=0, count=128)     # nout 255
    b = dict(a, in_off=1 << 20, out_off=1 << 20, size=289)                                              # nout 256
    o = Outputs(4)
    assert o.call(lib, make_runs([a, b])) == _lib.CZ_OK
    assert list(o.cc) == [2, 2, 0] and o.region.value == 256
    assert [int(r) for r in o.waves["run"][:4]] == [1, 1, 0, 0]
    for shift in (dict(d_in=4097), dict(d_in=4104), dict(d_out=8193), dict(d_out=8200)):
        o = Outputs(4)
        assert o.call(lib, make_runs([a, b]), **shift) == _lib.CZ_OK
        assert list(o.cc) == [0, 0, 4] and o.region.value == 0, shift
    for field, v in (("in_stride", 392), ("out_stride", 264), ("in_off", 8), ("out_off", 1)):
        o = Outputs(4)
        assert o.call(lib, make_runs([dict(a, **{field: v}), b])) == _lib.CZ_OK
        assert list(o.cc) == [2, 0, 2], field


def test_python_plan(lib):
    from jeromq_amd import batch
    runs = make_runs([GOOD, dict(GOOD, in_off=1 << 20, out_off=1 << 20, size=1033, in_stride=1152, out_stride=1024,
                                 count=65)])
    p = batch.plan_fanin(runs, 4096, 8192)
    assert isinstance(p, batch.FaninPlan)
    assert (p.nruns, p.nwaves, p.class_count, p.region_stride) == (2, 5, [1, 2, 2], 128)
    assert p.waves.dtype == batch.FANOUT_WAVE_DTYPE and len(p.waves) == 5
    assert batch.plan_fanin(runs[:0], 4096, 8192).nwaves == 0


def test_launch_arguments_are_checked_before_the_device(lib):
    from jeromq_amd import _lib
    f = lib.cz_open_fanin_runs
    p = 4096  # any non-null address: a rejected call never reads it
    cc = (ctypes.c_uint32 * 3)(1, 1, 1)
    for k in (0, 2, 5, 6, 7, 8, 9):     # d_runs, d_waves, d_in, d_subs, d_subkeys, d_out, d_status
        a = [p, 2, p, cc, 256, p, p, p, p, p, None, None]
        a[k] = None
        assert f(*a) == _lib.CZ_EINVAL, k
    assert f(p, 2, p, None, 256, p, p, p, p, p, None, None) == _lib.CZ_EINVAL
    # nothing to do, nothing launched, nothing read
    assert f(None, 0, None, cc, 0, None, None, None, None, None, None, None) == _lib.CZ_OK
    assert f(None, 3, None, (ctypes.c_uint32 * 3)(0, 0, 0), 0, None, None, None, None, None, None, None) == _lib.CZ_OK


@pytest.mark.skipif(os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK), reason="GPU present")
def test_no_cpu_fallback(lib):
    from jeromq_amd import _lib
    runs = make_runs([dict(GOOD, count=4)])
    o = Outputs(1)
    assert o.call(lib, runs) == _lib.CZ_OK
    body = ctypes.create_string_buffer(4 * 256)
    subs = (_lib.cz_fanin_sub * 4)()
    keys = ctypes.create_string_buffer(32)
    out = ctypes.create_string_buffer(b"\x5a" * (4 * 128), 4 * 128)
    status = (ctypes.c_uint16 * 4)(*([0x5a5a] * 4))
    adr = ctypes.addressof
    assert lib.cz_open_fanin_runs(runs.ctypes.data, 1, o.waves.ctypes.data, o.cc, o.region.value, adr(body), adr(subs),
                                  adr(keys), adr(out), adr(status), None, None) == _lib.CZ_EHIP
    assert out.raw == b"\x5a" * (4 * 128) and list(status) == [0x5a5a] * 4


def test_python_bounds_checks(lib):
    """batch.open_fanin_runs' host-side checks, on stand-ins for the tensors (nothing is launched)"""
    from jeromq_amd import batch

    class T:
        def __init__(self, n):
            self.n = n

        def numel(self):
            return self.n

    runs = make_runs([dict(GOOD, count=4)])          # bodies end at 3 * 256 + 133, owned slots at 4 * 128
    ok = (T(901), T(512), None, 4, T(4), T(4))
    batch._check_fanin_bounds(runs, *ok)
    for k, small in ((0, T(900)), (1, T(511)), (3, 3), (4, T(3)), (5, T(3))):
        a = list(ok)
        a[k] = small
        with pytest.raises(ValueError):
            batch._check_fanin_bounds(runs, *a)
    subs = np.zeros(4, dtype=batch.FANIN_SUB_DTYPE)
    subs["flags"][1] = batch.FANIN_CHECK_NONCE | batch.FANIN_FLOOR_IS_BODY
    subs["floor"] = (1 << 40, 901 - 16, 1 << 40, 1 << 40)          # plain floors may be any value
    batch._check_fanin_bounds(runs, ok[0], ok[1], subs, *ok[3:])
    subs["floor"][1] = 901 - 15
    with pytest.raises(ValueError):
        batch._check_fanin_bounds(runs, ok[0], ok[1], subs, *ok[3:])


def test_tune_fanin_short(lib):
    """the knob's protocol as the other knobs: the previous value comes back, negative values clamp to 0"""
    old = lib.cz_tune(b"fanin_short", 4096)
    try:
        assert lib.cz_tune(b"fanin_short", -5) == 4096
        assert lib.cz_tune(b"fanin_short", 100) == 0
        assert lib.cz_tune(b"fanin_short", 100) == 100
    finally:
        lib.cz_tune(b"fanin_short", old)
    assert lib.cz_tune(b"fanin_short", old) == old


def test_shipped_default_is_the_measured_rule(lib):
    """the shipped fanin_short is what the rule gives from the committed measurement (tools/fanin_bench.py)"""
    import json
    with open(os.path.join(ROOT, "profiles", "fanin", "fanin.json")) as f:
        measured = json.load(f)
    default = lib.cz_tune(b"fanin_short", 0)
    lib.cz_tune(b"fanin_short", default)
    assert default == measured["fanin_short_rule"]
    sys_path_tools = os.path.join(ROOT, "tools")
    import importlib.util
    spec = importlib.util.spec_from_file_location("fanin_bench", os.path.join(sys_path_tools, "fanin_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.fanin_short_rule(measured["device_legs"], measured["engine"])[1] == default


def test_engine_accessor_without_an_engine(lib):
    assert lib.cz_engine_fanin_frames(None) == 0


def test_kernel_metadata(product):
    from test_acceptor_host import kernel_notes
    from test_occupancy import waves_per_simd
    notes = kernel_notes(product)
    runs = [(n, f) for n, f in notes.items() if re.search(r"\d+k_open_fanin_runsI", n)]
    assert len(runs) == 3, [n for n, _ in runs]  # ST_LINES, ST_REGION, ST_DIRECT
    for name, f in runs:
        assert f["private_segment_fixed_size"] == 0, f"{name} uses {f['private_segment_fixed_size']} bytes of scratch"
        assert f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, name
        got = waves_per_simd(f["vgpr_count"], f["agpr_count"])
        assert got >= 3, f"{name}: {f['vgpr_count']} VGPRs + {f['agpr_count']} AGPRs = {got} waves per SIMD"
        assert f["group_segment_fixed_size"] == 0, name   # dynamic LDS only: the launch sizes each class's own
