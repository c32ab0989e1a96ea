"""CPU: the split PUB fan-out (cz_plan_fanout_split, cz_seal_fanout_split, k_seal_fanout_tiles, k_fanout_join)
without a device -- the tile and join records' layouts against the C header, every refusal of the planner with
its outputs untouched, the capacity protocol, the cut points against cz_plan_segments' for one descriptor of the
same length, every (run, subscriber, block) covered by exactly one tile, the partial-record ranges, the class and
longest-first order, the launch's argument checks before the device, no CPU fallback, and the kernels' AMDGPU
metadata read as tests/test_fanout_runs_host.py reads it."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from cz_testlib import DESC_DTYPE, ROOT
from test_fanout_runs_host import GOOD, make_runs, round_up

HEADER = os.path.join(ROOT, "include", "curvezmq_mi355x.h")
TILE_FIELDS = ("run", "first", "first_block", "nblocks", "part", "nseg")
JOIN_FIELDS = ("run", "first", "part", "nseg")
LINES, DIRECT = 0, 1
WHOLE = 0xFFFFFFFF
SENT = 0xDEADBEEF
# payload lengths at the box's block edges: body block counts 1, 1, 2, 3, 4, 4, 4, 4, 5, 7, 64, 65, 1025
EDGE_LENS = [0, 31, 95, 159, 160, 175, 176, 223, 224, 415, 4063, 4096, 65536]


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
    offs = ",".join([f"offsetof(cz_fanout_tile,{f})" for f in TILE_FIELDS] + ["sizeof(cz_fanout_join)"] +
                    [f"offsetof(cz_fanout_join,{f})" for f in JOIN_FIELDS])
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "curvezmq_mi355x.h"\n'
                 'int main(void){size_t v[] = {sizeof(cz_fanout_tile),' + offs + ',CZ_FANOUT_TILE_LINES,'
                 'CZ_FANOUT_TILE_DIRECT};for (unsigned i = 0; i < sizeof v / sizeof *v; i++) printf("%zu ", v[i]);return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(c), "-o",
                           str(exe)])
    want = [24, 0, 4, 8, 12, 16, 20, 16, 0, 4, 8, 12, LINES, DIRECT]
    assert list(map(int, subprocess.check_output([str(exe)], text=True).split())) == want
    from jeromq_amd import _lib, batch
    assert ctypes.sizeof(_lib.cz_fanout_tile) == 24 and ctypes.sizeof(_lib.cz_fanout_join) == 16
    assert [getattr(_lib.cz_fanout_tile, f).offset for f in TILE_FIELDS] == want[1:7]
    assert [getattr(_lib.cz_fanout_join, f).offset for f in JOIN_FIELDS] == want[8:12]
    assert batch.FANOUT_TILE_DTYPE.itemsize == 24 and batch.FANOUT_JOIN_DTYPE.itemsize == 16
    assert [batch.FANOUT_TILE_DTYPE.fields[f][1] for f in TILE_FIELDS] == want[1:7]
    assert [batch.FANOUT_JOIN_DTYPE.fields[f][1] for f in JOIN_FIELDS] == want[8:12]
    assert (_lib.CZ_FANOUT_TILE_LINES, _lib.CZ_FANOUT_TILE_DIRECT) == (LINES, DIRECT)


class Outputs:
    """the planner's outputs, pre-filled so that a refused call can be shown to have written nothing"""

    def __init__(self, tile_cap, join_cap=None):
        from jeromq_amd import batch
        join_cap = tile_cap if join_cap is None else join_cap
        self.tiles = np.full(max(tile_cap, 1) * 6, SENT, dtype=np.uint32).view(batch.FANOUT_TILE_DTYPE)
        self.joins = np.full(max(join_cap, 1) * 4, SENT, dtype=np.uint32).view(batch.FANOUT_JOIN_DTYPE)
        self.tile_cap, self.join_cap = tile_cap, join_cap
        self.ntiles, self.njoins, self.npart = ctypes.c_uint32(SENT), ctypes.c_uint32(SENT), ctypes.c_uint32(SENT)
        self.cc = (ctypes.c_uint32 * 2)(SENT, SENT)

    def call(self, lib, runs, d_in=4096, seg_blocks=2, nruns=None):
        return lib.cz_plan_fanout_split(runs.ctypes.data if runs is not None else None,
                                        len(runs) if nruns is None else nruns, d_in, seg_blocks, self.tiles.ctypes.data,
                                        self.tile_cap, ctypes.byref(self.ntiles), self.cc, self.joins.ctypes.data,
                                        self.join_cap, ctypes.byref(self.njoins), ctypes.byref(self.npart))

    def tables_untouched(self):
        return (np.all(self.tiles.view(np.uint32) == SENT) and np.all(self.joins.view(np.uint32) == SENT)
                and list(self.cc) == [SENT] * 2)

    def untouched(self):
        return self.tables_untouched() and [self.ntiles.value, self.njoins.value, self.npart.value] == [SENT] * 3


def test_plan_refusals_leave_the_outputs_untouched(lib):
    """every refusal of cz_plan_fanout, the bad run last behind two good ones"""
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
        runs = make_runs([GOOD, dict(GOOD, out_off=1 << 20), row])
        for seg in (0, 1, 2):
            o = Outputs(64)
            assert o.call(lib, runs, seg_blocks=seg) == rc, row
            assert o.untouched(), row
    runs = make_runs([GOOD])
    o = Outputs(64)
    assert o.call(lib, None, nruns=1) == _lib.CZ_EINVAL and o.untouched()
    assert o.call(lib, runs, d_in=None) == _lib.CZ_EINVAL and o.untouched()
    t, j, cc = o.tiles.ctypes.data, o.joins.ctypes.data, o.cc
    nt, nj, npart = ctypes.byref(o.ntiles), ctypes.byref(o.njoins), ctypes.byref(o.npart)
    f = lib.cz_plan_fanout_split
    assert f(runs.ctypes.data, 1, 4096, 2, t, 64, None, cc, j, 64, nj, npart) == _lib.CZ_EINVAL
    assert f(runs.ctypes.data, 1, 4096, 2, t, 64, nt, None, j, 64, nj, npart) == _lib.CZ_EINVAL
    assert f(runs.ctypes.data, 1, 4096, 2, t, 64, nt, cc, j, 64, None, npart) == _lib.CZ_EINVAL
    assert f(runs.ctypes.data, 1, 4096, 2, t, 64, nt, cc, j, 64, nj, None) == _lib.CZ_EINVAL
    assert o.untouched()


def test_partial_record_index_limit(lib):
    """2^32 - 2 is the last partial-record index: 0xffffffff in a tile means a body in one tile"""
    from jeromq_amd import _lib
    # 2^24 subscribers x 256 one-block segments = 2^32 records: one too many; 255 blocks fit
    over = make_runs([dict(GOOD, len=256 * 64 - 33, out_stride=256 * 64, count=1 << 24)])
    o = Outputs(0)
    assert o.call(lib, over, seg_blocks=1) == _lib.CZ_EINVAL and o.untouched()
    fits = make_runs([dict(GOOD, len=255 * 64 - 33, out_stride=256 * 64, count=1 << 24)])
    o = Outputs(0)
    assert o.call(lib, fits, seg_blocks=1) == _lib.CZ_EINVAL          # (capacity only: the sizes are set)
    assert o.npart.value == 255 << 24 and o.ntiles.value == 255 << 18 and o.njoins.value == 1 << 18
    assert o.tables_untouched()


def test_plan_capacity_protocol(lib):
    from jeromq_amd import _lib
    # 133 B -> 3 blocks (2 segments at seg_blocks 2 would be whole: 3 <= 3), 1000 B -> 17 blocks, 9 segments
    runs = make_runs([dict(GOOD, len=1000, out_stride=1152), dict(GOOD, out_off=1 << 20, count=64),
                      dict(GOOD, out_off=2 << 20, len=1000, out_stride=1152, count=1)])
    tiles, joins, parts = 3 * 9 + 1 + 9, 3 + 1, 130 * 9 + 9
    for tcap, jcap in ((0, 0), (tiles - 1, joins), (tiles, joins - 1)):
        o = Outputs(tcap, jcap)
        assert o.call(lib, runs) == _lib.CZ_EINVAL
        assert [o.ntiles.value, o.njoins.value, o.npart.value] == [tiles, joins, parts] and o.tables_untouched()
    o = Outputs(tiles, joins)
    f = lib.cz_plan_fanout_split
    out = (ctypes.byref(o.ntiles), o.cc, o.joins.ctypes.data, joins, ctypes.byref(o.njoins), ctypes.byref(o.npart))
    assert f(runs.ctypes.data, 3, 4096, 2, None, tiles, *out) == _lib.CZ_EINVAL     # a null table with tiles to write
    assert o.ntiles.value == tiles and o.tables_untouched()
    assert f(runs.ctypes.data, 3, 4096, 2, o.tiles.ctypes.data, tiles, ctypes.byref(o.ntiles), o.cc, None, joins,
             ctypes.byref(o.njoins), ctypes.byref(o.npart)) == _lib.CZ_EINVAL
    assert o.tables_untouched()
    o = Outputs(tiles + 2, joins + 2)
    assert o.call(lib, runs) == _lib.CZ_OK
    assert [o.ntiles.value, o.njoins.value, o.npart.value, sum(o.cc)] == [tiles, joins, parts, tiles]
    assert np.all(o.tiles.view(np.uint32)[6 * tiles:] == SENT) and np.all(o.joins.view(np.uint32)[4 * joins:] == SENT)
    # no runs, and runs without subscribers: empty tables, CZ_OK
    o = Outputs(0)
    assert f(None, 0, None, 2, None, 0, ctypes.byref(o.ntiles), o.cc, None, 0, ctypes.byref(o.njoins),
             ctypes.byref(o.npart)) == _lib.CZ_OK
    assert [o.ntiles.value, o.njoins.value, o.npart.value, list(o.cc)] == [0, 0, 0, [0, 0]]
    o = Outputs(0)
    assert o.call(lib, make_runs([dict(GOOD, count=0), dict(GOOD, count=0, len=5000, out_stride=5120)])) == _lib.CZ_OK
    assert [o.ntiles.value, o.njoins.value, o.npart.value, list(o.cc)] == [0, 0, 0, [0, 0]]


def segment_cuts(lib, length, seg_blocks):
    """[(first_block, nblocks)] of cz_plan_segments for one seal descriptor of `length` bytes; seg_blocks 1, which
    that planner refuses, by the rule it states (whole up to 1.5 x seg_blocks blocks, else seg_blocks-block pieces)"""
    from jeromq_amd import _lib, batch
    nblk = (length + 33 + 63) // 64
    if seg_blocks < 2:
        return [(0, nblk)] if nblk <= seg_blocks + seg_blocks // 2 else [(b, 1) for b in range(nblk)]
    d = np.zeros(1, dtype=DESC_DTYPE)
    d["len"], d["prev"] = length, -1
    seg = np.zeros(nblk + 1, dtype=batch.SEGMENT_DTYPE)
    comb = np.zeros(1, dtype=batch.COMBINE_DTYPE)
    n, nc, npart = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.cz_plan_segments(d.ctypes.data, 1, 0, seg_blocks, seg.ctypes.data, len(seg), ctypes.byref(n),
                                comb.ctypes.data, 1, ctypes.byref(nc), ctypes.byref(npart)) == _lib.CZ_OK
    return sorted((int(s["first_block"]), int(s["nblocks"])) for s in seg[:n.value])


def plan(lib, runs, d_in=4096, seg_blocks=2):
    from jeromq_amd import _lib
    o = Outputs(0)
    o.call(lib, runs, d_in=d_in, seg_blocks=seg_blocks)
    o = Outputs(o.ntiles.value, o.njoins.value)
    assert o.call(lib, runs, d_in=d_in, seg_blocks=seg_blocks) == _lib.CZ_OK
    return o.tiles[:o.ntiles.value], o.joins[:o.njoins.value], o.npart.value, list(o.cc)


@pytest.mark.parametrize("seg_blocks", [1, 2, 3, 128])
def test_cut_points_are_the_segment_planners(lib, seg_blocks):
    split_above = seg_blocks + seg_blocks // 2
    lens = sorted(set(EDGE_LENS + [64 * b - 33 + d for b in (split_above, split_above + 1, 2 * seg_blocks,
                                                               2 * seg_blocks + 1) for d in (0, 1) if 64 * b - 33 + d >= 0]))
    for length in lens:
        for count in (1, 64, 130):
            mlen = length + 33
            runs = make_runs([dict(GOOD, len=length, out_stride=round_up(mlen, 128), count=count)])
            tiles, joins, npart, cc = plan(lib, runs, seg_blocks=seg_blocks)
            want = segment_cuts(lib, length, seg_blocks)
            for first in range(0, count, 64):
                got = sorted((int(t["first_block"]), int(t["nblocks"])) for t in tiles if int(t["first"]) == first)
                assert got == want, (length, count, first)
            assert len(tiles) == len(want) * ((count + 63) // 64)
            assert all(int(t["nseg"]) == len(want) for t in tiles)
            if len(want) == 1:
                assert all(int(t["part"]) == WHOLE for t in tiles) and len(joins) == 0 and npart == 0
            else:
                assert len(joins) == (count + 63) // 64 and npart == count * len(want)


def mixed_runs(rng, n):
    rows, off = [], 0
    for k in range(n):
        length = int(rng.choice(EDGE_LENS[:-1] + [1000]))
        mlen = length + 33
        stride = [round_up(mlen, 128), round_up(mlen, 128) + 128, mlen, mlen + 7][k % 4]
        count = int(rng.choice([0, 1, 63, 64, 65, 130, 257]))
        rows.append(dict(payload_off=int(rng.integers(0, 64)) * [16, 16, 8, 1][k % 4], out_off=off, out_stride=stride,
                         len=length, flags=k % 4, first_sub=int(rng.integers(0, 1000)), count=count))
        off = round_up(off + count * stride + 64, 128)
    return make_runs(rows)


@pytest.mark.parametrize("d_in,seg_blocks", [(1 << 20, 2), ((1 << 20) + 8, 2), (1 << 20, 1), (1 << 20, 3), (1 << 20, 0)])
def test_plan_tables(lib, d_in, seg_blocks):
    rng = np.random.default_rng(d_in + seg_blocks)
    runs = mixed_runs(rng, 60)
    tiles, joins, npart, cc = plan(lib, runs, d_in=d_in, seg_blocks=seg_blocks)
    assert sum(cc) == len(tiles)
    T = tiles.tolist()                       # (run, first, first_block, nblocks, part, nseg) as Python ints
    R = [dict(zip(runs.dtype.names, r)) for r in runs.tolist()]
    # every (run, subscriber, block) covered by exactly one tile
    cover, by_pair = {}, {}
    for run, first, b0, nb, part, nseg in T:
        r = R[run]
        nblk = (r["len"] + 33 + 63) // 64
        assert first % 64 == 0 and first < r["count"] and nb >= 1 and b0 + nb <= nblk
        cover.setdefault((run, first), np.zeros(nblk, dtype=np.int32))[b0:b0 + nb] += 1
        by_pair.setdefault((run, first), []).append((part, b0, nseg))
    assert sorted(cover) == sorted((k, f) for k, r in enumerate(R) for f in range(0, r["count"], 64))
    assert all(np.all(c == 1) for c in cover.values())
    # class: a full wave of a 16-byte aligned payload is of the line class; lines first, then lane-wise
    cls = [LINES if first + 64 <= R[run]["count"] and (d_in + R[run]["payload_off"]) % 16 == 0 else DIRECT
           for run, first, *_ in T]
    assert cls == [LINES] * cc[LINES] + [DIRECT] * cc[DIRECT]
    if d_in % 16 == 0:
        assert cc[LINES] and cc[DIRECT]
    # the longest first inside a class
    for a, b in ((0, cc[LINES]), (cc[LINES], len(T))):
        n = [t[3] for t in T[a:b]]
        assert n == sorted(n, reverse=True)
    # partial records: lane l of a tile writes part + l * nseg; a (run, subscriber)'s nseg records are consecutive
    # from its join's, the ranges of different pairs disjoint and inside npart
    owner = np.full(npart, -1, dtype=np.int64)
    pair_id = {}
    for run, first, part, nseg in joins.tolist():
        lanes = min(64, R[run]["count"] - first)
        assert lanes >= 1 and nseg >= 2
        for l in range(lanes):
            pid = pair_id.setdefault((run, first + l), len(pair_id))
            a = part + l * nseg
            assert a + nseg <= npart and np.all(owner[a:a + nseg] == -1)
            owner[a:a + nseg] = pid
    assert np.all(owner >= 0)                                      # dense: nothing allocated that no pair uses
    seen = np.zeros(npart, dtype=np.int32)
    for run, first, b0, nb, part, nseg in T:
        if part == WHOLE:
            assert nseg == 1 and b0 == 0
            continue
        for l in range(min(64, R[run]["count"] - first)):
            assert owner[part + l * nseg] == pair_id[(run, first + l)]
            seen[part + l * nseg] += 1
    assert np.all(seen == 1)                                        # every record written by exactly one (tile, lane)
    # ... in block order inside a pair: record s of a pair is its s-th segment, nseg the same in each
    for key, mine in by_pair.items():
        mine.sort()
        assert [b for _, b, _ in mine] == sorted(b for _, b, _ in mine), key
        assert len({n for _, _, n in mine}) == 1 and mine[0][2] == len(mine), key
        if mine[0][0] != WHOLE:
            assert [p for p, _, _ in mine] == list(range(mine[0][0], mine[0][0] + len(mine))), key


def test_seg_blocks_zero_is_the_flush_rule(lib):
    """batch_seg_blocks(total blocks, longest run's blocks): max(ceil(total / 65536), the one-frame optimum -- the
    largest s >= 2 with 18 s^2 <= nblk), capped at 128"""
    def rule(total, longest):
        s = 2
        while (s + 1) * (s + 1) * 18 <= longest:
            s += 1
        return min(128, max((total + 65535) // 65536, s))
    for length, count in ((4096, 64), (65536, 130), (4096, 1 << 17), (100, 64), (1 << 20, 64)):
        nblk = (length + 33 + 63) // 64
        runs = make_runs([dict(GOOD, len=length, out_stride=round_up(length + 33, 128), count=count),
                          dict(GOOD, out_off=1 << 40, count=64)])
        o = Outputs(0)
        o.call(lib, runs, seg_blocks=0)
        auto = [o.ntiles.value, o.njoins.value, o.npart.value]
        o = Outputs(0)
        o.call(lib, runs, seg_blocks=rule(count * nblk + 64 * 3, nblk))
        assert auto == [o.ntiles.value, o.njoins.value, o.npart.value], (length, count)


def test_python_plan(lib):
    from jeromq_amd import batch
    runs = make_runs([GOOD, dict(GOOD, out_off=1 << 20, len=1000, out_stride=1152, count=65)])
    p = batch.plan_fanout_split(runs, 4096, 8192, seg_blocks=2)
    # 100 B: 3 blocks, whole, 3 waves; 1000 B: 17 blocks, 9 segments x 2 waves
    assert (p.nruns, len(p.tiles), len(p.joins), p.npart, p.class_count) == (2, 3 + 18, 2, 65 * 9, [2 + 9, 1 + 9])
    assert p.tiles.dtype == batch.FANOUT_TILE_DTYPE and p.joins.dtype == batch.FANOUT_JOIN_DTYPE
    assert len(batch.plan_fanout_split(runs[:0], 4096, 8192).tiles) == 0
    assert len(batch.plan_fanout_split(runs, 4096, 8192).tiles) > 0       # seg_blocks 0


def test_launch_arguments_are_checked_before_the_device(lib):
    from jeromq_amd import _lib
    f = lib.cz_seal_fanout_split
    p = 4096  # any non-null address: a rejected call never reads it
    cc = (ctypes.c_uint32 * 2)(1, 1)
    for k in (0, 2, 6, 7, 8, 9):
        a = [p, 2, p, cc, p, 1, p, p, p, p, p, None]
        a[k] = None
        assert f(*a) == _lib.CZ_EINVAL, k
    assert f(p, 2, p, None, p, 1, p, p, p, p, p, None) == _lib.CZ_EINVAL
    assert f(p, 2, p, cc, None, 1, p, p, p, p, p, None) == _lib.CZ_EINVAL       # joins without a table
    assert f(p, 2, p, cc, p, 1, p, p, p, p, None, None) == _lib.CZ_EINVAL       # ... or without a workspace
    # nothing to do, nothing launched, nothing read
    assert f(None, 0, None, cc, None, 0, None, None, None, None, None, None) == _lib.CZ_OK
    assert f(None, 3, None, (ctypes.c_uint32 * 2)(0, 0), None, 0, None, None, None, None, None, None) == _lib.CZ_OK


@pytest.mark.skipif(os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK), reason="GPU present")
def test_no_cpu_fallback(lib):
    from jeromq_amd import _lib
    runs = make_runs([dict(GOOD, count=4, len=1000, out_stride=1152)])
    tiles, joins, npart, cc = plan(lib, runs)
    pay = ctypes.create_string_buffer(1024)
    subs = (_lib.cz_fanout_sub * 4)()
    keys = ctypes.create_string_buffer(32)
    out = ctypes.create_string_buffer(4 * 1152)
    work = ctypes.create_string_buffer(64 * npart)
    adr = ctypes.addressof
    assert lib.cz_seal_fanout_split(runs.ctypes.data, 1, tiles.ctypes.data, (ctypes.c_uint32 * 2)(*cc), joins.ctypes.data,
                                    len(joins), adr(pay), adr(subs), adr(keys), adr(out), adr(work), None) == _lib.CZ_EHIP
    assert out.raw == bytes(4 * 1152)


def test_tune_fanout_split(lib):
    """the knob's protocol as the other knobs: the previous value comes back, negative values clamp to 0"""
    old = lib.cz_tune(b"fanout_split", 4096)
    try:
        assert lib.cz_tune(b"fanout_split", -5) == 4096
        assert lib.cz_tune(b"fanout_split", 100) == 0
        assert lib.cz_tune(b"fanout_split", 100) == 100
    finally:
        lib.cz_tune(b"fanout_split", old)
    assert lib.cz_tune(b"fanout_split", old) == old


def test_default_follows_from_the_committed_measurement(lib):
    """the rule of tools/fanout_bench.py --split, applied again to the committed legs, gives the shipped default"""
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from fanout_bench import fanout_split_rule
    with open(os.path.join(ROOT, "profiles", "fanout", "fanout_split.json")) as f:
        m = json.load(f)
    verdict, best = fanout_split_rule(m["split_legs"], m["engine_split"])
    assert best == m["fanout_split_rule"] and verdict == m["fanout_split_verdict"]
    old = lib.cz_tune(b"fanout_split", 0)
    lib.cz_tune(b"fanout_split", old)
    assert old == best


def test_kernel_metadata(product):
    """Still four code objects; the line instantiation of k_seal_fanout_tiles carries strictly less per-lane
    state than k_seal_segments_lines (no descriptor, no segment record, uniform bounds), so it may use no more
    VGPRs and no more scratch than that kernel of the same library, and runs 3 waves per SIMD."""
    from test_acceptor_host import kernel_notes
    from test_occupancy import waves_per_simd
    assert len(product.device_code_objects(product.PRODUCT_LIB)) == 4
    notes = kernel_notes(product)
    tiles = {n: f for n, f in notes.items() if re.search(r"\d+k_seal_fanout_tilesI", n)}
    assert len(tiles) == 2, list(tiles)   # ST_LINES (1), ST_DIRECT (0)
    (lines,) = [f for n, f in tiles.items() if "k_seal_fanout_tilesILi1E" in n]
    (seg,) = [f for n, f in notes.items() if re.search(r"\d+k_seal_segments_lines", n)]
    assert lines["vgpr_count"] <= seg["vgpr_count"], (lines["vgpr_count"], seg["vgpr_count"])
    assert lines["private_segment_fixed_size"] <= seg["private_segment_fixed_size"], \
        (lines["private_segment_fixed_size"], seg["private_segment_fixed_size"])
    got = waves_per_simd(lines["vgpr_count"], lines["agpr_count"])
    assert got >= 3, f"{lines['vgpr_count']} VGPRs + {lines['agpr_count']} AGPRs = {got} waves per SIMD"
    for name, f in tiles.items():
        assert f["group_segment_fixed_size"] == 0, name   # dynamic LDS only
    (join,) = [f for n, f in notes.items() if re.search(r"\d+k_fanout_join", n)]
    assert join["private_segment_fixed_size"] == 0 and join["group_segment_fixed_size"] == 0
