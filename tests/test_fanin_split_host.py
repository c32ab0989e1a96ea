"""CPU: the split fan-in open (cz_plan_fanin_split, cz_open_fanin_split, k_open_fanin_tiles, k_fanin_join) without
a device -- the records' layouts and the two prototypes against the C header, every refusal of the planner with its
outputs untouched, the 2^32 - 1 limits, the capacity protocol, the cut points against cz_plan_segments(open = 1) for
one descriptor of the run's size, every box block MACed and every payload chunk emitted by exactly one tile
(open_seg_geom's rule restated here), the partial-record ranges, the class and longest-first order, seg_blocks 0
against the flush rule restated, the launch's argument checks before the device, no CPU fallback, the knob and its
default against the committed measurement, and the kernels' AMDGPU metadata."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from cz_testlib import DESC_DTYPE, ROOT
from test_fanin_host import GOOD, make_runs

HEADER = os.path.join(ROOT, "include", "curvezmq_mi355x.h")
TILE_FIELDS = ("run", "first", "first_block", "nblocks", "part", "nseg")
JOIN_FIELDS = ("run", "first", "part", "nseg")
RUN_FIELDS = ("in_off", "in_stride", "out_off", "out_stride", "size", "first_sub", "count", "reserved")
SUB_FIELDS = ("floor", "key_idx", "flags")
LINES, DIRECT = 0, 1
WHOLE = 0xFFFFFFFF
SENT = 0xDEADBEEF
SIZES = (33, 97, 161, 225, 4129, 65569)      # the issue's body sizes: 1, 2, 3, 4, 65 and 1025 blocks


def round_up(v, a):
    return (v + a - 1) // a * a


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
    """section 3g reuses the records of 3e and 3f unchanged; its two calls have the issue's prototypes"""
    c = tmp_path / "layout.c"
    offs = ",".join([f"offsetof(cz_fanout_tile,{f})" for f in TILE_FIELDS] + ["sizeof(cz_fanout_join)"] +
                    [f"offsetof(cz_fanout_join,{f})" for f in JOIN_FIELDS] + ["sizeof(cz_fanin_run)"] +
                    [f"offsetof(cz_fanin_run,{f})" for f in RUN_FIELDS] + ["sizeof(cz_fanin_sub)"] +
                    [f"offsetof(cz_fanin_sub,{f})" for f in SUB_FIELDS])
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "curvezmq_mi355x.h"\n'
                 'int (*plan)(const cz_fanin_run *, uint32_t, const void *, const void *, uint32_t, cz_fanout_tile *, '
                 'uint32_t, uint32_t *, uint32_t[2], cz_fanout_join *, uint32_t, uint32_t *, uint32_t *) = '
                 'cz_plan_fanin_split;\n'
                 'int (*open)(const cz_fanin_run *, uint32_t, const cz_fanout_tile *, const uint32_t[2], '
                 'const cz_fanout_join *, uint32_t, const void *, const cz_fanin_sub *, const void *, void *, void *, '
                 'uint16_t *, uint64_t *, void *) = cz_open_fanin_split;\n'
                 'uint64_t (*frames)(const cz_engine *) = cz_engine_fanin_split_frames;\n'
                 'int main(void){size_t v[] = {sizeof(cz_fanout_tile),' + offs + ',CZ_FANOUT_TILE_LINES,'
                 'CZ_FANOUT_TILE_DIRECT,CZ_FANIN_CHECK_NONCE,CZ_FANIN_FLOOR_IS_BODY};'
                 'for (unsigned i = 0; i < sizeof v / sizeof *v; i++) printf("%zu ", v[i]);return 0;}\n')
    obj = tmp_path / "layout.o"
    # (compiled, not linked: the prototypes are checked by the initialisers, the values by the preprocessor)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-c", str(c), "-o",
                           str(obj)])
    from jeromq_amd import _lib, batch
    want_tile, want_join = [0, 4, 8, 12, 16, 20], [0, 4, 8, 12]
    want_run, want_sub = [0, 8, 16, 24, 32, 36, 40, 44], [0, 8, 12]
    assert ctypes.sizeof(_lib.cz_fanout_tile) == 24 and ctypes.sizeof(_lib.cz_fanout_join) == 16
    assert ctypes.sizeof(_lib.cz_fanin_run) == 48 and ctypes.sizeof(_lib.cz_fanin_sub) == 16
    assert [getattr(_lib.cz_fanout_tile, f).offset for f in TILE_FIELDS] == want_tile
    assert [getattr(_lib.cz_fanout_join, f).offset for f in JOIN_FIELDS] == want_join
    assert [getattr(_lib.cz_fanin_run, f).offset for f in RUN_FIELDS] == want_run
    assert [getattr(_lib.cz_fanin_sub, f).offset for f in SUB_FIELDS] == want_sub
    assert [batch.FANOUT_TILE_DTYPE.fields[f][1] for f in TILE_FIELDS] == want_tile
    assert [batch.FANOUT_JOIN_DTYPE.fields[f][1] for f in JOIN_FIELDS] == want_join
    assert [batch.FANIN_RUN_DTYPE.fields[f][1] for f in RUN_FIELDS] == want_run
    assert [batch.FANIN_SUB_DTYPE.fields[f][1] for f in SUB_FIELDS] == want_sub
    # the same numbers from the C compiler
    c2 = tmp_path / "values.c"
    c2.write_text(c.read_text().replace("= cz_plan_fanin_split", "= 0").replace("= cz_open_fanin_split", "= 0")
                  .replace("= cz_engine_fanin_split_frames", "= 0"))
    exe = tmp_path / "values"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(c2), "-o", str(exe)])
    want = [24] + want_tile + [16] + want_join + [48] + want_run + [16] + want_sub + [LINES, DIRECT, 1, 2]
    assert list(map(int, subprocess.check_output([str(exe)], text=True).split())) == want
    text = open(HEADER).read()
    assert text.index("---- 3f.") < text.index("---- 3g.") < text.index("cz_plan_fanin_split(")


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

    def call(self, lib, runs, d_in=4096, d_out=8192, seg_blocks=2, nruns=None):
        return lib.cz_plan_fanin_split(runs.ctypes.data if runs is not None else None,
                                       len(runs) if nruns is None else nruns, d_in, d_out, seg_blocks,
                                       self.tiles.ctypes.data, self.tile_cap, ctypes.byref(self.ntiles), self.cc,
                                       self.joins.ctypes.data, self.join_cap, ctypes.byref(self.njoins),
                                       ctypes.byref(self.npart))

    def tables_untouched(self):
        return (np.all(self.tiles.view(np.uint32) == SENT) and np.all(self.joins.view(np.uint32) == SENT)
                and list(self.cc) == [SENT] * 2)

    def untouched(self):
        return self.tables_untouched() and [self.ntiles.value, self.njoins.value, self.npart.value] == [SENT] * 3


def test_plan_refusals_leave_the_outputs_untouched(lib):
    """every refusal of cz_plan_fanin (tests/test_fanin_host.py's list), the bad run last behind two good ones"""
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
        runs = make_runs([GOOD, dict(GOOD, out_off=1 << 20, in_off=1 << 20), row])
        for seg in (0, 1, 2):
            o = Outputs(64)
            assert o.call(lib, runs, seg_blocks=seg) == _lib.CZ_EINVAL, row
            assert o.untouched(), row
    # one frame needs no stride: the same strides pass with count 1
    o = Outputs(64)
    assert o.call(lib, make_runs([dict(GOOD, out_stride=99, in_stride=1, count=1)])) == _lib.CZ_OK
    runs = make_runs([GOOD])
    o = Outputs(64)
    assert o.call(lib, None, nruns=1) == _lib.CZ_EINVAL and o.untouched()
    assert o.call(lib, runs, d_in=None) == _lib.CZ_EINVAL and o.untouched()
    assert o.call(lib, runs, d_out=None) == _lib.CZ_EINVAL and o.untouched()
    t, j, cc = o.tiles.ctypes.data, o.joins.ctypes.data, o.cc
    nt, nj, npart = ctypes.byref(o.ntiles), ctypes.byref(o.njoins), ctypes.byref(o.npart)
    f = lib.cz_plan_fanin_split
    assert f(runs.ctypes.data, 1, 4096, 8192, 2, t, 64, None, cc, j, 64, nj, npart) == _lib.CZ_EINVAL
    assert f(runs.ctypes.data, 1, 4096, 8192, 2, t, 64, nt, None, j, 64, nj, npart) == _lib.CZ_EINVAL
    assert f(runs.ctypes.data, 1, 4096, 8192, 2, t, 64, nt, cc, j, 64, None, npart) == _lib.CZ_EINVAL
    assert f(runs.ctypes.data, 1, 4096, 8192, 2, t, 64, nt, cc, j, 64, nj, None) == _lib.CZ_EINVAL
    assert o.untouched()


def test_index_limits(lib):
    """tiles, join waves and partial records are counted in 32 bits: 2^32 - 1 of each is the most"""
    from jeromq_amd import _lib
    # 2^24 bodies of 257 blocks at seg_blocks 1 = 256 segments each: 2^32 records, one too many; 256 blocks fit
    over = make_runs([dict(GOOD, size=257 * 64, in_stride=257 * 64, out_stride=257 * 64, count=1 << 24)])
    o = Outputs(0)
    assert o.call(lib, over, seg_blocks=1) == _lib.CZ_EINVAL and o.untouched()
    fits = make_runs([dict(GOOD, size=256 * 64, in_stride=256 * 64, out_stride=256 * 64, count=1 << 24)])
    o = Outputs(0)
    assert o.call(lib, fits, seg_blocks=1) == _lib.CZ_EINVAL          # (capacity only: the sizes are set)
    assert o.npart.value == 255 << 24 and o.ntiles.value == 255 << 18 and o.njoins.value == 1 << 18
    assert o.tables_untouched()
    # tiles alone: 2^31 - 64 bodies (2^25 - 1 waves) x 128 segments = 2^32 - 128 tiles fit the tile count, but
    # their 2^38 records do not
    many = make_runs([dict(GOOD, size=129 * 64, in_stride=129 * 64, out_stride=129 * 64, count=(1 << 31) - 64)])
    o = Outputs(0)
    assert o.call(lib, many, seg_blocks=1) == _lib.CZ_EINVAL and o.untouched()


def test_plan_capacity_protocol(lib):
    from jeromq_amd import _lib
    # 133 B: 3 blocks, whole at seg_blocks 2 (3 <= 3); 1033 B: 17 blocks, ceil(16 / 2) = 8 segments
    big = dict(GOOD, size=1033, in_stride=1152, out_stride=1024)
    runs = make_runs([big, dict(GOOD, out_off=1 << 20, in_off=1 << 20, count=64),
                      dict(big, out_off=2 << 20, in_off=2 << 20, count=1)])
    tiles, joins, parts = 3 * 8 + 1 + 8, 3 + 1, 130 * 8 + 8
    for tcap, jcap in ((0, 0), (tiles - 1, joins), (tiles, joins - 1)):
        o = Outputs(tcap, jcap)
        assert o.call(lib, runs) == _lib.CZ_EINVAL
        assert [o.ntiles.value, o.njoins.value, o.npart.value] == [tiles, joins, parts] and o.tables_untouched()
    o = Outputs(tiles, joins)
    f = lib.cz_plan_fanin_split
    out = (ctypes.byref(o.ntiles), o.cc, o.joins.ctypes.data, joins, ctypes.byref(o.njoins), ctypes.byref(o.npart))
    assert f(runs.ctypes.data, 3, 4096, 8192, 2, None, tiles, *out) == _lib.CZ_EINVAL   # a null table with tiles to write
    assert o.ntiles.value == tiles and o.tables_untouched()
    assert f(runs.ctypes.data, 3, 4096, 8192, 2, o.tiles.ctypes.data, tiles, ctypes.byref(o.ntiles), o.cc, None, joins,
             ctypes.byref(o.njoins), ctypes.byref(o.npart)) == _lib.CZ_EINVAL
    assert o.tables_untouched()
    o = Outputs(tiles + 2, joins + 2)
    assert o.call(lib, runs) == _lib.CZ_OK
    assert [o.ntiles.value, o.njoins.value, o.npart.value, sum(o.cc)] == [tiles, joins, parts, tiles]
    assert np.all(o.tiles.view(np.uint32)[6 * tiles:] == SENT) and np.all(o.joins.view(np.uint32)[4 * joins:] == SENT)
    # no runs, and runs without bodies: empty tables, CZ_OK
    o = Outputs(0)
    assert f(None, 0, None, None, 2, None, 0, ctypes.byref(o.ntiles), o.cc, None, 0, ctypes.byref(o.njoins),
             ctypes.byref(o.npart)) == _lib.CZ_OK
    assert [o.ntiles.value, o.njoins.value, o.npart.value, list(o.cc)] == [0, 0, 0, [0, 0]]
    o = Outputs(0)
    assert o.call(lib, make_runs([dict(GOOD, count=0), dict(big, count=0)])) == _lib.CZ_OK
    assert [o.ntiles.value, o.njoins.value, o.npart.value, list(o.cc)] == [0, 0, 0, [0, 0]]


def rule_cuts(size, seg_blocks):
    """the issue's rule: whole up to 1.5 x seg_blocks blocks, else ceil((nblk - 1) / seg_blocks) segments, segment 0
    = blocks [0, seg_blocks + 1), segment s >= 1 from block s * seg_blocks + 1, the last one the remainder.  At
    seg_blocks 1 that makes a two-block body one segment: it stays whole; a longer one is [0, 2), then one block each"""
    nblk = max(1, (size + 63) // 64)
    ns = 1 if nblk <= seg_blocks + seg_blocks // 2 else (nblk - 1 + seg_blocks - 1) // seg_blocks
    if ns == 1:
        return [(0, nblk)]
    starts = [0] + [s * seg_blocks + 1 for s in range(1, ns)] + [nblk]
    return [(starts[s], starts[s + 1] - starts[s]) for s in range(ns)]


def segment_cuts(lib, size, seg_blocks):
    """[(first_block, nblocks)] of cz_plan_segments for one open descriptor of `size` bytes"""
    from jeromq_amd import _lib, batch
    nblk = max(1, (size + 63) // 64)
    d = np.zeros(1, dtype=DESC_DTYPE)
    d["len"], d["prev"] = size, -1
    seg = np.zeros(nblk + 1, dtype=batch.SEGMENT_DTYPE)
    comb = np.zeros(1, dtype=batch.COMBINE_DTYPE)
    n, nc, npart = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.cz_plan_segments(d.ctypes.data, 1, 1, seg_blocks, seg.ctypes.data, len(seg), ctypes.byref(n),
                                comb.ctypes.data, 1, ctypes.byref(nc), ctypes.byref(npart)) == _lib.CZ_OK
    return sorted((int(s["first_block"]), int(s["nblocks"])) for s in seg[:n.value])


def plan(lib, runs, d_in=4096, d_out=8192, seg_blocks=2):
    from jeromq_amd import _lib
    o = Outputs(0)
    o.call(lib, runs, d_in=d_in, d_out=d_out, seg_blocks=seg_blocks)
    o = Outputs(o.ntiles.value, o.njoins.value)
    assert o.call(lib, runs, d_in=d_in, d_out=d_out, seg_blocks=seg_blocks) == _lib.CZ_OK
    return o.tiles[:o.ntiles.value], o.joins[:o.njoins.value], o.npart.value, list(o.cc)


def test_rule_restated_for_seg_blocks_1():
    assert rule_cuts(33, 1) == [(0, 1)] and rule_cuts(97, 1) == [(0, 2)]
    assert rule_cuts(161, 1) == [(0, 2), (2, 1)] and rule_cuts(289, 1) == [(0, 2), (2, 1), (3, 1), (4, 1)]
    assert rule_cuts(225, 2) == [(0, 3), (3, 1)] and rule_cuts(4129, 3) == [(0, 4)] + [(3 * s + 1, 3) for s in range(1, 21)] + [(64, 1)]


@pytest.mark.parametrize("seg_blocks", [1, 2, 3, 128])
def test_cut_points_are_the_segment_planners(lib, seg_blocks):
    split_above = seg_blocks + seg_blocks // 2
    sizes = sorted(set(SIZES + tuple(64 * b + d for b in (split_above, split_above + 1, 2 * seg_blocks, 2 * seg_blocks + 1)
                                     for d in (-1, 0, 1)) + (0, 1, 32)))
    for size in sizes:
        nout = max(size - 33, 0)
        want = rule_cuts(size, seg_blocks)
        if seg_blocks >= 2:
            assert want == segment_cuts(lib, size, seg_blocks), size
        for count in (1, 64, 130):
            runs = make_runs([dict(GOOD, size=size, in_stride=round_up(max(size, 1), 128),
                                   out_stride=round_up(max(nout, 1), 128), count=count)])
            tiles, joins, npart, cc = plan(lib, runs, seg_blocks=seg_blocks)
            for first in range(0, count, 64):
                got = sorted((int(t["first_block"]), int(t["nblocks"])) for t in tiles if int(t["first"]) == first)
                assert got == want, (size, count, first)
            assert len(tiles) == len(want) * ((count + 63) // 64)
            assert all(int(t["nseg"]) == len(want) for t in tiles)
            if len(want) == 1:
                assert all(int(t["part"]) == WHOLE for t in tiles) and len(joins) == 0 and npart == 0
            else:
                assert len(joins) == (count + 63) // 64 and npart == count * len(want)


def chunk_range(size, b0, nb):
    """open_seg_geom restated: a tile of box blocks [b0, b0 + nb) emits payload chunks [cb, ce)"""
    if size < 33:
        return 0, 0
    nblk, nout = (size + 63) // 64, size - 33
    bend = min(b0 + nb, nblk)
    return (b0 - 1 if b0 else 0), ((nout + 63) // 64 if bend == nblk else bend - 1)


def mixed_runs(rng, n):
    rows, io, oo = [], 0, 0
    for k in range(n):
        size = int(rng.choice(SIZES[:-1] + (32, 34, 96, 129, 1033)))
        nout = max(size - 33, 0)
        out_stride = [round_up(max(nout, 1), 128), round_up(max(nout, 1), 128) + 128, max(nout, 64), nout + 7][k % 4]
        in_stride = [round_up(size, 128), round_up(size, 16), size, size + 8][(k // 4) % 4]
        count = int(rng.choice([0, 1, 63, 64, 65, 130, 257]))
        rows.append(dict(in_off=io + int(rng.integers(0, 4)) * [16, 16, 8, 1][k % 4], in_stride=in_stride, out_off=oo,
                         out_stride=out_stride, size=size, first_sub=int(rng.integers(0, 1000)), count=count))
        io = round_up(io + count * in_stride + 128, 128)
        oo = round_up(oo + count * out_stride + 64, 128)
    return make_runs(rows)


@pytest.mark.parametrize("d_in,seg_blocks", [(1 << 20, 2), ((1 << 20) + 8, 2), (1 << 20, 1), (1 << 20, 3), (1 << 20, 0)])
def test_plan_tables(lib, d_in, seg_blocks):
    rng = np.random.default_rng(d_in + seg_blocks)
    runs = mixed_runs(rng, 80)
    tiles, joins, npart, cc = plan(lib, runs, d_in=d_in, seg_blocks=seg_blocks)
    assert sum(cc) == len(tiles)
    T = tiles.tolist()                       # (run, first, first_block, nblocks, part, nseg) as Python ints
    R = [dict(zip(runs.dtype.names, r)) for r in runs.tolist()]
    # for every (run, 64 bodies): every box block MACed by exactly one tile, every payload chunk emitted by exactly
    # one tile, tiles after the first starting at block 2 or later
    mac, emit, by_pair = {}, {}, {}
    for run, first, b0, nb, part, nseg in T:
        r = R[run]
        nblk = max(1, (r["size"] + 63) // 64)
        nchunk = (max(r["size"] - 33, 0) + 63) // 64
        assert first % 64 == 0 and first < r["count"] and nb >= 1 and b0 + nb <= nblk and (b0 == 0 or b0 >= 2)
        mac.setdefault((run, first), np.zeros(nblk, dtype=np.int32))[b0:b0 + nb] += 1
        cb, ce = chunk_range(r["size"], b0, nb)
        assert cb <= ce <= nchunk
        emit.setdefault((run, first), np.zeros(nchunk, dtype=np.int32))[cb:ce] += 1
        by_pair.setdefault((run, first), []).append((part, b0, nseg))
    assert sorted(mac) == sorted((k, f) for k, r in enumerate(R) for f in range(0, r["count"], 64))
    assert all(np.all(c == 1) for c in mac.values()) and all(np.all(c == 1) for c in emit.values())
    # class: a full wave whose body base and in_stride are on 16 bytes is of the line class; lines first
    cls = [LINES if first + 64 <= R[run]["count"] and (d_in + R[run]["in_off"]) % 16 == 0
           and R[run]["in_stride"] % 16 == 0 else DIRECT for run, first, *_ in T]
    assert cls == [LINES] * cc[LINES] + [DIRECT] * cc[DIRECT]
    assert cc[DIRECT] and (cc[LINES] or d_in % 16)
    # inside a class the tiles with the most output chunks first
    for a, b in ((0, cc[LINES]), (cc[LINES], len(T))):
        n = [ce - cb for cb, ce in (chunk_range(R[t[0]]["size"], t[2], t[3]) for t in T[a:b])]
        assert n == sorted(n, reverse=True)
    # partial records: lane l of a tile writes part + l * nseg; a body's nseg records are consecutive from its
    # join's, the ranges of different bodies disjoint, dense and inside npart
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
    assert np.all(owner >= 0)
    seen = np.zeros(npart, dtype=np.int32)
    for run, first, b0, nb, part, nseg in T:
        if part == WHOLE:
            assert nseg == 1 and b0 == 0
            continue
        for l in range(min(64, R[run]["count"] - first)):
            assert owner[part + l * nseg] == pair_id[(run, first + l)]
            seen[part + l * nseg] += 1
    assert np.all(seen == 1)
    # ... in segment order: record s of a body is its s-th segment, nseg the same in each
    for key, mine in by_pair.items():
        mine.sort()
        assert [b for _, b, _ in mine] == sorted(b for _, b, _ in mine), key
        assert len({n for _, _, n in mine}) == 1 and mine[0][2] == len(mine), key
        if mine[0][0] != WHOLE:
            assert [p for p, _, _ in mine] == list(range(mine[0][0], mine[0][0] + len(mine))), key
    # one join record per 64 bodies of a split run, in run order
    want_joins = [(k, f) for k, r in enumerate(R) for f in range(0, r["count"], 64)
                  if len(rule_cuts(r["size"], seg_blocks or flush_rule(runs))) > 1]
    assert [(j[0], j[1]) for j in joins.tolist()] == want_joins


def flush_rule(runs):
    """flush_seg_blocks restated: the length cz_engine_flush_in picks for a flush of the runs' total body bytes"""
    total = sum(int(r["count"]) * int(r["size"]) for r in runs)
    return min(128, max(4, (total // 64 + 65535) // 65536))


def test_seg_blocks_zero_is_the_flush_rule(lib):
    for size, count in ((4129, 64), (65569, 130), (4129, 1 << 14), (4129, 1 << 17), (133, 64), (65569, 1 << 16), (1 << 20, 1 << 13)):
        runs = make_runs([dict(GOOD, size=size, in_stride=round_up(size, 128), out_stride=round_up(size - 33, 128), count=count),
                          dict(GOOD, in_off=1 << 40, out_off=1 << 40, count=64)])
        o = Outputs(0)
        o.call(lib, runs, seg_blocks=0)
        auto = [o.ntiles.value, o.njoins.value, o.npart.value]
        o = Outputs(0)
        o.call(lib, runs, seg_blocks=flush_rule(runs))
        assert auto == [o.ntiles.value, o.njoins.value, o.npart.value], (size, count)
    assert {flush_rule(make_runs([dict(GOOD, size=s, count=c)])) for s, c in ((4129, 64), (4129, 1 << 14), (1 << 20, 1 << 13))} \
        == {4, 17, 128}


def test_python_plan(lib):
    from jeromq_amd import batch
    runs = make_runs([GOOD, dict(GOOD, in_off=1 << 20, out_off=1 << 20, size=1033, in_stride=1152, out_stride=1024, count=65)])
    p = batch.plan_fanin_split(runs, 4096, 8192, seg_blocks=2)
    # 133 B: 3 blocks, whole, 3 waves; 1033 B: 17 blocks, 8 segments x 2 waves
    assert (p.nruns, len(p.tiles), len(p.joins), p.npart, p.class_count) == (2, 3 + 16, 2, 65 * 8, [2 + 8, 1 + 8])
    assert p.tiles.dtype == batch.FANOUT_TILE_DTYPE and p.joins.dtype == batch.FANOUT_JOIN_DTYPE
    assert p.runs.dtype == batch.FANIN_RUN_DTYPE
    assert len(batch.plan_fanin_split(runs[:0], 4096, 8192).tiles) == 0
    # seg_blocks 0 -> 4 for so few bytes: 17 blocks are ceil(16 / 4) = 4 segments x 2 waves, plus the 3 whole waves
    assert len(batch.plan_fanin_split(runs, 4096, 8192).tiles) == 3 + 8


def test_launch_arguments_are_checked_before_the_device(lib):
    from jeromq_amd import _lib
    f = lib.cz_open_fanin_split
    p = 4096  # any non-null address: a rejected call never reads it
    cc = (ctypes.c_uint32 * 2)(1, 1)
    #       runs n tiles cc joins nj in subs keys out work status nonces stream
    for k in (0, 2, 6, 7, 8, 9, 11):
        a = [p, 2, p, cc, p, 1, p, p, p, p, p, p, p, None]
        a[k] = None
        assert f(*a) == _lib.CZ_EINVAL, k
    assert f(p, 2, p, None, p, 1, p, p, p, p, p, p, p, None) == _lib.CZ_EINVAL
    assert f(p, 2, p, cc, None, 1, p, p, p, p, p, p, p, None) == _lib.CZ_EINVAL       # joins without a table
    assert f(p, 2, p, cc, p, 1, p, p, p, p, None, p, p, None) == _lib.CZ_EINVAL       # ... or without a workspace
    # nothing to do, nothing launched, nothing read
    assert f(None, 0, None, cc, None, 0, None, None, None, None, None, None, None, None) == _lib.CZ_OK
    assert f(None, 3, None, (ctypes.c_uint32 * 2)(0, 0), None, 0, None, None, None, None, None, None, None, None) == _lib.CZ_OK


@pytest.mark.skipif(os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK), reason="GPU present")
def test_no_cpu_fallback(lib):
    """with no device the call fails with CZ_EHIP and writes nothing: d_joins / d_work null with njoins 0 and a null
    d_nonces pass the argument checks and reach the device"""
    from jeromq_amd import _lib
    adr = ctypes.addressof
    for size, stride in ((1033, 1152), (133, 256)):
        runs = make_runs([dict(GOOD, count=4, size=size, in_stride=stride, out_stride=1024)])
        tiles, joins, npart, cc = plan(lib, runs)
        assert (len(joins) == 0) == (size == 133)
        body = ctypes.create_string_buffer(4 * stride)
        subs = (_lib.cz_fanin_sub * 4)()
        keys = ctypes.create_string_buffer(32)
        out = ctypes.create_string_buffer(4 * 1024)
        work = ctypes.create_string_buffer(64 * max(npart, 1))
        status = (ctypes.c_uint16 * 4)(*[0x5A5A] * 4)
        assert lib.cz_open_fanin_split(runs.ctypes.data, 1, tiles.ctypes.data, (ctypes.c_uint32 * 2)(*cc),
                                       joins.ctypes.data if len(joins) else None, len(joins), adr(body), adr(subs),
                                       adr(keys), adr(out), adr(work) if len(joins) else None, adr(status), None,
                                       None) == _lib.CZ_EHIP
        assert out.raw == bytes(4 * 1024) and list(status) == [0x5A5A] * 4


def test_tune_fanin_split(lib):
    """the knob's protocol as the other knobs: the previous value comes back, negative values clamp to 0; it leaves
    fanin_short alone"""
    short = lib.cz_tune(b"fanin_short", 100)
    old = lib.cz_tune(b"fanin_split", 4096)
    try:
        assert lib.cz_tune(b"fanin_split", -5) == 4096
        assert lib.cz_tune(b"fanin_split", 100) == 0
        assert lib.cz_tune(b"fanin_split", 100) == 100
        assert lib.cz_tune(b"fanin_short", 100) == 100
    finally:
        lib.cz_tune(b"fanin_split", old)
        lib.cz_tune(b"fanin_short", short)
    assert lib.cz_tune(b"fanin_split", old) == old
    from jeromq_amd.engine import CurveBatchEngine
    assert isinstance(CurveBatchEngine.fanin_split_frames, property)


def test_default_follows_from_the_committed_measurement(lib):
    """the rule of tools/fanin_bench.py --split, applied again to the committed legs, gives the shipped default"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from fanin_bench import fanin_split_rule
    with open(os.path.join(ROOT, "profiles", "fanin", "fanin_split.json")) as f:
        m = json.load(f)
    assert sorted({r["len"] for r in m["split_legs"]}) == [1024, 4096, 16384, 65536]
    assert {(r["runs"], r["n"]) for r in m["split_legs"]} == {(1, 64), (16, 64), (1, 1024), (16, 1024), (256, 1024)}
    assert m["reps"] == 7 and all(len(r["split_all_ms"]) == 7 for r in m["split_legs"])
    verdict, best = fanin_split_rule(m["split_legs"], m["engine_split"])
    assert best == m["fanin_split_rule"] and verdict == m["fanin_split_verdict"]
    old = lib.cz_tune(b"fanin_split", 0)
    lib.cz_tune(b"fanin_split", old)
    assert old == best


def test_kernel_metadata(product):
    """Still four code objects; the line instantiation of k_open_fanin_tiles carries less per-lane state than
    k_open_segments (no descriptor, no segment record, uniform bounds): 3 waves per SIMD with no more scratch than
    that kernel of the same library; the lane-wise instantiation and the join without scratch."""
    from test_acceptor_host import kernel_notes
    from test_occupancy import waves_per_simd
    assert len(product.device_code_objects(product.PRODUCT_LIB)) == 4
    notes = kernel_notes(product)
    tiles = {n: f for n, f in notes.items() if re.search(r"\d+k_open_fanin_tilesI", n)}
    assert len(tiles) == 2, list(tiles)   # ST_LINES (1), ST_DIRECT (0)
    (lines,) = [f for n, f in tiles.items() if "k_open_fanin_tilesILi1E" in n]
    (direct,) = [f for n, f in tiles.items() if "k_open_fanin_tilesILi0E" in n]
    (seg,) = [f for n, f in notes.items() if re.search(r"\d+k_open_segmentsE", n)]
    assert lines["private_segment_fixed_size"] <= seg["private_segment_fixed_size"], \
        (lines["private_segment_fixed_size"], seg["private_segment_fixed_size"])
    assert lines["vgpr_count"] <= seg["vgpr_count"], (lines["vgpr_count"], seg["vgpr_count"])
    got = waves_per_simd(lines["vgpr_count"], lines["agpr_count"])
    assert got >= 3, f"{lines['vgpr_count']} VGPRs + {lines['agpr_count']} AGPRs = {got} waves per SIMD"
    assert direct["private_segment_fixed_size"] == 0
    for name, f in tiles.items():
        assert f["group_segment_fixed_size"] == 0, name   # dynamic LDS only
    (join,) = [f for n, f in notes.items() if re.search(r"\d+k_fanin_joinE", n)]
    assert join["private_segment_fixed_size"] == 0 and join["group_segment_fixed_size"] == 0
