"""GPU: the grouped PUB fan-out (cz_plan_fanout + cz_seal_fanout_runs, k_seal_fanout_runs) and the engine's
routing through it.

Every byte comparison is against two yardsticks that share no code with the new kernel: the CPU oracle
(or_seal_batch with one descriptor per (run, subscriber), the descriptors of a run sharing in_off) and the
existing device path (cz_seal_batch on the same descriptors) -- never k_seal_fanout.  Whole sentinel-filled
buffers are compared: the guard bytes before, between and after the runs' regions must be intact and an owned
slot must be zero past its body.  The engine's wire streams are compared with V2Encoder(oracle seal) of each
connection's frames, nonces counted by the test."""
import ctypes

import numpy as np
import pytest

from cz_testlib import DESC_DTYPE, oracle, or_curve_encode, splitmix_bytes, splitmix_words, v2_encode
from test_gpu_fanout import EDGE_COUNTERS, NKEYS, SENT, owns, round_up, shared_desc, subscribers

pytestmark = pytest.mark.gpu

LINES, REGION, DIRECT = 0, 1, 2
GUARD = 64


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from jeromq_amd import _lib, batch
    dev = torch.device("cuda:0")
    precom = splitmix_words(NKEYS * 4, 0xFA1).view(np.uint8).copy()   # NKEYS x 32 bytes
    keys = torch.from_numpy(precom).to(dev).view(NKEYS, 32)
    sub = batch.subkeys(keys, _lib.CZ_DIR_C2S)
    return torch, dev, batch, _lib, precom, sub


class Group:
    """Runs laid out in one input and one output buffer: every payload between bytes that differ from it, the
    output regions GUARD bytes apart (extent: whole slots where the stride owns them, else up to the last body)."""

    def __init__(self, seed):
        self.rows, self.subs, self.payloads, self.seed = [], [], [], seed
        self.in_at, self.out_at = 64, 256

    def add(self, length, subs, flags, stride=None, in_phase=0, out_phase=0, share_subs_at=None):
        mlen = length + 33
        stride = stride or round_up(mlen, 128)
        count = len(subs)
        in_off = round_up(self.in_at, 16) + in_phase
        out_off = round_up(self.out_at, 16) + out_phase
        first_sub = sum(len(s) for s in self.subs)
        self.subs.append(subs)
        self.payloads.append((in_off, splitmix_bytes(length, self.seed * 1000 + len(self.rows))))
        self.rows.append(dict(payload_off=in_off, out_off=out_off, out_stride=stride, len=length, flags=flags,
                              first_sub=first_sub, count=count))
        self.in_at = in_off + length + 16
        extent = 0 if count == 0 else (count * stride if owns(stride) else (count - 1) * stride + mlen)
        self.out_at = out_off + extent + GUARD

    def build(self, batch):
        runs = np.zeros(len(self.rows), dtype=batch.FANOUT_RUN_DTYPE)
        for k, row in enumerate(self.rows):
            for f, v in row.items():
                runs[f][k] = v
        hin = np.frombuffer(splitmix_bytes(self.in_at + 64, self.seed), dtype=np.uint8).copy() | 0x80
        for off, p in self.payloads:
            # (payload bytes with the top bit clear where the filler has it set: a read off by any phase shows)
            hin[off:off + len(p)] = np.frombuffer(p, dtype=np.uint8) & 0x7f
        subs = np.concatenate(self.subs) if self.subs else np.zeros(0, dtype=batch.FANOUT_SUB_DTYPE)
        descs = [shared_desc(self.subs[k], r["len"], r["flags"], r["payload_off"], r["out_off"], r["out_stride"])
                 for k, r in enumerate(self.rows)]
        return runs, hin, subs, descs, self.out_at + 256


def seal_and_check(env, g, what, table=None):
    """One grouped call into a sentinel-filled buffer, compared whole with the oracle and body by body with
    cz_seal_batch.  table = (waves, class_count, region_stride) replaces the planner's."""
    torch, dev, batch, _lib, precom, sub = env
    runs, hin, subs, descs, out_bytes = g.build(batch)
    d_in = torch.from_numpy(hin).to(dev)
    d_subs = torch.from_numpy(np.ascontiguousarray(subs).view(np.uint8).copy()).to(dev) if len(subs) else \
        torch.zeros(16, dtype=torch.uint8, device=dev)
    d_out = torch.full((out_bytes,), SENT, dtype=torch.uint8, device=dev)
    plan = batch.plan_fanout(runs, d_in, d_out)
    if table is not None:
        plan = batch.FanoutPlan(runs, table[0], table[1], table[2])
    batch.seal_fanout_runs(plan.to(dev), d_in, d_subs, sub, d_out)
    desc = np.concatenate(descs)
    d_ref = torch.full((out_bytes,), SENT, dtype=torch.uint8, device=dev)
    batch.seal_batch(torch.from_numpy(desc.view(np.uint8).copy()).to(dev), len(desc), d_in, d_ref, sub, desc_np=desc)
    torch.cuda.synchronize()
    want = np.full(out_bytes, SENT, dtype=np.uint8)
    for r in runs:
        if owns(int(r["out_stride"])):   # the run owns whole slots: zeros past each body
            want[int(r["out_off"]):int(r["out_off"]) + int(r["count"]) * int(r["out_stride"])] = 0
    oracle().or_seal_batch(desc.ctypes.data, len(desc), hin.ctypes.data, want.ctypes.data, precom.ctypes.data, 0, 8)
    got, ref = d_out.cpu().numpy(), d_ref.cpu().numpy()
    whole = np.array_equal(got, want)
    for k, d in enumerate(descs):
        mlen = int(runs["len"][k]) + 33
        for i, o in enumerate(d["out_off"]):
            o = int(o)
            if not whole:
                assert np.array_equal(got[o:o + mlen], want[o:o + mlen]), \
                    f"{what}: run {k} {g.rows[k]} body {i} differs from the oracle"
            assert np.array_equal(got[o:o + mlen], ref[o:o + mlen]), f"{what}: run {k} body {i} differs from cz_seal_batch"
    if not whole:
        bad = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{what}: byte {bad} outside the bodies is {got[bad]:#x}, expected {want[bad]:#x}")
    return plan, runs, hin, subs, d_out


MIX_LENS = [0, 31, 47, 100, 223, 224, 4097]
MIX_COUNTS = [1, 63, 64, 65, 130, 257]


@pytest.mark.parametrize("distinct", [True, False], ids=["key_per_subscriber", "three_keys"])
def test_one_call_mixes_every_class_and_edge(env, distinct):
    """7 lengths x 6 counts x 4 strides = 168 runs in one call: a 256-lane workgroup holds waves of different
    runs and run edges fall inside workgroups; flags 0..3 per run, payloads and output regions (64 guard bytes
    apart) at byte phases 0, 8 and 1, counters at the nonce edges inside a wave."""
    batch = env[2]
    rng = np.random.default_rng(11 + distinct)
    g = Group(21)
    for k in range(168):
        length = MIX_LENS[k % 7]
        mlen = length + 33
        stride = [round_up(mlen, 128), round_up(mlen, 128) + 128, mlen, mlen + 7][(k // 42) % 4]
        # (phases spread so that each length keeps aligned runs of both slot strides: 20 line waves, 29 region
        # waves, 315 lane-wise ones)
        g.add(length, subscribers(rng, MIX_COUNTS[(k // 7) % 6], distinct), k % 4, stride,
              in_phase=[0, 0, 0, 8, 1][(k * 7 + k // 42) % 5], out_phase=[0, 0, 0, 8, 1][(k * 3 + k // 7) % 5])
    plan = seal_and_check(env, g, f"mixed, distinct {distinct}")[0]
    assert all(plan.class_count), plan.class_count      # the call really used all three launches
    assert plan.nwaves == sum((r["count"] + 63) // 64 for r in g.rows)


def test_publish_shape_and_round_trip(env):
    """Sixteen runs to the same 130 subscribers, subscriber j's counter in run r = c_j + r with c_j straddling
    2^32 for some j; all payloads distinct, eight of equal length (a wave that read its neighbour run's record
    would still write a body of the right length).  Oracle first, then every body opens."""
    torch, dev, batch, _lib, precom, sub = env
    rng = np.random.default_rng(5)
    base = subscribers(rng, 130, True)
    for j in range(0, 130, 9):
        base["counter"][j] = (1 << 32) - 8 + (j % 16)     # crosses 2^32 inside the sixteen runs
    lens = [300, 100, 300, 223, 300, 224, 300, 31, 300, 1000, 300, 47, 300, 500, 300, 0]
    g = Group(22)
    for r, length in enumerate(lens):
        s = base.copy()
        s["counter"] = base["counter"] + np.uint64(r)      # (wraps mod 2^64 as the nonce does)
        g.add(length, s, r % 4)
    plan, runs, hin, subs, d_out = seal_and_check(env, g, "publish shape")
    assert plan.class_count[LINES] and plan.class_count[REGION] and plan.class_count[DIRECT] == 16
    n = 16 * 130
    odesc = np.zeros(n, dtype=DESC_DTYPE)
    pstride = 1024
    for r in range(16):
        sl = slice(r * 130, (r + 1) * 130)
        odesc["in_off"][sl] = runs["out_off"][r] + np.arange(130, dtype=np.uint64) * runs["out_stride"][r]
        odesc["len"][sl] = lens[r] + 33
    odesc["out_off"] = np.arange(n, dtype=np.uint64) * np.uint64(pstride)
    odesc["key_idx"] = subs["key_idx"]
    odesc["prev"] = -1
    d_plain = torch.full((n * pstride,), SENT, dtype=torch.uint8, device=dev)
    status = torch.zeros(n, dtype=torch.int16, device=dev)
    nonces = torch.zeros(n, dtype=torch.int64, device=dev)
    batch.open_batch(torch.from_numpy(odesc.view(np.uint8).copy()).to(dev), n, d_out, d_plain, sub, status,
                     nonces=nonces, desc_np=odesc)
    torch.cuda.synchronize()
    st = status.cpu().numpy().view(np.uint16)
    assert np.all((st & 0xff) == _lib.CZ_STATUS_OK), np.flatnonzero((st & 0xff) != 0)
    assert np.array_equal(st >> 8, np.repeat(np.arange(16) % 4, 130))
    assert np.array_equal(nonces.cpu().numpy().view(np.uint64), subs["counter"])
    plain = d_plain.cpu().numpy().reshape(n, pstride)
    for r, length in enumerate(lens):
        off = int(runs["payload_off"][r])
        assert np.all(plain[r * 130:(r + 1) * 130, :length] == hin[None, off:off + length]), f"run {r}"


def test_300_runs_of_5_subscribers(env):
    """every wave partial, 300 wave records for 1500 lanes"""
    rng = np.random.default_rng(6)
    g = Group(23)
    for k in range(300):
        g.add([100, 223, 31, 600][k % 4], subscribers(rng, 5, k % 2 == 0), k % 4)
    plan = seal_and_check(env, g, "300 x 5")[0]
    assert plan.class_count == [0, 0, 300]


def test_engine_group_shape(env):
    """16 runs x 1024 subscribers x 100 B, slots of 256 bytes: the region class, 256 waves in one launch"""
    rng = np.random.default_rng(7)
    g = Group(24)
    for k in range(16):
        s = np.zeros(1024, dtype=env[2].FANOUT_SUB_DTYPE)
        s["counter"] = rng.integers(0, 1 << 64, size=1024, dtype=np.uint64)
        s["counter"][5:5 + len(EDGE_COUNTERS)] = EDGE_COUNTERS
        s["key_idx"] = rng.integers(0, NKEYS, size=1024)
        g.add(100, s, k % 4)
    plan = seal_and_check(env, g, "16 x 1024 x 100 B")[0]
    assert plan.class_count == [0, 256, 0] and plan.region_stride == 256


def test_one_run_alone_and_an_empty_run_in_the_middle(env):
    rng = np.random.default_rng(8)
    for length, count in ((100, 130), (1000, 65), (47, 3)):
        g = Group(25)
        g.add(length, subscribers(rng, count, True), 1)
        seal_and_check(env, g, f"one run, len {length} count {count}")
    g = Group(26)
    g.add(224, subscribers(rng, 130, True), 0)
    g.add(4097, subscribers(rng, 0, True), 1)           # count 0: no wave, nothing written
    g.add(100, subscribers(rng, 65, False), 2)
    g.add(31, subscribers(rng, 0, True), 3, stride=64)
    g.add(223, subscribers(rng, 64, True), 3)
    plan = seal_and_check(env, g, "empty runs")[0]
    assert plan.nwaves == 3 + 2 + 1 and plan.nruns == 5
    # and a call of empty runs only launches nothing
    g = Group(27)
    g.add(100, subscribers(rng, 0, True), 0)
    assert seal_and_check(env, g, "only an empty run")[0].nwaves == 0


def test_class_is_never_a_correctness_choice(env):
    """Runs whose out_off or payload is off 16-byte alignment next to aligned ones, under a wave table that
    puts every run's full waves in a staged slice it does not qualify for: the misaligned lines-shaped and all
    the region-shaped runs in the lines slice, the misaligned region-shaped and all the lines-shaped runs in
    the region slice.  Each wave must fall back to the lane-wise path by its own run's checks."""
    batch = env[2]
    rng = np.random.default_rng(9)
    g = Group(28)
    shapes = []   # (slice the full waves go to)
    for length, out_phase, in_phase, to in (
            (1000, 0, 0, LINES),      # aligned, qualifies: staged
            (1000, 8, 0, LINES),      # out_off off 16-byte alignment in the lines slice
            (1000, 1, 0, LINES),
            (1000, 0, 1, LINES),      # payload at byte phase 1 in the lines slice (per_lane_ptr)
            (100, 0, 0, LINES),       # region-shaped in the lines slice
            (100, 0, 0, REGION),      # aligned, qualifies: staged
            (100, 1, 0, REGION),      # out_off off alignment in the region slice
            (100, 0, 8, REGION),      # payload off alignment in the region slice
            (1000, 0, 0, REGION),     # lines-shaped in the region slice: its 64 slots exceed the partition
            (31, 0, 0, REGION)):      # stride 64, smaller than the partition's: staged
        g.add(length, subscribers(rng, 130, len(shapes) % 2 == 0), len(shapes) % 4, in_phase=in_phase,
              out_phase=out_phase)
        shapes.append(to)
    waves = {LINES: [], REGION: [], DIRECT: []}
    for r, to in enumerate(shapes):
        waves[to] += [(r, 0), (r, 64)]
        waves[DIRECT].append((r, 128))
    table = np.array(waves[LINES] + waves[REGION] + waves[DIRECT], dtype=batch.FANOUT_WAVE_DTYPE)
    seal_and_check(env, g, "forced classes", table=(table, [len(waves[c]) for c in (LINES, REGION, DIRECT)], 256))
    # the same runs with every wave in the lane-wise slice, and with a region partition too small for any run
    direct = np.array(sorted(sum(waves.values(), [])), dtype=batch.FANOUT_WAVE_DTYPE)
    seal_and_check(env, g, "all lane-wise", table=(direct, [0, 0, len(direct)], 0))
    seal_and_check(env, g, "partition of 16-byte slots", table=(table, [len(waves[c]) for c in (LINES, REGION, DIRECT)], 16))


# ---- engine ------------------------------------------------------------------------------------

NCON = 520


def _precom(i):
    return splitmix_bytes(32, 4242 + i)


class Leg:
    """one engine flushed under its own knob values, and the test's own record of what it queued"""

    def __init__(self, knobs):
        from jeromq_amd.engine import CurveBatchEngine
        self.knobs = knobs
        self.eng = CurveBatchEngine(arena_bytes=4 << 20)
        self.cc = [self.eng.add_connection(_precom(i), as_server=False) for i in range(NCON)]

    def flush(self, L, ops):
        for op in ops:
            if op[0] == "send":
                assert self.eng.send(self.cc[op[1]], op[2], more=op[3]) == 0
            else:
                assert self.eng.publish([self.cc[c] for c in op[1]], op[2], more=op[3]) == len(op[1])
        old = {k: L.lib().cz_tune(k, v) for k, v in self.knobs.items()}
        try:
            self.eng.flush_out()
        finally:
            for k, v in old.items():
                L.lib().cz_tune(k, v)
        return [self.eng.wire_out(c) for c in self.cc]


def _expected(ops, sent):
    """per connection V2Encoder(oracle seal) of its frames in send order; `sent` counts the frames so far"""
    out = [[] for _ in range(NCON)]
    for op in ops:
        for c in ([op[1]] if op[0] == "send" else op[1]):
            out[c].append(v2_encode(or_curve_encode(op[2], 1 if op[3] else 0, 3 + sent[c], 0, _precom(c))))
            sent[c] += 1
    return [b"".join(x) for x in out]


def _flushes():
    p = [splitmix_bytes(n, 900 + k) for k, n in enumerate([100, 223, 5000, 100, 223, 17, 4096, 4096, 100])]
    every, first130, shuffled = list(range(NCON)), list(range(130)), list(np.random.default_rng(3).permutation(NCON))
    short = [("pub", first130, p[0], False), ("send", 7, p[5], False), ("pub", every, p[1], True),
             ("pub", every, p[2], False),                      # 5000 B: above the knob, stays in the segment plan
             ("send", 7, p[5], False), ("send", 300, p[2], False),
             ("pub", list(range(63)), p[3], False),            # below the 64-frame floor
             ("pub", first130, p[4], False), ("pub", shuffled, p[3], False), ("send", 519, p[0], False)]
    # over 16 MiB of wire: several groups, 4 KiB publishes (routed by fanout_min 64) split by their edges,
    # short ones between them
    big = []
    for k in range(14):
        big += [("pub", every, p[6 + k % 2], k % 3 == 0), ("pub", first130 if k % 2 else shuffled, p[8], False)]
    return short, big


def test_engine_routes_short_publishes(env):
    """Two engines take the same traffic flush after flush over the buffers the last flush left, one routing by
    fanout_short 4096 (fanout_min at its default, then 64 for the 4 KiB flush), one with fanout_short 0: equal
    wires, equal to the oracle's.  Then fanout_min 0 with fanout_short set: nothing is routed, same wire."""
    L = env[3]
    tune = L.lib().cz_tune
    default_min, default_short = tune(b"fanout_min", 1 << 18), tune(b"fanout_short", 0)
    assert default_min == 1 << 18 and default_short >= 0
    assert tune(b"fanout_short", default_short) == 0 and tune(b"fanout_min", default_min) == 1 << 18
    routed, plain = Leg({b"fanout_short": 4096}), Leg({b"fanout_short": 0})
    short, big = _flushes()
    sent = [0] * NCON
    try:
        for name, ops, knobs in (("short", short, {}), ("big", big, {b"fanout_min": 64}), ("short again", short, {}),
                                 ("fanout_min 0", short, {b"fanout_min": 0})):
            routed.knobs = {b"fanout_short": 4096, **knobs}
            wires = [routed.flush(L, ops), plain.flush(L, ops)]
            want = _expected(ops, sent)
            if name == "big":
                assert sum(len(w) for w in want) > 16 << 20
            for c in range(NCON):
                assert wires[0][c] == want[c], f"{name}, routed: connection {c}"
                assert wires[1][c] == want[c], f"{name}, unrouted: connection {c}"
            for leg in (routed, plain):
                assert [leg.eng.nonce(x) for x in leg.cc] == [3 + s for s in sent], name
    finally:
        routed.eng.close()
        plain.eng.close()
    assert tune(b"fanout_short", default_short) == default_short and tune(b"fanout_min", default_min) == default_min
