"""GPU: the split PUB fan-out (cz_plan_fanout_split + cz_seal_fanout_split: k_seal_fanout_tiles on a subscriber x
segment grid, k_fanout_join) and the engine's routing through it (cz_tune "fanout_split").

Every byte comparison is against two yardsticks that share no code with the new kernels: the CPU oracle
(or_seal_batch with one descriptor per (run, subscriber), the descriptors of a run sharing in_off) and the
existing device path (cz_seal_batch on the same descriptors) -- never a fan-out kernel.  Whole sentinel-filled
buffers are compared: the guard bytes before, between and after the runs' regions must be intact and an owned
slot must be zero past its body.  The engine's wire streams are compared with V2Encoder(oracle seal) of each
connection's frames, nonces counted by the test."""
import numpy as np
import pytest

import fanout_steer as fs
from cz_testlib import DESC_DTYPE, oracle, splitmix_bytes
from test_gpu_fanout import SENT, owns, round_up, subscribers
from test_gpu_fanout_runs import NCON, Group, Leg, _expected, _precom
from test_gpu_fanout_runs import env  # noqa: F401  (the module's fixture: 257 keys, C2S subkeys)

pytestmark = pytest.mark.gpu

LINES, DIRECT = 0, 1
WHOLE = 0xFFFFFFFF
# body block counts 1, 1, 3, 4, 4, 4, 4, 5, 7, 64, 65: the unsplit frame, the largest unsplit one at seg_blocks 2
# (3 blocks), a last block of 1 (160), 16 (175) and 17 (176) bytes, even and odd segment counts, a one-block
# remainder, an odd block count for the pair loop
GRID_LENS = [0, 31, 159, 160, 175, 176, 223, 224, 415, 4063, 4096]
GRID_COUNTS = [1, 63, 64, 65, 130]
PHASES = [0, 0, 0, 8, 1]


def _oracle_single(precom):
    def fill(desc, hin, want):
        oracle().or_seal_batch(desc.ctypes.data, len(desc), hin.ctypes.data, want.ctypes.data, precom.ctypes.data, 0, 8)
    return fill


def _oracle_both_directions(desc, hin, want):
    """the key table of fanout_steer.py: entry t is precom t % NPRE under direction t // NPRE"""
    for direction in (0, 1):
        part = desc[desc["key_idx"] // fs.NPRE == direction].copy()
        part["key_idx"] %= fs.NPRE
        oracle().or_seal_batch(part.ctypes.data, len(part), hin.ctypes.data, want.ctypes.data, fs.PRECOMS.ctypes.data,
                               direction, 8)


def seal_and_check(env, g, what, seg_blocks, tables=None, sub=None, fill=None):
    """One split call into a sentinel-filled buffer, compared whole with the oracle and body by body with
    cz_seal_batch.  tables(plan) may replace the planner's tiles / joins / class_count / npart."""
    torch, dev, batch, _lib, precom, sub0 = env
    sub = sub0 if sub is None else sub
    fill = fill or _oracle_single(precom)
    runs, hin, subs, descs, out_bytes = g.build(batch)
    d_in = torch.from_numpy(hin).to(dev)
    d_subs = torch.from_numpy(np.ascontiguousarray(subs).view(np.uint8).copy()).to(dev)
    d_out = torch.full((out_bytes,), SENT, dtype=torch.uint8, device=dev)
    plan = batch.plan_fanout_split(runs, d_in, d_out, seg_blocks)
    if tables is not None:
        tables(plan)
    # the partial records start as garbage: a join that read a record no tile wrote shows
    work = torch.full((64 * max(plan.npart, 1),), 0xC3, dtype=torch.uint8, device=dev)
    batch.seal_fanout_split(plan.to(dev), d_in, d_subs, sub, d_out, work=work)
    desc = np.concatenate(descs)
    d_ref = torch.full((out_bytes,), SENT, dtype=torch.uint8, device=dev)
    batch.seal_batch(torch.from_numpy(desc.view(np.uint8).copy()).to(dev), len(desc), d_in, d_ref, sub, desc_np=desc)
    torch.cuda.synchronize()
    want = np.full(out_bytes, SENT, dtype=np.uint8)
    for r in runs:
        if owns(int(r["out_stride"])):   # the run owns whole slots: zeros past each body
            want[int(r["out_off"]):int(r["out_off"]) + int(r["count"]) * int(r["out_stride"])] = 0
    fill(desc, hin, want)
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


def grid(rng, lens, counts, distinct, seed):
    """every length x count x stride, flags 0..3, payloads and output regions at byte phases 0, 8 and 1; every
    other aligned region starts on a 128-byte line (EmitSegLines), the others 16-byte aligned (EmitShiftLines)"""
    g = Group(seed)
    k = 0
    for si in range(4):
        for count in counts:
            for length in lens:
                mlen = length + 33
                stride = [round_up(mlen, 128), round_up(mlen, 128) + 128, mlen, mlen + 7][si]
                out_phase = PHASES[(k * 3 + k // 7) % 5]
                if out_phase == 0 and k % 2 == 0:
                    g.out_at = round_up(g.out_at, 128)
                g.add(length, subscribers(rng, count, distinct), k % 4, stride, in_phase=PHASES[(k * 7 + si) % 5],
                      out_phase=out_phase)
                k += 1
    return g


@pytest.mark.parametrize("distinct", [True, False], ids=["key_per_subscriber", "three_keys"])
def test_grid_coverage(env, distinct):
    """11 lengths x 5 counts x 4 strides = 220 runs in one call at seg_blocks 2: a 256-lane workgroup holds waves
    of different runs and tiles, the tiles of one body meet inside cache lines, neighbouring bodies share lines at
    the dense strides; counters 2^32 - 1, 2^32, 2^63 and 2^64 - 2 inside one wave (subscribers())."""
    rng = np.random.default_rng(31 + distinct)
    g = grid(rng, GRID_LENS, GRID_COUNTS, distinct, 41)
    plan = seal_and_check(env, g, f"grid, distinct {distinct}", 2)[0]
    assert plan.class_count[LINES] and plan.class_count[DIRECT] and len(plan.joins)     # all three launches
    split = {int(t["run"]) for t in plan.tiles if int(t["part"]) != WHOLE}
    assert {g.rows[r]["len"] for r in split} == {160, 175, 176, 223, 224, 415, 4063, 4096}


def test_smallest_grid_with_a_join(env):
    """seg_blocks 1 on 1, 2 and 4 blocks: every tile is one block, tiles start at odd blocks (64 bytes into a line)"""
    rng = np.random.default_rng(33)
    g = grid(rng, [31, 95, 160], GRID_COUNTS, True, 42)
    plan = seal_and_check(env, g, "seg_blocks 1", 1)[0]
    assert plan.class_count[LINES] and plan.class_count[DIRECT] and len(plan.joins)
    assert set(plan.tiles["nblocks"].tolist()) == {1} and set(plan.tiles["nseg"].tolist()) == {1, 2, 4}


def test_nine_segments_the_ninth_a_single_block(env):
    rng = np.random.default_rng(34)
    g = Group(43)
    g.add(65536, subscribers(rng, 130, True), 1)
    plan = seal_and_check(env, g, "64 KiB x 130, seg_blocks 128", 128)[0]
    assert sorted(set(zip(plan.tiles["first_block"].tolist(), plan.tiles["nblocks"].tolist()))) == \
        [(128 * s, 128) for s in range(8)] + [(1024, 1)]
    assert plan.class_count == [18, 9] and len(plan.joins) == 3 and plan.npart == 130 * 9


def test_seg_blocks_zero(env):
    """the engine's segment length for the call's own size"""
    rng = np.random.default_rng(35)
    g = Group(44)
    g.add(4096, subscribers(rng, 130, True), 0)
    g.add(1024, subscribers(rng, 65, False), 3, stride=1057)
    plan = seal_and_check(env, g, "seg_blocks 0", 0)[0]
    assert len(plan.joins) == 3 + 2           # 65 and 17 blocks, both split at the automatic length (2 or 3 blocks)


def _own_tables(rng, runs, d_in_al, reverse=True):
    """tiles cut at random block boundaries, unequal lengths, another cut per wave; listed in reverse order"""
    def tables(plan):
        tiles, joins, part = [], [], 0
        for r, row in enumerate(runs):
            nblk = (row["len"] + 33 + 63) // 64
            for first in range(0, row["count"], 64):
                lanes = min(64, row["count"] - first)
                ncut = int(rng.integers(1, min(nblk, 7))) if nblk > 1 else 0
                cuts = [0] + sorted(rng.choice(np.arange(1, nblk), size=ncut, replace=False).tolist()) + [nblk] if ncut \
                    else [0, nblk]
                nseg = len(cuts) - 1
                cls = LINES if lanes == 64 and d_in_al(r) else DIRECT
                for s in range(nseg):
                    tiles.append((cls, (r, first, cuts[s], cuts[s + 1] - cuts[s], part + s if nseg > 1 else WHOLE, nseg)))
                if nseg > 1:
                    joins.append((r, first, part, nseg))
                    part += lanes * nseg
        if reverse:
            tiles.reverse()
            joins.reverse()
        tiles.sort(key=lambda t: t[0])          # (stable: by class, reversed inside)
        plan.tiles = np.array([t for _, t in tiles], dtype=plan.tiles.dtype)
        plan.joins = np.array(joins, dtype=plan.joins.dtype)
        plan.class_count = [sum(1 for c, _ in tiles if c == LINES), sum(1 for c, _ in tiles if c == DIRECT)]
        plan.npart = part
    return tables


def test_caller_built_tiles(env):
    """A caller's own tile table, as tests/test_gpu_segments.py does for frames: segments of unequal lengths --
    combine_tag's per-segment power path -- cut at random block boundaries, another cut for every wave of a run,
    a single-tile body with a partial record beside whole ones, tiles and joins listed in reverse order."""
    rng = np.random.default_rng(36)
    g = Group(45)
    for k, (length, count) in enumerate(((4096, 130), (1000, 65), (415, 64), (4063, 70), (100, 130), (31, 5))):
        g.add(length, subscribers(rng, count, k % 2 == 0), k % 4, in_phase=[0, 0, 8, 0, 1, 0][k],
              stride=None if k != 3 else 4063 + 33 + 7)
    in_al = [row["payload_off"] % 16 == 0 for row in g.rows]
    plan = seal_and_check(env, g, "caller-built tiles", 2, tables=_own_tables(rng, g.rows, lambda r: in_al[r]))[0]
    assert plan.class_count[LINES] and plan.class_count[DIRECT] and len(plan.joins)
    assert len({int(t["nblocks"]) for t in plan.tiles if int(t["run"]) == 0}) > 2


def test_class_is_never_a_correctness_choice(env):
    """Runs whose payload or output is off 16-byte alignment and partial waves under tables that put every tile
    into the line slice, then every tile into the lane-wise slice: each wave checks its own run."""
    rng = np.random.default_rng(37)
    g = Group(46)
    for k, (length, in_phase, out_phase, count) in enumerate((
            (1000, 0, 0, 130),     # aligned: the line emitters in the line slice
            (1000, 1, 0, 130),     # payload at byte phase 1 (per_lane_ptr)
            (1000, 8, 0, 65),
            (1000, 0, 1, 130),     # output at byte phase 1: EmitShiftLines
            (1000, 0, 8, 64),
            (4063, 1, 1, 70),
            (223, 0, 0, 63),       # no full wave
            (100, 0, 0, 5))):      # whole bodies
        g.add(length, subscribers(rng, count, k % 2 == 0), k % 4, in_phase=in_phase, out_phase=out_phase,
              stride=None if k != 5 else 4063 + 33 + 7)

    def all_in(cls):
        def tables(plan):
            plan.class_count = [len(plan.tiles), 0] if cls == LINES else [0, len(plan.tiles)]
        return tables
    seal_and_check(env, g, "every tile in the line slice", 2, tables=all_in(LINES))
    seal_and_check(env, g, "every tile in the lane-wise slice", 2, tables=all_in(DIRECT))
    seal_and_check(env, g, "every tile in the line slice, seg_blocks 3", 3, tables=all_in(LINES))


# ---- steered Poly1305 edges -------------------------------------------------------------------------
COUNT = 70                         # one full wave and a tail of 6
STEERED_LANES = (0, 37, 63, 67)    # first / inner / last lane of the wave, and a tail lane


@pytest.fixture(scope="module")
def steer_sub(env):
    torch, dev, batch, _lib = env[:4]
    keys = torch.from_numpy(fs.PRECOMS.copy()).to(dev).view(fs.NPRE, 32)
    return torch.cat([batch.subkeys(keys, _lib.CZ_DIR_C2S), batch.subkeys(keys, _lib.CZ_DIR_S2C)])


@pytest.mark.parametrize("length", [223, 4063])
def test_steered_poly1305_edges(env, steer_sub, length):
    """One payload steered (poly_steer.steer, through fanout_steer.cases: built from the oracle and asserted
    against it while built) so that ONE subscriber's MAC walks every ps.TARGETS entry and the h + m ripples; that
    subscriber sits at lanes 0, 37, 63 of the full wave and 67 of the tail, every other lane seals the same
    payload under another key and counter.  seg_blocks 2: 4 blocks in two segments, 64 blocks in 32 -- the
    accumulator's edge is reached in the join, from partials.  All the cases of a length ride in one call, one
    run per case, alternating 128-byte slots (the line class for the full wave) with the dense unaligned layout."""
    batch = env[2]
    rng = np.random.default_rng(6000 + length)
    built = fs.cases(length)
    assert [c.name for c in built] == [s[0] for s in fs.specs(length)] and len(built) >= 48
    mlen = length + 33
    g = Group(47)
    for k, case in enumerate(built):
        assert len(case.payload) == length
        subs = np.zeros(COUNT, dtype=batch.FANOUT_SUB_DTYPE)
        subs["counter"] = rng.integers(0, 1 << 64, size=COUNT, dtype=np.uint64)
        subs["key_idx"] = rng.integers(0, 2 * fs.NPRE, size=COUNT)
        for lane in STEERED_LANES:
            subs[lane] = (case.counter, case.key_idx, 0)
        dense = k % 2 == 1
        g.add(length, subs, case.flags, stride=mlen + 7 if dense else None, in_phase=[0, 0, 1][k % 3],
              out_phase=1 if dense else 0)
        g.payloads[-1] = (g.payloads[-1][0], case.payload)

    def build(b, inner=g.build):
        # (Group.build clears the payload's top bit against its filler; the steered payload goes in as it is)
        runs, hin, subs, descs, out_bytes = inner(b)
        for off, p in g.payloads:
            hin[off:off + len(p)] = np.frombuffer(p, dtype=np.uint8)
        return runs, hin, subs, descs, out_bytes
    g.build = build
    plan, runs, hin, subs, d_out = seal_and_check(env, g, f"steered, len {length}", 2, sub=steer_sub,
                                                  fill=_oracle_both_directions)
    assert plan.class_count[LINES] and plan.class_count[DIRECT] and len(plan.joins) == 2 * len(built)
    got = d_out.cpu().numpy()
    for k, case in enumerate(built):
        for lane in STEERED_LANES:
            o = int(runs["out_off"][k]) + lane * int(runs["out_stride"][k])
            body = got[o:o + mlen].tobytes()
            assert body[16:32] == case.tag, f"{case.name}: lane {lane} tag {body[16:32].hex()} != {case.tag.hex()}"
            assert body == case.body, f"{case.name}: lane {lane}"


def test_round_trip(env):
    """split runs opened again by cz_open_batch: every status OK, flags, nonces and payloads back"""
    torch, dev, batch, _lib, precom, sub = env
    rng = np.random.default_rng(38)
    g = Group(48)
    lens = [4096, 415, 1000, 160]
    for r, length in enumerate(lens):
        g.add(length, subscribers(rng, 130, True), r % 4)
    plan, runs, hin, subs, d_out = seal_and_check(env, g, "round trip", 2)
    assert len(plan.joins) == 4 * 3
    n, pstride = len(lens) * 130, 4224
    odesc = np.zeros(n, dtype=DESC_DTYPE)
    for r, length in enumerate(lens):
        sl = slice(r * 130, (r + 1) * 130)
        odesc["in_off"][sl] = runs["out_off"][r] + np.arange(130, dtype=np.uint64) * runs["out_stride"][r]
        odesc["len"][sl] = length + 33
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
    assert np.array_equal(st >> 8, np.repeat(np.arange(len(lens)) % 4, 130))
    assert np.array_equal(nonces.cpu().numpy().view(np.uint64), subs["counter"])
    plain = d_plain.cpu().numpy().reshape(n, pstride)
    for r, length in enumerate(lens):
        off = int(runs["payload_off"][r])
        assert np.all(plain[r * 130:(r + 1) * 130, :length] == hin[None, off:off + length]), f"run {r}"


# ---- engine ------------------------------------------------------------------------------------------
def _traffic():
    """publishes of 1024, 4096 and 65 536 bytes to 64, 65 and 520 connections between sends; the 64 KiB publishes
    to all 520 make 34 MiB of wire each, so the flush runs in groups and their edges cut those publishes"""
    p = {n: splitmix_bytes(n, 7000 + n) for n in (1024, 4096, 65536, 1000, 17, 5000)}
    lists = {64: list(range(100, 164)), 65: list(np.random.default_rng(4).permutation(NCON)[:65]), 520: list(range(NCON))}
    small = [("send", 7, p[17], False)]
    for k, (n, size) in enumerate([(1024, 64), (4096, 65), (1024, 520), (65536, 64), (4096, 520), (1024, 65),
                                   (4096, 64), (65536, 65), (1000, 520), (1024, 63)]):   # (1000 B and 63 frames: not routed)
        small += [("pub", lists.get(size, list(range(63))), p[n], k % 3 == 0), ("send", (7, 300, 519)[k % 3], p[5000], False)]
    big = [("send", 7, p[17], False), ("pub", lists[520], p[65536], False), ("send", 300, p[5000], True),
           ("pub", lists[520], p[4096], True), ("pub", lists[65], p[1024], False), ("send", 519, p[17], False)]
    return small, big


def test_engine_routes_long_publishes(env):
    """Two engines take the same flushes, one with fanout_split 1024 and one with 0 (the rule off): both wires equal
    each other and V2Encoder(oracle seal), flush after flush over the buffers the last one left; then a second
    engine's flush_in delivers every message of the routed wire."""
    from jeromq_amd.engine import CurveBatchEngine
    L = env[3]
    tune = L.lib().cz_tune
    default = tune(b"fanout_split", 0)
    assert tune(b"fanout_split", default) == 0
    routed, plain = Leg({b"fanout_split": 1024}), Leg({b"fanout_split": 0})
    small, big = _traffic()
    sent = [0] * NCON
    try:
        for name, ops in (("small", small), ("big", big), ("small again", small)):
            before = list(sent)
            wires = [routed.flush(L, ops), plain.flush(L, ops)]
            want = _expected(ops, sent)
            if name == "big":
                assert sum(len(w) for w in want) > 32 << 20      # several groups: a publish cut by their edges
            for c in range(NCON):
                assert wires[0][c] == want[c], f"{name}, routed: connection {c}"
                assert wires[1][c] == want[c], f"{name}, unrouted: connection {c}"
            for leg in (routed, plain):
                assert [leg.eng.nonce(x) for x in leg.cc] == [3 + s for s in sent], name
            if name != "small":
                continue
            # receive leg, on the first flush (every length to every list size): the routed wire delivered
            rx = CurveBatchEngine(arena_bytes=1 << 16)
            try:
                rc = [rx.add_connection(_precom(i), as_server=True) for i in range(NCON)]
                for c in range(NCON):
                    assert rx.recv(rc[c], wires[0][c]) == 0
                rx.flush_in()
                for c in range(NCON):
                    msgs = [(op[2], 1 if op[3] else 0) for op in ops
                            for x in ([op[1]] if op[0] == "send" else op[1]) if x == c]
                    assert rx.error(rc[c]) == (0, 0), f"connection {c}"
                    assert rx.messages_in(rc[c]) == msgs, f"connection {c}"
                    assert len(msgs) == sent[c] - before[c] and rx.peer_nonce(rc[c]) == 2 + sent[c]
            finally:
                rx.close()
    finally:
        routed.eng.close()
        plain.eng.close()
    assert tune(b"fanout_split", default) == default
