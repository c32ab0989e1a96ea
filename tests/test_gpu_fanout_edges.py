"""GPU: the PUB fan-out path at its Poly1305 edges, across flush-group edges and on connections
other than the default one.

1. k_seal_fanout (cz_seal_fanout) on steered payloads.  The kernel instantiates seal_frame three
   more times (ST_LINES, ST_REGION, ST_DIRECT, each with the lane-wise code for partial waves), in
   the per-lane-key form; random payloads reach the conditional subtraction of p, the h4 folds, the
   all-ones carry chains and the all-zero / all-ones tags with probability ~2^-100.  fanout_steer.py
   steers one payload for one (key, counter) pair; that pair sits at lanes 0, 37 and 63 of a full
   wave and at lane 67 of the tail, every other lane seals the same payload under a random key and
   counter.  The whole sentinel-filled output buffer is compared with the oracle (or_seal_batch, one
   call per direction of the mixed key table), and the steered lanes with the body whose tag is the
   big-integer poly_steer.poly1305.

2. cz_engine_publish across flush-group edges.  A flush of 16 MiB or more runs as several groups on
   their own streams; a publish cut by a group edge is two cz_seal_fanout runs, and a run below
   fanout_min returns to the segment plan.  Two engines (publish runs routed to cz_seal_fanout from
   4 frames up, and never) take the same traffic flush after flush, so every flush runs over the
   device buffers the one before left.  Expected nonces come from this module's own count of the
   frames it queued, never from the engine.  Where the edges fall is proved on the CPU
   (tests/test_fanout_steer.py); nothing here depends on it.

3. Publish on S2C connections, at nonces around 2^32, 2^63 and 2^64, in place from a msg_alloc
   buffer at interior offsets 1 and 8, with COMMAND and MORE, with a remove_connection between the
   publish and the flush, and delivered by a receiving engine's flush_in.

Every comparison is bit-exact against the CPU oracle; the routed and the unrouted engine's wires are
compared with each other in addition to that.
"""
import ctypes

import numpy as np
import pytest

import fanout_steer as fs
from cz_testlib import DESC_DTYPE, oracle, or_curve_encode, splitmix_bytes, v2_encode
from test_gpu_fanout import SENT, _precom, check, owns, shared_desc

pytestmark = pytest.mark.gpu

COUNT = 70                         # one full wave and a tail of 6
STEERED_LANES = (0, 37, 63, 67)    # first / inner / last lane of the wave, and a tail lane
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from jeromq_amd import _lib, batch
    dev = torch.device("cuda:0")
    keys = torch.from_numpy(fs.PRECOMS.copy()).to(dev).view(fs.NPRE, 32)
    sub = torch.cat([batch.subkeys(keys, _lib.CZ_DIR_C2S), batch.subkeys(keys, _lib.CZ_DIR_S2C)])
    return torch, dev, batch, _lib, sub


# ---- 1. the kernel on steered payloads ----------------------------------------------------------------
def _launch(env, rng, case, stride, out_phase, in_phase):
    """One launch of COUNT subscribers over the steered payload; (got, want, desc) over the whole
    sentinel-filled buffer, as test_gpu_fanout.run_fanout returns them"""
    torch, dev, batch, _lib, sub = env
    length = len(case.payload)
    mlen = length + 33
    subs = np.zeros(COUNT, dtype=batch.FANOUT_SUB_DTYPE)
    subs["counter"] = rng.integers(0, 1 << 64, size=COUNT, dtype=np.uint64)
    subs["key_idx"] = rng.integers(0, 2 * fs.NPRE, size=COUNT)
    for lane in STEERED_LANES:
        subs[lane] = (case.counter, case.key_idx, 0)
    # the payload between guard bytes, at the asked byte phase
    in_off = 64 + in_phase
    hin = rng.integers(0, 256, size=in_off + length + 256, dtype=np.uint8)
    hin[in_off:in_off + length] = np.frombuffer(case.payload, dtype=np.uint8)
    out_off0 = 256 + out_phase
    out_bytes = out_off0 + (COUNT - 1) * stride + (stride if owns(stride) else mlen) + 256
    d_in = torch.from_numpy(hin).to(dev)
    d_subs = torch.from_numpy(subs.view(np.uint8).copy()).to(dev)
    d_out = torch.full((out_bytes,), SENT, dtype=torch.uint8, device=dev)
    batch.seal_fanout(d_in[in_off:], length, case.flags, d_subs, sub, d_out[out_off0:], stride, COUNT)
    torch.cuda.synchronize()
    desc = shared_desc(subs, length, case.flags, in_off, out_off0, stride)
    want = np.full(out_bytes, SENT, dtype=np.uint8)
    if owns(stride):
        want[out_off0:out_off0 + COUNT * stride] = 0   # the batch owns whole slots: zeros past each body
    for direction in (0, 1):
        part = desc[desc["key_idx"] // fs.NPRE == direction].copy()
        part["key_idx"] %= fs.NPRE
        oracle().or_seal_batch(part.ctypes.data, len(part), hin.ctypes.data, want.ctypes.data, fs.PRECOMS.ctypes.data,
                               direction, 8)
    return d_out.cpu().numpy(), want, desc


@pytest.mark.parametrize("length,layout", fs.layout_cases())
def test_fanout_steered_payloads(env, length, layout):
    """Every spec at this length: 48 launches (50 from three MAC blocks up), twice that for
    dense_unaligned.  slots128: stride round_up(mlen, 128), ST_LINES from payload 223 (body 256) up
    and ST_REGION below; region16: a multiple of 16 up to 256 that is no multiple of 128, ST_REGION;
    dense_unaligned: stride mlen + 7 from an output base at byte phase 1, ST_DIRECT, the payload at
    phase 0 (aligned source) and at phase 1 (per_lane_ptr).  The tail of 6 runs the lane-wise code
    of whichever kernel the full wave took."""
    rng = np.random.default_rng(5000 + length)
    mlen = length + 33
    stride = fs.LAYOUTS[layout](mlen)
    out_phase, in_phases = (1, (0, 1)) if layout == "dense_unaligned" else (0, (0,))
    built = fs.cases(length)
    assert len(built) == len(fs.specs(length))
    for case in built:
        for in_phase in in_phases:
            what = f"len {length} {layout} in+{in_phase} {case.name}"
            got, want, desc = _launch(env, rng, case, stride, out_phase, in_phase)
            for lane in STEERED_LANES:
                o = int(desc["out_off"][lane])
                body = got[o:o + mlen].tobytes()
                assert body[16:32] == case.tag, f"{what}: lane {lane} tag {body[16:32].hex()} != {case.tag.hex()}"
                assert body == case.body, f"{what}: lane {lane}"
            check(got, want, want, desc, what)


# ---- 2. publishes across flush-group edges ----------------------------------------------------------
class Leg:
    """One engine and this module's own count of the frames it queued per connection"""

    def __init__(self, fanout_min, roles, starts, arena):
        from jeromq_amd.engine import CurveBatchEngine
        self.fanout_min, self.roles, self.starts = fanout_min, roles, starts
        self.eng = CurveBatchEngine(arena_bytes=arena)
        self.cc = [self.eng.add_connection(_precom(i), as_server=roles[i], cn_nonce=starts[i])
                   for i in range(len(roles))]
        self.sent = [0] * len(roles)

    def queue(self, sc):
        eng, bufs = self.eng, {}
        for op in sc.ops:
            if op[0] == "alloc":
                p = sc.payloads[op[1]]
                bufs[op[1]] = eng.msg_alloc(len(p))
                assert bufs[op[1]] is not None
                ctypes.memmove(bufs[op[1]], p, len(p))
            elif op[0] == "send":
                _, c, name, more, command = op
                assert eng.send(self.cc[c], bufs.get(name, sc.payloads[name]), more=more, command=command) == 0
                self.sent[c] += 1
            else:
                _, ids, name, more, command = op
                assert eng.publish([self.cc[c] for c in ids], bufs.get(name, sc.payloads[name]), more=more,
                                   command=command) == len(ids)
                for c in ids:
                    self.sent[c] += 1

    def flush(self, L, gone=()):
        """flush_out under this leg's fanout_min; every connection's wire (None for the removed ones)"""
        old = L.lib().cz_tune(b"fanout_min", self.fanout_min)
        try:
            self.eng.flush_out()
        finally:
            L.lib().cz_tune(b"fanout_min", old)
        return [None if i in gone else self.eng.wire_out(c) for i, c in enumerate(self.cc)]


def _roles(ncon):
    return [i % 2 == 0 for i in range(ncon)]   # alternating server (S2C) and client (C2S)


def _starts(roles, at=None):
    return [(at or {}).get(i, 2 if s else 3) for i, s in enumerate(roles)]


def _expected(frames, payloads, roles, nonce0):
    """per connection: V2Encoder(oracle seal) of its frames in send order under its own direction,
    nonces counted up from nonce0[c]"""
    out = [[] for _ in roles]
    for f in frames:
        k = len(out[f.conn])
        body = or_curve_encode(payloads[f.name], f.flags, (nonce0[f.conn] + k) & M64, 1 if roles[f.conn] else 0,
                               _precom(f.conn))
        out[f.conn].append(v2_encode(body))
    return [b"".join(x) for x in out]


@pytest.fixture(scope="module")
def legs(env):
    """the routed and the unrouted engine of the whole sweep, 520 connections each"""
    roles = _roles(fs.NCON)
    pair = [Leg(fs.SWEEP_FANOUT_MIN, roles, _starts(roles), 4 << 20), Leg(1 << 30, roles, _starts(roles), 4 << 20)]
    yield pair
    for leg in pair:
        leg.eng.close()


def _flush_and_check(env, legs, sc):
    L = env[3]
    before = list(legs[0].sent)
    assert legs[1].sent == before
    wires = []
    for leg in legs:
        leg.queue(sc)
        wires.append(leg.flush(L))
    want = _expected(sc.frames(), sc.payloads, legs[0].roles, [(s + b) & M64 for s, b in zip(legs[0].starts, before)])
    for leg, wire, how in zip(legs, wires, ("routed", "unrouted")):
        for c in range(fs.NCON):
            assert wire[c] == want[c], f"{sc.name}, {how}: connection {c} ({len(wire[c])} bytes, want {len(want[c])})"
            assert leg.eng.nonce(leg.cc[c]) == (leg.starts[c] + leg.sent[c]) & M64, f"{sc.name}, {how}: nonce of {c}"
    assert wires[0] == wires[1]
    return wires


@pytest.mark.parametrize("k", fs.SWEEP_K)
@pytest.mark.parametrize("side", ["trailing", "leading"])
def test_publish_split_by_a_group_edge(env, legs, side, k):
    """Four publishes of 8192 bytes (four payloads, the second with MORE) to 520 connections and 2 k
    sends behind or in front: two groups, the edge k frames into the third publish or k frames before
    the end of the second, so the run on the short side is empty, one frame, fanout_min - 1 (both
    back in the segment plan), fanout_min and fanout_min + 1 frames."""
    _flush_and_check(env, legs, fs.edge_sweep(side, k))


def test_publish_split_by_two_edges(env, legs):
    """One publish to a list of 3300 entries, the 520 ids repeated in a shuffled order: three groups,
    three runs, and an id named several times gets consecutive nonces"""
    _flush_and_check(env, legs, fs.two_edges())


def test_mixed_flush(env, legs):
    """Publishes of 0, 100, 223 and 65 536 bytes to lists of 3, 63, 64, 65 and 520 between sends of
    other sizes, a payload msg_alloc'ed first and queued last; the gather-write pieces of two
    connections whose frames interleave with others' join to their streams."""
    sc = fs.mixed()
    wires = _flush_and_check(env, legs, sc)
    frames = sc.frames()
    for leg, wire in zip(legs, wires):
        for c in fs.IOV_CONNS:
            # one piece per run of consecutive frames of the connection
            runs = []
            for i, f in enumerate(frames):
                if f.conn == c:
                    n = fs.frame_wire_bytes(len(sc.payloads[f.name]))
                    if i and frames[i - 1].conn == c:
                        runs[-1] += n
                    else:
                        runs.append(n)
            pieces = leg.eng.wire_iov(leg.cc[c])
            assert [n for _, n in pieces] == runs and len(runs) > 3
            assert b"".join(ctypes.string_at(a, n) for a, n in pieces) == wire[c]


# ---- 3. publish on non-default connections -------------------------------------------------------------
NCON4 = 130
AT_2_32, BELOW_2_63, AT_2_64, WRAPS = (10, 11), (100, 101), (102, 103), 110
REMOVED = (3, 64)


@pytest.mark.parametrize("fanout_min", [2, 1 << 30])
def test_publish_on_other_connections(env, fanout_min):
    """130 connections, servers (S2C) and clients (C2S) mixed; 10 and 11 start at nonce 2^32 - 2 and
    cross 2^32, 100 and 101 at 2^63 - 3 with three frames (they stay below 2^63), 102 and 103 at
    2^64 - 8 with three frames, 110 at 2^64 - 8 with thirteen (its nonce wraps to 0).  Publishes with
    MORE and with COMMAND, in place from a msg_alloc buffer at interior offsets 1 and 8 (the
    per_lane_ptr path of the kernel when routed), connections 3 and 64 removed between the last
    publish and the flush: their frames leave, everyone else's wire and nonce are the oracle's, and an
    id added again starts clean.

    Receive leg: every stream is fed in random pieces over two flush_in calls to a second engine
    whose connections have the opposite role, the same precom and cn_peer_nonce one below the sender's
    start; every payload and flags value arrives in order, peer_nonce ends at the last nonce sent,
    no connection fails.  Connection 110, whose stream wraps 2^64, is left out of the receive leg (no
    stream here crosses 2^63): the replay check compares nonces as signed longs, which is pinned at
    kernel level (tests/test_gpu_parity.py::test_open_signed_nonce_compare, tests/test_gpu_fuzz.py)."""
    from jeromq_amd.engine import CurveBatchEngine
    L = env[3]
    rng = np.random.default_rng(130)
    roles = [i % 3 != 1 for i in range(NCON4)]
    at = {c: (1 << 32) - 2 for c in AT_2_32}
    at.update({c: (1 << 63) - 3 for c in BELOW_2_63})
    at.update({c: (1 << 64) - 8 for c in AT_2_64 + (WRAPS,)})
    assert {roles[c] for c in AT_2_32} == {roles[c] for c in BELOW_2_63} == {roles[c] for c in AT_2_64} == {False, True}
    leg = Leg(fanout_min, roles, _starts(roles, at), 1 << 20)
    eng, cc = leg.eng, leg.cc
    msgs = [[] for _ in range(NCON4)]   # (payload, flags) per connection, in send order

    def publish(ids, payload, data, more=False, command=False):
        assert eng.publish([cc[c] for c in ids], payload, more=more, command=command) == len(ids)
        for c in ids:
            msgs[c].append((data, (L.CZ_MSG_MORE if more else 0) | (L.CZ_MSG_COMMAND if command else 0)))

    every = list(range(NCON4))
    y, z, w = splitmix_bytes(4096, 41), splitmix_bytes(100, 42), splitmix_bytes(0, 43)
    publish(every, y, y, more=True)
    publish(every[:70], z, z, command=True)
    raw = splitmix_bytes(300, 44)
    buf = eng.msg_alloc(len(raw))
    assert buf is not None and ctypes.addressof(buf) % 16 == 0
    ctypes.memmove(buf, raw, len(raw))
    publish(every, (ctypes.c_uint8 * 200).from_address(ctypes.addressof(buf) + 1), raw[1:201])
    publish(every[5:75], (ctypes.c_uint8 * 223).from_address(ctypes.addressof(buf) + 8), raw[8:231], more=True,
            command=True)
    # published where they lie: the arena grew by nothing, the next buffer follows the 300 bytes
    probe = eng.msg_alloc(1)
    assert ctypes.addressof(probe) == ctypes.addressof(buf) + 304
    for j in range(10):
        p = splitmix_bytes(50 + 30 * j, 50 + j)
        assert eng.send(cc[WRAPS], p, more=j % 2 == 1) == 0
        msgs[WRAPS].append((p, L.CZ_MSG_MORE if j % 2 == 1 else 0))
    publish(every, w, w)
    assert [len(msgs[c]) for c in BELOW_2_63 + AT_2_64 + (WRAPS,)] == [3, 3, 3, 3, 13]
    for c in REMOVED:
        eng.remove_connection(cc[c])
    wires = leg.flush(L, gone=REMOVED)
    live = [c for c in every if c not in REMOVED]
    for c in live:
        want = b"".join(v2_encode(or_curve_encode(p, fl, (leg.starts[c] + k) & M64, 1 if roles[c] else 0, _precom(c)))
                        for k, (p, fl) in enumerate(msgs[c]))
        assert wires[c] == want, f"connection {c}"
        assert eng.nonce(cc[c]) == (leg.starts[c] + len(msgs[c])) & M64
    assert eng.nonce(cc[WRAPS]) == 5 and eng.nonce(cc[AT_2_32[0]]) == (1 << 32) + 3
    # nothing of the removed connections' is on the wire: the flush holds the live frames only
    assert sum(len(wires[c]) for c in live) == sum(fs.frame_wire_bytes(len(p)) for c in live for p, _ in msgs[c])
    for c in REMOVED:
        with pytest.raises(L.CzError):
            eng.wire_out(cc[c])
    # an id added again starts clean: its own key, the default nonce, only the new frame
    fresh_key = splitmix_bytes(32, 4242)
    fresh = eng.add_connection(fresh_key, as_server=True)
    assert fresh in [cc[c] for c in REMOVED]
    assert eng.publish([fresh, cc[0], fresh], z) == 3
    again = leg.flush(L, gone=REMOVED)
    assert eng.wire_out(fresh) == b"".join(v2_encode(or_curve_encode(z, 0, 2 + k, 1, fresh_key)) for k in range(2))
    assert eng.nonce(fresh) == 4
    assert again[0] == v2_encode(or_curve_encode(z, 0, leg.starts[0] + len(msgs[0]), 1 if roles[0] else 0, _precom(0)))
    assert eng.nonce(cc[0]) == leg.starts[0] + len(msgs[0]) + 1
    eng.close()

    # receive leg
    rx = CurveBatchEngine(arena_bytes=1 << 16)
    heard = [c for c in live if c != WRAPS]
    assert set(AT_2_32 + BELOW_2_63 + AT_2_64) <= set(heard)
    rc = {c: rx.add_connection(_precom(c), as_server=not roles[c], cn_peer_nonce=(leg.starts[c] - 1) & M64)
          for c in heard}
    got = {c: [] for c in heard}
    cut = {c: int(rng.integers(1, len(wires[c]))) for c in heard}
    for half in (0, 1):
        for c in heard:
            part = wires[c][:cut[c]] if half == 0 else wires[c][cut[c]:]
            pos = 0
            while pos < len(part):
                step = int(rng.integers(1, 3000))
                assert rx.recv(rc[c], part[pos:pos + step]) == 0
                pos += step
        rx.flush_in()
        for c in heard:
            got[c] += rx.messages_in(rc[c])
    for c in heard:
        assert rx.error(rc[c]) == (0, 0), f"connection {c}"
        assert got[c] == msgs[c], f"connection {c}"
        assert rx.peer_nonce(rc[c]) == (leg.starts[c] + len(msgs[c]) - 1) & M64
    rx.close()
