"""GPU: batch.relay_streams (cz_relay_streams) against tests/relay_streams_model.py -- V2Decoder's walk, the
receive rule of tests/rx_model.py and the CPU oracle's seal; tests/test_relay_streams_host.py checks that model
against rx_model.stream_model.  Truth never comes from the library under test.

Whole 0xA5-filled buffers are compared: every accepted body is byte for byte the oracle's seal under the outbound
key and counter + k, headers are unchanged, rejected bodies are zeros, and the bytes around and between the
streams, trailing partial frames included, are untouched.  The second yardstick is batch.relay_batch out of place
on descriptors built from wire.parse with prev chains."""
import functools

import numpy as np
import pytest

import rx_model as rx
from cz_testlib import DESC_DTYPE, or_curve_encode, splitmix_bytes, v2_encode
from relay_streams_model import stream_expect

pytestmark = pytest.mark.gpu

SENT = 0xA5
OTHER = 0x5A                # the fill of an out-of-place output
PRECOMS = (rx.PRECOM, splitmix_bytes(32, 4243))
KIN, KOUT = 0, 3            # table rows: 2k pair k client-to-server, 2k + 1 server-to-client
COUNTER0 = (1 << 64) - 40   # the outbound counters of the later streams wrap
COUNTS = (1, 63, 65, 257)   # 257: one past BLOCK, for k_v2_place's shares
# body sizes per frame slot: the smallest, the flags byte only, the block edge on both sides, the 2-byte to 9-byte
# header edge
SIZES = (33, 34, 33 + 63, 33 + 64, 33 + 65, 255, 256)
FAULTS = (None, "tag", "replay", "name", "short20", "short12")
TAILS = (b"", b"\x01", b"\x02\x00\x00\x00\x00", b"\x00\x28" + bytes(range(10)), b"\x02" + bytes(8))
TAIL_RC = (0, 0, 0, 0, rx.CZ_EPROTO)    # a header cut short twice, a body cut short, LARGE with size 0


class _Gpu:
    pass


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from jeromq_amd import _lib, batch, wire
    g = _Gpu()
    g.torch, g.dev, g.L, g.batch, g.wire = torch, torch.device("cuda:0"), _lib, batch, wire
    rows = []
    for p in PRECOMS:
        k = torch.tensor(list(p), dtype=torch.uint8, device=g.dev).view(1, 32)
        rows += [batch.subkeys(k, _lib.CZ_DIR_C2S), batch.subkeys(k, _lib.CZ_DIR_S2C)]
    g.subkeys = torch.cat(rows)
    return g


def _stream(i):
    """stream i: 5, 4, 3, 2, 1, 0 frames (i % 6); the five-frame streams carry one fault in the middle, the
    four-frame ones a tail, every second three-frame one MORE on every frame; stream 2 holds the 4129-byte body.
    Returns (bytes, floor, expected scan rc)."""
    nf, j = (5 - i) % 6, i // 6
    floor = 10 + 3 * i
    fault = FAULTS[j % len(FAULTS)] if nf == 5 else None
    frames = b""
    for k in range(nf):
        size = 4129 if (i, k) == (2, 1) else SIZES[(i + 2 * k) % len(SIZES)]
        more = 1 if (nf == 3 and j % 2 == 0) else (i + k) & 1
        nonce = floor + 1 + 2 * k
        if k == 2 and fault == "replay":
            nonce = floor + 1 + 2 * (k - 1)
        body = bytearray(or_curve_encode(splitmix_bytes(size - 33, 1000 * i + k), more, nonce, KIN & 1, PRECOMS[KIN >> 1]))
        if k == 2 and fault == "tag":
            body[16 + (i % 16)] ^= 1 << (i % 8)
        elif k == 2 and fault == "name":
            body[3] ^= 0x20
        elif k == 2 and fault in ("short20", "short12"):
            body = body[:int(fault[5:])]
        frames += v2_encode(bytes(body), more)
    t = j % len(TAILS) if nf == 4 else 0
    return frames + TAILS[t], floor, TAIL_RC[t]


@functools.lru_cache(maxsize=None)
def build(n):
    """the wire of n streams packed 3..18 bytes apart (every byte phase), what the model expects of each, and the
    expected buffers in place and out of place; computed once per n"""
    streams = [_stream(i) for i in range(n)]
    at, offs = 5, []
    for i, (w, _f, _rc) in enumerate(streams):
        offs.append(at)
        at += len(w) + 3 + i % 16
    host = np.full(at + 64, SENT, dtype=np.uint8)
    for o, (w, _f, _rc) in zip(offs, streams):
        host[o:o + len(w)] = np.frombuffer(w, dtype=np.uint8)
    mem = host.tobytes()
    exps = [stream_expect(w, f, KIN & 1, PRECOMS[KIN >> 1], (COUNTER0 + 7 * i) & rx.M64, KOUT & 1, PRECOMS[KOUT >> 1],
                          behind=mem[o + len(w):o + len(w) + 16]) for i, (o, (w, f, _rc)) in enumerate(zip(offs, streams))]
    inplace, outplace = host.copy(), np.full(len(host), OTHER, dtype=np.uint8)
    for o, e in zip(offs, exps):
        inplace[o:o + e.consumed] = np.frombuffer(e.out, dtype=np.uint8)
        outplace[o:o + e.consumed] = np.frombuffer(e.out, dtype=np.uint8)
    if n >= 63:         # the table holds what it says
        assert {o % 4 for o in offs} == {0, 1, 2, 3} and any(len(w) == 0 for w, _f, _rc in streams)
        assert {e.fail_status for e in exps} == {rx.ST_OK, rx.ST_CRYPTO, rx.ST_SEQUENCE, rx.ST_COMMAND, rx.ST_MALFORMED}
        assert any(0 < e.whole_bytes < e.ok_bytes for e in exps) and any(e.whole_bytes == 0 < e.ok_bytes for e in exps)
        assert any(e.rc == rx.CZ_EPROTO and e.ok_frames == 4 for e in exps)
        assert sum(s == 4129 for e in exps for _h, _b, s in e.frames) == 1
        assert any(e.consumed < len(w) for e, (w, _f, _rc) in zip(exps, streams))
    return streams, offs, host, exps, inplace, outplace


def _run(g, n, in_place, desc_cap=None, kin=KIN, kout=KOUT, counters=None, host=None):
    streams, offs, host0, exps, _i, _o = build(n)
    host = host0 if host is None else host
    W, B, t, u8 = g.wire, g.batch, g.torch, g.torch.uint8
    st = np.zeros(n, dtype=W.V2_STREAM_DTYPE)
    st["off"], st["len"] = offs, [len(w) for w, _f, _rc in streams]
    st["floor"], st["key_idx"] = [f for _w, f, _rc in streams], kin
    to = np.zeros(n, dtype=B.FANOUT_SUB_DTYPE)
    to["counter"] = [(COUNTER0 + 7 * i) & rx.M64 for i in range(n)] if counters is None else counters
    to["key_idx"] = kout
    N = sum(len(e.frames) for e in exps)
    cap = max(N, 1)
    d_wire = t.from_numpy(host.copy()).to(g.dev)
    d_out = d_wire if in_place else t.full((len(host),), OTHER, dtype=u8, device=g.dev)
    buf = dict(scan=t.full((n * 32,), SENT, dtype=u8, device=g.dev), desc=t.full((cap * 40,), SENT, dtype=u8, device=g.dev),
               to_frames=t.full((cap * 16,), SENT, dtype=u8, device=g.dev),
               status=t.full((cap,), -1, dtype=t.int16, device=g.dev), nonces=t.full((cap,), -1, dtype=t.int64, device=g.dev),
               results=t.full((n * 32,), SENT, dtype=u8, device=g.dev))
    rc, nframes = B.relay_streams(W.to_device(st, g.dev), W.to_device(to, g.dev), d_wire, d_out, buf["scan"], buf["desc"],
                                  buf["to_frames"], g.subkeys, buf["status"], buf["nonces"], buf["results"],
                                  desc_cap=desc_cap, streams_np=st, to_np=to)
    t.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in buf.items()}
    got.update(rc=rc, nframes=nframes, N=N, out=d_out.cpu().numpy(), wire=d_wire.cpu().numpy(), to=to, st=st)
    return got


def _check(g, n, got, exps, offs, want_out):
    B, W = g.batch, g.wire
    bad = []
    assert (got["rc"], got["nframes"]) == (0, got["N"])
    if got["out"].tobytes() != want_out.tobytes():
        d = np.flatnonzero(got["out"] != want_out)
        bad.append(f"output differs at {len(d)} bytes, first {d[:8]}")
    scan = got["scan"].view(W.V2_STREAM_RESULT_DTYPE)
    cut = got["results"].view(B.RELAY_STREAM_RESULT_DTYPE)
    desc, tof = got["desc"].view(DESC_DTYPE), got["to_frames"].view(B.FANOUT_SUB_DTYPE)
    status, nonces = got["status"].view(np.uint16), got["nonces"].view(np.uint64)
    first = 0
    for s, (o, e) in enumerate(zip(offs, exps)):
        if (int(scan[s]["first"]), int(scan[s]["nframes"]), int(scan[s]["consumed"]), int(scan[s]["rc"])) != \
                (first, len(e.frames), e.consumed, e.rc):
            bad.append(f"stream {s}: scan {scan[s]}, model first {first}, {len(e.frames)} frames, {e.consumed}, rc {e.rc}")
            first += len(e.frames)
            continue
        c = cut[s]
        if (int(c["ok_bytes"]), int(c["whole_bytes"]), int(c["peer_nonce"]), int(c["ok_frames"]), int(c["fail_status"]),
                int(c["reserved"])) != (e.ok_bytes, e.whole_bytes, e.peer_nonce, e.ok_frames, e.fail_status, 0):
            bad.append(f"stream {s}: cut {c}, model {e.ok_bytes} {e.whole_bytes} {e.peer_nonce:#x} {e.ok_frames} {e.fail_status}")
        for k, (_h, boff, size) in enumerate(e.frames):
            j, where = first + k, f"stream {s} frame {k}"
            d = desc[j]
            if (int(d["in_off"]), int(d["out_off"]), int(d["len"]), int(d["key_idx"]), int(d["counter"]), int(d["flags"]),
                    int(d["prev"])) != (o + boff, o + boff, size, int(got["st"][s]["key_idx"]), e.floors[k], g.L.CZ_DESC_CHECK_NONCE, -1):
                bad.append(f"{where}: descriptor {d}, floor {e.floors[k]:#x}")
            if (int(tof[j]["counter"]), int(tof[j]["key_idx"]), int(tof[j]["reserved"])) != \
                    ((int(got["to"][s]["counter"]) + k) & rx.M64, int(got["to"][s]["key_idx"]), 0):
                bad.append(f"{where}: outbound record {tof[j]}")
            if int(status[j]) != e.status[k]:
                bad.append(f"{where}: status {int(status[j]):#x}, model {e.status[k]:#x}")
            if e.nonces[k] is not None and int(nonces[j]) != e.nonces[k]:
                bad.append(f"{where}: nonce {int(nonces[j]):#x}, model {e.nonces[k]:#x}")
        first += len(e.frames)
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("in_place", [True, False], ids=["in_place", "out_of_place"])
def test_relay_streams_against_the_model(gpu, n, in_place):
    _streams, offs, host, exps, inplace, outplace = build(n)
    got = _run(gpu, n, in_place)
    _check(gpu, n, got, exps, offs, inplace if in_place else outplace)
    if not in_place:
        assert got["wire"].tobytes() == host.tobytes(), "the input of an out-of-place call changed"


def test_equals_relay_batch_on_parsed_descriptors_with_prev_chains(gpu):
    """the host route: wire.parse per stream, descriptors chained by prev, batch.relay_batch out of place --
    bodies, status and nonces are those of relay_streams, the short bodies' floors (read across the body's end)
    included"""
    g, n = gpu, 65
    streams, offs, host, exps, _inplace, outplace = build(n)
    got = _run(g, n, False)
    rows = []
    for s, (o, (w, floor, _rc)) in enumerate(zip(offs, streams)):
        frames, _consumed, _prc = g.wire.parse(w)
        for k, f in enumerate(frames):
            rows.append((o + int(f["body_off"]), o + int(f["body_off"]), int(f["size"]), KIN, floor,
                         g.L.CZ_DESC_CHECK_NONCE, len(rows) - 1 if k else -1))
    d = np.array(rows, dtype=DESC_DTYPE)
    assert len(d) == got["N"]
    tof = got["to_frames"].view(g.batch.FANOUT_SUB_DTYPE)[:len(d)].copy()
    t = g.torch
    d_in = t.from_numpy(host.copy()).to(g.dev)
    d_out = t.full((len(host),), OTHER, dtype=t.uint8, device=g.dev)
    status = t.full((len(d),), -1, dtype=t.int16, device=g.dev)
    nonces = t.full((len(d),), -1, dtype=t.int64, device=g.dev)
    g.batch.relay_batch(g.wire.to_device(d, g.dev), g.wire.to_device(tof, g.dev), len(d), d_in, d_out, g.subkeys, status,
                        nonces=nonces, desc_np=d, to_np=tof)
    t.cuda.synchronize()
    out = d_out.cpu().numpy()
    for r in d:                     # relay_batch writes bodies only
        a, b = int(r["out_off"]), int(r["out_off"]) + int(r["len"])
        assert out[a:b].tobytes() == got["out"][a:b].tobytes() == outplace[a:b].tobytes()
    assert status.cpu().numpy().view(np.uint16).tolist() == got["status"].view(np.uint16)[:len(d)].tolist()
    assert nonces.cpu().numpy().view(np.uint64).tolist() == got["nonces"].view(np.uint64)[:len(d)].tolist()


def test_equal_keys_and_counters_give_the_received_bytes(gpu):
    """inbound and outbound key equal and the outbound counter equal to the first inbound nonce: a stream whose
    nonces rise by one and whose flags bytes hold only MORE leaves exactly as it came"""
    g, t = gpu, gpu.torch
    bodies = [or_curve_encode(splitmix_bytes(sz - 33, 77 + k), k & 1, 500 + k, 0, rx.PRECOM)
              for k, sz in enumerate((33, 97, 256, 98))]
    w = b"".join(v2_encode(b, k & 1) for k, b in enumerate(bodies))
    host = np.full(3 + len(w) + 32, SENT, dtype=np.uint8)
    host[3:3 + len(w)] = np.frombuffer(w, dtype=np.uint8)
    st = np.zeros(1, dtype=g.wire.V2_STREAM_DTYPE)
    st["off"], st["len"], st["floor"], st["key_idx"] = 3, len(w), 499, 0
    to = np.zeros(1, dtype=g.batch.FANOUT_SUB_DTYPE)
    to["counter"], to["key_idx"] = 500, 0
    d_wire = t.from_numpy(host.copy()).to(g.dev)
    z = lambda nbytes: t.zeros(nbytes, dtype=t.uint8, device=g.dev)     # noqa: E731
    results = z(32)
    rc, nframes = g.batch.relay_streams(g.wire.to_device(st, g.dev), g.wire.to_device(to, g.dev), d_wire, d_wire, z(32),
                                        z(4 * 40), z(4 * 16), g.subkeys, z(8).view(t.int16), z(32).view(t.int64), results)
    t.cuda.synchronize()
    assert (rc, nframes) == (0, 4)
    assert d_wire.cpu().numpy().tobytes() == host.tobytes()
    c = results.cpu().numpy().view(g.batch.RELAY_STREAM_RESULT_DTYPE)[0]
    assert (int(c["ok_bytes"]), int(c["whole_bytes"]), int(c["peer_nonce"]), int(c["ok_frames"]), int(c["fail_status"])) == \
        (len(w), len(w) - 2 - 98, 503, 4, 0)


@pytest.mark.parametrize("in_place", [True, False], ids=["in_place", "out_of_place"])
def test_enomem_fills_the_totals_and_writes_nothing(gpu, in_place):
    n = 65
    _streams, _offs, host, _exps, _inplace, _outplace = build(n)
    N = _run(gpu, n, in_place)["N"]
    got = _run(gpu, n, in_place, desc_cap=N - 1)
    assert got["rc"] == gpu.L.CZ_ENOMEM and got["nframes"] == N
    assert got["wire"].tobytes() == host.tobytes()
    if not in_place:
        assert got["out"].tobytes() == bytes([OTHER]) * len(host)
    for name in ("desc", "to_frames", "results"):
        assert got[name].tobytes() == bytes([SENT]) * got[name].size, name
    assert np.all(got["status"] == -1) and np.all(got["nonces"] == -1)
