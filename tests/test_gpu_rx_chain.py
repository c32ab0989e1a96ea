"""GPU: the receive nonce chain of every receiver against the one model of tests/rx_model.py.

Receivers: cz_open_batch (k_open_desc, in order and through d_order), cz_open_segments (open_header,
k_open_combine), cz_open_uniform in three body layouts (both floor loads, the phase-sorted carry kernel
and the tail behind it), CurveClientMechanism / CurveServerMechanism (decode frame by frame: open_one;
decodeBatch: decode_batch) and CurveBatchEngine in both roles (flush_in: one flush, two flushes, many
connections, the 4096-frame parse chunk, the pipelined 16-group flush).  Every scenario of the table
runs through every receiver that can take it (cz_open_uniform takes the uniform-size chains only),
bit-exact against the model: statuses, flags, nonces, payloads, events, cnPeerNonce, and what lies
around the outputs.  Wire frames of 0, 7, 8, 16 and 32 bytes are the table's cut bodies."""
import numpy as np
import pytest

import rx_model as rx
from cz_testlib import DESC_DTYPE, v2_encode

pytestmark = pytest.mark.gpu

SENT = 0xA5      # what every output buffer holds before a call
GUARD = 64       # bytes between two outputs of a descriptor batch
PAD = 256        # bytes before and after a uniform batch's buffers


class _Gpu:
    pass


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from jeromq_amd import _lib, batch
    g = _Gpu()
    g.torch, g.dev, g.L, g.batch = torch, torch.device("cuda:0"), _lib, batch
    k = torch.tensor(list(rx.PRECOM), dtype=torch.uint8, device=g.dev).view(1, 32)
    g.subkeys = torch.cat([batch.subkeys(k, _lib.CZ_DIR_C2S), batch.subkeys(k, _lib.CZ_DIR_S2C)])
    return g


def _r(n, a):
    return (n + a - 1) // a * a


def _dev(g, a):
    return g.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(g.dev)


# ---- raw, per frame: descriptors ------------------------------------------------------------------
def _desc_layout(sc, role):
    """bodies in 16-byte aligned slots, frame i chained to i - 1; outputs in 16-byte aligned slots with
    GUARD bytes of sentinel before, between and after them"""
    bodies = sc.bodies(role)[:sc.raw_count(role)]
    desc = np.zeros(len(bodies), dtype=DESC_DTYPE)
    io, oo = 0, GUARD
    for i, b in enumerate(bodies):
        desc[i] = (io, oo, len(b), rx.from_server(role), sc.floor, 0x100, i - 1)
        io += _r(max(len(b), 1), 16)
        oo += _r(max(len(b) - 33, 0), 16) + GUARD
    hin = np.zeros(io + 64, dtype=np.uint8)
    for i, b in enumerate(bodies):
        hin[int(desc[i]["in_off"]):int(desc[i]["in_off"]) + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return desc, hin, oo


def _check_raw(sc, role, what, desc, st, out, nn, bad):
    exp = sc.raw_expect(role)
    bodies = sc.bodies(role)
    if out[:GUARD].tobytes() != bytes([SENT]) * GUARD:
        bad.append(f"{what} {sc.name}: bytes before the first output changed")
    for i, (est, efl, epay, enonce) in enumerate(exp):
        o, plen = int(desc[i]["out_off"]), max(len(bodies[i]) - 33, 0)
        region = out[o:o + plen]
        where = f"{what} {sc.name} frame {i}"
        if (st[i] & 0xff) != est:
            bad.append(f"{where}: status {st[i] & 0xff}, model {est}")
            continue
        if est == rx.ST_OK:
            if st[i] >> 8 != efl:
                bad.append(f"{where}: flags byte {st[i] >> 8:#x}, model {efl:#x}")
            if region.tobytes() != epay:
                bad.append(f"{where}: payload differs")
        else:
            if st[i] >> 8:
                bad.append(f"{where}: a rejected frame's status carries {st[i] >> 8:#x}")
            # zero after a bad tag; zero or untouched where the header promises nothing
            ok = not region.any() if est == rx.ST_CRYPTO else bool(np.all((region == 0) | (region == SENT)))
            if not ok:
                bad.append(f"{where}: a rejected frame's output holds other bytes than zero / the sentinel")
        if nn is not None and enonce is not None and int(nn[i]) != enonce:
            bad.append(f"{where}: nonce {int(nn[i]):#x}, model {enonce:#x}")
        nxt = int(desc[i + 1]["out_off"]) if i + 1 < len(exp) else len(out)
        if out[o + _r(plen, 16):nxt].tobytes() != bytes([SENT]) * (nxt - o - _r(plen, 16)):
            bad.append(f"{where}: bytes behind the output slot changed")


@pytest.mark.parametrize("role", rx.ROLES)
@pytest.mark.parametrize("order", ["in_order", "reversed"])
def test_open_batch(gpu, role, order):
    g, bad = gpu, []
    for sc in rx.scenarios():
        desc, hin, ob = _desc_layout(sc, role)
        n = len(desc)
        d_out = g.torch.full((ob,), SENT, dtype=g.torch.uint8, device=g.dev)
        status = g.torch.full((n,), -1, dtype=g.torch.int16, device=g.dev)
        nonces = g.torch.zeros(n, dtype=g.torch.int64, device=g.dev)
        d_order = _dev(g, np.arange(n - 1, -1, -1, dtype=np.uint32)).view(g.torch.int32) if order == "reversed" else None
        g.batch.open_batch(_dev(g, desc), n, _dev(g, hin), d_out, g.subkeys, status, nonces=nonces, order=d_order,
                           desc_np=desc)
        g.torch.cuda.synchronize()
        _check_raw(sc, role, "open_batch", desc, status.cpu().numpy().view(np.uint16), d_out.cpu().numpy(),
                   nonces.cpu().numpy().view(np.uint64), bad)
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("role", rx.ROLES)
def test_open_segments(gpu, role):
    """seg_blocks = 2: every body over 192 bytes is split, the 300 033-byte one into 2344 segments; a
    split frame rejected early leaves its status to the first segment, one rejected by its tag to the
    combine, and its successor reads its floor from it"""
    g, bad = gpu, []
    for sc in rx.scenarios():
        desc, hin, ob = _desc_layout(sc, role)
        n = len(desc)
        plan = g.batch.SegmentPlan(desc, open_=True, seg_blocks=2).to(g.dev)
        if any(len(b) > 192 for b in sc.bodies(role)[:n]):
            assert plan.ncomb > 0, sc.name
        d_out = g.torch.full((ob,), SENT, dtype=g.torch.uint8, device=g.dev)
        status = g.torch.full((n,), -1, dtype=g.torch.int16, device=g.dev)
        nonces = g.torch.zeros(n, dtype=g.torch.int64, device=g.dev)
        g.batch.open_segments(_dev(g, desc), plan, _dev(g, hin), d_out, g.subkeys, status, nonces=nonces, desc_np=desc)
        g.torch.cuda.synchronize()
        _check_raw(sc, role, "open_segments", desc, status.cpu().numpy().view(np.uint16), d_out.cpu().numpy(),
                   nonces.cpu().numpy().view(np.uint64), bad)
    assert not bad, "\n".join(bad[:20])


# ---- raw, per frame: uniform batches ----------------------------------------------------------------
def _in_stride(layout, size):
    if layout == "aligned16":
        return _r(size, 16)
    if layout == "dense":          # bodies back to back: any byte offset
        return size
    s = _r(size, 8)                # 8-byte aligned and not 16: the 8-byte floor load, the carry kernel
    return s if s % 16 == 8 else s + 8


@pytest.mark.parametrize("role", rx.ROLES)
@pytest.mark.parametrize("layout", ["aligned16", "dense", "stride8"])
def test_open_uniform(gpu, role, layout):
    g, bad = gpu, []
    lib = g.L.lib()
    old = lib.cz_tune(b"open_carry", 1)      # the phase-sorted carry kernel on for 8-byte strides
    try:
        for sc in rx.scenarios():
            if not sc.uniform:
                continue
            size, count, bodies, exp = sc.uniform, len(sc.frames), sc.bodies(role), sc.raw_expect(role)
            nout = size - 33
            ist, ost = _in_stride(layout, size), _r(nout, 128)     # the batch owns whole 128-byte slots
            hin = np.zeros(PAD + count * ist + PAD, dtype=np.uint8)
            for i, b in enumerate(bodies):
                assert len(b) == size
                hin[PAD + i * ist:PAD + i * ist + size] = np.frombuffer(b, dtype=np.uint8)
            d_in = _dev(g, hin)
            d_out = g.torch.full((PAD + count * ost + PAD,), SENT, dtype=g.torch.uint8, device=g.dev)
            status = g.torch.full((count,), -1, dtype=g.torch.int16, device=g.dev)
            g.batch.open_uniform(d_in[PAD:PAD + count * ist], ist, d_out[PAD:PAD + count * ost], ost, count, size,
                                 g.subkeys[rx.from_server(role)], sc.floor, status, check=True)
            g.torch.cuda.synchronize()
            st, out = status.cpu().numpy().view(np.uint16), d_out.cpu().numpy()
            if out[:PAD].tobytes() != bytes([SENT]) * PAD or out[-PAD:].tobytes() != bytes([SENT]) * PAD:
                bad.append(f"{layout} {sc.name}: bytes around the batch's output changed")
            slots = out[PAD:PAD + count * ost].reshape(count, ost)
            for i, (est, efl, epay, _n) in enumerate(exp):
                where = f"{layout} {sc.name} frame {i}"
                if (st[i] & 0xff) != est:
                    bad.append(f"{where}: status {st[i] & 0xff}, model {est}")
                elif est == rx.ST_OK:
                    if st[i] >> 8 != efl:
                        bad.append(f"{where}: flags byte {st[i] >> 8:#x}, model {efl:#x}")
                    if slots[i, :nout].tobytes() != epay:
                        bad.append(f"{where}: payload differs")
                    if slots[i, nout:].any():
                        bad.append(f"{where}: slot bytes past the payload are not zero")
                elif st[i] >> 8 or slots[i].any():
                    bad.append(f"{where}: a rejected frame's slot is not zero (status {st[i]:#x})")
    finally:
        lib.cz_tune(b"open_carry", old)
    assert not bad, "\n".join(bad[:20])


# ---- the mechanisms ---------------------------------------------------------------------------------
@pytest.mark.parametrize("role", rx.ROLES)
def test_mechanism_decode_and_decode_batch(gpu, role):
    """decode frame by frame (one launch per body: open_one's host header checks) and decodeBatch (one
    segmented launch) on fresh mechanisms: the same delivered prefix, cnPeerNonce and event as the model,
    and as each other"""
    from jeromq_amd.mechanism import CurveClientMechanism, CurveServerMechanism, Msg
    cls = CurveServerMechanism if role == rx.SERVER else CurveClientMechanism
    bad = []
    for sc in rx.scenarios():
        e, bodies = sc.expect(role), sc.bodies(role)
        want = (e.delivered, e.peer_nonce, e.event)
        one, many = cls(rx.PRECOM, cn_peer_nonce=sc.floor), cls(rx.PRECOM, cn_peer_nonce=sc.floor)
        got1 = []
        for b in bodies:
            m = one.decode(Msg(b))
            if m is None:              # the engine tears the connection down here
                break
            got1.append((m.data, m.flags))
        got2 = [(m.data, m.flags) for m in many.decodeBatch([Msg(b) for b in bodies])]
        r1, r2 = (got1, one.cnPeerNonce, one.last_event), (got2, many.cnPeerNonce, many.last_event)
        one.close()
        many.close()
        for what, r in (("decode", r1), ("decodeBatch", r2)):
            if r != want:
                bad.append(f"{what} {sc.name}: delivered {len(r[0])} (same bytes: {r[0] == want[0]}), cnPeerNonce "
                           f"{r[1]:#x}, event {r[2]:#x}; model {len(want[0])}, {want[1]:#x}, {want[2]:#x}")
        if r1 != r2:
            bad.append(f"{sc.name}: decode and decodeBatch differ")
    assert not bad, "\n".join(bad[:20])


# ---- the engine ---------------------------------------------------------------------------------------
def _run_streams(g, role, conns, eng=None):
    """conns: [(name, cn_peer_nonce, [wire bytes of flush 0, flush 1, ...])], every list equally long.
    All connections live in one engine (eng: a shared one, which gets its connections removed again);
    after each flush every connection is compared with stream_model.  Returns the disagreements."""
    from jeromq_amd.engine import CurveBatchEngine
    own = eng is None
    if own:
        eng = CurveBatchEngine(arena_bytes=1 << 20)
    bad = []
    ids = [eng.add_connection(rx.PRECOM, as_server=role == rx.SERVER, cn_peer_nonce=floor) for _, floor, _ in conns]
    models = [rx.stream_model(role, floor, [(p, True) for p in pieces]) for _, floor, pieces in conns]
    for k in range(len(conns[0][2])):
        for j, (name, _floor, pieces) in enumerate(conns):
            before = models[j][k - 1] if k else None
            rc = eng.recv(ids[j], pieces[k])
            want_rc = before["error"][0] if before and before["refused"] else 0
            if rc != want_rc:
                bad.append(f"{name} flush {k}: recv returned {rc}, model {want_rc}")
        eng.flush_in()
        for j, (name, _floor, _pieces) in enumerate(conns):
            m = models[j][k]
            got = (eng.messages_in(ids[j]), eng.error(ids[j]), eng.peer_nonce(ids[j]))
            want = (m["delivered"], m["error"], m["peer_nonce"])
            if got != want:
                bad.append(f"{name} flush {k}: delivered {len(got[0])} (a prefix of the model's: "
                           f"{got[0] == want[0][:len(got[0])]}), error {got[1]}, peer_nonce {got[2]:#x}; model "
                           f"{len(want[0])}, {want[1]}, {want[2]:#x}")
    # a torn-down connection refuses further bytes, a healthy one takes them
    for j, (name, _floor, _pieces) in enumerate(conns):
        err = models[j][-1]["error"]
        rc = eng.recv(ids[j], b"\x00")
        if rc != err[0]:
            bad.append(f"{name}: recv after the last flush returned {rc}, error {err}")
    if own:
        eng.close()
    else:
        for c in ids:
            eng.remove_connection(c)
    return bad


def _clean_wire(role, seed, count=5):
    return b"".join(v2_encode(rx.build_body(f, role)) for f in rx._chain(2, count, seed))


@pytest.mark.parametrize("role", rx.ROLES)
def test_engine_one_flush_per_scenario(gpu, role):
    """each scenario alone in its flush, between two healthy neighbours"""
    from jeromq_amd.engine import CurveBatchEngine
    eng, bad = CurveBatchEngine(arena_bytes=1 << 20), []
    a, b = _clean_wire(role, 31), _clean_wire(role, 32)
    for sc in rx.scenarios():
        bad += _run_streams(gpu, role, [("neighbour a", 2, [a]), (sc.name, sc.floor, [sc.wire(role)]),
                                        ("neighbour b", 2, [b])], eng=eng)
    eng.close()
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("role", rx.ROLES)
def test_engine_all_scenarios_in_one_flush(gpu, role):
    """every scenario on its own connection, healthy connections first, last and in between: one flush"""
    conns = [("neighbour first", 2, [_clean_wire(role, 40)])]
    for i, sc in enumerate(rx.scenarios()):
        conns.append((sc.name, sc.floor, [sc.wire(role)]))
        if i % 10 == 9:
            conns.append((f"neighbour {i}", 2, [_clean_wire(role, 41 + i)]))
    conns.append(("neighbour last", 2, [_clean_wire(role, 39)]))
    bad = _run_streams(gpu, role, conns)
    assert not bad, "\n".join(bad[:20])


def _cuts(sc, role):
    """byte offsets that cut the scenario's wire at the frame boundaries around its first fault (or first
    rejected frame), and once inside that frame"""
    e = sc.expect(role)
    p = e.failed_at if e.failed_at is not None else (sc.faults() or [len(sc.frames) // 2])[0]
    starts = [0]
    for b in sc.bodies(role):
        starts.append(starts[-1] + len(v2_encode(b)))
    cuts = {starts[min(max(q, 0), len(sc.frames))] for q in (p - 1, p, p + 1, p + 2)}
    cuts.add(starts[p] + (starts[p + 1] - starts[p]) // 2)
    return sorted(cuts)


@pytest.mark.parametrize("role", rx.ROLES)
def test_engine_two_flushes_cut_around_the_fault(gpu, role):
    """the floor of a flush's first frame is c.peer_nonce: a replay, an equal nonce, a bad tag or a bad name
    as frame 0 of the second flush, a failure as the last frame of the first, and a partial frame kept"""
    conns = [("neighbour", 2, [_clean_wire(role, 50), b""])]
    for sc in rx.single_fault_scenarios():
        wire = sc.wire(role)
        for cut in _cuts(sc, role):
            conns.append((f"{sc.name} cut at {cut}", sc.floor, [wire[:cut], wire[cut:]]))
    bad = _run_streams(gpu, role, conns)
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("role", rx.ROLES)
def test_engine_v2_flags_and_headers(gpu, role):
    """V2Decoder gives a MESSAGE frame with the COMMAND bit to the mechanism like any other
    (StreamEngine.decodeAndPush), and takes a LARGE header for a body under 256 bytes; the decrypted
    flags alone count.  A crypto failure followed in the same flush by a LARGE header of size 0: the
    earlier event wins; the header alone is a framing error without an event."""
    from cz_testlib import V2DecoderModel
    good = [rx.build_body(f, role) for f in rx._chain(2, 4, 77)]
    bad_tag = rx.build_body(rx._chain(2, 4, 77)[2]._replace(fault="tag"), role)
    large0 = bytes([2]) + bytes(8)
    flagged = (v2_encode(good[0]) + bytes([4, len(good[1])]) + good[1] + bytes([5, len(good[2])]) + good[2] +
               bytes([2]) + len(good[3]).to_bytes(8, "big") + good[3])
    d = V2DecoderModel()
    d.feed(flagged)
    assert d.error is None and [(s, f) for _, s, f in d.msgs] == [(len(good[0]), 0), (len(good[1]), 2),
                                                                 (len(good[2]), 3), (len(good[3]), 0)]
    (m,) = rx.stream_model(role, 2, [(flagged, True)])
    assert [f for _, f in m["delivered"]] == [0, 1, 2, 3] and m["error"] == (0, 0)   # the sealed flags, not the wire's
    failing = v2_encode(good[0]) + v2_encode(good[1]) + v2_encode(bad_tag) + large0 + v2_encode(good[3])
    (m,) = rx.stream_model(role, 2, [(failing, True)])
    assert m["error"] == (rx.CZ_EPROTO, rx.EV_CRYPTOGRAPHIC) and len(m["delivered"]) == 2
    framing = v2_encode(good[0]) + large0 + v2_encode(good[1])
    (m,) = rx.stream_model(role, 2, [(framing, True)])
    assert m["error"] == (rx.CZ_EPROTO, 0) and len(m["delivered"]) == 1
    bad = _run_streams(gpu, role, [("neighbour", 2, [_clean_wire(role, 60)]), ("wire flags and LARGE", 2, [flagged]),
                                   ("bad tag then LARGE 0", 2, [failing]), ("LARGE 0", 2, [framing]),
                                   ("neighbour", 2, [_clean_wire(role, 61)])])
    assert not bad, "\n".join(bad)


@pytest.fixture(scope="module")
def long_chain():
    """8193 valid 34-byte bodies of one client, nonces 3..; shared, never changed"""
    frames = [rx.Frame(3 + i, 34, None, i & 3, 80000 + i) for i in range(8193)]
    return frames, [rx.build_body(f, rx.SERVER) for f in frames]


@pytest.mark.parametrize("count,replay_at", [(4095, None), (4096, None), (4097, None), (8193, None), (8193, 4095),
                                             (8193, 4096), (8193, 4097)])
def test_engine_parse_chunk_edge(gpu, long_chain, count, replay_at):
    """flush_in parses a connection 4096 frames at a time and re-bases the body offsets: a chain that
    ends on, before and behind the edge, and a replay on each side of it"""
    frames, bodies = long_chain
    bodies = list(bodies[:count])
    if replay_at is not None:
        bodies[replay_at] = rx.build_body(frames[replay_at]._replace(nonce=frames[replay_at - 1].nonce), rx.SERVER)
    wire = b"".join(v2_encode(b) for b in bodies)
    (m,) = rx.stream_model(rx.SERVER, 2, [(wire, True)])
    assert len(m["delivered"]) == (count if replay_at is None else replay_at)
    assert m["error"] == ((0, 0) if replay_at is None else (rx.CZ_EPROTO, rx.EV_INVALID_SEQUENCE))
    bad = _run_streams(gpu, rx.SERVER, [("neighbour", 2, [_clean_wire(rx.SERVER, 70)]),
                                        (f"{count} frames, replay at {replay_at}", 2, [wire]),
                                        ("neighbour", 2, [_clean_wire(rx.SERVER, 71)])])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("role", rx.ROLES)
def test_engine_pipelined_flush_with_failures(gpu, role):
    """Just over 64 MiB received on 32 connections: flush_in runs 16 groups on host threads with
    group-relative prev indices and per-group status / nonce offsets.  One failing frame in a
    connection of the first group (its first frame, bad tag), of a middle group (a middle frame, a
    split body with a bad name) and of the last group (its last frame, a replay); every other
    connection delivers everything.  Bodies from the oracle."""
    nconn, big = 32, 700033
    conns, total = [], 0
    for c in range(nconn):
        sizes = [34, big, 97, big, 161, big, 96]
        frames, n = [], 1000 * c + 2
        for i, size in enumerate(sizes):
            n += 1 + (i & 1)
            frames.append(rx.Frame(n, size, None, i & 3, 90000 + 10 * c + i))
        if c == 0:
            frames[0] = frames[0]._replace(fault="tag")
        elif c == nconn // 2:
            frames[3] = frames[3]._replace(fault="name3")
        elif c == nconn - 1:
            frames[-1] = frames[-1]._replace(nonce=frames[-2].nonce)
        wire = b"".join(v2_encode(rx.build_body(f, role)) for f in frames)
        total += len(wire)
        conns.append((f"connection {c}", 1000 * c + 2, [wire]))
    assert (64 << 20) <= total < (64 << 20) + (1 << 20)
    for c, want in ((0, 0), (nconn // 2, 3), (nconn - 1, 6)):
        (m,) = rx.stream_model(role, conns[c][1], [(conns[c][2][0], True)])
        assert len(m["delivered"]) == want and m["refused"]
    bad = _run_streams(gpu, role, conns)
    assert not bad, "\n".join(bad[:20])
