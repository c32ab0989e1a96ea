"""GPU: the scanned flush_in (cz_tune "scan_in") against the unscanned one and the model.

Two engines receive the same wire, one flushed with scan_in = 65536 and one with 0, in both roles, 70
connections.  After every flush they must agree with each other and with rx_model.stream_model on the delivered
messages, cnPeerNonce, error and event of every connection; the scanned engine reports every whole frame of the
flush as scanned, the other none."""
import pytest

import rx_model as rx
from cz_testlib import v2_encode

pytestmark = pytest.mark.gpu

NCONN = 70
SCAN = 65536
PAYLOADS = (0, 100, 300, 4096)


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from jeromq_amd import _lib
    return _lib


def _frames(c, count, first_nonce=3, sizes=PAYLOADS):
    """connection c's frames: payload sizes rotate through `sizes`, starting somewhere else on each connection"""
    return [rx.Frame(first_nonce + 2 * i, sizes[(c + i) % len(sizes)] + 33, None, (c + i) & 3, 100000 + 100 * c + i)
            for i in range(count)]


def _wire(frames, role):
    return [v2_encode(rx.build_body(f, role)) for f in frames]


def _run(L, role, conns, expect_taken=True, scan=SCAN):
    """conns: [(name, cn_peer_nonce, [wire bytes of flush 0, flush 1, ...])]"""
    from jeromq_amd import wire as W
    from jeromq_amd.engine import CurveBatchEngine
    lib = L.lib()
    engs = [CurveBatchEngine(arena_bytes=1 << 20), CurveBatchEngine(arena_bytes=1 << 20)]
    old = lib.cz_tune(b"scan_in", 0)
    bad = []
    try:
        ids = [[e.add_connection(rx.PRECOM, as_server=role == rx.SERVER, cn_peer_nonce=floor) for _, floor, _ in conns]
               for e in engs]
        assert ids[0] == ids[1]
        ids = ids[0]
        models = [rx.stream_model(role, floor, [(p, True) for p in pieces]) for _, floor, pieces in conns]
        pending = [b""] * len(conns)
        for k in range(len(conns[0][2])):
            whole = receiving = 0
            for j, (name, _floor, pieces) in enumerate(conns):
                before = models[j][k - 1] if k else None
                want_rc = before["error"][0] if before and before["refused"] else 0
                for e in engs:
                    rc = e.recv(ids[j], pieces[k])
                    if rc != want_rc:
                        bad.append(f"{name} flush {k}: recv returned {rc}, model {want_rc}")
                if want_rc == 0:
                    buf = pending[j] + pieces[k]
                    frames, consumed, _rc = W.parse(buf)
                    whole += len(frames)
                    receiving += 1 if buf else 0
                    pending[j] = buf[consumed:]
            if expect_taken:
                assert receiving >= 64
            lib.cz_tune(b"scan_in", scan)
            engs[0].flush_in()
            lib.cz_tune(b"scan_in", 0)
            engs[1].flush_in()
            if engs[0].scan_frames != (whole if expect_taken else 0):
                bad.append(f"flush {k}: scan_frames {engs[0].scan_frames}, whole frames {whole}, taken {expect_taken}")
            if engs[1].scan_frames != 0:
                bad.append(f"flush {k}: the unscanned engine reports {engs[1].scan_frames} scanned frames")
            for j, (name, _floor, _pieces) in enumerate(conns):
                m = models[j][k]
                want = (m["delivered"], m["error"], m["peer_nonce"])
                got = [(e.messages_in(ids[j]), e.error(ids[j]), e.peer_nonce(ids[j])) for e in engs]
                for what, g in zip(("scanned", "unscanned"), got):
                    if g != want:
                        bad.append(f"{what} {name} flush {k}: delivered {len(g[0])} (a prefix of the model's: "
                                   f"{g[0] == want[0][:len(g[0])]}), error {g[1]}, peer_nonce {g[2]:#x}; model "
                                   f"{len(want[0])}, {want[1]}, {want[2]:#x}")
    finally:
        lib.cz_tune(b"scan_in", old)
        for e in engs:
            e.close()
    return bad


@pytest.mark.parametrize("role", rx.ROLES)
def test_mixed_sizes(gpu, role):
    conns = [(f"connection {c}", 2, [b"".join(_wire(_frames(c, 4 + c % 3), role))]) for c in range(NCONN)]
    bad = _run(gpu, role, conns)
    assert not bad, "\n".join(bad[:20])


def _cut_points(frames_wire):
    """inside the first short header, inside the first LARGE header and inside a body"""
    starts, at = [], 0
    for w in frames_wire:
        starts.append(at)
        at += len(w)
    short = next(s for s, w in zip(starts, frames_wire) if not w[0] & 2)
    large = next(s for s, w in zip(starts, frames_wire) if w[0] & 2)
    body = next(s for s, w in zip(starts, frames_wire) if len(w) > 100)
    return [short + 1, large + 4, body + 60], at


@pytest.mark.parametrize("role", rx.ROLES)
@pytest.mark.parametrize("flushes", [2, 3])
def test_wire_fed_in_pieces(gpu, role, flushes):
    """a partial frame waits in the receive buffer: the next flush's stream starts with it"""
    conns = []
    for c in range(NCONN):
        fw = _wire(_frames(c, 6), role)
        cuts, total = _cut_points(fw)
        whole = b"".join(fw)
        if flushes == 2:
            a = cuts[c % 3]
            pieces = [whole[:a], whole[a:]]
        else:
            a, b = sorted({cuts[c % 3], cuts[(c + 1) % 3]})
            pieces = [whole[:a], whole[a:b], whole[b:]]
        assert all(pieces) and sum(map(len, pieces)) == total
        conns.append((f"connection {c} cut {c % 3}", 2, pieces))
    bad = _run(gpu, role, conns)
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("role", rx.ROLES)
def test_failures_while_the_others_carry_on(gpu, role):
    """a bad tag, a replay and a LARGE size 0, each on one connection behind good frames; in the second flush
    the failed connections receive again (refused) and the others carry on"""
    conns = []
    for c in range(NCONN):
        fr = _frames(c, 8)
        if c == 5:
            fr[2] = fr[2]._replace(fault="tag")
        elif c == 17:
            fr[3] = fr[3]._replace(nonce=fr[2].nonce, fault="replay")
        fw = _wire(fr, role)
        if c == 40:
            fw[2:2] = [bytes([2]) + bytes(8)]
        conns.append((f"connection {c}", 2, [b"".join(fw[:5]), b"".join(fw[5:])]))
    for c, (n, err) in ((5, (2, (rx.CZ_EPROTO, rx.EV_CRYPTOGRAPHIC))),
                        (17, (3, (rx.CZ_EPROTO, rx.EV_INVALID_SEQUENCE if role == rx.SERVER else rx.EV_CRYPTOGRAPHIC))),
                        (40, (2, (rx.CZ_EPROTO, 0)))):
        m = rx.stream_model(role, 2, [(p, True) for p in conns[c][2]])
        assert (len(m[0]["delivered"]), m[0]["error"]) == (n, err) and m[1]["delivered"] == []
    bad = _run(gpu, role, conns)
    assert not bad, "\n".join(bad[:20])


def test_63_connections_are_not_taken(gpu):
    role = rx.SERVER
    conns = [(f"connection {c}", 2, [b"".join(_wire(_frames(c, 3), role))]) for c in range(63)]
    bad = _run(gpu, role, conns, expect_taken=False)
    assert not bad, "\n".join(bad[:20])


def test_one_connection_over_the_byte_bound_is_not_taken(gpu):
    role = rx.CLIENT
    conns = [(f"connection {c}", 2, [b"".join(_wire(_frames(c, 17 if c == 7 else 3, sizes=PAYLOADS[3 if c == 7 else 0:]), role))])
             for c in range(NCONN)]
    assert len(conns[7][2][0]) > SCAN and all(len(p[0]) < SCAN for i, (_, _, p) in enumerate(conns) if i != 7)
    bad = _run(gpu, role, conns, expect_taken=False)
    assert not bad, "\n".join(bad[:20])


def test_the_byte_bound_is_inclusive(gpu):
    """a connection holding exactly scan_in bytes is taken, one byte more is not"""
    role = rx.CLIENT
    conns = [(f"connection {c}", 2, [b"".join(_wire(_frames(c, 3), role))]) for c in range(NCONN)]
    longest = max(len(p[0]) for _, _, p in conns)
    assert longest < SCAN
    bad = _run(gpu, role, conns, expect_taken=False, scan=longest - 1)
    bad += _run(gpu, role, conns, expect_taken=True, scan=longest)
    assert not bad, "\n".join(bad[:20])
