"""GPU: cz_engine_flush_in routed through the fan-in open (cz_tune "fanin_short") against rx_model.

The same wire goes through an engine with fanin_short at 4096 and through one at 0 (the segment plan alone).  In
both, every connection's delivered payloads and flags, cnPeerNonce, error and event after every flush are those
of rx_model.stream_model (V2Decoder and the mechanism's receive rule, payload truth from the CPU oracle);
fanin_frames is what the routing rule, restated here, gives for the flush's frame sizes on the routed engine, and
0 on the other."""
import pytest

import rx_model as rx
from cz_testlib import v2_encode

pytestmark = pytest.mark.gpu

NCONN = 130


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from jeromq_amd import _lib
    return _lib.lib()


def routed_frames(sizes, short):
    """the rule of cz_engine_flush_in for one flush group: maximal runs of consecutive equal body sizes, in
    connection order; a run of at least 64 frames of at least 33 bytes with a payload of at most `short` is routed"""
    total, i = 0, 0
    while short and i < len(sizes):
        j = i
        while j < len(sizes) and sizes[j] == sizes[i]:
            j += 1
        if j - i >= 64 and sizes[i] >= 33 and sizes[i] - 33 <= short:
            total += j - i
        i = j
    return total


class Conn:
    """one connection: its frames (rx_model.Frame) and the byte offsets at which its wire is cut into flushes"""

    def __init__(self, name, floor, frames, cuts=()):
        self.name, self.floor, self.frames, self.cuts = name, floor, list(frames), tuple(cuts)

    def pieces(self, role, nflush):
        bodies = [rx.build_body(f, role) for f in self.frames]
        wire = b"".join(v2_encode(b) for b in bodies)
        edges = [0] + list(self.cuts) + [len(wire)] * (nflush - len(self.cuts))
        starts, o = [], 0
        for b in bodies:
            o += len(v2_encode(b))
            starts.append(o)                       # a frame is whole once the wire reaches its end
        per_flush = [[len(b) for b, end in zip(bodies, starts) if edges[k] < end <= edges[k + 1]] for k in range(nflush)]
        return [wire[edges[k]:edges[k + 1]] for k in range(nflush)], per_flush


def run_engines(lib, role, conns, nflush=1):
    """Both engines over the same wire.  Returns (disagreements with the model, fanin_frames of the routed engine
    per flush, the rule's count per flush)."""
    from jeromq_amd.engine import CurveBatchEngine
    built = [c.pieces(role, nflush) for c in conns]
    models = [rx.stream_model(role, c.floor, [(p, True) for p in b[0]]) for c, b in zip(conns, built)]
    bad, seen, want_routed = [], [], []
    old = lib.cz_tune(b"fanin_short", 0)
    try:
        for short in (4096, 0):
            lib.cz_tune(b"fanin_short", short)
            eng = CurveBatchEngine(arena_bytes=1 << 20)
            ids = [eng.add_connection(rx.PRECOM, as_server=role == rx.SERVER, cn_peer_nonce=c.floor) for c in conns]
            for k in range(nflush):
                sizes = []
                for j, c in enumerate(conns):
                    before = models[j][k - 1] if k else None
                    refused = bool(before and before["refused"])
                    rc = eng.recv(ids[j], built[j][0][k])
                    if rc != (before["error"][0] if refused else 0):
                        bad.append(f"fanin_short {short}: {c.name} flush {k}: recv returned {rc}")
                    if not refused:
                        # (frames behind a carried partial frame complete in this flush: the model's count says so)
                        sizes += built[j][1][k]
                eng.flush_in()
                if short:
                    seen.append(eng.fanin_frames)
                    want_routed.append(routed_frames(sizes, short))
                elif eng.fanin_frames:
                    bad.append(f"fanin_short 0: flush {k} routed {eng.fanin_frames} frames")
                for j, c in enumerate(conns):
                    m = models[j][k]
                    got = (eng.messages_in(ids[j]), eng.error(ids[j]), eng.peer_nonce(ids[j]))
                    want = (m["delivered"], m["error"], m["peer_nonce"])
                    if got != want:
                        bad.append(f"fanin_short {short}: {c.name} flush {k}: delivered {len(got[0])} (a prefix of the "
                                   f"model's: {got[0] == want[0][:len(got[0])]}), error {got[1]}, peer_nonce {got[2]:#x}; "
                                   f"model {len(want[0])}, {want[1]}, {want[2]:#x}")
            eng.close()
    finally:
        lib.cz_tune(b"fanin_short", old)
    return bad, seen, want_routed


def chain(j, count, size, floor=2):
    return rx._chain(floor, count, 3000 + 7 * j, size_of=lambda i: size)


@pytest.mark.parametrize("role", rx.ROLES)
@pytest.mark.parametrize("payload", [100, 0, 256])
def test_routing_on_and_off(gpu, role, payload):
    conns = [Conn(f"conn {j}", 2 + j, chain(j, 1 + j % 5, payload + 33, floor=2 + j)) for j in range(NCONN)]
    bad, seen, want = run_engines(gpu, role, conns)
    assert not bad, "\n".join(bad[:20])
    assert seen == want == [sum(1 + j % 5 for j in range(NCONN))]


@pytest.mark.parametrize("role", rx.ROLES)
def test_runs_broken_by_other_sizes(gpu, role):
    """connection 40's middle frame has another size: the run is split around a frame that stays in the segment
    plan, whose prev chain resolves to a routed frame and which is the floor of the routed frame after it;
    connection 100's middle frame is the 300 033-byte body the segment plan splits; connection 101's second frame
    replays that of a neighbour size"""
    conns = []
    for j in range(NCONN):
        fr = chain(j, 3, 133)
        if j == 40:
            fr[1] = fr[1]._replace(size=161)
        if j == 100:
            fr[1] = fr[1]._replace(size=rx.BIG)
        if j == 101:
            fr[1] = fr[1]._replace(size=97)
            rx._set_fault(fr, 2, 2, "replay")          # the routed frame behind it replays the unrouted one's nonce
        conns.append(Conn(f"conn {j}", 2, fr))
    bad, seen, want = run_engines(gpu, role, conns)
    assert not bad, "\n".join(bad[:20])
    # (the two 133-byte frames between the bodies of connections 100 and 101 are a run of 2: they stay)
    assert seen == want and want[0] == (40 * 3 + 1) + (1 + 59 * 3 + 1) + (1 + 28 * 3)


@pytest.mark.parametrize("role", rx.ROLES)
def test_failures_inside_a_routed_run(gpu, role):
    conns = []
    for j in range(NCONN):
        fr = chain(j, 4, 133)
        kind, at = {5: ("replay", 0), 64: ("replay", 1), 70: ("tag", 2), 71: ("ct_last", 3), 90: ("name3", 1), 91: ("name7", 1),
                    92: ("flags_ff", 0), 93: ("replay_tag", 2), 129: ("wrong_dir", 3), 0: ("tag", 0)}.get(j, (None, 0))
        if kind:
            rx._set_fault(fr, 2, at, kind)
        conns.append(Conn(f"conn {j} {kind}@{at}", 2, fr))
    bad, seen, want = run_engines(gpu, role, conns)
    assert not bad, "\n".join(bad[:20])
    assert seen == want == [NCONN * 4]


@pytest.mark.parametrize("role", rx.ROLES)
def test_two_flushes(gpu, role):
    """every chain is cut between two flushes -- at a frame edge, or inside a frame that is then carried over -- so
    the second flush's first frame of a connection checks against the cnPeerNonce the first flush left; one
    connection fails in the first flush and refuses the second's bytes"""
    frame = len(v2_encode(bytes(133)))
    conns = []
    for j in range(NCONN):
        fr = chain(j, 4, 133)
        if j == 9:
            rx._set_fault(fr, 2, 1, "tag")
        if j == 10:
            rx._set_fault(fr, 2, 2, "replay")          # frame 0 of the second flush replays the first flush's last
        cut = 2 * frame + (0, 0, 1, 60, frame - 1)[j % 5]
        conns.append(Conn(f"conn {j} cut at {cut}", 2, fr, cuts=(cut,)))
    bad, seen, want = run_engines(gpu, role, conns, nflush=2)
    assert not bad, "\n".join(bad[:20])
    assert seen == want and seen[0] == 2 * NCONN and seen[1] > 64


def test_fewer_than_64_equal_frames(gpu):
    conns = [Conn(f"conn {j}", 2, chain(j, 3, 133)) for j in range(21)]          # 63 frames
    bad, seen, want = run_engines(gpu, rx.SERVER, conns)
    assert not bad, "\n".join(bad[:20])
    assert seen == want == [0]
    # ... and 64 frames of which one has another size
    conns = [Conn(f"conn {j}", 2, chain(j, 2, 133)) for j in range(32)]
    conns[20].frames[0] = conns[20].frames[0]._replace(size=134)
    bad, seen, want = run_engines(gpu, rx.SERVER, conns)
    assert not bad, "\n".join(bad[:20])
    assert seen == want == [0]
