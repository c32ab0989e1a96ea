"""GPU: cz_engine_flush_in routed through the split fan-in open (cz_tune "fanin_split") against rx_model.

The same wire goes through an engine with fanin_split at 1000 and through one at 0 (the segment plan alone), with
fanin_short at 100 in both so that the short rule's precedence is exercised.  In both, every connection's delivered
payloads and flags, cnPeerNonce, error and event after every flush are those of rx_model.stream_model (V2Decoder and
the mechanism's receive rule, payload truth from the CPU oracle); fanin_split_frames and fanin_frames are what the
routing rules, restated here, give for the flush's frame sizes."""
import pytest

import rx_model as rx
from cz_testlib import v2_encode
from test_gpu_fanin_engine import Conn, chain, routed_frames

pytestmark = pytest.mark.gpu

NCONN = 70
SHORT, SPLIT = 100, 1000
BIG = 4129 + 64          # 4160-byte payloads: 66 blocks, split at flush_in's segment length 4


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from jeromq_amd import _lib
    return _lib.lib()


def split_frames(sizes, short, split):
    """the rule of cz_engine_flush_in for one flush group: maximal runs of consecutive equal body sizes; a run of
    at least 64 frames of at least 33 bytes that fanin_short does not take and whose payload is at least `split`"""
    total, i = 0, 0
    while split and i < len(sizes):
        j = i
        while j < len(sizes) and sizes[j] == sizes[i]:
            j += 1
        full = j - i >= 64 and sizes[i] >= 33
        if full and not (short and sizes[i] - 33 <= short) and sizes[i] - 33 >= split:
            total += j - i
        i = j
    return total


def run_engines(lib, role, conns, nflush=1, short=SHORT):
    """Both engines over the same wire.  Returns (disagreements with the model, (fanin_split_frames, fanin_frames)
    of the routed engine per flush, the rules' counts per flush)."""
    from jeromq_amd.engine import CurveBatchEngine
    built = [c.pieces(role, nflush) for c in conns]
    models = [rx.stream_model(role, c.floor, [(p, True) for p in b[0]]) for c, b in zip(conns, built)]
    bad, seen, want = [], [], []
    old_short, old_split = lib.cz_tune(b"fanin_short", short), lib.cz_tune(b"fanin_split", 0)
    try:
        for split in (SPLIT, 0):
            lib.cz_tune(b"fanin_split", split)
            eng = CurveBatchEngine(arena_bytes=1 << 20)
            ids = [eng.add_connection(rx.PRECOM, as_server=role == rx.SERVER, cn_peer_nonce=c.floor) for c in conns]
            for k in range(nflush):
                sizes = []
                for j, c in enumerate(conns):
                    before = models[j][k - 1] if k else None
                    refused = bool(before and before["refused"])
                    rc = eng.recv(ids[j], built[j][0][k])
                    if rc != (before["error"][0] if refused else 0):
                        bad.append(f"fanin_split {split}: {c.name} flush {k}: recv returned {rc}")
                    if not refused:
                        sizes += built[j][1][k]
                eng.flush_in()
                if split:
                    seen.append((eng.fanin_split_frames, eng.fanin_frames))
                    want.append((split_frames(sizes, short, split), routed_frames(sizes, short)))
                elif eng.fanin_split_frames:
                    bad.append(f"fanin_split 0: flush {k} routed {eng.fanin_split_frames} frames")
                for j, c in enumerate(conns):
                    m = models[j][k]
                    got = (eng.messages_in(ids[j]), eng.error(ids[j]), eng.peer_nonce(ids[j]))
                    wnt = (m["delivered"], m["error"], m["peer_nonce"])
                    if got != wnt:
                        bad.append(f"fanin_split {split}: {c.name} flush {k}: delivered {len(got[0])} (a prefix of the "
                                   f"model's: {got[0] == wnt[0][:len(got[0])]}), error {got[1]}, peer_nonce {got[2]:#x}; "
                                   f"model {len(wnt[0])}, {wnt[1]}, {wnt[2]:#x}")
            eng.close()
    finally:
        lib.cz_tune(b"fanin_short", old_short)
        lib.cz_tune(b"fanin_split", old_split)
    return bad, seen, want


@pytest.mark.parametrize("role", rx.ROLES)
def test_routing_on_and_off(gpu, role):
    conns = [Conn(f"conn {j}", 2 + j, chain(j, 1 + j % 3, BIG, floor=2 + j)) for j in range(NCONN)]
    bad, seen, want = run_engines(gpu, role, conns)
    assert not bad, "\n".join(bad[:20])
    assert seen == want == [(sum(1 + j % 3 for j in range(NCONN)), 0)]


@pytest.mark.parametrize("role", rx.ROLES)
def test_short_runs_keep_precedence_and_other_sizes_stay(gpu, role):
    """connections 0..34 send two 133-byte frames each (a run of 70 that fanin_short takes), the others two long
    frames each (a run of 70 for the split call); connection 50's second frame has another long size and stays in
    the segment plan: its prev chain resolves to a routed frame and it is the floor of the routed frame behind it;
    connection 60's second frame replays that of its first"""
    conns = []
    for j in range(NCONN):
        fr = chain(j, 2, 133 if j < 35 else BIG)
        if j == 50:
            fr[1] = fr[1]._replace(size=BIG + 64)
        if j == 60:
            rx._set_fault(fr, 2, 1, "replay")
        conns.append(Conn(f"conn {j}", 2, fr))
    bad, seen, want = run_engines(gpu, role, conns)
    assert not bad, "\n".join(bad[:20])
    # (the long frames behind connection 50's odd one are a run of 38: they stay too)
    assert seen == want == [(0, 70)]
    conns[50].frames[1] = conns[50].frames[1]._replace(size=BIG)
    conns += [Conn(f"conn {j}", 2, chain(j, 2, BIG)) for j in range(NCONN, NCONN + 32)]
    conns[80].frames[0] = conns[80].frames[0]._replace(size=BIG + 64)
    bad, seen, want = run_engines(gpu, role, conns)
    assert not bad, "\n".join(bad[:20])
    assert seen == want == [(90, 70)]      # 45 connections' frames before the odd one; the 43 behind it stay


@pytest.mark.parametrize("role", rx.ROLES)
def test_failures_inside_a_split_run(gpu, role):
    conns = []
    for j in range(NCONN):
        fr = chain(j, 3, BIG)
        kind, at = {5: ("replay", 0), 64: ("replay", 1), 65: ("tag", 2), 66: ("ct_last", 1), 30: ("name3", 1), 31: ("name7", 1),
                    32: ("flags_ff", 0), 33: ("replay_tag", 2), 69: ("wrong_dir", 2), 0: ("tag", 0)}.get(j, (None, 0))
        if kind:
            rx._set_fault(fr, 2, at, kind)
        conns.append(Conn(f"conn {j} {kind}@{at}", 2, fr))
    bad, seen, want = run_engines(gpu, role, conns)
    assert not bad, "\n".join(bad[:20])
    assert seen == want == [(NCONN * 3, 0)]


def test_two_flushes(gpu):
    """every chain is cut between two flushes -- at a frame edge, or inside a frame that is then carried over -- so
    the second flush's first frame of a connection checks against the cnPeerNonce the first flush left"""
    frame = len(v2_encode(bytes(BIG)))
    conns = []
    for j in range(NCONN):
        fr = chain(j, 4, BIG)
        if j == 9:
            rx._set_fault(fr, 2, 1, "tag")
        if j == 10:
            rx._set_fault(fr, 2, 2, "replay")
        cut = 2 * frame + (0, 0, 1, 60, frame - 1)[j % 5]
        conns.append(Conn(f"conn {j} cut at {cut}", 2, fr, cuts=(cut,)))
    bad, seen, want = run_engines(gpu, rx.SERVER, conns, nflush=2, short=0)
    assert not bad, "\n".join(bad[:20])
    assert seen == want and seen[0] == (2 * NCONN, 0) and seen[1][0] > 64


def test_fewer_than_64_equal_frames(gpu):
    conns = [Conn(f"conn {j}", 2, chain(j, 3, BIG)) for j in range(21)]          # 63 frames
    bad, seen, want = run_engines(gpu, rx.SERVER, conns)
    assert not bad, "\n".join(bad[:20])
    assert seen == want == [(0, 0)]
