"""The receive model (tests/rx_model.py) on the CPU: it accepts what libzmq accepted, names the
reference's events, and its scenario table keeps the coverage the device tests rely on."""
import json
import os
import re

import pytest

import rx_model as rx
from cz_testlib import splitmix_bytes, v2_encode

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
S = json.load(open(os.path.join(HERE, "golden", "libzmq_session.json")))
SESSIONS = [(S["precom"], S["c2s"], S["s2c"], S["ready_nonce"]),
            (S["server_session"]["precom"], S["server_session"]["c2s"], S["server_session"]["s2c"], 1)]


@pytest.mark.parametrize("session", [0, 1])
@pytest.mark.parametrize("role", rx.ROLES)
def test_model_accepts_the_libzmq_session_and_rejects_its_replays(session, role):
    precom, c2s, s2c, ready_nonce = SESSIONS[session]
    precom = bytes.fromhex(precom)
    # the handshake's last nonces: a server has seen INITIATE (2), a client READY
    msgs, floor = (c2s, 2) if role == rx.SERVER else (s2c, ready_nonce)
    m = rx.RxModel(role, floor, precom)
    for v in msgs:
        body = bytes.fromhex(v["body"])
        assert m.decode(body) == (rx.ST_OK, 0, splitmix_bytes(v["n"], v["seed"]), v["flags"])
        assert m.peer_nonce == v["nonce"]
        # the same body again: a replay, whatever came before it, and the state does not move
        for earlier in msgs:
            r = rx.RxModel(role, v["nonce"], precom)
            if earlier["nonce"] > v["nonce"]:
                break
            st, ev, payload, fl = r.decode(bytes.fromhex(earlier["body"]))
            assert (st, payload, fl) == (rx.ST_SEQUENCE, None, None)
            assert ev == (rx.EV_INVALID_SEQUENCE if role == rx.SERVER else rx.EV_CRYPTOGRAPHIC)
            assert r.peer_nonce == v["nonce"] and r.dead and r.decode(body) is None
    # opened as the other direction the first body fails its tag, and cnPeerNonce has moved
    other = rx.RxModel(rx.CLIENT if role == rx.SERVER else rx.SERVER, floor, precom)
    assert other.decode(bytes.fromhex(msgs[0]["body"]))[:2] == (rx.ST_CRYPTO, rx.EV_CRYPTOGRAPHIC)
    assert other.peer_nonce == msgs[0]["nonce"]


def test_events_are_the_references_names_and_the_headers_values():
    with open(os.path.join(HERE, "golden", "reference_java.json")) as f:
        ref = json.load(f)["files"]
    names = {m.strip() for m in ref["ZMQ.java"]["members"]}
    header = open(os.path.join(ROOT, "include", "curvezmq_mi355x.h")).read()
    for value, name in rx.EVENT_NAMES.items():
        assert name in names
        macro = "CZ_ZMTP_" + name[len("ZMQ_PROTOCOL_ERROR_ZMTP_"):]
        assert int(re.search(rf"#define {macro} (0x[0-9a-fA-F]+)", header).group(1), 16) == value
    for st, nm in rx.STATUS_NAMES.items():
        assert int(re.search(rf"#define CZ_STATUS_{nm} (\d+)", header).group(1)) == st
    for k in ("CZ_EPROTO", "CZ_EMSGSIZE"):
        assert int(re.search(rf"#define {k} \((-\d+)\)", header).group(1)) == getattr(rx, k)
    # the compared values are Java longs: the comparison is signed
    for f in ("io/mechanism/curve/CurveClientMechanism.java", "io/mechanism/curve/CurveServerMechanism.java"):
        assert "private long cnPeerNonce;" in ref[f]["members"]
    assert rx.event_for(rx.ST_SEQUENCE, rx.SERVER) == rx.EV_INVALID_SEQUENCE
    assert rx.event_for(rx.ST_SEQUENCE, rx.CLIENT) == rx.EV_CRYPTOGRAPHIC
    for role in rx.ROLES:
        assert rx.event_for(rx.ST_CRYPTO, role) == rx.EV_CRYPTOGRAPHIC
        assert rx.event_for(rx.ST_COMMAND, role) == rx.EV_UNEXPECTED_COMMAND
        assert rx.event_for(rx.ST_MALFORMED, role) == rx.EV_MALFORMED_COMMAND_MESSAGE


def test_signed_comparison():
    assert rx.s64((1 << 63) - 1) == (1 << 63) - 1 and rx.s64(1 << 63) == -(1 << 63) and rx.s64((1 << 64) - 1) == -1
    for name, (floor, nonces, want) in rx.NONCE_RUNS.items():
        sc = next(s for s in rx.scenarios() if s.name == f"run:{name}")
        assert sc.floor == floor and tuple(f.nonce for f in sc.frames) == nonces
        for role in rx.ROLES:
            assert tuple(e[0] for e in sc.raw_expect(role)) == want, name


def test_scenario_table_coverage():
    """every fault kind at every position, every nonce run, every size, every chain length: an edit
    that thins the table fails here"""
    table = rx.scenarios()
    tags = {t for s in table for t in s.tags}
    for kind in rx.FAULT_KINDS:
        for pos in rx.POSITIONS:
            assert ("fault", kind, pos) in tags, (kind, pos)
    assert len(rx.FAULT_KINDS) == 14 and rx.POSITIONS == ("0", "1", "63", "64", "65", "last")
    assert rx.CHAIN_LENGTHS == (1, 64, 65, 130) and rx.BODY_SIZES == (33, 34, 96, 97, 161, 4129, 300033)
    for name in rx.NONCE_RUNS:
        assert ("run", name) in tags
    grid = [s for s in table if any(t[0] == "fault" for t in s.tags)]
    assert {len(s.frames) for s in grid} == set(rx.CHAIN_LENGTHS)
    # the tags tell the truth: the named frame carries the named fault, and no other frame is damaged
    for s in grid:
        (p,) = s.faults()
        for t in s.tags:
            if t[0] == "fault":
                assert t[1] == s.frames[p].fault and (t[2] == str(p) or (t[2] == "last" and p == len(s.frames) - 1)), s.name
            elif t[0] == "len":
                assert t[1] == len(s.frames)
    assert {f.size for s in table for f in s.frames} == set(rx.BODY_SIZES)
    assert {len(b) for s in table for b in s.bodies(rx.SERVER)} >= {0, 7, 8, 16, 20, 32} | set(rx.BODY_SIZES)
    # the split body: accepted, rejected early as SEQUENCE and as COMMAND, rejected by its tag, and
    # followed by a frame whose floor is its nonce (one accepted, one a replay of it)
    big = {s.name: s for s in table if s.name.startswith("big:")}
    st = {n: [e[0] for e in s.raw_expect(rx.SERVER)] for n, s in big.items()}
    assert st["big:ok_then_next"] == [0, 0, 0, 0] and st["big:ok_then_replay_of_it"] == [0, 0, rx.ST_SEQUENCE, 0]
    assert st["big:replay"][1] == rx.ST_SEQUENCE and st["big:name3"][1] == rx.ST_COMMAND
    assert st["big:tag"][1] == rx.ST_CRYPTO and st["big:ct_last"][1] == rx.ST_CRYPTO
    assert st["big:replay@0"] == [rx.ST_SEQUENCE, 0]
    assert all(any(f.size == rx.BIG for f in s.frames) for s in big.values())
    # uniform chains: every size, every fault that keeps the size at every position in some chain, the
    # runs inside the chain, and a fault on the first frame behind the phase-sorted block
    uni = [s for s in table if s.uniform]
    assert {s.uniform for s in uni} == set(rx.UNIFORM_SIZES)
    for size in rx.UNIFORM_SIZES:
        seen = {(t[1], t[2]) for s in uni if s.uniform == size and len(s.frames) == 130 for t in s.tags
                if t[0] == "uniform_fault"}
        assert {p for _, p in seen} == {0, 1, 63, 64, 65, 129}
        assert {k for k, _ in seen} == set(rx.UNIFORM_KINDS)
    carry = [s for s in uni if len(s.frames) > rx.CARRY_FRAMES]
    assert carry and all(s.frames[rx.CARRY_FRAMES].fault and s.uniform == 4129 for s in carry)
    for s in uni:
        nonces = [f.nonce for f in s.frames]
        for floor, run, want in rx.NONCE_RUNS.values():
            at = next(i for i in range(len(nonces)) if tuple(nonces[i:i + len(run) + 1]) == (floor,) + run)
            assert tuple(e[0] for e in s.raw_expect(rx.SERVER)[at + 1:at + 1 + len(run)]) == want
    assert len(table) == len({s.name for s in table})


@pytest.mark.parametrize("role", rx.ROLES)
def test_expectations_are_self_consistent(role):
    for s in rx.scenarios():
        bodies, e, raw = s.bodies(role), s.expect(role), s.raw_expect(role)
        faults = s.faults()
        # the delivered prefix ends at the first failure, and holds what was sealed
        n_ok = len(e.delivered)
        assert n_ok == (e.failed_at if e.failed_at is not None else len(bodies)), s.name
        for i in range(n_ok):
            fl = 3 if s.frames[i].fault == "flags_ff" else s.frames[i].flags
            assert e.delivered[i] == (s.payload(i), fl), (s.name, i)
        # until the first failure the chained per-frame rule and the sequential rule are one rule
        first_raw = next((i for i, r in enumerate(raw) if r[0] != rx.ST_OK), None)
        if first_raw is not None or len(raw) == len(bodies):
            assert first_raw == e.failed_at, s.name
            if first_raw is not None:
                assert raw[first_raw][0] == e.status, s.name
        for i, r in enumerate(raw):
            if r[0] == rx.ST_OK:
                want_flags = 0xff if s.frames[i].fault == "flags_ff" else s.frames[i].flags
                assert r[1:] == (want_flags, s.payload(i), s.frames[i].nonce), (s.name, i)
        # cnPeerNonce moves on OK and CRYPTO, and on nothing else
        before = s.frames[e.failed_at - 1].nonce if e.failed_at else s.floor
        if e.failed_at is None:
            assert e.peer_nonce == s.frames[-1].nonce and e.event == 0
        elif e.status == rx.ST_CRYPTO:
            assert e.peer_nonce == rx.wire_nonce(bodies[e.failed_at]) != before, s.name
        else:
            assert e.status in (rx.ST_SEQUENCE, rx.ST_COMMAND, rx.ST_MALFORMED) and e.peer_nonce == before, s.name
        assert e.event == (rx.event_for(e.status, role) if e.failed_at is not None else 0)
        # a single-fault scenario fails exactly where its fault says, or not at all
        if s.uniform is None and faults:
            (p,) = faults
            want = rx.FAULT_STATUS[s.frames[p].fault]
            assert (e.failed_at, e.status) == ((p, want) if want else (None, 0)), s.name
        elif s.uniform is None and not s.name.startswith("run:"):
            assert e.failed_at is None, s.name


@pytest.mark.parametrize("role", rx.ROLES)
def test_stream_model_agrees_with_the_sequence_model(role):
    """one flush, two flushes cut inside a frame, and byte by byte: the same deliveries"""
    for s in rx.single_fault_scenarios():
        if any(f.size == rx.BIG for f in s.frames) and not s.name.endswith("replay@0"):
            continue   # (the long bodies add nothing here)
        wire, e = s.wire(role), s.expect(role)
        err = (rx.CZ_EPROTO, e.event) if e.failed_at is not None else (0, 0)
        (one,) = rx.stream_model(role, s.floor, [(wire, True)])
        assert (one["delivered"], one["peer_nonce"], one["error"]) == (e.delivered, e.peer_nonce, err), s.name
        assert one["refused"] == (e.failed_at is not None)
        cut = len(wire) // 2
        two = rx.stream_model(role, s.floor, [(wire[:cut], True), (wire[cut:], True)])
        assert two[0]["delivered"] + two[1]["delivered"] == e.delivered, s.name
        assert (two[1]["peer_nonce"], two[1]["error"]) == (e.peer_nonce, err), s.name
        assert two[0]["delivered"] == e.delivered[:len(two[0]["delivered"])]


def test_stream_model_framing():
    good = [rx.build_body(rx.Frame(3 + i, 40 + i, None, i & 3, 60 + i), rx.SERVER) for i in range(3)]
    bad = rx.build_body(rx.Frame(9, 50, "tag", 0, 70), rx.SERVER)
    large0 = bytes([2]) + bytes(8)                                   # LARGE header, size 0: EPROTO
    # a V2 COMMAND bit on a MESSAGE frame, and a LARGE header under 256 bytes, change nothing
    wire = v2_encode(good[0]) + bytes([4, len(good[1])]) + good[1] + bytes([2]) + len(good[2]).to_bytes(8, "big") + good[2]
    (r,) = rx.stream_model(rx.SERVER, 2, [(wire, True)])
    assert [f for _, f in r["delivered"]] == [0, 1, 2] and r["error"] == (0, 0) and r["peer_nonce"] == 5
    # a framing error after good frames: no event; a mechanism failure ahead of it wins
    (r,) = rx.stream_model(rx.SERVER, 2, [(v2_encode(good[0]) + large0 + v2_encode(good[1]), True)])
    assert len(r["delivered"]) == 1 and r["error"] == (rx.CZ_EPROTO, 0) and r["refused"]
    (r,) = rx.stream_model(rx.SERVER, 2, [(v2_encode(good[0]) + v2_encode(bad) + large0, True)])
    assert len(r["delivered"]) == 1 and r["error"] == (rx.CZ_EPROTO, rx.EV_CRYPTOGRAPHIC) and r["peer_nonce"] == 9
    # a partial frame is kept; bytes after a teardown are dropped
    w = v2_encode(good[0]) + v2_encode(good[1])
    a, b = rx.stream_model(rx.SERVER, 2, [(w[:len(w) - 5], True), (w[len(w) - 5:], True)])
    assert len(a["delivered"]) == 1 and len(b["delivered"]) == 1 and b["error"] == (0, 0)
    a, b = rx.stream_model(rx.SERVER, 2, [(v2_encode(bad), True), (v2_encode(good[0]), True)])
    assert a["refused"] and b["delivered"] == [] and b["error"] == a["error"]
