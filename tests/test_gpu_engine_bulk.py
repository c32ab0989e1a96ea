"""GPU: the bulk session hand-over (k_session_subkeys, k_scatter_wipe; cz_engine_add_conns,
cz_engine_add_accepted_batch, cz_engine_add_connected_batch, cz_engine_remove_conns and the two
release_batch calls).

Truth is the CPU oracle: every wire byte a connection sends must be the V2 framing of the MESSAGE body
or_curve_encode makes under that session's cnPrecom, role and nonce, and every connection must deliver a
message the oracle sealed for it.  The handshake commands come from the CPU model tests/hs_model.py.  An
engine built by the loop of single adds (the path the bulk calls replace) appears only as a second witness
for the ids.  Shapes: one lane pair, the 64-lane wave edge (32 sessions) and the 256-lane block edge (128
sessions) on both sides, a batch that grows the subkey table past its first capacity (64 connections), and
reused ids whose key slots are scattered."""
import ctypes

import numpy as np
import pytest

import hs_model as M
import test_gpu_acceptor as TA
import test_gpu_connector as TC
from cz_testlib import or_beforenm, or_curve_encode, splitmix_bytes, v2_encode

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from jeromq_amd import _lib, acceptor, connector, engine
    return type("G", (), {"lib": _lib, "acceptor": acceptor, "connector": connector, "engine": engine})


def key(i, seed=0):
    return splitmix_bytes(32, 9100000 + 1000 * seed + i)


def sent(tag, k):
    return splitmix_bytes(100, 77000 + 1000 * tag + k)


def received(tag, k):
    return splitmix_bytes(100, 88000 + 1000 * tag + k)


def queue(eng, conns, tag):
    for k, (cid, _, _, _, _) in enumerate(conns):
        assert eng.send(cid, sent(tag, k)) == 0, f"connection {cid}"


def check_flushed(eng, conns, tag):
    """after flush_out: every connection's wire bytes are the oracle's for its key, role and next nonce"""
    for k, (cid, precom, server, tx, _) in enumerate(conns):
        want = v2_encode(or_curve_encode(sent(tag, k), 0, tx, int(server), precom))
        assert eng.wire_out(cid) == want, f"connection {cid} (item {k}) seals other bytes than the oracle"
        assert eng.nonce(cid) == tx + 1


def deliver(eng, conns, tag):
    """every connection is handed one message the oracle sealed as its peer, one above its nonce floor"""
    for k, (cid, precom, server, _, rx) in enumerate(conns):
        assert eng.recv(cid, v2_encode(or_curve_encode(received(tag, k), 0, rx + 1, int(not server), precom))) == 0


def check_delivered(eng, conns, tag):
    for k, (cid, _, _, _, rx) in enumerate(conns):
        assert eng.error(cid) == (0, 0), f"connection {cid} (item {k})"
        assert eng.messages_in(cid) == [(received(tag, k), 0)], f"connection {cid} (item {k})"
        assert eng.peer_nonce(cid) == rx + 1


def traffic(eng, conns, tag):
    """conns: [(id, cnPrecom, as_server, next nonce to send, last peer nonce accepted)].  One 100-byte
    message each way on every connection; returns conns with the counters moved on."""
    queue(eng, conns, tag)
    eng.flush_out()
    check_flushed(eng, conns, tag)
    deliver(eng, conns, tag)
    eng.flush_in()
    check_delivered(eng, conns, tag)
    return [(cid, precom, server, tx + 1, rx + 1) for cid, precom, server, tx, rx in conns]


EDGE_NONCES = [2, 3, (1 << 32) - 1, (1 << 63) - 1, 1 << 32, 1]


@pytest.mark.parametrize("count", [1, 31, 32, 33, 127, 128, 129, 130])
def test_wave_and_block_edges(gpu, count):
    rng = np.random.default_rng(count)
    roles = [bool(x) for x in rng.integers(0, 2, size=count)]
    roles[0], roles[-1] = True, count == 1     # both roles in every batch of more than one
    keys = [key(i, count) for i in range(count)]
    tx = [EDGE_NONCES[(i + count) % len(EDGE_NONCES)] for i in range(count)]
    rx = [EDGE_NONCES[(3 * i + 2) % len(EDGE_NONCES)] for i in range(count)]
    eng = gpu.engine.CurveBatchEngine(arena_bytes=1 << 20)
    ids = eng.add_connections(keys, as_server=roles, cn_nonce=tx, cn_peer_nonce=rx)
    assert ids == list(range(count))
    for i in range(count):
        assert (eng.nonce(ids[i]), eng.peer_nonce(ids[i])) == (tx[i], rx[i])
    traffic(eng, list(zip(ids, keys, roles, tx, rx)), 1)
    eng.close()


def test_default_nonces_per_role(gpu):
    eng = gpu.engine.CurveBatchEngine(arena_bytes=1 << 20)
    ids = eng.add_connections([key(0, 50), key(1, 50)], as_server=[True, False])
    assert [(eng.nonce(c), eng.peer_nonce(c)) for c in ids] == [(2, 2), (3, 1)]
    assert eng.add_connections([]) == []
    assert eng.add_connections([key(2, 50)]) == [2] and (eng.nonce(2), eng.peer_nonce(2)) == (3, 1)


def test_drop_in_ids_and_reused_key_slots(gpu):
    """two engines with one history; the six adds by loop in one, by batch in the other"""
    engines = [gpu.engine.CurveBatchEngine(arena_bytes=1 << 20) for _ in range(2)]
    old = [key(i, 60) for i in range(10)]
    new = [key(i, 61) for i in range(6)]
    roles = [bool(i & 1) for i in range(10)]
    new_roles = [True, False, False, True, True, False]
    for eng in engines:
        assert [eng.add_connection(old[i], as_server=roles[i]) for i in range(10)] == list(range(10))
        for c in (2, 7, 5):
            eng.remove_connection(c)
    by_loop = [engines[0].add_connection(new[i], as_server=new_roles[i]) for i in range(6)]
    by_batch = engines[1].add_connections(new, as_server=new_roles)
    assert by_batch == by_loop == [5, 7, 2, 10, 11, 12]
    live = {i: (old[i], roles[i]) for i in range(10) if i not in (2, 7, 5)}
    live.update({cid: (new[j], new_roles[j]) for j, cid in enumerate(by_batch)})
    assert len(live) == 13
    conns = [(cid, k, srv, 2 if srv else 3, 2 if srv else 1) for cid, (k, srv) in sorted(live.items())]
    wires = []
    for eng in engines:
        traffic(eng, conns, 2)       # oracle-correct under the new keys: ids 5, 7 and 2 included
        wires.append([eng.wire_out(cid) for cid, *_ in conns])
    assert wires[0] == wires[1]
    for j, cid in enumerate(by_batch[:3]):
        stale = v2_encode(or_curve_encode(sent(2, [c[0] for c in conns].index(cid)), 0, 2 if roles[cid] else 3,
                                          int(roles[cid]), old[cid]))
        assert engines[1].wire_out(cid) != stale


def test_table_growth_inside_a_batch(gpu):
    """the subkey table's first capacity is 4096 bytes, 64 connections: a batch of 200 behind three
    connections with queued messages grows it once and keeps what it held"""
    eng = gpu.engine.CurveBatchEngine(arena_bytes=1 << 20)
    first = [(eng.add_connection(key(i, 70), as_server=bool(i & 1)), key(i, 70), bool(i & 1), 2 if i & 1 else 3,
              2 if i & 1 else 1) for i in range(3)]
    queue(eng, first, 3)
    keys = [key(i, 71) for i in range(200)]
    roles = [i % 3 == 0 for i in range(200)]
    ids = eng.add_connections(keys, as_server=roles)
    assert ids == list(range(3, 203))
    eng.flush_out()
    check_flushed(eng, first, 3)
    first = [(cid, k, srv, tx + 1, rx) for cid, k, srv, tx, rx in first]
    rest = [(ids[i], keys[i], roles[i], 2 if roles[i] else 3, 2 if roles[i] else 1) for i in range(200)]
    traffic(eng, first + rest, 4)


def test_from_the_acceptor(gpu):
    L = gpu.lib
    n = 130
    failed = {5, 64, 129}
    conns = [TA.conn(i, 2) for i in range(n)]
    acc = TA.make_acceptor(gpu, conns, max_pending=n + 2)
    r1 = acc.hello([c["hello"] for c in conns])
    assert [r[3] for r in r1] == [c["welcome"] for c in conns]
    slots = [r[2] for r in r1]
    inits = [TA.initiate_of(c, vouch_flip=40) if i in failed else TA.initiate_of(c) for i, c in enumerate(conns)]
    r2 = acc.initiate(slots, inits)
    assert [i for i, r in enumerate(r2) if r[0] != 0] == sorted(failed)
    # the client's side of each session: cnPrecom = beforenm(S', c')
    precom = [or_beforenm(M.public_key(c["seph"]), c["ceph"]) for c in conns]
    unused = sorted(set(range(n + 2)) - set(slots))
    assert len(unused) == 2
    named = slots + [slots[7], n + 2, unused[0], -1, 1 << 30]
    eng = gpu.engine.CurveBatchEngine(arena_bytes=1 << 20)
    ids = eng.add_accepted_many(acc, named)
    assert [j for j, c in enumerate(ids) if c < 0] == sorted(failed) + [n + 1, n + 2, n + 3, n + 4]
    assert all(c == L.CZ_EINVAL for c in ids if c < 0)
    good = [j for j, c in enumerate(ids) if c >= 0]
    assert [ids[j] for j in good] == list(range(n - len(failed) + 1))     # no id consumed by a failed item
    assert good[-1] == n and ids[n] != ids[7]                               # the doubled slot: two connections
    which = list(range(n)) + [7]
    live = [(ids[j], precom[which[j]], True, 2, 2) for j in good]
    for j in good:
        assert acc.session(named[j])[0] == precom[which[j]]
    live = traffic(eng, live, 5)
    # release_many is all or nothing
    for bad in (slots + [unused[1]], slots + [slots[3]], slots[:4] + [-1], slots[:4] + [n + 2]):
        with pytest.raises(L.CzError):
            acc.release_many(bad)
        assert acc.pending() == n
    assert acc.session(slots[0])[0] == precom[0]
    acc.release_many(slots)
    assert acc.pending() == 0
    for s in (slots[0], slots[5], slots[-1]):
        with pytest.raises(L.CzError):
            acc.session(s)
    with pytest.raises(L.CzError):
        acc.release_many([slots[0]])
    # the connections outlive the slots: the release did not overtake the engine's read of the keys
    traffic(eng, live, 6)


def test_from_the_connector(gpu):
    L = gpu.lib
    n = 70
    failed = {0, 33, 64}
    conns = [TC.conn(i, 31, srv=i % 3, ready_nonce=1 + 5 * i) for i in range(n)]
    assert len({c["spub"] for c in conns}) == 3
    con = TC.make_connector(gpu, conns, max_pending=n + 2)
    r1 = con.hello([c["spub"] for c in conns])
    assert [r[3] for r in r1] == [c["hello"] for c in conns]
    slots = [r[2] for r in r1]
    r2 = con.welcome(slots, [c["welcome"] for c in conns])
    assert [r[3] for r in r2] == [c["initiate"] for c in conns]
    r3 = con.ready(slots, [TC.flip(c["ready"], 20) if i in failed else c["ready"] for i, c in enumerate(conns)])
    assert [i for i, r in enumerate(r3) if r[0] != 0] == sorted(failed)
    unused = sorted(set(range(n + 2)) - set(slots))
    named = slots + [slots[69], unused[0], n + 2]
    eng = gpu.engine.CurveBatchEngine(arena_bytes=1 << 20)
    ids = eng.add_connected_many(con, named)
    assert [j for j, c in enumerate(ids) if c < 0] == sorted(failed) + [n + 1, n + 2]
    good = [j for j, c in enumerate(ids) if c >= 0]
    assert [ids[j] for j in good] == list(range(n - len(failed) + 1)) and ids[n] != ids[69]
    which = list(range(n)) + [69]
    # client role: cn_nonce 3, the READY's nonce as peer nonce
    live = [(ids[j], conns[which[j]]["precom"], False, 3, 1 + 5 * which[j]) for j in good]
    for cid, _, _, tx, rx in live:
        assert (eng.nonce(cid), eng.peer_nonce(cid)) == (tx, rx)
    for j in good:
        assert con.session(named[j]) == (conns[which[j]]["precom"], 3, 1 + 5 * which[j])
    live = traffic(eng, live, 7)
    for bad in (slots + [unused[1]], slots + [slots[0]]):
        with pytest.raises(L.CzError):
            con.release_many(bad)
        assert con.pending() == n
    con.release_many(slots)
    assert con.pending() == 0
    with pytest.raises(L.CzError):
        con.session(slots[1])
    traffic(eng, live, 8)


def test_bulk_remove(gpu):
    L = gpu.lib
    n = 130
    keys = [key(i, 90) for i in range(n)]
    roles = [i % 5 < 2 for i in range(n)]
    eng = gpu.engine.CurveBatchEngine(arena_bytes=1 << 20)
    ids = eng.add_connections(keys, as_server=roles)
    conns = [(ids[i], keys[i], roles[i], 2 if roles[i] else 3, 2 if roles[i] else 1) for i in range(n)]
    queue(eng, conns, 9)
    deliver(eng, conns, 9)
    gone = [(7 * i + 3) % n for i in range(65)]
    assert len(set(gone)) == 65
    named = gone[:20] + [gone[4]] + gone[20:] + [1000]
    rcs = eng.remove_connections(named)
    assert rcs == [0] * 20 + [L.CZ_EINVAL] + [0] * 45 + [L.CZ_EINVAL]
    # the survivors' flush: their own bytes, in their own order, and nothing of the removed
    eng.flush_out()
    eng.flush_in()
    for k, (cid, precom, server, tx, rx) in enumerate(conns):
        if cid in gone:
            with pytest.raises(L.CzError):
                eng.wire_out(cid)
            with pytest.raises(L.CzError):
                eng.messages_in(cid)
            assert eng.send(cid, b"x") == L.CZ_EINVAL and eng.recv(cid, b"x") == L.CZ_EINVAL
            assert eng.error(cid)[0] == L.CZ_EINVAL and eng.nonce(cid) == 0
            continue
        assert eng.wire_out(cid) == v2_encode(or_curve_encode(sent(9, k), 0, tx, int(server), precom)), cid
        assert eng.error(cid) == (0, 0) and eng.messages_in(cid) == [(received(9, k), 0)], cid
    assert eng.remove_connections([gone[0], gone[64]]) == [L.CZ_EINVAL] * 2
    # a following batch add reuses exactly those ids, last removed first
    fresh = [key(i, 91) for i in range(66)]
    again = eng.add_connections(fresh, as_server=True)
    assert again == gone[::-1] + [n]
    survivors = [(cid, k, srv, tx + 1, rx + 1) for cid, k, srv, tx, rx in conns if cid not in gone]
    traffic(eng, survivors + [(cid, fresh[j], True, 2, 2) for j, cid in enumerate(again)], 10)


def test_a_refused_call_hands_out_nothing(gpu):
    L = gpu.lib
    lib = L.lib()
    E = L.CZ_EINVAL
    eng = gpu.engine.CurveBatchEngine(arena_bytes=1 << 20)
    assert eng.add_connections([key(i, 95) for i in range(3)]) == [0, 1, 2]
    eng.remove_connection(1)
    conns = [TA.conn(i, 2) for i in range(2)]
    acc = TA.make_acceptor(gpu, conns, max_pending=2)
    slots = [r[2] for r in acc.hello([c["hello"] for c in conns])]
    assert [r[0] for r in acc.initiate(slots, [TA.initiate_of(c) for c in conns])] == [0, 0]
    arr = np.array(slots, dtype=np.int32)
    ids = np.full(2, 7, dtype=np.int32)
    keys = key(0, 96) + key(1, 96)
    n64 = np.array([2, 2], dtype=np.uint64)
    assert lib.cz_engine_add_accepted_batch(eng._h, acc._h, 2, arr.ctypes.data, None) == E
    assert lib.cz_engine_add_accepted_batch(eng._h, acc._h, 2, None, ids.ctypes.data) == E and ids.tolist() == [E, E]
    assert lib.cz_engine_add_conns(eng._h, 2, None, keys, n64.ctypes.data, n64.ctypes.data, None) == E
    assert lib.cz_engine_add_conns(eng._h, 2, None, None, n64.ctypes.data, n64.ctypes.data, ids.ctypes.data) == E
    assert lib.cz_engine_add_accepted_batch(eng._h, acc._h, 0, None, None) == L.CZ_OK
    # every item refused: no id consumed either
    assert eng.add_accepted_many(acc, [-1, 2, 99]) == [E, E, E]
    # the next ids are the ones that were next before: the removed id, then a new one
    assert eng.add_connection(key(2, 96)) == 1 and eng.add_connection(key(3, 96)) == 3
    assert eng.add_accepted_many(acc, slots) == [4, 5]
    traffic(eng, [(4 + i, or_beforenm(M.public_key(c["seph"]), c["ceph"]), True, 2, 2) for i, c in enumerate(conns)], 11)
