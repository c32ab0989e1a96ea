"""GPU: the batched CURVE handshake kernels at their Poly1305 and X25519 edges.

test_gpu_acceptor.py and test_gpu_connector.py feed the nine handshake kernels keys, nonces and bytes
from splitmix_bytes and one recorded session, which take the rare branches of poly_block /
poly_finish (probability ~2^-100) and of fe_to_words (~2^-250) never.  tests/hs_steer.py builds whole
handshakes in which one box's Poly1305 or one key agreement sits on such a branch
(test_hs_steer.py shows on the CPU that each does); here the compiled kernels get them: xs_fixed<4> and
xs_fixed<8> in registers, xs_mem at the chunk and keystream-block edges, k_x25519_jobs in all six of its
roles, with non-canonical and low-order points and the extreme scalars.

Bit-exact comparisons only.  The yardstick is tests/hs_model.py, and for a sample of lanes of every
kernel path -- every low-order point among them -- also the per-connection state machine cz_hs fed the
same bytes and injected values.  Every batch is one stage call of at most about 200 lanes: steered
lanes, their copies with one tag bit flipped (which must be refused as CRYPTOGRAPHIC), and honest
random lanes of the two existing suites on both sides of the 64-lane workgroup edge and in a partial
last workgroup, which must come out as the model says, steered neighbours or not.
"""
import pytest

import hs_model as M
import hs_steer as hs
import test_gpu_acceptor as TA
import test_gpu_connector as TC
from hs_steer import CLIENT_PUB, CLIENT_SEC, SERVER_SEC, ZMQ_DEALER, ZMQ_ROUTER
from test_gpu_connector import gpu  # noqa: F401  (the fixture: _lib, acceptor, connector, engine, hs)

pytestmark = pytest.mark.gpu
CRYPTOGRAPHIC = TA.CRYPTOGRAPHIC
assert (TA.SERVER_SEC, TC.CLIENT_SEC, TC.CLIENT_PUB) == (SERVER_SEC, CLIENT_SEC, CLIENT_PUB)


# ---- honest neighbours, from the existing suites' conn() ------------------------------------------
def honest_acc(i, seed, sident=b""):
    c = TA.conn(i, seed)
    ini = TA.initiate_of(c, socket_type=ZMQ_DEALER)
    ready, facts = M.server_ready(ini, c["state"], socket_type=ZMQ_ROUTER, identity=sident)
    return {"side": "acc", "name": f"honest {i}", "honest": True, "flip": None, "seph": c["seph"],
            "entropy": c["entropy"], "hello": c["hello"], "welcome": c["welcome"], "initiate": ini, "ready": ready,
            "precom": facts["precom"], "client_key": c["cpub"], "peer_identity": b"", "sident": sident, "poly": {},
            "x": {}}


def honest_con(i, seed, cident=b""):
    c = TC.conn(i, seed, ctype=ZMQ_DEALER, cident=cident, stype=ZMQ_ROUTER)
    return {"side": "con", "name": f"honest {i}", "honest": True, "flip": None, "ceph": c["ceph"],
            "vnonce": c["vnonce"], "spub": c["spub"], "hello": c["hello"], "welcome": c["welcome"],
            "initiate": c["initiate"], "ready": c["ready"], "precom": c["precom"], "cident": cident,
            "peer_type": b"ROUTER", "peer_x": None, "poly": {}, "x": {}}


def interleave(steered, honest):
    """an honest lane after every second steered one, then honest lanes until the last workgroup is a
    partial one; both kinds on each side of the 64-lane edge"""
    out, k = [], 0
    for i, lane in enumerate(steered):
        out.append(lane)
        if i % 2:
            out.append(honest(k))
            k += 1
    while len(out) % 64 in (0, 1) or len(out) < 66:
        out.append(honest(k))
        k += 1
    kinds = [bool(x.get("honest")) for x in out]
    assert 64 < len(out) <= 200 and len(out) % 64
    assert {True, False} == set(kinds[:64]) == set(kinds[64:]) and {True, False} <= set(kinds[len(out) // 64 * 64 - 3:])
    return out


def around(steered, honest, at):
    """one steered lane at index `at` of 66 otherwise honest lanes"""
    out = [honest(k) for k in range(65)]
    out.insert(at, steered)
    return out


def sample(lanes, every=4):
    """the lanes that also go to cz_hs: the first and every `every`-th steered lane with its flipped copies,
    the all-zero and all-ones tags, every low-order point and extreme scalar, and two honest lanes"""
    pick, n, honest = set(), 0, 0
    for i, lane in enumerate(lanes):
        if lane.get("honest"):
            honest += 1
            if honest <= 2:
                pick.add(i)
            continue
        if lane["flip"] is None:
            n += 1
        rare = "pad-tag-" in lane["name"] or any(v[0] in ("low-order", "extreme-scalar") for v in lane["x"].values())
        if n % every == 1 or rare:
            pick.add(i)
    return pick


# ---- the acceptor ---------------------------------------------------------------------------------------
def cz_hs_accept(gpu, lane):
    """what a cz_hs server with the lane's injected values makes of the lane's two commands"""
    srv = gpu.hs.CurveServerHandshake(SERVER_SEC, socket_type=ZMQ_ROUTER, identity=lane["sident"],
                                      ephemeral_secret=lane["seph"], entropy=lane["entropy"])
    assert srv.processHandshakeCommand(lane["hello"]) == 0
    ev = srv.last_event
    rc, reply = srv.nextHandshakeCommand()
    assert rc == 0
    if reply.data[:6] == b"\x05ERROR":
        return ev, reply.data
    rc = srv.processHandshakeCommand(lane["initiate"])
    if rc != 0:
        assert rc == gpu.hs.EPROTO
        return ev, reply.data, gpu.lib.CZ_EPROTO, srv.last_event
    rc, ready = srv.nextHandshakeCommand()
    assert rc == 0
    return ev, reply.data, 0, 0, ready.data, srv.session(), srv.client_key(), srv.peer_property("Identity")


def run_acceptor(gpu, lanes, check=()):
    """Both stages of one acceptor over `lanes`, one hello() and one initiate() call, every lane against
    the model; the lanes in `check` also against cz_hs."""
    L = gpu.lib
    n = len(lanes)
    (sident,) = {x["sident"] for x in lanes}
    acc = gpu.acceptor.CurveAcceptor(SERVER_SEC, socket_type=ZMQ_ROUTER, identity=sident, max_pending=n,
                                     ephemeral_secrets=[x["seph"] for x in lanes], entropy=[x["entropy"] for x in lanes])
    r1 = acc.hello([x["hello"] for x in lanes])
    live = []
    for i, x in enumerate(lanes):
        if x["flip"] == "hello":        # an ERROR reply and no slot
            assert r1[i] == (0, CRYPTOGRAPHIC, -1, M.ERROR_EMPTY), x["name"]
        else:
            assert r1[i][:2] == (0, 0) and r1[i][2] >= 0 and r1[i][3] == x["welcome"], f"WELCOME of lane {i}: {x['name']}"
            live.append(i)
    assert acc.pending() == len(live) and len({r1[i][2] for i in live}) == len(live)
    r2 = dict(zip(live, acc.initiate([r1[i][2] for i in live], [lanes[i]["initiate"] for i in live])))
    views = {}
    for i, x in enumerate(lanes):
        slot = r1[i][2]
        if i not in r2:
            views[i] = (r1[i][1], r1[i][3])
        elif x["flip"]:                 # refused, and no session on the slot
            assert r2[i] == (L.CZ_EPROTO, CRYPTOGRAPHIC, slot, b""), x["name"]
            with pytest.raises(L.CzError):
                acc.session(slot)
            views[i] = (0, r1[i][3], r2[i][0], r2[i][1])
        else:
            assert r2[i] == (0, 0, slot, x["ready"]), f"READY of lane {i}: {x['name']}"
            assert acc.session(slot) == (x["precom"], 2, 2), f"session of lane {i}: {x['name']}"
            assert acc.client_key(slot) == x["client_key"], x["name"]
            assert acc.peer_property(slot, "Identity") == x["peer_identity"], x["name"]
            assert acc.peer_property(slot, "Socket-Type") == b"DEALER"
            views[i] = (0, r1[i][3], 0, 0, r2[i][3], acc.session(slot), acc.client_key(slot),
                        acc.peer_property(slot, "Identity"))
    acc.close()
    for i in sorted(check):
        assert views[i] == cz_hs_accept(gpu, lanes[i]), f"cz_hs on lane {i}: {lanes[i]['name']}"
    return views


def test_acceptor_hello_boxes_at_every_target(gpu):
    """xs_fixed<4,true> in k_acc_welcome; every second steered HELLO also carries a C' steered for s"""
    lanes = interleave(hs.acc_hello_lanes(), lambda k: honest_acc(k, 31))
    assert sum(1 for x in lanes if x["flip"] == "hello") == len(hs.ALL_POLY) + 6
    run_acceptor(gpu, lanes, sample(lanes, 8))


def test_acceptor_cookies_at_every_target(gpu):
    """xs_fixed<4,false> in k_acc_welcome seals the steered cookie, xs_fixed<4,true> in k_acc_initiate opens it"""
    lanes = interleave(hs.acc_cookie_lanes(), lambda k: honest_acc(k, 32))
    run_acceptor(gpu, lanes, sample(lanes, 8))


@pytest.mark.parametrize("rot", hs.ROTS)
def test_acceptor_initiate_boxes_at_every_target(gpu, rot):
    """xs_mem<true> in k_acc_initiate, identity lengths INIT_LENS rotated through the targets"""
    lanes = interleave(hs.acc_initiate_lanes(rot), lambda k: honest_acc(k, 33 + rot))
    run_acceptor(gpu, lanes, sample(lanes, 8))


@pytest.mark.parametrize("i", range(len(hs.PER_INSTANCE)), ids=hs.PER_INSTANCE)
def test_acceptor_ready_seal(gpu, i):
    """xs_mem<false> in k_acc_ready: the acceptor's own identity steers the READY it seals for one connection"""
    lane = hs.acc_ready_lanes()[i]
    at = (0, 63, 64, 65)[i % 4]
    lanes = around(lane, lambda k: honest_acc(k, 36, lane["sident"]), at)
    run_acceptor(gpu, lanes, {at, (at + 1) % 66})


@pytest.mark.parametrize("job", hs.ACC_JOBS)
def test_acceptor_key_agreements(gpu, job):
    """k_x25519_jobs as the acceptor runs it: the 33 steered classes, the non-canonical and the low-order
    points of one job, and S' = s'.9 at the extreme scalars, through both stages to the session"""
    steered = hs.acc_x_lanes(job) + hs.acc_base_lanes()
    lanes = interleave(steered, lambda k: honest_acc(k, 37))
    assert len(steered) == 33 + 21 + 7 + 3
    run_acceptor(gpu, lanes, sample(lanes))


# ---- the connector --------------------------------------------------------------------------------------
def cz_hs_connect(gpu, lane):
    """what a cz_hs client with the lane's injected values sends and makes of the lane's two commands"""
    cli = gpu.hs.CurveClientHandshake(CLIENT_PUB, CLIENT_SEC, lane["spub"], socket_type=ZMQ_DEALER,
                                      identity=lane["cident"], ephemeral_secret=lane["ceph"], entropy=lane["vnonce"])
    rc, hello = cli.nextHandshakeCommand()
    assert rc == 0
    rc = cli.processHandshakeCommand(lane["welcome"])
    if rc != 0:
        assert rc == gpu.hs.EPROTO
        return hello.data, gpu.lib.CZ_EPROTO, cli.last_event
    rc, ini = cli.nextHandshakeCommand()
    assert rc == 0
    rc = cli.processHandshakeCommand(lane["ready"])
    if rc != 0:
        assert rc == gpu.hs.EPROTO
        return hello.data, 0, 0, ini.data, gpu.lib.CZ_EPROTO, cli.last_event
    return hello.data, 0, 0, ini.data, 0, 0, cli.session(), cli.peer_property("X"), cli.peer_property("Socket-Type")


def run_connector(gpu, lanes, check=()):
    """All three stages of one connector over `lanes`, one call each, every lane against the model; the
    lanes in `check` also against cz_hs."""
    L = gpu.lib
    n = len(lanes)
    (cident,) = {x["cident"] for x in lanes}
    con = gpu.connector.CurveConnector(CLIENT_PUB, CLIENT_SEC, socket_type=ZMQ_DEALER, identity=cident, max_pending=n,
                                       ephemeral_secrets=[x["ceph"] for x in lanes],
                                       vouch_nonces=[x["vnonce"] for x in lanes])
    r1 = con.hello([x["spub"] for x in lanes])
    slots = [r[2] for r in r1]
    assert sorted(slots) == list(range(n))
    for i, x in enumerate(lanes):
        assert r1[i] == (0, 0, slots[i], x["hello"]), f"HELLO of lane {i}: {x['name']}"
        assert con.server_key(slots[i]) == x["spub"], x["name"]
    r2 = con.welcome(slots, [x["welcome"] for x in lanes])
    live = []
    for i, x in enumerate(lanes):
        if x["flip"] == "welcome":
            assert r2[i] == (L.CZ_EPROTO, CRYPTOGRAPHIC, slots[i], b""), x["name"]
        else:
            assert r2[i] == (0, 0, slots[i], x["initiate"]), f"INITIATE of lane {i}: {x['name']}"
            live.append(i)
    r3 = dict(zip(live, con.ready([slots[i] for i in live], [lanes[i]["ready"] for i in live])))
    views = {}
    for i, x in enumerate(lanes):
        if x["flip"]:
            if i in r3:
                assert r3[i] == (L.CZ_EPROTO, CRYPTOGRAPHIC, slots[i], b""), x["name"]
            with pytest.raises(L.CzError):
                con.session(slots[i])
            views[i] = (r1[i][3],) + r2[i][:2] + ((r2[i][3],) + r3[i][:2] if i in r3 else ())
        else:
            assert r3[i] == (0, 0, slots[i], b""), f"READY of lane {i}: {x['name']}"
            assert con.session(slots[i]) == (x["precom"], 3, 1), f"session of lane {i}: {x['name']}"
            assert con.error_status(slots[i]) == 0
            assert con.peer_property(slots[i], "X") == x["peer_x"], x["name"]
            assert con.peer_property(slots[i], "Socket-Type") == x["peer_type"], x["name"]
            views[i] = (r1[i][3], 0, 0, r2[i][3], 0, 0, con.session(slots[i]), con.peer_property(slots[i], "X"),
                        con.peer_property(slots[i], "Socket-Type"))
    assert con.pending() == n
    con.close()
    for i in sorted(check):
        assert views[i] == cz_hs_connect(gpu, lanes[i]), f"cz_hs on lane {i}: {lanes[i]['name']}"
    return views


@pytest.mark.parametrize("job", hs.CON_JOBS)
def test_connector_key_agreements(gpu, job):
    """k_x25519_jobs as the connector runs it: steered, non-canonical and low-order server keys given to
    hello() (kH), and S' inside the WELCOME box (cnPrecom, kV); C' = c'.9 at the extreme scalars"""
    steered = hs.con_x_lanes(job) + hs.con_base_lanes()
    lanes = interleave(steered, lambda k: honest_con(k, 41))
    assert len(steered) == 33 + 21 + 7 + 3
    run_connector(gpu, lanes, sample(lanes))


def test_connector_welcome_boxes_at_every_target(gpu):
    """xs_fixed<8,true> in k_con_welcome, steered through the cookie bytes"""
    lanes = interleave(hs.con_welcome_lanes(), lambda k: honest_con(k, 42))
    assert sum(1 for x in lanes if x["flip"] == "welcome") == len(hs.ALL_POLY) + 6
    run_connector(gpu, lanes, sample(lanes, 8))


@pytest.mark.parametrize("rot", hs.ROTS)
def test_connector_ready_boxes_at_every_target(gpu, rot):
    """xs_mem<true> in k_con_ready, plaintext lengths READY_LENS rotated through the targets"""
    lanes = interleave(hs.con_ready_lanes(rot), lambda k: honest_con(k, 43 + rot))
    run_connector(gpu, lanes, sample(lanes, 8))


@pytest.mark.parametrize("i", range(len(hs.PER_INSTANCE)), ids=hs.PER_INSTANCE)
def test_connector_initiate_seal(gpu, i):
    """xs_mem<false> in k_con_initiate: the connector's own identity steers the INITIATE it seals for one connection"""
    lane = hs.con_initiate_lanes()[i]
    at = (0, 63, 64, 65)[i % 4]
    lanes = around(lane, lambda k: honest_con(k, 46, lane["cident"]), at)
    run_connector(gpu, lanes, {at, (at + 1) % 66})
