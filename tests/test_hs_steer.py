"""CPU: the steered handshakes of tests/hs_steer.py exist, are what they claim to be, and hs_model --
the yardstick of test_gpu_hs_edges.py -- accepts every one of them and refuses each with one tag bit
flipped.  Shown here, without a GPU:
  * every command of every steered lane is accepted by the model for an open and reproduced byte for
    byte by the model for a seal;
  * every key agreement on a steered, non-canonical or low-order point is what the big-integer ladder
    x25519_steer.x25519_ref gives, and what hs_model (through the oracle) used;
  * every Poly1305 case takes, on the restated device arithmetic, the branch it is named for, and per
    kernel path the cases together take every rare branch of poly_finish;
  * every X25519 case satisfies its x25519_steer.CLASSES predicate on the restated device arithmetic.
"""
import functools

import pytest

import hs_model as M
import hs_steer as hs
import poly_steer as ps
import x25519_steer as xs
from cz_testlib import or_beforenm
from hs_steer import CLIENT_PUB, CLIENT_SEC, SERVER_SEC, ZMQ_DEALER, ZMQ_ROUTER

ACC_LISTS = [("hello", hs.acc_hello_lanes), ("cookie", hs.acc_cookie_lanes), ("ready", hs.acc_ready_lanes)] + \
            [("initiate", functools.partial(hs.acc_initiate_lanes, r)) for r in hs.ROTS]
CON_LISTS = [("welcome", hs.con_welcome_lanes), ("initiate", hs.con_initiate_lanes)] + \
            [("ready", functools.partial(hs.con_ready_lanes, r)) for r in hs.ROTS]
# where each steered box lies in the command that carries it (tag first)
BOX_AT = {("acc", "hello"): ("hello", 120), ("acc", "cookie"): ("initiate", 25), ("acc", "initiate"): ("initiate", 113),
          ("acc", "ready"): ("ready", 14), ("con", "welcome"): ("welcome", 24), ("con", "initiate"): ("initiate", 113),
          ("con", "ready"): ("ready", 14)}
# the key a lane's job must end at
JOB_KEY = {"acc k1": "k1", "acc cnPrecom": "precom", "acc k3": "k3", "con kH": "kh", "con cnPrecom": "precom",
           "con kV": "kv"}


def test_model_accepts_every_steered_lane_and_reproduces_every_seal():
    n = 0
    for lane in hs.all_lanes():
        if lane["flip"]:
            continue
        n += 1
        if lane["side"] == "acc":
            welcome, state = M.server_welcome(lane["hello"], SERVER_SEC, lane["seph"], lane["entropy"])
            assert welcome == lane["welcome"] and state == lane["state"], lane["name"]
            ready, facts = M.server_ready(lane["initiate"], state, socket_type=ZMQ_ROUTER, identity=lane["sident"])
            assert ready == lane["ready"] and facts["precom"] == lane["precom"], lane["name"]
            assert facts["client_key"] == lane["client_key"], lane["name"]
            assert facts["metadata"] == M.metadata(ZMQ_DEALER, lane["peer_identity"]), lane["name"]
        else:
            assert M.client_hello(lane["spub"], lane["ceph"]) == lane["hello"], lane["name"]
            got = M.client_open_welcome(lane["welcome"], lane["spub"], lane["ceph"])
            assert got is not None and got[0] == lane["sp"], lane["name"]
            ini = M.client_initiate(lane["welcome"], CLIENT_PUB, CLIENT_SEC, lane["spub"], lane["ceph"], lane["vnonce"],
                                    socket_type=ZMQ_DEALER, identity=lane["cident"])
            assert ini == lane["initiate"], lane["name"]
            meta = M.client_open_ready(lane["ready"], lane["sp"], lane["ceph"])
            assert meta is not None and meta.endswith(M.prop(b"X", lane["peer_x"])), lane["name"]
    per_target, per_instance = len(hs.ALL_POLY), len(hs.PER_INSTANCE)
    assert n == 9 * per_target + 2 * per_instance + 6 * 61 + 2 * 3


def test_key_agreements_are_the_big_integer_ladders():
    """on every lane that carries a point: x25519_ref gives the secret the point's name says, its
    HSalsa20 is the key the lane was sealed under, and the oracle (so hs_model) computes the same"""
    seen = {}
    for lane in hs.all_lanes():
        for job, (kind, pname, k, u) in lane["x"].items():
            shared = xs.x25519_ref(k, u)
            seen.setdefault(job, set()).add(kind)
            if kind == "extreme-scalar":
                mine = lane["sp"] if lane["side"] == "acc" else lane["hello"][80:112]
                assert mine == shared == M.public_key(k), lane["name"]
                continue
            if kind == "steered":
                assert int.from_bytes(shared, "little") == int(pname.split("t=")[1], 16), lane["name"]
            if kind == "low-order":
                assert shared == bytes(32), lane["name"]
            assert lane[JOB_KEY[job]] == hs.hsalsa(shared) == or_beforenm(u, k), lane["name"]
    kinds = {"steered", "noncanonical", "low-order"}
    assert seen == {**{j: kinds for j in hs.ACC_JOBS + hs.CON_JOBS}, "acc base": {"extreme-scalar"},
                    "con base": {"extreme-scalar"}}


def test_points_travel_exactly_as_sent():
    """a non-canonical key is used masked and reduced, but echoed and compared as its 32 bytes"""
    for job in hs.ACC_JOBS + hs.CON_JOBS:
        lanes = hs.acc_x_lanes(job) if job.startswith("acc") else hs.con_x_lanes(job)
        assert [x["x"][job][:2] for x in lanes] == [p[:2] for p in hs.points(hs.JOB_SCALAR[job])] and len(lanes) == 61
        for lane in lanes:
            u = lane["x"][job][3]
            if job in ("acc k1", "acc cnPrecom"):
                assert lane["hello"][80:112] == u == lane["state"]["cli_eph"]
            elif job == "acc k3":
                assert lane["client_key"] == u
            elif job == "con kH":
                assert lane["spub"] == u
            else:
                assert lane["sp"] == u
    hi = [p for p in hs.points(SERVER_SEC) if p[0] == "noncanonical"]
    assert len(hi) == 21 and all(int.from_bytes(u, "little") >= xs.P for _, _, u in hi)


@pytest.mark.parametrize("side,lists", [("acc", ACC_LISTS), ("con", CON_LISTS)], ids=("acceptor", "connector"))
def test_poly_cases_reach_the_branches_they_are_named_for(side, lists):
    seen = {}
    for box, make in lists:
        cmd, at = BOX_AT[side, box]
        lanes = [x for x in make() if x["flip"] is None]
        assert len(lanes) == (len(hs.PER_INSTANCE) if (side, box) in (("acc", "ready"), ("con", "initiate")) else
                              len(hs.ALL_POLY))
        for lane in lanes:
            name, ct, key = lane["poly"][box]
            assert hs.reaches(name, ct, key, seen.setdefault(box, {})), lane["name"]
            assert lane[cmd][at:at + 16 + len(ct)] == ps.poly1305(ct, key) + ct, lane["name"]
            tag, _ = ps.device_finish(ps.device_state(ct, key), ps.key_s(key))
            assert tag == lane[cmd][at:at + 16]
    for box, s in seen.items():
        if (side, box) in (("acc", "ready"), ("con", "initiate")):      # the few targets of the per-instance seals
            assert {0, 1, 3, 4} <= s["h4"] and 2 in s["fold_ripple"] and (1, 1, 1) in s["pad_carry"], box
            continue
        # per kernel path, what test_poly_steer.py asks of the targets as a whole
        assert s["ge"] == {False, True}, box
        assert s["h4"] == {0, 1, 2, 3, 4}, box
        assert 4 in s["g_ripple"], box
        assert s["fold_ripple"] >= {0, 1, 2, 3}, box
        assert s["pad_carry"] >= {(0, 0, 0), (1, 1, 1), (0, 1, 1), (0, 0, 1)}, box


def test_initiate_and_ready_lengths():
    """the xs_mem boxes: every length of INIT_LENS / READY_LENS under 16 targets or more, last chunks of 1,
    15 and 16 bytes, the Salsa20 block edge and both neighbours, the longest and the shortest"""
    got = {}
    for r in hs.ROTS:
        for lane in hs.acc_initiate_lanes(r):
            if lane["flip"] is None:
                got.setdefault(len(lane["initiate"]) - 113 - 16 - 163, set()).add(lane["poly"]["initiate"][0])
    assert sorted(got) == sorted(hs.INIT_LENS) and min(len(v) for v in got.values()) >= 16
    assert set().union(*got.values()) == set(hs.ALL_POLY)
    got = {}
    for r in hs.ROTS:
        for lane in hs.con_ready_lanes(r):
            if lane["flip"] is None:
                got.setdefault(len(lane["ready"]) - 30, set()).add(lane["poly"]["ready"][0])
    assert sorted(got) == sorted(hs.READY_LENS) and min(len(v) for v in got.values()) >= 14
    assert {len(x["sident"]) for x in hs.acc_ready_lanes()} == set(hs.SEAL_LENS)
    assert {len(x["cident"]) for x in hs.con_initiate_lanes()} == set(hs.SEAL_LENS)


@functools.lru_cache(maxsize=None)
def device(k, u):
    return xs.device_x25519(k, u)


def test_x25519_cases_satisfy_their_class_on_the_restated_device_arithmetic():
    n = 0
    for lane in hs.all_lanes():
        for job, (kind, pname, k, u) in lane["x"].items():
            if kind != "steered" or lane["flip"]:
                continue
            out, br = device(k, u)
            cls = pname.split(" t=")[0]
            assert out == xs.x25519_ref(k, u), lane["name"]
            assert xs.CLASSES[cls][1](br), lane["name"]
            n += 1
    assert n == 6 * 33 + len(hs.ALL_POLY) // 2
    assert device.cache_info().currsize == 4 * 33      # s, s', c', c


def test_one_flipped_tag_bit_is_refused_by_the_model():
    n = 0
    words = {}
    for lane in hs.all_lanes():
        if lane["flip"] is None:
            continue
        assert hs.model_refuses(lane), lane["name"]
        n += 1
        if "pad-tag-" in lane["name"]:      # one flip in each of the four tag words
            words.setdefault((lane["side"], lane["name"].split(" flip ")[0]), set()).add(lane["name"].split(" word ")[1][0])
    assert n == 9 * (len(hs.ALL_POLY) + 6)
    assert len(words) == 9 * 2 and all(w == {"0", "1", "2", "3"} for w in words.values())


def test_census_counts_every_path():
    rows = hs.census()
    assert len(rows) == len(hs.PATHS) and all(r[1] > 0 for r in rows)
    assert [r[1] for r in rows[:7]] == [50, 50, 150, 14, 50, 14, 150] and all(r[1] == r[2] for r in rows[:7])
    assert [r[3] for r in rows[7:13]] == [33 + 25] + [33] * 5
