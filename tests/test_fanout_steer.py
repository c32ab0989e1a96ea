"""CPU: the inputs of tests/test_gpu_fanout_edges.py exist, all of them, and the flush scenarios
cut their publishes where their names say.

Steered cases: every (payload length, spec) case of fanout_steer.py is built -- ps.steer raises when
it cannot solve and nothing here catches or skips, so the share of cases left out is zero -- each
payload's seal for its one steered subscriber is reproduced by the oracle (asserted while building)
and carries the big-integer Poly1305 tag, and the census lists what was built.

Flush scenarios: flush_groups() restates the grouping rule of cz_engine_flush_out; for each scenario
the group edges are located inside the publishes, so the GPU module's traffic is known to split a
publish by one edge (with 0, 1, fanout_min - 1, fanout_min and fanout_min + 1 frames on the short
side), by two edges, and to spread 20 publishes over several groups.
"""
import pytest

import fanout_steer as fs
import poly_steer as ps
from cz_testlib import or_curve_decode


@pytest.mark.parametrize("n", fs.FAN_LENS)
def test_every_steered_case_builds(n):
    specs = fs.specs(n)
    built = fs.cases(n)
    assert [c.name for c in built] == [s[0] for s in specs]
    for c in built:
        assert len(c.payload) == n and len(c.body) == n + 33
        key = ps.message_keystream(fs.precom(c.key_idx % fs.NPRE), c.direction, c.counter, 32)
        assert c.key_idx // fs.NPRE == c.direction
        assert c.tag == ps.poly1305(c.body[32:], key), c.name
        # the body opens to the payload and the flags under the same key and direction
        opened = or_curve_decode(c.body, c.direction, fs.precom(c.key_idx % fs.NPRE))
        assert opened == (0, c.payload, c.flags, c.counter), c.name
    tags = {c.tag for c in built}
    assert bytes(16) in tags and b"\xff" * 16 in tags


def test_census_is_complete():
    by_len, by_layout = fs.census()
    names = [name for name, _ in ps.TARGETS]
    assert len(names) == 48
    for n in fs.FAN_LENS:
        want = names + (["h+m-ripple-0", "h+m-ripple-3"] if n >= 47 else [])
        assert by_len[n] == want, n
    assert {n: len(v) for n, v in by_len.items()} == {31: 48, 32: 48, 46: 48, 47: 50, 95: 50, 96: 50, 223: 50,
                                                      224: 50, 4063: 50}
    assert sum(len(v) for v in by_len.values()) == 444
    every = [c for n in fs.FAN_LENS for c in fs.cases(n)]
    assert {(c.direction, c.counter) for c in every} == {(d, c) for d in (0, 1) for c in fs.EDGE_COUNTERS}
    assert {c.flags for c in every} == {0, 1, 2, 3}
    assert {c.key_idx for c in every} == set(range(2 * fs.NPRE))
    # layouts: slots of whole lines and the dense unaligned stride at every length; a multiple of 16
    # up to 256 that is no multiple of 128 exists for bodies of 64, 65, 79, 80 and 129 bytes only
    assert by_layout == {"slots128": fs.FAN_LENS, "region16": [31, 32, 46, 47, 96], "dense_unaligned": fs.FAN_LENS}
    assert [fs.stride_region16(n + 33) for n in by_layout["region16"]] == [64, 80, 80, 80, 144]
    assert len(fs.layout_cases()) == 23


def test_flush_groups_rule():
    assert fs.frame_wire_bytes(0) == 35 and fs.frame_wire_bytes(222) == 257 and fs.frame_wire_bytes(223) == 265
    assert fs.flush_groups([]) == []
    assert fs.flush_groups([100] * 1000) == [(0, 1000)]                  # below 16 MiB: one group
    n = (16 << 20) // fs.frame_wire_bytes(8192)                          # 2037 frames: 64 bytes short of 16 MiB
    assert fs.flush_groups([8192] * n) == [(0, n)]
    assert fs.flush_groups([8192] * (n + 1)) == [(0, (n + 2) // 2), ((n + 2) // 2, n + 1)]
    g = fs.flush_groups([65536] * 4096)                                  # 256 MiB: the cap of 16 groups
    assert len(g) == 16 and all(b - a == 256 for a, b in g)
    # one long frame in front: it closes group 0 and group 1 in the rule's terms, the loop closes one
    # group per frame, so the flush has fewer groups than G
    g = fs.flush_groups([20 << 20] + [100] * 10)
    assert g[0] == (0, 1) and g[-1][1] == 11 and len(g) == 2


def _where(sc, i):
    """(publish number, frames of it before send index i)"""
    fr = sc.frames()
    pub = fr[i].pub
    return pub, sum(1 for f in fr[:i] if f.pub == pub)


@pytest.mark.parametrize("k", fs.SWEEP_K)
def test_edge_sweep_edges(k):
    """one edge; trailing sends push it k frames into the third publish, leading sends pull it k
    frames before the end of the second: the run on the short side has k frames"""
    sc = fs.edge_sweep("trailing", k)
    fr, g = sc.frames(), sc.groups()
    assert len(fr) == 4 * fs.NCON + 2 * k and len(g) == 2
    edge = g[0][1]
    assert edge == 2 * fs.NCON + k
    if k:
        assert _where(sc, edge) == (3, k) and _where(sc, edge - 1) == (3, k - 1)
    else:
        assert _where(sc, edge) == (3, 0) and fr[edge - 1].pub == 2
    sc = fs.edge_sweep("leading", k)
    fr, g = sc.frames(), sc.groups()
    assert len(fr) == 4 * fs.NCON + 2 * k and len(g) == 2
    edge = g[0][1]
    assert [f.pub for f in fr[:2 * k]] == [0] * (2 * k)
    if k:
        assert _where(sc, edge) == (2, fs.NCON - k) and [f.pub for f in fr[edge:edge + k + 1]] == [2] * k + [3]
    else:
        assert _where(sc, edge) == (3, 0) and fr[edge - 1].pub == 2
    assert set(fs.SWEEP_K) == {0, 1, fs.SWEEP_FANOUT_MIN - 1, fs.SWEEP_FANOUT_MIN, fs.SWEEP_FANOUT_MIN + 1}


def test_sweep_publishes_differ_only_in_payload_and_more():
    sc = fs.edge_sweep("trailing", 3)
    pubs = [op for op in sc.ops if op[0] == "publish"]
    assert [len(sc.payloads[op[2]]) for op in pubs] == [8192] * 4
    assert [op[3] for op in pubs] == [False, True, False, False]
    assert len({sc.payloads[op[2]] for op in pubs}) == 4
    assert {op[1] for op in sc.ops if op[0] == "send"} == set(fs.SEND_CONNS)


def test_two_edges():
    sc = fs.two_edges()
    fr = sc.frames()
    assert len(fr) == 3300 and {f.pub for f in fr} == {1}
    assert sc.groups() == [(0, 1100), (1100, 2200), (2200, 3300)]
    ids = [f.conn for f in fr]
    assert set(ids) == set(range(fs.NCON)) and ids != sorted(ids)
    assert min(ids.count(c) for c in range(fs.NCON)) >= 6                          # every id repeats


def test_mixed():
    sc = fs.mixed()
    fr, g = sc.frames(), sc.groups()
    lens = [len(sc.payloads[f.name]) for f in fr]
    assert sum(fs.frame_wire_bytes(n) for n in lens) >= 16 << 20 and len(g) >= 2
    pubs = [op for op in sc.ops if op[0] == "publish"]
    assert sorted((len(sc.payloads[op[2]]), len(op[1])) for op in pubs) == sorted(
        (n, s) for n in (0, 100, 223, 65536) for s in (3, 63, 64, 65, 520))
    # a publish is cut by an edge, and publishes lie whole inside a group next to other frames
    cut = [e for _, e in g[:-1] if fr[e].pub and fr[e - 1].pub == fr[e].pub]
    assert cut
    # the msg_alloc'ed payload is queued last but lies first in the arena
    assert sc.ops[0] == ("alloc", "early") and sc.ops[-1][:3] == ("send", 7, "early")
    # the wire_iov connections' frames interleave with others'
    for c in fs.IOV_CONNS:
        at = [i for i, f in enumerate(fr) if f.conn == c]
        assert sum(1 for a, b in zip(at, at[1:]) if b != a + 1) >= 3


def test_scenario_list():
    names = [sc.name for sc in fs.scenarios()]
    assert len(names) == len(set(names)) == 12
