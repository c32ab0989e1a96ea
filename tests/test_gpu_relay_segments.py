"""GPU: the segmented CURVE relay (cz_relay_segments) against the CPU oracle and the receive model.

Truth never comes from the library: bodies are sealed by the oracle and damaged here or as
tests/rx_model.py damages them, and the expected status, nonce and output body of every frame are
tests/relay_model.relay_expect's.  The second yardstick is relay_batch on the device, byte-equal in
output, status and nonces.  Whole sentinel-filled buffers are compared, as tests/test_gpu_relay.py does:
the guard bytes between the bodies, the status and nonce entries around the call's range, and the bytes
around the workspace -- its 128 bytes per part are the only thing the call may scribble on."""
import ctypes
import functools

import numpy as np
import pytest

import rx_model as rx
from cz_testlib import DESC_DTYPE
from test_gpu_relay import GUARD, M64, MARGIN, NPAIR, PRECOMS, SENT, Fr, _dev, _expect_batch, _r, gpu, make_body  # noqa: F401
from test_gpu_segments import _uneven_plan

pytestmark = pytest.mark.gpu

# frames of one segment, whatever the segment length of the test: early rejects, the flags byte only, the
# block edge, the w03 tail, two blocks and a tail
UNSPLIT = (0, 7, 8, 32, 33, 34, 64, 65, 129)
LAST = (1, 16, 17, 64)          # bytes in the last block: the w03 tail (<= 16) and the partial Poly1305 block


def _boundary_blocks(s):
    """body block counts around the cuts of segment length s (tests/test_gpu_segments.py::_boundary_lengths)"""
    return sorted({s + s // 2, s + s // 2 + 1, 2 * s, 2 * s + 1, 3 * s - 1, 5 * s + 2})


def _frame(i, size, seed=0, fault=None, nonce=None, floor=None, prev=-1, check=True):
    """frame i of a batch: keys cycle through all table rows on both sides (equal on some frames)"""
    kin, kout = (i + seed) % (2 * NPAIR), (3 * i + 1 + seed) % (2 * NPAIR)
    if i % 5 == 0:
        kout = kin
    if nonce is None:
        nonce = (1 << 32) * (i + 1) + 77 + i
    counter = nonce if i % 4 == 0 else (1 << 40) + 13 * i
    body = make_body(size, nonce, i & 3, 700 + 31 * seed + i, kin, fault)
    return Fr(body, nonce - 1 if floor is None else floor, kin, counter, kout, check=check, prev=prev)


def _flip(fr, off, bit=0x10):
    b = bytearray(fr.body)
    b[off] ^= bit
    fr.body = bytes(b)
    return fr


@functools.lru_cache(maxsize=None)
def _cut_edge_frames(s):
    """every boundary block count of segment length s with every last-block size, and the unsplit sizes"""
    sizes = [64 * (nblk - 1) + last for nblk in _boundary_blocks(s) for last in LAST]
    sizes = [z for z in dict.fromkeys(sizes) if z >= 33] + list(UNSPLIT)
    return tuple(_frame(i, z, seed=s) for i, z in enumerate(sizes))


# ---- plans ---------------------------------------------------------------------------------------------
def _set_plan(plan, segs, combs, npart, batch):
    plan.segments = np.array(segs, dtype=batch.SEGMENT_DTYPE).reshape(-1)
    plan.combines = np.array(combs, dtype=batch.COMBINE_DTYPE).reshape(-1)
    plan.nseg, plan.ncomb, plan.npart = len(plan.segments), len(plan.combines), npart
    return plan


def plan_planner(g, desc, s):
    """cz_plan_segments(open = 1): the plan an open_segments of the same descriptors takes.  The planner
    refuses seg_blocks 1, so that plan is built here by the same rule (section 3b's caller-built plan)."""
    if s >= 2:
        return g.batch.SegmentPlan(desc, open_=True, seg_blocks=s)
    segs, combs, npart = [], [], 0
    for i, d in enumerate(desc):
        nblk = max((int(d["len"]) + 63) // 64, 1)
        if nblk <= s + s // 2:
            segs.append((i, 0, nblk, 0xFFFFFFFF))
            continue
        ns = (nblk - 1 + s - 1) // s
        combs.append((i, npart, ns, 0))
        for k in range(ns):
            b0 = k * s + 1 if k else 0
            b1 = (k + 1) * s + 1 if k + 1 < ns else nblk
            segs.append((i, b0, b1 - b0, npart + k))
        npart += ns
    return _set_plan(g.batch.SegmentPlan(desc, open_=True, seg_blocks=2), segs, combs, npart, g.batch)


def plan_by_blocks(g, desc, s):
    """the planner's plan with its segments sorted by block count, longest first (any order is legal): the
    relay's chunk count is the block count, so full waves of one count take the line emitters"""
    plan = plan_planner(g, desc, s)
    plan.segments = plan.segments[np.argsort(-plan.segments["nblocks"].astype(np.int64), kind="stable")]
    return plan


def plan_uneven(seed, min_b0):
    def make(g, desc, s):
        return _uneven_plan(g.batch.SegmentPlan(desc, open_=True, seg_blocks=s), np.random.default_rng(seed), True, min_b0)
    return make


# ---- one call, everything compared ------------------------------------------------------------------------
def _layout(g, frames, in_a, out_a, slot, phase):
    """body i at a `slot`-aligned start + phase + in_a, its output at one + phase + out_a, at least GUARD
    sentinel bytes around every output"""
    n = len(frames)
    desc = np.zeros(n, dtype=DESC_DTYPE)
    to = np.zeros(n, dtype=g.batch.FANOUT_SUB_DTYPE)
    io, oo = slot, _r(GUARD, slot)
    for i, f in enumerate(frames):
        desc[i] = (io + phase + in_a, oo + phase + out_a, len(f.body), f.kin, f.floor, 0x100 if f.check else 0, f.prev)
        to[i] = (f.counter, f.kout, 0)
        io += _r(len(f.body) + phase + in_a, slot) + slot
        oo += _r(len(f.body) + phase + out_a, slot) + _r(GUARD, slot)
    hin = np.full(io + 64, 0x3C, dtype=np.uint8)
    for i, f in enumerate(frames):
        hin[int(desc[i]["in_off"]):int(desc[i]["in_off"]) + len(f.body)] = np.frombuffer(f.body, dtype=np.uint8)
    return desc, to, hin, oo + 64


def _call(g, desc, to, plan, d_in, out_bytes, stream=None):
    """relay_segments into fresh sentinel-filled buffers; returns (out, status, nonces, workspace margins ok)"""
    t, n = g.torch, len(desc)
    d_out = t.full((out_bytes,), SENT, dtype=t.uint8, device=g.dev)
    status = t.full((n + 2 * MARGIN,), -1, dtype=t.int16, device=g.dev)
    nonces = t.full((n + 2 * MARGIN,), -7, dtype=t.int64, device=g.dev)
    plan.to(g.dev, records=2)
    work = 128 * max(plan.npart, 1)
    big = t.full((64 + work + 64,), SENT, dtype=t.uint8, device=g.dev)
    plan.d_work = big[64:64 + work]
    g.batch.relay_segments(_dev(g, desc), _dev(g, to), plan, d_in, d_out, g.subkeys, status[MARGIN:MARGIN + n],
                           nonces=nonces[MARGIN:MARGIN + n], stream=stream, desc_np=desc, to_np=to)
    return d_out, status, nonces, big


def run_segments(g, frames, s, make_plan=plan_planner, in_a=0, out_a=0, slot=16, phase=0, roundtrip=False):
    frames = list(frames)
    n = len(frames)
    desc, to, hin, out_bytes = _layout(g, frames, in_a, out_a, slot, phase)
    plan = make_plan(g, desc, s)
    exp = _expect_batch(frames)
    want = np.full(out_bytes, SENT, dtype=np.uint8)
    for i, (_st, _n, ob) in enumerate(exp):
        want[int(desc[i]["out_off"]):int(desc[i]["out_off"]) + len(ob)] = np.frombuffer(ob, dtype=np.uint8)
    t = g.torch
    d_in = _dev(g, hin)
    d_out, status, nonces, big = _call(g, desc, to, plan, d_in, out_bytes)
    # the second yardstick: one lane per frame on the device
    d_out2 = t.full((out_bytes,), SENT, dtype=t.uint8, device=g.dev)
    status2 = t.full((n,), -1, dtype=t.int16, device=g.dev)
    nonces2 = t.full((n,), -7, dtype=t.int64, device=g.dev)
    g.batch.relay_batch(_dev(g, desc), _dev(g, to), n, d_in, d_out2, g.subkeys, status2, nonces=nonces2, desc_np=desc,
                        to_np=to)
    t.cuda.synchronize()
    st = status.cpu().numpy().view(np.uint16)
    nn = nonces.cpu().numpy().view(np.uint64)
    out = d_out.cpu().numpy()
    bad = []
    for i, (est, enonce, ob) in enumerate(exp):
        o = int(desc[i]["out_off"])
        if st[MARGIN + i] != est:
            bad.append(f"frame {i} (size {len(frames[i].body)}): status {st[MARGIN + i]:#x}, model {est:#x}")
        elif out[o:o + len(ob)].tobytes() != ob:
            d = np.flatnonzero(out[o:o + len(ob)] != np.frombuffer(ob, dtype=np.uint8))
            bad.append(f"frame {i} (size {len(frames[i].body)}, status {est:#x}): {len(d)} output bytes differ, first at {int(d[0])}")
        if enonce is not None and int(nn[MARGIN + i]) != enonce:
            bad.append(f"frame {i}: nonce {int(nn[MARGIN + i]):#x}, model {enonce:#x}")
    assert not bad, "\n".join(bad[:12])
    assert np.array_equal(out, want), "bytes outside the relayed bodies changed"
    for a in (st, nn):
        edge = np.concatenate([a[:MARGIN], a[MARGIN + n:]])
        assert np.all(edge == edge[0]) and edge[0] in (0xffff, (1 << 64) - 7), "entries outside the call's range changed"
    edges = big.cpu().numpy()
    assert np.all(edges[:64] == SENT) and np.all(edges[-64:] == SENT), "bytes around the workspace changed"
    assert np.array_equal(out, d_out2.cpu().numpy()), "output differs from relay_batch's"
    assert np.array_equal(st[MARGIN:MARGIN + n], status2.cpu().numpy().view(np.uint16)), "statuses differ from relay_batch's"
    assert np.array_equal(nn[MARGIN:MARGIN + n], nonces2.cpu().numpy().view(np.uint64)), "nonces differ from relay_batch's"
    if roundtrip:
        _roundtrip(g, frames, desc, to, d_out, st[MARGIN:MARGIN + n])
    return out, st[MARGIN:MARGIN + n], plan


def _roundtrip(g, frames, desc, to, d_out, st):
    """the relayed bodies open under the outbound key to the oracle's payloads and its flags & 3"""
    t, n = g.torch, len(frames)
    rdesc = desc.copy()
    po = 0
    for i in range(n):
        rdesc[i] = (desc[i]["out_off"], po, desc[i]["len"], to[i]["key_idx"], (int(to[i]["counter"]) - 1) & M64, 0x100, -1)
        po += _r(max(int(desc[i]["len"]), 33) - 33, 16) + 16
    d_back = t.zeros(po + 64, dtype=t.uint8, device=g.dev)
    st3 = t.full((n,), -1, dtype=t.int16, device=g.dev)
    g.batch.open_batch(_dev(g, rdesc), n, d_out, d_back, g.subkeys, st3, desc_np=rdesc)
    t.cuda.synchronize()
    st3, back, seen = st3.cpu().numpy().view(np.uint16), d_back.cpu().numpy(), 0
    for i, f in enumerate(frames):
        floor = rx.wire_nonce(frames[f.prev].body) if f.prev >= 0 else f.floor
        mst, flags, payload, _n = rx.frame_status(f.body, floor, f.check, f.kin & 1, PRECOMS[f.kin >> 1])
        assert (st[i] & 0xff) == mst
        if mst != rx.ST_OK:
            continue
        p = int(rdesc[i]["out_off"])
        assert st3[i] == (flags & 3) << 8, f"frame {i}: relayed body opens with status {st3[i]:#x}"
        assert back[p:p + len(payload)].tobytes() == payload, f"frame {i}: round trip payload differs"
        seen += 1
    assert seen


# ---- cut edges, unsplit frames, alignments -------------------------------------------------------------------
@pytest.mark.parametrize("s,in_a,out_a", [(1, 0, 0), (2, 1, 3), (3, 8, 8), (5, 15, 0)])
def test_cut_edges(gpu, s, in_a, out_a):
    """frames of 1.5 s, 1.5 s + 1, 2 s, 2 s + 1, 3 s - 1 and 5 s + 2 blocks, each ending 1, 16, 17 and 64
    bytes into its last block, with the unsplit sizes in the same batch: combine_tag's one-, two- and
    many-segment paths, the w03 tail and the partial Poly1305 block at a cut"""
    _out, _st, plan = run_segments(gpu, _cut_edge_frames(s), s, in_a=in_a, out_a=out_a, roundtrip=True)
    nsegs = {int(c["nseg"]) for c in plan.combines}
    assert 2 in nsegs and max(nsegs) > 2 and (s != 1 or 1 in nsegs)


def test_one_long_frame_at_the_default_segment_length(gpu):
    _out, st, plan = run_segments(gpu, [_frame(1, 65569)], gpu.batch.SEG_BLOCKS, roundtrip=True)
    assert plan.nseg == 8 and plan.ncomb == 1 and st[0] & 0xff == rx.ST_OK


def test_unsplit_frames_in_one_batch(gpu):
    frames = [_frame(i, z, seed=3) for i, z in enumerate(UNSPLIT + (4129,))]
    _out, _st, plan = run_segments(gpu, frames, gpu.batch.SEG_BLOCKS, roundtrip=True)
    assert plan.ncomb == 0 and plan.nseg == len(frames)


@functools.lru_cache(maxsize=None)
def _alignment_frames():
    sizes = UNSPLIT + tuple(64 * (nblk - 1) + last for nblk, last in ((4, 1), (5, 16), (7, 17), (12, 64)))
    return tuple(_frame(i, z, seed=5) for i, z in enumerate(sizes))


@pytest.mark.parametrize("out_a", (0, 3, 8))
@pytest.mark.parametrize("in_a", (0, 1, 8, 15))
def test_alignments(gpu, in_a, out_a):
    """split and unsplit frames at every input alignment x output alignment: lane-wise, byte-exact"""
    run_segments(gpu, _alignment_frames(), 2, in_a=in_a, out_a=out_a)


# ---- the line path ---------------------------------------------------------------------------------------------
class _Tune:
    def __init__(self, g, **knobs):
        self.lib, self.knobs, self.old = g.L.lib(), knobs, {}

    def __enter__(self):
        for k, v in self.knobs.items():
            self.old[k] = self.lib.cz_tune(k.encode(), v)
            assert self.old[k] >= 0

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.lib.cz_tune(k.encode(), v)


@functools.lru_cache(maxsize=None)
def _line_frames(count):
    """frames of 7 blocks, the last one of 1, 16, 17 or 64 bytes: at segment length 2 three segments each"""
    return tuple(_frame(i, 64 * 6 + LAST[i % 4], seed=7) for i in range(count))


@pytest.mark.parametrize("seglines,shift16", [(1, 1), (0, 1), (1, 0)])
@pytest.mark.parametrize("phase", (0, 16), ids=("slots128", "slots16"))
def test_line_path(gpu, phase, seglines, shift16):
    """64 frames of 7 blocks at segment length 2, the plan sorted by block count: 192 segments in three full
    waves of one chunk count, on 128-byte slots (EmitSegLines) and on slots 16 bytes off them
    (EmitShiftLines, or EmitSegLines without shift16), with the knobs on and off"""
    with _Tune(gpu, seglines=seglines, shift16=shift16):
        _out, st, plan = run_segments(gpu, _line_frames(64), 2, make_plan=plan_by_blocks, slot=128, phase=phase)
    assert plan.nseg == 192 and plan.ncomb == 64
    for w in range(3):
        assert len(set(plan.segments["nblocks"][64 * w:64 * w + 64])) == 1
    assert np.all(st & 0xff == rx.ST_OK)


@pytest.mark.parametrize("phase", (0, 16), ids=("slots128", "slots16"))
def test_line_path_with_a_partial_last_wave(gpu, phase):
    """one frame more: a wave of mixed block counts and a partial last wave store lane by lane behind the
    line-staged ones; and the planner's own order (keyed on the open's chunk count) over the same frames"""
    _out, _st, plan = run_segments(gpu, _line_frames(65), 2, make_plan=plan_by_blocks, slot=128, phase=phase)
    assert plan.nseg == 195
    run_segments(gpu, _line_frames(65), 2, slot=128, phase=phase)


# ---- rejects -----------------------------------------------------------------------------------------------------
def _rejected(kind, i=1):
    """a frame of 7 blocks (three segments at segment length 2), or a cut one, rejected as `kind` says"""
    size = 64 * 6 + 17
    if kind == "command":
        return _frame(i, size, fault="name3"), rx.ST_COMMAND
    if kind == "malformed":
        return _frame(i, 20, fault=None), rx.ST_MALFORMED
    if kind == "sequence":
        return _frame(i, size, nonce=900, floor=900), rx.ST_SEQUENCE
    off = {"flip_seg0": 40, "flip_middle": 64 * 3 + 5, "flip_last_seg": 64 * 5 + 3, "flip_last_byte": size - 1, "flip_tag": 20}[kind]
    return _flip(_frame(i, size), off), rx.ST_CRYPTO


REJECTS = ("command", "malformed", "sequence", "flip_seg0", "flip_middle", "flip_last_seg", "flip_last_byte", "flip_tag")


@pytest.mark.parametrize("kind", REJECTS)
def test_rejected_frame_alone_and_between_neighbours(gpu, kind):
    """the status, zeros over exactly the frame's bytes, and its neighbours (a split and an unsplit one) intact"""
    fr, want = _rejected(kind)
    out, st, _plan = run_segments(gpu, [fr], 2, out_a=3)
    assert st[0] == want and not out[GUARD + 3:GUARD + 3 + len(fr.body)].any()
    _out, st, _plan = run_segments(gpu, [_frame(0, 64 * 4 + 1), fr, _frame(2, 129), _frame(3, 64 * 8)], 2, in_a=1, roundtrip=True)
    assert [int(x) & 0xff for x in st] == [rx.ST_OK, want, rx.ST_OK, rx.ST_OK]


def test_sequence_chains_across_split_and_unsplit_frames(gpu):
    """prev chains of one connection: every frame must beat the wire nonce of the frame before it, split or
    not, accepted or not; a replayed nonce is SEQUENCE on a split frame (every segment zeroes its range) and
    on an unsplit one"""
    kin, kout = 3, 6
    sizes = (129, 64 * 6 + 17, 65, 64 * 9 + 1, 64 * 4 + 16, 34, 64 * 5)
    nonces = (10, 11, 11, 11, 12, 12, 1 << 40)
    frames = []
    for i, (z, nv) in enumerate(zip(sizes, nonces)):
        frames.append(Fr(make_body(z, nv, i & 3, 5000 + i, kin), 9, kin, (1 << 50) + i, kout, prev=i - 1))
    _out, st, plan = run_segments(gpu, frames, 2, roundtrip=True)
    assert plan.ncomb == 4
    ok, seq = rx.ST_OK, rx.ST_SEQUENCE
    assert [int(x) & 0xff for x in st] == [ok, ok, seq, seq, ok, seq, ok]


@pytest.mark.parametrize("kind", ("command", "flip_middle"))
def test_rejected_frame_inside_a_full_uniform_wave(gpu, kind):
    """one frame of the line-path batch rejected: before decryption, its three waves go lane-wise and each of
    its segments zeroes its own range; by its tag, the waves stay line-staged and the combine zeroes the body"""
    frames = list(_line_frames(64))
    size = len(frames[10].body)
    frames[10] = _frame(10, size, seed=7, fault="name3") if kind == "command" else _flip(_frame(10, size, seed=7), 64 * 3 + 5)
    _out, st, _plan = run_segments(gpu, frames, 2, make_plan=plan_by_blocks, slot=128)
    want = rx.ST_COMMAND if kind == "command" else rx.ST_CRYPTO
    assert [int(x) & 0xff for x in st] == [want if i == 10 else rx.ST_OK for i in range(64)]


# ---- caller-built plans ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,min_b0", [(1, 1), (2, 2)])
def test_caller_built_uneven_plans(gpu, seed, min_b0):
    """random uneven cuts of the planner's plan at segment length 6 (2..6 segments per split frame, in the
    order a caller left them): cuts from block 1 on -- the relay needs no "block 2 or later" rule -- and
    cuts that obey the open's rule"""
    sizes = [64 * (nblk - 1) + last for nblk, last in ((10, 1), (11, 16), (13, 17), (20, 64), (31, 5), (40, 33), (9, 64))]
    frames = [_frame(i, z, seed=11 + seed) for i, z in enumerate(sizes + [33, 129, 64 * 9])]
    frames.insert(4, _flip(_frame(40, 64 * 12 + 7, seed=seed), 64 * 7))
    _out, st, plan = run_segments(gpu, frames, 6, make_plan=plan_uneven(seed, min_b0), in_a=seed, out_a=8 * (seed - 1),
                                  roundtrip=True)
    assert plan.ncomb >= 7 and len({int(x) for x in plan.segments["nblocks"]}) > 2
    assert st[4] == rx.ST_CRYPTO


# ---- graph capture -------------------------------------------------------------------------------------------------------
def _graph_topology(graph):
    """(nodes, edges as index pairs) of a captured graph, from the HIP runtime the process already holds"""
    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
    hip = ctypes.CDLL(path)
    hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    hip.hipGraphGetEdges.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    nn = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(nn)) == 0
    nodes = (ctypes.c_void_p * max(nn.value, 1))()
    assert hip.hipGraphGetNodes(graph, nodes, ctypes.byref(nn)) == 0
    ne = ctypes.c_size_t(0)
    assert hip.hipGraphGetEdges(graph, None, None, ctypes.byref(ne)) == 0
    src, dst = (ctypes.c_void_p * max(ne.value, 1))(), (ctypes.c_void_p * max(ne.value, 1))()
    if ne.value:
        assert hip.hipGraphGetEdges(graph, src, dst, ctypes.byref(ne)) == 0
    ids = [nodes[i] for i in range(nn.value)]
    return ids, [(ids.index(src[i]), ids.index(dst[i])) for i in range(ne.value)]


def test_graph_capture_and_replay(gpu):
    """one capture on a non-default stream and one replay: two kernel nodes in a single chain (segments, then
    combine), no parallel branch, and the replay's output byte-equal to the eager call's"""
    t = gpu.torch
    frames = [_frame(i, z, seed=9) for i, z in enumerate((64 * 6 + 17, 129, 64 * 4 + 1, 33, 64 * 11))]
    desc, to, hin, out_bytes = _layout(gpu, frames, 0, 0, 16, 0)
    d_in = _dev(gpu, hin)
    plan = plan_planner(gpu, desc, 2)
    eager, st_e, nn_e, _big = _call(gpu, desc, to, plan, d_in, out_bytes)
    t.cuda.synchronize()
    d_desc, d_to = _dev(gpu, desc), _dev(gpu, to)
    n = len(frames)
    d_out = t.full((out_bytes,), SENT, dtype=t.uint8, device=gpu.dev)
    status = t.full((n,), -1, dtype=t.int16, device=gpu.dev)
    nonces = t.full((n,), -7, dtype=t.int64, device=gpu.dev)
    plan2 = plan_planner(gpu, desc, 2).to(gpu.dev, records=2)
    side = t.cuda.Stream()
    graph = t.cuda.CUDAGraph(keep_graph=True)
    t.cuda.synchronize()
    with t.cuda.graph(graph, stream=side):
        gpu.batch.relay_segments(d_desc, d_to, plan2, d_in, d_out, gpu.subkeys, status, nonces=nonces, stream=side)
    t.cuda.synchronize()
    assert np.all(d_out.cpu().numpy() == SENT), "the capture ran the kernels"
    nodes, edges = _graph_topology(int(graph.raw_cuda_graph()))
    assert len(nodes) == 2 and len(edges) == 1, (len(nodes), edges)       # a single chain: nothing to run in parallel
    graph.replay()
    t.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), eager.cpu().numpy())
    assert np.array_equal(status.cpu().numpy(), st_e.cpu().numpy()[MARGIN:MARGIN + n])
    assert np.array_equal(nonces.cpu().numpy(), nn_e.cpu().numpy()[MARGIN:MARGIN + n])
    exp = _expect_batch(frames)
    out = d_out.cpu().numpy()
    for i, (_st, _n, ob) in enumerate(exp):
        o = int(desc[i]["out_off"])
        assert out[o:o + len(ob)].tobytes() == ob
