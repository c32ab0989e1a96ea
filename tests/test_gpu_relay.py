"""GPU: the CURVE relay (cz_relay_batch, cz_relay_uniform) against the CPU oracle and the receive model.

Truth never comes from the kernel under test: bodies are sealed by the oracle and damaged as
tests/rx_model.py damages them; the expected status and nonce are rx_model.frame_status /
chain_expect; the expected output body is or_curve_encode(payload, flags & 3, to.counter, direction,
key_out) over the oracle's decode, and zeros for a rejected frame.  The second yardstick is
open_batch -> seal_batch on the device, byte-equal.  Whole sentinel-filled buffers are compared: the
bytes before, between and after the bodies, owned slots past their bodies, rejected frames' slots,
and the status and nonce entries outside the call's range."""
import numpy as np
import pytest

import rx_model as rx
from cz_testlib import DESC_DTYPE, or_curve_encode, splitmix_bytes
from relay_model import relay_expect

pytestmark = pytest.mark.gpu

SENT = 0xA5
GUARD = 48                  # sentinel bytes between two bodies of a descriptor batch
MARGIN = 3                  # status / nonce entries before and after the call's range
NPAIR = 5                   # key pairs; table row 2k is pair k client-to-server, 2k + 1 server-to-client
PRECOMS = [rx.PRECOM] + [splitmix_bytes(32, 4242 + k) for k in range(1, NPAIR)]
M64 = rx.M64

# the smallest shapes that reach each code path: early rejects; the flags byte only; the block edge; the
# w03 tail (at most 16 bytes in the last block); 4129; one lane of 1025 blocks
SIZES = (0, 7, 8, 32, 33, 34, 48, 49, 64, 65, 80, 81, 96, 97, 128, 129, 161, 4129, 65569)
IN_ALIGN = (0, 1, 4, 8, 15)
OUT_ALIGN = (0, 3, 8)


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
    rows = []
    for p in PRECOMS:
        k = torch.tensor(list(p), dtype=torch.uint8, device=g.dev).view(1, 32)
        rows += [batch.subkeys(k, _lib.CZ_DIR_C2S), batch.subkeys(k, _lib.CZ_DIR_S2C)]
    g.subkeys = torch.cat(rows)
    return g


def _r(n, a):
    return (n + a - 1) // a * a


def _dev(g, a):
    return g.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(g.dev)


def _role(kidx):
    """the receiver role that opens what table row kidx sealed"""
    return rx.CLIENT if kidx & 1 else rx.SERVER


def make_body(size, nonce, flags, seed, kidx, fault=None):
    """a body sealed by the oracle under table row kidx, damaged as rx_model damages; sizes under 33 are cuts"""
    fr = rx.Frame(nonce & M64, max(size, 64) if size < 33 else size, fault, flags, seed)
    body = rx.build_body(fr, _role(kidx), PRECOMS[kidx >> 1])
    return body[:size] if size < 33 else body


def expect_frame(body, floor, check, kin, counter, kout):
    """(status word, wire nonce or None, output bytes) of one relayed frame, from the model and the oracle"""
    return relay_expect(body, floor, check, kin & 1, PRECOMS[kin >> 1], counter, kout & 1, PRECOMS[kout >> 1])


class Fr:
    """one frame of a descriptor batch"""

    def __init__(self, body, floor, kin, counter, kout, check=True, prev=-1):
        self.body, self.floor, self.kin, self.counter, self.kout, self.check, self.prev = (
            body, floor & M64, kin, counter & M64, kout, check, prev)


def _expect_batch(frames):
    out = []
    for f in frames:
        floor = rx.wire_nonce(frames[f.prev].body) if f.prev >= 0 else f.floor
        out.append(expect_frame(f.body, floor, f.check, f.kin, f.counter, f.kout))
    return out


def run_batch(g, frames, in_a=0, out_a=0, order=None, inplace=False, yardstick=False):
    """Relay `frames` with body i at a 16-byte slot start + in_a and its output at one + out_a, GUARD
    sentinel bytes around every output; compare the whole output buffer, status and nonce arrays."""
    n = len(frames)
    desc = np.zeros(n, dtype=DESC_DTYPE)
    to = np.zeros(n, dtype=g.batch.FANOUT_SUB_DTYPE)
    io, oo = 16, GUARD
    for i, f in enumerate(frames):
        desc[i] = (io + in_a, io + in_a if inplace else oo + out_a, len(f.body), f.kin, f.floor,
                   0x100 if f.check else 0, f.prev)
        to[i] = (f.counter, f.kout, 0)
        io += _r(len(f.body) + in_a, 16) + 16
        oo += _r(len(f.body) + out_a, 16) + GUARD
    hin = np.full(io + 64, 0x3C, dtype=np.uint8)
    for i, f in enumerate(frames):
        hin[int(desc[i]["in_off"]):int(desc[i]["in_off"]) + len(f.body)] = np.frombuffer(f.body, dtype=np.uint8)
    want = hin.copy() if inplace else np.full(oo + 64, SENT, dtype=np.uint8)
    exp = _expect_batch(frames)
    for i, (_st, _n, ob) in enumerate(exp):
        want[int(desc[i]["out_off"]):int(desc[i]["out_off"]) + len(ob)] = np.frombuffer(ob, dtype=np.uint8)
    d_in = _dev(g, hin)
    d_out = d_in if inplace else g.torch.full((len(want),), SENT, dtype=g.torch.uint8, device=g.dev)
    status = g.torch.full((n + 2 * MARGIN,), -1, dtype=g.torch.int16, device=g.dev)
    nonces = g.torch.full((n + 2 * MARGIN,), -7, dtype=g.torch.int64, device=g.dev)
    d_order = None if order is None else _dev(g, np.asarray(order, dtype=np.uint32)).view(g.torch.int32)
    g.batch.relay_batch(_dev(g, desc), _dev(g, to), n, d_in, d_out, g.subkeys, status[MARGIN:MARGIN + n],
                        nonces=nonces[MARGIN:MARGIN + n], order=d_order, desc_np=desc, to_np=to)
    g.torch.cuda.synchronize()
    st = status.cpu().numpy().view(np.uint16)
    nn = nonces.cpu().numpy().view(np.uint64)
    out = d_out.cpu().numpy()
    bad = []
    for i, (est, enonce, ob) in enumerate(exp):
        o = int(desc[i]["out_off"])
        if st[MARGIN + i] != est:
            bad.append(f"frame {i} (size {len(frames[i].body)}): status {st[MARGIN + i]:#x}, model {est:#x}")
        elif out[o:o + len(ob)].tobytes() != ob:
            bad.append(f"frame {i} (size {len(frames[i].body)}, status {est:#x}): output body differs")
        if enonce is not None and int(nn[MARGIN + i]) != enonce:
            bad.append(f"frame {i}: nonce {int(nn[MARGIN + i]):#x}, model {enonce:#x}")
    assert not bad, "\n".join(bad[:12])
    assert np.array_equal(out, want), "bytes outside the relayed bodies changed"
    for a in (st, nn):
        edge = np.concatenate([a[:MARGIN], a[MARGIN + n:]])
        assert np.all(edge == edge[0]) and edge[0] in (0xffff, (1 << 64) - 7), "entries outside the call's range changed"
    if yardstick and not inplace:
        _yardsticks(g, frames, desc, to, d_in, out, st[MARGIN:MARGIN + n], nn[MARGIN:MARGIN + n], exp)
    return out, st[MARGIN:MARGIN + n]


def _yardsticks(g, frames, desc, to, d_in, out, st, nn, exp):
    """open_batch -> seal_batch on the device gives the same bodies, statuses and nonces; and every
    accepted relayed body opens under the outbound key to the original payload and flags & 3"""
    n = len(frames)
    t = g.torch
    ok = (st & 0xff) == 0
    # open into payload slots, then seal them with the outbound records
    odesc = desc.copy()
    sdesc = desc.copy()
    po = 0
    for i in range(n):
        odesc[i]["out_off"] = po
        sdesc[i] = (po, desc[i]["out_off"], max(int(desc[i]["len"]), 33) - 33, to[i]["key_idx"], to[i]["counter"],
                    (int(st[i]) >> 8) & 3, -1)
        po += _r(max(int(desc[i]["len"]), 33) - 33, 16) + 16
    d_plain = t.zeros(po + 64, dtype=t.uint8, device=g.dev)
    st2 = t.full((n,), -1, dtype=t.int16, device=g.dev)
    nn2 = t.full((n,), -7, dtype=t.int64, device=g.dev)
    g.batch.open_batch(_dev(g, odesc), n, d_in, d_plain, g.subkeys, st2, nonces=nn2, desc_np=odesc)
    d_out2 = t.full((len(out),), SENT, dtype=t.uint8, device=g.dev)
    g.batch.seal_batch(_dev(g, sdesc), n, d_plain, d_out2, g.subkeys, desc_np=sdesc)
    # round trip: the relayed bodies under the outbound keys, each frame its own floor
    rdesc = desc.copy()
    for i in range(n):
        rdesc[i] = (desc[i]["out_off"], odesc[i]["out_off"], desc[i]["len"], to[i]["key_idx"],
                    (int(to[i]["counter"]) - 1) & M64, 0, -1)
    d_back = t.zeros_like(d_plain)
    st3 = t.full((n,), -1, dtype=t.int16, device=g.dev)
    g.batch.open_batch(_dev(g, rdesc), n, _dev(g, out), d_back, g.subkeys, st3, desc_np=rdesc)
    t.cuda.synchronize()
    assert np.array_equal(st2.cpu().numpy().view(np.uint16), st), "statuses differ from open_batch's"
    assert np.array_equal(nn2.cpu().numpy().view(np.uint64), nn), "nonces differ from open_batch's"
    out2, back, plain = d_out2.cpu().numpy(), d_back.cpu().numpy(), d_plain.cpu().numpy()
    st3 = st3.cpu().numpy().view(np.uint16)
    for i in range(n):
        if not ok[i]:
            continue
        o, ln, p = int(desc[i]["out_off"]), int(desc[i]["len"]), int(odesc[i]["out_off"])
        assert out[o:o + ln].tobytes() == out2[o:o + ln].tobytes(), f"frame {i}: differs from open_batch -> seal_batch"
        assert st3[i] == ((int(st[i]) >> 8) & 3) << 8, f"frame {i}: relayed body opens with status {st3[i]:#x}"
        assert back[p:p + ln - 33].tobytes() == plain[p:p + ln - 33].tobytes(), f"frame {i}: round trip payload differs"


def _size_frames(seed):
    """one frame of every size; keys cycle through all rows on both sides (equal on some frames), the
    outbound counter equals the inbound nonce on every fourth frame"""
    frames = []
    for i, size in enumerate(SIZES):
        kin, kout = (i + seed) % (2 * NPAIR), (3 * i + 1 + seed) % (2 * NPAIR)
        if i % 5 == 0:
            kout = kin
        nonce = (1 << 32) * (i + 1) + 77 + i
        counter = nonce if i % 4 == 0 else (1 << 40) + 13 * i
        frames.append(Fr(make_body(size, nonce, i & 3, 600 + 31 * seed + i, kin), nonce - 1, kin, counter, kout))
    return frames


@pytest.mark.parametrize("out_a", OUT_ALIGN)
@pytest.mark.parametrize("in_a", IN_ALIGN)
def test_sizes_and_alignments(gpu, in_a, out_a):
    """every size at every input alignment x output alignment, so (in - out) % 4 takes every value;
    against the oracle, open_batch -> seal_batch, and the round trip under the outbound key"""
    run_batch(gpu, _size_frames(in_a + out_a), in_a, out_a, yardstick=True)


def test_order_gives_the_identical_result(gpu):
    frames = _size_frames(2)
    a, sa = run_batch(gpu, frames, 1, 3)
    perm = np.random.default_rng(5).permutation(len(frames))
    b, sb = run_batch(gpu, frames, 1, 3, order=perm)
    assert np.array_equal(a, b) and np.array_equal(sa, sb)


_SMALL = (34, 96, 97, 161, 33, 80, 129)


def _fault_chain(count, kind, seed):
    """`count` frames of one connection chained by prev, `kind` at lanes 0, 1, 63, 64, 65 and the last"""
    spots = {p for p in (0, 1, 63, 64, 65, count - 1) if p < count}
    kin, kout = seed % (2 * NPAIR), (seed * 7 + 3) % (2 * NPAIR)
    floor = ((1 << 32) - 40, (1 << 63) + 7, 2)[seed % 3]
    frames, n = [], floor
    for i in range(count):
        n = (n + 1 + (i % 3 == 0)) & M64
        fault = kind if i in spots else None
        nonce = n
        if fault in ("replay", "replay_tag"):
            nonce = rx.wire_nonce(frames[i - 1].body) if i else floor
        size = _SMALL[(i + seed) % len(_SMALL)]
        body = make_body(size, nonce, i & 3, 9000 + 200 * seed + i, kin, fault)
        # a body under 16 bytes holds no whole nonce for its successor's floor: that frame takes an explicit one
        prev = i - 1 if i and len(frames[i - 1].body) >= 16 else -1
        frames.append(Fr(body, floor if i == 0 else n - 1, kin, (1 << 33) + i, kout, prev=prev))
    return frames


@pytest.mark.parametrize("count", rx.CHAIN_LENGTHS)
def test_faults(gpu, count):
    """every fault kind at lanes 0, 1, 63, 64, 65 and the last lane: the status, and zeros over exactly
    len bytes (the sentinel around them stays); the frame behind a rejected one chains to its nonce"""
    for k, kind in enumerate(rx.FAULT_KINDS):
        frames = _fault_chain(count, kind, k)
        _out, st = run_batch(gpu, frames, in_a=k % 2, out_a=(0, 3, 8)[k % 3])
        spots = [p for p in (0, 1, 63, 64, 65, count - 1) if p < count]
        want = rx.FAULT_STATUS[kind]
        # (a replay at a lane whose predecessor's nonce it repeats; "name7" and "flags_ff" are accepted)
        assert all((st[p] & 0xff) == want for p in spots), (kind, [int(st[p]) for p in spots])


def test_chains_and_signed_floor(gpu):
    """prev chains over the model's nonce runs: gaps, equal and backward nonces (a chain whose previous
    frame is rejected), and floors and nonces around 2^32 and 2^63 compared as a signed long"""
    for r, (name, (floor, nonces, statuses)) in enumerate(rx.NONCE_RUNS.items()):
        kin, kout = (2 * r + 1) % (2 * NPAIR), (r + 4) % (2 * NPAIR)
        frames = [Fr(make_body(_SMALL[i % len(_SMALL)], n, i & 3, 300 + i, kin), floor, kin, (1 << 63) - 2 + i, kout,
                     prev=i - 1) for i, n in enumerate(nonces)]
        _out, st = run_batch(gpu, frames, in_a=r % 2, yardstick=True)
        assert [int(s) & 0xff for s in st] == list(statuses), name


@pytest.mark.parametrize("in_a", (0, 5))
def test_in_place(gpu, in_a):
    """prev < 0, output over the input, aligned and unaligned, accepted and rejected frames: the buffer
    afterwards equals the expected out-of-place output, and the bytes between the bodies are unchanged"""
    frames = _size_frames(4)
    kinds = ("tag", "ct_last", "name3", "wrong_dir", "cut16", "flags_ff", "name7")
    for j, kind in enumerate(kinds):
        size = (4129, 161, 97, 257, 64, 130, 81)[j]
        kin = j % (2 * NPAIR)
        frames.append(Fr(make_body(size, 500 + j, j & 3, 70 + j, kin, kind), 499 + j, kin, 900 + j, (kin + 3) % (2 * NPAIR)))
    frames.append(Fr(make_body(200, 50, 1, 99, 2), 50, 2, 7, 3))      # SEQUENCE: nonce == floor
    run_batch(gpu, frames, in_a=in_a, inplace=True)


# ---- cz_relay_uniform -------------------------------------------------------------------------------
PAD = 256
LINE_SIZES, LANE_SIZES = (256, 257, 4129), (34, 161, 4129)
COUNTS = (1, 63, 64, 65, 257)


def _uniform_bodies(size, count, kin, nonce0, faults):
    bodies, n = [], nonce0
    for i in range(count):
        kind = faults.get(i)
        nonce = n
        if kind in ("replay", "replay_tag"):
            nonce = rx.wire_nonce(bodies[i - 1]) if i else nonce0 - 1
        bodies.append(make_body(size, nonce, i & 3, 40000 + size * 3 + i, kin, kind))
        n = (n + 1 + (i % 5 == 0)) & M64
    return bodies


def run_uniform(g, size, count, ist, ost, in_base=0, out_base=0, counter0=(5 << 32) - 10, nonce0=(3 << 32) - 20,
                check=True, kin=3, kout=6):
    """one cz_relay_uniform call over oracle bodies with rejected frames in the middle of wave 0 and, when
    the count allows, in the partial last wave; whole output buffer and status array compared"""
    faults = {p: k for p, k in ((5, "name3"), (20, "tag"), (21, "flags_ff"), (40, "replay"), (41, "name7"),
                                (62, "replay_tag"), (64, "wrong_dir"), (130, "ct_last"), (256, "tag")) if p < count}
    bodies = _uniform_bodies(size, count, kin, nonce0, faults)
    floor0 = (nonce0 - 1) & M64
    if check:
        model = rx.chain_expect(bodies, floor0, kin & 1, PRECOMS[kin >> 1])
    else:
        model = [rx.frame_status(b, 0, False, kin & 1, PRECOMS[kin >> 1]) for b in bodies]
    owns = (ost % 128 == 0 and ost < (1 << 25)) or (ost % 16 == 0 and ost <= 256)
    hin = np.full(PAD + in_base + count * ist + PAD, 0x3C, dtype=np.uint8)
    want = np.full(PAD + out_base + count * ost + PAD, SENT, dtype=np.uint8)
    want_st = np.full(count + 2 * MARGIN, 0xffff, dtype=np.uint16)
    for i, (b, (st, fl, pay, _n)) in enumerate(zip(bodies, model)):
        hin[PAD + in_base + i * ist:PAD + in_base + i * ist + size] = np.frombuffer(b, dtype=np.uint8)
        o = PAD + out_base + i * ost
        ob = bytes(size)
        if st == rx.ST_OK:
            ob = or_curve_encode(pay, fl & 3, (counter0 + i) & M64, kout & 1, PRECOMS[kout >> 1])
            want_st[MARGIN + i] = fl << 8
        else:
            want_st[MARGIN + i] = st
        want[o:o + size] = np.frombuffer(ob, dtype=np.uint8)
        if owns:
            want[o + size:o + ost] = 0
    t = g.torch
    d_in = _dev(g, hin)
    d_out = t.full((len(want),), SENT, dtype=t.uint8, device=g.dev)
    status = t.full((count + 2 * MARGIN,), -1, dtype=t.int16, device=g.dev)
    a, b = PAD + in_base, PAD + out_base
    out_end = b + (count * ost if owns else (count - 1) * ost + size)
    g.batch.relay_uniform(d_in[a:a + (count - 1) * ist + size], ist, d_out[b:out_end], ost, count, size, g.subkeys[kin],
                          floor0, g.subkeys[kout], counter0 & M64, status[MARGIN:MARGIN + count], check=check)
    t.cuda.synchronize()
    st = status.cpu().numpy().view(np.uint16)
    out = d_out.cpu().numpy()
    bad = [f"frame {i}: status {st[MARGIN + i]:#x}, model {want_st[MARGIN + i]:#x}" for i in range(count)
           if st[MARGIN + i] != want_st[MARGIN + i]]
    assert not bad, "\n".join(bad[:12])
    assert np.array_equal(st, want_st), "status entries outside the call's range changed"
    if not np.array_equal(out, want):
        diff = np.flatnonzero(out != want)
        where = [(int(d) - b) // ost if b <= d < b + count * ost else -1 for d in diff[:6]]
        pytest.fail(f"{len(diff)} output bytes differ, first at {int(diff[0]) - b} (frames {where})")
    return st[MARGIN:MARGIN + count]


# (size, out_stride): 4224 and 384 owning and line-staged; 144 owning and lane-wise; 4129 and 4136 not owning
LINE_CASES = [(256, 384), (257, 384), (256, 4224), (257, 4224), (4129, 4224)]
LANE_CASES = [(34, 144), (34, 4136), (161, 4129), (161, 4136), (161, 384), (4129, 4129), (4129, 4136)]


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("size,ost", LINE_CASES)
def test_uniform_line_path(gpu, size, ost, count):
    """everything on 16 bytes, out_stride a line multiple: full waves line-staged, the partial last wave
    lane-wise behind them; inbound nonces and outbound counters cross a multiple of 2^32 inside wave 0"""
    run_uniform(gpu, size, count, _r(size, 16) + 16, ost)


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("size,ost", LANE_CASES)
def test_uniform_lane_wise(gpu, size, ost, count):
    run_uniform(gpu, size, count, _r(size, 16), ost)


@pytest.mark.parametrize("size,ost", LINE_CASES + LANE_CASES)
def test_uniform_input_at_base_plus_1(gpu, size, ost):
    """the same layouts from bodies one byte off a 16-byte base (lane-wise whatever the stride), and from
    the dense input stride"""
    run_uniform(gpu, size, 65, _r(size, 16) + 16, ost, in_base=1)
    run_uniform(gpu, size, 130, size, ost, in_base=1)


def test_uniform_output_off_alignment(gpu):
    """an owning stride from an output base off 16 bytes: lane-wise, the slots still written whole"""
    run_uniform(gpu, 257, 65, 272, 384, out_base=8)
    run_uniform(gpu, 34, 65, 48, 144, out_base=1)


@pytest.mark.parametrize("size,ost", [(257, 384), (4129, 4224), (161, 4136)])
def test_uniform_counter_wraps(gpu, size, ost):
    """counter0 = 2^64 - 3 wraps as cz_seal_uniform wraps; inbound nonces across 2^63 are a signed step back"""
    run_uniform(gpu, size, 65, _r(size, 16), ost, counter0=(1 << 64) - 3)
    st = run_uniform(gpu, size, 64, _r(size, 16), ost, nonce0=(1 << 63) - 8)
    assert (st & 0xff).tolist().count(rx.ST_SEQUENCE) >= 2      # the step into the negative, and the replay


@pytest.mark.parametrize("size,ost", [(257, 384), (161, 4136)])
def test_uniform_without_check(gpu, size, ost):
    st = run_uniform(gpu, size, 65, _r(size, 16), ost, check=False)
    assert st[40] & 0xff == rx.ST_OK and st[62] & 0xff == rx.ST_CRYPTO     # replay accepted, replay_tag by its tag


def test_uniform_short_sizes_write_only_zeros(gpu):
    """size < 33: every frame is COMMAND or MALFORMED and only zeros are written"""
    for size, ost in ((32, 48), (8, 24), (7, 144), (20, 128)):
        hin = np.frombuffer(b"".join(make_body(64, 9 + i, 0, i, 0)[:size].ljust(32, b"\0") for i in range(70)), dtype=np.uint8)
        t = gpu.torch
        d_out = t.full((70 * ost + 64,), SENT, dtype=t.uint8, device=gpu.dev)
        status = t.full((70,), -1, dtype=t.int16, device=gpu.dev)
        gpu.batch.relay_uniform(_dev(gpu, hin), 32, d_out, ost, 70, size, gpu.subkeys[0], 1, gpu.subkeys[1], 5, status)
        t.cuda.synchronize()
        owns = (ost % 128 == 0) or (ost % 16 == 0 and ost <= 256)
        out = d_out.cpu().numpy()
        slots = out[:70 * ost].reshape(70, ost)
        assert not slots[:, :size].any() and np.all(out[70 * ost:] == SENT)
        assert np.all(slots[:, size:] == (0 if owns else SENT))
        want = rx.ST_MALFORMED if size >= 8 else rx.ST_COMMAND
        assert np.all(status.cpu().numpy().view(np.uint16) == want)
