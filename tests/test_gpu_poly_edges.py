"""GPU: the compiled Poly1305 at its reduction and carry edges, on steered inputs.

The other GPU suites feed the kernels random payloads, which reach the rare branches of a
hand-written Poly1305 -- the conditional subtraction of p, the h4 folds, all-ones carry chains in
`h + m`, `h + 5` and `h + pad`, the radix-2^26 joins of segment and thread partials, the OR of the
tag comparison -- with probability ~2^-100.  poly_steer.py solves one ciphertext block so that the
accumulator (of a frame, of each segment, of each thread of the one-launch box) ends at a chosen
residue; every inlined copy of the Horner loop, the final partial block and the tag step gets
every target: the uniform / descriptor seal and open lanes, the segment kernels with combine_tag,
and k_nacl_one with keystream keys and with caller-chosen keys (maximal, zero, power-of-two r).

All comparisons are bit-exact against bodies whose tag is the big-integer poly_steer.poly1305 and
which the oracle reproduces (asserted while the inputs are built).
"""
import ctypes
import functools
import random
from contextlib import contextmanager, nullcontext

import numpy as np
import pytest

import poly_steer as ps
from cz_testlib import DESC_DTYPE, load_golden, or_box_afternm, or_curve_encode

pytestmark = pytest.mark.gpu

G = load_golden()
PRECOM = bytes.fromhex(G["keys"]["precom"])
COUNTER0 = 0x0000_0001_FFFF_FF9C   # the high nonce word changes at frame 100: wave 1 of a batch is not uniform


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch, torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    from jeromq_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def subkeys(torch_dev, L):
    torch, dev = torch_dev
    from jeromq_amd import batch
    k = torch.tensor(list(PRECOM), dtype=torch.uint8, device=dev).view(1, 32)
    return torch.cat([batch.subkeys(k, L.CZ_DIR_C2S), batch.subkeys(k, L.CZ_DIR_S2C)])


@contextmanager
def _knob(L, name, value):
    lib = L.lib()
    old = lib.cz_tune(name, value)
    assert old >= 0
    try:
        yield
    finally:
        lib.cz_tune(name, old)


def _xor(a, b):
    assert len(a) == len(b)
    return (int.from_bytes(a, "little") ^ int.from_bytes(b, "little")).to_bytes(len(a), "little")


def _r16(n):
    return max(16, (n + 15) // 16 * 16)


def _r128(n):
    return max(128, (n + 127) // 128 * 128)


def _dev(torch_dev, a):
    torch, dev = torch_dev
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)


class Frame:
    """A MESSAGE whose ciphertext is steered: payload / flags / counter to seal, body to open"""

    def __init__(self, name, counter, msg, direction=0):
        ks = ps.message_keystream(PRECOM, direction, counter, 32 + len(msg))
        self.name, self.counter, self.key = name, counter, ks[:32]
        plain = _xor(msg, ks[32:])
        self.flags, self.payload = plain[0], plain[1:]
        self.tag = ps.poly1305(msg, self.key)
        self.body = b"\x07MESSAGE" + counter.to_bytes(8, "big") + self.tag + msg
        assert or_curve_encode(self.payload, self.flags, counter, direction, PRECOM) == self.body, name


def _frame_key_head(counter, flags):
    ks = ps.message_keystream(PRECOM, 0, counter, 33)
    return ks[:32], bytes([ks[32] ^ flags])


def _specs(mac_len):
    """what a frame's accumulator is steered to: every final target, and the h + m ripples"""
    out = [(name, f, None) for name, f in ps.TARGETS]
    if mac_len >= 48:
        out += [(f"h+m-ripple-{x}", None, x) for x in (0, 3)]
    return out


# The uniform kernels stage whole waves of 64 frames (the LINES / SHIFT / REGION emitters, the
# dword-aligned INA loads, the carry kernel) and send the frames of a partial last wave through the
# lane-wise direct code.  So every uniform batch here is three full waves and a partial one, and the
# specs (at most 50) cycle through it: each full wave and the tail see every spec.
SEAL_FRAMES = 3 * 64 + 50          # tail: 50 consecutive frames = every spec
OPEN_FRAMES = 3 * 64 - 8 + 50      # + 8 tampered in front (wave 0) + 8 at the end (the tail of 58)


@functools.lru_cache(maxsize=None)
def uniform_frames(n):
    """SEAL_FRAMES frames of payload n bytes, the specs cycled, counters COUNTER0 + i"""
    rng = random.Random(1000 + n)
    specs = _specs(n + 1)
    assert len(specs) <= 50
    frames = []
    for i in range(SEAL_FRAMES):
        name, f, x = specs[i % len(specs)]
        key, head = _frame_key_head(COUNTER0 + i, i & 3)
        if f is not None:
            msg = ps.steer(key, n + 1, f(ps.key_s(key)), rng, head)
        else:
            msg = ps.hm_ripple(key, n + 1, x, rng, head)
        frames.append(Frame(name, COUNTER0 + i, msg))
        assert frames[-1].flags == i & 3
    return frames


def _tag_tampered(frames):
    """(frame, body) with one bit flipped in each of the four tag words, for the frames whose tag
    is all zero / all ones: a tag comparison that skips a word accepts one of them"""
    out = []
    for fr in frames:
        if fr.tag in (bytes(16), b"\xff" * 16):
            for w in range(4):
                bad = bytearray(fr.body)
                bad[16 + 4 * w + (w + 1) % 4] ^= 1 << (2 * w + 1)
                out.append((fr, bytes(bad)))
    return out


UNIFORM_LENS = [31, 32, 46, 47, 95, 96, 4063]


# ---- uniform / descriptor seal ------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["slots128", "dense_out", "unaligned_in", "box", "batch"])
@pytest.mark.parametrize("n", UNIFORM_LENS)
def test_seal_steered_frames(torch_dev, subkeys, n, layout):
    """Three full waves (staged: whole-line / byte-shifted / region emitters by the output stride;
    "unaligned_in" with dword-aligned loads in k_seal_uniform_ina from 64 payload bytes up, the
    plain kernel's unaligned loads below) and a tail of 50 frames on the lane-wise direct code."""
    torch, dev = torch_dev
    from jeromq_amd import batch
    frames = uniform_frames(n)
    count = len(frames)
    assert count % 64 and count > 3 * 64 and {fr.tag for fr in frames} >= {bytes(16), b"\xff" * 16}
    flags = torch.tensor([fr.flags for fr in frames], dtype=torch.uint8, device=dev)
    base, in_stride, out_stride = 0, _r16(n), _r128(n + 33)
    if layout == "dense_out":
        out_stride = n + 33
    elif layout == "unaligned_in":
        base, in_stride = 1, n + 1 + n % 2   # odd stride: every byte phase
    elif layout == "box":
        in_stride = _r16(n + 33)
    hin = np.full(base + count * in_stride + 64, 0x5C, dtype=np.uint8)   # box bytes 0..31: garbage
    for i, fr in enumerate(frames):
        o = base + i * in_stride
        data = bytes([fr.flags]) + fr.payload if layout == "box" else fr.payload
        o += 32 if layout == "box" else 0
        hin[o:o + len(data)] = np.frombuffer(data, dtype=np.uint8)
    d_in = torch.from_numpy(hin).to(dev)
    d_out = torch.full((count * out_stride + 64,), 0xA5, dtype=torch.uint8, device=dev)
    if layout == "box":
        batch.seal_uniform_box(d_in, in_stride, d_out, out_stride, count, n, subkeys[0], COUNTER0)
    elif layout == "batch":
        desc = np.zeros(count, dtype=DESC_DTYPE)
        for i, fr in enumerate(frames):
            desc[i] = (i * in_stride, i * out_stride, n, 0, fr.counter, fr.flags, -1)
        batch.seal_batch(_dev(torch_dev, desc), count, d_in, d_out, subkeys, desc_np=desc)
    else:
        batch.seal_uniform(d_in[base:], in_stride, d_out, out_stride, count, n, subkeys[0], COUNTER0, flags8=flags)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    bad = [i for i, fr in enumerate(frames) if out[i * out_stride:i * out_stride + n + 33].tobytes() != fr.body]
    assert not bad, _where(bad, count, [frames[i].name for i in bad])


def _where(bad, count, names):
    """which code a batch's wrong frames ran on: the staged full waves or the lane-wise tail"""
    tail = count // 64 * 64
    return (f"{len(bad)} frames wrong: {sum(i < tail for i in bad)} in the full waves, "
            f"{sum(i >= tail for i in bad)} in the tail; first {names[:4]}")


# ---- open ---------------------------------------------------------------------------------------
def _check_open(L, items, st, plain, out_off, n):
    """items: (frame, body, tampered)"""
    bad = []
    for i, (fr, body, tampered) in enumerate(items):
        p = plain[out_off(i):out_off(i) + n]
        if tampered:   # rejected, and nothing of the plaintext left behind
            ok = st[i] & 0xff == L.CZ_STATUS_CRYPTO and not p.any()
        else:
            ok = st[i] & 0xff == L.CZ_STATUS_OK and st[i] >> 8 == fr.flags and p.tobytes() == fr.payload
        if not ok:
            bad.append(i)
    assert not bad, _where(bad, len(items), [f"{items[i][0].name}{' (tampered tag)' if items[i][2] else ''}: status "
                                             f"{int(st[i]):#x}" for i in bad])


def _open_items(n):
    """8 tampered bodies, OPEN_FRAMES good ones, the 8 tampered again: 3 full waves (the tampered in
    wave 0) and a tail of 58 (50 good = every spec, and the tampered)"""
    frames = uniform_frames(n)[:OPEN_FRAMES]
    bad = [(fr, body, True) for fr, body in _tag_tampered(frames[:len(_specs(n + 1))])]
    assert len(bad) == 8
    items = bad + [(fr, fr.body, False) for fr in frames] + bad
    assert len(items) == 3 * 64 + 58
    return items


def _open_cases():
    """(n, layout, knob, value).  The knobs only where they select other device code: "open_ina"
    for bodies off 16-byte alignment under cz_open_uniform (cz_open_batch has no knob, 16-byte
    aligned slots take neither); "open_carry" where the carry kernel can run at all, which needs
    256 payload bytes: of these lengths 4063 alone (8-byte aligned bodies: on / off; any byte
    offset: the A/B value 2)."""
    out = []
    for n in UNIFORM_LENS:
        out += [(n, "batch", None, None), (n, "batch_unaligned", None, None), (n, "slots", None, None),
                (n, "dense8", b"open_ina", 1), (n, "dense8", b"open_ina", 0),
                (n, "dense1", b"open_ina", 1), (n, "dense1", b"open_ina", 0)]
        if n >= 256:
            out += [(n, "dense8", b"open_carry", 1), (n, "dense8", b"open_carry", 0), (n, "dense1", b"open_carry", 2)]
    return out


@pytest.mark.parametrize("n,layout,knob,value", _open_cases())
def test_open_steered_frames(torch_dev, subkeys, L, n, layout, knob, value):
    """Every steered frame opens OK with its payload and flags; the all-zero and all-ones tags with
    one bit flipped in each tag word are rejected with a zeroed payload, in a full (staged) wave
    and in the partial last wave (lane-wise code).  dense8 at 4063 bytes (bodies 4096 apart from
    an 8-byte aligned base: line phase period 1) runs its three whole waves through the
    phase-sorted carry kernel and the tail through the second launch."""
    torch, dev = torch_dev
    from jeromq_amd import batch
    size = n + 33
    items = _open_items(n)
    count = len(items)
    base = 0
    in_stride = {"batch": _r16(size), "batch_unaligned": size + 2 - size % 2 + 1, "slots": _r128(size),
                 "dense8": (size + 7) // 8 * 8, "dense1": size + size % 2 + 1}[layout]
    if layout == "dense8":
        base = 8 if in_stride % 16 == 0 else 0
    elif layout in ("dense1", "batch_unaligned"):
        base = 3
    out_stride = _r128(n) if layout != "batch" else _r16(n)
    hin = np.zeros(base + count * in_stride + 64, dtype=np.uint8)
    for i, (_, body, _) in enumerate(items):
        hin[base + i * in_stride:base + i * in_stride + size] = np.frombuffer(body, dtype=np.uint8)
    d_in = torch.from_numpy(hin).to(dev)
    d_plain = torch.full((count * out_stride + 64,), 0xEE, dtype=torch.uint8, device=dev)
    status = torch.full((count,), -1, dtype=torch.int16, device=dev)
    with _knob(L, knob, value) if knob else nullcontext():
        if layout.startswith("batch"):
            desc = np.zeros(count, dtype=DESC_DTYPE)
            for i in range(count):
                desc[i] = (base + i * in_stride, i * out_stride, size, 0, 0, 0, -1)
            batch.open_batch(_dev(torch_dev, desc), count, d_in, d_plain, subkeys, status, desc_np=desc)
        else:
            batch.open_uniform(d_in[base:], in_stride, d_plain, out_stride, count, size, subkeys[0], 0, status,
                               check=False)
        torch.cuda.synchronize()
    _check_open(L, items, status.cpu().numpy().view(np.uint16), d_plain.cpu().numpy(), lambda i: i * out_stride, n)


# ---- segments -----------------------------------------------------------------------------------
# cuts of a frame's box blocks [0, nblk): every segment after the first starts at block >= 2 (the
# open's rule); equal middle segments, and a middle segment of another length (its own f26_pow);
# "unsplit": one segment with no partial record, the tag step inlined in the segment kernels;
# "one": one segment with a record that the combine kernel finishes
SEG_SHAPES = {"unsplit": None, "one": [], "two": [3], "two_late": [7], "three": [2, 5], "four_equal": [2, 4, 6], "four_uneven": [2, 5, 7],
              "four_uneven_first_mid": [3, 4, 6]}


def _seg_pieces(cuts, mac_len):
    """MAC'd bytes per segment: box block b holds box bytes [64 b, 64 b + 64), the MAC covers box
    bytes >= 32"""
    edges = [0] + list(cuts or []) + [(mac_len + 32 + 63) // 64]
    lens = []
    for a, b in zip(edges, edges[1:]):
        lens.append(min(64 * b, mac_len + 32) - max(64 * a, 32))
    assert sum(lens) == mac_len and all(x > 0 for x in lens)
    return edges, lens


@functools.lru_cache(maxsize=None)
def segment_frames():
    """Frames of 8..12 box blocks, one per (shape, target): every segment's partial record on an edge
    residue (ps.PARTIALS), the joined accumulator on the target; plus, per shape, the inputs on which
    f26_to32 carries out of limb 4 (ps.steer_carry_out), and for one-segment records the residues
    2^53 + e and 2^79 + e the device holds with h4 = 4 and all-ones low limbs."""
    rng = random.Random(26)
    frames, plans = [], []
    ctr = COUNTER0

    def add(name, cuts, mac_len, make):
        nonlocal ctr
        key, head = _frame_key_head(ctr, len(frames) & 3)
        edges, lens = _seg_pieces(cuts, mac_len)
        frames.append(Frame(name, ctr, make(key, lens, head)))
        plans.append(None if cuts is None else edges)
        ctr += 1

    for si, (shape, cuts) in enumerate(SEG_SHAPES.items()):
        for j, (name, f) in enumerate(ps.TARGETS):
            mac_len = 64 * (7 + (j + si) % 5) + [1, 16, 17, 33, 48, 63, 64][j % 7] - 32
            parts = [ps.PARTIALS[(j + i) % len(ps.PARTIALS)] for i in range(len(cuts or []))]
            add(f"{shape}/{name}", cuts, mac_len,
                lambda key, lens, head: ps.steer_pieces(key, lens, parts, f(ps.key_s(key)), rng, head))
        if cuts:
            for k in range(1, 6):
                add(f"{shape}/to32-carry-out-{k}", cuts, 64 * 9 + 32 + 7 * k,
                    lambda key, lens, head: ps.steer_carry_out(key, lens, k, rng, head)[0])
        else:
            for e in range(5):
                for hi in (53, 79):
                    add(f"{shape}/one-record-2^{hi}+{e}", cuts, 64 * 8 + 5 + e,
                        lambda key, lens, head: ps.steer(key, lens[0], (1 << hi) + e, rng, head))
    return frames, plans


def _segment_plan(torch_dev, desc, plans, open_):
    """A caller-built plan: every frame split at its own cuts, one combine record per frame (a
    one-segment frame too: its record goes through the combine kernel)"""
    torch, dev = torch_dev
    from jeromq_amd import batch
    plan = batch.SegmentPlan(desc[:1], open_=open_)
    segs, combs, npart = [], [], 0
    for f, edges in enumerate(plans):
        if edges is None:
            segs.append((f, 0, (int(desc[f]["len"]) + (0 if open_ else 33) + 63) // 64, 0xFFFFFFFF))
            continue
        combs.append((f, npart, len(edges) - 1, 0))
        for s in range(len(edges) - 1):
            segs.append((f, edges[s], edges[s + 1] - edges[s], npart + s))
        npart += len(edges) - 1
    plan.segments = np.array(segs, dtype=batch.SEGMENT_DTYPE)
    plan.combines = np.array(combs, dtype=batch.COMBINE_DTYPE)
    plan.nseg, plan.ncomb, plan.npart = len(segs), len(combs), npart
    return plan.to(dev)


@pytest.mark.parametrize("seglines", [1, 0])
def test_seal_segments_steered_partials(torch_dev, subkeys, L, seglines):
    torch, dev = torch_dev
    from jeromq_amd import batch
    frames, plans = segment_frames()
    desc = np.zeros(len(frames), dtype=DESC_DTYPE)
    io = oo = 0
    for i, fr in enumerate(frames):
        desc[i] = (io, oo, len(fr.payload), 0, fr.counter, fr.flags, -1)
        io += _r16(len(fr.payload))
        oo += _r128(len(fr.body))
    hin = np.zeros(io + 64, dtype=np.uint8)
    for i, fr in enumerate(frames):
        hin[int(desc[i]["in_off"]):int(desc[i]["in_off"]) + len(fr.payload)] = np.frombuffer(fr.payload, dtype=np.uint8)
    plan = _segment_plan(torch_dev, desc, plans, False)
    d_out = torch.zeros(oo + 64, dtype=torch.uint8, device=dev)
    with _knob(L, b"seglines", seglines):
        batch.seal_segments(_dev(torch_dev, desc), plan, _dev(torch_dev, hin), d_out, subkeys, desc_np=desc)
        torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    for i, fr in enumerate(frames):
        o = int(desc[i]["out_off"])
        got = out[o:o + len(fr.body)].tobytes()
        assert got[:32] == fr.body[:32], f"{fr.name}: tag {got[16:32].hex()} != {fr.tag.hex()}"
        assert got == fr.body, fr.name


@pytest.mark.parametrize("seglines", [1, 0])
def test_open_segments_steered_partials(torch_dev, subkeys, L, seglines):
    torch, dev = torch_dev
    from jeromq_amd import batch
    frames, plans = segment_frames()
    bad = _tag_tampered(frames)
    assert len(bad) >= 8 * len(SEG_SHAPES)
    items = [(fr, fr.body, False) for fr in frames] + [(fr, body, True) for fr, body in bad]
    plans = plans + [plans[frames.index(fr)] for fr, _ in bad]
    desc = np.zeros(len(items), dtype=DESC_DTYPE)
    io = oo = 0
    for i, (fr, body, _) in enumerate(items):
        desc[i] = (io, oo, len(body), 0, 0, 0, -1)
        io += _r16(len(body))
        oo += _r16(len(fr.payload))
    hin = np.zeros(io + 64, dtype=np.uint8)
    for i, (_, body, _) in enumerate(items):
        hin[int(desc[i]["in_off"]):int(desc[i]["in_off"]) + len(body)] = np.frombuffer(body, dtype=np.uint8)
    plan = _segment_plan(torch_dev, desc, plans, True)
    d_plain = torch.full((oo + 64,), 0xA5, dtype=torch.uint8, device=dev)
    status = torch.full((len(items),), -1, dtype=torch.int16, device=dev)
    with _knob(L, b"seglines", seglines):
        batch.open_segments(_dev(torch_dev, desc), plan, _dev(torch_dev, hin), d_plain, subkeys, status, desc_np=desc)
        torch.cuda.synchronize()
    st, plain = status.cpu().numpy().view(np.uint16), d_plain.cpu().numpy()
    for i, (fr, body, tampered) in enumerate(items):
        p = plain[int(desc[i]["out_off"]):int(desc[i]["out_off"]) + len(fr.payload)]
        if tampered:
            assert st[i] & 0xff == L.CZ_STATUS_CRYPTO, f"{fr.name}: tampered tag accepted"
            assert not p.any(), f"{fr.name}: rejected frame leaked plaintext"
        else:
            assert st[i] & 0xff == L.CZ_STATUS_OK, f"{fr.name}: status {st[i]:#x}"
            assert st[i] >> 8 == fr.flags and p.tobytes() == fr.payload, fr.name


# ---- k_nacl_one -----------------------------------------------------------------------------------
NACL_SIZES = [64, 65, 128, 129, 64 * 256, 64 * 256 + 1, 64 * 513, 81921]
NACL_T = 256      # k_nacl_one: threads, thread t owns box blocks [t w, t w + w), w = ceil(nblk / 256)
MUST = ("freeze+0", "freeze+4", "freeze-p-1", "pad-tag-zero", "pad-tag-ones", "fold-2^96+4", "h4-1*2^128+0")


def _thread_pieces(mlen):
    nblk = (mlen + 63) // 64
    w = (nblk + NACL_T - 1) // NACL_T
    last = (nblk - 1) // w
    lens = [min(64 * w * (t + 1), mlen) - max(64 * w * t, 32) for t in range(last + 1)]
    assert sum(lens) == mlen - 32 and all(x > 0 for x in lens)
    return lens


def _targets_for(mlen, salt=0):
    """every target at the small sizes; at the large ones a rotating quarter plus the rarest"""
    if mlen <= 129:
        return list(ps.TARGETS)
    return [t for j, t in enumerate(ps.TARGETS) if t[0] in MUST or (j + salt) % 4 == 0]


@pytest.mark.parametrize("mlen", NACL_SIZES)
def test_nacl_one_steered_thread_partials(L, torch_dev, mlen):
    """cz_box_afternm / cz_box_open_afternm with a zero prefix (the MAC key is the keystream): every
    thread's partial on an edge residue, the joined accumulator on each target; at the sizes whose
    last thread holds two MAC blocks also the inputs on which f26_to32 carries out of limb 4."""
    lib = L.lib()
    rng = random.Random(mlen)
    k = rng.randbytes(32)
    lens = _thread_pieces(mlen)
    cases = [(name, f, None) for name, f in _targets_for(mlen, mlen)]
    if len(lens) >= 2 and lens[-1] >= 32:
        cases += [(f"to32-carry-out-{c}", None, c) for c in range(1, 6)]
    # the knob pins the one-launch kernel for the two-pass size whatever the library's threshold is
    with _knob(L, b"nacl_one_max", 1 << 22):
        _nacl_steered_cases(lib, rng, k, mlen, lens, cases)


def _nacl_steered_cases(lib, rng, k, mlen, lens, cases):
    for j, (name, f, carry) in enumerate(cases):
        n24 = rng.randbytes(24)
        ks = ps.box_keystream(k, n24, mlen)
        key = ks[:32]
        if carry:
            msg = ps.steer_carry_out(key, lens, carry, rng)[0]
        else:
            parts = [ps.PARTIALS[(j + t) % len(ps.PARTIALS)] for t in range(len(lens) - 1)]
            msg = ps.steer_pieces(key, lens, parts, f(ps.key_s(key)), rng)
        tag = ps.poly1305(msg, key)
        m = bytes(32) + _xor(msg, ks[32:])
        want = bytes(16) + tag + msg
        assert or_box_afternm(m, n24, k) == (0, want), name
        c = ctypes.create_string_buffer(mlen)
        assert lib.cz_box_afternm(c, m, mlen, n24, k) == 0, name
        assert c.raw[16:32] == tag, f"{name}: tag {c.raw[16:32].hex()} != {tag.hex()}"
        assert c.raw == want, name
        back = ctypes.create_string_buffer(mlen)
        assert lib.cz_box_open_afternm(back, want, mlen, n24, k) == 0, f"{name}: open rejected a good box"
        assert back.raw == m, name
        if tag in (bytes(16), b"\xff" * 16):
            for w in range(4):
                bad = bytearray(want)
                bad[16 + 4 * w + w] ^= 0x10 << (w % 4)
                sentinel = ctypes.create_string_buffer(b"\xaa" * mlen, mlen)
                assert lib.cz_box_open_afternm(sentinel, bytes(bad), mlen, n24, k) == -1, f"{name}: tag word {w}"
                assert sentinel.raw == b"\xaa" * mlen


def _limb(i, v):
    return (v << (32 * i)).to_bytes(16, "little")


CHOSEN_R = [("clamp-all-ones", b"\xff" * 16), ("zero", bytes(16)), ("one", _limb(0, 1)), ("two", _limb(0, 2)),
            ("4*2^32", _limb(1, 4)), ("2^124", _limb(3, 1 << 28)), ("2^123", _limb(3, 1 << 27)),
            ("limb0-max", _limb(0, 0x0FFFFFFC)), ("limb1-max", _limb(1, 0x0FFFFFFC)),
            ("limb2-max", _limb(2, 0x0FFFFFFC)), ("limb3-max", _limb(3, 0x0FFFFFFC))]


@pytest.mark.parametrize("mlen", NACL_SIZES)
def test_nacl_one_chosen_keys(L, torch_dev, mlen):
    """cz_box_afternm and cz_secretbox with m[0:32] != 0: NaCl keys the MAC with c[0:32], so
    m = keystream ^ (K32 || M) makes the device compute Poly1305(K32, M) for r maximal, zero, 1, 2,
    4 * 2^32, 2^124 (key bytes: the clamp takes that bit, so r = 0 again), 2^123 (the top bit a
    clamped r can have) and each single limb at its clamp, s zero and all ones, M all ff, all zero
    and steered to every target: the whole product.  The steered messages of one key share their
    bytes up to the last 272..287, so a key's accumulator over them is computed once.

    Under r = 1, 2, 4 * 2^32, ... the accumulator is nearly the plain sum of the blocks, and with the
    few blocks of the small boxes (under 17 MAC blocks) some residues have no preimage or very
    rare ones: there, and nowhere else, a target may fail to steer.  What ran is recorded: every
    target is sealed under the maximal r at every size, and from 17 MAC blocks up under every
    non-zero r."""
    lib = L.lib()
    rng = random.Random(7 * mlen)
    k, n24 = rng.randbytes(32), rng.randbytes(24)
    ks = ps.box_keystream(k, n24, mlen)
    nmsg = mlen - 32
    ntail = min(nmsg, 272 + nmsg % 16)
    bulk = rng.randbytes(nmsg - ntail)
    ran = {}
    for rname, rbytes in CHOSEN_R:
        for sbytes in (bytes(16), b"\xff" * 16):
            key32 = rbytes + sbytes
            s = ps.key_s(key32)
            hb = ps.accumulate(bulk, key32)
            msgs = [("ff", b"\xff" * nmsg), ("zero", bytes(nmsg))]
            for name, f in ps.TARGETS if ps.key_r(key32) else ():
                try:
                    msgs.append((name, bulk + ps.steer_from(key32, hb, ntail, f(s), rng)))
                    ran.setdefault(rname, set()).add(name)
                except RuntimeError:
                    assert nmsg < 272 and rname != "clamp-all-ones", (rname, name, nmsg)
            for name, msg in msgs:
                m = _xor(ks, key32 + msg)
                # the big-integer reference, continued from the shared bytes' accumulator
                h = ps.accumulate(msg[len(bulk):], key32, hb) if msg.startswith(bulk) and bulk else ps.accumulate(msg, key32)
                tag = ((h + s) & ps.M128).to_bytes(16, "little")
                want = bytes(16) + tag + msg
                assert or_box_afternm(m, n24, k) == (0, want)
                for fn in (lib.cz_box_afternm, lib.cz_secretbox):
                    c = ctypes.create_string_buffer(b"\x5a" * mlen, mlen)
                    assert fn(c, m, mlen, n24, k) == 0
                    assert c.raw[16:32] == tag, f"r {rname}, s {sbytes[:1].hex()}, M {name}: tag {c.raw[16:32].hex()}"
                    assert c.raw == want, f"r {rname}, M {name}"
    every = {name for name, _ in ps.TARGETS}
    assert ran["clamp-all-ones"] == every
    assert set(ran) == {rname for rname, rb in CHOSEN_R if ps.key_r(rb + bytes(16))}
    if nmsg >= 272:
        assert all(v == every for v in ran.values())
