"""GPU: the device address arithmetic at its stride limits and past 4 GiB.

The hot stores of this library are buffer stores with a 32-bit per-lane offset from a wave-uniform
base, and each emitter is only correct because a launcher, or the kernel itself, keeps an offset
below a bound ("32-bit offset bounds").  The other suites use strides of a few
KiB and outputs that lie together, so a wrong bound never shows there; it would not show as a wrong
tag either, but as a body written over a neighbour or outside the batch.  Every case here sits on
one of those bounds -- the largest stride a staged emitter accepts, the first one it refuses, the
last and first output offsets on either side of the WaveRel window -- with frame offsets that cross
2^32 bytes, and checks BYTES only:

  - the bodies / payloads, gathered on the device into one small tensor, against the CPU oracle
    (cz_testlib.or_curve_encode);
  - the slot padding, through a strided view on the device: exactly zero where the batch owns its
    slots, exactly the sentinel the buffer was filled with where it does not (the predicates below
    are the ownership rule of include/curvezmq_mi355x.h, sections 3 and 3c);
  - a 64 MiB guard region of the sentinel in front of and behind every batch, inside the same
    allocation: a wrapped 32-bit offset lands near the batch, not at random.  The scattered layouts
    (segments, descriptors, v2 copies) go further: their outputs are overwritten with the sentinel
    after the comparison and the whole allocation must then be the sentinel.

Which kernel or emitter served a layout cannot be observed through bytes and is not checked: a
refused stride must simply give the same bytes lane by lane.  The path selection itself
(pick_staging, czk_seal_uniform / czk_open_uniform / czk_seal_fanout, WaveRel::init, fanout_owns)
was checked by reading the launchers when these cases were chosen.

No test holds more than 9 GiB of device memory; multi-GiB buffers never travel to the host.
"""
import ctypes
import functools
from contextlib import ExitStack, contextmanager

import numpy as np
import pytest

from cz_testlib import DESC_DTYPE, load_golden, or_curve_encode, splitmix_bytes, v2_encode

pytestmark = pytest.mark.gpu

G = load_golden()
PRECOM = bytes.fromhex(G["keys"]["precom"])
SENT = 0xA7                 # what every output buffer is filled with
GUARD = 64 << 20            # sentinel region in front of and behind every batch
COUNTER0 = 0x0000_0002_0000_0005
N = 351                     # payload bytes of the stride-limit cases: a 384-byte body, three lines


# ---- the ownership rule of the header after this change, by the stride alone ----------------------
def _owns(out_stride):
    return (out_stride % 128 == 0 and out_stride < (1 << 25)) or (out_stride % 16 == 0 and out_stride <= 256)


def seal_uniform_owns(out_stride):
    """cz_seal_uniform / cz_seal_uniform_box (header section 3)"""
    return _owns(out_stride)


def open_uniform_owns(out_stride):
    """cz_open_uniform (header section 3)"""
    return _owns(out_stride)


def fanout_owns(out_stride):
    """cz_seal_fanout / a run of cz_seal_fanout_runs (header section 3c)"""
    return _owns(out_stride)


# ---- fixtures and device helpers ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if torch.cuda.get_device_properties(0).total_memory < (16 << 30):
        pytest.skip("device has less than 16 GiB in total")
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


@pytest.fixture(autouse=True)
def _free_device_memory(torch_dev):
    yield
    torch_dev[0].cuda.empty_cache()


@contextmanager
def _knobs(L, **kv):
    lib = L.lib()
    with ExitStack() as st:
        for name, value in kv.items():
            old = lib.cz_tune(name.encode(), value)
            assert old >= 0, name
            st.callback(lib.cz_tune, name.encode(), old)
        yield


def _sentinel(torch_dev, nbytes):
    torch, dev = torch_dev
    buf = torch.full((nbytes,), SENT, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 128 == 0
    return buf


def _rows(torch_dev, buf, base, stride, count, width):
    """rows i = buf[base + i * stride : +width], a view"""
    assert base + (count - 1) * stride + width <= buf.numel()
    return torch_dev[0].as_strided(buf, (count, width), (stride, 1), base)


def _put(torch_dev, buf, base, stride, rows):
    torch, dev = torch_dev
    rows = np.array(rows, dtype=np.uint8, order="C")    # (a writable copy: the oracle's arrays are shared)
    _rows(torch_dev, buf, base, stride, rows.shape[0], rows.shape[1]).copy_(torch.from_numpy(rows).to(dev))


def _get(torch_dev, buf, base, stride, count, width):
    return _rows(torch_dev, buf, base, stride, count, width).contiguous().cpu().numpy()


def _all(view, value):
    """every byte of a device view equals value (two reductions, no temporary of the view's size)"""
    return view.numel() == 0 or (int(view.min()) == value and int(view.max()) == value)


def _check_slots(torch_dev, buf, base, stride, count, width, owns, what):
    """padding of `count` slots by the ownership rule, and the guards around them"""
    if stride > width:
        pad = _rows(torch_dev, buf, base + width, stride, count, stride - width)
        assert _all(pad, 0 if owns else SENT), f"{what}: slot padding is not all {'zero' if owns else 'sentinel'}"
    assert _all(buf[:base], SENT), f"{what}: bytes in front of the batch were written"
    assert _all(buf[base + count * stride:], SENT), f"{what}: bytes behind the batch were written"


def _at(torch_dev, offs, width):
    """index tensor of the bytes [o, o + width) for every o in offs"""
    torch, dev = torch_dev
    o = torch.from_numpy(np.asarray(offs, dtype=np.int64)).to(dev)
    return o[:, None] + torch.arange(width, device=dev, dtype=torch.int64)[None, :]


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    bad = np.nonzero(np.any(got != want, axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(want)} rows differ, first {bad[:6].tolist()}"


# ---- oracle frames, computed once per shape ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _frames(n, count, counter0=COUNTER0):
    """(payloads (count, n), flags (count,), bodies (count, n + 33)) of one connection direction"""
    pay = np.frombuffer(splitmix_bytes(count * n, 0xADD2E55 + n), dtype=np.uint8).reshape(count, n)
    flags = (np.arange(count) % 4).astype(np.uint8)
    bodies = np.stack([np.frombuffer(or_curve_encode(pay[i].tobytes(), int(flags[i]), counter0 + i, 0, PRECOM),
                                     dtype=np.uint8) for i in range(count)])
    for a in (pay, flags, bodies):
        a.setflags(write=False)
    return pay, flags, bodies


def _dev_u8(torch_dev, a):
    torch, dev = torch_dev
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)


# ---- cases 1 and 2: uniform seal at the LINES and SHIFT limits --------------------------------------------
def _seal_uniform_case(torch_dev, subkeys, n, count, out_stride, in_stride, in_base, box=False):
    torch, dev = torch_dev
    from jeromq_amd import batch
    pay, flags, bodies = _frames(n, count)
    d_in = _sentinel(torch_dev, in_base + count * in_stride + 64)
    if box:     # 0^32 || flags || payload; the 32 leading bytes are not read and stay the sentinel
        _put(torch_dev, d_in, in_base + 32, in_stride, np.concatenate([flags[:, None], pay], axis=1))
    else:
        _put(torch_dev, d_in, in_base, in_stride, pay)
    buf = _sentinel(torch_dev, GUARD + count * out_stride + GUARD)
    if box:
        batch.seal_uniform_box(d_in[in_base:], in_stride, buf[GUARD:], out_stride, count, n, subkeys[0], COUNTER0)
    else:
        batch.seal_uniform(d_in[in_base:], in_stride, buf[GUARD:], out_stride, count, n, subkeys[0], COUNTER0,
                           flags8=_dev_u8(torch_dev, flags))
    torch.cuda.synchronize()
    what = f"seal n={n} out_stride={out_stride} in_stride={in_stride}"
    _same(_get(torch_dev, buf, GUARD, out_stride, count, n + 33), bodies, what)
    _check_slots(torch_dev, buf, GUARD, out_stride, count, n + 33, seal_uniform_owns(out_stride), what)


# 130 = two full waves and a tail of two; frame 128 starts past 2^32 bytes from the base.  The first
# stride is the largest the line emitter takes (64 * stride < 2^31), the second must go lane by lane,
# and there the payload slots are 2^25 + 16 apart as well, so i * in_stride crosses 2^32 too.
@pytest.mark.parametrize("box", [False, True], ids=["payload", "box"])
@pytest.mark.parametrize("out_stride,in_stride", [((1 << 25) - 128, 352), (1 << 25, (1 << 25) + 16)],
                         ids=["2^25-128", "2^25"])
def test_seal_uniform_lines_limit(torch_dev, subkeys, out_stride, in_stride, box):
    if box and in_stride == 352:
        in_stride = 416     # a box is n + 33 = 384 bytes
    _seal_uniform_case(torch_dev, subkeys, N, 130, out_stride, in_stride, 0, box)


# 325 = a full workgroup (which class_permute reorders), a full wave outside it, and a tail.  Neither
# stride owns anything: every byte between bodies keeps the sentinel.  The second input layout takes
# the launcher's other branch (payloads off 16-byte alignment), which repeats the bound.
@pytest.mark.parametrize("in_stride,in_base", [(352, 0), (353, 1)], ids=["aligned-in", "packed-in"])
@pytest.mark.parametrize("out_stride", [(1 << 22) - 1, (1 << 22) + 1], ids=["2^22-1", "2^22+1"])
def test_seal_uniform_shift_limit(torch_dev, subkeys, out_stride, in_stride, in_base):
    _seal_uniform_case(torch_dev, subkeys, N, 256 + 64 + 5, out_stride, in_stride, in_base)


# The ownership rule at its small edges: the first stride past the region limit (64 * 272 > 16 KiB,
# owns nothing), a line-multiple slot whose body is too short for the line emitter, a slot longer
# than the body's last line, and a line-multiple stride from a base off 16-byte alignment.
SMALL_OWNERSHIP = [(100, 272, 0), (100, 384, 0), (N, 1024, 0), (N, 4224, 8), (100, 256, 0), (100, 144, 8)]


@pytest.mark.parametrize("n,out_stride,out_base", SMALL_OWNERSHIP)
def test_seal_uniform_ownership(torch_dev, subkeys, n, out_stride, out_base):
    torch, dev = torch_dev
    from jeromq_amd import batch
    count = 130
    pay, flags, bodies = _frames(n, count)
    in_stride = (n + 15) // 16 * 16
    d_in = _sentinel(torch_dev, count * in_stride)
    _put(torch_dev, d_in, 0, in_stride, pay)
    base = GUARD + out_base
    buf = _sentinel(torch_dev, base + count * out_stride + GUARD)
    batch.seal_uniform(d_in, in_stride, buf[base:], out_stride, count, n, subkeys[0], COUNTER0,
                       flags8=_dev_u8(torch_dev, flags))
    torch.cuda.synchronize()
    what = f"seal n={n} out_stride={out_stride} base+{out_base}"
    _same(_get(torch_dev, buf, base, out_stride, count, n + 33), bodies, what)
    _check_slots(torch_dev, buf, base, out_stride, count, n + 33, seal_uniform_owns(out_stride), what)


# ---- cases 3 and 4: uniform open ---------------------------------------------------------------------------
def _open_uniform_case(torch_dev, L, subkeys, n, count, out_stride, in_stride, in_base, out_base=0, replay=None):
    torch, dev = torch_dev
    from jeromq_amd import batch
    pay, flags, bodies = _frames(n, count)
    bodies = bodies.copy()
    want_st = flags.astype(np.uint16) << 8
    want = pay.copy()
    if replay is not None:      # frame `replay` carries the nonce of the frame before it
        bodies[replay, 8:16] = bodies[replay - 1, 8:16]
        want_st[replay] = L.CZ_STATUS_SEQUENCE
        want[replay] = 0
    d_in = _sentinel(torch_dev, in_base + count * in_stride + 64)
    _put(torch_dev, d_in, in_base, in_stride, bodies)
    base = GUARD + out_base
    buf = _sentinel(torch_dev, base + count * out_stride + GUARD)
    status = torch.full((count,), -1, dtype=torch.int16, device=dev)
    batch.open_uniform(d_in[in_base:], in_stride, buf[base:], out_stride, count, n + 33, subkeys[0], COUNTER0 - 1,
                       status)
    torch.cuda.synchronize()
    what = f"open nout={n} out_stride={out_stride} in_stride={in_stride}"
    st = status.cpu().numpy().view(np.uint16)
    assert np.array_equal(st, want_st), f"{what}: statuses differ at {np.nonzero(st != want_st)[0][:6].tolist()}"
    _same(_get(torch_dev, buf, base, out_stride, count, n), want, what)
    _check_slots(torch_dev, buf, base, out_stride, count, n, open_uniform_owns(out_stride), what)


@pytest.mark.parametrize("out_stride", [(1 << 25) - 128, 1 << 25], ids=["2^25-128", "2^25"])
def test_open_uniform_lines_limit(torch_dev, L, subkeys, out_stride):
    _open_uniform_case(torch_dev, L, subkeys, N, 130, out_stride, 384, 0)       # bodies in 128-byte multiple slots


@pytest.mark.parametrize("out_stride", [(1 << 22) - 1, (1 << 22) + 1], ids=["2^22-1", "2^22+1"])
def test_open_uniform_shift_limit(torch_dev, L, subkeys, out_stride):
    _open_uniform_case(torch_dev, L, subkeys, N, 256 + 64 + 5, out_stride, N + 33, 0)   # bodies dense


@pytest.mark.parametrize("n,out_stride,out_base", SMALL_OWNERSHIP)
def test_open_uniform_ownership(torch_dev, L, subkeys, n, out_stride, out_base):
    _open_uniform_case(torch_dev, L, subkeys, n, 130, out_stride, (n + 33 + 15) // 16 * 16, 0, out_base)


# Bodies of 296 bytes back to back from an 8-byte (not 16-byte) aligned base: the line phase repeats
# every P = 128 / gcd(296 mod 128, 128) = 16 frames, and the phase-sorted carry kernel gives its line
# emitter a lane stride of P * out_stride.  64 * P * (2^21 - 128) = 2^31 - 2^17 is the last product
# the launcher accepts; at 2^21 it declines and k_open_uniform takes the whole batch.  Both strides
# own their slots.  Frame 1024, the first after the whole blocks, replays frame 1023's nonce.
@pytest.mark.parametrize("open_carry", [1, 0])
@pytest.mark.parametrize("out_stride", [(1 << 21) - 128, 1 << 21], ids=["2^21-128", "2^21"])
def test_open_uniform_carry_limit(torch_dev, L, subkeys, out_stride, open_carry):
    with _knobs(L, open_carry=open_carry):
        _open_uniform_case(torch_dev, L, subkeys, 263, 64 * 16 + 37, out_stride, 296, 8, replay=1024)


# ---- case 5: segment kernels, outputs far apart --------------------------------------------------------------
# The segment kernels take segs[t] for thread t (class_permute serves the uniform ST_SHIFT kernels
# only), so list order is lane order: lane 0 of wave 0 is the first single-segment frame, lane 0 of
# wave 1 the first segment of the first split frame.  All outputs of a run are of one line class
# (offset 0 or 16 in their 128-byte line, bit 6 clear), so a wave is never `mixed` and
# EmitShiftLines flushes through FL_PHASE, where its WaveRel branch sits.
SEG_N = 460                       # a 493-byte body: 8 box blocks
SEG_SINGLE, SEG_SPLIT = 64, 32    # one full wave of whole frames, one of two-segment frames
SEG_X = GUARD + (1 << 30) + (1 << 20)
SEG_PITCH = 1024
SEG_SPLIT_SHIFT = 1 << 17         # the split frames repeat the single frames' layout this much higher
FAR = (1 << 32) + (1 << 20)
# one size for every layout: an offset wrapped at 32 bits lands up to 4 GiB above the lowest output,
# which must still be inside the allocation (and its sentinel) to be seen
SEG_BYTES = SEG_X + FAR + SEG_SPLIT_SHIFT + 64 * SEG_PITCH + GUARD
SEG_EDGE = SEG_SINGLE - 2         # the single-segment frame that lies apart in layouts (b) .. (d)


def _seg_layout(name):
    """out_off of the 64 single-segment frames, in lane order (multiples of 128)"""
    near = [SEG_X + SEG_PITCH * i for i in range(SEG_SINGLE)]
    if name == "a":        # a window of 2^30 - 256 bytes with frames at both ends; lane 0 at the top
        lo, w = SEG_X - (1 << 29), (1 << 30) - 256
        offs = [lo + SEG_PITCH * i for i in range(SEG_SINGLE)]
        for k, i in enumerate(i for i in range(SEG_SINGLE) if i % 4 in (0, 3)):   # (the split frames alternate too)
            offs[i] = lo + w - 128 - SEG_PITCH * k
        return offs
    edge = {"b": (1 << 30) - 128, "c": 1 << 30, "d0": -(1 << 30), "d1": -(1 << 30) - 128}
    if name in edge:       # frame 62: its offset is also that of the last split frame
        near[SEG_EDGE] = SEG_X + edge[name]
        return near
    assert name in ("e", "f")
    return [o + (FAR if i >= SEG_SINGLE // 2 else 0) for i, o in enumerate(near)]


def _seg_offsets(name, phase):
    single = _seg_layout(name)
    split = [single[2 * k] + SEG_SPLIT_SHIFT for k in range(SEG_SPLIT)]
    offs = np.array(single + split, dtype=np.uint64) + np.uint64(phase)
    order = np.arange(len(offs))
    if name == "f":        # layout (e) with the list reversed: a far frame leads each wave
        order = np.concatenate([order[:SEG_SINGLE][::-1], order[SEG_SINGLE:][::-1]])
    return offs, order


def _seg_plan(torch_dev, desc, order, open_):
    """A caller-built plan (as _segment_plan of test_gpu_poly_edges.py): frames [0, 64) whole, frames
    [64, 96) cut at block 4, segments listed in `order` of the frames"""
    from jeromq_amd import batch
    plan = batch.SegmentPlan(desc[:1], open_=open_)
    segs, combs, part = [], [], {}
    for f in range(SEG_SINGLE, len(desc)):
        part[f] = 2 * len(combs)
        combs.append((f, part[f], 2, 0))
    for f in order:
        if f < SEG_SINGLE:
            segs.append((f, 0, 8, 0xFFFFFFFF))
        else:
            segs += [(f, 0, 4, part[f]), (f, 4, 4, part[f] + 1)]
    plan.segments = np.array(segs, dtype=batch.SEGMENT_DTYPE)
    plan.combines = np.array(combs, dtype=batch.COMBINE_DTYPE)
    plan.nseg, plan.ncomb, plan.npart = len(segs), len(combs), 2 * len(combs)
    assert plan.nseg == 128
    return plan.to(torch_dev[1])


SEG_VARIANTS = {"lines128": (0, {}), "shift16": (16, {"shift16": 1}), "lines16": (16, {"shift16": 0}),
                "direct": (0, {"seglines": 0})}
SEG_LAYOUTS = ["a", "b", "c", "d0", "d1", "e", "f"]


def _seg_frames():
    return _frames(SEG_N, SEG_SINGLE + SEG_SPLIT)


def _scattered(torch_dev, buf, offs, width, want, what):
    """the rows at offs equal want, and nothing else in buf was written"""
    idx = _at(torch_dev, offs, width)
    _same(buf[idx].cpu().numpy(), want, what)
    buf[idx] = SENT
    assert _all(buf, SENT), f"{what}: bytes outside the outputs were written"


@pytest.mark.parametrize("variant", list(SEG_VARIANTS))
@pytest.mark.parametrize("layout", SEG_LAYOUTS)
def test_seal_segments_far_outputs(torch_dev, L, subkeys, layout, variant):
    torch, dev = torch_dev
    from jeromq_amd import batch
    phase, knobs = SEG_VARIANTS[variant]
    pay, flags, bodies = _seg_frames()
    count = len(pay)
    offs, order = _seg_offsets(layout, phase)
    desc = np.zeros(count, dtype=DESC_DTYPE)
    desc["in_off"] = np.arange(count, dtype=np.uint64) * 464
    desc["out_off"], desc["len"], desc["flags"] = offs, SEG_N, flags
    desc["counter"] = COUNTER0 + np.arange(count, dtype=np.uint64)
    desc["prev"] = -1
    d_in = _sentinel(torch_dev, count * 464)
    _put(torch_dev, d_in, 0, 464, pay)
    buf = _sentinel(torch_dev, SEG_BYTES)
    plan = _seg_plan(torch_dev, desc, order, False)
    with _knobs(L, **knobs):
        batch.seal_segments(_dev_u8(torch_dev, desc), plan, d_in, buf, subkeys, desc_np=desc)
        torch.cuda.synchronize()
    _scattered(torch_dev, buf, offs, SEG_N + 33, bodies, f"seal_segments {layout}/{variant}")


@pytest.mark.parametrize("variant", list(SEG_VARIANTS))
@pytest.mark.parametrize("layout", SEG_LAYOUTS)
def test_open_segments_far_outputs(torch_dev, L, subkeys, layout, variant):
    torch, dev = torch_dev
    from jeromq_amd import batch
    phase, knobs = SEG_VARIANTS[variant]
    pay, flags, bodies = _seg_frames()
    count = len(pay)
    offs, order = _seg_offsets(layout, phase)
    bodies, want = bodies.copy(), pay.copy()
    want_st = flags.astype(np.uint16) << 8
    # two tampered bodies whose payload slots lie in the far half (the far frame of layouts b .. d):
    # a whole frame and a split one, so the segment kernel's and the combine kernel's zeroing run
    for f in (SEG_EDGE, count - 1):
        bodies[f, 200] ^= 0x40
        want[f], want_st[f] = 0, L.CZ_STATUS_CRYPTO
    desc = np.zeros(count, dtype=DESC_DTYPE)
    desc["in_off"] = np.arange(count, dtype=np.uint64) * 496
    desc["out_off"], desc["len"] = offs, SEG_N + 33
    desc["counter"], desc["flags"], desc["prev"] = COUNTER0 - 1, L.CZ_DESC_CHECK_NONCE, -1
    d_in = _sentinel(torch_dev, count * 496)
    _put(torch_dev, d_in, 0, 496, bodies)
    buf = _sentinel(torch_dev, SEG_BYTES)
    status = torch.full((count,), -1, dtype=torch.int16, device=dev)
    plan = _seg_plan(torch_dev, desc, order, True)
    with _knobs(L, **knobs):
        batch.open_segments(_dev_u8(torch_dev, desc), plan, d_in, buf, subkeys, status, desc_np=desc)
        torch.cuda.synchronize()
    what = f"open_segments {layout}/{variant}"
    st = status.cpu().numpy().view(np.uint16)
    assert np.array_equal(st, want_st), f"{what}: statuses differ at {np.nonzero(st != want_st)[0][:6].tolist()}"
    _scattered(torch_dev, buf, offs, SEG_N, want, what)


def test_desc_batch_offsets_past_4gib(torch_dev, L, subkeys):
    """cz_seal_batch / cz_open_batch with layout (e) for in_off and out_off alike: half the frames lie
    more than 2^32 bytes above the others in both buffers"""
    torch, dev = torch_dev
    from jeromq_amd import batch
    pay, flags, bodies = _seg_frames()
    count = len(pay)
    far = np.where(np.arange(count) % 2 == 1, FAR, 0).astype(np.uint64)
    desc = np.zeros(count, dtype=DESC_DTYPE)
    desc["in_off"] = np.arange(count, dtype=np.uint64) * 464 + far + np.uint64(3)
    desc["out_off"] = np.uint64(GUARD) + np.arange(count, dtype=np.uint64) * 640 + far + np.uint64(5)
    desc["len"], desc["flags"], desc["prev"] = SEG_N, flags, -1
    desc["counter"] = COUNTER0 + np.arange(count, dtype=np.uint64)
    d_in = _sentinel(torch_dev, FAR + count * 464 + 64)
    d_in[_at(torch_dev, desc["in_off"], SEG_N)] = torch.from_numpy(pay.copy()).to(dev)
    buf = _sentinel(torch_dev, GUARD + FAR + count * 640 + GUARD)
    batch.seal_batch(_dev_u8(torch_dev, desc), count, d_in, buf, subkeys, desc_np=desc)
    torch.cuda.synchronize()
    idx = _at(torch_dev, desc["out_off"], SEG_N + 33)
    _same(buf[idx].cpu().numpy(), bodies, "seal_batch")
    # open the bodies where they lie, back over the payload buffer
    odesc = desc.copy()
    odesc["in_off"], odesc["out_off"] = desc["out_off"], desc["in_off"]
    odesc["len"], odesc["counter"], odesc["flags"] = SEG_N + 33, COUNTER0 - 1, L.CZ_DESC_CHECK_NONCE
    d_in.fill_(SENT)
    status = torch.full((count,), -1, dtype=torch.int16, device=dev)
    batch.open_batch(_dev_u8(torch_dev, odesc), count, buf, d_in, subkeys, status, desc_np=odesc)
    torch.cuda.synchronize()
    assert np.array_equal(status.cpu().numpy().view(np.uint16), flags.astype(np.uint16) << 8)
    _scattered(torch_dev, d_in, odesc["out_off"], SEG_N, pay, "open_batch")
    _scattered(torch_dev, buf, desc["out_off"], SEG_N + 33, bodies, "seal_batch")


# ---- case 6: fan-out ------------------------------------------------------------------------------------------
def _fanout_subs(count, first=0):
    from jeromq_amd import batch
    subs = np.zeros(count, dtype=batch.FANOUT_SUB_DTYPE)
    subs["counter"] = COUNTER0 + 7 * (first + np.arange(count, dtype=np.uint64))
    subs["key_idx"] = (first + np.arange(count)) % 2
    return subs


@functools.lru_cache(maxsize=None)
def _fanout_bodies(n, count, flags, first=0):
    payload = splitmix_bytes(n, 0xFA0 + n)
    subs = _fanout_subs(count, first)
    return payload, np.stack([np.frombuffer(or_curve_encode(payload, flags, int(s["counter"]), int(s["key_idx"]),
                                                             PRECOM), dtype=np.uint8) for s in subs])


@pytest.mark.parametrize("out_stride", [(1 << 25) - 128, 1 << 25], ids=["2^25-128", "2^25"])
def test_seal_fanout_lines_limit(torch_dev, subkeys, out_stride):
    torch, dev = torch_dev
    from jeromq_amd import batch
    count = 130
    payload, bodies = _fanout_bodies(N, count, 1)
    d_pay = _dev_u8(torch_dev, np.frombuffer(payload, dtype=np.uint8))
    buf = _sentinel(torch_dev, GUARD + count * out_stride + GUARD)
    batch.seal_fanout(d_pay, N, 1, _dev_u8(torch_dev, _fanout_subs(count)), subkeys, buf[GUARD:], out_stride, count)
    torch.cuda.synchronize()
    what = f"fanout out_stride={out_stride}"
    _same(_get(torch_dev, buf, GUARD, out_stride, count, N + 33), bodies, what)
    _check_slots(torch_dev, buf, GUARD, out_stride, count, N + 33, fanout_owns(out_stride), what)


def test_seal_fanout_runs_limits(torch_dev, L, subkeys):
    """Three runs in one call: the largest staged stride, the first lane-wise one, and a region-class
    run whose payload and output both lie past 2^32.  66 subscribers each (a full wave and a tail of
    two: three 130-slot runs of 32 MiB slots would not fit the memory cap; the second run's slots
    still cross 2^32).  The planner's classes are czk_fanout_class's for each run alone, and the bytes
    are cz_seal_fanout's run by run."""
    torch, dev = torch_dev
    from jeromq_amd import batch
    count = 66
    s1, s2, s3, n3 = (1 << 25) - 128, 1 << 25, 144, 100
    pay_off3 = (1 << 32) + 48
    runs = np.zeros(3, dtype=batch.FANOUT_RUN_DTYPE)
    o2 = GUARD + count * s1 + GUARD
    o3 = o2 + count * s2 + GUARD
    runs[0] = (0, GUARD, s1, N, 1, 0, count)
    runs[1] = (0, o2, s2, N, 1, count, count)
    runs[2] = (pay_off3, o3, s3, n3, 2, 2 * count, count)
    assert o2 + (count - 1) * s2 > (1 << 32) and o3 > (1 << 32)
    pay12, want0 = _fanout_bodies(N, count, 1, 0)
    _, want1 = _fanout_bodies(N, count, 1, count)
    pay3, want2 = _fanout_bodies(n3, count, 2, 2 * count)
    wants = [want0, want1, want2]
    d_in = _sentinel(torch_dev, pay_off3 + 128)
    d_in[:N] = _dev_u8(torch_dev, np.frombuffer(pay12, dtype=np.uint8))
    d_in[pay_off3:pay_off3 + n3] = _dev_u8(torch_dev, np.frombuffer(pay3, dtype=np.uint8))
    subs = _dev_u8(torch_dev, _fanout_subs(3 * count))
    buf = _sentinel(torch_dev, o3 + count * s3 + GUARD)
    plan = batch.plan_fanout(runs, d_in, buf)
    lib = L.lib()
    lib.czk_fanout_class.restype = ctypes.c_int
    lib.czk_fanout_class.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int]
    cc = [0, 0, 0]
    for r in runs:
        al = (d_in.data_ptr() + int(r["payload_off"])) % 16 == 0 and (buf.data_ptr() + int(r["out_off"])) % 16 == 0 \
            and int(r["out_stride"]) % 16 == 0
        cc[lib.czk_fanout_class(int(r["out_stride"]), int(r["len"]), count, int(al))] += 1    # the run's full wave
        cc[2] += 1                                                                            # its partial wave: lane-wise
    assert plan.class_count == cc == [1, 1, 4], (plan.class_count, cc)      # lines, region, lane-wise
    plan.to(dev)

    def check(what):
        got = []
        for r, want in zip(runs, wants):
            base, st, ln = int(r["out_off"]), int(r["out_stride"]), int(r["len"]) + 33
            got.append(_get(torch_dev, buf, base, st, count, ln))
            _same(got[-1], want, f"{what} stride {st}")
            pad = _rows(torch_dev, buf, base + ln, st, count, st - ln)
            assert _all(pad, 0 if fanout_owns(st) else SENT), f"{what} stride {st}: padding"
        for a, b in ((0, GUARD), (GUARD + count * s1, o2), (o2 + count * s2, o3), (o3 + count * s3, buf.numel())):
            assert _all(buf[a:b], SENT), f"{what}: bytes between the runs [{a}, {b}) were written"
        return got

    batch.seal_fanout_runs(plan, d_in, subs, subkeys, buf)
    torch.cuda.synchronize()
    grouped = check("fanout_runs")
    buf.fill_(SENT)
    for k, r in enumerate(runs):
        po, oo = int(r["payload_off"]), int(r["out_off"])
        batch.seal_fanout(d_in[po:], int(r["len"]), int(r["flags"]), subs[16 * count * k:], subkeys, buf[oo:],
                          int(r["out_stride"]), count)
    torch.cuda.synchronize()
    alone = check("fanout run by run")
    for a, b in zip(grouped, alone):
        assert np.array_equal(a, b)


# ---- case 7: cz_v2_copy -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("header", [0, 1], ids=["plain", "header"])
def test_v2_copy_offsets_past_4gib(torch_dev, L, header):
    """64 items of sizes 0, 1, 255, 256 and 4096 with src_off / dst_off on both sides of 2^32 at byte
    phases 0, 1, 3 and 15 (every pair of phases), one destination straddling 2^32"""
    torch, dev = torch_dev
    from jeromq_amd import wire
    sizes, phases = [0, 1, 255, 256, 4096], [0, 1, 3, 15]
    items = np.zeros(64, dtype=wire.V2_ITEM_DTYPE)
    src = np.frombuffer(splitmix_bytes(64 * 4096, 0x7C0), dtype=np.uint8).reshape(64, 4096)
    want = []
    for i in range(64):
        size, more = sizes[i % 5], (i >> 2) & 1
        s_far, d_far = (i & 1) * FAR, ((i >> 1) & 1) * FAR
        items[i] = (4096 + s_far + 8192 * i + phases[i % 4], GUARD + d_far + 8192 * i + phases[(i // 4) % 4], size,
                    (L.CZ_V2_ITEM_HEADER | more) if header else 0)
        want.append(v2_encode(src[i, :size], more) if header else src[i, :size].tobytes())
    items[19]["dst_off"] = (1 << 32) - 100      # size 4096: the copy runs across 2^32
    d_src = _sentinel(torch_dev, FAR + 64 * 8192 + 8192)
    d_src[_at(torch_dev, items["src_off"], 4096)] = torch.from_numpy(src.copy()).to(dev)
    buf = _sentinel(torch_dev, GUARD + FAR + 64 * 8192 + GUARD)
    wire.copy(_dev_u8(torch_dev, items), d_src, buf)
    torch.cuda.synchronize()
    idx = _at(torch_dev, items["dst_off"], 4096 + 9)
    got = buf[idx].cpu().numpy()
    for i, w in enumerate(want):
        assert got[i, :len(w)].tobytes() == w, f"item {i} (size {sizes[i % 5]})"
        assert np.all(got[i, len(w):] == SENT), f"item {i}: bytes behind the copy were written"
    buf[idx] = SENT
    assert _all(buf, SENT), "bytes outside the items were written"


# ---- the host-staged caller that relies on the rule ---------------------------------------------------------
def test_ctx_seal_uniform_whole_slots(L, torch_dev):
    """cz_ctx_seal_uniform promises whole zeroed slots and leaves the zeros of an owning stride to the
    kernel.  A first batch leaves body bytes all over the context's device buffer; the second one's
    stride is a line multiple whose 133-byte bodies are too short for the line emitter."""
    lib = L.lib()
    ctx = ctypes.c_void_p()
    L.check(lib.cz_ctx_create(ctypes.byref(ctx), 0))
    try:
        L.check(lib.cz_ctx_set_keys(ctx, PRECOM, 1, L.CZ_DIR_C2S))
        count = 130
        for n, ost in ((N, 385), (100, 384), (100, 272)):
            pay, flags, bodies = _frames(n, count)
            hin = np.ascontiguousarray(pay)
            hout = np.full(count * ost, SENT, dtype=np.uint8)
            L.check(lib.cz_ctx_seal_uniform(ctx, count, n, hin.ctypes.data, n, hout.ctypes.data, ost, COUNTER0,
                                            flags.ctypes.data, 96))
            got = hout.reshape(count, ost)
            _same(got[:, :n + 33], bodies, f"ctx seal stride {ost}")
            assert not got[:, n + 33:].any(), f"ctx seal stride {ost}: slot padding is not zero"
    finally:
        lib.cz_ctx_destroy(ctx)
