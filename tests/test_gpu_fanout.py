"""GPU: the PUB fan-out seal (cz_seal_fanout, k_seal_fanout) and cz_engine_publish.

One payload sealed for N subscribers, each under its own key and nonce.  Every check is byte for
byte against two yardsticks that share no code with the new kernel: the CPU oracle (or_seal_batch
with N descriptors sharing one in_off) and the existing device path (cz_seal_batch with the same
descriptors).  The engine's wire streams are compared with V2Encoder(oracle seal) of each
connection's messages in send order, as tests/test_gpu_engine.py builds them."""
import ctypes

import numpy as np
import pytest

from cz_testlib import (DESC_DTYPE, oracle, oracle_check_full, or_curve_encode, splitmix_bytes, splitmix_words,
                        v2_encode)

pytestmark = pytest.mark.gpu

BLOCK = 256
NKEYS = BLOCK + 1
SENT = 0xA5
# payload lengths at the box's block edges (mlen = len + 33): 30/31/32 around one block, 47 a last
# block of exactly 16 box bytes (ksblock_w03), 95/96 around two blocks, 4096/4097 an even and an odd
# block count for the pair loop
LENS = [0, 1, 30, 31, 32, 47, 48, 95, 96, 4096, 4097]
COUNTS = [1, 63, 64, 65, 130, BLOCK + 1]
EDGE_COUNTERS = [(1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 2]


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from jeromq_amd import _lib, batch
    dev = torch.device("cuda:0")
    precom = splitmix_words(NKEYS * 4, 0xFA0).view(np.uint8).copy()   # NKEYS x 32 bytes
    keys = torch.from_numpy(precom).to(dev).view(NKEYS, 32)
    sub = batch.subkeys(keys, _lib.CZ_DIR_C2S)
    return torch, dev, batch, _lib, precom, sub


def round_up(v, a):
    return (v + a - 1) // a * a


def owns(stride):
    """the ownership rule of include/curvezmq_mi355x.h section 3c"""
    return (stride % 128 == 0 and stride < (1 << 25)) or (stride % 16 == 0 and stride <= 256)


def subscribers(rng, count, distinct):
    """key_idx not monotonic; arbitrary counters with the nonce edges next to each other inside a wave
    (2^32 - 1 beside 2^32: the high nonce word differs between neighbouring lanes)"""
    subs = np.zeros(count, dtype=[("counter", "<u8"), ("key_idx", "<u4"), ("reserved", "<u4")])
    subs["counter"] = rng.integers(0, 1 << 64, size=count, dtype=np.uint64)
    for w in range(0, count, 64):
        at = w + (5 if w + 5 + len(EDGE_COUNTERS) <= count else 0)
        for k, c in enumerate(EDGE_COUNTERS[:max(0, count - at)]):
            subs["counter"][at + k] = c
    subs["key_idx"] = rng.permutation(NKEYS)[:count] if distinct else (np.arange(count) * 2 + 1) % 3
    return subs


def shared_desc(subs, length, flags, in_off, out_off0, stride):
    d = np.zeros(len(subs), dtype=DESC_DTYPE)
    d["in_off"] = in_off
    d["out_off"] = out_off0 + np.arange(len(subs), dtype=np.uint64) * np.uint64(stride)
    d["len"] = length
    d["key_idx"] = subs["key_idx"]
    d["counter"] = subs["counter"]
    d["flags"] = flags
    d["prev"] = -1
    return d


def run_fanout(env, rng, length, count, distinct, flags, stride=None, out_phase=0, in_phase=0):
    """One fan-out launch into a sentinel-filled buffer; returns (got, want from the oracle, bodies
    from cz_seal_batch) over the whole buffer, guard bytes before and after included."""
    torch, dev, batch, _lib, precom, sub = env
    mlen = length + 33
    stride = stride or round_up(mlen, 128)
    subs = subscribers(rng, count, distinct)
    # the payload between bytes that differ from it, at the asked byte phase
    in_off = 64 + in_phase
    hin = np.frombuffer(splitmix_bytes(in_off + length + 80, 77 + length), dtype=np.uint8).copy()
    hin[:in_off] |= 0x80
    hin[in_off + length:] |= 0x80
    out_off0 = 256 + out_phase
    out_bytes = out_off0 + (count - 1) * stride + (stride if owns(stride) else mlen) + 256
    d_in = torch.from_numpy(hin).to(dev)
    d_subs = torch.from_numpy(subs.view(np.uint8).copy()).to(dev)
    d_out = torch.full((out_bytes,), SENT, dtype=torch.uint8, device=dev)
    batch.seal_fanout(d_in[in_off:], length, flags, d_subs, sub, d_out[out_off0:], stride, count)
    desc = shared_desc(subs, length, flags, in_off, out_off0, stride)
    d_ref = torch.full((out_bytes,), SENT, dtype=torch.uint8, device=dev)
    batch.seal_batch(torch.from_numpy(desc.view(np.uint8).copy()).to(dev), count, d_in, d_ref, sub, desc_np=desc)
    torch.cuda.synchronize()
    want = np.full(out_bytes, SENT, dtype=np.uint8)
    if owns(stride):
        want[out_off0:out_off0 + count * stride] = 0   # the batch owns whole slots: zeros past each body
    oracle().or_seal_batch(desc.ctypes.data, count, hin.ctypes.data, want.ctypes.data, precom.ctypes.data, 0, 8)
    return d_out.cpu().numpy(), want, d_ref.cpu().numpy(), desc


def check(got, want, ref, desc, what):
    mlen = int(desc["len"][0]) + 33
    if not np.array_equal(got, want):
        for i, o in enumerate(desc["out_off"]):
            o = int(o)
            assert np.array_equal(got[o:o + mlen], want[o:o + mlen]), f"{what}: body {i} differs from the oracle"
        bad = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{what}: byte {bad} outside the bodies is {got[bad]:#x}, expected {want[bad]:#x}")
    for i, o in enumerate(desc["out_off"]):
        o = int(o)
        assert np.array_equal(got[o:o + mlen], ref[o:o + mlen]), f"{what}: body {i} differs from cz_seal_batch"


@pytest.mark.parametrize("length", LENS)
def test_small_batches(env, length):
    """Block-edge lengths x partial / full / full + partial waves and the workgroup edge x 3 cycled
    keys and one key per subscriber, flags 0..3 in turn, counters at the nonce edges."""
    rng = np.random.default_rng(1000 + length)
    k = 0
    for count in COUNTS:
        for distinct in (False, True):
            got, want, ref, desc = run_fanout(env, rng, length, count, distinct, k % 4)
            check(got, want, ref, desc, f"len {length} count {count} distinct {distinct} flags {k % 4}")
            k += 1


def test_64k_payload_one_wave(env):
    rng = np.random.default_rng(65536)
    got, want, ref, desc = run_fanout(env, rng, 65536, 64, True, 3)
    check(got, want, ref, desc, "len 65536 count 64")


@pytest.mark.parametrize("length", [31, 47, 100, 4097])
def test_layouts(env, length):
    """Four strides (slots of 128-byte lines, the same + 128 with zeros past the body, dense, dense + 7)
    x output base and payload at byte phases 0, 8 and 1; the whole buffer is compared, so the guard
    bytes before the first slot, after the last and (strides that do not own their slots) between
    bodies must be intact, and an owned slot's bytes past the body must be zero."""
    rng = np.random.default_rng(2000 + length)
    mlen = length + 33
    k = 0
    for stride in (round_up(mlen, 128), round_up(mlen, 128) + 128, mlen, mlen + 7):
        for out_phase in (0, 8, 1):
            for in_phase in (0, 8, 1):
                got, want, ref, desc = run_fanout(env, rng, length, 130, k % 2 == 0, k % 4, stride, out_phase,
                                                  in_phase)
                check(got, want, ref, desc, f"len {length} stride {stride} out+{out_phase} in+{in_phase}")
                k += 1


def test_round_trip(env):
    """The bodies of one 130-subscriber batch open under the same key table: CZ_STATUS_OK, the
    payload and the flags byte for every subscriber."""
    torch, dev, batch, _lib, precom, sub = env
    rng = np.random.default_rng(3)
    length, count, flags = 1000, 130, 2
    stride = round_up(length + 33, 128)
    subs = subscribers(rng, count, True)
    payload = np.frombuffer(splitmix_bytes(length, 31), dtype=np.uint8).copy()
    d_in = torch.from_numpy(payload).to(dev)
    d_out = torch.zeros(count * stride, dtype=torch.uint8, device=dev)
    batch.seal_fanout(d_in, length, flags, torch.from_numpy(subs.view(np.uint8).copy()).to(dev), sub, d_out, stride,
                      count)
    pstride = round_up(length, 16)
    odesc = np.zeros(count, dtype=DESC_DTYPE)
    odesc["in_off"] = np.arange(count, dtype=np.uint64) * np.uint64(stride)
    odesc["out_off"] = np.arange(count, dtype=np.uint64) * np.uint64(pstride)
    odesc["len"] = length + 33
    odesc["key_idx"] = subs["key_idx"]
    odesc["prev"] = -1
    d_plain = torch.zeros(count * pstride, dtype=torch.uint8, device=dev)
    status = torch.zeros(count, dtype=torch.int16, device=dev)
    nonces = torch.zeros(count, dtype=torch.int64, device=dev)
    batch.open_batch(torch.from_numpy(odesc.view(np.uint8).copy()).to(dev), count, d_out, d_plain, sub, status,
                     nonces=nonces, desc_np=odesc)
    torch.cuda.synchronize()
    st = status.cpu().numpy().view(np.uint16)
    assert np.all((st & 0xff) == _lib.CZ_STATUS_OK), st
    assert np.all((st >> 8) == flags)
    assert np.array_equal(nonces.cpu().numpy().view(np.uint64), subs["counter"])
    plain = d_plain.cpu().numpy().reshape(count, pstride)
    assert np.all(plain[:, :length] == payload[None, :])


def test_larger_batch(env):
    """2^14 subscribers x 4 KiB (64 MiB of bodies), one key each, against the oracle and cz_seal_batch."""
    torch, dev, batch, _lib, _, _ = env
    count, length = 1 << 14, 4096
    stride = round_up(length + 33, 128)
    precom = splitmix_words(count * 4, 0xB16).view(np.uint8).copy()
    sub = batch.subkeys(torch.from_numpy(precom).to(dev).view(count, 32), _lib.CZ_DIR_C2S)
    rng = np.random.default_rng(4)
    subs = np.zeros(count, dtype=[("counter", "<u8"), ("key_idx", "<u4"), ("reserved", "<u4")])
    subs["counter"] = rng.integers(0, 1 << 64, size=count, dtype=np.uint64)
    subs["key_idx"] = rng.permutation(count)
    d_in = torch.from_numpy(np.frombuffer(splitmix_bytes(length, 5), dtype=np.uint8).copy()).to(dev)
    d_out = torch.full((count * stride,), SENT, dtype=torch.uint8, device=dev)
    batch.seal_fanout(d_in, length, 1, torch.from_numpy(subs.view(np.uint8).copy()).to(dev), sub, d_out, stride, count)
    desc = shared_desc(subs, length, 1, 0, 0, stride)
    d_ref = torch.empty_like(d_out)
    batch.seal_batch(torch.from_numpy(desc.view(np.uint8).copy()).to(dev), count, d_in, d_ref, sub, desc_np=desc)
    torch.cuda.synchronize()
    assert oracle_check_full(d_in, d_out, desc, precom) == count
    got = d_out.view(count, stride)
    assert torch.equal(got[:, :length + 33], d_ref.view(count, stride)[:, :length + 33])
    assert int(got[:, length + 33:].max()) == 0   # the batch owns its slots


# ---- engine ------------------------------------------------------------------------------------

def _precom(i):
    return splitmix_bytes(32, 777 + i)


def _wire(msgs, precom, nonce0):
    return b"".join(v2_encode(or_curve_encode(p, fl, nonce0 + k, 0, precom)) for k, (p, fl) in enumerate(msgs))


def _engine(arena, ncon):
    from jeromq_amd.engine import CurveBatchEngine
    e = CurveBatchEngine(arena_bytes=arena)
    return e, [e.add_connection(_precom(i), as_server=False) for i in range(ncon)]


def _tear_down(eng, conn):
    """a frame with a bad tag arrives on `conn`: the engine tears the connection down"""
    body = bytearray(or_curve_encode(b"hello", 0, 2, 1, _precom(conn)))
    body[20] ^= 1
    eng.recv(conn, v2_encode(bytes(body)))
    eng.flush_in()
    assert eng.error(conn)[0] != 0


@pytest.mark.parametrize("fanout_min", [64, 2])
def test_engine_publish(env, fanout_min):
    """send / publish interleaved on 5 connections, one of them torn down before: every wire stream
    is V2Encoder(oracle seal) of the connection's messages in send order, nonces advance by the
    frames queued, and the failed connection is skipped.  fanout_min 64 keeps these short publishes
    in the segment plan, 2 sends each through cz_seal_fanout as a partial wave."""
    _, _, _, L, _, _ = env
    old = L.lib().cz_tune(b"fanout_min", fanout_min)
    try:
        _engine_publish_scenario(L)
    finally:
        L.lib().cz_tune(b"fanout_min", old)


def _engine_publish_scenario(L):
    eng, cc = _engine(1 << 20, 5)
    A, B, C, D, E = cc
    _tear_down(eng, D)
    x, y, z = splitmix_bytes(300, 1), splitmix_bytes(4096, 2), splitmix_bytes(17, 3)
    p1, p2 = splitmix_bytes(1000, 4), splitmix_bytes(0, 5)
    sent = {c: [] for c in cc}
    assert eng.send(A, x) == 0
    sent[A].append((x, 0))
    assert eng.publish([A, B, C], y) == 3
    for c in (A, B, C):
        sent[c].append((y, 0))
    assert eng.send(A, z) == 0
    sent[A].append((z, 0))
    assert eng.publish(cc, p1, more=True) == 4          # D has failed: skipped
    assert eng.publish(cc, p2) == 4
    for c in (A, B, C, E):
        sent[c] += [(p1, 1), (p2, 0)]
    assert eng.publish([B, B], z) == 2                  # an id named twice: consecutive nonces
    sent[B] += [(z, 0), (z, 0)]
    # an unknown id: CZ_EINVAL, nothing queued (the nonces and wire streams below would show it)
    ids = (ctypes.c_int * 3)(A, 99, B)
    q = ctypes.c_uint32(5)
    assert L.lib().cz_engine_publish(eng._h, ids, 3, y, len(y), 0, ctypes.byref(q)) == L.CZ_EINVAL
    assert q.value == 0
    with pytest.raises(L.CzError):
        eng.publish([A, -1], y)
    eng.flush_out()
    for c in cc:
        assert eng.wire_out(c) == _wire(sent[c], _precom(c), 3), f"connection {c}"
        if c != D:
            assert eng.nonce(c) == 3 + len(sent[c])
    assert eng.wire_out(D) == b""
    eng.close()


def test_engine_publish_stages_the_payload_once(env):
    """A 64 KiB arena carries a 4 KiB publish to 1000 connections; the same traffic as 1000 send
    copies fills it (CZ_ENOMEM).  A full arena refuses a publish with nothing queued."""
    _, _, _, L, _, _ = env
    eng, cc = _engine(64 << 10, 1000)
    y = splitmix_bytes(4096, 9)
    assert eng.publish(cc, y) == 1000
    eng.flush_out()
    for c in (cc[0], cc[63], cc[64], cc[999]):
        assert eng.wire_out(c) == _wire([(y, 0)], _precom(c), 3)
    rcs = [eng.send(c, y) for c in cc]
    assert L.CZ_ENOMEM in rcs and rcs[0] == 0
    nq = rcs.index(L.CZ_ENOMEM)
    ids = (ctypes.c_int * 1000)(*cc)
    q = ctypes.c_uint32(5)
    assert L.lib().cz_engine_publish(eng._h, ids, 1000, y, len(y), 0, ctypes.byref(q)) == L.CZ_ENOMEM
    assert q.value == 0
    assert L.lib().cz_engine_publish(eng._h, ids, 1000, y, L.CZ_MESSAGE_MAX + 1, 0, None) == L.CZ_EMSGSIZE
    eng.flush_out()
    for k, c in enumerate(cc[:nq + 2]):
        assert eng.wire_out(c) == (_wire([(y, 0)], _precom(c), 4) if k < nq else b"")
    eng.close()


def test_engine_both_routings_give_the_same_wire(env):
    """130 publish frames between sends, with the fan-out routing on (fanout_min 64) and off (2^30):
    identical wire bytes, equal to the oracle's."""
    _, _, _, L, _, _ = env
    y, z = splitmix_bytes(4096, 11), splitmix_bytes(100, 12)
    wires = {}
    for fmin in (64, 1 << 30):
        old = L.lib().cz_tune(b"fanout_min", fmin)
        try:
            eng, cc = _engine(1 << 20, 130)
            assert eng.send(cc[7], z) == 0
            assert eng.publish(cc, y, more=True) == 130
            assert eng.publish(cc[:70], z) == 70
            assert eng.send(cc[7], z, command=True) == 0
            eng.flush_out()
            wires[fmin] = [eng.wire_out(c) for c in cc]
            eng.close()
        finally:
            L.lib().cz_tune(b"fanout_min", old)
    assert wires[64] == wires[1 << 30]
    for k, c in enumerate(cc):
        msgs = ([(z, 0)] if k == 7 else []) + [(y, 1)] + ([(z, 0)] if k < 70 else []) + ([(z, 2)] if k == 7 else [])
        assert wires[64][k] == _wire(msgs, _precom(c), 3), f"connection {k}"
