"""GPU: batch.open_streams (cz_open_streams) as one more receiver against the one model of tests/rx_model.py.

Every single-fault scenario and the four nonce runs of the table, V2-framed as one stream per scenario and all
scenarios of a role in one call: the device scans the streams, places them, emits the descriptors and opens
every frame from the wire bytes where they lie, at any byte alignment.  Bit-exact against the model: status,
flags byte, nonce and payload of every frame, zero or untouched output for a rejected frame.  The 300 033-byte
bodies are left out: valid here, but slow with one lane per frame."""
import numpy as np
import pytest

import rx_model as rx
from cz_testlib import DESC_DTYPE, v2_encode

pytestmark = pytest.mark.gpu

SENT = 0xA5
ALIGN = 128


class _Gpu:
    pass


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from jeromq_amd import _lib, batch, wire
    g = _Gpu()
    g.torch, g.dev, g.L, g.batch, g.wire = torch, torch.device("cuda:0"), _lib, batch, wire
    k = torch.tensor(list(rx.PRECOM), dtype=torch.uint8, device=g.dev).view(1, 32)
    g.subkeys = torch.cat([batch.subkeys(k, _lib.CZ_DIR_C2S), batch.subkeys(k, _lib.CZ_DIR_S2C)])
    return g


def table():
    """the scenarios this receiver takes: not the uniform chains (one size: the fan-in's ground), not the
    300 033-byte bodies"""
    out = [s for s in rx.single_fault_scenarios() if all(f.size != rx.BIG for f in s.frames)]
    assert sum(s.name.startswith("run:") for s in out) == 4 and len(out) > 80
    return out


def _r(n, a):
    return (n + a - 1) // a * a


def _slot(size):
    return _r(max(size - 33, 1), ALIGN)


def _build(g, scs, role):
    """the wire of `scs` (each scenario's chained frames, as the raw receivers take them), streams packed
    3..18 bytes apart so that bodies start at every byte residue, 16 readable bytes behind the last one"""
    W = g.wire
    bodies = [sc.bodies(role)[:sc.raw_count(role)] for sc in scs]
    wires = [b"".join(v2_encode(b) for b in bs) for bs in bodies]
    st = np.zeros(len(scs), dtype=W.V2_STREAM_DTYPE)
    at = 5
    for i, w in enumerate(wires):
        st[i]["off"], st[i]["len"] = at, len(w)
        at += len(w) + 3 + i % 16
    st["floor"] = np.array([sc.floor for sc in scs], dtype=np.uint64)
    st["key_idx"] = rx.from_server(role)
    host = np.full(at + 16, 0xC3, dtype=np.uint8)
    for i, w in enumerate(wires):
        o = int(st[i]["off"])
        host[o:o + len(w)] = np.frombuffer(w, dtype=np.uint8)
    return bodies, st, g.torch.from_numpy(host).to(g.dev)


def _buffers(g, nstreams, nframes, slot_bytes):
    t, u8 = g.torch, g.torch.uint8
    return dict(results=t.full((nstreams * 32,), SENT, dtype=u8, device=g.dev),
                desc=t.full((max(nframes, 1) * 40,), SENT, dtype=u8, device=g.dev),
                out=t.full((slot_bytes + ALIGN,), SENT, dtype=u8, device=g.dev),
                status=t.full((max(nframes, 1),), -1, dtype=t.int16, device=g.dev),
                nonces=t.full((max(nframes, 1),), -1, dtype=t.int64, device=g.dev))


@pytest.mark.parametrize("role", rx.ROLES)
def test_open_streams_against_the_model(gpu, role):
    g, bad = gpu, []
    scs = table()
    bodies, st, d_wire = _build(g, scs, role)
    N = sum(len(b) for b in bodies)
    S = sum(_slot(len(x)) for b in bodies for x in b)
    buf = _buffers(g, len(scs), N, S)
    rc, nframes, slot_bytes = g.batch.open_streams(g.wire.to_device(st, g.dev), d_wire, buf["results"], buf["desc"],
                                                   buf["out"], g.subkeys, buf["status"], nonces=buf["nonces"],
                                                   out_cap=S)
    g.torch.cuda.synchronize()
    assert (rc, nframes, slot_bytes) == (0, N, S)
    res = buf["results"].cpu().numpy().view(g.wire.V2_STREAM_RESULT_DTYPE)
    desc = buf["desc"].cpu().numpy().view(DESC_DTYPE)
    out = buf["out"].cpu().numpy()
    status = buf["status"].cpu().numpy().view(np.uint16)
    nonces = buf["nonces"].cpu().numpy().view(np.uint64)
    assert out[S:].tobytes() == bytes([SENT]) * ALIGN, "bytes behind the last slot changed"
    first = 0
    for i, sc in enumerate(scs):
        exp, bs = sc.raw_expect(role), bodies[i]
        assert len(exp) == len(bs)
        if (int(res[i]["first"]), int(res[i]["nframes"]), int(res[i]["rc"])) != (first, len(bs), 0) or \
                int(res[i]["consumed"]) != int(st[i]["len"]):
            bad.append(f"{sc.name}: stream result {res[i]}, expected first {first}, {len(bs)} frames")
            first += len(bs)
            continue
        for k, (est, efl, epay, enonce) in enumerate(exp):
            j, where = first + k, f"{sc.name} frame {k}"
            o, plen = int(desc[j]["out_off"]), max(len(bs[k]) - 33, 0)
            if int(desc[j]["len"]) != len(bs[k]) or o % ALIGN or o + _slot(len(bs[k])) > S:
                bad.append(f"{where}: descriptor {desc[j]}")
                continue
            region = out[o:o + plen]
            if (status[j] & 0xff) != est:
                bad.append(f"{where}: status {status[j] & 0xff}, model {est}")
                continue
            if est == rx.ST_OK:
                if status[j] >> 8 != efl:
                    bad.append(f"{where}: flags byte {status[j] >> 8:#x}, model {efl:#x}")
                if region.tobytes() != epay:
                    bad.append(f"{where}: payload differs")
            else:
                if status[j] >> 8:
                    bad.append(f"{where}: a rejected frame's status carries {status[j] >> 8:#x}")
                ok = not region.any() if est == rx.ST_CRYPTO else bool(np.all((region == 0) | (region == SENT)))
                if not ok:
                    bad.append(f"{where}: a rejected frame's output holds other bytes than zero / the sentinel")
            if enonce is not None and int(nonces[j]) != enonce:
                bad.append(f"{where}: nonce {int(nonces[j]):#x}, model {enonce:#x}")
            rest = out[o + _r(plen, 16):o + _slot(len(bs[k]))]
            if rest.tobytes() != bytes([SENT]) * len(rest):
                bad.append(f"{where}: slot bytes behind the payload's last 16-byte row changed")
        first += len(bs)
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("short", ["desc_cap", "out_cap"])
def test_enomem_fills_the_totals_and_opens_nothing(gpu, short):
    g, role = gpu, rx.SERVER
    scs = table()[:70]
    bodies, st, d_wire = _build(g, scs, role)
    N = sum(len(b) for b in bodies)
    S = sum(_slot(len(x)) for b in bodies for x in b)
    buf = _buffers(g, len(scs), N, S)
    caps = dict(desc_cap=N - 1, out_cap=S) if short == "desc_cap" else dict(desc_cap=N, out_cap=S - 1)
    rc, nframes, slot_bytes = g.batch.open_streams(g.wire.to_device(st, g.dev), d_wire, buf["results"], buf["desc"],
                                                   buf["out"], g.subkeys, buf["status"], nonces=buf["nonces"], **caps)
    g.torch.cuda.synchronize()
    assert rc == g.L.CZ_ENOMEM and (nframes, slot_bytes) == (N, S)
    for name in ("desc", "out"):
        assert buf[name].cpu().numpy().tobytes() == bytes([SENT]) * buf[name].numel(), name
    assert np.all(buf["status"].cpu().numpy() == -1) and np.all(buf["nonces"].cpu().numpy() == -1)
    # one more and it opens
    rc, nframes, slot_bytes = g.batch.open_streams(g.wire.to_device(st, g.dev), d_wire, buf["results"], buf["desc"],
                                                   buf["out"], g.subkeys, buf["status"], nonces=buf["nonces"],
                                                   desc_cap=N, out_cap=S)
    g.torch.cuda.synchronize()
    assert (rc, nframes, slot_bytes) == (0, N, S) and np.all(buf["status"].cpu().numpy() != -1)
