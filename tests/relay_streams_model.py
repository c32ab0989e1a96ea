"""cz_relay_streams (header section 3j) restated on the CPU: V2Decoder over one received stream (the state
machine of cz_testlib.V2DecoderModel), then for every whole frame the relay of tests/relay_model.py -- the
receive rule of tests/rx_model.py and the CPU oracle's seal -- with each frame's replay floor taken from the
wire bytes of the frame before it, and the cut that says what of the stream may leave.  Never the library under
test.  tests/test_relay_streams_host.py checks this model against rx_model.stream_model."""
from collections import namedtuple

import rx_model as rx
from cz_testlib import V2DecoderModel
from relay_model import relay_expect

# rc as cz_v2_parse returns it
RC = {None: 0, "EPROTO": rx.CZ_EPROTO, "EMSGSIZE": rx.CZ_EMSGSIZE}

StreamExpect = namedtuple("StreamExpect", "frames consumed rc out status nonces floors ok_frames ok_bytes whole_bytes "
                                          "peer_nonce fail_status")


def stream_expect(stream, floor, in_from_server, precom_in, counter, out_from_server, precom_out, behind=b"",
                  maxmsgsize=-1):
    """What cz_relay_streams leaves of one stream.  `behind`: the bytes that follow the stream in memory (the
    floor of the frame behind a body shorter than 16 bytes is read across that body's end).
    frames: [(header offset, body offset, size)] of the whole frames; consumed; rc; out: the `consumed` bytes as
    they leave (headers unchanged, accepted bodies re-sealed with counter + k, rejected bodies zeros); status /
    nonces / floors per frame (nonce None where the kernel sets none); then the cut record's fields."""
    stream = bytes(stream)
    dec = V2DecoderModel(maxmsgsize)
    dec.feed(stream)
    mem = stream + bytes(behind) + bytes(16)
    frames, out, status, nonces, floors = [], bytearray(), [], [], []
    at = 0
    for k, (off, size, _fl) in enumerate(dec.msgs):
        frames.append((at, off, size))
        fl = floor if k == 0 else int.from_bytes(mem[frames[k - 1][1] + 8:frames[k - 1][1] + 16], "big")
        st, nonce, body = relay_expect(stream[off:off + size], fl, True, in_from_server, precom_in,
                                       (counter + k) & rx.M64, out_from_server, precom_out)
        out += stream[at:off] + body
        status.append(st)
        nonces.append(nonce)
        floors.append(fl)
        at = off + size
    ok_frames, ok_bytes, whole, peer, fail = 0, 0, 0, floor & rx.M64, rx.ST_OK
    for k, st in enumerate(status):
        if st & 0xff != rx.ST_OK:
            fail = st & 0xff
            if fail == rx.ST_CRYPTO:
                peer = nonces[k]
            break
        ok_frames, ok_bytes, peer = k + 1, frames[k][1] + frames[k][2], nonces[k]
        if not (st >> 8) & 1:
            whole = ok_bytes
    return StreamExpect(frames, at, RC[dec.error], bytes(out), status, nonces, floors, ok_frames, ok_bytes, whole, peer,
                        fail)


def engine_expect(exp, role):
    """(delivered frames, peer_nonce, (error, event)) of a source connection of `role` whose received bytes gave
    `exp`: the first rejected frame fails it as flush_in would, a framing error behind good frames gives the
    framing error with event 0"""
    if exp.fail_status != rx.ST_OK:
        return exp.ok_frames, exp.peer_nonce, (rx.CZ_EPROTO, rx.event_for(exp.fail_status, role))
    return exp.ok_frames, exp.peer_nonce, (exp.rc, 0)
