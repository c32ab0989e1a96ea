"""The relay restated on the CPU: Proxy.forward (zmq/Proxy.java:140-160) is from.recv, then to.send --
Mechanism.decode on one connection, a Msg, Mechanism.encode on another.  The composition of the
receive model (tests/rx_model.py) and the CPU oracle, never of the library under test."""
import rx_model as rx
from cz_testlib import or_curve_encode


def relay_expect(body, floor, check, in_from_server, precom_in, counter, out_from_server, precom_out):
    """What a relay of one received body leaves: (status word as cz_open_batch writes it, the inbound wire
    nonce or None, the output bytes).  Accepted: the body Mechanism.encode produces for the Msg decode
    delivers -- the payload, only the MORE and COMMAND bits of the decrypted flags byte
    (CurveServerMechanism.java:207-213), the outbound counter and key.  Rejected: zeros, len(body) of them."""
    st, flags, payload, nonce = rx.frame_status(body, floor, check, in_from_server, precom_in)
    if st != rx.ST_OK:
        return st, nonce, bytes(len(body))
    return st | (flags << 8), nonce, or_curve_encode(payload, flags & 3, counter & rx.M64, out_from_server, precom_out)
