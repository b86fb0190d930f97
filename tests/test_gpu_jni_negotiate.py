"""The two negotiating handshake natives through the JNI glue in the fake JNIEnv
(tests/jni_harness.py), called as GpuHandshakeNegotiator calls them: the results are
the C ABI's, which tests/test_gpu_handshake_negotiate.py pins to the model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import handshake_oracle as H
from tests import hsneggen, jni_harness

OK, EINVAL = 0, -1
KEY = "dGhlIHNhbXBsZSBub25jZQ=="
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _image(compress=1, decompress=2):
    from snf4j_amd import DeflateNegotiation, Negotiation
    return bytes(Negotiation(("chat", "superchat"), DeflateNegotiation(compress, decompress)).native())


def test_java_image_layout_matches_the_struct():
    """GpuHandshakeNegotiator.pack() writes the struct's offsets, and both natives are
    called from it (no JDK here: the sources are read)."""
    from snf4j_amd._lib import HsNegotiation
    assert (HsNegotiation.protocol_off.offset, HsNegotiation.protocol_bytes.offset) == (8, 48)
    with open(os.path.join(ROOT, "java/org/snf4j/websocket/gpu/GpuPerMessageDeflateExtension.java")) as fh:
        java = fh.read()
    with open(os.path.join(ROOT, "java/org/snf4j/websocket/gpu/Wsg.java")) as fh:
        wsg = fh.read()
    assert "b, 48 + at, p.length" in java and "b[8 + 2 * (k + 1)]" in java and "b[9 + 2 * (k + 1)]" in java
    assert "Wsg.handshakeAcceptNegotiateBatchHost(" in java and "Wsg.handshakeValidateNegotiateBatchHost(" in java
    consts = dict(re.findall(r"static final int (HS_NEG\w+) = (\d+);", wsg))
    assert consts == {"HS_NEGOTIATION_BYTES": str(C.sizeof(HsNegotiation)), "HS_NEG_RESP_STRIDE": "384",
                      "HS_NEG_MAX_PROTOCOLS": "16", "HS_NEG_MAX_PROTOCOL_BYTES": "256"}
    img = _image()
    assert (img[0], img[1], img[3], img[4]) == (2, 1, 1, 2) and img[48:57] == b"chatsuper"
    assert int.from_bytes(img[10:12], "little") == 4 and int.from_bytes(img[12:14], "little") == 13


@pytest.mark.gpu
def test_jni_negotiate_natives_gpu():
    from snf4j_amd._lib import (HS_EXPECTED_STRIDE, HS_NEG_RESP_STRIDE, HS_NEGOTIATED_DTYPE, HS_RESULT_DTYPE, HsConfig,
                                HsNegotiation, lib)
    jni = jni_harness.Jni()
    ctx = jni.call("open", 0)
    assert ctx
    try:
        reqs = [hsneggen.server_request(dict(protocol=p, extensions=e), KEY) for p, e in [
            ("superchat, chat", hsneggen.BROWSER_OFFER), (None, "permessage-deflate; server_max_window_bits=7"),
            ("zzz", "permessage-deflate; client_no_context_takeover"), (None, None)]]
        n = len(reqs)
        packed = np.frombuffer(b"".join(reqs), np.uint8).copy()
        off = np.concatenate([[0], np.cumsum([len(r) for r in reqs])]).astype(np.uint64)
        resp, res = np.zeros(n * HS_NEG_RESP_STRIDE, np.uint8), np.zeros(n, HS_RESULT_DTYPE)
        ng = np.zeros(n, HS_NEGOTIATED_DTYPE)
        cfg, img = jni.ints([65536, 0, 0, 0, 0]), jni.bytes_(_image())
        assert jni.call("handshakeAcceptNegotiateBatchHost", ctx, cfg, img, jni.direct(packed),
                        jni.direct(off.view(np.uint8)), n, jni.direct(resp), jni.direct(res.view(np.uint8)),
                        jni.direct(ng.view(np.uint8))) == OK
        # == the C ABI on the same batch
        resp2, res2, ng2 = np.zeros_like(resp), np.zeros_like(res), np.zeros_like(ng)
        neg = HsNegotiation.from_buffer_copy(_image())
        assert lib.wsg_handshake_accept_negotiate_batch_host(
            C.c_void_p(ctx), C.byref(HsConfig(65536, 0, 0, 0, 0)), C.byref(neg), packed.ctypes.data, off.ctypes.data,
            n, resp2.ctypes.data, res2.ctypes.data, ng2.ctypes.data) == OK
        assert np.array_equal(res, res2) and np.array_equal(ng, ng2)
        for i in range(n):  # (a slot's bytes past resp_len are not written)
            a = slice(i * HS_NEG_RESP_STRIDE, i * HS_NEG_RESP_STRIDE + int(res["resp_len"][i]))
            assert res["resp_len"][i] and np.array_equal(resp[a], resp2[a]), i
        assert list(res["http_status"]) == [101, 400, 101, 101] and int(res["cause"][1]) == 24
        # decompress REQUIRED: client_no_context_takeover in every accepted answer
        assert list(ng["ext"]) == [3, 0, 3, 0] and list(ng["proto_len"]) == [9, 0, 0, 0]
        first = resp[:int(res["resp_len"][0])].tobytes()
        assert first.endswith(b"\r\nSec-WebSocket-Protocol: superchat\r\nSec-WebSocket-Extensions: permessage-deflate; "
                              b"client_no_context_takeover\r\n\r\n")
        # the client native on the server's answers (its compress side is the one REQUIRED:
        # an answer without server_no_context_takeover must not be a decline here)
        cimg = jni.bytes_(_image(2, 1))
        answers = [resp[i * HS_NEG_RESP_STRIDE:][:int(res["resp_len"][i])].tobytes() for i in (0, 2, 3)]
        m = len(answers)
        rp = np.frombuffer(b"".join(answers), np.uint8).copy()
        roff = np.concatenate([[0], np.cumsum([len(a) for a in answers])]).astype(np.uint64)
        keys = np.frombuffer((KEY * m).encode(), np.uint8).copy()
        exp, cres = np.zeros(m * HS_EXPECTED_STRIDE, np.uint8), np.zeros(m, HS_RESULT_DTYPE)
        cng = np.zeros(m, HS_NEGOTIATED_DTYPE)
        assert jni.call("handshakeValidateNegotiateBatchHost", ctx, cfg, cimg, jni.direct(rp),
                        jni.direct(roff.view(np.uint8)), jni.direct(keys), m, jni.direct(exp),
                        jni.direct(cres.view(np.uint8)), jni.direct(cng.view(np.uint8))) == OK
        # a client that lists subprotocols closes on an answer without one (:476)
        assert list(cres["kind"]) == [H.FINISHED, H.CLOSING, H.CLOSING]
        assert list(cres["cause"]) == [0, H.C_MISSING_SUBPROTOCOL, H.C_MISSING_SUBPROTOCOL]
        assert int(cng["ext"][0]) == 3 and int(cng["proto_len"][0]) == 9 and not cng["ext"][1:].any()
        assert exp[:28].tobytes().decode() == H.answer_key(KEY)
        # an image of the wrong size, and a malformed one, are EINVAL
        args = (jni.direct(packed), jni.direct(off.view(np.uint8)), n, jni.direct(resp), jni.direct(res.view(np.uint8)),
                jni.direct(ng.view(np.uint8)))
        assert jni.call("handshakeAcceptNegotiateBatchHost", ctx, cfg, jni.bytes_(_image()[:-1]), *args) == EINVAL
        bad = bytearray(_image())
        bad[3] = 3
        assert jni.call("handshakeAcceptNegotiateBatchHost", ctx, cfg, jni.bytes_(bad), *args) == EINVAL
    finally:
        jni.call("close", ctx)
        jni.free_all()
