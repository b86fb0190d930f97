"""Client handshake with the negotiation on the GPU (k_hs_validate_neg through
BatchClientHandshaker with a Negotiation) against tests/hsnegotiate.py, the restatement
of Handshaker.validateSubProtocol / validateExtensions over one
PerMessageDeflateExtension; and both sides end to end, down to the codec flags."""
import random

import numpy as np
import pytest

from oracle import handshake_oracle as H
from tests import hsneggen
from tests import hsnegotiate as N
from tests.golden import fixtures

pytestmark = pytest.mark.gpu

KEY = "dGhlIHNhbXBsZSBub25jZQ=="


def _negotiation(st: N.Settings):
    from snf4j_amd import DeflateNegotiation, Negotiation
    return Negotiation(tuple(st.subprotocols), DeflateNegotiation(*st.deflate) if st.deflate else None,
                       st.other_extensions)


def _gpu(responses, keys, st: N.Settings, max_length=65536):
    from snf4j_amd import BatchClientHandshaker, ClientConfig
    return BatchClientHandshaker(ClientConfig(max_length, (), False, _negotiation(st))).validate(responses, keys)


def _deflate(ext: int):
    """ClientHandshakeOutcome.deflate of the model's EXT_* bits: (clientNoContext, serverNoContext)."""
    return (bool(ext & N.EXT_CLIENT_NC), bool(ext & N.EXT_SERVER_NC)) if ext & N.EXT_DEFLATE else None


def _expect_equal(resp, g, r):
    if r["kind"] == H.DEFER:
        assert (g.kind, g.cause) == (H.DEFER, r["cause"]), (resp, g, r)
        assert g.subprotocol is None and g.deflate is None, (resp, g)
        return
    assert r["kind"] is not None, (resp, g)
    assert (g.kind, g.status, g.cause) == (r["kind"], r["status"], r["cause"]), (resp, g, r)
    assert g.message == N.message(r), (resp, g, r)
    assert (g.subprotocol, g.deflate) == (r["subprotocol"], _deflate(r["ext"])), (resp, g, r)
    if r["frame_len"]:
        assert g.frame_len == r["frame_len"], (resp, g, r)
    if r["expected"] is not None:
        assert g.expected == r["expected"], (resp, g, r)


def _resp(protocol=None, extensions=None, key=KEY):
    return hsneggen.client_response(dict(protocol=protocol, extensions=extensions), key)


def test_client_negotiate_kat_gpu():
    for v in fixtures.load("handshake_negotiate"):
        if v["kind"] == "client":
            g = _gpu([hsneggen.client_response(v, KEY)], [KEY], hsneggen.settings(v))[0]
            e = v["expect"]
            assert g.finished == e["finished"] and g.kind in (H.FINISHED, H.CLOSING), (v, g)
            assert (g.subprotocol, g.deflate) == (e["protocol"], None), (v, g)
        elif v["kind"] == "validate_response":
            st = N.Settings((), (v["compress"], v["decompress"]), False)
            g, e = _gpu([_resp(None, v["element"])], [KEY], st)[0], v["expect"]
            if e is not None and "error" in e:
                assert (g.kind, g.message) == (H.CLOSING, "Invalid extension: " + e["error"]), (v, g)
            elif e is None:  # a wrong name or a decline: validateExtensions false, no reason
                assert (g.kind, g.cause, g.message) == (H.CLOSING, H.C_INVALID_EXTENSIONS, None), (v, g)
            else:
                assert g.finished and g.deflate == (e["cn"], e["sn"]), (v, g)
        elif v["kind"] == "parse" and "error" in v["expect"] and N.split_extension(v["element"])[0] == N.NAME:
            g = _gpu([_resp(None, v["element"])], [KEY], N.Settings((), (N.OPTIONAL, N.OPTIONAL), False))[0]
            assert (g.kind, g.message) == (H.CLOSING, "Invalid extension: " + v["expect"]["error"]), (v, g)


@pytest.mark.parametrize("seed", range(3))
def test_client_negotiate_random_gpu(seed):
    causes, finished = {}, 0
    for st, keys, resps in hsneggen.client_groups(seed):
        for resp, key, g in zip(resps, keys, _gpu(resps, keys, st)):
            r = N.validate(resp, key, st)
            _expect_equal(resp, g, r)
            causes[r["cause"]] = causes.get(r["cause"], 0) + 1
            finished += r["kind"] == H.FINISHED and bool(r["ext"])
    # the model alone reaches each "Invalid extension: ..." text, the silent refusal and
    # the negotiated finish
    assert all(causes.get(c, 0) >= 15 for c in N.EXT_TEXTS), causes
    assert causes.get(H.C_INVALID_EXTENSIONS, 0) >= 50 and causes.get(H.C_INVALID_SUBPROTOCOL, 0) >= 50, causes
    assert finished >= 200, finished


def test_client_negotiate_edges_gpu():
    oo = N.Settings(("chat", "superchat"), (N.OPTIONAL, N.OPTIONAL), False)
    six = ["permessage-deflate; server_no_context_takeover; Server_No_Context_Takeover",     # Duplicated parameter
           "permessage-deflate; client_no_context_takeover=1",                               # Unnecessary parameter value
           "permessage-deflate; server_max_window_bits",                                     # Missing parameter value
           "permessage-deflate; client_max_window_bits=2147483648",                          # Invalid ... value format
           "permessage-deflate; server_max_window_bits=16",                                  # Invalid parameter value
           "permessage-deflate; "]
    six[5] += "=15"                                                                          # Unexpected parameter ("")
    resps = [_resp("chat", e) for e in six]
    resps += [_resp("chat", "permessage-deflate, permessage-deflate"),          # a second accepted element
              _resp("chat", "permessage-deflate; client_max_window_bits"),      # no value: -1 < 15, declined
              _resp("chat", "permessage-deflate; client_max_window_bits=15"),
              _resp("chat", ""), _resp("chat", " , "),                          # present but empty: no extension
              _resp("chat", "x-webkit-deflate-frame"),
              _resp("chat", "x-webkit-deflate-frame, permessage-deflate; bogus"),   # the first element decides
              _resp("chat, superchat", None), _resp("superchat", None), _resp("*", None), _resp("", None),
              _resp(None, None), _resp(" superchat \t", "permessage-deflate;server_no_context_takeover")]
    outs = _gpu(resps, [KEY] * len(resps), oo)
    for resp, g in zip(resps, outs):
        _expect_equal(resp, g, N.validate(resp, KEY, oo))
    assert [o.cause for o in outs[:6]] == [25, 26, 27, 28, 29, 30]
    assert [o.message for o in outs[:6]] == ["Invalid extension: " + N.EXT_TEXTS[c] for c in range(25, 31)]
    assert [(o.kind, o.cause) for o in outs[6:8]] == [(H.CLOSING, H.C_INVALID_EXTENSIONS)] * 2
    assert outs[8].finished and outs[8].deflate == (False, False)
    assert outs[9].finished and outs[10].finished and outs[9].deflate is None
    assert [o.cause for o in outs[11:13]] == [H.C_INVALID_EXTENSIONS] * 2
    assert outs[13].message == "Invalid websocket sub protocol: chat, superchat"   # the whole value, not its tokens
    assert outs[14].finished and outs[14].subprotocol == "superchat"
    assert outs[15].cause == H.C_INVALID_SUBPROTOCOL and outs[17].cause == H.C_MISSING_SUBPROTOCOL
    assert outs[18].finished and outs[18].deflate == (False, True)
    # "*" is an entry like any other on this side
    star = N.Settings(("*",), None, False)
    outs = _gpu([_resp("*"), _resp("chat"), _resp(None, "permessage-deflate")], [KEY] * 3, star)
    assert outs[0].subprotocol == "*" and outs[1].cause == H.C_INVALID_SUBPROTOCOL
    assert outs[2].cause == H.C_MISSING_SUBPROTOCOL
    # REQUIRED and absent is a decline here (acceptOffer would have switched it on)
    for pair, ext, ok in [((N.REQUIRED, N.OPTIONAL), "permessage-deflate", False),
                          ((N.REQUIRED, N.OPTIONAL), "permessage-deflate; client_no_context_takeover", True),
                          ((N.OPTIONAL, N.REQUIRED), "permessage-deflate; client_no_context_takeover", False),
                          ((N.OPTIONAL, N.REQUIRED), "permessage-deflate; server_no_context_takeover", True),
                          ((N.FORBIDDEN, N.OPTIONAL), "permessage-deflate; client_no_context_takeover", False)]:
        st = N.Settings((), pair, False)
        g = _gpu([_resp(None, ext)], [KEY], st)[0]
        _expect_equal(_resp(None, ext), g, N.validate(_resp(None, ext), KEY, st))
        assert g.finished == ok and (ok or g.cause == H.C_INVALID_EXTENSIONS), (pair, ext, g)
    # other_extensions defers the field; without a Negotiation the old entry point answers
    g = _gpu([_resp(None, "permessage-deflate")], [KEY], N.Settings((), (1, 1), True))[0]
    assert (g.kind, g.cause) == (H.DEFER, H.D_EXTENSION)
    from snf4j_amd import BatchClientHandshaker, ClientConfig
    rs = [_resp("chat", None), _resp(None, "permessage-deflate"), _resp(None, None)]
    old = BatchClientHandshaker(ClientConfig(65536, ("chat",), True)).validate(rs, [KEY] * 3)
    assert [(o.kind, o.cause) for o in old] == [(H.DEFER, H.D_SUBPROTOCOL), (H.CLOSING, H.C_MISSING_SUBPROTOCOL),
                                                 (H.CLOSING, H.C_MISSING_SUBPROTOCOL)]
    assert all(o.subprotocol is None and o.deflate is None for o in old)


@pytest.mark.parametrize("server_pair,client_pair,offer_params", [
    ((N.OPTIONAL, N.OPTIONAL), (N.OPTIONAL, N.OPTIONAL), ""),
    ((N.REQUIRED, N.OPTIONAL), (N.OPTIONAL, N.OPTIONAL), "; client_max_window_bits"),
    ((N.OPTIONAL, N.OPTIONAL), (N.REQUIRED, N.REQUIRED), "; client_no_context_takeover; server_no_context_takeover"),
])
def test_negotiate_end_to_end_gpu(server_pair, client_pair, offer_params):
    """client_request with offers -> server negotiate -> client negotiate on the server's
    response: both switch with consistent flags, and a message compressed with the
    server's encoder flag inflates with the client's decoder flag."""
    from snf4j_amd import (BatchClientHandshaker, BatchHandshaker, ClientConfig, Context, DeflateNegotiation,
                           HandshakeConfig, Negotiation)
    from snf4j_amd._lib import DEFLATE_STATE_DTYPE, DESC_DTYPE, INFLATE_STATE_DTYPE
    from snf4j_amd.context import DEFLATE_SESSION_BYTES
    from snf4j_amd.handshake import client_request
    ctx = Context(0)
    req = client_request("/chat", "snf4j.org", KEY, subprotocols=("superchat", "chat"),
                         extension_offers=("permessage-deflate" + offer_params,))
    server = BatchHandshaker(HandshakeConfig(negotiation=Negotiation(("chat",), DeflateNegotiation(*server_pair))),
                             ctx)
    client = BatchClientHandshaker(ClientConfig(negotiation=Negotiation(("superchat", "chat"),
                                                                        DeflateNegotiation(*client_pair))), ctx)
    s = server.accept([req])[0]
    assert s.switched and s.subprotocol == "chat" and s.deflate is not None, s
    c = client.validate([s.response], [KEY])[0]
    assert c.finished and c.subprotocol == "chat" and c.deflate is not None, c
    # (serverNoContext, clientNoContext) on the server is (clientNoContext, serverNoContext) on the client
    assert s.deflate == (c.deflate[1], c.deflate[0]), (s, c)
    enc_no_context, dec_no_context = s.deflate[0], c.deflate[1]
    assert enc_no_context == dec_no_context
    # two 1 KiB messages of two fragments each through the server's encoder and the client's decoder
    rng = random.Random(5)
    words = [b"alpha", b"beta", b"gamma", b"delta", b"websocket", b"deflate"]
    body = b" ".join(rng.choice(words) for _ in range(400))[:2048]
    desc = np.zeros(4, dtype=DESC_DTYPE)
    desc["payload_off"], desc["payload_len"] = [0, 512, 1024, 1536], 512
    desc["opcode"], desc["flags"] = [1, 0, 1, 0], [0x00, 0x80, 0x00, 0x80]
    sf = np.array([0, 4], dtype=np.uint32)
    out, od = ctx.deflate_host(6, enc_no_context, desc, sf, np.frombuffer(body, np.uint8),
                               np.zeros(1, DEFLATE_STATE_DTYPE), np.zeros(DEFLATE_SESSION_BYTES, np.uint8))
    assert all(int(o["flags"]) & 0x02 for o in od) and int(od[0]["flags"]) & 0x40 and int(od[2]["flags"]) & 0x40
    wire = od.copy()
    wire["flags"] &= 0xF0   # FIN and RSV travel; WSG_DESC_DEFLATED is the encoder's note, not a frame bit
    wire["status"] = 0
    got, odesc, res, rf = ctx.inflate_host(dec_no_context, wire, sf, np.concatenate([out, np.zeros(16, np.uint8)]),
                                           np.zeros(1, INFLATE_STATE_DTYPE), np.zeros(32768, np.uint8),
                                           np.array([0, 4096], dtype=np.uint64))
    assert int(res["error"][0]) == 0 and int(res["n_delivered"][0]) == 4 and int(rf[0]) == 0xFFFFFFFF
    plain = b"".join(got[int(o["payload_off"]):int(o["payload_off"]) + int(o["payload_len"])].tobytes() for o in odesc)
    assert plain == body
    ctx.close()
