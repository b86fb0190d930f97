"""Server handshake with the negotiation on the GPU (k_hs_accept_neg through
BatchHandshaker with a Negotiation) against tests/hsnegotiate.py, the restatement of
Handshaker.acceptSubProtocol / acceptExtensions over one PerMessageDeflateExtension
that tests/test_hsnegotiate_model.py pins to the reference's own test vectors."""
import pytest

from oracle import handshake_oracle as H
from tests import hsgen, hsneggen
from tests import hsnegotiate as N
from tests.golden import fixtures

pytestmark = pytest.mark.gpu

KEY = "dGhlIHNhbXBsZSBub25jZQ=="


def _negotiation(st: N.Settings):
    from snf4j_amd import DeflateNegotiation, Negotiation
    return Negotiation(tuple(st.subprotocols), DeflateNegotiation(*st.deflate) if st.deflate else None,
                       st.other_extensions)


def _gpu(requests, st: N.Settings, **cfg):
    from snf4j_amd import BatchHandshaker, HandshakeConfig
    c = HandshakeConfig(cfg.get("max_length", 65536), cfg.get("ignore_host", False), False, False,
                        cfg.get("host_policy", False), _negotiation(st))
    return BatchHandshaker(c).accept(requests)


def _deflate(ext: int):
    """HandshakeOutcome.deflate of the model's EXT_* bits: (serverNoContext, clientNoContext)."""
    return (bool(ext & N.EXT_SERVER_NC), bool(ext & N.EXT_CLIENT_NC)) if ext & N.EXT_DEFLATE else None


def _expect_equal(req, g, r):
    if r["kind"] == H.DEFER:
        assert (g.kind, g.cause) == (H.DEFER, r["cause"]), (req, g, r)
        assert g.subprotocol is None and g.deflate is None, (req, g)
        return
    assert r["kind"] is not None, (req, g)
    assert (g.kind, g.status, g.cause) == (r["kind"], r["status"], r["cause"]), (req, g, r)
    assert g.response == r["response"], (req, g, r)
    assert g.message == N.message(r), (req, g, r)
    assert (g.subprotocol, g.deflate) == (r["subprotocol"], _deflate(r["ext"])), (req, g, r)
    if r["frame_len"]:
        assert g.frame_len == r["frame_len"], (req, g, r)


def test_negotiate_kat_gpu():
    for v in fixtures.load("handshake_negotiate"):
        if v["kind"] == "server":
            g = _gpu([hsneggen.server_request(v, KEY)], hsneggen.settings(v))[0]
            e = v["expect"]
            assert (g.kind, g.status, g.cause, g.message) == (H.ACCEPT, e["status"], 0, None), (v, g)
            assert g.response == hsneggen.expected_response(e, KEY), (v, g)
            assert (g.subprotocol, g.deflate) == (e["protocol"], None), (v, g)
        elif v["kind"] == "accept_offer":
            # one offer through the whole path: declined or a wrong name gives the plain 101,
            # a throw the 400
            st = N.Settings((), (v["compress"], v["decompress"]), False)
            req = hsneggen.server_request(dict(protocol=None, extensions=v["element"]), KEY)
            g, e = _gpu([req], st)[0], v["expect"]
            if e is not None and "error" in e:
                assert (g.status, g.cause, g.message) == (400, 24, "Invalid websocket request extension"), (v, g)
                assert g.response == b"HTTP/1.1 400 Bad Request\r\n\r\n" and g.deflate is None, (v, g)
                continue
            assert g.switched and g.deflate == (None if e is None else (e["sn"], e["cn"])), (v, g)
            ext = v.get("response") or (None if e is None else N.join_extension(N.response_items(e)))
            assert g.response == hsneggen.expected_response(dict(status=101, protocol=None, extensions=ext), KEY), (v, g)
        elif v["kind"] == "parse" and "error" in v["expect"]:
            # every InvalidExtensionException text is the same 400 on this side
            req = hsneggen.server_request(dict(protocol=None, extensions=v["element"]), KEY)
            g = _gpu([req], N.Settings((), (N.OPTIONAL, N.OPTIONAL), False))[0]
            named = N.split_extension(v["element"])[0] == N.NAME      # (the upper-cased vectors are not parsed)
            assert (g.status, g.cause) == ((400, 24) if named else (101, 0)), (v, g)


@pytest.mark.parametrize("seed", range(3))
def test_negotiate_random_gpu(seed):
    results = []
    for st, reqs in hsneggen.server_groups(seed):
        model = [N.accept(r, st) for r in reqs]
        for req, g, r in zip(reqs, _gpu(reqs, st), model):
            _expect_equal(req, g, r)
        results += [(r, hsneggen.offered_deflate(req)) for req, r in zip(reqs, model)]
    # the model alone reaches every class of verdict often enough that a kernel which
    # always deferred (or never negotiated) could not have passed
    hsneggen.assert_server_coverage(results)


def _req(protocol=None, extensions=None):
    return hsneggen.server_request(dict(protocol=protocol, extensions=extensions), KEY)


def test_negotiate_edges_gpu():
    oo = N.Settings(("chat", "superchat"), (N.OPTIONAL, N.OPTIONAL), False)
    reqs = [_req(None, hsneggen.BROWSER_OFFER),
            # a declined first offer (server_max_window_bits below 15), then an accepted one
            _req("superchat, chat", "permessage-deflate; server_max_window_bits=10, permessage-deflate; "
                                    "server_no_context_takeover"),
            # an accepted offer, then an invalid one: every offer is parsed
            _req(None, "permessage-deflate, permessage-deflate; client_max_window_bits=7"),
            _req(None, "permessage-deflate, permessage-deflate; x"),
            _req(None, "x-webkit-deflate-frame; bogus==, permessage-deflate; client_no_context_takeover"),
            _req(None, 'permessage-deflate; client_max_window_bits="15"; server_max_window_bits = +015'),
            _req(None, 'permessage-deflate; client_max_window_bits=" 15"'),
            _req(None, "permessage-deflate; server_max_window_bits=\"\""),
            _req(None, "permessage-deflate; =1"), _req(None, ";, ;permessage-deflate;;"), _req(None, ", ,"),
            _req("zz", None), _req("", ""), _req(",chat", ",")]
    outs = _gpu(reqs, oo)
    for req, g in zip(reqs, outs):
        _expect_equal(req, g, N.accept(req, oo))
    assert outs[0].switched and outs[0].deflate == (False, False) and outs[0].response.endswith(
        b"=\r\nSec-WebSocket-Extensions: permessage-deflate\r\n\r\n")
    assert outs[1].switched and outs[1].deflate == (True, False) and outs[1].subprotocol == "superchat"
    assert outs[1].response.endswith(b"\r\nSec-WebSocket-Protocol: superchat\r\nSec-WebSocket-Extensions: "
                                     b"permessage-deflate; server_no_context_takeover\r\n\r\n")
    assert [(o.status, o.cause) for o in outs[2:4]] == [(400, 24), (400, 24)]
    assert outs[4].deflate == (False, True)
    # REQUIRED on both sides puts both parameters into the answer of a bare offer
    rr = N.Settings((), (N.REQUIRED, N.REQUIRED), False)
    g = _gpu([reqs[0]], rr)[0]
    _expect_equal(reqs[0], g, N.accept(reqs[0], rr))
    assert g.deflate == (True, True) and g.response.endswith(
        b"permessage-deflate; client_no_context_takeover; server_no_context_takeover\r\n\r\n")


def test_negotiate_token_cap_gpu():
    """A chosen subprotocol of WSG_HS_NEG_MAX_TOKEN bytes is answered, one byte more is
    deferred; an unmatched long token is no reason to defer."""
    from snf4j_amd import _lib
    assert _lib.HS_NEG_MAX_TOKEN == N.MAX_TOKEN
    at, over = "a" * N.MAX_TOKEN, "b" * (N.MAX_TOKEN + 1)
    star = N.Settings(("*",), (N.REQUIRED, N.REQUIRED), False)
    reqs = [_req(at, hsneggen.BROWSER_OFFER), _req(over, hsneggen.BROWSER_OFFER), _req("x, " + over, None)]
    outs = _gpu(reqs, star)
    for req, g in zip(reqs, outs):
        _expect_equal(req, g, N.accept(req, star))
    assert outs[0].subprotocol == at and len(outs[0].response) <= _lib.HS_NEG_RESP_STRIDE - 16
    assert (outs[1].kind, outs[1].cause) == (H.DEFER, H.D_SUBPROTOCOL)
    assert outs[2].subprotocol == "x"
    listed = N.Settings((at, over, "chat"), None, False)
    outs = _gpu([_req("chat, " + over), _req(over + ", chat"), _req(at)], listed)
    assert outs[0].subprotocol == "chat" and outs[1].kind == H.DEFER and outs[2].subprotocol == at


def test_negotiate_other_extensions_and_none_gpu():
    """other_extensions defers an extensions field as the old path does; without a
    Negotiation the outcomes are the old entry point's."""
    from snf4j_amd import BatchHandshaker, HandshakeConfig
    import random
    other = N.Settings(("chat",), (N.OPTIONAL, N.OPTIONAL), True)
    reqs = [_req("chat", hsneggen.BROWSER_OFFER), _req("chat", None), _req("chat", "")]
    outs = _gpu(reqs, other)
    for req, g in zip(reqs, outs):
        _expect_equal(req, g, N.accept(req, other))
    assert (outs[0].kind, outs[0].cause) == (H.DEFER, H.D_EXTENSION) and outs[1].subprotocol == "chat"
    rng = random.Random(99)
    batch = [hsneggen.request(rng) for _ in range(600)] + [hsgen.request(rng) for _ in range(400)]
    for flags in ((False, False), (True, True)):
        old = BatchHandshaker(HandshakeConfig(65536, False, *flags)).accept(batch)
        for req, g in zip(batch, old):
            d = H.gpu_defers(req, subprotocols=flags[0], extensions=flags[1])
            r = H.accept(req, subprotocols=flags[0], extensions=flags[1])
            if d is not None:
                assert (g.kind, g.cause) == (H.DEFER, d), (req, g)
            else:
                assert (g.kind, g.status, g.cause, g.response) == (r["kind"], r["status"], r["cause"], r["response"])
            assert g.subprotocol is None and g.deflate is None
    # lists beyond the ABI caps fall back to the old flags: offers are deferred
    big = N.Settings(tuple("p%d" % i for i in range(17)), (N.OPTIONAL, N.OPTIONAL), False)
    outs = _gpu([_req("p3", None), _req(None, hsneggen.BROWSER_OFFER), _req(None, None)], big)
    assert [(o.kind, o.cause) for o in outs[:2]] == [(H.DEFER, H.D_SUBPROTOCOL), (H.DEFER, H.D_EXTENSION)]
    assert outs[2].switched


def test_negotiate_rejects_malformed_settings_gpu():
    """WSG_API_EINVAL for a malformed wsg_hs_negotiation."""
    import numpy as np
    from snf4j_amd import Context, _lib
    from snf4j_amd._lib import HsConfig, HsNegotiation
    ctx = Context(0)
    req = np.frombuffer(_req(), dtype=np.uint8)
    off = np.array([0, req.size], dtype=np.uint64)

    def call(**kw):
        g = HsNegotiation()
        g.n_protocols, g.protocol_off[1], g.protocol_off[2] = 2, 4, 5
        for k, val in kw.items():
            if k == "off":
                for i, x in enumerate(val):
                    g.protocol_off[i] = x
            else:
                setattr(g, k, val)
        return ctx.handshake_accept_negotiate_host(HsConfig(65536, 0, 0, 0, 0), g, req, off)

    assert int(call()[1]["http_status"][0]) == 101
    for bad in (dict(n_protocols=17), dict(off=[0, 5, 4]), dict(off=[1, 4, 5]), dict(off=[0, 4, 257]),
                dict(compress_no_context=3), dict(decompress_no_context=3), dict(deflate=2), dict(other_extensions=2)):
        with pytest.raises(_lib.WsgError, match="malformed"):
            call(**bad)
    ctx.close()
