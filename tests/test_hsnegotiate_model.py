"""tests/hsnegotiate.py (the checker of the negotiating handshake kernels) against
tests/golden/handshake_negotiate_kat.json: vectors transcribed by hand from the
reference's PerMessageDeflateParamsTest, PerMessageDeflateExtensionTest,
HandshakeUtilsTest.testExtensions and HanshakerTest.  No GPU."""
import pytest

from oracle import handshake_oracle as H
from tests import hsnegotiate as N
from tests import hsneggen
from tests.golden import fixtures

KEY = "dGhlIHNhbXBsZSBub25jZQ=="
VECTORS = fixtures.load("handshake_negotiate")


def _of(kind):
    vs = [v for v in VECTORS if v["kind"] == kind]
    assert vs
    return vs


def test_parse_vectors():
    for v in _of("parse"):
        e = v["expect"]
        ext = N.split_extension(v["element"])
        if "error" in e:
            with pytest.raises(N.InvalidExtension) as x:
                N.parse_params(ext)
            assert str(x.value) == e["error"], v
        else:
            assert N.parse_params(ext) == e, v


def test_split_and_join_vectors():
    for v in _of("split"):
        assert N.split_extension(v["element"]) == v["expect"], v
    for v in _of("join"):
        assert N.join_extension(v["items"]) == v["expect"], v


@pytest.mark.parametrize("kind", ["accept_offer", "validate_response"])
def test_offer_and_response_vectors(kind):
    fn = N.accept_offer if kind == "accept_offer" else N.validate_response
    for v in _of(kind):
        e, ext = v["expect"], N.split_extension(v["element"])
        if e is not None and "error" in e:
            with pytest.raises(N.InvalidExtension) as x:
                fn(ext, v["compress"], v["decompress"])
            assert str(x.value) == e["error"], v
            continue
        got = fn(ext, v["compress"], v["decompress"])
        assert got == e, v
        if "response" in v:
            assert N.join_extension(N.response_items(got)) == v["response"], v
    assert N.accept_offer([], 1, 1) is None and N.validate_response([], 1, 1) is None


def test_server_vectors():
    for v in _of("server"):
        r = N.accept(hsneggen.server_request(v, KEY), hsneggen.settings(v))
        e = v["expect"]
        assert (r["kind"], r["status"], r["subprotocol"]) == (H.ACCEPT, e["status"], e["protocol"]), v
        assert r["response"] == hsneggen.expected_response(e, KEY), v


def test_client_vectors():
    for v in _of("client"):
        r = N.validate(hsneggen.client_response(v, KEY), KEY, hsneggen.settings(v))
        e = v["expect"]
        assert r["kind"] == (H.FINISHED if e["finished"] else H.CLOSING), v
        assert r["subprotocol"] == e["protocol"], v


def test_messages_cover_the_six_texts():
    assert sorted(N.EXT_TEXTS) == list(range(25, 31))
    assert N.MESSAGES[24] == "Invalid websocket request extension"
    assert N.MESSAGES[28] == "Invalid extension: Invalid parameter value format"


def test_generator_coverage_one_seed():
    """The condition the GPU test asserts for each of its seeds, on the model alone."""
    hsneggen.assert_server_coverage([(N.accept(r, st), hsneggen.offered_deflate(r))
                                     for st, reqs in hsneggen.server_groups(0) for r in reqs])
