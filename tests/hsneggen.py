"""Requests and responses for the negotiation parity tests (tests/hsnegotiate.py is the
checker): builders for the fixture vectors and a grammar-based generator of
Sec-WebSocket-Protocol / Sec-WebSocket-Extensions fields on both sides."""
from __future__ import annotations

import base64
import random

from oracle import handshake_oracle as H
from tests import hsgen
from tests import hsnegotiate as N

PAIRS = [(c, d) for c in (N.FORBIDDEN, N.OPTIONAL, N.REQUIRED) for d in (N.FORBIDDEN, N.OPTIONAL, N.REQUIRED)]
PROTO_LISTS = [("chat", "superchat"), (), ("*",), ("v1.proto", "chat"), ("chat", "*", "x")]
PARAMS = ["client_no_context_takeover", "server_no_context_takeover", "client_max_window_bits",
          "server_max_window_bits"]
VALUES = [None, '""', "7", "8", "15", "16", '"15"', "+15", "015", '" 15"', "x", "-1", "2147483648"]
BROWSER_OFFER = "permessage-deflate; client_max_window_bits"


# ------------------------------------------------------------------ fixture vectors
def settings(v) -> N.Settings:
    return N.Settings(tuple(v["subprotocols"] or ()), tuple(v["deflate"]) if v["deflate"] else None, False)


def _with(fields, v):
    if v["protocol"] is not None:
        fields.append(("Sec-WebSocket-Protocol", v["protocol"]))
    if v["extensions"] is not None:
        fields.append(("Sec-WebSocket-Extensions", v["extensions"]))
    return fields


def server_request(v, key: str) -> bytes:
    return H.request("/uri", _with([("Host", "snf4j.org"), ("Upgrade", "websocket"), ("Connection", "Upgrade"),
                                    ("Sec-WebSocket-Key", key), ("Sec-WebSocket-Version", "13")], v))


def expected_response(e, key: str) -> bytes:
    return H.format_response(e["status"], _with([("Upgrade", "websocket"), ("Connection", "Upgrade"),
                                                 ("Sec-WebSocket-Accept", H.answer_key(key))], e))


def client_response(v, key: str) -> bytes:
    return H.response(101, "Switching Protocols", _with([("Upgrade", "websocket"), ("Connection", "Upgrade"),
                                                         ("Sec-WebSocket-Accept", H.answer_key(key))], v))


# ------------------------------------------------------------------ the grammar
def _case(rng, s):
    r = rng.random()
    return s if r < 0.85 else (s.upper() if r < 0.93 else s.title())


def _blank(rng):
    return rng.choice(["", "", "", " ", "  ", "\t"])


def _wild(rng) -> str:
    """One "name[=value]" item over the whole grammar: any name, any value."""
    name = rng.choice(PARAMS)
    if rng.random() < 0.15:
        name = rng.choice(["", "x", "client_no_context", "server_max_window_bit"])
    value = None if rng.random() < 0.25 else rng.choice(VALUES)
    return _case(rng, name) + ("" if value is None else _blank(rng) + "=" + _blank(rng) + value)


def element(rng: random.Random, tame_p: float = 0.8) -> str:
    """One element of Sec-WebSocket-Extensions (an offer, or a server's answer)."""
    r = rng.random()
    name = N.NAME if r < 0.86 else rng.choice(["Permessage-Deflate", "x-webkit-deflate-frame", ""])
    tame = rng.random() < tame_p
    items = [name]
    k = rng.choice([0, 0, 1, 1, 1, 2, 2, 3])
    names = rng.sample(PARAMS, k) if tame else None
    for j in range(k):
        items.append(_tame(rng, names[j]) if tame else _wild(rng))
    if not tame and k and rng.random() < 0.35:
        items.append(items[-1])                                  # a duplicate
    sep = rng.choice([";", "; ", "; ", " ; "])
    s = sep.join(items)
    if rng.random() < 0.08:
        s += rng.choice([";", ";;", " ;", "=", ";="])             # stray separators
    return s


def _tame(rng, name) -> str:
    """An item that usually parses: no value on the no-context names, 15 (or 8, a decline) on the windows."""
    if not name.endswith("_bits"):
        return _case(rng, name)
    value = rng.choice(["15", "15", "15", '"15"', "+15", "015", "8"] + ([None] * 4 if name == PARAMS[2] else []))
    return _case(rng, name) + ("" if value is None else _blank(rng) + "=" + _blank(rng) + value)


def extensions_field(rng: random.Random, lo=0, hi=3, tame_p=0.8) -> str | None:
    n = rng.randint(lo, hi)
    if n == 0:
        return rng.choice([None, None, "", " , "])
    s = rng.choice([",", ", ", ", ", " , "]).join(element(rng, tame_p) for _ in range(n))
    if rng.random() < 0.05:
        s = rng.choice([",", ", ,"]) + s
    return s


def protocol_field(rng: random.Random) -> str | None:
    r = rng.random()
    if r < 0.35:
        return None
    if r < 0.96:
        return rng.choice(["chat", "superchat, chat", "x, chat", "zzz", "", " chat ,", ",, superchat", "Chat",
                           "v1.proto", "mqtt, v1.proto", "chat;q=1, chat"])
    return rng.choice(["a" * N.MAX_TOKEN, "b" * (N.MAX_TOKEN + 1), "zz, " + "c" * 200])


def _key(rng) -> str:
    return base64.b64encode(bytes(rng.randrange(256) for _ in range(16))).decode()


def request(rng: random.Random) -> bytes:
    """A server request: mostly one that reaches the negotiation, else tests/hsgen's mix."""
    if rng.random() < 0.12:
        return hsgen.request(rng)
    fields = [("Host", "snf4j.org"), ("Upgrade", "websocket"), ("Connection", "Upgrade"),
              ("Sec-WebSocket-Key", _key(rng)), ("Sec-WebSocket-Version", "13")]
    p, e = protocol_field(rng), extensions_field(rng)
    if p is not None:
        fields.append(("Sec-WebSocket-Protocol", p))
    if e is not None:
        fields.append(("Sec-WebSocket-Extensions", e))
    if rng.random() < 0.3:
        rng.shuffle(fields)
    raw = H.request(rng.choice(["/uri", "/chat?room=1"]), fields)
    if rng.random() < 0.1:
        raw += bytes([0x81, 0x85]) + bytes(rng.randrange(256) for _ in range(9))
    return raw


def server_groups(seed: int, n: int = 4000) -> list:
    """[(Settings, requests)]: n requests in all, dealt over the nine NoContext pairs
    (starting at pair `seed`, so the subprotocol lists rotate against them)."""
    rng = random.Random(7000 + seed)
    out = []
    for k in range(9):
        st = N.Settings(PROTO_LISTS[(seed + k) % len(PROTO_LISTS)], PAIRS[(seed + k) % 9], False)
        out.append((st, [request(rng) for _ in range(n // 9 + (k < n % 9))]))
    return out


def server_coverage(results) -> dict:
    """What the model decided, by the classes the random test must exercise."""
    c = dict(deflate_00=0, deflate_c0=0, deflate_0s=0, deflate_cs=0, all_declined=0, invalid_extension=0,
             subprotocol=0)
    for r, offered in results:
        if r["kind"] != H.ACCEPT:
            continue
        if r["status"] == 400 and r["cause"] == N.C_INVALID_REQUEST_EXTENSION:
            c["invalid_extension"] += 1
        if r["status"] != 101:
            continue
        if r["subprotocol"] is not None:
            c["subprotocol"] += 1
        if r["ext"]:
            c["deflate_" + ("c" if r["ext"] & N.EXT_CLIENT_NC else "0")
              + ("s" if r["ext"] & N.EXT_SERVER_NC else "0")] += 1
        elif offered:
            c["all_declined"] += 1
    return c


def offered_deflate(req: bytes) -> bool:
    """The request carries an offer named permessage-deflate (so a 101 without the
    extension means every such offer was declined)."""
    flen, lines, _ = H.available(req)
    if not flen:
        return False
    try:
        s = H.parse_request(req[:flen], lines).get("Sec-WebSocket-Extensions")
    except H.InvalidHandshake:
        return False
    return any(N.split_extension(e)[:1] == [N.NAME] for e in N.values(s or ""))


def assert_server_coverage(results, floor: int = 50):
    c = server_coverage(results)
    assert all(v >= floor for v in c.values()), c


# ------------------------------------------------------------------ client side
def response(rng: random.Random, key: str, st: N.Settings) -> bytes:
    """A server's answer: mostly valid up to the key challenge, then the answers to the
    lists of `st` and their wrong forms."""
    fields = [("Upgrade", "websocket"), ("Connection", "Upgrade"), ("Sec-WebSocket-Accept", H.answer_key(key))]
    r = rng.random()
    if st.subprotocols and r < 0.93:
        fields.append(("Sec-WebSocket-Protocol", rng.choice(list(st.subprotocols) * 8 + ["zzz", "", "chat, superchat",
                                                                                       " chat", "*"])))
    elif not st.subprotocols and r < 0.1:
        fields.append(("Sec-WebSocket-Protocol", "chat"))
    e = extensions_field(rng, 0, 2, tame_p=0.7)
    if e is not None:
        fields.append(("Sec-WebSocket-Extensions", e))
    if rng.random() < 0.2:
        rng.shuffle(fields)
    raw = H.response(101, "Switching Protocols", fields)
    x = rng.random()
    if x < 0.04:
        raw = raw.replace(b"101", b"200", 1)
    elif x < 0.08:
        raw = raw[:rng.randrange(len(raw))]
    elif x < 0.12:
        raw = raw.replace(b"\r\n", b"\r\n folded\r\n", 1)
    elif x < 0.2:
        raw += bytes(rng.randrange(256) for _ in range(rng.randrange(1, 20)))
    return raw


def client_groups(seed: int, n: int = 4000) -> list:
    """[(Settings, keys, responses)] over the nine NoContext pairs."""
    rng = random.Random(8000 + seed)
    out = []
    for k in range(9):
        st = N.Settings(PROTO_LISTS[(seed + k) % len(PROTO_LISTS)], PAIRS[(seed + k) % 9], False)
        keys = [_key(rng) for _ in range(n // 9 + (k < n % 9))]
        out.append((st, keys, [response(rng, key, st) for key in keys]))
    return out
