"""CPU restatement of the reference's handshake negotiation, the checker of
k_hs_accept_neg / k_hs_validate_neg (TEST INFRASTRUCTURE ONLY).

Restated from (paths under snf4j-websocket/src/main/java/org/snf4j/websocket/):
  handshake/Handshaker.java:259-278     acceptSubProtocol
  handshake/Handshaker.java:294-325     acceptExtensions
  handshake/Handshaker.java:386-403     the 101 response's two extra fields
  handshake/Handshaker.java:462-485     validateSubProtocol
  handshake/Handshaker.java:487-533     validateExtensions
  handshake/HandshakeUtils.java:195-247 extension(String) / extension(List)
  handshake/HttpUtils.java:319-334      values(s, regex)
  extensions/compress/PerMessageDeflateParams.java:83-154     set / setInt / parse
  extensions/compress/PerMessageDeflateExtension.java:177-301 wrongName / acceptOffer /
                                                              validateResponse / response

Everything before the negotiation is oracle.handshake_oracle's: accept / validate are
called with `subprotocols` and `extensions` off (negotiation is the last step on both
sides, so the base verdict decides all that comes before), and gpu_defers /
gpu_defers_client likewise for the deferred forms that remain.
tests/golden/handshake_negotiate_kat.json pins this file to the reference's own tests.
"""
from __future__ import annotations

from dataclasses import dataclass

from oracle import handshake_oracle as H

FORBIDDEN, OPTIONAL, REQUIRED = 0, 1, 2
NAME = "permessage-deflate"
MAX_TOKEN = 96                       # WSG_HS_NEG_MAX_TOKEN: a longer chosen subprotocol is deferred
EXT_DEFLATE, EXT_CLIENT_NC, EXT_SERVER_NC = 1, 2, 4

C_INVALID_REQUEST_EXTENSION = 24
C_EXT_DUPLICATED, C_EXT_UNNECESSARY_VALUE, C_EXT_MISSING_VALUE = 25, 26, 27
C_EXT_VALUE_FORMAT, C_EXT_VALUE, C_EXT_UNEXPECTED = 28, 29, 30
EXT_TEXTS = {C_EXT_DUPLICATED: "Duplicated parameter", C_EXT_UNNECESSARY_VALUE: "Unnecessary parameter value",
             C_EXT_MISSING_VALUE: "Missing parameter value", C_EXT_VALUE_FORMAT: "Invalid parameter value format",
             C_EXT_VALUE: "Invalid parameter value", C_EXT_UNEXPECTED: "Unexpected parameter"}
MESSAGES = dict(H.MESSAGES)
MESSAGES[C_INVALID_REQUEST_EXTENSION] = "Invalid websocket request extension"
MESSAGES.update({c: "Invalid extension: " + t for c, t in EXT_TEXTS.items()})


class InvalidExtension(Exception):
    def __init__(self, cause):
        super().__init__(EXT_TEXTS[cause])
        self.cause = cause


@dataclass(frozen=True)
class Settings:
    """The config the negotiation reads: getSupportedSubProtocols() and a
    getSupportedExtensions() of at most one PerMessageDeflateExtension."""
    subprotocols: tuple = ()
    deflate: tuple | None = None      # (compressNoContext, decompressNoContext)
    other_extensions: bool = False


def values(s: str, sep: str = ",") -> list:
    """HttpUtils.values(s, regex): split, trim, drop the empty ones."""
    if not s:
        return []
    return [t for t in (H.java_trim(x) for x in s.split(sep)) if t]


def split_extension(ext: str) -> list:
    """HandshakeUtils.extension(String): [name, p1, v1 | None, p2, ...]."""
    items = values(ext, ";")
    if len(items) <= 1:
        return items
    out = [items[0]]
    for item in items[1:]:
        pos = item.find("=")
        if pos >= 0:
            value = H.java_trim(item[pos + 1:])
            if len(value) > 1 and value[0] == '"' and value[-1] == '"':
                value = value[1:-1]
            out += [H.java_trim(item[:pos]), value]
        else:
            out += [item, None]
    return out


def join_extension(items: list) -> str:
    """HandshakeUtils.extension(List)."""
    s = items[0]
    for i in range(1, len(items), 2):
        s += "; " + items[i]
        if items[i + 1] is not None:
            s += "=" + items[i + 1]
    return s


def parse_params(ext: list) -> dict:
    """PerMessageDeflateParams.parse: cn / sn booleans, cx / sx None, -1 (no value) or 8..15."""
    names = ["client_no_context_takeover", "server_no_context_takeover", "client_max_window_bits",
             "server_max_window_bits"]
    val = [0, 0, 0, 0]
    for i in range(1, len(ext), 2):
        p, v = ext[i], ext[i + 1]
        k = names.index(p.lower()) if p.lower() in names else -1   # equalsIgnoreCase (ASCII here)
        if k < 0:
            raise InvalidExtension(C_EXT_UNEXPECTED)
        if val[k] != 0:
            raise InvalidExtension(C_EXT_DUPLICATED)
        if k < 2:
            if v is not None:
                raise InvalidExtension(C_EXT_UNNECESSARY_VALUE)
            val[k] = -1
            continue
        if v is None:
            if k == 3:
                raise InvalidExtension(C_EXT_MISSING_VALUE)
            val[k] = -1
            continue
        x = H.parse_int(v)
        if x is None:
            raise InvalidExtension(C_EXT_VALUE_FORMAT)
        if not 8 <= x <= 15:
            raise InvalidExtension(C_EXT_VALUE)
        val[k] = x
    return dict(cn=val[0] == -1, sn=val[1] == -1, cx=val[2] or None, sx=val[3] or None)


def accept_offer(ext: list, compress: int, decompress: int):
    """PerMessageDeflateExtension.acceptOffer: None (wrong name or declined) or
    dict(cn, sn) of the accepted extension's params."""
    if len(ext) < 1 or ext[0] != NAME:
        return None
    p = parse_params(ext)
    cn = sn = False
    if p["cn"]:
        if decompress == FORBIDDEN:
            return None
        cn = True
    elif decompress == REQUIRED:
        cn = True
    if p["sn"]:
        if compress == FORBIDDEN:
            return None
        sn = True
    elif compress == REQUIRED:
        sn = True
    if p["sx"] is not None and p["sx"] < 15:
        return None
    return dict(cn=cn, sn=sn)


def validate_response(ext: list, compress: int, decompress: int):
    """PerMessageDeflateExtension.validateResponse."""
    if len(ext) < 1 or ext[0] != NAME:
        return None
    p = parse_params(ext)
    cn = sn = False
    if p["cn"]:
        if compress == FORBIDDEN:
            return None
        cn = True
    elif compress == REQUIRED:
        return None
    if p["sn"]:
        if decompress == FORBIDDEN:
            return None
        sn = True
    elif decompress == REQUIRED:
        return None
    if p["cx"] is not None and p["cx"] < 15:   # (a client_max_window_bits without a value is -1)
        return None
    return dict(cn=cn, sn=sn)


def response_items(params: dict) -> list:
    """PerMessageDeflateExtension.response()."""
    out = [NAME]
    if params["cn"]:
        out += ["client_no_context_takeover", None]
    if params["sn"]:
        out += ["server_no_context_takeover", None]
    return out


def _ext_bits(params) -> int:
    if params is None:
        return 0
    return EXT_DEFLATE | (EXT_CLIENT_NC if params["cn"] else 0) | (EXT_SERVER_NC if params["sn"] else 0)


def _fields(data: bytes, flen: int, client: bool):
    lines = H.available(data)[1]
    return (H.parse_response(data[:flen], lines)[1] if client else H.parse_request(data[:flen], lines))


def accept(data: bytes, st: Settings, max_length=65536, ignore_host=False, host_policy=False) -> dict:
    """HandshakeDecoder.decode + Handshaker.accept with the negotiation of `st`, as
    k_hs_accept_neg answers: oracle.accept's dict plus subprotocol (str | None) and
    ext (EXT_* bits); kind DEFER with the cause for what the kernel defers."""
    d = H.gpu_defers(data, max_length, ignore_host, False, False, host_policy)
    r = dict(H.accept(data, max_length, ignore_host, False, False, host_policy), subprotocol=None, ext=0)
    if d is not None:
        return dict(r, kind=H.DEFER, status=0, cause=d, detail=None, response=b"")
    if not (r["kind"] == H.ACCEPT and r["status"] == 101):
        return r
    f = _fields(data, r["frame_len"], False)
    sub = None
    s = f.get("Sec-WebSocket-Protocol")                       # acceptSubProtocol
    if s and st.subprotocols:
        for req in values(s):
            if any(sup == "*" or req == sup for sup in st.subprotocols):
                sub = req
                break
    if sub is not None and len(sub) > MAX_TOKEN:
        return dict(r, kind=H.DEFER, status=0, cause=H.D_SUBPROTOCOL, response=b"")
    params = None
    s = f.get("Sec-WebSocket-Extensions")                     # acceptExtensions
    if s:
        if st.other_extensions:
            return dict(r, kind=H.DEFER, status=0, cause=H.D_EXTENSION, response=b"")
        if st.deflate is not None:
            try:
                for e in values(s):
                    p = accept_offer(split_extension(e), *st.deflate)
                    if p is not None and params is None:
                        params = p
            except InvalidExtension:
                return dict(r, status=400, cause=C_INVALID_REQUEST_EXTENSION, response=H.format_response(400, []))
    fields = [("Upgrade", "websocket"), ("Connection", "Upgrade"),
              ("Sec-WebSocket-Accept", H.answer_key(f.get("Sec-WebSocket-Key")))]
    if sub is not None:
        fields.append(("Sec-WebSocket-Protocol", sub))
    if params is not None:
        fields.append(("Sec-WebSocket-Extensions", join_extension(response_items(params))))
    return dict(r, response=H.format_response(101, fields), subprotocol=sub, ext=_ext_bits(params))


def validate(data: bytes, key: str, st: Settings, max_length=65536) -> dict:
    """HandshakeDecoder(clientMode).decode + Handshaker.validate with the negotiation of
    `st`, as k_hs_validate_neg answers: oracle.validate's dict plus ext (EXT_* bits)."""
    d = H.gpu_defers_client(data, key, max_length, None, False)
    r = dict(H.validate(data, key, max_length, None, False), ext=0)
    if d is not None:
        return dict(r, kind=H.DEFER, cause=d, detail=None)
    # the base run (no lists configured) decides everything up to the key challenge: its
    # verdicts from there on are the ones the lists change
    if not (r["kind"] == H.FINISHED or
            (r["kind"] == H.CLOSING and r["cause"] in (H.C_INVALID_SUBPROTOCOL, H.C_INVALID_EXTENSIONS))):
        return r
    r.update(kind=H.CLOSING, cause=H.C_NONE, detail=None, subprotocol=None)
    f = _fields(data, r["frame_len"], True)
    received = f.get("Sec-WebSocket-Protocol")                 # validateSubProtocol
    if st.subprotocols:
        if received is None:
            return dict(r, cause=H.C_MISSING_SUBPROTOCOL)
        if received not in st.subprotocols:
            return dict(r, cause=H.C_INVALID_SUBPROTOCOL, detail=received)
        r["subprotocol"] = received
    elif received is not None:
        return dict(r, cause=H.C_INVALID_SUBPROTOCOL, detail=received)
    received = f.get("Sec-WebSocket-Extensions")               # validateExtensions
    params = None
    if received is not None:
        if st.other_extensions:
            return dict(r, kind=H.DEFER, cause=H.D_EXTENSION, subprotocol=None)
        if st.deflate is None:
            return dict(r, cause=H.C_INVALID_EXTENSIONS, subprotocol=None)
        for e in values(received):
            try:
                p = validate_response(split_extension(e), *st.deflate)
            except InvalidExtension as x:
                return dict(r, cause=x.cause, subprotocol=None)
            if p is None or params is not None:
                return dict(r, cause=H.C_INVALID_EXTENSIONS, subprotocol=None)
            params = p
    return dict(r, kind=H.FINISHED, ext=_ext_bits(params))


def message(r: dict):
    """The exception message / closing reason of a verdict."""
    m = MESSAGES.get(r["cause"]) if r["kind"] in (H.PARSE_ERROR, H.ACCEPT, H.CLOSING) else None
    if m and "%s" in m:
        m = m % ((r["detail"], r["expected"]) if r["cause"] == H.C_INVALID_ACCEPT else r["detail"])
    return m
