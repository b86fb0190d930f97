#!/usr/bin/env python3
"""Kernel time of the server handshake with and without the negotiation on the device
(DESIGN.md §8): k_hs_accept against k_hs_accept_neg on bench.py's handshake batch
(2^20 browser-like upgrade requests, random keys), and k_hs_accept_neg on the same
requests carrying the browser's extension offer and a subprotocol.

  python tools/time_handshake_negotiate.py [--n 1048576] [--steps 10] [--rounds 7]

Each launch is bracketed by a HIP event pair on the context's stream (the library's own
kernel timing, wsg_set_timing).  The three cases alternate within a round, so drift of
the machine lands on all of them; a case's figure is the median over the rounds of its
mean launch time, its spread the min..max over the rounds.  Prints one JSON line.
Needs a GPU: there is no CPU path."""
import argparse
import base64
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def batch(n, extra):
    """bench.py handshake_line's batch, with `extra` header fields before the key."""
    from oracle import handshake_oracle as H
    tmpl = H.request("/chat?room=lobby", [
        ("Host", "ws.example.com:8080"), ("Connection", "Upgrade"), ("Pragma", "no-cache"),
        ("Cache-Control", "no-cache"), ("User-Agent", "Mozilla/5.0 (X11; Linux x86_64) AppleWebKit/537.36"),
        ("Upgrade", "websocket"), ("Origin", "https://example.com"), ("Sec-WebSocket-Version", "13"),
        ("Accept-Encoding", "gzip, deflate, br"), ("Accept-Language", "en-US,en;q=0.9")] + extra + [
        ("Sec-WebSocket-Key", "A" * 24)])
    kpos = tmpl.index(b"A" * 24)
    raw = np.random.default_rng(0x4A5).integers(0, 256, (n, 16), dtype=np.uint8)
    k24 = np.frombuffer(b"".join(base64.b64encode(r.tobytes()) for r in raw), dtype=np.uint8).reshape(n, 24)
    buf = np.tile(np.frombuffer(tmpl, dtype=np.uint8), (n, 1))
    buf[:, kpos:kpos + 24] = k24
    return buf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    import torch
    from snf4j_amd import Context, DeflateNegotiation, Negotiation
    from snf4j_amd._lib import (HS_NEG_RESP_STRIDE, HS_NEGOTIATED_DTYPE, HS_RESP_STRIDE, HS_RESULT_DTYPE, HsConfig)
    from tests import hsnegotiate as N
    assert torch.cuda.is_available(), "needs a GPU"
    dev, n = torch.device("cuda:0"), a.n
    ctx = Context(0)
    cfg = HsConfig(65536, 0, 0, 0, 0)
    neg = Negotiation(("chat", "superchat"), DeflateNegotiation()).native()
    none = Negotiation().native()
    st = N.Settings(("chat", "superchat"), (N.OPTIONAL, N.OPTIONAL), False)
    plain = batch(n, [])
    offer = batch(n, [("Sec-WebSocket-Extensions", "permessage-deflate; client_max_window_bits"),
                      ("Sec-WebSocket-Protocol", "superchat, chat")])
    resp = torch.empty(n * HS_NEG_RESP_STRIDE, dtype=torch.uint8, device=dev)
    res = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    ng = torch.empty(n * 8, dtype=torch.uint8, device=dev)

    def dev_batch(buf):
        return (torch.from_numpy(buf.reshape(-1)).to(dev),
                torch.arange(n + 1, dtype=torch.int64, device=dev) * buf.shape[1])

    p_req, p_off = dev_batch(plain)
    o_req, o_off = dev_batch(offer)
    cases = {
        "k_hs_accept plain": ("k_hs_accept", lambda: ctx.handshake_accept_device(cfg, p_req, p_off, resp, res, n=n)),
        "k_hs_accept_neg plain": ("k_hs_accept_neg", lambda: ctx.handshake_accept_negotiate_device(
            cfg, neg, p_req, p_off, resp, res, ng, n=n)),
        "k_hs_accept_neg offer": ("k_hs_accept_neg", lambda: ctx.handshake_accept_negotiate_device(
            cfg, neg, o_req, o_off, resp, res, ng, n=n)),
        # the same longer requests with nothing configured (both fields ignored): what the
        # two extra header lines cost before any of the negotiation runs
        "k_hs_accept_neg offer, no lists": ("k_hs_accept_neg", lambda: ctx.handshake_accept_negotiate_device(
            cfg, none, o_req, o_off, resp, res, ng, n=n)),
    }
    # results first: every request switches, and the two kernels write the same bytes for plain requests
    outs = {}
    for name, (_, step) in cases.items():
        step()
        torch.cuda.synchronize(dev)
        r = res.cpu().numpy().view(HS_RESULT_DTYPE).copy()
        assert (r["http_status"] == 101).all(), name
        stride = HS_RESP_STRIDE if name == "k_hs_accept plain" else HS_NEG_RESP_STRIDE
        rl = int(r["resp_len"][0])
        outs[name] = (r, resp.cpu().numpy()[:n * stride].reshape(n, stride)[:, :rl].copy(),
                      ng.cpu().numpy().view(HS_NEGOTIATED_DTYPE).copy())
    assert np.array_equal(outs["k_hs_accept plain"][0], outs["k_hs_accept_neg plain"][0])
    assert np.array_equal(outs["k_hs_accept plain"][1], outs["k_hs_accept_neg plain"][1])
    g = outs["k_hs_accept_neg offer"][2]
    assert (g["ext"] == 1).all() and (g["proto_len"] == 9).all()
    assert not outs["k_hs_accept_neg offer, no lists"][2].view(np.uint64).any()
    for i in (0, n // 2, n - 1):
        assert outs["k_hs_accept_neg offer"][1][i].tobytes() == N.accept(offer[i].tobytes(), st)["response"], i
    ctx.set_timing(True)
    per = {name: [] for name in cases}
    for rnd in range(a.rounds + 1):           # round 0 warms up
        for name, (kernel, step) in cases.items():
            ctx.reset_timing()
            for _ in range(a.steps):
                step()
            ctx.sync()
            ms, cnt = ctx.timing()[kernel]
            assert cnt == a.steps, (name, cnt)
            if rnd:
                per[name].append(ms / cnt)
    out = {"n": n, "request_bytes": {"plain": int(plain.shape[1]), "offer": int(offer.shape[1])},
           "steps": a.steps, "rounds": a.rounds, "unit": "ms per launch",
           "cases": {name: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                     for name, v in per.items()}}
    print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
