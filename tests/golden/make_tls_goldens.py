#!/usr/bin/env python3
"""Generate tests/golden/tls_hellos.json: ClientHellos as the interpreter's OpenSSL writes them, as hex, each with the host name and the
protocol list that were asked for.

A hello is made in memory: ssl.SSLContext.wrap_bio over two ssl.MemoryBIO, do_handshake() (which wants to read, as nobody answers) and
whatever then lies in the outgoing BIO.  No socket is opened.  The cases vary the maximum version (TLS 1.3, TLS 1.2), the host name
(none, 3 .. 72 bytes) and the ALPN list (none, one name, several).  tests/tls_model.py must find in every hello exactly what was asked
for, or this script aborts.  The output is data only.
"""
import json
import os
import ssl
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))

import tls_model as TLS  # noqa: E402

LONG = ".".join(["a" * 20, "b" * 20, "c" * 20, "examp"]) + ".org"          # 72 bytes
assert len(LONG) == 72
# (maximum version, host name or None, ALPN names or None)
CASES = [
    ("1.3", "example.com", ["h2", "http/1.1"]),
    ("1.3", "example.com", None),
    ("1.3", None, ["h2", "http/1.1"]),
    ("1.3", None, None),
    ("1.2", "example.com", ["h2", "http/1.1"]),
    ("1.2", "example.com", None),
    ("1.2", None, ["http/1.1"]),
    ("1.2", None, None),
    ("1.3", "a.b", ["h2"]),
    ("1.3", "www.youtube.com", ["h2", "http/1.1", "spdy/3.1"]),
    ("1.2", "x.io", ["h2"]),
    ("1.3", LONG, ["h2", "http/1.1"]),
    ("1.2", LONG, None),
    ("1.3", "sixteen-byte.net", ["dot"]),
    ("1.3", "mail.example.org", ["imap", "pop3", "managesieve", "acme-tls/1"]),
    ("1.2", "xn--bcher-kva.example", ["h2", "http/1.1"]),
]


def client_hello(max_version: str, host, alpn) -> bytes:
    ctx = ssl.SSLContext(ssl.PROTOCOL_TLS_CLIENT)
    ctx.check_hostname = False
    ctx.verify_mode = ssl.CERT_NONE
    ctx.maximum_version = ssl.TLSVersion.TLSv1_3 if max_version == "1.3" else ssl.TLSVersion.TLSv1_2
    if alpn:
        ctx.set_alpn_protocols(alpn)
    incoming, outgoing = ssl.MemoryBIO(), ssl.MemoryBIO()
    obj = ctx.wrap_bio(incoming, outgoing, server_hostname=host)
    try:
        obj.do_handshake()
    except ssl.SSLWantReadError:
        pass
    return outgoing.read()


def main() -> None:
    out = []
    for max_version, host, alpn in CASES:
        p = client_hello(max_version, host, alpn)
        t = TLS.locate(p)
        assert t is not None and not t["flags"] & TLS.TRUNCATED, (max_version, host, alpn)
        assert t["sni"] == (host.encode() if host else None), (host, t["sni"])
        assert t["alpn"] == (",".join(alpn).encode() if alpn else None), (alpn, t["alpn"])
        assert t["hs_len"] + 9 == len(p) and t["n_alpn"] == len(alpn or [])
        out.append({"max_version": max_version, "sni": host, "alpn": alpn, "hex": p.hex()})
        print(f"TLS {max_version}  {len(p):4d} bytes  {t['n_ext']:2d} extensions  sni {host}  alpn {alpn}")
    with open(os.path.join(HERE, "tls_hellos.json"), "w") as f:
        json.dump({"source": ssl.OPENSSL_VERSION + ", ssl.MemoryBIO; held to tests/tls_model.py", "hellos": out}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
