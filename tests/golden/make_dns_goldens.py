#!/usr/bin/env python3
"""Generate tests/golden/dns_qnames.json: per UDP fixture, how many payloads the definition of kmpgpu_dns_locate (include/kmpgpu.h)
accepts, how many of them are queries and responses, the bytes of all their names, and the table name -> count.

Two formulations must agree on every payload or this script aborts: tests/dns_model.py, and a walk written here on its own.  Where
dnspython is installed, dns.name.from_wire must give the same labels for every accepted payload as well.  The sums must be the ones
written down when the feature was specified (SUMS).  The output is data only; names are written as latin-1 text.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import multithreading_string_matching_amd as K  # noqa: E402
import dns_model as DNS  # noqa: E402

DATA = os.path.join(HERE, "data")
FIXTURES = ["very_big_udp.pcap", "big_udp.pcap"]
# accepted, responses, name bytes
SUMS = {"very_big_udp.pcap": (13768, 6855, 358717), "big_udp.pcap": (1943, None, 45858)}


def walk(p: bytes):
    """the first question's labels, or None: the second formulation"""
    if len(p) < 17 or p[4] << 8 | p[5] == 0:
        return None
    i, labels = 12, []
    while i < len(p) and p[i]:
        c = p[i]
        if c > 63 or i + 1 + c > len(p):
            return None
        labels.append(p[i + 1:i + 1 + c])
        i += 1 + c
    if i >= len(p) or i - 11 > 255 or i + 5 > len(p):
        return None
    return labels


def main() -> None:
    try:
        import dns.name
    except ImportError:
        dns = None
        print("dnspython is not installed: the model and the walk of this script must still agree")
    out = {}
    for pcap in FIXTURES:
        arena = K.HostArena.from_pcap(os.path.join(DATA, pcap), "udp")
        names, queries, responses, name_bytes = {}, 0, 0, 0
        for k in range(arena.n_pkts):
            p = bytes(arena.payload(k))
            t, labels = DNS.locate(p), walk(p)
            assert (t is None) == (labels is None), (pcap, k)
            if t is None:
                continue
            assert t["name"] == b".".join(labels) and t["n_labels"] == len(labels), (pcap, k)
            if dns is not None:
                assert list(dns.name.from_wire(p, 12)[0].labels[:-1]) == labels, (pcap, k)
            queries += t["kind"] == DNS.QUERY
            responses += t["kind"] == DNS.RESPONSE
            name_bytes += t["name_len"]
            key = t["name"].decode("latin-1")
            names[key] = names.get(key, 0) + 1
        accepted = queries + responses
        want = SUMS[pcap]
        assert accepted == want[0] and name_bytes == want[2] and want[1] in (None, responses), (pcap, accepted, responses, name_bytes)
        out[pcap] = {"payloads": arena.n_pkts, "accepted": accepted, "queries": queries, "responses": responses, "name_bytes": name_bytes,
                     "names": dict(sorted(names.items()))}
        print(f"{pcap:20s} {arena.n_pkts:6d} payloads, {accepted:6d} accepted, {responses:6d} responses, {name_bytes:7d} name bytes, {len(names):4d} names")
    with open(os.path.join(HERE, "dns_qnames.json"), "w") as f:
        json.dump({"source": "tests/dns_model.py == the walk of make_dns_goldens.py" + (" == dnspython" if dns is not None else ""),
                   "fixtures": out}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
