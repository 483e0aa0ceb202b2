"""tests/base64_model.py, the position-wise definition of kmpgpu_load_base64, against hand-written verdicts and against Python's re +
base64 run by run.  No GPU needed."""
import base64

import numpy as np
import pytest

import base64_model as BM


@pytest.mark.parametrize("urlsafe", [False, True])
@pytest.mark.parametrize("min_run", [4, 5, 8])
def test_random_strings_against_re_and_base64(min_run, urlsafe):
    rng = np.random.default_rng(100 * min_run + urlsafe)
    n = 20000                                          # per case: 120 000 strings in all
    for L in rng.integers(0, 40, n):
        t = BM.random_payload(rng, int(L))
        want = BM.decode_re(t, min_run, urlsafe)
        assert BM.decode(t, min_run, urlsafe) == want, t
        assert BM.changed(t, min_run, urlsafe) == (want != t), t


def test_the_two_authorization_cases():
    t = b"Authorization: Basic YWRtaW46YWRtaW4=\r\n"
    assert BM.decode(t, 14) == b"Authorization: Basic admin:admin\r\n"
    noise = base64.b64decode(b"Authorizatio=")                 # 13 letters, m % 4 == 1: the last one yields nothing
    assert len(noise) == 9
    assert BM.decode(t, 8) == noise + b": Basic admin:admin\r\n"
    assert BM.changed(t, 14) and BM.changed(t, 8) and not BM.changed(t, 16) and BM.decode(t, 16) == t


def test_a_jwt_under_url():
    head, body = b'{"alg":"HS256","typ":"JWT"}', b'{"sub":"1234567890","name":"John Doe","admin":true,"x":"\xfb\xff"}'
    h, b = BM.encode(head, True, pad=False), BM.encode(body, True, pad=False)
    assert b"-" in b or b"_" in b
    t = b"Cookie: jwt=" + h + b"." + b + b".sig\r\n"
    assert BM.decode(t, 16, urlsafe=True) == b"Cookie: jwt=" + head + b"." + body + b".sig\r\n"
    # without the flag '-' and '_' cut the body into runs of their own
    assert BM.decode(t, 16, urlsafe=False) != BM.decode(t, 16, urlsafe=True)


@pytest.mark.parametrize("m, data", [(8, b"foobar"), (9, b"foobar"), (6, b"foob"), (7, b"fooba")])
@pytest.mark.parametrize("n_eq", [0, 1, 2, 3])
def test_every_m_mod_4_with_every_padding(m, data, n_eq):
    run = {8: b"Zm9vYmFy", 9: b"Zm9vYmFyQ", 6: b"Zm9vYg", 7: b"Zm9vYmE"}[m]
    assert len(run) == m
    used = min(n_eq, {2: 2, 3: 1}.get(m % 4, 0))
    t = b"<" + run + b"=" * n_eq + b">"
    assert BM.decode(t, 4) == b"<" + data + b"=" * (n_eq - used) + b">"
    assert BM.decode(t[:-1], 4) == b"<" + data + b"=" * (n_eq - used)      # the '=' end at L
    assert BM.decode(t, m + 1) == t


def test_min_run_is_exact():
    assert BM.decode(b" QUJD ", 4) == b" ABC " and BM.decode(b" QUJD ", 5) == b" QUJD "
    r15, r16 = b"QUJDREVGR0hJSktM"[:15], b"QUJDREVGR0hJSktM"
    assert BM.decode(b"." + r15 + b".", 16) == b"." + r15 + b"."
    assert BM.decode(b"." + r16 + b".", 16) == b".ABCDEFGHIJKL."
    assert BM.decode(b"." + r15 + b".", 15) == b".ABCDEFGHIJK."       # m % 4 == 3: 11 bytes, 2 bits dropped


def test_the_two_alphabets():
    assert BM.decode(b"++//++//", 4) == base64.b64decode(b"++//++//") and BM.decode(b"++//++//", 4, urlsafe=True) == b"++//++//"
    assert BM.decode(b"--__--__", 4, urlsafe=True) == base64.b64decode(b"++//++//") and BM.decode(b"--__--__", 4) == b"--__--__"
    # the other alphabet's two bytes end a run
    assert BM.decode(b"QUJD+QUJD", 4, urlsafe=True) == b"ABC+ABC" and BM.decode(b"QUJD-QUJD", 4) == b"ABC-ABC"
    assert BM.decode(b"QUJD+QUJD", 4) == base64.b64decode(b"QUJD+QUJ")          # one run of 9: the last byte yields nothing


def test_a_run_that_ends_at_the_payloads_end():
    assert BM.decode(b"x=QUJDRA", 4) == b"x=ABCD" and BM.decode(b"QUJDRA=", 4) == b"ABCD" and BM.decode(b"QUJDRA", 4) == b"ABCD"
    assert BM.decode(b"", 4) == b"" and BM.decode(b"QUJ", 4) == b"QUJ" and not BM.changed(b"QUJ", 4)
    assert BM.decode(b"AAAA", 4) == b"\0\0\0"                            # a decoded 0x00 is a byte like any other


def test_packed_image_and_bitmap():
    payloads = [b"", b"QUJD", b"x" * 3 + b"." * 13, b"==QUJDRA==", b"plain text"]
    m = BM.load_base64(payloads, min_run=4)
    assert m["payloads"] == [b"", b"ABC", b"x" * 3 + b"." * 13, b"==ABCD", b"\xa6V\xa2 \xb5\xecm"]
    assert m["off"].tolist() == [0, 16, 32, 48, 64] and m["len"].tolist() == [0, 3, 16, 6, 7]
    assert m["changed"].tolist() == [False, True, False, True, True] and m["words"].tolist() == [0b11010]
    assert m["stats"] == {"n_payloads": 5, "n_changed": 3, "bytes_in": 40, "bytes_out": 32}
    p = BM.load_base64(payloads, min_run=6, only_changed=True)
    assert p["payloads"] == [b"==ABCD"] and p["index"].tolist() == [3] and p["words"].tolist() == [0b01000]
    assert p["stats"] == {"n_payloads": 1, "n_changed": 1, "bytes_in": 10, "bytes_out": 6}
    none = BM.load_base64([b"abc", b""], only_changed=True)
    assert none["payloads"] == [] and none["arena"].size == 0 and none["words"].tolist() == [0]
