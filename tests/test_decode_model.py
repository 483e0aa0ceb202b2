"""tests/decode_model.py, the position-wise definition of kmpgpu_load_decoded, against Python's urllib.parse.unquote_to_bytes (with
plus: the same function after '+' was replaced by a space).  No GPU needed."""
from urllib.parse import unquote_to_bytes

import numpy as np
import pytest

import decode_model as DM


def reference(t: bytes, plus: bool) -> bytes:
    return unquote_to_bytes(t.replace(b"+", b" ") if plus else t)


@pytest.mark.parametrize("plus", [False, True])
def test_random_strings_over_the_hostile_alphabet(plus):
    rng = np.random.default_rng(7 + plus)
    n = 60000                                          # per mode: 120 000 strings in all
    lengths = rng.integers(0, 25, n)
    for L in lengths:
        t = DM.random_payload(rng, int(L))
        want = reference(t, plus)
        assert DM.decode(t, plus) == want, t
        assert DM.changed(t, plus) == (want != t), t


@pytest.mark.parametrize("payload, want, want_plus", [
    (b"%%41", b"%A", b"%A"),
    (b"%2%41", b"%2A", b"%2A"),
    (b"%4", b"%4", b"%4"),
    (b"%", b"%", b"%"),
    (b"a%00b", b"a\x00b", b"a\x00b"),
    (b"%2e%2E%2f", b"../", b"../"),
    (b"a%2Bb+c", b"a+b+c", b"a+b c"),
    (b"", b"", b""),
    (b"%41", b"A", b"A"),
    (b"GET /%61dmin", b"GET /admin", b"GET /admin"),
    (b"%252e", b"%2e", b"%2e"),
    (b"%4g%g4%", b"%4g%g4%", b"%4g%g4%"),
])
def test_cases_by_hand(payload, want, want_plus):
    assert DM.decode(payload) == want == reference(payload, False)
    assert DM.decode(payload, plus=True) == want_plus == reference(payload, True)
    assert DM.changed(payload) == (want != payload) and DM.changed(payload, True) == (want_plus != payload)


def test_packed_image_and_bitmap():
    payloads = [b"", b"%41", b"x" * 16, b"a+b", b"%2e" * 11, b"plain"]
    m = DM.load_decoded(payloads)
    assert m["payloads"] == [b"", b"A", b"x" * 16, b"a+b", b"." * 11, b"plain"]
    assert m["off"].tolist() == [0, 16, 32, 48, 64, 80] and m["len"].tolist() == [0, 1, 16, 3, 11, 5]
    assert m["arena"].size == 96 and m["arena"][16:32].tobytes() == b"A" + b"\0" * 15 and not m["arena"][:16].any()
    assert m["changed"].tolist() == [False, True, False, False, True, False] and m["words"].tolist() == [0b010010]
    assert m["index"].tolist() == list(range(6))
    assert m["stats"] == {"n_payloads": 6, "n_changed": 2, "bytes_in": 60, "bytes_out": 36}
    p = DM.load_decoded(payloads, plus=True, only_changed=True)
    assert p["payloads"] == [b"A", b"a b", b"." * 11] and p["index"].tolist() == [1, 3, 4] and p["words"].tolist() == [0b011010]
    assert p["off"].tolist() == [0, 16, 32] and p["stats"] == {"n_payloads": 3, "n_changed": 3, "bytes_in": 39, "bytes_out": 15}
    none = DM.load_decoded([b"abc", b""], only_changed=True)
    assert none["payloads"] == [] and none["arena"].size == 0 and none["words"].tolist() == [0]
    assert DM.words(np.ones(65, dtype=bool)).tolist() == [0xFFFFFFFFFFFFFFFF, 1]


def test_escape_all_shrinks_to_a_third():
    data = bytes(range(256))
    assert DM.decode(DM.escape_all(data)) == data and len(DM.escape_all(data)) == 3 * len(data)
