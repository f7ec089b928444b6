"""CPU tier of the message front ends: the cases of tests/frontend_cases.py through the lanes the gfx950 kernels are built from,
compiled by g++ (tests/emul) — msg_frontend_lane (SHA-256 + strict DER, sha256_dev.h) and the P-256 keyed step behind it, the
secp256k1 _msgs_keyed form, ed_msg_frontend_lane (SHA-512 + mod L, sha512_dev.h) and the Ed25519 _msgs_keyed form.  It proves the
generators and the expected verdicts without a GPU: the conditions on the constructed signatures are asserted here, and the C
oracle, OpenSSL and the Python twins agree wherever more than one of them can judge a case.  tests/test_gpu_frontends.py sends
the same cases to the kernels."""
import ctypes
import hashlib

import pytest

import ed25519_py as ed
import frontend_cases as fc
import p256_py as pc
from test_ed25519_keyed_cpu import kemul as ed_emul  # noqa: F401  (the fixtures that build the emulators)
from test_emul_device_algo import emul  # noqa: F401
from test_k256_keyed_cpu import kemul as k256_emul  # noqa: F401


def _bits(bm, n):
    return [bool((bm[i >> 3] >> (i & 7)) & 1) for i in range(n)]


def _offsets(parts):
    o = (ctypes.c_uint64 * (len(parts) + 1))()
    for i, p in enumerate(parts):
        o[i + 1] = o[i] + len(p)
    return o


def _wrong(cases, got, want):
    return [c.name for c, g, w in zip(cases, got, want) if g != w][:12]


def _calls(scheme):
    """[(what, cases)]: each family in a call of its own, the ladder in both packings, and the all-empty batch"""
    fams = fc.families(scheme)
    out = [(f, cs) for f, cs in sorted(fams.items())]
    out.append(("a shuffled", fc.ladder(scheme)[1]))
    out.append(("all empty", fc.empty_batch(scheme)))
    return out


# ---- the generators' own conditions -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["p256", "k256"])
def test_accepted_integers_of_every_length_exist(scheme):
    """(b): for each of 1, 2, 31, 32 bytes and 32 bytes with a sign byte, an ACCEPTED case has an r of that length and an accepted
    case has an s of that length; every pair has its own key; the short values are where the issue puts them."""
    cases = fc.short_integers(scheme)
    cover = fc.shape_cover(cases)
    for which in "rs":
        for shape in fc.INT_SHAPES:
            assert cover[(which, shape)] >= 1, (which, shape)
    assert all(c.want and c.rule == fc.OWN for c in cases)
    assert len({c.key for c in cases}) == len(cases) == 42
    ints = [tuple(int.from_bytes(b, "big") for b in pc.parse_der_sig(c.sig)) for c in cases]
    assert {s for _, s in ints} == {1, 0x7F, 0x80, 0xFFFF, (1 << 247) + 0x1234, (fc.CURVES[scheme].N - 1) // 2, fc.CURVES[scheme].N - 1}
    assert min(r for r, _ in ints) < 0x80 and len({r for r, _ in ints}) == 6
    # the DER lengths on the wire: 1, 2, 31, 32 and 33 content bytes all occur
    assert {c.sig[3] for c in cases} >= {1, 2, 31, 32, 33}


def test_the_cases_between_the_orders_lie_between_the_orders():
    k, p = fc.between("k256"), fc.between("p256")
    named = {c.name: c for c in k + p}
    r, s = (int.from_bytes(b, "big") for b in pc.parse_der_sig(named["c_r_between_the_orders"].sig))
    assert fc.N_P256 <= r < fc.N_K256 and s < fc.N_P256
    r, s = (int.from_bytes(b, "big") for b in pc.parse_der_sig(named["c_s_between_the_orders"].sig))
    assert fc.N_P256 <= s < fc.N_K256 and r < fc.N_P256
    assert [c.want for c in k] == [True, True, True, False, False, False, False]
    assert [c.want for c in p] == [False, False, True, False]
    # the P-256 cases carry the secp256k1 cases' bytes, and each curve is sent the other's key
    assert named["c_k256_r_between_the_orders"].sig == named["c_r_between_the_orders"].sig
    assert named["c_k256_s_between_the_orders"].sig == named["c_s_between_the_orders"].sig
    assert named["c_k256_key_bytes"].key == named["c_r_between_the_orders"].key in fc.keys("p256")
    assert named["c_p256_key_bytes"].key == named["c_r_below_the_order"].key in fc.keys("k256")
    r, _ = (int.from_bytes(b, "big") for b in pc.parse_der_sig(named["c_r_below_the_order"].sig))
    assert r < fc.N_P256 and all(fc.lift_x(fc.CURVES["p256"], x) is None for x in range(r + 1, fc.N_P256))


@pytest.mark.parametrize("scheme", fc.SCHEMES)
def test_ladder_and_slot_rules_are_what_the_issue_asks(scheme):
    up, shuffled, perm = fc.ladder(scheme)
    assert [len(c.msg) for c in up if c.want] == fc.LADDER_LENGTHS
    assert {len(c.msg) % 128 for c in up} == set(range(128))
    assert len(up) == 266 + 3 * 265 and sorted(perm) == list(range(len(up))) and perm != sorted(perm)
    assert [c.name for c in shuffled] == [up[p].name for p in perm]
    for length in (1, 55, 56, 119, 120, 65537):           # the last byte is part of what is signed
        last = next(c for c in up if c.name == "a_len%d_last_byte_flipped" % length)
        good = next(c for c in up if c.name == "a_len%d" % length)
        assert last.msg[:-1] == good.msg[:-1] and last.msg[-1] != good.msg[-1] and last.sig == good.sig and not last.want
    rules = {c.name: c for c in fc.slot_rules(scheme)}
    for name in ("e_slot_eq_nkeys", "e_slot_ffffffff"):
        c = rules[name]
        assert c.key == fc.keys(scheme)[0] and not c.want and fc.judge(scheme, c.key, c.msg, c.sig)      # slot 0's key accepts it
    assert fc.slot_of(scheme, rules["e_slot_0"]) == 0 and fc.slot_of(scheme, rules["e_slot_eq_nkeys"]) == len(fc.keys(scheme))
    assert fc.slot_of(scheme, rules["e_slot_ffffffff"]) == 0xFFFFFFFF
    assert rules["e_empty_message"].want and rules["e_empty_message"].msg == b""


# ---- the judges against each other --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["p256", "k256"])
def test_oracle_openssl_and_python_twin_agree_on_the_constructed_cases(scheme, openssl_check):
    """(b), (c), (d) and the key cases of (e): `want` is the C oracle's; OpenSSL (strict-DER judge for P-256, the parsed integers for
    secp256k1) and the Python twin give the same verdict, and OpenSSL's strict-DER test equals the Python strict parse on every bend."""
    assert fc.openssl() is not None
    fams = fc.families(scheme)
    cases = fams["b"] + fams["c"] + fams["d"] + [c for c in fams["e"] if c.rule == fc.OWN]
    for c in cases:
        assert fc.judge_openssl(scheme, c.key, c.msg, c.sig) == c.want, c.name
        assert fc.judge_python(scheme, c.key, c.msg, c.sig) == c.want, c.name
    for c in fams["d"]:
        assert bool(fc.openssl().sbvssl_p256_der_is_strict(c.sig, len(c.sig))) == (pc.parse_der_sig(c.sig) is not None), c.name
    assert sum(c.want for c in cases) >= 48 and sum(not c.want for c in cases) >= 140


def test_oracle_openssl_and_python_twin_agree_on_ed25519(openssl_check):
    cases = fc.slot_rules("ed25519") + fc.empty_batch("ed25519") + fc.ladder("ed25519")[0][:80]
    for c in cases:
        if c.rule != fc.OWN:
            continue
        assert fc.judge_openssl("ed25519", c.key, c.msg, c.sig) == c.want, c.name
        assert fc.judge_python("ed25519", c.key, c.msg, c.sig) == c.want, c.name


# ---- the lanes ----------------------------------------------------------------------------------------------------------------------
def test_p256_front_end_lane_and_keyed_step(emul):
    """Every P-256 case through msg_frontend_lane, the message and the signature read in place from the call's packed buffers (so
    the lane starts at every address residue): the record is the strict parse's r | s (zeros when refused) and hashlib's SHA-256.
    The records then go through the emulated keyed step with the cases' slots: the verdicts are `want`, in both packings."""
    V, S = ctypes.c_void_p, ctypes.c_size_t
    keys = fc.keys("p256")
    verdicts = {}
    for what, cases in _calls("p256"):
        msgs, sigs, slots, _, want = fc.batch("p256", cases)
        mbuf, sbuf = ctypes.create_string_buffer(b"".join(msgs) + b"\0"), ctypes.create_string_buffer(b"".join(sigs) + b"\0")
        mo, so = _offsets(msgs), _offsets(sigs)
        recs = ctypes.create_string_buffer(96 * len(cases))
        emul.sbve_msg_frontend.argtypes = [V, S, V, S, V]
        for i, c in enumerate(cases):
            emul.sbve_msg_frontend(ctypes.addressof(mbuf) + mo[i], len(c.msg), ctypes.addressof(sbuf) + so[i], len(c.sig),
                                   ctypes.addressof(recs) + 96 * i)
            rs = fc.strict_rs(c.sig)
            assert recs.raw[96 * i:96 * i + 96] == (rs or bytes(64)) + hashlib.sha256(c.msg).digest(), c.name
        emul.sbve_msg_frontend.argtypes = [ctypes.c_char_p, S, ctypes.c_char_p, S, ctypes.c_char_p]
        bm = ctypes.create_string_buffer((len(cases) + 7) // 8)
        emul.sbve_p256_verify_batch_keyed(recs.raw, (ctypes.c_uint32 * len(cases))(*slots), len(cases), b"".join(keys), len(keys), bm, 64, 1)
        got = _bits(bm.raw, len(cases))
        assert got == want, (what, _wrong(cases, got, want))
        verdicts[what] = got
    perm = fc.ladder("p256")[2]
    assert verdicts["a shuffled"] == [verdicts["a"][p] for p in perm]


def test_secp256k1_msgs_keyed_form(k256_emul):
    """Every secp256k1 case through the emulated _msgs_keyed form (front end lane, stage A with this curve's range checks, stage B),
    each family in one call: the verdicts are `want`, the same in both packings of the ladder."""
    keys = fc.keys("k256")
    verdicts = {}
    for what, cases in _calls("k256"):
        msgs, sigs, slots, _, want = fc.batch("k256", cases)
        n = len(cases)
        bm = ctypes.create_string_buffer((n + 7) // 8)
        rc = k256_emul.sbvk256_verify_msgs_keyed(b"".join(msgs) + b"\0", _offsets(msgs), b"".join(sigs) + b"\0", _offsets(sigs),
                                                 (ctypes.c_uint32 * n)(*slots), n, b"".join(keys), len(keys), bm)
        assert rc == 0
        got = _bits(bm.raw, n)
        assert got == want, (what, _wrong(cases, got, want))
        verdicts[what] = got
    perm = fc.ladder("k256")[2]
    assert verdicts["a shuffled"] == [verdicts["a"][p] for p in perm]


def test_ed25519_front_end_lane_and_msgs_keyed_form(emul, ed_emul):
    """Every Ed25519 case through ed_msg_frontend_lane (the unkeyed entry's lane): the tuple is R | S | A | SHA-512(R | A | M) mod L by
    hashlib; and through the emulated _msgs_keyed form with the cases' slots: a slot outside the registry is rejected although slot
    0's key, whose encoding the lane hashes for it, accepts the signature."""
    keys = fc.keys("ed25519")
    emul.sbve_ed_msg_frontend.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    t = ctypes.create_string_buffer(128)
    verdicts = {}
    for what, cases in _calls("ed25519"):
        msgs, sigs, slots, pks, want = fc.batch("ed25519", cases)
        if what != "a shuffled":
            for c in cases:
                emul.sbve_ed_msg_frontend(c.sig, c.key, c.msg, len(c.msg), t)
                k = int.from_bytes(hashlib.sha512(c.sig[:32] + c.key + c.msg).digest(), "little") % ed.L
                assert t.raw == c.sig + c.key + k.to_bytes(32, "little"), c.name
        n = len(cases)
        bm = ctypes.create_string_buffer((n + 7) // 8)
        ed_emul.sbvk_verify_msgs_keyed(b"".join(sigs), b"".join(msgs) + b"\0", _offsets(msgs), (ctypes.c_uint32 * n)(*slots), n,
                                       b"".join(keys), len(keys), bm)
        got = _bits(bm.raw, n)
        assert got == want, (what, _wrong(cases, got, want))
        verdicts[what] = got
    perm = fc.ladder("ed25519")[2]
    assert verdicts["a shuffled"] == [verdicts["a"][p] for p in perm]
