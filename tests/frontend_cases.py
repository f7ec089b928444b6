"""Cases of the message front ends — the entries that take raw bytes and hash and parse them before any curve arithmetic
(include/sbv.h: sbv_p256_verify_msgs_keyed, sbv_p256_verify_msgs_keyed_sharded, sbv_secp256k1_verify_msgs_keyed,
sbv_ed25519_verify_msgs, sbv_ed25519_verify_msgs_keyed) — shared by the CPU tier (tests/test_frontend_cases_cpu.py: the lanes as host
code) and the GPU tier (tests/test_gpu_frontends.py: the kernels), so that both run the same cases.  No GPU code is imported here.

A case is (name, key, message, signature bytes, slot rule, want).  The slot rule says which slot the case is sent with once
keys(scheme) is registered in order into an empty registry: OWN = the slot of `key`, NKEYS = the first slot behind the registry,
MAX = 0xFFFFFFFF.  `want` comes from code that shares nothing with the lanes: hashlib for the hashes, p256_py.parse_der_sig for the
strict parse, the C oracles (sbvo_p256_verify_asn1, sbvo_k256_verify_raw, sbvo_ed25519_verify) for the verdicts; a slot outside the
registry is a reject by the rule of include/sbv.h.  Honest signatures come from the C oracles' signers.

Families (the ECDSA curves have all five, Ed25519 has (a) and (e)):
  (a) ladder     every message length 0..260 and 1023, 1024, 1025, 4097, 65 537, honestly signed, and for every length above 0 three
                 twins with the first, the middle and the LAST byte flipped; two packings of the same cases, ascending and shuffled
  (b) short      ACCEPTED signatures whose r or s is 1, 2, 31 or 32 bytes long, with and without a sign byte: random signing cannot
                 make them, so the key is derived from the signature, Q = r^-1 (s R - e G) with R = lift_x(r) (public-key recovery)
  (c) between    r or s in [N of P-256, N of secp256k1): accepted on secp256k1, rejected on P-256; r = N, N + 1, 2^256 - 1 of
                 secp256k1 rejected; r = the x-coordinate at or next below N - 1 of P-256 accepted; one curve's key bytes in the
                 other curve's registry
  (d) DER        generated bends of two accepted signatures (every INTEGER with and without a sign byte), each applied to r and to s
  (e) slots      slots outside the registry under a signature that slot 0's key accepts, a slot whose key is no point, and an empty
                 message"""
import collections
import ctypes
import functools
import hashlib
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ed25519_py as ed  # noqa: E402
import k256_py as kc  # noqa: E402
import p256_py as pc  # noqa: E402

SCHEMES = ("p256", "k256", "ed25519")
OWN, NKEYS, MAX = "own", "nkeys", "max"
Case = collections.namedtuple("Case", "name key msg sig rule want")

LADDER_LENGTHS = list(range(261)) + [1023, 1024, 1025, 4097, 65537]
LONGEST = 65537
INT_SHAPES = (1, 2, 31, 32, 33)                    # significant bytes of an INTEGER; 33 = 32 bytes and a sign byte
N_P256, N_K256 = pc.N, kc.N
assert N_P256 < N_K256

Curve = collections.namedtuple("Curve", "name mod P N a b")
CURVES = {"p256": Curve("p256", pc, pc.P, pc.N, pc.A, pc.B), "k256": Curve("k256", kc, kc.P, kc.N, 0, kc.B)}


def sha256(m):
    return hashlib.sha256(m).digest()


def be32(v):
    return v.to_bytes(32, "big")


# ---- the judges ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle():
    so = os.path.join(ROOT, "oracle", "libsbv_oracle.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    lib = ctypes.CDLL(so)
    C, S = ctypes.c_char_p, ctypes.c_size_t
    lib.sbvo_p256_verify_asn1.argtypes = [C, C, C, S, C, S]
    lib.sbvo_k256_verify_raw.argtypes = [C, C, C, C, C]
    lib.sbvo_ed25519_verify.argtypes = [C, C, S, C, S]
    for name in ("sbvo_p256_sign", "sbvo_k256_sign"):
        getattr(lib, name).argtypes = [C, C, C, C]
    for name in ("sbvo_p256_pubkey", "sbvo_k256_pubkey", "sbvo_ed25519_public_key"):
        getattr(lib, name).argtypes = [C, C]
        getattr(lib, name).restype = None
    lib.sbvo_ed25519_sign.argtypes = [C, C, S, C]
    lib.sbvo_ed25519_sign.restype = None
    return lib


@functools.lru_cache(maxsize=None)
def openssl():
    """the OpenSSL third opinion, or None where libcrypto was not there to build it"""
    so = os.path.join(ROOT, "oracle", "libsbv_openssl.so")
    if not os.path.exists(so):
        return None
    lib = ctypes.CDLL(so)
    C, S = ctypes.c_char_p, ctypes.c_size_t
    lib.sbvssl_p256_verify_asn1.argtypes = [C, C, C, S, C, S]
    lib.sbvssl_p256_der_is_strict.argtypes = [C, S]
    lib.sbvssl_k256_verify_tuple.argtypes = [C]
    lib.sbvssl_ed25519_verify.argtypes = [C, C, S, C]
    return lib


def strict_rs(sig):
    """r | s as 64 bytes from the strict parse, or None: refused, or an integer of more than 32 significant bytes"""
    got = pc.parse_der_sig(sig)
    if got is None or len(got[0]) > 32 or len(got[1]) > 32:
        return None
    return got[0].rjust(32, b"\0") + got[1].rjust(32, b"\0")


def judge(scheme, key, msg, sig):
    """the C oracle's verdict on (key, message, signature bytes) with the key's own slot"""
    o = oracle()
    if scheme == "p256":
        return bool(o.sbvo_p256_verify_asn1(key[:32], key[32:], sha256(msg), 32, sig, len(sig)))
    if scheme == "k256":
        rs = strict_rs(sig)
        return rs is not None and bool(o.sbvo_k256_verify_raw(rs[:32], rs[32:], sha256(msg), key[:32], key[32:]))
    return bool(o.sbvo_ed25519_verify(key, msg, len(msg), sig, len(sig)))


def judge_openssl(scheme, key, msg, sig):
    """OpenSSL's verdict under the same input rules, or None without libcrypto"""
    lib = openssl()
    if lib is None:
        return None
    if scheme == "p256":
        return bool(lib.sbvssl_p256_verify_asn1(key[:32], key[32:], sha256(msg), 32, sig, len(sig)))
    if scheme == "k256":
        rs = strict_rs(sig)                    # "on the parsed integers": OpenSSL judges the curve, not the parse
        return rs is not None and bool(lib.sbvssl_k256_verify_tuple(rs + sha256(msg) + key))
    return bool(lib.sbvssl_ed25519_verify(key, msg, len(msg), sig))


def judge_python(scheme, key, msg, sig):
    """the Python twin's verdict (slow: a scalar multiplication takes milliseconds)"""
    if scheme == "ed25519":
        return ed.verify(key, msg, sig)
    rs = strict_rs(sig)
    if rs is None:
        return False
    f = [int.from_bytes(b, "big") for b in (rs[:32], rs[32:], key[:32], key[32:])]
    return CURVES[scheme].mod.verify_raw(f[0], f[1], sha256(msg), f[2], f[3])


# ---- keys and honest signatures -----------------------------------------------------------------------------------------------------
def _scalar(label, n):
    return int.from_bytes(sha256(label.encode()), "big") % (n - 1) + 1


@functools.lru_cache(maxsize=None)
def signer(scheme, i):
    """(secret, public key bytes) of honest signer i: an ECDSA scalar and Qx | Qy, or an Ed25519 seed and the encoding"""
    o = oracle()
    if scheme == "ed25519":
        seed = sha256(b"front end ed25519 signer %d" % i)
        pk = ctypes.create_string_buffer(32)
        o.sbvo_ed25519_public_key(seed, pk)
        return seed, pk.raw
    d = be32(_scalar("front end %s signer %d" % (scheme, i), CURVES[scheme].N))
    q = ctypes.create_string_buffer(64)
    getattr(o, "sbvo_%s_pubkey" % scheme)(d, q)
    return d, q.raw


def sign_ints(scheme, i, msg, nonce=0):
    """(r, s) of signer i over SHA-256(msg) by the C oracle's signer, the nonce derived from the message and `nonce`"""
    d, _ = signer(scheme, i)
    k = be32(_scalar("nonce %d %s" % (nonce, sha256(msg).hex()), CURVES[scheme].N))
    rs = ctypes.create_string_buffer(64)
    assert getattr(oracle(), "sbvo_%s_sign" % scheme)(d, k, sha256(msg), rs) == 0
    return int.from_bytes(rs.raw[:32], "big"), int.from_bytes(rs.raw[32:], "big")


def sign(scheme, i, msg):
    """the signature bytes an honest signer sends: minimal DER for the ECDSA curves, R | S for Ed25519"""
    if scheme == "ed25519":
        sig = ctypes.create_string_buffer(64)
        oracle().sbvo_ed25519_sign(signer(scheme, i)[0], msg, len(msg), sig)
        return sig.raw
    return pc.der_encode_sig(*sign_ints(scheme, i, msg))


def honest(scheme, name, i, msg):
    key, sig = signer(scheme, i)[1], sign(scheme, i, msg)
    return Case(name, key, msg, sig, OWN, judge(scheme, key, msg, sig))


# ---- (a) the length ladder ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ladder(scheme):
    """(cases in ascending length, the same cases in a seeded shuffle, the shuffle: shuffled[j] = ascending[perm[j]])"""
    rng = random.Random(0xF207 + SCHEMES.index(scheme))
    up = []
    for n, length in enumerate(LADDER_LENGTHS):
        msg = rng.randbytes(length)
        c = honest(scheme, "a_len%d" % length, n % 3, msg)
        assert c.want, c.name
        up.append(c)
        if length:
            for tag, at in (("first", 0), ("middle", length // 2), ("last", length - 1)):
                bent = msg[:at] + bytes([msg[at] ^ 1]) + msg[at + 1:]
                twin = Case("a_len%d_%s_byte_flipped" % (length, tag), c.key, bent, c.sig, OWN, judge(scheme, c.key, bent, c.sig))
                assert not twin.want, twin.name
                up.append(twin)
    starts, at = set(), 0
    for c in up:
        starts.add(at % 16)
        at += len(c.msg)
    assert len(starts) == 16                         # packed back to back, the messages start at every address residue mod 16
    perm = list(range(len(up)))
    rng.shuffle(perm)
    return up, [up[p] for p in perm], perm


# ---- (b), (c): signatures chosen first, keys derived from them ----------------------------------------------------------------------
def lift_x(cv, x):
    """the point of abscissa x with the even ordinate, or None (both fields have p = 3 mod 4)"""
    if not 0 <= x < cv.P:
        return None
    rhs = (x * x * x + cv.a * x + cv.b) % cv.P
    y = pow(rhs, (cv.P + 1) // 4, cv.P)
    if y * y % cv.P != rhs:
        return None
    return (x, y if y % 2 == 0 else cv.P - y)


def next_x(cv, start, step=1):
    x = start
    while lift_x(cv, x) is None:
        x += step
    return x


def derived_key(cv, r, s, msg):
    """Q with r = x(e / s G + r / s Q): Q = r^-1 (s R - e G), R = lift_x(r)"""
    e = int.from_bytes(sha256(msg), "big") % cv.N
    ri = pow(r, -1, cv.N)
    q = cv.mod.pt_add(cv.mod.pt_mul(s * ri % cv.N, lift_x(cv, r)), cv.mod.pt_mul((cv.N - e) * ri % cv.N, cv.mod.G))
    assert q is not None
    return be32(q[0]) + be32(q[1])


def int_shape(v):
    """the class of INT_SHAPES an INTEGER of value v falls into, or None"""
    sig = max(1, (v.bit_length() + 7) // 8)
    if sig == 32 and v >> 255:
        return 33
    return sig if sig in INT_SHAPES else None


def _accepted(scheme, name, key, msg, sig):
    """a constructed case every judge at hand must accept"""
    c = Case(name, key, msg, sig, OWN, judge(scheme, key, msg, sig))
    assert c.want, name
    assert judge_openssl(scheme, key, msg, sig) in (True, None), name
    return c


@functools.lru_cache(maxsize=None)
def short_integers(scheme):
    """(b): 6 values of r x 7 values of s, each pair under its own derived key"""
    cv = CURVES[scheme]
    rs = [("1byte", next_x(cv, 1)), ("2bytes", next_x(cv, 0x100)), ("31bytes", next_x(cv, 1 << 240)), ("31bytes_top_bit", next_x(cv, 1 << 247)),
          ("32bytes", next_x(cv, 1 << 248)), ("32bytes_top_bit", next_x(cv, 1 << 255))]
    assert [int_shape(r) for _, r in rs] == [1, 2, 31, 31, 32, 33] and rs[0][1] < 0x80 and rs[1][1] < 0x8000
    ss = [("1", 1), ("7f", 0x7F), ("80", 0x80), ("ffff", 0xFFFF), ("31bytes", (1 << 247) + 0x1234), ("half", (cv.N - 1) // 2), ("n_minus_1", cv.N - 1)]
    assert [int_shape(s) for _, s in ss] == [1, 1, 1, 2, 31, 32, 33]
    out = []
    for rn, r in rs:
        for sn, s in ss:
            name = "b_r_%s_s_%s" % (rn, sn)
            msg = name.encode()
            out.append(_accepted(scheme, name, derived_key(cv, r, s, msg), msg, pc.der_encode_sig(r, s)))
    assert len({c.key for c in out}) == len(out)
    cover = shape_cover(out)
    assert all(cover[(which, shape)] for which in "rs" for shape in INT_SHAPES), cover
    return out


def shape_cover(cases):
    """{("r" | "s", shape): accepted cases whose INTEGER has that shape}, over the strict parse of the signature bytes"""
    cover = {(which, shape): 0 for which in "rs" for shape in INT_SHAPES}
    for c in cases:
        got = pc.parse_der_sig(c.sig)
        if not c.want or got is None:
            continue
        for which, b in zip("rs", got):
            shape = int_shape(int.from_bytes(b, "big"))
            if shape is not None:
                cover[(which, shape)] += 1
    return cover


@functools.lru_cache(maxsize=None)
def _between():
    """(c) for both curves at once: the secp256k1 signatures are also sent to P-256, and each curve's key bytes to the other curve"""
    k, p = CURVES["k256"], CURVES["p256"]
    rng = random.Random(0xBE7)
    out = {"k256": [], "p256": []}
    # secp256k1: r between the orders, with s and with n - s under the same key
    r = next_x(k, N_P256 + 5)
    assert N_P256 <= r < N_K256
    s = rng.randrange(1, N_P256)
    msg = b"c_r_between_the_orders"
    kkey = derived_key(k, r, s, msg)
    r_between = pc.der_encode_sig(r, s)
    out["k256"] += [_accepted("k256", "c_r_between_the_orders", kkey, msg, r_between),
                    _accepted("k256", "c_r_between_the_orders_n_minus_s", kkey, msg, pc.der_encode_sig(r, N_K256 - s))]
    # ... s between the orders
    r2, s2 = next_x(k, rng.randrange(1, N_P256)), N_P256 + 7
    msg2 = b"c_s_between_the_orders"
    s_between = pc.der_encode_sig(r2, s2)
    out["k256"].append(_accepted("k256", "c_s_between_the_orders", derived_key(k, r2, s2, msg2), msg2, s_between))
    # ... r at and above the order
    for name, big in (("n", N_K256), ("n_plus_1", N_K256 + 1), ("2_256_minus_1", (1 << 256) - 1)):
        sig = pc.der_encode_sig(big, s)
        out["k256"].append(Case("c_r_eq_" + name, kkey, msg, sig, OWN, judge("k256", kkey, msg, sig)))
    # P-256: the same bytes against a registered key of that curve
    pkey = signer("p256", 0)[1]
    for name, m, sig in (("c_k256_r_between_the_orders", msg, r_between), ("c_k256_s_between_the_orders", msg2, s_between)):
        out["p256"].append(Case(name, pkey, m, sig, OWN, judge("p256", pkey, m, sig)))
    # ... r just below the order
    r3 = next_x(p, N_P256 - 1, -1)
    s3 = rng.randrange(1, N_P256)
    msg3 = b"c_r_below_the_order"
    top = _accepted("p256", "c_r_below_the_order", derived_key(p, r3, s3, msg3), msg3, pc.der_encode_sig(r3, s3))
    out["p256"].append(top)
    # the same 64 key bytes in both registries: a point of one curve, no point of the other
    out["p256"].append(Case("c_k256_key_bytes", kkey, msg, r_between, OWN, judge("p256", kkey, msg, r_between)))
    out["k256"].append(Case("c_p256_key_bytes", top.key, msg3, top.sig, OWN, judge("k256", top.key, msg3, top.sig)))
    for scheme, accepted in (("k256", 3), ("p256", 1)):
        assert sum(c.want for c in out[scheme]) == accepted, [(c.name, c.want) for c in out[scheme]]
    return out


def between(scheme):
    return _between()[scheme]


# ---- (d) the DER ladder -------------------------------------------------------------------------------------------------------------
def _der_len(n):
    return bytes([n]) if n < 128 else b"\x81" + bytes([n])


def _tlv(tag, body):
    return bytes([tag]) + _der_len(len(body)) + body


def _min_int(v):
    b = v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big")
    return b"\0" + b if b[0] & 0x80 else b


def der_bends(r, s):
    """[(name, bytes)]: the bends of the issue applied to the signature (r, s), the INTEGER bends once to r and once to s"""
    good = pc.der_encode_sig(r, s)
    out = [("minimal", good)]
    for which in "rs":
        v = r if which == "r" else s
        m, mag = _min_int(v), v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big")
        other = _tlv(2, _min_int(s if which == "r" else r))

        def seq(x_tlv, seq_len=None):
            body = x_tlv + other if which == "r" else other + x_tlv
            return b"\x30" + _der_len(len(body) if seq_len is None else seq_len(len(body))) + body
        n = bytes([len(m)])
        for name, x in (("extra_leading_00", _tlv(2, b"\0" + m)), ("sign_byte_dropped", _tlv(2, mag)), ("ff_padded", _tlv(2, b"\xff" + mag)),
                        ("empty_integer", _tlv(2, b"")), ("33_byte_value", _tlv(2, b"\x01" + mag.rjust(32, b"\0"))),
                        ("34_bytes_zero_padded", _tlv(2, b"\0\0" + mag.rjust(32, b"\0"))), ("zero", _tlv(2, b"\0")),
                        ("length_81", b"\x02\x81" + n + m), ("length_82_00", b"\x02\x82\x00" + n + m), ("length_84_00_00_00", b"\x02\x84\0\0\0" + n + m),
                        ("length_85", b"\x02\x85\0\0\0\0" + n + m), ("length_indefinite", b"\x02\x80" + m), ("length_indefinite_closed", b"\x02\x80" + m + b"\0\0"),
                        ("tag_bit_string", b"\x03" + n + m), ("tag_context", b"\x82" + n + m), ("tag_constructed", b"\x22" + n + m),
                        ("length_plus_1", b"\x02" + bytes([len(m) + 1]) + m), ("length_minus_1", b"\x02" + bytes([len(m) - 1]) + m)):
            out.append(("%s_%s" % (which, name), seq(x)))
        # the INTEGER one byte longer with the SEQUENCE counting the byte it lacks: for s it runs past the SEQUENCE and the input
        out.append(("%s_runs_past_the_sequence" % which, seq(b"\x02" + bytes([len(m) + 1]) + m, lambda k: k + 1)))
    body = good[2:]
    n = bytes([len(body)])
    out += [("seq_length_81", b"\x30\x81" + n + body), ("seq_length_82_00", b"\x30\x82\x00" + n + body), ("seq_length_84_00_00_00", b"\x30\x84\0\0\0" + n + body),
            ("seq_length_indefinite", b"\x30\x80" + body), ("seq_length_indefinite_closed", b"\x30\x80" + body + b"\0\0"),
            ("seq_length_minus_1", b"\x30" + bytes([len(body) - 1]) + body), ("seq_length_plus_1", b"\x30" + bytes([len(body) + 1]) + body),
            ("trailing_byte_inside", b"\x30" + bytes([len(body) + 1]) + body + b"\0"), ("trailing_byte_after", good + b"\0"),
            ("seq_tag_set", b"\x31" + good[1:]), ("seq_tag_primitive", b"\x10" + good[1:]), ("seq_tag_integer", b"\x02" + good[1:]),
            ("three_integers", _tlv(0x30, body + _tlv(2, _min_int(s)))), ("one_integer", _tlv(0x30, _tlv(2, _min_int(r)))),
            ("nested_sequence", _tlv(0x30, good)), ("sequence_of_sequence_and_s", _tlv(0x30, _tlv(0x30, _tlv(2, _min_int(r))) + _tlv(2, _min_int(s)))),
            ("single_byte_30", b"\x30"), ("single_byte_02", b"\x02"), ("single_byte_00", b"\0"), ("empty", b""), ("empty_sequence", b"\x30\0")]
    s_tag = 4 + good[3]
    for at in (0, 1, 2, 3, s_tag, s_tag + 1):                # one byte of the header missing, at every position of it
        out.append(("header_byte_%d_missing" % at, good[:at] + good[at + 1:]))
    for k in list(range(1, 7)) + [s_tag, s_tag + 1, s_tag + 2, len(good) - 1]:
        out.append(("cut_to_%d_bytes" % k, good[:k]))
    return out


@functools.lru_cache(maxsize=None)
def der_ladder(scheme):
    """(d): the bends of two honest signatures of signer 1, one whose r and s both need a sign byte and one where neither does"""
    out = []
    for tag, top in (("sign_bytes", 1), ("no_sign_bytes", 0)):
        msg = b"der ladder " + tag.encode()
        nonce = 0
        while True:
            r, s = sign_ints(scheme, 1, msg, nonce)
            if r >> 255 == top and s >> 255 == top and r.bit_length() > 248 and s.bit_length() > 248:
                break
            nonce += 1
        key = signer(scheme, 1)[1]
        for name, sig in der_bends(r, s):
            out.append(Case("d_%s_%s" % (tag, name), key, msg, sig, OWN, judge(scheme, key, msg, sig)))
            if out[-1].want:                         # what is accepted is the one encoding of its integers
                assert sig == pc.der_encode_sig(r, s), out[-1].name
    assert sum(c.want for c in out) >= 2 and sum(not c.want for c in out) >= 140
    return out


# ---- (e) slot rules -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def slot_rules(scheme):
    key0 = signer(scheme, 0)[1]
    msg = b"valid under the key of slot 0"
    sig = sign(scheme, 0, msg)
    assert judge(scheme, key0, msg, sig)
    out = [Case("e_slot_0", key0, msg, sig, OWN, True), Case("e_slot_eq_nkeys", key0, msg, sig, NKEYS, False),
           Case("e_slot_ffffffff", key0, msg, sig, MAX, False)]
    if scheme == "ed25519":
        bad = next(bytes([b]) + bytes(31) for b in range(2, 256) if ed.decompress(bytes([b]) + bytes(31)) is None)
    else:
        bad = key0[:63] + bytes([key0[63] ^ 1])
        assert not CURVES[scheme].mod.on_curve(int.from_bytes(bad[:32], "big"), int.from_bytes(bad[32:], "big"))
    out.append(Case("e_key_is_no_point", bad, msg, sig, OWN, judge(scheme, bad, msg, sig)))
    assert not out[-1].want
    out.append(honest(scheme, "e_empty_message", 2, b""))
    assert out[-1].want
    return out


@functools.lru_cache(maxsize=None)
def empty_batch(scheme):
    """cases whose messages are all empty (the message pointer of such a call may be null): honest ones and one bent signature"""
    out = [honest(scheme, "e_all_empty_%d" % i, i % 3, b"") for i in range(5)]
    c = out[1]
    bent = c.sig[:-1] + bytes([c.sig[-1] ^ 1])
    out.insert(2, Case("e_all_empty_bent", c.key, b"", bent, OWN, judge(scheme, c.key, b"", bent)))
    assert [c.want for c in out] == [True, True, False, True, True, True]
    return out


# ---- the whole set ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def families(scheme):
    """{family: cases}; the ladder in its ascending packing"""
    out = {"a": ladder(scheme)[0]}
    if scheme != "ed25519":
        out.update(b=short_integers(scheme), c=between(scheme), d=der_ladder(scheme))
    out["e"] = slot_rules(scheme)
    return out


@functools.lru_cache(maxsize=None)
def keys(scheme):
    """the registry of the scheme's tests: every key of every case, in order of first appearance; slot 0 is honest signer 0's"""
    seen = {}
    for cases in list(families(scheme).values()) + [empty_batch(scheme), filler(scheme)]:
        for c in cases:
            seen.setdefault(c.key, len(seen))
    out = list(seen)
    assert out[0] == signer(scheme, 0)[1]
    return out


def slot_of(scheme, case):
    if case.rule == OWN:
        return keys(scheme).index(case.key)
    return len(keys(scheme)) if case.rule == NKEYS else 0xFFFFFFFF


def batch(scheme, cases):
    """(messages, signatures, slots, keys, want) of a call that sends `cases` in order"""
    index = {k: i for i, k in enumerate(keys(scheme))}
    slots = [index[c.key] if c.rule == OWN else len(index) if c.rule == NKEYS else 0xFFFFFFFF for c in cases]
    return [c.msg for c in cases], [c.sig for c in cases], slots, [c.key for c in cases], [c.want for c in cases]


@functools.lru_cache(maxsize=None)
def filler(scheme):
    """97 honest cases with short messages, to fill a batch around the cases under test"""
    return [honest(scheme, "filler_%d" % i, i % 3, b"filler %d" % i * (i % 5)) for i in range(97)]


def interleaved(scheme, cases, n, shift=0):
    """n cases: those of `cases` from index `shift` on (cyclically) alternating with honest filler"""
    fill = filler(scheme)
    out = []
    for j in range(n):
        out.append(cases[(shift + j // 2) % len(cases)] if j % 2 == 0 else fill[(j // 2) % len(fill)])
    return out


def sample(scheme, count=32):
    """a seeded sample over all families, for calls that send one case alone"""
    rng = random.Random(0x5A3 + SCHEMES.index(scheme))
    fams = families(scheme)
    pool = [c for f, cs in sorted(fams.items()) for c in cs if f != "a" or len(c.msg) < 4097]
    picked = rng.sample(pool, count - len(fams))
    picked += [rng.choice(cs) for _, cs in sorted(fams.items())]          # no family left out
    return picked
