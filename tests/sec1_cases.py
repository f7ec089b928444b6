"""Cases of the SEC1 key decoders (include/sbv.h: sbv_p256_decode_keys, sbv_secp256k1_decode_keys, the _sec1 verify entries,
sbv_debug_sec1_op), shared by the CPU tier (tests/test_sec1_cpu.py: the lanes as host code) and the GPU tier (tests/test_gpu_sec1.py: the
kernels).  No GPU code is imported here.

The model is Python integers and nothing else: pow(c, (p + 1) // 4, p) for the root and the rules of SEC1 2.3.4 as Go applies them
(elliptic.Unmarshal, elliptic.UnmarshalCompressed).  Every expected output comes from decode() / sqrt() / lift() below.

  known answers   tests/golden/sec1_keys.json: the base points of both curves, the RFC 6979 A.2.5 key, the secp256k1 keys of d = 1, 2, 3,
                  each compressed and uncompressed
  generated       per curve: 300 seeded points compressed under both prefixes (the wrong one gives the negated y) and uncompressed; the
                  non-residue abscissae met while drawing them, under both prefixes; the edges of x around 0 and p; uncompressed keys
                  with Y negated, Y + 1, Y + p, X >= p; every prefix byte at lengths 33 and 65; every length 0..70 under 02 and 04; (0, 0)
  packings        stride(curve): the 33-byte cases as one m x 33 array; mixed(curve): every case in a seeded order in which each kind
                  (33 bytes, 65 bytes, any other length) is spread evenly, so that every wavefront holds lanes of all three
  bad offsets     broken_offsets(curve): the mixed table with single entries spoiled (a decreasing pair, an entry behind the upload);
                  lane_slice() is the kernel's rule
  unit ops        op_cases(curve, op): the 192-byte records of sbv_debug_sec1_op and their 128-byte answers
  verify cases    verify_cases(scheme): every ECDSA case of tests/msgs_generic_cases.py with its key as compressed, uncompressed or, for a
                  share, a refused encoding; want = the oracle's verdict under the 64 bytes decode() gives"""
import collections
import functools
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))

Curve = collections.namedtuple("Curve", "id name p a b gx gy")
P256 = Curve(0, "p256", 2**256 - 2**224 + 2**192 + 2**96 - 1, -3, 0x5AC635D8AA3A93E7B3EBBD55769886BC651D06B0CC53B0F63BCE3C3E27D2604B,
             0x6B17D1F2E12C4247F8BCE6E563A440F277037D812DEB33A0F4A13945D898C296, 0x4FE342E2FE1A7F9B8EE7EB4A7C0F9E162BCE33576B315ECECBB6406837BF51F5)
K256 = Curve(1, "k256", 2**256 - 2**32 - 977, 0, 7,
             0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798, 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)
CURVES = (P256, K256)
BY_NAME = {c.name: c for c in CURVES}
X_WITH_Y_1 = {"p256": 0x8d0177ebab9c6e9e10db6dd095dbac0d6375e8a97b70f611875d877f0069d2c7,
              "k256": 0xcbb0deab125754f1fdb2038b0434ed9cb3fb53ab735391129994a535d925f673}
OP_IN, OP_OUT = 192, 128
ZERO64 = bytes(64)


def be32(v):
    return v.to_bytes(32, "big")


# ---- the model --------------------------------------------------------------------------------------------------------------------
def rhs(cv, x):
    return (x * x * x + cv.a * x + cv.b) % cv.p


def sqrt(cv, a):
    """(a^((p+1)/4) mod p, a is a square) — p = 3 mod 4 on both curves"""
    a %= cv.p
    y = pow(a, (cv.p + 1) // 4, cv.p)
    return y, y * y % cv.p == a


def lift(cv, x, parity):
    """y of the point with abscissa x and that parity of y, or None"""
    if x >= cv.p:
        return None
    y, ok = sqrt(cv, rhs(cv, x))
    if not ok:
        return None
    return y if y & 1 == parity else cv.p - y


def on_curve(cv, x, y):
    return x < cv.p and y < cv.p and (y * y - rhs(cv, x)) % cv.p == 0


def decode(cv, key):
    """(64 bytes X | Y, ok) of a SEC1 octet string; 64 zero bytes and 0 when refused"""
    if len(key) == 65 and key[0] == 4:
        x, y = int.from_bytes(key[1:33], "big"), int.from_bytes(key[33:], "big")
        if on_curve(cv, x, y):
            return key[1:], 1
    elif len(key) == 33 and key[0] in (2, 3):
        x = int.from_bytes(key[1:], "big")
        y = lift(cv, x, key[0] & 1)
        if y is not None:
            return key[1:] + be32(y), 1
    return ZERO64, 0


def compress(key64):
    return bytes([2 + (key64[63] & 1)]) + key64[:32]


def uncompressed(key64):
    return b"\x04" + key64


# ---- known answers ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden():
    with open(os.path.join(HERE, "golden", "sec1_keys.json")) as f:
        return json.load(f)["keys"]


def golden_cases(cv):
    """(name, key bytes, X | Y bytes) of the file's keys of this curve, each in its two accepted encodings"""
    out = []
    for k in golden():
        if k["curve"] != cv.name:
            continue
        xy = bytes.fromhex(k["x"] + k["y"])
        out.append((k["name"] + "_compressed", bytes.fromhex(k["compressed"]), xy))
        out.append((k["name"] + "_uncompressed", bytes.fromhex(k["uncompressed"]), xy))
    return out


# ---- generated cases --------------------------------------------------------------------------------------------------------------
N_POINTS = 300


@functools.lru_cache(maxsize=None)
def drawn(cv):
    """(points, non-residue abscissae): seeded x until N_POINTS of them carry a point; the model decides which"""
    rng = random.Random(0x5EC1 + cv.id)
    pts, non = [], []
    while len(pts) < N_POINTS:
        x = rng.randrange(cv.p)
        y = lift(cv, x, rng.randrange(2))
        if y is None:
            non.append(x)
        else:
            pts.append((x, y))
    return pts, non


@functools.lru_cache(maxsize=None)
def cases(cv):
    """[(name, key bytes)] — every decode case of the curve, known answers first"""
    p = cv.p
    out = [(n, k) for n, k, _ in golden_cases(cv)]
    pts, non = drawn(cv)
    for i, (x, y) in enumerate(pts):
        out.append(("pt%d_02" % i, b"\x02" + be32(x)))
        out.append(("pt%d_03" % i, b"\x03" + be32(x)))
        out.append(("pt%d_04" % i, b"\x04" + be32(x) + be32(y)))
    for i, x in enumerate(non):
        out.append(("non%d_02" % i, b"\x02" + be32(x)))
        out.append(("non%d_03" % i, b"\x03" + be32(x)))
    for x in (0, 1, 2, 3, p - 2, p - 1, p, p + 1, 2**256 - 1):
        for pre in (2, 3):
            out.append(("x_edge_%x_%02x" % (x, pre), bytes([pre]) + be32(x)))
        y = lift(cv, x % p, 0)
        out.append(("x_edge_%x_04" % x, b"\x04" + be32(x) + be32(y if y is not None else 1)))
    # uncompressed keys bent in Y and in X
    for i, (x, y) in enumerate(pts[:40]):
        out.append(("pt%d_y_negated" % i, b"\x04" + be32(x) + be32(p - y)))
        out.append(("pt%d_y_plus_1" % i, b"\x04" + be32(x) + be32((y + 1) % p)))
        if y + p < 2**256:
            out.append(("pt%d_y_plus_p" % i, b"\x04" + be32(x) + be32(y + p)))
        if x + p < 2**256:
            out.append(("pt%d_x_plus_p" % i, b"\x04" + be32(x + p) + be32(y)))
            out.append(("pt%d_x_plus_p_02" % i, b"\x02" + be32(x + p)))
    # small ordinates and abscissae leave room for + p on either curve
    rng = random.Random(0x5EC2 + cv.id)
    small = []
    while len(small) < 12:
        x = rng.randrange(2**256 - p)
        y = lift(cv, x, 0)
        if y is not None:
            small.append((x, y))
    for i, (x, y) in enumerate(small):
        out.append(("small%d_04" % i, b"\x04" + be32(x) + be32(y)))
        out.append(("small%d_x_plus_p_04" % i, b"\x04" + be32(x + p) + be32(y)))
        out.append(("small%d_x_plus_p_02" % i, bytes([2 + (y & 1)]) + be32(x + p)))
    # Y + p fits in 256 bits only for a tiny Y: the points with y = 1 (the abscissae tests/msgs_generic_cases.py uses for the same purpose)
    x1 = X_WITH_Y_1[cv.name]
    assert on_curve(cv, x1, 1) and p + 1 < 2**256
    out.append(("y_eq_1", b"\x04" + be32(x1) + be32(1)))
    out.append(("y_eq_1_plus_p", b"\x04" + be32(x1) + be32(p + 1)))
    out.append(("y_eq_1_compressed", b"\x03" + be32(x1)))
    out.append(("x_eq_p_y_valid", b"\x04" + be32(p) + be32(pts[0][1])))
    out.append(("y_eq_p", b"\x04" + be32(pts[0][0]) + be32(p)))
    out.append(("y_all_ones", b"\x04" + be32(pts[0][0]) + be32(2**256 - 1)))
    # every prefix byte at both lengths, over a valid point
    x, y = pts[1]
    for pre in range(256):
        out.append(("prefix_%02x_len33" % pre, bytes([pre]) + be32(x)))
        out.append(("prefix_%02x_len65" % pre, bytes([pre]) + be32(x) + be32(y)))
    # every length 0..70 under 02 and 04: the valid key cut short or followed by more
    x, y = pts[2]
    body = be32(x) + be32(y) + bytes(range(1, 7))
    for n in range(71):
        out.append(("len%d_02" % n, (b"\x02" + body)[:n]))
        out.append(("len%d_04" % n, (b"\x04" + body)[:n]))
    out.append(("zero_zero", b"\x04" + ZERO64))
    out.append(("infinity", b"\x00"))
    return out


@functools.lru_cache(maxsize=None)
def expected(cv):
    """[(64 bytes, ok)] of cases(cv)"""
    return [decode(cv, k) for _, k in cases(cv)]


def kind(key):
    return 0 if len(key) == 33 else 1 if len(key) == 65 else 2


# ---- packings ---------------------------------------------------------------------------------------------------------------------
def offsets_of(keys):
    off = [0]
    for k in keys:
        off.append(off[-1] + len(k))
    return off


@functools.lru_cache(maxsize=None)
def stride(cv):
    """(indices into cases(cv), m x 33 bytes): the 33-byte cases in a seeded order"""
    cs = cases(cv)
    idx = [i for i, (_, k) in enumerate(cs) if len(k) == 33]
    random.Random(0x5EC3 + cv.id).shuffle(idx)
    return idx, b"".join(cs[i][1] for i in idx)


@functools.lru_cache(maxsize=None)
def mixed(cv):
    """(indices, packed bytes, offsets): every case; each kind shuffled, then spread evenly over the whole order"""
    cs = cases(cv)
    rng = random.Random(0x5EC4 + cv.id)
    keyed = []
    for kd in (0, 1, 2):
        idx = [i for i, (_, k) in enumerate(cs) if kind(k) == kd]
        rng.shuffle(idx)
        keyed += [((j + 0.5) / len(idx), kd, i) for j, i in enumerate(idx)]
    idx = [i for _, _, i in sorted(keyed)]
    keys = [cs[i][1] for i in idx]
    return idx, b"".join(keys), offsets_of(keys)


def lane_slice(off, i, key_bytes, stride33=False):
    """(k0, k1) lane i of k_sec1_decode_keys decodes: its pair when monotone and inside the upload, else the empty key"""
    k0, k1 = (33 * i, 33 * i + 33) if stride33 else (off[i], off[i + 1])
    return (k0, k1) if k0 <= k1 <= key_bytes else (0, 0)


def decode_packed(cv, blob, off, m, key_bytes=None, stride33=False):
    """the model of one kernel launch: (m x 64 bytes, m ok bytes)"""
    key_bytes = len(blob) if key_bytes is None else key_bytes
    res = [decode(cv, blob[slice(*lane_slice(off, i, key_bytes, stride33))]) for i in range(m)]
    return b"".join(r[0] for r in res), bytes(r[1] for r in res)


@functools.lru_cache(maxsize=None)
def broken_offsets(cv):
    """(packed bytes, offsets, spoiled lanes): 520 keys of the mixed packing — all valid encodings, so that every refusal is the offsets' —
    with single table entries spoiled: lane 3 and 4 (entry 4 pulled below entry 3), lane 64 (entry 65 behind the upload, which also empties
    lane 65), lane 130 (entry 131 = 2^63), the last lane (its end one byte behind the upload)"""
    cs, ex = cases(cv), expected(cv)
    idx = [i for i in mixed(cv)[0] if ex[i][1]][:520]
    keys = [cs[i][1] for i in idx]
    off = offsets_of(keys)
    blob = b"".join(keys)
    off[4] = off[3] - 1
    off[65] = len(blob) + 7
    off[131] = 1 << 63
    off[520] = len(blob) + 1
    return blob, off, (3, 4, 64, 65, 130, 131, 519)


# ---- unit operations --------------------------------------------------------------------------------------------------------------
def op_record(a, parity=0):
    return be32(a) + bytes(31) + bytes([parity]) + bytes(OP_IN - 64)


def op_answer(words, ok):
    return (words + bytes(OP_OUT - 1 - len(words)) + b"\x01") if ok else bytes(OP_OUT)


@functools.lru_cache(maxsize=None)
def op_cases(cv, op):
    """(records, answers).  op 0: squares and non-squares at 0, 1, 4, p - 1, around p, random values, and a^2 (whose root is a or p - a);
    op 1: abscissae of points and of none under both parities, the edges, parity bytes above 1"""
    p = cv.p
    rng = random.Random(0x5EC5 + 2 * cv.id + op)
    ins, outs = [], []
    if op == 0:
        vals = [0, 1, 4, p - 1, p - 4, 2, 3, p, p + 1, p + 4, 2**256 - 1, rhs(cv, cv.gx)]
        vals += [rng.randrange(2**256) for _ in range(200)]
        roots = [rng.randrange(1, p) for _ in range(100)]
        vals += [r * r % p for r in roots]
        for a in vals:
            y, ok = sqrt(cv, a)
            ins.append(op_record(a))
            outs.append(op_answer(be32(y), ok))
        for r, a in zip(roots, vals[-100:]):
            y, ok = sqrt(cv, a)
            assert ok and y in (r, p - r)
    else:
        pts, non = drawn(cv)
        xs = [x for x, _ in pts[:120]] + non[:120] + [0, 1, 2, 3, p - 2, p - 1, p, p + 1, 2**256 - 1, cv.gx]
        for x in xs:
            for parity in (0, 1):
                y = lift(cv, x, parity)
                ins.append(op_record(x, parity))
                outs.append(op_answer(be32(x) + be32(y), True) if y is not None else bytes(OP_OUT))
        for parity in (2, 3, 255):
            ins.append(op_record(cv.gx, parity))
            outs.append(bytes(OP_OUT))
    return ins, outs


# ---- verify cases -----------------------------------------------------------------------------------------------------------------
VCase = collections.namedtuple("VCase", "name key msg sig want key64")


def reencode(i, key64):
    """the SEC1 form case i travels in: compressed, uncompressed, or (every seventh) one of the refused encodings of a good key"""
    if i % 7 == 6:
        r = (i // 7) % 5
        return [bytes([6 + (key64[63] & 1)]) + key64, b"\x05" + key64[:32], compress(key64)[:32], uncompressed(key64) + b"\x00", b"\x00"][r]
    return compress(key64) if i % 2 == 0 else uncompressed(key64)


def verify_cases(scheme, generic_cases):
    """generic_cases (tests/msgs_generic_cases.py: name key msg sig want) -> VCases.  want is the oracle's verdict on the 64 bytes the
    model decodes, which is the definition of the _sec1 entries; where those are the case's own key the generic want is reused."""
    import frontend_cases as fc
    cv = BY_NAME[scheme]
    out = []
    for i, c in enumerate(generic_cases):
        key = reencode(i, c.key)
        key64, ok = decode(cv, key)
        want = bool(ok) and (c.want if key64 == c.key else fc.judge(scheme, key64, c.msg, c.sig))
        out.append(VCase(c.name, key, c.msg, c.sig, want, key64))
    return out
