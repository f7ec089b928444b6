"""Cases and expected values of the BIP-340 Schnorr tests, shared by the CPU tier (tests/test_k256_schnorr_cpu.py: the emulated lanes
and the host forms) and the GPU tier (tests/test_gpu_k256_schnorr.py: the kernels), so that both run the same cases.  Expected values
come from the model below: Python integers, hashlib and oracle/k256_py.py for the curve (its constants, its point addition and, on
samples, its multiplication: `mul` here is a windowed Jacobian ladder only because the affine one costs 12 ms a call, and the CPU tier
holds it to kp.pt_mul).  The model has no tie to the C sources and reproduces the two known answers of tests/golden/bip340.json."""
import functools
import hashlib
import json
import os
import random

import k256_py as kp
import k256_sign_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
N, P = kp.N, kp.P
OP_IN, OP_OUT = sc.OP_IN, sc.OP_OUT
be32, op_record, op_result = sc.be32, sc.op_record, sc.op_result
FF = b"\xff" * 32
EDGE_KEYS = [1, 2, 3, N - 2, N - 1]
REFUSED_KEYS = [0, N, 2**256 - 1]


def vectors():
    with open(os.path.join(HERE, "golden", "bip340.json")) as f:
        return [{k: bytes.fromhex(v) for k, v in vec.items()} for vec in json.load(f)["vectors"]]


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def tagged(tag, data):
    t = hashlib.sha256(tag.encode()).digest()
    return hashlib.sha256(t + t + data).digest()


def _jdbl(p):
    x, y, z = p
    a, b = x * x % P, y * y % P
    c = b * b % P
    d = 4 * x * b % P
    e = 3 * a
    x3 = (e * e - 2 * d) % P
    return x3, (e * (d - x3) - 8 * c) % P, 2 * y * z % P


def _jadd(p, q):
    """Jacobian + Jacobian, neither infinity; None for p = -q"""
    x1, y1, z1 = p
    x2, y2, z2 = q
    z1z1, z2z2 = z1 * z1 % P, z2 * z2 % P
    u1, u2 = x1 * z2z2 % P, x2 * z1z1 % P
    s1, s2 = y1 * z2 * z2z2 % P, y2 * z1 * z1z1 % P
    if u1 == u2:
        return _jdbl(p) if s1 == s2 else None
    h, r = (u2 - u1) % P, (s2 - s1) % P
    hh = h * h % P
    hhh, v = h * hh % P, u1 * hh % P
    x3 = (r * r - hhh - 2 * v) % P
    return x3, (r * (v - x3) - s1 * hhh) % P, h * z1 * z2 % P


def mul(k, pt):
    """k * pt for an affine point (None = infinity), 4-bit windows from the top; affine result"""
    k %= N
    if k == 0 or pt is None:
        return None
    tab = [None, (pt[0], pt[1], 1)]
    for i in range(2, 16):
        tab.append(_jadd(tab[i - 1], tab[1]))
    acc = None
    for shift in range(252, -1, -4):
        if acc is not None:
            for _ in range(4):
                acc = _jdbl(acc)
        w = (k >> shift) & 15
        if w:
            acc = tab[w] if acc is None else _jadd(acc, tab[w])
    if acc is None:
        return None
    zi = pow(acc[2], -1, P)
    return acc[0] * zi * zi % P, acc[1] * zi * zi * zi % P


@functools.lru_cache(maxsize=None)
def gmul(k):
    return mul(k, kp.G)


def lift_x(x):
    """the point with this x and even y, or None (x >= p, or x^3 + 7 no square)"""
    if x >= P:
        return None
    c = (x**3 + 7) % P
    y = pow(c, (P + 1) // 4, P)
    if y * y % P != c:
        return None
    return x, (y if y % 2 == 0 else P - y)


def expand(d0):
    """(record d | P.x, P.x, ok) of a private key as a 256-bit integer; a key outside [1, n-1] gives zeros and 0"""
    if not 1 <= d0 < N:
        return bytes(64), bytes(32), 0
    pt = gmul(d0)
    d = d0 if pt[1] % 2 == 0 else N - d0
    return be32(d) + be32(pt[0]), be32(pt[0]), 1


def nonce(rec, msg, aux):
    """k' of "Default Signing" from a record"""
    t = bytes(a ^ b for a, b in zip(rec[:32], tagged("BIP0340/aux", aux)))
    return int.from_bytes(tagged("BIP0340/nonce", t + rec[32:] + msg), "big") % N


def sign_with_nonce(d, px, k0, msg, negate=True):
    """R.x | s for the nonce k' on integers; negate=False keeps k = k' whatever the parity of R.y (the "parity" cases)"""
    if not 1 <= k0 < N:
        return None
    R = gmul(k0)
    k = N - k0 if negate and R[1] % 2 else k0
    e = int.from_bytes(tagged("BIP0340/challenge", be32(R[0]) + px + msg), "big") % N
    return be32(R[0]) + be32((k + e * d) % N)


def sign(rec, msg, aux):
    """(sig, ok) from a record: the signing lane's contract (a refused record: zeros and 0)"""
    d = int.from_bytes(rec[:32], "big")
    if not 1 <= d < N:
        return bytes(64), 0
    sig = sign_with_nonce(d, rec[32:], nonce(rec, msg, aux), msg)
    return (bytes(64), 0) if sig is None else (sig, 1)


def final_point(pk, msg, sig):
    """("refused", None) for a range or lift failure, else ("point", R) with R = s G - e P (None = infinity)"""
    Pt = lift_x(int.from_bytes(pk, "big"))
    r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
    if Pt is None or r >= P or s >= N:
        return "refused", None
    e = int.from_bytes(tagged("BIP0340/challenge", sig[:32] + pk + msg), "big") % N
    return "point", kp.pt_add(gmul(s), mul(N - e, Pt))


def verify(pk, msg, sig):
    kind, R = final_point(pk, msg, sig)
    return 1 if kind == "point" and R is not None and R[1] % 2 == 0 and R[0] == int.from_bytes(sig[:32], "big") else 0


# ---- the signing cases ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def triples():
    """[(key as an integer below 2^256, message, aux)]: the edge keys, the refused keys, zero and all-FF messages and aux, seeded ones"""
    rng = random.Random(0xB1F340)
    out = [(d, rng.randbytes(32), rng.randbytes(32)) for d in EDGE_KEYS + REFUSED_KEYS + [6]]          # 6 G has odd y
    for m in (bytes(32), FF):
        for a in (bytes(32), FF):
            out.append((rng.randrange(1, N), m, a))
    out += [(3, bytes(32), bytes(32)), (N - 3, FF, FF)]
    while len(out) < 300:
        out.append((rng.randrange(1, N), rng.randbytes(32), rng.randbytes(32)))
    return out


def key_blob():
    return b"".join(be32(d) for d, _, _ in triples())


@functools.lru_cache(maxsize=None)
def expanded():
    """[(record, P.x, ok)] of triples()"""
    return [expand(d) for d, _, _ in triples()]


@functools.lru_cache(maxsize=None)
def signed(zero_aux=False):
    """[(sig, ok)] of triples(), key i signing message i; zero_aux: as with aux = NULL"""
    return [sign(rec, m, bytes(32) if zero_aux else a) for (rec, _, _), (_, m, a) in zip(expanded(), triples())]


@functools.lru_cache(maxsize=None)
def parity_coverage():
    """{(key's y odd, nonce's y odd)} over the valid triples"""
    seen = set()
    for (d0, m, a), (rec, _, ok) in zip(triples(), expanded()):
        if ok:
            seen.add((gmul(d0)[1] % 2, gmul(nonce(rec, m, a))[1] % 2))
    return seen


# ---- the verification cases -----------------------------------------------------------------------------------------------------------
def _flip(b, bit):
    return bytes(x ^ (1 << (bit % 8)) if i == bit // 8 else x for i, x in enumerate(b))


def _non_residue_x(rng):
    while True:
        x = rng.randrange(P)
        if lift_x(x) is None:
            return x


@functools.lru_cache(maxsize=None)
def cases():
    """[(category, pk, msg, sig)]"""
    rng = random.Random(0x340CA5E)
    out = []
    valid = [(i, rec, pk, m, a, sig) for i, ((_, m, a), (rec, pk, _), (sig, ok)) in enumerate(zip(triples(), expanded(), signed())) if ok]
    for j, (i, rec, pk, m, a, sig) in enumerate(valid):
        out.append(("valid", pk, m, sig))
        out.append(("msg_bit", pk, _flip(m, rng.randrange(256)), sig))
        out.append(("r_bit", pk, m, _flip(sig[:32], rng.randrange(256)) + sig[32:]))
        out.append(("s_bit", pk, m, sig[:32] + _flip(sig[32:], rng.randrange(256))))
        other = next(valid[(j + t) % len(valid)][2] for t in range(1, 4) if valid[(j + t) % len(valid)][2] != pk)      # d and n - d share a key
        out.append(("other_key", other, m, sig))
        out.append(("neg_s", pk, m, sig[:32] + be32((N - int.from_bytes(sig[32:], "big")) % N)))
        k0 = nonce(rec, m, a)
        if gmul(k0)[1] % 2:                        # the un-negated nonce: the right x under an odd y
            out.append(("parity", pk, m, sign_with_nonce(int.from_bytes(rec[:32], "big"), pk, k0, m, negate=False)))
    # infinity: s = e d, so that s G - e P vanishes, for r = 0 and r = 1
    for r in (0, 1):
        for d0 in (rng.randrange(1, N), 6):
            rec, pk, _ = expand(d0)
            m = rng.randbytes(32)
            e = int.from_bytes(tagged("BIP0340/challenge", be32(r) + pk + m), "big") % N
            out.append(("infinity", pk, m, be32(r) + be32(e * int.from_bytes(rec[:32], "big") % N)))
    i0, rec0, pk0, m0, a0, sig0 = valid[10]
    # r an x of no curve point, s = 0, and the ranges
    for _ in range(4):
        out.append(("r_off_curve", pk0, m0, be32(_non_residue_x(rng)) + sig0[32:]))
    out.append(("s_zero", pk0, m0, sig0[:32] + bytes(32)))
    for r in (P, 2**256 - 1, P - 1):
        out.append(("range", pk0, m0, be32(r) + sig0[32:]))
    for s in (N, 2**256 - 1, N - 1):
        out.append(("range", pk0, m0, sig0[:32] + be32(s)))
    for pk in (P, 2**256 - 1, 0, P - 1):
        out.append(("range", be32(pk), m0, sig0))
    for _ in range(8):
        out.append(("pk_off_curve", be32(_non_residue_x(rng)), m0, sig0))
    # the two known answers and a spoiled copy of each
    for v in vectors():
        out.append(("vector", v["pk"], v["msg"], v["sig"]))
        out.append(("vector_spoiled", v["pk"], v["msg"], v["sig"][:63] + bytes([v["sig"][63] ^ 1])))
    return out


@functools.lru_cache(maxsize=None)
def expected_all():
    """bytes: the verdict of every case of cases(), from the model"""
    return bytes(verify(pk, m, sig) for _, pk, m, sig in cases())


def arrays():
    cs = cases()
    return b"".join(c[1] for c in cs), b"".join(c[2] for c in cs), b"".join(c[3] for c in cs)


def category_counts():
    """{category: [rejected, accepted]}"""
    out = {}
    for (cat, *_), ok in zip(cases(), expected_all()):
        out.setdefault(cat, [0, 0])[ok] += 1
    return out


# ---- the unit operations: (input records, expected output records) ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def op0_cases():
    """the tagged hashes against hashlib: edge and seeded data under every selector"""
    rng = random.Random(0x0340)
    datas = [(bytes(32),) * 3, (FF,) * 3, (bytes(32), FF, bytes(32)), (b"\x80" + bytes(31),) * 3, (bytes(31) + b"\x01", FF, b"\x7f" * 32)]
    datas += [(rng.randbytes(32), rng.randbytes(32), rng.randbytes(32)) for _ in range(20)]
    ins, outs = [], []
    for a, b, c in datas:
        for sel, tag in enumerate(("BIP0340/aux", "BIP0340/nonce", "BIP0340/challenge")):
            ins.append(op_record(a, b, c, 0, 0, sel))
            outs.append(op_result(1, tagged(tag, a if sel == 0 else a + b + c)))
    return ins, outs


@functools.lru_cache(maxsize=None)
def op1_cases():
    """lift_x: 0, small values, p - 1, p, 2^256 - 1, 40 seeded x on the curve and 40 on none"""
    rng = random.Random(0x1340)
    xs = [0, 1, 2, 3, 4, 5, 6, 7, P - 1, P - 2, P, P + 1, 2**256 - 1, kp.GX]
    on, off = [], []
    while len(on) < 40 or len(off) < 40:
        x = rng.randrange(P)
        (off if lift_x(x) is None else on).append(x)
    xs += on[:40] + off[:40]
    ins = [op_record(x) for x in xs]
    outs = []
    for x in xs:
        pt = lift_x(x)
        outs.append(op_result(0) if pt is None else op_result(1, pt[1]))
    return ins, outs


def _op2_out(pt, ok):
    return bytes(OP_OUT) if pt is None else be32(pt[0]) + be32(pt[1]) + bytes(32) + be32(ok)


@functools.lru_cache(maxsize=None)
def op2_cases():
    """the final check: Jacobian points with Z != 1 of both parities against r = x, x + 1 and x - 1, Z = 1, and Z = 0"""
    rng = random.Random(0x2340)
    ins, outs = [], []
    seen = [0, 0]
    while min(seen) < 12:
        pt = gmul(rng.randrange(1, N))
        seen[pt[1] % 2] += 1
        for z in (rng.randrange(2, P), 1, P - 1):
            X, Y = pt[0] * z * z % P, pt[1] * z * z * z % P
            for r in (pt[0], (pt[0] + 1) % P, (pt[0] - 1) % P, pt[0] ^ (1 << 255) if pt[0] ^ (1 << 255) < P else 0):
                ins.append(op_record(X, Y, z, r))
                outs.append(_op2_out(pt, 1 if r == pt[0] and pt[1] % 2 == 0 else 0))
        ins.append(op_record(X, Y, 0, pt[0]))
        outs.append(_op2_out(None, 0))
    return ins, outs


@functools.lru_cache(maxsize=None)
def op3_cases():
    """the signing equation: k' in {0, 1, n - 1, n, 2^256 - 1}, seeded nonces of both parities, d at its edges"""
    rng = random.Random(0x3340)
    ks = [0, 1, N - 1, N, 2**256 - 1, 2, 6, N - 6]
    seen = [0, 0]
    while min(seen) < 10:
        k = rng.randrange(1, N)
        seen[gmul(k)[1] % 2] += 1
        ks.append(k)
    ins, outs = [], []
    for j, k in enumerate(ks):
        d = (1, N - 1, 0)[j % 3] if j % 4 == 3 else rng.randrange(1, N)
        px, m = rng.randbytes(32), rng.randbytes(32)
        ins.append(op_record(d, px, k, m))
        sig = sign_with_nonce(d, px, k, m)
        outs.append(op_result(0) if sig is None else op_result(1, sig))
    return ins, outs


def all_op_cases():
    return [op0_cases(), op1_cases(), op2_cases(), op3_cases()]


@functools.lru_cache(maxsize=None)
def walk_cases():
    """op 2 of sbv_debug_secp256k1_recover_op, u2 (x, y) + u1 G, with u2 = 0, with u1 = 0 and with both 0 (infinity)"""
    rng = random.Random(0x4340)
    ins, outs = [], []
    for _ in range(6):
        pt = gmul(rng.randrange(1, N))
        for u1, u2 in ((rng.randrange(1, N), 0), (1, 0), (N - 1, 0), (0, rng.randrange(1, N)), (0, 1), (0, N - 1), (0, 0),
                       (rng.randrange(1, N), rng.randrange(1, N))):
            ins.append(op_record(pt[0], pt[1], u1, u2))
            q = kp.pt_add(mul(u2, pt), gmul(u1))
            outs.append(op_result(0) if q is None else op_result(1, q[0], q[1]))
    return ins, outs


# ---- large batches: the case set tiled with a rotation, expected values stay the model's ------------------------------------------------
def tiled(n, shift=0):
    """n verification items made of cases(), tile t rotated by shift + 7 t: (pks, msgs, sigs, ok)"""
    pks, msgs, sigs = arrays()
    ok = expected_all()
    m = len(ok)
    o = [bytearray() for _ in range(4)]
    t = 0
    while len(o[3]) < n:
        rot = (shift + 7 * t) % m
        for dst, src, w in zip(o, (pks, msgs, sigs, ok), (32, 32, 64, 1)):
            dst += src[w * rot:] + src[:w * rot]
        t += 1
    return tuple(bytes(b[:w * n]) for b, w in zip(o, (32, 32, 64, 1)))


def tiled_sign(n, shift=0):
    """n signing items: key_index and messages and aux of triples(), rotated as above: (key_index, msgs, aux, sigs, ok); the records
    are those of expanded() in order"""
    tr, sg = triples(), signed()
    m = len(tr)
    idx, msgs, aux, sigs, ok = [], bytearray(), bytearray(), bytearray(), bytearray()
    t = 0
    while len(idx) < n:
        rot = (shift + 7 * t) % m
        for k in list(range(rot, m)) + list(range(rot)):
            idx.append(k)
            msgs += tr[k][1]
            aux += tr[k][2]
            sigs += sg[k][0]
            ok.append(sg[k][1])
        t += 1
    return idx[:n], bytes(msgs[:32 * n]), bytes(aux[:32 * n]), bytes(sigs[:64 * n]), bytes(ok[:n])
