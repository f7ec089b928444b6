"""Cases and expected values of the secp256k1 public-key recovery tests, shared by the CPU tier (tests/test_k256_recover_cpu.py: the
emulated lanes and the host form) and the GPU tier (tests/test_gpu_k256_recover.py: the kernels), so that both run the same cases.
Expected values come from Python integers only: `recover` of k256_sign_cases (the model that proved the signer's recovery ids),
oracle/k256_py.py for points, and the input rules of include/sbv.h stated here on integers."""
import functools
import random

import k256_py as kp
import k256_sign_cases as sc

N, P = kp.N, kp.P
HALF = (N - 1) // 2
LOW_S = 1                                      # SBV_K256_RECOVER_LOW_S
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
OP_IN, OP_OUT = sc.OP_IN, sc.OP_OUT
be32, pub_bytes = sc.be32, sc.pub_bytes


@functools.lru_cache(maxsize=None)
def _model(rs, recid, digest):
    return sc.recover(rs, recid, digest)


def expected(rs, recid, digest, flags=0):
    """(Qx | Qy, ok) by the rules of include/sbv.h on integers; a refused input is 64 zero bytes and 0"""
    r, s = int.from_bytes(rs[:32], "big"), int.from_bytes(rs[32:], "big")
    if not (1 <= r < N and 1 <= s < N) or recid > 3 or (flags & LOW_S and s > HALF):
        return bytes(64), 0
    q = _model(rs, recid, digest)                  # None: x >= p, no root, or infinity
    return (bytes(64), 0) if q is None else (pub_bytes(q), 1)


def is_square(a):
    return pow(a % P, (P - 1) // 2, P) in (0, 1)


def sqrt_p(a):
    y = pow(a, (P + 1) // 4, P)
    return y if y * y % P == a % P else None


def lift(r, recid):
    """the point R' of (r, recid) or None"""
    x = r + (N if recid & 2 else 0)
    if recid > 3 or x >= P:
        return None
    y = sqrt_p(x**3 + 7)
    if y is None:
        return None
    return (x, y if (y & 1) == (recid & 1) else P - y)


def case(cat, r, s, recid, digest, flags=0):
    return (cat, be32(r) + be32(s), recid, digest if isinstance(digest, bytes) else be32(digest), flags)


@functools.lru_cache(maxsize=None)
def signer_pubs():
    """d G of sign_cases(), from the big-integer twin"""
    memo = {}
    out = []
    for d, _ in sc.sign_cases():
        if d not in memo:
            memo[d] = pub_bytes(kp.pt_mul(d, kp.G))
        out.append(memo[d])
    return out


def _liftable_r(rng):
    while True:
        r = rng.randrange(1, N)
        if is_square(r**3 + 7):
            return r


@functools.lru_cache(maxsize=None)
def cases():
    """[(category, r | s, recid, digest, flags)]"""
    rng = random.Random(0x2EC0FE2)
    out = []
    # the signer's own signatures: flags = 0 recovered without the rule, the low-S ones under SBV_K256_RECOVER_LOW_S; and the twins
    for sflags, rflags in ((0, 0), (sc.LOW_S, LOW_S)):
        for (d, h), (rs, rid) in zip(sc.sign_cases(), sc.sign_expected(sflags)):
            out.append(("signed", rs, rid, h, rflags))
            out.append(("twin", rs, rid ^ 1, h, rflags))
    r0, s0, h0 = _liftable_r(rng), rng.randrange(1, N), rng.randbytes(32)
    # refused inputs
    for r, s, rid in ((0, s0, 0), (N, s0, 0), (N + 1, s0, 1), (r0, 0, 0), (r0, N, 1), (r0, s0, 4), (r0, s0, 255), (r0, s0, 128),
                      (P - N, s0, 2), (P - N, s0, 3), (P - N + 5, s0, 2), (N - 1, s0, 2), (N - 1, s0, 3), (2**255, s0, 2)):
        out.append(case("refused", r, s, rid, h0))
    k = 0
    while k < 50:
        r = rng.randrange(1, N)
        if not is_square(r**3 + 7):
            out.append(case("refused", r, rng.randrange(1, N), k & 1, rng.randbytes(32)))
            k += 1
    for s in (HALF + 1, N - 1, rng.randrange(HALF + 1, N), rng.randrange(HALF + 1, N)):
        out.append(case("refused", r0, s, 0, h0, LOW_S))
        out.append(case("high_s_allowed", r0, s, 0, h0, 0))
    # the + n branch, valid: x in [n, p) on the curve, r = x - n
    for start, want in ((N + 1, 3), (N + (P - N) // 5, 1), (N + (P - N) // 2, 1), (N + 4 * ((P - N) // 5), 1)):
        x = start
        while want:
            if is_square(x**3 + 7):
                for rid in (2, 3):
                    out.append(case("plus_n", x - N, rng.randrange(1, N), rid, rng.randbytes(32)))
                want -= 1
            x += 1
    x = P - 1
    while not is_square(x**3 + 7):
        x -= 1
    out.append(case("plus_n", x - N, rng.randrange(1, HALF), 2, rng.randbytes(32), LOW_S))
    # infinity: R = k G, e = s k: s R = e G; and e +- 1: Q = -+ r^-1 G
    for _ in range(4):
        kk, s = rng.randrange(1, N), rng.randrange(1, N)
        R = kp.pt_mul(kk, kp.G)
        r, rid, e = R[0] % N, (R[1] & 1) | (2 if R[0] >= N else 0), s * kk % N
        out.append(case("infinity", r, s, rid, e))
        out.append(case("near_infinity", r, s, rid, (e + 1) % N))
        out.append(case("near_infinity", r, s, rid, (e - 1) % N))
        out.append(case("near_infinity", r, s, rid ^ 1, e))           # the other root: 2 s k r^-1 G
    # digest edges under any signature
    for h in sc.EDGE_DIGESTS:
        out.append(case("digest_edge", r0, s0, 0, h))
        out.append(case("digest_edge", _liftable_r(rng), rng.randrange(1, HALF), 1, h, LOW_S))
    # scalar edges
    for s in (1, N - 1, HALF, HALF + 1):
        for flags in (0, LOW_S):
            out.append(case("scalar_edge", r0, s, 1, h0, flags))
    ri0 = pow(r0, -1, N)
    sevens, eights = int("7" * 32, 16), int("8" * 32, 16)
    u2s = [1, 2**127 + 5, 2**128 - 1, LAMBDA, LAMBDA * (2**100 + 3) % N, (N - LAMBDA) % N]          # a GLV half of 0
    u2s += [int(c * 64, 16) for c in "1789ae"]                                                       # all-equal nibbles
    u2s += [(a + b * LAMBDA) % N for a in (0, sevens, eights) for b in (sevens, eights)]             # ... in the halves
    for u2 in u2s:
        out.append(case("scalar_edge", r0, u2 * r0 % N, 0, rng.randbytes(32)))
    # u1 = (n - e) r^-1 that carries out of window 16 of the comb (u1 + 0x8000...8000 >= 2^256), and the boundary
    edge = 2**256 - int("8000" * 16, 16)
    for u1 in (N - 1, N - 2, edge, edge - 1, edge + 1, 2**255 + 12345, 0, 1):
        e = (N - u1 * r0) % N
        assert (N - e) * ri0 % N == u1
        out.append(case("scalar_edge", r0, s0, 1, e))
    return out


@functools.lru_cache(maxsize=None)
def expected_all():
    """[(Qx | Qy, ok)] of cases()"""
    return [expected(rs, rid, h, flags) for _, rs, rid, h, flags in cases()]


def by_flags(flags):
    """(indices into cases(), sigs, recid, digests) of the cases of one flag setting, as the arrays of a call"""
    idx = [i for i, c in enumerate(cases()) if c[4] == flags]
    cs = [cases()[i] for i in idx]
    return idx, b"".join(c[1] for c in cs), bytes(min(c[2], 255) for c in cs), b"".join(c[3] for c in cs)


def category_counts():
    """{category: [refused, recovered]}"""
    out = {}
    for (cat, *_), (_, ok) in zip(cases(), expected_all()):
        out.setdefault(cat, [0, 0])[ok] += 1
    return out


# ---- the unit operations: (input records, expected output records), records as in k256_sign_cases ------------------------------------
FE_EDGES = [0, 1, 2, 3, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, 977, 2**32 + 977, 2**29 - 1, 2**29, 2**58 - 1, 2**116, 2**232 - 1, 2**232,
            2**255, (2**256 - 1) % P, 2**256 % P, int("5" * 64, 16), int("a" * 64, 16) % P, int("1fffffff" * 8, 16)]


@functools.lru_cache(maxsize=None)
def op0_cases():
    """square roots: small values, squares of the field's edge values, 50 residues and 50 non-residues, and values >= p"""
    rng = random.Random(0x5017)
    vals = [0, 1, 4, P - 1, 7] + [v * v % P for v in FE_EDGES]
    res, non = [], []
    while len(res) < 50 or len(non) < 50:
        a = rng.randrange(P)
        (res if is_square(a) else non).append(a)
    vals += res[:50] + non[:50] + [P, P + 4, 2**256 - 1]             # any 256-bit value is taken as its residue
    ins = [sc.op_record(v) for v in vals]
    outs = []
    for v in vals:
        y = sqrt_p(v % P)
        outs.append(sc.op_result(0) if y is None else sc.op_result(1, y))
    return ins, outs


@functools.lru_cache(maxsize=None)
def op1_cases():
    rng = random.Random(0x11F7)
    pairs = [(r, rid) for r in (1, 2, 3, P - N - 2, P - N - 1, P - N, P - N + 1, N - 1, N, P - 1, P, 2**256 - 1, 0) for rid in (0, 1, 2, 3)]
    pairs += [(rng.randrange(1, N), rng.randrange(4)) for _ in range(60)] + [(rng.randrange(P - N), 2 + (i & 1)) for i in range(20)]
    pairs += [(1, 4), (1, 255), (1, 2**32 - 1)]
    ins, outs = [], []
    for r, rid in pairs:
        ins.append(sc.op_record(r, rid))
        pt = lift(r, rid)
        outs.append(sc.op_result(0) if pt is None else sc.op_result(1, pt[0], pt[1]))
    return ins, outs


@functools.lru_cache(maxsize=None)
def op2_cases():
    """u2 (x, y) + u1 G: infinity from +-G with u1 = -+u2, u1 = 0, u2 = 1, doubling-shaped sums and seeded ones"""
    rng = random.Random(0x2256)
    G, nG = kp.G, kp.pt_neg(kp.G)
    quads = []
    for u2 in (1, 2, N - 1, rng.randrange(1, N), rng.randrange(1, N)):
        quads += [(G, (N - u2) % N, u2), (nG, u2, u2)]                # infinity
        quads += [(G, (N - u2 + 1) % N, u2), (nG, (u2 + 1) % N, u2)]  # G exactly
        quads += [(G, u2, u2)]                                        # 2 u2 G
    pts = [kp.pt_mul(rng.randrange(1, N), kp.G) for _ in range(6)]
    for pt in pts:
        quads += [(pt, 0, rng.randrange(1, N)), (pt, rng.randrange(1, N), 1), (pt, 0, 1), (pt, rng.randrange(N), rng.randrange(1, N))]
    d = rng.randrange(1, N)
    pt = kp.pt_mul(d, kp.G)
    di = pow(d, -1, N)
    for u2 in (rng.randrange(1, N), 5):
        quads += [(pt, (N - u2 * d) % N, u2), (pt, (1 - u2 * d) % N, u2)]         # infinity and G through a point that is not G
    assert di
    ins, outs = [], []
    for pt, u1, u2 in quads:
        ins.append(sc.op_record(pt[0], pt[1], u1, u2))
        q = kp.pt_add(kp.pt_mul(u2, pt), kp.pt_mul(u1, kp.G))
        outs.append(sc.op_result(0) if q is None else sc.op_result(1, q[0], q[1]))
    return ins, outs


def all_op_cases():
    return [op0_cases(), op1_cases(), op2_cases()]


# ---- large batches: the case set tiled with a rotation, expected values stay the model's ------------------------------------------------
def tiled(flags, n, shift=0):
    """n items made of the cases of one flag setting, tile t rotated by shift + 7 t: (sigs, recid, digests, pubs, ok)"""
    idx, sigs, rid, digs = by_flags(flags)
    exp = expected_all()
    m = len(idx)
    pubs, ok = b"".join(exp[i][0] for i in idx), bytes(exp[i][1] for i in idx)
    o = [bytearray() for _ in range(5)]
    t = 0
    while len(o[1]) < n:
        rot = (shift + 7 * t) % m
        for dst, src, w in zip(o, (sigs, rid, digs, pubs, ok), (64, 1, 32, 64, 1)):
            dst += src[w * rot:] + src[:w * rot]
        t += 1
    return tuple(bytes(b[:w * n]) for b, w in zip(o, (64, 1, 32, 64, 1)))
