"""Case generators and big-integer references for the device-arithmetic unit tier (tools/devunit.hip).

One generator gen_<op>(rng, n) and one checker chk_<op>(rec, out) per op of the unit library; the names are the product's.
A generator returns input records (lists of Python ints, one per 32-bit word of the op's record; signed limbs as signed ints):
first the edge cases — the values the CPU tier uses plus limb patterns at every bound the headers state — then n random ones.
Every record is constructed INSIDE the op's documented contract, never filtered: run_op() counts the cases it checks and the
tests assert checked == generated.  tests/test_devunit_cpu.py proves the "inside the contract" half by running every record
through a g++ build of the same primitives with the SBV_*_CHECK assertions on (a breach aborts).

A checker compares the op's output with Python big integers (oracle/*.py for the group laws, hashlib for SHA-512): the value
modulo the prime AND the output form the header promises (limb ranges, value interval).  It never looks at another build of
the source under test.  Used by both backends of the library: 0 = host loop (CPU tier), 1 = gfx950 kernel (GPU tier).
"""
import ctypes
import hashlib
import hmac
import os
import random
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ed25519_py as ed  # noqa: E402
import k256_py as kc  # noqa: E402
import p256_py as ec  # noqa: E402
import p256_sign_cases as sign_cases  # noqa: E402

SEED = 0xD3C0DE
M29 = (1 << 29) - 1
P, N = ec.P, ec.N
R = 1 << 261                      # Montgomery radix of p256_fe29.h / p256_sc29.h
R32 = 1 << 256                    # ... of the 8 x 32 forms (p256_fe.h, p256_sc.h)
RINV_P, RINV_N = pow(R, -1, P), pow(R, -1, N)
P25, L25 = ed.P, ed.L
KP, KN = kc.P, kc.N
MODULI = [P, N, P25, KP, KN]      # modinv30.h: the five moduli of the library, indexed as devunit's modinfo_of()
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72

BAD_OP, BAD_ARG, NOT_AVAILABLE = -1000, -1001, -1002


# ---- the library -------------------------------------------------------------------------------------------------------------
def load(path=None):
    """ctypes handle on tools/libsbv_devunit.so (built by tools/Makefile) or on another build of tools/devunit.hip"""
    lib = ctypes.CDLL(path or os.path.join(ROOT, "tools", "libsbv_devunit.so"))
    lib.sbvd_run.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    lib.sbvd_op_words.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    lib.sbvd_op_name.restype = ctypes.c_char_p
    lib.ops = {}
    for i in range(lib.sbvd_op_count()):
        a, b = ctypes.c_uint32(), ctypes.c_uint32()
        assert lib.sbvd_op_words(i, ctypes.byref(a), ctypes.byref(b)) == 0
        lib.ops[lib.sbvd_op_name(i).decode()] = (i, a.value, b.value, bool(lib.sbvd_op_is_cross_lane(i)))
    return lib


def build_checked():
    """g++ build of tools/devunit.hip with every contract assertion on (host backend only), next to the emulator"""
    src = os.path.join(ROOT, "tools", "devunit.hip")
    so = os.path.join(ROOT, "tests", "emul", "libsbv_devunit_check.so")
    csrc = os.path.join(ROOT, "consensus_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-misleading-indentation", "-DSBV_F29_CHECK",
                               "-DSBV_F25_CHECK", "-DSBV_K256_CHECK", "-x", "c++", src, "-o", so])
    return so


class HipError(Exception):
    pass


def launch(lib, backend, name, recs):
    """one sbvd_run over the records -> outputs as lists of SIGNED 32-bit ints (u() makes a word of one)"""
    idx, in_w, out_w, _ = lib.ops[name]
    arr = np.array(recs, dtype=np.int64)
    assert arr.shape == (len(recs), in_w), (name, arr.shape, in_w)
    buf = np.ascontiguousarray((arr & 0xFFFFFFFF).astype(np.uint32))
    out = np.empty((len(recs), out_w), dtype=np.uint32)
    rc = lib.sbvd_run(backend, idx, buf.ctypes.data, out.ctypes.data, len(recs))
    if rc != 0:
        raise HipError(f"sbvd_run({name}, backend {backend}, {len(recs)} cases) returned {rc}")
    return out.view(np.int32).tolist()


def hexs(vals):
    return "[" + " ".join(("-" if v < 0 else "") + hex(abs(v)) for v in vals) + "]"


def run_op(lib, backend, name, n_random, seed=SEED):
    """generate, run, check every case; returns (generated, checked).  A mismatch raises with op, case index, input and output in hex."""
    rng = random.Random(f"{seed}:{name}")
    recs = GEN[name](rng, n_random)
    outs = launch(lib, backend, name, recs)
    chk = CHK[name]
    checked = 0
    for i, (rec, out) in enumerate(zip(recs, outs)):
        try:
            chk(rec, out)
        except AssertionError as e:
            raise AssertionError(f"{name} (backend {backend}) case {i} of {len(recs)}: {e}\n  in  = {hexs(rec)}\n  out = {hexs(out)}") from None
        checked += 1
    return len(recs), checked


# ---- limbs -------------------------------------------------------------------------------------------------------------------
def u(x):
    return x & 0xFFFFFFFF


def val29(l):
    return sum(v << (29 * i) for i, v in enumerate(l))


def tight(x):
    """limbs 0..7 in [0, 2^29), limb 8 the (signed) rest"""
    return [(x >> (29 * i)) & M29 for i in range(8)] + [x >> 232]


def words(x, n=8):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def wval(w):
    return sum(u(v) << (32 * i) for i, v in enumerate(w))


def loose(rng, bits=29, top_lo=-(1 << 24), top_hi=1 << 25):
    """limbs 0..7 uniform in (-2^bits, 2^bits), limb 8 in [top_lo, top_hi): a sum / difference of tight values"""
    x = rng.getrandbits(8 * (bits + 1))
    m = (1 << (bits + 1)) - 1
    return [max(((x >> ((bits + 1) * i)) & m) - (1 << bits), 1 - (1 << bits)) for i in range(8)] + [rng.randrange(top_lo, top_hi)]


def spread(rng, x, k=2):
    """the value x on non-canonical limbs: random borrows between neighbours (|limb| stays below (k + 1) 2^29)"""
    l = tight(x) if x >= 0 else [-v for v in tight(-x)]
    for i in range(8):
        d = rng.randrange(-k, k + 1)
        l[i] += d << 29
        l[i + 1] -= d
    return l


def edge_values(m, r=R):
    return [0, 1, 2, m - 1, m - 2, (m - 1) // 2, 2**32 - 1, 2**32, 2**64 - 1, 2**96, 2**128 - 1, 2**192, 2**224 - 1, 2**255 % m,
            (2**256 - 1) % m, 0xFFFFFFFF00000000FFFFFFFF00000000FFFFFFFF00000000FFFFFFFF00000000 % m,
            0x00000000FFFFFFFF00000000FFFFFFFF00000000FFFFFFFF00000000FFFFFFFF % m, r % m, (r * r) % m]


def check_limbs(out, lo=0, hi=1 << 29):
    assert all(lo <= out[i] < hi for i in range(8)), "limbs 0..7 outside [%s, %s)" % (hex(lo), hex(hi))


# ---- P-256 field (p256_fe29.h) ---------------------------------------------------------------------------------------------------
F29_EDGE = [0, 1, P - 1, P, 2 * P, (1 << 256) - 1, R % P, (1 << 232) - 1, M29, M29 << 29] + edge_values(P)[2:]
BIG = (1 << 29) + (1 << 25)          # the loosest limb f29_mul documents (value-reduced coordinates plus a carry)
BIGX = (1 << 29) + (1 << 26)         # ... and the hot-path forms


def f29_patterns(big):
    """limb patterns at the bounds of the operand contract: all limbs extreme, alternating signs, one extreme limb, both ends of limb 8"""
    pats = []
    for s in (1, -1):
        pats += [[s * big] * 8 + [s * (1 << 24)], [s * (1 << 29)] * 8 + [-s * (1 << 24)], [s * M29] * 8 + [s * (1 << 24)],
                 [s * M29, -s * M29] * 4 + [s * (1 << 24)], [s * big, -s * big] * 4 + [-s * (1 << 24)], [0] * 8 + [s * ((1 << 25) - 1)]]
        for i in range(9):
            pats.append([0] * i + [s * (M29 if i < 8 else (1 << 24))] + [0] * (8 - i))
    return pats


def f29_operand(rng, big=BIG):
    k = rng.randrange(6)
    if k == 0:
        return tight(rng.randrange(2 * P))
    if k == 1:
        return [-v for v in tight(rng.randrange(2 * P))]
    if k == 2:
        return loose(rng)
    if k == 3:
        return tight(rng.choice(F29_EDGE))
    if k == 4:                                                   # the last 2^32 below the upper end of a product's output interval
        return tight(3 * P // 2 - rng.getrandbits(32))
    return rng.choice(f29_patterns(big))


def f29_pairs(rng, n, big=BIG):
    pats = f29_patterns(big)
    recs = [tight(a) + tight(b) for a in F29_EDGE for b in F29_EDGE]
    recs += [a + b for a in pats for b in pats[::3]]
    recs += [f29_operand(rng, big) + f29_operand(rng, big) for _ in range(n)]
    return recs


def f29_singles(rng, n, big=BIG):
    return [tight(a) for a in F29_EDGE] + f29_patterns(big) + [f29_operand(rng, big) for _ in range(n)]


def chk_mont_product(out, prod, m):
    """r = prod / R mod m exactly as a word-by-word Montgomery reduction leaves it: r R = prod + k m with 0 <= k < R"""
    v = val29(out)
    check_limbs(out)
    assert (v * R - prod) % m == 0, "value != product / R (mod m): got " + hex(v)
    assert prod <= v * R < prod + m * R, "value outside (prod / R, prod / R + m): " + hex(v)


def gen_f29_mul(rng, n):
    return f29_pairs(rng, n)


def chk_f29_mul(rec, out):
    chk_mont_product(out, val29(rec[:9]) * val29(rec[9:18]), P)


def gen_f29_sqr(rng, n):
    return f29_singles(rng, n)


def chk_f29_sqr(rec, out):
    chk_mont_product(out, val29(rec) ** 2, P)


def chk_reduce_x(out, prod):
    v = val29(out)
    check_limbs(out)
    assert (v * R - prod) % P == 0, "value != product / R (mod p): got " + hex(v)
    assert abs(v * R - prod) <= 401 * P * R // 100, "value further than 4.01 p from product / R: " + hex(v)


def x_operand(rng):
    k = rng.randrange(5)
    if k == 0:
        return tight(rng.randrange(5 * P))
    if k == 1:
        return [-v for v in tight(rng.randrange(5 * P))]
    if k == 2:
        return loose(rng)
    if k == 3:
        return tight(5 * P - 1 - rng.getrandbits(32))
    s = rng.choice((1, -1))
    return [s * BIGX] * 8 + [s * rng.randrange(1 << 26)]


def gen_f29_mulx(rng, n):
    pats = f29_patterns(BIGX)
    return [tight(a) + tight(b) for a in F29_EDGE for b in F29_EDGE[::2]] + [a + b for a in pats for b in pats[::3]] + \
           [x_operand(rng) + x_operand(rng) for _ in range(n)]


def chk_f29_mulx(rec, out):
    chk_reduce_x(out, val29(rec[:9]) * val29(rec[9:18]))


def gen_f29_sqrx(rng, n):
    return [tight(a) for a in F29_EDGE] + f29_patterns(BIGX) + [x_operand(rng) for _ in range(n)]


def chk_f29_sqrx(rec, out):
    chk_reduce_x(out, val29(rec) ** 2)


def chk_red_q(out, want):
    v = val29(out)
    assert (v * R - want) % P == 0, "value != expected (mod p): got " + hex(v)
    assert -(1 << 231) < v < (1 << 256) + (1 << 231), "value outside (-2^231, 2^256 + 2^231): " + hex(v)
    check_limbs(out, -(1 << 27) + 1, (1 << 29) + (1 << 27))


def gen_f29_mul_sub_mul(rng, n):
    pats = f29_patterns(BIGX)
    recs = [a + b + c + d for a in pats[::5] for b in pats[::7] for c in pats[1::5] for d in pats[2::7]]
    recs += [tight(a) + tight(b) + tight(b) + tight(a) for a in F29_EDGE for b in F29_EDGE[::3]]          # a b - b a = 0
    return recs + [x_operand(rng) + x_operand(rng) + x_operand(rng) + x_operand(rng) for _ in range(n)]


def chk_f29_mul_sub_mul(rec, out):
    a, b, c, d = (val29(rec[9 * i:9 * i + 9]) for i in range(4))
    chk_red_q(out, a * b - c * d)


def sub_val_operand(rng):
    return [x + y for x, y in zip(tight(rng.randrange(5 * P)), tight(rng.randrange(9 * P)))]       # PPP + 2 Q of the mixed addition


def gen_f29_sqr_sub_val(rng, n):
    top = [x + y for x, y in zip(tight(5 * P - 1), tight(9 * P - 1))]
    recs = [a + w for a in f29_patterns(BIGX) for w in (tight(0), top, [M29] * 8 + [1 << 26], [2 * M29] * 8 + [0])]
    recs += [tight(a) + tight(a * a * RINV_P % P) for a in F29_EDGE]                                        # a^2 - a^2 = 0
    return recs + [x_operand(rng) + sub_val_operand(rng) for _ in range(n)]


def chk_f29_sqr_sub_val(rec, out):
    chk_red_q(out, val29(rec[:9]) ** 2 - val29(rec[9:]) * R)


def canon_input(rng):
    """any value in (-16 p, 16 p) on limbs |v[i]| < 2^31"""
    k = rng.randrange(4)
    if k == 0:
        return loose(rng, 31, -(1 << 27), 1 << 27)
    if k == 1:
        return spread(rng, rng.randrange(-16 * P + 1, 16 * P))
    if k == 2:
        return spread(rng, rng.randrange(-15, 16) * P + rng.randrange(-2, 3))
    s = rng.choice((1, -1))
    return spread(rng, s * (16 * P - 1 - rng.getrandbits(32)), 1)           # the last 2^32 of the range


def gen_f29_canon(rng, n):
    recs = [spread(rng, k * P + d) for k in range(-15, 16) for d in (-1, 0, 1)]
    recs += [tight(16 * P - 1), [-v for v in tight(16 * P - 1)], [(1 << 31) - 1] * 8 + [(1 << 27) - 1], [-(1 << 31) + 1] * 8 + [-(1 << 27) + 1],
             [(1 << 31) - 1, -(1 << 31) + 1] * 4 + [0], [M29] * 8 + [-1], [0] * 8 + [-(1 << 27)]]
    recs += [tight(a) for a in F29_EDGE]
    return recs + [canon_input(rng) for _ in range(n)]


def chk_f29_canon(rec, out):
    a = val29(rec)
    assert abs(a) < 16 * P
    assert out == tight(a % P), "not the canonical limbs of " + hex(a % P)


gen_f29_norm = gen_f29_canon


def chk_f29_norm(rec, out):
    assert val29(out) == val29(rec), "value changed"
    check_limbs(out, -7, (1 << 29) + 8)


gen_f29_norm_red = gen_f29_canon


def chk_f29_norm_red(rec, out):
    v = val29(out)
    assert (v - val29(rec)) % P == 0, "value changed (mod p)"
    assert -(1 << 229) < v < (1 << 256) + (1 << 229), "value outside (-2^229, 2^256 + 2^229): " + hex(v)
    check_limbs(out, -(1 << 25) - 7, (1 << 29) + (1 << 25) + 8)


def gen_f29_is_zero(rng, n):
    recs = []
    for k in range(-16, 17):
        for _ in range(4):
            l = spread(rng, k * P)
            recs.append(list(l))
            l[rng.randrange(8)] += 1 + rng.randrange(5)
            recs.append(l)
    recs += [tight(a) for a in F29_EDGE]
    return recs + [canon_input(rng) for _ in range(n)]


def chk_f29_is_zero(rec, out):
    assert out == [1 if val29(rec) % P == 0 else 0]


gen_f29_maybe_zero = gen_f29_is_zero


def chk_f29_maybe_zero(rec, out):
    # the filter as the header states it (a multiple k p, |k| <= 16, has low limb -k mod 2^29) ...
    assert out == [1 if ((rec[0] + 16) & M29) <= 32 else 0]
    # ... and what the callers rely on: it never misses a zero
    assert out == [1] or val29(rec) % P != 0


def gen_f29_pack(rng, n):
    return [tight(a % P) for a in F29_EDGE] + [tight(P - 1 - rng.getrandbits(32)) for _ in range(8)] + [tight(rng.randrange(P)) for _ in range(n)]


def chk_f29_pack(rec, out):
    assert wval(out) == val29(rec)


def gen_words256(rng, n, m=1 << 256):
    return [words(a % m) for a in F29_EDGE + edge_values(m if m < (1 << 256) else P)] + \
           [words(m - 1 - rng.getrandbits(32)) for _ in range(8)] + [words(rng.randrange(m)) for _ in range(n)]


def gen_f29_unpack(rng, n):
    return gen_words256(rng, n) + [words(0xFFFFFFFF00000000FFFFFFFF00000000FFFFFFFF00000000FFFFFFFF00000000), words((1 << 256) - 1)]


def chk_f29_unpack(rec, out):
    assert out == tight(wval(rec))


def gen_f29_from_fe(rng, n):
    return gen_words256(rng, n, P)


def chk_f29_from_fe(rec, out):
    chk_mont_product(out, wval(rec) * ((1 << 266) % P), P)           # X = x 2^256  ->  x 2^261


def gen_f29_from_plain(rng, n):
    return gen_words256(rng, n)


def chk_f29_from_plain(rec, out):
    chk_mont_product(out, wval(rec) * (R * R % P), P)


def gen_f29_to_fe(rng, n):
    return f29_singles(rng, n)


def chk_f29_to_fe(rec, out):
    assert wval(out) == val29(rec) * pow(32, -1, P) % P               # x 2^261 -> x 2^256, canonical


def gen_f29_inv(rng, n):
    return gen_f29_canon(rng, n)


def chk_f29_inv(rec, out):
    a = val29(rec) % P
    v = val29(out)
    check_limbs(out)
    want = pow(a, -1, P) * R * R % P if a else 0
    assert v % P == want, "not the inverse: " + hex(v % P)
    assert -1 < v < 2 * P


gen_f29_inv_ct, chk_f29_inv_ct = gen_f29_inv, chk_f29_inv


def gen_f29_mulchain(rng, n):
    """chains of dependent products: the device keeps values loose from one operation to the next"""
    recs = []
    for k in (0, 1, 2, 3, 8):
        recs += [tight(a) + tight(b) + [k] for a in F29_EDGE[::2] for b in (0, 1, P - 1, 2 * P - 1, R % P, 3 * P // 2)]
        recs += [a + tight(2 * P - 1) + [k] for a in f29_patterns(BIG)]
    return recs + [f29_operand(rng) + tight(rng.randrange(2 * P)) + [rng.choice((2, 3, 8))] for _ in range(n)]


def chk_f29_mulchain(rec, out):
    a, b, k = val29(rec[:9]), val29(rec[9:18]), rec[18]
    v = val29(out)
    assert (v - a * pow(b * RINV_P, k, P)) % P == 0, "value != a (b / R)^k (mod p)"
    if k:
        check_limbs(out)
        assert -P // 2 - 1 < v < 3 * P // 2 + 1, "value outside (-p/2, 3p/2): " + hex(v)
    else:
        assert out == rec[:9]


# ---- P-256 scalars (p256_sc29.h, p256_sc.h) and the division-step inversions (modinv30.h) -----------------------------------------------
S29_EDGE = [0, 1, N - 1, N, (1 << 256) - 1, R % N, (R * R) % N] + edge_values(N)[2:]


def gen_s29_mul(rng, n):
    pats = f29_patterns(BIG)
    recs = [tight(a) + tight(b) for a in S29_EDGE for b in S29_EDGE]
    recs += [a + b for a in pats for b in pats[::3]]
    return recs + [f29_operand(rng) + f29_operand(rng) for _ in range(n)]


def chk_s29_mul(rec, out):
    chk_mont_product(out, val29(rec[:9]) * val29(rec[9:18]), N)


def s29_canon_input(rng):
    k = rng.randrange(3)
    if k == 0:
        return spread(rng, rng.randrange(-2 * N + 1, 3 * N))
    if k == 1:
        return spread(rng, rng.randrange(-1, 3) * N + rng.randrange(-2, 3))
    return spread(rng, rng.choice((3 * N - 1 - rng.getrandbits(32), -2 * N + 1 + rng.getrandbits(32))), 1)


def gen_s29_canon(rng, n):
    recs = [spread(rng, k * N + d) for k in range(-2, 3) for d in (-1, 0, 1) if -2 * N < k * N + d < 3 * N]
    recs += [tight(3 * N - 1), [-v for v in tight(2 * N - 1)]] + [tight(a) for a in S29_EDGE]
    return recs + [s29_canon_input(rng) for _ in range(n)]


def chk_s29_canon(rec, out):
    a = val29(rec)
    assert -2 * N < a < 3 * N
    assert out == tight(a % N), "not the canonical limbs of " + hex(a % N)


gen_s29_inv = gen_s29_canon


def chk_s29_inv(rec, out):
    a = val29(rec) % N
    v = val29(out)
    check_limbs(out)
    assert v % N == (pow(a, -1, N) * R * R % N if a else 0), "not the inverse: " + hex(v % N)
    assert -1 < v < 2 * N


gen_s29_inv_ct, chk_s29_inv_ct = gen_s29_inv, chk_s29_inv


def gen_sc_mul(rng, n):
    e = edge_values(N, R32)
    return [words(a) + words(b) for a in e for b in e] + [words(rng.randrange(N)) + words(rng.randrange(N)) for _ in range(n)]


def chk_sc_mul(rec, out):
    assert wval(out) == wval(rec[:8]) * wval(rec[8:]) * pow(R32, -1, N) % N


def gen_resid(m, r):
    def gen(rng, n):
        e = edge_values(m, r) + [m - 1 - rng.getrandbits(32) for _ in range(4)] + [rng.randrange(1 << k) for k in (8, 31, 61, 200) for _ in range(4)]
        return [words(a) for a in e] + [words(rng.randrange(m)) for _ in range(n)]
    return gen


def chk_mont_inv(m, r):
    def chk(rec, out):
        a = wval(rec)
        assert wval(out) == (pow(a * pow(r, -1, m), -1, m) * r % m if a else 0)
    return chk


gen_sc_inv = gen_sc_inv_gcd = gen_resid(N, R32)
chk_sc_inv = chk_sc_inv_gcd = chk_mont_inv(N, R32)
gen_fe_inv_gcd, chk_fe_inv_gcd = gen_resid(P, R32), chk_mont_inv(P, R32)


def gen_modinv30(rng, n):
    recs = []
    for which, m in enumerate(MODULI):
        xs = [0, 1, 2, 3, m - 1, m - 2, (m - 1) // 2, (m + 1) // 2, m // 3, 2**32, 2**64 - 1, 2**128, 2**255 % m, 2**256 % m, (2**256 - 1) % m,
              2**30, 2**30 - 1, 2**60 + 1, (1 << 200) - 1]
        xs += [rng.randrange(1, 1 << rng.randrange(1, 256)) % m for _ in range(40)]
        xs += [rng.randrange(m) for _ in range((n + 4) // 5)]
        recs += [[which] + words(x) for x in xs]
    return recs


def chk_modinv30(rec, out):
    m, x = MODULI[rec[0]], wval(rec[1:])
    assert wval(out) == (pow(x, -1, m) if x else 0)


gen_modinv30_ct, chk_modinv30_ct = gen_modinv30, chk_modinv30


# ---- P-256 points (p256_pt29.h) ---------------------------------------------------------------------------------------------------
def mont(x):
    return x * R % P


def sqrt_p(a):
    r = pow(a, (P + 1) // 4, P)                     # p = 3 (mod 4)
    return r if r * r % P == a % P else None


def point_with_x_from(x0):
    """the first curve point with x >= x0 (P-256 has cofactor 1: every curve point is in the group)"""
    x = x0
    while True:
        y = sqrt_p((x * x * x + ec.A * x + ec.B) % P)
        if y is not None:
            return (x, y)
        x += 1


_pts = None


def points():
    """a pool of group elements: small and large multiples of G, their neighbours, and the points whose x lies in [n, p)"""
    global _pts
    if _pts is None:
        rng = random.Random(f"{SEED}:points")
        ks = [1, 2, 3, 4, 5, 7, 8, 16, N - 1, N - 2, N - 3, (N - 1) // 2, (N + 1) // 2] + [rng.randrange(1, N) for _ in range(40)]
        _pts = [ec.pt_mul(k, ec.G) for k in ks] + [point_with_x_from(N), point_with_x_from(N + (1 << 64)), point_with_x_from(P - (1 << 20))]
        _pts += [ec.pt_neg(q) for q in _pts[:8]]
    return _pts


def fe_forms(rng, v, lo_k, hi_k):
    """a tight representation of the residue v (canonical value) shifted by a multiple of p from [lo_k, hi_k]"""
    return tight(v + rng.randrange(lo_k, hi_k + 1) * P)


def vr_forms(rng, v):
    """value-reduced forms of the residue v: the canonical one, and v + p / v - p where they fit (-2^231, 2^256 + 2^231)"""
    forms = [v]
    if v + P < (1 << 256) + (1 << 231):
        forms.append(v + P)
    if v - P > -(1 << 231):
        forms.append(v - P)
    return tight(rng.choice(forms))


def xyzz_of(rng, pt, noncanon=0):
    """an XYZZ record of the affine point (None = infinity).  noncanon 1: X sits in [p, 2^256 + 2^231), 2: X is negative — zz is then
    chosen so that X = x zz^2 R takes such a value; ZZ, ZZZ always carry a random multiple of p within +-4 p"""
    if pt is None:
        return [0] * 36 + [1]
    x, y = pt
    while True:
        if noncanon:
            v = rng.getrandbits(rng.choice((8, 64, 200, 223))) + 1
            zz2 = v * pow(mont(x), -1, P) % P       # X = v  <=>  zz^2 = v / (x R)
            zz = sqrt_p(zz2)
            if zz is None:
                continue
        else:
            zz = rng.randrange(1, P)
        break
    z2, z3 = zz * zz % P, zz * zz * zz % P
    X, Y = mont(x * z2), mont(y * z3)
    if noncanon == 1:
        Xl = tight(X + P)
    elif noncanon == 2:
        Xl = tight(X - P) if X - P > -(1 << 231) else tight(X)
    else:
        Xl = vr_forms(rng, X)
    return Xl + vr_forms(rng, Y) + fe_forms(rng, mont(z2), -4, 3) + fe_forms(rng, mont(z3), -4, 3) + [0]


def affine_of_xyzz(out):
    if out[36]:
        return None
    X, Y, ZZ, ZZZ = (val29(out[9 * i:9 * i + 9]) for i in range(4))
    assert ZZ % P != 0, "finite point with ZZ = 0"
    assert pow(ZZ, 3, P) == pow(ZZZ, 2, P) * R % P, "ZZ^3 != ZZZ^2"
    return (X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P)


def aff_rec(pt):
    """affine point as unpacked from a table: canonical tight limbs of x R, y R"""
    return tight(mont(pt[0])) + tight(mont(pt[1]))


def check_vr(l, what, slack=27):
    v = val29(l)
    assert -(1 << 231) < v < (1 << 256) + (1 << 231), what + " not value-reduced: " + hex(v)
    assert all(-(1 << slack) - 8 < l[i] < (1 << 29) + (1 << slack) + 8 for i in range(8)), what + " limbs too loose"


def check_xyzz_form(out, zz_bound):
    if out[36]:
        return
    check_vr(out[:9], "X")
    check_vr(out[9:18], "Y")
    for k, nm in ((18, "ZZ"), (27, "ZZZ")):
        check_limbs(out[k:k + 9])
        assert abs(val29(out[k:k + 9])) < zz_bound * P, nm + " outside +-%d p" % zz_bound


def pair_cases(rng, n, mk):
    """(accumulator, addend) pairs: generic, P + P, P + (-P), infinity on either side, each with canonical and non-canonical coordinates"""
    pts = points()
    recs = []
    for a in pts[:24]:
        for nc in (0, 1, 2):
            recs += [mk(a, a, nc), mk(a, ec.pt_neg(a), nc), mk(a, pts[1], nc), mk(None, a, nc), mk(a, None, nc)]
    recs.append(mk(None, None, 0))
    for _ in range(n):
        a, b = rng.choice(pts), rng.choice(pts)
        k = rng.randrange(16)
        recs.append(mk(a, a if k == 0 else ec.pt_neg(a) if k == 1 else b, rng.choice((0, 0, 0, 1, 2))))
    return [r for r in recs if r is not None]


def gen_pt29_madd(rng, n):
    def mk(a, b, nc):
        if b is None:
            return None                              # the addend of a mixed addition is a table entry: never infinity
        neg = rng.randrange(2)
        return xyzz_of(rng, a, nc) + aff_rec(ec.pt_neg(b) if neg else b) + [neg]
    return pair_cases(rng, n, mk)


def rec_affine(rec):
    """the affine point an 18-limb x | y record holds"""
    return (val29(rec[:9]) * RINV_P % P, val29(rec[9:18]) * RINV_P % P)


def chk_pt29_madd(rec, out):
    a = affine_of_xyzz(rec[:37])
    q = rec_affine(rec[37:55])
    want = ec.pt_add(a, ec.pt_neg(q) if rec[55] else q)
    assert affine_of_xyzz(out) == want, "sum differs: want " + (hexs(want) if want else "infinity")
    if a is not None and want is not None and a != want:
        check_xyzz_form(out, 5 if q[0] != a[0] else 3)


def gen_pt29_add(rng, n):
    return pair_cases(rng, n, lambda a, b, nc: xyzz_of(rng, a, nc) + xyzz_of(rng, b, (nc * 2) % 3))


def chk_pt29_add(rec, out):
    a, b = affine_of_xyzz(rec[:37]), affine_of_xyzz(rec[37:])
    want = ec.pt_add(a, b)
    assert affine_of_xyzz(out) == want, "sum differs: want " + (hexs(want) if want else "infinity")
    if a is not None and b is not None and want is not None and a[0] != b[0]:
        check_xyzz_form(out, 5)


def gen_pt29_dbl(rng, n):
    pts = points()
    recs = [xyzz_of(rng, a, nc) for a in pts for nc in (0, 1, 2)] + [xyzz_of(rng, None)]
    return recs + [xyzz_of(rng, rng.choice(pts), rng.choice((0, 0, 1, 2))) for _ in range(n)]


def chk_pt29_dbl(rec, out):
    a = affine_of_xyzz(rec)
    assert affine_of_xyzz(out) == ec.pt_add(a, a), "not the double"
    if a is None:
        assert out == rec, "infinity must stay as it was"
    else:
        check_xyzz_form(out, 3)


def gen_pt29_mdbl(rng, n):
    pts = points()
    recs = []
    for a in pts:
        x, y = tight(mont(a[0])), tight(mont(a[1]))
        recs += [x + y, x + [-v for v in tight(mont(-a[1] % P))]]           # y as f29_cneg leaves it in the P == Q branch of pt29_madd
    return recs + [aff_rec(point_with_x_from(rng.randrange(P))) for _ in range(n)]


def chk_pt29_mdbl(rec, out):
    a = rec_affine(rec)
    assert affine_of_xyzz(out) == ec.pt_add(a, a), "not the double"
    check_xyzz_form(out, 3)


def jac_of(rng, pt, zform=0):
    """Jacobian X Y Z of the point with value-reduced coordinates; zform 1: Z carries a multiple of p within +-4 p (pt29_dbl_jacx)"""
    x, y = pt
    z = rng.randrange(1, P)
    Z = mont(z)
    return vr_forms(rng, mont(x * z * z)) + vr_forms(rng, mont(y * z * z * z)) + (fe_forms(rng, Z, -4, 3) if zform else vr_forms(rng, Z))


def affine_of_jac(l):
    X, Y, Z = (val29(l[9 * i:9 * i + 9]) * RINV_P % P for i in range(3))
    if Z == 0:
        return None
    zi = pow(Z, -1, P)
    return (X * zi * zi % P, Y * zi * zi * zi % P)


def gen_pt29_mdbl_a(rng, n):
    """the table builder's view: a Jacobian point (X : Y : Z) of P-256 is the affine point (X, Y) of the curve with a4 = -3 Z^4"""
    pts = points()
    recs = []
    for i in range(len(pts) + n):
        a = pts[i] if i < len(pts) else rng.choice(pts)
        j = jac_of(rng, a)
        z = val29(j[18:]) * RINV_P % P
        recs.append(j[:18] + vr_forms(rng, mont(-3 * pow(z, 4, P) % P)))
    return recs


def chk_pt29_mdbl_a(rec, out):
    # the affine doubling law on y^2 = x^3 + a4 x + b' (b' never enters), in big integers
    X, Y, a4 = (val29(rec[9 * i:9 * i + 9]) * RINV_P % P for i in range(3))
    lam = (3 * X * X + a4) * pow(2 * Y, -1, P) % P
    u3 = (lam * lam - 2 * X) % P
    assert affine_of_xyzz(out) == (u3, (lam * (X - u3) - Y) % P), "not the double on y^2 = x^3 + a4 x + b'"
    check_xyzz_form(out, 3)


def gen_pt29_dbl_jac(rng, n):
    pts = points()
    recs = [jac_of(rng, a) for a in pts for _ in range(3)]
    recs.append(vr_forms(rng, mont(5)) + vr_forms(rng, mont(7)) + tight(0))          # Z = 0 stays 0
    return recs + [jac_of(rng, rng.choice(pts)) for _ in range(n)]


def chk_jac_dbl(rec, out):
    a = affine_of_jac(rec[:27])
    got = affine_of_jac(out[:27])
    assert got == ec.pt_add(a, a), "not the double"
    for k, nm in ((0, "X"), (9, "Y"), (18, "Z")):
        check_vr(out[k:k + 9], nm)


def chk_pt29_dbl_jac(rec, out):
    chk_jac_dbl(rec, out)


def gen_pt29_dbl_jacx(rng, n):
    pts = points()
    recs = [jac_of(rng, a, 1) + [0] for a in pts for _ in range(3)] + [[0] * 27 + [1]]
    return recs + [jac_of(rng, rng.choice(pts), 1) + [0] for _ in range(n)]


def chk_pt29_dbl_jacx(rec, out):
    assert out[27] == rec[27], "the infinity flag must stay"
    if not rec[27]:
        chk_jac_dbl(rec, out)


def gen_pt29_madd_jacx(rng, n):
    def mk(a, b, nc):
        if b is None:
            return None
        neg = rng.randrange(2)
        acc = [0] * 27 + [1] if a is None else jac_of(rng, a, 1) + [0]
        return acc + aff_rec(ec.pt_neg(b) if neg else b) + [neg]
    return pair_cases(rng, n, mk)


def chk_pt29_madd_jacx(rec, out):
    a = None if rec[27] else affine_of_jac(rec[:27])
    q = rec_affine(rec[28:46])
    want = ec.pt_add(a, ec.pt_neg(q) if rec[46] else q)
    got = None if out[27] else affine_of_jac(out[:27])
    assert got == want, "sum differs: want " + (hexs(want) if want else "infinity")
    assert out[27] or val29(out[18:27]) % P != 0


def gen_apt29_add_with_inverse(rng, n):
    pts = points()
    recs = []
    for i in range(len(pts) * 2 + n):
        a, b = (pts[i // 2], pts[(i // 2 + 1 + i % 2) % len(pts)]) if i < 2 * len(pts) else (rng.choice(pts), rng.choice(pts))
        if a[0] == b[0]:
            b = ec.pt_add(a, a)                      # the builder's case: distinct x (a prime-order group: 2 a != +-a)
        dinv = mont(pow(b[0] - a[0], -1, P))
        recs.append(aff_rec(a) + aff_rec(b) + tight(dinv + rng.randrange(2) * P))
    return recs


def chk_apt29_add_with_inverse(rec, out):
    a, b = rec_affine(rec[:18]), rec_affine(rec[18:36])
    assert a[0] != b[0]
    assert rec_affine(out) == ec.pt_add(a, b), "sum differs"
    for k, nm in ((0, "x"), (9, "y")):
        v = val29(out[k:k + 9])
        assert -(1 << 229) < v < (1 << 256) + (1 << 229), nm + " outside (-2^229, 2^256 + 2^229)"


def gen_pt29_rx_matches(rng, n):
    pts = points()
    recs = []
    for i in range(len(pts) + n):
        a = pts[i] if i < len(pts) else rng.choice(pts)
        x = a[0]
        rs = [x % N, (x % N + 1) % N, (x % N - 1) % N, rng.randrange(N)]      # for x >= n, x % n = x - n: only the second comparison sees it
        if i < len(pts):
            for nc in (0, 1, 2):
                recs += [xyzz_of(rng, a, nc) + words(r) for r in rs]
        else:
            recs.append(xyzz_of(rng, a, rng.choice((0, 0, 1, 2))) + words(rs[0] if i & 1 else rng.choice(rs[1:])))
    recs += [xyzz_of(rng, None) + words(r) for r in (0, 1, N - 1)]
    return recs


def chk_pt29_rx_matches(rec, out):
    a = affine_of_xyzz(rec[:37])
    r = wval(rec[37:])
    assert out == [1 if a is not None and a[0] % N == r else 0]


# ---- Ed25519 (ed25519_fe.h, ed25519_core.h, sha512_dev.h) ---------------------------------------------------------------------------
POS25 = [(51 * i + 1) // 2 for i in range(10)]
W25 = [25 if i & 1 else 26 for i in range(10)]
TIGHT25 = [(1 << (w - 1)) + (1 << 19) for w in W25]          # what SBV_F25_CHECK calls 1 x tight
D25, SQRTM1 = ed.D, ed.SQRT_M1


def val25(l):
    return sum(v << POS25[i] for i, v in enumerate(l))


def canon25(v):
    """the limbs in [0, 2^w) of 0 <= v < 2^255 (fe25_from_words form: 2 x tight)"""
    return [(v >> POS25[i]) & ((1 << W25[i]) - 1) for i in range(10)]


def bal25(v):
    """a tight (balanced) representation of the residue v, as a carry pass leaves one"""
    l = canon25(v % P25)
    for _ in range(2):
        for i in range(10):
            if l[i] >= 1 << (W25[i] - 1):
                l[i] -= 1 << W25[i]
                if i < 9:
                    l[i + 1] += 1
                else:
                    l[0] += 19
    return l


def rand25(rng, mult):
    """limbs uniform within mult x tight"""
    return [rng.randrange(-mult * t, mult * t + 1) for t in TIGHT25]


def pats25(mult):
    lim = [mult * t for t in TIGHT25]
    pats = [lim, [-v for v in lim], [v if i & 1 else -v for i, v in enumerate(lim)], [-v if i & 1 else v for i, v in enumerate(lim)], [0] * 10]
    for i in range(10):
        pats += [[0] * i + [lim[i]] + [0] * (9 - i), [0] * i + [-lim[i]] + [0] * (9 - i)]
    return pats


F25_EDGE = [0, 1, 2, 19, P25 - 1, P25 - 2, (P25 - 1) // 2, (P25 + 1) // 2, 2**255 - 20, D25, SQRTM1, 2**128, 2**252, (1 << 255) % P25 + 5]


def operand25(rng, mult):
    k = rng.randrange(4)
    if k == 0:
        return rand25(rng, mult)
    if k == 1:
        return bal25(rng.randrange(P25))
    if k == 2:
        return canon25(rng.getrandbits(255)) if mult >= 2 else bal25(rng.choice(F25_EDGE))
    return rng.choice(pats25(mult))


def check_tight25(out):
    assert all(abs(out[i]) <= TIGHT25[i] for i in range(10)), "limbs not tight"


def gen_fe25_mul(rng, n):
    recs = [a + b for a in pats25(8) for b in pats25(3)[::2]] + [bal25(a) + bal25(b) for a in F25_EDGE for b in F25_EDGE]
    return recs + [operand25(rng, 8) + operand25(rng, 3) for _ in range(n)]


def chk_fe25_mul(rec, out):
    assert (val25(out) - val25(rec[:10]) * val25(rec[10:])) % P25 == 0, "value != a b (mod p)"
    check_tight25(out)


def gen_fe25_sqr(rng, n):
    return pats25(3) + [bal25(a) for a in F25_EDGE] + [operand25(rng, 3) for _ in range(n)]


def chk_fe25_sqr(rec, out):
    assert (val25(out) - val25(rec) ** 2) % P25 == 0, "value != a^2 (mod p)"
    check_tight25(out)


def gen_fe25_carry(rng, n):
    big = (1 << 31) - 1
    recs = [[big] * 10, [-big - 1] * 10, [big, -big - 1] * 5, [-big - 1, big] * 5] + pats25(8) + [canon25(a) for a in F25_EDGE]
    for i in range(10):
        recs += [[0] * i + [big] + [0] * (9 - i), [0] * i + [-big - 1] + [0] * (9 - i)]
    return recs + [[rng.randrange(-big - 1, big + 1) for _ in range(10)] for _ in range(n)]


def chk_fe25_carry(rec, out):
    assert (val25(out) - val25(rec)) % P25 == 0, "value changed (mod p)"
    check_tight25(out)


def gen_fe25_add(rng, n):
    return [a + b for a in pats25(8) for b in pats25(8)[::4]] + [operand25(rng, 8) + operand25(rng, 8) for _ in range(n)]


def chk_fe25_add(rec, out):
    assert out == [a + b for a, b in zip(rec[:10], rec[10:])]


gen_fe25_sub = gen_fe25_add


def chk_fe25_sub(rec, out):
    assert out == [a - b for a, b in zip(rec[:10], rec[10:])]


def gen_fe25_neg(rng, n):
    return pats25(8) + [operand25(rng, 8) for _ in range(n)]


def chk_fe25_neg(rec, out):
    assert out == [-a for a in rec]


def freeze_inputs(rng, n):
    recs = pats25(7) + [bal25(a) for a in F25_EDGE] + [canon25(a) for a in F25_EDGE]
    recs += [canon25(P25 + k) for k in range(19)] + [canon25(P25 - 1 - k) for k in range(4)]              # the non-canonical residues p .. 2^255 - 1
    recs += [[a + 7 * b for a, b in zip(bal25(P25 - 1 - k), bal25(0))] for k in range(2)]
    return recs + [operand25(rng, 7) for _ in range(n)]


gen_fe25_freeze = freeze_inputs


def chk_fe25_freeze(rec, out):
    assert wval(out) == val25(rec) % P25


def gen_fe25_from_words(rng, n):
    xs = F25_EDGE + [2**255 - 1, 2**256 - 1, 2**255, 2**255 + P25, P25, P25 + 1, 0xFFFFFFFF00000000FFFFFFFF00000000FFFFFFFF00000000FFFFFFFF00000000]
    return [words(x) for x in xs] + [words(rng.getrandbits(256)) for _ in range(n)]


def chk_fe25_from_words(rec, out):
    assert out == canon25(wval(rec) & ((1 << 255) - 1))


def gen_fe25_inv(rng, n):
    return pats25(1) + [bal25(a) for a in F25_EDGE] + [rand25(rng, 1) if rng.randrange(2) else bal25(rng.randrange(P25)) for _ in range(n)]


def chk_fe25_inv(rec, out):
    a = val25(rec) % P25
    assert val25(out) % P25 == (pow(a, -1, P25) if a else 0), "not the inverse"
    check_tight25(out)


gen_fe25_inv_gcd = gen_fe25_inv


def chk_fe25_inv_gcd(rec, out):
    a = val25(rec) % P25
    assert out == canon25(pow(a, -1, P25) if a else 0), "not the canonical limbs of the inverse"


gen_fe25_pow22523 = gen_fe25_inv


def chk_fe25_pow22523(rec, out):
    assert val25(out) % P25 == pow(val25(rec) % P25, (P25 - 5) // 8, P25)
    check_tight25(out)


gen_fe25_is_negative = freeze_inputs


def chk_fe25_is_negative(rec, out):
    assert out == [val25(rec) % P25 & 1]


_edpts = None


def ed_points():
    """multiples of B and the eight points of small order (affine x, y)"""
    global _edpts
    if _edpts is None:
        rng = random.Random(f"{SEED}:edpoints")
        def aff(p):
            zi = pow(p[2], -1, P25)
            return (p[0] * zi % P25, p[1] * zi % P25)
        ks = [1, 2, 3, 4, 7, 8, L25 - 1, L25 - 2, (L25 + 1) // 2] + [rng.randrange(1, L25) for _ in range(24)]
        _edpts = [aff(ed.pt_mul(k, ed.B)) for k in ks]
        # small order: (0, 1), (0, -1), (+-sqrt(-1), 0) and the four points of order 8
        small = [(0, 1), (0, P25 - 1), (SQRTM1, 0), (P25 - SQRTM1, 0)]
        e8 = ed.decompress(bytes.fromhex("26e8958fc2b227b045c3f489f2ef98f0d5dfac05d3c63339b13802886d53fc05"))
        if e8 is not None:                           # a point of order 8, so that every small order is covered
            assert aff(ed.pt_mul(8, e8)) == (0, 1) and aff(ed.pt_mul(4, e8)) != (0, 1)
            p8 = aff(e8)
            small += [p8, (P25 - p8[0], p8[1]), (p8[0], P25 - p8[1]), (P25 - p8[0], P25 - p8[1])]
        _edpts += small
        _edpts += [aff(ed.pt_add((q[0], q[1], 1, q[0] * q[1] % P25), ed.pt_mul(5, ed.B))) for q in small]       # mixed order
    return _edpts


def ed_ext(pt):
    return (pt[0], pt[1], 1, pt[0] * pt[1] % P25)


def ed_aff(p):
    zi = pow(p[2], -1, P25)
    return (p[0] * zi % P25, p[1] * zi % P25)


def ept_of(rng, pt, z=None):
    x, y = pt
    z = z if z is not None else rng.randrange(1, P25)
    return bal25(x * z) + bal25(y * z) + bal25(z) + bal25(x * y % P25 * z)


def affine_of_ept(l, need_t=True):
    X, Y, Z, T = (val25(l[10 * i:10 * i + 10]) % P25 for i in range(4))
    assert Z != 0, "Z = 0"
    if need_t:
        assert T * Z % P25 == X * Y % P25, "T Z != X Y"
    zi = pow(Z, -1, P25)
    return (X * zi % P25, Y * zi % P25)


def check_ept_tight(out):
    for i in range(4):
        check_tight25(out[10 * i:10 * i + 10])


def gen_ed_dbl(rng, n):
    pts = ed_points()
    return [ept_of(rng, a, z) for a in pts for z in (1, None, None)] + [ept_of(rng, rng.choice(pts)) for _ in range(n)]


def chk_ed_dbl(rec, out):
    a = affine_of_ept(rec)
    assert affine_of_ept(out) == ed_aff(ed.pt_add(ed_ext(a), ed_ext(a))), "not the double"
    check_ept_tight(out)


def ed_pairs(rng, n, mk):
    pts = ed_points()
    recs = []
    for a in pts:
        recs += [mk(a, a, 0, 0), mk(a, a, 1, 0), mk(a, pts[0], 0, 0), mk(a, pts[3], 1, 0), mk(a, pts[1], 0, 1), mk((0, 1), a, 0, 0), mk(a, (0, 1), 1, 0)]
    for _ in range(n):
        a, b = rng.choice(pts), rng.choice(pts)
        recs.append(mk(a, a if rng.randrange(16) == 0 else b, rng.randrange(2), 1 if rng.randrange(16) == 0 else 0))
    return recs


def gen_ed_add_pniels(rng, n):
    def mk(a, b, neg, skip):
        q = ept_of(rng, b)
        X, Y, Z, T = (q[10 * i:10 * i + 10] for i in range(4))
        t2d = bal25(val25(T) * 2 * D25)
        return ept_of(rng, a) + [y + x for x, y in zip(X, Y)] + [y - x for x, y in zip(X, Y)] + Z + t2d + [neg, skip]
    return ed_pairs(rng, n, mk)


def chk_ed_add(rec, out, b):
    a = affine_of_ept(rec[:40])
    neg, skip = rec[-2], rec[-1]
    if skip:
        assert out == rec[:40], "a skipped addition must leave the accumulator as it was"
        return
    bb = ed_ext(b)
    want = ed_aff(ed.pt_add(ed_ext(a), ed.pt_neg(bb) if neg else bb))
    assert affine_of_ept(out) == want, "sum differs"
    check_ept_tight(out)


def chk_ed_add_pniels(rec, out):
    ypx, ymx, z = (val25(rec[40 + 10 * i:50 + 10 * i]) % P25 for i in range(3))
    zi = pow(z, -1, P25)
    y, x = (ypx + ymx) * pow(2, -1, P25) * zi % P25, (ypx - ymx) * pow(2, -1, P25) * zi % P25
    assert val25(rec[70:80]) % P25 == 2 * D25 * x * y * z % P25
    chk_ed_add(rec, out, (x, y))


def gen_ed_add_aniels(rng, n):
    def mk(a, b, neg, skip):
        x, y = b
        return ept_of(rng, a) + canon25((y + x) % P25) + canon25((y - x) % P25) + canon25(2 * D25 * x * y % P25) + [neg, skip]
    return ed_pairs(rng, n, mk)


def chk_ed_add_aniels(rec, out):
    ypx, ymx = (val25(rec[40 + 10 * i:50 + 10 * i]) % P25 for i in range(2))
    chk_ed_add(rec, out, ((ypx - ymx) * pow(2, -1, P25) % P25, (ypx + ymx) * pow(2, -1, P25) % P25))


def gen_ed_decompress(rng, n):
    pts = ed_points()
    encs = [y | (sx << 255) for (x, y) in pts for sx in (0, 1)]
    encs += [(P25 + k) | (sx << 255) for k in range(19) for sx in (0, 1)]                  # non-canonical y >= p, accepted as y mod p
    encs += [1 | (1 << 255), (P25 - 1) | (1 << 255), 0, 1 << 255, 2, P25 - 2, 2**255 - 1, 2**256 - 1]   # x = 0 with the sign bit; small order
    encs += [rng.getrandbits(256) for _ in range(n // 2)]                                  # about half are non-squares
    pool = [ed.encode(ed.pt_mul(rng.randrange(1, L25), ed.B)) for _ in range(16)]
    encs += [int.from_bytes(rng.choice(pool), "little") ^ (rng.randrange(2) << 255) for _ in range(n - n // 2)]
    return [words(e) for e in encs]


def chk_ed_decompress(rec, out):
    want = ed.decompress(wval(rec).to_bytes(32, "little"))
    assert out[0] == (0 if want is None else 1), "verdict differs"
    if want is not None:
        assert affine_of_ept(out[1:]) == (want[0], want[1]), "point differs"
        check_ept_tight(out[1:])


def gen_ed_encoding_matches(rng, n):
    pts = ed_points()
    recs = []
    for a in pts + [rng.choice(pts) for _ in range(n)]:
        x, y = a
        e = y | ((x & 1) << 255)
        alts = [e, e ^ (1 << 255), e ^ 1, (e + 1) % (1 << 256), rng.getrandbits(256)]
        if y < 19:
            alts.append(e + P25)                     # the non-canonical encoding of the same point: byte for byte it differs
        r = ept_of(rng, a)
        recs += [r + words(v) for v in alts]
    return recs


def chk_ed_encoding_matches(rec, out):
    x, y = affine_of_ept(rec[:40])
    assert out == [1 if wval(rec[40:]) == y | ((x & 1) << 255) else 0]


def gen_mod_l_512(rng, n):
    xs = [0, 1, L25 - 1, L25, L25 + 1, 2 * L25, 2**252, 2**252 - 1, 2**253, 2**255, 2**256, 2**512 - 1, (L25 - 1) ** 2, L25 * L25, 2**511, L25 << 259,
          (L25 << 259) - 1, 2**412, 2**316, 2**384 - 1]
    xs += [rng.getrandbits(512) for _ in range(n)]
    return [words(x, 16) for x in xs]


def chk_mod_l_512(rec, out):
    assert wval(out) == wval(rec) % L25


SHA_LENS = [0, 47, 48, 111, 112, 175, 176, 1024, 1, 63, 64, 65, 127, 128, 239, 240, 1023]


def gen_sha512_ram(rng, n):
    recs = []
    for mlen in SHA_LENS + [rng.randrange(1025) for _ in range(n)]:
        data = rng.randbytes(64 + mlen) + bytes(1024 - mlen)
        recs.append([mlen] + list(np.frombuffer(data, dtype="<u4").astype(np.int64)))
    return recs


def chk_sha512_ram(rec, out):
    data = np.array(rec[1:], dtype=np.int64).astype("<u4").tobytes()[:64 + rec[0]]
    got = b"".join(((u(out[2 * i + 1]) << 32) | u(out[2 * i])).to_bytes(8, "big") for i in range(8))
    assert got == hashlib.sha512(data).digest()


# ---- the P-256 signer's helpers (sha256_dev.h, hmac_sha256_dev.h, p256_sign.h) -----------------------------------------------------
SHA256_LENS = [0, 1, 54, 55, 56, 57, 63, 64, 65, 118, 119, 120, 127, 128, 1023, 1024]


def gen_sha256_msg(rng, n):
    recs = []
    for mlen in SHA256_LENS + [rng.randrange(1025) for _ in range(n)]:
        data = rng.randbytes(mlen) + b"\xa5" * (1024 - mlen)          # what lies behind the message must not be hashed
        recs.append([mlen] + list(np.frombuffer(data, dtype="<u4").astype(np.int64)))
    return recs


def chk_sha256_msg(rec, out):
    data = np.array(rec[1:], dtype=np.int64).astype("<u4").tobytes()[:rec[0]]
    assert be_bytes(out) == hashlib.sha256(data).digest()


def be_words(b):
    """bytes -> big-endian word values, as the signer's lanes hold K, V, x and h"""
    return [int.from_bytes(b[i:i + 4], "big") for i in range(0, len(b), 4)]


def be_bytes(ws):
    return b"".join(u(w).to_bytes(4, "big") for w in ws)


def _mac256(key, data):
    return hmac.new(key, data, hashlib.sha256).digest()


HMAC_EDGE = [bytes(32), b"\xff" * 32]


def hmac_kv(rng, n):
    """(K, V): every pairing of the all-zero and all-0xFF strings, then n random ones"""
    return [(k, v) for k in HMAC_EDGE for v in HMAC_EDGE] + [(rng.randbytes(32), rng.randbytes(32)) for _ in range(n)]


def gen_hmac_v(rng, n):
    return [be_words(k) + be_words(v) for k, v in hmac_kv(rng, n)]


def chk_hmac_v(rec, out):
    assert be_bytes(out) == _mac256(be_bytes(rec[:8]), be_bytes(rec[8:16]))


def gen_hmac_v_tag(rng, n):
    """every edge (K, V) under tags 0, 1, 0xFF and both shapes; the random ones draw a tag and a shape.  With tail_only set, x and h
    hold garbage that must not be read."""
    recs = []
    kvs = hmac_kv(rng, n)
    for i, (k, v) in enumerate(kvs):
        for tag, tail in ([(t, s) for t in (0, 1, 0xFF) for s in (0, 1)] if i < 4 else [(rng.choice([0, 1, 0xFF]), rng.randrange(2))]):
            x, h = (rng.choice(HMAC_EDGE + [rng.randbytes(32)]) for _ in range(2))
            recs.append(be_words(k) + be_words(v) + [tag] + be_words(x) + be_words(h) + [tail])
    return recs


def chk_hmac_v_tag(rec, out):
    msg = be_bytes(rec[8:16]) + bytes([rec[16]])
    if not rec[33]:
        msg += be_bytes(rec[17:33])
    assert be_bytes(out) == _mac256(be_bytes(rec[:8]), msg)


SIGN_EDGE_KEYS = [1, 2, N - 2, N - 1]


def gen_sign29_finish(rng, n):
    """x | d | k | e, plain integers: x < p, d and k in [1, N-1], e < N.  x around N (x = N gives r = 0), a triple with
    e + r d = 0 mod N (s = 0) and its neighbour e + 1, e = N - 1 with r d = N - 1 (the lazily added e + r d at its largest), the edge
    keys as d and k under e of {0, 1, N-1}, 200 seeded cases, then n random ones"""
    quads = [(x, rng.randrange(1, N), rng.randrange(1, N), rng.randrange(N)) for x in (1, N - 1, N, N + 1, P - 1)]
    for x in (rng.randrange(1, N), rng.randrange(N + 1, P)):                # r = x and r = x - N
        r, d, k = x % N, rng.randrange(1, N), rng.randrange(1, N)
        e0 = (N - r * d % N) % N
        quads += [(x, d, k, e0), (x, d, k, (e0 + 1) % N)]
        quads.append((x, (N - 1) * pow(r, -1, N) % N, k, N - 1))                # r d = N - 1 and e = N - 1
    quads += [(rng.randrange(1, P), d, k, e) for d in SIGN_EDGE_KEYS for k in SIGN_EDGE_KEYS for e in (0, 1, N - 1)]
    seeded = random.Random(0x29F1)
    quads += [(seeded.randrange(1, P), seeded.randrange(1, N), seeded.randrange(1, N), seeded.randrange(N)) for _ in range(200)]
    quads += [(rng.randrange(1, P), rng.randrange(1, N), rng.randrange(1, N), rng.randrange(N)) for _ in range(n)]
    return [words(x) + words(d) + words(k) + words(e) for x, d, k, e in quads]


def chk_sign29_finish(rec, out):
    x, d, k, e = (wval(rec[8 * i:8 * i + 8]) for i in range(4))
    want = sign_cases.finish(x, d, k, e)
    if want is None:
        assert x == N or (e + x % N * d) % N == 0, "the reference refuses a case that has r != 0 and s != 0"
        assert [u(v) for v in out] == [0] * 17, "a refused case must answer all zero"
    else:
        assert (wval(out[:8]), wval(out[8:16]), u(out[16])) == (want[0], want[1], 1)


# ---- secp256k1 (k256_fe.h, k256_sc.h, k256_core.h) ---------------------------------------------------------------------------------
K_TOP_LO, K_TOP_HI = -(1 << 20), (1 << 24) + (1 << 20)          # limb 8 of a reduced value


def kred(rng, v):
    """a reduced representation of the residue v: the canonical one, or v +- p where limb 8 allows it"""
    v %= KP
    forms = [v]
    if (v + KP) >> 232 <= K_TOP_HI:
        forms.append(v + KP)
    if (v - KP) >> 232 >= K_TOP_LO:
        forms.append(v - KP)
    return tight(rng.choice(forms))


def krand(rng):
    """any reduced limbs"""
    x = rng.getrandbits(232)
    return [(x >> (29 * i)) & M29 for i in range(8)] + [rng.randrange(K_TOP_LO, K_TOP_HI + 1)]


K_EDGE = [v % KP for v in edge_values(KP)] + [KP - 977, 977, 2**32 + 977, KP - 2**32]
K_RED_PATS = [[M29] * 8 + [K_TOP_HI], [0] * 8 + [K_TOP_LO], [M29] * 8 + [K_TOP_LO], [0] * 8 + [K_TOP_HI], [0] * 9, tight(KP), [M29, 0] * 4 + [1 << 24],
              [0x1FFFFC2F] + [0] * 8, [977] + [0] * 8]
K_RAW_PATS = [[M29] * 8 + [K_TOP_HI], [-M29] * 8 + [-K_TOP_HI], [M29, -M29] * 4 + [2**24], [-M29, M29] * 4 + [-(2**20)], [0] * 8 + [K_TOP_HI], [M29] * 9,
              [-M29] * 9, [1] + [0] * 8, [0] * 9]
K_WIDE = [[3 * M29] * 8 + [3 * 2**24], [-3 * M29, 3 * M29] * 4 + [2**25]]


def kop(rng):
    k = rng.randrange(4)
    return krand(rng) if k == 0 else kred(rng, rng.randrange(KP)) if k == 1 else kred(rng, rng.choice(K_EDGE)) if k == 2 else rng.choice(K_RED_PATS)


def kdiff(rng):
    return [a - b for a, b in zip(kop(rng), kop(rng))]


def check_kred(out):
    check_limbs(out)
    assert K_TOP_LO <= out[8] <= K_TOP_HI, "limb 8 outside the reduced range"


def gen_kfe_mul(rng, n):
    recs = [a + b for a in K_RAW_PATS + K_RED_PATS for b in K_RAW_PATS[::3] + K_WIDE + K_RED_PATS[::2]]
    recs += [tight(a) + tight(b) for a in K_EDGE for b in K_EDGE[::3]]
    for _ in range(n):
        k = rng.randrange(3)
        recs.append(kop(rng) + kop(rng) if k == 0 else kdiff(rng) + kdiff(rng) if k == 1 else [3 * v for v in kop(rng)] + kop(rng))
    return recs


def chk_kfe_mul(rec, out):
    assert (val29(out) - val29(rec[:9]) * val29(rec[9:])) % KP == 0, "value != a b (mod p)"
    check_kred(out)


def gen_kfe_sqr(rng, n):
    return K_RAW_PATS + K_RED_PATS + [tight(a) for a in K_EDGE] + [kop(rng) if rng.randrange(2) else kdiff(rng) for _ in range(n)]


def chk_kfe_sqr(rec, out):
    assert (val29(out) - val29(rec) ** 2) % KP == 0, "value != a^2 (mod p)"
    check_kred(out)


def kpairs(rng, n):
    return [a + b for a in K_RED_PATS for b in K_RED_PATS] + [tight(a) + tight(b) for a in K_EDGE for b in K_EDGE[::3]] + [kop(rng) + kop(rng) for _ in range(n)]


gen_kfe_add = gen_kfe_sub = kpairs


def chk_kfe_add(rec, out):
    assert (val29(out) - val29(rec[:9]) - val29(rec[9:])) % KP == 0
    check_kred(out)


def chk_kfe_sub(rec, out):
    assert (val29(out) - val29(rec[:9]) + val29(rec[9:])) % KP == 0
    check_kred(out)


def gen_kfe_lin(rng, n):
    recs = [a + b + [k, m] for a in K_RED_PATS for b in K_RED_PATS[::2] for k, m in ((1, 8), (4, 1), (3, 8), (16, 16), (0, 16), (16, 0))]
    return recs + [kop(rng) + kop(rng) + [rng.randrange(17), rng.randrange(17)] for _ in range(n)]


def chk_kfe_lin(rec, out):
    assert (val29(out) - val29(rec[:9]) * rec[18] + val29(rec[9:18]) * rec[19]) % KP == 0
    check_kred(out)


def gen_kfe_lin3(rng, n):
    recs = [a + b + c + [kb, kc] for a in K_RED_PATS[::2] for b in K_RED_PATS[::2] for c in K_RED_PATS[::3] for kb, kc in ((1, 2), (8, 8), (0, 0))]
    return recs + [kop(rng) + kop(rng) + kop(rng) + [rng.randrange(9), rng.randrange(9)] for _ in range(n)]


def chk_kfe_lin3(rec, out):
    assert (val29(out) - val29(rec[:9]) + val29(rec[9:18]) * rec[27] + val29(rec[18:27]) * rec[28]) % KP == 0
    check_kred(out)


def gen_kfe_cneg(rng, n):
    return [a + [s] for a in K_RED_PATS + [tight(v) for v in K_EDGE] for s in (0, 1)] + [kop(rng) + [rng.randrange(2)] for _ in range(n)]


def chk_kfe_cneg(rec, out):
    assert (val29(out) - (-val29(rec[:9]) if rec[9] else val29(rec[:9]))) % KP == 0
    check_kred(out)


def ksingles(rng, n):
    return K_RED_PATS + [tight(v) for v in K_EDGE] + [kred(rng, k * KP) for k in (0, 1, 0, 1)] + [kop(rng) for _ in range(n)]


gen_kfe_inv = gen_kfe_is_zero = gen_kfe_maybe_zero = gen_kfe_to_words = ksingles


def chk_kfe_inv(rec, out):
    a = val29(rec) % KP
    assert val29(out) % KP == (pow(a, -1, KP) if a else 0), "not the inverse"
    check_kred(out)


def chk_kfe_is_zero(rec, out):
    assert out == [1 if val29(rec) % KP == 0 else 0]


def chk_kfe_maybe_zero(rec, out):
    assert out == [1 if rec[0] in (0, 0x1FFFFC2F) else 0]
    assert out == [1] or val29(rec) % KP != 0


def chk_kfe_to_words(rec, out):
    assert wval(out) == val29(rec) % KP


def gen_kfe_equal(rng, n):
    recs = []
    for i in range(len(K_EDGE) + n):
        v = K_EDGE[i] if i < len(K_EDGE) else rng.randrange(KP)
        recs += [kred(rng, v) + kred(rng, v), kred(rng, v) + kred(rng, v + rng.choice((1, -1, 977, 1 << 29, 1 << 232)))]
    return recs


def chk_kfe_equal(rec, out):
    assert out == [1 if (val29(rec[:9]) - val29(rec[9:])) % KP == 0 else 0]


def gen_kfe_from_words(rng, n):
    return [words(v) for v in K_EDGE + [KP, KP + 1, 2**256 - 1, 2**255]] + [words(rng.getrandbits(256)) for _ in range(n)]


def chk_kfe_from_words(rec, out):
    x = wval(rec)
    assert out == [(x >> (29 * i)) & M29 for i in range(8)] + [x >> 232]


KSC_EDGE = [v % KN for v in edge_values(KN)] + [LAMBDA, KN - LAMBDA]


def gen_ksc_mul(rng, n):
    return [words(a) + words(b) for a in KSC_EDGE for b in KSC_EDGE[::2]] + [words(rng.randrange(KN)) + words(rng.randrange(KN)) for _ in range(n)]


def chk_ksc_mul(rec, out):
    assert wval(out) == wval(rec[:8]) * wval(rec[8:]) % KN


def gen_ksc_inv(rng, n):
    return [words(a) for a in KSC_EDGE] + [words(rng.randrange(KN)) for _ in range(n)]


def chk_ksc_inv(rec, out):
    a = wval(rec)
    assert wval(out) == (pow(a, -1, KN) if a else 0)


def gen_ksc_reduce512(rng, n):
    xs = [0, 1, KN, KN - 1, KN + 1, 2**256, 2**256 - 1, 2**512 - 1, (KN - 1) ** 2, KN * KN, 2**511, 2**385 - 1, 2**385, (2**256 - 1) ** 2, KN << 256, (KN << 256) - 1]
    return [words(x, 16) for x in xs] + [words(rng.getrandbits(512), 16) for _ in range(n)]


def chk_ksc_reduce512(rec, out):
    assert wval(out) == wval(rec) % KN


_glv = None


def glv_edge_scalars():
    global _glv
    if _glv is None:
        _glv = _glv_edge_scalars()
    return _glv


def _glv_edge_scalars():
    """the edge list of tests/test_k256_cpu.py::test_glv_decomposition_of_scalars, lattice vectors re-derived from (n, lambda)"""
    import math
    r0, r1, t0, t1, rows = KN, LAMBDA, 0, 1, []
    while r1:
        q = r0 // r1
        r0, r1, t0, t1 = r1, r0 - q * r1, t1, t0 - q * t1
        rows.append((r0, t0))
    i = next(i for i, (r, _) in enumerate(rows) if r < math.isqrt(KN))
    a1, b1 = rows[i][0], -rows[i][1]
    a2, b2 = min([(rows[i - 1][0], -rows[i - 1][1]), (rows[i + 1][0], -rows[i + 1][1])], key=lambda v: v[0] ** 2 + v[1] ** 2)
    n = KN
    ks = [0, 1, 2, n - 1, n, n + 1, 2**256 - 1, LAMBDA, n - LAMBDA, LAMBDA + 1, (n + 1) // 2, n // 2, a1, a2, abs(b1), abs(b2), 2**128, 2**128 - 1, 2**255]
    # The rounding carry of ksc_mul_shift384: scalars whose product k g has bit 383 set and bits 384..415 all ones, so that the
    # + 2^383 ripples through word 12 into word 13 (and, for the last ones, through words 12 and 13 into word 14).  Random scalars
    # meet this with probability 2^-33 per product.  g1, g2 = round(2^384 b2 / n), round(2^384 (-b1) / n) as k256_sc.h derives them.
    rng = random.Random(f"{SEED}:glv-carry")
    for g in ((2**384 * b2 + n // 2) // n, (2**384 * (-b1) + n // 2) // n):
        for ones in (32, 64):
            for _ in range(4):
                while True:
                    t = rng.getrandbits(90 - (ones - 32))
                    target = (t << (384 + ones)) + (((1 << ones) - 1) << 384) + (1 << 383)
                    k = -(-target // g)
                    if k < n and (k * g) >> 383 & ((1 << (ones + 1)) - 1) == (1 << (ones + 1)) - 1:
                        break
                ks.append(k)
    return ks


def gen_ksc_split_lambda(rng, n):
    return [words(k) for k in glv_edge_scalars()] + [words(rng.randrange(KN)) for _ in range(n)]


def chk_ksc_split_lambda(rec, out):
    k = wval(rec)
    k1, k2 = wval(out[:8]), wval(out[8:16])
    assert out[16] in (0, 1) and out[17] in (0, 1)
    assert ((-k1 if out[16] else k1) + (-k2 if out[17] else k2) * LAMBDA - k) % KN == 0, "k != +-k1 +- k2 lambda (mod n)"
    assert k1 < 1 << 128 and k2 < 1 << 128, "a half wider than 128 bits"


def split_lambda_bulk(lib, backend, n_random, seed=SEED):
    """ksc_split_lambda on n_random scalars (the edge scalars first, random ones for the rest), packed with numpy; returns (generated, checked, widest half in bits)"""
    rng = random.Random(f"{seed}:split_lambda_bulk")
    edge = glv_edge_scalars()
    n_random -= len(edge)                               # a launch holds at most 2^20 cases, the edge scalars included
    raw = b"".join(k.to_bytes(32, "little") for k in edge) + rng.randbytes(32 * n_random)
    n = len(edge) + n_random
    buf = np.frombuffer(raw, dtype="<u4").reshape(n, 8).copy()
    out = np.empty((n, 18), dtype=np.uint32)
    rc = lib.sbvd_run(backend, lib.ops["ksc_split_lambda"][0], buf.ctypes.data, out.ctypes.data, n)
    if rc != 0:
        raise HipError(f"sbvd_run(ksc_split_lambda, backend {backend}, {n} cases) returned {rc}")
    halves = out[:, :16].astype("<u4").tobytes()
    flags = out[:, 16:].tolist()
    worst = checked = 0
    for i in range(n):
        k = int.from_bytes(raw[32 * i:32 * i + 32], "little")
        k1 = int.from_bytes(halves[64 * i:64 * i + 32], "little")
        k2 = int.from_bytes(halves[64 * i + 32:64 * i + 64], "little")
        f1, f2 = flags[i]
        ok = f1 in (0, 1) and f2 in (0, 1) and ((-k1 if f1 else k1) + (-k2 if f2 else k2) * LAMBDA - k) % KN == 0 and k1 >> 128 == 0 and k2 >> 128 == 0
        assert ok, f"ksc_split_lambda (backend {backend}) case {i}: k = {hex(k)}, k1 = {hex(k1)} (neg {f1}), k2 = {hex(k2)} (neg {f2})"
        worst = max(worst, k1.bit_length(), k2.bit_length())
        checked += 1
    return n, checked, worst


_kpts = None


def kpoints():
    global _kpts
    if _kpts is None:
        rng = random.Random(f"{SEED}:kpoints")
        g = (kc.GX, kc.GY)
        ks = [1, 2, 3, 4, 7, 8, KN - 1, KN - 2, (KN + 1) // 2, LAMBDA] + [rng.randrange(1, KN) for _ in range(30)]
        _kpts = [kc.pt_mul(k, g) for k in ks]
    return _kpts


def kjac_of(rng, pt):
    if pt is None:
        return kop(rng) + kop(rng) + kop(rng) + [1]           # inf is authoritative: the coordinates are then arbitrary
    z = rng.randrange(1, KP)
    return kred(rng, pt[0] * z * z) + kred(rng, pt[1] * z * z * z) + kred(rng, z) + [0]


def affine_of_kjac(l):
    if l[27]:
        return None
    X, Y, Z = (val29(l[9 * i:9 * i + 9]) % KP for i in range(3))
    assert Z != 0, "finite point with Z = 0"
    zi = pow(Z, -1, KP)
    return (X * zi * zi % KP, Y * zi * zi * zi % KP)


def check_kjac_form(out):
    for i in range(3):
        check_kred(out[9 * i:9 * i + 9])


def gen_kpt_dbl(rng, n):
    pts = kpoints()
    return [kjac_of(rng, a) for a in pts for _ in range(3)] + [kjac_of(rng, None)] + [kjac_of(rng, rng.choice(pts)) for _ in range(n)]


def chk_kpt_dbl(rec, out):
    assert out[27] == rec[27], "the infinity flag must be copied"
    if not rec[27]:
        a = affine_of_kjac(rec)
        assert affine_of_kjac(out) == kc.pt_add(a, a), "not the double"
    check_kjac_form(out)


def gen_kpt_madd(rng, n):
    pts = kpoints()
    recs = []

    def mk(a, b, neg, skip):
        bb = kc.pt_neg(b) if neg else b
        return kjac_of(rng, a) + kred(rng, bb[0]) + kred(rng, bb[1]) + [neg, skip]
    for a in pts[:20]:
        for neg in (0, 1):
            recs += [mk(a, a, neg, 0), mk(a, kc.pt_neg(a), neg, 0), mk(a, pts[2], neg, 0), mk(None, a, neg, 0), mk(a, pts[3], neg, 1), mk(None, a, neg, 1)]
    for _ in range(n):
        a, b = rng.choice(pts), rng.choice(pts)
        k = rng.randrange(16)
        recs.append(mk(None if k == 3 else a, a if k == 0 else kc.pt_neg(a) if k == 1 else b, rng.randrange(2), 1 if k == 2 else 0))
    return recs


def chk_kpt_madd(rec, out):
    a = affine_of_kjac(rec[:28])
    q = (val29(rec[28:37]) % KP, val29(rec[37:46]) % KP)
    neg, skip = rec[46], rec[47]
    if skip:
        assert out == rec[:28], "a skipped addition must return the accumulator as it was"
        return
    want = kc.pt_add(a, kc.pt_neg(q) if neg else q)
    assert affine_of_kjac(out) == want, "sum differs: want " + (hexs(want) if want else "infinity")
    check_kjac_form(out)


def gen_k256_on_curve(rng, n):
    pts = kpoints()
    recs = []
    for a in pts + [rng.choice(pts) for _ in range(n)]:
        x, y = a
        recs += [kred(rng, x) + kred(rng, y), kred(rng, x) + kred(rng, -y), kred(rng, x + 1) + kred(rng, y), kred(rng, x) + kred(rng, y + rng.choice((1, 977, 1 << 200))),
                 kred(rng, rng.randrange(KP)) + kred(rng, rng.randrange(KP))]
    recs += [tight(0) + tight(0), kred(rng, 0) + kred(rng, pow(7, (KP + 1) // 4, KP))]
    return recs


def chk_k256_on_curve(rec, out):
    x, y = val29(rec[:9]) % KP, val29(rec[9:]) % KP
    assert out == [1 if (y * y - x * x * x - 7) % KP == 0 else 0]


# ---- cross-lane ops (device only): the quad chains through DPP and the __shfl_xor sum -------------------------------------------------
CHAIN_NS = [0, 1, 2, 3, 4, 8, 33, 128, 256]


def chain_counts(rng, quads):
    """doublings per quad: the fixed list first, then 1..64; neighbouring quads of a wavefront get different counts"""
    return [CHAIN_NS[q] if q < len(CHAIN_NS) else rng.randrange(1, 65) for q in range(quads)]


def run_chain(lib, name, quads, seed=SEED):
    """one launch of a quad chain: quad q doubles ITS point n_q times (16 quads per wavefront, every quad another point and count).
    Every lane's result is checked (a neighbour's point must not leak in) and the four lanes of a quad must agree bit for bit."""
    assert quads % 16 == 0
    rng = random.Random(f"{seed}:{name}")
    ns = chain_counts(rng, quads)
    recs, wants = [], []
    for q in range(quads):
        if name == "x_keychain29":
            pt = points()[q % len(points())] if q < 64 else ec.pt_mul(rng.randrange(1, N), ec.G)
            rec = aff_rec(pt) + [ns[q]]
            wants.append(ec.pt_mul(pow(2, ns[q], N), pt))
        elif name == "x_k256chain":
            pt = kpoints()[q % len(kpoints())]
            rec = kred(rng, pt[0]) + kred(rng, pt[1]) + [ns[q]]
            wants.append(kc.pt_mul(pow(2, ns[q], KN), pt))
        else:
            pt = ed_points()[q % len(ed_points())]
            rec = ept_of(rng, pt, 1 if q & 1 else None) + [ns[q]]
            wants.append(ed_aff(ed.pt_mul(1 << ns[q], ed_ext(pt))))
        recs += [rec] * 4
    outs = launch(lib, 1, name, recs)
    checked = 0
    for lane, out in enumerate(outs):
        q = lane >> 2
        try:
            assert out == outs[4 * q], "the lanes of the quad disagree"
            if name == "x_keychain29":
                got = affine_of_jac(out[:27])
                z = val29(out[18:27]) * RINV_P % P
                assert got == wants[q], "not 2^n P"
                assert val29(out[27:]) * RINV_P % P == -3 * pow(z, 4, P) % P, "T != -3 Z^4"
            elif name == "x_k256chain":
                assert affine_of_kjac(out + [0]) == wants[q], "not 2^n P"
                if ns[q]:
                    check_kjac_form(out)
            else:
                assert affine_of_ept(out) == wants[q], "not 2^n P"
                if ns[q]:
                    check_ept_tight(out)
        except AssertionError as e:
            raise AssertionError(f"{name} lane {lane} (quad {q}, {ns[q]} doublings): {e}\n  in  = {hexs(recs[lane])}\n  out = {hexs(out)}") from None
        checked += 1
    return len(recs), checked


def run_shfl_sum(lib, lanes, groups=16, seed=SEED):
    """the butterfly of the cooperative kernels: groups of `lanes` lanes, lane i holds k_i P (some lanes infinity, some equal, some
    opposite, so that the tree doubles and cancels inside); afterwards EVERY lane of the group holds the sum"""
    assert (groups * lanes) % 64 == 0
    rng = random.Random(f"{seed}:x_shfl_sum:{lanes}")
    recs, wants = [], []
    for g in range(groups):
        pt = points()[g % len(points())]
        ks = [rng.randrange(1, 1 << 16) for _ in range(lanes)]
        shape = g % 6
        if shape == 1:
            ks[1] = ks[0]                                        # equal neighbours: a doubling at the first level
        elif shape == 2:
            ks[1] = -ks[0]                                       # opposite neighbours: infinity at the first level
        elif shape == 3:
            ks[rng.randrange(lanes)] = 0                         # a lane at infinity
        elif shape == 4:
            ks = [0] * lanes                                     # all at infinity
        elif shape == 5 and lanes >= 4:
            ks[2], ks[3] = ks[1], ks[0]                          # equal partial sums: a doubling at the second level
        wants.append(ec.pt_mul(sum(ks) % N, pt) if sum(ks) % N else None)
        for k in ks:
            recs.append(xyzz_of(rng, ec.pt_mul(k % N, pt) if k % N else None, rng.choice((0, 0, 1, 2))) + [lanes])
    outs = launch(lib, 1, "x_shfl_sum", recs)
    checked = 0
    for lane, out in enumerate(outs):
        g = lane // lanes
        try:
            assert affine_of_xyzz(out) == wants[g], "not the sum of the group's lanes: want " + (hexs(wants[g]) if wants[g] else "infinity")
        except AssertionError as e:
            raise AssertionError(f"x_shfl_sum lane {lane} (group {g} of {lanes} lanes): {e}\n  in  = {hexs(recs[lane])}\n  out = {hexs(out)}") from None
        checked += 1
    return len(recs), checked


CROSS_LANE = ["x_keychain29", "x_edchain", "x_k256chain", "x_shfl_sum"]

# SLOW: ops whose case (kernel or big-integer reference) costs a modular inversion or a group operation
SLOW = {"f29_inv", "f29_inv_ct", "s29_inv", "s29_inv_ct", "sc_inv", "sc_inv_gcd", "fe_inv_gcd", "modinv30", "modinv30_ct",
        "pt29_dbl", "pt29_madd", "pt29_add", "pt29_mdbl", "pt29_mdbl_a", "pt29_dbl_jac", "pt29_dbl_jacx", "pt29_madd_jacx",
        "apt29_add_with_inverse", "pt29_rx_matches", "fe25_inv", "fe25_inv_gcd", "fe25_pow22523", "ed_dbl", "ed_add_pniels",
        "ed_add_aniels", "ed_decompress", "ed_encoding_matches", "sha512_ram", "sha256_msg", "sign29_finish", "kfe_inv", "ksc_inv", "kpt_dbl", "kpt_madd", "k256_on_curve"}

GEN = {k[4:]: v for k, v in list(globals().items()) if k.startswith("gen_") and callable(v)}
CHK = {k[4:]: v for k, v in list(globals().items()) if k.startswith("chk_") and callable(v)}

# random cases per op and backend (1 = gfx950 kernel, 0 = host loop: a sixteenth).  The big-integer check, not the kernel, is the cost
# (20 - 60 us per case with its generation), so the counts are what keeps the GPU file inside its share of the tier's time.
N_RANDOM = {1: {"cheap": 1 << 16, "slow": 1 << 12}, 0: {"cheap": 1 << 12, "slow": 1 << 8}}
N_SPLIT_LAMBDA = {1: 1 << 20, 0: 1 << 16}


def n_random(name, backend):
    return N_RANDOM[backend]["slow" if name in SLOW else "cheap"]
