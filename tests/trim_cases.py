"""Case generators and big-integer references for the unit ops of tools/devunit_trim.hip: the 32-bit canonical form of a table
store (f29_canon32), the affine + affine and the x-only mixed additions (pt29_mmadd, pt29_madd_x) and the comb walkers that use
them at their two ends (gphase29_point from infinity, qphase29_point in front of the x comparison).

Shared by the CPU tier (tests/test_emul_trim.py: a g++ build with the contract assertions on, backend 0) and the GPU tier
(tests/test_gpu_trim.py: the gfx950 build, backend 1).  Same conventions as tests/arith_cases.py, whose helpers are used: a
generator returns records of Python ints inside the op's documented contract, a checker compares an output with Python big
integers and, where the op has a longer twin, with the twin's output of the same lane."""
import random

import numpy as np

import arith_cases as ac
from arith_cases import M29, N, P, ec, tight, val29, words

LIM = 1 << 30                         # f29_canon32's contract: every limb in [-2^30, 2^30)
WINDOWS, PER_WINDOW = 33, 128         # a key's 8-bit comb (SBV_GTAB_WINDOWS x SBV_GTAB_PER_WINDOW)
OFFSET = sum(1 << (8 * j + 7) for j in range(WINDOWS))


def in_canon32_contract(l):
    return all(-LIM <= v < LIM for v in l)


# ---- f29_canon32 ---------------------------------------------------------------------------------------------------------------
def canon32_edges(rng):
    recs = []
    for k in range(-66, 67):                                  # |k| <= 64 fits the contract; the filter below drops the rest
        for base in (k * P, k << 256):
            for d in (-2, -1, 0, 1, 2):
                recs.append(tight(base + d))                                   # tight form
                recs.append(ac.spread(rng, base + d, 1))                       # loose form: borrows of +-2^29 between neighbours
    recs = [r for r in recs if in_canon32_contract(r)]
    lo, hi = -LIM, LIM - 1
    recs += [[lo] * 9, [hi] * 9, [lo, hi] * 4 + [lo], [hi, lo] * 4 + [hi], [0] * 9]
    for i in range(9):
        recs += [[0] * i + [lo] + [0] * (8 - i), [0] * i + [hi] + [0] * (8 - i), [hi] * i + [lo] + [hi] * (8 - i), [lo] * i + [hi] + [lo] * (8 - i)]
    return recs


def canon32_mul_output(rng):
    """what f29_mul / f29_sqr return: limbs 0..7 exact, value within (-2p, 3p)"""
    return tight(rng.randrange(-2 * P + 1, 3 * P))


def canon32_norm_red_output(rng):
    """what f29_norm_red returns: limbs 0..7 within 2^25 + 8 of [0, 2^29), value within (-2^229, 2^256 + 2^229)"""
    s = (1 << 25) + 7
    return [rng.randrange(-s, (1 << 29) + s + 1) for _ in range(8)] + [rng.randrange(0, 1 << 24)]


def gen_canon32(rng, n):
    """edges, then n of each class, then n over the whole contract"""
    recs = canon32_edges(rng)
    recs += [canon32_mul_output(rng) for _ in range(n)]
    recs += [canon32_norm_red_output(rng) for _ in range(n)]
    recs += [[rng.randrange(-LIM, LIM) for _ in range(9)] for _ in range(n)]
    return recs


def chk_canon32(rec, out):
    want = (val29(rec) % P)
    want = [(want >> (29 * i)) & M29 for i in range(9)]
    assert out[:9] == want, "f29_canon32: not the canonical limbs of the value"
    assert out[9:18] == want, "f29_canon differs"


# ---- points ----------------------------------------------------------------------------------------------------------------------
def padd(a, b):
    """affine addition on plain integers (None = infinity)"""
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        lam = (3 * a[0] * a[0] + ec.A) * pow(2 * a[1], -1, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return (x, (lam * (a[0] - x) - a[1]) % P)


_pool = None


def point_pool():
    """arith_cases' pool of group elements plus 200 sums of its members"""
    global _pool
    if _pool is None:
        rng = random.Random(f"{ac.SEED}:trim-pool")
        pts = list(ac.points())
        for _ in range(200):
            s = padd(rng.choice(pts), rng.choice(pts))
            if s is not None:
                pts.append(s)
        _pool = pts
    return _pool


def vr_point(rng, pt):
    """x1 | y1 as an accumulator of pt29_madd holds them: value-reduced forms of the Montgomery residues"""
    return ac.vr_forms(rng, ac.mont(pt[0])) + ac.vr_forms(rng, ac.mont(pt[1]))


def gen_mmadd(rng, n):
    pts = point_pool()
    recs = []
    for a in pts[:32]:
        for neg in (0, 1):
            recs.append(vr_point(rng, a) + ac.aff_rec(a) + [neg])                   # q = +(x1, y1): doubling, or infinity when negated
            recs.append(vr_point(rng, a) + ac.aff_rec(ec.pt_neg(a)) + [neg])        # q = -(x1, y1)
    for _ in range(n):
        a, b = rng.choice(pts), rng.choice(pts)
        recs.append(vr_point(rng, a) + ac.aff_rec(b) + [rng.randrange(2)])
    return recs


def chk_mmadd(rec, out):
    a = ac.rec_affine(rec[:18])
    q = ac.rec_affine(rec[18:36])
    want = padd(a, ec.pt_neg(q) if rec[36] else q)
    assert want == ec.pt_add(a, ec.pt_neg(q) if rec[36] else q)
    assert ac.affine_of_xyzz(out[:37]) == want, "pt29_mmadd: sum differs from the big-integer sum"
    assert ac.affine_of_xyzz(out[37:74]) == want, "pt29_madd on (x1, y1, 1, 1) differs from the big-integer sum"
    if want is not None and a[0] != q[0]:
        ac.check_xyzz_form(out[:37], 5)


def gen_madd_x(rng, n):
    return ac.gen_pt29_madd(rng, n)      # xyzz | q | neg: generic, P + P, P + (-P), from infinity, canonical and worst-case-bound coordinates


def x_of_xyzz(out):
    """X / ZZ of a finite record (Y and ZZZ are not looked at)"""
    ZZ = val29(out[18:27])
    assert ZZ % P != 0, "finite point with ZZ = 0"
    return val29(out[:9]) * pow(ZZ, -1, P) % P


def chk_madd_x(rec, out):
    ac.chk_pt29_madd(rec, out[37:74])                          # the full addition against big integers
    want = ac.affine_of_xyzz(out[37:74])
    assert bool(out[36]) == (want is None), "pt29_madd_x: infinity flag differs"
    if want is not None:
        assert x_of_xyzz(out) == want[0], "pt29_madd_x: X / ZZ differs from pt29_madd's"
        ac.check_vr(out[:9], "X")
        ac.check_limbs(out[18:27])


# ---- walkers ---------------------------------------------------------------------------------------------------------------------
def comb_of(pt):
    """the 8-bit comb of a point as the table builders store it: entry j * 128 + (m - 1) = m * 2^(8 j) * pt, 16 words each"""
    tab = np.zeros((WINDOWS * PER_WINDOW, 16), dtype=np.uint32)
    base = pt
    for j in range(WINDOWS):
        acc = None
        for m in range(1, PER_WINDOW + 1):
            acc = padd(acc, base)
            tab[j * PER_WINDOW + m - 1] = words(ac.mont(acc[0])) + words(ac.mont(acc[1]))
        for _ in range(8):
            base = padd(base, base)
    return tab


def listed_scalars():
    """the scalars the two ends of a walk can go wrong on (all below n)"""
    one = lambda j, m=5: m << (8 * j)
    return [0, 1, one(0), one(16), one(31), one(0, 0x7F), one(31, 0x7F),
            one(0) + one(30), one(3) + one(31), one(29) + one(31, 3),           # exactly two non-zero digits: the second addition comes late
            (0x1234 << 8) + one(20), one(20) + one(25),                             # first window zero
            (N >> 8) & ~0xFF, one(0, 9) + one(7, 9),                                # last window(s) zero
            (0x7F << 248) | (0x80 << 240), (1 << 255) - 1, (0x7F << 248) | (0xFF << 240) | 77,      # top byte 0x7F, the carry window taken
            1 << 255, (1 << 255) + 12345, N - 2, N - (1 << 200),                  # top bit set: the n - u2 form of the Q walk
            N - 1]


_multiples = {}


def scalar_points(pt, count, tag):
    """count pairs (s, s * pt) with s uniform below n: a random start, then steps from a pool of 64 random multiples (one affine
    addition per pair instead of a scalar multiplication)"""
    key = (pt, count, tag)
    if key not in _multiples:
        rng = random.Random(f"{ac.SEED}:trim-multiples:{tag}")
        steps = []
        for _ in range(64):
            t = rng.randrange(1, N)
            steps.append((t, ec.pt_mul(t, pt)))
        s = rng.randrange(1, N)
        cur = ec.pt_mul(s, pt)
        out = []
        for _ in range(count):
            t, tp = rng.choice(steps)
            s, cur = (s + t) % N, padd(cur, tp)
            out.append((s, cur))
        _multiples[key] = out
    return _multiples[key]


def q_partial(u2, j0):
    """the multiple of Q that qphase29_point adds over the windows [j0, 33): u2 with its top bit set is walked as -(n - u2)"""
    flip = u2 >> 255
    k = (N - u2 if flip else u2) + OFFSET
    s = sum((((k >> (8 * j)) & 0xFF) - 128) << (8 * j) for j in range(j0, WINDOWS))
    return -s if flip else s


G_POINT = (ec.GX, ec.GY)
Q_SCALAR = 0x1F2E3D4C5B6A79880123456789ABCDEFFEDCBA98765432100F1E2D3C4B5A6978 % N
_qpoint = None


def q_point():
    global _qpoint
    if _qpoint is None:
        _qpoint = ec.pt_mul(Q_SCALAR, G_POINT)
    return _qpoint


_mul_cache = {}


def mul_cached(k, pt):
    k %= N
    if (k, pt) not in _mul_cache:
        _mul_cache[(k, pt)] = ec.pt_mul(k, pt) if k else None
    return _mul_cache[(k, pt)]


def walk_g_cases(n_random):
    """(record, expected point) pairs: every scalar with x_only off and on"""
    pairs = [(u, mul_cached(u, G_POINT)) for u in listed_scalars()] + scalar_points(G_POINT, n_random, "g")
    return [(words(u) + [xo], want) for u, want in pairs for xo in (0, 1)]


LAST_CHUNK_J0 = 25


def walk_q_cases(n_random):
    """the whole walk (j0 = 0) and the last chunk alone (j0 = 25), onto infinity and onto a random accumulator, x_only off and on.
    Last-chunk scalars take their high bytes from a small pool, so that the multiples they need are computed once."""
    rng = random.Random(f"{ac.SEED}:trim-walk-q")
    Q = q_point()
    pts = point_pool()
    cases = []

    def add(u2, j0, want_mult):
        for xo in (0, 1):
            r0 = None if rng.randrange(4) == 0 else rng.choice(pts)
            want = padd(r0, want_mult)
            if r0 is not None and want_mult is not None and r0[0] == want_mult[0]:
                continue                                      # (never met: the accumulator is unrelated to Q)
            cases.append((words(u2) + [xo, j0] + ac.xyzz_of(rng, r0), want))

    for u in listed_scalars():
        add(u, 0, mul_cached(u, Q))
        add(u, LAST_CHUNK_J0, mul_cached(q_partial(u, LAST_CHUNK_J0), Q))
    for s, sp in scalar_points(Q, n_random, "q"):
        add(s, 0, sp)
    highs = [rng.getrandbits(56) | (b << 55) for b in (0, 1) for _ in range(8)]
    for _ in range(n_random // 4):
        u2 = ((rng.choice(highs) << 200) | rng.getrandbits(200)) % N
        add(u2, LAST_CHUNK_J0, mul_cached(q_partial(u2, LAST_CHUNK_J0), Q))
    return cases


def chk_walk(rec, out, want):
    x_only = rec[8]
    assert bool(out[36]) == (want is None), "infinity flag differs"
    if want is None:
        return
    if x_only:
        assert x_of_xyzz(out) == want[0], "x of the result differs from the big-integer multiple"
    else:
        assert ac.affine_of_xyzz(out) == want, "the result differs from the big-integer multiple"


def set_combs(lib, device):
    """upload the comb of G (comb 0) and of the key (comb 1); returns the two arrays (kept alive by the caller)"""
    import ctypes
    lib.sbvt_set_comb.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    tabs = [np.ascontiguousarray(comb_of(G_POINT)), np.ascontiguousarray(comb_of(q_point()))]
    for which, tab in enumerate(tabs):
        rc = lib.sbvt_set_comb(which, tab.ctypes.data, 1 if device else 0)
        if rc != 0:
            raise ac.HipError(f"sbvt_set_comb({which}) returned {rc}")
    return tabs


def run_checked(lib, backend, name, recs, chk):
    outs = ac.launch(lib, backend, name, recs)
    for i, (rec, out) in enumerate(zip(recs, outs)):
        try:
            chk(rec, out)
        except AssertionError as e:
            raise AssertionError(f"{name} (backend {backend}) case {i} of {len(recs)}: {e}\n  in  = {ac.hexs(rec)}\n  out = {ac.hexs(out)}") from None
    return len(recs)


def run_walk(lib, backend, name, cases):
    recs = [c[0] for c in cases]
    outs = ac.launch(lib, backend, name, recs)
    for i, ((rec, want), out) in enumerate(zip(cases, outs)):
        try:
            chk_walk(rec, out, want)
        except AssertionError as e:
            raise AssertionError(f"{name} (backend {backend}) case {i} of {len(recs)}: {e}\n  in  = {ac.hexs(rec)}\n  out = {ac.hexs(out)}") from None
    return len(recs)
