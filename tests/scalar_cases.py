"""Chosen scalars for every scalar-multiplication path: forgers, walker models and case families.

Between the arithmetic (tools/devunit.hip, tests/arith_cases.py) and the whole-batch parity tests sits the layer that turns a
scalar into table lookups and additions: the signed recodings (gcomb_recode / gcomb_digit, add_const_limbs + comb_digit, the GLV
nibbles of the secp256k1 one-lane kernel, the digits of the Ed25519 one-lane kernel), the sign flip u2 -> n - u2, the carry window,
the giant / baby split of the narrow P-256 walk, and the table rows those walks index.  Random scalars almost never produce a digit
that is exactly 0 or exactly 2^(bits-1), a carry, or an accumulator that equals the entry about to be added.  A signer who knows
the private key can: for any (u1, u2) there is a valid signature, and this module builds it.

Pure Python big integers on top of oracle/p256_py.py, oracle/k256_py.py and oracle/ed25519_py.py.

  forgers   forge_ecdsa(curve, d, u1, u2) -> r | s | e | Q with Q = dG, R = u1 G + u2 Q, r = R.x mod n, s = r / u2, e = u1 s;
            forge_ed25519(a, S, k) -> R | S | A | k with A = aB, R = [S]B - [k]A.  Every forged tuple has a rejecting twin.
  models    Comb: width, window count, offset recoding, flip rule, order of additions of one comb walker.  The models CHOOSE
            inputs; they never judge a verdict (the Python twins, the C oracle and OpenSSL do, tests/test_scalar_cases_cpu.py).
            Widths and run lengths are read from consensus_amd/csrc (the #defines and the defaults of sbv_api.hip), not repeated.
  families  range edges, uniform digits, one non-zero digit per window, the carry threshold, the builders' run boundaries,
            GLV halves, and accumulators that meet +entry (a doubling inside the mixed addition) or -entry (infinity) mid-walk.

cases(scheme) is deterministic (fixed seeds): the CPU tier, the GPU tier and its child processes regenerate the same list."""
import collections
import os
import random
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "consensus_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ed25519_py as ed  # noqa: E402
import k256_py as kc  # noqa: E402
import p256_py as ec  # noqa: E402

SCHEMES = ("p256", "k256", "ed25519")
CURVES = {"p256": ec, "k256": kc}
ORDER = {"p256": ec.N, "k256": kc.N, "ed25519": ed.L}


# ---- what the library defines --------------------------------------------------------------------------------------------------
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def define(header, name):
    """the integer value of `#define name <literal>` in consensus_amd/csrc/<header>"""
    m = re.search(r"^#define\s+%s\s+\(?(0x[0-9A-Fa-f]+|\d+)u?\)?\s*(//.*)?$" % re.escape(name), _src(header), re.M)
    assert m, (header, name)
    return int(m.group(1), 0)


def default_int(name):
    """the initialiser of `int name = <literal>;` in sbv_api.hip (a width the library reads once at start-up)"""
    m = re.search(r"^int\s+%s\s*=\s*(\d+)\s*;" % re.escape(name), _src("sbv_api.hip"), re.M)
    assert m, name
    return int(m.group(1))


def u256_const(header, name):
    """`const u256 name = {{w0, ..., w7}}` or `u256 r = {{...}}` inside `name()`: little-endian 32-bit words -> int"""
    m = re.search(r"\b%s(?:\(\)\s*\{\s*u256\s+r)?\s*=\s*\{\{([^}]*)\}\}" % re.escape(name), _src(header))
    assert m, (header, name)
    words = [int(w.strip().rstrip("u"), 0) for w in m.group(1).split(",")]
    assert len(words) == 8, (name, words)
    return sum(w << (32 * i) for i, w in enumerate(words))


KEY_WINDOWS = define("p256_core.h", "SBV_GTAB_WINDOWS")                  # 33: 32 signed bytes and the carry
KEY_PER_WINDOW = define("p256_core.h", "SBV_GTAB_PER_WINDOW")            # 128
KEY_BITS = KEY_PER_WINDOW.bit_length()                                   # 8
G_BITS = {"p256": default_int("g_gbits"), "k256": default_int("g_k256_gbits"), "ed25519": default_int("g_ed_bbits")}
G_BITS_ONE_LANE = {"p256": define("p256_core.h", "SBV_G16_PER_WINDOW").bit_length(),          # the one-lane kernels' tables: 16
                   "k256": define("k256_core.h", "SBV_K256_G_PER_WINDOW").bit_length(),
                   "ed25519": define("ed25519_core.h", "SBV_ED_B16_PER_WINDOW").bit_length()}
K256_WIDE_BITS = define("k256_keyed.h", "SBV_K256_WIDE_BITS")
K256_WIDE_RUN = define("k256_keyed.h", "SBV_K256_WIDE_RUN")
ED_KEY_WINDOWS = define("ed25519_group.h", "SBV_ED_KEY_WINDOWS")
ED_WIDE_BITS = define("ed25519_core.h", "SBV_ED_HOT_BITS")
ED_WIDE_RUN = define("ed25519_core.h", "SBV_ED_HOT_LANE_ENTRIES")
P256_WIDE_FILL = define("p256_widetab29.h", "SBV_WIDETAB_T")
P256_WIDE_BITS = (16, 18)                                                # sbv_p256_wide_keys takes the width per call: the two the GPU tier sets
NARROW_PER_WINDOW = define("p256_comb29.h", "SBV_NARROW_PER_WINDOW")


def ecdsa_windows(bits):
    return (257 + bits - 1) // bits                                      # gcomb_make / kgcomb_make


def ed_windows(bits):
    return (254 + bits - 1) // bits                                      # edcomb_windows


# ---- walker models -------------------------------------------------------------------------------------------------------------
class Comb:
    """One comb walker: `windows` signed digits of `bits` bits taken from scalar + sum_j 2^(bits j + bits - 1) (no carry chain
    between digits), windows walked in ascending order, the table row of window j read at |digit| - 1, a zero digit skipped.
    flip: a scalar with bit 255 set is walked as n - scalar with every digit's sign inverted.  descending: the one-lane kernels
    walk their 4-bit digits from the top with doublings between them.  role: the scalar it walks (u1 / u2, S / k)."""

    def __init__(self, scheme, name, role, bits, windows, flip=False, descending=False, narrow=False, sequential=True, paths=""):
        self.scheme, self.name, self.role, self.bits, self.windows = scheme, name, role, bits, windows
        self.flip, self.descending, self.narrow, self.paths = flip, descending, narrow, paths
        self.sequential = sequential and not descending             # one accumulator takes the terms in order: mid-walk collisions can be aimed
        self.n = ORDER[scheme]
        self.half = 1 << (bits - 1)
        self.offset = sum(1 << (bits * j + bits - 1) for j in range(windows))

    def flips(self, u):
        return self.flip and (u >> 255) & 1 == 1

    def digits(self, u):
        """the signed digit the walker applies in every window: sum_j digit_j 2^(bits j) == u (mod n)"""
        v = self.n - u if self.flips(u) else u
        k = v + self.offset
        assert k >> (self.bits * self.windows) == 0, (self.name, hex(u))
        d = [((k >> (self.bits * j)) & (2 * self.half - 1)) - self.half for j in range(self.windows)]
        return [-x for x in d] if self.flips(u) else d

    def terms(self, u):
        """the additions of the walk, in order: (window, part, multiple of the base point), zero parts skipped"""
        out = []
        for j, d in enumerate(self.digits(u)):
            if d == 0:
                continue
            if not self.narrow:
                out.append((j, "entry", d << (self.bits * j)))
                continue
            sign, ad = (-1 if d < 0 else 1), abs(d)                      # narrow_split: |d| = 16 a + b, a in 0..8, b in -7..8
            a = (ad + 7) >> 4
            b = ad - 16 * a
            if a:
                out.append((j, "giant", sign * 16 * a << (self.bits * j)))
            if b:
                out.append((j, "baby", sign * b << (self.bits * j)))
        return out[::-1] if self.descending else out

    def carry_threshold(self):
        """the smallest walked scalar whose top window is not zero, for a comb whose top window holds only the recoding's carry"""
        assert self.bits * (self.windows - 1) == 256, self.name
        return (1 << 256) - (self.offset - (1 << (self.bits * self.windows - 1)))

    def realize(self, want, alone=False):
        """a scalar in [1, n) whose digits are want[j] in every window j named (the windows above the highest one named absorb the
        sign), or None when no such scalar exists.  alone: every other digit is zero, but for a borrow of +-1 in the next window"""
        v = sum(d << (self.bits * j) for j, d in want.items())
        top = self.bits * (max(want) + 1)
        for c in (v, v + (1 << top), v - (1 << top)):
            u = c % self.n if (self.flip and -self.n < c < 0) else c
            if not 0 < u < self.n or (u + self.offset) >> (self.bits * self.windows):
                continue
            if self.scheme == "ed25519" and u >= 1 << 253:
                continue
            d = self.digits(u)
            rest = [(j, x) for j, x in enumerate(d) if x and j not in want]
            if all(d[j] == x for j, x in want.items()) and (not alone or rest in ([], [(max(want) + 1, 1)], [(max(want) + 1, -1)])):
                return u
        return None


def walkers(scheme):
    """every comb walker of a scheme, by name"""
    if scheme == "ed25519":
        ws = [Comb(scheme, "b%d" % G_BITS[scheme], "S", G_BITS[scheme], ed_windows(G_BITS[scheme]), paths="grouped, keyed: comb of B at the default width"),
              Comb(scheme, "b%d" % G_BITS_ONE_LANE[scheme], "S", G_BITS_ONE_LANE[scheme], ed_windows(G_BITS_ONE_LANE[scheme]), paths="one-lane kernel (ed_add_sB); SBV_ED_B_BITS=16"),
              Comb(scheme, "key8", "k", KEY_BITS, ED_KEY_WINDOWS, paths="grouped and registered 8-bit combs of -A (ed_qphase_lane)"),
              Comb(scheme, "wide%d" % ED_WIDE_BITS, "k", ED_WIDE_BITS, ed_windows(ED_WIDE_BITS), paths="hot-key pool and widened slots (ed_qphase_wide_lane)"),
              Comb(scheme, "lane4", "k", 4, 64, descending=True, paths="one-lane kernel: k + 0x88..8, 64 nibbles from the top")]
        return collections.OrderedDict((w.name, w) for w in ws)
    gb, g1 = G_BITS[scheme], G_BITS_ONE_LANE[scheme]
    ws = [Comb(scheme, "g%d" % gb, "u1", gb, ecdsa_windows(gb), paths="comb of G at the default width"),
          Comb(scheme, "g%d" % g1, "u1", g1, ecdsa_windows(g1), paths="comb of G of the one-lane kernel; SBV_G_BITS / SBV_K256_G_BITS = 16"),
          Comb(scheme, "key8", "u2", KEY_BITS, KEY_WINDOWS, flip=True, paths="grouped step and one-lane registered form on 8-bit combs (qphase29_point, k256_qphase_point)")]
    if scheme == "p256":
        ws += [Comb(scheme, "wide%d" % b, "u2", b, ecdsa_windows(b), flip=True, paths="widened slots and hot keys (wide_qphase29_point)") for b in P256_WIDE_BITS]
        ws += [Comb(scheme, "key8c", "u2", KEY_BITS, KEY_WINDOWS, sequential=False,
                    paths="8-lane and one-launch registered forms on 8-bit combs (keyed29_partial_lane): u2 + 0x80..80 WITHOUT the flip, so the carry "
                          "window is walked for every u2 >= T; the terms are dealt to the lanes, no single accumulator takes them in order"),
               Comb(scheme, "narrow", "u2", KEY_BITS, KEY_WINDOWS, flip=True, narrow=True, paths="rows-only keys of the grouped step (qphase29_point_narrow)"),
               Comb(scheme, "lane4", "u2", 4, 65, descending=True, paths="one-lane generic kernel: u2 + 0x88..8, 64 nibbles and the carry")]
    else:
        ws += [Comb(scheme, "wide%d" % K256_WIDE_BITS, "u2", K256_WIDE_BITS, ecdsa_windows(K256_WIDE_BITS), paths="widened slots: k256_gphase_point on the key's comb, no flip")]
    return collections.OrderedDict((w.name, w) for w in ws)


# the GLV recoding of the secp256k1 one-lane kernel (k256_sc.h: ksc_split_lambda; k256_core.h: k256_verify_lane)
def glv_split(k):
    """(k1, neg1, k2, neg2) as ksc_split_lambda returns them; constants read from k256_sc.h"""
    n = kc.N
    g1, g2 = u256_const("k256_sc.h", "g1"), u256_const("k256_sc.h", "g2")
    mb1, mb2 = u256_const("k256_sc.h", "minus_b1"), u256_const("k256_sc.h", "minus_b2")
    lam = u256_const("k256_sc.h", "k256_lambda_words")
    k %= n
    c1, c2 = (k * g1 + (1 << 383)) >> 384, (k * g2 + (1 << 383)) >> 384
    r2 = (c1 * mb1 + c2 * mb2) % n
    r1 = (k - r2 * lam) % n
    neg1, neg2 = n - r1 < r1, n - r2 < r2
    return (n - r1 if neg1 else r1), neg1, (n - r2 if neg2 else r2), neg2


GLV_EIGHTS = int("8" * 32, 16)                                           # the offset of 32 nibbles: a half + this >= 2^128 sets the carry nibble


def glv_carries(k):
    k1, _, k2, _ = glv_split(k)
    return (k1 + GLV_EIGHTS) >> 128 != 0, (k2 + GLV_EIGHTS) >> 128 != 0


# ---- fixed-base multiplication by the twins' own addition (32 additions from a table of 8-bit windows) -------------------------
_TABLES = {}


def _table(scheme):
    if scheme not in _TABLES:
        if scheme == "ed25519":
            add, base, ident = ed.pt_add, ed.B, ed.IDENT
        else:
            add, base, ident = CURVES[scheme].pt_add, (CURVES[scheme].GX, CURVES[scheme].GY), None
        rows = []
        for _ in range(32):
            row, p = [ident], ident
            for _ in range(255):
                p = add(p, base)
                row.append(p)
            rows.append(row)
            base = add(row[255], base)
        _TABLES[scheme] = (add, ident, rows)
    return _TABLES[scheme]


def base_mul(scheme, k):
    """k * G (ECDSA curves: affine point or None) or k * B (Ed25519: extended point)"""
    add, acc, rows = _table(scheme)
    k %= ORDER[scheme]
    for j in range(32):
        m = (k >> (8 * j)) & 255
        if m:
            acc = add(acc, rows[j][m])
    return acc


# ---- forgers -------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "scheme walker family name tuple expect designed_reject a b d")
Case.__doc__ = """tuple: the 160-byte (ECDSA: r | s | e | Qx | Qy, big-endian) or 128-byte (Ed25519: R | S | A | k, little-endian) input;
expect: the verdict by construction (the CPU tier holds the twins, the oracle and OpenSSL to it); designed_reject: no valid signature
exists for these scalars (R is infinity); a, b: u1, u2 or S, k; d: the private key"""


def _be(x):
    return x.to_bytes(32, "big")


def pubkey(scheme, d):
    if scheme == "ed25519":
        return ed.encode(base_mul(scheme, d))
    q = base_mul(scheme, d)
    return _be(q[0]) + _be(q[1])


def forge_ecdsa(scheme, d, u1, u2):
    """(tuple, valid): a signature of hash e under Q = dG whose verification computes exactly u1 and u2.  valid is False when
    R = u1 G + u2 Q is infinity or R.x = 0 mod n: no signature exists, the tuple carries r = 1 and must reject."""
    n = ORDER[scheme]
    assert 0 <= u1 < n and 0 < u2 < n and 0 < d < n
    R = base_mul(scheme, u1 + u2 * d)
    r = R[0] % n if R is not None else 0
    valid = r != 0
    if not valid:
        r = 1
    s = r * pow(u2, -1, n) % n
    e = u1 * s % n
    return _be(r) + _be(s) + _be(e) + pubkey(scheme, d), valid


def forge_ed25519(a, S, k):
    """R | S | A | k with A = aB and R = [S]B - [k]A: always valid for S, k < L"""
    assert 0 <= S < ed.L and 0 <= k < ed.L
    R = base_mul("ed25519", S - k * a)
    return ed.encode(R) + S.to_bytes(32, "little") + pubkey("ed25519", a) + k.to_bytes(32, "little")


def twin(scheme, t):
    """the same scalars in the walk, a verdict that must be reject: one hash bit flipped (ECDSA: u1 changes with e, r and s and so
    u2 stay; the existing wide-comb test's twin), one bit of R flipped (Ed25519: S and k stay)"""
    b = bytearray(t)
    if scheme == "ed25519":
        b[1] ^= 0x10
    else:
        b[70] ^= 4
    return bytes(b)


# ---- families ------------------------------------------------------------------------------------------------------------------
KEY_SEED = {"p256": 0x51CA1A5, "k256": 0x51CA1A6, "ed25519": 0x51CA1A7}


def private_keys(scheme):
    """(d, d_rows): the key every case signs with, and a second one for the rows-only walk (few tuples per batch)"""
    rng = random.Random(KEY_SEED[scheme])
    return rng.randrange(1, ORDER[scheme]), rng.randrange(1, ORDER[scheme])


def _edges(scheme):
    n = ORDER[scheme]
    if scheme == "ed25519":
        return [("0", 0), ("1", 1), ("2", 2), ("L-1", n - 1), ("L-2", n - 2), ("(L-1)/2", (n - 1) // 2), ("(L+1)/2", (n + 1) // 2), ("2^252", 1 << 252),
                ("2^252-1", (1 << 252) - 1), ("2^252+1", (1 << 252) + 1), ("2^251", 1 << 251)]
    return [("0", 0), ("1", 1), ("2", 2), ("n-1", n - 1), ("n-2", n - 2), ("(n-1)/2", (n - 1) // 2), ("(n+1)/2", (n + 1) // 2), ("2^255-1", (1 << 255) - 1),
            ("2^255", 1 << 255), ("2^255+1", (1 << 255) + 1), ("top-bit-clear-max", min(n - 1, (1 << 255) - 1)), ("n-2^255", n - (1 << 255))]


def builder_multiples(w):
    """the multiples on both sides of every run boundary of the builder that makes this comb's rows on the device"""
    if w.bits == KEY_BITS:                                               # rows step: babies 1..8, giants 16 a; fill: the other 112
        return [1, 7, 8, 9, 15, 16, 17, 127, 128]
    ms = {1, 2, w.half - 1, w.half}
    if w.scheme == "k256":
        run = [K256_WIDE_RUN]                                            # k256_widetab_lane: runs of 64, four per 256 (c = 0..3)
        ms |= {k * K256_WIDE_RUN + e for k in (1, 2, 3, 4) for e in (-1, 0, 1)}
    elif w.scheme == "ed25519":
        run = [ED_WIDE_RUN]                                              # ed_widetab_lane: 32 entries per lane
        ms |= {k * ED_WIDE_RUN + e for k in (1, 2, 8) for e in (-1, 0, 1)}
    else:
        babies = 1 << (w.bits // 2)                                      # p256_widetab29.h: chains (babies, giants), fill in chunks of SBV_WIDETAB_T
        run = [P256_WIDE_FILL, babies]
        ms |= {k * P256_WIDE_FILL + e for k in (1, 2) for e in (-1, 0, 1)} | {k * babies + e for k in (1, 2) for e in (-1, 0, 1)}
        ms |= {w.half - babies + e for e in (-1, 0, 1)}
    ms |= {63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257}      # the list every wide comb gets, whatever its run length
    assert all(r >= 1 for r in run)
    return sorted(m for m in ms if 1 <= m <= w.half)


K256_C3_MULTIPLES = [193, 200, 255, 256, 449, 512, 32705, 32768]         # m0 = 64 q with q & 3 == 3: a C_j + 192 B_j = (a + 1) C_j - 64 B_j


def _scalar_plans(scheme):
    """(walker, family, name, scalar or None) for every single-scalar family; None = the model says no scalar in range has these digits"""
    n = ORDER[scheme]
    plans = []
    for w in walkers(scheme).values():
        if w.narrow:
            continue                                                     # same digits as key8: its own families are the split's boundaries, below
        top = w.windows - 1
        carry_top = scheme != "ed25519" and w.bits * top == 256          # the top window holds only the recoding's carry
        free = range(top) if carry_top else range(w.windows)
        for name, v in _edges(scheme):
            plans.append((w, "edges", name, v))
        # uniform digits below the top two windows (those absorb the sign and keep the scalar in range)
        low = list(free)[:-1]
        for name, x in (("zero", 0), ("minus-one", -1), ("plus-max", w.half - 1), ("minus-half", -w.half)):
            if x == 0:
                plans.append((w, "uniform", name, 0))
                continue
            u = None
            for cut in (len(low), len(low) - 1):
                u = u or w.realize({j: x for j in low[:cut]})
            plans.append((w, "uniform", name, u))
        for j in free:
            for name, x in (("+1", 1), ("-1", -1), ("+half", w.half), ("-half", -w.half)):
                plans.append((w, "single", "w%d:%s" % (j, name), w.realize({j: x}, alone=True)))
        if carry_top:
            T = w.carry_threshold()
            vals = [("T-1", T - 1), ("T", T), ("T+1", T + 1)]
            if w.flip:
                vals += [("n-T", n - T), ("n-T+1", n - T + 1), ("n-T-1", n - T - 1), ("flip-top-0x7F", n - ((0x7F << 248) | ((1 << 248) - 1))),
                         ("2^255-1-carry", (1 << 255) - 1)]
            plans += [(w, "carry", name, v % n) for name, v in vals]
        if w.role in ("u2", "k") and not w.descending:
            ms = builder_multiples(w)
            rows = list(free)
            for s in range(len(ms)):                                     # a Latin square: rotation s puts multiple ms[(j + s) % len] in window j
                for sign in (1, -1):
                    want = {j: sign * ms[(j + s) % len(ms)] for j in rows}
                    want = {j: (-abs(x) if abs(x) == w.half else x) for j, x in want.items()}     # +2^(bits-1) exists only as a flipped digit: the single family
                    u = w.realize(want) or w.realize({j: x for j, x in want.items() if j != rows[-1]})
                    plans.append((w, "builder", "rot%d:%s" % (s, "+" if sign > 0 else "-"), u))
            if scheme == "k256" and w.bits == K256_WIDE_BITS:
                for s in range(len(K256_C3_MULTIPLES)):
                    want = {j: -K256_C3_MULTIPLES[(j + s) % len(K256_C3_MULTIPLES)] for j in rows}
                    u = w.realize(want) or w.realize({j: x for j, x in want.items() if j != rows[-1]})
                    plans.append((w, "builder-c3", "rot%d" % s, u))
    return plans


def _glv_plans():
    """(name, u2): halves at the bound, the four sign combinations, the carry nibble of either half"""
    n, lam = kc.N, u256_const("k256_sc.h", "k256_lambda_words")
    nocarry, carry = (1 << 128) - GLV_EIGHTS - 1, (1 << 128) - GLV_EIGHTS
    out = []
    for s1 in (1, -1):
        for s2 in (1, -1):
            for h1, h2 in ((1, 1), (nocarry, nocarry), (carry, 1), (1, carry), (carry, carry), ((1 << 127) - 1, (1 << 127) - 1), (1 << 127, 3)):
                out.append(("%s%x %s%x" % ("+" if s1 > 0 else "-", h1, "+" if s2 > 0 else "-", h2), (s1 * h1 + s2 * h2 * lam) % n))
    rng = random.Random(0x61F)                                           # the bound itself: the largest halves among seeded scalars
    pool = [rng.randrange(1, n) for _ in range(4000)]
    out.append(("max-k1", max(pool, key=lambda k: glv_split(k)[0])))
    out.append(("max-k2", max(pool, key=lambda k: glv_split(k)[2])))
    return [(name, k) for name, k in out if k]


def _collision_plans(scheme, d):
    """(walker, name, u1, u2, infinity): u1 chosen so that the accumulator before the t-th addition of the Q phase is + that entry
    (a doubling inside the mixed addition) or - it (the sum is infinity; the next addition lands on infinity).  The G phase comes
    first, so the accumulator is u1 G + sum of the earlier terms of u2 Q; with Q = dG: u1 = d (+-term_t - sum_{i<t} term_i)."""
    n = ORDER[scheme]
    rng = random.Random(KEY_SEED[scheme] ^ 0xC0)
    out = []
    for w in walkers(scheme).values():
        if w.role != "u2" or not w.sequential:
            continue
        for flipped in (False, True):
            u2 = rng.randrange(1 << 254, 1 << 255) if not (flipped and w.flip) else rng.randrange((1 << 255) + 1, n)
            terms = w.terms(u2)
            picks = {"first": 0, "middle": len(terms) // 2, "last": len(terms) - 1}
            if w.narrow:                                                 # against the giant and against the baby of one window
                mid = next(i for i in range(len(terms) // 2, len(terms) - 1) if terms[i][1] == "giant" and terms[i + 1][1] == "baby" and terms[i][0] == terms[i + 1][0])
                picks = {"first": 0, "giant": mid, "baby": mid + 1, "last": len(terms) - 1}
            for where, t in picks.items():
                for sign, kind in ((1, "doubling"), (-1, "infinity")):
                    u1 = d * (sign * terms[t][2] - sum(x[2] for x in terms[:t])) % n
                    name = "%s:%s:%s%s" % (where, terms[t][1], kind, ":flip" if w.flips(u2) else "")
                    out.append((w, name, u1, u2, sign < 0 and t == len(terms) - 1))
    return out


def _build(scheme):
    n = ORDER[scheme]
    d, d_rows = private_keys(scheme)
    rng = random.Random(KEY_SEED[scheme] ^ 0xF0)
    out, unreachable = [], []

    def emit(w, family, name, a, b, key=d, infinity=False):
        if scheme == "ed25519":
            t, valid = forge_ed25519(key, a, b), True
        else:
            t, valid = forge_ecdsa(scheme, key, a, b)
        assert valid != infinity, (scheme, w.name, family, name)
        out.append(Case(scheme, w.name, family, name, t, valid, not valid, a, b, key))
        out.append(Case(scheme, w.name, family, name + "/twin", twin(scheme, t), False, not valid, a, b, key))

    for w, family, name, v in _scalar_plans(scheme):
        if v is None or (v == 0 and w.role == "u2"):
            unreachable.append((w.name, family, name))                   # no scalar of the range has these digits (u2 = 0 has no signature)
            continue
        other = rng.randrange(1, n)
        a, b = (v, other) if w.role in ("u1", "S") else (other, v)
        emit(w, family, name, a, b)
    if scheme == "p256":                                                 # the rows-only walk: every |digit| on both sides of the giant / baby split
        w = walkers(scheme)["narrow"]
        ms = [1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 120, 121, 127, 128]
        for s in range(len(ms)):
            for sign in (1, -1):
                want = {j: sign * ms[(j + s) % len(ms)] for j in range(KEY_WINDOWS - 1)}
                want = {j: (-abs(x) if abs(x) == w.half else x) for j, x in want.items()}
                u2 = w.realize(want) or w.realize({j: x for j, x in want.items() if j != KEY_WINDOWS - 2})
                assert u2, (s, sign)
                emit(w, "builder", "rot%d:%s" % (s, "+" if sign > 0 else "-"), rng.randrange(1, n), u2, key=d_rows)
        T = w.carry_threshold()
        for name, v in (("T-1", T - 1), ("T", T), ("T+1", T + 1), ("n-T", n - T), ("n-T+1", n - T + 1), ("1", 1), ("n-1", n - 1)):
            emit(w, "carry", name, rng.randrange(1, n), v, key=d_rows)
    if scheme == "k256":
        glv = Comb(scheme, "glv", "u2", 4, 33, descending=True, paths="one-lane kernel: GLV halves, 32 nibbles and the carry each")
        for name, k in _glv_plans():
            emit(glv, "glv", name, rng.randrange(1, n), k)
    if scheme != "ed25519":
        for key in (d, d_rows):                                          # the rows-only walk has its own key
            for w, name, u1, u2, infinity in _collision_plans(scheme, key):
                if w.narrow == (key == d_rows):
                    emit(w, "collision", name, u1, u2, key=key, infinity=infinity)
    else:                                                                # complete additions: no exceptional case, a P = Q doubling mid-walk all the same
        for w in (walkers(scheme)["key8"], walkers(scheme)["wide%d" % ED_WIDE_BITS]):
            k = rng.randrange(1 << 251, 1 << 252)
            terms = w.terms(k)
            for where, t in (("first", 0), ("middle", len(terms) // 2), ("last", len(terms) - 1)):
                # the comb holds multiples of -A = -aB: accumulator [S]B - a sum_{i<t} term_i B == -a term_t B
                S = d * (sum(x[2] for x in terms[:t]) - terms[t][2]) % n
                emit(w, "doubling", where, S, k)
    return out, unreachable


_CASES = {}


def cases(scheme):
    """the case list of a scheme (computed once per process)"""
    if scheme not in _CASES:
        _CASES[scheme] = _build(scheme)
    return _CASES[scheme][0]


def unreachable(scheme):
    """(walker, family, name) of the digit patterns no scalar of the range produces: listed, never dropped silently"""
    cases(scheme)
    return _CASES[scheme][1]


def blob(cs):
    return b"".join(c.tuple for c in cs)


def by_walker(cs, *names):
    return [c for c in cs if c.walker in names]


def split_keyed(scheme, tuples):
    """(records, slots, keys) of the registered-key form: the tuples without their key, first-appearance slots"""
    width, lo, hi = (128, 64, 96) if scheme == "ed25519" else (160, 96, 160)
    keys, index, recs, slots = [], {}, bytearray(), []
    for i in range(len(tuples) // width):
        t = tuples[width * i:width * (i + 1)]
        k = t[lo:hi]
        if k not in index:
            index[k] = len(keys)
            keys.append(k)
        recs += t[:lo] + t[hi:]
        slots.append(index[k])
    return bytes(recs), slots, keys


if __name__ == "__main__":
    for sc in SCHEMES:
        cs = cases(sc)
        print(sc, len(cs), "cases;", len(unreachable(sc)), "unreachable digit patterns;",
              dict(collections.Counter((c.walker, c.family) for c in cs)))
