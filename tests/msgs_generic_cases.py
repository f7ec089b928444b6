"""Cases of the raw-message entries of the GENERIC verifiers (include/sbv.h: sbv_p256_verify_msgs, sbv_secp256k1_verify_msgs,
sbv_p256_verify_msgs_sharded), shared by the CPU tier (tests/test_msgs_generic_cpu.py: the lane as host code) and the GPU tier
(tests/test_gpu_msgs_generic.py: the kernel).  No GPU code is imported here.

The ECDSA cases of tests/frontend_cases.py, families (a)-(e) of both curves, are mapped to (name, key, message, signature bytes, want)
with the slot rule DROPPED: the case's own key travels with it, so want = frontend_cases.judge(scheme, key, msg, sig) — a case the
keyed entries reject for its slot is judged on its signature here.  Added to them:

  key cases   under a signature the honest key accepts: Qx = p; Qy = p + 1, which a verifier that reduced coordinates would take for
              the valid ordinate 1 (the abscissa is one of the curve's points with y = 1); one bit of Qy flipped; (0, 0); the other
              curve's key bytes; the negated key (Qx, p - Qy), a point of the curve that is not the signer
  long tail   the signer layout of tests/stream_cases.py over raw messages: 12 signers above and 12 below the 256 uses from which the
              P-256 step fills a key's table, and 100 keys used once, shuffled; every fifth signature spoiled (a message byte, a
              signature bit, or another signer's key), so the expected bits come from the generator

tuples(scheme, cases) builds what the host route builds today: strict_rs | hashlib SHA-256 | key, zeros for r | s where the parse
refuses — the input of verify_batch / secp256k1_verify_batch the entries must agree with bit for bit."""
import collections
import functools
import hashlib
import random

import frontend_cases as fc

SCHEMES = ("p256", "k256")
Case = collections.namedtuple("Case", "name key msg sig want")

# abscissae of points with y = 1 (roots of x^3 + a x + b - 1; asserted below)
X_WITH_Y_1 = {"p256": 0x8d0177ebab9c6e9e10db6dd095dbac0d6375e8a97b70f611875d877f0069d2c7,
              "k256": 0xcbb0deab125754f1fdb2038b0434ed9cb3fb53ab735391129994a535d925f673}

MAIN, SIGNERS, SINGLES, LIGHT_USES = 8229, 24, 100, 85        # tests/stream_cases.py: the long-tailed batch


def generic(scheme, c):
    """a front-end case without its slot rule, judged on its own key"""
    return Case(c.name, c.key, c.msg, c.sig, fc.judge(scheme, c.key, c.msg, c.sig))


@functools.lru_cache(maxsize=None)
def families(scheme):
    """{family: cases} of (a)-(e); the ladder in its ascending packing"""
    return {f: [generic(scheme, c) for c in cs] for f, cs in fc.families(scheme).items()}


@functools.lru_cache(maxsize=None)
def ladder(scheme):
    up, shuffled, perm = fc.ladder(scheme)
    up = [generic(scheme, c) for c in up]
    return up, [up[p] for p in perm], perm


@functools.lru_cache(maxsize=None)
def empty_batch(scheme):
    return [generic(scheme, c) for c in fc.empty_batch(scheme)]


@functools.lru_cache(maxsize=None)
def filler(scheme):
    return [generic(scheme, c) for c in fc.filler(scheme)]


@functools.lru_cache(maxsize=None)
def key_cases(scheme):
    cv = fc.CURVES[scheme]
    other = "k256" if scheme == "p256" else "p256"
    key = fc.signer(scheme, 0)[1]
    msg = b"accepted under the key of signer 0"
    sig = fc.sign(scheme, 0, msg)
    qx, qy = key[:32], key[32:]
    x1 = X_WITH_Y_1[scheme]
    assert cv.mod.on_curve(x1, 1) and cv.P + 1 < 1 << 256
    bent = key[:63] + bytes([key[63] ^ 1])
    negated = qx + fc.be32(cv.P - int.from_bytes(qy, "big"))
    assert cv.mod.on_curve(int.from_bytes(negated[:32], "big"), int.from_bytes(negated[32:], "big"))
    keys = [("k_honest", key), ("k_qx_eq_p", fc.be32(cv.P) + qy), ("k_qy_eq_p_plus_1", fc.be32(x1) + fc.be32(cv.P + 1)),
            ("k_qy_eq_1_reduced", fc.be32(x1) + fc.be32(1)), ("k_qy_bit_flipped", bent), ("k_zero_zero", bytes(64)),
            ("k_other_curve", fc.signer(other, 0)[1]), ("k_negated", negated)]
    out = [Case(name, k, msg, sig, fc.judge(scheme, k, msg, sig)) for name, k in keys]
    assert [c.want for c in out] == [True] + [False] * 7, [(c.name, c.want) for c in out]
    return out


@functools.lru_cache(maxsize=None)
def long_tail(scheme):
    """MAIN cases in a seeded shuffle: 12 signers with LIGHT_USES signatures each, 12 with the rest between them, SINGLES signers with
    one; case i with i % 5 == 4 is spoiled, rotating through a flipped message byte, a flipped bit of the signature's last byte and
    the key of another (heavy) signer.  want is the construction's (the CPU tier holds it to the oracles)."""
    rng = random.Random(0x7A11 + SCHEMES.index(scheme))
    heavy = MAIN - SINGLES - LIGHT_USES * (SIGNERS // 2)
    who = []
    for s in range(SIGNERS // 2):
        who += [100 + s] * (heavy // (SIGNERS // 2) + (1 if s < heavy % (SIGNERS // 2) else 0))
        who += [200 + s] * LIGHT_USES
    who += [1000 + s for s in range(SINGLES)]
    assert len(who) == MAIN
    rng.shuffle(who)
    uses = collections.Counter(who)
    assert sorted(uses.values()) == [1] * SINGLES + [LIGHT_USES] * 12 + sorted(uses[100 + s] for s in range(12)) and min(uses[100 + s] for s in range(12)) > 256
    out = []
    for i, w in enumerate(who):
        msg = b"long tail %d " % i + rng.randbytes(i % 90)
        key, sig = fc.signer(scheme, w)[1], fc.sign(scheme, w, msg)
        want = i % 5 != 4
        if not want:
            cause = (i // 5) % 3 if w < 1000 else (i // 5) % 2          # a key used once keeps its key
            if cause == 0:
                msg = msg[:-1] + bytes([msg[-1] ^ 1])
            elif cause == 1:
                sig = sig[:-1] + bytes([sig[-1] ^ 1])
            else:
                key = fc.signer(scheme, 100 + (i % 12 if 100 + i % 12 != w else (i + 1) % 12))[1]        # one of the heavy signers, never the signer
        out.append(Case("tail_%d" % i, key, msg, sig, want))
    return out


def interleaved(scheme, cases, n, shift=0):
    """n cases: those of `cases` from index `shift` on (cyclically) alternating with honest filler"""
    fill = filler(scheme)
    return [cases[(shift + j // 2) % len(cases)] if j % 2 == 0 else fill[(j // 2) % len(fill)] for j in range(n)]


def pool(scheme):
    """every case but the ladder's long messages, for the interleaved calls"""
    fams = families(scheme)
    return [c for f in sorted(fams) if f != "a" for c in fams[f]] + key_cases(scheme) + [c for c in fams["a"] if len(c.msg) <= 260][::7]


def sample(scheme, count=32):
    """a seeded sample over all families and the key cases, for calls that send one case alone"""
    rng = random.Random(0x6E3 + SCHEMES.index(scheme))
    fams = dict(families(scheme), k=key_cases(scheme))
    every = [c for f, cs in sorted(fams.items()) for c in cs if f != "a" or len(c.msg) < 4097]
    return rng.sample(every, count - len(fams)) + [rng.choice(cs) for _, cs in sorted(fams.items())]


def batch(cases):
    """(messages, signatures, keys, want) of a call that sends `cases` in order"""
    return [c.msg for c in cases], [c.sig for c in cases], [c.key for c in cases], [c.want for c in cases]


def tuple_of(c):
    """the 160-byte tuple the host route builds for a case: strict parse (zeros when refused) | SHA-256 | key"""
    return (fc.strict_rs(c.sig) or bytes(64)) + hashlib.sha256(c.msg).digest() + c.key


def tuples(cases):
    return b"".join(tuple_of(c) for c in cases)


# ---- the kernel's slice check, as a model ---------------------------------------------------------------------------------------------
def lane_slice(moff, soff, i, mbase, sbase, mbytes, sbytes):
    """(m0, m1, s0, s1) lane i of k_msg_frontend_tuples hashes and parses: its slice of both tables relative to the bases when they are
    monotone and inside the uploads, else the empty message and the empty signature (unsigned 64-bit arithmetic, as on the device)"""
    M = (1 << 64) - 1
    m0, m1, s0, s1 = (moff[i] - mbase) & M, (moff[i + 1] - mbase) & M, (soff[i] - sbase) & M, (soff[i + 1] - sbase) & M
    if not (m0 <= m1 <= mbytes and s0 <= s1 <= sbytes):
        return 0, 0, 0, 0
    return m0, m1, s0, s1


def quorum_bits(want, keys, group, quorum):
    """bit p = proposal p (cases [p * group, (p + 1) * group)) carries >= quorum accepted signatures by DISTINCT keys"""
    return [len({keys[i] for i in range(p * group, (p + 1) * group) if want[i]}) >= quorum for p in range(len(want) // group)]
