"""Cases and expected values of BIP-340 Schnorr verification against registered secp256k1 keys, shared by the CPU tier
(tests/test_k256_schnorr_keyed_cpu.py: the emulated lanes and the host forms) and the GPU tier (tests/test_gpu_k256_schnorr_keyed.py).
Everything of the scheme itself is tests/k256_schnorr_cases.py's (imported, nothing redefined): its 1 967 verification cases are mapped
to (message, signature, slot) under a registry that holds every key twice, as x | y_even and as x | p - y_even, and the verdict stays
the model's.  New here: the registry layout, a direct model of the keyed lane (held to the generic model by the CPU tier), the batch
orders that make the four wavefront compositions, and the walk cases of the debug op, which steer the accumulator through the private
scalars the case set knows."""
import functools

import k256_py as kp
import k256_schnorr_cases as sc

N, P = sc.N, sc.P
OP_IN, OP_OUT = sc.OP_IN, sc.OP_OUT
be32, op_record, op_result = sc.be32, sc.op_record, sc.op_result
NO_SLOT = 0xFFFFFFFF
WAVE = 64


# ---- the registry -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lift_key(pk):
    """(64 key bytes, ok) of an x-only key: x | y of lift_x, or x | 0^32 and 0 (sbv_secp256k1_schnorr_lift_keys)"""
    pt = sc.lift_x(int.from_bytes(pk, "big"))
    return (pk + bytes(32), 0) if pt is None else (pk + be32(pt[1]), 1)


@functools.lru_cache(maxsize=None)
def xonly_keys():
    """the distinct x-only keys of the case set, in order of appearance"""
    seen, out = set(), []
    for _, pk, _, _ in sc.cases():
        if pk not in seen:
            seen.add(pk)
            out.append(pk)
    return out


@functools.lru_cache(maxsize=None)
def registry():
    """(keys, slot_of, valid): the 64-byte keys in slot order as sbv_secp256k1_register_keys assigns slots on an empty registry (equal
    bytes share a slot); slot_of[parity][pk]; valid[slot].  A key on the curve is registered twice, with even and with odd y; a refused
    one once, as lift_keys leaves it, which makes an invalid slot."""
    keys, index, valid = [], {}, []

    def reg(k, ok):
        if k not in index:
            index[k] = len(keys)
            keys.append(k)
            valid.append(ok)
        return index[k]

    slot_of = ({}, {})
    for pk in xonly_keys():
        k, ok = lift_key(pk)
        slot_of[0][pk] = reg(k, ok)
        slot_of[1][pk] = reg(pk + be32(P - int.from_bytes(k[32:], "big")), 1) if ok else slot_of[0][pk]
    return keys, slot_of, valid


def out_of_range_slot():
    return len(registry()[0])


def point_of(slot):
    k = registry()[0][slot]
    return int.from_bytes(k[:32], "big"), int.from_bytes(k[32:], "big")


# ---- the direct model of the keyed lane ---------------------------------------------------------------------------------------------
def verify_keyed(key, msg, sig):
    """the verdict for a slot that holds `key` (Qx | Qy of either parity): R = s G + u2 Q with u2 = n - e (even Qy) or e (odd Qy)"""
    qx, qy = int.from_bytes(key[:32], "big"), int.from_bytes(key[32:], "big")
    r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
    if qx >= P or qy >= P or not kp.on_curve(qx, qy) or r >= P or s >= N:
        return 0
    e = int.from_bytes(sc.tagged("BIP0340/challenge", sig[:32] + key[:32] + msg), "big") % N
    u2 = e if qy % 2 else (N - e) % N
    R = kp.pt_add(sc.gmul(s), sc.mul(u2, (qx, qy)))
    return 1 if R is not None and R[0] == r and R[1] % 2 == 0 else 0


# ---- the verification items -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def items():
    """[(category, parity, msg, sig, slot, ok)]: every case of the generic set under its even and its odd registration ("other_key"
    becomes another slot; a refused key an invalid slot), then valid signatures against slot numbers out of range"""
    _, slot_of, _ = registry()
    exp = sc.expected_all()
    out = []
    for parity in (0, 1):
        for (cat, pk, m, sig), ok in zip(sc.cases(), exp):
            out.append((cat, parity, m, sig, slot_of[parity][pk], ok))
    good = [c for c in sc.cases() if c[0] == "valid"][:6]
    for j, (_, pk, m, sig) in enumerate(good):
        out.append(("no_slot", j % 2, m, sig, (out_of_range_slot(), NO_SLOT, out_of_range_slot() + 64)[j % 3], 0))
    return out


def is_live(item):
    keys, _, valid = registry()
    _, _, _, sig, slot, _ = item
    return slot < len(keys) and valid[slot] == 1 and int.from_bytes(sig[:32], "big") < P and int.from_bytes(sig[32:], "big") < N


def arrays(its=None):
    its = items() if its is None else its
    return b"".join(i[2] for i in its), b"".join(i[3] for i in its), [i[4] for i in its], bytes(i[5] for i in its)


def generic_arrays(its=None):
    """(pks, msgs, sigs) of the same items for sbv_secp256k1_schnorr_verify: pk = the slot's Qx; items without a slot are left out"""
    keys = registry()[0]
    its = [i for i in (items() if its is None else its) if i[4] < len(keys)]
    return b"".join(keys[i[4]][:32] for i in its), b"".join(i[2] for i in its), b"".join(i[3] for i in its), bytes(i[5] for i in its)


# ---- widened slots and the batch order that makes the four wavefront compositions ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def steer_key():
    """(pk, d) of the key the range and edge cases of the generic set hang on: d G = lift_x(pk), the even registration"""
    pk = next(c[1] for c in sc.cases() if c[0] == "s_zero")
    rec = next(rec for rec, px, ok in sc.expanded() if ok and px == pk)
    return pk, int.from_bytes(rec[:32], "big")


@functools.lru_cache(maxsize=None)
def wide_slots():
    """three slots to widen: both registrations of the steering key and the even one of the first valid case's key"""
    _, slot_of, _ = registry()
    pk0 = steer_key()[0]
    pk1 = next(c[1] for c in sc.cases() if c[0] == "valid" and c[1] != pk0)
    return [slot_of[0][pk0], slot_of[1][pk0], slot_of[0][pk1]]


@functools.lru_cache(maxsize=None)
def wide_batch():
    """the items ordered for a registry whose wide_slots() own 16-bit combs: wavefront 0 all live and wide; wavefront 1 one live narrow
    lane among 63 wide (the wavefront stays narrow); wavefront 2 one dead lane among 63 wide (wide; the dead lane walks comb 0);
    wavefront 3 no live lane; then every item in its own order"""
    its = items()
    W = set(wide_slots())
    lw = [i for i in its if is_live(i) and i[4] in W]
    ln = [i for i in its if is_live(i) and i[4] not in W]
    dead = [i for i in its if not is_live(i)]
    dead_wide = [i for i in dead if i[4] in W]                      # r >= p or s >= n against a widened slot
    assert len(lw) >= 12 and ln and len(dead) >= 30 and dead_wide and any(i[5] for i in lw) and any(not i[5] for i in lw)
    cyc = lambda k, off: [lw[(off + j) % len(lw)] for j in range(k)]
    w0 = cyc(WAVE, 0)
    w1 = cyc(WAVE - 1, 5)
    w1.insert(17, ln[0])
    w2 = cyc(WAVE - 1, 9)
    w2.insert(40, dead_wide[0])
    w3 = [dead[(7 * j) % len(dead)] for j in range(WAVE)]
    return w0 + w1 + w2 + w3 + list(its)


def wide_lanes(its, widened):
    """lanes that take the 16-bit walk when `widened` slots own one: whole wavefronts with a live lane and no live narrow lane"""
    W, total = set(widened), 0
    for w0 in range(0, len(its), WAVE):
        wave = its[w0:w0 + WAVE]
        live = [i for i in wave if is_live(i)]
        if live and all(i[4] in W for i in live):
            total += len(wave)
    return total


def tiled(n, shift=0):
    """n items made of items(), tile t rotated by shift + 7 t: (msgs, sigs, slots, ok)"""
    its = items()
    m = len(its)
    out, t = [], 0
    while len(out) < n:
        rot = (shift + 7 * t) % m
        out += its[rot:] + its[:rot]
        t += 1
    return arrays(out[:n])


# ---- the walk cases of the debug op: u1 G + u2 Q_slot ---------------------------------------------------------------------------------
def first_term_8(u2):
    """the first non-zero term of k256_qphase_point's walk of u2, as a signed multiple of Q: a scalar with its top bit set is walked
    as n - u2 with every sign flipped; digit j = byte j of (u2 + 0x80..80) - 0x80, window 32 = the carry"""
    flip = u2 >> 255
    v = N - u2 if flip else u2
    k = v + int.from_bytes(b"\x80" * 32, "big")
    for j in range(33):
        d = (k >> 256) if j == 32 else ((k >> (8 * j)) & 0xFF) - 0x80
        if d:
            return (-d if flip else d) << (8 * j)
    return 0


def first_term_16(u2):
    """the same for the 16-bit comb (gcomb_recode: no flip; digit j = window j of (u2 + sum 2^(16 j + 15)) - 2^15)"""
    k = u2 + sum(1 << (16 * j + 15) for j in range(17))
    for j in range(17):
        d = ((k >> (16 * j)) & 0xFFFF) - 0x8000
        if d:
            return d << (16 * j)
    return 0


def digits_sum_8(u2):
    """all of the 8-bit walk's terms added up: must be u2 mod n (the CPU tier checks it)"""
    flip = u2 >> 255
    v = N - u2 if flip else u2
    k = v + int.from_bytes(b"\x80" * 32, "big")
    tot = sum((((k >> (8 * j)) & 0xFF) - 0x80) << (8 * j) for j in range(32)) + ((k >> 256) << 256)
    return (-tot if flip else tot) % N


CARRY_EDGE = int.from_bytes(b"\x7f" * 31 + b"\x80", "big")       # the smallest scalar whose 8-bit recoding carries into window 32
CARRY_ALL = int.from_bytes(b"\x7f" + b"\x80" * 31, "big")        # every byte at the threshold: each digit carries into the next


@functools.lru_cache(maxsize=None)
def walk_scalars():
    """[(label, u1, u2, parity)] for the steering key's slots: parity 0 = Q = d G, parity 1 = Q = -d G"""
    import random
    rng = random.Random(0x5340)
    _, d = steer_key()
    out = []
    edge = [0, 1, 2, N - 2, N - 1, 2**255 - 1, 2**255]
    for parity in (0, 1):
        dq = d if parity == 0 else N - d
        for u1 in edge:
            for u2 in edge:
                out.append(("pairs", u1, u2, parity))
        for u2 in (2**255 - 1, 2**255, 2**255 + 1, N - 2**255):                        # either side of the flip
            out.append(("flip", rng.randrange(1, N), u2, parity))
        for u2 in (CARRY_EDGE - 1, CARRY_EDGE, CARRY_ALL, N - CARRY_EDGE, N - CARRY_ALL, N - CARRY_EDGE + 1):
            out.append(("carry", rng.randrange(1, N), u2, parity))
            out.append(("carry", 0, u2, parity))
        for u2 in (rng.randrange(1, N), rng.randrange(1, N), 1, N - 1, CARRY_ALL, 2**255):
            out.append(("cancel", (-u2 * dq) % N, u2, parity))                          # the sum is infinity
        for u2 in (rng.randrange(1, N), rng.randrange(1, N) | (1 << 255), rng.randrange(1, 2**190) << 64, CARRY_EDGE, CARRY_ALL, 2**255, 3):
            for t in (first_term_8(u2), first_term_16(u2)):
                out.append(("meet", (t * dq) % N, u2, parity))                           # the first key addition meets its own entry
                out.append(("back", (-t * dq) % N, u2, parity))                          # ... or takes the accumulator back to infinity
        for _ in range(4):
            out.append(("seeded", rng.randrange(1, N), rng.randrange(1, N), parity))
    return out


@functools.lru_cache(maxsize=None)
def walk_cases():
    """(input records, slots, expected output records, labels); the last cases name a slot out of range and an invalid slot"""
    _, slot_of, valid = registry()
    pk, d = steer_key()
    ins, slots, outs, labels = [], [], [], []
    for label, u1, u2, parity in walk_scalars():
        slot = slot_of[parity][pk]
        q = kp.pt_add(sc.gmul(u1), sc.mul(u2, point_of(slot)))
        ins.append(op_record(u1, u2))
        slots.append(slot)
        outs.append(op_result(0) if q is None else op_result(1, q[0], q[1]))
        labels.append(label)
    for slot in (out_of_range_slot(), NO_SLOT, valid.index(0)):
        ins.append(op_record(5, 7))
        slots.append(slot)
        outs.append(op_result(0))
        labels.append("dead")
    return ins, slots, outs, labels
