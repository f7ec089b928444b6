"""CPU tier for registered secp256k1 keys (include/sbv.h: sbv_secp256k1_register_keys and the _keyed entries).

The keyed step's lanes (consensus_amd/csrc/k256_keyed.h) run lane by lane in tests/emul/k256_keyed_emul.cc — the registry's chain /
rows / fill lanes, the wide-comb builder lanes, stage A on records, stage B with the wavefront ballot that picks the 16-bit combs —
against the golden vectors, the oracle and oracle/k256_py.py; the comb builders are compared byte for byte; and the C-ABI refuses
without a device."""
import ctypes
import hashlib
import json
import multiprocessing
import os
import random
import subprocess
import sys

import pytest

import consensus_amd as sbv

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
import k256_py as kc  # noqa: E402

THREADS = os.cpu_count() or 1
TAB_BYTES = 33 * 128 * 64


@pytest.fixture(scope="module")
def kemul():
    src = os.path.join(HERE, "emul", "k256_keyed_emul.cc")
    so = os.path.join(HERE, "emul", "libsbv_k256_keyed_emul.so")
    csrc = os.path.join(HERE, "..", "consensus_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-misleading-indentation", src, "-o", so])
    lib = ctypes.CDLL(so)
    V, S = ctypes.c_void_p, ctypes.c_size_t
    lib.sbvk256_verify_keyed.argtypes = [ctypes.c_char_p, V, S, ctypes.c_char_p, S, V, V, V]
    lib.sbvk256_verify_keyed.restype = ctypes.c_ulong
    lib.sbvk256_verify_msgs_keyed.argtypes = [ctypes.c_char_p, V, ctypes.c_char_p, V, V, S, ctypes.c_char_p, S, V]
    lib.sbvk256_tables.argtypes = [ctypes.c_char_p, V, V, V]
    lib.sbvk256_wide_mismatches.argtypes = [ctypes.c_char_p]
    lib.sbvk256_wide_mismatches.restype = ctypes.c_long
    return lib


@pytest.fixture(scope="module")
def koracle(oracle):
    oracle.sbvo_k256_verify_batch.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
    oracle.sbvo_k256_gen_batch.argtypes = [ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_int]
    return oracle


@pytest.fixture(scope="module")
def k256_vectors():
    return json.load(open(os.path.join(GOLDEN, "k256_vectors.json")))["vectors"]


def _bits(bm, n):
    return [bool((bm[i >> 3] >> (i & 7)) & 1) for i in range(n)]


def _registry(keys):
    """slot of every key: first appearance order, equal bytes share a slot (the library's rule)"""
    index, distinct, slots = {}, [], []
    for k in keys:
        if k not in index:
            index[k] = len(distinct)
            distinct.append(k)
        slots.append(index[k])
    return distinct, slots


def _keyed(kemul, recs, slots, keys, widen=None):
    n = len(slots)
    bm = ctypes.create_string_buffer(max(1, (n + 7) // 8))
    sl = (ctypes.c_uint32 * max(1, n))(*slots)
    w = (ctypes.c_uint8 * len(keys))(*widen) if widen is not None else None
    valid = ctypes.create_string_buffer(max(1, len(keys)))
    wide_lanes = kemul.sbvk256_verify_keyed(recs, sl, n, b"".join(keys), len(keys), w, bm, valid)
    return _bits(bm.raw, n), wide_lanes, list(valid.raw[:len(keys)])


def _key_is_point(k):
    x, y = int.from_bytes(k[:32], "big"), int.from_bytes(k[32:], "big")
    return x < kc.P and y < kc.P and kc.on_curve(x, y)


def _py_verify(t):
    return kc.verify_tuple(t)


def _py_verify_all(tuples):
    with multiprocessing.get_context("fork").Pool(THREADS) as pool:
        return pool.map(_py_verify, tuples, chunksize=64)


def test_golden_vectors_through_the_keyed_step(kemul, k256_vectors):
    """Every golden vector as a registered-key record, keys registered by first appearance: the file's verdict with 8-bit combs
    and with every valid slot widened; keys off the curve, with a coordinate >= p and (0, 0) land in invalid slots."""
    vs = k256_vectors
    assert len(vs) == 121
    tuples = [bytes.fromhex(v["tuple"]) for v in vs]
    want = [v["accept"] for v in vs]
    keys, slots = _registry([t[96:] for t in tuples])
    recs = b"".join(t[:96] for t in tuples)
    got, wl, valid = _keyed(kemul, recs, slots, keys)
    assert got == want, [v["name"] for v, g in zip(vs, got) if g != v["accept"]]
    assert wl == 0
    assert valid == [1 if _key_is_point(k) else 0 for k in keys]
    named = {v["name"]: slots[i] for i, v in enumerate(vs)}
    for name in ("q_off_curve_y_plus_1", "q_x_eq_p", "q_y_eq_p", "q_zero_zero"):
        assert valid[named[name]] == 0 and not got[[v["name"] for v in vs].index(name)], name
    # widened, a dozen slots at a time (35.7 MB each): a batch of the vectors that sign under them, all other slots narrow
    for a in range(0, len(keys), 12):
        idx = [i for i in range(len(vs)) if a <= slots[i] < a + 12]
        sub = keys[a:a + 12]
        got, wl, _ = _keyed(kemul, b"".join(tuples[i][:96] for i in idx), [slots[i] - a for i in idx], sub, widen=[1] * len(sub))
        assert got == [want[i] for i in idx], [vs[i]["name"] for i, g in zip(idx, got) if g != want[i]]
        assert wl > 0


def test_random_batch_equals_the_oracle_and_the_python_reference(kemul, koracle):
    """20 480 generator tuples over 13 keys with 1-in-3 corruptions: the emulated keyed bitmap equals the oracle's and k256_py's.  A
    corruption that altered key bytes registers the altered key as a slot of its own: no tuple is left out."""
    n = 20480
    tup = ctypes.create_string_buffer(160 * n)
    exp = ctypes.create_string_buffer(n // 8)
    koracle.sbvo_k256_gen_batch(0x6BE1, n, 13, 3, tup, exp, THREADS)
    want = ctypes.create_string_buffer(n // 8)
    koracle.sbvo_k256_verify_batch(tup, n, want, THREADS)
    assert want.raw == exp.raw
    tuples = [tup.raw[160 * i:160 * i + 160] for i in range(n)]
    keys, slots = _registry([t[96:] for t in tuples])
    assert len(keys) > 13
    got, wl, valid = _keyed(kemul, b"".join(t[:96] for t in tuples), slots, keys)
    want = _bits(want.raw, n)
    assert got == want, [i for i in range(n) if got[i] != want[i]][:8]
    assert any(want) and not all(want) and 0 in valid and wl == 0
    assert got == _py_verify_all(tuples)


def test_mixed_wavefronts_take_the_walk_the_ballot_rule_predicts(kemul, koracle):
    """Six wavefronts: all wide, all narrow, mixed, wide with dead lanes (bad slot, invalid key, s = 0), all dead, and a ragged wide
    tail.  The lanes that took the wide walk are those of the wavefronts whose live lanes all own a 16-bit comb; verdicts do not
    depend on the walk."""
    n = 5 * 64 + 17
    tup = ctypes.create_string_buffer(160 * n)
    exp = ctypes.create_string_buffer((n + 7) // 8)
    koracle.sbvo_k256_gen_batch(0x6BE2, n, 4, 0, tup, exp, THREADS)
    tuples = [bytearray(tup.raw[160 * i:160 * i + 160]) for i in range(n)]
    base, _ = _registry([bytes(t[96:]) for t in tuples])
    assert len(base) == 4
    invalid = base[0][:63] + bytes([base[0][63] ^ 1])
    keys = base + [invalid]                         # slots 0, 1: wide; 2, 3: narrow; 4: invalid (asked to widen: stays as it is)
    widen = [1, 1, 0, 0, 1]
    key_of = lambda i, pool: base[pool[i % len(pool)]]
    rng = random.Random(5)
    slots, want = [], []
    for i, t in enumerate(tuples):
        wave = i // 64
        pool = {0: (0, 1), 1: (2, 3), 2: (0, 2), 3: (0, 1), 4: (0, 1), 5: (1,)}[wave]
        d = None
        for j in range(n):                          # a generator tuple under the wanted key
            if bytes(tuples[(i + j) % n][96:]) == key_of(i, pool):
                d = bytes(tuples[(i + j) % n])
                break
        t[:] = d
        slot, ok = base.index(bytes(t[96:])), True
        if wave == 2 and i % 7 == 0:
            t[rng.randrange(96)] ^= 1 << rng.randrange(8)         # a live reject
            ok = False
        if wave == 3 and i % 4 == 1:
            slot, ok = 4 + rng.randrange(1, 1 << 20), False       # out of range
        if wave == 3 and i % 4 == 2:
            slot, ok = 4, False                                   # invalid key
        if wave == 3 and i % 4 == 3:
            t[32:64] = bytes(32)                                  # s = 0
            ok = False
        if wave == 4:
            slot, ok = (4, False) if i % 2 else (99, False)
        slots.append(slot); want.append(ok)
    recs = b"".join(bytes(t[:96]) for t in tuples)
    got, wl, valid = _keyed(kemul, recs, slots, keys, widen=widen)
    assert valid == [1, 1, 1, 1, 0]
    assert got == want
    assert wl == 64 + 64 + 17                       # waves 0, 3 and 5; wave 4 has no live lane and stays on the 8-bit walk
    narrow, wl0, _ = _keyed(kemul, recs, slots, keys)
    assert narrow == want and wl0 == 0
    everything, wl1, _ = _keyed(kemul, recs, slots, keys, widen=[1] * 5)
    assert everything == want and wl1 == 64 * 4 + 17


def test_the_three_builders_make_the_same_table(kemul, k256_vectors):
    """The registered slot's 8-bit comb from the chain / rows / fill lanes = the host builder's = the grouped step's lanes on the same
    key, byte for byte, for random keys, G, -G and the golden edge keys that are points; keys that are no points are refused by all
    three; the 16-bit comb of the device-builder lanes = the host builder's."""
    rng = random.Random(0x6B)
    pts = [kc.pt_mul(rng.randrange(1, kc.N), kc.G) for _ in range(8)] + [kc.G, kc.pt_neg(kc.G)]
    keys = [p[0].to_bytes(32, "big") + p[1].to_bytes(32, "big") for p in pts]
    edge = {bytes.fromhex(v["tuple"])[96:] for v in k256_vectors if v["class"] == "key"}
    keys += sorted(edge)
    assert any(not _key_is_point(k) for k in keys)
    a, b, c = (ctypes.create_string_buffer(TAB_BYTES) for _ in range(3))
    for k in keys:
        flags = kemul.sbvk256_tables(k, a, b, c)
        if not _key_is_point(k):
            assert flags == 0, k.hex()
            continue
        assert flags == 7, k.hex()
        assert a.raw == b.raw == c.raw, k.hex()
        # spot checks against the Python reference: entry (j, m) = m * 2^(8 j) * Q
        Q = (int.from_bytes(k[:32], "big"), int.from_bytes(k[32:], "big"))
        for j, m in ((0, 1), (0, 128), (7, 77), (31, 128), (32, 1)):
            e = kc.pt_mul(m << (8 * j), Q)
            o = (j * 128 + m - 1) * 64
            assert a.raw[o:o + 32] == e[0].to_bytes(32, "little") and a.raw[o + 32:o + 64] == e[1].to_bytes(32, "little"), (j, m)
        assert a.raw[(32 * 128 + 1) * 64:] == bytes(127 * 64)          # the carry window holds one entry
    for k in keys[:2] + keys[8:10]:
        assert kemul.sbvk256_wide_mismatches(k) == 0, k.hex()
    assert kemul.sbvk256_wide_mismatches(bytes(64)) == -1


def _der_int(v):
    b = v.to_bytes((v.bit_length() + 8) // 8 or 1, "big")
    return b"\x02" + bytes([len(b)]) + b


def _der(r, s):
    body = _der_int(r) + _der_int(s)
    return b"\x30" + bytes([len(body)]) + body


def test_msgs_keyed_front_end(kemul, golden_vectors):
    """Messages + DER signatures through the front end lane and the keyed step: honest secp256k1 signatures (both s), tampered ones,
    and the 28 golden DER classes as byte strings; the verdict is k256_py's on (SHA-256(msg), the strict parse).  Offset tables that
    do not start at 0 or decrease are refused."""
    ds = [1000 + 7 * i for i in range(3)]
    pts = [kc.pt_mul(d, kc.G) for d in ds]
    keys = [p[0].to_bytes(32, "big") + p[1].to_bytes(32, "big") for p in pts]
    msgs, ders, slots = [], [], []
    for i in range(30):
        m = b"keyed message %d" % i
        r, s = kc.sign(ds[i % 3], 777 + i, hashlib.sha256(m).digest())
        if i % 5 == 1:
            s = kc.N - s
        if i % 5 == 2:
            m += b"!"
        if i % 5 == 3:
            r = r % (kc.N - 1) + 1
        msgs.append(m); ders.append(_der(r, s)); slots.append(i % 3)
    der_vs = [v for v in golden_vectors if v["kind"] == "asn1" and v["class"] == "der"]
    assert len(der_vs) == 28
    r0, s0 = kc.sign(ds[0], 4242, hashlib.sha256(b"der").digest())
    for v in der_vs:
        msgs.append(b"der"); ders.append(bytes.fromhex(v["sig"])); slots.append(0)
    msgs.append(b"der"); ders.append(_der(r0, s0)); slots.append(0)
    msgs.append(b"der"); ders.append(_der(r0, s0) + b"\x00"); slots.append(0)          # trailing byte: strict parse refuses
    msgs.append(b""); ders.append(b""); slots.append(1)
    want = []
    for m, d, sl in zip(msgs, ders, slots):
        rs = sbv.parse_der(d)
        want.append(rs is not None and kc.verify_raw(int.from_bytes(rs[:32], "big"), int.from_bytes(rs[32:], "big"),
                                                     hashlib.sha256(m).digest(), pts[sl][0], pts[sl][1]))
    assert sum(want) >= 13 and want[-3] and not want[-2]
    n = len(msgs)

    def offs(parts):
        o = (ctypes.c_uint64 * (n + 1))()
        for i, p in enumerate(parts):
            o[i + 1] = o[i] + len(p)
        return o
    mo, so = offs(msgs), offs(ders)
    bm = ctypes.create_string_buffer((n + 7) // 8)
    sl = (ctypes.c_uint32 * n)(*slots)
    args = (b"".join(msgs) + b"\0", mo, b"".join(ders) + b"\0", so, sl, n, b"".join(keys), len(keys), bm)
    assert kemul.sbvk256_verify_msgs_keyed(*args) == 0
    assert _bits(bm.raw, n) == want
    bad = offs(msgs)
    bad[0] = 1
    assert kemul.sbvk256_verify_msgs_keyed(args[0], bad, *args[2:]) == -2
    bad = offs(ders)
    bad[5], bad[6] = bad[6], bad[5]
    assert kemul.sbvk256_verify_msgs_keyed(*args[:3], bad, *args[4:]) == -2


def _has_gpu():
    try:
        return sbv.device_count() > 0
    except Exception:
        return False


def test_every_new_symbol_is_exported_and_wrapped():
    lib = sbv.load()
    for name in ("register_keys", "key_count", "clear_keys", "wide_keys", "widen_keys", "wide_key_stats", "wide_selfcheck",
                 "verify_batch_keyed", "verify_batch_keyed_dev", "verify_msgs_keyed"):
        assert getattr(lib, "sbv_secp256k1_" + name) is not None
        assert callable(getattr(sbv, "secp256k1_" + name))
    hdr = open(os.path.join(HERE, "..", "include", "sbv.h")).read()
    assert hdr.count("int sbv_secp256k1_") == 12


@pytest.mark.skipif(_has_gpu(), reason="only meaningful where no GPU is visible")
def test_every_new_entry_refuses_without_a_device():
    lib = sbv.load()
    assert lib.sbv_init(0) == -1                    # SBV_ENODEV: after it every entry refuses as its siblings do
    out = ctypes.create_string_buffer(8)
    slot = (ctypes.c_uint32 * 1)()
    stats = (ctypes.c_uint32 * 4)()
    offs = (ctypes.c_uint64 * 2)(0, 3)
    V, S = ctypes.c_void_p, ctypes.c_size_t
    lib.sbv_secp256k1_register_keys.argtypes = [ctypes.c_char_p, S, V]
    lib.sbv_secp256k1_wide_keys.argtypes = [ctypes.c_uint32]
    lib.sbv_secp256k1_widen_keys.argtypes = [V, S]
    lib.sbv_secp256k1_wide_key_stats.argtypes = [V]
    lib.sbv_secp256k1_wide_selfcheck.argtypes = [ctypes.c_uint32]
    lib.sbv_secp256k1_verify_batch_keyed.argtypes = [ctypes.c_char_p, V, S, V]
    lib.sbv_secp256k1_verify_batch_keyed_dev.argtypes = [V, V, S, V, V]
    lib.sbv_secp256k1_verify_msgs_keyed.argtypes = [ctypes.c_char_p, V, ctypes.c_char_p, V, V, S, V]
    sibling = lib.sbv_secp256k1_verify_batch(bytes(160), 1, out)
    assert sibling == -5
    assert lib.sbv_secp256k1_register_keys(bytes(64), 1, slot) == sibling
    assert lib.sbv_secp256k1_key_count() == sibling
    assert lib.sbv_secp256k1_clear_keys() == sibling
    assert lib.sbv_secp256k1_wide_keys(16) == sibling
    assert lib.sbv_secp256k1_widen_keys(slot, 1) == sibling
    assert lib.sbv_secp256k1_wide_key_stats(stats) == sibling
    assert lib.sbv_secp256k1_wide_selfcheck(0) == sibling
    assert lib.sbv_secp256k1_verify_batch_keyed(bytes(96), slot, 1, out) == sibling
    assert lib.sbv_secp256k1_verify_batch_keyed_dev(ctypes.addressof(out), ctypes.addressof(slot), 1, ctypes.addressof(out), None) == sibling
    assert lib.sbv_secp256k1_verify_msgs_keyed(b"abc", offs, b"\x30\x00\x00", offs, slot, 1, out) == sibling
    with pytest.raises(sbv.SbvError) as ei:
        sbv.secp256k1_register_keys([bytes(64)])
    assert ei.value.code == -5
    with pytest.raises(sbv.SbvError) as ei:
        sbv.secp256k1_verify_batch_keyed(bytes(96), [0])
    assert ei.value.code == -5


def test_verifier_routes_registered_secp256k1_signers_through_the_keyed_forms(oracle):
    """Scheme::SECP256K1 over the CPU stand-in backend with a key registry: RegisterConsenter takes a slot of the curve's registry and
    widens it; a 15-vote commit burst at N = 16 goes through verify_k256_keyed with the consenters' slots, an all-registered-client
    proposal through verify_k256_msgs_keyed with the clients' slots, a proposal with one unregistered client through the generic
    tuples, and a backend whose keyed virtuals answer -2 takes the generic tuples throughout.  The verdicts are the same in all four."""
    import hostlib
    from hostlib import INVALID, OK
    from test_host_verifier import Harness, coalesced_burst
    lib = hostlib.load()
    lib.sbvh_backend_keyed_batches.restype = ctypes.c_uint64
    lib.sbvh_backend_keyed_batches.argtypes = [ctypes.c_void_p]
    lib.sbvh_backend_register_k256.restype = ctypes.c_long
    lib.sbvh_backend_register_k256.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    lib.sbvh_backend_last_k256_slots.restype = ctypes.c_size_t
    lib.sbvh_backend_last_k256_slots.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    oracle.sbvo_k256_verify_batch.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]

    def last_slots(hx):
        buf = (ctypes.c_uint32 * 4096)()
        n = lib.sbvh_backend_last_k256_slots(hx.v, buf, 4096)
        return list(buf[:n])

    def pubkey(signer):
        q = ctypes.create_string_buffer(64)
        lib.sbvh_signer_public_key(signer, q)
        return q.raw

    def scenario(hx, keyed):
        """-> (verdicts, keyed batches seen per step)"""
        out, seen = [], []
        reqs = [hx.request("alice%d" % (i % 3), "r%d" % i, payload=bytes([i])) for i in range(100)]
        prop = (hostlib.payload_encode(reqs), b"h", b"m", 0)
        k = lib.sbvh_backend_keyed_batches(hx.v)
        hx.batches.clear()
        st, infos = hx.verify_proposal(prop)
        out.append((st, len(infos), list(hx.batches)))
        seen.append(lib.sbvh_backend_keyed_batches(hx.v) - k)
        if keyed:
            want = [lib.sbvh_backend_register_k256(hx.v, pubkey(hx.clients["alice%d" % (i % 3)])) for i in range(100)]
            assert min(want) >= 0 and last_slots(hx) == want
        bad = list(reqs)
        bad[13] = hx.request("alice1", "r13", corrupt=True)
        out.append(hx.verify_proposal((hostlib.payload_encode(bad), b"h", b"m", 0))[0])
        # the commit burst: 15 votes, one of them tampered
        sigs = [hx.sign_proposal(i, prop, b"") for i in range(1, 16)]
        sid, val, msg = sigs[6]
        sigs[6] = (sid, val[:10] + bytes([val[10] ^ 4]) + val[11:], msg)
        k = lib.sbvh_backend_keyed_batches(hx.v)
        out.append(coalesced_burst(hx, [lambda i=i: hx.verify_consenter_sig(sigs[i], prop)[0] for i in range(15)]))
        seen.append(lib.sbvh_backend_keyed_batches(hx.v) - k)
        if keyed:
            node_slot = {lib.sbvh_backend_register_k256(hx.v, pubkey(hx.nodes[i])) for i in range(1, 16)}
            ls = last_slots(hx)                         # the last backend batch of the burst: one slot per vote, each a voter's, none twice
            assert len(node_slot) == 15 and len(ls) == hx.batches[-1] and len(set(ls)) == len(ls) and set(ls) <= node_slot
            if len(hx.batches) == 1:
                assert sorted(ls) == sorted(node_slot)
        # one unregistered client: added while device client keys are off, it has no slot -> the generic tuples
        lib.sbvh_set_device_client_keys(hx.v, 0)
        s = lib.sbvh_signer_new_scheme(2, 0, hashlib.sha256(b"late-k256-client").digest())
        lib.sbvh_register_client(hx.v, b"bob", pubkey(s))
        hx.clients["bob"] = s
        reqs[17] = hx.request("bob", "r17", payload=b"x")
        k = lib.sbvh_backend_keyed_batches(hx.v)
        hx.batches.clear()
        st, infos = hx.verify_proposal((hostlib.payload_encode(reqs), b"h", b"m", 0))
        out.append((st, infos[17], list(hx.batches)))
        seen.append(lib.sbvh_backend_keyed_batches(hx.v) - k)
        return out, seen

    hx = Harness(lib, oracle, n_nodes=16, scheme=2, backend_kind=2, wait_us=2000)
    try:
        assert lib.sbvh_backend_widened_keys(hx.v) == 16                   # every consenter's slot widened, no client's
        keyed_out, seen = scenario(hx, True)
        assert seen[0] == 1 and seen[1] >= 1 and seen[2] == 0, seen
        # slots are keyed by the 64 key bytes, and the registry is not the P-256 one
        q = pubkey(hx.nodes[0])
        assert lib.sbvh_backend_register_k256(hx.v, q) == lib.sbvh_backend_register_k256(hx.v, q) >= 0
    finally:
        hx.close()
    # a backend whose keyed virtuals answer "unsupported" (-2, no registry): the old path, the same verdicts
    plain = Harness(lib, oracle, n_nodes=16, scheme=2, backend_kind=1, wait_us=2000)
    try:
        assert lib.sbvh_backend_register_k256(plain.v, bytes(64)) == -1 and lib.sbvh_backend_widened_keys(plain.v) == 0
        plain_out, seen = scenario(plain, False)
        assert seen == [0, 0, 0]
    finally:
        plain.close()
    assert keyed_out == plain_out
    assert keyed_out[0] == (OK, 100, [100]) and keyed_out[1] == INVALID and keyed_out[2] == [OK] * 6 + [INVALID] + [OK] * 8
    assert keyed_out[3] == (OK, ("bob", "r17"), [100])


@pytest.mark.parametrize("backend_kind", [1, 2])
def test_decision_replay_under_secp256k1_takes_the_keyed_records(oracle, backend_kind):
    """VerifyConsenterSigBatch under Scheme::SECP256K1 over 40 decisions x Q signatures of a 7-node cluster with every 7th signature
    spoiled (flipped value byte, unknown signer, message bound to another proposal, another consenter's signature under this
    signer's ID): no spoiled one accepted, no honest one rejected.  With a registry (kind 2) the batch is ONE verify_k256_keyed call
    whose pre-rejected entries carry slot 0xFFFFFFFF and whose other slots are the consenters'; without one (kind 1) it is the
    generic tuples, with the same verdicts."""
    import hostlib
    from test_host_verifier import Harness
    lib = hostlib.load()
    lib.sbvh_backend_keyed_batches.restype = ctypes.c_uint64
    lib.sbvh_backend_keyed_batches.argtypes = [ctypes.c_void_p]
    lib.sbvh_backend_register_k256.restype = ctypes.c_long
    lib.sbvh_backend_register_k256.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    lib.sbvh_backend_last_k256_slots.restype = ctypes.c_size_t
    lib.sbvh_backend_last_k256_slots.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    oracle.sbvo_k256_verify_batch.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
    hx = Harness(lib, oracle, scheme=2, wait_us=200, backend_kind=backend_kind)
    try:
        counts = (ctypes.c_uint64 * 4)()
        k0 = lib.sbvh_backend_keyed_batches(hx.v)
        hx.batches.clear()
        assert lib.sbvh_batch_faults(hx.v, 7, 40, 4, counts) == 0
        spoiled, spoiled_accepted, honest, honest_rejected = list(counts)
        n = 40 * 5                                                         # Q = 5 at N = 7
        assert spoiled == len([i for i in range(n) if i % 7 == 3]) and honest == n - spoiled
        assert spoiled_accepted == 0 and honest_rejected == 0
        assert hx.batches == [n]
        if backend_kind == 2:
            assert lib.sbvh_backend_keyed_batches(hx.v) == k0 + 1
            buf = (ctypes.c_uint32 * 4096)()
            m = lib.sbvh_backend_last_k256_slots(hx.v, buf, 4096)
            slots = list(buf[:m])
            assert m == n
            pre = [x for x in slots if x == 0xFFFFFFFF]
            assert 0 < len(pre) < spoiled                                  # unknown signers and unbound messages; the others reach the curve
            assert len({x for x in slots if x != 0xFFFFFFFF}) == 7         # the seven consenters' slots
        else:
            assert lib.sbvh_backend_keyed_batches(hx.v) == 0
    finally:
        hx.close()
