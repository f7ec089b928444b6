"""CPU tier for registered Ed25519 keys (include/sbv.h: sbv_ed25519_register_keys and the _keyed entries).

The keyed step's lanes (consensus_amd/csrc/ed25519_keyed.h) run lane by lane in tests/emul/ed_keyed_emul.cc — expand, G phase, keyed
Q phase with the wavefront ballot that picks the 16-bit combs, finish — against the golden vectors and the oracle; the C-ABI refuses
without a device; and the C++ Verifier routes Ed25519 consenter bursts and registered-client proposals through the keyed backend forms
(CPU stand-in backend)."""
import ctypes
import json
import os
import random
import subprocess

import pytest

import consensus_amd as sbv
import ed25519_py as ed

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
L = ed.L


@pytest.fixture(scope="module")
def kemul():
    src = os.path.join(HERE, "emul", "ed_keyed_emul.cc")
    so = os.path.join(HERE, "emul", "libsbv_ed_keyed_emul.so")
    csrc = os.path.join(HERE, "..", "consensus_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-misleading-indentation", "-DSBV_F25_CHECK",
                               src, "-o", so])
    lib = ctypes.CDLL(so)
    V, S = ctypes.c_void_p, ctypes.c_size_t
    lib.sbvk_verify_keyed.argtypes = [ctypes.c_char_p, V, S, ctypes.c_char_p, S, V, V, V]
    lib.sbvk_verify_keyed.restype = ctypes.c_ulong
    lib.sbvk_verify_msgs_keyed.argtypes = [ctypes.c_char_p, ctypes.c_char_p, V, V, S, ctypes.c_char_p, S, V]
    lib.sbvk_host_comb.argtypes = [ctypes.c_char_p, V]
    lib.sbvk_wide_mismatches.argtypes = [ctypes.c_char_p]
    lib.sbvk_wide_mismatches.restype = ctypes.c_long
    return lib


@pytest.fixture(scope="module")
def ed_vectors():
    return json.load(open(os.path.join(GOLDEN, "ed25519_vectors.json")))["vectors"]


def _bits(bm, n):
    return [bool((bm[i >> 3] >> (i & 7)) & 1) for i in range(n)]


def _registry(pks):
    """slot of every key: first appearance order, equal bytes share a slot (the library's rule)"""
    index, encs, slots = {}, [], []
    for pk in pks:
        if pk not in index:
            index[pk] = len(encs)
            encs.append(pk)
        slots.append(index[pk])
    return encs, slots


def _keyed(kemul, recs, slots, encs, widen=None):
    n = len(slots)
    bm = ctypes.create_string_buffer(max(1, (n + 7) // 8))
    sl = (ctypes.c_uint32 * max(1, n))(*slots)
    w = (ctypes.c_uint8 * len(encs))(*widen) if widen is not None else None
    wide_lanes = kemul.sbvk_verify_keyed(recs, sl, n, b"".join(encs), len(encs), w, bm, None)
    return _bits(bm.raw, n), wide_lanes


def _oracle_bits(oracle, tuples, n):
    oracle.sbvo_ed25519_verify_batch.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
    want = ctypes.create_string_buffer((n + 7) // 8)
    oracle.sbvo_ed25519_verify_batch(tuples, n, want, os.cpu_count() or 1)
    return _bits(want.raw, n)


def _rec(t):
    return t[:64] + t[96:128]


def test_golden_vectors_through_the_keyed_step(kemul, oracle, ed_vectors):
    """Every golden vector as a registered-key record: expand -> G -> keyed Q -> finish gives the file's verdict and the oracle's; the
    key that fails to decode lands on an invalid slot."""
    tuples = [ed.pack_tuple(bytes.fromhex(v["pk"]), bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"])) for v in ed_vectors]
    encs, slots = _registry([t[64:96] for t in tuples])
    got, _ = _keyed(kemul, b"".join(_rec(t) for t in tuples), slots, encs)
    want = [v["accept"] for v in ed_vectors]
    assert got == want, [v["name"] for v, g in zip(ed_vectors, got) if g != v["accept"]]
    assert got == _oracle_bits(oracle, b"".join(tuples), len(tuples))
    invalid = [e for e in encs if ed.decompress(e) is None]
    assert invalid, "the vector file holds a key that does not decode"
    tab = ctypes.create_string_buffer(4096 * 96)
    for e in invalid:
        assert kemul.sbvk_host_comb(e, tab) == 0
    assert kemul.sbvk_host_comb(encs[0], tab) == 1


def test_golden_vectors_through_the_keyed_front_end(kemul, ed_vectors):
    """The _msgs_keyed form: k hashed by the keyed front end lane from the registry's encoding."""
    vs = [v for v in ed_vectors if len(bytes.fromhex(v["sig"])) == 64]
    encs, slots = _registry([bytes.fromhex(v["pk"]) for v in vs])
    msgs = [bytes.fromhex(v["msg"]) for v in vs]
    offs = (ctypes.c_uint64 * (len(vs) + 1))()
    for i, m in enumerate(msgs):
        offs[i + 1] = offs[i] + len(m)
    bm = ctypes.create_string_buffer((len(vs) + 7) // 8)
    sl = (ctypes.c_uint32 * len(vs))(*slots)
    kemul.sbvk_verify_msgs_keyed(b"".join(bytes.fromhex(v["sig"]) for v in vs), b"".join(msgs) + b"\0", offs, sl, len(vs),
                                 b"".join(encs), len(encs), bm)
    assert _bits(bm.raw, len(vs)) == [v["accept"] for v in vs]


def test_random_batch_narrow_and_wide_combs_agree(kemul, oracle):
    """A generator batch over three keys plus out-of-range slots and S >= L / k >= L records: the oracle's verdicts (a reject for
    every bad record) with 8-bit combs, with every key widened, and with one key widened (mixed wavefronts)."""
    oracle.sbvo_ed25519_gen_batch.argtypes = [ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_int]
    n = 640
    tup = ctypes.create_string_buffer(128 * n)
    exp = ctypes.create_string_buffer((n + 7) // 8)
    oracle.sbvo_ed25519_gen_batch(0xED4E1, n, 3, 0, tup, exp, os.cpu_count() or 1)
    tuples = [bytearray(tup.raw[128 * i:128 * i + 128]) for i in range(n)]
    rng = random.Random(7)
    for i in range(0, n, 5):                      # a flipped bit of R or S: rejects over the three registered keys
        tuples[i][rng.randrange(64)] ^= 1 << rng.randrange(8)
    # a key that is no point, registered: its slot is invalid
    bad = next(bytes([b]) + bytes(31) for b in range(2, 256) if ed.decompress(bytes([b]) + bytes(31)) is None)
    for i in (577, 600):
        tuples[i][64:96] = bad
    encs, slots = _registry([bytes(t[64:96]) for t in tuples])
    assert len(encs) == 4
    want = _oracle_bits(oracle, b"".join(bytes(t) for t in tuples), n)
    assert any(want) and not all(want) and not want[577] and not want[600]
    # the last wavefront: out-of-range slots, S >= L, k >= L (all rejects); the others untouched
    for i in range(576, n):
        kind = i % 3
        if kind == 0:
            slots[i] = len(encs) + rng.randrange(1 << 20)
        elif kind == 1:
            tuples[i][32:64] = (L + rng.randrange(1 << 200)).to_bytes(32, "little")
        else:
            tuples[i][96:128] = (L + rng.randrange(1 << 200)).to_bytes(32, "little")
        want[i] = False
    recs = b"".join(_rec(bytes(t)) for t in tuples)
    narrow, wl = _keyed(kemul, recs, slots, encs)
    assert narrow == want and wl == 0
    wide, wl = _keyed(kemul, recs, slots, encs, widen=[1] * len(encs))
    assert wide == want
    assert wl == 576                              # every wavefront but the last (out-of-range and invalid slots have no comb)
    mixed, wl = _keyed(kemul, recs, slots, encs, widen=[1] + [0] * (len(encs) - 1))
    assert mixed == want and wl == 0


def test_wide_comb_of_the_device_builder_equals_the_host_reference(kemul, oracle):
    """ed_widetab_lane on a registry comb (the device builder of sbv_ed25519_widen_keys) = build_ed_window_of on -A at 16 bits, byte
    for byte; an encoding that is no point has no wide comb."""
    pk = ed.public_key(bytes(range(32)))
    assert kemul.sbvk_wide_mismatches(pk) == 0
    bad = next(bytes([b]) + bytes(31) for b in range(2, 256) if ed.decompress(bytes([b]) + bytes(31)) is None)
    assert kemul.sbvk_wide_mismatches(bad) == -1


def _has_gpu():
    try:
        return sbv.device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="only meaningful where no GPU is visible")
def test_every_new_entry_refuses_before_init():
    lib = sbv.load()
    out = ctypes.create_string_buffer(8)
    slot = (ctypes.c_uint32 * 1)()
    stats = (ctypes.c_uint32 * 4)()
    offs = (ctypes.c_uint64 * 2)(0, 3)
    V, S = ctypes.c_void_p, ctypes.c_size_t
    lib.sbv_ed25519_register_keys.argtypes = [ctypes.c_char_p, S, V]
    lib.sbv_ed25519_wide_keys.argtypes = [ctypes.c_uint32]
    lib.sbv_ed25519_widen_keys.argtypes = [V, S]
    lib.sbv_ed25519_wide_key_stats.argtypes = [V]
    lib.sbv_ed25519_wide_selfcheck.argtypes = [ctypes.c_uint32]
    lib.sbv_ed25519_verify_batch_keyed.argtypes = [ctypes.c_char_p, V, S, V]
    lib.sbv_ed25519_verify_batch_keyed_dev.argtypes = [V, V, S, V, V]
    lib.sbv_ed25519_verify_msgs_keyed.argtypes = [ctypes.c_char_p, ctypes.c_char_p, V, V, S, V]
    assert lib.sbv_ed25519_register_keys(bytes(32), 1, slot) == -5
    assert lib.sbv_ed25519_key_count() == -5
    assert lib.sbv_ed25519_clear_keys() == -5
    assert lib.sbv_ed25519_wide_keys(16) == -5
    assert lib.sbv_ed25519_widen_keys(slot, 1) == -5
    assert lib.sbv_ed25519_wide_key_stats(stats) == -5
    assert lib.sbv_ed25519_wide_selfcheck(0) == -5
    assert lib.sbv_ed25519_verify_batch_keyed(bytes(96), slot, 1, out) == -5
    assert lib.sbv_ed25519_verify_batch_keyed_dev(ctypes.addressof(out), ctypes.addressof(slot), 1, ctypes.addressof(out), None) == -5
    assert lib.sbv_ed25519_verify_msgs_keyed(bytes(64), b"abc", offs, slot, 1, out) == -5
    with pytest.raises(sbv.SbvError) as ei:
        sbv.ed25519_register_keys([bytes(32)])
    assert ei.value.code == -5
    with pytest.raises(sbv.SbvError) as ei:
        sbv.ed25519_verify_batch_keyed(bytes(96), [0])
    assert ei.value.code == -5


def test_verifier_routes_registered_ed25519_signers_through_the_keyed_forms(oracle):
    """Scheme::ED25519 over the CPU stand-in backend with a key registry: RegisterConsenter takes a slot and widens it, a 15-vote commit
    burst at N = 16 goes through verify_ed25519_keyed and an all-registered-client proposal through verify_ed25519_msgs_keyed, with the
    oracle's verdicts; a proposal with an unregistered client takes the generic tuples.  Slots are keyed by the encoding's bytes."""
    import hashlib

    import hostlib
    from hostlib import INVALID, OK
    from test_host_verifier import Harness, coalesced_burst
    lib = hostlib.load()
    lib.sbvh_backend_keyed_batches.restype = ctypes.c_uint64
    lib.sbvh_backend_keyed_batches.argtypes = [ctypes.c_void_p]
    lib.sbvh_backend_register_ed25519.restype = ctypes.c_long
    lib.sbvh_backend_register_ed25519.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    oracle.sbvo_ed25519_verify_batch.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
    hx = Harness(lib, oracle, n_nodes=16, scheme=1, backend_kind=2, wait_us=2000)
    try:
        assert lib.sbvh_backend_widened_keys(hx.v) == 16                   # every consenter's slot widened, no client's
        reqs = [hx.request("alice%d" % (i % 3), "r%d" % i, payload=bytes([i])) for i in range(100)]
        prop = (hostlib.payload_encode(reqs), b"h", b"m", 0)
        k0 = lib.sbvh_backend_keyed_batches(hx.v)
        hx.batches.clear()
        st, infos = hx.verify_proposal(prop)
        assert st == OK and len(infos) == 100 and hx.batches == [100]
        assert lib.sbvh_backend_keyed_batches(hx.v) == k0 + 1              # the registered-client proposal: verify_ed25519_msgs_keyed
        bad = list(reqs)
        bad[13] = hx.request("alice1", "r13", corrupt=True)
        assert hx.verify_proposal((hostlib.payload_encode(bad), b"h", b"m", 0))[0] == INVALID
        # the commit burst: 15 votes, one of them tampered
        sigs = [hx.sign_proposal(i, prop, b"") for i in range(1, 16)]
        sid, val, msg = sigs[6]
        sigs[6] = (sid, val[:10] + bytes([val[10] ^ 4]) + val[11:], msg)
        k1 = lib.sbvh_backend_keyed_batches(hx.v)
        res = coalesced_burst(hx, [lambda i=i: hx.verify_consenter_sig(sigs[i], prop)[0] for i in range(15)])
        assert res == [OK] * 6 + [INVALID] + [OK] * 8
        assert lib.sbvh_backend_keyed_batches(hx.v) > k1
        # an unregistered signer: a client added while device client keys are off has no slot -> the generic tuples
        lib.sbvh_set_device_client_keys(hx.v, 0)
        s = lib.sbvh_signer_new_scheme(1, 0, hashlib.sha256(b"late-ed-client").digest())
        q = ctypes.create_string_buffer(64)
        lib.sbvh_signer_public_key(s, q)
        lib.sbvh_register_client(hx.v, b"bob", q.raw)
        hx.clients["bob"] = s
        reqs[17] = hx.request("bob", "r17", payload=b"x")
        k2 = lib.sbvh_backend_keyed_batches(hx.v)
        hx.batches.clear()
        st, infos = hx.verify_proposal((hostlib.payload_encode(reqs), b"h", b"m", 0))
        assert st == OK and infos[17] == ("bob", "r17") and hx.batches == [100]
        assert lib.sbvh_backend_keyed_batches(hx.v) == k2
        # slot identity: bytes, not points (y = 1 and y = 1 + p both encode the identity)
        a1, a2 = (1).to_bytes(32, "little"), (1 + ed.P).to_bytes(32, "little")
        s1, s2 = lib.sbvh_backend_register_ed25519(hx.v, a1), lib.sbvh_backend_register_ed25519(hx.v, a2)
        assert s1 >= 0 and s2 >= 0 and s1 != s2 and lib.sbvh_backend_register_ed25519(hx.v, a1) == s1
    finally:
        hx.close()
    # a backend without a registry: the Ed25519 Verifier behaves as before (no slot, no keyed batch)
    plain = Harness(lib, oracle, n_nodes=4, scheme=1, backend_kind=1, wait_us=10)
    try:
        assert lib.sbvh_backend_register_ed25519(plain.v, bytes(32)) == -1
        assert lib.sbvh_backend_widened_keys(plain.v) == 0
        prop = (hostlib.payload_encode([plain.request("alice0", "r0")]), b"h", b"m", 0)
        assert plain.verify_proposal(prop)[0] == OK and lib.sbvh_backend_keyed_batches(plain.v) == 0
    finally:
        plain.close()
