"""GPU tier for registered Ed25519 keys (include/sbv.h: sbv_ed25519_register_keys and the _keyed entries) through the C-ABI:
verdicts against the golden vectors, the oracle, OpenSSL and the generic entry sbv_ed25519_verify_batch, narrow and widened."""
import ctypes
import json
import os

import pytest

import consensus_amd as sbv
import ed25519_py as ed

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gpu():
    sbv.init(0)
    sbv.ed25519_clear_keys()
    yield sbv
    sbv.ed25519_clear_keys()


def _gen(oracle, seed, n, nkeys, inv):
    oracle.sbvo_ed25519_gen_batch.argtypes = [ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_int]
    tup = ctypes.create_string_buffer(128 * n)
    exp = ctypes.create_string_buffer((n + 7) // 8)
    oracle.sbvo_ed25519_gen_batch(seed, n, nkeys, inv, tup, exp, os.cpu_count() or 1)
    return tup, exp


def _oracle(oracle, tup, n):
    oracle.sbvo_ed25519_verify_batch.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
    want = ctypes.create_string_buffer((n + 7) // 8)
    oracle.sbvo_ed25519_verify_batch(tup, n, want, os.cpu_count() or 1)
    return want.raw


def _records(tup, n):
    """128-byte tuples -> (n x 96 records R | S | k, the distinct encodings in first-seen order, slot of each tuple)"""
    import numpy as np
    t = np.frombuffer(tup, dtype=np.uint8, count=128 * n).reshape(n, 128)
    recs = np.ascontiguousarray(np.concatenate([t[:, :64], t[:, 96:]], axis=1)).tobytes()
    keys, inv = np.unique(t[:, 64:96], axis=0, return_inverse=True)
    first = np.full(len(keys), n, dtype=np.int64)
    np.minimum.at(first, inv.reshape(-1), np.arange(n))
    order = np.argsort(first)
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    encs = [keys[k].tobytes() for k in order]
    return recs, encs, rank[inv.reshape(-1)].astype(np.uint32)


def _keyed_host(recs, slots, n):
    out = ctypes.create_string_buffer((n + 7) // 8)
    lib = sbv.load()
    lib.sbv_ed25519_verify_batch_keyed.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    sbv._check(lib.sbv_ed25519_verify_batch_keyed(recs, slots.ctypes.data, n, out))
    return out.raw


def test_golden_vectors_keyed_and_msgs_keyed(gpu):
    vs = json.load(open(os.path.join(GOLDEN, "ed25519_vectors.json")))["vectors"]
    tuples = [ed.pack_tuple(bytes.fromhex(v["pk"]), bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"])) for v in vs]
    gpu.ed25519_clear_keys()
    slots = gpu.ed25519_register_keys([t[64:96] for t in tuples])
    got = sbv.bitmap_to_list(gpu.ed25519_verify_batch_keyed(b"".join(t[:64] + t[96:] for t in tuples), slots), len(vs))
    assert got == [v["accept"] for v in vs], [v["name"] for v, g in zip(vs, got) if g != v["accept"]]
    m = [i for i, v in enumerate(vs) if len(bytes.fromhex(v["sig"])) == 64]
    got = sbv.bitmap_to_list(gpu.ed25519_verify_msgs_keyed([bytes.fromhex(vs[i]["sig"]) for i in m], [bytes.fromhex(vs[i]["msg"]) for i in m],
                                                          [slots[i] for i in m]), len(m))
    assert got == [vs[i]["accept"] for i in m]
    # widened: the same verdicts; every widened slot's comb equals the host builder's
    gpu.ed25519_widen_keys(sorted(set(slots)))
    got = sbv.bitmap_to_list(gpu.ed25519_verify_batch_keyed(b"".join(t[:64] + t[96:] for t in tuples), slots), len(vs))
    assert got == [v["accept"] for v in vs]
    wide = gpu.ed25519_wide_key_stats()
    assert wide[0] > 0 and wide[1] == 16 and wide[3] == 65536


def test_slot_rules_and_bookkeeping(gpu):
    """Slots by encoding bytes: two encodings of the identity (y = 1 and y = 1 + p) get two slots, the same bytes one; a signature
    R = [s]B verifies against both (k differs, [k]A does not).  Out-of-range slots and S >= L are rejects; clear_keys resets."""
    gpu.ed25519_clear_keys()
    assert gpu.ed25519_key_count() == 0
    a1 = (1).to_bytes(32, "little")
    a2 = (1 + ed.P).to_bytes(32, "little")
    s = [gpu.ed25519_register_keys([a1, a2, a1])[i] for i in range(3)]
    assert s[0] != s[1] and s[0] == s[2] and gpu.ed25519_key_count() == 2
    assert gpu.ed25519_register_keys([a2]) == [s[1]]
    S = 123456789
    R = ed.encode(ed.pt_mul(S, ed.decompress(bytes.fromhex("5866666666666666666666666666666666666666666666666666666666666666"))))
    msg = b"identity"
    rec = lambda a: R + S.to_bytes(32, "little") + ed.hram(R, a, msg).to_bytes(32, "little")
    got = sbv.bitmap_to_list(gpu.ed25519_verify_batch_keyed(rec(a1) + rec(a2) + rec(a1) + rec(a1), [s[0], s[1], 7, 1 << 31]), 4)
    assert got == [True, True, False, False]
    bad = R + (ed.L + S).to_bytes(32, "little") + ed.hram(R, a1, msg).to_bytes(32, "little")
    assert gpu.ed25519_verify_batch_keyed(bad, [s[0]]) == b"\x00"
    gpu.ed25519_clear_keys()
    assert gpu.ed25519_key_count() == 0
    assert gpu.ed25519_verify_batch_keyed(rec(a1), [0]) == b"\x00"           # no registry: every slot is out of range
    assert gpu.ed25519_register_keys([a2]) == [0]
    assert gpu.ed25519_verify_batch_keyed(rec(a2), [0]) == b"\x01"
    gpu.ed25519_clear_keys()


@pytest.mark.parametrize("n", [1, 15, 32, 33, 64, 65, 4097])
def test_ragged_sizes_match_oracle(gpu, oracle, n):
    tup, exp = _gen(oracle, 0xEDC0 + n, n, 5, 3)
    gpu.ed25519_clear_keys()
    recs, encs, slots = _records(tup.raw, n)
    assert list(gpu.ed25519_register_keys(encs)) == list(range(len(encs)))
    want = _oracle(oracle, tup.raw, n)
    assert _keyed_host(recs, slots, n) == want == gpu.ed25519_verify_batch(tup.raw, n)


@pytest.mark.parametrize("nkeys", [16, 1024])
def test_full_batch_narrow_then_widened(gpu, oracle, openssl_check, nkeys):
    """2^20 signatures over 16 / 1024 keys: the oracle's, OpenSSL's and sbv_ed25519_verify_batch's bitmap, with 8-bit combs and after
    widen_keys (16 keys: every slot wide; 1024: the first 64, the default cap); the device-pointer entry equals the host one."""
    import numpy as np
    import torch
    n = 1 << 20
    seed = 0xED16 + nkeys
    tup, _ = _gen(oracle, seed, n, nkeys, 0)
    # every 8th signature gets one bit of R | S flipped (the generator's own flips also hit keys: thousands of one-off encodings)
    t = np.frombuffer(tup, dtype=np.uint8).reshape(n, 128)
    idx = np.arange(7, n, 8)
    t[idx, (idx * 7919) % 64] ^= (1 << (idx % 8)).astype(np.uint8)
    gpu.ed25519_clear_keys()
    recs, encs, slots = _records(tup.raw, n)
    assert list(gpu.ed25519_register_keys(encs)) == list(range(len(encs)))
    want = _oracle(oracle, tup.raw, n)
    openssl_check.sbvssl_ed25519_verify_gen_batch.argtypes = [ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t,
                                                              ctypes.c_void_p, ctypes.c_int]
    ssl = ctypes.create_string_buffer(n // 8)
    openssl_check.sbvssl_ed25519_verify_gen_batch(seed, tup.raw, 0, n, ssl, os.cpu_count() or 1)
    assert want == ssl.raw and sum(bin(b).count("1") for b in want) == n - n // 8
    generic = ctypes.create_string_buffer(n // 8)
    sbv._check(sbv.load().sbv_ed25519_verify_batch(ctypes.addressof(tup), n, ctypes.addressof(generic)))
    assert generic.raw == want
    narrow = _keyed_host(recs, slots, n)
    assert narrow == want, [i for i in range(n // 8) if narrow[i] != want[i]][:8]
    gpu.ed25519_widen_keys(range(len(encs)))
    st = gpu.ed25519_wide_key_stats()
    assert st[0] == min(len(encs), 64) and len(encs) == nkeys
    wide = _keyed_host(recs, slots, n)
    assert wide == want, [i for i in range(n // 8) if wide[i] != want[i]][:8]
    # the device-pointer entry on device-resident records
    d_r = torch.frombuffer(bytearray(recs), dtype=torch.uint8).cuda()
    d_s = torch.from_numpy(slots.view(np.int32)).cuda()
    d_b = torch.zeros(n // 8, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream()
    gpu.ed25519_verify_batch_keyed_dev(d_r.data_ptr(), d_s.data_ptr(), n, d_b.data_ptr(), stream.cuda_stream)
    torch.cuda.synchronize()
    assert bytes(d_b.cpu().numpy().tobytes()) == want
    if nkeys == 16:
        for s in range(len(encs)):
            if ed.decompress(encs[s]) is not None:
                assert gpu.ed25519_wide_selfcheck(s), s
    gpu.ed25519_clear_keys()


def test_registry_grows_and_clears(gpu, oracle):
    """Registration in several calls grows the registry past its first allocation (64 slots) with the combs copied on the device;
    slots registered after clear_keys are valid."""
    n = 3000
    tup, _ = _gen(oracle, 0xED77, n, 150, 0)
    recs, encs, slots = _records(tup.raw, n)
    gpu.ed25519_clear_keys()
    for a in range(0, len(encs), 40):
        assert gpu.ed25519_register_keys(encs[a:a + 40]) == list(range(a, min(a + 40, len(encs))))
    gpu.ed25519_widen_keys([0, 1, 2])
    assert gpu.ed25519_key_count() == len(encs) > 64
    want = _oracle(oracle, tup.raw, n)
    assert _keyed_host(recs, slots, n) == want
    gpu.ed25519_clear_keys()
    assert gpu.ed25519_key_count() == 0 and gpu.ed25519_wide_key_stats()[0] == 0
    assert gpu.ed25519_register_keys(encs) == list(range(len(encs)))
    assert _keyed_host(recs, slots, n) == want
    gpu.ed25519_clear_keys()
