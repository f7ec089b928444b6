"""GPU tier for registered secp256k1 keys (include/sbv.h: sbv_secp256k1_register_keys and the _keyed entries) through the C-ABI:
verdicts against the golden vectors, the oracle, OpenSSL (NID_secp256k1) and the generic entry sbv_secp256k1_verify_batch, narrow
and widened.  Every comparison is exact."""
import ctypes
import hashlib
import json
import os
import sys
import time

import pytest

import consensus_amd as sbv

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
THREADS = os.cpu_count() or 1
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))


@pytest.fixture(scope="module")
def gpu():
    sbv.init(0)
    sbv.secp256k1_clear_keys()
    t0 = time.perf_counter()
    yield sbv
    sbv.secp256k1_clear_keys()
    print(f"\ntest_gpu_k256_keyed: {time.perf_counter() - t0:.0f} s of wall time")


@pytest.fixture(scope="module")
def koracle(oracle):
    oracle.sbvo_k256_verify_batch.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
    oracle.sbvo_k256_gen_batch.argtypes = [ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_int]
    return oracle


def _gen(koracle, seed, n, nkeys, inv):
    tup = ctypes.create_string_buffer(160 * max(n, 1))
    exp = ctypes.create_string_buffer((n + 7) // 8 or 1)
    koracle.sbvo_k256_gen_batch(seed, n, nkeys, inv, tup, exp, THREADS)
    return tup, exp


def _oracle(koracle, tup, n):
    want = ctypes.create_string_buffer((n + 7) // 8 or 1)
    koracle.sbvo_k256_verify_batch(tup, n, want, THREADS)
    return want.raw[:(n + 7) // 8]


def _records(tup, n):
    """160-byte tuples -> (n x 96 records r | s | hash, the distinct keys in first-seen order, slot of each tuple).  A corruption
    that altered key bytes makes a key of its own: no tuple is left out."""
    import numpy as np
    t = np.frombuffer(tup, dtype=np.uint8, count=160 * n).reshape(n, 160)
    recs = np.ascontiguousarray(t[:, :96]).tobytes()
    if n == 0:
        return recs, [], np.zeros(0, dtype=np.uint32)
    keys, inv = np.unique(t[:, 96:], axis=0, return_inverse=True)
    first = np.full(len(keys), n, dtype=np.int64)
    np.minimum.at(first, inv.reshape(-1), np.arange(n))
    order = np.argsort(first)
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    return recs, [keys[k].tobytes() for k in order], rank[inv.reshape(-1)].astype(np.uint32)


def _keyed_host(recs, slots, n):
    out = ctypes.create_string_buffer((n + 7) // 8 or 1)
    lib = sbv.load()
    lib.sbv_secp256k1_verify_batch_keyed.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    sbv._check(lib.sbv_secp256k1_verify_batch_keyed(recs, slots.ctypes.data, n, out))
    return out.raw[:(n + 7) // 8]


def _der_int(v):
    b = v.to_bytes((v.bit_length() + 8) // 8 or 1, "big")
    return b"\x02" + bytes([len(b)]) + b


def _der(r, s):
    body = _der_int(r) + _der_int(s)
    return b"\x30" + bytes([len(body)]) + body


def test_golden_vectors_keyed_widened_and_msgs_keyed(gpu):
    """The 121 golden vectors through verify_batch_keyed with 8-bit combs and with every valid slot widened.  The vectors carry
    digests, not messages, so they cannot go through the message front end (it hashes what it is given): verify_msgs_keyed gets 42
    freshly signed messages with DER signatures instead — both s, tampered messages and r, DER that does not parse — judged by the
    construction, and malformed offset tables, which it must refuse with SBV_EINVAL."""
    import k256_py as kc
    vs = json.load(open(os.path.join(GOLDEN, "k256_vectors.json")))["vectors"]
    tuples = [bytes.fromhex(v["tuple"]) for v in vs]
    want = [v["accept"] for v in vs]
    gpu.secp256k1_clear_keys()
    slots = gpu.secp256k1_register_keys([t[96:] for t in tuples])
    recs = b"".join(t[:96] for t in tuples)
    got = sbv.bitmap_to_list(gpu.secp256k1_verify_batch_keyed(recs, slots), len(vs))
    assert got == want, [v["name"] for v, g in zip(vs, got) if g != v["accept"]]
    assert got == sbv.bitmap_to_list(gpu.secp256k1_verify_batch(b"".join(tuples)), len(vs))
    # widened: every valid slot (the cap is raised to hold them all), the same verdicts, every comb equal to the host builder's
    distinct = sorted(set(slots))
    gpu.secp256k1_wide_keys(len(distinct))
    try:
        gpu.secp256k1_widen_keys(distinct)
        wide = gpu.secp256k1_wide_key_stats()
        key_of_slot = {sl: t[96:] for sl, t in zip(slots, tuples)}
        points = [sl for sl in distinct if int.from_bytes(key_of_slot[sl][:32], "big") < kc.P and int.from_bytes(key_of_slot[sl][32:], "big") < kc.P
                  and kc.on_curve(int.from_bytes(key_of_slot[sl][:32], "big"), int.from_bytes(key_of_slot[sl][32:], "big"))]
        assert 0 < len(points) < len(distinct)
        assert wide == (len(points), 16, len(distinct), 17 * 32768 * 64 // 1024)       # every valid distinct key, no invalid one
        got = sbv.bitmap_to_list(gpu.secp256k1_verify_batch_keyed(recs, slots), len(vs))
        assert got == want, [v["name"] for v, g in zip(vs, got) if g != v["accept"]]
        for sl in distinct:
            if sl in points:
                if sl in points[:6]:                                       # the full-batch test checks every widened slot; a few here
                    assert gpu.secp256k1_wide_selfcheck(sl), sl
            else:
                with pytest.raises(sbv.SbvError):
                    gpu.secp256k1_wide_selfcheck(sl)                       # an invalid slot stays as it is: no wide comb
    finally:
        gpu.secp256k1_wide_keys(0)
        gpu.secp256k1_wide_keys(64)
    assert gpu.secp256k1_wide_key_stats()[0] == 0
    # the message front end: fresh signatures over messages (the vectors carry digests, not messages), DER-encoded
    gpu.secp256k1_clear_keys()
    msgs, ders, sl, exp = [], [], [], []
    keys = [kc.pt_mul(1000 + 7 * i, kc.G) for i in range(3)]
    slot_of = gpu.secp256k1_register_keys([kc.make_tuple(1, 1, bytes(32), Q)[96:] for Q in keys])
    for i in range(40):
        m = b"keyed message %d" % i
        d = 1000 + 7 * (i % 3)
        r, s = kc.sign(d, 12345 + i, hashlib.sha256(m).digest())
        ok = True
        if i % 5 == 1:
            s = kc.N - s                      # the other valid s: ECDSA accepts it
        if i % 5 == 2:
            m += b"!"
            ok = False
        if i % 5 == 3:
            r = (r + 1) % kc.N or 1
            ok = False
        msgs.append(m); ders.append(_der(r, s)); sl.append(slot_of[i % 3]); exp.append(ok)
    msgs.append(b"short"); ders.append(b"\x30\x00"); sl.append(slot_of[0]); exp.append(False)      # DER that does not parse
    msgs.append(b""); ders.append(b""); sl.append(slot_of[0]); exp.append(False)
    assert sbv.bitmap_to_list(gpu.secp256k1_verify_msgs_keyed(msgs, ders, sl), len(msgs)) == exp
    # malformed offset tables are refused (SBV_EINVAL), whichever of the two tables it is
    lib = sbv.load()
    n = len(msgs)

    def offs(parts):
        o = (ctypes.c_uint64 * (n + 1))()
        for i, p in enumerate(parts):
            o[i + 1] = o[i] + len(p)
        return o

    def call(mo, so):
        out = ctypes.create_string_buffer((n + 7) // 8)
        arr = (ctypes.c_uint32 * n)(*sl)
        return lib.sbv_secp256k1_verify_msgs_keyed(b"".join(msgs) + b"\0", mo, b"".join(ders) + b"\0", so, arr, n, out), out.raw

    rc, bm = call(offs(msgs), offs(ders))
    assert rc == 0 and sbv.bitmap_to_list(bm, n) == exp
    for which in (0, 1):
        nonzero, decreasing = offs(msgs if which == 0 else ders), offs(msgs if which == 0 else ders)
        nonzero[0] = 1
        decreasing[5], decreasing[6] = decreasing[6], decreasing[5]
        assert decreasing[6] < decreasing[5]
        for bad in (nonzero, decreasing):
            rc, _ = call(bad, offs(ders)) if which == 0 else call(offs(msgs), bad)
            assert rc == -2, (which, rc)
    gpu.secp256k1_clear_keys()


def test_slot_rules_bookkeeping_and_the_other_curve(gpu, oracle, koracle):
    """Equal keys share a slot, slots are numbered by first registration, invalid keys get invalid slots, out-of-range slots reject
    without error, clear_keys restarts the numbering; a key registered in the P-256 registry too is judged by each entry on its
    own curve."""
    import k256_py as kc
    gpu.secp256k1_clear_keys()
    assert gpu.secp256k1_key_count() == 0
    n = 64
    tup, exp = _gen(koracle, 0x6B51, n, 2, 0)
    recs, keys, slots = _records(tup.raw, n)
    assert len(keys) == 2
    off_curve = keys[0][:63] + bytes([keys[0][63] ^ 1])
    big_x = (kc.P + 1).to_bytes(32, "big") + keys[0][32:]
    s = gpu.secp256k1_register_keys([keys[0], keys[1], keys[0], off_curve, bytes(64), big_x, keys[1]])
    assert s == [0, 1, 0, 2, 3, 4, 1] and gpu.secp256k1_key_count() == 5
    assert gpu.secp256k1_register_keys([big_x, keys[0]]) == [4, 0]
    assert _keyed_host(recs, slots, n) == exp.raw[:n // 8] == b"\xff" * (n // 8)
    import numpy as np
    for bad in (2, 3, 4, 5, 77, 1 << 31, 0xFFFFFFFF):          # invalid slots, then out-of-range ones: rejects, no error
        sl = slots.copy()
        sl[::2] = bad
        assert sbv.bitmap_to_list(_keyed_host(recs, sl, n), n) == [i % 2 == 1 for i in range(n)]
    swapped = (1 - slots.astype(np.int64)).astype(np.uint32)   # the other signer's slot
    assert _keyed_host(recs, swapped, n) == bytes(n // 8)
    # the same 64 bytes in the P-256 registry: its slot is an invalid P-256 key, and its numbering is its own
    gpu.clear_keys()
    pt, pe = ctypes.create_string_buffer(160 * n), ctypes.create_string_buffer(n // 8)
    oracle.sbvo_gen_batch.argtypes = [ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    oracle.sbvo_gen_batch(0x6B52, n, 1, 0, pt, pe, THREADS)
    pkey = pt.raw[96:160]
    assert gpu.register_keys([pkey, keys[0]]) == [0, 1]
    ks = gpu.secp256k1_register_keys([pkey])
    assert ks == [5]
    precs = b"".join(pt.raw[160 * i:160 * i + 96] for i in range(n))
    assert gpu.verify_batch_keyed(precs, [0] * n) == b"\xff" * (n // 8)             # P-256 signatures under the P-256 key
    assert gpu.verify_batch_keyed(recs, [1] * n) == bytes(n // 8)                   # secp256k1 signatures under the P-256 registry: rejects
    assert _keyed_host(precs, np.full(n, ks[0], dtype=np.uint32), n) == bytes(n // 8)   # P-256 signatures under this registry: rejects
    assert _keyed_host(recs, slots, n) == b"\xff" * (n // 8)
    gpu.clear_keys()
    gpu.secp256k1_clear_keys()
    assert gpu.secp256k1_key_count() == 0
    assert _keyed_host(recs, slots, n) == bytes(n // 8)        # no registry: every slot is out of range
    assert gpu.secp256k1_register_keys([keys[1], keys[0]]) == [0, 1]
    assert _keyed_host(recs, (1 - slots.astype(np.int64)).astype(np.uint32), n) == b"\xff" * (n // 8)
    with pytest.raises(sbv.SbvError) as ei:
        gpu.secp256k1_widen_keys([2])                          # unregistered
    assert ei.value.code == -2
    gpu.secp256k1_clear_keys()


@pytest.mark.parametrize("n", [0, 1, 7, 15, 63, 64, 65, 257, 1000, 20000])
def test_ragged_sizes_match_oracle(gpu, koracle, n):
    tup, exp = _gen(koracle, 0x6B00 + n, n, 13, 3)
    gpu.secp256k1_clear_keys()
    recs, keys, slots = _records(tup.raw, n)
    assert gpu.secp256k1_register_keys(keys) == list(range(len(keys)))
    want = exp.raw[:(n + 7) // 8]
    assert _keyed_host(recs, slots, n) == want
    assert gpu.secp256k1_verify_batch(tup.raw[:160 * n], n) == want
    if n >= 15:
        gpu.secp256k1_widen_keys(range(min(len(keys), 13)))     # mixed wavefronts: the corrupted keys' slots stay narrow
        assert _keyed_host(recs, slots, n) == want
    gpu.secp256k1_clear_keys()


@pytest.mark.parametrize("nkeys", [16, 1024])
def test_full_batch_narrow_then_widened(gpu, koracle, openssl_check, nkeys):
    """2^20 signatures over 16 / 1024 keys: the oracle's, OpenSSL's and sbv_secp256k1_verify_batch's bitmap, with 8-bit combs and
    after widen_keys (16 keys: every slot wide; 1024: the first 64, the default cap); the device-pointer entry on a caller stream
    equals the host one."""
    import numpy as np
    import torch
    n = 1 << 20
    tup, _ = _gen(koracle, 0x6B16 + nkeys, n, nkeys, 0)
    # every 8th signature gets one bit of r | s | hash flipped (the keys stay: exactly nkeys slots)
    t = np.frombuffer(tup, dtype=np.uint8, count=160 * n).reshape(n, 160)
    idx = np.arange(7, n, 8)
    t[idx, (idx * 7919) % 96] ^= (1 << (idx % 8)).astype(np.uint8)
    gpu.secp256k1_clear_keys()
    recs, keys, slots = _records(tup.raw, n)
    assert len(keys) == nkeys and gpu.secp256k1_register_keys(keys) == list(range(nkeys))
    want = _oracle(koracle, tup, n)
    openssl_check.sbvssl_k256_verify_batch.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
    ssl = ctypes.create_string_buffer(n // 8)
    openssl_check.sbvssl_k256_verify_batch(tup, n, ssl, THREADS)
    assert want == ssl.raw and sum(bin(b).count("1") for b in want) == n - n // 8
    kstats = gpu.key_cache_stats(sbv.SCHEME_SECP256K1)
    narrow = _keyed_host(recs, slots, n)
    assert narrow == want, [i for i in range(n // 8) if narrow[i] != want[i]][:8]
    assert gpu.key_cache_stats(sbv.SCHEME_SECP256K1) == kstats          # the keyed step has no grouping state
    assert gpu.secp256k1_verify_batch(tup.raw, n) == want
    gpu.secp256k1_widen_keys(range(nkeys))
    st = gpu.secp256k1_wide_key_stats()
    assert st == (min(nkeys, 64), 16, 64, 17 * 32768 * 64 // 1024)
    wide = _keyed_host(recs, slots, n)
    assert wide == want, [i for i in range(n // 8) if wide[i] != want[i]][:8]
    for s in range(st[0]):
        assert gpu.secp256k1_wide_selfcheck(s), s
    with pytest.raises(sbv.SbvError):
        gpu.secp256k1_wide_selfcheck(nkeys)                            # no wide comb
    # the device-pointer entry on device-resident records, on a stream of the caller's
    d_r = torch.frombuffer(bytearray(recs), dtype=torch.uint8).cuda()
    d_s = torch.from_numpy(slots.view(np.int32)).cuda()
    d_b = torch.zeros(n // 8, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        gpu.secp256k1_verify_batch_keyed_dev(d_r.data_ptr(), d_s.data_ptr(), n, d_b.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert bytes(d_b.cpu().numpy().tobytes()) == want
    # lowering the cap returns the slots beyond it to their 8-bit combs
    gpu.secp256k1_wide_keys(4)
    assert gpu.secp256k1_wide_key_stats()[0] == 4 and _keyed_host(recs, slots, n) == want
    gpu.secp256k1_wide_keys(64)
    gpu.secp256k1_clear_keys()


def test_dev_entry_small_batches_on_a_caller_stream(gpu, koracle):
    import numpy as np
    import torch
    gpu.secp256k1_clear_keys()
    stream = torch.cuda.Stream()
    for n in (15, 1000):
        tup, exp = _gen(koracle, 0x6BDE + n, n, 4, 3)
        recs, keys, slots = _records(tup.raw, n)
        gpu.secp256k1_register_keys(keys)
        slots = np.array(gpu.secp256k1_register_keys([tup.raw[160 * i + 96:160 * i + 160] for i in range(n)]), dtype=np.uint32)
        d_r = torch.frombuffer(bytearray(recs), dtype=torch.uint8).cuda()
        d_s = torch.from_numpy(slots.view(np.int32)).cuda()
        d_b = torch.zeros((n + 7) // 8, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            gpu.secp256k1_verify_batch_keyed_dev(d_r.data_ptr(), d_s.data_ptr(), n, d_b.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert bytes(d_b.cpu().numpy().tobytes()) == exp.raw[:(n + 7) // 8]
    gpu.secp256k1_clear_keys()


def test_registry_growth_and_isolation(gpu, oracle, koracle):
    """Registration in several calls grows the registry past 64, 128 and 256 slots with the combs copied on the device and every
    earlier slot still verifying; generic grouped secp256k1 batches and P-256 keyed batches in between leave every bitmap and the
    generic step's key-table-cache statistics as they were."""
    import numpy as np
    K = sbv.SCHEME_SECP256K1
    n = 6000
    tup, _ = _gen(koracle, 0x6B77, n, 300, 0)
    recs, keys, slots = _records(tup.raw, n)
    assert len(keys) == 300
    want = _oracle(koracle, tup, n)
    g, ge = _gen(koracle, 0x6B78, 1 << 13, 40, 5)              # a generic batch of other keys: grouped (the key-table cache is on)
    pn = 512
    pt, pe = ctypes.create_string_buffer(160 * pn), ctypes.create_string_buffer(pn // 8)
    oracle.sbvo_gen_batch.argtypes = [ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    oracle.sbvo_gen_batch(0x6B79, pn, 6, 4, pt, pe, THREADS)
    p = np.frombuffer(pt, dtype=np.uint8, count=160 * pn).reshape(pn, 160)
    gpu.clear_keys()
    pslots = gpu.register_keys([p[i, 96:].tobytes() for i in range(pn)])
    precs = np.ascontiguousarray(p[:, :96]).tobytes()
    gpu.secp256k1_clear_keys()
    seen = np.zeros(n, dtype=bool)
    for a in range(0, len(keys), 50):
        b = min(a + 50, len(keys))
        assert gpu.secp256k1_register_keys(keys[a:b]) == list(range(a, b))
        assert gpu.secp256k1_key_count() == b
        if a == 50:
            gpu.secp256k1_widen_keys([0, 1, 2])                  # wide combs survive the growth too
        # tuples whose slot exists so far verify; the others are out of range: rejects
        live = slots < b
        got = np.array(sbv.bitmap_to_list(_keyed_host(recs, slots, n), n))
        assert (got == (np.array(sbv.bitmap_to_list(want, n)) & live)).all(), a
        seen |= live
        assert gpu.secp256k1_verify_batch(g.raw, 1 << 13) == ge.raw
        before = gpu.key_cache_stats(K)
        assert _keyed_host(recs, slots, n) == bytes(np.packbits(got, bitorder="little"))
        assert gpu.key_cache_stats(K) == before
        assert gpu.verify_batch_keyed(precs, pslots) == pe.raw
    assert seen.all() and gpu.secp256k1_key_count() == 300 and gpu.secp256k1_wide_key_stats()[0] == 3
    assert _keyed_host(recs, slots, n) == want
    for s in (0, 1, 2):
        assert gpu.secp256k1_wide_selfcheck(s)
    gpu.secp256k1_clear_keys()
    gpu.clear_keys()
    assert gpu.secp256k1_key_count() == 0 and gpu.secp256k1_wide_key_stats()[0] == 0
    assert gpu.secp256k1_register_keys(keys) == list(range(len(keys)))
    assert _keyed_host(recs, slots, n) == want
    gpu.secp256k1_clear_keys()
