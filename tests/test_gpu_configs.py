"""GPU tier (`-m gpu`): every BASELINE.json config that has signatures in it, at its FULL size, through the C-ABI, with the
whole accept bitmap diffed against BOTH independent CPU opinions — the oracle (oracle/p256_oracle.c, the restatement of
Go's crypto/ecdsa rules) and OpenSSL's ECDSA_do_verify (oracle/openssl_check.c) — not against the generator's
by-construction flags only.

  configs[1]  2^20 tuples, 1024 keys, 7/8 valid                      (the headline batch)
  configs[2]  K = 10 000 request signatures of one proposal           (VerifyProposal, internal/bft/view.go:553-559)
  configs[3]  50 000 proposals x 11 consenter signatures = 550 000    (commit quorum at N = 16: internal/bft/util.go:183-187,
              per-proposal quorum = >= Q distinct valid signers, internal/bft/viewchanger.go:681-727)

Parity stays "partial" by the task's rule (the reference holds no vectors for this path and there is no Go toolchain
to run crypto/ecdsa here — DESIGN.md §3); what these tests establish is that the GPU agrees bit for bit with two
independent implementations of the same rules on every tuple of every config."""
import ctypes
import os

import pytest

import consensus_amd as sbv
import p256_py as ec

pytestmark = pytest.mark.gpu

THREADS = os.cpu_count() or 1


@pytest.fixture(scope="module")
def gpu():
    sbv.init(0)
    yield sbv
    sbv.shutdown()


def _gen(oracle, seed, n, nkeys, inv_every):
    tup = ctypes.create_string_buffer(160 * n)
    exp = ctypes.create_string_buffer((n + 7) // 8)
    oracle.sbvo_gen_batch(seed, n, nkeys, inv_every, tup, exp, THREADS)
    return tup, exp.raw[:(n + 7) // 8]


def _cpu_opinions(oracle, openssl_check, tup, n):
    openssl_check.sbvssl_p256_verify_batch.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
    a = ctypes.create_string_buffer((n + 7) // 8)
    b = ctypes.create_string_buffer((n + 7) // 8)
    oracle.sbvo_p256_verify_batch(ctypes.addressof(tup), n, ctypes.addressof(a), THREADS)
    openssl_check.sbvssl_p256_verify_batch(ctypes.addressof(tup), n, ctypes.addressof(b), THREADS)
    return a.raw, b.raw


def _gpu_bitmap(gpu, tup, n):
    got = ctypes.create_string_buffer((n + 7) // 8)
    gpu.verify_batch_ptr(ctypes.addressof(tup), n, ctypes.addressof(got))
    return got.raw


def _diff(a, b):
    return [i for i in range(len(a)) if a[i] != b[i]][:8]


def test_config1_full_2_20_bitmap_equals_oracle_and_openssl(gpu, oracle, openssl_check):
    n = 1 << 20
    tup, exp = _gen(oracle, 0x5B7F2026, n, 1024, 8)
    got = _gpu_bitmap(gpu, tup, n)
    assert got == exp, _diff(got, exp)
    ssl = ctypes.create_string_buffer(n // 8)
    openssl_check.sbvssl_p256_verify_batch.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
    openssl_check.sbvssl_p256_verify_batch(ctypes.addressof(tup), n, ctypes.addressof(ssl), THREADS)
    assert got == ssl.raw, _diff(got, ssl.raw)                       # every one of the 2^20 verdicts, independently
    # the oracle redoes a quarter of the batch (it is ~2x slower than OpenSSL's assembly)
    m = n // 4
    part = ctypes.create_string_buffer(m // 8)
    oracle.sbvo_p256_verify_batch(ctypes.addressof(tup), m, ctypes.addressof(part), THREADS)
    assert got[:m // 8] == part.raw
    # grouping switched off (all-distinct-keys kernel) must give the same 2^20 verdicts
    gpu.set_grouping(False)
    try:
        assert _gpu_bitmap(gpu, tup, n) == got
    finally:
        gpu.set_grouping(True)


@pytest.mark.parametrize("nkeys, inv_every", [(400, 8), (10000, 8), (64, 0)])
def test_config2_k_10000_request_signatures(gpu, oracle, openssl_check, nkeys, inv_every):
    """One proposal's K = 10 000 request signatures as VerifyProposal ships them (one batch): 400 clients (the default
    request pool size), every request from its own client, and the all-valid case a correct leader produces."""
    n = 10000
    tup, exp = _gen(oracle, 0xC2 + nkeys, n, nkeys, inv_every)
    got = _gpu_bitmap(gpu, tup, n)
    a, b = _cpu_opinions(oracle, openssl_check, tup, n)
    assert got == exp == a == b, (_diff(got, a), _diff(got, b))
    if inv_every == 0:
        assert got == b"\xff" * (n // 8)
    # the same signatures against registered client keys (what the host Verifier does after RegisterClient)
    if nkeys <= 400:
        raw = tup.raw
        keys = sorted({raw[160 * i + 96:160 * i + 160] for i in range(n)})
        gpu.clear_keys()
        slot_of = dict(zip(keys, gpu.register_keys(keys)))
        rsh = b"".join(raw[160 * i:160 * i + 96] for i in range(n))
        slots = [slot_of[raw[160 * i + 96:160 * i + 160]] for i in range(n)]
        assert gpu.verify_batch_keyed(rsh, slots, n) == got
        gpu.clear_keys()


def test_config3_550000_consenter_signatures_and_quorum(gpu, oracle, openssl_check):
    """50 000 proposals x Q = 11 signatures, 16 consenter keys, ~1/8 of the signatures corrupted: full bitmap vs both CPU
    opinions through the generic entry (in-step key grouping) AND the registered-key entry, then the per-proposal quorum
    the commit path needs: a proposal is decided when >= Q - 1 = 10 foreign signatures verify (view.go:446, 531)."""
    P, Q = 50000, 11
    n = P * Q
    tup, exp = _gen(oracle, 0xC3, n, 16, 8)
    got = _gpu_bitmap(gpu, tup, n)
    a, b = _cpu_opinions(oracle, openssl_check, tup, n)
    assert got == exp, _diff(got, exp)
    assert got == a, _diff(got, a)
    assert got == b, _diff(got, b)
    raw = tup.raw
    # corrupted-key tuples carry single-bit variants of the 16 consenter keys: they get no slot (unknown signer -> reject)
    counts = {}
    for i in range(n):
        k = raw[160 * i + 96:160 * i + 160]
        counts[k] = counts.get(k, 0) + 1
    signer_keys = sorted(k for k, c in counts.items() if c > 1000)
    assert len(signer_keys) == 16
    gpu.clear_keys()
    slot_of = dict(zip(signer_keys, gpu.register_keys(signer_keys)))
    rsh = b"".join(raw[160 * i:160 * i + 96] for i in range(n))
    slots = [slot_of.get(raw[160 * i + 96:160 * i + 160], 0xFFFFFFFF) for i in range(n)]
    keyed = gpu.verify_batch_keyed(rsh, slots, n)
    assert keyed == got, _diff(keyed, got)          # a corrupted key is rejected by either form
    # ... and with the consenters' wide combs (sbv_p256_widen_keys, round 4: 13 + 16 additions), which is what a Verifier that
    # registered its consenters runs; then 11 of the 16 only: wavefronts of wide and of 8-bit slots side by side
    try:
        gpu.wide_keys(16, 64)
        gpu.widen_keys(list(slot_of.values()))
        assert gpu.wide_key_stats()[0] == 16
        wide = gpu.verify_batch_keyed(rsh, slots, n)
        assert wide == got, _diff(wide, got)
        gpu.wide_keys(16, 11)
        assert gpu.wide_key_stats()[0] == 11
        some = gpu.verify_batch_keyed(rsh, slots, n)
        assert some == got, _diff(some, got)
        gpu.wide_keys()                                  # the default: width by count — 16 keys get 20-bit combs
        gpu.widen_keys(list(slot_of.values()))
        assert gpu.wide_key_stats()[:2] == (16, 20)
        auto = gpu.verify_batch_keyed(rsh, slots, n)
        assert auto == got, _diff(auto, got)
    finally:
        gpu.wide_keys()
        gpu.clear_keys()
    bits = sbv.bitmap_to_list(got, n)
    want = sbv.bitmap_to_list(a, n)
    decided_gpu = sum(1 for p in range(P) if sum(bits[p * Q:(p + 1) * Q]) >= Q - 1)
    decided_cpu = sum(1 for p in range(P) if sum(want[p * Q:(p + 1) * Q]) >= Q - 1)
    assert decided_gpu == decided_cpu
    assert 0 < decided_gpu < P                        # the mix really contains proposals that miss quorum


def test_sharded_entry_world_of_one_with_rccl_and_quorum_bits(oracle):
    """The native multi-GPU entry on the box we have (one GPU): sbv_init_all finds 1 device; with SBV_RCCL=1 the bitmap
    still travels through ncclAllGather (one rank), so the collective code path is exercised; the per-proposal quorum
    bits (>= Q - 1 = 10 accepted signatures by distinct keys) are computed on the device.  Eight-GPU behaviour is the
    driver's to measure."""
    os.environ["SBV_RCCL"] = "1"
    os.environ["SBV_SHARD_MIN"] = str(1 << 16)
    try:
        sbv.shutdown()
        ndev = sbv.init_all()
        assert ndev >= 1
        P, Q = 30000, 11
        n = P * Q
        tup, exp = _gen(oracle, 0xC4, n, 16, 8)
        got = ctypes.create_string_buffer((n + 7) // 8)
        qb = ctypes.create_string_buffer((P + 7) // 8)
        info = sbv.verify_batch_sharded(ctypes.addressof(tup), n, ctypes.addressof(got), group=Q, quorum=Q - 1,
                                        quorum_out_ptr=ctypes.addressof(qb))
        assert got.raw == exp, _diff(got.raw, exp)
        assert info.devices == ndev and info.shards >= 1
        assert info.mode == 1                                        # the RCCL all-gather ran (world size = devices used)
        bits = sbv.bitmap_to_list(exp, n)
        raw = tup.raw
        want_q = []
        for p in range(P):
            keys = {raw[160 * i + 96:160 * i + 160] for i in range(p * Q, (p + 1) * Q) if bits[i]}
            want_q.append(len(keys) >= Q - 1)
        assert sbv.bitmap_to_list(qb.raw, P) == want_q
        assert 0 < sum(want_q) < P
        # duplicate signers must not count twice: proposal 0 becomes ten copies of ONE valid signature + one more signer
        i0 = next(i for i in range(Q) if bits[i])
        dup = bytearray(raw[:160 * Q])
        for j in range(Q - 1):
            dup[160 * j:160 * (j + 1)] = raw[160 * i0:160 * (i0 + 1)]
        t2 = ctypes.create_string_buffer(bytes(dup) + raw[160 * Q:160 * 5632 * 2])
        n2 = len(t2.raw) // 160 // Q * Q
        g2 = ctypes.create_string_buffer((n2 + 7) // 8)
        q2 = ctypes.create_string_buffer((n2 // Q + 7) // 8)
        sbv.verify_batch_sharded(ctypes.addressof(t2), n2, ctypes.addressof(g2), group=Q, quorum=Q - 1, quorum_out_ptr=ctypes.addressof(q2))
        assert sbv.bitmap_to_list(g2.raw, Q)[:Q - 1] == [True] * (Q - 1)      # ten accepted signatures ...
        assert sbv.bitmap_to_list(q2.raw, 1) == [False]                        # ... by one signer: no quorum
        # replica routing of a small batch, and the explicit-device entry
        m = 4096
        small = ctypes.create_string_buffer(m // 8)
        info = sbv.verify_batch_sharded(ctypes.addressof(tup), m, ctypes.addressof(small))
        assert small.raw == exp[:m // 8] and info.shards == 1
        on = ctypes.create_string_buffer(m // 8)
        sbv.verify_batch_on(0, ctypes.addressof(tup), m, ctypes.addressof(on))
        assert on.raw == exp[:m // 8]
    finally:
        os.environ.pop("SBV_RCCL", None)
        os.environ.pop("SBV_SHARD_MIN", None)
        sbv.shutdown()


def test_config3_over_8_logical_devices(oracle):
    """VERDICT r5 #1b: configs[3] — 50 000 proposals x 11 consenter signatures "sharded over 8 GPUs" — through the in-library multi-device
    path as an 8-GPU node runs it, on the one GPU this tier has: SBV_LOGICAL_DEVICES=8 folds eight contexts (shrunken pools) onto it.
    Eight shards of whole proposals from eight host threads, shard offsets > 0, quorum bits per shard, the bitmap gathered through the
    host (RCCL needs one rank per physical device); a batch that fills three of the eight devices (idle contexts); a small batch on the
    replica route.  Generic entry, registered-key entry and the message front end; every verdict against the generator's (the
    full-size oracle + OpenSSL diff of the same batch is test_config3_registered_key_sharded_entry_550000's)."""
    import hashlib
    import numpy as np
    from consensus_amd import shard
    os.environ["SBV_LOGICAL_DEVICES"] = "8"
    os.environ["SBV_SHARD_MIN"] = str(1 << 16)
    try:
        sbv.shutdown()
        ndev = sbv.init_all()
        assert ndev == 8 and sbv.device_count() >= 1
        P, Q = 50000, 11
        n = P * Q
        tup, exp = _gen(oracle, 0xC3, n, 16, 8)
        first = (ctypes.c_size_t * 17)()
        lib = sbv.load()
        lib.sbv_shard_plan.restype = ctypes.c_size_t
        lib.sbv_shard_plan.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
        assert lib.sbv_shard_plan(n, 8, Q, 1 << 16, first) == 8 and all(first[k] % Q == 0 and first[k] % 8 == 0 for k in range(8))
        # generic entry: 160-byte tuples, every context groups its shard and builds / caches the consenters' tables itself
        got = ctypes.create_string_buffer((n + 7) // 8)
        qb = ctypes.create_string_buffer((P + 7) // 8)
        info = sbv.verify_batch_sharded(ctypes.addressof(tup), n, ctypes.addressof(got), group=Q, quorum=Q - 1, quorum_out_ptr=ctypes.addressof(qb))
        assert got.raw == exp, _diff(got.raw, exp)
        m_or = 11 * 8000                                                          # the oracle's own verdicts on the first 8 000 proposals, and one
        ob = ctypes.create_string_buffer(m_or // 8)                               # whole shard further in (shard 5: offsets > 0)
        oracle.sbvo_p256_verify_batch(ctypes.addressof(tup), m_or, ctypes.addressof(ob), THREADS)
        assert got.raw[:m_or // 8] == ob.raw
        s5, e5 = first[5], first[6]
        ob5 = ctypes.create_string_buffer((e5 - s5) // 8)
        oracle.sbvo_p256_verify_batch(ctypes.addressof(tup) + 160 * s5, e5 - s5, ctypes.addressof(ob5), THREADS)
        assert got.raw[s5 // 8:e5 // 8] == ob5.raw
        assert info.devices == 8 and info.shards == 8 and info.mode == 2          # 8 shards, gathered through the host
        assert info.tuples_per_shard == first[1] and info.h2d_us > 0 and info.kernels_us > 0
        want_q = shard.quorum_bits(tup.raw, exp, n, Q, Q - 1)
        assert qb.raw == want_q and 0 < sum(sbv.bitmap_to_list(want_q, P)) < P
        assert sbv.pool_stats()["gpu_share"] == 8
        # three of eight devices busy, five idle; then one device (replica route, round-robin over the contexts)
        m3 = first[3]
        g3 = ctypes.create_string_buffer((m3 + 7) // 8)
        os.environ["SBV_SHARD_MIN"] = str(first[1])
        sbv.shutdown()
        assert sbv.init_all() == 8
        info = sbv.verify_batch_sharded(ctypes.addressof(tup), m3, ctypes.addressof(g3), group=Q, quorum=Q - 1)
        assert g3.raw == exp[:m3 // 8] and info.shards == 3 and info.devices == 8
        for _ in range(9):                                   # more small calls than contexts: every context serves at least one
            small = ctypes.create_string_buffer(4096 // 8)
            info = sbv.verify_batch_sharded(ctypes.addressof(tup), 4096, ctypes.addressof(small))
            assert small.raw == exp[:4096 // 8] and info.shards == 1
        on = ctypes.create_string_buffer(4096 // 8)
        sbv.verify_batch_on(5, ctypes.addressof(tup), 4096, ctypes.addressof(on))      # an explicit logical device
        assert on.raw == exp[:4096 // 8]
        # registered-key entry: the registry and the consenters' wide combs replicated on all eight contexts
        os.environ["SBV_SHARD_MIN"] = str(1 << 16)
        sbv.shutdown()
        assert sbv.init_all() == 8
        t2 = np.frombuffer(tup.raw, dtype=np.uint8).reshape(n, 160)
        keys, counts = np.unique(t2[:, 96:160], axis=0, return_counts=True)
        signer_keys = [bytes(k) for k in keys[counts > 1000]]
        assert len(signer_keys) == 16
        slot_of = dict(zip(signer_keys, sbv.register_keys(signer_keys)))
        sbv.widen_keys(list(slot_of.values()))
        slots = np.fromiter((slot_of.get(bytes(k), 0xFFFFFFFF) for k in t2[:, 96:160]), dtype=np.uint32, count=n)
        rsh = np.ascontiguousarray(t2[:, :96]).reshape(-1)
        gk = np.zeros((n + 7) // 8, dtype=np.uint8)
        qk = np.zeros((P + 7) // 8, dtype=np.uint8)
        info = sbv.verify_batch_keyed_sharded(rsh.ctypes.data, slots.ctypes.data, n, gk.ctypes.data, Q, Q - 1, qk.ctypes.data)
        assert gk.tobytes() == exp, _diff(gk.tobytes(), exp)
        assert info.shards == 8 and info.mode == 2 and qk.tobytes() == shard.quorum_bits_slots(slots, exp, n, Q, Q - 1) == want_q
        # the message front end over the eight contexts: SHA-256 + DER on each shard, offset tables sliced per shard and per piece
        nm = 8 * 8192 * Q // Q                                # 65 536 messages: below the minimum per device -> forced apart by SBV_SHARD_MIN
        os.environ["SBV_SHARD_MIN"] = "4096"
        os.environ["SBV_SHARD_PIECE_KEYED"] = "2048"
        sbv.shutdown()
        assert sbv.init_all() == 8
        rng = np.random.default_rng(5)
        ds = [int.from_bytes(hashlib.sha256(b"logical %d" % i).digest(), "big") % (ec.N - 1) + 1 for i in range(4)]
        pubs = [ec.pt_mul(d, ec.G) for d in ds]
        sl = sbv.register_keys([q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big") for q in pubs])
        msgs = [bytes([i & 255, (i >> 8) & 255]) * int(rng.integers(0, 40)) for i in range(nm)]
        kidx = [i % 4 for i in range(nm)]
        rs, okb = sbv.sign_batch(b"".join(d.to_bytes(32, "big") for d in ds), b"".join(hashlib.sha256(m).digest() for m in msgs), kidx)
        assert okb == b"\x01" * nm
        sigs, want = [], []
        for i in range(nm):
            sig = ec.der_encode_sig(int.from_bytes(rs[64 * i:64 * i + 32], "big"), int.from_bytes(rs[64 * i + 32:64 * i + 64], "big"))
            good = True
            if i % 7 == 3:
                sig = sig[:-1]; good = False
            if i % 9 == 5:
                msgs[i] = msgs[i] + b"?"; good = False
            sigs.append(sig); want.append(good)
        gm, _, info = sbv.verify_msgs_keyed_sharded(msgs, sigs, [sl[k] for k in kidx])
        assert info.shards == 8 and sbv.bitmap_to_list(gm, nm) == want
    finally:
        for k in ("SBV_LOGICAL_DEVICES", "SBV_SHARD_MIN", "SBV_SHARD_PIECE_KEYED"):
            os.environ.pop(k, None)
        sbv.shutdown()


def test_start_up_of_eight_contexts_does_not_race_with_their_first_batches(oracle):
    """Round 6 found a device-side race as old as the key-table cache: its hash table, entry counter and the hot keys' bookkeeping were
    initialised with bare hipMemset calls — ordered in the NULL stream only — right in front of the first grouped batch on the library's
    non-blocking streams.  With eight contexts starting on one GPU the null stream is busy, and in one start-up of ~60 a late fill wiped
    what the first batch had just published; from the third batch on honest signatures of up to 8 of the 16 signers were rejected
    (profiles/r06/stress_logical_before_fix_*).  sbv_api.hip: memset_now().  Ten start-ups here (tools/stress_logical.py runs hundreds):
    every verdict of four calls each, and the bookkeeping of a context checked against the host builder."""
    import numpy as np
    os.environ["SBV_LOGICAL_DEVICES"] = "8"
    os.environ["SBV_SHARD_MIN"] = str(1 << 16)
    try:
        P, Q = 50000, 11
        n = P * Q
        tup, exp = _gen(oracle, 0xC3, n, 16, 8)
        for cycle in range(10):
            sbv.shutdown()
            assert sbv.init_all() == 8
            for call in range(4):
                got = ctypes.create_string_buffer((n + 7) // 8)
                sbv.verify_batch_sharded(ctypes.addressof(tup), n, ctypes.addressof(got), group=Q, quorum=Q - 1)
                assert got.raw == exp, (cycle, call, _diff(got.raw, exp))
            if cycle in (0, 9):
                promoted, differ, _, _, _, inconsistent, shared, handed_out = sbv.debug_hot_check(cycle % 8)
                assert promoted == handed_out and promoted >= 10 and differ == 0 and inconsistent == 0 and shared == 0
    finally:
        os.environ.pop("SBV_LOGICAL_DEVICES", None)
        os.environ.pop("SBV_SHARD_MIN", None)
        sbv.shutdown()


def test_small_device_gets_smaller_pools_not_enomem(oracle):
    """the grouping pools default to 25 GB (65 536 groups + 16 384 cached keys); round 5 returned SBV_ENOMEM for every
    grouped batch on a device that could not hold them.  SBV_POOL_BUDGET_MB stands in for the small device: the pools are halved until
    they fit (sbv_p256_pool_stats reports it), with a budget below the smallest pools the batch is verified by the one-lane kernel
    instead of failing — the verdicts are the generator's either way."""
    n = 1 << 17
    tup, exp = _gen(oracle, 0xD1, n, 512, 8)
    try:
        os.environ["SBV_POOL_BUDGET_MB"] = "2048"
        sbv.shutdown()
        sbv.init(0)
        sbv.key_cache(True, 16384)
        got = ctypes.create_string_buffer(n // 8)
        sbv.verify_batch_ptr(ctypes.addressof(tup), n, ctypes.addressof(got))
        assert got.raw == exp, _diff(got.raw, exp)
        st = sbv.pool_stats()
        assert st["shrunk"] and 0 < st["groups_per_batch"] < 65536 and st["nomem_fallbacks"] == 0, st
        assert (st["cache_keys"] + st["groups_per_batch"]) * 304 * 1024 <= 2200 << 20
        assert sbv.last_group_stats()[1] > n // 2                # the batch still took the grouped step
        os.environ["SBV_POOL_BUDGET_MB"] = "8"                   # not even 128 table slots: no pools at all
        sbv.shutdown()
        sbv.init(0)
        got = ctypes.create_string_buffer(n // 8)
        sbv.verify_batch_ptr(ctypes.addressof(tup), n, ctypes.addressof(got))
        assert got.raw == exp, _diff(got.raw, exp)
        st = sbv.pool_stats()
        assert st["nomem_fallbacks"] == 1 and st["groups_per_batch"] == 0, st
    finally:
        os.environ.pop("SBV_POOL_BUDGET_MB", None)
        sbv.shutdown()


_SETTERS_DROP = r"""
import ctypes, os, sys
sys.path.insert(0, os.getcwd())
import consensus_amd as sbv
oracle = ctypes.CDLL(os.path.join("oracle", "libsbv_oracle.so"))
P256, K256, ED = sbv.SCHEME_P256, sbv.SCHEME_SECP256K1, sbv.SCHEME_ED25519
n = 4 * 512
batch = {}
for scheme, gen, size, seed in ((P256, oracle.sbvo_gen_batch, 160, 0x5E71), (K256, oracle.sbvo_k256_gen_batch, 160, 0x5E72),
                                (ED, oracle.sbvo_ed25519_gen_batch, 128, 0x5E73)):
    gen.argtypes = [ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    tup = ctypes.create_string_buffer(size * n); exp = ctypes.create_string_buffer(n // 8)
    gen(seed, n, 4, 0, tup, exp, 8)                      # 4 signers x 512 tuples, all valid
    assert exp.raw == b"\xff" * (n // 8)
    batch[scheme] = (tup.raw, exp.raw)
verify = {P256: sbv.verify_batch, K256: sbv.secp256k1_verify_batch, ED: sbv.ed25519_verify_batch}
setter = {P256: sbv.hot_keys, K256: sbv.k256_hot_keys, ED: sbv.ed_hot_keys}
stats = {P256: sbv.hot_key_stats, K256: sbv.k256_hot_key_stats, ED: sbv.ed_hot_key_stats}

def run(scheme, times=1):
    for _ in range(times):
        assert verify[scheme](batch[scheme][0], n) == batch[scheme][1], scheme

def state(scheme):                                       # (promoted combs, pool capacity, cached keys)
    return stats[scheme]()[:2] + sbv.key_cache_stats(scheme)[:1]

sbv.init(0)
try:
    sbv.set_grouping(True, 1, 8, 64)
    for s in (P256, K256, ED):
        setter[s](8, 64)
    for s in (P256, K256, ED):
        run(s, 2)                                        # the combs are promoted behind the first batch
    if any(stats[s]()[1] == 0 for s in (P256, K256, ED)):
        print("no room for the pool")
        sys.exit(0)
    for s in (P256, K256, ED):
        assert state(s) == (4, 8, 4), (s, state(s))
    sbv.ed_hot_keys(16, 64)                              # 1: Ed25519's pool and cache only
    assert state(ED) == (0, 0, 0) and state(P256) == (4, 8, 4) and state(K256) == (4, 8, 4), [state(s) for s in (P256, K256, ED)]
    run(ED, 2)
    assert state(ED) == (4, 16, 4), state(ED)
    sbv.k256_hot_keys(16, 64)                            # 2: secp256k1's pool and cache only
    assert state(K256) == (0, 0, 0) and state(P256) == (4, 8, 4) and state(ED) == (4, 16, 4), [state(s) for s in (P256, K256, ED)]
    run(K256, 2)
    assert state(K256) == (4, 16, 4), state(K256)
    sbv.hot_keys(16, 64)                                 # 3: the P-256 setter drops every scheme's pool and cache
    assert [state(s) for s in (P256, K256, ED)] == [(0, 0, 0)] * 3, [state(s) for s in (P256, K256, ED)]
    for s in (P256, K256, ED):                           # 4: the verdicts are still the generator's
        run(s)
    print("setters ok")
finally:
    sbv.hot_keys(1024, 4096); sbv.ed_hot_keys(1024, 4096); sbv.k256_hot_keys(0, 4096)
    sbv.set_grouping(True, sbv.GROUP_MIN_BATCH_DEFAULT, 0, 0)
"""


def test_hot_key_setters_drop_only_what_they_own():
    """A hot-key setter called with a new pool size frees pools that the next grouped batch rebuilds.  sbv_ed25519_hot_keys and
    sbv_secp256k1_hot_keys drop their own scheme's comb pool and key-table cache; sbv_p256_hot_keys drops all three schemes', because
    the P-256 pools are freed together with the grouping arrays the other two share.  In a fresh process: per scheme one batch of
    4 signers x 512 valid tuples (2 048 tuples), verified twice with pools of 8 combs from 64 hits on, so that every scheme holds 4
    promoted combs and 4 cached keys; then each setter in turn, reading (promoted, capacity, cached keys) of all three schemes."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if "HOT_KEYS" not in k and "HOT_MIN_HITS" not in k}
    out = subprocess.run([sys.executable, "-c", _SETTERS_DROP], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    if out.returncode == 0 and "no room for the pool" in out.stdout:
        pytest.skip("no room for the pool")
    assert out.returncode == 0 and "setters ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


def test_config3_registered_key_sharded_entry_550000(oracle, openssl_check):
    """configs[3] as BASELINE.json words it, on the consenters' resident combs: sbv_p256_verify_batch_keyed_sharded over
    550 000 = 50 000 x 11 records r | s | hash + key slots, 16 registered consenter keys with their wide combs.  Accept bitmap ==
    oracle == OpenSSL == the generic sharded entry on every signature; quorum bits (>= Q - 1 accepted signatures by distinct SLOTS)
    == the generic entry's (distinct KEYS) == the rule restated in Python; with SBV_RCCL=1 the bitmap travels through the
    one-rank all-gather.  Then: duplicate signers, unknown slots, a ragged batch, uploads in small pieces, 8-bit combs only."""
    import numpy as np
    from consensus_amd import shard
    os.environ["SBV_RCCL"] = "1"
    os.environ["SBV_SHARD_MIN"] = str(1 << 16)
    try:
        sbv.shutdown()
        ndev = sbv.init_all()
        assert ndev >= 1
        P, Q = 50000, 11
        n = P * Q
        tup, exp = _gen(oracle, 0xC3, n, 16, 8)
        a, b = _cpu_opinions(oracle, openssl_check, tup, n)
        assert a == b == exp
        t2 = np.frombuffer(tup.raw, dtype=np.uint8).reshape(n, 160)
        keys, counts = np.unique(t2[:, 96:160], axis=0, return_counts=True)
        signer_keys = [bytes(k) for k in keys[counts > 1000]]
        assert len(signer_keys) == 16
        sbv.clear_keys()
        slot_of = dict(zip(signer_keys, sbv.register_keys(signer_keys)))
        sbv.widen_keys(list(slot_of.values()))
        assert sbv.wide_key_stats()[:2] == (16, 20)
        slots = np.fromiter((slot_of.get(bytes(k), 0xFFFFFFFF) for k in t2[:, 96:160]), dtype=np.uint32, count=n)
        rsh = np.ascontiguousarray(t2[:, :96]).reshape(-1)

        def keyed(rsh_a, slots_a, m, group=Q, quorum=Q - 1):
            got = np.zeros((m + 7) // 8, dtype=np.uint8)
            qb = np.zeros(((m // group if group else 0) + 7) // 8 + 1, dtype=np.uint8)
            info = sbv.verify_batch_keyed_sharded(rsh_a.ctypes.data, slots_a.ctypes.data, m, got.ctypes.data, group, quorum,
                                                  qb.ctypes.data if group else 0)
            return got.tobytes(), qb.tobytes()[:((m // group if group else 0) + 7) // 8], info

        got, qb, info = keyed(rsh, slots, n)
        assert got == a, _diff(got, a)                                   # every one of the 550 000 verdicts: oracle and OpenSSL
        assert info.devices == ndev and info.mode == 1 and info.h2d_us > 0 and info.kernels_us > 0
        g2 = ctypes.create_string_buffer((n + 7) // 8)
        q2 = ctypes.create_string_buffer((P + 7) // 8)
        sbv.verify_batch_sharded(ctypes.addressof(tup), n, ctypes.addressof(g2), group=Q, quorum=Q - 1, quorum_out_ptr=ctypes.addressof(q2))
        assert g2.raw == got and q2.raw == qb                            # == the generic sharded entry, bitmap and quorum bits
        assert qb == shard.quorum_bits_slots(slots, got, n, Q, Q - 1) == shard.quorum_bits(tup.raw, got, n, Q, Q - 1)
        assert 0 < sum(sbv.bitmap_to_list(qb, P)) < P
        # duplicate signers must not count twice: proposal 0 becomes ten copies of ONE valid signature + one more signer
        bits = sbv.bitmap_to_list(got, Q)
        i0 = next(i for i in range(Q) if bits[i])
        m2 = 5632 * 2
        r2, s2 = rsh[:96 * m2].copy(), slots[:m2].copy()
        for j in range(Q - 1):
            r2[96 * j:96 * (j + 1)] = rsh[96 * i0:96 * (i0 + 1)]
            s2[j] = slots[i0]
        gd, qd, _ = keyed(r2, s2, m2)
        assert sbv.bitmap_to_list(gd, Q)[:Q - 1] == [True] * (Q - 1) and sbv.bitmap_to_list(qd, 1) == [False]
        assert gd[2:] == got[2:m2 // 8] and qd[1:] == qb[1:len(qd)]      # everything else as before (replica route: one device, no split)
        # an unknown / out-of-range slot is a reject, not an error
        s3 = slots[:4096].copy()
        s3[::7] = 0xFFFFFFFF
        s3[3::7] = 1 << 20
        g3, _, _ = keyed(rsh[:96 * 4096], s3, 4096, 0, 0)
        w3 = sbv.bitmap_to_list(got, 4096)
        assert sbv.bitmap_to_list(g3, 4096) == [w3[i] and i % 7 not in (0, 3) for i in range(4096)]
        # ragged size, no groups
        m4 = 100003
        g4, _, _ = keyed(rsh[:96 * m4], slots[:m4], m4, 0, 0)
        assert sbv.bitmap_to_list(g4, m4) == sbv.bitmap_to_list(got, m4)
        # the 8-bit combs every key keeps give the same verdicts (wide combs off frees them on every device)
        sbv.wide_keys(0, 0)
        assert sbv.wide_key_stats()[0] == 0
        g5, q5, _ = keyed(rsh, slots, n)
        assert g5 == got and q5 == qb
        sbv.wide_keys()
        sbv.widen_keys(list(slot_of.values()))
        # uploads in small pieces beside the kernels: 11 264-signature pieces alternate between the two slots
        os.environ["SBV_SHARD_PIECE_KEYED"] = "16384"
        sbv.shutdown()
        assert sbv.init_all() >= 1
        assert dict(zip(signer_keys, sbv.register_keys(signer_keys))) == slot_of      # a fresh process-wide registry: the same slot numbers
        sbv.widen_keys(list(slot_of.values()))
        g6, q6, info = keyed(rsh, slots, n)
        assert g6 == got and q6 == qb and info.h2d_us > 0
    finally:
        for k in ("SBV_RCCL", "SBV_SHARD_MIN", "SBV_SHARD_PIECE_KEYED"):
            os.environ.pop(k, None)
        try:
            sbv.wide_keys()
            sbv.clear_keys()
        except sbv.SbvError:
            pass
        sbv.shutdown()


# ---- key-affine partition: device g verifies the tuples of "its" keys only ------------------------------
def test_two_threads_in_the_sharded_entry_keep_their_own_bitmaps(oracle):
    """the all-gather phase of a sharded call used to run without the device's lock, so a second caller
    could overwrite (or free) the gather buffer in between.  One multi-shard call at a time now owns the gather buffers
    (g_sharded_mu).  Two threads, different batches, SBV_RCCL=1 (world of one: every call takes the collective path), many
    rounds: every call must return ITS batch's bitmap and quorum bits."""
    import threading
    os.environ["SBV_RCCL"] = "1"
    os.environ["SBV_SHARD_MIN"] = str(1 << 14)
    try:
        sbv.shutdown()
        assert sbv.init_all() >= 1
        Q = 11
        jobs = []
        for seed, P in ((0xD1, 3000), (0xD2, 4500)):
            n = P * Q
            tup, exp = _gen(oracle, seed, n, 16, 8)
            jobs.append((tup, exp, n, P))
        errors = []

        def worker(k):
            tup, exp, n, P = jobs[k]
            for _ in range(12):
                got = ctypes.create_string_buffer((n + 7) // 8)
                qb = ctypes.create_string_buffer((P + 7) // 8)
                sbv.verify_batch_sharded(ctypes.addressof(tup), n, ctypes.addressof(got), group=Q, quorum=Q - 1, quorum_out_ptr=ctypes.addressof(qb))
                if got.raw != exp:
                    errors.append((k, _diff(got.raw, exp)))
                    return

        th = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=300)
        assert not any(t.is_alive() for t in th), "a sharded call did not return"
        assert not errors, errors[:2]
    finally:
        os.environ.pop("SBV_RCCL", None)
        os.environ.pop("SBV_SHARD_MIN", None)
        sbv.shutdown()


def test_sharded_entry_uploads_in_pieces_beside_the_kernels(oracle):
    """verify_shard's two upload slots: with SBV_SHARD_PIECE = 16384 a 330 000-tuple call runs as 30 pieces of 11 264 tuples
    (the granule of group = 11 is 5 632) alternating between the two slots, the copy of piece i + 1 on the copy stream while
    piece i's kernels run; accept bitmap and quorum bits must equal the one-piece run's (key-table cache off: whole launches)
    and the generator's.  Also through the explicit-device entry, whose pieces have no group."""
    os.environ["SBV_SHARD_PIECE"] = "16384"
    try:
        sbv.shutdown()
        assert sbv.init_all() >= 1
        P, Q = 30000, 11
        n = P * Q
        tup, exp = _gen(oracle, 0xC7, n, 16, 8)
        outs = []
        for cache in (True, False, True):
            sbv.key_cache(cache)
            got = ctypes.create_string_buffer((n + 7) // 8)
            qb = ctypes.create_string_buffer((P + 7) // 8)
            info = sbv.verify_batch_sharded(ctypes.addressof(tup), n, ctypes.addressof(got), group=Q, quorum=Q - 1,
                                            quorum_out_ptr=ctypes.addressof(qb))
            assert got.raw == exp, (cache, _diff(got.raw, exp))
            assert info.h2d_us > 0 and info.kernels_us > 0
            outs.append(qb.raw)
        assert outs[0] == outs[1] == outs[2]
        bits = sbv.bitmap_to_list(exp, n)
        raw = tup.raw
        want_q = [len({raw[160 * i + 96:160 * i + 160] for i in range(p * Q, (p + 1) * Q) if bits[i]}) >= Q - 1 for p in range(P)]
        assert sbv.bitmap_to_list(outs[0], P) == want_q
        m = 100003                                    # ragged: 6 pieces of 16 384 and a tail of 1 699
        on = ctypes.create_string_buffer((m + 7) // 8)
        sbv.verify_batch_on(0, ctypes.addressof(tup), m, ctypes.addressof(on))
        assert sbv.bitmap_to_list(on.raw, m) == bits[:m]
    finally:
        os.environ.pop("SBV_SHARD_PIECE", None)
        sbv.key_cache(True)
        sbv.shutdown()


def test_key_affine_parts_are_disjoint_cover_the_batch_and_match_the_numpy_hash(gpu, oracle):
    """sbv_p256_verify_batch_dev_part on a device-resident 2^18 batch (256 keys, 1/5 corrupted), parts = 1, 3, 8: each part's
    bitmap has bits only at tuples whose key hashes to that part (consensus_amd/shard.py: key_parts is the numpy twin of the
    device hash), the parts' member counts add up to n, their bitmaps are disjoint and their OR is the full verdict bitmap."""
    import numpy as np
    import torch
    from consensus_amd import shard
    sbv.init(0)                        # the test above shuts the library down
    n = 1 << 18
    tup, exp = _gen(oracle, 0xAFF1, n, 256, 5)
    d_t = torch.frombuffer(tup, dtype=torch.uint8).cuda()
    stream = torch.cuda.current_stream()
    want = np.unpackbits(np.frombuffer(exp, dtype=np.uint8), bitorder="little")[:n]
    for parts in (1, 3, 8):
        ids = shard.key_parts(tup.raw, n, parts)
        acc = np.zeros(n, dtype=np.uint8)
        total = 0
        for p in range(parts):
            d_w = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device="cuda")        # the entry zeroes it itself
            members = gpu.verify_batch_dev_part(d_t.data_ptr(), n, p, parts, d_w.data_ptr(), stream.cuda_stream)
            torch.cuda.synchronize()
            bits = np.unpackbits(d_w.cpu().numpy().view(np.uint8), bitorder="little")[:n]
            assert members == int((ids == p).sum()), (parts, p)
            assert not bits[ids != p].any(), (parts, p)                 # nothing outside the part
            assert (bits[ids == p] == want[ids == p]).all(), (parts, p)
            assert not (acc & bits).any()
            acc |= bits
            total += members
        assert total == n and (acc == want).all(), parts


def test_sharded_entry_by_key_on_one_gpu_rehearses_an_8_way_partition(gpu, oracle, openssl_check):
    """The key-affine mode of sbv_p256_verify_batch_sharded with 8 parts on the one visible GPU (parts run one after another):
    550 000 consenter signatures = 50 000 proposals x 11 (configs[3]) with duplicated signers inside some proposals — accept
    bitmap and per-proposal quorum bits equal the contiguous mode's, the oracle's and the rule restated in numpy."""
    import numpy as np
    from consensus_amd import shard
    group, quorum, props = 11, 10, 50000
    n = group * props
    tup, exp = _gen(oracle, 0xAFF2, n, 16, 9)
    raw = bytearray(tup.raw)
    for p in range(0, props, 97):                        # every 97th proposal: signer of tuple 0 signs twice -> one distinct signer fewer
        raw[160 * (p * group + 1) + 96:160 * (p * group + 1) + 160] = raw[160 * (p * group) + 96:160 * (p * group) + 160]
        raw[160 * (p * group + 1):160 * (p * group + 1) + 96] = raw[160 * (p * group):160 * (p * group) + 96]
    buf = ctypes.create_string_buffer(bytes(raw), len(raw))
    a, b = _cpu_opinions(oracle, openssl_check, buf, n)
    assert a == b
    want_q = shard.quorum_bits(bytes(raw), a, n, group, quorum)
    for rccl in (False, True):                 # host OR of the per-device bitmaps, then the in-place ncclAllReduce with a world of one
        if rccl:
            os.environ["SBV_RCCL"] = "1"
        try:
            sbv.shutdown()
            gpu.init_all()
            res = {}
            for label, by_key in (("contiguous", False), ("by key, 8 parts", True)):
                gpu.shard_mode(by_key, 8 if by_key else 0)
                try:
                    got = ctypes.create_string_buffer((n + 7) // 8)
                    qb = ctypes.create_string_buffer((props + 7) // 8)
                    info = gpu.verify_batch_sharded(ctypes.addressof(buf), n, ctypes.addressof(got), group, quorum, ctypes.addressof(qb))
                    res[label] = (got.raw, qb.raw, info.mode, info.shards)
                finally:
                    gpu.shard_mode(False, 0)
            assert res["contiguous"][0] == a[:(n + 7) // 8], _diff(res["contiguous"][0], a)
            assert res["by key, 8 parts"][0] == res["contiguous"][0]
            assert res["by key, 8 parts"][1] == res["contiguous"][1] == want_q
            assert res["by key, 8 parts"][2] == (3 if rccl else 4) and res["by key, 8 parts"][3] == 8, res["by key, 8 parts"][2:]
        finally:
            os.environ.pop("SBV_RCCL", None)
    sbv.shutdown()
    sbv.init(0)
