"""GPU tier for the secp256k1 hot keys (include/sbv.h: sbv_secp256k1_hot_keys; consensus_amd/csrc/k256_group.h "hot keys"), through
the C-ABI and the Python wrapper: cache slots that keep signing get 16-bit combs of Q, built on the device behind a batch's verdicts;
the wavefronts of the key-sorted list whose live lanes all own one take the wide pass.  Expected bitmaps are the generator's; promoted
combs are held to the host builder's byte for byte (sbv_secp256k1_hot_selfcheck).  The pool is off by default: every test switches it
on for itself and restores k256_hot_keys(0, 0) and the grouping defaults."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

import consensus_amd as sbv

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
THREADS = os.cpu_count() or 1
K256 = sbv.SCHEME_SECP256K1


@pytest.fixture(scope="module")
def gpu():
    sbv.init(0)
    yield sbv


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


@pytest.fixture(scope="module")
def batches(koracle):
    """every generator batch of this module, made once: name -> (tuples, expected verdicts as a list)"""
    def gen(seed, n, nkeys, inv):
        tup, exp = _gen(koracle, seed, n, nkeys, inv)
        return tup.raw[:160 * n], sbv.bitmap_to_list(exp.raw, n)
    out = {"four": gen(0x4071, 4096, 4, 8), "a64": gen(0x4072, 1 << 15, 64, 8), "c32": gen(0x4073, 1 << 14, 32, 8)}
    for k in range(3):
        out["set%d" % k] = gen(0x4080 + k, 8 * 4096, 8, 9)
    for k in range(5):
        out["round%d" % k] = gen(0x4090 + k, 4096, 8, 8)
    return out


def _tuples(blob):
    return [blob[160 * i:160 * i + 160] for i in range(len(blob) // 160)]


def _pack(bits):
    out = bytearray((len(bits) + 7) // 8)
    for i, b in enumerate(bits):
        if b:
            out[i >> 3] |= 1 << (i & 7)
    return bytes(out)


def _run(gpu, blob, want):
    n = len(blob) // 160
    got = gpu.secp256k1_verify_batch(blob, n)
    assert got == _pack(want), [i for i, (g, w) in enumerate(zip(sbv.bitmap_to_list(got, n), want)) if g != w][:8]
    return gpu.k256_hot_key_stats()


def _off(gpu):
    gpu.k256_hot_keys(0, 0)
    gpu.set_grouping(True, sbv.GROUP_MIN_BATCH_DEFAULT, 0, 0)


def test_all_hot_signers_take_the_wide_pass(gpu, batches):
    """4 096 tuples by 4 signers, every 8th corrupted, a pool of 8 from 64 hits on.  Batch 1: the generator's bitmap, nobody served
    wide, 4 keys promoted behind the verdicts.  Batch 2: every grouped lane goes through the wide pass.  The four combs equal the host
    builder's.  With the pool switched off again the stats are (0, 0, 0) and the verdicts unchanged."""
    blob, want = batches["four"]
    try:
        gpu.set_grouping(True, 1, 8, 64)
        gpu.k256_hot_keys(8, 64)
        promoted, cap, wide, min_hits = _run(gpu, blob, want)
        assert (promoted, cap, wide, min_hits) == (4, 8, 0, 64)
        promoted, cap, wide, _ = _run(gpu, blob, want)
        grouped = int(gpu.debug_group_readout()["counters"][1])
        assert promoted == 4 and grouped > 3000 and wide == grouped, (promoted, wide, grouped)
        for i in range(4):
            assert gpu.k256_hot_selfcheck(i), i
        gpu.k256_hot_keys(0, 0)
        assert _run(gpu, blob, want)[:3] == (0, 0, 0)
        assert _run(gpu, blob, want)[:3] == (0, 0, 0)
    finally:
        _off(gpu)


def test_some_hot_signers_and_mixed_wavefronts(gpu, batches):
    """Batch A (2^15 tuples, 64 signers) promotes all 64 into a pool of 64.  Batch B holds those 64 signers and 32 new ones: a mixed
    wavefront stays with the 8-bit kernel, so the wide pass serves, of each hot signer's run of c lanes, at least c - 126 (the lanes in
    wavefronts wholly inside the run) and at most c.  Three runs: every verdict the generator's, the pool stays with its 64 owners (it is
    full and the counts are alike: the hysteresis trades nothing).  Sizes 4 095 and 4 097 of the same mix leave the last block of the
    XCD-aware order ragged."""
    a_blob, a_want = batches["a64"]
    c_blob, c_want = batches["c32"]
    ta, tc = _tuples(a_blob), _tuples(c_blob)
    mix, mix_want = [], []
    for i in range(1 << 14):                                  # A, A, C, A, A, C, ...: 2^15 + 2^14 tuples, cut to 2^15
        mix += [ta[2 * i], ta[2 * i + 1], tc[i]]
        mix_want += [a_want[2 * i], a_want[2 * i + 1], c_want[i]]
    n = 1 << 15
    mix, mix_want = mix[:n], mix_want[:n]
    count_a = {}
    for t in ta:
        count_a[t[96:]] = count_a.get(t[96:], 0) + 1
    hot = {k for k, c in count_a.items() if c >= 64}
    assert len(hot) == 64

    def bounds(tuples):
        cnt = {}
        for t in tuples:
            if t[96:] in hot:
                cnt[t[96:]] = cnt.get(t[96:], 0) + 1
        return sum(max(0, c - 126) for c in cnt.values()), sum(cnt.values())

    try:
        gpu.set_grouping(True, 1, 8, 1024)
        gpu.k256_hot_keys(64, 64)
        promoted, cap, wide, _ = _run(gpu, a_blob, a_want)
        assert cap == 64 and promoted == 64 and wide == 0, (promoted, cap, wide)
        lo, hi = bounds(mix)
        assert 0 < lo < hi
        b_blob = b"".join(mix)
        for rnd in range(3):
            promoted, _, wide, _ = _run(gpu, b_blob, mix_want)
            assert promoted == 64 and lo <= wide <= hi, (rnd, promoted, lo, wide, hi)
        for i in (0, 31, 63):
            assert gpu.k256_hot_selfcheck(i), i
        for m in (4095, 4097):
            lo, hi = bounds(mix[:m])
            promoted, _, wide, _ = _run(gpu, b"".join(mix[:m]), mix_want[:m])
            assert promoted == 64 and lo <= wide <= hi, (m, promoted, lo, wide, hi)
    finally:
        _off(gpu)


def test_golden_vectors_and_scalar_cases_through_promoted_combs(gpu):
    """The two inputs of the CPU tier on the device.  tests/golden/k256_vectors.json x 40 from 30 hits on: the file's verdicts in three
    consecutive batches, keys promoted, every promoted comb the host builder's for its owner (a key that is no point has no such comb);
    the u1 G = +-u2 Q vectors alone, all served from wide combs, keep their verdicts.  The wide16 and g20 scalar cases with their
    rejecting twins: the cases' own verdicts from the 8-bit combs and after promotion."""
    import scalar_cases as sc
    vs = json.load(open(os.path.join(GOLDEN, "k256_vectors.json")))["vectors"]
    blob = b"".join(bytes.fromhex(v["tuple"]) for v in vs) * 40
    want = [v["accept"] for v in vs] * 40
    try:
        gpu.set_grouping(True, 1, 8, 1024)
        gpu.k256_hot_keys(16, 30)
        for rnd in range(3):
            promoted, cap, wide, _ = _run(gpu, blob, want)
            assert cap == 16, (rnd, promoted, cap, wide)
        assert 1 <= promoted <= 16 and wide > 0, (promoted, wide)
        for i in range(promoted):
            assert gpu.k256_hot_selfcheck(i), i
        # the group-law vectors in a batch of their own: every lane from a wide comb
        pm = [v for v in vs if v["name"].startswith("u1G_eq_")]
        assert len(pm) == 6 and {v["accept"] for v in pm} == {True, False}
        gpu.k256_hot_keys(0, 0)
        gpu.k256_hot_keys(8, 30)
        pblob = b"".join(bytes.fromhex(v["tuple"]) for v in pm) * 40
        pwant = [v["accept"] for v in pm] * 40
        assert _run(gpu, pblob, pwant)[2] == 0
        promoted, _, wide, _ = _run(gpu, pblob, pwant)
        assert promoted == len({bytes.fromhex(v["tuple"])[96:] for v in pm}) and wide == len(pwant), (promoted, wide)
        # the scalar cases: the list repeated until every key of it has passed min_hits
        cs = sc.by_walker(sc.cases("k256"), "wide%d" % sc.K256_WIDE_BITS, "g%d" % sc.G_BITS["k256"])
        keys = {c.tuple[96:] for c in cs}
        min_hits, reps = 600, 1
        while min(sum(1 for c in cs if c.tuple[96:] == k) for k in keys) * reps < min_hits:
            reps += 1
        sblob, swant = sc.blob(cs) * reps, [c.expect for c in cs] * reps
        gpu.k256_hot_keys(0, 0)
        gpu.k256_hot_keys(8, min_hits)
        promoted, _, wide, _ = _run(gpu, sblob, swant)
        assert promoted == len(keys) and wide == 0
        promoted, _, wide, _ = _run(gpu, sblob, swant)
        assert wide == len(swant), (promoted, wide)
        for i in range(promoted):
            assert gpu.k256_hot_selfcheck(i), i
    finally:
        _off(gpu)


def test_pool_follows_a_changing_signer_set(gpu, batches):
    """The life cycle (p256_group.h: decay, eviction with hysteresis — the shared kernels) on this scheme's pool: 8 combs, three disjoint
    sets of 8 signers one after another.  The set that signs now takes the pool over from the set that stopped; every comb a new owner
    got equals the host builder's comb for ITS key; every verdict of every batch is the generator's."""
    n = 8 * 4096
    try:
        gpu.set_grouping(True, 1, 8, 64)
        gpu.k256_hot_keys(8, 2048)
        for k in range(3):
            blob, want = batches["set%d" % k]
            settled_at = None
            for call in range(48):
                h = _run(gpu, blob, want)
                assert h[1] == 8, (k, call, h)
                if h[2] >= n * 0.80:                           # (nearly) the whole batch through the wide pass: this set owns the pool
                    settled_at = call
                    break
            assert settled_at is not None and (settled_at <= 2 if k == 0 else 3 <= settled_at), (k, settled_at)
            for _ in range(2):
                h = _run(gpu, blob, want)
            assert h[0] == 8 and h[1] == 8 and h[2] >= n * 0.80, (k, h)
            for i in range(8):
                assert gpu.k256_hot_selfcheck(i), (k, i)
    finally:
        _off(gpu)


def test_neighbour_schemes_share_the_grouping_arrays(gpu, oracle, batches):
    """The grouping arrays and the event behind which a batch's promotions are published are shared between the schemes: five rounds of a
    promoting secp256k1 batch, a grouped P-256 batch and a grouped Ed25519 batch of 4 096 tuples each.  Every bitmap equals its
    generator's; the secp256k1 combs hold afterwards; the P-256 pool reports no inconsistency."""
    oracle.sbvo_ed25519_gen_batch.argtypes = [ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_int]
    n = 4096
    ptup, pexp = ctypes.create_string_buffer(160 * n), ctypes.create_string_buffer(n // 8)
    oracle.sbvo_gen_batch(0x40A0, n, 4, 8, ptup, pexp, THREADS)
    etup, eexp = ctypes.create_string_buffer(128 * n), ctypes.create_string_buffer(n // 8)
    oracle.sbvo_ed25519_gen_batch(0x40A1, n, 4, 8, etup, eexp, THREADS)
    try:
        gpu.set_grouping(True, 1, 8, 64)
        gpu.k256_hot_keys(64, 64)
        for rnd in range(5):
            blob, want = batches["round%d" % rnd]
            h = _run(gpu, blob, want)
            assert h[1] == 64 and h[0] == 8 * (rnd + 1), (rnd, h)
            assert gpu.verify_batch(ptup.raw, n) == pexp.raw, rnd
            assert gpu.ed25519_verify_batch(etup.raw, n) == eexp.raw, rnd
        blob, want = batches["round0"]
        h = _run(gpu, blob, want)
        assert h[0] == 40 and h[2] > 3000, h
        for i in range(40):
            assert gpu.k256_hot_selfcheck(i), i
        chk = gpu.debug_hot_check()
        assert chk[1] == 0 and chk[5] == 0 and chk[6] == 0, chk
    finally:
        _off(gpu)


def test_forgetting_the_cache_forgets_the_promotions(gpu, batches):
    blob, want = batches["four"]
    try:
        gpu.set_grouping(True, 1, 8, 64)
        gpu.k256_hot_keys(8, 64)
        _run(gpu, blob, want)
        h = _run(gpu, blob, want)
        assert h[1] == 8 and h[0] == 4 and h[2] > 0, h
        gpu.key_cache(False, 0, K256)
        gpu.key_cache(True, 0, K256)
        assert gpu.k256_hot_key_stats()[0] == 0
        h = _run(gpu, blob, want)                              # from cold: the combs are rebuilt, nobody is served wide
        assert h[0] == 4 and h[2] == 0, h
        h = _run(gpu, blob, want)
        assert h[0] == 4 and h[2] > 3000, h
        for i in range(4):
            assert gpu.k256_hot_selfcheck(i), i
    finally:
        gpu.key_cache(True, 0, K256)
        _off(gpu)


def test_the_pool_is_off_unless_asked_for():
    """A fresh process that never calls sbv_secp256k1_hot_keys runs one grouped secp256k1 batch: no pool, nobody served wide."""
    code = r"""
import ctypes, os, sys
sys.path.insert(0, os.getcwd())
import consensus_amd as sbv
oracle = ctypes.CDLL(os.path.join("oracle", "libsbv_oracle.so"))
oracle.sbvo_k256_gen_batch.argtypes = [ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
n = 4096
tup = ctypes.create_string_buffer(160 * n); exp = ctypes.create_string_buffer(n // 8)
oracle.sbvo_k256_gen_batch(0x4071, n, 4, 8, tup, exp, 8)
sbv.init(0)
sbv.set_grouping(True, 1, 8, 64)
for _ in range(2):
    assert sbv.secp256k1_verify_batch(tup.raw, n) == exp.raw
groups, grouped, _, _ = sbv.last_group_stats()
assert groups == 4 and grouped > 3000, (groups, grouped)
promoted, cap, wide, min_hits = sbv.k256_hot_key_stats()
assert (promoted, cap, wide, min_hits) == (0, 0, 0, 4096), (promoted, cap, wide, min_hits)
print("off ok")
"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("SBV_K256_HOT")}
    out = subprocess.run([sys.executable, "-c", code], cwd=os.path.join(HERE, ".."), env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "off ok" in out.stdout, out.stdout + out.stderr
