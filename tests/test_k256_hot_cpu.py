"""CPU tier for the secp256k1 hot keys (include/sbv.h: sbv_secp256k1_hot_keys; consensus_amd/csrc/k256_group.h "hot keys").

tests/emul/k256_hot_emul.cc runs the lanes the kernels are made of, in launch order, on a persistent key-table cache: grouping, the
key-sorted list, the 8-bit combs, the G lane, the class lane, the wave rule (k256_wave_is_wide, the one function both Q kernels call),
the wide lane or the 8-bit lanes, and the tail (decay, select, evict, k256_widetab_lane, publish).  Verdicts are held to the oracle,
the golden vectors and the scalar cases' own; promoted combs to the host builder, entry by entry.  (The emulator's comb of G is 16 bits wide: the g20 cases
run here as scalars, at their 20-bit window boundaries only on the device.)"""
import ctypes
import json
import os
import subprocess

import pytest

import consensus_amd as sbv
import scalar_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
THREADS = os.cpu_count() or 1
WIDE, FULL, NONE = 2, 0, 3                      # p256_group.h: SBV_Q_WIDE, SBV_Q_FULL, SBV_Q_NONE
NO_COMB, NOT_CACHED = 0xFFFFFFFF, 0xFFFFFFFE


@pytest.fixture(scope="module")
def hemul():
    src = os.path.join(HERE, "emul", "k256_hot_emul.cc")
    so = os.path.join(HERE, "emul", "libsbv_k256_hot_emul.so")
    csrc = os.path.join(HERE, "..", "consensus_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-misleading-indentation", src, "-o", so])
    lib = ctypes.CDLL(so)
    V, S, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    lib.sbvk256hot_reset.argtypes = [U, U, U]
    lib.sbvk256hot_key_cache.argtypes = [ctypes.c_int]
    lib.sbvk256hot_verify.argtypes = [ctypes.c_char_p, S, V, V]
    lib.sbvk256hot_wave_classes.argtypes = [V, S]
    lib.sbvk256hot_wave_classes.restype = S
    lib.sbvk256hot_wide_of_key.argtypes = [ctypes.c_char_p]
    lib.sbvk256hot_wide_of_key.restype = U
    lib.sbvk256hot_hits_of_key.argtypes = [ctypes.c_char_p]
    lib.sbvk256hot_hits_of_key.restype = U
    lib.sbvk256hot_owner_key.argtypes = [U, V]
    lib.sbvk256hot_comb_mismatches.argtypes = [U]
    lib.sbvk256hot_comb_mismatches.restype = ctypes.c_long
    return lib


@pytest.fixture(scope="module")
def koracle(oracle):
    oracle.sbvo_k256_verify_batch.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
    oracle.sbvo_k256_gen_batch.argtypes = [ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_int]
    return oracle


def _bits(bm, n):
    return [bool((bm[i >> 3] >> (i & 7)) & 1) for i in range(n)]


def _gen(koracle, seed, n, nkeys, inv):
    tup = ctypes.create_string_buffer(160 * n)
    exp = ctypes.create_string_buffer((n + 7) // 8)
    koracle.sbvo_k256_gen_batch(seed, n, nkeys, inv, tup, exp, THREADS)
    want = ctypes.create_string_buffer((n + 7) // 8)
    koracle.sbvo_k256_verify_batch(tup, n, want, THREADS)
    assert want.raw == exp.raw
    return tup.raw, _bits(want.raw, n)


def _oracle(koracle, tuples):
    n = len(tuples) // 160
    want = ctypes.create_string_buffer((n + 7) // 8)
    koracle.sbvo_k256_verify_batch(tuples, n, want, THREADS)
    return _bits(want.raw, n)


def _run(hemul, tuples):
    """one emulated grouped batch -> (verdicts, stats): stats = groups, lanes, live lanes served wide, promoted keys, wide wavefronts,
    8-bit wavefronts with a live lane, wavefronts without one, evictions so far"""
    n = len(tuples) // 160
    bm = ctypes.create_string_buffer(max(1, (n + 7) // 8))
    st = (ctypes.c_uint32 * 8)()
    hemul.sbvk256hot_verify(tuples, n, bm, st)
    return _bits(bm.raw, n), list(st)


def _classes(hemul):
    buf = ctypes.create_string_buffer(4096)
    m = hemul.sbvk256hot_wave_classes(buf, 4096)
    return list(buf.raw[:m])


def _owner(hemul, index):
    key = ctypes.create_string_buffer(64)
    return key.raw if hemul.sbvk256hot_owner_key(index, key) else None


def _by_key(tuples):
    out = {}
    for i in range(len(tuples) // 160):
        out.setdefault(tuples[160 * i + 96:160 * i + 160], []).append(tuples[160 * i:160 * i + 160])
    return out


def test_every_batch_equals_the_oracle_and_every_promoted_comb_the_host_builders(hemul, koracle):
    """2 048 generator tuples over 6 signers with every 8th corrupted, a pool of 4 combs from 200 hits on: cold (nobody served wide),
    promoting, served wide, the pool full (two signers stay on their 8-bit combs, similar counts trade nothing) and with the feature
    off.  Verdicts equal sbvo_k256_verify_batch in every batch; every promoted comb equals the host builder's, entry by entry."""
    n = 2048
    tuples, want = _gen(koracle, 0x407, n, 6, 8)
    signers = sorted(((len(v), k) for k, v in _by_key(tuples).items()), reverse=True)[:6]
    assert all(c > 250 for c, _ in signers)
    hemul.sbvk256hot_reset(1024, 4, 200)
    got, st = _run(hemul, tuples)                             # cold: every comb is built in this batch, nobody is wide
    assert got == want and st[2] == 0 and st[4] == 0 and st[3] == 4, st
    assert any(want) and not all(want)
    got, st = _run(hemul, tuples)                             # four signers are served from their combs
    assert got == want and st[3] == 4 and st[4] > 0, st
    wide_keys = [k for _, k in signers if hemul.sbvk256hot_wide_of_key(k) < 4]
    assert len(wide_keys) == 4
    assert 0 < st[2] <= sum(c for c, k in signers if k in wide_keys)
    assert st[2] >= sum(max(0, c - 126) for c, k in signers if k in wide_keys)
    for i in range(4):
        assert hemul.sbvk256hot_comb_mismatches(i) == 0, i
    owners = [_owner(hemul, i) for i in range(4)]
    for _ in range(2):                                        # the pool is full, the counts are alike: nobody trades a comb
        got, st2 = _run(hemul, tuples)
        assert got == want and st2[3] == 4 and st2[7] == 0 and st2[2] == st[2], st2
    assert [_owner(hemul, i) for i in range(4)] == owners
    hemul.sbvk256hot_reset(1024, 0, 200)                      # the library's default: no pool
    for _ in range(2):
        got, st = _run(hemul, tuples)
        assert got == want and st[2:5] == [0, 0, 0], st
    assert set(_classes(hemul)) <= {FULL, NONE}


def test_golden_vectors_through_promoted_combs(hemul):
    """tests/golden/k256_vectors.json repeated 40 times, combs from 30 hits on: the file's verdicts in three consecutive batches; keys
    that keep signing are promoted, keys that are no points (off the curve, a coordinate >= p, (0, 0)) never own a comb, and the
    vectors whose u1 G = +-u2 Q (the doubling and infinity inside the last addition) keep their verdicts when served from a wide comb."""
    vs = json.load(open(os.path.join(GOLDEN, "k256_vectors.json")))["vectors"]
    blob = b"".join(bytes.fromhex(v["tuple"]) for v in vs) * 40
    want = [v["accept"] for v in vs] * 40
    hemul.sbvk256hot_reset(256, 8, 30)
    stats = []
    for rnd in range(3):
        got, st = _run(hemul, blob)
        assert got == want, (rnd, [vs[i % len(vs)]["name"] for i in range(len(want)) if got[i] != want[i]][:8])
        stats.append(st)
    assert stats[0][2] == 0 and stats[1][2] > 0 and stats[2][2] > 0, stats
    assert 1 <= stats[2][3] <= 8
    named = {v["name"]: bytes.fromhex(v["tuple"])[96:] for v in vs}
    for name in ("q_off_curve_y_plus_1", "q_x_eq_p", "q_y_eq_p", "q_zero_zero"):
        assert hemul.sbvk256hot_wide_of_key(named[name]) == NO_COMB, name
        assert hemul.sbvk256hot_hits_of_key(named[name]) >= 30, name          # counted like everybody: what keeps it out is its valid byte
    owners = [_owner(hemul, i) for i in range(stats[2][3])]
    assert all(o is not None for o in owners)
    for i in range(len(owners)):
        assert hemul.sbvk256hot_comb_mismatches(i) == 0, i
    # the pool holds 8 of the file's ~100 keys: the group-law vectors get combs of their own in a batch of theirs
    pm = [v for v in vs if v["name"].startswith("u1G_eq_")]
    assert len(pm) == 6 and {v["accept"] for v in pm} == {True, False}
    pkeys = {bytes.fromhex(v["tuple"])[96:] for v in pm}
    assert len(pkeys) <= 8
    blob = b"".join(bytes.fromhex(v["tuple"]) for v in pm) * 40
    want = [v["accept"] for v in pm] * 40
    hemul.sbvk256hot_reset(256, 8, 30)
    got, st = _run(hemul, blob)
    assert got == want and st[2] == 0 and st[3] == len(pkeys), st
    got, st = _run(hemul, blob)
    assert got == want, [pm[i % 6]["name"] for i in range(len(want)) if got[i] != want[i]][:8]
    assert st[2] == len(want) and st[5] == 0, st              # every one of them was served from a wide comb
    for k in pkeys:
        assert hemul.sbvk256hot_comb_mismatches(hemul.sbvk256hot_wide_of_key(k)) == 0


def test_scalar_cases_from_the_8_bit_combs_and_after_promotion(hemul):
    """The wide16 and g20 cases of scalar_cases.cases("k256") with their rejecting twins, the list repeated until every key of it has
    passed min_hits: once from the 8-bit combs (the first batch promotes behind its verdicts), once served from the promoted combs.
    Both runs give the cases' own verdicts."""
    cs = sc.by_walker(sc.cases("k256"), "wide%d" % sc.K256_WIDE_BITS, "g%d" % sc.G_BITS["k256"])
    assert len(cs) >= 300 and any(c.expect for c in cs) and any(not c.expect for c in cs)
    keys = {c.tuple[96:] for c in cs}
    min_hits = 600
    reps = 1
    while min(sum(1 for c in cs if c.tuple[96:] == k) for k in keys) * reps < min_hits:
        reps += 1
    blob = sc.blob(cs) * reps
    want = [c.expect for c in cs] * reps
    hemul.sbvk256hot_reset(64, 4, min_hits)
    got, st = _run(hemul, blob)
    assert got == want, [cs[i % len(cs)].name for i in range(len(want)) if got[i] != want[i]][:8]
    assert st[2] == 0 and st[3] == len(keys), st
    got, st = _run(hemul, blob)
    assert got == want, [(cs[i % len(cs)].walker, cs[i % len(cs)].family, cs[i % len(cs)].name) for i in range(len(want)) if got[i] != want[i]][:8]
    assert st[2] == len(want) and st[5] == 0, st              # every lane was served from a promoted comb
    for k in keys:
        assert hemul.sbvk256hot_comb_mismatches(hemul.sbvk256hot_wide_of_key(k)) == 0


def test_wave_rule(hemul, koracle):
    """Three wavefronts of the key-sorted list, laid out through the group order the sort uses: 63 lanes of a promoted key and one of
    an unpromoted key stay with the 8-bit kernel; 63 wide lanes and one dead lane (a key that is no point) take the wide pass; a
    wavefront of dead lanes takes neither walk's verdict — it stays with the 8-bit kernel, which writes its rejects."""
    tuples, want = _gen(koracle, 0x3A7E, 1024, 2, 0)
    per_key = _by_key(tuples)
    (ka, ta), (kb, tb) = sorted(per_key.items(), key=lambda kv: -len(kv[1]))[:2]
    assert len(ta) >= 400 and len(tb) >= 400
    hemul.sbvk256hot_reset(64, 4, 300)
    warm = b"".join(ta[:400])
    got, st = _run(hemul, warm)                               # key A alone passes min_hits and is promoted
    assert all(got) and st[3] == 1
    assert hemul.sbvk256hot_wide_of_key(ka) == 0 and hemul.sbvk256hot_wide_of_key(kb) == NOT_CACHED
    dead = bytearray(ta[0])
    dead[159] ^= 1                                            # y + 1: off the curve
    dead = bytes(dead)
    # groups by first appearance: A, B, dead; three groups fill one row of the sort's order, so the list is A x 126 | B | dead x 65
    batch = b"".join(ta[:63]) + tb[0] + dead * 65 + b"".join(ta[63:126])
    got, st = _run(hemul, batch)
    n = len(batch) // 160
    assert got == _oracle(koracle, batch)
    assert got[:64] == [True] * 64 and not any(got[64:129]) and all(got[129:])
    # the list: group 0 (A, 126 lanes), group 1 (B, 1 lane), group 2 (dead, 65 lanes) = lanes 0..125 | 126 | 127..191
    cls = _classes(hemul)
    assert n == 192 and len(cls) == 3
    assert cls[0] == WIDE                                     # lanes 0..63: all A
    assert cls[1] == FULL                                     # lanes 64..127: 62 x A, B (live, unpromoted), one dead lane
    assert cls[2] == NONE                                     # lanes 128..191: all dead
    assert st[2] == 64 and st[4] == 1 and st[5] == 1 and st[6] == 1, st
    # 63 wide lanes and one dead lane: the wide pass; the dead lane is not counted
    batch2 = b"".join(ta[:63]) + dead
    got, st = _run(hemul, batch2)
    assert got == [True] * 63 + [False]
    assert _classes(hemul) == [WIDE] and st[2] == 63, st
    # 63 wide lanes and one lane of an unpromoted key: the 8-bit kernel
    batch3 = b"".join(ta[:63]) + tb[1]
    got, st = _run(hemul, batch3)
    assert got == [True] * 64
    assert _classes(hemul) == [FULL] and st[2] == 0, st
    # all dead: neither
    got, st = _run(hemul, dead * 64)
    assert not any(got) and _classes(hemul) == [NONE] and st[2] == 0 and st[4] == 0 and st[5] == 0 and st[6] == 1, st


def test_pool_follows_a_changing_signer_set(hemul, koracle):
    """Three disjoint sets of 4 signers over a pool of 4: the set that signs now takes the pool over from the set that stopped (decay
    every 16th batch, eviction with hysteresis: the shared lane functions).  The first set settles within 2 batches, a later one not
    before 3 — its counts must first pass twice the decayed counts of the owners; every re-assigned comb is the host builder's for
    its new owner; every verdict of every batch is the oracle's."""
    n = 1024
    sets = [_gen(koracle, 0x11FE + k, n, 4, 9) for k in range(3)]
    hemul.sbvk256hot_reset(1024, 4, 200)                      # the cache holds every key of the three sets, the corrupted ones included
    seen_owners = set()
    for k, (tuples, want) in enumerate(sets):
        signers = [key for key, v in _by_key(tuples).items() if len(v) > 100]
        assert len(signers) == 4 and not (set(signers) & seen_owners)
        settled_at = None
        for call in range(48):
            got, st = _run(hemul, tuples)
            assert got == want, (k, call)
            if st[2] >= n * 0.6:                              # most of the batch through the wide pass: this set owns the pool
                settled_at = call
                break
        assert settled_at is not None and (settled_at <= 2 if k == 0 else 3 <= settled_at), (k, settled_at)
        got, st = _run(hemul, tuples)
        assert got == want and st[3] == 4
        owners = {_owner(hemul, i) for i in range(4)}
        assert owners == set(signers), k
        for i in range(4):
            assert hemul.sbvk256hot_comb_mismatches(i) == 0, (k, i)
        seen_owners |= owners
    assert st[7] >= 8                                         # two take-overs of four combs


def test_forgetting_the_cache_forgets_the_promotions(hemul, koracle):
    tuples, want = _gen(koracle, 0xF0E, 512, 2, 8)
    hemul.sbvk256hot_reset(64, 4, 100)
    for _ in range(2):
        got, st = _run(hemul, tuples)
        assert got == want
    assert st[3] == 2 and st[2] > 0
    hemul.sbvk256hot_key_cache(0)
    hemul.sbvk256hot_key_cache(1)
    got, st = _run(hemul, tuples)                             # from cold again: combs are rebuilt, nobody is wide
    assert got == want and st[2] == 0 and st[3] == 2, st
    got, st = _run(hemul, tuples)
    assert got == want and st[2] > 0
    for i in range(2):
        assert hemul.sbvk256hot_comb_mismatches(i) == 0


def test_new_entries_are_exported_wrapped_and_off_by_default():
    lib = sbv.load()
    for name in ("hot_keys", "hot_key_stats", "hot_selfcheck"):
        assert getattr(lib, "sbv_secp256k1_" + name) is not None
        assert callable(getattr(sbv, "k256_" + name))
    hdr = open(os.path.join(HERE, "..", "include", "sbv.h")).read()
    for name in ("hot_keys", "hot_key_stats", "hot_selfcheck"):
        assert "sbv_secp256k1_%s(" % name in hdr
    # that the pool is off unless asked for is a matter of behaviour: tests/test_gpu_k256_hot.py::test_the_pool_is_off_unless_asked_for
    # holds a fresh process to it (capacity 0, nobody served wide); here, the setter before sbv_init only records the setting
    lib.sbv_secp256k1_hot_keys.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    assert lib.sbv_secp256k1_hot_keys(4097, 0) == -2          # SBV_EINVAL: more than 4 096 combs
