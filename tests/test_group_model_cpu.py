"""CPU tier: the checker of the grouping lists (tests/group_model.py) has teeth before it is pointed at a GPU.

A sequential builder (group_model.build_readout: the lane functions of p256_group.h, one tuple after the other) makes correct read-outs
for small batches of all three tuple formats — sorted and unsorted step, cache off / cold / warm / full, a flooded table with orphans —
and the checker finds nothing.  Then one mutation at a time, each of a kind a wrong cooperative kernel could produce (a tuple dropped
from the sorted list, a workgroup's share missing from a count, a run order of 0, 1, 2, ...), must be reported by the invariant it
breaks.  Last, the emulator's read-out (tests/emul: the lane functions compiled from the product headers) of the P-256, Ed25519 and
secp256k1 grouped steps passes the same checker unchanged."""
import copy
import ctypes
import random

import numpy as np
import pytest

import consensus_amd as sbv
import ed25519_py as ed
import group_model as gm
import hashflood
import k256_py as kc
import p256_py as ec
from test_emul_device_algo import emul  # noqa: F401  (the fixture that builds tests/emul)

P256, K256, ED = gm.SCHEME_P256, gm.SCHEME_SECP256K1, gm.SCHEME_ED25519


def _good_keys(scheme, count):
    if scheme == ED:
        return [ed.public_key(bytes([i + 1]) * 32) for i in range(count)]
    mod = ec if scheme == P256 else kc
    out, pt = [], None
    for _ in range(count):
        pt = mod.pt_add(pt, mod.G)
        out.append(pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big"))
    return out


def _batch(scheme, keys, rng):
    """One tuple per entry of `keys`: random bytes around the key (the grouping reads nothing else)."""
    stride, off, words = gm.KEYLOC[scheme]
    a = np.frombuffer(bytes(rng.getrandbits(8) for _ in range(stride * len(keys))), dtype=np.uint8).reshape(len(keys), stride).copy()
    for i, k in enumerate(keys):
        a[i, off:off + 4 * words] = np.frombuffer(k, dtype=np.uint8)
    return a.tobytes()


def _bad_key(scheme, rng):
    while True:
        k = bytes(rng.getrandbits(8) for _ in range(4 * gm.KEYLOC[scheme][2]))
        if not gm.key_ok(scheme, k):
            return k


def _mixed(scheme, rng, n=700, nkeys=9):
    """Round-robin over good keys with one-bit variants and bad singles in between: groups of every size around a threshold of 8, good
    and bad keys on the ungrouped side, more than two workgroups of 256."""
    good = _good_keys(scheme, nkeys + 3)
    keys = []
    for i in range(n):
        k = good[(i * i + i // 7) % nkeys] if i % 5 else good[i % 3]
        if i % 11 == 10:
            k = bytes([k[0] ^ (1 << (i % 8))]) + k[1:]           # a one-bit variant, repeated now and then
        if i % 17 == 16:
            k = _bad_key(scheme, rng)
        if i % 97 == 96:
            k = good[nkeys + i % 3]                             # good keys below any threshold but 1: the one-lane list
        keys.append(k)
    return _batch(scheme, keys, rng)


# ---- the twins ---------------------------------------------------------------------------------------------------------------------------
def test_the_numpy_hash_is_the_scalar_twin():
    rng = random.Random(1)
    for words in (16, 8):
        w = np.array([[rng.getrandbits(32) for _ in range(words)] for _ in range(50)], dtype=np.uint32)
        for seed in (0, 1, 0xDEADBEEF, 0xFFFFFFFF):
            want = [hashflood.grouping_hash([int(x) for x in row], seed) for row in w]
            assert gm.grouping_hash(w, seed).tolist() == want


def test_key_checks_agree_with_the_python_oracles():
    rng = random.Random(2)
    for scheme, mod in ((P256, ec), (K256, kc)):
        for k in _good_keys(scheme, 4):
            assert gm.key_ok(scheme, k)
            assert not gm.key_ok(scheme, k[:63] + bytes([k[63] ^ 1]))
        assert not gm.key_ok(scheme, mod.P.to_bytes(32, "big") + bytes(32))                       # x = p: not below p
    for _ in range(40):
        k = bytes(rng.getrandbits(8) for _ in range(32))
        y = int.from_bytes(k, "little") & ((1 << 255) - 1)
        if y < ed.P:                                                                              # the oracle's decompress refuses y >= p, the device takes it mod p
            x_is_zero = y in (1, ed.P - 1)
            assert gm.key_ok(ED, k) == (ed.decompress(k) is not None) or x_is_zero
    assert gm.key_ok(ED, ed.public_key(b"k" * 32))
    assert gm.sort_order(17).tolist() == [0, 8, 16, 1, 9, 2, 10, 3, 11, 4, 12, 5, 13, 6, 14, 7, 15]


# ---- correct read-outs pass -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [P256, K256, ED])
@pytest.mark.parametrize("sorted_step", [True, False])
@pytest.mark.parametrize("min_count,max_groups", [(1, 4096), (8, 4096), (16, 64), (2, 3)])
def test_builder_readouts_pass(scheme, sorted_step, min_count, max_groups):
    rng = random.Random(100 + scheme)
    batch = _mixed(scheme, rng)
    ro = gm.build_readout(batch, scheme, 11, min_count, max_groups, seed=0x1234ABCD, sorted_step=sorted_step)
    assert gm.check(batch, gm.KEYLOC[scheme], ro) == []
    if max_groups == 3:
        assert ro["groups"] == 3 < int(ro["counters"][0])


@pytest.mark.parametrize("scheme", [P256, ED])
def test_builder_readouts_pass_with_the_cache_cold_warm_and_full(scheme):
    rng = random.Random(7)
    cache = {"keys": np.zeros((1, 16), dtype=np.uint32), "count": np.zeros(4, dtype=np.uint32)}
    loc = gm.KEYLOC[scheme]
    first = _mixed(scheme, rng, n=400, nkeys=6)
    ro = gm.build_readout(first, scheme, 10, 8, 64, cache=cache, kc_cap=8)
    assert gm.check(first, loc, ro) == [] and int(ro["cache_count"][2]) == ro["groups"] > 0
    before = copy.deepcopy(cache)
    second = _mixed(scheme, rng, n=300, nkeys=9)                   # the same six keys, now cached (grouped whatever their count), and three new ones
    ro = gm.build_readout(second, scheme, 10, 8, 64, cache=cache, kc_cap=8)
    assert gm.check(second, loc, ro, cache_before=before) == []
    assert int(ro["cache_count"][1]) >= 6 and int(ro["cache_count"][0]) == 8 and (ro["tslot"] >= 8).any()       # hits, a full cache, per-batch slots
    assert "cache.cold" in _names(gm.check(second, loc, ro))                                                   # ... which only the read-out from before explains


def _flooded(min_count, with_cache):
    rng = random.Random(11)
    flood = hashflood.colliding_keys(80, 10, 0, rng)
    keys = _good_keys(P256, 5) * 8
    for k in flood:
        keys += [k, k]
    rng.shuffle(keys)
    batch = _batch(P256, keys, rng)
    cache = {"keys": np.zeros((1, 16), dtype=np.uint32), "count": np.zeros(4, dtype=np.uint32)} if with_cache else None
    return batch, gm.build_readout(batch, P256, 10, min_count, 4096, seed=0, cache=cache, kc_cap=512)


@pytest.mark.parametrize("min_count,with_cache", [(2, False), (1, True)])
def test_flooded_table_with_legitimate_orphans_passes(min_count, with_cache):
    batch, ro = _flooded(min_count, with_cache)
    assert gm.check(batch, gm.KEYLOC[P256], ro) == []
    rep = ro["rep"].astype(np.int64)
    in_table = np.zeros(ro["n"], dtype=bool)
    in_table[ro["ht"][ro["ht"] != 0].astype(np.int64) - 1] = True
    orphans = np.flatnonzero((rep == np.arange(ro["n"])) & ~in_table)
    assert orphans.size == 2 * (80 - 64 + 5) or orphans.size >= 2 * 16          # at most 64 keys of the flood found room in the window
    if with_cache:                                                                # min_count 1: every orphan is a group of its own, its key cached twice
        keys = [bytes(r) for r in ro["cache_keys"].view(np.uint8).reshape(-1, 64)]
        assert len(set(keys)) < len(keys)
        other = copy.deepcopy(ro)
        other["min_count"] = 2                                                    # the same cache behind a batch that cannot explain the duplicates
        assert "cache.dup" in _names(gm.check(batch, gm.KEYLOC[P256], other))


# ---- one mutation at a time -----------------------------------------------------------------------------------------------------------
def _names(violations):
    return {v.split(":")[0] for v in violations}


@pytest.fixture(scope="module")
def base():
    rng = random.Random(42)
    batch = _mixed(P256, rng)
    cache = {"keys": np.zeros((1, 16), dtype=np.uint32), "count": np.zeros(4, dtype=np.uint32)}
    warm = _batch(P256, _good_keys(P256, 17)[12:] * 9, rng)                # five keys the batch under test does not use
    gm.build_readout(warm, P256, 10, 8, 64, cache=cache, kc_cap=64)
    before = copy.deepcopy(cache)
    ro = gm.build_readout(batch, P256, 11, 8, 4096, seed=0x51ED, cache=cache, kc_cap=64)
    assert gm.check(batch, gm.KEYLOC[P256], ro, cache_before=before) == []
    assert ro["groups"] >= 9 and int(ro["counters"][3]) > 0 and int(ro["counters"][2]) > 0
    return batch, ro, before


def _run_of(ro, k):
    return np.flatnonzero(ro["grp_of"] == k)


def m_dropped(ro, batch):
    ro["grp_idx"] = np.delete(ro["grp_idx"], 5)
    ro["grp_of"] = np.delete(ro["grp_of"], 5)
    ro["counters"][1] -= 1


def m_twice(ro, batch):
    run = _run_of(ro, 1)
    ro["grp_idx"][run[0]] = ro["grp_idx"][run[1]]


def m_swapped(ro, batch):
    a, b = _run_of(ro, 0)[0], _run_of(ro, 1)[0]
    for name in ("grp_idx", "grp_of"):
        ro[name][a], ro[name][b] = ro[name][b], ro[name][a]


def m_gcount(ro, batch):
    ro["gcount"][2] += 1


def m_natural_order(ro, batch):
    order = np.argsort(ro["grp_of"], kind="stable")
    ro["grp_idx"], ro["grp_of"] = ro["grp_idx"][order], ro["grp_of"][order]


def m_one_sample_short(ro, batch):
    ro["min_count"] = ro["min_samples"] = int(ro["cnt"][ro["group_rep"]].min()) + 1


def m_workgroup_share(ro, batch):
    rep = ro["rep"].astype(np.int64)
    r = int(ro["group_rep"][0])
    second = np.flatnonzero((rep == r) & (np.arange(ro["n"]) // 256 == 1))          # what the workgroup of tuples 256..511 counted
    assert second.size
    ro["cnt"][r] -= second.size


def m_foreign_rep(ro, batch):
    a, b = int(ro["group_rep"][0]), int(ro["group_rep"][1])
    i = int(np.flatnonzero(ro["rep"] == a)[-1])
    ro["rep"][i] = b


def m_foreign_tslot(ro, batch):
    used = set(ro["tslot"].tolist())
    free = [s for s in range(int(min(ro["cache_count"][0], ro["kc_cap"]))) if s not in used]
    ro["tslot"][3] = free[0]                                                           # a cached comb of a key this batch does not hold


def m_shared_tslot(ro, batch):
    ro["tslot"][3] = ro["tslot"][4]


def m_bad_key_listed(ro, batch):
    listed = set(ro["ung_idx"].tolist())
    i = next(int(c) for c in ro["ung_cand"] if int(c) not in listed)
    ro["ung_idx"] = np.append(ro["ung_idx"], np.uint32(i))
    ro["counters"][2] += 1
    ro["counters"][3] -= 1


def m_acc_two(ro, batch):
    ro["acc"][17] = 2


def m_slots_mismatch(ro, batch):
    i = int(ro["grp_idx"][0])
    ro["slots"][i] = gm.NONE


def m_gcursor(ro, batch):
    ro["gcursor"][1] -= 1


def m_candidate_lost(ro, batch):
    ro["ung_cand"] = ro["ung_cand"][:-1]
    ro["counters"][4] -= 1


MUTATIONS = [(m_dropped, "sort.perm"), (m_twice, "sort.perm"), (m_swapped, "sort.runs"), (m_gcount, "sort.gcount"), (m_natural_order, "sort.order"),
             (m_one_sample_short, "groups.eligible"), (m_workgroup_share, "cnt.exact"), (m_foreign_rep, "rep.key"), (m_foreign_tslot, "cache.key"),
             (m_shared_tslot, "cache.tslot_unique"), (m_bad_key_listed, "ung.idx"), (m_acc_two, "acc.range"), (m_slots_mismatch, "slots.match"),
             (m_gcursor, "sort.gcursor"), (m_candidate_lost, "ung.cand")]


@pytest.mark.parametrize("mutate,name", MUTATIONS, ids=[m.__name__[2:] for m, _ in MUTATIONS])
def test_a_mutation_is_reported_by_the_invariant_it_breaks(base, mutate, name):
    batch, ro, before = base
    ro = copy.deepcopy(ro)
    mutate(ro, batch)
    assert name in _names(gm.check(batch, gm.KEYLOC[P256], ro, cache_before=before))


def test_an_orphan_whose_probe_window_has_a_hole_is_reported():
    batch, ro = _flooded(2, False)
    assert gm.check(batch, gm.KEYLOC[P256], ro) == []
    ro = copy.deepcopy(ro)
    # a tuple of a key that HAS its entry gives up as if the window were full: its window holds its key
    rep = ro["rep"].astype(np.int64)
    i = int(np.flatnonzero(rep != np.arange(ro["n"]))[0])
    ro["rep"][i] = i
    assert "orphan.window" in _names(gm.check(batch, gm.KEYLOC[P256], ro))
    # and a real orphan of the flood in front of a window from which one entry has gone
    batch, ro = _flooded(2, False)
    words = gm.key_words(batch, gm.KEYLOC[P256])
    home = int(gm.grouping_hash(words, 0)[[i for i in range(ro["n"]) if ro["rep"][i] == i and (ro["ht"] != i + 1).all()][0]]) & ro["ht_mask"]
    ro["ht"][(home + 63) & ro["ht_mask"]] = 0
    assert "orphan.window" in _names(gm.check(batch, gm.KEYLOC[P256], ro))


def test_the_verdict_bytes_are_compared_with_the_bitmap(base):
    batch, ro, before = base
    ro = copy.deepcopy(ro)
    ro["acc"][::3] = 1
    ro["acc"][np.flatnonzero(ro["slots"] == gm.NONE)] = 0
    bitmap = np.packbits(ro["acc"] == 1, bitorder="little").tobytes()
    assert gm.check(batch, gm.KEYLOC[P256], ro, cache_before=before, bitmap=bitmap) == []
    flipped = bytearray(bitmap)
    flipped[2] ^= 0x10
    assert "acc.bitmap" in _names(gm.check(batch, gm.KEYLOC[P256], ro, cache_before=before, bitmap=bytes(flipped)))


# ---- the emulator's read-out: the lane functions' own output passes unchanged ---------------------------------------------------------
def _emul_readout(emul):
    emul.sbve_group_readout_array.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]

    def header():
        out = (ctypes.c_uint32 * 16)()
        emul.sbve_group_readout_header(out)
        return tuple(out)
    return sbv.group_readout_from(header, emul.sbve_group_readout_array)


def _gen(oracle, name, stride, seed, n, nkeys, inv):
    fn = getattr(oracle, name)
    fn.argtypes = [ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    tup, exp = ctypes.create_string_buffer(stride * n), ctypes.create_string_buffer((n + 7) // 8)
    fn(seed, n, nkeys, inv, tup, exp, 4)
    return tup.raw, exp.raw


def test_emulated_p256_grouped_steps_pass_the_checker(emul, oracle, golden_vectors):
    """The batches of test_grouped_by_key_inside_the_batch_matches_generic and of the key-sorted test, sorted and unsorted, and the
    flooded table of the probe-bound test."""
    emul.sbve_p256_verify_batch_grouped.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                    ctypes.c_void_p]
    emul.sbve_set_hash_seed.argtypes = [ctypes.c_uint32]
    vs = [v for v in golden_vectors if v["kind"] == "tuple"]
    n = 900
    tup, exp = _gen(oracle, "sbvo_gen_batch", 160, 0x6B, n, 7, 5)
    off = next(bytes.fromhex(v["tuple"]) for v in vs if v["name"] == "q_off_curve_y_plus_1")
    allt = b"".join(bytes.fromhex(v["tuple"]) for v in vs) + tup + off * 40          # an INVALID key becomes a group
    total = len(allt) // 160
    serial = 0
    try:
        for sort, configs in ((1, [(8, 64, 12, 0), (64, 64, 12, 0), (1, 4096, 12, 0x9E3779B9), (8, 3, 12, 5), (2, 64, 11, 0), (10**6, 64, 12, 0)]),
                              (0, [(8, 64, 12, 0), (1, 4096, 12, 7)])):
            emul.sbve_set_group_sort(sort)
            for min_count, max_groups, ht_bits, seed in configs:
                emul.sbve_set_hash_seed(seed)
                bm = ctypes.create_string_buffer((total + 7) // 8)
                emul.sbve_p256_verify_batch_grouped(allt, total, bm, min_count, max_groups, ht_bits, None)
                ro = _emul_readout(emul)
                assert ro["serial"] > serial and ro["sorted"] == sort and ro["scheme"] == P256 and ro["seed"] == seed
                serial = ro["serial"]
                assert gm.check(allt, gm.KEYLOC[P256], ro, bitmap=bm.raw) == [], (sort, min_count, max_groups)
                assert ro["groups"] == {3: 3, 10**6: 0}.get(max_groups if max_groups == 3 else min_count, ro["groups"])
        # a flooded table (seed 0, 2^10 entries): orphans, found legitimate
        emul.sbve_set_group_sort(1)
        emul.sbve_set_hash_seed(0)
        rng = random.Random(5)
        flood = hashflood.colliding_keys(70, 10, 0, rng)
        rows = np.frombuffer(tup, dtype=np.uint8).reshape(n, 160)[:200].copy()
        for j in range(140):
            rows[j, 96:160] = np.frombuffer(flood[j // 2], dtype=np.uint8)
        blob = rows.tobytes()
        bm = ctypes.create_string_buffer(25)
        emul.sbve_p256_verify_batch_grouped(blob, 200, bm, 2, 64, 10, None)
        ro = _emul_readout(emul)
        assert gm.check(blob, gm.KEYLOC[P256], ro, bitmap=bm.raw) == []
        assert int(np.count_nonzero(ro["ht"])) < len(set(gm.key_words(blob, gm.KEYLOC[P256]).view(np.uint8).reshape(200, 64).tobytes()[i * 64:(i + 1) * 64] for i in range(200)))
    finally:
        emul.sbve_set_group_sort(1)
        emul.sbve_set_hash_seed(0)


def test_emulated_p256_cache_steps_pass_the_checker(emul, oracle):
    emul.sbve_p256_verify_batch_grouped.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                    ctypes.c_void_p]
    emul.sbve_key_cache.argtypes = [ctypes.c_int, ctypes.c_uint32]
    n = 192
    try:
        emul.sbve_key_cache(1, 8)
        before = None
        for seed, nkeys in ((0xCA, 5), (0xCA, 5), (0xCA, 12)):               # cold, warm, more keys than the cache holds
            tup, exp = _gen(oracle, "sbvo_gen_batch", 160, seed, n, nkeys, 6)
            bm = ctypes.create_string_buffer(n // 8)
            emul.sbve_p256_verify_batch_grouped(tup, n, bm, 8, 64, 12, None)
            ro = _emul_readout(emul)
            assert gm.check(tup, gm.KEYLOC[P256], ro, cache_before=before, bitmap=bm.raw) == [] and bm.raw == exp
            before = {"keys": ro["cache_keys"].copy(), "count": ro["cache_count"].copy()}
        assert int(ro["cache_count"][1]) == 5 and (ro["tslot"] >= 8).any()
    finally:
        emul.sbve_key_cache(0, 0)


def test_emulated_ed25519_and_secp256k1_grouped_steps_pass_the_checker(emul, oracle):
    emul.sbve_ed25519_verify_batch_grouped.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                       ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    emul.sbve_k256_verify_batch_grouped.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                    ctypes.c_int, ctypes.c_void_p]
    n = 192
    rng = random.Random(9)
    tup, exp = _gen(oracle, "sbvo_ed25519_gen_batch", 128, 0xED25, n, 7, 5)
    rows = np.frombuffer(tup, dtype=np.uint8).reshape(n, 128).copy()
    for i in range(0, n, 13):                                                 # singles with random key bytes: half of them are no points
        rows[i, 64:96] = np.frombuffer(bytes(rng.getrandbits(8) for _ in range(32)), dtype=np.uint8)
    blob = rows.tobytes()
    try:
        for sort in (1, 0):
            emul.sbve_set_group_sort(sort)
            for min_count, max_groups in ((8, 64), (1, 64), (2, 3)):
                bm = ctypes.create_string_buffer(n // 8)
                emul.sbve_ed25519_verify_batch_grouped(blob, n, bm, min_count, max_groups, 12, 2, 4, None)
                ro = _emul_readout(emul)
                assert ro["scheme"] == ED and ro["sorted"] == sort
                assert gm.check(blob, gm.KEYLOC[ED], ro, bitmap=bm.raw) == [], (sort, min_count, max_groups)
    finally:
        emul.sbve_set_group_sort(1)
    tup, exp = _gen(oracle, "sbvo_k256_gen_batch", 160, 0x6B, n, 6, 5)
    for min_count, max_groups in ((2, 512), (8, 64), (4, 2)):
        bm = ctypes.create_string_buffer(n // 8)
        emul.sbve_k256_verify_batch_grouped(tup, n, bm, min_count, max_groups, 12, 2, None)
        ro = _emul_readout(emul)
        assert ro["scheme"] == K256
        assert gm.check(tup, gm.KEYLOC[K256], ro, bitmap=bm.raw) == [] and bm.raw == exp, (min_count, max_groups)
