"""GPU tier: the grouping lists of a batch against a plain model (tests/group_model.py).

Every grouped batch leaves a hash table, representatives, counts, a group assignment, a key-sorted list with its cursors, an ungrouped
list and table slots behind — built by the cooperative kernels of consensus_amd/csrc/group_kernels_common.h (ballot rounds, LDS
tables and histograms, a 1024-lane scan), which have no host form — and the verdicts show next to nothing of it: a tuple listed twice
or a run split in two only costs time, a tuple left out of every list keeps the verdict byte of the batch before.  Here every call is
checked twice: the bitmap against the oracle's verdicts, and the read-out of the step (consensus_amd.debug_group_readout) against the
model's invariants, which hold for every legal interleaving of the atomics.  The shapes are the smallest at which each piece can go
wrong: the launch geometry (64 / 256 / 1024 / 8192 tuples and their neighbours), the layouts that steer the per-wavefront counting
(shortcut, one representative for all lanes, 63 ballot rounds), the thresholds with their sampling, the group counts at the rows of the
modulo-8 run order, at the scan's lanes and at the switch from LDS histograms to plain atomics (16 384), a flooded table, the key-table
cache, the unsorted step, and verdict bytes left by the previous batch.

Batches are real signatures from the oracles' generators (every 8th tuple with one flipped bit, so some keys are one-bit variants),
re-laid with numpy; where many distinct keys are wanted the key bytes are random (grouping happens before any curve check).  What needs
another process environment (SBV_GROUP_SORT, SBV_HASH_SEED, SBV_GROUP_SAMPLE_SHIFT) runs in a child: this file is its own driver."""
import ctypes
import json
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), HERE]

import numpy as np  # noqa: E402

import consensus_amd as sbv  # noqa: E402
import group_model as gm  # noqa: E402
import hashflood  # noqa: E402

THREADS = min(os.cpu_count() or 1, 16)
POOL, POOL_KEYS, PAD_KEYS = 4096, 61, 17100      # 61 signers: coprime to the generator's "every 8th tuple corrupted", so every key has rejected rows too
PAD = 1000                                   # key codes: 0..60 = the signers of the pool, PAD + j = random key bytes number j,
VAR, VARIANTS = 500, 150                     # VAR + j = the j-th one-bit variant of a signer's key (one pool row each, repeated when used again)
SCHEMES = {"p256": (gm.SCHEME_P256, 160, "sbvo_gen_batch", "sbvo_p256_verify_batch", "verify_batch"),
           "k256": (gm.SCHEME_SECP256K1, 160, "sbvo_k256_gen_batch", "sbvo_k256_verify_batch", "secp256k1_verify_batch"),
           "ed25519": (gm.SCHEME_ED25519, 128, "sbvo_ed25519_gen_batch", "sbvo_ed25519_verify_batch", "ed25519_verify_batch")}
STATS = {name: {"readouts": 0, "max_groups": 0} for name in SCHEMES}


class Scheme:
    """The tuples of one scheme a test draws from: POOL generated ones (61 signers, every 8th corrupted) and 2 x PAD_KEYS copies of
    them under random key bytes (pad key j on rows 2j and 2j + 1), each with the oracle's verdict."""

    def __init__(self, name, oracle):
        self.name = name
        self.id, self.stride, gen, ver, call = SCHEMES[name]
        self.keyloc = gm.KEYLOC[self.id]
        self.verify = getattr(sbv, call)
        _, off, words = self.keyloc
        kb = 4 * words
        g, v = getattr(oracle, gen), getattr(oracle, ver)
        g.argtypes = [ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        v.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
        self._oracle_verify = v
        tup, exp = ctypes.create_string_buffer(self.stride * POOL), ctypes.create_string_buffer(POOL // 8)
        g(0x67726F75, POOL, POOL_KEYS, 8, tup, exp, THREADS)
        pool = np.frombuffer(tup.raw, dtype=np.uint8).reshape(POOL, self.stride)
        pool_exp = np.unpackbits(np.frombuffer(exp.raw, dtype=np.uint8), bitorder="little")[:POOL].astype(bool)
        rng = np.random.default_rng(0x5EED + self.id)
        npad = 2 * PAD_KEYS if name == "p256" else 2 * 2700
        pad = pool[np.arange(npad) % POOL].copy()
        pad[:, off:off + kb] = np.repeat(rng.integers(0, 256, size=(npad // 2, kb), dtype=np.uint8), 2, axis=0)
        self.rows = np.concatenate([pool, pad])
        self.exp = np.concatenate([pool_exp, self.oracle(pad)])
        self.pad_base, self.pad_keys = POOL, npad // 2
        # the signers' rows by key and by verdict; a row whose key bytes were hit by the flipped bit is a one-bit variant: a key of its own
        keys = pool[:, off:off + kb]
        self.by_key = {True: [], False: [], None: []}
        self.variants, self.variant_of = [], []
        for k in range(POOL_KEYS):
            mine = np.arange(k, POOL, POOL_KEYS)
            uniq, inv, cnts = np.unique(keys[mine], axis=0, return_inverse=True, return_counts=True)
            same = mine[inv.reshape(-1) == np.argmax(cnts)]
            for r in np.setdiff1d(mine, same):
                assert int(np.unpackbits(keys[r] ^ keys[same[0]]).sum()) == 1          # one flipped bit, in the key bytes
                self.variants.append(int(r))
                self.variant_of.append(k)
            for want in (True, False, None):
                sel = same if want is None else same[pool_exp[same] == want]
                assert sel.size >= 1
                self.by_key[want].append(sel)
        self.variants, self.variant_of = np.array(self.variants), np.array(self.variant_of)
        assert self.variants.size >= VARIANTS

    def oracle(self, rows):
        rows = np.ascontiguousarray(rows)
        n = rows.shape[0]
        out = ctypes.create_string_buffer((n + 7) // 8)
        self._oracle_verify(rows.ctypes.data, n, out, THREADS)
        return np.unpackbits(np.frombuffer(out.raw, dtype=np.uint8), bitorder="little")[:n].astype(bool)

    def take(self, codes, valid=None, shift=0):
        """Row indices for a sequence of key codes: the m-th use of a code takes the (m + shift)-th of its rows, cyclically.  valid:
        only rows the oracle accepts / rejects (signers only)."""
        codes = np.asarray(codes, dtype=np.int64)
        order = np.argsort(codes, kind="stable")
        sc = codes[order]
        start = np.flatnonzero(np.concatenate(([True], sc[1:] != sc[:-1])))
        occ = np.empty(codes.size, dtype=np.int64)
        occ[order] = np.arange(codes.size) - np.repeat(start, np.diff(np.concatenate((start, [codes.size])))) + shift
        out = np.empty(codes.size, dtype=np.int64)
        is_pad = codes >= PAD
        assert (codes[is_pad] - PAD < self.pad_keys).all()
        out[is_pad] = self.pad_base + 2 * (codes[is_pad] - PAD) + (occ[is_pad] & 1)
        is_var = (codes >= VAR) & ~is_pad
        out[is_var] = self.variants[codes[is_var] - VAR]
        for k in np.unique(codes[~is_pad & ~is_var]):
            rows = self.by_key[valid][int(k)]
            sel = np.flatnonzero(codes == k)
            out[sel] = rows[occ[sel] % rows.size]
        return out


def run(s, idx, cache_before=None, dup_allowed=None, expect=None):
    """One call: bitmap against the oracle, read-out against the model, the serial advanced.  Returns the read-out."""
    batch = np.ascontiguousarray(s.rows[idx])
    n = batch.shape[0]
    serial = sbv.debug_group_header()[11]
    bm = s.verify(batch.tobytes(), n)
    got = np.unpackbits(np.frombuffer(bm, dtype=np.uint8), bitorder="little")[:n].astype(bool)
    want = s.exp[idx] if expect is None else expect
    assert (got == want).all(), f"{int((got != want).sum())} verdicts differ from the oracle's, first at {int(np.flatnonzero(got != want)[0])}"
    ro = sbv.debug_group_readout()
    assert ro is not None and ro["serial"] == serial + 1, "the grouped step did not run"
    assert ro["scheme"] == s.id and ro["n"] == n
    violations = gm.check(batch, s.keyloc, ro, cache_before=cache_before, bitmap=bm, dup_allowed=dup_allowed)
    assert violations == [], violations[:6]
    STATS[s.name]["readouts"] += 1
    STATS[s.name]["max_groups"] = max(STATS[s.name]["max_groups"], ro["groups"])
    return ro


# ---- layouts: key codes for n tuples ----------------------------------------------------------------------------------------------------
def lay_round_robin(n, K=40):
    return np.arange(n) % K                                    # a wavefront's first representative is nobody else's: the shortcut


def lay_blocks(n, length, K=40):
    return (np.arange(n) // length) % K                        # all lanes share one representative; runs straddle wavefronts (100)


def lay_one_key(n):
    return np.zeros(n, dtype=np.int64)


def lay_ninety(n):
    c = np.zeros(n, dtype=np.int64)
    rest = np.arange(9, n, 10)
    c[rest] = PAD + np.arange(rest.size)
    return c


def lay_wave63(n):
    """Per wavefront: its first key once more at lane 37, 62 distinct keys on the other lanes: 63 ballot rounds."""
    c = PAD + np.arange(n)
    w = np.arange(n) // 64
    first = (np.arange(n) % 64 == 0) | (np.arange(n) % 64 == 37)
    c[first] = w[first] % 8
    return c


def lay_unique(n):
    return PAD + np.arange(n)                                  # 0 groups: the sort kernels return early


def lay_variants(n):
    """All 61 signers round-robin, and among them 150 one-bit variants of their keys: 60 used once or twice (singles beside the key they
    differ from in one bit), 30 used 5 and 30 used 8 times (groups of their own).  A key comparison that skipped a word, or a bit,
    would merge a variant with its signer."""
    uses = np.array([1, 1, 2, 5, 8])[np.arange(VARIANTS) % 5]
    c = np.concatenate([np.repeat(VAR + np.arange(VARIANTS), uses), np.arange(n - int(uses.sum())) % POOL_KEYS])
    np.random.default_rng(61).shuffle(c)
    return c


def groups_by_key_bytes(s, idx, min_count):
    """Number of distinct keys — by their actual bytes — with at least min_count tuples in the batch."""
    _, off, words = s.keyloc
    _, counts = np.unique(s.rows[idx][:, off:off + 4 * words], axis=0, return_counts=True)
    return int((counts >= min_count).sum())


LAYOUTS = {"variants": lay_variants, "round_robin": lay_round_robin, "blocks64": lambda n: lay_blocks(n, 64), "blocks100": lambda n: lay_blocks(n, 100), "one_key": lay_one_key,
           "ninety": lay_ninety, "wave63": lay_wave63, "unique": lay_unique}


def lay_groups(G, uses=2, singles=37):
    """G keys with `uses` tuples each (the first 40 the signers, the rest random key bytes), and a few keys used once, shuffled."""
    keys = np.concatenate([np.arange(min(G, 40)), PAD + np.arange(max(G - 40, 0))])
    c = np.concatenate([np.repeat(keys, uses), PAD + max(G - 40, 0) + np.arange(singles)])
    np.random.default_rng(G).shuffle(c)
    return c


def lay_thresholds():
    """Keys used 1, 2, 3, 7, 8, 9, 14 ... 129 times: something on either side of every threshold, exact or sampled."""
    uses = [1, 2, 3, 7, 8, 9, 14, 15, 16, 17, 24, 31, 32, 33, 48, 63, 64, 65, 100, 129]
    c = np.concatenate([np.full(u, k) for k, u in enumerate(uses)] + [PAD + np.arange(50)])
    np.random.default_rng(7).shuffle(c)
    return c


def expected_sampling(min_count, n):
    """(min_count, sample_mask, min_samples) the step must report for an explicit threshold: exact below 16, every 8th tuple from 16
    on, and at most 32 below 2^18 tuples (sbv_api.hip: enqueue, variant_view)."""
    if n < (1 << 18) and min_count > 32:
        min_count = 32
    return (min_count,) + gm.threshold(min_count)


# ---- the child: cases that need another process environment ---------------------------------------------------------------------------
def _oracle_lib():
    return ctypes.CDLL(os.path.join(ROOT, "oracle", "libsbv_oracle.so"))


def child(case):
    sbv.init(0)
    lib = _oracle_lib()
    out = {"case": case, "facts": {}}
    if case == "sample_shift":                                 # the P-256 default path: 8 uses, counted on every 4th tuple
        s = Scheme("p256", lib)
        sbv.key_cache(False)
        sbv.set_grouping(True, 1, 0, 4096)
        ro = run(s, s.take(lay_thresholds()))
        out["facts"] = {k: ro[k] for k in ("min_count", "sample_mask", "min_samples", "groups")}
        run(s, s.take(lay_round_robin(2597)))
    elif case.startswith("unsorted:"):
        for name in (case.split(":")[1],):
            s = Scheme(name, lib)
            sbv.key_cache(False, 0, s.id)
            sbv.set_grouping(True, 1, 4, 4096)
            for lay in LAYOUTS.values():
                ro = run(s, s.take(lay(2597)))
                assert ro["sorted"] == 0
            sbv.set_grouping(True, 1, 2, 4096)
            ro = run(s, s.take(lay_groups(1033)))
            assert ro["sorted"] == 0
        out["facts"] = {"sorted": 0}
    elif case == "flood":
        for name, min_count, cache in (("p256", 2, False), ("ed25519", 2, False), ("p256", 1, True)):
            s = Scheme(name, lib)
            words = s.keyloc[2]
            sbv.key_cache(False, 0, s.id)
            if cache:
                sbv.key_cache(True, 1024, s.id)
            sbv.set_grouping(True, 1, min_count, 4096)
            flood = hashflood.colliding_keys(200, 16, 0, random.Random(3), nwords=words)
            honest = s.take(lay_round_robin(1000))
            rows = s.rows[s.take(PAD + np.arange(400) // 2)].copy()          # 200 pairs of tuples; their keys become the flood's
            for j in range(400):
                rows[j, s.keyloc[1]:s.keyloc[1] + 4 * words] = np.frombuffer(flood[j // 2], dtype=np.uint8)
            base = s.rows.shape[0]
            s.rows = np.concatenate([s.rows, rows])
            s.exp = np.concatenate([s.exp, s.oracle(rows)])
            idx = np.concatenate([honest, base + np.arange(400)])
            np.random.default_rng(1).shuffle(idx)
            ro = run(s, idx)
            assert ro["seed"] == 0 and ro["ht_mask"] <= 0xFFFF
            is_flood = idx >= base
            rep = ro["rep"].astype(np.int64)
            in_table = np.zeros(ro["n"], dtype=bool)
            in_table[ro["ht"][ro["ht"] != 0].astype(np.int64) - 1] = True
            entries = int((in_table & is_flood).sum())
            orphans = (rep == np.arange(ro["n"])) & ~in_table
            orphans &= is_flood
            assert entries <= 64
            assert int(orphans.sum()) == 400 - 2 * entries                     # every other tuple of the flood represents itself
            if min_count == 2:
                assert (ro["slots"][orphans] == gm.NONE).all()               # ... and is ungrouped
            out["facts"][f"{name}_{min_count}"] = {"entries": entries, "orphans": int(orphans.sum()), "groups": ro["groups"],
                                                   "cached": int(ro["cache_count"][0])}
    else:
        raise SystemExit(f"unknown case {case}")
    out["stats"] = STATS
    print(json.dumps(out))


if __name__ == "__main__":
    child(sys.argv[1])
    sys.exit(0)

import pytest  # noqa: E402

pytestmark = pytest.mark.gpu
ALL = ["p256", "k256", "ed25519"]


@pytest.fixture(scope="module")
def gpu():
    sbv.init(0)
    # the Ed25519 hot keys' pool (64 MiB per comb) is rebuilt with the comb pool whenever the group capacity changes — seconds per test
    # here, and nothing the grouping lists depend on: off for this module
    sbv.ed_hot_keys(0)
    yield sbv
    print("group structure read-outs:", json.dumps(STATS))           # (-s shows it) per scheme: read-outs checked, largest group count
    sbv.ed_hot_keys(1024)
    sbv.set_grouping(True, sbv.GROUP_MIN_BATCH_DEFAULT, 0, 0)
    for scheme, cap in ((sbv.SCHEME_P256, 16384), (sbv.SCHEME_SECP256K1, 1024), (sbv.SCHEME_ED25519, 1024)):
        sbv.key_cache(False, 0, scheme)
        sbv.key_cache(True, cap, scheme)


_pools = {}


@pytest.fixture
def scheme(request, gpu, oracle):
    name = request.param
    if name not in _pools:
        _pools[name] = Scheme(name, oracle)
    for sid in (sbv.SCHEME_P256, sbv.SCHEME_SECP256K1, sbv.SCHEME_ED25519):
        sbv.key_cache(False, 0, sid)                          # cache off unless a test says otherwise: every group cold, tslot = kc.cap + k
    return _pools[name]


def _run_child(case, env_extra):
    env = dict(os.environ)
    for k in ("SBV_HASH_SEED", "SBV_GROUP_SORT", "SBV_GROUP_SAMPLE_SHIFT"):
        env.pop(k, None)
    env.update(env_extra)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), case], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    for name, st in r["stats"].items():
        STATS[name]["readouts"] += st["readouts"]
        STATS[name]["max_groups"] = max(STATS[name]["max_groups"], st["max_groups"])
    return r


# ---- sizes at the launch geometry ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 8191, 8192, 8193, 16385])
@pytest.mark.parametrize("scheme", ALL, indirect=True)
def test_sizes_at_the_launch_geometry(scheme, n):
    sbv.set_grouping(True, 1, 4, 4096)
    ro = run(scheme, scheme.take(lay_round_robin(n)))
    assert ro["groups"] == (40 if n >= 160 else 0)


# ---- layouts that steer the per-wavefront counting ----------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("scheme", ALL, indirect=True)
def test_layouts(scheme, layout):
    sbv.set_grouping(True, 1, 4, 4096)
    idx = scheme.take(LAYOUTS[layout](2597))
    ro = run(scheme, idx)
    want = groups_by_key_bytes(scheme, idx, 4)
    assert ro["groups"] == want
    if layout == "variants":                                    # the signers and (bar two variants that flipped the same bit) 60 variants of theirs
        assert POOL_KEYS + 55 <= want <= POOL_KEYS + 60
    else:
        assert want == {"one_key": 1, "ninety": 1, "wave63": 8, "unique": 0, "blocks100": 26}.get(layout, 40)
    if layout == "unique":
        assert int(ro["counters"][1]) == 0 and int(ro["counters"][4]) == 2597


# ---- thresholds -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_count", [1, 8, 15, 16, 64, 10**6])
@pytest.mark.parametrize("scheme", ALL, indirect=True)
def test_thresholds_exact_and_sampled(scheme, min_count):
    """Below 2^18 tuples the product caps an explicit threshold at 32 (sbv_api.hip: enqueue, variant_view), so at these sizes 64 and
    10^6 run ONE configuration — 32 uses, every 8th tuple counted, min_samples 4 — and "nothing is eligible" is out of reach on the
    GPU under this tier's size limit (the emulator test covers 10^6 giving 0 groups).  Both cases stay: the header must report the cap."""
    sbv.set_grouping(True, 1, min_count, 4096)
    codes = lay_thresholds()
    ro = run(scheme, scheme.take(codes))
    assert (ro["min_count"], ro["sample_mask"], ro["min_samples"]) == expected_sampling(min_count, codes.size)
    if min_count < 16:                                          # exact: the keys with at least min_count tuples, nobody else
        uses = np.bincount(codes[codes < PAD])
        assert ro["groups"] == int((uses >= min_count).sum()) + (50 if min_count == 1 else 0)


def test_default_threshold_with_every_4th_tuple_counted():
    r = _run_child("sample_shift", {"SBV_GROUP_SAMPLE_SHIFT": "2"})
    assert (r["facts"]["min_count"], r["facts"]["sample_mask"], r["facts"]["min_samples"]) == (8, 3, 2), r


# ---- group counts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 7, 8, 9, 15, 16, 17, 1023, 1024, 1025, 1032, 1033])
@pytest.mark.parametrize("scheme", ALL, indirect=True)
def test_group_counts_at_the_rows_of_the_run_order_and_the_lanes_of_the_scan(scheme, groups):
    sbv.set_grouping(True, 1, 2, 4096)
    ro = run(scheme, scheme.take(lay_groups(groups)))
    assert ro["groups"] == groups


@pytest.mark.parametrize("groups", [2048, 2049])
@pytest.mark.parametrize("scheme", ["k256", "ed25519"], indirect=True)
def test_group_counts_at_the_capacity_of_the_variants(scheme, groups):
    sbv.set_grouping(True, 1, 2, 4096)
    ro = run(scheme, scheme.take(lay_groups(groups)))
    assert ro["max_groups"] == 2048 and ro["groups"] == 2048 and int(ro["counters"][0]) == groups


@pytest.mark.parametrize("max_groups", [3, 64])
@pytest.mark.parametrize("scheme", ALL, indirect=True)
def test_more_eligible_keys_than_groups(scheme, max_groups):
    sbv.set_grouping(True, 1, 2, max_groups)
    try:
        ro = run(scheme, scheme.take(lay_groups(100)))
        assert ro["groups"] == max_groups and int(ro["counters"][0]) == 100
        assert int(ro["counters"][1]) == 2 * max_groups                       # the rest is ungrouped (or rejected for its key)
    finally:
        sbv.set_grouping(True, 1, 2, 4096)


@pytest.mark.parametrize("groups", [16383, 16384, 16385, 17000])
@pytest.mark.parametrize("scheme", ["p256"], indirect=True)
def test_sort_from_the_last_histogram_to_plain_atomics(scheme, groups):
    """SBV_SORT_LDS_GROUPS = 16 384: the last batch one LDS histogram holds, the switch, and the direct atomics beyond."""
    sbv.set_grouping(True, 1, 2, 20000)
    try:
        ro = run(scheme, scheme.take(lay_groups(groups)))
        assert ro["max_groups"] == 20000 and ro["groups"] == groups
        assert (ro["groups"] > 16384) == (groups > 16384)
    finally:
        sbv.set_grouping(True, 1, 2, 4096)


# ---- the unsorted step and the flooded table ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["p256", "ed25519"])
def test_unsorted_step(name):
    r = _run_child("unsorted:" + name, {"SBV_GROUP_SORT": "0"})
    assert r["stats"][name]["readouts"] == len(LAYOUTS) + 1 and r["facts"] == {"sorted": 0}, r


def test_flooded_table():
    """200 keys on one home slot under a known seed, two tuples each, among honest tuples: at most 64 of them get entries, every other
    tuple of theirs is a legitimate orphan, verdicts are unchanged; with min_count 1 and the cache on an orphan is a group of its own and
    its key may be cached twice — the only duplicates the model admits."""
    r = _run_child("flood", {"SBV_HASH_SEED": "0"})
    for key in ("p256_2", "ed25519_2", "p256_1"):
        assert 0 < r["facts"][key]["entries"] <= 64 and r["facts"][key]["orphans"] >= 400 - 128, r
    one = r["facts"]["p256_1"]
    assert one["cached"] == one["groups"] == 40 + one["entries"] + one["orphans"], r         # every orphan a group and a cache slot of its own


# ---- the key-table cache --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["p256", "ed25519"], indirect=True)
def test_cache_cold_warm_half_new_and_too_small(scheme):
    sbv.set_grouping(True, 1, 4, 4096)
    sid = scheme.id

    def snapshot(ro):
        return {"keys": ro["cache_keys"].copy(), "count": ro["cache_count"].copy()}
    try:
        sbv.key_cache(True, 128, sid)                                          # empty (the fixture switched it off)
        ro = run(scheme, scheme.take(lay_round_robin(1000)))                   # cold: every group misses
        assert (int(ro["cache_count"][1]), int(ro["cache_count"][2])) == (0, 40) and ro["kc_cap"] == 128
        ro = run(scheme, scheme.take(lay_round_robin(1000), shift=7), cache_before=snapshot(ro))       # the same keys, other signatures
        assert (int(ro["cache_count"][1]), int(ro["cache_count"][2])) == (40, 0) and (ro["cold"] == 0).all()
        near = np.flatnonzero(scheme.variant_of[:VARIANTS] < 40)[:20]                                   # one-bit variants of CACHED keys arrive:
        idx = scheme.take(np.concatenate([lay_round_robin(800), np.repeat(VAR + near[:10], 5), VAR + near[10:]]), shift=11)
        misses = groups_by_key_bytes(scheme, idx, 4) - 40                                               # five uses: groups, and every one misses
        ro = run(scheme, idx, cache_before=snapshot(ro))
        assert 9 <= misses <= 10 and (int(ro["cache_count"][1]), int(ro["cache_count"][2])) == (40, misses)
        ro = run(scheme, scheme.take(20 + lay_round_robin(1000)), cache_before=snapshot(ro))            # half of the keys are new
        assert (int(ro["cache_count"][1]), int(ro["cache_count"][2])) == (20, 20)
        sbv.key_cache(False, 0, sid)
        sbv.key_cache(True, 16, sid)                                           # a capacity below the key set
        ro = run(scheme, scheme.take(lay_round_robin(1000)))
        assert ro["kc_cap"] == 16 and int((ro["tslot"] < 16).sum()) == 16 and int((ro["tslot"] >= 16).sum()) == 24
        ro = run(scheme, scheme.take(lay_round_robin(1000), shift=3), cache_before=snapshot(ro))
        assert (int(ro["cache_count"][1]), int(ro["cache_count"][2])) == (16, 24)
    finally:
        sbv.key_cache(False, 0, sid)


# ---- verdict bytes of the batch before ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["p256", "k256"], indirect=True)
def test_no_verdict_byte_survives_from_the_batch_before(scheme):
    """The verdict bytes are not cleared between batches of these two schemes: a tuple that no list holds would keep what the batch before
    left at its index.  All valid, then — same n, other layout — all invalid in every class (grouped, ungrouped, rejected for the key):
    every bit and every byte 0; then the other way round."""
    sbv.set_grouping(True, 1, 4, 4096)
    n = 1500
    valid = scheme.take(np.concatenate([lay_round_robin(n - 40, 30), 30 + np.arange(40) % 20]), valid=True)     # groups, and keys used twice
    invalid = np.concatenate([scheme.take(40 + np.arange(n - 500) % 20, valid=False),                           # grouped under other keys
                              scheme.take(np.arange(20), valid=False),                                          # ungrouped, good keys
                              scheme.take(PAD + np.arange(480))])                                               # random key bytes
    np.random.default_rng(2).shuffle(invalid)
    assert scheme.exp[valid].all() and not scheme.exp[invalid].any()
    for first, second in ((valid, invalid), (invalid, valid)):
        run(scheme, first)
        ro = run(scheme, second)
        assert (ro["acc"] == (1 if second is valid else 0)).all()
        assert int(ro["counters"][1]) > 0 and int(ro["counters"][2]) > 0
