"""Test helper: a plain model of the in-step key grouping (consensus_amd/csrc/p256_group.h, group_kernels_common.h), in Python and numpy.

check(batch, keyloc, ro, ...) takes the bytes of a batch, where its tuple format keeps the key (stride, offset, 32-bit words: 160 / 96 /
16 for P-256 and secp256k1, 128 / 64 / 8 for Ed25519) and a READ-OUT of the state a grouped step left behind (the dict of
consensus_amd.debug_group_readout, of the emulator's twin, or of build_readout below) and returns the list of violated invariants as
strings "name: detail".  No invariant depends on which tuple won a compare-and-swap or in which order atomics landed: each holds for
every legal interleaving of the kernels and fails for every result that no interleaving can produce.

    rep.*     representatives: key bytes, idempotence, who may point at whom
    orphan.*  a tuple that represents itself without a table entry: only behind a full probe window of other keys
    ht.*      the open-addressing table: entries are non-orphan representatives, once each, within the probe bound, no hole on the way
    cnt.*     the sampled counts per representative
    groups.*  who got a group, counters[0], the bijection group_rep <-> slot_of, slots
    ung.*     the candidates, the ungrouped list behind the key check, counters[3] and the verdict bytes of the rejected
    sort.*    the key-sorted list: exact counts, a permutation, grp_of, contiguous runs in the order of group_sort_group_at, cursors
    list.*    the unsorted step's grouped list (a permutation, any order)
    cache.*   table slots of the groups against the scheme's key-table cache
    acc.*     verdict bytes against the returned bitmap

build_readout() is the sequential reference builder: the lane functions of p256_group.h, one tuple after the other."""
import numpy as np

NONE = 0xFFFFFFFF
MAX_PROBES = 64
SCHEME_P256, SCHEME_SECP256K1, SCHEME_ED25519 = 0, 1, 2
KEYLOC = {SCHEME_P256: (160, 96, 16), SCHEME_SECP256K1: (160, 96, 16), SCHEME_ED25519: (128, 64, 8)}
_M = np.uint64(0xFFFFFFFF)


def key_words(batch, keyloc):
    """[n][words] uint32: the key words of every tuple as the device loads them (little-endian)."""
    stride, off, words = keyloc
    a = np.frombuffer(bytes(batch), dtype=np.uint8) if not isinstance(batch, np.ndarray) else batch.reshape(-1)
    n = a.size // stride
    return np.ascontiguousarray(a[:n * stride].reshape(n, stride)[:, off:off + 4 * words]).view("<u4").reshape(n, words)


def grouping_hash(words, seed):
    """numpy twin of group_find_rep_t's hash (tests/hashflood.py has the scalar one): [n][words] uint32 -> [n] uint32."""
    w = words.astype(np.uint64)
    seed = np.uint64(seed)
    h = np.full(w.shape[0], 0x9E3779B1, dtype=np.uint64) ^ seed
    for j in range(w.shape[1]):
        h = ((h ^ w[:, j]) * np.uint64(0x85EBCA77)) & _M
        h ^= h >> np.uint64(15)
    h = ((h ^ ((seed * np.uint64(0x27D4EB2F)) & _M)) * np.uint64(0xC2B2AE3D)) & _M
    return (h ^ (h >> np.uint64(16))).astype(np.uint32)


def group_sampled(i, sample_mask):
    """numpy twin of p256_group.h's group_sampled: which tuple indices are counted."""
    h = (np.asarray(i, dtype=np.uint64) * np.uint64(0x9E3779B1)) & _M
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x85EBCA77)) & _M
    return ((h >> np.uint64(24)) & np.uint64(sample_mask)) == 0


def sort_order(groups):
    """The groups in the order of their runs (group_sort_group_at: 0, 8, 16, ..., 1, 9, ...)."""
    rows = (groups + 7) >> 3
    p = np.arange(rows * 8, dtype=np.int64)
    k = (p % max(rows, 1)) * 8 + p // max(rows, 1)
    return k[k < groups]


def threshold(min_count, shift=None):
    """(sample_mask, min_samples) of group_set_threshold (shift None) / group_set_sampling."""
    if shift is None:
        shift = 3 if min_count >= 16 else 0
    return (1 << shift) - 1, max(min_count >> shift, 1)


# ---- the curve checks in front of the one-lane kernels (Python twins of the oracles) -------------------------------------------------
def _key_ok_weierstrass(kb, p, a, b):
    x, y = int.from_bytes(kb[:32], "big"), int.from_bytes(kb[32:], "big")
    return x < p and y < p and (y * y - (x * x * x + a * x + b)) % p == 0


def key_ok(scheme, kb):
    """The verdict of the key check on the key bytes of one tuple: pointFromAffine (P-256), the same on secp256k1, and for Ed25519
    whether the encoding decompresses (ed25519_core.h: a non-canonical y is taken mod p, "-0" is accepted)."""
    kb = bytes(kb)
    if scheme == SCHEME_P256:
        import p256_py as ec
        return _key_ok_weierstrass(kb, ec.P, ec.A, ec.B)
    if scheme == SCHEME_SECP256K1:
        import k256_py as kc
        return _key_ok_weierstrass(kb, kc.P, 0, kc.B)
    import ed25519_py as ed
    y = (int.from_bytes(kb, "little") & ((1 << 255) - 1)) % ed.P
    u, v = (y * y - 1) % ed.P, (ed.D * y * y + 1) % ed.P
    x2 = u * pow(v, -1, ed.P) % ed.P
    return x2 == 0 or pow(x2, (ed.P - 1) // 2, ed.P) == 1


def _key16(words):
    """[m][16] cache key words of [m][words] key words (Ed25519: padded with zeros)."""
    out = np.zeros((words.shape[0], 16), dtype=np.uint32)
    out[:, :words.shape[1]] = words
    return out


def _rows_as_ids(*arrays):
    """One id per distinct row over several [m_i][w] arrays: list of id arrays."""
    allrows = np.concatenate(arrays, axis=0) if len(arrays) > 1 else arrays[0]
    if allrows.shape[0] == 0:
        return [np.zeros(0, dtype=np.int64) for _ in arrays]
    void = np.ascontiguousarray(allrows).view(np.dtype((np.void, allrows.dtype.itemsize * allrows.shape[1]))).reshape(-1)
    _, inv = np.unique(void, return_inverse=True)
    inv = inv.reshape(-1)
    out, at = [], 0
    for a in arrays:
        out.append(inv[at:at + a.shape[0]])
        at += a.shape[0]
    return out


def _zeros_between(zcum, a, b, size):
    """Number of empty table entries in the circular range [a, b) of lengths < size (zcum: exclusive prefix sums of `entry == 0`)."""
    a, b = a.astype(np.int64), b.astype(np.int64)
    return np.where(b >= a, zcum[b] - zcum[a], zcum[size] - zcum[a] + zcum[b])


class _Report(list):
    def add(self, name, detail):
        if len(self) < 200:
            self.append(f"{name}: {detail}")


def _first(mask):
    idx = np.flatnonzero(mask)
    return f"{idx.size} of them, first at {int(idx[0])}" if idx.size else "none"


def check(batch, keyloc, ro, cache_before=None, bitmap=None, dup_allowed=None):
    """Violated invariants of read-out `ro` for `batch` (module docstring).  cache_before: {"keys": [m][16] words, "count": [4]} of the
    scheme's key-table cache read out BEFORE the batch (None: it was empty).  bitmap: the verdict bitmap the call returned.
    dup_allowed: set of key bytes (16 words) that earlier batches of the same context may already have cached twice (legitimate orphans
    of batches with min_count 1, see legit_orphan_keys); this batch's own are added by the checker.

    Ungrouped side: the candidates (`ung_cand`, `counters[4]`) pass the scheme's key check on their way to `ung_idx` in EVERY sorted
    step, Ed25519 included: its launcher classifies into `ung_cand` (ed25519_group_kernels.hip:289) and runs k_ed_keycheck over them
    (:321), which rejects an encoding that does not decompress (`counters[3]`, verdict byte 0).  Only the unsorted Ed25519 split
    (k_ed_group_split) lists its candidates in `ung_idx` without a key check.  The model follows the kernels here, not the older
    description of the Ed25519 step as having no key check in front of the one-lane kernel."""
    bad = _Report()
    n = int(ro["n"])
    scheme = int(ro["scheme"])
    words = key_words(batch, keyloc)
    if words.shape[0] != n:
        bad.add("header.n", f"read-out of {n} tuples for a batch of {words.shape[0]}")
        return bad
    idx = np.arange(n, dtype=np.int64)
    rep = np.asarray(ro["rep"], dtype=np.int64)
    cnt = np.asarray(ro["cnt"], dtype=np.int64)
    slot_of = np.asarray(ro["slot_of"], dtype=np.int64)
    slots = np.asarray(ro["slots"], dtype=np.int64)
    counters = np.asarray(ro["counters"], dtype=np.int64)
    ht = np.asarray(ro["ht"], dtype=np.int64)
    mask = int(ro["ht_mask"])
    if ht.size != mask + 1 or (mask & (mask + 1)):
        bad.add("header.ht", f"table of {ht.size} entries for mask {mask:#x}")
        return bad
    (kid,) = _rows_as_ids(words)

    # ---- representatives ------------------------------------------------------------------------------------------------------------
    if ((rep < 0) | (rep >= n)).any():
        bad.add("rep.range", _first((rep < 0) | (rep >= n)))
        return bad
    if (kid[rep] != kid).any():
        bad.add("rep.key", "rep[i] holds other key bytes than i: " + _first(kid[rep] != kid))
    if (rep[rep] != rep).any():
        bad.add("rep.idempotent", "rep[rep[i]] != rep[i]: " + _first(rep[rep] != rep))
    is_rep = rep == idx
    # the table
    pos = np.flatnonzero(ht)
    holder = ht[pos] - 1
    in_table = np.zeros(n, dtype=bool)
    window = min(MAX_PROBES, mask + 1)
    home = grouping_hash(words, int(ro["seed"])).astype(np.int64) & mask
    zcum = np.concatenate(([0], np.cumsum(ht == 0)))
    if ((holder < 0) | (holder >= n)).any():
        bad.add("ht.entry", "entry beyond the batch: " + _first((holder < 0) | (holder >= n)))
        return bad
    if np.unique(holder).size != holder.size:
        bad.add("ht.once", "a tuple holds more than one entry")
    in_table[holder] = True
    if (~is_rep[holder]).any():
        bad.add("ht.entry", "entry of a tuple that does not represent itself: " + _first(~is_rep[holder]))
    if np.unique(kid[holder]).size != holder.size:
        bad.add("ht.distinct_keys", "two entries hold the same key bytes")
    dist = (pos - home[holder]) & mask
    if (dist >= window).any():
        bad.add("ht.probe_bound", f"entry {window} or more probes from its home slot: " + _first(dist >= window))
    holes = _zeros_between(zcum, home[holder], pos, mask + 1)
    if (holes != 0).any():
        bad.add("ht.hole", "empty entry between an entry and its home slot: " + _first(holes != 0))
    # orphans: representatives without an entry.  Nobody can have found them, and they gave up only behind a full window of other keys.
    orphan = is_rep & ~in_table
    if (orphan[rep] & ~is_rep).any():
        bad.add("rep.unique", "a tuple points at a representative that has no table entry: " + _first(orphan[rep] & ~is_rep))
    key_has_entry = np.zeros(int(kid.max()) + 1 if n else 0, dtype=bool)
    key_has_entry[kid[holder]] = True
    entry_of_key = np.full(key_has_entry.size, -1, dtype=np.int64)
    entry_of_key[kid[holder]] = holder
    wrong = in_table[rep] & (entry_of_key[kid] != rep) & (kid[rep] == kid)
    if wrong.any():
        bad.add("rep.unique", "two representatives with table entries for one key: " + _first(wrong))
    split = ~orphan & key_has_entry[kid] & (rep != entry_of_key[kid])
    if split.any():
        bad.add("rep.unique", "a tuple does not point at its key's table entry: " + _first(split))
    o = np.flatnonzero(orphan)
    if o.size:
        if window > mask:                            # a table smaller than the probe bound: the window is the whole table
            empty_in_window = np.full(o.size, int(zcum[mask + 1]))
        else:
            empty_in_window = _zeros_between(zcum, home[o], (home[o] + window) & mask, mask + 1)
        same_key_in_window = key_has_entry[kid[o]]       # an entry sits within the window of its key's home slot (ht.probe_bound)
        illegit = (empty_in_window != 0) | same_key_in_window
        if illegit.any():
            bad.add("orphan.window", "a tuple represents itself although its probe window had room or held its key: " + _first_of(o, illegit))

    # ---- counts ---------------------------------------------------------------------------------------------------------------------
    sampled = group_sampled(idx, int(ro["sample_mask"]))
    want_cnt = np.bincount(rep[sampled], minlength=n)
    if (want_cnt != cnt).any():
        bad.add("cnt.exact", "cnt differs from the number of sampled tuples of the representative: " + _first(want_cnt != cnt) +
                f" (got {int(cnt[np.flatnonzero(want_cnt != cnt)[0]])}, want {int(want_cnt[np.flatnonzero(want_cnt != cnt)[0]])})")

    # ---- groups ---------------------------------------------------------------------------------------------------------------------
    kc_on = bool(ro["kc_enabled"])
    kc_cap = int(ro["kc_cap"])
    w16 = _key16(words)
    before_keys = np.zeros((0, 16), dtype=np.uint32)
    before_count = 0
    if cache_before is not None:
        before_count = min(int(cache_before["count"][0]), kc_cap)
        before_keys = np.asarray(cache_before["keys"], dtype=np.uint32).reshape(-1, 16)[:before_count]
    after_count_raw = int(ro["cache_count"][0])
    after_count = min(after_count_raw, kc_cap)
    after_keys = np.asarray(ro["cache_keys"], dtype=np.uint32).reshape(-1, 16)[:after_count]
    tid, bid, aid = _rows_as_ids(w16, before_keys, after_keys)
    cached_before = np.isin(tid, bid) if kc_on else np.zeros(n, dtype=bool)
    eligible = is_rep & ((want_cnt >= int(ro["min_samples"])) | cached_before)
    max_groups = int(ro["max_groups"])
    if counters[0] != int(eligible.sum()):
        bad.add("groups.counter", f"counters[0] = {int(counters[0])}, eligible representatives = {int(eligible.sum())}")
    groups = min(int(counters[0]), max_groups)
    group_rep = np.asarray(ro["group_rep"], dtype=np.int64)[:groups]
    if group_rep.size != groups:
        bad.add("groups.readout", f"{group_rep.size} entries of group_rep for {groups} groups")
        return bad
    has_slot = slot_of != NONE
    if ((group_rep < 0) | (group_rep >= n)).any() or np.unique(group_rep).size != groups:
        bad.add("groups.bijection", "group_rep holds a tuple twice or one beyond the batch")
    else:
        if (slot_of[group_rep] != np.arange(groups)).any():
            bad.add("groups.bijection", "slot_of[group_rep[k]] != k: " + _first(slot_of[group_rep] != np.arange(groups)))
        if int(has_slot.sum()) != groups:
            bad.add("groups.slot_of_none", f"{int(has_slot.sum())} tuples hold a slot, {groups} groups")
        if (~eligible[group_rep]).any():
            k = int(np.flatnonzero(~eligible[group_rep])[0])
            bad.add("groups.eligible", f"group {k} belongs to tuple {int(group_rep[k])}, which is no representative at or above the threshold "
                    f"(count {int(want_cnt[group_rep[k]])}, min_samples {int(ro['min_samples'])})")
    if (has_slot & ~eligible).any():
        bad.add("groups.eligible", "slot_of set for a tuple that is not eligible: " + _first(has_slot & ~eligible))
    if (slots != slot_of[rep]).any():
        bad.add("slots.match", "slots[i] != slot_of[rep[i]]: " + _first(slots != slot_of[rep]))

    # ---- ungrouped side -------------------------------------------------------------------------------------------------------------
    acc = np.asarray(ro["acc"], dtype=np.int64)
    sorted_step = bool(ro["sorted"])
    cand = np.flatnonzero(slots == NONE)
    checks_keys = sorted_step or scheme != SCHEME_ED25519        # the unsorted Ed25519 split lists its candidates without a key check
    if sorted_step:
        got = np.asarray(ro["ung_cand"], dtype=np.int64)[:int(counters[4])]
        if counters[4] != cand.size or not np.array_equal(np.sort(got), cand):
            bad.add("ung.cand", f"ung_cand[:counters[4] = {int(counters[4])}] is no permutation of the {cand.size} tuples without a group")
    if checks_keys:
        stride, off, nw = keyloc
        raw = np.frombuffer(bytes(batch), dtype=np.uint8) if not isinstance(batch, np.ndarray) else batch.reshape(-1)
        verdict = {}
        ok = np.zeros(cand.size, dtype=bool)
        for j, i in enumerate(cand):
            k = int(kid[i])
            if k not in verdict:
                verdict[k] = key_ok(scheme, raw[i * stride + off:i * stride + off + 4 * nw].tobytes())
            ok[j] = verdict[k]
    else:
        ok = np.ones(cand.size, dtype=bool)
    got = np.asarray(ro["ung_idx"], dtype=np.int64)[:int(counters[2])]
    if counters[2] != int(ok.sum()) or not np.array_equal(np.sort(got), cand[ok]):
        extra = np.setdiff1d(got, cand[ok])
        bad.add("ung.idx", f"ung_idx[:counters[2] = {int(counters[2])}] is no permutation of the {int(ok.sum())} candidates with a good key" +
                (f" (tuple {int(extra[0])} does not belong there)" if extra.size else ""))
    if counters[3] != int((~ok).sum()):
        bad.add("ung.rejected", f"counters[3] = {int(counters[3])}, candidates with a bad key = {int((~ok).sum())}")
    if (acc[cand[~ok]] != 0).any():
        bad.add("ung.rejected", "verdict byte of a tuple rejected for its key is not 0: " + _first_of(cand[~ok], acc[cand[~ok]] != 0))

    # ---- grouped side ---------------------------------------------------------------------------------------------------------------
    grouped = np.flatnonzero(slots != NONE)
    if (slots[grouped] >= groups).any():
        bad.add("slots.range", "a tuple holds a group number beyond the batch's groups")
        return bad
    total = int(counters[1])
    grp_idx = np.asarray(ro["grp_idx"], dtype=np.int64)[:total]
    if sorted_step:
        gcount = np.asarray(ro["gcount"], dtype=np.int64)[:groups]
        gcursor = np.asarray(ro["gcursor"], dtype=np.int64)[:groups]
        grp_of = np.asarray(ro["grp_of"], dtype=np.int64)[:total]
        want_gcount = np.bincount(slots[grouped], minlength=groups)[:groups] if groups else np.zeros(0, dtype=np.int64)
        if (gcount != want_gcount).any():
            k = int(np.flatnonzero(gcount != want_gcount)[0])
            bad.add("sort.gcount", f"gcount[{k}] = {int(gcount[k])}, tuples with slots == {k}: {int(want_gcount[k])}")
        if total != int(gcount.sum()):
            bad.add("sort.total", f"counters[1] = {total}, sum of gcount = {int(gcount.sum())}")
        if grp_idx.size != total or grp_of.size != total:
            bad.add("sort.readout", "lists shorter than counters[1]")
            return bad
        if total != grouped.size or not np.array_equal(np.sort(grp_idx), grouped):
            missing, extra = np.setdiff1d(grouped, grp_idx), np.setdiff1d(grp_idx, grouped)
            twice = total - np.unique(grp_idx).size
            bad.add("sort.perm", f"grp_idx[:{total}] is no permutation of the {grouped.size} grouped tuples ({missing.size} missing, {extra.size} foreign, "
                    f"{twice} listed again)")
        inb = (grp_idx >= 0) & (grp_idx < n)
        if (~inb).any() or (grp_of[inb] != slots[grp_idx[inb]]).any():
            bad.add("sort.grp_of", "grp_of[L] != slots[grp_idx[L]]: " + _first(~inb | (grp_of != slots[np.clip(grp_idx, 0, max(n - 1, 0))])))
        # runs: the positions of a group are contiguous, and the runs follow the order of group_sort_group_at
        if total:
            change = np.flatnonzero(np.diff(grp_of) != 0) + 1
            run_groups = grp_of[np.concatenate(([0], change))]
            if np.unique(run_groups).size != run_groups.size:
                bad.add("sort.runs", "the positions of a group are not one contiguous run")
            else:
                order = sort_order(groups)
                rank = np.full(groups + 1, -1, dtype=np.int64)
                rank[order] = np.arange(order.size)
                rg = np.clip(run_groups, 0, groups)
                if (run_groups >= groups).any() or (np.diff(rank[rg]) <= 0).any():
                    bad.add("sort.order", "the runs do not follow each other in the order 0, 8, 16, ..., 1, 9, ...")
        order = sort_order(groups)
        ends = np.zeros(groups, dtype=np.int64)
        if groups:
            ends[order] = np.cumsum(want_gcount[order])
        if (gcursor != ends).any():
            k = int(np.flatnonzero(gcursor != ends)[0])
            bad.add("sort.gcursor", f"gcursor[{k}] = {int(gcursor[k])}, end of run {k} = {int(ends[k])}")
    else:
        if total != grouped.size or grp_idx.size != total or not np.array_equal(np.sort(grp_idx), grouped):
            bad.add("list.perm", f"grp_idx[:counters[1] = {total}] is no permutation of the {grouped.size} grouped tuples")

    # ---- table slots and the key-table cache ----------------------------------------------------------------------------------------
    tslot = np.asarray(ro["tslot"], dtype=np.int64)[:groups]
    cold = np.asarray(ro["cold"], dtype=np.int64)[:groups]
    ccount = np.asarray(ro["cache_count"], dtype=np.int64)
    if groups and np.unique(group_rep).size == groups and not ((group_rep < 0) | (group_rep >= n)).any():
        if np.unique(tslot).size != groups:
            bad.add("cache.tslot_unique", "two groups share a table slot")
        if not kc_on:
            if (tslot != kc_cap + np.arange(groups)).any() or (cold != 1).any():
                bad.add("cache.off", "cache off: tslot[k] != kc.cap + k or cold[k] != 1: " + _first((tslot != kc_cap + np.arange(groups)) | (cold != 1)))
        else:
            gk = tid[group_rep]
            was_cached = cached_before[group_rep]
            if ((cold == 0) != was_cached).any():
                bad.add("cache.cold", "cold[k] == 0 for a key that was not cached before the batch, or 1 for one that was: " + _first((cold == 0) != was_cached))
            inside = tslot < kc_cap
            over = inside & (tslot >= after_count)
            if over.any():
                bad.add("cache.key", "table slot beyond the cache's slots handed out: " + _first(over))
            chk = np.flatnonzero(inside & ~over)
            if chk.size and (aid[tslot[chk]] != gk[chk]).any():
                k = int(chk[np.flatnonzero(aid[tslot[chk]] != gk[chk])[0]])
                bad.add("cache.key", f"group {k} (tuple {int(group_rep[k])}) has table slot {int(tslot[k])}, which holds another key")
            outside = ~inside
            if (tslot[outside] != kc_cap + np.flatnonzero(outside)).any() or (cold[outside] != 1).any():
                bad.add("cache.key", "a slot outside the cache is not the group's per-batch slot kc.cap + k, or not cold")
            if outside.any() and after_count_raw < kc_cap:
                bad.add("cache.key", "a group took a per-batch slot although the cache had room")
            if min(before_count + int((~was_cached).sum()), kc_cap) != after_count:
                bad.add("cache.counts", f"cached keys: {before_count} before + {int((~was_cached).sum())} misses, {after_count} after (capacity {kc_cap})")
    ok_reps = groups == 0 or (np.unique(group_rep).size == groups and not ((group_rep < 0) | (group_rep >= n)).any())
    if ok_reps:
        want_hits = int(cached_before[group_rep].sum()) if kc_on and groups else 0
        want_miss = groups - want_hits if kc_on else 0
        if ccount[1] != want_hits or ccount[2] != want_miss:
            bad.add("cache.counts", f"hits / misses = {int(ccount[1])} / {int(ccount[2])}, model {want_hits} / {want_miss}")
    if kc_on and before_count and not np.array_equal(after_keys[:before_count], before_keys):
        bad.add("cache.key", "a key cached before the batch was rewritten")
    # duplicates among the cached keys: only keys that had a legitimate orphan in a batch with min_count == 1
    allowed = set(dup_allowed or ())
    if int(ro["min_count"]) == 1:
        allowed |= legit_orphan_keys(batch, keyloc, ro)
    if after_keys.shape[0]:
        uniq, first, counts = np.unique(aid, return_index=True, return_counts=True)
        for j in np.flatnonzero(counts > 1):
            if after_keys[first[j]].tobytes() not in allowed:
                bad.add("cache.dup", f"key of cache slot {int(first[j])} is cached {int(counts[j])} times")

    # ---- verdict bytes --------------------------------------------------------------------------------------------------------------
    if ((acc != 0) & (acc != 1)).any():
        bad.add("acc.range", "verdict byte that is neither 0 nor 1: " + _first((acc != 0) & (acc != 1)))
    if bitmap is not None:
        bits = np.unpackbits(np.frombuffer(bytes(bitmap), dtype=np.uint8), bitorder="little")[:n]
        if (bits != (acc == 1)).any():
            bad.add("acc.bitmap", "verdict byte differs from the returned bit: " + _first(bits != (acc == 1)))
    return bad


def _first_of(index, mask):
    sel = np.asarray(index)[np.asarray(mask)]
    return f"{sel.size} of them, first at {int(sel[0])}" if sel.size else "none"


def legit_orphan_keys(batch, keyloc, ro):
    """Key bytes (16 cache words) of the tuples that represent themselves without a table entry."""
    words = key_words(batch, keyloc)
    n = words.shape[0]
    rep = np.asarray(ro["rep"], dtype=np.int64)
    ht = np.asarray(ro["ht"], dtype=np.int64)
    in_table = np.zeros(n, dtype=bool)
    h = ht[ht != 0] - 1
    in_table[h[(h >= 0) & (h < n)]] = True
    o = np.flatnonzero((rep == np.arange(n)) & ~in_table)
    w16 = _key16(words[o])
    return {w16[j].tobytes() for j in range(o.size)}


# ---- the sequential reference builder ------------------------------------------------------------------------------------------------
def build_readout(batch, scheme, ht_bits, min_count, max_groups, seed=0, sorted_step=True, shift=None, cache=None, kc_cap=0, acc=None, serial=1):
    """What the lane functions of p256_group.h leave behind when they run one tuple after the other (group_insert_lane,
    group_assign_lane, key_cache_phase_lookup / _insert, group_classify_lane + group_keycheck_lane or group_split_lane, the counting
    sort).  cache: {"keys": [m][16], "count": [4]} updated in place when given (the cache is then ON; its own hash table is modelled as a
    dict: lookups always find what was inserted).  acc: verdict bytes to carry (default: zeros)."""
    keyloc = KEYLOC[scheme]
    words = key_words(batch, keyloc)
    n = words.shape[0]
    mask = (1 << ht_bits) - 1
    sample_mask, min_samples = threshold(min_count, shift)
    home = grouping_hash(words, seed).astype(np.int64) & mask
    keyb = [words[i].tobytes() for i in range(n)]
    ht = np.zeros(mask + 1, dtype=np.uint32)
    rep = np.zeros(n, dtype=np.uint32)
    cnt = np.zeros(n, dtype=np.uint32)
    sampled = group_sampled(np.arange(n), sample_mask)
    for i in range(n):
        slot, mine = int(home[i]), i
        for _ in range(min(MAX_PROBES, mask + 1)):
            v = int(ht[slot])
            if v == 0:
                ht[slot] = i + 1
                break
            if keyb[v - 1] == keyb[i]:
                mine = v - 1
                break
            slot = (slot + 1) & mask
        rep[i] = mine
        if sampled[i]:
            cnt[mine] += 1
    kc_on = cache is not None
    w16 = _key16(words)
    cached = {}
    if kc_on:
        m = min(int(cache["count"][0]), kc_cap)
        for s in range(m):
            cached.setdefault(np.asarray(cache["keys"], dtype=np.uint32).reshape(-1, 16)[s].tobytes(), s)
    counters = np.zeros(12, dtype=np.uint32)
    slot_of = np.full(n, NONE, dtype=np.uint32)
    group_rep = []
    for i in range(n):
        if rep[i] == i and (cnt[i] >= min_samples or (kc_on and w16[i].tobytes() in cached)):
            got = int(counters[0])
            counters[0] += 1
            if got < max_groups:
                slot_of[i] = got
                group_rep.append(i)
    groups = len(group_rep)
    tslot = np.zeros(groups, dtype=np.uint32)
    cold = np.ones(groups, dtype=np.uint8)
    ccount = np.zeros(4, dtype=np.uint32)
    keys_out = np.zeros((max(kc_cap, 1), 16), dtype=np.uint32)
    if kc_on:
        ccount[0] = cache["count"][0]
        have = np.asarray(cache["keys"], dtype=np.uint32).reshape(-1, 16)
        keys_out[:have.shape[0]] = have[:keys_out.shape[0]]
        for k, r in enumerate(group_rep):
            s = cached.get(w16[r].tobytes())
            if s is not None:
                tslot[k], cold[k] = s, 0
                ccount[1] += 1
        for k, r in enumerate(group_rep):
            if cold[k]:
                ccount[2] += 1
                if ccount[0] < kc_cap:
                    tslot[k] = ccount[0]
                    keys_out[int(ccount[0])] = w16[r]
                    ccount[0] += 1
                else:
                    tslot[k] = kc_cap + k
        cache["keys"], cache["count"] = keys_out.copy(), ccount.copy()
    else:
        tslot[:] = kc_cap + np.arange(groups)
    slots = slot_of[rep]
    acc = np.zeros(n, dtype=np.uint8) if acc is None else np.array(acc, dtype=np.uint8)
    raw = np.frombuffer(bytes(batch), dtype=np.uint8)
    stride, off, nw = keyloc
    cand = [i for i in range(n) if slots[i] == NONE]
    checks_keys = sorted_step or scheme != SCHEME_ED25519
    ung_idx = []
    for i in reversed(cand):                     # any order is legal: not the tuple order
        if not checks_keys or key_ok(scheme, raw[i * stride + off:i * stride + off + 4 * nw].tobytes()):
            ung_idx.append(i)
        else:
            acc[i] = 0
            counters[3] += 1
    counters[2] = len(ung_idx)
    counters[4] = len(cand) if sorted_step else 0
    grouped = [i for i in range(n) if slots[i] != NONE]
    gcount = np.bincount(slots[grouped].astype(np.int64), minlength=groups)[:groups].astype(np.uint32) if groups else np.zeros(0, dtype=np.uint32)
    gcursor = np.zeros(groups, dtype=np.uint32)
    counters[1] = len(grouped)
    if sorted_step:
        order = sort_order(groups)
        start = np.zeros(groups, dtype=np.int64)
        if groups:
            start[order] = np.concatenate(([0], np.cumsum(gcount[order].astype(np.int64))[:-1]))
        cur = start.copy()
        grp_idx = np.zeros(len(grouped), dtype=np.uint32)
        grp_of = np.zeros(len(grouped), dtype=np.uint32)
        for i in reversed(grouped):
            k = int(slots[i])
            grp_idx[cur[k]], grp_of[cur[k]] = i, k
            cur[k] += 1
        gcursor = cur.astype(np.uint32)
    else:
        grp_idx = np.array(list(reversed(grouped)), dtype=np.uint32)
        grp_of = np.zeros(0, dtype=np.uint32)
        gcount = np.zeros(groups, dtype=np.uint32)
    return {"scheme": scheme, "n": n, "ht_mask": mask, "max_groups": max_groups, "min_count": min_count, "sample_mask": sample_mask,
            "min_samples": min_samples, "seed": seed, "sorted": 1 if sorted_step else 0, "kc_cap": kc_cap, "kc_enabled": 1 if kc_on else 0,
            "serial": serial, "groups": groups, "ht": ht, "rep": rep, "cnt": cnt, "slot_of": slot_of, "group_rep": np.array(group_rep, dtype=np.uint32),
            "counters": counters, "slots": slots.astype(np.uint32), "grp_idx": grp_idx, "grp_of": grp_of, "ung_idx": np.array(ung_idx, dtype=np.uint32),
            "ung_cand": np.array(cand if sorted_step else [], dtype=np.uint32), "gcount": gcount, "gcursor": gcursor, "tslot": tslot, "cold": cold,
            "acc": acc, "cache_keys": keys_out[:min(int(ccount[0]), kc_cap)].copy(), "cache_count": ccount}
