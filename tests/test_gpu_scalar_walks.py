"""GPU tier: every scalar-multiplication path walked with the chosen scalars of tests/scalar_cases.py.

The reference is the agreed list of tests/test_scalar_cases_cpu.py (Python twin == C oracle == OpenSSL == the verdict by
construction); here the C oracle judges the same tuples once more on this machine, and every bitmap of the device is compared with
that list bit for bit, naming family and case on a mismatch.  Every case set goes through every path that can serve it:

  P-256      generic entry: one-lane kernel (grouping off), the grouped step's one-launch form, its ungrouped list, its phased form with
             full tables and rows-only keys mixed, hot keys; registered keys: one-launch (<= 32), 8-lane (<= 32768), one-lane (> 32768) with 8-bit
             combs, widened to 16 and to 18 bits; host and _dev entries
  secp256k1  generic one-lane, grouped, the grouped step's ungrouped list, key-table cache cold and warm; registered narrow and widened in the three
             k256_keyed_prep_T regimes (< 2^14, < 2^17, >= 2^17)
  Ed25519    one-lane, grouped, the grouped step's ungrouped list (k_ed_generic_list; k_ed_generic_quad in the child that sets
             SBV_ED_UNGROUPED_QUAD=1), hot-key pool; registered narrow and widened.  Through tuples only: the message entries compute
             k = SHA-512(R | A | M) themselves, so a chosen k cannot reach them.

A size regime is reached by padding the case list with seeded valid tuples of the oracle's generators up to the smallest size that
selects the form.  What no emulator can do is the wavefront: the registered-key batches start with wavefronts in which all 64 lanes
carry, exactly one does (lane 0, 31, 63), none does, one dead lane (slot out of range, invalid slot, r = 0 / S = L) or one narrow slot
sits among 63 wide ones, and they end in a partly filled wavefront (1, 63, 65 records).  Which walk such a wavefront then takes is
the kernel's business and differs: the secp256k1 and Ed25519 kernels leave dead lanes out of the wide / narrow ballot, so theirs stay
wide; the P-256 kernels ask wave_all(slot is wide) of every lane, so a lane whose slot is out of range (clamped to slot 0: wide) or
whose scalar is dead keeps the wavefront wide, while the invalid slot — a key that is no point is never widened — sends it back to
the 8-bit combs, like the narrow slot.  The verdicts must be right either way.

The composition is what the device sees where record i sits in lane i % 64: the one-lane registered forms (P-256 above 32768
records, Ed25519 at every size) and the secp256k1 kernel, whose stage B takes one record per lane at every size (k256_keyed_prep_T
changes how many records a lane of STAGE A inverts together, not the layout of the verify kernel).  In the P-256 8-lane form a
wavefront holds 8 records and in the one-launch form 4, so there the same records are a plain case list, not a composition.

What shows that a path ran: the grouped step's counters (groups, grouped, ungrouped tuples, table classes), the key-table-cache and
hot-key statistics and the wide-key statistics, asserted below.  The registered-key size regimes and the one-lane generic kernels
have no counter in the library: there the batch size, checked against the thresholds the code defines, and the unchanged cache
statistics are what the tests hold on to.  Settings read at start-up run in a fresh child process each, one at a time; the library
does not report them back, so the test checks that each name is one the library's sources read."""
import ctypes
import os
import subprocess
import sys
import time

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import consensus_amd as sbv  # noqa: E402
import scalar_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)
WIDTH = {"p256": 160, "k256": 160, "ed25519": 128}
OOB, INVALID = "slot out of range", "invalid slot"


# ---- the reference, once per process ---------------------------------------------------------------------------------------------
_ORACLE = None


def oracle_lib():
    global _ORACLE
    if _ORACLE is None:
        lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "libsbv_oracle.so"))
        for name in ("sbvo_gen_batch", "sbvo_k256_gen_batch", "sbvo_ed25519_gen_batch"):
            getattr(lib, name).argtypes = [ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        for name in ("sbvo_p256_verify_batch", "sbvo_k256_verify_batch", "sbvo_ed25519_verify_batch"):
            getattr(lib, name).argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
        _ORACLE = lib
    return _ORACLE


def oracle_verdicts(scheme, tuples):
    n = len(tuples) // WIDTH[scheme]
    bm = ctypes.create_string_buffer((n + 7) // 8 or 1)
    getattr(oracle_lib(), {"p256": "sbvo_p256_verify_batch", "k256": "sbvo_k256_verify_batch", "ed25519": "sbvo_ed25519_verify_batch"}[scheme])(tuples, n, bm, THREADS)
    return sbv.bitmap_to_list(bm.raw, n)


class Lane:
    """one record of a batch: the tuple, how its slot is named in the registered-key form, the agreed verdict and a label"""
    __slots__ = ("tuple", "slot", "expect", "label")

    def __init__(self, t, expect, label, slot="own"):
        self.tuple, self.slot, self.expect, self.label = t, slot, expect, label


_REF = {}
PAD_BASE = 4096


def reference(scheme):
    """(cases, cases as lanes, padding): the agreed verdicts, checked against the C oracle here once more; the padding is 4096 seeded
    tuples over 4 keys, every 9th corrupted, with the generator's verdicts — repeated as often as a size regime needs"""
    if scheme not in _REF:
        cs = sc.cases(scheme)
        assert oracle_verdicts(scheme, sc.blob(cs)) == [c.expect for c in cs]
        lanes = [Lane(c.tuple, c.expect, "%s/%s/%s" % (c.walker, c.family, c.name)) for c in cs]
        n = PAD_BASE
        tup, exp = ctypes.create_string_buffer(WIDTH[scheme] * n), ctypes.create_string_buffer((n + 7) // 8)
        getattr(oracle_lib(), {"p256": "sbvo_gen_batch", "k256": "sbvo_k256_gen_batch", "ed25519": "sbvo_ed25519_gen_batch"}[scheme])(0x5CA1A0, n, 4, 9, tup, exp, THREADS)
        _REF[scheme] = (cs, lanes, (scheme, tup.raw, sbv.bitmap_to_list(exp.raw, n)))
    return _REF[scheme]


class Batch:
    """`lanes` of one scheme, followed by the scheme's padding tuples up to n records in all"""

    def __init__(self, scheme, lanes, n=None):
        n = len(lanes) if n is None else n
        self.scheme, self.lanes, self.extra, self.n = scheme, lanes, n - len(lanes), n
        assert self.extra >= 0, (len(lanes), n)
        self.tuples = b"".join(l.tuple for l in lanes)
        self.expect = [l.expect for l in lanes]
        if self.extra:
            _, base, bits = reference(scheme)[2]
            reps = -(-self.extra // PAD_BASE)
            self.tuples += (base * reps)[:self.extra * WIDTH[scheme]]
            self.expect += (bits * reps)[:self.extra]

    def label(self, i):
        return self.lanes[i].label if i < len(self.lanes) else "padding %d" % ((i - len(self.lanes)) % PAD_BASE)


def compare(tag, batch, bitmap):
    got = sbv.bitmap_to_list(bitmap, batch.n)
    bad = [(i, batch.label(i), g) for i, (e, g) in enumerate(zip(batch.expect, got)) if g != e]
    assert not bad, (tag, len(bad), bad[:8])


# ---- wavefront composition for the registered-key forms ----------------------------------------------------------------------------
def wavefronts(scheme, walker):
    """Wavefronts of 64 lanes for a batch whose first key is walked by `walker` (key8, or the wide comb it was widened to) and whose
    second key keeps its 8-bit comb: all carry, one carries at lane 0 / 31 / 63, none carries, one dead lane of each kind among 63 live
    ones, one narrow slot among 63 wide ones (on P-256 the invalid slot, too, makes its wavefront narrow: see the module's text).  Carrying = the model's top digit of the scalar is not zero, for `walker` when its top
    window is the recoding's carry, else for the 8-bit comb (the 18-bit comb's 15th window holds real digits: it is always walked)."""
    cs, lanes, _ = reference(scheme)
    ws = sc.walkers(scheme)
    d, d2 = sc.private_keys(scheme)
    w = ws[walker] if scheme != "ed25519" and ws[walker].bits * (ws[walker].windows - 1) == 256 else ws["key8"]
    pick = [(c, l) for c, l in zip(cs, lanes) if c.d == d and c.walker in (walker, w.name)]
    if scheme == "ed25519":                                          # no carry window: the wavefronts differ in their slots only
        carriers, quiet = [], [l for c, l in pick]
    else:
        def carries(c):
            return w.digits(c.b)[w.windows - 1] != 0
        carriers = [l for c, l in pick if c.family == "carry" and c.walker == w.name and carries(c)]
        quiet = [l for c, l in pick if not carries(c)]
        assert len(carriers) >= 4 and len(quiet) >= 64
    out = []

    def wave(special, where):
        lanes64 = [quiet[(7 * len(out) + i) % len(quiet)] for i in range(64)]
        for k, s in zip(where, special):
            lanes64[k] = s
        out.extend(lanes64)

    if carriers:
        wave([carriers[i % len(carriers)] for i in range(64)], range(64))
        for at in (0, 31, 63):
            wave([carriers[at % len(carriers)]], [at])
    wave([], [])
    live = quiet[5]
    dead_scalar = bytearray(live.tuple)
    if scheme == "ed25519":
        dead_scalar[32:64] = sc.ed.L.to_bytes(32, "little")          # S = L: not canonical
    else:
        dead_scalar[0:32] = bytes(32)                                # r = 0
    for at, lane in ((17, Lane(live.tuple, False, OOB, slot=OOB)), (40, Lane(live.tuple, False, INVALID, slot=INVALID)),
                     (63, Lane(bytes(dead_scalar), False, "r = 0 / S = L"))):
        wave([lane], [at])
    rng_scalars = [(0x1234567 + 977 * i, 0x7654321 + 1013 * i) for i in range(2)]
    other = []
    for a, b in rng_scalars:                                         # the second key's lanes: forged here, judged by the oracle below
        t = sc.forge_ed25519(d2, a, b) if scheme == "ed25519" else sc.forge_ecdsa(scheme, d2, a, b)[0]
        other += [Lane(t, True, "second key"), Lane(sc.twin(scheme, t), False, "second key/twin")]
    assert oracle_verdicts(scheme, Batch(scheme, other).tuples) == [l.expect for l in other]
    wave([other[0]], [9])
    wave([other[1]], [0])
    return out


def invalid_key(scheme):
    if scheme != "ed25519":
        return bytes(64)                                             # (0, 0) is on neither curve
    for y in range(2, 100):
        enc = y.to_bytes(32, "little")
        if sc.ed.decompress(enc) is None:
            return enc
    raise AssertionError("no invalid encoding found")


def keyed_form(batch, slot_of, bad_slot):
    """records and slots of the registered-key form; a lane named OOB gets a slot beyond the registry, INVALID the slot of a key that
    is no point"""
    scheme = batch.scheme
    w = WIDTH[scheme]
    lo, hi = (64, 96) if scheme == "ed25519" else (96, 160)
    recs = b"".join(l.tuple[:lo] + l.tuple[hi:] for l in batch.lanes)
    slots = [0xFFFFFFF0 if l.slot == OOB else bad_slot if l.slot == INVALID else slot_of[l.tuple[lo:hi]] for l in batch.lanes]
    if batch.extra:
        base = reference(scheme)[2][1]
        reps = -(-batch.extra // PAD_BASE)
        recs += (b"".join(base[w * i:w * i + lo] + base[w * i + hi:w * (i + 1)] for i in range(PAD_BASE)) * reps)[:batch.extra * (w - (hi - lo))]
        slots += ([slot_of[base[w * i + lo:w * i + hi]] for i in range(PAD_BASE)] * reps)[:batch.extra]
    assert len(recs) == (w - (hi - lo)) * batch.n and len(slots) == batch.n
    return recs, slots


API = {
    "p256": dict(register=sbv.register_keys, clear=sbv.clear_keys, keyed=sbv.verify_batch_keyed, keyed_dev=sbv.verify_batch_keyed_dev, widen=sbv.widen_keys,
                 wide_stats=sbv.wide_key_stats, selfcheck=sbv.wide_selfcheck, generic=sbv.verify_batch, generic_dev=sbv.verify_batch_dev, cache=sbv.SCHEME_P256),
    "k256": dict(register=sbv.secp256k1_register_keys, clear=sbv.secp256k1_clear_keys, keyed=sbv.secp256k1_verify_batch_keyed,
                 keyed_dev=sbv.secp256k1_verify_batch_keyed_dev, widen=sbv.secp256k1_widen_keys, wide_stats=sbv.secp256k1_wide_key_stats,
                 selfcheck=sbv.secp256k1_wide_selfcheck, generic=sbv.secp256k1_verify_batch, generic_dev=sbv.secp256k1_verify_batch_dev, cache=sbv.SCHEME_SECP256K1),
    "ed25519": dict(register=sbv.ed25519_register_keys, clear=sbv.ed25519_clear_keys, keyed=sbv.ed25519_verify_batch_keyed,
                    keyed_dev=sbv.ed25519_verify_batch_keyed_dev, widen=sbv.ed25519_widen_keys, wide_stats=sbv.ed25519_wide_key_stats,
                    selfcheck=sbv.ed25519_wide_selfcheck, generic=sbv.ed25519_verify_batch, generic_dev=sbv.ed25519_verify_batch_dev, cache=sbv.SCHEME_ED25519),
}


def dev_call(fn, n, *host_buffers):
    """a _dev entry on device copies of the buffers, on a stream of the caller's; returns the bitmap"""
    import numpy as np
    import torch
    d = [torch.from_numpy(np.frombuffer(bytearray(b), dtype=np.uint8).copy()).cuda() for b in host_buffers]
    out = torch.zeros((n + 7) // 8, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fn(*[x.data_ptr() for x in d], n, out.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    return bytes(out.cpu().numpy().tobytes())


def run_registered(scheme, sizes, widths, small_forms=False):
    """The case list behind the composed wavefronts through the registered-key entries at every size of `sizes` (padded; the sizes end
    in a partly filled wavefront), with 8-bit combs (width 0) and with the first key widened (16 / 18).  Returns what ran."""
    import numpy as np
    api = API[scheme]
    cs, lanes, pad = reference(scheme)
    d, d2 = sc.private_keys(scheme)
    lo, hi = (64, 96) if scheme == "ed25519" else (96, 160)
    ran = []
    api["clear"]()
    try:
        main, second = sc.pubkey(scheme, d), sc.pubkey(scheme, d2)
        w = WIDTH[scheme]
        pad_keys = list(dict.fromkeys(pad[1][w * i + lo:w * i + hi] for i in range(PAD_BASE)))
        keys = [main, second, invalid_key(scheme)] + pad_keys
        reg = api["register"](keys)
        slot_of = dict(zip(keys, reg))
        assert reg[:3] == [0, 1, 2]
        for bits in widths:
            if scheme == "p256":
                sbv.wide_keys(bits or 16, 64)
            if bits:
                api["widen"]([reg[0]])
                st = api["wide_stats"]()
                assert st[0] == 1 and st[1] == bits, st
                assert api["selfcheck"](reg[0])                      # the comb built on the device == the host builder's, byte for byte
            else:
                assert api["wide_stats"]()[0] == 0
            front = wavefronts(scheme, "wide%d" % bits if bits else "key8")
            for n in sizes:
                batch = Batch(scheme, front + lanes, n)
                recs, slots = keyed_form(batch, slot_of, reg[2])
                compare((scheme, "keyed", bits, n), batch, api["keyed"](recs, slots, n))
                ran.append((bits, n))
            n = sizes[0]
            batch = Batch(scheme, front + lanes, n)
            recs, slots = keyed_form(batch, slot_of, reg[2])
            compare((scheme, "keyed_dev", bits, n), batch, dev_call(api["keyed_dev"], n, recs, np.array(slots, dtype=np.uint32).tobytes()))
            if small_forms:                                           # the one-launch form: 32 records a call, the ragged end included
                for a in range(0, len(front + lanes), 32):
                    part = Batch(scheme, (front + lanes)[a:a + 32])
                    recs, slots = keyed_form(part, slot_of, reg[2])
                    compare((scheme, "one-launch", bits, a), part, api["keyed"](recs, slots, part.n))
                ran.append((bits, 32))
    finally:
        if scheme == "p256":
            sbv.wide_keys()
        api["clear"]()
    return ran


@pytest.fixture(scope="module")
def gpu():
    sbv.init(0)
    t0 = time.perf_counter()
    yield sbv
    for s in sc.SCHEMES:
        API[s]["clear"]()
    print(f"\ntest_gpu_scalar_walks: {time.perf_counter() - t0:.0f} s of wall time")


_REKEYED = {}


def rekeyed(scheme):
    """The scalars of every case whose design does not depend on the private key (all but the mid-walk families), each forged again
    under a key of its own: a batch in which no key signs more than a tuple and its twin.  Verdicts by construction, and the C
    oracle's here.  Nothing is lost with the mid-walk families: the list kernels walk 4-bit digits from the top with doublings
    between them, a walk for which no collision can be aimed (scalar_cases.Comb.sequential)."""
    if scheme not in _REKEYED:
        d = sc.private_keys(scheme)[0]
        lanes = []
        for i, c in enumerate(x for x in sc.cases(scheme) if x.family not in ("collision", "doubling") and not x.name.endswith("/twin")):
            di = (d + 1 + i) % sc.ORDER[scheme] or 1
            t = sc.forge_ed25519(di, c.a, c.b) if scheme == "ed25519" else sc.forge_ecdsa(scheme, di, c.a, c.b)[0]
            label = "own key/%s/%s/%s" % (c.walker, c.family, c.name)
            lanes += [Lane(t, True, label), Lane(sc.twin(scheme, t), False, label + "/twin")]
        batch = Batch(scheme, lanes)
        assert oracle_verdicts(scheme, batch.tuples) == batch.expect
        _REKEYED[scheme] = batch
    return _REKEYED[scheme]


def ungrouped_list(scheme):
    """The grouped step's ungrouped list has kernels of its own (verify29_lane_generic_rec; the secp256k1 list; k_ed_generic_list, or
    k_ed_generic_quad under SBV_ED_UNGROUPED_QUAD=1: four lanes per tuple).  A key stays on it only while it signs fewer tuples of the
    batch than the threshold, and the library caps an explicit threshold at 32 below 2^18 tuples — so the chosen scalars reach it under
    keys of their own (rekeyed), two uses each against a threshold of 8.  The step's counters say that nothing was grouped."""
    batch = rekeyed(scheme)
    sbv.set_grouping(True, 1, 8, 64)
    compare((scheme, "grouped step, every key below the threshold"), batch, API[scheme]["generic"](batch.tuples, batch.n))
    groups, grouped, ungrouped, rejected = sbv.last_group_stats()
    assert grouped == 0 and ungrouped >= batch.n, (scheme, groups, grouped, ungrouped, rejected, batch.n)


# ---- P-256 -------------------------------------------------------------------------------------------------------------------------
def run_p256_generic():
    """the generic entry: one-lane kernel, the grouped step's one-launch form, the phased form (full tables and rows-only keys in one
    batch), host and _dev entries; returns (group stats, table classes) of the phased batch"""
    cs, lanes, pad = reference("p256")
    total = len(lanes)
    alone = Batch("p256", lanes)
    try:
        sbv.set_grouping(False)
        sbv.key_cache(False)
        before = sbv.key_cache_stats()
        compare("one-lane", alone, sbv.verify_batch(alone.tuples, total))
        assert sbv.last_timing().n == total
        compare("one-lane _dev", alone, dev_call(sbv.verify_batch_dev, total, alone.tuples))
        assert sbv.key_cache_stats() == before
        for n in (32769, 32768 + 63):                                 # above 32768 with grouping off: still one lane per tuple
            batch = Batch("p256", lanes, n)
            compare(("one-lane", n), batch, sbv.verify_batch(batch.tuples, n))
        sbv.set_grouping(True, 64, 2, 4096)
        compare("grouped one-launch", alone, sbv.verify_batch(alone.tuples, total))
        st = sbv.last_group_stats()
        assert st[0] == 2 and st[1] == total, st                       # both keys grouped, nothing left to the one-lane kernel
        ungrouped_list("p256")
        sbv.set_grouping(True, 64, 2, 4096)
        n = 32768 + 65
        batch = Batch("p256", lanes, n)
        compare("grouped phased", batch, sbv.verify_batch(batch.tuples, n))
        compare("grouped phased _dev", batch, dev_call(sbv.verify_batch_dev, n, batch.tuples))
        return sbv.last_group_stats(), sbv.last_table_classes()
    finally:
        sbv.key_cache(True)
        sbv.set_grouping(True, sbv.GROUP_MIN_BATCH_DEFAULT, 0, 0)


def test_p256_generic_entry_one_lane_grouped_full_tables_and_rows_only(gpu):
    cs, lanes, pad = reference("p256")
    st, cl = run_p256_generic()
    rows_only = sum(1 for c in cs if c.walker == "narrow")
    # the two keys of the cases and the padding's 4 signers (its corrupted keys come back a few times each and are grouped too); the case
    # key and the signers earn full tables, the second key of the cases (102 uses < 256) is served from its rows alone
    assert st[0] >= 6 and st[1] >= len(lanes), st
    assert cl[0] >= 5 and cl[2] >= rows_only, (cl, rows_only)


def test_p256_hot_keys_take_the_wide_pass(gpu):
    """sbv_p256_hot_keys: the case key is promoted to a 16-bit comb built on the device behind the first batch; the later batches
    walk its tuples through the wide pass (the model `wide16`: every row's first and last entry, every builder boundary)."""
    cs, lanes, pad = reference("p256")
    n = 32768 + 1
    batch = Batch("p256", lanes, n)
    blob = batch.tuples
    try:
        sbv.set_grouping(True, 64, 2, 4096)
        sbv.key_cache(False)
        sbv.key_cache(True)
        sbv.hot_keys(8, 600)
        for i in range(4):                                            # cold, warm (the hits are counted), promoted behind it, served wide
            compare(("hot keys", i), batch, sbv.verify_batch(blob, n))
        h = sbv.hot_key_stats()
        main = sum(1 for c in cs if c.d == sc.private_keys("p256")[0])
        assert 1 <= h[0] <= 8 and h[2] >= main, (h, main)              # the case key and the padding's signers: their tuples through the wide pass
        assert all(sbv.hot_selfcheck(i) for i in range(h[0]))
    finally:
        sbv.hot_keys(1024, 4096)
        sbv.key_cache(False)
        sbv.key_cache(True)
        sbv.set_grouping(True, sbv.GROUP_MIN_BATCH_DEFAULT, 0, 0)


@pytest.mark.parametrize("bits", [0, 16, 18])
def test_p256_registered_keys_three_forms(gpu, bits):
    """8-lane form (the composed wavefronts + every case, 65 records in the last wavefront), one-lane form (32768 + 1, + 63), the
    one-launch form 32 records at a time; 8-bit combs, widened to 16 and to 18 bits"""
    front = len(wavefronts("p256", "key8")) + len(reference("p256")[1])
    ran = run_registered("p256", [front + (65 - front) % 64, 32768 + 1, 32768 + 63], [bits], small_forms=True)
    assert [r[1] for r in ran] == [front + (65 - front) % 64, 32769, 32831, 32] and ran[0][1] % 64 == 1 and ran[0][1] <= 32768


# ---- secp256k1 ---------------------------------------------------------------------------------------------------------------------
def run_generic(scheme, grouped_sizes):
    """one-lane kernel (grouping off), then the grouped step with the key-table cache off, cold and warm; returns the cache statistics"""
    api = API[scheme]
    cs, lanes, pad = reference(scheme)
    total = len(lanes)
    stats = []
    try:
        sbv.set_grouping(False)
        before = sbv.key_cache_stats(api["cache"])
        alone = Batch(scheme, lanes)
        compare((scheme, "one-lane"), alone, api["generic"](alone.tuples, total))
        compare((scheme, "one-lane _dev"), alone, dev_call(api["generic_dev"], total, alone.tuples))
        assert sbv.key_cache_stats(api["cache"]) == before
        sbv.set_grouping(True, 64, 2, 4096)
        sbv.key_cache(False, 0, api["cache"])
        for n in grouped_sizes:
            batch = Batch(scheme, lanes, n)
            compare((scheme, "grouped, cache off", n), batch, api["generic"](batch.tuples, n))
        ungrouped_list(scheme)
        sbv.set_grouping(True, 64, 2, 4096)
        sbv.key_cache(True, 1024, api["cache"])
        for tag in ("cold", "warm"):
            n = grouped_sizes[-1]
            batch = Batch(scheme, lanes, n)
            compare((scheme, "grouped", tag), batch, api["generic"](batch.tuples, n))
            stats.append(sbv.key_cache_stats(api["cache"]))
        return stats
    finally:
        sbv.key_cache(False, 0, api["cache"])
        sbv.key_cache(True, 1024, api["cache"])
        sbv.set_grouping(True, sbv.GROUP_MIN_BATCH_DEFAULT, 0, 0)


def test_k256_generic_one_lane_grouped_and_the_key_table_cache(gpu):
    total = len(reference("k256")[1])
    cold, warm = run_generic("k256", [total, total + 1000 - (total + 1000) % 64 + 63])
    assert cold[1] == 0 and cold[2] >= 5 and cold[0] == cold[2], cold      # the case key and the padding's four signers: built
    assert warm[2] == 0 and warm[1] == cold[0], (cold, warm)               # ... and found again


@pytest.mark.parametrize("bits", [0, 16])
def test_k256_registered_keys_in_the_three_prep_regimes(gpu, bits):
    """k256_keyed_prep_T: one record per lane below 2^14 records, four below 2^17, eight from there on"""
    front = len(wavefronts("k256", "key8")) + len(reference("k256")[1])
    small = front + (65 - front) % 64
    assert small < 1 << 14
    ran = run_registered("k256", [small, (1 << 14) + 1, (1 << 17) + 63], [bits])
    assert [r[1] for r in ran] == [small, 16385, 131135]


# ---- Ed25519 -----------------------------------------------------------------------------------------------------------------------
def test_ed25519_generic_one_lane_grouped_and_the_key_table_cache(gpu):
    total = len(reference("ed25519")[1])
    cold, warm = run_generic("ed25519", [total, total + 1000 - (total + 1000) % 64 + 1])
    assert cold[1] == 0 and cold[2] >= 5 and cold[0] == cold[2], cold
    assert warm[2] == 0 and warm[1] == cold[0], (cold, warm)


def test_ed25519_hot_key_pool_takes_the_wide_pass(gpu):
    cs, lanes, pad = reference("ed25519")
    n = len(lanes) + 2000
    batch = Batch("ed25519", lanes, n)
    blob = batch.tuples
    try:
        sbv.set_grouping(True, 64, 2, 4096)
        sbv.key_cache(False, 0, sbv.SCHEME_ED25519)
        sbv.key_cache(True, 1024, sbv.SCHEME_ED25519)
        sbv.ed_hot_keys(8, 400)
        for i in range(4):
            compare(("ed hot keys", i), batch, sbv.ed25519_verify_batch(blob, n))
        h = sbv.ed_hot_key_stats()
        assert 1 <= h[0] <= 8 and h[2] >= len(lanes) - 128, h           # the case key's tuples (all but the wavefronts at the ends of its run) through the wide pass
        assert all(sbv.ed_hot_selfcheck(i) for i in range(h[0]))
    finally:
        sbv.ed_hot_keys(1024, 4096)
        sbv.key_cache(False, 0, sbv.SCHEME_ED25519)
        sbv.key_cache(True, 1024, sbv.SCHEME_ED25519)
        sbv.set_grouping(True, sbv.GROUP_MIN_BATCH_DEFAULT, 0, 0)


@pytest.mark.parametrize("bits", [0, 16])
def test_ed25519_registered_keys(gpu, bits):
    front = len(wavefronts("ed25519", "key8")) + len(reference("ed25519")[1])
    sizes = [front + (r - front) % 64 for r in (1, 63, 65)]
    ran = run_registered("ed25519", sizes, [bits])
    assert [r[1] % 64 for r in ran] == [1, 63, 1]


# ---- settings read once at start-up: a fresh child process each --------------------------------------------------------------------
def child(what):
    """runs in a child process whose environment holds the setting under test; regenerates the cases (fixed seeds)"""
    assert any(os.environ.get(name) == value for env, w in SETTINGS if w == what for name, value in env.items()), what
    sbv.init(0)
    if what == "p256":
        st, cl = run_p256_generic()
        assert st[1] >= len(reference("p256")[1]) and cl[0] >= 5 and cl[2] > 0, (st, cl)
        run_registered("p256", [len(wavefronts("p256", "key8")) + len(reference("p256")[1])], [0])
    elif what == "k256":
        total = len(reference("k256")[1])
        run_generic("k256", [total])
        run_registered("k256", [len(wavefronts("k256", "key8")) + total], [0])
    elif what == "ed25519":
        total = len(reference("ed25519")[1])
        run_generic("ed25519", [total, total + 3000])                 # ungrouped_list inside: every case through the ungrouped list's kernel
        run_registered("ed25519", [len(wavefronts("ed25519", "key8")) + total], [0])
    print("scalar walks ok: " + what)


SETTINGS = [({"SBV_G_BITS": "16"}, "p256"), ({"SBV_QPHASE_LDS": "1"}, "p256"), ({"SBV_K256_G_BITS": "16"}, "k256"),
            ({"SBV_ED_B_BITS": "16"}, "ed25519"), ({"SBV_ED_UNGROUPED_QUAD": "1"}, "ed25519")]


def test_settings_read_at_start_up_in_fresh_children(gpu):
    """SBV_G_BITS / SBV_K256_G_BITS / SBV_ED_B_BITS = 16 against the defaults the tests above run with, SBV_QPHASE_LDS=1 (the LDS-staged
    chunk launches of the phased grouped step) and SBV_ED_UNGROUPED_QUAD=1: one child at a time, each under its own timeout; the first
    child that fails ends the test and no further one is started."""
    sources = "".join(open(os.path.join(sc.CSRC, f)).read() for f in sorted(os.listdir(sc.CSRC)) if f.endswith(".hip"))
    for env, what in SETTINGS:
        assert all('getenv("%s")' % name in sources for name in env), env      # a misspelt name would test the defaults once more
        r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); import test_gpu_scalar_walks as t; t.child(%r)" % (HERE, what)],
                           env=dict(os.environ, **env), capture_output=True, text=True, timeout=180, cwd=ROOT)
        assert r.returncode == 0 and r.stdout.strip().endswith("scalar walks ok: " + what), (env, r.returncode, r.stdout[-500:], r.stderr[-1500:])
