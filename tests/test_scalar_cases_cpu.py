"""CPU tier for tests/scalar_cases.py: proves the generators before a GPU sees them.

  reference  every case has ONE verdict: the Python twin, the C oracle and (both ECDSA curves) OpenSSL agree with the verdict by construction —
             forged tuples accept, their twins reject, the designed infinities reject.  tests/test_gpu_scalar_walks.py uses that list.
  models     decoding every scalar through its walker model gives the digits the family names; the mid-walk cases' partial sums
             equal +- the entry; the GLV model is the emulator's split; the widths are the library's.
  emulator   every case through the host-compiled lanes of its path (a second system under test, never the reference), and the
             comb-of-G / comb-of-B cases through the comb-walk entries at their own width.
  counts     per family and walker, asserted: nothing is skipped silently."""
import collections
import ctypes
import multiprocessing
import os
import re
import subprocess

import pytest

import scalar_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
THREADS = min(16, os.cpu_count() or 1)
V, S, U32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32


def _emul_lib(src_name, so_name, defs):
    src, so = os.path.join(HERE, "emul", src_name), os.path.join(HERE, "emul", so_name)
    csrc = os.path.join(HERE, "..", "consensus_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-misleading-indentation"] + defs + [src, "-o", so])
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def emul():
    lib = _emul_lib("emul.cc", "libsbv_emul.so", ["-DSBV_F29_CHECK", "-DSBV_F25_CHECK", "-DSBV_K256_CHECK"])
    lib.sbve_p256_verify_batch.argtypes = [ctypes.c_char_p, S, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    lib.sbve_p256_verify_batch_keyed.argtypes = [ctypes.c_char_p, V, S, ctypes.c_char_p, U32, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    lib.sbve_p256_verify_batch_grouped.argtypes = [ctypes.c_char_p, S, ctypes.c_char_p, U32, U32, U32, V]
    lib.sbve_set_keyed_wide.argtypes = [ctypes.c_int, ctypes.c_uint]
    lib.sbve_set_full_table_min.argtypes = [U32]
    lib.sbve_hot_keys.argtypes = [U32, U32]
    lib.sbve_key_cache.argtypes = [ctypes.c_int, U32]
    lib.sbve_coop_disagreements.restype = lib.sbve_small_disagreements.restype = ctypes.c_ulong
    lib.sbve_k256_verify_batch.argtypes = [ctypes.c_char_p, S, ctypes.c_char_p]
    lib.sbve_k256_verify_batch_grouped.argtypes = [ctypes.c_char_p, S, ctypes.c_char_p, U32, U32, U32, ctypes.c_int, V]
    lib.sbve_ed25519_verify_batch.argtypes = [ctypes.c_char_p, S, ctypes.c_char_p]
    lib.sbve_ed25519_verify_batch_grouped.argtypes = [ctypes.c_char_p, S, ctypes.c_char_p, U32, U32, U32, ctypes.c_int, ctypes.c_int, V]
    lib.sbve_ed_hot_keys.argtypes = [U32, U32]
    lib.sbve_scheme_key_cache.argtypes = [ctypes.c_int, ctypes.c_int, U32]
    return lib


@pytest.fixture(scope="module")
def k256_keyed_emul():
    lib = _emul_lib("k256_keyed_emul.cc", "libsbv_k256_keyed_emul.so", [])
    lib.sbvk256_verify_keyed.argtypes = [ctypes.c_char_p, V, S, ctypes.c_char_p, S, V, V, V]
    lib.sbvk256_verify_keyed.restype = ctypes.c_ulong
    return lib


@pytest.fixture(scope="module")
def ed_keyed_emul():
    lib = _emul_lib("ed_keyed_emul.cc", "libsbv_ed_keyed_emul.so", ["-DSBV_F25_CHECK"])
    lib.sbvk_verify_keyed.argtypes = [ctypes.c_char_p, V, S, ctypes.c_char_p, S, V, V, V]
    lib.sbvk_verify_keyed.restype = ctypes.c_ulong
    return lib


def _bits(bm, n):
    return [bool((bm[i >> 3] >> (i & 7)) & 1) for i in range(n)]


def _mismatch(cs, got):
    """family and case of every verdict that is not the agreed one"""
    return [(c.walker, c.family, c.name, g) for c, g in zip(cs, got) if g != c.expect][:10]


def _twin_verdict(job):
    scheme, t = job
    return {"p256": sc.ec, "k256": sc.kc, "ed25519": sc.ed}[scheme].verify_tuple(t)


# ---- reference verdicts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", sc.SCHEMES)
def test_every_case_has_one_agreed_verdict(oracle, openssl_check, scheme):
    """Python twin == C oracle == OpenSSL (both ECDSA curves) == the verdict by construction, for every case.  Ed25519 has two judges,
    not three: OpenSSL verifies a message and hashes k itself, so a tuple with a chosen k cannot be put to it."""
    cs = sc.cases(scheme)
    with multiprocessing.get_context("fork").Pool(THREADS) as pool:
        twin = pool.map(_twin_verdict, [(scheme, c.tuple) for c in cs], chunksize=32)
    assert not _mismatch(cs, twin)
    fn = {"p256": oracle.sbvo_p256_verify_tuple, "k256": oracle.sbvo_k256_verify_tuple, "ed25519": oracle.sbvo_ed25519_verify_tuple}[scheme]
    fn.argtypes = [ctypes.c_char_p]
    assert not _mismatch(cs, [bool(fn(c.tuple)) for c in cs])
    if scheme != "ed25519":
        judge = getattr(openssl_check, "sbvssl_%s_verify_tuple" % scheme)
        judge.argtypes = [ctypes.c_char_p]
        assert not _mismatch(cs, [bool(judge(c.tuple)) for c in cs])
    # forged cases accept and their twins reject; the only scalars without a valid signature are the designed infinities
    for c in cs:
        assert c.expect == (not c.name.endswith("/twin") and not c.designed_reject), c
        if c.designed_reject:
            assert c.family == "collision" and ":infinity" in c.name and c.name.startswith("last"), c
    want = 0 if scheme == "ed25519" else 2 * 2 * sum(1 for w in sc.walkers(scheme).values() if w.role == "u2" and w.sequential)
    assert sum(c.designed_reject for c in cs) == want             # the last addition of either sign of scalar, with its twin, per comb walker


# ---- counts ------------------------------------------------------------------------------------------------------------------------
COUNTS = {
    "p256": {"g20": dict(edges=24, uniform=8, single=74), "g16": dict(edges=24, uniform=8, single=96, carry=6),
             "key8": dict(edges=22, uniform=6, single=252, carry=16, builder=36, collision=24),
             "wide16": dict(edges=22, uniform=6, single=124, carry=16, builder=112, collision=24),
             "wide18": dict(edges=22, uniform=6, single=116, builder=124, collision=24),
             "key8c": dict(edges=22, uniform=6, single=192, carry=6, builder=36),
             "lane4": dict(edges=22, uniform=6, single=384, carry=6), "narrow": dict(builder=56, carry=14, collision=32)},
    "k256": {"g20": dict(edges=24, uniform=8, single=74), "g16": dict(edges=24, uniform=8, single=96, carry=6),
             "key8": dict(edges=22, uniform=6, single=252, carry=16, builder=36, collision=24),
             "wide16": {"edges": 22, "uniform": 6, "single": 96, "carry": 6, "builder": 64, "builder-c3": 16, "collision": 24},
             "glv": dict(glv=60)},
    "ed25519": {"b20": dict(edges=22, uniform=8, single=74), "b16": dict(edges=22, uniform=8, single=92),
                "key8": dict(edges=22, uniform=8, single=188, builder=36, doubling=6),
                "wide16": dict(edges=22, uniform=8, single=92, builder=76, doubling=6), "lane4": dict(edges=22, uniform=8, single=380)},
}
UNREACHABLE = {"p256": 143, "k256": 53, "ed25519": 151}


@pytest.mark.parametrize("scheme", sc.SCHEMES)
def test_case_counts_per_family_and_walker(scheme):
    """Every family of every walker has the number of cases it was designed with (each forged tuple counts with its twin); the digit
    patterns that no scalar of the range produces are counted too, and are only of the kinds the recoding rules out."""
    cs = sc.cases(scheme)
    got = collections.defaultdict(dict)
    for (w, f), k in collections.Counter((c.walker, c.family) for c in cs).items():
        got[w][f] = k
    assert dict(got) == COUNTS[scheme]
    assert len(cs) == sum(sum(f.values()) for f in COUNTS[scheme].values())
    assert len({c.tuple for c in cs}) >= len(cs) - 8 * len(sc.walkers(scheme))      # edge scalars repeat between walkers of one role, nothing else
    un = sc.unreachable(scheme)
    assert len(un) == UNREACHABLE[scheme]
    ws = sc.walkers(scheme)
    for w, family, name in un:
        m = re.match(r"w(\d+):([+-])(1|half)$", name)
        if family in ("edges", "uniform"):
            assert name in ("0", "zero") and ws[w].role == "u2", (w, family, name)          # u2 = 0 has no signature
        else:
            # +2^(bits-1) is a digit only of a flipped walk; a negative digit needs a window above it to borrow from; the top windows of
            # a scalar below n (below L < 2^253) take few values
            assert family == "single" and m, (w, family, name)
            j, top = int(m.group(1)), ws[w].windows - 1
            assert (m.group(2) == "+" and m.group(3) == "half" and not ws[w].flip) or j >= top - (2 if scheme == "ed25519" else 1), (w, name)


# ---- the models do what they claim ---------------------------------------------------------------------------------------------------
def test_model_widths_are_the_librarys():
    assert sc.KEY_WINDOWS == 33 and sc.KEY_BITS == 8 and sc.ED_KEY_WINDOWS == 32 and sc.NARROW_PER_WINDOW == 16
    assert sc.G_BITS == {"p256": 20, "k256": 20, "ed25519": 20} and set(sc.G_BITS_ONE_LANE.values()) == {16}
    assert (sc.K256_WIDE_BITS, sc.define("k256_keyed.h", "SBV_K256_WIDE_WINDOWS"), sc.K256_WIDE_RUN) == (16, 17, 64)
    assert (sc.ED_WIDE_BITS, sc.define("ed25519_core.h", "SBV_ED_HOT_WINDOWS"), sc.ED_WIDE_RUN) == (16, 16, 32)
    assert sc.define("p256_core.h", "SBV_G16_WINDOWS") == sc.ecdsa_windows(16) == 17 and sc.define("ed25519_core.h", "SBV_ED_B16_WINDOWS") == sc.ed_windows(16)
    shape = {s: {w.name: (w.bits, w.windows, w.flip) for w in sc.walkers(s).values()} for s in sc.SCHEMES}
    assert shape["p256"] == {"g20": (20, 13, False), "g16": (16, 17, False), "key8": (8, 33, True), "wide16": (16, 17, True), "wide18": (18, 15, True),
                             "key8c": (8, 33, False), "narrow": (8, 33, True), "lane4": (4, 65, False)}
    assert shape["k256"] == {"g20": (20, 13, False), "g16": (16, 17, False), "key8": (8, 33, True), "wide16": (16, 17, False)}
    assert shape["ed25519"] == {"b20": (20, 13, False), "b16": (16, 16, False), "key8": (8, 32, False), "wide16": (16, 16, False), "lane4": (4, 64, False)}
    import consensus_amd as sbv
    assert sbv.WIDE_BITS_AUTO == 1                                  # widths 16 and 18 are set per call (sbv_p256_wide_keys)


@pytest.mark.parametrize("scheme", sc.SCHEMES)
def test_decoding_a_case_through_its_model_gives_the_intended_digits(scheme):
    """Big integers only: digits sum back to the scalar, and every family's scalars have the digits its name says."""
    ws = dict(sc.walkers(scheme))
    n = sc.ORDER[scheme]
    seen = collections.Counter()
    for c in sc.cases(scheme):
        if c.name.endswith("/twin") or c.walker == "glv":
            continue
        w = ws[c.walker]
        u = c.a if w.role in ("u1", "S") else c.b
        d = w.digits(u)
        assert sum(x << (w.bits * j) for j, x in enumerate(d)) % n == u and all(-w.half <= x <= w.half for x in d), c
        assert sum(t[2] for t in w.terms(u)) % n == u
        top = w.windows - 1
        if c.family == "single":
            m = re.match(r"w(\d+):([+-])(1|half)$", c.name)
            j, x = int(m.group(1)), (1 if m.group(3) == "1" else w.half) * (1 if m.group(2) == "+" else -1)
            others = [(i, y) for i, y in enumerate(d) if y and i != j]
            assert d[j] == x and (others == [] or (others[0][0] == j + 1 and abs(others[0][1]) == 1 and len(others) == 1)), (c, d)
            seen[(c.walker, j, abs(x))] += 1
        elif c.family == "uniform":
            x = {"zero": 0, "minus-one": -1, "plus-max": w.half - 1, "minus-half": -w.half}[c.name]
            assert all(y == x for y in d[:top - 2]) and (x != 0 or not any(d)), (c, d)
        elif c.family == "carry":
            T = w.carry_threshold()
            walked = n - u if w.flips(u) else u
            assert (d[top] != 0) == (walked >= T) and abs(d[top]) <= 1, (c, d)
            seen[(c.walker, "carries", d[top] != 0)] += 1
            seen[(c.walker, top - 1, abs(d[top - 1]))] += 1      # at the threshold every digit below the carry is -2^(bits-1): the top row's last entry
        elif c.family in ("builder", "builder-c3"):
            ms = sc.K256_C3_MULTIPLES if c.family == "builder-c3" else ([1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 120, 121, 127, 128] if w.narrow else sc.builder_multiples(w))
            s = int(re.match(r"rot(\d+)", c.name).group(1))
            rows = top - 1 if w.bits * top == 256 or scheme == "ed25519" else top      # the last row may have gone to keeping the scalar in range
            assert [abs(x) for x in d[:rows]] == [ms[(j + s) % len(ms)] for j in range(rows)], (c, d)
            for j in range(rows):
                seen[(c.walker, j, abs(d[j]))] += 1
        elif c.family == "collision":
            where, part, kind = c.name.split(":")[:3]
            terms = w.terms(c.b)
            hits = [t for t in range(len(terms)) if (c.a + c.d * sum(x[2] for x in terms[:t])) % n == (c.d * terms[t][2] * (1 if kind == "doubling" else -1)) % n]
            assert len(hits) == 1 and terms[hits[0]][1] == part, (c, hits)
            assert hits[0] == {"first": 0, "last": len(terms) - 1}.get(where, hits[0]) and (where in ("first", "last") or 0 < hits[0] < len(terms) - 1)
            assert ("flip" in c.name) == w.flips(c.b)
            seen[(c.walker, "collision", part, kind, w.flips(c.b))] += 1
        elif c.family == "doubling":
            terms = w.terms(c.b)
            assert sum(1 for t in range(len(terms)) if (c.a - c.d * sum(x[2] for x in terms[:t])) % n == (-c.d * terms[t][2]) % n) == 1, c
    for w in ws.values():
        if w.narrow:
            assert all(seen[(w.name, "collision", part, kind, f)] for part in ("giant", "baby") for kind in ("doubling", "infinity") for f in (False, True))
            continue
        carry_top = scheme != "ed25519" and w.bits * (w.windows - 1) == 256
        rows = w.windows - 1 if carry_top else w.windows - (2 if scheme == "ed25519" else 1)
        for j in range(rows):                                        # the first and the last entry of every row below the top
            assert seen[(w.name, j, 1)] and seen[(w.name, j, w.half)], (w.name, j)
        if carry_top:
            assert seen[(w.name, "carries", True)] and seen[(w.name, "carries", False)], w.name
        if w.role in ("u2", "k") and not w.descending:               # every builder multiple in every row the square covers
            for j in range(rows - 1):
                assert all(seen[(w.name, j, m)] for m in sc.builder_multiples(w)), (w.name, j)
            if w.role == "u2" and w.sequential:
                assert all(seen[(w.name, "collision", "entry", kind, f)] for kind in ("doubling", "infinity") for f in ((False, True) if w.flip else (False,)))


def test_glv_model_is_the_emulators_split_and_the_family_covers_it(emul):
    """ksc_split_lambda in Python == the host-compiled one on every GLV case; the family holds the four sign combinations, either
    half with its carry nibble set and clear (the two never carry together: the reduced lattice cell does not reach that corner), and
    halves at the bound (above 2^127)."""
    out = (ctypes.c_uint32 * 18)()
    emul.sbve_k256_split_lambda.argtypes = [V, V]
    signs, carries, big = set(), set(), 0
    for c in sc.cases("k256"):
        if c.walker != "glv" or c.name.endswith("/twin"):
            continue
        k1, n1, k2, n2 = sc.glv_split(c.b)
        emul.sbve_k256_split_lambda((ctypes.c_uint32 * 8)(*[(c.b >> (32 * i)) & 0xFFFFFFFF for i in range(8)]), out)
        assert (k1, k2) == (sum(out[i] << (32 * i) for i in range(8)), sum(out[8 + i] << (32 * i) for i in range(8))), c
        assert (int(n1), int(n2)) == (out[16], out[17]), c
        assert ((-k1 if n1 else k1) + (-k2 if n2 else k2) * sc.u256_const("k256_sc.h", "k256_lambda_words")) % sc.kc.N == c.b
        signs.add((n1, n2))
        carries.add(sc.glv_carries(c.b))
        big += k1 >> 127 != 0 or k2 >> 127 != 0
    assert len(signs) == 4 and carries == {(False, False), (True, False), (False, True)} and big >= 4


# ---- the emulator: a second system under test ------------------------------------------------------------------------------------------
def _run(fn, total, *args):
    bm = ctypes.create_string_buffer((total + 7) // 8)
    fn(*args, bm)
    return _bits(bm.raw, total)


def test_p256_cases_through_the_emulated_lanes(emul):
    """One-lane generic (both widths of the comb of G), registered keys in the three forms with 8-bit combs and with 16- and 18-bit wide
    combs, the grouped step with full tables, with rows only, and with hot keys."""
    cs = sc.cases("p256")
    blob, total = sc.blob(cs), len(cs)
    rsh, slots, keys = sc.split_keyed("p256", blob)
    arr = (ctypes.c_uint32 * total)(*slots)
    stats, classes, hs = (ctypes.c_uint32 * 4)(), (ctypes.c_uint32 * 3)(), (ctypes.c_uint32 * 4)()
    try:
        for gbits in (16, 20):
            emul.sbve_set_gcomb_bits(gbits)
            bm = ctypes.create_string_buffer((total + 7) // 8)
            emul.sbve_p256_verify_batch(blob, total, bm, 64, 4)
            assert not _mismatch(cs, _bits(bm.raw, total)), gbits
        for bits in (0, 16, 18):
            emul.sbve_set_keyed_wide(bits or 16, 1 if bits else 0)    # slot 0: the key every comb case signs with (the rows-only key stays narrow)
            for form in (0, 1):
                emul.sbve_set_keyed_coop(form)
                bm = ctypes.create_string_buffer((total + 7) // 8)
                emul.sbve_p256_verify_batch_keyed(rsh, arr, total, b"".join(keys), len(keys), bm, 64, 4)
                assert not _mismatch(cs, _bits(bm.raw, total)), (bits, form)
            emul.sbve_set_keyed_coop(3)                          # the one-launch form: 32 records a call
            got = []
            for off in range(0, total, 32):
                m = min(32, total - off)
                bm = ctypes.create_string_buffer((m + 7) // 8)
                emul.sbve_p256_verify_batch_keyed(rsh[96 * off:96 * (off + m)], (ctypes.c_uint32 * m)(*slots[off:off + m]), m, b"".join(keys), len(keys), bm, 64, 1)
                got += _bits(bm.raw, m)
            assert not _mismatch(cs, got), (bits, "one-launch")
        assert emul.sbve_coop_disagreements() == 0 and emul.sbve_small_disagreements() == 0
        for full_min, want_rows in ((8, False), (1 << 30, True)):
            emul.sbve_set_full_table_min(full_min)
            bm = ctypes.create_string_buffer((total + 7) // 8)
            emul.sbve_p256_verify_batch_grouped(blob, total, bm, 2, 16, 10, stats)
            assert not _mismatch(cs, _bits(bm.raw, total)), full_min
            emul.sbve_last_table_classes(classes)
            assert stats[1] == total and (classes[2] == total if want_rows else classes[2] == 0 and classes[0] == 2), (list(stats), list(classes))
        emul.sbve_set_full_table_min(8)
        emul.sbve_key_cache(1, 16)
        emul.sbve_hot_keys(2, 50)
        for _ in range(2):                                       # promoted behind the first batch, the wide pass in the second
            bm = ctypes.create_string_buffer((total + 7) // 8)
            emul.sbve_p256_verify_batch_grouped(blob, total, bm, 2, 16, 10, stats)
            assert not _mismatch(cs, _bits(bm.raw, total))
        emul.sbve_hot_stats(hs)
        assert hs[0] == 2 and hs[2] >= total - 128, list(hs)
    finally:
        emul.sbve_set_keyed_coop(0)
        emul.sbve_set_keyed_wide(16, 0)
        emul.sbve_set_gcomb_bits(16)
        emul.sbve_hot_keys(0, 4096)
        emul.sbve_key_cache(0, 0)
        emul.sbve_set_full_table_min(256)


def test_k256_cases_through_the_emulated_lanes(emul, k256_keyed_emul):
    """One-lane GLV kernel, the grouped step (1 to 4 chunks), registered keys with 8-bit combs and widened (combs built by the device's
    builder lanes, the c = 3 runs included)."""
    cs = sc.cases("k256")
    blob, total = sc.blob(cs), len(cs)
    bm = ctypes.create_string_buffer((total + 7) // 8)
    emul.sbve_k256_verify_batch(blob, total, bm)
    assert not _mismatch(cs, _bits(bm.raw, total))
    stats = (ctypes.c_uint32 * 4)()
    for chunks in (1, 3):
        bm = ctypes.create_string_buffer((total + 7) // 8)
        emul.sbve_k256_verify_batch_grouped(blob, total, bm, 2, 16, 10, chunks, stats)
        assert not _mismatch(cs, _bits(bm.raw, total)), chunks
        assert stats[1] == total, list(stats)
    recs, slots, keys = sc.split_keyed("k256", blob)
    arr = (ctypes.c_uint32 * total)(*slots)
    for widen, lanes in ((None, 0), ((ctypes.c_uint8 * len(keys))(*[1] * len(keys)), total)):
        bm = ctypes.create_string_buffer((total + 7) // 8)
        wide = k256_keyed_emul.sbvk256_verify_keyed(recs, arr, total, b"".join(keys), len(keys), widen, bm, None)
        assert not _mismatch(cs, _bits(bm.raw, total)), lanes
        assert wide == lanes


def test_ed25519_cases_through_the_emulated_lanes(emul, ed_keyed_emul):
    """One-lane kernel, the grouped step at both widths of the comb of B, the hot-key pool, registered keys narrow and widened."""
    cs = sc.cases("ed25519")
    blob, total = sc.blob(cs), len(cs)
    bm = ctypes.create_string_buffer((total + 7) // 8)
    emul.sbve_ed25519_verify_batch(blob, total, bm)
    assert not _mismatch(cs, _bits(bm.raw, total))
    stats, hs = (ctypes.c_uint32 * 4)(), (ctypes.c_uint32 * 6)()
    try:
        for bbits in (16, 20):
            emul.sbve_set_ed_b_bits(bbits)
            bm = ctypes.create_string_buffer((total + 7) // 8)
            emul.sbve_ed25519_verify_batch_grouped(blob, total, bm, 8, 64, 12, 2, 4, stats)
            assert not _mismatch(cs, _bits(bm.raw, total)), bbits
            assert stats[1] == total, list(stats)
        emul.sbve_scheme_key_cache(2, 1, 16)
        emul.sbve_ed_hot_keys(2, 250)
        for _ in range(2):
            bm = ctypes.create_string_buffer((total + 7) // 8)
            emul.sbve_ed25519_verify_batch_grouped(blob, total, bm, 8, 64, 12, 2, 4, stats)
            assert not _mismatch(cs, _bits(bm.raw, total))
        emul.sbve_ed_hot_stats(hs)
        assert hs[0] == 1 and hs[2] >= total - 64, list(hs)
    finally:
        emul.sbve_set_ed_b_bits(16)
        emul.sbve_ed_hot_keys(0, 4096)
        emul.sbve_scheme_key_cache(2, 0, 0)
    recs, slots, keys = sc.split_keyed("ed25519", blob)
    arr = (ctypes.c_uint32 * total)(*slots)
    for widen, lanes in ((None, 0), ((ctypes.c_uint8 * len(keys))(*[1] * len(keys)), total)):
        bm = ctypes.create_string_buffer((total + 7) // 8)
        wide = ed_keyed_emul.sbvk_verify_keyed(recs, arr, total, b"".join(keys), len(keys), widen, bm, None)
        assert not _mismatch(cs, _bits(bm.raw, total)), lanes
        assert wide == lanes


def _words(x):
    return (ctypes.c_uint32 * 8)(*[(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)])


def test_comb_walk_entries_at_the_width_of_each_family(emul):
    """The comb-walk entries of the emulator alone, each family at the width it was made for: sbve_k256_gcomb_mul walks u1 of the
    secp256k1 g16 and g20 cases through k256_gphase_point at 16 and at 20 bits (the grouped emulation above has the 16-bit comb only),
    sbve_ed_comb_mul walks S of the Ed25519 b16 and b20 cases through ed_add_sB_comb; the point that comes out == the twins' own sum."""
    emul.sbve_k256_gcomb_mul.argtypes = [V, ctypes.c_int, V]
    emul.sbve_ed_comb_mul.argtypes = [V, ctypes.c_char_p]
    out = (ctypes.c_uint32 * 16)()
    walked = collections.Counter()
    for name, w in sc.walkers("k256").items():
        if w.role != "u1":
            continue
        for c in sc.cases("k256"):
            if c.walker != name or c.name.endswith("/twin"):
                continue
            got = emul.sbve_k256_gcomb_mul(_words(c.a), w.bits, out)
            want = sc.base_mul("k256", c.a)
            if want is None:
                assert got == 0, (name, c.name)
            else:
                assert got == 1 and (sum(out[i] << (32 * i) for i in range(8)), sum(out[8 + i] << (32 * i) for i in range(8))) == want, (name, c.family, c.name)
            walked[name] += 1
    enc = ctypes.create_string_buffer(32)
    try:
        for name, w in sc.walkers("ed25519").items():
            if w.role != "S":
                continue
            emul.sbve_set_ed_b_bits(w.bits)
            for c in sc.cases("ed25519"):
                if c.walker != name or c.name.endswith("/twin"):
                    continue
                emul.sbve_ed_comb_mul(_words(c.a), enc)
                assert enc.raw == sc.ed.encode(sc.base_mul("ed25519", c.a)), (name, c.family, c.name)
                walked[name] += 1
    finally:
        emul.sbve_set_ed_b_bits(16)
    assert walked == {"g20": 53, "g16": 67, "b20": 52, "b16": 61}, walked
