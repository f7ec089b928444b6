"""GPU tier of the raw-message entries of the generic verifiers: the cases of tests/msgs_generic_cases.py through verify_msgs,
secp256k1_verify_msgs and verify_msgs_sharded (include/sbv.h: sbv_p256_verify_msgs, sbv_secp256k1_verify_msgs,
sbv_p256_verify_msgs_sharded), so that the hipcc-compiled k_msg_frontend_tuples hashes every message length, parses every DER shape
and carries every key the CPU tier (tests/test_msgs_generic_cpu.py) has proved on the emulated lane.  Every call's bitmap is compared
whole with the case module's `want` — hashlib, the Python strict parse and the C oracles — and, bit for bit, with verify_batch /
secp256k1_verify_batch on the tuples the host route builds from the same cases.

One process, one launch at a time.  A binding that raises SbvError with a device error fails its test and every later test of the
module is skipped: nothing more is launched on a device that has just faulted."""
import ctypes
import os
import subprocess
import sys
import time

import pytest

import consensus_amd as sbv
import msgs_generic_cases as mg

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SBV_EINVAL, SBV_EDEVICE, SBV_ENOTINIT = -2, -4, -5        # include/sbv.h
ENTRY = {"p256": sbv.verify_msgs, "k256": sbv.secp256k1_verify_msgs}
TUPLES = {"p256": sbv.verify_batch, "k256": sbv.secp256k1_verify_batch}
# sizes at which the launch geometry gains a wavefront or a workgroup (k_msg_frontend_tuples: 256 lanes per workgroup; the bitmap: 64
# verdicts per ballot), at which the step changes form (the grouped step from 64 tuples on) and the ragged size of the stream tier
SIZES = (1, 63, 64, 65, 255, 256, 257, 511, 513, 8229)


class Device:
    faulted = None


@pytest.fixture(scope="module")
def dev():
    sbv.init(0)
    t0 = time.perf_counter()
    yield Device()
    print(f"\ntest_gpu_msgs_generic: {time.perf_counter() - t0:.1f} s of wall time")


def guarded(dev, fn, *args, **kw):
    if dev.faulted:
        pytest.skip("an earlier call of this module returned a device error: " + dev.faulted)
    try:
        return fn(*args, **kw)
    except sbv.SbvError as e:
        if e.code == SBV_EDEVICE:
            dev.faulted = str(e)
        raise


def check(dev, scheme, cases, what):
    """one call of the entry: the whole bitmap equals `want` and equals the tuple entry's on the host-built tuples"""
    msgs, sigs, keys, want = mg.batch(cases)
    n = len(cases)
    got = sbv.bitmap_to_list(guarded(dev, ENTRY[scheme], msgs, sigs, keys), n)
    assert got == want, (scheme, what, [c.name for c, g in zip(cases, got) if g != c.want][:12])
    ref = sbv.bitmap_to_list(guarded(dev, TUPLES[scheme], mg.tuples(cases), n), n)
    assert got == ref, (scheme, what, [c.name for c, g, r in zip(cases, got, ref) if g != r][:12])
    return got


@pytest.mark.parametrize("scheme", mg.SCHEMES)
def test_ladder_in_both_packings_then_short_calls(dev, scheme):
    """(a): every length 0..260, 1023, 1024, 1025, 4097 and 65 537 with its flipped twins in ONE call; the same cases shuffled, verdict
    by verdict the same; then short calls, whose uploads leave the long call's bytes behind them in the staging buffers"""
    up, shuffled, perm = mg.ladder(scheme)
    a = check(dev, scheme, up, "ascending")
    b = check(dev, scheme, shuffled, "shuffled")
    assert b == [a[p] for p in perm]
    check(dev, scheme, mg.families(scheme)["e"], "family e behind the ladder")
    check(dev, scheme, mg.empty_batch(scheme), "empty messages behind the ladder")
    check(dev, scheme, mg.filler(scheme), "filler behind the ladder")


@pytest.mark.parametrize("family", ["b", "c", "d", "e"])
@pytest.mark.parametrize("scheme", mg.SCHEMES)
def test_family_in_one_call(dev, scheme, family):
    got = check(dev, scheme, mg.families(scheme)[family], family)
    if family == "b":
        assert all(got) and len(got) == 42
    if family == "e":
        assert got == [True, True, True, False, True]          # no slot rule here: the two slot cases are judged on their signature


@pytest.mark.parametrize("scheme", mg.SCHEMES)
def test_sample_of_cases_alone(dev, scheme):
    """32 cases over all families and the key cases, each alone in a call"""
    cases = mg.sample(scheme)
    assert len(cases) == 32
    for c in cases:
        check(dev, scheme, [c], c.name)


@pytest.mark.parametrize("scheme", mg.SCHEMES)
def test_cases_interleaved_with_honest_filler_at_the_geometry_edges(dev, scheme):
    """every case but the long messages alternating with honest filler, at every size of SIZES; each size starts at another case, so
    that every case is sent"""
    pool = mg.pool(scheme)
    shift = calls = 0
    while shift < len(pool) or calls < len(SIZES):
        n = SIZES[calls % len(SIZES)]
        check(dev, scheme, mg.interleaved(scheme, pool, n, shift), "n = %d from case %d" % (n, shift))
        shift += (n + 1) // 2
        calls += 1
    assert calls >= len(SIZES)


@pytest.mark.parametrize("scheme", mg.SCHEMES)
def test_key_cases(dev, scheme):
    """Qx = p, Qy = p + 1 over the point with y = 1 (and that point itself), a flipped bit of Qy, (0, 0), the other curve's key and the
    negated key under a signature the honest key accepts: one accept, seven rejects, in one call and between honest filler"""
    cases = mg.key_cases(scheme)
    assert check(dev, scheme, cases, "key cases") == [True] + [False] * 7
    check(dev, scheme, mg.interleaved(scheme, cases, 70), "key cases in a grouped step")


def _raw_call(scheme, msgs_blob, mo, sigs_blob, so, keys_blob, n, out):
    lib = sbv.load()
    fn = lib.sbv_p256_verify_msgs if scheme == "p256" else lib.sbv_secp256k1_verify_msgs
    C, U64P = ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)
    fn.argtypes = [C, U64P, C, U64P, C, ctypes.c_size_t, ctypes.c_void_p]
    return fn(msgs_blob, mo, sigs_blob, so, keys_blob, n, out)


def _tables(parts):
    o = (ctypes.c_uint64 * (len(parts) + 1))()
    for i, p in enumerate(parts):
        o[i + 1] = o[i] + len(p)
    return o


@pytest.mark.parametrize("scheme", mg.SCHEMES)
def test_all_messages_empty_and_a_null_message_pointer(dev, scheme):
    cases = mg.empty_batch(scheme)
    _, sigs, keys, want = mg.batch(cases)
    n = len(cases)
    out = ctypes.create_string_buffer((n + 7) // 8)
    zero = (ctypes.c_uint64 * (n + 1))()

    def call():
        sbv._check(_raw_call(scheme, None, zero, b"".join(sigs), _tables(sigs), b"".join(keys), n, out))
    guarded(dev, call)
    assert sbv.bitmap_to_list(out.raw, n) == want == [True, True, False, True, True, True]


@pytest.mark.parametrize("scheme", mg.SCHEMES)
def test_a_call_of_1000_then_a_call_of_10(dev, scheme):
    """no verdict of the first call survives in the second: the ten cases are rejects where the first call's first ten were accepts"""
    big = mg.interleaved(scheme, mg.filler(scheme), 1000)
    got = check(dev, scheme, big, "1 000")
    assert all(got[:10])
    rejects = [c for c in mg.families(scheme)["d"] if not c.want][:10]
    assert len(rejects) == 10
    assert check(dev, scheme, rejects, "10 behind 1 000") == [False] * 10
    mixed = rejects[:5] + mg.filler(scheme)[:5]
    assert check(dev, scheme, mixed, "10 mixed") == [False] * 5 + [True] * 5


@pytest.mark.parametrize("scheme", mg.SCHEMES)
def test_long_tailed_signers_cold_then_warm(dev, scheme):
    """12 signers above and 12 below the 256 uses of a full P-256 table and 100 keys used once, the keys written by the front end: the
    grouped step builds its tables from them.  Cold (the key-table cache emptied by a restart of the library) and again warm."""
    cases = mg.long_tail(scheme)
    msgs, sigs, keys, want = mg.batch(cases)
    assert want == [i % 5 != 4 for i in range(mg.MAIN)]
    guarded(dev, sbv.shutdown)
    guarded(dev, sbv.init, 0)
    tuples = mg.tuples(cases)
    for run in ("cold", "warm", "warm again"):
        got = sbv.bitmap_to_list(guarded(dev, ENTRY[scheme], msgs, sigs, keys), mg.MAIN)
        assert got == want, (scheme, run, [i for i, (g, w) in enumerate(zip(got, want)) if g != w][:12])
    assert sbv.bitmap_to_list(guarded(dev, TUPLES[scheme], tuples, mg.MAIN), mg.MAIN) == want


@pytest.mark.parametrize("scheme", mg.SCHEMES)
def test_refused_calls_leave_the_library_as_it_was(dev, scheme):
    """each null pointer, a first offset != 0, a decreasing table and n = 2^21 + 1 (with one-element arrays: refused before they are
    read) are SBV_EINVAL; a good call follows each and verifies"""
    cases = mg.key_cases(scheme) + mg.filler(scheme)[:9]
    msgs, sigs, keys, want = mg.batch(cases)
    n = len(cases)
    mb, sb, kb = b"".join(msgs), b"".join(sigs), b"".join(keys)
    mo, so = _tables(msgs), _tables(sigs)
    out = ctypes.create_string_buffer((n + 7) // 8)
    first_not_0 = _tables(msgs)
    first_not_0[0] = 1
    dec_m, dec_s = _tables(msgs), _tables(sigs)
    dec_m[3], dec_s[5] = dec_m[2] - 1, dec_s[4] - 1
    one = (ctypes.c_uint64 * 1)(0)
    refused = [("null msg_offsets", (mb, None, sb, so, kb, n, out)), ("null sig_offsets", (mb, mo, sb, None, kb, n, out)),
               ("null keys", (mb, mo, sb, so, None, n, out)), ("null bitmap", (mb, mo, sb, so, kb, n, None)),
               ("null msgs with bytes to read", (None, mo, sb, so, kb, n, out)), ("null sigs with bytes to read", (mb, mo, None, so, kb, n, out)),
               ("first message offset 1", (mb, first_not_0, sb, so, kb, n, out)), ("message offsets decrease", (mb, dec_m, sb, so, kb, n, out)),
               ("signature offsets decrease", (mb, mo, sb, dec_s, kb, n, out)),
               ("n = 2^21 + 1", (b"\0", one, b"\0", one, b"\0" * 64, (1 << 21) + 1, ctypes.create_string_buffer(1)))]
    for what, args in refused:
        rc = guarded(dev, _raw_call, scheme, *args)
        assert rc == SBV_EINVAL, (what, rc)
        check(dev, scheme, cases, "behind: " + what)
    assert _raw_call(scheme, None, None, None, None, None, 0, None) == 0            # n == 0: SBV_OK, nothing read or written


_NOT_INIT = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
import consensus_amd as sbv
lib = sbv.load()
C, U64P = ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)
one, out = (ctypes.c_uint64 * 2)(0, 1), ctypes.create_string_buffer(8)
rcs = []
for name in ("sbv_p256_verify_msgs", "sbv_secp256k1_verify_msgs"):
    fn = getattr(lib, name)
    fn.argtypes = [C, U64P, C, U64P, C, ctypes.c_size_t, ctypes.c_void_p]
    rcs += [fn(b"m", one, b"s", one, bytes(64), 1, out), fn(None, None, None, None, None, 0, None)]
print("before-init", *rcs)
"""


def test_before_init_the_entries_answer_enotinit(dev):
    r = subprocess.run([sys.executable, "-c", _NOT_INIT, ROOT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("before-init"))
    assert line == "before-init " + " ".join(["%d" % SBV_ENOTINIT] * 4)


# ---- the sharded entry ----------------------------------------------------------------------------------------------------------------
def _with_pieces(dev, piece, body):
    """body() with SBV_SHARD_PIECE = piece read by a fresh sbv_init_all; the module's plain sbv_init(0) afterwards"""
    os.environ["SBV_SHARD_PIECE"] = str(piece)
    try:
        guarded(dev, sbv.shutdown)
        assert guarded(dev, sbv.init_all) >= 1
        body()
    finally:
        os.environ.pop("SBV_SHARD_PIECE", None)
        sbv.shutdown()
        sbv.init(0)


@pytest.mark.parametrize("place", ["last of a piece", "first of a piece"])
def test_sharded_entry_in_three_pieces_with_the_long_message_at_a_piece_edge(dev, place):
    """verify_msgs_sharded with SBV_SHARD_PIECE = 512: 1 536 signatures go up as three pieces of 512, each with its slice of the offset
    tables and its keys; the 65 537-byte message and its twins the last case of each piece in one run, the first in the other"""
    up = mg.ladder("p256")[0]
    long4 = [c for c in up if len(c.msg) == 65537]
    rest = [c for c in up if len(c.msg) != 65537]
    assert len(long4) == 4 and len(rest) == 1057
    rest += mg.interleaved("p256", mg.key_cases("p256") + mg.families("p256")["d"], 1536 - 4 - len(rest))
    at = (511, 1023, 1535, 700) if place == "last of a piece" else (0, 512, 1024, 700)
    cases = list(rest)
    for pos, c in sorted(zip(at, long4)):
        cases.insert(pos, c)
    assert len(cases) == 1536 and [cases[p] for p in at] == long4
    msgs, sigs, keys, want = mg.batch(cases)

    def body():
        got, q, info = guarded(dev, sbv.verify_msgs_sharded, msgs, sigs, keys)
        got = sbv.bitmap_to_list(got, len(cases))
        assert info.shards == 1 and q is None
        assert got == want, (place, [(i, c.name) for i, (c, g) in enumerate(zip(cases, got)) if g != c.want][:12])
        assert got == sbv.bitmap_to_list(guarded(dev, sbv.verify_batch, mg.tuples(cases), len(cases)), len(cases))
    _with_pieces(dev, 512, body)


def test_sharded_entry_quorum_bits_by_distinct_keys(dev):
    """group = 3, quorum = 2: the granule of a piece is lcm(512, 8 x 3) = 1 536 signatures, so 4 608 signatures go up in three pieces
    of 1 536 (SBV_SHARD_PIECE = 1536).  Proposals of three signatures by one, two and three distinct keys, accepted and spoiled: the
    quorum bits are the model's, the accept bits `want` and the tuple route's."""
    fill, tail = mg.filler("p256"), mg.long_tail("p256")
    cases = []
    for p in range(1536):
        kind = p % 4
        if kind == 0:
            cases += tail[3 * p:3 * p + 3]                               # whatever the long tail holds: mixed signers, every fifth spoiled
        elif kind == 1:
            cases += [fill[(3 * p) % 97], fill[(3 * p + 3) % 97], fill[(3 * p + 6) % 97]]        # honest signatures, often by one key
        elif kind == 2:
            cases += [fill[p % 97], fill[(p + 1) % 97], mg.key_cases("p256")[1 + p % 7]]         # two keys accepted, one key case rejected
        else:
            cases += [fill[p % 97], mg.families("p256")["d"][1 + p % 100], mg.key_cases("p256")[5]]
    assert len(cases) == 4608
    msgs, sigs, keys, want = mg.batch(cases)
    want_q = mg.quorum_bits(want, keys, 3, 2)
    assert 200 < sum(want_q) < 1336

    def body():
        got, q, info = guarded(dev, sbv.verify_msgs_sharded, msgs, sigs, keys, 3, 2)
        assert info.shards == 1
        assert sbv.bitmap_to_list(got, 4608) == want
        assert sbv.bitmap_to_list(q, 1536) == want_q
        assert sbv.bitmap_to_list(got, 4608) == sbv.bitmap_to_list(guarded(dev, sbv.verify_batch, mg.tuples(cases), 4608), 4608)
    _with_pieces(dev, 1536, body)


_LOGICAL = r"""
import os, sys
root = sys.argv[1]
sys.path[:0] = [root, os.path.join(root, "tests"), os.path.join(root, "oracle")]
import consensus_amd as sbv
import msgs_generic_cases as mg
assert sbv.init_all() == 3
up = mg.ladder("p256")[0]
cases = [c for c in up if len(c.msg) < 4097] + mg.interleaved("p256", mg.pool("p256"), 2048)
cases = cases[:3072]
assert len(cases) == 3072
msgs, sigs, keys, want = mg.batch(cases)
got, _, info = sbv.verify_msgs_sharded(msgs, sigs, keys)
print("shards", info.shards, info.devices, info.tuples_per_shard)
print("whole", "equal" if sbv.bitmap_to_list(got, 3072) == want else "DIFFERS")
# offset tables that do not start at 0: the same call with 1 000 and 77 bytes in front of the messages and the signatures
mo, so = [1000], [77]
for m, s in zip(msgs, sigs):
    mo.append(mo[-1] + len(m)); so.append(so[-1] + len(s))
got2, q2, info2 = sbv.verify_msgs_sharded([b"\xee" * 1000 + msgs[0]] + msgs[1:], [b"\x30" * 77 + sigs[0]] + sigs[1:], keys, 3, 2, offsets=(mo, so))
print("based", "equal" if sbv.bitmap_to_list(got2, 3072) == want else "DIFFERS", info2.shards)
print("quorum", "equal" if sbv.bitmap_to_list(q2, 1024) == mg.quorum_bits(want, keys, 3, 2) else "DIFFERS")
# sbv_shard_mode is not consulted: the key-affine mode set, the split stays contiguous
sbv.shard_mode(True, 3)
got3, _, info3 = sbv.verify_msgs_sharded(msgs, sigs, keys)
print("mode", "equal" if got3 == got else "DIFFERS", info3.shards, info3.mode)
sbv.shutdown()
"""


def test_sharded_entry_over_three_logical_devices(dev):
    """a child process under SBV_LOGICAL_DEVICES=3 with SBV_SHARD_MIN=1024: 3 072 signatures in three shards on three contexts (shard
    offsets > 0, each shard's slice of the tables starting above 0), then the same call with offset tables that do not start at 0 and
    with quorum bits, then with the key-affine mode set, which this entry does not follow"""
    env = dict(os.environ, SBV_LOGICAL_DEVICES="3", SBV_SHARD_MIN="1024")
    r = subprocess.run([sys.executable, "-c", _LOGICAL, ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = dict(ln.split(" ", 1) for ln in r.stdout.splitlines() if ln.split(" ", 1)[0] in ("shards", "whole", "based", "quorum", "mode"))
    assert lines["shards"].split()[:2] == ["3", "3"], lines
    assert lines["whole"] == "equal" and lines["based"] == "equal 2", lines           # whole proposals of 3 in whole bitmap words: shards of 1 536
    assert lines["quorum"] == "equal", lines
    assert lines["mode"].split()[:2] == ["equal", "3"] and lines["mode"].split()[2] in ("1", "2"), lines


# ---- the host Verifier over the real backend -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [0, 2, 1])
def test_verifier_sends_unregistered_clients_through_the_device_front_end(dev, scheme, oracle):
    """Scheme P-256, secp256k1 and Ed25519 over libsbv.so: a proposal that carries requests of clients without a slot takes ONE call of
    the raw-message entry (sbv_p256_verify_msgs, sbv_secp256k1_verify_msgs, sbv_ed25519_verify_msgs) instead of tuples built by the
    host workers; the verdicts are the callback backend's on the same bytes (tests/test_msgs_generic_cpu.py)"""
    import hostlib
    from test_host_verifier import Harness
    from test_msgs_generic_cpu import proposals_of_unregistered_clients, unregistered_clients
    lib = hostlib.load()
    hx = Harness(lib, oracle, backend_kind=0, wait_us=10, scheme=scheme)
    try:
        unregistered_clients(lib, hx, scheme)
        assert proposals_of_unregistered_clients(lib, hx) == 5
        assert hx.batches == []                                # nothing went to the stand-in
    finally:
        hx.close()
        sbv.init(0)


def test_ed25519_rewire_equals_the_tuple_route(dev):
    """what the Verifier now sends for unregistered Ed25519 clients (sbv_ed25519_verify_msgs) against what it sent before
    (make_tuple_ed25519 per request = ed25519_make_tuples, then ed25519_verify_batch): the same bitmap on the Ed25519 ladder, the
    key cases of its slot family and a wrong-length signature laid out as the Verifier lays it out (R = 0, S = 2^256 - 1)"""
    import frontend_cases as fc
    cases = [c for c in fc.ladder("ed25519")[0] + fc.slot_rules("ed25519") + fc.empty_batch("ed25519") if c.rule == fc.OWN]
    msgs, sigs, _, pks, want = fc.batch("ed25519", cases)
    msgs, sigs, pks, want = msgs + [b"short signature"], sigs + [bytes(32) + b"\xff" * 32], pks + [pks[0]], want + [False]
    n = len(msgs)
    got = sbv.bitmap_to_list(guarded(dev, sbv.ed25519_verify_msgs, sigs, pks, msgs), n)
    tuples = guarded(dev, sbv.ed25519_make_tuples, sigs, pks, msgs)
    assert got == sbv.bitmap_to_list(guarded(dev, sbv.ed25519_verify_batch, tuples, n), n) == want
