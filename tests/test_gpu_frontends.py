"""GPU tier of the message front ends: the cases of tests/frontend_cases.py through the five entries that take raw bytes —
verify_msgs_keyed, verify_msgs_keyed_sharded, secp256k1_verify_msgs_keyed, ed25519_verify_msgs, ed25519_verify_msgs_keyed — so that
the hipcc-compiled k_msg_frontend, k_ed_msg_frontend and k_ed_keyed_msg_frontend hash every message length and parse every DER
shape the CPU tier (tests/test_frontend_cases_cpu.py) has proved on the emulated lanes.  Expected verdicts are the case module's:
hashlib, the Python strict parse and the C oracles, never another build of the lanes.

One process, one launch at a time.  A binding that raises SbvError with a device error fails its test and every later test of the
module is skipped: nothing more is launched on a device that has just faulted.  The three registries are filled once for the
module, in the order of frontend_cases.keys(), and emptied behind it."""
import ctypes
import os
import time

import pytest

import consensus_amd as sbv
import frontend_cases as fc

pytestmark = pytest.mark.gpu
SBV_EDEVICE = -4                                   # include/sbv.h

REGISTER = {"p256": sbv.register_keys, "k256": sbv.secp256k1_register_keys, "ed25519": sbv.ed25519_register_keys}
CLEAR = {"p256": sbv.clear_keys, "k256": sbv.secp256k1_clear_keys, "ed25519": sbv.ed25519_clear_keys}
ENTRIES = ["p256", "k256", "ed25519", "ed25519_unkeyed"]

# Batch sizes at which an entry's step changes form, and the line each comes from.  No entry changes kernels below 8 192 tuples
# (enqueue_keyed: launch_p256_verify_keyed takes k_p256_verify_keyed_coop up to coop_max_batch() = 32 768 and prep_chunk_T stays 1
# below 131 072; launch_k256_verify_keyed: k256_keyed_prep_T stays 1 below 2^14; launch_ed25519_verify_keyed has one form), so
# the sizes are those at which the launch geometry gains a wavefront, a workgroup or a lane's share:
SIZES = {
    # enqueue_keyed -> launch_p256_verify_keyed: SBV_COOP_LANES = 8 lanes per signature, so a wavefront holds 8 signatures and a
    # workgroup of SBV_VERIFY_BLOCK = 256 lanes 32; k_msg_frontend and the bitmap bytes: 256 per workgroup, 64 per ballot
    "p256": (7, 8, 9, 32, 33, 63, 64, 65, 256, 257),
    # launch_k256_verify_keyed: k_k256_keyed_prep 64 lanes per workgroup at T = 1; k_k256_keyed_verify SBV_VERIFY_BLOCK = 256, one
    # ballot of 64 verdicts per wavefront
    "k256": (63, 64, 65, 255, 256, 257),
    # launch_ed25519_verify_keyed: k_ed_gphase / k_ed_keyed_qphase SBV_VERIFY_BLOCK = 256 with one ballot per wavefront, k_ed_finish
    # one inversion per SBV_ED_FINISH_T = 8 tuples, k_pack_bitmap 8 verdicts per byte; k_ed_keyed_msg_frontend 256 per workgroup
    "ed25519": (7, 8, 9, 63, 64, 65, 256, 257),
}


class Device:
    faulted = None


@pytest.fixture(scope="module")
def dev():
    sbv.init(0)
    for scheme in fc.SCHEMES:
        CLEAR[scheme]()
        assert REGISTER[scheme](fc.keys(scheme)) == list(range(len(fc.keys(scheme))))
    t0 = time.perf_counter()
    yield Device()
    for scheme in fc.SCHEMES:
        CLEAR[scheme]()
    print(f"\ntest_gpu_frontends: {time.perf_counter() - t0:.1f} s of wall time")


def guarded(dev, fn, *args):
    if dev.faulted:
        pytest.skip("an earlier call of this module returned a device error: " + dev.faulted)
    try:
        return fn(*args)
    except sbv.SbvError as e:
        if e.code == SBV_EDEVICE:
            dev.faulted = str(e)
        raise


def own(cases):
    """the cases the unkeyed entry can be sent: it takes the key itself, so a slot outside the registry has no form there"""
    return [c for c in cases if c.rule == fc.OWN]


def send(dev, entry, cases):
    """the verdicts of `cases`, in one call of `entry`"""
    scheme = "ed25519" if entry == "ed25519_unkeyed" else entry
    msgs, sigs, slots, keys, _ = fc.batch(scheme, cases)
    if entry == "p256":
        bm = guarded(dev, sbv.verify_msgs_keyed, msgs, sigs, slots)
    elif entry == "k256":
        bm = guarded(dev, sbv.secp256k1_verify_msgs_keyed, msgs, sigs, slots)
    elif entry == "ed25519":
        bm = guarded(dev, sbv.ed25519_verify_msgs_keyed, sigs, msgs, slots)
    else:
        bm = guarded(dev, sbv.ed25519_verify_msgs, sigs, keys, msgs)
    return sbv.bitmap_to_list(bm, len(cases))


def check(dev, entry, cases, what):
    if entry == "ed25519_unkeyed":
        cases = own(cases)
    got = send(dev, entry, cases)
    want = [c.want for c in cases]
    assert got == want, (entry, what, [c.name for c, g, w in zip(cases, got, want) if g != w][:12])
    return got


@pytest.mark.parametrize("entry", ENTRIES)
def test_ladder_in_both_packings_then_short_messages(dev, entry):
    """(a): every length 0..260, 1023, 1024, 1025, 4097 and 65 537 with its three flipped twins in ONE call, so that the lanes of a
    wavefront hash different lengths; then the same cases shuffled, verdict by verdict the same — what lies behind a message is not
    hashed; then calls with short messages only, whose uploads leave the long call's bytes behind them in the staging buffers."""
    scheme = "ed25519" if entry == "ed25519_unkeyed" else entry
    up, shuffled, perm = fc.ladder(scheme)
    a = check(dev, entry, up, "ascending")
    b = check(dev, entry, shuffled, "shuffled")
    assert b == [a[p] for p in perm]
    check(dev, entry, fc.slot_rules(scheme), "slot rules behind the ladder")
    check(dev, entry, fc.empty_batch(scheme), "empty messages behind the ladder")
    check(dev, entry, fc.filler(scheme), "filler behind the ladder")


@pytest.mark.parametrize("family", ["b", "c", "d", "e"])
@pytest.mark.parametrize("entry", ["p256", "k256"])
def test_ecdsa_family_in_one_call(dev, entry, family):
    """(b) accepted r and s of 1, 2, 31 and 32 bytes, (c) r and s between the two orders, (d) the generated DER bends, (e) the slot
    rules: all cases of a family in one call, so that the lanes of a wavefront parse different shapes."""
    cases = fc.families(entry)[family]
    got = check(dev, entry, cases, family)
    if family == "b":
        assert all(got) and len(got) == 42
    if family == "e":
        assert got == [True, False, False, False, True]


@pytest.mark.parametrize("entry", ENTRIES)
def test_sample_of_cases_alone(dev, entry):
    """32 cases over all families, each alone in a call (n = 1: one live lane in the only wavefront)"""
    scheme = "ed25519" if entry == "ed25519_unkeyed" else entry
    cases = fc.sample(scheme)
    assert len(cases) == 32
    for c in cases:
        if entry == "ed25519_unkeyed" and c.rule != fc.OWN:
            continue
        assert send(dev, entry, [c]) == [c.want], (entry, c.name)


@pytest.mark.parametrize("entry", ENTRIES)
def test_families_interleaved_with_honest_filler_at_the_geometry_edges(dev, entry):
    """The families other than the ladder, and the ladder's cases of up to 260 bytes, alternating with honest filler, at every size of
    SIZES; each size starts at another case, so that every case is sent."""
    scheme = "ed25519" if entry == "ed25519_unkeyed" else entry
    fams = fc.families(scheme)
    pool = [c for f in sorted(fams) if f != "a" for c in fams[f]] + [c for c in fams["a"] if len(c.msg) <= 260][::7]
    sizes = SIZES[scheme]
    shift = calls = 0
    while shift < len(pool) or calls < len(sizes):         # go round the sizes until every case and every size has been sent
        n = sizes[calls % len(sizes)]
        check(dev, entry, fc.interleaved(scheme, pool, n, shift), "n = %d from case %d" % (n, shift))
        shift += (n + 1) // 2
        calls += 1


@pytest.mark.parametrize("entry", ENTRIES)
def test_all_messages_empty_and_a_null_message_pointer(dev, entry):
    """A batch whose messages are all empty may come with a null `msgs` pointer (check_offsets: the payload is null only when empty)"""
    scheme = "ed25519" if entry == "ed25519_unkeyed" else entry
    cases = fc.empty_batch(scheme)
    _, sigs, slots, keys, want = fc.batch(scheme, cases)
    n = len(cases)
    lib = sbv.load()
    V, S, C, U64P = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)
    zero =(ctypes.c_uint64 * (n + 1))()
    so = (ctypes.c_uint64 * (n + 1))()
    for i, s in enumerate(sigs):
        so[i + 1] = so[i] + len(s)
    arr = (ctypes.c_uint32 * n)(*slots)
    out = ctypes.create_string_buffer((n + 7) // 8)

    def call():                                            # the argument types are the bindings' own; None is the null pointer
        if entry == "p256":
            sbv._check(lib.sbv_p256_verify_msgs_keyed(None, zero, b"".join(sigs), so, arr, n, out))
        elif entry == "k256":
            lib.sbv_secp256k1_verify_msgs_keyed.argtypes = [C, U64P, C, U64P, V, S, V]
            sbv._check(lib.sbv_secp256k1_verify_msgs_keyed(None, zero, b"".join(sigs), so, arr, n, out))
        elif entry == "ed25519":
            lib.sbv_ed25519_verify_msgs_keyed.argtypes = [C, C, U64P, V, S, V]
            sbv._check(lib.sbv_ed25519_verify_msgs_keyed(b"".join(sigs), None, zero, arr, n, out))
        else:
            sbv._check(lib.sbv_ed25519_verify_msgs(b"".join(sigs), b"".join(keys), None, zero, n, out))
    guarded(dev, call)
    assert sbv.bitmap_to_list(out.raw, n) == want == [True, True, False, True, True, True]


def test_ed25519_entries_agree_with_the_tuple_route(dev):
    """The unkeyed entry equals ed25519_make_tuples + ed25519_verify_batch (k hashed on the host); the keyed entry equals the unkeyed
    one and `want` — on the whole ladder and the slot cases that have a key."""
    cases = own(fc.ladder("ed25519")[0] + fc.slot_rules("ed25519") + fc.empty_batch("ed25519"))
    msgs, sigs, _, pks, want = fc.batch("ed25519", cases)
    unkeyed = send(dev, "ed25519_unkeyed", cases)
    tuples = guarded(dev, sbv.ed25519_make_tuples, sigs, pks, msgs)
    assert unkeyed == sbv.bitmap_to_list(guarded(dev, sbv.ed25519_verify_batch, tuples, len(cases)), len(cases))
    assert send(dev, "ed25519", cases) == unkeyed == want


@pytest.mark.parametrize("place", ["last of a piece", "first of a piece"])
def test_sharded_front_end_with_the_long_message_at_a_piece_edge(dev, place):
    """verify_msgs_keyed_sharded with SBV_SHARD_PIECE_KEYED = 512 (keyed_piece: 1 536 signatures go up as three pieces of 512, each
    with its slice of the offset tables): the ladder and filler, the 65 537-byte message and its twins the last case of each piece
    in one run and the first case of each piece in the other."""
    up = fc.ladder("p256")[0]
    long4 = [c for c in up if len(c.msg) == fc.LONGEST]
    rest = [c for c in up if len(c.msg) != fc.LONGEST]
    assert len(long4) == 4 and len(rest) == 1057
    rest += fc.interleaved("p256", fc.slot_rules("p256") + fc.der_ladder("p256"), 1536 - 4 - len(rest))
    at = (511, 1023, 1535, 700) if place == "last of a piece" else (0, 512, 1024, 700)
    cases = list(rest)
    for pos, c in sorted(zip(at, long4)):
        cases.insert(pos, c)
    assert len(cases) == 1536 and [cases[p] for p in at] == long4
    msgs, sigs, _, _, want = fc.batch("p256", cases)
    os.environ["SBV_SHARD_PIECE_KEYED"] = "512"
    try:
        guarded(dev, sbv.shutdown)
        assert guarded(dev, sbv.init_all) >= 1
        slot = guarded(dev, sbv.register_keys, fc.keys("p256"))
        assert slot == list(range(len(slot)))
        slots = fc.batch("p256", cases)[2]
        got, _, info = guarded(dev, sbv.verify_msgs_keyed_sharded, msgs, sigs, slots)
        got = sbv.bitmap_to_list(got, len(cases))
        assert info.shards == 1                            # one device's share, so the pieces are this call's
        assert got == want, (place, [(i, c.name) for i, (c, g) in enumerate(zip(cases, got)) if g != c.want][:12])
    finally:
        os.environ.pop("SBV_SHARD_PIECE_KEYED", None)
        sbv.shutdown()
        sbv.init(0)
        for scheme in fc.SCHEMES:                          # the module's registries, as the fixture left them
            CLEAR[scheme]()
            assert REGISTER[scheme](fc.keys(scheme)) == list(range(len(fc.keys(scheme))))
