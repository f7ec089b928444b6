"""GPU tier of BIP-340 Schnorr verification against registered secp256k1 keys (include/sbv.h: sbv_secp256k1_schnorr_lift_keys,
sbv_secp256k1_schnorr_verify_keyed, their _stream forms and sbv_debug_secp256k1_schnorr_keyed_op), through the C-ABI and the Python
wrapper.

Every byte the device writes is compared with tests/k256_schnorr_keyed_cases.py (the cases of the CPU tier,
tests/test_k256_schnorr_keyed_cpu.py): the 1 967 cases of the generic Schnorr set against slots of both parities, first on 8-bit
combs, then with three slots widened and the batch ordered so that a wavefront is all wide, has one live narrow lane, one dead lane, or
no live lane.  The verdicts are also held to sbv_secp256k1_schnorr_verify on the same items.  The _stream entry runs under callers that
do not synchronise, with the delay of tests/test_gpu_stream_order.py.  The tests run in the order of this file: the registry is built
once, widened once, and cleared by the last test."""
import ctypes
import hashlib
import os
import random
import subprocess
import sys
import time

import numpy as np
import pytest

import consensus_amd as sbv
import hostlib
import k256_schnorr_cases as sc
import k256_schnorr_keyed_cases as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, P = cases.N, cases.P
EINVAL, ENOTINIT = -2, -5
SENTINEL = 0x3C
T0 = time.perf_counter()


def _dev(torch, data, dtype=np.uint8):
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=dtype).copy()).cuda()


def _slots_dev(torch, slots):
    return torch.from_numpy(np.array(slots, dtype=np.uint32).view(np.int32)).cuda()


def _bad(got, its):
    return [(i, its[i][0], its[i][1], its[i][4]) for i in range(len(its)) if got[i] != its[i][5]]


@pytest.fixture(scope="module")
def reg():
    """the model's registry on the device: every key of the case set as x | y_even and x | p - y_even, the refused keys as lift_keys
    leaves them; the slots are the model's"""
    sbv.init(0)
    sbv.secp256k1_clear_keys()
    t = time.perf_counter()
    cases.items()
    cases.walk_cases()
    t1 = time.perf_counter()
    keys, slot_of, valid = cases.registry()
    assert sbv.secp256k1_register_keys(keys) == list(range(len(keys)))
    print("\n[secp256k1 schnorr keyed] the model: %.1f s; %d keys registered: %.2f s" % (t1 - t, len(keys), time.perf_counter() - t1))
    yield keys
    sbv.secp256k1_clear_keys()
    sbv.secp256k1_wide_keys(64)
    print("\n[secp256k1 schnorr keyed] wall time of this file: %.1f s" % (time.perf_counter() - T0))


@pytest.fixture(scope="module")
def wide(reg):
    """three slots widened; the device-built 16-bit combs equal the host builder's"""
    slots = cases.wide_slots()
    sbv.secp256k1_wide_keys(64)
    sbv.secp256k1_widen_keys(slots)
    assert sbv.secp256k1_wide_key_stats()[0] == 3
    for s in slots:
        assert sbv.secp256k1_wide_selfcheck(s), s
    return slots


# ---- lifting --------------------------------------------------------------------------------------------------------------------------
def test_lifting_against_the_model_with_refused_keys_in_the_batch(reg):
    pks = cases.xonly_keys() + [cases.be32(x) for x in (0, 1, 2, 3, 7, P - 1, P, P + 1, 2**256 - 1)]
    want = [cases.lift_key(pk) for pk in pks]
    keys, ok = sbv.secp256k1_schnorr_lift_keys(b"".join(pks))
    assert keys == b"".join(w[0] for w in want) and ok == bytes(w[1] for w in want)
    assert ok.count(0) >= 12 and ok.count(1) >= 299
    # lift + register gives the even registration's slot; a refused key gets its invalid slot
    slot_of = cases.registry()[1][0]
    some = cases.xonly_keys()[:5] + [pk for pk in cases.xonly_keys() if cases.lift_key(pk)[1] == 0][:3]
    slots, ok2 = sbv.secp256k1_schnorr_register_keys(b"".join(some))
    assert slots == [slot_of[pk] for pk in some] and ok2 == b"\x01" * 5 + b"\x00" * 3
    assert sbv.secp256k1_key_count() == len(reg)


# ---- every case, 8-bit combs ---------------------------------------------------------------------------------------------------------
def test_every_case_on_the_8_bit_combs(reg):
    assert sbv.secp256k1_wide_key_stats()[0] == 0
    its = cases.items()
    msgs, sigs, slots, want = cases.arrays()
    ok = sbv.secp256k1_schnorr_verify_keyed(msgs, sigs, slots)
    assert not _bad(ok, its), (len(_bad(ok, its)), _bad(ok, its)[:8])
    assert ok == want and ok.count(1) == 2 * 299


def test_agreement_with_the_generic_verifier(reg):
    """byte for byte what sbv_secp256k1_schnorr_verify answers for the same items with pk = the slot's Qx"""
    its = [i for i in cases.items() if i[4] < len(reg)]
    pks, msgs, sigs, want = cases.generic_arrays()
    generic = sbv.secp256k1_schnorr_verify(pks, msgs, sigs)
    keyed = sbv.secp256k1_schnorr_verify_keyed(msgs, sigs, [i[4] for i in its])
    assert keyed == generic == want


def test_walk_cases_on_the_8_bit_combs(reg):
    ins, slots, want, labels = cases.walk_cases()
    got = sbv.debug_secp256k1_schnorr_keyed_op(0, ins, slots)
    bad = [(i, labels[i]) for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (len(bad), bad[:8])


# ---- the same with three slots widened ---------------------------------------------------------------------------------------------------
def test_every_case_with_three_slots_widened_and_the_four_wavefront_compositions(wide):
    its = cases.wide_batch()
    assert cases.wide_lanes(its, wide) >= 128
    msgs, sigs, slots, want = cases.arrays(its)
    ok = sbv.secp256k1_schnorr_verify_keyed(msgs, sigs, slots)
    assert not _bad(ok, its), (len(_bad(ok, its)), _bad(ok, its)[:8])
    # ... and the plain order again, now that some wavefronts may be wide
    msgs, sigs, slots, want = cases.arrays()
    assert sbv.secp256k1_schnorr_verify_keyed(msgs, sigs, slots) == want


def test_walk_cases_on_the_16_bit_combs(wide):
    """every live lane's slot is widened, so every wavefront of the debug op walks the 16-bit combs"""
    ins, slots, want, labels = cases.walk_cases()
    assert {s for s, l in zip(slots, labels) if l != "dead"} <= set(wide)
    got = sbv.debug_secp256k1_schnorr_keyed_op(0, ins, slots)
    bad = [(i, labels[i]) for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (len(bad), bad[:8])


# ---- launch geometry ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 8229])
def test_launch_geometry_every_byte_and_nothing_behind_n(wide, n):
    import torch
    msgs, sigs, slots, want = cases.tiled(n, n)
    d_msg, d_sig, d_sl = _dev(torch, msgs), _dev(torch, sigs), _slots_dev(torch, slots)
    d_ok = torch.full((n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sbv.secp256k1_schnorr_verify_keyed_stream(d_msg.data_ptr(), d_sig.data_ptr(), d_sl.data_ptr(), n, d_ok.data_ptr())
    torch.cuda.synchronize()
    ok = d_ok.cpu().numpy().tobytes()
    if ok[:n] != want:
        bad = [i for i in range(n) if ok[i] != want[i]]
        raise AssertionError("n = %d: %d verdicts differ, first %s" % (n, len(bad), bad[:8]))
    assert ok[n:] == bytes([SENTINEL]) * 64, (n, "bytes behind the last ok were written")
    assert sbv.secp256k1_schnorr_verify_keyed(msgs, sigs, slots) == want                              # the host-pointer form
    # lifting: the first n keys of the tiled key list, sentinels behind keys64 and ok
    pks = (b"".join(cases.xonly_keys()) * (n // 300 + 1))[:32 * n]
    d_pk = _dev(torch, pks)
    d_keys = torch.full((64 * (n + 2),), SENTINEL, dtype=torch.uint8, device="cuda")
    d_lok = torch.full((n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sbv.secp256k1_schnorr_lift_keys_stream(d_pk.data_ptr(), n, d_keys.data_ptr(), d_lok.data_ptr())
    torch.cuda.synchronize()
    wl = [cases.lift_key(pks[32 * i:32 * i + 32]) for i in range(n)]
    assert d_keys.cpu().numpy().tobytes() == b"".join(w[0] for w in wl) + bytes([SENTINEL]) * 128, n
    assert d_lok.cpu().numpy().tobytes() == bytes(w[1] for w in wl) + bytes([SENTINEL]) * 64, n


# ---- refused calls --------------------------------------------------------------------------------------------------------------------
def test_refused_calls(wide):
    import torch
    lib = sbv.load()
    V, S = ctypes.c_void_p, ctypes.c_size_t
    lib.sbv_secp256k1_schnorr_lift_keys.argtypes = [V, S, V, V]
    lib.sbv_secp256k1_schnorr_lift_keys_stream.argtypes = [V, S, V, V, V]
    lib.sbv_secp256k1_schnorr_verify_keyed.argtypes = [V, V, V, S, V]
    lib.sbv_secp256k1_schnorr_verify_keyed_stream.argtypes = [V, V, V, S, V, V]
    lib.sbv_debug_secp256k1_schnorr_keyed_op.argtypes = [ctypes.c_int, V, V, V, S]
    n = 5
    msgs, sigs, slots, want = cases.tiled(n, 2)
    pks = b"".join(cases.xonly_keys()[:n])
    sent = lambda k: ctypes.create_string_buffer(bytes([SENTINEL]) * k, k)
    buf = lambda x: ctypes.create_string_buffer(x, len(x))
    sl = (ctypes.c_uint32 * n)(*slots)
    # host-pointer forms: null pointers; n = 0 writes nothing; ok of lift_keys may be null
    okb = sent(n)
    good = [buf(msgs), buf(sigs), sl, n, okb]
    for pos in (0, 1, 2, 4):
        args = list(good)
        args[pos] = None
        assert lib.sbv_secp256k1_schnorr_verify_keyed(*args) == EINVAL, pos
    assert lib.sbv_secp256k1_schnorr_verify_keyed(None, None, None, 0, None) == 0 and okb.raw == bytes([SENTINEL]) * n
    assert lib.sbv_secp256k1_schnorr_verify_keyed(*good) == 0 and okb.raw == want
    kb, lok = sent(64 * n), sent(n)
    assert lib.sbv_secp256k1_schnorr_lift_keys(None, n, kb, lok) == EINVAL and lib.sbv_secp256k1_schnorr_lift_keys(buf(pks), n, None, lok) == EINVAL
    assert lib.sbv_secp256k1_schnorr_lift_keys(None, 0, None, None) == 0 and kb.raw == bytes([SENTINEL]) * 64 * n
    assert lib.sbv_secp256k1_schnorr_lift_keys(buf(pks), n, kb, None) == 0
    assert kb.raw == b"".join(cases.lift_key(pks[32 * i:32 * i + 32])[0] for i in range(n)) and lok.raw == bytes([SENTINEL]) * n
    # the _stream forms: the same rules and the 4-byte alignment of the data
    t = {k: torch.full((4096,), SENTINEL, dtype=torch.uint8, device="cuda") for k in ("msg", "sig", "slot", "ok", "pk", "keys", "lok")}
    t["msg"][:32 * n] = _dev(torch, msgs)
    t["sig"][:64 * n] = _dev(torch, sigs)
    t["slot"][:4 * n] = _dev(torch, np.array(slots, dtype=np.uint32).tobytes())
    t["pk"][:32 * n] = _dev(torch, pks)
    torch.cuda.synchronize()
    p = {k: v.data_ptr() for k, v in t.items()}
    good = [p["msg"], p["sig"], p["slot"], n, p["ok"], None]
    for pos in (0, 1, 2, 4):
        args = list(good)
        args[pos] = None
        assert lib.sbv_secp256k1_schnorr_verify_keyed_stream(*args) == EINVAL, pos
    for pos in (0, 1, 2):
        for off in (1, 2):
            args = list(good)
            args[pos] += off
            assert lib.sbv_secp256k1_schnorr_verify_keyed_stream(*args) == EINVAL, (pos, off)
    args = list(good)
    args[3] = 0
    assert lib.sbv_secp256k1_schnorr_verify_keyed_stream(*args) == 0
    args[3] = (1 << 32) + 1
    assert lib.sbv_secp256k1_schnorr_verify_keyed_stream(*args) == EINVAL
    good_l = [p["pk"], n, p["keys"], p["lok"], None]
    for pos in (0, 2):
        args = list(good_l)
        args[pos] = None
        assert lib.sbv_secp256k1_schnorr_lift_keys_stream(*args) == EINVAL, pos
        args = list(good_l)
        args[pos] += 2
        assert lib.sbv_secp256k1_schnorr_lift_keys_stream(*args) == EINVAL, pos
    torch.cuda.synchronize()
    assert all(bool((t[k] == SENTINEL).all()) for k in ("ok", "keys", "lok"))                         # refused calls wrote nothing
    args = list(good)
    args[4] += 3                                                        # an odd address for the byte array is fine
    assert lib.sbv_secp256k1_schnorr_verify_keyed_stream(*args) == 0
    torch.cuda.synchronize()
    assert t["ok"].cpu().numpy().tobytes()[3:3 + n] == want
    # the debug op: only op 0, at most 65 536 cases
    rec = buf(cases.op_record(1, 1))
    out = sent(128)
    one = (ctypes.c_uint32 * 1)(0)
    for op in (-1, 1, 2):
        assert lib.sbv_debug_secp256k1_schnorr_keyed_op(op, rec, one, out, 1) == EINVAL
    assert lib.sbv_debug_secp256k1_schnorr_keyed_op(0, None, one, out, 1) == EINVAL
    assert lib.sbv_debug_secp256k1_schnorr_keyed_op(0, rec, None, out, 1) == EINVAL
    assert lib.sbv_debug_secp256k1_schnorr_keyed_op(0, rec, one, None, 1) == EINVAL
    assert lib.sbv_debug_secp256k1_schnorr_keyed_op(0, rec, one, out, 65537) == EINVAL and out.raw == bytes([SENTINEL]) * 128
    assert lib.sbv_debug_secp256k1_schnorr_keyed_op(0, None, None, None, 0) == 0


# ---- one slot, two schemes --------------------------------------------------------------------------------------------------------------
def test_one_slot_serves_ecdsa_and_schnorr_under_both_parities(wide):
    """a key registered once, as ECDSA registers it (Qx | Qy of whatever parity), accepts an ECDSA record through
    secp256k1_verify_batch_keyed and a BIP-340 signature through the new entry"""
    ds = [cases.be32(d) for d in range(2, 14)]
    pubs, pok = sbv.secp256k1_pubkeys(b"".join(ds))
    assert pok == b"\x01" * len(ds)
    parity = [pubs[64 * i + 63] & 1 for i in range(len(ds))]
    pick = [parity.index(0), parity.index(1)]
    for i in pick:
        d, q = ds[i], pubs[64 * i:64 * i + 64]
        (slot,) = sbv.secp256k1_register_keys([q])
        digest = hashlib.sha256(b"one slot, two schemes %d" % i).digest()
        esig, _, eok = sbv.secp256k1_sign_batch(d, digest, low_s=True)
        assert eok == b"\x01"
        rec, px, xok = sbv.secp256k1_schnorr_expand_keys(d)
        assert xok == b"\x01" and px == q[:32]
        ssig, sok = sbv.secp256k1_schnorr_sign(rec, digest)
        assert sok == b"\x01"
        spoiled = ssig[:40] + bytes([ssig[40] ^ 4]) + ssig[41:]
        assert sbv.bitmap_to_list(sbv.secp256k1_verify_batch_keyed(esig + digest, [slot]), 1) == [True]
        assert sbv.secp256k1_schnorr_verify_keyed(digest * 2, ssig + spoiled, [slot, slot]) == b"\x01\x00"
        assert sbv.secp256k1_schnorr_verify(px * 2, digest * 2, ssig + spoiled) == b"\x01\x00"


# ---- the first secp256k1 call of a process --------------------------------------------------------------------------------------------
_FIRST_CALL = r"""
import ctypes, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import consensus_amd as sbv
msgs, sigs, pks = (bytes.fromhex(x) for x in sys.argv[2:5])
n = len(sigs) // 64
dev = lambda x: torch.from_numpy(np.frombuffer(x, dtype=np.uint8).copy()).cuda()
d_msg, d_sig = dev(msgs), dev(sigs)
d_slot = torch.zeros(n, dtype=torch.int32, device="cuda")
d_out = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
lib = sbv.load()
V, S = ctypes.c_void_p, ctypes.c_size_t
lib.sbv_secp256k1_schnorr_verify_keyed_stream.argtypes = [V, V, V, S, V, V]
print("before-init", lib.sbv_secp256k1_schnorr_verify_keyed_stream(d_msg.data_ptr(), d_sig.data_ptr(), d_slot.data_ptr(), n, d_out.data_ptr(), None))
sbv.init(0)
st = torch.cuda.Stream()
torch.cuda.synchronize()
# the first secp256k1 call of the process: the _stream keyed verifier, on an empty registry
sbv.secp256k1_schnorr_verify_keyed_stream(d_msg.data_ptr(), d_sig.data_ptr(), d_slot.data_ptr(), n, d_out.data_ptr(), stream=st.cuda_stream)
torch.cuda.synchronize()
print("empty", d_out.cpu().numpy().tobytes().hex())
# lifting and registration upload no comb of G: the next call is the first that walks it
slots, ok = sbv.secp256k1_schnorr_register_keys(pks)
assert len(slots) == n
d_slot = torch.from_numpy(np.array(slots, dtype=np.uint32).view(np.int32)).cuda()
torch.cuda.synchronize()
sbv.secp256k1_schnorr_verify_keyed_stream(d_msg.data_ptr(), d_sig.data_ptr(), d_slot.data_ptr(), n, d_out.data_ptr(), stream=st.cuda_stream)
torch.cuda.synchronize()
print("out", d_out.cpu().numpy().tobytes().hex())
"""


def test_first_secp256k1_call_of_a_process_is_the_stream_entry(reg):
    """nothing has uploaded the comb of G before the _stream entry runs; before sbv_init the entry answers SBV_ENOTINIT"""
    idx = [i for i, c in enumerate(sc.cases()) if c[0] in ("valid", "s_bit", "pk_off_curve")][:300]
    good = [sc.cases()[i] for i in idx]
    pks = [c[1] for c in good]
    n = len(good)
    want = bytes(sc.expected_all()[i] for i in idx)
    assert want.count(1) >= 100 and want.count(0) >= 100
    r = subprocess.run([sys.executable, "-c", _FIRST_CALL, ROOT, b"".join(c[2] for c in good).hex(), b"".join(c[3] for c in good).hex(), b"".join(pks).hex()],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(ln.split(" ", 1) for ln in r.stdout.splitlines() if ln.startswith(("before-init", "empty", "out")))
    assert lines["before-init"] == "%d" % ENOTINIT
    assert bytes.fromhex(lines["empty"]) == bytes(n)
    assert bytes.fromhex(lines["out"]) == want


# ---- the _stream entry under callers that do not synchronise ----------------------------------------------------------------------------
N_STREAM = 8229


@pytest.fixture(scope="module")
def streams(wide):
    import torch
    from test_gpu_stream_order import DELAY_FACTOR, DELAY_MAX_MS, DELAY_MIN_MS, Delay

    class S:
        pass
    s = S()
    s.torch = torch
    s.want, s.src = {}, {}
    for g, shift in (("x", 0), ("y", 401)):                              # two generations: the same items, rotated against each other
        msgs, sigs, slots, ok = cases.tiled(N_STREAM, shift)
        s.want[g] = ok
        s.src[g] = [_dev(torch, msgs), _dev(torch, sigs), _slots_dev(torch, slots)]
    assert s.want["x"] != s.want["y"]
    s.bufs = [torch.empty_like(a) for a in s.src["x"]]
    s.outs = [torch.full((N_STREAM,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(3)]
    s.hosts = [torch.zeros(N_STREAM, dtype=torch.uint8).pin_memory() for _ in range(3)]
    s.stream = torch.cuda.Stream()
    torch.cuda.synchronize()                          # the fills above ran on the default stream

    def produce(g):
        for dst, a in zip(s.bufs, s.src[g]):
            dst.copy_(a, non_blocking=True)

    def call(k):
        """the entry from the input buffers, then the copy of the result into pinned memory: all on one stream"""
        b = s.bufs
        sbv.secp256k1_schnorr_verify_keyed_stream(b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), N_STREAM, s.outs[k].data_ptr(),
                                                  stream=s.stream.cuda_stream)
        s.hosts[k].copy_(s.outs[k], non_blocking=True)

    def check(k, g, what):
        got, want = s.hosts[k].numpy().tobytes(), s.want[g]
        if got != want:
            other = s.want["x" if g == "y" else "y"]
            a, w = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
            what_else = "the OTHER generation's" if got == other else "a mixture: %d bytes differ, first at %d" % (int((a != w).sum()), int(np.flatnonzero(a != w)[0]))
            raise AssertionError("%s: output %d is not generation %s's but %s" % (what, k, g.upper(), what_else))
    s.produce, s.call, s.check = produce, call, check
    s.delay = Delay(torch)
    with torch.cuda.stream(s.stream):
        produce("x")
        call(0)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call(0)
        b.record()
        torch.cuda.synchronize()
    ms = a.elapsed_time(b)
    s.delay_ms = min(DELAY_MAX_MS, max(DELAY_MIN_MS, DELAY_FACTOR * ms))
    check(0, "x", "warm call")
    print("\n[secp256k1 schnorr keyed, stream order] one warm call of %d: %.3f ms; delay %.1f ms" % (N_STREAM, ms, s.delay_ms))
    return s


def _held_back(s):
    """the delay on the current stream and an event behind it: still pending after the last enqueue = the GPU had everything queued first"""
    s.delay(s.delay_ms)
    gate = s.torch.cuda.Event()
    gate.record()
    return gate


@pytest.mark.parametrize("overwrite", [False, True], ids=["late_producer", "early_overwriter"])
def test_stream_late_producer_and_early_overwriter(streams, overwrite):
    s, torch = streams, streams.torch
    with torch.cuda.stream(s.stream):
        s.produce("x")
        torch.cuda.synchronize()
        gate = _held_back(s)
        s.produce("y")
        s.call(1)
        if overwrite:
            s.produce("x")
            s.hosts[1].copy_(s.outs[1], non_blocking=True)
        pending = not gate.query()
    torch.cuda.synchronize()
    assert pending, "the delay had run out before the last enqueue: the schedule proved nothing"
    s.check(1, "y", "early overwriter" if overwrite else "late producer")
    if overwrite:
        for dst, a in zip(s.bufs, s.src["x"]):
            assert torch.equal(dst, a)


def test_stream_x_y_x_back_to_back(streams):
    s, torch = streams, streams.torch
    with torch.cuda.stream(s.stream):
        gate = _held_back(s)
        for k, g in enumerate("xyx"):
            s.produce(g)
            s.call(k)
        pending = not gate.query()
    torch.cuda.synchronize()
    assert pending, "the delay had run out before the last enqueue: the schedule proved nothing"
    for k, g in enumerate("xyx"):
        s.check(k, g, "X-Y-X")


# ---- round trip -----------------------------------------------------------------------------------------------------------------------
def test_round_trip_on_the_device(wide):
    """expand -> sign -> lift + register -> spoil every third signature in one bit -> keyed verify, 8 229 items under 37 keys"""
    import torch
    n, nk = N_STREAM, 37
    keys = b"".join(cases.be32(int.from_bytes(hashlib.sha256(b"k256-schnorr-keyed-roundtrip%d" % i).digest(), "big") % (N - 1) + 1) for i in range(nk))
    rng = random.Random(0x8229)
    msgs, aux = rng.randbytes(32 * n), rng.randbytes(32 * n)
    idx = [(5 * i + i // nk) % nk for i in range(n)]
    d_keys, d_msg, d_aux, d_idx = _dev(torch, keys), _dev(torch, msgs), _dev(torch, aux), _slots_dev(torch, idx)
    d_rec, d_pk, d_eok = (torch.zeros(k, dtype=torch.uint8, device="cuda") for k in (64 * nk, 32 * nk, nk))
    d_sig, d_sok, d_vok = (torch.zeros(k, dtype=torch.uint8, device="cuda") for k in (64 * n, n, n))
    d_k64, d_lok = torch.zeros(64 * nk, dtype=torch.uint8, device="cuda"), torch.zeros(nk, dtype=torch.uint8, device="cuda")
    spoil_bit = torch.from_numpy(np.array([rng.randrange(512) if i % 3 == 2 else -1 for i in range(n)], dtype=np.int64)).cuda()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    sp = st.cuda_stream
    with torch.cuda.stream(st):
        sbv.secp256k1_schnorr_expand_keys_stream(d_keys.data_ptr(), nk, d_rec.data_ptr(), d_pk.data_ptr(), d_eok.data_ptr(), sp)
        sbv.secp256k1_schnorr_sign_stream(d_rec.data_ptr(), nk, d_idx.data_ptr(), d_msg.data_ptr(), d_aux.data_ptr(), n, d_sig.data_ptr(), d_sok.data_ptr(), sp)
        sbv.secp256k1_schnorr_lift_keys_stream(d_pk.data_ptr(), nk, d_k64.data_ptr(), d_lok.data_ptr(), sp)
        rows = torch.nonzero(spoil_bit >= 0).flatten()
        bits = spoil_bit[rows]
        flat = rows * 64 + bits // 8
        d_sig[flat] = d_sig[flat] ^ (1 << (bits % 8)).to(torch.uint8)
    torch.cuda.synchronize()
    # registration takes host pointers: the lifted keys come back once; the slots go to the device
    k64 = d_k64.cpu().numpy().tobytes()
    slots = sbv.secp256k1_register_keys([k64[64 * i:64 * i + 64] for i in range(nk)])
    d_slot = _slots_dev(torch, [slots[k] for k in idx])
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        sbv.secp256k1_schnorr_verify_keyed_stream(d_msg.data_ptr(), d_sig.data_ptr(), d_slot.data_ptr(), n, d_vok.data_ptr(), sp)
    torch.cuda.synchronize()
    assert bool((d_eok == 1).all()) and bool((d_sok == 1).all()) and bool((d_lok == 1).all())
    assert d_vok.cpu().numpy().tobytes() == bytes(0 if i % 3 == 2 else 1 for i in range(n))


# ---- the host layer -----------------------------------------------------------------------------------------------------------------------
def test_host_verify_schnorr_keyed_on_the_gpu_backend_equals_the_cpu_backend(wide):
    """Verifier::RegisterSchnorrKey and VerifySchnorrKeyed: one device call on the GPU backend, a loop over the host form on the CPU one"""
    host = hostlib.load()
    C = ctypes.c_char_p
    host.sbvh_register_schnorr_key.argtypes = [hostlib.V, C]
    host.sbvh_register_schnorr_key.restype = ctypes.c_long
    host.sbvh_backend_register_k256.argtypes = [hostlib.V, C]
    host.sbvh_backend_register_k256.restype = ctypes.c_long
    host.sbvh_verify_schnorr_keyed.argtypes = [hostlib.V, C, C, ctypes.c_void_p, ctypes.c_size_t, C]
    cb = hostlib.BACKEND_FN(lambda tuples, n, bitmap, user: 0)
    keys, _, valid = cases.registry()
    its = cases.wide_batch()
    msgs, sigs, slots, want = cases.arrays(its)
    n = len(its)
    got = []
    for kind in (0, 2):                                                 # libsbv.so on device 0, then the callback backend with a registry
        h = host.sbvh_verifier_new_scheme(2, kind, 0, cb, None, 64, 50, 0)
        try:
            for s, k in enumerate(keys):
                even = valid[s] == 0 or k[63] % 2 == 0
                assert (host.sbvh_register_schnorr_key(h, k[:32]) if even else host.sbvh_backend_register_k256(h, k)) == s, s
            ok = ctypes.create_string_buffer(n)
            assert host.sbvh_verify_schnorr_keyed(h, msgs, sigs, (ctypes.c_uint32 * n)(*slots), n, ok) == hostlib.OK
            got.append(ok.raw)
        finally:
            host.sbvh_verifier_free(h)
    assert got[0] == got[1] == want


# ---- an empty registry: the last test of the file --------------------------------------------------------------------------------------
def test_an_empty_registry_rejects_every_item(wide):
    import torch
    sbv.secp256k1_clear_keys()
    assert sbv.secp256k1_key_count() == 0
    n = 130
    msgs, sigs, slots, want = cases.tiled(n)
    assert want.count(1) > 0
    assert sbv.secp256k1_schnorr_verify_keyed(msgs, sigs, slots) == bytes(n)
    d_msg, d_sig, d_sl = _dev(torch, msgs), _dev(torch, sigs), _slots_dev(torch, slots)
    d_ok = torch.full((n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    sbv.secp256k1_schnorr_verify_keyed_stream(d_msg.data_ptr(), d_sig.data_ptr(), d_sl.data_ptr(), n, d_ok.data_ptr(), stream=st.cuda_stream)
    torch.cuda.synchronize()
    assert d_ok.cpu().numpy().tobytes() == bytes(n) + bytes([SENTINEL]) * 64
    ins, wslots, _, _ = cases.walk_cases()
    assert sbv.debug_secp256k1_schnorr_keyed_op(0, ins[:70], wslots[:70]) == [bytes(cases.OP_OUT)] * 70
