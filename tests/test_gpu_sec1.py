"""GPU tier of the SEC1 key decoders (include/sbv.h: sbv_p256_decode_keys, sbv_secp256k1_decode_keys, their _stream forms, the
_sec1 verify entries and sbv_debug_sec1_op), through the C-ABI and the Python wrapper.

Every byte the device writes is compared with the Python-integer model of tests/sec1_cases.py (the cases of the CPU tier,
tests/test_sec1_cpu.py): every case of both curves in the 33-byte stride and in the mixed packing whose wavefronts all hold 33-byte,
65-byte and refused lengths; the unit operations; the launch geometry with sentinels behind both outputs; offset tables with single
spoiled entries through the _stream form; refused calls, each followed by a good one; a child process whose first call is each _stream
entry; the _stream entries under callers that do not synchronise, with the delay of tests/test_gpu_stream_order.py; the _sec1 verify
entries against the oracle's verdicts and against verify_msgs fed the decoded keys, cold and warm; and the round trips through the
registries and the device's own public keys."""
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import consensus_amd as sbv
import msgs_generic_cases as mg
import sec1_cases as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOTINIT = -2, -5
SENTINEL = 0x3C
N_BIG = 8229
DECODE = {0: sbv.p256_decode_keys, 1: sbv.secp256k1_decode_keys}
DECODE_STREAM = {0: sbv.p256_decode_keys_stream, 1: sbv.secp256k1_decode_keys_stream}
SYMBOL = {0: "sbv_p256_decode_keys", 1: "sbv_secp256k1_decode_keys"}
SEC1_ENTRY = {"p256": sbv.p256_verify_msgs_sec1, "k256": sbv.secp256k1_verify_msgs_sec1}
ENTRY = {"p256": sbv.verify_msgs, "k256": sbv.secp256k1_verify_msgs}
IDS = [c.name for c in cases.CURVES]


@pytest.fixture(scope="module", autouse=True)
def dev():
    sbv.init(0)
    t0 = time.perf_counter()
    yield
    print(f"\ntest_gpu_sec1: {time.perf_counter() - t0:.1f} s of wall time")


def _dev(torch, data, dtype=np.uint8):
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=dtype).copy()).cuda()


def _differ(cv, idx, keys64, ok):
    cs, ex = cases.cases(cv), cases.expected(cv)
    return [(i, cs[i][0]) for k, i in enumerate(idx) if (keys64[64 * k:64 * k + 64], ok[k]) != ex[i]]


def _tiled(cv, n):
    """n keys of the mixed packing, cyclically: (keys, model keys64, model ok)"""
    cs, ex = cases.cases(cv), cases.expected(cv)
    idx = cases.mixed(cv)[0]
    pick = [idx[j % len(idx)] for j in range(n)]
    return [cs[i][1] for i in pick], b"".join(ex[i][0] for i in pick), bytes(ex[i][1] for i in pick)


# ---- every case, both packings ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv", cases.CURVES, ids=IDS)
def test_every_case_in_the_mixed_packing(cv):
    idx, blob, off = cases.mixed(cv)
    assert len(idx) == len(cases.cases(cv)) <= N_BIG
    keys64, ok = DECODE[cv.id](blob, offsets=off)
    bad = _differ(cv, idx, keys64, ok)
    assert not bad, (len(bad), bad[:8])
    assert ok.count(1) >= 900 and ok.count(0) >= 900
    assert all(keys64[64 * k:64 * k + 64] == cases.ZERO64 for k in range(len(idx)) if not ok[k])


@pytest.mark.parametrize("cv", cases.CURVES, ids=IDS)
def test_every_compressed_case_in_the_33_byte_stride(cv):
    idx, blob = cases.stride(cv)
    keys64, ok = DECODE[cv.id](blob)
    bad = _differ(cv, idx, keys64, ok)
    assert not bad, (len(bad), bad[:8])
    assert ok.count(1) >= 600 and ok.count(0) >= 600


@pytest.mark.parametrize("cv", cases.CURVES, ids=IDS)
def test_known_answers(cv):
    g = cases.golden_cases(cv)
    keys64, ok = DECODE[cv.id]([k for _, k, _ in g])
    assert ok == b"\x01" * len(g) and keys64 == b"".join(xy for _, _, xy in g)


# ---- the unit operations -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [0, 1])
@pytest.mark.parametrize("cv", cases.CURVES, ids=IDS)
def test_unit_operations(cv, op):
    ins, want = cases.op_cases(cv, op)
    got = sbv.debug_sec1_op(cv.id, op, ins)
    bad = [i for i in range(len(ins)) if got[i] != want[i]]
    assert not bad, (cv.name, op, len(bad), bad[:8])


# ---- launch geometry ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, N_BIG])
@pytest.mark.parametrize("cv", cases.CURVES, ids=IDS)
def test_launch_geometry_every_byte_and_nothing_behind_m(cv, n):
    import torch
    keys, want64, wantok = _tiled(cv, n)
    blob, off = b"".join(keys), cases.offsets_of(keys)
    d_k = _dev(torch, b"\x00" + blob)[1:]                                  # an odd address for the packed keys
    d_off = _dev(torch, np.array(off, dtype=np.uint64).tobytes(), np.int64)
    d_64 = torch.full((64 * (n + 2),), SENTINEL, dtype=torch.uint8, device="cuda")
    d_ok = torch.full((n + 64 + 3,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    DECODE_STREAM[cv.id](d_k.data_ptr(), d_off.data_ptr(), len(blob), n, d_64.data_ptr(), d_ok.data_ptr() + 3)
    torch.cuda.synchronize()
    assert d_64.cpu().numpy().tobytes() == want64 + bytes([SENTINEL]) * 128, n
    assert d_ok.cpu().numpy().tobytes() == bytes([SENTINEL]) * 3 + wantok + bytes([SENTINEL]) * 64, n
    # ok == NULL: the keys alone
    d_64.fill_(SENTINEL)
    torch.cuda.synchronize()
    DECODE_STREAM[cv.id](d_k.data_ptr(), d_off.data_ptr(), len(blob), n, d_64.data_ptr(), 0)
    torch.cuda.synchronize()
    assert d_64.cpu().numpy().tobytes() == want64 + bytes([SENTINEL]) * 128, n
    # the host-pointer form, with and without ok
    assert DECODE[cv.id](keys) == (want64, wantok)
    assert DECODE[cv.id](keys, want_ok=False) == (want64, None)


@pytest.mark.parametrize("cv", cases.CURVES, ids=IDS)
def test_the_stride_form_refuses_keys_behind_key_bytes(cv):
    """key_bytes covers 100 of 130 keys, the 101st by 32 of its 33 bytes: 30 refused keys, no read behind the buffer's stated size"""
    import torch
    idx, blob = cases.stride(cv)
    n, cover = 130, 100 * 33 + 32
    want64, wantok = cases.decode_packed(cv, blob[:33 * n], None, n, key_bytes=cover, stride33=True)
    assert wantok[100:] == bytes(30) and wantok[:100].count(1) >= 20
    d_k = _dev(torch, blob[:33 * n])
    d_64 = torch.full((64 * n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_ok = torch.full((n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    DECODE_STREAM[cv.id](d_k.data_ptr(), 0, cover, n, d_64.data_ptr(), d_ok.data_ptr())
    torch.cuda.synchronize()
    assert d_64.cpu().numpy().tobytes() == want64 + bytes([SENTINEL]) * 64
    assert d_ok.cpu().numpy().tobytes() == wantok + bytes([SENTINEL]) * 64


# ---- offset tables that fail single lanes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv", cases.CURVES, ids=IDS)
def test_bad_offset_pairs_refuse_their_lanes_and_no_other(cv):
    import torch
    blob, off, spoiled = cases.broken_offsets(cv)
    m = len(off) - 1
    want64, wantok = cases.decode_packed(cv, blob, off, m)
    assert [i for i in range(m) if not wantok[i]] == list(spoiled)          # every key is a valid encoding: the refusals are the offsets'
    d_k, d_off = _dev(torch, blob), _dev(torch, np.array(off, dtype=np.uint64).tobytes(), np.int64)
    d_64 = torch.full((64 * m + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_ok = torch.full((m + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    DECODE_STREAM[cv.id](d_k.data_ptr(), d_off.data_ptr(), len(blob), m, d_64.data_ptr(), d_ok.data_ptr())
    torch.cuda.synchronize()
    assert d_ok.cpu().numpy().tobytes() == wantok + bytes([SENTINEL]) * 64
    assert d_64.cpu().numpy().tobytes() == want64 + bytes([SENTINEL]) * 64
    # the host form refuses such a table as a whole
    lib = sbv.load()
    fn = getattr(lib, SYMBOL[cv.id])
    fn.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p]
    out = ctypes.create_string_buffer(bytes([SENTINEL]) * 64 * m, 64 * m)
    assert fn(blob, (ctypes.c_uint64 * (m + 1))(*off), m, out, None) == EINVAL and out.raw == bytes([SENTINEL]) * 64 * m


# ---- refused calls -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cv", cases.CURVES, ids=IDS)
def test_refused_calls_each_followed_by_a_good_one(cv):
    import torch
    lib = sbv.load()
    V, S, U64P = ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)
    host, stream = getattr(lib, SYMBOL[cv.id]), getattr(lib, SYMBOL[cv.id] + "_stream")
    host.argtypes = [V, U64P, S, V, V]
    stream.argtypes = [V, V, S, S, V, V, V]
    lib.sbv_debug_sec1_op.argtypes = [ctypes.c_int, ctypes.c_int, V, V, S]
    n = 9
    keys, want64, wantok = _tiled(cv, n)
    blob, off = b"".join(keys), cases.offsets_of(keys)
    assert 0 < wantok.count(1) < n
    sent = lambda k: ctypes.create_string_buffer(bytes([SENTINEL]) * k, k)
    buf = lambda x: ctypes.create_string_buffer(x, len(x))
    table = lambda o: (ctypes.c_uint64 * len(o))(*o)
    kb, okb = sent(64 * n), sent(n)

    def good_host():
        k2, o2 = sent(64 * n), sent(n)
        assert host(buf(blob), table(off), n, k2, o2) == 0 and (k2.raw, o2.raw) == (want64, wantok)
    first_not_0, decreasing = list(off), list(off)
    first_not_0[0] = 1
    decreasing[4] = decreasing[3] - 1
    for what, args in [("null keys", (None, table(off), n, kb, okb)), ("null keys64", (buf(blob), table(off), n, None, okb)),
                       ("null keys, stride", (None, None, n, kb, okb)), ("first offset 1", (buf(blob), table(first_not_0), n, kb, okb)),
                       ("offsets decrease", (buf(blob), table(decreasing), n, kb, okb)), ("m = 2^32 + 1", (buf(blob), None, (1 << 32) + 1, kb, okb))]:
        assert host(*args) == EINVAL, what
        assert kb.raw == bytes([SENTINEL]) * 64 * n and okb.raw == bytes([SENTINEL]) * n, what
        good_host()
    assert host(None, None, 0, None, None) == 0                          # m == 0: SBV_OK, nothing read or written
    assert host(buf(blob), table(off), n, kb, None) == 0 and kb.raw == want64 and okb.raw == bytes([SENTINEL]) * n
    # the _stream form: null pointers, the alignment of keys64 (4) and of the offsets (8), m = 2^32 + 1
    t = {k: torch.full((4096,), SENTINEL, dtype=torch.uint8, device="cuda") for k in ("keys", "off", "k64", "ok")}
    t["keys"][:len(blob)] = _dev(torch, blob)
    t["off"][:8 * (n + 1)] = _dev(torch, np.array(off, dtype=np.uint64).tobytes())
    torch.cuda.synchronize()
    p = {k: v.data_ptr() for k, v in t.items()}
    good = [p["keys"], p["off"], len(blob), n, p["k64"], p["ok"], None]

    def good_stream():
        assert stream(*good) == 0
        torch.cuda.synchronize()
        assert t["k64"].cpu().numpy().tobytes()[:64 * n] == want64 and t["ok"].cpu().numpy().tobytes()[:n] == wantok
        t["k64"].fill_(SENTINEL)
        t["ok"].fill_(SENTINEL)
        torch.cuda.synchronize()
    refused = []
    for pos in (0, 4):
        args = list(good)
        args[pos] = None
        refused.append(("null at %d" % pos, args))
    for o in (1, 2, 3):
        args = list(good)
        args[4] += o
        refused.append(("keys64 + %d" % o, args))
    for o in (1, 2, 4):
        args = list(good)
        args[1] += o
        refused.append(("offsets + %d" % o, args))
    args = list(good)
    args[3] = (1 << 32) + 1
    refused.append(("m = 2^32 + 1", args))
    for what, args in refused:
        assert stream(*args) == EINVAL, what
        torch.cuda.synchronize()
        assert bool((t["k64"] == SENTINEL).all()) and bool((t["ok"] == SENTINEL).all()), what
        good_stream()
    args = list(good)
    args[3] = 0
    assert stream(*args) == 0
    # the debug op: ops 0 and 1, curves 0 and 1, at most 65 536 cases
    rec, out = buf(cases.op_record(4)), sent(128)
    for curve, op in ((cv.id, -1), (cv.id, 2), (2, 0), (-1, 1)):
        assert lib.sbv_debug_sec1_op(curve, op, rec, out, 1) == EINVAL, (curve, op)
    assert lib.sbv_debug_sec1_op(cv.id, 0, None, out, 1) == EINVAL and lib.sbv_debug_sec1_op(cv.id, 0, rec, None, 1) == EINVAL
    assert lib.sbv_debug_sec1_op(cv.id, 0, rec, out, 65537) == EINVAL and out.raw == bytes([SENTINEL]) * 128
    assert lib.sbv_debug_sec1_op(cv.id, 0, None, None, 0) == 0
    assert lib.sbv_debug_sec1_op(cv.id, 0, rec, out, 1) == 0 and out.raw == cases.op_answer(cases.be32(cases.sqrt(cv, 4)[0]), True)
    good_host()


# ---- the first call of a process ---------------------------------------------------------------------------------------------------------
_FIRST_CALL = r"""
import ctypes, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import consensus_amd as sbv
symbol, blob = sys.argv[2], bytes.fromhex(sys.argv[3])
off = [int(x) for x in sys.argv[4].split(",")]
m = len(off) - 1
d_k = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
d_off = torch.from_numpy(np.array(off, dtype=np.uint64).view(np.int64)).cuda()
d_64 = torch.full((64 * m,), 7, dtype=torch.uint8, device="cuda")
d_ok = torch.full((m,), 7, dtype=torch.uint8, device="cuda")
lib = sbv.load()
V, S = ctypes.c_void_p, ctypes.c_size_t
fn = getattr(lib, symbol + "_stream")
fn.argtypes = [V, V, S, S, V, V, V]
host = getattr(lib, symbol)
host.argtypes = [V, V, S, V, V]
print("before-init", fn(d_k.data_ptr(), d_off.data_ptr(), len(blob), m, d_64.data_ptr(), d_ok.data_ptr(), None), fn(None, None, 0, 0, None, None, None),
      host(None, None, 0, None, None))
sbv.init(0)
st = torch.cuda.Stream()
torch.cuda.synchronize()
assert fn(d_k.data_ptr(), d_off.data_ptr(), len(blob), m, d_64.data_ptr(), d_ok.data_ptr(), st.cuda_stream) == 0
torch.cuda.synchronize()
print("keys", d_64.cpu().numpy().tobytes().hex())
print("ok", d_ok.cpu().numpy().tobytes().hex())
"""


@pytest.mark.parametrize("cv", cases.CURVES, ids=IDS)
def test_first_call_of_a_process_is_the_stream_entry(cv):
    """nothing of the library has run on the device before the _stream entry; before sbv_init the entries answer SBV_ENOTINIT"""
    keys, want64, wantok = _tiled(cv, 200)
    r = subprocess.run([sys.executable, "-c", _FIRST_CALL, ROOT, SYMBOL[cv.id], b"".join(keys).hex(), ",".join(map(str, cases.offsets_of(keys)))],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(ln.split(" ", 1) for ln in r.stdout.splitlines() if ln.startswith(("before-init", "keys", "ok")))
    assert lines["before-init"] == " ".join(["%d" % ENOTINIT] * 3)
    assert bytes.fromhex(lines["keys"]) == want64 and bytes.fromhex(lines["ok"]) == wantok


# ---- the _stream entries under callers that do not synchronise ---------------------------------------------------------------------------
@pytest.fixture(scope="module", params=cases.CURVES, ids=IDS)
def streams(request):
    import torch
    from test_gpu_stream_order import DELAY_FACTOR, DELAY_MAX_MS, DELAY_MIN_MS, Delay
    cv = request.param

    class S:
        pass
    s = S()
    s.torch = torch
    s.want, s.src = {}, {}
    # two generations of one size: the compressed cases in the stride's order, and the same rotated, so that every lane's answer differs
    idx, blob = cases.stride(cv)
    m = len(idx)
    reps = N_BIG // m + 1
    for g, shift in (("x", 0), ("y", 401)):
        order = [idx[(j + shift) % m] for j in range(N_BIG)]
        ex = cases.expected(cv)
        s.want[g] = (b"".join(ex[i][0] for i in order), bytes(ex[i][1] for i in order))
        s.src[g] = _dev(torch, ((blob * (reps + 1))[33 * shift:])[:33 * N_BIG])
    assert s.want["x"] != s.want["y"]
    s.buf = torch.empty_like(s.src["x"])
    s.outs = [(torch.full((64 * N_BIG,), SENTINEL, dtype=torch.uint8, device="cuda"), torch.full((N_BIG,), SENTINEL, dtype=torch.uint8, device="cuda")) for _ in range(3)]
    s.hosts = [(torch.zeros(64 * N_BIG, dtype=torch.uint8).pin_memory(), torch.zeros(N_BIG, dtype=torch.uint8).pin_memory()) for _ in range(3)]
    s.stream = torch.cuda.Stream()
    torch.cuda.synchronize()

    def produce(g):
        s.buf.copy_(s.src[g], non_blocking=True)

    def call(k):
        DECODE_STREAM[cv.id](s.buf.data_ptr(), 0, 33 * N_BIG, N_BIG, s.outs[k][0].data_ptr(), s.outs[k][1].data_ptr(), stream=s.stream.cuda_stream)
        for h, o in zip(s.hosts[k], s.outs[k]):
            h.copy_(o, non_blocking=True)

    def check(k, g, what):
        got = tuple(h.numpy().tobytes() for h in s.hosts[k])
        if got != s.want[g]:
            other = s.want["x" if g == "y" else "y"]
            raise AssertionError("%s: output %d is not generation %s's but %s" % (what, k, g.upper(), "the OTHER generation's" if got == other else "a mixture"))
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
    print("\n[sec1 %s, stream order] one warm call of %d: %.3f ms; delay %.1f ms" % (cv.name, N_BIG, ms, s.delay_ms))
    return s


def _held_back(s):
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
        pending = not gate.query()
    torch.cuda.synchronize()
    assert pending, "the delay had run out before the last enqueue: the schedule proved nothing"
    s.check(1, "y", "early overwriter" if overwrite else "late producer")
    if overwrite:
        assert torch.equal(s.buf, s.src["x"])


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


# ---- the _sec1 verify entries -------------------------------------------------------------------------------------------------------------
def _verify_check(scheme, vcs, what):
    """one call of the _sec1 entry: equals want, and equals verify_msgs fed the keys decode_keys writes (which equal the model's)"""
    cv = cases.BY_NAME[scheme]
    n = len(vcs)
    msgs, sigs, keys = [c.msg for c in vcs], [c.sig for c in vcs], [c.key for c in vcs]
    got = sbv.bitmap_to_list(SEC1_ENTRY[scheme](msgs, sigs, keys), n)
    assert got == [c.want for c in vcs], (scheme, what, [c.name for c, g in zip(vcs, got) if g != c.want][:12])
    keys64, _ = DECODE[cv.id](keys)
    assert keys64 == b"".join(c.key64 for c in vcs)
    ref = sbv.bitmap_to_list(ENTRY[scheme](msgs, sigs, keys64), n)
    assert got == ref, (scheme, what, [c.name for c, g, r in zip(vcs, got, ref) if g != r][:12])
    return got


@pytest.mark.parametrize("scheme", mg.SCHEMES)
def test_verify_msgs_sec1_on_every_generic_case(scheme):
    """the ladder, families b-e, the key cases and the empty messages of tests/msgs_generic_cases.py, keys re-encoded"""
    fams = mg.families(scheme)
    pool = mg.ladder(scheme)[0] + [c for f in "bcde" for c in fams[f]] + mg.key_cases(scheme) + mg.empty_batch(scheme)
    vcs = cases.verify_cases(scheme, pool)
    got = _verify_check(scheme, vcs, "every case")
    refused = [i for i, c in enumerate(vcs) if c.key64 == cases.ZERO64]
    assert len(refused) >= len(vcs) // 8 and not any(got[i] for i in refused) and got.count(True) >= 100
    # compressed keys alone, as one m x 33 array: the stride form of the entry
    comp = [c for c in vcs if len(c.key) == 33][:300]
    bits = sbv.bitmap_to_list(SEC1_ENTRY[scheme]([c.msg for c in comp], [c.sig for c in comp], b"".join(c.key for c in comp)), len(comp))
    assert bits == [c.want for c in comp]
    for n in (1, 63, 65, 257):
        _verify_check(scheme, vcs[5:5 + n], "n = %d" % n)


@pytest.mark.parametrize("scheme", mg.SCHEMES)
def test_verify_msgs_sec1_long_tailed_signers_cold_then_warm(scheme):
    """8 229 signatures under the long-tailed signer layout, keys decoded per signature in front of the grouped step: cold (the
    key-table cache emptied by a restart of the library) and again with the cache warm"""
    vcs = cases.verify_cases(scheme, mg.long_tail(scheme))
    assert len(vcs) == N_BIG
    sbv.shutdown()
    sbv.init(0)
    msgs, sigs, keys = [c.msg for c in vcs], [c.sig for c in vcs], [c.key for c in vcs]
    want = [c.want for c in vcs]
    assert want.count(True) > 5000 and want.count(False) > 2000
    for run in ("cold", "warm"):
        got = sbv.bitmap_to_list(SEC1_ENTRY[scheme](msgs, sigs, keys), N_BIG)
        assert got == want, (scheme, run, [i for i, (g, w) in enumerate(zip(got, want)) if g != w][:12])
    keys64, _ = DECODE[cases.BY_NAME[scheme].id](keys)
    assert sbv.bitmap_to_list(ENTRY[scheme](msgs, sigs, keys64), N_BIG) == want


@pytest.mark.parametrize("scheme", mg.SCHEMES)
def test_verify_msgs_sec1_refused_calls(scheme):
    lib = sbv.load()
    fn = getattr(lib, "sbv_p256_verify_msgs_sec1" if scheme == "p256" else "sbv_secp256k1_verify_msgs_sec1")
    C, U64P = ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)
    fn.argtypes = [C, U64P, C, U64P, C, U64P, ctypes.c_size_t, ctypes.c_void_p]
    vcs = cases.verify_cases(scheme, mg.key_cases(scheme) + mg.filler(scheme)[:9])
    n = len(vcs)
    table = lambda parts: (ctypes.c_uint64 * (len(parts) + 1))(*cases.offsets_of(parts))
    msgs, sigs, keys = [c.msg for c in vcs], [c.sig for c in vcs], [c.key for c in vcs]
    mb, sb, kb = b"".join(msgs), b"".join(sigs), b"".join(keys)
    mo, so, ko = table(msgs), table(sigs), table(keys)
    out = ctypes.create_string_buffer((n + 7) // 8)
    bad_first, dec = table(keys), table(keys)
    bad_first[0] = 1
    dec[3] = dec[2] - 1
    one = (ctypes.c_uint64 * 1)(0)
    for what, args in [("null keys", (mb, mo, sb, so, None, ko, n, out)), ("null bitmap", (mb, mo, sb, so, kb, ko, n, None)),
                       ("null msg_offsets", (mb, None, sb, so, kb, ko, n, out)), ("first key offset 1", (mb, mo, sb, so, kb, bad_first, n, out)),
                       ("key offsets decrease", (mb, mo, sb, so, kb, dec, n, out)),
                       ("n = 2^21 + 1", (b"\0", one, b"\0", one, b"\0" * 33, None, (1 << 21) + 1, ctypes.create_string_buffer(1)))]:
        assert fn(*args) == EINVAL, what
        _verify_check(scheme, vcs, "behind: " + what)
    assert fn(None, None, None, None, None, None, 0, None) == 0


# ---- the host layer ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", mg.SCHEMES)
def test_host_verifier_decodes_and_verifies_on_the_gpu_backend(scheme):
    """Verifier::DecodeKeys and VerifyMsgsSec1: one device call each on the GPU backend"""
    import hostlib
    cv = cases.BY_NAME[scheme]
    host = hostlib.load()
    C, S, U64P = ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)
    host.sbvh_decode_keys.argtypes = [hostlib.V, C, U64P, S, C, C]
    host.sbvh_verify_msgs_sec1.argtypes = [hostlib.V, C, U64P, C, U64P, C, U64P, S, C]
    cb = hostlib.BACKEND_FN(lambda tuples, n, bitmap, user: 0)
    fams = mg.families(scheme)
    vcs = cases.verify_cases(scheme, [c for f in "bcde" for c in fams[f]] + mg.key_cases(scheme) + mg.filler(scheme)[:40])
    n = len(vcs)
    table = lambda parts: (ctypes.c_uint64 * (len(parts) + 1))(*cases.offsets_of(parts))
    msgs, sigs, keys = [c.msg for c in vcs], [c.sig for c in vcs], [c.key for c in vcs]
    h = host.sbvh_verifier_new_scheme(0 if scheme == "p256" else 2, 0, 0, cb, None, 64, 50, 0)
    try:
        idx, blob, off = cases.mixed(cv)
        m = len(idx)
        keys64, ok = ctypes.create_string_buffer(64 * m), ctypes.create_string_buffer(m)
        assert host.sbvh_decode_keys(h, blob, (ctypes.c_uint64 * (m + 1))(*off), m, keys64, ok) == hostlib.OK
        assert not _differ(cv, idx, keys64.raw, ok.raw)
        out = ctypes.create_string_buffer((n + 7) // 8)
        assert host.sbvh_verify_msgs_sec1(h, b"".join(msgs), table(msgs), b"".join(sigs), table(sigs), b"".join(keys), table(keys), n, out) == hostlib.OK
        assert sbv.bitmap_to_list(out.raw, n) == [c.want for c in vcs]
    finally:
        host.sbvh_verifier_free(h)


# ---- round trips ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", mg.SCHEMES)
def test_decode_then_register_then_verify_keyed(scheme):
    """compressed keys -> decode_keys -> register_keys -> verify_msgs_keyed: the route for signers that repeat"""
    cv = cases.BY_NAME[scheme]
    point = lambda c: cases.on_curve(cv, int.from_bytes(c.key[:32], "big"), int.from_bytes(c.key[32:], "big"))
    fill = mg.filler(scheme)[:40] + [c for c in mg.families(scheme)["d"] if not c.want and point(c)][:10]
    assert len(fill) == 50
    signers = sorted({c.key for c in fill})
    keys64, ok = DECODE[cv.id](b"".join(cases.compress(k) for k in signers))
    assert ok == b"\x01" * len(signers) and keys64 == b"".join(signers)
    clear, register, keyed = ((sbv.clear_keys, sbv.register_keys, sbv.verify_msgs_keyed) if scheme == "p256" else
                              (sbv.secp256k1_clear_keys, sbv.secp256k1_register_keys, sbv.secp256k1_verify_msgs_keyed))
    clear()
    try:
        slots = register([keys64[64 * i:64 * i + 64] for i in range(len(signers))])
        slot_of = dict(zip(signers, slots))
        got = sbv.bitmap_to_list(keyed([c.msg for c in fill], [c.sig for c in fill], [slot_of[c.key] for c in fill]), len(fill))
        assert got == [c.want for c in fill] and got.count(True) == 40
    finally:
        clear()


def test_device_public_keys_compressed_in_python_decode_to_themselves():
    n = 1000
    ds = b"".join(cases.be32(int.from_bytes(b"sec1 round trip %d" % i, "big") + 1) for i in range(n))
    pubs, pok = sbv.secp256k1_pubkeys(ds)
    assert pok == b"\x01" * n
    comp = b"".join(cases.compress(pubs[64 * i:64 * i + 64]) for i in range(n))
    assert {comp[33 * i] for i in range(n)} == {2, 3}
    assert sbv.secp256k1_decode_keys(comp) == (pubs, b"\x01" * n)
    assert sbv.secp256k1_decode_keys([b"\x04" + pubs[64 * i:64 * i + 64] for i in range(n)]) == (pubs, b"\x01" * n)
