"""GPU tier of the raw-message ECDSA signers (include/sbv.h: sbv_sha256_msgs, sbv_p256_sign_msgs, sbv_secp256k1_sign_msgs, their
_stream forms and sbv_debug_ecdsa_der_op; consensus_amd/csrc/ecdsa_sign_msgs_kernels.hip).

The kernels are held byte for byte to the model of tests/ecdsa_sign_msgs_cases.py (Python integers, hashlib, hmac) on every case, and
to the emulator of the CPU tier (tests/emul/ecdsa_sign_msgs_emul.cc: the same lanes under g++) where a batch is too large for the
model.  No batch exceeds 8 229 items."""
import ctypes
import hashlib
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import consensus_amd as sbv
import ecdsa_sign_msgs_cases as cases
import frontend_cases as fc
import hostlib
from test_ecdsa_sign_msgs_cpu import case_keys, emul, sign_msgs  # noqa: F401  (emul is a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOTINIT = -2, -5
N, NK = cases.LARGE, 64
SIGNERS = {"p256": sbv.p256_sign_msgs, "k256": sbv.secp256k1_sign_msgs}
VERIFIERS = {"p256": sbv.verify_msgs, "k256": sbv.secp256k1_verify_msgs}


@pytest.fixture(scope="module", autouse=True)
def _init():
    sbv.init(0)
    yield


def keys_of(count, tag):
    return b"".join(cases.be32(int.from_bytes(hashlib.sha256(tag + b"%d" % i).digest(), "big") % (cases.kc.N - 1) + 1) for i in range(count))


def messages(n, seed):
    """n messages with lengths from the hash list's short end and a few long ones, seeded"""
    rng = random.Random(seed)
    pool = rng.randbytes(8192)
    out = []
    for i in range(n):
        ln = rng.choice((0, 1, 3, 55, 56, 63, 64, 65, 119, 120, 200)) if i % 7 else rng.randrange(261)
        at = rng.randrange(len(pool) - ln)
        out.append(pool[at:at + ln])
    return out


def split(sigs, soff):
    return [sigs[soff[i]:soff[i + 1]] for i in range(len(soff) - 1)]


def packed(recs, lens):
    return [r[:n] for r, n in zip(recs, lens)]


# ---- DER and low-S through the debug entry ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", cases.CURVES)
def test_every_der_case_on_the_device(curve):
    cs = cases.der_cases()
    got = sbv.debug_ecdsa_der_op(cases.CURVE_ID[curve], [cases.be32(r) + cases.be32(s) for r, s, _ in cs])
    for (r, s, der), (rec, ln) in zip(cs, got):
        assert ln == len(der) and rec == der + bytes(72 - ln), (r, s)


@pytest.mark.parametrize("curve", cases.CURVES)
def test_low_s_cases_on_the_device(curve):
    ss = cases.low_s_cases(curve)
    got = sbv.debug_ecdsa_der_op(cases.CURVE_ID[curve], [cases.be32(9) + cases.be32(s) for s in ss], low_s=True)
    plain = sbv.debug_ecdsa_der_op(cases.CURVE_ID[curve], [cases.be32(9) + cases.be32(s) for s in ss])
    for s, (rec, ln), (prec, pln) in zip(ss, got, plain):
        want = cases.der_model(9, cases.low_s_model(curve, s)[0])
        assert rec == want + bytes(72 - len(want)) and ln == len(want), s
        assert prec[:pln] == cases.der_model(9, s), s


# ---- the hash kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shuffled", [False, True], ids=["ascending", "shuffled"])
def test_every_hash_case_at_every_alignment(shuffled):
    msgs, starts = cases.pack_at_alignments(cases.hash_messages(), shuffled)
    assert {(len(m), a) for m in cases.hash_messages() for a in range(4)} <= {(len(m), s % 4) for m, s in zip(msgs, starts)}
    assert len(msgs) <= cases.LARGE
    assert sbv.sha256_msgs(msgs) == [hashlib.sha256(m).digest() for m in msgs]


# ---- the signing cases through the host forms ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("low_s", [False, True], ids=["flags0", "low_s"])
@pytest.mark.parametrize("curve", cases.CURVES)
def test_signing_cases_equal_the_model(curve, low_s):
    cs = cases.sign_cases(curve)
    want = cases.expected(curve, low_s)
    out = SIGNERS[curve](case_keys(curve), [c.msg for c in cs], low_s=low_s)
    sigs, soff, ok = out[0], out[1], out[-1]
    assert soff[0] == 0 and len(soff) == len(cs) + 1 and len(sigs) == soff[-1]
    assert split(sigs, soff) == [w[0] for w in want] and ok == bytes(w[2] for w in want)
    if curve == "k256":
        assert out[2] == bytes(w[1] for w in want)
    known = cases.known_answers(curve)
    if curve == "p256" and not low_s or curve == "k256" and low_s:
        for i, c in enumerate(cs):
            if c.name in known:
                assert fc.strict_rs(sigs[soff[i]:soff[i + 1]]) == cases.be32(known[c.name][0]) + cases.be32(known[c.name][1]), c.name
    # an index out of range, between honest neighbours
    idx = list(range(len(cs)))
    idx[5], idx[200] = len(cs), 0xFFFFFFFF
    out = SIGNERS[curve](case_keys(curve), [c.msg for c in cs], key_index=idx, low_s=low_s)
    got = split(out[0], out[1])
    assert got[5] == got[200] == b"" and out[-1][5] == out[-1][200] == 0
    assert [g for i, g in enumerate(got) if i not in (5, 200)] == [w[0] for i, w in enumerate(want) if i not in (5, 200)]
    if curve == "k256":
        assert out[2][5] == out[2][200] == 0


# ---- launch geometry with sentinels, through the _stream forms ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def large(emul):
    """8 229 messages under 64 keys with a seeded index, and what the emulator signs for them: {(curve, flags): (records, lens, recid, ok)}"""
    class L:
        pass
    g = L()
    g.keys = keys_of(NK, b"ecdsa-sign-msgs-large")
    g.msgs = messages(N, 0x8229)
    rng = random.Random(0x1D)
    g.index = [rng.randrange(NK) for _ in range(N)]
    g.want = {(c, f): sign_msgs(emul, c, g.keys, g.msgs, key_index=g.index, flags=f) for c in cases.CURVES for f in (0, cases.LOW_S)}
    return g


def stream_call(torch, curve, keys, nk, index, blob, offs, n, low_s, stream=0):
    """one _stream call on fresh buffers with sentinels behind every output and the workspace: (records, lens, recid, ok) as bytes"""
    SENT = 0x3C
    dev = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()            # noqa: E731
    d_keys, d_msgs = dev(keys), dev(blob + b"\0")
    d_off = torch.from_numpy(np.array(offs, dtype=np.uint64).view(np.int64)).cuda()
    d_idx = None if index is None else torch.from_numpy(np.array(index, dtype=np.uint32).view(np.int32)).cuda()
    work = sbv.ecdsa_sign_msgs_workspace(n)
    assert work == 96 * n
    d_rec, d_len, d_rid, d_ok, d_work = (torch.full((size + 64,), SENT, dtype=torch.uint8, device="cuda") for size in (72 * n, n, n, n, work))
    args = (d_keys.data_ptr(), nk, 0 if d_idx is None else d_idx.data_ptr(), d_msgs.data_ptr(), d_off.data_ptr(), n, d_rec.data_ptr(), d_len.data_ptr())
    if curve == "p256":
        sbv.p256_sign_msgs_stream(*args, d_ok.data_ptr(), d_work.data_ptr(), low_s=low_s, stream=stream)
    else:
        sbv.secp256k1_sign_msgs_stream(*args, d_rid.data_ptr(), d_ok.data_ptr(), d_work.data_ptr(), low_s=low_s, stream=stream)
    torch.cuda.synchronize()
    out = []
    for t, size in ((d_rec, 72 * n), (d_len, n), (d_rid, n), (d_ok, n), (d_work, work)):
        b = t.cpu().numpy().tobytes()
        assert b[size:] == bytes([SENT]) * 64, "a sentinel behind an output was overwritten"
        out.append(b[:size])
    if curve == "p256":
        assert out[2] == bytes([SENT]) * n          # no recid array in the P-256 form: nothing wrote there
    return out[0], out[1], out[2], out[3]


@pytest.mark.parametrize("n", cases.GEOMETRY)
@pytest.mark.parametrize("curve", cases.CURVES)
def test_launch_geometry_with_sentinels(curve, n, large, emul):
    import torch
    low = n % 2 == 1                                  # both flag settings across the sizes
    msgs = large.msgs[:n]
    index = large.index[:n] if n > 64 else None       # the null index at the small sizes: key i % n_keys
    want = large.want[curve, cases.LOW_S if low else 0]
    if index is None:
        want = sign_msgs(emul, curve, large.keys, msgs, flags=cases.LOW_S if low else 0)
    rec, lens, rid, ok = stream_call(torch, curve, large.keys, NK, index, b"".join(msgs), cases.offsets_of(msgs), n, low)
    assert ok == bytes(want[3][:n]) == b"\x01" * n and lens == bytes(want[1][:n])
    for i in range(n):
        assert rec[72 * i:72 * i + 72] == want[0][i], i
        assert rec[72 * i + lens[i]:72 * i + 72] == bytes(72 - lens[i]), i                    # zero behind len
    if curve == "k256":
        assert rid == bytes(want[2][:n])


def test_stream_form_refuses_a_decreasing_pair_per_lane(large, emul):
    import torch
    n = 70
    msgs = large.msgs[:n]
    offs = cases.offsets_of(msgs)
    at = next(i for i in range(3, n - 3) if len(msgs[i - 1]) > 1 and len(msgs[i]) > 1)
    bent = list(offs)
    bent[at] = offs[at - 1] - 1 if offs[at - 1] else offs[at + 1] + 1
    bad = [i for i in range(n) if bent[i] > bent[i + 1]]
    assert bad and len(bad) <= 2
    for curve in cases.CURVES:
        rec, lens, rid, ok = stream_call(torch, curve, large.keys, NK, large.index[:n], b"".join(msgs), bent, n, False)
        want = sign_msgs(emul, curve, large.keys, b"".join(msgs), key_index=large.index[:n], offsets=bent, mbytes=2 ** 64 - 1)
        assert ok == bytes(want[3]) and lens == bytes(want[1]) and rec == b"".join(want[0])
        for i in bad:
            assert ok[i] == 0 and lens[i] == 0 and rec[72 * i:72 * i + 72] == bytes(72)
        assert sum(ok) == n - len(bad)
        if curve == "k256":
            assert rid == bytes(want[2]) and all(rid[i] == 0 for i in bad)
    # and the hash entry's _stream form gives such a lane the digest of the empty message
    d_msgs = torch.from_numpy(np.frombuffer(b"".join(msgs) + b"\0", dtype=np.uint8).copy()).cuda()
    d_off = torch.from_numpy(np.array(bent, dtype=np.uint64).view(np.int64)).cuda()
    d_dig = torch.zeros(32 * n + 32, dtype=torch.uint8, device="cuda")
    sbv.sha256_msgs_stream(d_msgs.data_ptr(), d_off.data_ptr(), n, d_dig.data_ptr())
    torch.cuda.synchronize()
    got = d_dig.cpu().numpy().tobytes()
    blob = b"".join(msgs)
    assert got[32 * n:] == bytes(32)
    for i in range(n):
        m = b"" if i in bad else blob[bent[i]:bent[i + 1]]
        assert got[32 * i:32 * i + 32] == hashlib.sha256(m).digest(), i


# ---- refused calls, each followed by a good call ------------------------------------------------------------------------------------
def test_refused_calls_write_nothing_and_the_next_call_signs():
    import torch
    lib = sbv.load()
    C, V, U32, S = ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t
    U64P = ctypes.POINTER(ctypes.c_uint64)
    lib.sbv_p256_sign_msgs.argtypes = [C, U32, V, C, U64P, S, U32, C, U64P, C]
    lib.sbv_secp256k1_sign_msgs.argtypes = [C, U32, V, C, U64P, S, U32, C, U64P, C, C]
    lib.sbv_sha256_msgs.argtypes = [C, U64P, S, C]
    lib.sbv_p256_sign_msgs_stream.argtypes = [V, U32, V, V, V, S, U32, V, V, V, V, V]
    lib.sbv_secp256k1_sign_msgs_stream.argtypes = [V, U32, V, V, V, S, U32, V, V, V, V, V, V]
    lib.sbv_sha256_msgs_stream.argtypes = [V, V, S, V, V]
    lib.sbv_debug_ecdsa_der_op.argtypes = [ctypes.c_int, U32, C, C, C, S]
    key, msgs = cases.be32(0x1234567), [b"one", b"", b"three"]
    blob, n = b"".join(msgs), 3
    good = (ctypes.c_uint64 * 4)(*cases.offsets_of(msgs))
    want = {c: SIGNERS[c](key, msgs) for c in cases.CURVES}
    FILL = b"\xa7"

    def fresh():
        return ctypes.create_string_buffer(FILL * 216, 216), (ctypes.c_uint64 * 4)(*([0xA7A7] * 4)), ctypes.create_string_buffer(FILL * 3, 3), ctypes.create_string_buffer(FILL * 3, 3)

    def untouched(sigs, soff, rid, ok):
        return sigs.raw == FILL * 216 and list(soff) == [0xA7A7] * 4 and rid.raw == FILL * 3 and ok.raw == FILL * 3

    def host(curve, keys=key, nk=1, m=blob, off=good, count=n, flags=0, drop=None):
        sigs, soff, rid, ok = fresh()
        a = [keys, nk, None, m, off, count, flags, sigs, soff] + ([rid, ok] if curve == "k256" else [ok])
        if drop is not None:
            a[drop] = None
        rc = getattr(lib, "sbv_%s_sign_msgs" % ("p256" if curve == "p256" else "secp256k1"))(*a)
        return rc, untouched(sigs, soff, rid, ok)

    for curve in cases.CURVES:
        nonzero = (ctypes.c_uint64 * 4)(1, 3, 3, 8)
        decreasing = (ctypes.c_uint64 * 4)(0, 3, 2, 8)
        refusals = [dict(drop=0), dict(drop=4), dict(drop=7), dict(drop=8), dict(drop=10 if curve == "k256" else 9), dict(nk=0),
                    dict(flags=2), dict(flags=0x80000001), dict(count=(1 << 21) + 1), dict(off=nonzero), dict(off=decreasing), dict(drop=3)]
        for r in refusals:
            assert host(curve, **r) == (EINVAL, True), (curve, r)
            assert SIGNERS[curve](key, msgs) == want[curve], (curve, r)                        # the next call signs
        assert host(curve, count=0) == (0, True)                                              # n == 0: SBV_OK, nothing written
        empties = SIGNERS[curve](key, None, offsets=[0, 0, 0])                                # msgs may be null when every message is empty
        assert empties[-1] == b"\x01\x01" and split(empties[0], empties[1]) == [SIGNERS[curve](key, [b""])[0]] * 2

    dig = ctypes.create_string_buffer(FILL * 96, 96)
    for a in ((blob, None, n, dig), (blob, good, n, None), (None, good, n, dig), (blob, good, (1 << 21) + 1, dig),
              (blob, (ctypes.c_uint64 * 4)(1, 3, 3, 8), n, dig), (blob, (ctypes.c_uint64 * 4)(0, 3, 2, 8), n, dig)):
        assert lib.sbv_sha256_msgs(*a) == EINVAL and dig.raw == FILL * 96, a
        assert sbv.sha256_msgs(msgs) == [hashlib.sha256(m).digest() for m in msgs]
    assert lib.sbv_sha256_msgs(blob, good, 0, dig) == 0 and dig.raw == FILL * 96

    # the _stream forms: null and misaligned device pointers, flags, sizes
    buf = torch.full((4096,), 0xA7, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    assert p % 8 == 0
    d_off = torch.from_numpy(np.array(cases.offsets_of(msgs), dtype=np.uint64).view(np.int64)).cuda()
    d_key = torch.from_numpy(np.frombuffer(key, dtype=np.uint8).copy()).cuda()
    d_msg = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    for curve in cases.CURVES:
        k = curve == "k256"
        base = [d_key.data_ptr(), 1, None, d_msg.data_ptr(), d_off.data_ptr(), n, 0, p, p + 1024] + ([p + 1100] if k else []) + [p + 1200, p + 2048, None]
        fn = lib.sbv_secp256k1_sign_msgs_stream if k else lib.sbv_p256_sign_msgs_stream
        nrec, nlen, nok, nwork = 7, 8, 10 if k else 9, 11 if k else 10
        bends = [(0, None), (4, None), (nrec, None), (nlen, None), (nok, None), (nwork, None), (1, 0), (6, 2), (5, (1 << 21) + 1),
                 (0, d_key.data_ptr() + 1), (2, p + 2), (nrec, p + 2), (nwork, p + 2049), (4, d_off.data_ptr() + 4)]
        for at, value in bends:
            a = list(base)
            a[at] = value
            assert fn(*a) == EINVAL, (curve, at, value)
            torch.cuda.synchronize()
            assert bool((buf == 0xA7).all()), (curve, at, value)
        a = list(base)
        a[5] = 0
        assert fn(*a) == 0
        assert fn(*base) == 0                                                                 # a good call signs, the message pointer at any address
        torch.cuda.synchronize()
        got = buf.cpu().numpy().tobytes()
        lens = got[1024:1024 + n]
        assert got[1200:1200 + n] == b"\x01" * n
        assert b"".join(got[72 * i:72 * i + lens[i]] for i in range(n)) == want[curve][0]
        buf.fill_(0xA7)
    for at, value in ((1, None), (3, None), (1, d_off.data_ptr() + 4), (3, p + 2), (2, (1 << 21) + 1)):
        a = [d_msg.data_ptr(), d_off.data_ptr(), n, p, None]
        a[at] = value
        assert lib.sbv_sha256_msgs_stream(*a) == EINVAL, (at, value)
    for a in ((2, 0, bytes(64)), (0, 2, bytes(64)), (0, 0, None)):
        assert lib.sbv_debug_ecdsa_der_op(a[0], a[1], a[2], ctypes.create_string_buffer(72), ctypes.create_string_buffer(1), 1) == EINVAL


# ---- a process whose first library call after sbv_init is a _stream signer ----------------------------------------------------------
_FIRST_CALL = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import consensus_amd as sbv
curve, keys, blob = sys.argv[2], bytes.fromhex(sys.argv[3]), bytes.fromhex(sys.argv[4])
offs = [int(x) for x in sys.argv[5].split(",")]
n, nk = len(offs) - 1, len(keys) // 32
dev = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()
d_keys, d_msgs = dev(keys), dev(blob)
d_off = torch.from_numpy(np.array(offs, dtype=np.uint64).view(np.int64)).cuda()
d_out = torch.zeros(75 * n, dtype=torch.uint8, device="cuda")
d_work = torch.zeros(96 * n, dtype=torch.uint8, device="cuda")
o = d_out.data_ptr()
def call():
    if curve == "p256":
        sbv.p256_sign_msgs_stream(d_keys.data_ptr(), nk, 0, d_msgs.data_ptr(), d_off.data_ptr(), n, o, o + 72 * n, o + 74 * n, d_work.data_ptr(), low_s=True, stream=st)
    else:
        sbv.secp256k1_sign_msgs_stream(d_keys.data_ptr(), nk, 0, d_msgs.data_ptr(), d_off.data_ptr(), n, o, o + 72 * n, o + 73 * n, o + 74 * n, d_work.data_ptr(), low_s=True, stream=st)
st = 0
try:
    call()
    print("before-init none")
except sbv.SbvError as e:
    print("before-init", e.code)
sbv.init(0)
s = torch.cuda.Stream()
st = s.cuda_stream
torch.cuda.synchronize()
call()
torch.cuda.synchronize()
print("out", d_out.cpu().numpy().tobytes().hex())
"""


@pytest.mark.parametrize("curve", cases.CURVES)
def test_first_call_of_a_process_is_the_stream_signer(curve, emul):
    """nothing has uploaded a comb of G or run any other entry before the _stream signer; before sbv_init it answers SBV_ENOTINIT"""
    n, nk = 300, 7
    keys, msgs = keys_of(nk, b"first-call-" + curve.encode()), messages(n, 0xF157)
    offs = cases.offsets_of(msgs)
    r = subprocess.run([sys.executable, "-c", _FIRST_CALL, ROOT, curve, keys.hex(), (b"".join(msgs) + b"\0").hex(), ",".join(map(str, offs))],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(ln.split(" ", 1) for ln in r.stdout.splitlines() if ln.startswith(("before-init", "out")))
    assert lines["before-init"] == str(ENOTINIT)
    recs, lens, rid, ok = sign_msgs(emul, curve, keys, msgs, flags=cases.LOW_S)
    want = b"".join(recs) + bytes(lens) + (bytes(rid) if curve == "k256" else bytes(n)) + bytes(ok)
    assert bytes.fromhex(lines["out"]) == want


# ---- the _stream entries under callers that do not synchronise ----------------------------------------------------------------------
class _Gen:
    """one generation of inputs — keys, messages (packed), offsets — and what the emulator makes of them"""

    def __init__(self, lib, tag, index):
        self.keys = keys_of(NK, b"ecdsa-sign-msgs-stream-" + tag)
        self.msgs = messages(N, 0x57 + tag[0])
        blob = b"".join(self.msgs)
        self.arrays = [np.frombuffer(self.keys, dtype=np.uint8), np.frombuffer(blob + b"\0", dtype=np.uint8),
                       np.array(cases.offsets_of(self.msgs), dtype=np.uint64).view(np.int64)]
        self.want = _pad(b"".join(hashlib.sha256(m).digest() for m in self.msgs))
        for curve, flags in (("p256", cases.LOW_S), ("k256", 0)):
            recs, lens, rid, ok = sign_msgs(lib, curve, self.keys, self.msgs, key_index=index, flags=flags)
            self.want += _pad(b"".join(recs) + bytes(lens) + (bytes(rid) if curve == "k256" else b"") + bytes(ok))
        assert len(self.want) == OUT_BYTES


def _pad(b):
    """a section of the output buffer, filled up to a multiple of 8 bytes with the buffer's fill (nothing writes there)"""
    return b + b"\x3c" * (-len(b) % 8)


def _up8(v):
    return (v + 7) & ~7


P_AT = _up8(32 * N)                      # the P-256 section of an output buffer: records, lengths, ok
K_AT = P_AT + _up8(74 * N)               # the secp256k1 section: records, lengths, recid, ok
OUT_BYTES = K_AT + _up8(75 * N)


@pytest.fixture(scope="module")
def streams(emul):
    import torch
    from test_gpu_stream_order import DELAY_FACTOR, DELAY_MAX_MS, DELAY_MIN_MS, Delay

    class S:
        pass
    s = S()
    s.torch = torch
    rng = random.Random(0x8229)
    s.index = [rng.randrange(NK) for _ in range(N)]
    s.gen = {"x": _Gen(emul, b"x", s.index), "y": _Gen(emul, b"y", s.index)}
    s.src = {g: [torch.from_numpy(a.copy()).cuda() for a in s.gen[g].arrays] for g in "xy"}
    size = max(s.src["x"][1].numel(), s.src["y"][1].numel())
    s.bufs = [torch.empty_like(s.src["x"][0]), torch.zeros(size, dtype=torch.uint8, device="cuda"), torch.empty_like(s.src["x"][2])]
    s.d_index = torch.from_numpy(np.array(s.index, dtype=np.uint32).view(np.int32)).cuda()
    s.outs = [torch.full((OUT_BYTES,), 0x3C, dtype=torch.uint8, device="cuda") for _ in range(3)]
    s.work = [torch.empty(2 * 96 * N, dtype=torch.uint8, device="cuda") for _ in range(3)]
    s.hosts = [torch.zeros(OUT_BYTES, dtype=torch.uint8).pin_memory() for _ in range(3)]
    s.stream = torch.cuda.Stream()

    def produce(g):
        for dst, a in zip(s.bufs, s.src[g]):
            dst[:a.numel()].copy_(a, non_blocking=True)

    def call(k):
        """sha256_msgs_stream, the P-256 signer under low-S and the secp256k1 signer, then the copy into pinned memory: all on s.stream"""
        sp, o, w = s.stream.cuda_stream, s.outs[k].data_ptr(), s.work[k].data_ptr()
        head = (s.bufs[0].data_ptr(), NK, s.d_index.data_ptr(), s.bufs[1].data_ptr(), s.bufs[2].data_ptr(), N)
        sbv.sha256_msgs_stream(s.bufs[1].data_ptr(), s.bufs[2].data_ptr(), N, o, sp)
        p = o + P_AT
        sbv.p256_sign_msgs_stream(*head, p, p + 72 * N, p + 73 * N, w, low_s=True, stream=sp)
        q = o + K_AT
        sbv.secp256k1_sign_msgs_stream(*head, q, q + 72 * N, q + 73 * N, q + 74 * N, w + 96 * N, stream=sp)
        s.hosts[k].copy_(s.outs[k], non_blocking=True)

    def check(k, g, what):
        got, want = s.hosts[k].numpy().tobytes(), s.gen[g].want
        if got != want:
            other = s.gen["x" if g == "y" else "y"].want
            a, w = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
            kind = "the OTHER generation's" if got == other else "a mixture: %d bytes differ, first at %d" % (int((a != w).sum()), int(np.flatnonzero(a != w)[0]))
            raise AssertionError("%s: output %d is not generation %s's but %s" % (what, k, g.upper(), kind))
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
    s.call_ms = a.elapsed_time(b)
    s.delay_ms = min(DELAY_MAX_MS, max(DELAY_MIN_MS, DELAY_FACTOR * s.call_ms))
    check(0, "x", "warm call")
    print("\n[ecdsa sign msgs, stream order] one warm hash + two signers of %d: %.3f ms; delay %.1f ms" % (N, s.call_ms, s.delay_ms))
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
            assert torch.equal(dst[:a.numel()], a)


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


# ---- round trip: sign, spoil every third message, verify the packed output as returned ----------------------------------------------
@pytest.mark.parametrize("low_s", [False, True], ids=["flags0", "low_s"])
@pytest.mark.parametrize("curve", cases.CURVES)
def test_round_trip_through_the_raw_message_verifier(curve, low_s, large, oracle):
    pub = getattr(oracle, "sbvo_%s_pubkey" % curve)
    pub.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    q = ctypes.create_string_buffer(64)
    pubs = []
    for k in range(NK):
        pub(large.keys[32 * k:32 * k + 32], q)
        pubs.append(q.raw)
    out = SIGNERS[curve](large.keys, large.msgs, key_index=large.index, low_s=low_s)
    sigs, soff, ok = out[0], out[1], out[-1]
    assert ok == b"\x01" * N
    want = large.want[curve, cases.LOW_S if low_s else 0]
    assert sigs == b"".join(packed(want[0], want[1]))
    if low_s:
        half = (cases.order(curve) - 1) // 2
        assert all(int.from_bytes(fc.strict_rs(sg)[32:], "big") <= half for sg in split(sigs, soff))
    msgs = [m if i % 3 else (bytes([m[0] ^ 1]) + m[1:] if m else b"\x01") for i, m in enumerate(large.msgs)]
    lib = sbv.load()
    U64P = ctypes.POINTER(ctypes.c_uint64)
    name = "sbv_p256_verify_msgs" if curve == "p256" else "sbv_secp256k1_verify_msgs"
    getattr(lib, name).argtypes = [ctypes.c_char_p, U64P, ctypes.c_char_p, U64P, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    bm = ctypes.create_string_buffer((N + 7) // 8)
    moff = (ctypes.c_uint64 * (N + 1))(*cases.offsets_of(msgs))
    rc = getattr(lib, name)(b"".join(msgs), moff, sigs, (ctypes.c_uint64 * (N + 1))(*soff), b"".join(pubs[k] for k in large.index), N, bm)
    assert rc == 0
    assert sbv.bitmap_to_list(bm.raw, N) == [i % 3 != 0 for i in range(N)]


# ---- above the C-ABI ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme,curve", [(0, "p256"), (2, "k256")])
def test_host_sign_batch_on_the_device_equals_a_loop_of_sign(scheme, curve):
    host = hostlib.load()
    V, S, C = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p
    host.sbvh_sign_batch.restype = S
    host.sbvh_sign_batch.argtypes = [V, C, ctypes.POINTER(ctypes.c_uint64), S, C, S]
    host.sbvh_sign_batch_low_s.restype = S
    host.sbvh_sign_batch_low_s.argtypes = [V, C, ctypes.POINTER(ctypes.c_uint64), S, ctypes.c_int, C, S]
    msgs = messages(300, 0x300)
    d = int.from_bytes(keys_of(1, b"host-sign-batch")[:32], "big")
    offs = (ctypes.c_uint64 * 301)(*cases.offsets_of(msgs))
    signer = host.sbvh_signer_new_scheme(scheme, 1, cases.be32(d))
    try:
        out, one = ctypes.create_string_buffer(80 * 300), ctypes.create_string_buffer(80)
        assert host.sbvh_sign_batch(signer, b"".join(msgs) + b"\0", offs, 300, out, 80) == 300
        for i, m in enumerate(msgs):
            k = host.sbvh_sign(signer, m, len(m), one, 80)
            assert out.raw[80 * i:80 * i + k] == one.raw[:k], i
        dev = SIGNERS[curve](cases.be32(d), msgs[:1])[0]
        assert out.raw[:len(dev)] == dev and out.raw[len(dev):80] == bytes(80 - len(dev))      # ... and that is the device's signature
        assert host.sbvh_sign_batch_low_s(signer, b"".join(msgs) + b"\0", offs, 300, 1, out, 80) == 300
        low = split(*SIGNERS[curve](cases.be32(d), msgs, low_s=True)[:2])
        for i in range(300):
            assert out.raw[80 * i:80 * i + len(low[i])] == low[i], i
    finally:
        host.sbvh_signer_free(signer)


def test_smoke_passes():
    """start-up: __graft_entry__.smoke() in a process of its own, the raw-message signing step included"""
    r = subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.smoke()"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "smoke ok: raw-message P-256 signing" in r.stdout
