"""Batch signing on the GPU (sbv_p256_sign_batch) through the C-ABI: bit-identical to the host Signer
(RFC 6979) and to the RFC 6979 A.2.5 known answers; every signature verifies on the device and under the oracle.

The second half holds every byte the device writes to an independent signer (tests/p256_sign_cases.py: hmac / hashlib, Python integers
and oracle/p256_py.py) and to the emulated lanes that tests/test_emul_sign.py pins to it: the RFC 6979 retry inside a diverged
wavefront, the launch geometry with sentinels behind the outputs, rejected lanes, the refused calls of the two entries, the first call
of a process and the 16-bit comb of G."""
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
import p256_sign_cases as cases
import test_emul_sign as cpu_tier
from test_emul_device_algo import emul  # noqa: F401  (fixture: builds tests/emul/libsbv_emul.so)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOTINIT = -2, -5
SENTINEL = 0x3C
T0 = time.perf_counter()
N_ORDER = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551


@pytest.fixture(scope="module")
def host():
    return hostlib.load()


@pytest.fixture(scope="module", autouse=True)
def _init():
    sbv.init(0)
    yield
    print("\n[p256 sign] wall time of this file: %.1f s" % (time.perf_counter() - T0))


def test_rfc6979_known_answers_on_the_gpu(rfc6979):
    d = bytes.fromhex(rfc6979["private_key"])
    kat = [s for s in rfc6979["signatures"] if s["hash_alg"] == "sha256"]
    sigs, ok = sbv.sign_batch(d, b"".join(bytes.fromhex(s["hash"]) for s in kat))
    assert ok == b"\x01\x01"
    for i, s in enumerate(kat):
        assert sigs[64 * i:64 * i + 64].hex() == s["r"] + s["s"]


def test_gpu_signatures_equal_the_host_signers_and_verify(host, oracle):
    rng = np.random.default_rng(20260921)
    nk, n = 37, 1 << 14
    keys = b"".join(int.to_bytes(int.from_bytes(rng.bytes(32), "big") % (N_ORDER - 1) + 1, 32, "big") for _ in range(nk))
    digests = rng.bytes(32 * (n - 2)) + b"\x00" * 32 + b"\xff" * 32
    index = rng.integers(0, nk, n).astype(np.uint32)
    sigs, ok = sbv.sign_batch(keys, digests, [int(x) for x in index])
    assert ok == b"\x01" * n
    pubs = []
    for k in range(nk):
        q = ctypes.create_string_buffer(64)
        assert host.sbvh_pubkey(keys[32 * k:32 * k + 32], q) == 0
        pubs.append(q.raw)
    for i in list(range(0, n, 257)) + [n - 2, n - 1]:                  # the host signer is slow: a stride of the batch
        rs = ctypes.create_string_buffer(64)
        assert host.sbvh_sign_rfc6979(keys[32 * int(index[i]):32 * int(index[i]) + 32], digests[32 * i:32 * i + 32], rs) == 0
        assert sigs[64 * i:64 * i + 64] == rs.raw, i
    tuples = b"".join(sigs[64 * i:64 * i + 64] + digests[32 * i:32 * i + 32] + pubs[int(index[i])] for i in range(n))
    bm = sbv.verify_batch(tuples, n)                                     # sign -> verify round trip on the device
    assert bm == b"\xff" * (n // 8)
    want = ctypes.create_string_buffer(n // 8)
    oracle.sbvo_p256_verify_batch(tuples[:160 * 2048], 2048, want, 8)    # and under the oracle
    assert want.raw[:256] == b"\xff" * 256


def test_bad_keys_and_indices(host):
    keys = b"\x00" * 32 + N_ORDER.to_bytes(32, "big") + (1).to_bytes(32, "big")
    sigs, ok = sbv.sign_batch(keys, hashlib.sha256(b"x").digest() * 4, [0, 1, 2, 3])
    assert ok == b"\x00\x00\x01\x00"
    assert sigs[:128] == b"\x00" * 128 and sigs[192:] == b"\x00" * 64
    rs = ctypes.create_string_buffer(64)
    assert host.sbvh_sign_rfc6979((1).to_bytes(32, "big"), hashlib.sha256(b"x").digest(), rs) == 0
    assert sigs[128:192] == rs.raw


def test_signing_rate_is_reported(capsys):
    """Not a pass/fail bar: prints the device signing rate at 2^18 signatures (device-resident buffers, event-free wall clock)."""
    import torch
    n, nk = 1 << 18, 1024
    rng = np.random.default_rng(7)
    keys = torch.from_numpy(np.frombuffer(b"".join(int.to_bytes(int.from_bytes(rng.bytes(32), "big") % (N_ORDER - 1) + 1, 32, "big")
                                                   for _ in range(nk)), dtype=np.uint8).copy()).cuda()
    dig = torch.from_numpy(np.frombuffer(rng.bytes(32 * n), dtype=np.uint8).copy()).cuda()
    sig = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
    ok = torch.empty(n, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    for rep in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sbv.sign_batch_dev(keys.data_ptr(), nk, 0, dig.data_ptr(), n, sig.data_ptr(), ok.data_ptr(), st.cuda_stream)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    assert int(ok.sum().item()) == n
    with capsys.disabled():
        print("\n[sign] %d signatures in %.3f ms = %.1f M signatures/s" % (n, dt * 1e3, n / dt / 1e6))


# ---- every byte against the independent signer and the emulated lanes ----------------------------------------------------------------
N = cases.N


def _sig(blob, i):
    return blob[64 * i:64 * i + 64]


def _keys(count, label=b"p256-sign-key"):
    return [int.from_bytes(hashlib.sha256(label + b"%d" % i).digest(), "big") % (N - 1) + 1 for i in range(count)]


def _digests(n, seed):
    return random.Random(seed).randbytes(32 * n)


def _dev(torch, data, dtype=np.uint8):
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=dtype).copy()).cuda()


def test_device_equals_the_independent_python_signer():
    """the 300 seeded pairs and the edge digests under the edge keys, case i under key i with a null index"""
    pairs, want = cases.sign_cases(), cases.sign_expected()
    keys, digests = cases.blobs(pairs)
    sigs, ok = sbv.sign_batch(keys, digests)
    assert ok == b"\x01" * len(pairs)
    bad = [i for i in range(len(pairs)) if _sig(sigs, i) != want[i]]
    assert not bad, (len(bad), bad[:8])


def test_retry_vector_inside_a_diverged_wavefront(emul):
    """the one input whose first candidate is >= N at lanes 0, 63, 64 and 255 of 256: those lanes run RFC 6979 section 3.2 h (the
    33-byte HMAC) and a second scalar multiplication while the 63 other lanes of their wavefronts are done"""
    v = cases.retry_vector()
    n, lanes = 256, (0, 63, 64, 255)
    keys = [cases.be32(d) for d in _keys(n, b"p256-sign-retry")]
    dig = bytearray(_digests(n, 0x4E7))
    for lane in lanes:
        keys[lane] = cases.be32(v["d"])
        dig[32 * lane:32 * lane + 32] = v["digest"]
    keys, dig = b"".join(keys), bytes(dig)
    sigs, ok = sbv.sign_batch(keys, dig)
    assert ok == b"\x01" * n
    assert [_sig(sigs, lane) for lane in lanes] == [v["sig"]] * 4
    assert (sigs, ok) == cpu_tier.sign(emul, keys, dig)


def _geometry_digests(n):
    """random digests with the edge digests at the first and last lanes of a wavefront, of a workgroup (256 lanes) and of the batch"""
    dig = bytearray(_digests(n, 0x6E0 + n))
    spots = [0, 63, 64, 127, 255, 256, 511, 8191, 8192, n - 1]
    for j, lane in enumerate(s for s in spots if s < n):
        dig[32 * lane:32 * lane + 32] = cases.be32(cases.EDGE_DIGESTS[j % len(cases.EDGE_DIGESTS)])
    return bytes(dig)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 8229])
def test_launch_geometry_every_byte_and_nothing_behind_n(emul, n):
    import torch
    nk = 37
    keys = b"".join(cases.be32(d) for d in _keys(nk))
    digests = _geometry_digests(n)
    rng = random.Random(0x37 + n)
    index = [rng.randrange(nk) for _ in range(n)]
    d_keys, d_dig = _dev(torch, keys), _dev(torch, digests)
    d_idx = torch.from_numpy(np.array(index, dtype=np.uint32).view(np.int32)).cuda()
    for idx, d_index in ((None, 0), (index, d_idx.data_ptr())):
        want = cpu_tier.sign(emul, keys, digests, idx)
        assert want[1] == b"\x01" * n
        d_sig = torch.full((64 * n + 128,), SENTINEL, dtype=torch.uint8, device="cuda")
        d_ok = torch.full((n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        sbv.sign_batch_dev(d_keys.data_ptr(), nk, d_index, d_dig.data_ptr(), n, d_sig.data_ptr(), d_ok.data_ptr())
        torch.cuda.synchronize()
        for name, got, exp in (("sigs", d_sig, want[0]), ("ok", d_ok, want[1])):
            raw = got.cpu().numpy().tobytes()
            assert raw[:len(exp)] == exp, (name, n, idx is not None)
            assert raw[len(exp):] == bytes([SENTINEL]) * (len(raw) - len(exp)), (name, n, idx is not None, "bytes behind the last item were written")
        assert sbv.sign_batch(keys, digests, idx) == want, (n, idx is not None)          # the host-pointer form: the same bytes


def test_rejected_lanes_in_the_middle_of_a_wave(emul):
    good = _keys(5, b"p256-sign-reject")
    keys = b"".join(cases.be32(d) for d in good + cases.REJECTED_KEYS)
    n = 192
    digests = _digests(n, 0x4EC7)
    idx = [i % 5 for i in range(n)]
    bad = {70: 5, 71: 6, 100: 7, 101: 8, 102: 0xFFFFFFFF, 130: 5}             # d = 0, N, 2^256 - 1, the indices n_keys and 0xFFFFFFFF
    for i, v in bad.items():
        idx[i] = v
    sigs, ok = sbv.sign_batch(keys, digests, idx)
    for i in range(n):
        if i in bad:
            assert (ok[i], _sig(sigs, i)) == (0, bytes(64)), i
        else:
            assert (ok[i], _sig(sigs, i)) == (1, cases.py_sign(good[idx[i]], digests[32 * i:32 * i + 32])[0]), i
    assert (sigs, ok) == cpu_tier.sign(emul, keys, digests, idx)


def test_refused_calls():
    import torch
    lib = sbv.load()
    V, S, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    lib.sbv_p256_sign_batch.argtypes = [V, U, V, V, S, V, V]
    lib.sbv_p256_sign_batch_dev.argtypes = [V, U, V, V, S, V, V, V]
    n, nk = 3, 2
    key_ints = _keys(nk, b"p256-sign-refused")
    keys = ctypes.create_string_buffer(b"".join(cases.be32(d) for d in key_ints), 32 * nk)
    dig = ctypes.create_string_buffer(_digests(n, 0x4EF), 32 * n)
    order = [0, 1, 0]
    idx = (ctypes.c_uint32 * n)(*order)
    want = b"".join(cases.py_sign(key_ints[k], dig.raw[32 * i:32 * i + 32])[0] for i, k in enumerate(order))
    fill = lambda k: ctypes.create_string_buffer(bytes([SENTINEL]) * k, k)                     # noqa: E731
    sig, okb = fill(64 * n), fill(n)
    good = [keys, nk, idx, dig, n, sig, okb]

    def host_refuses(args, what):
        """the refusal, then a good call that still signs correctly"""
        assert lib.sbv_p256_sign_batch(*args) == EINVAL, what
        s2, o2 = fill(64 * n), fill(n)
        assert lib.sbv_p256_sign_batch(keys, nk, idx, dig, n, s2, o2) == 0 and (s2.raw, o2.raw) == (want, b"\x01" * n), what

    for pos in (0, 3, 5, 6):                                           # keys, digests, sigs, ok
        args = list(good)
        args[pos] = None
        host_refuses(args, pos)
    host_refuses([keys, 0, idx, dig, n, sig, okb], "n_keys == 0")
    assert lib.sbv_p256_sign_batch(keys, nk, idx, dig, 0, sig, okb) == 0                        # n = 0: nothing is written
    assert lib.sbv_p256_sign_batch(None, 0, None, None, 0, None, None) == 0
    assert (sig.raw, okb.raw) == (bytes([SENTINEL]) * 64 * n, bytes([SENTINEL]) * n)            # ... by the refused calls either
    # the _dev form: the same rules, and the 4-byte alignment of keys, key index, digests and sigs
    t = {k: torch.full((512,), SENTINEL, dtype=torch.uint8, device="cuda") for k in ("keys", "idx", "dig", "sig", "ok")}
    t["keys"][:32 * nk] = _dev(torch, keys.raw)
    t["dig"][:32 * n] = _dev(torch, dig.raw)
    t["idx"][:4 * n] = _dev(torch, bytes(idx))
    p = {k: v.data_ptr() for k, v in t.items()}
    good = [p["keys"], nk, p["idx"], p["dig"], n, p["sig"], p["ok"], None]
    g_sig, g_ok = (torch.full((512,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(2))

    def dev_refuses(args, what):
        assert lib.sbv_p256_sign_batch_dev(*args) == EINVAL, what
        g_sig.fill_(SENTINEL)
        g_ok.fill_(SENTINEL)
        torch.cuda.synchronize()
        assert lib.sbv_p256_sign_batch_dev(p["keys"], nk, p["idx"], p["dig"], n, g_sig.data_ptr(), g_ok.data_ptr(), None) == 0, what
        torch.cuda.synchronize()
        assert g_sig.cpu().numpy().tobytes() == want + bytes([SENTINEL]) * (512 - 64 * n), what
        assert g_ok.cpu().numpy().tobytes() == b"\x01" * n + bytes([SENTINEL]) * (512 - n), what

    for pos in (0, 3, 5, 6):
        args = list(good)
        args[pos] = None
        dev_refuses(args, pos)
    args = list(good)
    args[1] = 0
    dev_refuses(args, "n_keys == 0")
    for pos in (0, 2, 3, 5):                                           # keys, key index, digests, sigs
        for off in (1, 2, 3):
            args = list(good)
            args[pos] += off
            dev_refuses(args, (pos, off))
    args = list(good)
    args[4] = 0
    assert lib.sbv_p256_sign_batch_dev(*args) == 0                     # n = 0: nothing is written
    torch.cuda.synchronize()
    assert t["sig"].cpu().numpy().tobytes() == bytes([SENTINEL]) * 512 and t["ok"].cpu().numpy().tobytes() == bytes([SENTINEL]) * 512
    for off in (1, 2, 3):                                              # ok is a byte array: any address
        args = list(good)
        args[6] += off
        t["sig"].fill_(SENTINEL)
        t["ok"].fill_(SENTINEL)
        torch.cuda.synchronize()
        assert lib.sbv_p256_sign_batch_dev(*args) == 0, off
        torch.cuda.synchronize()
        assert t["sig"].cpu().numpy().tobytes()[:64 * n] == want, off
        assert t["ok"].cpu().numpy().tobytes() == bytes([SENTINEL]) * off + b"\x01" * n + bytes([SENTINEL]) * (512 - off - n), off


_FIRST_CALL = r"""
import ctypes, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import consensus_amd as sbv
keys, digests, want = (bytes.fromhex(a) for a in sys.argv[2:5])
n, nk = len(digests) // 32, len(keys) // 32
d_keys = torch.from_numpy(np.frombuffer(keys, dtype=np.uint8).copy()).cuda()
d_dig = torch.from_numpy(np.frombuffer(digests, dtype=np.uint8).copy()).cuda()
d_out = torch.zeros(65 * n, dtype=torch.uint8, device="cuda")
lib = sbv.load()
V = ctypes.c_void_p
lib.sbv_p256_sign_batch_dev.argtypes = [V, ctypes.c_uint32, V, V, ctypes.c_size_t, V, V, V]
lib.sbv_p256_sign_batch.argtypes = [ctypes.c_char_p, ctypes.c_uint32, V, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p]
print("before-init", lib.sbv_p256_sign_batch_dev(d_keys.data_ptr(), nk, None, d_dig.data_ptr(), n, d_out.data_ptr(), d_out.data_ptr() + 64 * n, None),
      lib.sbv_p256_sign_batch(keys, nk, None, digests, n, ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(n)))
sbv.init(0)
st = torch.cuda.Stream()
torch.cuda.synchronize()
sbv.sign_batch_dev(d_keys.data_ptr(), nk, 0, d_dig.data_ptr(), n, d_out.data_ptr(), d_out.data_ptr() + 64 * n, st.cuda_stream)
torch.cuda.synchronize()
print("first-call", "equal" if d_out.cpu().numpy().tobytes() == want else "DIFFERS")
"""


def test_first_call_of_a_process_is_the_dev_signer_on_a_side_stream(emul):
    """before sbv_init both entries answer SBV_ENOTINIT; after it, nothing else has run when sbv_p256_sign_batch_dev signs"""
    n, nk = 300, 7
    keys = b"".join(cases.be32(d) for d in _keys(nk, b"p256-sign-first"))
    digests = _digests(n, 0xF157)
    sigs, ok = cpu_tier.sign(emul, keys, digests)
    assert ok == b"\x01" * n
    r = subprocess.run([sys.executable, "-c", _FIRST_CALL, ROOT, keys.hex(), digests.hex(), (sigs + ok).hex()], capture_output=True, text=True,
                       timeout=180)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(ln.split(" ", 1) for ln in r.stdout.splitlines() if ln.startswith(("before-init", "first-call")))
    assert lines == {"before-init": "%d %d" % (ENOTINIT, ENOTINIT), "first-call": "equal"}, r.stdout[-2000:]


_G_BITS = r"""
import sys
sys.path.insert(0, sys.argv[1])
import consensus_amd as sbv
keys, digests, want = (bytes.fromhex(a) for a in sys.argv[2:5])
sbv.init(0)
sigs, ok = sbv.sign_batch(keys, digests)
print("g-bits-16", "equal" if sigs + ok == want else "DIFFERS")
"""


def test_the_16_bit_comb_of_g_signs_the_same_bytes():
    """SBV_G_BITS is read once at start-up: a fresh child with the 16-bit comb (the emulator's) against this process's 20-bit one"""
    csrc = os.path.join(ROOT, "consensus_amd", "csrc")
    assert any('getenv("SBV_G_BITS")' in open(os.path.join(csrc, f)).read() for f in os.listdir(csrc) if f.endswith(".hip"))
    assert os.environ.get("SBV_G_BITS") in (None, "20")                       # this process runs the default
    v = cases.retry_vector()
    keys, digests = cases.blobs(cases.sign_cases() + [(v["d"], v["digest"])])
    sigs, ok = sbv.sign_batch(keys, digests)
    assert ok == b"\x01" * len(ok) and sigs == b"".join(cases.sign_expected()) + v["sig"]
    r = subprocess.run([sys.executable, "-c", _G_BITS, ROOT, keys.hex(), digests.hex(), (sigs + ok).hex()], env=dict(os.environ, SBV_G_BITS="16"),
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0 and "g-bits-16 equal" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_round_trip_of_the_sign_cases_through_the_verifier():
    """verify_batch accepts every signature of sign_cases() and rejects each with one digest bit flipped"""
    pairs = cases.sign_cases()
    keys, digests = cases.blobs(pairs)
    sigs, ok = sbv.sign_batch(keys, digests)
    assert ok == b"\x01" * len(pairs)
    tup = [_sig(sigs, i) + h + cases.pubkey(d) for i, (d, h) in enumerate(pairs)]
    assert sbv.bitmap_to_list(sbv.verify_batch(b"".join(tup), len(tup)), len(tup)) == [True] * len(tup)
    flipped = [t[:64] + cases.be32(int.from_bytes(t[64:96], "big") ^ (1 << (i % 256))) + t[96:] for i, t in enumerate(tup)]
    assert sbv.bitmap_to_list(sbv.verify_batch(b"".join(flipped), len(tup)), len(tup)) == [False] * len(tup)
