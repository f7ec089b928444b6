"""GPU tier of the BIP-340 Schnorr entries over secp256k1 (include/sbv.h: sbv_secp256k1_schnorr_verify, _expand_keys, _sign, their
_stream forms, sbv_secp256k1_schnorr_verify_workspace, sbv_debug_secp256k1_schnorr_op), through the C-ABI and the Python wrapper.

Every byte the device writes is compared with the Python model of tests/k256_schnorr_cases.py (the cases of the CPU tier,
tests/test_k256_schnorr_cpu.py).  Large batches tile the case set with a rotation, so their expected values are the model's too.  The
_stream entries run under callers that do not synchronise — late producer, early overwriter, X-Y-X, two streams with two workspaces —
with the delay of tests/test_gpu_stream_order.py."""
import ctypes
import hashlib
import os
import random
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import consensus_amd as sbv
import hostlib
import k256_schnorr_cases as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = cases.N
EINVAL, ENOTINIT = -2, -5
SENTINEL = 0x3C
STRIP = 1536                                       # bytes of one lane's table strip (include/sbv.h)
TAIL = 4096                                        # sentinel bytes behind a workspace
LANES = int(re.search(r"#define SBV_K256_RECOVER_LANES (\d+)", open(os.path.join(ROOT, "include", "sbv.h")).read()).group(1))
T0 = time.perf_counter()


@pytest.fixture(scope="module", autouse=True)
def _init():
    sbv.init(0)
    yield
    print("\n[secp256k1 schnorr] wall time of this file: %.1f s" % (time.perf_counter() - T0))


@pytest.fixture(scope="module")
def model():
    """the expected values of every case, from the Python model, once"""
    t = time.perf_counter()
    exp = cases.expected_all()
    cases.signed()
    cases.signed(True)
    print("\n[secp256k1 schnorr] the model of %d cases and %d triples: %.1f s" % (len(exp), len(cases.triples()), time.perf_counter() - t))
    return exp


def _dev(torch, data, dtype=np.uint8):
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=dtype).copy()).cuda()


def _idx_dev(torch, idx):
    return torch.from_numpy(np.array(idx, dtype=np.uint32).view(np.int32)).cuda()


def _records():
    return b"".join(w[0] for w in cases.expanded())


# ---- every case -----------------------------------------------------------------------------------------------------------------------
def test_every_case_against_the_model(model):
    ok = sbv.secp256k1_schnorr_verify(*cases.arrays())
    bad = [(i, cases.cases()[i][0]) for i in range(len(model)) if ok[i] != model[i]]
    assert not bad, (len(bad), bad[:8])
    assert ok.count(1) >= 299 and ok.count(0) >= 1600


@pytest.mark.parametrize("op", [0, 1, 2, 3])
def test_unit_operations_on_the_device(op):
    ins, want = cases.all_op_cases()[op]
    got = sbv.debug_secp256k1_schnorr_op(op, ins)
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (op, len(bad), bad[:8])


def test_the_walk_with_a_zero_scalar_on_the_device():
    """op 2 of sbv_debug_secp256k1_recover_op with u2 = 0 (new with this scheme), u1 = 0 and both (infinity)"""
    ins, want = cases.walk_cases()
    got = sbv.debug_secp256k1_recover_op(2, ins)
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (len(bad), bad[:8])


def test_known_answers_on_the_device():
    vs = cases.vectors()
    exp, pks, ok = sbv.secp256k1_schnorr_expand_keys(b"".join(v["d"] for v in vs))
    assert ok == b"\x01\x01" and pks == b"".join(v["pk"] for v in vs)
    sigs, sok = sbv.secp256k1_schnorr_sign(exp, b"".join(v["msg"] for v in vs), b"".join(v["aux"] for v in vs))
    assert sok == b"\x01\x01" and sigs == b"".join(v["sig"] for v in vs)
    assert sbv.secp256k1_schnorr_verify(pks, b"".join(v["msg"] for v in vs), sigs) == b"\x01\x01"


def test_expansion_against_the_model_with_refused_keys_in_the_batch(model):
    want = cases.expanded()
    exp, pks, ok = sbv.secp256k1_schnorr_expand_keys(cases.key_blob())
    assert exp == _records() and pks == b"".join(w[1] for w in want) and ok == bytes(w[2] for w in want)
    refused = [i for i, w in enumerate(want) if not w[2]]
    assert len(refused) == 3 and 0 < refused[0] and refused[-1] < len(want) - 1
    assert all(exp[64 * i:64 * i + 64] == bytes(64) and pks[32 * i:32 * i + 32] == bytes(32) for i in refused)
    exp2, none, ok2 = sbv.secp256k1_schnorr_expand_keys(cases.key_blob(), want_pks=False)
    assert (exp2, none, ok2) == (exp, None, ok)


def test_signatures_byte_for_byte_with_aux_and_without(model):
    tr = cases.triples()
    msgs, aux = b"".join(t[1] for t in tr), b"".join(t[2] for t in tr)
    sigs, ok = sbv.secp256k1_schnorr_sign(_records(), msgs, aux)
    assert sigs == b"".join(s for s, _ in cases.signed()) and ok == bytes(o for _, o in cases.signed())
    sigs0, ok0 = sbv.secp256k1_schnorr_sign(_records(), msgs, None)
    assert sigs0 == b"".join(s for s, _ in cases.signed(True)) and ok0 == ok
    assert sbv.secp256k1_schnorr_sign(_records(), msgs, bytes(len(aux))) == (sigs0, ok0) and sigs0 != sigs
    # the index rule: explicit indices, two of them out of range
    idx, m2, a2, s2, o2 = cases.tiled_sign(337, 5)
    assert sbv.secp256k1_schnorr_sign(_records(), m2, a2, idx) == (s2, o2)
    idx[3], idx[100] = len(tr), 2**32 - 1
    s3, o3 = sbv.secp256k1_schnorr_sign(_records(), m2, a2, idx)
    assert o3 == o2[:3] + b"\x00" + o2[4:100] + b"\x00" + o2[101:]
    assert s3 == s2[:192] + bytes(64) + s2[256:6400] + bytes(64) + s2[6464:]


# ---- launch geometry ------------------------------------------------------------------------------------------------------------------
def _verify_stream(torch, n, pks, msgs, sigs, stream=0):
    """the _stream verifier on fresh buffers with sentinels behind ok and the workspace: (ok buffer, workspace, its size)"""
    d_pk, d_msg, d_sig = _dev(torch, pks), _dev(torch, msgs), _dev(torch, sigs)
    wb = sbv.secp256k1_schnorr_verify_workspace(n)
    assert wb == min(n, LANES) * STRIP
    d_ok = torch.full((n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_work = torch.full((wb + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert d_work.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    sbv.secp256k1_schnorr_verify_stream(d_pk.data_ptr(), d_msg.data_ptr(), d_sig.data_ptr(), n, d_ok.data_ptr(), d_work.data_ptr(), wb, stream=stream)
    torch.cuda.synchronize()
    return d_ok, d_work, wb


def _check_verify_geometry(torch, n, shift=0):
    pks, msgs, sigs, want = cases.tiled(n, shift)
    d_ok, d_work, wb = _verify_stream(torch, n, pks, msgs, sigs)
    ok = d_ok.cpu().numpy().tobytes()
    if ok[:n] != want:
        bad = [i for i in range(n) if ok[i] != want[i]]
        raise AssertionError("n = %d: %d verdicts differ, first %s" % (n, len(bad), bad[:8]))
    assert ok[n:] == bytes([SENTINEL]) * 64, (n, "bytes behind the last ok were written")
    assert bool((d_work[wb:] == SENTINEL).all()), (n, "bytes behind the workspace were written")
    return pks, msgs, sigs, want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_launch_geometry_every_byte_and_nothing_behind_n(model, n):
    import torch
    # verify
    pks, msgs, sigs, want = _check_verify_geometry(torch, n, shift=n)
    assert sbv.secp256k1_schnorr_verify(pks, msgs, sigs) == want                                    # the host-pointer form
    # expand: the first n keys, sentinels behind the records, the keys and ok
    keys = (cases.key_blob() * 2)[:32 * n]
    want_e = (cases.expanded() * 2)[:n]
    d_keys = _dev(torch, keys)
    d_exp = torch.full((64 * (n + 2),), SENTINEL, dtype=torch.uint8, device="cuda")
    d_pk = torch.full((32 * (n + 2),), SENTINEL, dtype=torch.uint8, device="cuda")
    d_ok = torch.full((n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sbv.secp256k1_schnorr_expand_keys_stream(d_keys.data_ptr(), n, d_exp.data_ptr(), d_pk.data_ptr(), d_ok.data_ptr())
    torch.cuda.synchronize()
    exp, pk, ok = (t.cpu().numpy().tobytes() for t in (d_exp, d_pk, d_ok))
    assert exp == b"".join(w[0] for w in want_e) + bytes([SENTINEL]) * 128, n
    assert pk == b"".join(w[1] for w in want_e) + bytes([SENTINEL]) * 64, n
    assert ok == bytes(w[2] for w in want_e) + bytes([SENTINEL]) * 64, n
    assert sbv.secp256k1_schnorr_expand_keys(keys) == (exp[:64 * n], pk[:32 * n], ok[:n])            # the host-pointer form
    # sign: n items under all the records, sentinels behind sigs and ok
    idx, m2, a2, s2, o2 = cases.tiled_sign(n, n)
    d_rec, d_idx, d_m, d_a = _dev(torch, _records()), _idx_dev(torch, idx), _dev(torch, m2), _dev(torch, a2)
    d_sig = torch.full((64 * (n + 2),), SENTINEL, dtype=torch.uint8, device="cuda")
    d_ok = torch.full((n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sbv.secp256k1_schnorr_sign_stream(d_rec.data_ptr(), len(cases.triples()), d_idx.data_ptr(), d_m.data_ptr(), d_a.data_ptr(), n, d_sig.data_ptr(),
                                      d_ok.data_ptr())
    torch.cuda.synchronize()
    assert d_sig.cpu().numpy().tobytes() == s2 + bytes([SENTINEL]) * 128, n
    assert d_ok.cpu().numpy().tobytes() == o2 + bytes([SENTINEL]) * 64, n
    assert sbv.secp256k1_schnorr_sign(_records(), m2, a2, idx) == (s2, o2)                           # the host-pointer form


@pytest.mark.parametrize("n", [LANES - 1, LANES, LANES + 1, 2 * LANES + 3], ids=["lanes-1", "lanes", "lanes+1", "2lanes+3"])
def test_capped_grid_reuses_its_strips(model, n):
    """around the cap of the grid: the last lane idle, every lane once, lane 0 twice, every lane twice or three times"""
    import torch
    _check_verify_geometry(torch, n, shift=3)


def test_host_pointer_form_beyond_the_cap(model):
    n = LANES + 300
    pks, msgs, sigs, want = cases.tiled(n, 11)
    assert sbv.secp256k1_schnorr_verify(pks, msgs, sigs) == want


# ---- refused calls --------------------------------------------------------------------------------------------------------------------
def test_refused_calls(model):
    import torch
    lib = sbv.load()
    V, S, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    lib.sbv_secp256k1_schnorr_verify.argtypes = [V, V, V, S, V]
    lib.sbv_secp256k1_schnorr_verify_stream.argtypes = [V, V, V, S, V, V, S, V]
    lib.sbv_secp256k1_schnorr_verify_workspace.argtypes = [S]
    lib.sbv_secp256k1_schnorr_verify_workspace.restype = S
    lib.sbv_secp256k1_schnorr_expand_keys.argtypes = [V, S, V, V, V]
    lib.sbv_secp256k1_schnorr_expand_keys_stream.argtypes = [V, S, V, V, V, V]
    lib.sbv_secp256k1_schnorr_sign.argtypes = [V, U, V, V, V, S, V, V]
    lib.sbv_secp256k1_schnorr_sign_stream.argtypes = [V, U, V, V, V, S, V, V, V]
    assert [lib.sbv_secp256k1_schnorr_verify_workspace(k) for k in (0, 1, 2, LANES, LANES + 1, 1 << 40)] == \
        [0, STRIP, 2 * STRIP, LANES * STRIP, LANES * STRIP, LANES * STRIP]
    n = 3
    pks, msgs, sigs, want = cases.tiled(n)
    keys = cases.key_blob()[:32 * n]
    recs = _records()[:64 * n]
    sent = lambda k: ctypes.create_string_buffer(bytes([SENTINEL]) * k, k)
    buf = lambda x: ctypes.create_string_buffer(x, len(x))
    # host-pointer forms: null pointers, n_keys = 0, n = 0 writes nothing
    okb = sent(n)
    good = [buf(pks), buf(msgs), buf(sigs), n, okb]
    for pos in (0, 1, 2, 4):
        args = list(good)
        args[pos] = None
        assert lib.sbv_secp256k1_schnorr_verify(*args) == EINVAL, pos
    assert lib.sbv_secp256k1_schnorr_verify(None, None, None, 0, None) == 0 and okb.raw == bytes([SENTINEL]) * n
    assert lib.sbv_secp256k1_schnorr_verify(*good) == 0 and okb.raw == want
    e_rec, e_pk, e_ok = sent(64 * n), sent(32 * n), sent(n)
    good = [buf(keys), n, e_rec, e_pk, e_ok]
    for pos in (0, 2, 4):
        args = list(good)
        args[pos] = None
        assert lib.sbv_secp256k1_schnorr_expand_keys(*args) == EINVAL, pos
    assert lib.sbv_secp256k1_schnorr_expand_keys(None, 0, None, None, None) == 0 and e_rec.raw == bytes([SENTINEL]) * 64 * n
    assert lib.sbv_secp256k1_schnorr_expand_keys(*good) == 0 and e_rec.raw == recs
    s_sig, s_ok = sent(64 * n), sent(n)
    good = [buf(recs), n, None, buf(msgs), None, n, s_sig, s_ok]
    for pos in (0, 3, 6, 7):
        args = list(good)
        args[pos] = None
        assert lib.sbv_secp256k1_schnorr_sign(*args) == EINVAL, pos
    args = list(good)
    args[1] = 0
    assert lib.sbv_secp256k1_schnorr_sign(*args) == EINVAL
    assert lib.sbv_secp256k1_schnorr_sign(None, 0, None, None, None, 0, None, None) == 0 and s_sig.raw == bytes([SENTINEL]) * 64 * n
    assert lib.sbv_secp256k1_schnorr_sign(*good) == 0 and s_ok.raw == bytes(w[2] for w in cases.expanded()[:n])
    # the _stream forms: the same rules, the 4-byte alignment of the data, the workspace's 16 bytes and its size
    t = {k: torch.full((4096,), SENTINEL, dtype=torch.uint8, device="cuda") for k in ("pk", "msg", "sig", "ok", "key", "rec", "idx", "aux", "out")}
    t["work"] = torch.full((n * STRIP + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    t["pk"][:32 * n] = _dev(torch, pks)
    t["msg"][:32 * n] = _dev(torch, msgs)
    t["sig"][:64 * n] = _dev(torch, sigs)
    t["key"][:32 * n] = _dev(torch, keys)
    t["rec"][:64 * n] = _dev(torch, recs)
    t["idx"][:4 * n] = _dev(torch, np.arange(n, dtype=np.uint32).tobytes())
    t["aux"][:32 * n] = 0
    torch.cuda.synchronize()
    p = {k: v.data_ptr() for k, v in t.items()}
    good = [p["pk"], p["msg"], p["sig"], n, p["ok"], p["work"], n * STRIP, None]
    for pos in (0, 1, 2, 4, 5):
        args = list(good)
        args[pos] = None
        assert lib.sbv_secp256k1_schnorr_verify_stream(*args) == EINVAL, pos
    for pos in (0, 1, 2):
        for off in (1, 2):
            args = list(good)
            args[pos] += off
            assert lib.sbv_secp256k1_schnorr_verify_stream(*args) == EINVAL, (pos, off)
    for off in (1, 4, 8):
        args = list(good)
        args[5] += off
        args[6] += 64 - off
        assert lib.sbv_secp256k1_schnorr_verify_stream(*args) == EINVAL, off
    for short in (0, STRIP, (n - 1) * STRIP, n * STRIP - 1):
        args = list(good)
        args[6] = short
        assert lib.sbv_secp256k1_schnorr_verify_stream(*args) == EINVAL, short
    args = list(good)
    args[3] = 0
    assert lib.sbv_secp256k1_schnorr_verify_stream(*args) == 0
    good_e = [p["key"], n, p["out"], p["out"] + 1024, p["ok"], None]
    for pos in (0, 2, 4):
        args = list(good_e)
        args[pos] = None
        assert lib.sbv_secp256k1_schnorr_expand_keys_stream(*args) == EINVAL, pos
    for pos in (0, 2, 3):
        args = list(good_e)
        args[pos] += 2
        assert lib.sbv_secp256k1_schnorr_expand_keys_stream(*args) == EINVAL, pos
    good_s = [p["rec"], n, p["idx"], p["msg"], p["aux"], n, p["out"], p["ok"], None]
    for pos in (0, 3, 6, 7):
        args = list(good_s)
        args[pos] = None
        assert lib.sbv_secp256k1_schnorr_sign_stream(*args) == EINVAL, pos
    for pos in (0, 2, 3, 4, 6):
        args = list(good_s)
        args[pos] += 1
        assert lib.sbv_secp256k1_schnorr_sign_stream(*args) == EINVAL, pos
    args = list(good_s)
    args[1] = 0
    assert lib.sbv_secp256k1_schnorr_sign_stream(*args) == EINVAL
    torch.cuda.synchronize()
    assert all(bool((t[k] == SENTINEL).all()) for k in ("ok", "out", "work"))                       # refused calls wrote nothing
    args = list(good)
    args[4] += 3                                                        # an odd address for the byte array is fine
    assert lib.sbv_secp256k1_schnorr_verify_stream(*args) == 0
    assert lib.sbv_secp256k1_schnorr_sign_stream(*good_s) == 0
    torch.cuda.synchronize()
    assert t["ok"].cpu().numpy().tobytes()[3:3 + n] == want
    assert t["out"].cpu().numpy().tobytes()[:64 * n] == b"".join(cases.sign(recs[64 * i:64 * i + 64], msgs[32 * i:32 * i + 32], bytes(32))[0] for i in range(n))
    with pytest.raises(sbv.SbvError) as e:
        sbv.debug_secp256k1_schnorr_op(4, [bytes(cases.OP_IN)])
    assert e.value.code == EINVAL
    with pytest.raises(sbv.SbvError):
        sbv.debug_secp256k1_schnorr_op(-1, [bytes(cases.OP_IN)])


# ---- the first secp256k1 call of a process --------------------------------------------------------------------------------------------
_FIRST_CALL = r"""
import ctypes, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import consensus_amd as sbv
which = sys.argv[2]
a, b, c = (bytes.fromhex(x) for x in sys.argv[3:6])
dev = lambda x: torch.from_numpy(np.frombuffer(x, dtype=np.uint8).copy()).cuda()
d_a, d_b, d_c = dev(a), dev(b), dev(c)
lib = sbv.load()
V, S = ctypes.c_void_p, ctypes.c_size_t
if which == "verify":                              # pks, msgs, sigs
    n = len(c) // 64
    d_out = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_work = torch.zeros(1536 * n, dtype=torch.uint8, device="cuda")
    lib.sbv_secp256k1_schnorr_verify_stream.argtypes = [V, V, V, S, V, V, S, V]
    print("before-init", lib.sbv_secp256k1_schnorr_verify_stream(d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), n, d_out.data_ptr(), d_work.data_ptr(), 1536 * n, None))
else:                                              # records, msgs, aux
    n = len(b) // 32
    d_out = torch.zeros(65 * n, dtype=torch.uint8, device="cuda")
    lib.sbv_secp256k1_schnorr_sign_stream.argtypes = [V, ctypes.c_uint32, V, V, V, S, V, V, V]
    print("before-init", lib.sbv_secp256k1_schnorr_sign_stream(d_a.data_ptr(), len(a) // 64, None, d_b.data_ptr(), d_c.data_ptr(), n, d_out.data_ptr(), d_out.data_ptr() + 64 * n, None))
sbv.init(0)
st = torch.cuda.Stream()
torch.cuda.synchronize()
if which == "verify":
    sbv.secp256k1_schnorr_verify_stream(d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), n, d_out.data_ptr(), d_work.data_ptr(), 1536 * n, stream=st.cuda_stream)
else:
    sbv.secp256k1_schnorr_sign_stream(d_a.data_ptr(), len(a) // 64, 0, d_b.data_ptr(), d_c.data_ptr(), n, d_out.data_ptr(), d_out.data_ptr() + 64 * n, stream=st.cuda_stream)
torch.cuda.synchronize()
print("out", d_out.cpu().numpy().tobytes().hex())
"""


@pytest.mark.parametrize("which", ["verify", "sign"])
def test_first_secp256k1_call_of_a_process_is_a_stream_entry(model, which):
    """nothing has uploaded the comb of G before the _stream entry runs; before sbv_init the entries answer SBV_ENOTINIT"""
    n = 300
    if which == "verify":
        a, b, c, want = cases.tiled(n, 5)
    else:
        tr = cases.triples()
        a, b, c = _records(), b"".join(t[1] for t in tr), b"".join(t[2] for t in tr)
        want = b"".join(s for s, _ in cases.signed()) + bytes(o for _, o in cases.signed())
    r = subprocess.run([sys.executable, "-c", _FIRST_CALL, ROOT, which, a.hex(), b.hex(), c.hex()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(ln.split(" ", 1) for ln in r.stdout.splitlines() if ln.startswith(("before-init", "out")))
    assert lines["before-init"] == "%d" % ENOTINIT
    assert bytes.fromhex(lines["out"]) == want


# ---- the _stream entries under callers that do not synchronise ------------------------------------------------------------------------
N_STREAM = 8229


@pytest.fixture(scope="module")
def streams(model):
    import torch
    from test_gpu_stream_order import DELAY_FACTOR, DELAY_MAX_MS, DELAY_MIN_MS, Delay

    class S:
        pass
    s = S()
    s.torch = torch
    s.want, s.src = {"verify": {}, "sign": {}}, {"verify": {}, "sign": {}}
    s.recs = _dev(torch, _records())
    s.n_keys = len(cases.triples())
    for g, shift in (("x", 0), ("y", 401)):                              # two generations: the same cases, rotated against each other
        pks, msgs, sigs, ok = cases.tiled(N_STREAM, shift)
        s.want["verify"][g] = ok
        s.src["verify"][g] = [_dev(torch, pks), _dev(torch, msgs), _dev(torch, sigs)]
        idx, m2, a2, s2, o2 = cases.tiled_sign(N_STREAM, shift)
        s.want["sign"][g] = s2 + o2
        s.src["sign"][g] = [_idx_dev(torch, idx), _dev(torch, m2), _dev(torch, a2)]
    for kind in ("verify", "sign"):
        assert s.want[kind]["x"] != s.want[kind]["y"]
    s.bufs = {kind: [torch.empty_like(a) for a in s.src[kind]["x"]] for kind in ("verify", "sign")}
    s.wb = sbv.secp256k1_schnorr_verify_workspace(N_STREAM)
    s.size = {"verify": N_STREAM, "sign": 65 * N_STREAM}
    s.outs = {kind: [torch.full((s.size[kind],), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(3)] for kind in ("verify", "sign")}
    s.works = [torch.full((s.wb + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    s.hosts = {kind: [torch.zeros(s.size[kind], dtype=torch.uint8).pin_memory() for _ in range(3)] for kind in ("verify", "sign")}
    s.stream, s.stream2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()                          # the fills above ran on the default stream

    def produce(kind, g, bufs=None):
        for dst, a in zip(bufs or s.bufs[kind], s.src[kind][g]):
            dst.copy_(a, non_blocking=True)

    def call(kind, k, bufs=None, work=0, stream=None):
        """the entry from the input buffers, then the copy of the result into pinned memory: all on one stream"""
        b, o = bufs or s.bufs[kind], s.outs[kind][k].data_ptr()
        sp = (stream or s.stream).cuda_stream
        if kind == "verify":
            sbv.secp256k1_schnorr_verify_stream(b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), N_STREAM, o, s.works[work].data_ptr(), s.wb, stream=sp)
        else:
            sbv.secp256k1_schnorr_sign_stream(s.recs.data_ptr(), s.n_keys, b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), N_STREAM, o,
                                              o + 64 * N_STREAM, stream=sp)
        s.hosts[kind][k].copy_(s.outs[kind][k], non_blocking=True)

    def check(kind, k, g, what):
        got, want = s.hosts[kind][k].numpy().tobytes(), s.want[kind][g]
        if got != want:
            other = s.want[kind]["x" if g == "y" else "y"]
            a, w = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
            what_else = "the OTHER generation's" if got == other else "a mixture: %d bytes differ, first at %d" % (int((a != w).sum()), int(np.flatnonzero(a != w)[0]))
            raise AssertionError("%s, %s: output %d is not generation %s's but %s" % (what, kind, k, g.upper(), what_else))
    s.produce, s.call, s.check = produce, call, check
    s.delay = Delay(torch)
    s.delay_ms = {}
    for kind in ("verify", "sign"):
        with torch.cuda.stream(s.stream):
            produce(kind, "x")
            call(kind, 0)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call(kind, 0)
            b.record()
            torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        s.delay_ms[kind] = min(DELAY_MAX_MS, max(DELAY_MIN_MS, DELAY_FACTOR * ms))
        check(kind, 0, "x", "warm call")
        print("\n[secp256k1 schnorr, stream order] one warm %s of %d: %.3f ms; delay %.1f ms" % (kind, N_STREAM, ms, s.delay_ms[kind]))
    return s


def _held_back(s, kind):
    """the delay on the current stream and an event behind it: still pending after the last enqueue = the GPU had everything queued first"""
    s.delay(s.delay_ms[kind])
    gate = s.torch.cuda.Event()
    gate.record()
    return gate


@pytest.mark.parametrize("kind", ["verify", "sign"])
@pytest.mark.parametrize("overwrite", [False, True], ids=["late_producer", "early_overwriter"])
def test_stream_late_producer_and_early_overwriter(streams, overwrite, kind):
    s, torch = streams, streams.torch
    with torch.cuda.stream(s.stream):
        s.produce(kind, "x")
        torch.cuda.synchronize()
        gate = _held_back(s, kind)
        s.produce(kind, "y")
        s.call(kind, 1)
        if overwrite:
            s.produce(kind, "x")
            s.hosts[kind][1].copy_(s.outs[kind][1], non_blocking=True)
        pending = not gate.query()
    torch.cuda.synchronize()
    assert pending, "the delay had run out before the last enqueue: the schedule proved nothing"
    s.check(kind, 1, "y", "early overwriter" if overwrite else "late producer")
    if overwrite:
        for dst, a in zip(s.bufs[kind], s.src[kind]["x"]):
            assert torch.equal(dst, a)


@pytest.mark.parametrize("kind", ["verify", "sign"])
def test_stream_x_y_x_back_to_back(streams, kind):
    s, torch = streams, streams.torch
    with torch.cuda.stream(s.stream):
        gate = _held_back(s, kind)
        for k, g in enumerate("xyx"):
            s.produce(kind, g)
            s.call(kind, k)
        pending = not gate.query()
    torch.cuda.synchronize()
    assert pending, "the delay had run out before the last enqueue: the schedule proved nothing"
    for k, g in enumerate("xyx"):
        s.check(kind, k, g, "X-Y-X")
    assert all(bool((w[s.wb:] == SENTINEL).all()) for w in s.works)


def test_two_verify_streams_two_workspaces_at_once(streams):
    """two calls that overlap: each on its own stream, inputs and workspace, both queued behind a delay, one synchronise at the end"""
    s, torch = streams, streams.torch
    bufs2 = [torch.empty_like(a) for a in s.src["verify"]["y"]]
    torch.cuda.synchronize()
    gates = []
    for st, g, k, bufs, work in ((s.stream, "x", 0, s.bufs["verify"], 0), (s.stream2, "y", 1, bufs2, 1)):
        with torch.cuda.stream(st):
            gates.append(_held_back(s, "verify"))
            s.produce("verify", g, bufs)
            s.call("verify", k, bufs, work, st)
    pending = [not g.query() for g in gates]
    torch.cuda.synchronize()
    assert all(pending), "a delay had run out before the last enqueue: the schedule proved nothing"
    s.check("verify", 0, "x", "two streams")
    s.check("verify", 1, "y", "two streams")
    assert all(bool((w[s.wb:] == SENTINEL).all()) for w in s.works)


# ---- round trip -----------------------------------------------------------------------------------------------------------------------
def test_round_trip_on_the_device():
    """expand -> sign -> spoil every third signature in one bit -> verify, 8 229 items; nothing leaves the device in between"""
    import torch
    n, nk = N_STREAM, 37
    keys = b"".join(cases.be32(int.from_bytes(hashlib.sha256(b"k256-schnorr-roundtrip%d" % i).digest(), "big") % (N - 1) + 1) for i in range(nk))
    rng = random.Random(0x8229)
    msgs, aux = rng.randbytes(32 * n), rng.randbytes(32 * n)
    idx = [(5 * i + i // nk) % nk for i in range(n)]
    d_keys, d_msg, d_aux, d_idx = _dev(torch, keys), _dev(torch, msgs), _dev(torch, aux), _idx_dev(torch, idx)
    d_rec, d_pk, d_eok = (torch.zeros(k, dtype=torch.uint8, device="cuda") for k in (64 * nk, 32 * nk, nk))
    d_sig, d_sok, d_vok = (torch.zeros(k, dtype=torch.uint8, device="cuda") for k in (64 * n, n, n))
    wb = sbv.secp256k1_schnorr_verify_workspace(n)
    d_work = torch.zeros(wb, dtype=torch.uint8, device="cuda")
    spoil_bit = torch.from_numpy(np.array([rng.randrange(512) if i % 3 == 2 else -1 for i in range(n)], dtype=np.int64)).cuda()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    sp = st.cuda_stream
    with torch.cuda.stream(st):
        sbv.secp256k1_schnorr_expand_keys_stream(d_keys.data_ptr(), nk, d_rec.data_ptr(), d_pk.data_ptr(), d_eok.data_ptr(), sp)
        sbv.secp256k1_schnorr_sign_stream(d_rec.data_ptr(), nk, d_idx.data_ptr(), d_msg.data_ptr(), d_aux.data_ptr(), n, d_sig.data_ptr(), d_sok.data_ptr(), sp)
        rows = torch.nonzero(spoil_bit >= 0).flatten()
        bits = spoil_bit[rows]
        flat = rows * 64 + bits // 8
        d_sig[flat] = d_sig[flat] ^ (1 << (bits % 8)).to(torch.uint8)
        d_pks = d_pk.view(nk, 32)[d_idx.long()].contiguous()
        sbv.secp256k1_schnorr_verify_stream(d_pks.data_ptr(), d_msg.data_ptr(), d_sig.data_ptr(), n, d_vok.data_ptr(), d_work.data_ptr(), wb, sp)
    torch.cuda.synchronize()
    assert bool((d_eok == 1).all()) and bool((d_sok == 1).all())
    assert d_vok.cpu().numpy().tobytes() == bytes(0 if i % 3 == 2 else 1 for i in range(n))
    # three of the signatures against the model, from the private keys
    sigs = d_sig.cpu().numpy().tobytes()
    for i in (0, 1, n - 2):
        assert i % 3 != 2
        rec, _, _ = cases.expand(int.from_bytes(keys[32 * idx[i]:32 * idx[i] + 32], "big"))
        assert cases.sign(rec, msgs[32 * i:32 * i + 32], aux[32 * i:32 * i + 32]) == (sigs[64 * i:64 * i + 64], 1)


def test_host_verify_schnorr_on_the_gpu_backend_equals_the_cpu_backend(model):
    """Verifier::VerifySchnorr and the backend's signer: one device call on the GPU backend, a loop over the host forms on the CPU one"""
    host = hostlib.load()
    C = ctypes.c_char_p
    host.sbvh_verify_schnorr.argtypes = [hostlib.V, C, C, C, ctypes.c_size_t, C]
    host.sbvh_sign_schnorr.argtypes = [hostlib.V, C, ctypes.c_uint32, ctypes.c_void_p, C, C, ctypes.c_size_t, C, C]
    cb = hostlib.BACKEND_FN(lambda tuples, n, bitmap, user: 0)
    pks, msgs, sigs = cases.arrays()
    n = len(model)
    idx, m2, a2, s2, o2 = cases.tiled_sign(700, 3)
    got = []
    for kind in (0, 1):                                                 # libsbv.so on device 0, then the callback backend
        h = host.sbvh_verifier_new_scheme(2, kind, 0, cb, None, 64, 50, 0)
        try:
            ok = ctypes.create_string_buffer(n)
            assert host.sbvh_verify_schnorr(h, pks, msgs, sigs, n, ok) == hostlib.OK
            out, sok = ctypes.create_string_buffer(64 * 700), ctypes.create_string_buffer(700)
            assert host.sbvh_sign_schnorr(h, _records(), 300, (ctypes.c_uint32 * 700)(*idx), m2, a2, 700, out, sok) == 0
            got.append((ok.raw, out.raw, sok.raw))
        finally:
            host.sbvh_verifier_free(h)
    assert got[0] == got[1]
    assert got[0] == (model, s2, o2)
