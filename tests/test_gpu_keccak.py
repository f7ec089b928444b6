"""GPU tier of Keccak-256 and the Ethereum-style addresses (include/sbv.h: sbv_keccak256_msgs, sbv_secp256k1_addresses,
sbv_secp256k1_recover_addresses, their _stream forms and sbv_debug_keccak_op), through the C-ABI and the Python wrapper.

Every byte the device writes is compared with the Python-integer model of tests/keccak_cases.py (the cases of the CPU tier,
tests/test_keccak_cpu.py), which that tier holds to hashlib and to the published values.  Large batches tile the case sets with a
rotation, so their expected values are the model's too.  The _stream entries run under callers that do not synchronise — late
producer, early overwriter, X-Y-X — with the delay of tests/test_gpu_stream_order.py."""
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
import k256_recover_cases as rc
import k256_sign_cases as sc
import keccak_cases as kc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, LOW_S = rc.N, rc.LOW_S
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
    print("\n[keccak] wall time of this file: %.1f s" % (time.perf_counter() - T0))


@pytest.fixture(scope="module")
def model():
    """the expected addresses of every recovery case, from the Python-integer models, once"""
    t = time.perf_counter()
    exp = kc.recover_expected_all()
    print("\n[keccak] the model of %d recovery cases: %.1f s" % (len(exp), time.perf_counter() - t))
    return exp


def _dev(torch, data, dtype=np.uint8):
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=dtype).copy()).cuda()


def _bytes(t):
    return t.cpu().numpy().tobytes()


# ---- byte for byte against the model ---------------------------------------------------------------------------------------------------
def test_every_message_against_the_model():
    assert sbv.keccak256_msgs(kc.messages()) == kc.message_digests()
    blob, offs = kc.packed_messages()
    assert sbv.keccak256_msgs(blob, offs) == b"".join(kc.message_digests())
    g = kc.golden()
    assert [d.hex() for d in sbv.keccak256_msgs([bytes.fromhex(v["msg"]) for v in g["digests"]])] == [v["keccak256"] for v in g["digests"]]
    assert sbv.keccak256_msgs(None, [0, 0, 0]) == kc.keccak256(b"") * 2              # no buffer when every message is empty
    assert sbv.keccak256_msgs([]) == []


def test_every_permutation_state_against_the_model():
    got = sbv.debug_keccak_op(0, kc.states())
    bad = [i for i, (g, w) in enumerate(zip(got, kc.states_after())) if g != w]
    assert not bad, (len(bad), bad[:8])
    for op in (1, -1, 7):
        with pytest.raises(sbv.SbvError) as e:
            sbv.debug_keccak_op(op, kc.states()[:1])
        assert e.value.code == EINVAL
    assert sbv.debug_keccak_op(0, []) == []


def test_every_key_case_against_the_model():
    assert sbv.secp256k1_addresses(b"".join(kc.key_cases())) == b"".join(kc.key_addresses())
    g = kc.golden()
    pubs, ok = sbv.secp256k1_pubkeys(b"".join(bytes.fromhex(v["d"]) for v in g["addresses"]))
    assert ok == b"\x01\x01" and sbv.secp256k1_addresses(pubs).hex() == "".join(v["address"] for v in g["addresses"])
    assert sbv.secp256k1_addresses(b"") == b""


@pytest.mark.parametrize("flags", [0, LOW_S])
def test_every_recovery_case_against_the_model(model, flags):
    idx, sigs, rid, digs, want_addrs, want_ok = kc.recover_by_flags(flags)
    addrs, ok = sbv.secp256k1_recover_addresses(sigs, rid, digs, low_s=bool(flags))
    bad = [(i, rc.cases()[i][0]) for k, i in enumerate(idx) if (addrs[20 * k:20 * k + 20], ok[k]) != model[i]]
    assert not bad, (flags, len(bad), bad[:8])
    assert (addrs, ok) == (want_addrs, want_ok) and min(ok) == 0 and max(ok) == 1
    assert all(addrs[20 * k:20 * k + 20] == bytes(20) for k in range(len(idx)) if not ok[k])


# ---- launch geometry: every byte, and nothing behind the last one --------------------------------------------------------------------
def _tiled_messages(n, shift):
    """n messages from the case set rotated by `shift`: (blob, offsets, digests)"""
    msgs, digs = kc.messages(), kc.message_digests()
    m = len(msgs)
    pick = [(shift + i) % m for i in range(n)]
    offs = [0]
    for k in pick:
        offs.append(offs[-1] + len(msgs[k]))
    return b"".join(msgs[k] for k in pick), offs, b"".join(digs[k] for k in pick)


def _tiled_keys(n, shift):
    keys, addrs = kc.key_cases(), kc.key_addresses()
    m = len(keys)
    pick = [(shift + i) % m for i in range(n)]
    return b"".join(keys[k] for k in pick), b"".join(addrs[k] for k in pick)


def _msgs_stream(torch, blob, offs, lead=1, stream=0):
    """the _stream entry with the messages `lead` bytes into their buffer (any alignment) and a sentinel behind the digests"""
    n = len(offs) - 1
    d_msgs = torch.full((lead + len(blob) + 1,), SENTINEL, dtype=torch.uint8, device="cuda")
    if blob:
        d_msgs[lead:lead + len(blob)] = _dev(torch, blob)
    d_off = _dev(torch, np.array(offs, dtype=np.uint64).tobytes())
    d_dig = torch.full((32 * n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert d_off.data_ptr() % 8 == 0
    torch.cuda.synchronize()
    sbv.keccak256_msgs_stream(d_msgs.data_ptr() + lead, d_off.data_ptr(), n, d_dig.data_ptr(), stream)
    torch.cuda.synchronize()
    return _bytes(d_dig)


def _addresses_stream(torch, pubs, stream=0):
    n = len(pubs) // 64
    d_pub = _dev(torch, pubs)
    d_addr = torch.full((20 * n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sbv.secp256k1_addresses_stream(d_pub.data_ptr(), n, d_addr.data_ptr(), stream)
    torch.cuda.synchronize()
    return _bytes(d_addr)


def _recover_stream(torch, n, sigs, rid, digs, flags, stream=0):
    """the _stream entry on fresh buffers with sentinels behind addrs, ok and the workspace: (addrs, ok, workspace tensor, its size)"""
    d_sig, d_rid, d_dig = _dev(torch, sigs), _dev(torch, rid), _dev(torch, digs)
    wb = sbv.secp256k1_recover_workspace(n)
    assert wb == min(n, LANES) * STRIP
    d_addr = torch.full((20 * n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_ok = torch.full((n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_work = torch.full((wb + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert d_work.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    sbv.secp256k1_recover_addresses_stream(d_sig.data_ptr(), d_rid.data_ptr(), d_dig.data_ptr(), n, d_addr.data_ptr(), d_ok.data_ptr(),
                                           d_work.data_ptr(), wb, low_s=bool(flags), stream=stream)
    torch.cuda.synchronize()
    return _bytes(d_addr), _bytes(d_ok), d_work, wb


def _check_recover_geometry(torch, n, flags, shift=0):
    sigs, rid, digs, want_addrs, want_ok = kc.recover_tiled(flags, n, shift)
    addrs, ok, d_work, wb = _recover_stream(torch, n, sigs, rid, digs, flags)
    if addrs[:20 * n] != want_addrs or ok[:n] != want_ok:
        bad = [i for i in range(n) if addrs[20 * i:20 * i + 20] != want_addrs[20 * i:20 * i + 20] or ok[i] != want_ok[i]]
        raise AssertionError("n = %d, flags %d: %d items differ, first %s" % (n, flags, len(bad), bad[:8]))
    assert addrs[20 * n:] == bytes([SENTINEL]) * 64, (n, "bytes behind the last address were written")
    assert ok[n:] == bytes([SENTINEL]) * 64, (n, "bytes behind the last ok were written")
    assert bool((d_work[wb:] == SENTINEL).all()), (n, "bytes behind the workspace were written")
    return sigs, rid, digs, want_addrs, want_ok


GEOMETRY = [1, 63, 64, 65, 255, 256, 257, 8229]


@pytest.mark.parametrize("n", GEOMETRY)
def test_launch_geometry_of_the_message_entry(n):
    import torch
    blob, offs, want = _tiled_messages(n, n)
    for lead in (1, 8):
        got = _msgs_stream(torch, blob, offs, lead)
        assert got[:32 * n] == want, (n, lead)
        assert got[32 * n:] == bytes([SENTINEL]) * 64, (n, "bytes behind the last digest were written")
    assert sbv.keccak256_msgs(blob, offs) == want                                   # the host-pointer form


@pytest.mark.parametrize("n", GEOMETRY)
def test_launch_geometry_of_the_address_entry(n):
    """the stride is 20 bytes: a lane that stored a sixth dword would spoil its neighbour, and the last one the sentinel"""
    import torch
    pubs, want = _tiled_keys(n, n)
    got = _addresses_stream(torch, pubs)
    assert got[:20 * n] == want, n
    assert got[20 * n:] == bytes([SENTINEL]) * 64, (n, "bytes behind the last address were written")
    assert sbv.secp256k1_addresses(pubs) == want


@pytest.mark.parametrize("n", GEOMETRY)
def test_launch_geometry_of_the_recovery_entry(model, n):
    import torch
    for flags in (0, LOW_S):
        sigs, rid, digs, want_addrs, want_ok = _check_recover_geometry(torch, n, flags, shift=n)
        if n <= 257:
            assert sbv.secp256k1_recover_addresses(sigs, rid, digs, low_s=bool(flags)) == (want_addrs, want_ok), (n, flags)


@pytest.mark.parametrize("n", [LANES - 1, LANES, LANES + 1, 2 * LANES + 3], ids=["lanes-1", "lanes", "lanes+1", "2lanes+3"])
def test_capped_grid_reuses_its_strips(model, n):
    """around the cap of the grid: the last lane idle, every lane once, lane 0 twice, every lane twice or three times"""
    import torch
    _check_recover_geometry(torch, n, LOW_S if n == LANES + 1 else 0, shift=3)


@pytest.mark.parametrize("flags", [0, LOW_S])
def test_recover_addresses_agrees_with_addresses_of_recover(flags):
    """the same inputs through the fused entry and through the two entries it stands for: ok byte for byte; the address is the hash of
    the other entry's key wherever ok is 1 (a refused item's key is 64 zero bytes, whose hash is not the 20 zero bytes written)"""
    n = 3000
    sigs, rid, digs, _, _ = kc.recover_tiled(flags, n, 17)
    addrs, ok = sbv.secp256k1_recover_addresses(sigs, rid, digs, low_s=bool(flags))
    pubs, pok = sbv.secp256k1_recover(sigs, rid, digs, low_s=bool(flags))
    hashed = sbv.secp256k1_addresses(pubs)
    assert ok == pok and 0 < sum(ok) < n
    for i in range(n):
        assert addrs[20 * i:20 * i + 20] == (hashed[20 * i:20 * i + 20] if ok[i] else bytes(20)), i


# ---- refused calls -------------------------------------------------------------------------------------------------------------------
def test_refused_calls_of_the_hash_entries():
    import torch
    lib = sbv.load()
    V, S = ctypes.c_void_p, ctypes.c_size_t
    lib.sbv_keccak256_msgs.argtypes = [V, V, S, V]
    lib.sbv_keccak256_msgs_stream.argtypes = [V, V, S, V, V]
    lib.sbv_secp256k1_addresses.argtypes = [V, S, V]
    lib.sbv_secp256k1_addresses_stream.argtypes = [V, S, V, V]
    msgs = ctypes.create_string_buffer(b"abcdef", 6)
    offs = (ctypes.c_uint64 * 3)(0, 3, 6)
    dig = ctypes.create_string_buffer(bytes([SENTINEL]) * 64, 64)
    assert lib.sbv_keccak256_msgs(msgs, None, 2, dig) == EINVAL
    assert lib.sbv_keccak256_msgs(msgs, offs, 2, None) == EINVAL
    assert lib.sbv_keccak256_msgs(None, offs, 2, dig) == EINVAL                      # bytes to hash but no buffer
    for bad in ((1, 3, 6), (0, 4, 3), (0, 3, 2), (5, 5, 5)):                        # not from 0, decreasing
        assert lib.sbv_keccak256_msgs(msgs, (ctypes.c_uint64 * 3)(*bad), 2, dig) == EINVAL, bad
    assert lib.sbv_keccak256_msgs(None, None, 0, None) == 0 and lib.sbv_keccak256_msgs(msgs, offs, 0, dig) == 0
    assert dig.raw == bytes([SENTINEL]) * 64                                        # refused calls and n = 0 wrote nothing
    assert lib.sbv_keccak256_msgs(msgs, offs, 2, dig) == 0 and dig.raw == kc.keccak256(b"abc") + kc.keccak256(b"def")
    pub = ctypes.create_string_buffer(kc.key_cases()[0], 64)
    adr = ctypes.create_string_buffer(bytes([SENTINEL]) * 20, 20)
    assert lib.sbv_secp256k1_addresses(None, 1, adr) == EINVAL and lib.sbv_secp256k1_addresses(pub, 1, None) == EINVAL
    assert lib.sbv_secp256k1_addresses(None, 0, None) == 0 and adr.raw == bytes([SENTINEL]) * 20
    assert lib.sbv_secp256k1_addresses(pub, 1, adr) == 0 and adr.raw == kc.key_addresses()[0]
    # the _stream forms: null pointers, the alignment of digests / keys / addresses (4) and of the offsets (8); messages at any address
    t = {k: torch.full((4096,), SENTINEL, dtype=torch.uint8, device="cuda") for k in ("msg", "off", "dig", "pub", "adr")}
    t["msg"][3:9] = _dev(torch, b"abcdef")
    t["off"][:24] = _dev(torch, np.array([0, 3, 6], dtype=np.uint64).tobytes())
    t["off"][32:56] = _dev(torch, np.array([0, 5, 2], dtype=np.uint64).tobytes())   # a decreasing pair, which only the device sees
    t["pub"][:64] = _dev(torch, kc.key_cases()[0])
    torch.cuda.synchronize()
    p = {k: v.data_ptr() for k, v in t.items()}
    assert p["off"] % 8 == 0
    good = [p["msg"] + 3, p["off"], 2, p["dig"], None]
    for pos in (1, 3):
        args = list(good)
        args[pos] = None
        assert lib.sbv_keccak256_msgs_stream(*args) == EINVAL, pos
    for off in (1, 2, 4):
        args = list(good)
        args[1] += off
        assert lib.sbv_keccak256_msgs_stream(*args) == EINVAL, off
    for off in (1, 2, 3):
        args = list(good)
        args[3] += off
        assert lib.sbv_keccak256_msgs_stream(*args) == EINVAL, off
    args = list(good)
    args[2] = 0
    assert lib.sbv_keccak256_msgs_stream(*args) == 0 and lib.sbv_keccak256_msgs_stream(None, None, 0, None, None) == 0
    goodp = [p["pub"], 1, p["adr"], None]
    for pos in (0, 2):
        args = list(goodp)
        args[pos] = None
        assert lib.sbv_secp256k1_addresses_stream(*args) == EINVAL, pos
        for off in (1, 2, 3):
            args = list(goodp)
            args[pos] += off
            assert lib.sbv_secp256k1_addresses_stream(*args) == EINVAL, (pos, off)
    assert lib.sbv_secp256k1_addresses_stream(p["pub"], 0, p["adr"], None) == 0
    torch.cuda.synchronize()
    assert bool((t["dig"] == SENTINEL).all()) and bool((t["adr"] == SENTINEL).all())       # refused calls wrote nothing
    assert lib.sbv_keccak256_msgs_stream(*good) == 0 and lib.sbv_secp256k1_addresses_stream(*goodp) == 0
    assert lib.sbv_keccak256_msgs_stream(p["msg"] + 3, p["off"] + 32, 2, p["dig"] + 64, None) == 0
    torch.cuda.synchronize()
    dg, ad = _bytes(t["dig"]), _bytes(t["adr"])
    assert dg[:64] == kc.keccak256(b"abc") + kc.keccak256(b"def") and ad[:20] == kc.key_addresses()[0] and ad[20:24] == bytes([SENTINEL]) * 4
    assert dg[64:128] == kc.keccak256(b"abcde") + bytes(32) and dg[128:132] == bytes([SENTINEL]) * 4      # the decreasing pair: 32 zero bytes
    # all messages empty: no message buffer at all
    t["off"][64:88] = 0
    assert lib.sbv_keccak256_msgs_stream(None, p["off"] + 64, 2, p["dig"] + 128, None) == 0
    torch.cuda.synchronize()
    assert _bytes(t["dig"])[128:192] == kc.keccak256(b"") * 2


def test_refused_calls_of_the_recovery_entry():
    import torch
    lib = sbv.load()
    V, S, U = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    lib.sbv_secp256k1_recover_addresses.argtypes = [V, V, V, S, U, V, V]
    lib.sbv_secp256k1_recover_addresses_stream.argtypes = [V, V, V, S, U, V, V, V, S, V]
    n = 3
    sigs, rid, digs, want_addrs, want_ok = kc.recover_tiled(0, n)
    assert want_ok == b"\x01" * n
    b_sig, b_rid, b_dig = (ctypes.create_string_buffer(x, len(x)) for x in (sigs, rid, digs))
    adr, okb = (ctypes.create_string_buffer(bytes([SENTINEL]) * k, k) for k in (20 * n, n))
    good = [b_sig, b_rid, b_dig, n, 0, adr, okb]
    for pos in (0, 1, 2, 5, 6):
        args = list(good)
        args[pos] = None
        assert lib.sbv_secp256k1_recover_addresses(*args) == EINVAL, pos
    for flags in (2, 3, 0x80000000, 0xFFFFFFFE):
        args = list(good)
        args[4] = flags
        assert lib.sbv_secp256k1_recover_addresses(*args) == EINVAL, flags
    assert lib.sbv_secp256k1_recover_addresses(b_sig, b_rid, b_dig, 0, 0, adr, okb) == 0                      # n = 0: nothing is written
    assert lib.sbv_secp256k1_recover_addresses(None, None, None, 0, 0, None, None) == 0
    assert (adr.raw, okb.raw) == (bytes([SENTINEL]) * 20 * n, bytes([SENTINEL]) * n)
    assert lib.sbv_secp256k1_recover_addresses(*good) == 0 and (adr.raw, okb.raw) == (want_addrs, want_ok)
    # the _stream form: the same rules, the 4-byte alignment of sigs, digests and addrs, the workspace's 16 bytes and its size
    t = {k: torch.full((4096,), SENTINEL, dtype=torch.uint8, device="cuda") for k in ("sig", "rid", "dig", "adr", "ok")}
    t["work"] = torch.full((n * STRIP + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    t["sig"][:64 * n] = _dev(torch, sigs)
    t["rid"][:n] = _dev(torch, rid)
    t["dig"][:32 * n] = _dev(torch, digs)
    torch.cuda.synchronize()
    p = {k: v.data_ptr() for k, v in t.items()}
    good = [p["sig"], p["rid"], p["dig"], n, 0, p["adr"], p["ok"], p["work"], n * STRIP, None]
    for pos in (0, 1, 2, 5, 6, 7):
        args = list(good)
        args[pos] = None
        assert lib.sbv_secp256k1_recover_addresses_stream(*args) == EINVAL, pos
    for pos in (0, 2, 5):
        for off in (1, 2):
            args = list(good)
            args[pos] += off
            assert lib.sbv_secp256k1_recover_addresses_stream(*args) == EINVAL, (pos, off)
    for off in (1, 4, 8):                                                # a misaligned workspace
        args = list(good)
        args[7] += off
        args[8] += 64 - off
        assert lib.sbv_secp256k1_recover_addresses_stream(*args) == EINVAL, off
    for short in (0, STRIP, n * STRIP - 1):                              # an undersized one
        args = list(good)
        args[8] = short
        assert lib.sbv_secp256k1_recover_addresses_stream(*args) == EINVAL, short
    for flags in (2, 0x80000000):
        args = list(good)
        args[4] = flags
        assert lib.sbv_secp256k1_recover_addresses_stream(*args) == EINVAL, flags
    args = list(good)
    args[3] = 0
    assert lib.sbv_secp256k1_recover_addresses_stream(*args) == 0
    torch.cuda.synchronize()
    assert bool((t["adr"] == SENTINEL).all()) and bool((t["ok"] == SENTINEL).all()) and bool((t["work"] == SENTINEL).all())       # refused calls wrote nothing
    args = list(good)
    args[1] += 1                                                        # odd addresses for the byte arrays are fine
    args[6] += 3
    t["rid"][1:1 + n] = _dev(torch, rid)
    assert lib.sbv_secp256k1_recover_addresses_stream(*args) == 0
    torch.cuda.synchronize()
    assert _bytes(t["adr"])[:20 * n + 4] == want_addrs + bytes([SENTINEL]) * 4 and _bytes(t["ok"])[3:3 + n] == want_ok
    with pytest.raises(sbv.SbvError):
        sbv.secp256k1_recover_addresses_stream(p["sig"], p["rid"], p["dig"], n, p["adr"], p["ok"], p["work"], n * STRIP, flags=4)


_FIRST_CALL = r"""
import ctypes, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import consensus_amd as sbv
sigs, rid, digs = (bytes.fromhex(a) for a in sys.argv[2:5])
n = len(rid)
dev = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()
d_sig, d_rid, d_dig = dev(sigs), dev(rid), dev(digs)
d_out = torch.zeros(21 * n, dtype=torch.uint8, device="cuda")
d_work = torch.zeros(1536 * n, dtype=torch.uint8, device="cuda")
d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
lib = sbv.load()
V, S = ctypes.c_void_p, ctypes.c_size_t
lib.sbv_secp256k1_recover_addresses_stream.argtypes = [V] * 3 + [S, ctypes.c_uint32] + [V] * 3 + [S, V]
lib.sbv_secp256k1_recover_addresses.argtypes = [ctypes.c_char_p] * 3 + [S, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p]
lib.sbv_keccak256_msgs_stream.argtypes = [V, V, S, V, V]
lib.sbv_secp256k1_addresses_stream.argtypes = [V, S, V, V]
lib.sbv_debug_keccak_op.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, S]
args = [d_sig.data_ptr(), d_rid.data_ptr(), d_dig.data_ptr(), n, 0, d_out.data_ptr(), d_out.data_ptr() + 20 * n, d_work.data_ptr(), 1536 * n, None]
print("before-init", lib.sbv_secp256k1_recover_addresses_stream(*args),
      lib.sbv_secp256k1_recover_addresses(sigs, rid, digs, n, 0, ctypes.create_string_buffer(20 * n), ctypes.create_string_buffer(n)),
      lib.sbv_keccak256_msgs_stream(None, d_off.data_ptr(), n, d_work.data_ptr(), None),
      lib.sbv_secp256k1_addresses_stream(d_sig.data_ptr(), n, d_work.data_ptr(), None),
      lib.sbv_debug_keccak_op(0, bytes(200), ctypes.create_string_buffer(200), 1))
sbv.init(0)
st = torch.cuda.Stream()
torch.cuda.synchronize()
sbv.secp256k1_recover_addresses_stream(d_sig.data_ptr(), d_rid.data_ptr(), d_dig.data_ptr(), n, d_out.data_ptr(), d_out.data_ptr() + 20 * n,
                                       d_work.data_ptr(), 1536 * n, stream=st.cuda_stream)
torch.cuda.synchronize()
print("out", d_out.cpu().numpy().tobytes().hex())
"""


def test_first_secp256k1_call_of_a_process_is_the_stream_address_recovery(model):
    """nothing has uploaded the comb of G before the _stream entry runs; before sbv_init the entries answer SBV_ENOTINIT"""
    n = 300
    sigs, rid, digs, want_addrs, want_ok = kc.recover_tiled(0, n, 5)
    r = subprocess.run([sys.executable, "-c", _FIRST_CALL, ROOT, sigs.hex(), rid.hex(), digs.hex()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = dict(ln.split(" ", 1) for ln in r.stdout.splitlines() if ln.startswith(("before-init", "out")))
    assert lines["before-init"] == " ".join(["%d" % ENOTINIT] * 5)
    assert bytes.fromhex(lines["out"]) == want_addrs + want_ok


# ---- the _stream entries under callers that do not synchronise -------------------------------------------------------------------------
N_STREAM = 8229
ENTRIES = ["msgs", "addresses", "recover"]


class _Sched:
    """one _stream entry on two generations of inputs: device-resident sources, the input buffers the entry reads, three outputs with
    pinned host copies; `launch(inputs, out, stream)` enqueues the entry"""

    def __init__(self, torch, name):
        self.torch, self.name = torch, name
        n = N_STREAM
        self.want, self.src = {}, {}
        if name == "msgs":
            for g, shift in (("x", 0), ("y", 131)):
                blob, offs, digs = _tiled_messages(n, shift)
                self.want[g] = digs
                self.src[g] = [_dev(torch, blob), _dev(torch, np.array(offs, dtype=np.uint64).tobytes())]
            size = max(a.numel() for g in "xy" for a in self.src[g][:1])
            for g in "xy":                                               # one size for both generations' message buffers
                pad = torch.zeros(size, dtype=torch.uint8, device="cuda")
                pad[:self.src[g][0].numel()] = self.src[g][0]
                self.src[g][0] = pad
            self.out_bytes = 32 * n

            def launch(b, out, stream):
                sbv.keccak256_msgs_stream(b[0].data_ptr(), b[1].data_ptr(), n, out.data_ptr(), stream.cuda_stream)
        elif name == "addresses":
            for g, shift in (("x", 0), ("y", 41)):
                pubs, addrs = _tiled_keys(n, shift)
                self.want[g] = addrs
                self.src[g] = [_dev(torch, pubs)]
            self.out_bytes = 20 * n

            def launch(b, out, stream):
                sbv.secp256k1_addresses_stream(b[0].data_ptr(), n, out.data_ptr(), stream.cuda_stream)
        else:
            for g, shift in (("x", 0), ("y", 401)):
                sigs, rid, digs, addrs, ok = kc.recover_tiled(0, n, shift)
                self.want[g] = addrs + ok
                self.src[g] = [_dev(torch, sigs), _dev(torch, rid), _dev(torch, digs)]
            self.out_bytes = 21 * n
            self.wb = sbv.secp256k1_recover_workspace(n)
            self.work = torch.full((self.wb + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")

            def launch(b, out, stream):
                o = out.data_ptr()
                sbv.secp256k1_recover_addresses_stream(b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), n, o, o + 20 * n, self.work.data_ptr(),
                                                       self.wb, stream=stream.cuda_stream)
        self.launch = launch
        w = self.out_bytes // n
        same = sum(self.want["x"][w * i:w * i + w] == self.want["y"][w * i:w * i + w] for i in range(n))
        assert same < n // 10, (name, same)
        self.bufs = [torch.empty_like(a) for a in self.src["x"]]
        self.outs = [torch.full((self.out_bytes,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(3)]
        self.hosts = [torch.zeros(self.out_bytes, dtype=torch.uint8).pin_memory() for _ in range(3)]
        self.stream = torch.cuda.Stream()
        torch.cuda.synchronize()                      # the fills above ran on the default stream

    def produce(self, g):
        for dst, a in zip(self.bufs, self.src[g]):
            dst.copy_(a, non_blocking=True)

    def call(self, k):
        """the entry from the input buffers, then the copy of the result into pinned memory: all on one stream"""
        self.launch(self.bufs, self.outs[k], self.stream)
        self.hosts[k].copy_(self.outs[k], non_blocking=True)

    def check(self, k, g, what):
        got, want = self.hosts[k].numpy().tobytes(), self.want[g]
        if got != want:
            other = self.want["x" if g == "y" else "y"]
            a, w = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
            kind = "the OTHER generation's" if got == other else "a mixture: %d bytes differ, first at %d" % (int((a != w).sum()), int(np.flatnonzero(a != w)[0]))
            raise AssertionError("%s, %s: output %d is not generation %s's but %s" % (self.name, what, k, g.upper(), kind))


@pytest.fixture(scope="module")
def schedules(model):
    import torch
    from test_gpu_stream_order import DELAY_FACTOR, DELAY_MAX_MS, DELAY_MIN_MS, Delay
    delay = Delay(torch)
    out = {}
    for name in ENTRIES:
        s = _Sched(torch, name)
        s.delay = delay
        with torch.cuda.stream(s.stream):
            s.produce("x")
            s.call(0)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            s.call(0)
            b.record()
            torch.cuda.synchronize()
        s.call_ms = a.elapsed_time(b)
        s.delay_ms = min(DELAY_MAX_MS, max(DELAY_MIN_MS, DELAY_FACTOR * s.call_ms))
        s.check(0, "x", "warm call")
        print("\n[keccak, stream order] %s: one warm call of %d: %.3f ms; delay %.1f ms" % (name, N_STREAM, s.call_ms, s.delay_ms))
        out[name] = s
    return out


def _held_back(s):
    """the delay on the current stream and an event behind it: still pending after the last enqueue = the GPU had everything queued first"""
    s.delay(s.delay_ms)
    gate = s.torch.cuda.Event()
    gate.record()
    return gate


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("overwrite", [False, True], ids=["late_producer", "early_overwriter"])
def test_stream_late_producer_and_early_overwriter(schedules, entry, overwrite):
    s = schedules[entry]
    torch = s.torch
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


@pytest.mark.parametrize("entry", ENTRIES)
def test_stream_x_y_x_back_to_back(schedules, entry):
    s = schedules[entry]
    torch = s.torch
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
    if entry == "recover":
        assert bool((s.work[s.wb:] == SENTINEL).all())


# ---- the whole path on the device ------------------------------------------------------------------------------------------------------
def test_round_trip_on_the_device():
    """messages -> keccak256_msgs_stream -> secp256k1_sign_batch_stream (low-S) -> recover_addresses_stream, 8 229 items on one stream
    with nothing copied back in between; the result equals addresses_stream(pubkeys_stream(keys)); every third signature is spoiled
    and yields another address or ok = 0"""
    import torch
    n, nk = N_STREAM, 37
    rng = random.Random(0x8229)
    keys = b"".join(sc.be32(int.from_bytes(hashlib.sha256(b"keccak-roundtrip%d" % i).digest(), "big") % (N - 1) + 1) for i in range(nk))
    msgs = [rng.randbytes(rng.randrange(0, 300)) for _ in range(n)]
    offs = [0]
    for m in msgs:
        offs.append(offs[-1] + len(m))
    idx = [(5 * i + i // nk) % nk for i in range(n)]
    d_keys, d_msgs = _dev(torch, keys), _dev(torch, b"".join(msgs))
    d_off = _dev(torch, np.array(offs, dtype=np.uint64).tobytes())
    d_idx = torch.from_numpy(np.array(idx, dtype=np.uint32).view(np.int32)).cuda()
    d_dig = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    d_sig, d_rid, d_sok = (torch.zeros(k, dtype=torch.uint8, device="cuda") for k in (64 * n, n, n))
    d_addr, d_rok = torch.zeros(20 * n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_kpub, d_kok, d_kaddr = (torch.zeros(k, dtype=torch.uint8, device="cuda") for k in (64 * nk, nk, 20 * nk))
    wb = sbv.secp256k1_recover_workspace(n)
    d_work = torch.zeros(wb, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    sp = st.cuda_stream
    with torch.cuda.stream(st):
        sbv.keccak256_msgs_stream(d_msgs.data_ptr(), d_off.data_ptr(), n, d_dig.data_ptr(), sp)
        sbv.secp256k1_sign_batch_stream(d_keys.data_ptr(), nk, d_idx.data_ptr(), d_dig.data_ptr(), n, d_sig.data_ptr(), d_rid.data_ptr(), d_sok.data_ptr(),
                                        low_s=True, stream=sp)
        d_sig.view(n, 64)[0::3, 40] ^= 1                                # every third signature spoiled, on the device, in s
        sbv.secp256k1_recover_addresses_stream(d_sig.data_ptr(), d_rid.data_ptr(), d_dig.data_ptr(), n, d_addr.data_ptr(), d_rok.data_ptr(),
                                               d_work.data_ptr(), wb, low_s=True, stream=sp)
        sbv.secp256k1_pubkeys_stream(d_keys.data_ptr(), nk, d_kpub.data_ptr(), d_kok.data_ptr(), sp)
        sbv.secp256k1_addresses_stream(d_kpub.data_ptr(), nk, d_kaddr.data_ptr(), sp)
    torch.cuda.synchronize()
    assert _bytes(d_dig)[:32 * 64] == b"".join(kc.keccak256(m) for m in msgs[:64])                           # the first 64 digests by the model
    assert bool((d_sok == 1).all()) and bool((d_kok == 1).all())
    want = d_kaddr.view(nk, 20)[d_idx.long()]
    same = (d_addr.view(n, 20) == want).all(dim=1)
    good = same & (d_rok == 1)
    spoiled = torch.zeros(n, dtype=torch.bool, device="cuda")
    spoiled[0::3] = True
    assert bool(good[~spoiled].all()), "a recovered address is not its signer's"
    assert not bool(good[spoiled].any()), "a spoiled signature still gave its signer's address"
    assert bool((d_addr.view(n, 20)[d_rok == 0] == 0).all())


# ---- above the C-ABI ---------------------------------------------------------------------------------------------------------------------
def test_host_recover_addresses_on_the_gpu_backend_equals_the_cpu_backend(model):
    """Verifier::RecoverAddresses and Keccak256Batch: one device call each on the GPU backend, a loop over the host forms on the CPU
    backend, v as 27..30"""
    host = hostlib.load()
    host.sbvh_recover_addresses.argtypes = [hostlib.V, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p]
    host.sbvh_keccak256_batch.argtypes = [hostlib.V, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p]
    cb = hostlib.BACKEND_FN(lambda tuples, n, bitmap, user: 0)
    idx, sigs, rid, digs, want_addrs, want_ok = kc.recover_by_flags(0)
    n = len(idx)
    blob = b"".join(sigs[64 * k:64 * k + 64] + bytes([rid[k] + 27 if rid[k] <= 3 else rid[k]]) for k in range(n))
    mblob, offs = kc.packed_messages()
    m = len(offs) - 1
    got = []
    for kind in (0, 1):                                                 # libsbv.so on device 0, then the callback backend
        h = host.sbvh_verifier_new_scheme(2, kind, 0, cb, None, 64, 50, 0)
        try:
            addrs, ok, dig = ctypes.create_string_buffer(20 * n), ctypes.create_string_buffer(n), ctypes.create_string_buffer(32 * m)
            assert host.sbvh_recover_addresses(h, blob, digs, n, addrs, ok) == hostlib.OK
            assert host.sbvh_keccak256_batch(h, mblob, (ctypes.c_uint64 * (m + 1))(*offs), m, dig) == hostlib.OK
            got.append((addrs.raw, ok.raw, dig.raw))
        finally:
            host.sbvh_verifier_free(h)
    assert got[0] == got[1] == (want_addrs, want_ok, b"".join(kc.message_digests()))


def test_smoke_passes():
    """start-up: __graft_entry__.smoke() in a process of its own, the Keccak step included"""
    r = subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.smoke()"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "smoke ok: Keccak-256" in r.stdout
