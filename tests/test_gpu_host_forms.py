"""GPU tier of the buffer scope behind the host-pointer sign / Schnorr entries (consensus_amd/csrc/call_buffers.h): every optional host
pointer, absent and present, at sizes around a wavefront and a workgroup.

The host-pointer form of an entry uploads, launches the kernel of its `_stream` form, downloads and waits; an optional argument (key_index,
recid, aux, the pks of both expand entries, the ok of lift) that is NULL gets no device buffer and the kernel a null pointer.  So for each
combination the host form must return the bytes its `_stream` form writes into the caller's device buffers.  What those bytes have to be
is pinned elsewhere (tests/test_gpu_sign.py, test_gpu_k256_sign.py, test_gpu_k256_schnorr.py, test_gpu_k256_schnorr_keyed.py,
test_gpu_ed25519_sign.py); the Python bindings always pass recid, ok and pks, so the host forms are called through ctypes here."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

import consensus_amd as sbv
import ed_sign_cases as ed_cases
import p256_sign_cases as p256_cases

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 65, 257]
NK = 5
C, V, S, U32 = ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32


@pytest.fixture(scope="module", autouse=True)
def _init():
    sbv.init(0)


def _scalars(label, count=NK):
    """32-byte big-endian scalars well inside [1, 2^252]: valid private keys of all three schemes' entries"""
    return b"".join((int.from_bytes(hashlib.sha256(label + b"%d" % i).digest(), "big") >> 4 | 1).to_bytes(32, "big") for i in range(count))


def _index(n, nk=NK):
    rng = random.Random(0xCB + n)
    return [rng.randrange(nk) for _ in range(n)]


def _dev(data, dtype=np.uint8):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=dtype).copy()).cuda()


def _dev_index(index):
    import torch
    return torch.from_numpy(np.array(index, dtype=np.uint32).view(np.int32)).cuda()


def _out(nbytes):
    import torch
    return torch.zeros((max(1, nbytes),), dtype=torch.uint8, device="cuda")


def _bytes(t, nbytes):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().tobytes()[:nbytes]


def _host(name, argtypes, *args):
    fn = getattr(sbv.load(), name)
    fn.argtypes = argtypes
    rc = fn(*args)
    assert rc == 0, (name, rc, sbv.load().sbv_last_error())


@pytest.mark.parametrize("n", SIZES)
def test_p256_sign_key_index(n):
    keys, digests, index = _scalars(b"p256"), random.Random(n).randbytes(32 * n), _index(n)
    d_keys, d_dig, d_idx = _dev(keys), _dev(digests), _dev_index(index)
    for idx in (None, index):
        d_sig, d_ok = _out(64 * n), _out(n)
        sbv.sign_batch_dev(d_keys.data_ptr(), NK, d_idx.data_ptr() if idx else 0, d_dig.data_ptr(), n, d_sig.data_ptr(), d_ok.data_ptr())
        sigs, ok = ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(n)
        _host("sbv_p256_sign_batch", [C, U32, V, C, S, C, C], keys, NK, (U32 * n)(*idx) if idx else None, digests, n, sigs, ok)
        assert (sigs.raw, ok.raw) == (_bytes(d_sig, 64 * n), _bytes(d_ok, n)) and ok.raw == b"\x01" * n, (n, idx is None)


def test_p256_sign_then_verify_at_once():
    """the call after a host-form signer finds the context's stream idle and its signatures good"""
    n = 65
    ds = [int.from_bytes(hashlib.sha256(b"p256-sv%d" % i).digest(), "big") % (p256_cases.N - 1) + 1 for i in range(NK)]
    pubs = [p256_cases.pubkey(d) for d in ds]
    digests = random.Random(0x5F).randbytes(32 * n)
    sigs, ok = sbv.sign_batch(b"".join(p256_cases.be32(d) for d in ds), digests)
    bitmap = sbv.verify_batch(b"".join(sigs[64 * i:64 * i + 64] + digests[32 * i:32 * i + 32] + pubs[i % NK] for i in range(n)), n)
    assert ok == b"\x01" * n and sbv.bitmap_to_list(bitmap, n) == [True] * n


@pytest.mark.parametrize("n", SIZES)
def test_secp256k1_sign_key_index_and_recid(n):
    keys, digests, index = _scalars(b"k256"), random.Random(n).randbytes(32 * n), _index(n)
    d_keys, d_dig, d_idx = _dev(keys), _dev(digests), _dev_index(index)
    for idx in (None, index):
        for want_recid in (False, True):
            d_sig, d_rid, d_ok = _out(64 * n), _out(n), _out(n)
            sbv.secp256k1_sign_batch_stream(d_keys.data_ptr(), NK, d_idx.data_ptr() if idx else 0, d_dig.data_ptr(), n, d_sig.data_ptr(),
                                            d_rid.data_ptr() if want_recid else 0, d_ok.data_ptr())
            sigs, rid, ok = ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(n), ctypes.create_string_buffer(n)
            _host("sbv_secp256k1_sign_batch", [C, U32, V, C, S, U32, C, C, C], keys, NK, (U32 * n)(*idx) if idx else None, digests, n, 0,
                  sigs, rid if want_recid else None, ok)
            assert (sigs.raw, rid.raw, ok.raw) == (_bytes(d_sig, 64 * n), _bytes(d_rid, n), _bytes(d_ok, n)), (n, idx is None, want_recid)
            assert ok.raw == b"\x01" * n and (want_recid or rid.raw == bytes(n))         # an unwanted recid is not written


@pytest.mark.parametrize("n", SIZES)
def test_schnorr_expand_pks_and_sign_key_index_and_aux(n):
    keys = _scalars(b"schnorr", n)
    d_keys = _dev(keys)
    records = None
    for want_pks in (False, True):
        d_exp, d_pk, d_ok = _out(64 * n), _out(32 * n), _out(n)
        sbv.secp256k1_schnorr_expand_keys_stream(d_keys.data_ptr(), n, d_exp.data_ptr(), d_pk.data_ptr() if want_pks else 0, d_ok.data_ptr())
        exp, pks, ok = ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(32 * n), ctypes.create_string_buffer(n)
        _host("sbv_secp256k1_schnorr_expand_keys", [C, S, C, C, C], keys, n, exp, pks if want_pks else None, ok)
        assert (exp.raw, pks.raw, ok.raw) == (_bytes(d_exp, 64 * n), _bytes(d_pk, 32 * n), _bytes(d_ok, n)), (n, want_pks)
        assert ok.raw == b"\x01" * n and (pks.raw != bytes(32 * n)) == want_pks
        records = exp.raw
    nk = min(NK, n)                                                                      # sign under the first records
    msgs, aux, index = random.Random(n).randbytes(32 * n), random.Random(n + 1).randbytes(32 * n), _index(n, nk)
    d_rec, d_msg, d_aux, d_idx = _dev(records[:64 * nk]), _dev(msgs), _dev(aux), _dev_index(index)
    for idx in (None, index):
        for a in (None, aux):
            d_sig, d_ok = _out(64 * n), _out(n)
            sbv.secp256k1_schnorr_sign_stream(d_rec.data_ptr(), nk, d_idx.data_ptr() if idx else 0, d_msg.data_ptr(), d_aux.data_ptr() if a else 0, n,
                                              d_sig.data_ptr(), d_ok.data_ptr())
            sigs, ok = ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(n)
            _host("sbv_secp256k1_schnorr_sign", [C, U32, V, C, C, S, C, C], records[:64 * nk], nk, (U32 * n)(*idx) if idx else None, msgs, a, n,
                  sigs, ok)
            assert (sigs.raw, ok.raw) == (_bytes(d_sig, 64 * n), _bytes(d_ok, n)) and ok.raw == b"\x01" * n, (n, idx is None, a is None)


@pytest.mark.parametrize("n", SIZES)
def test_schnorr_lift_ok(n):
    pks = random.Random(0x11F7 + n).randbytes(32 * n)                                    # about half of all x are on the curve
    d_pks = _dev(pks)
    for want_ok in (False, True):
        d_keys, d_ok = _out(64 * n), _out(n)
        sbv.secp256k1_schnorr_lift_keys_stream(d_pks.data_ptr(), n, d_keys.data_ptr(), d_ok.data_ptr() if want_ok else 0)
        keys64, ok = ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(n)
        _host("sbv_secp256k1_schnorr_lift_keys", [C, S, C, C], pks, n, keys64, ok if want_ok else None)
        assert (keys64.raw, ok.raw) == (_bytes(d_keys, 64 * n), _bytes(d_ok, n)), (n, want_ok)
        assert want_ok or ok.raw == bytes(n)


@pytest.mark.parametrize("n", SIZES)
def test_ed25519_expand_pks_and_sign_key_index(n):
    seeds = b"".join(ed_cases.seeds(n))
    d_seeds = _dev(seeds)
    for want_pks in (False, True):
        d_exp, d_pk = _out(96 * n), _out(32 * n)
        sbv.ed25519_expand_keys_stream(d_seeds.data_ptr(), n, d_exp.data_ptr(), d_pk.data_ptr() if want_pks else 0)
        exp, pks = ctypes.create_string_buffer(96 * n), ctypes.create_string_buffer(32 * n)
        _host("sbv_ed25519_expand_keys", [C, S, C, C], seeds, n, exp, pks if want_pks else None)
        assert (exp.raw, pks.raw) == (_bytes(d_exp, 96 * n), _bytes(d_pk, 32 * n)), (n, want_pks)
        assert (pks.raw != bytes(32 * n)) == want_pks
    nk = min(NK, n)                                                                      # sign under the first records
    records = exp.raw[:96 * nk]
    rng = random.Random(0xED + n)
    msgs = [rng.randbytes(rng.randrange(200) if i else 0) for i in range(n)]             # n = 1: no message bytes at all
    blob = b"".join(msgs)
    offsets = np.cumsum([0] + [len(m) for m in msgs], dtype=np.uint64)
    index = _index(n, nk)
    d_rec, d_msgs, d_off, d_idx = _dev(records), _dev(blob + bytes(16)), _dev(offsets.tobytes(), np.int64), _dev_index(index)
    for idx in (None, index):
        d_sig, d_ok = _out(64 * n), _out(n)
        sbv.ed25519_sign_msgs_stream(d_rec.data_ptr(), nk, d_idx.data_ptr() if idx else 0, d_msgs.data_ptr(), d_off.data_ptr(), n, d_sig.data_ptr(),
                                     d_ok.data_ptr())
        sigs, ok = ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(n)
        _host("sbv_ed25519_sign_msgs", [C, U32, V, C, ctypes.POINTER(ctypes.c_uint64), S, C, C], records, nk, (U32 * n)(*idx) if idx else None, blob,
              (ctypes.c_uint64 * (n + 1))(*[int(o) for o in offsets]), n, sigs, ok)
        assert (sigs.raw, ok.raw) == (_bytes(d_sig, 64 * n), _bytes(d_ok, n)) and ok.raw == b"\x01" * n, (n, idx is None)
