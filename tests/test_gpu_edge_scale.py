"""GPU tier (`-m gpu`): the edge classes AT FULL SCALE.  The golden vectors (range edges, e = 0 / e >= N,
keys off the curve / >= p / (0,0), Q = +-G, u1*G = +-u2*Q, R.x in [N, p), hash lengths, …) used to ride in batches of ~20 k
tuples: three sort tiles, one launch.  Here every P-256 tuple vector is replicated 64 times — so that its key repeats often
enough to take the table path — and spliced at pseudo-random positions into

  * the 2^20 headline batch (128 sort tiles, all eight XCD eighths of the key-sorted Q phase), and
  * a 2^21 + 2^19 + 37 batch (chunked at kMaxChunk = 2^21: the vectors land in both launches and in the ragged tail),

with the key-table cache off, warm (second pass over the same batch) and overflowing (capacity 256 < 1024 signer keys).
Every spliced verdict must equal the vector's pinned one and the oracle's, the rest of the bitmap the generator's (which the
whole-batch oracle / OpenSSL tests of test_gpu_configs.py pin).  The Ed25519 and secp256k1 sets get the same treatment in
their own 2^20 batches."""
import ctypes
import json
import os
import random

import sys

import numpy as np
import pytest

import consensus_amd as sbv

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
THREADS = os.cpu_count() or 1
COPIES = 64


@pytest.fixture(scope="module")
def gpu():
    sbv.init(0)
    yield sbv
    sbv.set_grouping(True, sbv.GROUP_MIN_BATCH_DEFAULT, 0, 0)
    sbv.key_cache(True, 4096)


def _splice(base, expect_bits, vectors, tuple_bytes, seed):
    """base: uint8[n * tuple_bytes] (copied), expect_bits: uint8[n] 0/1 (copied); every vector (blob, accept) is written COPIES
    times at positions drawn without replacement -> (batch, expected bits, positions per vector)."""
    n = len(expect_bits)
    batch = base.copy().reshape(n, tuple_bytes)
    want = expect_bits.copy()
    rng = random.Random(seed)
    pos = rng.sample(range(n), COPIES * len(vectors))
    where = []
    for k, (blob, accept) in enumerate(vectors):
        p = pos[k * COPIES:(k + 1) * COPIES]
        batch[p] = np.frombuffer(blob, dtype=np.uint8)
        want[p] = 1 if accept else 0
        where.append(p)
    return batch.reshape(-1), want, where


def _report(got_bits, want_bits, where, names):
    bad = np.nonzero(got_bits != want_bits)[0]
    if len(bad) == 0:
        return None
    spliced = {p: names[k] for k, ps in enumerate(where) for p in ps}
    return [(int(i), spliced.get(int(i), "base batch"), int(want_bits[i])) for i in bad[:12]], len(bad)


def _bits(bitmap_bytes, n):
    return np.unpackbits(np.frombuffer(bitmap_bytes, dtype=np.uint8), bitorder="little")[:n]


def _p256_vectors():
    vs = [v for v in json.load(open(os.path.join(GOLDEN, "p256_vectors.json")))["vectors"] if v["kind"] == "tuple"]
    return vs, [(bytes.fromhex(v["tuple"]), v["accept"]) for v in vs]


def _run_ptr(gpu, batch, n):
    got = np.zeros((n + 7) // 8, dtype=np.uint8)
    gpu.verify_batch_ptr(batch.ctypes.data, n, got.ctypes.data)
    return _bits(got.tobytes(), n)


def test_p256_edge_vectors_spliced_into_the_headline_batch_cache_off_warm_overflowing(gpu, oracle):
    import synth
    n = 1 << 20
    tuples, valid = synth.gen_batch(0x5B7F2026, n)
    vs, vecs = _p256_vectors()
    batch, want, where = _splice(tuples, _bits(valid.tobytes(), n), vecs, 160, 0xED6E)
    # the oracle's own opinion on every spliced tuple (the pinned `accept` values are its verdicts on the vectors; this guards the splice itself)
    for k in range(0, len(vecs), 17):
        assert oracle.sbvo_p256_verify_tuple(batch[160 * where[k][0]:160 * where[k][0] + 160].tobytes()) == (1 if vecs[k][1] else 0)
    names = [v["name"] for v in vs]
    gpu.set_grouping(True, 0, 32, 0)          # 64 copies clear a threshold of 32 with the sampled count to spare
    try:
        for label, setup in (("cache off", lambda: gpu.key_cache(False)),
                             ("cache cold then warm", lambda: gpu.key_cache(True, 4096)),
                             ("cache overflowing", lambda: (gpu.key_cache(False), gpu.key_cache(True, 256)))):
            setup()
            for rnd in range(2):
                got = _run_ptr(gpu, batch, n)
                assert _report(got, want, where, names) is None, (label, rnd, _report(got, want, where, names))
            groups, grouped, generic, rejected = gpu.last_group_stats()
            # with the cache on, one caller's 2^20 tuples go up in four pieces of 2^18 beside their own kernels (round 5): the statistics are the last piece's
            assert groups >= 1024 and grouped > (900000 if label == "cache off" else 225000), (label, groups, grouped, generic, rejected)
        # the all-distinct-keys kernel on the same spliced batch
        gpu.key_cache(False)
        gpu.set_grouping(False)
        got = _run_ptr(gpu, batch, n)
        assert _report(got, want, where, names) is None, ("grouping off", _report(got, want, where, names))
    finally:
        gpu.set_grouping(True, sbv.GROUP_MIN_BATCH_DEFAULT, 0, 0)
        gpu.key_cache(True, 4096)


def test_p256_edge_vectors_spliced_into_a_chunked_ragged_batch(gpu):
    import synth
    n1 = 1 << 20
    tuples, valid = synth.gen_batch(0x5B7F2026, n1)
    n = (1 << 21) + (1 << 19) + 37                         # two launches (2^21 + the rest) and a ragged tail
    base = np.concatenate([tuples, tuples, tuples[:160 * (n - 2 * n1)]])
    b1 = _bits(valid.tobytes(), n1)
    bits = np.concatenate([b1, b1, b1[:n - 2 * n1]])
    vs, vecs = _p256_vectors()
    batch, want, where = _splice(base, bits, vecs, 160, 0xC4A6)
    in_tail = sum(1 for ps in where for p in ps if p >= (1 << 21))
    assert in_tail > 1000                                  # the second launch got its share of edge tuples
    names = [v["name"] for v in vs]
    gpu.set_grouping(True, 0, 32, 0)
    try:
        for label, setup in (("cache off", lambda: gpu.key_cache(False)), ("cache on, capacity 256", lambda: gpu.key_cache(True, 256)),
                             ("cache on", lambda: (gpu.key_cache(False), gpu.key_cache(True, 4096)))):
            setup()
            for rnd in range(2):
                got = _run_ptr(gpu, batch, n)
                assert _report(got, want, where, names) is None, (label, rnd, _report(got, want, where, names))
    finally:
        gpu.set_grouping(True, sbv.GROUP_MIN_BATCH_DEFAULT, 0, 0)
        gpu.key_cache(True, 4096)


def test_ed25519_edge_vectors_spliced_into_2_20(gpu, oracle):
    import ed25519_py as ed
    oracle.sbvo_ed25519_gen_batch.argtypes = [ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_int]
    n = 1 << 20
    tup = np.zeros(128 * n, dtype=np.uint8)
    exp = np.zeros(n // 8, dtype=np.uint8)
    oracle.sbvo_ed25519_gen_batch(0x5B7F2026, n, 1024, 8, tup.ctypes.data, exp.ctypes.data, THREADS)
    vs = json.load(open(os.path.join(GOLDEN, "ed25519_vectors.json")))["vectors"]
    vecs = [(ed.pack_tuple(bytes.fromhex(v["pk"]), bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"])), v["accept"]) for v in vs]
    batch, want, where = _splice(tup, _bits(exp.tobytes(), n), vecs, 128, 0xED25)
    names = [v["name"] for v in vs]
    for grouping in (True, False):
        gpu.set_grouping(grouping, 0, 32 if grouping else 0, 0)
        try:
            got = np.zeros(n // 8, dtype=np.uint8)
            sbv._check(sbv.load().sbv_ed25519_verify_batch(ctypes.c_void_p(batch.ctypes.data), n, ctypes.c_void_p(got.ctypes.data)))
            rep = _report(_bits(got.tobytes(), n), want, where, names)
            assert rep is None, (grouping, rep)
        finally:
            gpu.set_grouping(True, sbv.GROUP_MIN_BATCH_DEFAULT, 0, 0)


def test_secp256k1_edge_vectors_spliced_into_2_20(gpu, oracle):
    oracle.sbvo_k256_gen_batch.argtypes = [ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_int]
    n = 1 << 20
    tup = np.zeros(160 * n, dtype=np.uint8)
    exp = np.zeros(n // 8, dtype=np.uint8)
    oracle.sbvo_k256_gen_batch(0x5B7F2026, n, 1024, 8, tup.ctypes.data, exp.ctypes.data, THREADS)
    vs = json.load(open(os.path.join(GOLDEN, "k256_vectors.json")))["vectors"]
    vecs = [(bytes.fromhex(v["tuple"]), v["accept"]) for v in vs]
    batch, want, where = _splice(tup, _bits(exp.tobytes(), n), vecs, 160, 0x256C1)
    got = np.zeros(n // 8, dtype=np.uint8)
    sbv._check(sbv.load().sbv_secp256k1_verify_batch(ctypes.c_void_p(batch.ctypes.data), n, ctypes.c_void_p(got.ctypes.data)))
    rep = _report(_bits(got.tobytes(), n), want, where, [v["name"] for v in vs])
    assert rep is None, rep


def test_ed25519_batches_leave_the_p256_key_cache_alone(gpu, oracle):
    """Regression (round 3, found by test order): the Ed25519 grouped step wrote its per-batch group verdicts into the array whose
    first bytes are the validity flags of the P-256 key-table cache, so an Ed25519 batch with a repeated undecodable key
    switched cached P-256 signers to "invalid" and every later signature of theirs was rejected.  P-256 warm -> Ed25519 batch
    with 64 copies of every golden vector (undecodable keys among them) -> the same P-256 batch, still warm, same verdicts."""
    import ed25519_py as ed
    oracle.sbvo_ed25519_gen_batch.argtypes = [ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_int]
    n = 1 << 18
    tup = ctypes.create_string_buffer(160 * n)
    exp = ctypes.create_string_buffer(n // 8)
    oracle.sbvo_gen_batch(0x1CE, n, 300, 6, tup, exp, THREADS)
    etup = np.zeros(128 * n, dtype=np.uint8)
    eexp = np.zeros(n // 8, dtype=np.uint8)
    oracle.sbvo_ed25519_gen_batch(0x1CF, n, 300, 6, etup.ctypes.data, eexp.ctypes.data, THREADS)
    vs = json.load(open(os.path.join(GOLDEN, "ed25519_vectors.json")))["vectors"]
    vecs = [(ed.pack_tuple(bytes.fromhex(v["pk"]), bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"])), v["accept"]) for v in vs]
    ebatch, ewant, ewhere = _splice(etup, _bits(eexp.tobytes(), n), vecs, 128, 0xED26)

    def p256():
        got = ctypes.create_string_buffer(n // 8)
        gpu.verify_batch_ptr(ctypes.addressof(tup), n, ctypes.addressof(got))
        return got.raw
    gpu.key_cache(False)
    gpu.key_cache(True, 4096)
    gpu.set_grouping(True, 0, 32, 0)
    try:
        assert p256() == exp.raw
        assert p256() == exp.raw
        entries, hits, misses, cap = gpu.key_cache_stats()
        assert hits >= 300 and misses == 0
        got = np.zeros(n // 8, dtype=np.uint8)
        sbv._check(sbv.load().sbv_ed25519_verify_batch(ctypes.c_void_p(ebatch.ctypes.data), n, ctypes.c_void_p(got.ctypes.data)))
        assert _report(_bits(got.tobytes(), n), ewant, ewhere, [v["name"] for v in vs]) is None
        assert p256() == exp.raw                       # still warm, still right
        entries, hits, misses, cap = gpu.key_cache_stats()
        assert hits >= 300 and misses == 0
    finally:
        gpu.set_grouping(True, sbv.GROUP_MIN_BATCH_DEFAULT, 0, 0)


CHUNKED_N = (1 << 21) + (1 << 19) + 37        # two launches of kMaxChunk = 2^21 tuples and a ragged tail


@pytest.fixture(scope="module")
def chunked(gpu, oracle):
    """A generated batch of 2^16 (64 signers, every 8th signature corrupted) per scheme, tiled up to CHUNKED_N records; the keyed forms
    over its registered keys -> {scheme: (host-pointer entry, device-pointer entry, dominant kernel reported, inputs, expected bitmap)}."""
    base = 1 << 16
    reps = -(-CHUNKED_N // base)

    def gen(fn, rec_bytes, seed):
        fn.argtypes = [ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        tup = np.zeros(rec_bytes * base, dtype=np.uint8)
        exp = np.zeros(base // 8, dtype=np.uint8)
        fn(seed, base, 64, 8, tup.ctypes.data, exp.ctypes.data, THREADS)
        want = np.packbits(np.tile(_bits(exp.tobytes(), base), reps)[:CHUNKED_N], bitorder="little")
        return np.tile(tup.reshape(base, rec_bytes), (reps, 1))[:CHUNKED_N], want

    def slots(keys, register):
        uniq, inv = np.unique(keys, axis=0, return_inverse=True)
        return np.array(register([k.tobytes() for k in uniq]), dtype=np.uint32)[inv.reshape(-1)]

    lib = sbv.load()
    p256, p256_want = gen(oracle.sbvo_gen_batch, 160, 0xC4A7)
    ed, ed_want = gen(oracle.sbvo_ed25519_gen_batch, 128, 0xC4A8)
    k256, k256_want = gen(oracle.sbvo_k256_gen_batch, 160, 0xC4A9)
    gpu.clear_keys()
    gpu.ed25519_clear_keys()
    try:
        yield {
            "p256": (lib.sbv_p256_verify_batch, lib.sbv_p256_verify_batch_dev, True, [p256], p256_want),
            "ed25519": (lib.sbv_ed25519_verify_batch, lib.sbv_ed25519_verify_batch_dev, True, [ed], ed_want),
            "secp256k1": (lib.sbv_secp256k1_verify_batch, lib.sbv_secp256k1_verify_batch_dev, True, [k256], k256_want),
            "p256 keyed": (lib.sbv_p256_verify_batch_keyed, lib.sbv_p256_verify_batch_keyed_dev, False,
                           [p256[:, :96], slots(p256[:, 96:], gpu.register_keys)], p256_want),
            "ed25519 keyed": (lib.sbv_ed25519_verify_batch_keyed, lib.sbv_ed25519_verify_batch_keyed_dev, False,
                              [np.concatenate([ed[:, :64], ed[:, 96:]], axis=1), slots(ed[:, 64:96], gpu.ed25519_register_keys)], ed_want),
        }
    finally:
        gpu.clear_keys()
        gpu.ed25519_clear_keys()


def _on_device(arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).cuda() for a in arrays]


def _dev_call(entry, d_inputs, n):
    import torch
    entry.argtypes = [ctypes.c_void_p] * len(d_inputs) + [ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    d_b = torch.zeros((n + 7) // 8, dtype=torch.uint8, device="cuda")
    sbv._check(entry(*[ctypes.c_void_p(x.data_ptr()) for x in d_inputs], ctypes.c_size_t(n), ctypes.c_void_p(d_b.data_ptr()),
                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return d_b.cpu().numpy()


@pytest.mark.parametrize("scheme", ["ed25519", "secp256k1", "p256 keyed", "ed25519 keyed"])
def test_chunked_batches_through_the_host_and_device_entries(chunked, scheme):
    """More records than one launch holds (kMaxChunk = 2^21) through the host-pointer and the device-pointer entry: both walk the
    batch in chunks, and the bitmap equals the tiled batch's verdicts, ragged tail included."""
    host, dev, _, inputs, want = chunked[scheme]
    inputs = [np.ascontiguousarray(a) for a in inputs]
    host.argtypes = [ctypes.c_void_p] * len(inputs) + [ctypes.c_size_t, ctypes.c_void_p]
    got = np.zeros((CHUNKED_N + 7) // 8, dtype=np.uint8)
    sbv._check(host(*[ctypes.c_void_p(a.ctypes.data) for a in inputs], ctypes.c_size_t(CHUNKED_N), ctypes.c_void_p(got.ctypes.data)))
    assert (got == want).all(), (scheme, "host", np.nonzero(got != want)[0][:8])
    got = _dev_call(dev, _on_device(inputs), CHUNKED_N)
    assert (got == want).all(), (scheme, "device", np.nonzero(got != want)[0][:8])


@pytest.mark.parametrize("scheme", ["p256", "p256 keyed", "ed25519", "ed25519 keyed", "secp256k1"])
def test_profiling_levels_of_the_device_entries(gpu, chunked, scheme):
    """include/sbv.h, sbv_profile_enable: level 2 records only the pairs around the dominant kernel's launches (what bench.py keeps in
    its timed region), level 1 also an event triple per launch of the step.  At both levels every launch of the dominant kernel of the
    grouped P-256, Ed25519 and secp256k1 steps counts (one per chunk of windows: 1 to SBV_GROUP_MAX_CHUNKS = 4 per launch of the step)."""
    _, dev, dominant, inputs, _ = chunked[scheme]
    d_inputs = _on_device(inputs)
    launches = -(-CHUNKED_N // (1 << 21))
    _dev_call(dev, d_inputs, CHUNKED_N)            # tables and buffers set up outside the profiled calls
    gpu.profile_read_dominant()
    gpu.profile_read()
    seen = {}
    try:
        for level in (2, 1):
            gpu.profile_enable(level)
            _dev_call(dev, d_inputs, CHUNKED_N)
            seen[level] = (gpu.profile_read_dominant()[1], gpu.profile_read()[2])
    finally:
        gpu.profile_enable(False)
    assert seen[2][1] == 0 and seen[1][1] == launches, (scheme, seen)
    for dom, _ in seen.values():
        assert (launches <= dom <= 4 * launches) if dominant else dom == 0, (scheme, seen)
