"""GPU tier of the 32-bit canonical table store and the shortened comb ends: the unit ops of tools/devunit_trim.hip compiled by
hipcc -O3 for gfx950 from the product's headers, one case per lane, 4 096 lanes per op, against Python big integers
(tests/trim_cases.py: the generators and references of tests/test_emul_trim.py); then the product library end to end on the four
paths that store or walk through the changed code, against the generator's expected bitmap and the oracle.

One process, one launch at a time.  A launch that returns a HIP error fails its test and every later test of the module is
skipped: nothing more is launched on a device that has just faulted."""
import ctypes
import os
import random

import numpy as np
import pytest

import arith_cases as ac
import consensus_amd as sbv
import trim_cases as tc

pytestmark = pytest.mark.gpu
LANES = 4096
THREADS = min(os.cpu_count() or 1, 16)


class Device:
    def __init__(self, lib):
        self.lib = lib
        self.faulted = None


@pytest.fixture(scope="module")
def dev():
    so = os.path.join(ac.ROOT, "tools", "libsbv_devunit_trim.so")
    if not os.path.exists(so):
        pytest.skip("tools/libsbv_devunit_trim.so not built (make -C tools)")
    sbv.load()                                            # the product library first: it settles which HIP runtime the process holds
    d = Device(ac.load(so))
    d.combs = guarded(d, lambda lib: tc.set_combs(lib, device=True))
    return d


def guarded(dev, fn, *args):
    if dev.faulted:
        pytest.skip("an earlier launch of this module returned a HIP error: " + dev.faulted)
    try:
        return fn(dev.lib, *args)
    except (ac.HipError, sbv.SbvError) as e:
        dev.faulted = str(e)
        raise


def fill(recs, n=LANES):
    assert len(recs) >= n, len(recs)
    return recs[:n]


def test_canon32_on_the_device(dev):
    rng = random.Random(f"{ac.SEED}:canon32")
    edges = tc.canon32_edges(rng)
    recs = fill(edges + tc.gen_canon32(rng, (LANES - len(edges)) // 3 + 1)[len(edges):])
    assert guarded(dev, tc.run_checked, 1, "canon32", recs, tc.chk_canon32) == LANES


def test_mmadd_on_the_device(dev):
    recs = fill(tc.gen_mmadd(random.Random(f"{ac.SEED}:mmadd"), LANES))
    assert guarded(dev, tc.run_checked, 1, "mmadd", recs, tc.chk_mmadd) == LANES


def test_madd_x_on_the_device(dev):
    recs = fill(tc.gen_madd_x(random.Random(f"{ac.SEED}:madd_x"), LANES))
    assert guarded(dev, tc.run_checked, 1, "madd_x", recs, tc.chk_madd_x) == LANES


def test_g_walk_from_infinity_on_the_device(dev):
    cases = fill(tc.walk_g_cases(LANES // 2))
    assert guarded(dev, tc.run_walk, 1, "walk_g", cases) == LANES


def test_q_walk_whole_and_last_chunk_on_the_device(dev):
    cases = fill(tc.walk_q_cases(LANES // 2))
    assert sum(1 for r, _ in cases if r[9] == tc.LAST_CHUNK_J0) > 40
    assert guarded(dev, tc.run_walk, 1, "walk_q", cases) == LANES


# ---- the library, end to end -------------------------------------------------------------------------------------------------
def bits(bitmap, n):
    return np.unpackbits(np.frombuffer(bitmap, dtype=np.uint8), bitorder="little")[:n]


@pytest.fixture(scope="module")
def gpu(dev):
    guarded(dev, lambda lib: sbv.init(0))
    yield sbv
    sbv.set_grouping(True, sbv.GROUP_MIN_BATCH_DEFAULT, 0, 0)
    sbv.key_cache(True, 4096)
    sbv.hot_keys(1024, 4096)
    sbv.clear_keys()


def batch(oracle, seed, n, keys, every=8):
    """tuples, the generator's expected bitmap and the oracle's verdicts (the two must agree before the device is asked)"""
    tup = ctypes.create_string_buffer(160 * n)
    exp = ctypes.create_string_buffer((n + 7) // 8)
    oracle.sbvo_gen_batch(seed, n, keys, every, tup, exp, THREADS)
    want = ctypes.create_string_buffer((n + 7) // 8)
    oracle.sbvo_p256_verify_batch(tup, n, want, THREADS)
    assert np.array_equal(bits(want.raw, n), bits(exp.raw, n))
    assert 0 < int(bits(exp.raw, n).sum()) < n
    return tup.raw, bits(exp.raw, n)


N_THROUGHPUT = (1 << 15) + 512          # the smallest batch that takes the grouped throughput step (the cooperative form ends at 2^15)


def test_throughput_path_cold_cache_off(dev, gpu, oracle):
    tup, want = batch(oracle, 0x7E1A0001, N_THROUGHPUT, 16)
    gpu.set_grouping(True, 64, 0, 0)                     # with the cache off the built-in threshold of the grouped step is 2^17 tuples
    gpu.key_cache(False)
    try:
        for _ in range(2):                                # cold both times: nothing survives a call with the cache off
            got = guarded(dev, lambda lib: gpu.verify_batch(tup, N_THROUGHPUT))
            assert np.array_equal(bits(got, N_THROUGHPUT), want)
            groups, through_tables, _, _ = gpu.last_group_stats()
            print("group stats", gpu.last_group_stats(), "table classes", gpu.last_table_classes())
            # the sixteen signers are groups (a corrupted tuple whose flipped bit fell into its key is a key of its own and stays
            # outside): at least 7 tuples of 8 went through tables built, and filled, in this call
            assert groups == 16 and through_tables >= N_THROUGHPUT - N_THROUGHPUT // 8
            assert gpu.last_table_classes()[1] == 16          # ~2 000 tuples per key: far above the ~250 at which a table earns its fill
    finally:
        gpu.set_grouping(True, sbv.GROUP_MIN_BATCH_DEFAULT, 0, 0)


@pytest.mark.parametrize("n", [4096, N_THROUGHPUT])          # the cooperative form, and one lane per signature above 2^15
def test_registered_key_entry(dev, gpu, oracle, n):
    tup, want = batch(oracle, 0x7E1A0002, n, 4)
    t = np.frombuffer(tup, dtype=np.uint8).reshape(n, 160)
    keys = [bytes(k) for k in np.unique(t[:, 96:160], axis=0)]
    assert len(keys) >= 4                                 # the four signers (a corrupted tuple may carry a bent key of its own)
    gpu.clear_keys()
    slots = guarded(dev, lambda lib: gpu.register_keys(keys))
    slot_of = dict(zip(keys, slots))
    per_tuple = [slot_of[bytes(t[i, 96:160])] for i in range(n)]
    got = guarded(dev, lambda lib: gpu.verify_batch_keyed(t[:, :96].tobytes(), per_tuple, n))
    assert np.array_equal(bits(got, n), want)
    gpu.clear_keys()


def test_one_lane_path_grouping_off(dev, gpu, oracle):
    n = 512
    tup, want = batch(oracle, 0x7E1A0003, n, 16)
    gpu.set_grouping(False)
    try:
        got = guarded(dev, lambda lib: gpu.verify_batch(tup, n))
    finally:
        gpu.set_grouping(True, sbv.GROUP_MIN_BATCH_DEFAULT, 0, 0)
    assert np.array_equal(bits(got, n), want)


def test_hot_key_builder_selfcheck(dev, gpu, oracle):
    tup, want = batch(oracle, 0x7E1A0004, N_THROUGHPUT, 16)
    gpu.set_grouping(True, sbv.GROUP_MIN_BATCH_DEFAULT, 0, 0)
    gpu.key_cache(False)
    gpu.key_cache(True, 4096)
    gpu.hot_keys(2, 64)                                   # room for two 16-bit combs; a slot qualifies after 64 hits
    try:
        for _ in range(6):
            got = guarded(dev, lambda lib: gpu.verify_batch(tup, N_THROUGHPUT))
            assert np.array_equal(bits(got, N_THROUGHPUT), want)
            if gpu.hot_key_stats()[0] >= 2:
                break
        assert gpu.hot_key_stats()[0] == 2
        got = guarded(dev, lambda lib: gpu.verify_batch(tup, N_THROUGHPUT))          # ... and a batch served from them
        assert np.array_equal(bits(got, N_THROUGHPUT), want) and gpu.hot_key_stats()[2] > 0
        assert guarded(dev, lambda lib: gpu.hot_selfcheck(0)) and guarded(dev, lambda lib: gpu.hot_selfcheck(1))
    finally:
        gpu.hot_keys(1024, 4096)
