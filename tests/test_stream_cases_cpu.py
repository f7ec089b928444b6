"""CPU tier of the stream-ordering tests: the complementary batches of tests/stream_cases.py under the oracles, and the schedule table of
tests/test_gpu_stream_order.py against the `_dev` entries that include/sbv.h declares."""
import os
import re

import numpy as np
import pytest

import stream_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("scheme,n,singles", sc.gpu_pairs())
def test_pairs_get_the_bitmaps_they_claim(oracle, scheme, n, singles):
    """Every pair of the GPU tier: the oracle accepts exactly the even tuples of X and exactly the odd ones of Y — generic tuples and the
    tuples the keyed form stands for —, so the verdicts differ at every position; the two generations share their signers; every third
    spoiled tuple carries another signer's valid key; the long-tail batches hold 24 signers with at least 64 uses and the keys used once."""
    p = sc.pair(oracle, scheme, n, singles)
    assert p.n == n and p.x.shape == p.y.shape == (n, p.stride)
    for g in "xy":
        assert sc.oracle_bitmap(oracle, scheme, p.rows(g)) == p.want(g), g
        assert (p.tuples_of(g) == p.rows(g)).all()              # the keyed form stands for the very same tuples
    bx = np.unpackbits(np.frombuffer(p.want_x, dtype=np.uint8), bitorder="little")[:n]
    by = np.unpackbits(np.frombuffer(p.want_y, dtype=np.uint8), bitorder="little")[:n]
    assert (bx != by).all() and bx[0::2].all() and not bx[1::2].any()
    ko, kl = p.key_off, p.key_len
    keys = set(p.keys)
    assert len(keys) == min(sc.SIGNERS, n) + singles
    swapped = 0
    for g in "xy":
        rows = p.rows(g)
        for i in range(n):
            k = rows[i, ko:ko + kl].tobytes()
            assert k in keys                                        # also the spoiled tuples carry a valid key of the batch
            if k != p.base[i, ko:ko + kl].tobytes():
                assert p.cause[i] == 2 and i % 2 == (1 if g == "x" else 0)
                swapped += 1
            else:
                assert (rows[i] != p.base[i]).sum() == (0 if i % 2 == (0 if g == "x" else 1) else 1), i      # one flipped bit = one byte
    assert swapped == int((p.cause == 2).sum())
    if singles:
        _, counts = np.unique(p.base[:, ko:ko + kl], axis=0, return_counts=True)
        assert int((counts == 1).sum()) == singles and int((counts >= 64).sum()) == sc.SIGNERS
        assert int((counts >= 256).sum()) == sc.SIGNERS // 2                      # a full table / rows only in the P-256 step


def test_openssl_agrees_on_the_p256_pairs(oracle, openssl_check):
    from concurrent.futures import ThreadPoolExecutor

    def verdicts(rows, lo, hi):                                     # ctypes releases the GIL during the call
        return [bool(openssl_check.sbvssl_p256_verify_tuple(rows[i].tobytes())) for i in range(lo, hi)]

    with ThreadPoolExecutor(sc.THREADS) as pool:
        for n, singles in ((sc.MAIN, 0), (sc.MAIN, sc.SINGLES), (sc.ABOVE_THRESHOLD, 0), (sc.ONE_LANE, 0)):
            p = sc.pair(oracle, "p256", n, singles)
            for g in "xy":
                rows = p.rows(g)
                cuts = list(range(0, n, 256)) + [n]
                got = sum(pool.map(lambda lo_hi: verdicts(rows, *lo_hi), zip(cuts[:-1], cuts[1:])), [])
                assert got == [i % 2 == (0 if g == "x" else 1) for i in range(n)], (n, singles, g)


def test_digest_sets_differ_everywhere():
    keys, index, dx, dy = sc.digest_pair(sc.MAIN)
    assert len(keys) == 32 * 37 and index.shape == (sc.MAIN,) and int(index.max()) < 37
    assert (dx != dy).any(axis=1).all()


def _dev_entries_of_the_header():
    text = open(os.path.join(ROOT, "include", "sbv.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)             # declarations only: the comments name entries too
    return sorted(set(re.findall(r"\b(sbv_\w+?_dev(?:_part)?)\s*\(", text)))


def test_every_dev_entry_of_the_header_has_a_schedule():
    """include/sbv.h promises the same stream contract for every `_dev` / `_dev_part` entry: each one must appear in the schedule table of
    the GPU file, with at least the late producer and the early overwriter.  An entry added later without a schedule fails here."""
    import test_gpu_stream_order as so
    declared = _dev_entries_of_the_header()
    assert len(declared) >= 8 and "sbv_p256_verify_batch_dev" in declared and "sbv_p256_verify_batch_dev_part" in declared, declared
    assert sorted(so.ENTRIES) == declared, sorted(set(declared) ^ set(so.ENTRIES))
    for name, e in so.ENTRIES.items():
        assert {"late_producer", "early_overwriter"} <= set(e.schedules) or e.kind == "part", name
        assert set(e.schedules) <= set(so.SCHEDULES), name
        assert e.schedules, name
    for sched in so.SCHEDULES:
        assert any(sched in e.schedules for e in so.ENTRIES.values()), sched
