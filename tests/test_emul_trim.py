"""CPU tier of the 32-bit canonical table store and the shortened comb ends (p256_fe29.h: f29_canon32; p256_pt29.h: pt29_mmadd,
pt29_madd_x; p256_comb29.h: the walkers' two ends).  tests/emul/trim_emul.cc is built by g++ with -DSBV_F29_CHECK, so every
operand contract the code relies on is asserted while the cases run; every result is compared with Python big integers
(tests/trim_cases.py), and the tables the lane functions build are compared, byte for byte, with a second build of the same
source whose stores go through f29_canon (-DSBV_F29_STORE_REF)."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import arith_cases as ac
import trim_cases as tc

HERE = os.path.join(ac.ROOT, "tests", "emul")


def build(tag, extra):
    src = os.path.join(HERE, "trim_emul.cc")
    so = os.path.join(HERE, f"libsbv_trim_emul{tag}.so")
    csrc = os.path.join(ac.ROOT, "consensus_amd", "csrc")
    deps = [src, os.path.join(ac.ROOT, "tools", "devunit_trim.hip")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-misleading-indentation",
                               "-DSBV_F29_CHECK"] + extra + [src, "-o", so])
    return so


@pytest.fixture(scope="module")
def lib():
    l = ac.load(build("", []))
    l.combs = tc.set_combs(l, device=False)
    return l


@pytest.fixture(scope="module")
def ref_lib():
    """the same source with every table store forced onto f29_canon"""
    return ctypes.CDLL(build("_ref", ["-DSBV_F29_STORE_REF"]))


def test_canon32_matches_bigint_and_f29_canon(lib):
    rng = random.Random(f"{ac.SEED}:canon32")
    recs = tc.gen_canon32(rng, 100000)
    assert all(tc.in_canon32_contract(r) for r in recs)
    edges = tc.canon32_edges(random.Random(1))
    ks = {(tc.val29(r) + 2) // tc.P for r in edges}
    assert {-64, -1, 0, 1, 63} <= ks and len(edges) > 2000            # the multiples of p and of 2^256 reach both ends of the contract
    assert tc.run_checked(lib, 0, "canon32", recs, tc.chk_canon32) == len(recs) > 300000


@pytest.mark.parametrize("limbs", [[0] * 8 + [1 << 30], [-(1 << 30) - 1] + [0] * 8, [0, 0, 0, 1 << 30, 0, 0, 0, 0, 0]])
def test_canon32_outside_its_contract_trips_the_assertion(lib, limbs):
    """a child process: the assertion aborts"""
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); "
            "l.sbvt_canon32_abort((ctypes.c_int32 * 9)(*[int(v) for v in sys.argv[2:11]])); print('returned')")
    ok = subprocess.run([sys.executable, "-c", code, lib._name] + [str(v) for v in [0] * 9], capture_output=True, text=True)
    assert ok.returncode == 0 and "returned" in ok.stdout                 # inside the contract the same call returns
    bad = subprocess.run([sys.executable, "-c", code, lib._name] + [str(v) for v in limbs], capture_output=True, text=True)
    assert bad.returncode == -6 and "f29_canon32" in bad.stderr and "returned" not in bad.stdout


def test_mmadd_matches_madd_and_bigint(lib):
    rng = random.Random(f"{ac.SEED}:mmadd")
    recs = tc.gen_mmadd(rng, 10000)
    assert tc.run_checked(lib, 0, "mmadd", recs, tc.chk_mmadd) == len(recs) > 10000


def test_madd_x_matches_madd_on_x(lib):
    rng = random.Random(f"{ac.SEED}:madd_x")
    recs = tc.gen_madd_x(rng, 10000)
    assert tc.run_checked(lib, 0, "madd_x", recs, tc.chk_madd_x) == len(recs) > 10000


def test_fast_multiples_agree_with_the_oracle():
    """the references of the walker tests: the stepped multiples and the window sums against oracle/p256_py.py"""
    for s, sp in tc.scalar_points(tc.G_POINT, 1000, "g")[::250]:
        assert tc.ec.pt_mul(s, tc.G_POINT) == sp
    for u in tc.listed_scalars():
        assert tc.q_partial(u, 0) % tc.N == u


def test_g_walk_from_infinity(lib):
    cases = tc.walk_g_cases(1000)
    assert tc.run_walk(lib, 0, "walk_g", cases) == len(cases) >= 2 * (1000 + len(tc.listed_scalars()))


def test_q_walk_whole_and_last_chunk(lib):
    cases = tc.walk_q_cases(1000)
    assert sum(1 for r, _ in cases if r[9] == tc.LAST_CHUNK_J0) > 400 and sum(1 for r, _ in cases if r[9] == 0) > 2000
    assert tc.run_walk(lib, 0, "walk_q", cases) == len(cases)


def table_keys():
    off = (tc.G_POINT[0], (tc.G_POINT[1] + 1) % tc.P)                     # not on the curve
    assert not tc.ec.on_curve(*off)
    return [tc.G_POINT, tc.q_point(), tc.point_pool()[20], off]


def w8(x):
    return (ctypes.c_uint32 * 8)(*tc.words(x))


@pytest.mark.parametrize("k", range(4))
def test_key_table_bytes_do_not_depend_on_the_canonicaliser(lib, ref_lib, k):
    key = table_keys()[k]
    tabs = []
    for l in (lib, ref_lib):
        tab = np.zeros((tc.WINDOWS * tc.PER_WINDOW, 16), dtype=np.uint32)
        rows = np.zeros((tc.WINDOWS * 16, 16), dtype=np.uint32)
        l.sbvt_key_table(w8(key[0]), w8(key[1]), tab.ctypes.data_as(ctypes.c_void_p), rows.ctypes.data_as(ctypes.c_void_p))
        tabs.append((tab, rows))
    assert np.array_equal(tabs[0][0], tabs[1][0]) and np.array_equal(tabs[0][1], tabs[1][1])
    assert tabs[0][0][:32 * tc.PER_WINDOW].any(axis=1).all() and tabs[0][0][32 * tc.PER_WINDOW].any()      # every entry the builders own was written
    if tc.ec.on_curve(*key):                                              # ... and the table is the comb of the key
        assert np.array_equal(tabs[0][0][:32 * tc.PER_WINDOW + 1], tc.comb_of(key)[:32 * tc.PER_WINDOW + 1])
        j = 7
        compact = [tabs[0][0][j * 128 + b] for b in range(8)] + [tabs[0][0][j * 128 + 16 * a - 1] for a in range(1, 9)]
        assert np.array_equal(tabs[0][1][j * 16:j * 16 + 16], np.array(compact))


@pytest.mark.parametrize("k", range(4))
def test_one_lane_table_bytes_do_not_depend_on_the_canonicaliser(lib, ref_lib, k):
    key = table_keys()[k]
    outs = []
    for l in (lib, ref_lib):
        out = np.zeros((8, 16), dtype=np.uint32)
        l.sbvt_generic_qtab(w8(0x1234567 + k), w8(key[0]), w8(key[1]), out.ctypes.data_as(ctypes.c_void_p))
        outs.append(out)
    assert np.array_equal(outs[0], outs[1]) and outs[0].any(axis=1).all()
    if tc.ec.on_curve(*key):
        assert np.array_equal(outs[0], tc.comb_of(key)[:8])
