"""CPU tier of the device-arithmetic unit tests: every primitive of tools/devunit.hip through backend 0 (the product's headers
compiled by hipcc as HOST code, run in a loop) against Python big integers, on the cases of tests/arith_cases.py — the same
generators, packing, references and assertions that tests/test_gpu_devunit.py runs on the gfx950 kernels.  Backend 0 is a system
under test here, not a reference.  The same cases also run through a g++ build of the primitives with every SBV_*_CHECK contract
assertion on: a generator that leaves an op's documented contract aborts there."""
import ctypes
import os

import pytest

import arith_cases as ac


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ac.ROOT, "tools", "libsbv_devunit.so")
    if not os.path.exists(so):
        pytest.skip("tools/libsbv_devunit.so not built (make -C tools)")
    return ac.load(so)


@pytest.fixture(scope="module")
def checked():
    return ac.load(ac.build_checked())


def plain_ops():
    return [n for n in ac.GEN if n in ac.CHK]


def test_every_op_of_the_library_has_cases_and_a_reference(lib):
    plain = [n for n, (_, _, _, cross) in lib.ops.items() if not cross]
    assert sorted(plain) == sorted(plain_ops())
    assert sorted(n for n, (_, _, _, cross) in lib.ops.items() if cross) == sorted(ac.CROSS_LANE)


@pytest.mark.parametrize("name", plain_ops())
def test_op_matches_bigint_on_the_host_backend(lib, name):
    generated, checked_n = ac.run_op(lib, 0, name, ac.n_random(name, 0))
    assert checked_n == generated and generated > ac.n_random(name, 0)      # nothing skipped; the edge cases come on top


@pytest.mark.parametrize("name", plain_ops())
def test_generated_cases_stay_inside_the_contracts(checked, name):
    """the contract-checking build aborts on a breach; its results must be right as well (a third compiler on the same cases)"""
    generated, checked_n = ac.run_op(checked, 0, name, ac.n_random(name, 0))
    assert checked_n == generated


def test_glv_split_reaches_its_bound_on_the_host_backend(lib):
    n = ac.N_SPLIT_LAMBDA[0]
    generated, checked_n, widest = ac.split_lambda_bulk(lib, 0, n)
    assert checked_n == generated == n
    assert widest == 128                    # the test has reached the bound it guards


def test_bad_calls_return_errors(lib):
    buf = (ctypes.c_uint32 * 4096)()
    assert lib.sbvd_run(0, -1, buf, buf, 1) == ac.BAD_OP
    assert lib.sbvd_run(0, lib.sbvd_op_count(), buf, buf, 1) == ac.BAD_OP
    assert lib.sbvd_run(2, 0, buf, buf, 1) == ac.BAD_ARG
    assert lib.sbvd_run(0, 0, buf, buf, 0) == ac.BAD_ARG
    assert lib.sbvd_run(0, 0, buf, buf, (1 << 20) + 1) == ac.BAD_ARG
    assert lib.sbvd_run(0, 0, None, buf, 1) == ac.BAD_ARG
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.sbvd_op_words(-1, ctypes.byref(a), ctypes.byref(b)) == ac.BAD_OP
    for name in ac.CROSS_LANE:              # cross-lane ops exist on the device only
        assert lib.sbvd_run(0, lib.ops[name][0], buf, buf, 64) == ac.NOT_AVAILABLE
        assert lib.sbvd_run(1, lib.ops[name][0], buf, buf, 63) == ac.BAD_ARG


def test_device_backend_without_a_device_fails_cleanly(lib):
    """with no GPU visible (a child process that hides them) the device entry returns a HIP error code and does not crash"""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import arith_cases as ac; lib = ac.load(); "
            "import numpy as np; i = np.zeros((64, 18), np.uint32); o = np.zeros((64, 9), np.uint32); "
            "rc = lib.sbvd_run(1, lib.ops['f29_mul'][0], i.ctypes.data, o.ctypes.data, 64); print('rc', rc); "
            "sys.exit(0 if -1000 < rc < 0 else 1)") % os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rc -" in r.stdout, r.stdout     # no device visible: a HIP error code, not a crash
