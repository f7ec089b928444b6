"""GPU tier of the device-arithmetic unit tests: every primitive the product's kernels execute, compiled by hipcc -O3 for gfx950
from the product's own headers (tools/devunit.hip), one case per lane, against Python big integers — never against another
build of the same source.  Same generators, references and assertions as tests/test_devunit_cpu.py (tests/arith_cases.py), larger
random counts, plus the cross-lane ops that have no host form: the quad doubling chains through the DPP broadcast policies
(keychain_quad_dev, edchain_quad_dev, k256_quad_dev) and the __shfl_xor sum of the cooperative kernels.

One process, one launch at a time.  A launch that returns a HIP error fails its test and every later test of the module is
skipped: nothing more is launched on a device that has just faulted."""
import os

import pytest

import arith_cases as ac

pytestmark = pytest.mark.gpu


class Device:
    def __init__(self, lib):
        self.lib = lib
        self.faulted = None


@pytest.fixture(scope="module")
def dev():
    so = os.path.join(ac.ROOT, "tools", "libsbv_devunit.so")
    if not os.path.exists(so):
        pytest.skip("tools/libsbv_devunit.so not built (make -C tools)")
    return Device(ac.load(so))


def guarded(dev, fn, *args):
    if dev.faulted:
        pytest.skip("an earlier launch of this module returned a HIP error: " + dev.faulted)
    try:
        return fn(dev.lib, *args)
    except ac.HipError as e:
        dev.faulted = str(e)
        raise


def plain_ops():
    return [n for n in ac.GEN if n in ac.CHK]


def test_every_op_of_the_library_is_exercised(dev):
    plain = [n for n, (_, _, _, cross) in dev.lib.ops.items() if not cross]
    assert sorted(plain) == sorted(plain_ops())
    assert sorted(n for n, (_, _, _, cross) in dev.lib.ops.items() if cross) == sorted(ac.CROSS_LANE)


@pytest.mark.parametrize("name", plain_ops())
def test_op_matches_bigint_on_the_device(dev, name):
    generated, checked = guarded(dev, ac.run_op, 1, name, ac.n_random(name, 1))
    print(f"{name}: {checked} of {generated} cases checked")
    assert checked == generated and generated > ac.n_random(name, 1)


def test_glv_split_reaches_its_bound_on_the_device(dev):
    n = ac.N_SPLIT_LAMBDA[1]
    generated, checked, widest = guarded(dev, ac.split_lambda_bulk, 1, n)
    assert checked == generated == n and n - len(ac.glv_edge_scalars()) >= 10**6
    assert widest == 128                    # the test has reached the bound it guards


@pytest.mark.parametrize("name", ["x_keychain29", "x_edchain", "x_k256chain"])
def test_quad_chain_through_dpp_matches_bigint(dev, name):
    """16 quads per wavefront, every quad its own point and number of doublings; all four lanes of every quad are checked"""
    generated, checked = guarded(dev, ac.run_chain, name, 64)
    assert checked == generated == 256


@pytest.mark.parametrize("lanes", [2, 4, 8, 16])
def test_shfl_xor_sum_of_partial_points(dev, lanes):
    generated, checked = guarded(dev, ac.run_shfl_sum, lanes, 512 // lanes)
    assert checked == generated == 512
