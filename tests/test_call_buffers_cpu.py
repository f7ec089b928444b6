"""CPU tier of consensus_amd/csrc/call_buffers.h, the buffer scope of the host-pointer sign / recover / Schnorr entries of sbv_api.hip.

Its failure paths need a hipMalloc, a copy or a launch to fail, which no GPU test may provoke: tests/emul/call_buffers_test.cc brings a
fake runtime instead (malloc-backed, counts calls, fails the k-th, tracks pending work) and drives one scripted call shaped like the
signers through the clean run and through every single failure.  It asserts the status and error text, that nothing is issued after a
failure, that every buffer is freed once, never with work pending, and every secret one zeroed first, and the number of synchronises
of the clean run (1 without a secret buffer, 2 with one).  Built here as a program of its own with AddressSanitizer and UBSan."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "call_buffers_test.cc")


def test_call_buffers_against_a_fake_runtime(tmp_path):
    exe = str(tmp_path / "call_buffers_test")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-I" + os.path.join(rocm, "include"), "-D__HIP_PLATFORM_AMD__",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "call_buffers: ok" in r.stdout
