"""CPU tier of consensus_amd/csrc/shard_pieces.h: the piece plan and the piece pipeline behind verify_shard, verify_shard_keyed and
verify_shard_msgs of sbv_api.hip, one device's share of a sharded call.

The plan is arithmetic: tests/emul/shard_pieces_test.cc holds the sizes the GPU tests' docstrings quote ("3 pieces of 183 808", "30 pieces
of 11 264", "3 equal pieces of 5 120") as literal cases and sweeps m, group and piece size for what every plan has: whole granules, the
form's cap, pieces that cover the share with a non-empty last one.

The pipeline's order decides whether a staging set is overwritten under the kernels that read it, and its failure paths need a copy, a
wait or a launch to fail, which no GPU test may provoke.  The same program brings a fake runtime (streams and events are small integers;
it logs every call with its stream, fails the k-th, gives fixed durations) and drives a scripted share with one and with two kernel
streams, 1 to 4 pieces, the busy flag set and clear: the clean log against the ordering rules, the timing sums over the right event
pairs, then every single failure for its code and text, nothing enqueued after it, every stream drained before the first event is
destroyed, every event destroyed once.  Built here as a program of its own with AddressSanitizer and UBSan."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "shard_pieces_test.cc")


def test_shard_pieces_plan_and_pipeline_against_a_fake_runtime(tmp_path):
    exe = str(tmp_path / "shard_pieces_test")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-I" + os.path.join(rocm, "include"), "-D__HIP_PLATFORM_AMD__",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "shard_pieces: ok" in r.stdout
