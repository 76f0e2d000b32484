"""The step-fusion ledger (test_isaacgym_amd/csrc/mg_fusion.h): which deferred
sets a simulate reads and which refreshes launch nothing. tests/fusion_ledger_check.cpp
is built as a stand-alone host program that includes that header alone, and run.
It drives the ledger with an abstract machine in place of HIP through every
sequence of 5 calls (sets, simulate, refreshes, fetch, discard, rebind, capture
begins / ends) under every combination of the MG_FUSE_* bits, with and without
bound tensors, and checks against Isaac Gym's contract run on the same integers
that every reader observes the truth, that fused work stays within the capture
that recorded it, that nothing is fused with the bits off, and that the sequences
include/migym.h documents come out as documented. Its exit status is the verdict."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"


def test_fusion_ledger_keeps_the_tensor_contract(tmp_path):
    exe = str(tmp_path / "fusion_ledger_check")
    build = subprocess.run(
        [HIPCC, "-x", "c++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "test_isaacgym_amd", "csrc"),
         os.path.join(HERE, "fusion_ledger_check.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-2000:]
    assert "\n0 failures" in run.stdout
