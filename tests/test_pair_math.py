"""The pair helpers of test_isaacgym_amd/csrc/mg_pair.h against their scalar
originals (mg_math.h, the +Z row helpers): tests/pair_math_check.cpp is built
as a stand-alone host program (the build's -ffp-contract=off) and run; it calls
every pair helper and its scalar original on 100,000 seeded random triples and
quaternions plus signed zeros, denormals, infinities and NaN components, and
compares the bits of both halves (two NaNs compare equal). Its exit status is
the verdict."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"


def test_pair_helpers_match_scalar_bits(tmp_path):
    exe = str(tmp_path / "pair_math_check")
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(HIPCC)), "include")
    build = subprocess.run(
        [HIPCC, "-x", "c++", "-O3", "-ffp-contract=off", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
         "-I", rocm_include, "-I", os.path.join(ROOT, "test_isaacgym_amd", "csrc"),
         os.path.join(HERE, "pair_math_check.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-2000:]
    assert " 0 mismatches" in run.stdout
