"""The routing plan of the step features (test_isaacgym_amd/csrc/mg_route.h, DESIGN.md
§2.4): which launches a simulate issues, over which instances, with which features,
and which combinations are refused. tests/step_route_check.cpp is built as a
stand-alone host program that includes that header alone, and run. On one small
layout built by hand (uncoupled chain and non-chain groups, coupled groups with and
without an articulation, free bodies, a pile env, a static body) it plans every
combination of attractors on none, one or two bodies of each class, a force sensor,
contact reporting, joint friction and DOF forces, and checks that every stepped
instance is in exactly one launch, that owners step in their owner launch, that the
split rows are a stable permutation of the stepped rows, that every launch's build
(mg_route_builds: the choosers of mg_forms.h, the call mg_simulate makes), under
every MgRun, is built and carries exactly the routed features or else the route
holds a refusal, that built and carried bits do not depend on the MgRun, that an
unrefused launch's build needs no buffer the plan's inputs do not allocate, and that
the refusals keep their full texts and precedence. Its exit status is the verdict."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"


def test_step_route_covers_every_instance_and_refuses_what_is_not_built(tmp_path):
    exe = str(tmp_path / "step_route_check")
    build = subprocess.run(
        [HIPCC, "-x", "c++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "test_isaacgym_amd", "csrc"),
         os.path.join(HERE, "step_route_check.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-2000:]
    assert "\n0 failures" in run.stdout
