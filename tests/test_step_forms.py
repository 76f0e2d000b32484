"""Which kernel, at which size and form, a step launch runs (the choosers of
test_isaacgym_amd/csrc/mg_forms.h): tests/step_forms_check.cpp is built as a
stand-alone host program that includes that header alone, and run. It runs every
chooser over every combination of its inputs, every MgRun included, with block,
CU and chain counts exactly at and one past each threshold and sizes at and past
each limit, and checks that every chosen build is a built one, that every built
form is chosen by some input (a dead build fails), that the pointers a build
needs cover every bit of its own form word, and that the cases DESIGN.md names
come out as documented. Its exit status is the verdict."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = "/opt/rocm/bin/hipcc"


def test_step_forms_chosen_are_built_and_built_are_chosen(tmp_path):
    exe = str(tmp_path / "step_forms_check")
    build = subprocess.run(
        [HIPCC, "-x", "c++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "test_isaacgym_amd", "csrc"),
         os.path.join(HERE, "step_forms_check.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-2000:]
    assert "\n0 failures" in run.stdout
