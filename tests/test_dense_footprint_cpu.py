"""The shape rule behind the resident dense count (featurebase_amd/csrc/fbk_dense_policy.h: the plan's footprint bound and
the threshold), checked by a stand-alone host program built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dense_footprint_bound_and_threshold():
    out = os.path.join(ROOT, "build", "dense_footprint_check")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "scripts", "dense_footprint_check.cpp"), "-o", out])
    run = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "dense footprint ok" in run.stdout, run.stdout + run.stderr
