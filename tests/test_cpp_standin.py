"""The stand-in boost::multi_array (oracle/ref_shim/standin/) that lets the
reference DP sources compile for tests/test_oracle_dp_pinning.py: build and
run tests/cpp/standin_multi_array.cpp, which checks the Boost.MultiArray
properties those sources rely on (zero-initialised elements, also after
resize; row-major; chained operator[]; size() of arrays and sub-views;
shape() and num_elements()) on 1- to 4-D arrays."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_standin_multi_array(tmp_path):
    exe = str(tmp_path / "standin_multi_array")
    subprocess.run(["g++", "-O1", "-std=gnu++11", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "oracle", "ref_shim", "standin"),
                    os.path.join(ROOT, "tests", "cpp", "standin_multi_array.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr
