"""The factored gamma schedule (host/pack_shared_sums.cpp)
computes what the plain gamma schedule computes.  tools/shared_sums_check.cpp
packs a synthetic set with the library's packer and runs both schedules
symbolically: every real row, its shared-sum records expanded recursively,
must read exactly the plain row's multiset of (child, total gap exponent, lg,
pf); children are produced before they are read, never-stored rows are read
once by the next row, the layout's limits hold, and the set has shared-sum
rows at all.  The sets are those of tests/test_pack_threads.py, and like its
arrays the factored ones must not depend on the pack threads: the tool's hash
of them is equal with one thread and with eight."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ssc") / "shared_sums_check")
    lib = os.path.join(ROOT, "stem_kernel_amd")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "stem_kernel_amd", "csrc"), "-D__HIP_PLATFORM_AMD__",
                    os.path.join(ROOT, "tools", "shared_sums_check.cpp"), "-o", exe, "-L", lib, "-lstem_kernel_amd",
                    f"-Wl,-rpath,{lib}", "-L/opt/rocm/lib", "-lrccl"], check=True, timeout=600)
    return exe


@pytest.mark.parametrize("n,L", [(7, 40), (64, 300), (300, 150)])
def test_factored_schedule_equals_plain(checker, n, L):
    lines = {}
    for t in ("1", "8"):
        r = subprocess.run([checker, str(n), str(L)], env=dict(os.environ, SK_PACK_THREADS=t),
                           capture_output=True, text=True, timeout=300)
        line = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else r.stderr[-300:]
        print(t, line)
        assert r.returncode == 0 and line.startswith("ok "), line
        assert int(line.split("shared=")[1].split()[0]) > 0, line
        lines[t] = line
    assert lines["1"] == lines["8"], lines
