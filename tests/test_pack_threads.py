"""The dataset packing (host/pack.cpp pack_dataset, over pack_x.cpp, pack_y.cpp
and pack_sweep.cpp) runs its per-example passes on host threads and appends
at prefix offsets: the packed arrays must not depend on the thread count.
tools/pack_compare.cpp calls the library's sk::pack_dataset
(host/runtime_types.h) and hashes every packed array, one hash per list of
runtime_types.h: y (the y-role records in the plain order), x (the x-role
arrays, the per-example ex_* vectors and key tables), r (the renumbered y
records) and f (the factored gamma schedule) -- r and f are what the device
runs.  It is built here (host code only, at -O1: the packer it runs is the
library's, built as shipped) and run with one thread and with eight
(SK_PACK_THREADS), and both must equal GOLDEN.  Its y and x values are the
hashes of the serial packer before the threaded one (commit 61ba1f6^, built
in a worktree with this pack_compare.cpp), its r and f values those of the
one-file packer before it was split (commit 9b92a18, built likewise), so a
bug that does not depend on the thread count fails here too."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pack_compare(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pc") / "pack_compare")
    lib = os.path.join(ROOT, "stem_kernel_amd")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "stem_kernel_amd", "csrc"), "-D__HIP_PLATFORM_AMD__",
                    os.path.join(ROOT, "tools", "pack_compare.cpp"), "-o", exe, "-L", lib, "-lstem_kernel_amd",
                    f"-Wl,-rpath,{lib}", "-L/opt/rocm/lib", "-lrccl"], check=True, timeout=600)
    return exe


GOLDEN = {(300, 150): ("36d6bd2e8250904e", "287b3489cc46be35", "d97d6b913fcd5c64", "5466fe1e49a0330c"),
          (64, 300): ("88c43b92757d6d0c", "7683c19231feea38", "38d1453624e9121a", "4a46b469eccad71e"),
          (7, 40): ("5103f9f17bc7fe14", "f110ddedec494801", "9c80d80bf46f9050", "4391e0ff1458cbc0")}


@pytest.mark.parametrize("n,L", sorted(GOLDEN))
def test_packing_independent_of_threads(pack_compare, n, L):
    for t in ("1", "8"):
        r = subprocess.run([pack_compare, str(n), str(L)], env=dict(os.environ, SK_PACK_THREADS=t),
                           capture_output=True, text=True, timeout=300, check=True)
        line = r.stdout.strip().splitlines()[-1]
        assert line.startswith("rc=0"), line
        got = tuple(line.split(f" {k}-hash ")[1].split()[0] for k in "yxrf")
        assert got == GOLDEN[(n, L)], (t, got)
