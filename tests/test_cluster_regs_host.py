"""k_cluster's register path on the host (mapcaller_amd/csrc/mcx_glue.h cluster_read<CAP>, stage_cluster_pair_regs<CAP>; mcx_types.h hit_pack,
packed_hits_fit): tests/hostemu/cluster_regs_check.cpp, a program of its own built with the address and undefined-behaviour sanitizers, holds the
register path for every CAP against prep_seeds + cluster_seeds on the same hit lists and asks the guard around its bounds."""
import os
import subprocess

from conftest import ROOT


def test_the_register_path_equals_the_memory_path(tmp_path):
    exe = str(tmp_path / "cluster_regs_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unused-function", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "hostemu", "cluster_regs_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "all cases agree" in r.stdout
