"""csrc/lane_group.h: the bit functions the cooperative text kernels share, checked on the host
against serial code by tools/lane_group_host_check.cpp (built with sanitizers)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lane_group_check_program(tmp_path):
    """tools/lane_group_host_check.cpp builds with the command in its header and prints ok."""
    from alluxio_amd.ops.build import ROCM
    cxx = shutil.which("clang++") or os.path.join(ROCM, "lib", "llvm", "bin", "clang++")
    if not os.path.exists(cxx):
        pytest.skip("no clang++")
    exe = str(tmp_path / "lane_group_host_check")
    header = open(os.path.join(ROOT, "tools", "lane_group_host_check.cpp")).read().split("#include")[0]
    flags = "-std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined"
    assert flags in header and "-Ialluxio_amd/csrc tools/lane_group_host_check.cpp" in header
    subprocess.run([cxx, *flags.split(), "-Ialluxio_amd/csrc", "tools/lane_group_host_check.cpp", "-o", exe], cwd=ROOT,
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
