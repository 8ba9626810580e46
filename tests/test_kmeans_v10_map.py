"""The swept tile order of the v10 KMeans kernel (alink_amd/ops/csrc/kmeans_v10_map.h), checked on the CPU before
any kernel runs on it: tests/kmeans_v10_map_check.cpp is compiled with the host C++ compiler against the header the
kernel and its launch wrapper use, and walks every workgroup the way a loader wave does.

For chunks S of 1, 2 and 8 tiles, the tile counts of tests/test_kmeans_v10_sweep_gpu.py's shapes and bench.py's
1,562,500, grids of 1, 3, 4, 7 and 256 workgroups, windows of 3 and 4 owned tiles and of the production length, both
directions: every global tile is owned exactly once; every staged byte offset is non-negative and under 2 GiB from
its window's base and addresses the tile it should; every window lies inside X and holds every live byte of its
tiles; the reverse walk is the forward walk backwards; a phantom tile (the second tile of an odd last pair) is
flagged and its offset lies past its resource's end.  The same program is then built with AddressSanitizer and
UndefinedBehaviorSanitizer and run again: a plain program, nothing preloaded."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "alink_amd", "ops", "csrc")
SRC = os.path.join(HERE, "kmeans_v10_map_check.cpp")


def _cxx():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    return cxx


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.run([_cxx(), "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, SRC, "-o", exe],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert out.stdout.strip().splitlines()[-1].startswith("ok:"), out.stdout[-2000:]
    return out.stdout


def test_v10_map_walks_every_tile_once(tmp_path):
    _build_and_run(tmp_path, "map_check", ["-O2"])


def test_v10_map_under_address_and_ub_sanitizers(tmp_path):
    # gcc links the sanitizer runtimes dynamically unless told otherwise (clang links them statically): linked
    # statically, the program does not depend on the order in which shared libraries are loaded
    static = [] if "clang" in os.path.basename(_cxx()) else ["-static-libasan", "-static-libubsan"]
    _build_and_run(tmp_path, "map_check_san",
                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static])
