#!/usr/bin/env python3
"""Build the native parts of alink_amd in-tree.

* ``alink_amd/ops/libalink_hip.so``   — HIP/CDNA4 kernels, ``hipcc --offload-arch=gfx950`` (C ABI, ctypes)
* ``alink_amd/_native/libalink_native.so`` — host C++ runtime (CSV/libsvm/vector parsing, murmur3
  feature hashing, sample-sort helpers), ``g++ -O3`` (C ABI, ctypes)

* ``variants/libalink_hip_pfd.so``     — the same library with ``kmeans_v10.hip`` compiled ``-DKM10_PFD=1`` (the L2
  prefetch A/B that the default build compiles out; ``tests/test_kmeans_kernel_gpu.py`` checks it changes no result)

Incremental: a target is rebuilt only when a source is newer than it.  Usage:
    python build_native.py [--force] [--only hip|host]
"""
from __future__ import annotations

import argparse
import glob
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.abspath(__file__))
HIP_SRC = sorted(glob.glob(os.path.join(ROOT, "alink_amd", "ops", "csrc", "*.hip")))
HIP_OUT = os.path.join(ROOT, "alink_amd", "ops", "libalink_hip.so")
PFD_OUT = os.path.join(ROOT, "variants", "libalink_hip_pfd.so")
HOST_SRC = sorted(glob.glob(os.path.join(ROOT, "alink_amd", "_native", "csrc", "*.cpp")))
HOST_OUT = os.path.join(ROOT, "alink_amd", "_native", "libalink_native.so")
ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")


def _stale(out, srcs, extra=()):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(s) > t for s in list(srcs) + list(extra))


def _run(cmd):
    print("+", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def _hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _hip_headers():
    return glob.glob(os.path.join(ROOT, "alink_amd", "ops", "csrc", "*.h"))


def _hip_compile(job, force=False):
    src, obj, flags = job
    if force or _stale(obj, [src], _hip_headers()):
        os.makedirs(os.path.dirname(obj), exist_ok=True)
        _run([_hipcc(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-mcode-object-version=5",
              "-Wno-unused-command-line-argument", *flags, "-c", src, "-o", obj])
    return obj


def build_hip(force=False):
    """The kernel library and its ``pfd`` variant (tools/build_kmeans_variants.sh pfd: the library's other objects +
    kmeans_v10.hip with -DKM10_PFD=1).  Stale objects compile in parallel (MAX_JOBS, default min(8, cpus))."""
    need_lib = force or _stale(HIP_OUT, HIP_SRC, _hip_headers())
    need_pfd = force or _stale(PFD_OUT, HIP_SRC, _hip_headers())
    if not (need_lib or need_pfd):
        return HIP_OUT
    tmp = os.path.join(ROOT, "build", "hip")
    jobs = [(s, os.path.join(tmp, os.path.basename(s) + ".o"), ()) for s in HIP_SRC]
    v10 = os.path.join(ROOT, "alink_amd", "ops", "csrc", "kmeans_v10.hip")
    if need_pfd:
        jobs.append((v10, os.path.join(ROOT, "build", "variants", "pfd", "kmeans_v10.o"), ("-DKM10_PFD=1",)))
    workers = int(os.environ.get("MAX_JOBS", 0)) or min(8, os.cpu_count() or 1)
    with ThreadPoolExecutor(max_workers=max(1, workers)) as pool:
        objs = list(pool.map(lambda j: _hip_compile(j, force), jobs))
    lib_objs = objs[:len(HIP_SRC)]
    if need_lib:
        _run([_hipcc(), f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", HIP_OUT] + lib_objs)
    if need_pfd:
        os.makedirs(os.path.dirname(PFD_OUT), exist_ok=True)
        _run([_hipcc(), f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", PFD_OUT]
             + [o for s, o in zip(HIP_SRC, lib_objs) if s != v10] + [objs[-1]])
    return HIP_OUT


def build_host(force=False):
    if not HOST_SRC:
        return None
    headers = glob.glob(os.path.join(ROOT, "alink_amd", "_native", "csrc", "*.h"))
    if not force and not _stale(HOST_OUT, HOST_SRC, headers):
        return HOST_OUT
    cxx = shutil.which("g++") or "c++"
    _run([cxx, "-O3", "-std=c++17", "-fPIC", "-shared", "-march=x86-64-v2", "-fopenmp", "-o", HOST_OUT]
         + HOST_SRC)
    return HOST_OUT


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--force", action="store_true")
    ap.add_argument("--only", choices=["hip", "host"], default=None)
    a = ap.parse_args(argv)
    if a.only in (None, "host"):
        build_host(a.force)
    if a.only in (None, "hip"):
        build_hip(a.force)


if __name__ == "__main__":
    main(sys.argv[1:])
