"""The ray caster's device functions on the host -- TEST INFRASTRUCTURE: tests/host_sim/raycaster_host.cpp (wl_raycast_dev.h through the
stand-in hip_runtime.h, fp32) built ONCE per test process, the `hostlib` fixture that hands it out, and `host_scan`, which drives it
over arrays.  tests/test_raycaster_cpu.py uses it with every table; tests/test_lidar_cpu.py with zero starts."""
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT
from wheeledlab_amd import _abi as A

CLANG = os.environ.get("WL_HOST_CXX", "/opt/rocm/lib/llvm/bin/clang++")


@functools.lru_cache(maxsize=None)
def _build():
    with tempfile.TemporaryDirectory(prefix="host_sim") as d:      # the loaded library outlives its file
        out = os.path.join(d, "libwl_raycaster_host.so")
        subprocess.run([CLANG, "-O1", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                        "-I", os.path.join(ROOT, "tests", "host_sim", "hip_stub"), "-I", os.path.join(ROOT, "wheeledlab_amd", "csrc"),
                        os.path.join(ROOT, "tests", "host_sim", "raycaster_host.cpp"), "-o", out], check=True)
        lib = C.CDLL(out)
    lib.hs_raycast.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 7
    return lib


@pytest.fixture(scope="module")
def hostlib():
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no clang++ to build the host simulation")
    return _build()


def host_scan(hostlib, field, pos, quat, starts, dirs, max_distance, outside_z=0.0, z_scale=None, scale=None, vertical=False,
              offset_pos=(0.0, 0.0, 0.0), offset_rot=(1.0, 0.0, 0.0, 0.0), alignment="base"):
    """-> (dist [n, R], hits [n, R, 3]) of the device functions on the host; `starts` None: no start table (NULL), as a lidar passes it"""
    from tests import depth_cases as DC
    hfs, _keep = DC.hf_struct(field, outside_z, z_scale)
    d = np.ascontiguousarray(dirs, np.float32)
    s = None if starts is None else np.ascontiguousarray(starts, np.float32)
    sc = None if scale is None else np.ascontiguousarray(scale, np.float32)
    p = A.WlRayCastParams((C.c_float * 3)(*offset_pos), (C.c_float * 4)(*offset_rot), len(d), max_distance, A.RAYCAST_ALIGNMENTS[alignment],
                          int(vertical))
    dist, hits = np.zeros((len(pos), len(d)), np.float32), np.zeros((len(pos), len(d), 3), np.float32)
    ptr = lambda a: None if a is None else a.ctypes.data      # noqa: E731
    assert hostlib.hs_raycast(C.byref(p), C.byref(hfs), len(pos), np.ascontiguousarray(pos).ctypes.data, np.ascontiguousarray(quat).ctypes.data,
                              ptr(s), d.ctypes.data, ptr(sc), dist.ctypes.data, hits.ctypes.data) == 0
    return dist, hits
