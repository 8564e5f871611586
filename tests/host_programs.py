"""The small host-only C++ programs of the suite (tests/*.cpp that include the engine's headers),
compiled with g++ once per process into a temporary directory: the launch planner
(launch_plan_test.cpp; test_launch_plan.py, seglist_cases.py), the sketch launch planner
(sketch_plan_test.cpp; test_sketch_plan.py), key_hash (key_hash_test.cpp) and the heavy-hitter
readout's hash slices (hh_hash_test.cpp; hh_cases.py)."""

from __future__ import annotations

import atexit
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@functools.lru_cache(maxsize=None)
def _dir() -> str:
    d = tempfile.mkdtemp(prefix="gpuagg_host_")
    atexit.register(shutil.rmtree, d, True)
    return d


@functools.lru_cache(maxsize=None)
def build(name: str) -> str:
    """tests/<name>.cpp -> the path of its executable."""
    exe = os.path.join(_dir(), name)
    # (gpuagg_launch.h includes the HIP runtime's header: its host half, nothing is linked)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "retina_amd", "csrc"),
                    "-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(ROCM, "include"),
                    os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe], check=True)
    return exe


def planner() -> str:
    return build("launch_plan_test")


def sketch_planner() -> str:
    return build("sketch_plan_test")


def plan(exe: str, cases):
    """One "key=value ..." line of facts per case through the planner -> one dict per case: its
    fields as ints and "name", the variant's name."""
    out = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True, check=True).stdout
    res = []
    for ln in out.splitlines():
        head, name = ln.split(" name=")
        r = {k: int(v) for k, v in (w.split("=") for w in head.split())}
        r["name"] = name
        res.append(r)
    assert len(res) == len(cases)
    return res
