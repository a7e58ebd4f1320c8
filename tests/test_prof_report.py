"""The fused kernel's development report (BGX_FUSED_PROF, csrc/bgx_host_prof.cpp)
on the host: tests/cpuwave/prof_report_check.cpp fills 1,024 synthetic
workgroup slots (the median-duration and the slowest workgroup at indices 650
and 999, distinctive rows / tier-2 jobs / lane-steps in words 26-28, begin /
loop / end clocks in words 19, 20, 24, 25) and checks that the "median
workgroup ... slowest ..." and "last launch shape" lines carry those
workgroups' values and that the dump CSV has one line per workgroup that ran.
Built with AddressSanitizer and UBSan against the report's source alone: a
slot index scaled by anything but the slot width reads another workgroup's
words or leaves the array.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mlp-ppo-2ply-multi_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_report_reads_the_picked_workgroups_slots(tmp_path):
    exe = tmp_path / "prof_report_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I" + CSRC,
                    os.path.join(HERE, "cpuwave", "prof_report_check.cpp"),
                    os.path.join(CSRC, "bgx_host_prof.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    env = {**os.environ, "ASAN_OPTIONS": "verify_asan_link_order=0:detect_leaks=0"}
    r = subprocess.run([str(exe), str(tmp_path / "dump.csv")], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
