"""The pairing lines of the fused kernel's development report
(BGX_FUSED_PROF, csrc/bgx_host_prof.cpp) on the host:
tests/cpuwave/prof_pair_check.cpp fills words 88..94 of 1,024 synthetic
workgroup slots (rule-mode two-move job clocks and count, pipelined claims,
claims of a rule-mode non-doubles lane, claims that saw a partner, pair item
clocks and count) and checks the three lines' figures: the per-job clock, the
share of the item wave-us, the share of claims with a partner and the pairs
formed. Built with AddressSanitizer and UBSan against the report's source
alone.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mlp-ppo-2ply-multi_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_report_prints_the_pairing_survey(tmp_path):
    exe = tmp_path / "prof_pair_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I" + CSRC,
                    os.path.join(HERE, "cpuwave", "prof_pair_check.cpp"),
                    os.path.join(CSRC, "bgx_host_prof.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    env = {**os.environ, "ASAN_OPTIONS": "verify_asan_link_order=0:detect_leaks=0"}
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
