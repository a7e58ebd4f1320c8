"""The fused step's claim / publish / draw-wait protocol (csrc/bgx_claim.h) on
the host: tests/cpuwave/claim_check.cpp drives it with 12 std::thread "waves"
over std atomics, 1,500 random steps at 16 and at 32 lanes (ragged lane
ranges, random classes, random choice completion order, pairing on and off),
and checks that every lane is claimed exactly once, that a partner is a
pairable lane that was open, that left-over items end as no-ops, that the
draw wait ends only after every lane has published, and that no poll reaches
the bound. A stand-alone program built with ThreadSanitizer against the
header alone: a missing release / acquire order is a reported data race.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mlp-ppo-2ply-multi_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_claim_protocol_under_thread_sanitizer(tmp_path):
    exe = tmp_path / "claim_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=thread", "-fno-omit-frame-pointer",
                    "-pthread", "-I" + CSRC, os.path.join(HERE, "cpuwave", "claim_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "data race" not in r.stderr, r.stderr[-3000:]
