"""The fused 1-ply step's draws made ahead (DrawSlot, draw_fill and SlotRng,
csrc/bgx_engine.h) on the host (tests/cpuwave/draw_check.cpp, built with
AddressSanitizer and UBSan): a slot filled as the kernel's draw item fills it
and consumed by lane_advance gives, bit for bit, what LaneRng (the phased
engine's generator) gives on the same inputs: the sampling uniform, the dice,
the board words, the player, the final counter and every other state word,
the record, the episode header, the board row and the error flags.

Over 1,000 (seed, lane, counter) triples: lanes 0, 1, 4095 and 8191 with
lane_base 0 and 100,000, counters on both sides of 2^32 and at the top of the
64-bit range; every path of lane_advance (pass, move, move that ends the game,
move and pass at the max_steps truncation); per (seed, lane), counters searched
so that new_game's starter roll, its two re-rolls and its first roll come out
doubles (the loops' draws past the slot); scripted dice inside the table and
past its end; and the two packed dice pairs through the slot and back for all
36 x 36 values.
"""
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_slot_draws_equal_lane_rng_on_every_path(tmp_path):
    exe = tmp_path / "draw_check"
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(HERE, "cpuwave"), "-I" + os.path.join(REPO, "mlp-ppo-2ply-multi_amd", "csrc"),
                    "-I" + os.path.join(REPO, "include"), os.path.join(HERE, "cpuwave", "draw_check.cpp"),
                    "-o", str(exe), "-pthread"], check=True, capture_output=True, text=True)
    env = {**os.environ, "ASAN_OPTIONS": "verify_asan_link_order=0:detect_leaks=0"}
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(res)
    assert res["mismatches"] == 0
    assert res["triples"] >= 1000 and res["cases"] >= 5 * 800
    assert res["dice_pairs"] == 36 * 36
    # the paths ran: restarts, draws past the slot, every forced case re-rolled three times
    assert res["new_games"] >= 3 * 800
    assert res["beyond_slot"] >= res["new_games"] - res["scripted"]
    assert res["forced_rerolls"] > 300 and res["forced_long"] >= 0.75 * res["forced_rerolls"]
    assert 0 < res["exhausted"] < res["scripted"]
