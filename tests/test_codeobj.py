"""The shipped gfx950 code objects, inspected on the CPU (no GPU needed).

Round 4's only GPU memory-access fault came from a build of the 2-ply reply
kernel whose private frame was 540 B per lane (386 VGPRs spilled) and whose
job_off / job_cnt stores went through 64-bit pointers reloaded from
dynamically addressed private slots (`scratch_load_dwordx2 vD, vADDR, off`
feeding a `flat_store`): the MovegenArgs copy stayed in scratch because two
instantiations of a by-reference lambda captured it. Every build since keeps
the struct in registers and has run clean on the GPU (DESIGN.md section 4,
"The round-4 fault"). These checks keep the shipped library out of that
shape: no kernel has a dynamic stack, the movegen kernels' private frames stay
small, and no kernel loads a 64-bit value from a dynamically addressed
private slot. The code objects are read from libbgx.so itself (the
.hip_fatbin bundles), so the check covers exactly what ships."""
import os
import re
import shutil
import subprocess

import pytest
import yaml

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "mlp-ppo-2ply-multi_amd", "bgx", "libbgx.so")
LLVM = "/opt/rocm/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MOVEGEN_FRAME_MAX = 128   # bytes per lane (today: 0-80; the faulting build: 540)


def _code_objects(tmp_path):
    for tool in ("clang-offload-bundler", "llvm-readelf", "llvm-objdump"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip(f"{tool} not available")
    if shutil.which("objcopy") is None or not os.path.exists(LIB):
        pytest.skip("objcopy or libbgx.so missing")
    fat = tmp_path / "fatbin.bin"
    # with an output file of its own: without one objcopy rewrites libbgx.so in place, under the
    # feet of a process that has it mapped (the suite's own, once another test has loaded it)
    subprocess.run(["objcopy", "--dump-section", f".hip_fatbin={fat}", LIB, str(tmp_path / "libbgx.copy.so")],
                   check=True, capture_output=True)
    data = fat.read_bytes()
    starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), data)]
    assert starts, "no offload bundle in libbgx.so"
    out = []
    for k, s in enumerate(starts):   # one bundle per translation unit
        b = tmp_path / f"b{k}.bin"
        b.write_bytes(data[s:starts[k + 1] if k + 1 < len(starts) else len(data)])
        o = tmp_path / f"c{k}.o"
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                        f"--targets={TARGET}", f"--input={b}", f"--output={o}"], check=True, capture_output=True)
        out.append(o)
    return out


def _kernels(obj):
    txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(obj)], check=True,
                         capture_output=True, text=True).stdout
    doc = txt[txt.index("---"):]
    doc = doc[:doc.index("\n...") + 4] if "\n..." in doc else doc
    return yaml.safe_load(doc)["amdhsa.kernels"]


def test_kernel_frames_and_private_pointer_reloads(tmp_path):
    objs = _code_objects(tmp_path)
    names, frames = [], {}
    for o in objs:
        for k in _kernels(o):
            names.append(k[".name"])
            frames[k[".name"]] = k[".private_segment_fixed_size"]
            assert not k.get(".uses_dynamic_stack", False), k[".name"]
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", str(o)], check=True,
                             capture_output=True, text=True).stdout
        bad = re.findall(r"scratch_load_dwordx2 v\[\d+:\d+\], v\d+, off", dis)
        assert not bad, f"{o.name}: 64-bit loads from dynamically addressed private slots: {bad[:4]}"
    for want in ("movegen_reply_kernelILb1E", "movegen_reply_kernelILb0E", "fused_step_kernel", "mlp_kernel_il",
                 "top5_kernel", "movegen_block_kernel"):
        assert any(want in n for n in names), want
    for n, f in frames.items():
        if "movegen" in n:
            assert f <= MOVEGEN_FRAME_MAX, (n, f)
