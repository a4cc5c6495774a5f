"""csrc/scratch_layout.hpp: the one place where device scratch and index blocks are laid out.  The header is host-only,
so tests/cpp/scratch_layout_check.cpp is compiled with plain g++ (warnings are errors) and checks, for 0 .. capacity slots of
1 / 4 / 8 / 16-byte elements and raw bytes with counts 0, 1, 63, 64, 65, 2049: every offset a multiple of 256, slots in
order without overlap, bytes() >= the end of the last slot, bind() writes base + offset into the registered pointers and
nothing else, a zero-count slot stays inside the block, an empty layout is legal, and the offsets of bt_ensure's index block
for n in {1, 255, 256, 257, 120000} equal the expression it was carved with before.  A slot past the capacity aborts."""
import os
import signal
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hands-on-point-cloud-processing_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "scratch_layout_check.cpp")


def test_scratch_layout_properties(tmp_path):
    exe = tmp_path / "scratch_layout_check"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    # one slot past the capacity: reported (stderr) and fatal before anything is recorded for it
    r = subprocess.run([str(exe), "overflow"], capture_output=True, text=True, timeout=120)
    assert r.returncode == -signal.SIGABRT and r.stdout.startswith("full ") and "survived" not in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert "slots in one scratch Layout" in r.stderr
