"""The ticket arithmetic of rtgo_update_prims_device_async (csrc/rtgo_ticket_ring.h: the slot of a ticket, which tickets the context still
answers for, when a slot is reused), checked on the CPU by a stand-alone program with a main of its own, tests/ticket_ring_check.cpp,
built with -fsanitize=address,undefined and run as a child process.  Nothing of it is loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_ring_arithmetic_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler (the library's host half is built with one)"
    exe = str(tmp_path / "ticket_ring_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "raytracingo_amd", "csrc"), os.path.join(ROOT, "tests", "ticket_ring_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout[-2000:] + run.stderr[-2000:]
