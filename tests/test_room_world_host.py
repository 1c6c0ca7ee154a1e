"""The world-axis certificate of a room (csrc/rtgo_room_world.h: room_world_certify and room_world_margin, what render_roomw_kernel's
launches stand on), checked on the CPU by a stand-alone program with a main of its own, tests/room_world_check.cpp, built
with -fsanitize=address,undefined and run as a child process.  Nothing of it is loaded into Python.

The program synthesizes rooms (cornell's as the scene code composes it, with each wall first; negative scales, permuted axes, residues
of 1e-7 and 1e-6: accepted; a residue of 1e-3, a sheared frame, a 1e-3 room 100 units out: refused) and, per accepted room, holds the
float32 steering of 120 000 rays, under one-ulp nudges of each reciprocal, to a float64 evaluation in the frame form: no face the
reference could accept may be missing from the candidates.  -ffp-contract=off: the program's float32 is the kernel's, operation for
operation."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_certificate_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler (the library's host half is built with one)"
    exe = str(tmp_path / "room_world_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "raytracingo_amd", "csrc"), os.path.join(ROOT, "tests", "room_world_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout[-4000:] + run.stderr[-2000:]
    rooms = re.findall(r"rays (\d+), faces wanted \d+, .*exceptions (\d+)", run.stdout)
    assert len(rooms) >= 12 and all(int(n) >= 100000 and int(e) == 0 for n, e in rooms), rooms
    assert len(re.findall(r"certificate \d, margin -1", run.stdout)) >= 4, run.stdout[-2000:]


def test_the_header_has_no_hip_in_it():
    with open(os.path.join(ROOT, "raytracingo_amd", "csrc", "rtgo_room_world.h")) as f:
        text = f.read()
    assert "hip" not in re.sub(r"//[^\n]*", "", text).lower() and "__device__" not in text
