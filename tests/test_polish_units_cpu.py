"""CPU: the polisher's unit-list builder (csrc/polish_units.h) on its own - tests/polish_units_main.cpp compares it with a per-pair loop over random validity
maps (1 - 40 groups, 0 - 300 pairs each, 1 - 5 windows under a larger nwinmax, empty and stable groups, window positions with many ties) with 1, 2, 3 and 16 threads."""
import os, shutil, subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_unit_lists_equal_the_per_pair_loop(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler (the build needs one as well)"
    exe = str(tmp_path / "polish_units")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "ngspeciesid_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "polish_units_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "polish_units: ok" in r.stdout
