"""Builds tests/native/xlane_ref.cc, a stand-alone program (its own main) over the cross-lane check's host reference
(native/gpu/hip/xlane_ref.h, no HIP dependency), with AddressSanitizer and UBSan and runs it: every DPP control at
every lane, the gate, the swaps, the permutes and swizzles, whole runs and the rate phase's closed form, each at the
bounds of its lists."""
import os
import shutil
import subprocess

import pytest

from bacchus_gpu_controller_amd import REPO_ROOT

SOURCE = os.path.join(REPO_ROOT, "tests", "native", "xlane_ref.cc")
FLAGS = ["-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
         "-I", os.path.join(REPO_ROOT, "native")]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    out = str(tmp_path_factory.mktemp("xlane_ref") / "xlane_ref")
    subprocess.run([gxx, *FLAGS, SOURCE, "-o", out], check=True, timeout=300)
    return out


def test_xlane_reference_under_sanitizers(exe):
    # the program links the sanitizer runtime itself, so its place in the library list does not
    # matter: without this option an LD_PRELOAD inherited from the caller ends it before main
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr
