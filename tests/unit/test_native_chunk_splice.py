"""Builds tests/native/chunk_splice.cc, a stand-alone program (its own main), with
AddressSanitizer and UBSan and runs it: kube-lite's framed chunk writer against the copying
one over a stream pair, and the in-place resourceVersion splice for 1, 7 and 20 digits.
http.cc and net.cc are compiled with the sanitizers too; the rest comes from the built
core library."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from bacchus_gpu_controller_amd import REPO_ROOT

NATIVE = os.path.join(REPO_ROOT, "native")
SOURCES = [os.path.join(REPO_ROOT, "tests", "native", "chunk_splice.cc"),
           os.path.join(NATIVE, "core", "http.cc"), os.path.join(NATIVE, "core", "net.cc")]
FLAGS = ["-std=c++17", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Wno-unused-parameter", "-I", NATIVE]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    # the core library of this session's build (conftest's ensure_built): missing means the
    # build is broken, which is a failure like in every other test
    lib = os.path.join(REPO_ROOT, "build", "libbgc.a")
    assert os.path.exists(lib), f"{lib} is missing: the core build did not produce it"
    d = tmp_path_factory.mktemp("chunk_splice")
    objs = [str(d / (os.path.basename(s) + ".o")) for s in SOURCES]
    with ThreadPoolExecutor(len(SOURCES)) as pool:
        list(pool.map(lambda so: subprocess.run([gxx, *FLAGS, "-c", so[0], "-o", so[1]], check=True, timeout=300),
                      zip(SOURCES, objs)))
    out = str(d / "chunk_splice")
    subprocess.run([gxx, "-fsanitize=address,undefined", *objs, lib, "-lssl", "-lcrypto", "-lpthread", "-ldl", "-o", out],
                   check=True, timeout=300)
    return out


def test_framed_chunks_and_rv_splice_under_sanitizers(exe):
    # the program links the sanitizer runtime itself, so its place in the library list does not
    # matter: without this option an LD_PRELOAD inherited from the caller ends it before main
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr
