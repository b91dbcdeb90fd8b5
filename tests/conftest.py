import os
import pathlib
import shutil
import sys
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (runs on the GPU box via gpurun)")
    config.addinivalue_line("markers", "slow: multi-second integration test")


@pytest.fixture(scope="session", autouse=True)
def _native_built():
    """Build the C++ core/binaries (and HIP kernels) once per session, incrementally."""
    from bacchus_gpu_controller_amd.utils.build import ensure_built

    ensure_built()
    yield


@pytest.fixture(scope="session")
def nat():
    from bacchus_gpu_controller_amd import native

    return native()


@pytest.fixture(scope="session")
def reference_crd_path():
    p = "/root/reference/charts/bacchus-gpu-controller/templates/crd.yaml"
    return p if os.path.exists(p) else None


# sun_path of an AF_UNIX address holds 107 bytes; the longest name a test puts under its
# tmp_path is "pod-resources/kubelet.sock"
_UNIX_PATH_MAX = 107
_LONGEST_SOCKET_SUFFIX = len("/pod-resources/kubelet.sock")


@pytest.fixture
def tmp_path(tmp_path):
    """pytest's tmp_path, unless it lies so deep (a long TMPDIR or home directory) that the
    Unix sockets the tests bind under it would not fit in a socket address: then a short
    directory of its own, removed after the test."""
    if len(os.fsencode(str(tmp_path))) + _LONGEST_SOCKET_SUFFIX <= _UNIX_PATH_MAX:
        yield tmp_path
        return
    roots = [r for r in ("/tmp", "/var/tmp", "/dev/shm") if os.path.isdir(r) and os.access(r, os.W_OK | os.X_OK)]
    if not roots:
        pytest.fail(f"{tmp_path} is too long for a Unix socket path and no short temporary directory is writable")
    short = tempfile.mkdtemp(prefix="bgc-", dir=roots[0])
    try:
        yield pathlib.Path(short)
    finally:
        shutil.rmtree(short, ignore_errors=True)
