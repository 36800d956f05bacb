"""CPU test: csrc/enqueue_worker.{hpp,hip} on its own, under ThreadSanitizer.

tests/enqueue_worker_main.hip is a stand-alone program (its own main, no HIP call) that links
enqueue_worker.hip: job order, per-ticket error status, the cap on never-waited statuses, two
submitting threads, the ticket codec.  It is built with the library's compiler and flags plus
-fsanitize=thread on the host side and run as a child process, with the default polling and
with GNNFLOW_ENQUEUE_SPIN_US=0."""
import os
import shutil
import subprocess

import pytest

from gnnflow_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    try:
        hipcc = _build._hipcc()
    except RuntimeError:
        hipcc = None
    if hipcc is None or not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("enqueue_worker") / "enqueue_worker_main")
    cmd = [hipcc] + _build.FLAGS + [
        "--cuda-host-only", "-g", "-Xarch_host", "-fsanitize=thread", "-I", _build.CSRC,
        os.path.join(ROOT, "tests", "enqueue_worker_main.hip"),
        os.path.join(_build.CSRC, "enqueue_worker.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout + r.stderr
    return out


@pytest.mark.parametrize("spin_us", [None, "0"])
def test_enqueue_worker_under_tsan(program, spin_us):
    env = dict(os.environ)
    env.pop("GNNFLOW_ENQUEUE_SPIN_US", None)
    env.pop("GNNFLOW_ENQUEUE_LANES", None)
    if spin_us is not None:
        env["GNNFLOW_ENQUEUE_SPIN_US"] = spin_us
    r = subprocess.run([program], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ThreadSanitizer" not in r.stdout + r.stderr, r.stderr
    assert "all checks passed" in r.stdout
