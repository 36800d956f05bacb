"""CPU test: the LRU buffer sizes of csrc/feature_cache_ctx.hpp against the hand-written originals.

tests/lru_sizes_main.hip is a stand-alone program (its own main, no HIP call) that includes the
header and compares lru_queue_cap(), lru_bit_tiles() and compact_layout() with the expressions
they replaced, written out literally, over capacities around every boundary of the layout.  It
is built with the library's compiler and flags for the host only and run as a child process."""
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
    out = str(tmp_path_factory.mktemp("lru_sizes") / "lru_sizes_main")
    cmd = [hipcc] + _build.FLAGS + [
        "--cuda-host-only", "-g", "-I", _build.CSRC,
        os.path.join(ROOT, "tests", "lru_sizes_main.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout + r.stderr
    return out


def test_lru_sizes_equal_the_expressions_they_replaced(program):
    env = dict(os.environ)
    env.pop("GNNFLOW_LRU_QUEUE_MIN_CAPACITY", None)
    r = subprocess.run([program], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
