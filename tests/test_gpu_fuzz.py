"""GPU: a slice of the extended fuzzers (scripts/fuzz_lru_forms.py, scripts/fuzz_ingest.py) in the
suite: the LRU replacement order in both forms and the ingest in random chunk sizes on both
sides of the device-ordering threshold (in a child process, where the low threshold applies),
against the oracle after every step."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


@pytest.mark.parametrize("form", ["list", "queue"])
@pytest.mark.parametrize("seed", range(1000, 1012))
def test_lru_order_fuzz(seed, form, monkeypatch):
    import fuzz_lru_forms
    monkeypatch.delenv("GNNFLOW_LRU_QUEUE_MIN_CAPACITY", raising=False)
    fuzz_lru_forms.run(seed, 40, form)
    os.environ.pop("GNNFLOW_LRU_QUEUE_MIN_CAPACITY", None)


INGEST_SEEDS = range(2000, 2016)


@pytest.fixture(scope="module")
def ingest_fuzz_child():
    """scripts/fuzz_ingest.py over all the seeds in ONE fresh process: add_edges reads the
    device-ordering threshold once per process, so only a process that has not ingested yet can
    force it low.  GNNFLOW_INGEST_PROFILE=1 makes every accepted call report its phases on
    stderr; "dsort" is the device ordering."""
    import subprocess
    env = dict(os.environ, GNNFLOW_INGEST_DEVICE_SORT_MIN="20000", GNNFLOW_INGEST_PROFILE="1")
    return subprocess.run(
        [sys.executable, os.path.join(ROOT, "scripts", "fuzz_ingest.py"), "--permute",
         "--first", str(INGEST_SEEDS[0]), "--seeds", str(len(INGEST_SEEDS))],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)


def _not_phase_lines(stderr):
    return "\n".join(l for l in stderr.splitlines() if not l.startswith("add_edges n="))


@pytest.mark.parametrize("seed", INGEST_SEEDS)
def test_ingest_fuzz(seed, ingest_fuzz_child):
    p = ingest_fuzz_child
    done = [l for l in p.stdout.splitlines() if l.startswith("seed %3d ok " % seed)]
    assert len(done) == 1, p.stdout[-2000:] + _not_phase_lines(p.stderr)[-4000:]
    assert " permuted" in done[0]
    assert (" shifted" in done[0]) == (seed % 2 == 1)
    assert (" big-reject" in done[0]) == (seed // 2 % 2 == 1)


def test_ingest_fuzz_ran_both_orderings(ingest_fuzz_child):
    p = ingest_fuzz_child
    assert p.returncode == 0, p.stdout[-2000:] + _not_phase_lines(p.stderr)[-4000:]
    assert p.stdout.splitlines()[-1] == "all ok"
    calls = [l for l in p.stderr.splitlines() if l.startswith("add_edges n=")]
    device = [l for l in calls if " dsort " in l]
    host = [l for l in calls if " dsort " not in l]
    print("device-ordered calls:", len(device), " host-ordered calls:", len(host))
    assert device and host
    size = lambda l: int(l.split()[1][2:])                                   # noqa: E731
    assert min(map(size, device)) >= 20000 > max(map(size, host))
