"""GPU: the three orderings of add_edges (edge_store_ingest.hip) against the oracle, each in a
process where it really runs.  The device/host threshold GNNFLOW_INGEST_DEVICE_SORT_MIN is read
once per process, so every arrangement is a fresh child (tests/ingest_order_child.py, which
describes the scenarios); with GNNFLOW_INGEST_PROFILE=1 every accepted add_edges prints its phase
line on stderr, and "dsort" appears on the device path only — which path a call took is asserted
here from those lines, not assumed."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENARIOS = ["a", "b", "c", "d", "e", "f", "t"]
T = 4096
PHASE = re.compile(r"^add_edges n=(\d+) .*?:(.*)$")


def run_child(sort_min, scenarios=()):
    env = dict(os.environ, GNNFLOW_INGEST_DEVICE_SORT_MIN=sort_min, GNNFLOW_INGEST_PROFILE="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ingest_order_child.py"),
                        *scenarios], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    return p


def calls_of(stderr):
    """[(tag, [(n, phase names)])] in order: the phase lines that follow each `@@ tag`."""
    calls = []
    for line in stderr.splitlines():
        if line.startswith("@@ "):
            calls.append((line[3:], []))
            continue
        m = PHASE.match(line)
        if m and calls:
            calls[-1][1].append((int(m.group(1)), m.group(2).split()[0::2]))
    return calls


@pytest.mark.parametrize("sort_min", ["0", "4096", "1000000000"])
def test_every_ingest_ordering_equals_the_oracle(sort_min):
    p = run_child(sort_min)
    tail = p.stdout[-3000:] + "\n".join(l for l in p.stderr.splitlines()
                                        if not l.startswith(("add_edges n=", "@@ ")))[-4000:]
    assert p.returncode == 0, tail
    assert [l.split()[1] for l in p.stdout.splitlines() if l.startswith("ok ")] == SCENARIOS, tail

    calls = calls_of(p.stderr)
    assert calls[-1][0] == "end"
    ingests = {tag: lines for tag, lines in calls
               if not tag.startswith("scenario ") and tag != "end"}
    assert len(ingests) > 20
    for tag, lines in ingests.items():
        if tag.endswith("(rejected)"):
            assert lines == [], tag          # a rejected call never reaches its report
        else:
            assert len(lines) == 1, (tag, lines)

    def path(tag):
        return "device" if "dsort" in ingests[tag][0][1] else "host"

    accepted = [t for t in ingests if not t.endswith("(rejected)")]
    if sort_min == "0":
        assert all(path(t) == "device" for t in accepted), {t: path(t) for t in accepted}
    elif sort_min == "1000000000":
        assert all(path(t) == "host" for t in accepted), {t: path(t) for t in accepted}
        # the sparse-id batch took std::sort, the dense ones the counting sort
        assert "csort" not in ingests["c sparse"][0][1] and "csort" in ingests["c"][0][1]
    else:
        assert ingests["t T-1"][0][0] == T - 1 and path("t T-1") == "host"
        assert ingests["t T"][0][0] == T and path("t T") == "device"
        assert ingests["t T+1"][0][0] == T + 1 and path("t T+1") == "device"
        # T/2 edges with their reverses are T edges by the time they are ordered; either way the
        # child has compared the result with the oracle
        assert ingests["t T/2 reverse"][0][0] == T
        print("T/2 edges + reverse took the", path("t T/2 reverse"), "path")
        assert path("a") == "device" and path("c sparse") == "host"
        assert {path(t) for t in accepted} == {"device", "host"}
