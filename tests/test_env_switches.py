"""The environment switches the library reads are exactly the ones README.md's table lists."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = re.compile(r"GNNFLOW_[A-Z0-9_]+")


def _library_names():
    names = set()
    for dirpath, _dirs, files in os.walk(os.path.join(ROOT, "gnnflow_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp")):
                with open(os.path.join(dirpath, f), encoding="utf-8") as fh:
                    names.update(NAME.findall(fh.read()))
    return names


def _readme_table_names():
    names = set()
    with open(os.path.join(ROOT, "README.md"), encoding="utf-8") as fh:
        for line in fh:
            m = re.match(r"\| `(GNNFLOW_[A-Z0-9_]+)` \|", line)
            if m:
                names.add(m.group(1))
    return names


def test_readme_table_lists_every_switch():
    lib, table = _library_names(), _readme_table_names()
    assert lib, "no GNNFLOW_ name found under gnnflow_amd/"
    assert lib == table, ("read but not in the README table: %s; in the table but not read: %s"
                          % (sorted(lib - table), sorted(table - lib)))
