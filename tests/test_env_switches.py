"""The environment variables the library reads are declared once, in the table "Environment variables" of INTEGRATION.md: every
`CENET_*` name that product code passes to getenv / os.environ is a row, every row has a reader, and every row is set by a test or
a tool of the tree (a switch nobody sets selects a path nobody runs)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = r'"(CENET_[A-Z0-9_]+)"'


def _product_sources():
    return [f for ext in ("py", "hip", "h") for f in glob.glob(os.path.join(ROOT, "cenet_amd", "**", "*." + ext), recursive=True)]


def _readers():
    """{name: file} of the quoted CENET_* names passed to getenv / os.environ, directly or through a one-level helper (a function
    that hands its own parameter to getenv, like gemm_group.hip's grp_env)"""
    found = {}
    for f in _product_sources():
        src = open(f).read()
        calls = [r"\bgetenv\(\s*", r"\bos\.environ\.get\(\s*", r"\bos\.environ\[\s*", r"\bos\.getenv\(\s*"]
        for helper, param in re.findall(r"\b(\w+)\([^()]*\bchar\s*\*\s*(\w+)[^()]*\)\s*\{", src):
            if re.search(r"\b%s\([^()]*\)\s*\{[^}]*\bgetenv\(\s*%s\s*\)" % (helper, param), src):
                calls.append(r"\b%s\(\s*" % helper)
        for c in calls:
            for n in re.findall(c + NAME, src):
                found.setdefault(n, os.path.relpath(f, ROOT))
    return found


def _table():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "\n## Environment variables\n" in doc
    sec = doc.split("\n## Environment variables\n", 1)[1].split("\n## ", 1)[0]
    rows = {}
    for line in sec.splitlines():
        m = re.match(r"\|\s*`(CENET_[A-Z0-9_]+)`\s*\|([^|]*)\|", line)
        if m:
            assert m.group(1) not in rows, f"{m.group(1)} has two rows"
            rows[m.group(1)] = m.group(2).strip().strip("`")
    return rows


def _users():
    files = [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "__graft_entry__.py")]
    for d in ("tests", "tools"):
        files += [f for f in glob.glob(os.path.join(ROOT, d, "**", "*"), recursive=True)
                  if os.path.isfile(f) and f.endswith((".py", ".sh")) and os.path.abspath(f) != os.path.abspath(__file__)]
    return {f: open(f).read() for f in files}


def test_the_helper_reader_is_seen():
    r = _readers()
    assert r.get("CENET_GROUP_DEPTH") == os.path.join("cenet_amd", "csrc", "gemm_group.hip")  # (read through grp_env)
    assert r.get("CENET_WGRAD_HOLD_MB") == os.path.join("cenet_amd", "ops", "infra.py")


def test_every_reader_is_a_row_and_every_row_has_a_reader():
    readers, rows = _readers(), _table()
    assert sorted(readers) == sorted(rows), (sorted(set(readers) - set(rows)), sorted(set(rows) - set(readers)))
    for n, where in rows.items():
        assert readers[n] == os.path.join("cenet_amd", where), (n, where, readers[n])


def test_every_row_is_set_by_a_test_or_a_tool():
    users = _users()
    unused = [n for n in _table() if not any(re.search(r"\b%s\b" % n, src) for src in users.values())]
    assert not unused, f"read by the library, named by no test or tool: {unused}"
