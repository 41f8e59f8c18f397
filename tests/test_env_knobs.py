"""The environment variables the package and the library read are exactly the ones
INTEGRATION.md documents (section 5): a new knob has to be written down to pass."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorchrec_amd")

_PY_READ = re.compile(r"""os\.(?:environ\.(?:get|setdefault|pop)\(|environ\[|getenv\()\s*["']([^"']+)["']""")
_C_READ = re.compile(r"""\bgetenv\(\s*"([^"]+)"\s*\)""")


def _read_in_code():
    names = set()
    for d, dirs, files in os.walk(PKG):
        dirs[:] = [x for x in dirs if x not in ("lib", "__pycache__")]  # build products
        for f in files:
            pat = _PY_READ if f.endswith(".py") else _C_READ if f.endswith((".hip", ".h")) else None
            if pat is None:
                continue
            with open(os.path.join(d, f), encoding="utf-8") as fh:
                names.update(pat.findall(fh.read()))
    return names


def _documented():
    with open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8") as fh:
        text = fh.read()
    section = text.split("## 5. Environment variables", 1)[1].split("\n## ", 1)[0]
    return set(re.findall(r"^\| `([A-Z][A-Z0-9_]*)` \|", section, flags=re.M))


def test_environment_reads_match_the_documented_table():
    code, doc = _read_in_code(), _documented()
    assert code, "the scan found no environment reads at all: the patterns are stale"
    assert code == doc, (f"read but not in INTEGRATION.md section 5: {sorted(code - doc)}; "
                         f"documented but not read: {sorted(doc - code)}")
