"""The run-time route switches of the library stay the ten that a test forces: one reader (icamd_env_int in csrc/common.h), no other
getenv in csrc/, every switch in README.md's table and set by at least one test.  Reads source text only; the library is not loaded."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "imageclassification_amd", "csrc")

SWITCHES = {
    "ICAMD_ATTN_LONG",
    "ICAMD_CONV3X3_HALO",
    "ICAMD_CONV3X3_RESIDENT",
    "ICAMD_PW_RESIDENT",
    "ICAMD_GEMM_NT",
    "ICAMD_GEMM_TN",
    "ICAMD_WGRAD_RING",
    "ICAMD_WGRAD_HALO",
    "ICAMD_LN_NV3",
    "ICAMD_DWCONV_ROWS",
}


def _sources():
    paths = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert paths
    return {os.path.basename(p): open(p, encoding="utf-8").read() for p in paths}


def _helper_body(common):
    m = re.search(r"static inline int icamd_env_int\(const char\* name, int dflt\) \{(.*?)\n\}", common, re.S)
    assert m, "icamd_env_int is gone from common.h"
    return m.group(1)


def test_getenv_only_inside_the_helper():
    src = _sources()
    body = _helper_body(src["common.h"])
    assert body.count("getenv(") == 1
    for name, text in src.items():
        expected = 1 if name == "common.h" else 0
        assert text.count("getenv(") == expected, f"{name}: getenv outside icamd_env_int"


def test_helper_reads_exactly_the_ten_switches():
    calls = []
    for name, text in _sources().items():
        for m in re.finditer(r"icamd_env_int\(\s*([^,)]*)", text):
            arg = m.group(1).strip()
            if arg == "const char* name":        # the definition itself
                continue
            lit = re.fullmatch(r'"(\w+)"', arg)
            assert lit, f"{name}: icamd_env_int called with {arg!r}, not a string literal"
            calls.append(lit.group(1))
    assert set(calls) == SWITCHES
    assert len(calls) == len(SWITCHES), f"a switch has more than one reader: {sorted(calls)}"


def test_every_switch_is_in_the_readme_table():
    rows = [l for l in open(os.path.join(ROOT, "README.md"), encoding="utf-8") if l.startswith("| `ICAMD_")]
    in_table = {re.match(r"\| `(\w+)`", l).group(1) for l in rows}
    assert in_table == SWITCHES


def test_every_switch_is_set_by_a_test():
    me = os.path.abspath(__file__)
    texts = [open(p, encoding="utf-8").read() for p in glob.glob(os.path.join(ROOT, "tests", "*.py")) if os.path.abspath(p) != me]
    for s in sorted(SWITCHES):
        # set, not merely named: a keyword of dict(os.environ, ..., NAME=...) or an assignment to env["NAME"]
        sets = re.compile(r"dict\(os\.environ,[^)]*\b" + s + r"\s*=|\[[\"']" + s + r"[\"']\]\s*=[^=]")
        assert any(sets.search(t) for t in texts), f"no test sets {s}"
