"""CPU test (-m "not gpu") of the rule "a function that crosses translation units is declared once, in csrc/internal.hpp
(or, for the C ABI, include/yolat_hip.h), and both its definer and its callers include that declaration", per csrc/*.hip:

  * a host-only syntax pass (hipcc --cuda-host-only -fsyntax-only -Wmissing-prototypes, the Makefile's language flags)
    reports every non-static function that is defined without a declaration in sight.  None of them may be one of the
    library's own functions (yl_* / yolat_*): a definition its header does not see can change its return type or a default
    argument and still link.  Kernels (k_*) are ignored, many are non-static by design.
  * no .hip declares a yl_ function by hand: every line that starts with a return type followed by yl_<name>( must be the
    head of a definition, i.e. be followed by a body in that file."""
import glob
import os
import re
import subprocess

import pytest

from kernel_meta import CSRC, find_hipcc

SOURCES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hip")))
HEAD = re.compile(r"^[A-Za-z_][^\n;(){}=]*?[\s*&](yl_\w+)\(", re.M)


def test_sources_found():
    assert len(SOURCES) >= 25, SOURCES


@pytest.mark.parametrize("name", SOURCES)
def test_definitions_see_their_declaration(name):
    hipcc = find_hipcc()
    if hipcc is None:
        pytest.skip("hipcc is not on this machine")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-fsyntax-only", "-std=c++17",
                        "-Wmissing-prototypes", os.path.join(CSRC, name)], cwd=CSRC, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    found = re.findall(r"no previous prototype for function '(\w+)'", r.stderr)
    print(name, found)
    assert not [f for f in found if f.startswith(("yl_", "yolat_"))], found


def after_params(text, i):
    """text from the character behind the parenthesis that closes the one at text[i], comments and blanks skipped"""
    depth = 0
    while True:
        depth += (text[i] == "(") - (text[i] == ")")
        i += 1
        if depth == 0:
            break
    rest = text[i:]
    while True:
        stripped = re.sub(r"^(\s+|//[^\n]*|/\*.*?\*/)", "", rest, count=1, flags=re.S)
        if stripped == rest:
            return rest
        rest = stripped


@pytest.mark.parametrize("name", SOURCES)
def test_no_hand_written_declaration(name):
    with open(os.path.join(CSRC, name)) as f:
        text = f.read()
    heads = [(m.group(1), after_params(text, m.end() - 1)[:1]) for m in HEAD.finditer(text)]
    print(name, [h[0] for h in heads])
    assert not [fn for fn, nxt in heads if nxt != "{"], heads
