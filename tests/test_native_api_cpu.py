"""Every `dtfk_*` kernel entry point has one declaration, and its definition sees it.

`extern "C"` names are not mangled: a prototype that drifts from its definition
links cleanly and the launcher then reads its arguments from the wrong registers.
The compiler reports the drift ("conflicting types") only when the defining file
includes the declaring header, so this test keeps two rules over the text of
`csrc/`:

* no `.cpp` / `.hip` carries a prototype of a `dtfk_*` function of its own;
* every `dtfk_*` function defined under `csrc/` is declared in exactly one header
  under `csrc/`, and the defining file includes that header directly.

The scanner looks only for `dtfk_` declarations and `#include` lines.
"""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "csrc")
# the build's include directories (_build.py common_inc), after the includer's own
INCLUDE_DIRS = ("", "kernels", "runtime")

_COMMENT = re.compile(r"//[^\n]*|/\*.*?\*/", re.S)
_NAME = re.compile(r"\bdtfk_\w+\s*\(")
_INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', re.M)
_NOT_A_TYPE = {"return", "else", "case", "throw", "new", "delete", "sizeof", "co_return"}


def scan(text):
    """The `dtfk_*` declarations of one source text: a list of (name, kind), kind
    "definition" (a body follows the parameter list) or "prototype" (a `;` does).
    Calls are no declarations: a declaration has a type in front of the name."""
    text = _COMMENT.sub(" ", text)
    found = []
    for m in _NAME.finditer(text):
        # the token in front of the name: a type (an identifier, possibly `*` / `&` after it)
        head = text[:m.start()].rstrip()
        head = head.rstrip("*&").rstrip() if head.endswith(("*", "&")) else head
        word = re.search(r"[A-Za-z_]\w*$", head)
        if word is None or word.group(0) in _NOT_A_TYPE:
            continue
        # the end of the parameter list
        depth, i = 1, m.end()
        while i < len(text) and depth:
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        tail = text[i:].lstrip()
        name = m.group(0).rstrip("(").rstrip()
        if tail.startswith("{"):
            found.append((name, "definition"))
        elif tail.startswith(";"):
            found.append((name, "prototype"))
    return found


def includes(text):
    return _INCLUDE.findall(_COMMENT.sub(" ", text))


def check(files):
    """files: {path relative to csrc: text}.  Returns the list of violations."""
    errors = []
    declared = {}   # name -> headers that declare it
    decls = {rel: scan(text) for rel, text in files.items()}
    for rel, found in sorted(decls.items()):
        for name, kind in found:
            if kind != "prototype":
                continue
            if rel.endswith(".h"):
                declared.setdefault(name, []).append(rel)
            else:
                errors.append(f"{rel}: prototype of {name} outside a header")
    for rel, found in sorted(decls.items()):
        seen = set()
        for inc in includes(files[rel]):
            for d in (os.path.dirname(rel),) + INCLUDE_DIRS:
                seen.add(os.path.normpath(os.path.join(d, inc)))
        for name, kind in found:
            if kind != "definition":
                continue
            where = declared.get(name, [])
            if len(where) != 1:
                errors.append(f"{rel}: {name} is declared in {len(where)} headers {where}, expected exactly one")
            elif where[0] not in seen and where[0] != rel:
                errors.append(f"{rel}: defines {name} without including {where[0]}")
    return errors


def _tree():
    files = {}
    for root, _, names in os.walk(CSRC):
        for n in names:
            if n.endswith((".h", ".hip", ".cpp")):
                p = os.path.join(root, n)
                with open(p, encoding="utf-8") as f:
                    files[os.path.relpath(p, CSRC)] = f.read()
    return files


def test_no_prototype_outside_headers_and_every_definition_sees_its_declaration():
    files = _tree()
    defined = [n for found in map(scan, files.values()) for n, k in found if k == "definition"]
    assert len(defined) > 100, "the scanner found too few dtfk_ definitions to mean anything"
    assert len(defined) == len(set(defined)), "a dtfk_ function is defined twice"
    assert check(files) == []


def test_scanner_reports_a_stray_prototype_and_a_missing_include():
    header = ('#pragma once\nextern "C" {\n// the launcher\n'
              "hipError_t dtfk_demo(const float* x,\n                     int n, hipStream_t s);\n"
              "int dtfk_demo_rows(int n);\n}\n")
    good = ('#include "common.h"\n#include "demo_api.h"\nextern "C" hipError_t dtfk_demo(const float* x, int n,\n'
            "    hipStream_t s) {\n  return launch(x, n, s);\n}\nint dtfk_demo_rows(int n) { return (n + 63) / 64; }\n")
    caller = ('#include "kernels/demo_api.h"\nvoid f() {\n  ck(dtfk_demo(x, dtfk_demo_rows(n), cs()), "demo");\n'
              "  dtfk_demo_rows(3);\n  return dtfk_demo_rows(4) * 2;\n}\n")
    base = {"kernels/demo_api.h": header, "kernels/demo.hip": good, "bind_demo.cpp": caller}
    assert scan(good) == [("dtfk_demo", "definition"), ("dtfk_demo_rows", "definition")]
    assert scan(caller) == []
    assert check(base) == []

    stray = dict(base, **{"bind_demo.cpp": 'extern "C" {\nint dtfk_demo_rows(long n);\n}\n' + caller})
    assert check(stray) == ["bind_demo.cpp: prototype of dtfk_demo_rows outside a header"]

    blind = dict(base, **{"kernels/demo.hip": good.replace('#include "demo_api.h"\n', "")})
    assert check(blind) == ["kernels/demo.hip: defines dtfk_demo without including kernels/demo_api.h",
                            "kernels/demo.hip: defines dtfk_demo_rows without including kernels/demo_api.h"]

    # an include that only sits in a comment does not count, nor does an indirect one
    commented = dict(base, **{"kernels/demo.hip": good.replace('#include "demo_api.h"', '// #include "demo_api.h"')})
    assert len(check(commented)) == 2

    twice = dict(base, **{"kernels/other_api.h": "int dtfk_demo_rows(int n);\n"})
    assert check(twice) == ["kernels/demo.hip: dtfk_demo_rows is declared in 2 headers "
                            "['kernels/demo_api.h', 'kernels/other_api.h'], expected exactly one"]

    undeclared = dict(base, **{"kernels/demo_api.h": header.replace("int dtfk_demo_rows(int n);\n", "")})
    assert check(undeclared) == ["kernels/demo.hip: dtfk_demo_rows is declared in 0 headers [], expected exactly one"]
