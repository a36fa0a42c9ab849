"""What the header checks of the CPU suites share: the functions and struct members a public header declares, and the
controller's array list (QMPC_CTRL_ARRAYS, csrc/qmpc_glue.h) against what the binding knows of it."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared(name):
    """The int qmpc_...( functions that include/<name> declares."""
    return set(re.findall(r"^int (qmpc_\w+)\(", open(os.path.join(ROOT, "include", name)).read(), re.M))


def members(hdr, struct):
    """The member names of `typedef struct { ... } <struct>;` in the header text hdr, in order (pointers and arrays too)."""
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [n for decl in body.split(";") if decl.strip() for n in re.findall(r"\*?(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]


def ctrl_arrays():
    """QMPC_CTRL_ARRAYS -> {array: (element type, width)}."""
    src = open(os.path.join(ROOT, "quadruped_ctrl_amd", "csrc", "qmpc_glue.h")).read()
    body = re.search(r"#define QMPC_CTRL_ARRAYS\(X\)((?:.*\\\n)*.*)", src).group(1)
    return {n: (t, int(w)) for t, n, w in re.findall(r"X\((\w+), (\w+), (\d+)\)", body)}


def binding_agrees_with_ctrl_arrays():
    """QMPC_CTRL_ARRAYS (csrc/qmpc_glue.h) is the one list of the controller's device arrays; what the binding still has
    to know about it (read()'s int32 arrays, view()'s widths and element types) matches it."""
    from quadruped_ctrl_amd import binding
    arrays = ctrl_arrays()
    assert arrays and {t for t, _ in arrays.values()} <= {"float", "int"}   # (read() moves 4-byte elements)
    assert {n for n, (t, _) in arrays.items() if t == "int"} == set(binding.CTRL_INT_ARRAYS)
    for k, n in binding.CTRL_VIEW_WIDTH.items():
        t, w = arrays[dict(leg_q="q").get(k, k)]
        assert w == n and t == ("int" if k in ("safe", "counter") else "float"), k
