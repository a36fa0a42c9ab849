"""The compiled shape of one iteration of the event-form engine (stage 5 of qmpc_kernels.hip), checked without a GPU:
compiles one class to device assembly (hipcc -O3 -std=c++17 --offload-arch=gfx950 -Wno-unused-value -DQMPC_RB=<class>
--cuda-device-only -S) and counts, in the first-class non-command kernel qmpc_solve_kernel<RB, false, false, false>, in the
LDS-pool instantiation of the iteration (the markers are emitted by that instantiation only):

  region "select"   from the loop top to "delta known": the search for the next constraint, z = H^-1 c, the trips over the
                    stored events, delta / cn / sp;
  region "step"     from "delta known" to the loop end: ratio test, step, the add or drop event;
  region "hcol"     inside "select": the addresses and loads of the two columns of H^-1.

Per region: lgkm_waits (s_waitcnt that name lgkmcnt: the wave stands until LDS / scalar memory has answered), branches
(s_cbranch_*), saveexec (*_saveexec_*: an exec-mask region), ds (LDS instructions) and instructions (every instruction line).

The regions are delimited by MARKERS, comment-only inline asm that costs nothing ("; qmpc iter top", "; qmpc iter delta",
"; qmpc iter end", "; qmpc iter hcol begin", "; qmpc iter hcol end").  The count is over the TEXT between two markers, every
path laid out there together.  Only wait, branch, exec and ds_ mnemonics and the markers are read.

usage: python tools/engine_iter_shape.py [class ...]        (default: 1 6; prints one JSON line per class)
"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(ROOT, "quadruped_ctrl_amd", "csrc", "qmpc_kernels.hip")
TOP, DELTA, END = "; qmpc iter top", "; qmpc iter delta", "; qmpc iter end"
HCOL_B, HCOL_E = "; qmpc iter hcol begin", "; qmpc iter hcol end"


def assembly(rb, src=SRC):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, f"rb{rb}.s")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-value", f"-DQMPC_RB={rb}",
                        "--cuda-device-only", "-S", src, "-o", out], check=True, stderr=subprocess.DEVNULL)
        return open(out).read().splitlines()


def kernel_text(lines, rb):
    label = f"_Z17qmpc_solve_kernelILi{rb}ELb0ELb0ELb0EEv10QmpcParams:"
    start = next(i for i, l in enumerate(lines) if l.startswith(label))
    out = []
    for l in lines[start + 1:]:
        t = l.strip()
        if t.startswith(".Lfunc_end"):
            return out
        out.append(t)
    raise RuntimeError("kernel text without an end")


def between(text, a, b):
    ia = [i for i, t in enumerate(text) if t == a]
    ib = [i for i, t in enumerate(text) if t == b]
    if len(ia) != 1 or len(ib) != 1 or ia[0] >= ib[0]:
        raise RuntimeError(f"markers {a!r} / {b!r}: found {len(ia)} / {len(ib)} (one of each, in this order, is expected)")
    return text[ia[0] + 1:ib[0]]


def tally(reg):
    c = {"lgkm_waits": 0, "branches": 0, "saveexec": 0, "ds": 0, "instructions": 0}
    for t in reg:
        if not t or t[0] in ";." or t.endswith(":"):
            continue
        op = t.split()[0]
        c["instructions"] += 1
        if op == "s_waitcnt" and "lgkmcnt" in t:
            c["lgkm_waits"] += 1
        elif op.startswith("s_cbranch_"):
            c["branches"] += 1
        elif re.search(r"_saveexec_", op):
            c["saveexec"] += 1
        elif op.startswith("ds_"):
            c["ds"] += 1
    return c


def count(lines, rb):
    text = kernel_text(lines, rb)
    return {"class": rb, "select": tally(between(text, TOP, DELTA)), "step": tally(between(text, DELTA, END)),
            "hcol": tally(between(text, HCOL_B, HCOL_E))}


if __name__ == "__main__":
    for rb in [int(a) for a in sys.argv[1:]] or [1, 6]:
        print(json.dumps(count(assembly(rb), rb)))
