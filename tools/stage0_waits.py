"""The compiled shape of stage 0's loads, checked without a GPU: compiles one class of qmpc_kernels.hip to device assembly
(as DESIGN 0 says: hipcc -O3 -std=c++17 --offload-arch=gfx950 -Wno-unused-value -DQMPC_RB=<class> --cuda-device-only -S) and
counts, in the first-class non-command kernel qmpc_solve_kernel<RB, false, false, false>, the waits that stand between the
kernel's entry and the issue of stage 0's last load:

  kernarg waits   s_waitcnt that name lgkmcnt(0) and follow a scalar load from the kernarg segment (s[0:1], or the copy of it
                  the kernel makes) with no other such wait in between -- every one is a scalar round trip in front of the
                  loads behind it;
  vmcnt waits     s_waitcnt that name vmcnt -- a wave that waits for memory before its last load is out makes two round trips.

The region is delimited by MARKERS, comment-only inline asm that costs nothing: it runs from the kernel's label to the line
"; qmpc stage0 loads end", less the lines between "; qmpc size order begin" and "; qmpc size order end" (the size-order
builder of launches of several rounds and the re-fetch behind it, which the one-round path jumps over).  The count is over
the TEXT of that region, every path through it together; the order-hint path is in it.  Only wait instructions, scalar loads
and the markers are read.

usage: python tools/stage0_waits.py [class ...]        (default: 1 6; prints one JSON line per class)
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
END, SO_BEGIN, SO_END = "; qmpc stage0 loads end", "; qmpc size order begin", "; qmpc size order end"


def assembly(rb, src=SRC):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, f"rb{rb}.s")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-value", f"-DQMPC_RB={rb}",
                        "--cuda-device-only", "-S", src, "-o", out], check=True, stderr=subprocess.DEVNULL)
        return open(out).read().splitlines()


def region(lines, rb):
    """The lines of the first-class non-command kernel from its label to the end-of-loads marker, the size-order part cut out."""
    label = f"_Z17qmpc_solve_kernelILi{rb}ELb0ELb0ELb0EEv10QmpcParams:"
    start = next(i for i, l in enumerate(lines) if l.startswith(label))
    out, skip = [], False
    for l in lines[start + 1:]:
        t = l.strip()
        if t.startswith(".Lfunc_end"):
            raise RuntimeError("no end-of-loads marker in the kernel: " + END)
        if t == SO_BEGIN:
            skip = True
        elif t == SO_END:
            skip = False
        elif t == END:
            return out
        elif not skip:
            out.append(t)
    raise RuntimeError("kernel text ended without the marker")


def count(lines, rb):
    reg = region(lines, rb)
    kernarg_waits = vm_waits = 0
    pending = False   # a kernarg load has been issued and not been waited for
    karg = {"s[0:1]"}
    for t in reg:
        m = re.match(r"s_mov_b64 (s\[\d+:\d+\]), s\[0:1\]", t)
        if m:
            karg.add(m.group(1))
        if t.startswith("s_load_") and any(f", {k}," in t for k in karg):
            pending = True
        elif t.startswith("s_waitcnt"):
            if "vmcnt" in t:
                vm_waits += 1
            if "lgkmcnt(0)" in t and pending:
                kernarg_waits += 1
                pending = False
    return {"class": rb, "kernarg_waits": kernarg_waits, "vmcnt_waits": vm_waits, "region_lines": len(reg)}


if __name__ == "__main__":
    for rb in [int(a) for a in sys.argv[1:]] or [1, 6]:
        print(json.dumps(count(assembly(rb), rb)))
