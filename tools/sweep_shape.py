"""The compiled shape of the 64-row classes' sweep loop (stage 3 of qmpc_kernels.hip), checked without a GPU: compiles one class
to device assembly (hipcc -O3 -std=c++17 --offload-arch=gfx950 -Wno-unused-value -DQMPC_RB=<class> --cuda-device-only -S) and
counts, in the first-class non-command kernel qmpc_solve_kernel<RB, false, false, false>:

  loop      the text between "; qmpc sweep begin" and "; qmpc sweep end": ONE block of sixteen pivot columns (eight pivot pairs;
            the loop over the four blocks is not unrolled), every wave's paths laid out there together -- barriers (s_barrier),
            lgkm_waits (s_waitcnt that name lgkmcnt) and instructions;
  producer  each stretch between "; qmpc sweep producer begin" and "; qmpc sweep producer end" inside it: the path of the wave
            that publishes the next step's pivot pairs, one per step of the block -- load_waits (waits that name lgkmcnt from the
            path's first LDS load on: what the wave stands for once its loads are issued), ds_loads, ds_stores and instructions.

The kernel holds one copy of the loop per instantiation of the solve in it (staged or not); every copy is counted and the
copies are expected to agree on barriers and producer paths.  Only s_barrier, s_waitcnt, ds_ mnemonics and the markers are read.

usage: python tools/sweep_shape.py [class ...]        (default: 1 6; prints one JSON line per class)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from engine_iter_shape import assembly, kernel_text  # noqa: E402

BEGIN, END = "; qmpc sweep begin", "; qmpc sweep end"
P_BEGIN, P_END = "; qmpc sweep producer begin", "; qmpc sweep producer end"


def instructions(reg):
    return [t for t in reg if t and t[0] not in ";." and not t.endswith(":")]


def is_lgkm_wait(t):
    return t.split()[0] == "s_waitcnt" and "lgkmcnt" in t


def regions(text, a, b):
    """The stretches of text between marker a and the next marker b (markers alternate, a first)."""
    out, start = [], None
    for i, t in enumerate(text):
        if t == a:
            if start is not None:
                raise RuntimeError(f"marker {a!r} twice without {b!r}")
            start = i
        elif t == b:
            if start is None:
                raise RuntimeError(f"marker {b!r} without {a!r}")
            out.append(text[start + 1:i])
            start = None
    if start is not None or not out:
        raise RuntimeError(f"markers {a!r} / {b!r}: {len(out)} closed stretches, one left open: {start is not None}")
    return out


def producer(reg):
    ins = instructions(reg)
    first = next((i for i, t in enumerate(ins) if t.startswith("ds_read")), 0)  # (no load: they are issued in front of the path)
    return {"load_waits": sum(is_lgkm_wait(t) for t in ins[first:]),
            "ds_loads": sum(t.startswith("ds_read") for t in ins), "ds_stores": sum(t.startswith("ds_write") for t in ins),
            "instructions": len(ins)}


def loop(reg):
    ins = instructions(reg)
    return {"barriers": sum(t.split()[0] == "s_barrier" for t in ins), "lgkm_waits": sum(is_lgkm_wait(t) for t in ins),
            "instructions": len(ins), "producer": [producer(p) for p in regions(reg, P_BEGIN, P_END)]}


def count(lines, rb):
    return {"class": rb, "loops": [loop(r) for r in regions(kernel_text(lines, rb), BEGIN, END)]}


if __name__ == "__main__":
    for rb in [int(a) for a in sys.argv[1:]] or [1, 6]:
        print(json.dumps(count(assembly(rb), rb)))
