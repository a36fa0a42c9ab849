"""The compiled shape of stage 2 (assembly of H_red into registers) with respect to its LDS loads, checked without a GPU:
compiles one class of qmpc_kernels.hip to device assembly (as tools/engine_iter_shape.py does) and counts, in the first-class
non-command kernel qmpc_solve_kernel<RB, false, false, false>, the LDS load mnemonics in the text between the markers
"; qmpc assemble begin" (behind barrier 2) and "; qmpc sweep begin": every path of the stage laid out there together (the three
start axes of `fill`, the x_drag block, the gradient), once per copy of the solve in the kernel.

Stage 2 reads the E tables as 16-byte pairs (csrc/qmpc_etab.h): CW = 16 elements per thread and start axis, ds_read_b128 each.

usage: python tools/etab_shape.py [class ...]        (default: 1 6; prints one JSON line per class)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from engine_iter_shape import assembly, kernel_text  # noqa: E402
from sweep_shape import regions  # noqa: E402

BEGIN, END = "; qmpc assemble begin", "; qmpc sweep begin"
OPS = ("ds_read_b128", "ds_read2_b64", "ds_read_b64", "ds_read2st64_b64")


def count(lines, rb):
    out = []
    for reg in regions(kernel_text(lines, rb), BEGIN, END):
        ops = [t.split()[0] for t in reg if t and t[0] not in ";." and not t.endswith(":")]
        c = {op: sum(o == op for o in ops) for op in OPS}
        c["ds_read"] = sum(o.startswith("ds_read") for o in ops)
        c["instructions"] = len(ops)
        out.append(c)
    return {"class": rb, "stages": out}


if __name__ == "__main__":
    for rb in [int(a) for a in sys.argv[1:]] or [1, 6]:
        print(json.dumps(count(assembly(rb), rb)))
