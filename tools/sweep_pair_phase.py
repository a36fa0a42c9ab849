"""Profiling aid (build with -DQMPC_SWEEP_STAMP=<k0>, k0 a multiple of 4 inside a block of sixteen columns, e.g. 20): shader-clock
stamps of the wave that PRODUCES the next step's pivot pairs in the 64-row classes' sweep (its lane 0), in the step that starts at
pivot k0 -- the barrier is passed, the step's LDS loads are back, its last store is issued, the next barrier is passed -- and the
whole sweep by thread 0's stage stamps.  A step is one pivot pair where the class publishes one pair per barrier, two where it
publishes two (Cfg::SWP_PAIRS): the tool prints the step and the figure per pair.
usage: QMPC_LIB=variants/<v>/libqmpc.so python tools/sweep_pair_phase.py <config> <batch> [pairs per step, default 1]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from quadruped_ctrl_amd import workloads as W
from quadruped_ctrl_amd.binding import BatchedConvexMPC
cfg = sys.argv[1] if len(sys.argv) > 1 else "1"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
pairs = int(sys.argv[3]) if len(sys.argv) > 3 else 1
b = W.make_config(int(cfg), batch=B)
mpc = BatchedConvexMPC(0, max_batch=B, max_horizon=16)
mpc.set_max_stance(int((b["gait"] != 0).sum(1).max())); mpc.set_min_stance(int((b["gait"] != 0).sum(1).min()))
mpc.setup(b["dt"], b["horizon"], b["mu"], b["f_max"])
mpc.set_order_hint(0)
d = mpc.upload(b); o = mpc.alloc_outputs(B); inp, out = mpc.make_args(d, o)
for _ in range(3): mpc.solve_async(B, inp, out)
torch.cuda.synchronize()
clk = mpc.debug_clock(2 * B)
mpc.solve_async(B, inp, out); torch.cuda.synchronize()
c = clk.cpu().numpy().astype(np.float64)
s = c[B:, :4]
s = s[(s > 0).all(1)]
dd = np.diff(s, axis=1)
step = s[:, 3] - s[:, 0]
names = ["barrier passed -> loads back", "loads back -> last store issued", "last store issued -> next barrier passed"]
print(f"cfg{cfg} B={B}: one sweep step of {pairs} pair(s), producing wave (median cycles over {len(s)} robots): "
      f"step {np.median(step):.0f}, per pair {np.median(step) / pairs:.0f}")
for k, nm in enumerate(names):
    print(f"  {nm:42s} {np.median(dd[:, k]):7.0f}   {100 * np.median(dd[:, k]) / np.median(step):5.1f} %")
sw = c[:B, 4] - c[:B, 3]
sw = sw[(c[:B, 3] > 0) & (c[:B, 4] > 0)]
print(f"  whole sweep (thread 0, stage 3): median {np.median(sw):.0f}, min {sw.min():.0f}, max {sw.max():.0f}")
