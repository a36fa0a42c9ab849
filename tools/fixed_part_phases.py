"""Profiling aid (build with -DQMPC_FIXED_STAMP): when each WAVE of the 64-row class's workgroup gets through the stages in front of
the sweep -- its loads landed, its arrival at barriers 1 and 2, its part of H assembled -- relative to the workgroup's start.
The first-class kernels that batch their kernel arguments also stamp the FRONT of the workgroup, which thread 0's start stamp
does not see: the wave enters the kernel, its batch of kernel arguments is back, the last load of its stage 0 is issued; with
them the split is entry -> kernargs back -> loads issued -> loads landed, every figure relative to the wave's own entry.
usage: QMPC_LIB=variants/<v>/libqmpc.so python tools/fixed_part_phases.py <config> <batch>"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from quadruped_ctrl_amd import workloads as W
from quadruped_ctrl_amd.binding import BatchedConvexMPC
cfg = sys.argv[1] if len(sys.argv) > 1 else "1"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
b = W.make_config(int(cfg), batch=B)
mpc = BatchedConvexMPC(0, max_batch=B, max_horizon=16)
mpc.set_max_stance(int((b["gait"] != 0).sum(1).max())); mpc.set_min_stance(int((b["gait"] != 0).sum(1).min()))
mpc.setup(b["dt"], b["horizon"], b["mu"], b["f_max"])
mpc.set_order_hint(0)
d = mpc.upload(b); o = mpc.alloc_outputs(B); inp, out = mpc.make_args(d, o)
for _ in range(3): mpc.solve_async(B, inp, out)
torch.cuda.synchronize()
clk = mpc.debug_clock(3 * B)
mpc.solve_async(B, inp, out); torch.cuda.synchronize()
c = clk.cpu().numpy().astype(np.float64)
t0, w = c[:B, 0:1], c[B:2 * B].reshape(B, 4, 4)
ok = (w > 0).all((1, 2))
rel = w[ok] - t0[ok][:, :, None]
names = ["loads landed", "at barrier 1", "at barrier 2", "H assembled"]
print(f"cfg{cfg} B={B}: cycles since the workgroup's start, median over {int(ok.sum())} workgroups (wave 0 | 1 | 2 | 3 ; last wave)")
for k, nm in enumerate(names):
    med = np.median(rel[:, :, k], axis=0)
    last = np.bincount(rel[:, :, k].argmax(1), minlength=4) / rel.shape[0]
    print(f"  {nm:14s} " + " | ".join(f"{m:7.0f}" for m in med) + f" ; max {np.median(rel[:, :, k].max(1)):7.0f}, last is wave "
          + " ".join(f"{k2}:{f:.2f}" for k2, f in enumerate(last)))
print("  thread 0's stamps: stage ends", (np.median(c[:B, 1:4] - c[:B, 0:1], axis=0)).astype(int).tolist())
front = c[2 * B:].reshape(B, 4, 4)
okf = ok & (front[:, :, 0] > 0).all(1) & (front[:, :, 2] > 0).all(1)
if okf.any():
    f, w2, s0 = front[okf], w[okf], t0[okf]
    ent = f[:, :, 0]
    rows = [("kernargs back", f[:, :, 1] - ent), ("loads issued", f[:, :, 2] - ent), ("loads landed", w2[:, :, 0] - ent),
            ("at barrier 1", w2[:, :, 1] - ent)]
    print(f"  since the WAVE's entry into the kernel, median over {int(okf.sum())} workgroups (wave 0 | 1 | 2 | 3 ; slowest wave)")
    for nm, v in rows:
        print(f"  {nm:14s} " + " | ".join(f"{m:7.0f}" for m in np.median(v, axis=0)) + f" ; max {np.median(v.max(1)):7.0f}")
    print(f"  thread 0's start stamp comes {np.median(s0[:, 0] - ent[:, 0]):.0f} cycles after wave 0's entry;"
          f" first wave's entry to last wave at barrier 1: {np.median(w2[:, :, 1].max(1) - ent.min(1)):.0f}")
