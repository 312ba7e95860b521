"""Time the prioritized replay buffer on the GPU two ways: `buffer_fused=True` (csrc/per_buffer.hip: one launch per operation) and the
torch path (`buffer_fused=False`, rounds of small torch kernels) of the same build, in the same run.

    python tools/microbench/per_buffer.py            # prints one JSON line per capacity

Rows of the vehicle envs: obs 126 (pyth_veh3dofconti, pre_horizon 30) and its additional_info.  Capacities 2^20 and 10^6 (leaves on
two levels), every slot stored and every priority updated once before the clock starts.  Two timed operations: a replay step -
`sample_batch(256)` + `update_batch(idx, priorities)` with fp32 device priorities, as OffSerialTrainer issues them - and a store of
1024 rows (`add_tensors`).  Each: 5 warm-up calls, then 50 timed calls per path, the two paths ALTERNATING, every call bracketed by
a device synchronise; median and min .. max in ms, and torch / hip of the medians.  Afterwards, in a pass of its own, the device
activities (kernels and copies) of one call of each operation are counted from a torch.profiler trace.
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT]

from gops_amd.create_pkg.create_buffer import create_buffer  # noqa: E402

WARMUP, TIMED, BATCH, STORE = 5, 50, 256, 1024
INFO = {"state": (6,), "ref_points": (31, 4), "path_num": (), "u_num": (), "ref_time": (), "ref": (4,)}


def make(N, fused):
    buf = create_buffer(buffer_name="prioritized_replay_buffer", trainer="off_serial_trainer", seed=0, obsv_dim=126, action_dim=2,
                        buffer_max_size=N, buffer_device="cuda", buffer_fused=fused,
                        additional_info={k: {"shape": s, "dtype": np.float32} for k, s in INFO.items()})
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = {k: torch.randn((8192,) + tuple(v.shape[1:]), device="cuda", generator=g) for k, v in buf.buf.items()}
    for _ in range(0, N, 8192):
        buf.add_tensors(rows)
    for lo in range(N - 1, 2 * N - 1, 8192):   # every leaf its own priority
        idx = torch.arange(lo, min(lo + 8192, 2 * N - 1), device="cuda", dtype=torch.int32)
        buf.update_batch(idx, torch.rand(idx.numel(), device="cuda", generator=g))
    return buf, {k: v[:STORE] for k, v in rows.items()}


def operations(buf, rows):
    err = torch.rand(BATCH, device="cuda")
    parts = dict(sample_batch=lambda: buf.sample_batch(BATCH), store=lambda: buf.add_tensors(rows))
    last = {}

    def step():
        last["batch"] = buf.sample_batch(BATCH)
        buf.update_batch(last["batch"]["idx"], err)

    parts["update_batch"] = lambda: buf.update_batch(last["batch"]["idx"], err)
    return dict(step=step, store=parts["store"]), parts


def timed(fns):
    """fns: path -> callable; the paths alternate within every repetition."""
    ms = {k: [] for k in fns}
    for rep in range(WARMUP + TIMED):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep >= WARMUP:
                ms[k].append((time.perf_counter() - t0) * 1000)
    return {k: dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4)) for k, v in ms.items()}


def device_activities(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    for N in (1 << 20, 10 ** 6):
        bufs = {path: make(N, path == "hip") for path in ("hip", "torch")}
        assert all(b.path == path for path, (b, _) in bufs.items())
        ops = {path: operations(*bufs[path]) for path in bufs}
        row = dict(capacity=N, batch=BATCH, store_rows=STORE)
        for name in ("step", "store"):
            row[name] = timed({path: ops[path][0][name] for path in ops})
            row[name]["torch_over_hip"] = round(row[name]["torch"]["median_ms"] / row[name]["hip"]["median_ms"], 2)
        print(json.dumps(row), flush=True)
        ops["hip"][0]["step"](), ops["torch"][0]["step"]()   # (update_batch below reads the step's batch)
        print(json.dumps(dict(capacity=N, device_activities={path: {name: device_activities(fn) for name, fn in ops[path][1].items()}
                                                               for path in ops})), flush=True)
        del bufs, ops
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
