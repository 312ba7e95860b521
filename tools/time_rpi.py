"""Time RPI's policy evaluation on the oscillator example (B = 64, POLY value of degree 2): ms per `local_update` and us per gradient
step with the step count forced to a fixed number, for the single-launch device path and for the project's own eager host path:
    python tools/time_rpi.py [steps per local_update, default 1000]
One warm-up `local_update`, then REPEATS timed ones; the median and the min .. max spread are reported.  The count is forced by a
learning rate of 1e-8 (the work per step does not depend on it): the held-out Hamiltonian norm then never falls to 0.88 of its start,
so every local_update runs to `max_step_update_value`.  The device figure is the whole `local_update`: drawing the reset pool on the
host, its upload, the launch and the one sync; the pool's share (draw + upload, no launch) is timed on its own and printed too."""
import os
import statistics
import sys
import time

import numpy as np
import torch

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
from gops_amd.create_pkg.create_alg import create_alg  # noqa: E402

REPEATS = 7


def make(use_gpu, steps):
    np.random.seed(0)
    torch.manual_seed(0)
    alg = create_alg(algorithm="RPI", trainer="on_serial_trainer", seed=0, cnn_shared=False, use_gpu=use_gpu, is_adversary=True,
                     env_id="pyth_oscillatorconti", obsv_dim=2, action_dim=1, action_type="continu",
                     action_high_limit=np.ones(1, dtype=np.float32), action_low_limit=-np.ones(1, dtype=np.float32),
                     value_func_name="StateValue", value_func_type="POLY", value_degree=2, value_add_bias=True,
                     policy_act_distribution="default", max_newton_iteration=50, max_step_update_value=steps, print_interval=10 ** 9,
                     learning_rate=1e-8, gamma_atte=2.0, reset_batch_size=64, sample_batch_size=64, fixed_initial_state=[0.5, -0.5],
                     initial_state_range=[1.5, 1.5], state_threshold=[5.0, 5.0], lower_step=200, upper_step=700)
    w0 = torch.tensor([[1.0, 0.2, 0.5]])
    alg.networks.value.v.weight.data.copy_(w0)
    alg.networks.value_target.v.weight.data.copy_(w0)
    return alg


def run(use_gpu, steps):
    alg = make(use_gpu, steps)
    times = []
    for it in range(REPEATS + 1):
        if use_gpu:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        info = alg.local_update(None, it + 1)
        if use_gpu:
            torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        assert info["num_update_value"] == steps, info
    times = times[1:]
    med = statistics.median(times)
    print(f"RPI oscillator B=64 {'device (one launch)' if use_gpu else 'eager host path'}: {steps} steps per local_update, "
          f"median {med:.3f} ms (min {min(times):.3f} .. max {max(times):.3f}, {REPEATS} repeats after 1 warm-up), "
          f"{med * 1e3 / steps:.2f} us per gradient step")
    if use_gpu:
        pool = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            alg.reset_source.pool(steps + 1).to("cuda")
            torch.cuda.synchronize()
            pool.append((time.perf_counter() - t0) * 1e3)
        alg.reset_source.consume(0)   # (leave np.random where it was)
        print(f"    of which the reset pool ({steps + 1} draws on the host + upload): median {statistics.median(pool):.3f} ms "
              f"(min {min(pool):.3f} .. max {max(pool):.3f})")
    return med


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    dev = run(True, n)
    host = run(False, n)
    print(f"eager host / device: {host / dev:.1f}x")
