"""On-policy batched sampling on the GPU: `DeviceEnvSampler`'s closed loop plus what the reference's OnSampler adds for PPO
(gops/trainer/sampler/on_sampler.py:74-187) - the value targets `ret` and the generalised advantages `adv`.

The reference evaluates the value net once per step and once per finished segment and runs `_finish_trajs` per environment on the
host.  Here the N environments advance `steps_per_sample` = T steps, then ONE value forward runs over all T N observations and one
over all T N next observations (`gops_mlp_forward`), and `gops_gae` walks every environment's T steps backwards in one launch.
A segment ends where the episode terminated (`done`), where it hit `max_episode_steps` (`time_limited`), and at the horizon T - 1;
its last value estimate is `value(obs2) (1 - done)`.

`sample()` returns the reference's on-policy columns as device tensors, flattened time-major as `DeviceEnvSampler` concatenates
them: `obs, act, rew, done, logp, time_limited, ret, adv` + the info / next_info keys.
"""
import time

import torch

from gops_amd import hip_backend as hb
from gops_amd.trainer.sampler.device_env_sampler import DeviceEnvSampler
from gops_amd.utils.tensorboard_setup import tb_tags


class OnPolicyDeviceSampler(DeviceEnvSampler):
    def __init__(self, cfg: dict, env_model, *, gamma: float = 0.99, gae_lambda: float = 0.95, **kwargs):
        super().__init__(cfg, env_model, **kwargs)
        self.gamma, self.gae_lambda = gamma, gae_lambda
        self._value_net = None

    def _values(self, obs: torch.Tensor) -> torch.Tensor:
        """value(obs) [rows] through `gops_mlp_forward` (every call has T N rows)."""
        mlp = self.networks.value.hip_mlp()
        if self._value_net is None or self._value_net.batch != obs.shape[0]:
            self._value_net = hb.MlpNet(mlp, obs.shape[0], device=self.device)
        else:
            self._value_net.mlp = mlp
        return self._value_net.forward(obs).view(-1)

    @torch.no_grad()
    def sample(self):
        t0 = time.time()
        policy = self.networks.policy
        T, N = self.steps, self.n
        if self._choose_path():   # one launch: the kernel keeps the `time_limited` and `end` columns itself
            out = self._sample_fused()
            batch = self._fused_batch(out)
            limited, end = out["time_limited"].flatten() != 0, out["end"]
        else:
            zeros = torch.zeros(self.n, device=self.device)
            chunks, ends, limited = [], [], []
            for s in range(self.steps):
                row, over = self._step_once(policy, zeros)
                tlim = over & (row["done"] == 0)
                chunks.append(row)
                limited.append(tlim)
                ends.append(torch.ones_like(over) if s == self.steps - 1 else over)
            batch = {k: torch.cat([c[k] for c in chunks]) for k in chunks[0]}
            limited, end = torch.cat(limited), torch.cat(ends).to(torch.float32).view(T, N)
        val, val_next = self._values(batch["obs"].contiguous()), self._values(batch["obs2"].contiguous())
        ret, adv = hb.gae(batch["rew"].view(T, N), val.view(T, N), val_next.view(T, N), batch["done"].view(T, N),
                          end, self.gamma, self.gae_lambda)
        del batch["obs2"]
        batch.update(time_limited=limited, ret=ret.view(-1), adv=adv.view(-1))
        self.total += N * T
        return batch, {tb_tags["sampler_time"]: (time.time() - t0) * 1000}
