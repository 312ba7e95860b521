"""The fused prioritized replay buffer without a GPU: the C ABI of `gops_per_sample` / `_update` / `_fill`, their refusal codes (argument
checks before any HIP call: the pointers are never followed) and the path choice of `PrioritizedReplayBuffer` on a CPU device."""
import ctypes as C

import pytest

from abi_helpers import check_abi
from desc_helpers import BAD, UNS, P

from gops_amd import hip_backend as hb
from gops_amd.create_pkg.create_buffer import create_buffer


def test_abi_and_path_choice_on_a_cpu_device(tmp_path):
    check_abi(tmp_path, [("GopsPerKey", hb.GopsPerKey), ("GopsPerGather", hb.GopsPerGather)],
              ("gops_per_sample", "gops_per_update", "gops_per_fill"))
    kw = dict(buffer_name="prioritized_replay_buffer", trainer="off_serial_trainer", seed=0, obsv_dim=3, action_dim=1, buffer_max_size=8,
              buffer_device="cpu")
    assert create_buffer(**kw).path == "torch"
    with pytest.raises(RuntimeError, match="buffer_fused=True needs the buffer on the GPU"):
        create_buffer(buffer_fused=True, **kw)


def _sample(sum_tree=P, min_tree=P, N=8, size=4, B=4, u=P, n_keys=1, width=3, src=P):
    g = hb.GopsPerGather(n_keys=n_keys)
    g.key[0].src, g.key[0].dst, g.key[0].width = src, P, width
    return hb.lib().gops_per_sample(sum_tree, min_tree, N, size, 0.5, u, B, C.byref(g), P, P, None)


def _update(sum_tree=P, min_tree=P, maxp=P, N=8, idx=P, pr=P, B=4):
    return hb.lib().gops_per_update(sum_tree, min_tree, maxp, N, idx, pr, 0, B, 0.6, 1e-6, None)


def _fill(sum_tree=P, min_tree=P, N=8, ptr=0, n=4):
    return hb.lib().gops_per_fill(sum_tree, min_tree, P, N, ptr, n, None)


@pytest.mark.parametrize("call,kw,code", [
    (_sample, dict(sum_tree=None), BAD), (_sample, dict(min_tree=None), BAD), (_sample, dict(N=0), BAD), (_sample, dict(B=0), BAD),
    (_sample, dict(B=hb.PER_MAX_BATCH + 1), UNS), (_sample, dict(size=0), BAD), (_sample, dict(size=9), BAD), (_sample, dict(n_keys=hb.PER_MAX_KEYS + 1), UNS),
    (_sample, dict(width=-1), BAD), (_sample, dict(src=None), BAD), (_sample, dict(u=None), BAD), (_sample, dict(N=(1 << 29) + 1), UNS),
    (_update, dict(sum_tree=None), BAD), (_update, dict(min_tree=None), BAD), (_update, dict(maxp=None), BAD), (_update, dict(N=0), BAD),
    (_update, dict(B=0), BAD), (_update, dict(B=hb.PER_MAX_BATCH + 1), UNS), (_update, dict(idx=None), BAD), (_update, dict(pr=None), BAD),
    (_fill, dict(sum_tree=None), BAD), (_fill, dict(min_tree=None), BAD), (_fill, dict(N=0), BAD), (_fill, dict(n=0), BAD),
    (_fill, dict(n=9), BAD), (_fill, dict(ptr=8), BAD), (_fill, dict(ptr=-1), BAD)])
def test_refusal_codes(call, kw, code):
    assert call(**kw) == code
