"""Weight gradients of one workload from the default weight-gradient GEMM against the exact three-plane bf16 GEMM
(GOPS_VF_DW_EXACT), both in this process - the variant travels in the descriptors the algorithm class builds:
    python tools/dw_compare.py [workload]"""
import contextlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import alg_kwargs  # noqa: E402
from gops_amd import hip_backend as hb  # noqa: E402
from gops_amd.create_pkg.create_alg import create_alg  # noqa: E402
from gops_amd.utils.synthetic import CONFIGS, make_batch  # noqa: E402

workload = sys.argv[1] if len(sys.argv) > 1 else "target_veh3dof_fhadp_b4096_h30"
cfg = CONFIGS[workload]
os.environ["GOPS_HIP_GRAPH"] = "0"


def gradients(flags):
    hb.DEFAULT_VARIANT_FLAGS = flags
    torch.manual_seed(0)
    with contextlib.redirect_stdout(sys.stderr):
        alg = create_alg(**alg_kwargs(cfg, 0))
    alg.networks.to("cuda")
    data = {k: v.cuda() for k, v in make_batch(cfg, 1000).items()}
    _, info = alg.get_remote_update_info(data, 0)
    torch.cuda.synchronize()
    return [g.detach().cpu().clone() for g in info["grad"]]


a, b = gradients(0), gradients(hb.VF_DW_EXACT)
for i, (x, y) in enumerate(zip(a, b)):
    print(f"tensor {i} {tuple(x.shape)}: rel-L2 {((x - y).double().norm() / y.double().norm()).item():.3e}  max|diff|/max|ref| {((x - y).abs().max() / y.abs().max()).item():.3e}")
