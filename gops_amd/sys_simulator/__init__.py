"""Closed-loop simulation tools: the host-side optimal controller and its batched, device-resident counterpart."""
from gops_amd.sys_simulator.batch_opt_controller import BatchOptController
from gops_amd.sys_simulator.opt_controller import OptController

__all__ = ["BatchOptController", "OptController"]
