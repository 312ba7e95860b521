"""Shared by test_rnn_cpu.py and test_rnn_gpu.py: the arguments of a recurrent approximator and of PPO on the recurrent pair."""
import numpy as np

from gops_amd.utils.act_distribution import DiracDistribution, GaussDistribution

LIM = dict(act_low_lim=np.array([-1.0, -0.5], np.float32), act_high_lim=np.array([2.0, 0.5], np.float32))


def apprfunc_kwargs(name, hidden, activation="tanh", O=4, out=2):
    """create_apprfunc's arguments for the RNN class `name`: hidden[0] is the recurrence's width, hidden[1:] the heads' hidden layers;
    `out`: act_dim / act_num (StateValue has one output whatever it is)."""
    dist = GaussDistribution if name == "StochaPolicy" else DiracDistribution
    return dict(apprfunc="RNN", name=name, obs_dim=(5, O), act_dim=out, act_num=out, hidden_sizes=list(hidden), hidden_activation=activation,
                output_activation="linear", min_log_std=-20.0, max_log_std=2.0, action_distribution_cls=dist,
                act_low_lim=LIM["act_low_lim"][:out], act_high_lim=LIM["act_high_lim"][:out])


def ppo_kwargs(**over):
    """create_alg's arguments for PPO on the recurrent pair: stacks of L = 5 observations of 4, H = 16, head hidden (16,), A = 1; three
    repeats of two minibatches of 17 rows."""
    kw = dict(algorithm="PPO", trainer="on_serial_trainer", seed=0, cnn_shared=False, env_id="gym_cartpolecontiwithstack", obsv_dim=(5, 4),
              action_dim=1, action_type="continu", action_low_limit=np.array([-1.0], np.float32), action_high_limit=np.array([1.0], np.float32),
              policy_func_type="RNN", policy_func_name="StochaPolicy", policy_act_distribution="default", policy_hidden_sizes=[16, 16],
              policy_hidden_activation="tanh", value_func_type="RNN", value_func_name="StateValue", value_hidden_sizes=[16, 16],
              value_hidden_activation="tanh", learning_rate=1e-3, max_iteration=8, num_repeat=3, num_mini_batch=2, mini_batch_size=17,
              sample_batch_size=34, use_gpu=False)
    kw.update(over)
    return kw
