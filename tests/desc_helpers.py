"""Descriptions for the refusal tests, which need no device: every call they go into is refused by an argument check before the
library makes any HIP call, so a pointer is only ever compared with null (or tested for alignment) and never followed."""
from gops_amd import hip_backend as hb

BAD, UNS, WS = -1, -2, -3   # GOPS_ERR_BAD_ARG, GOPS_ERR_UNSUPPORTED, GOPS_ERR_WORKSPACE
P, ODD = 0x1000, 0x1004     # a pointer that is never followed (16-byte aligned) / one that is not 8-byte aligned
ELU = hb.ACT_IDS["elu"]


def struct(cls, **fields):
    s = cls()
    for k, v in fields.items():
        setattr(s, k, v)
    return s


def ptr_struct(cls, **null):
    """A struct of pointers, every one of them `P` but those named in `null` (field=value)."""
    return struct(cls, **{k: null.get(k, P) for k, _ in cls._fields_})


def mlp_desc(sizes, act=ELU, ptr=P, **fields):
    """A GopsMlp of these layer sizes with `ptr` for every weight and bias; `fields` are set last (n_layers, dtype, ...)."""
    m = hb.GopsMlp()
    m.n_layers = len(sizes) - 1
    for i, s in enumerate(sizes):
        m.sizes[i] = s
    for j in range(m.n_layers):
        m.weight[j] = m.bias[j] = ptr
    m.hidden_act = act
    for k, v in fields.items():
        setattr(m, k, v)
    return m


def env_desc(kind, obs_dim, act_dim, **fields):
    return struct(hb.GopsEnv, kind=kind, obs_dim=obs_dim, act_dim=act_dim, **fields)
