"""Host oracle of the categorical actor (csrc/nascar_actor.h: mlp_categorical, MLP_OUT_CATEGORICAL / MLP_OUT_MODE) -- TEST
INFRASTRUCTURE ONLY.  NumPy, importable without a GPU.

  uniform             the car's u in [0, 1) at (seed, step): one mix32 draw on policy_car's key with the salt CAT_SALT
  sample              the inverse-CDF draw on u, in `dtype` arithmetic: (index, logp, normalised prefix sums)
  mode                the first maximum of the logits
  PAIRS               action index -> the (throttle / brake, steering) pair that steps the env
"""
import numpy as np

import onpolicy_ref as R

CAT_SALT = 0x4341545F44524157       # include/nascar.h: the salt of the categorical actor's draw ("CAT_DRAW")
PAIRS = np.array([[0, 0], [1, 0], [-1, 0], [0, -1], [0, 1]], np.float32)    # nascar_step(discrete=1): model_block


def uniform(N, seed, step, ids=None, dtype=np.float64):
    """u = k * 2^-24 with k the 24-bit integer of onpolicy_ref.uniforms' second draw under CAT_SALT (exact in float32)"""
    dt = np.dtype(dtype).type
    _, k = R.uniforms(N, seed, step, ids, salt0=CAT_SALT, salt1=CAT_SALT)
    return k.astype(dt) * dt(1.0 / 16777216.0)


def sample(logits, u, dtype=np.float64):
    """(a [n] int64, logp [n], Pn [n, 4]) of logits [n, 5] and u [n]: m = max l, e = exp(l - m), P = cumsum(e) in index
    order, S = P[4], t = u * S, a = #{j < 4: t >= P_j}, logp = (l_a - m) - log(S); Pn = P[:4] / S are the boundaries of u."""
    dt = np.dtype(dtype).type
    l = np.asarray(logits, dt)
    m = l.max(axis=1)
    d = l - m[:, None]
    e = np.exp(d)
    P = np.empty_like(e)
    P[:, 0] = e[:, 0]
    for j in range(1, 5):
        P[:, j] = P[:, j - 1] + e[:, j]
    S = P[:, 4]
    t = np.asarray(u, dt) * S
    a = (t[:, None] >= P[:, :4]).sum(axis=1)
    logp = d[np.arange(len(a)), a] - np.log(S)
    return a.astype(np.int64), logp, P[:, :4] / S[:, None]


def logp_of(logits, a, dtype=np.float64):
    """Categorical(logits).log_prob(a) in `dtype` arithmetic, as sample writes it"""
    dt = np.dtype(dtype).type
    l = np.asarray(logits, dt)
    m = l.max(axis=1)
    d = l - m[:, None]
    e = np.exp(d)
    S = e[:, 0]
    for j in range(1, 5):
        S = S + e[:, j]
    return d[np.arange(len(a)), np.asarray(a, np.int64)] - np.log(S)


def mode(logits):
    """the first maximum (np.argmax returns the first occurrence)"""
    return np.argmax(np.asarray(logits), axis=1).astype(np.int64)


def band(logits32, logits64, u):
    """(margin, in_band [n]): margin = max(8 x max |float32 - float64| of the normalised prefix sums, 1e-6); a car is in the
    band when its u lies within the margin of any of its four float64 boundaries"""
    u = np.asarray(u, np.float64)
    _, _, p32 = sample(logits32, u, np.float32)
    _, _, p64 = sample(logits64, u, np.float64)
    margin = max(8 * float(np.abs(p32.astype(np.float64) - p64).max()), 1e-6)
    return margin, (np.abs(u[:, None] - p64) <= margin).any(axis=1)
