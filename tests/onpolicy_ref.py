"""Host oracle of the sampled actor-critic and of GAE (csrc/nascar_actor.h: MLP_OUT_SAMPLE, gae_kernel) -- TEST
INFRASTRUCTURE ONLY.  NumPy on np.float32 arrays and Python floats, so NumPy 2 promotion decides every rounding, as in
SB3's RolloutBuffer; importable without a GPU.

  uniforms / eps      the Box-Muller pair of a car at (seed, step) from two mix32 draws on policy_car's key
  sample              a = mu + std * eps, clip(a, -1, 1) and DiagGaussianDistribution.log_prob, in `dtype` arithmetic
  gae                 RolloutBuffer.compute_returns_and_advantage with the time-limit bootstrap added to the rewards
  gae_scalar          the same as a plain double loop over cars and steps in Python floats (float64)
"""
import math

import numpy as np

from drivers import hash_keys, mix32

SALT0 = 0x5A4D504C45            # include/nascar.h: the salts of the sampled actor's two draws
SALT1 = 0x3C6EF372FE94F82B
TEST_SEED = 20                  # the seed of the value tests (its clip share: tests/test_onpolicy_cpu.py)


def uniforms(N, seed, step, ids=None, salt0=SALT0, salt1=SALT1):
    """(k0, k1): the 24-bit integers behind u0 = (k0 + 1) / 2^24 in (0, 1] and u1 = k1 / 2^24 in [0, 1)"""
    key = hash_keys(N, seed, step, ids)
    return ((mix32(key ^ np.uint64(salt0)) >> np.uint32(8)).astype(np.int64),
            (mix32(key ^ np.uint64(salt1)) >> np.uint32(8)).astype(np.int64))


def eps(N, seed, step, ids=None, dtype=np.float32, **salts):
    """[N, 2] standard normal pairs: r = sqrt(-2 log u0), (r cos(2 pi u1), r sin(2 pi u1)), every operation in `dtype`"""
    dt = np.dtype(dtype).type
    k0, k1 = uniforms(N, seed, step, ids, **salts)
    u0 = (k0 + 1).astype(dt) * dt(1.0 / 16777216.0)       # exact in float32: 24-bit integers times 2^-24
    u1 = k1.astype(dt) * dt(1.0 / 16777216.0)
    r = np.sqrt(dt(-2.0) * np.log(u0))
    th = dt(2.0 * math.pi) * u1
    return np.stack([r * np.cos(th), r * np.sin(th)], axis=1)


def sample(mu, log_std, e, dtype=np.float32):
    """(a, clip(a), logp) from the means [N, 2], log_std [2] and the normal pairs e [N, 2], in `dtype` arithmetic:
    DiagGaussianDistribution.sample / log_prob (torch's Normal: -(a - mu)^2 / (2 var) - log_std - log(sqrt(2 pi)), summed
    over the two components) and OnPolicyAlgorithm.collect_rollouts' np.clip before env.step."""
    dt = np.dtype(dtype).type
    mu, e = np.asarray(mu, dt), np.asarray(e, dt)
    ls = np.asarray(log_std, np.float32).astype(dt)
    std = np.exp(ls)
    a = mu + std * e
    d = a - mu
    lp = (-(d * d) / (dt(2.0) * (std * std)) - ls) - dt(0.5 * math.log(2.0 * math.pi))
    return a, np.clip(a, dt(-1), dt(1)), lp[:, 0] + lp[:, 1]


def gae(rewards, values, timeout_values, done, gamma, gae_lambda, dtype=np.float32):
    """RolloutBuffer.compute_returns_and_advantage on [K, N] records, values [K + 1, N] (record K the bootstrap value),
    done [K, N] (terminated | truncated of the car's env at step k: SB3's episode_starts[k + 1]); gamma / gae_lambda are
    Python floats.  With float32 arrays NumPy 2 keeps every operation in float32 and rounds the Python-float products
    gamma and gamma * gae_lambda (formed in float64) to float32 where they meet an array.  Returns (advantages, returns)."""
    dt = np.dtype(dtype).type
    rewards, values, tv = np.asarray(rewards, dt), np.asarray(values, dt), np.asarray(timeout_values, dt)
    K = rewards.shape[0]
    rewards = rewards + gamma * tv                        # collect_rollouts: rewards[idx] += self.gamma * terminal_value
    adv = np.zeros_like(rewards)
    last = np.zeros(rewards.shape[1:], dt)
    for k in reversed(range(K)):
        nnt = dt(1.0) - np.asarray(done[k], dt)
        delta = rewards[k] + gamma * values[k + 1] * nnt - values[k]
        last = delta + gamma * gae_lambda * nnt * last
        adv[k] = last
    return adv, adv + values[:K]


def gae_scalar(rewards, values, timeout_values, done, gamma, gae_lambda):
    """the same recursion written out per car in Python floats"""
    K, N = np.shape(rewards)
    adv = [[0.0] * N for _ in range(K)]
    ret = [[0.0] * N for _ in range(K)]
    for n in range(N):
        last = 0.0
        for k in range(K - 1, -1, -1):
            nnt = 1.0 - float(done[k][n])
            r = float(rewards[k][n]) + gamma * float(timeout_values[k][n])
            delta = r + gamma * float(values[k + 1][n]) * nnt - float(values[k][n])
            last = delta + gamma * gae_lambda * nnt * last
            adv[k][n] = last
            ret[k][n] = last + float(values[k][n])
    return np.array(adv), np.array(ret)
