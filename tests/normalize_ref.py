"""Host oracle of the running normalisation (csrc/nascar_norm.h, BatchedCarEnv.set_normalize): Stable-Baselines3 2.7.0's
RunningMeanStd and VecNormalize restated in NumPy, expression by expression, with ONE deliberate deviation -- the batch
moments are taken in float64 over the float32 rows (`arr.astype(np.float64)` first; SB3 lets NumPy accumulate them in the
array's float32), which is what the device does.  Every car slot is one of SB3's envs; `dones` is per row."""
import numpy as np

OBS_DIM = 38
U = 2.0 ** -53      # float64 unit roundoff


class RunningMeanStd:
    def __init__(self, epsilon=1e-4, shape=()):
        self.mean = np.zeros(shape, np.float64)
        self.var = np.ones(shape, np.float64)
        self.count = epsilon

    def update(self, arr):
        arr = np.asarray(arr).astype(np.float64)
        self.update_from_moments(np.mean(arr, axis=0), np.var(arr, axis=0), arr.shape[0])

    def update_from_moments(self, batch_mean, batch_var, batch_count):
        delta = batch_mean - self.mean
        tot_count = self.count + batch_count
        new_mean = self.mean + delta * batch_count / tot_count
        m_a = self.var * self.count
        m_b = batch_var * batch_count
        m_2 = m_a + m_b + np.square(delta) * self.count * batch_count / (self.count + batch_count)
        new_var = m_2 / (self.count + batch_count)
        new_count = batch_count + self.count
        self.mean, self.var, self.count = new_mean, new_var, new_count


def normalize_obs(x, mean, var, clip_obs, epsilon=1e-8):
    """float32(clip((x - mean) / sqrt(var + epsilon), -clip_obs, clip_obs)), in float64 on float32 rows"""
    return np.clip((np.asarray(x).astype(np.float64) - mean) / np.sqrt(var + epsilon), -clip_obs, clip_obs).astype(np.float32)


def normalize_reward(r, ret_var, clip_reward, epsilon=1e-8):
    return np.clip(np.asarray(r).astype(np.float64) / np.sqrt(ret_var + epsilon), -clip_reward, clip_reward).astype(np.float32)


class VecNormalize:
    """the wrapper's arithmetic alone: reset(obs) and step_wait(obs, reward, dones, terminal_obs) on arrays [N, 38] / [N]"""

    def __init__(self, num_rows, norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0, gamma=0.99,
                 epsilon=1e-8, training=True):
        self.norm_obs, self.norm_reward, self.training = norm_obs, norm_reward, training
        self.clip_obs, self.clip_reward, self.gamma, self.epsilon = clip_obs, clip_reward, gamma, epsilon
        self.obs_rms = RunningMeanStd(shape=(OBS_DIM,))
        self.ret_rms = RunningMeanStd(shape=())
        self.returns = np.zeros(num_rows, np.float64)

    def _obs(self, x):
        x = np.asarray(x, np.float32)
        return normalize_obs(x, self.obs_rms.mean, self.obs_rms.var, self.clip_obs, self.epsilon) if self.norm_obs else x.copy()

    def _reward(self, r):
        r = np.asarray(r, np.float32)
        return normalize_reward(r, self.ret_rms.var, self.clip_reward, self.epsilon) if self.norm_reward else r.copy()

    def reset(self, obs):
        self.returns = np.zeros_like(self.returns)
        if self.training and self.norm_obs:
            self.obs_rms.update(obs)
        return self._obs(obs)

    def step_wait(self, obs, reward, dones, terminal_obs=None):
        """(normalised obs, normalised reward, normalised terminal rows of the done rows or None)"""
        if self.training and self.norm_obs:
            self.obs_rms.update(obs)
        nobs = self._obs(obs)
        if self.training and self.norm_reward:
            self.returns = self.returns * self.gamma + np.asarray(reward, np.float32)
            self.ret_rms.update(self.returns)
        nrew = self._reward(reward)
        dones = np.asarray(dones, bool)
        nterm = None if terminal_obs is None else self._obs(np.asarray(terminal_obs)[dones])
        self.returns[dones] = 0
        return nobs, nrew, nterm


def moment_bounds(rows, updates=1, n=None):
    """(mean bound, variance bound) per column of `rows` [., 38] for `updates` updates of n rows each (default: one batch,
    all the rows): 4 N u max|x| and 8 N u max|x|^2, the forward error of two differently ordered float64 sums of N terms"""
    rows = np.asarray(rows, np.float64)
    n = rows.shape[0] if n is None else n
    mx = np.abs(rows).max(axis=0)
    return updates * 4 * n * U * mx, updates * 8 * n * U * mx * mx


# ------------------------------------------------------------------ the inputs of tests/test_gpu_normalize.py
# Rows of the golden observations (test_onpolicy_cpu.golden_obs), batch i of n rows starting at START + i * n (wrapping):
# tests/test_normalize_cpu.py checks that they exercise what the GPU tests are about.
START = 189
CONDITION_SIZES = (31, 33, 96, 129, 185)            # the sizes the conditions are checked at (1 row has no variance)
RETURN_FIXTURE, RETURN_WARM, RETURN_K = "daytona_low_reward", 830, 16   # the returns test's window: steps [830, 846)


def batch_rows(obs, n, i=0):
    obs = np.asarray(obs)
    return np.ascontiguousarray(obs[(START + i * n + np.arange(n)) % len(obs)])
