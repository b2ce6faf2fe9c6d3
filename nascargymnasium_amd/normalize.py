"""The running statistics of `BatchedCarEnv.set_normalize` as a host record.

Stable-Baselines3's VecNormalize (which the reference wraps its A2C training envs in, learn/a2c.py:94-100) keeps a
RunningMeanStd over the 38 observation columns, one over the discounted returns, and the returns themselves.  The engine
keeps them on the device (csrc/nascar_norm.h); `NormStats` is what `norm_stats()` reads back and `load_norm_stats()` /
`set_normalize(stats=...)` upload: plain float64 NumPy arrays, saved as `.npz`.  A user who has opened an SB3
`vecnormalize.pkl` themselves brings its numbers in through the constructor -- nothing here unpickles anything:

    NormStats(vn.obs_rms.mean, vn.obs_rms.var, vn.obs_rms.count, vn.ret_rms.mean, vn.ret_rms.var, vn.ret_rms.count)
"""
import numpy as np

OBS_DIM = 38
RECORD = 2 * OBS_DIM + 4    # the device record: obs_mean [38], obs_var [38], obs_count, ret_mean, ret_var, ret_count


class NormStats:
    """obs_mean, obs_var [38]; obs_count, ret_mean, ret_var, ret_count scalars; returns [N] or None (None: the engine's
    returns are left as they are by load_norm_stats) -- all float64.  Raises ValueError on a wrong shape, a non-finite
    entry, a negative variance or a non-positive count."""
    FIELDS = ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count", "returns")

    def __init__(self, obs_mean, obs_var, obs_count, ret_mean, ret_var, ret_count, returns=None):
        self.obs_mean = np.array(obs_mean, dtype=np.float64)
        self.obs_var = np.array(obs_var, dtype=np.float64)
        self.obs_count, self.ret_mean = float(obs_count), float(ret_mean)
        self.ret_var, self.ret_count = float(ret_var), float(ret_count)
        self.returns = None if returns is None else np.array(returns, dtype=np.float64).reshape(-1)
        self.validate()

    @classmethod
    def fresh(cls, num_rows=None):
        """RunningMeanStd(epsilon=1e-4) as constructed: mean 0, var 1, count 1e-4 (and zero returns for num_rows rows)"""
        return cls(np.zeros(OBS_DIM), np.ones(OBS_DIM), 1e-4, 0.0, 1.0, 1e-4,
                   None if num_rows is None else np.zeros(int(num_rows)))

    def validate(self):
        for name in ("obs_mean", "obs_var"):
            a = getattr(self, name)
            if a.shape != (OBS_DIM,):
                raise ValueError(f"NormStats.{name}: shape {a.shape}, expected ({OBS_DIM},)")
        for name in self.FIELDS:
            a = getattr(self, name)
            if a is not None and not np.all(np.isfinite(a)):
                raise ValueError(f"NormStats.{name} is not finite")
        if np.any(self.obs_var < 0) or self.ret_var < 0:
            raise ValueError("NormStats: a variance is negative")
        if not (self.obs_count > 0 and self.ret_count > 0):
            raise ValueError("NormStats: a count is not positive")

    def record(self) -> np.ndarray:
        """the device record [80] float64"""
        return np.concatenate([self.obs_mean, self.obs_var,
                               [self.obs_count, self.ret_mean, self.ret_var, self.ret_count]]).astype(np.float64)

    @classmethod
    def from_record(cls, rec, returns=None):
        rec = np.asarray(rec, np.float64).reshape(-1)
        if rec.size != RECORD:
            raise ValueError(f"NormStats record: {rec.size} entries, expected {RECORD}")
        return cls(rec[:OBS_DIM], rec[OBS_DIM:2 * OBS_DIM], *rec[2 * OBS_DIM:], returns=returns)

    def save(self, path):
        arrays = {k: np.asarray(getattr(self, k), np.float64) for k in self.FIELDS if getattr(self, k) is not None}
        with open(path, "wb") as f:      # (np.savez would append .npz to a bare name)
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in cls.FIELDS[:-1] if k not in z.files]
            if missing:
                raise ValueError(f"{path}: no {missing} in the file")
            return cls(*[z[k] for k in cls.FIELDS[:-1]], returns=z["returns"] if "returns" in z.files else None)

    def __eq__(self, other):
        if not isinstance(other, NormStats):
            return NotImplemented
        return (np.array_equal(self.record(), other.record()) and
                (self.returns is None) == (other.returns is None) and
                (self.returns is None or np.array_equal(self.returns, other.returns)))

    def __repr__(self):
        return (f"NormStats(obs_count={self.obs_count!r}, ret_mean={self.ret_mean!r}, ret_var={self.ret_var!r}, "
                f"ret_count={self.ret_count!r}, returns={'None' if self.returns is None else self.returns.shape})")
