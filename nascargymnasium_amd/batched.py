"""BatchedCarEnv: E independent reference CarEnvs x C cars stepped by one fused
HIP kernel per step (libnascar.so), state resident in HBM.

All buffers are torch tensors on the HIP device; ``step`` launches on torch's
current stream and returns device tensors (no host sync).  This is the engine
under both the Gymnasium ``CarEnv`` (E=1, nascargymnasium_amd/car_env.py) and
the SB3-style ``VecCarEnv`` (nascargymnasium_amd/vec_env.py).
"""
import collections
import ctypes
from typing import Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from .track import build_walls, load_track, track_path


RaceLedger = collections.namedtuple("RaceLedger", ["ledger", "fastest_car", "ended"])   # BatchedCarEnv.race
RaceRank = collections.namedtuple("RaceRank", ["order", "position", "points"])           # BatchedCarEnv.race_rank


def _ptr(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class BatchedCarEnv:
    """E envs x C cars of the reference CarEnv on one GPU.

    track_file: one track (name or path) for all envs, or a sequence of E tracks
    (per-env track index; envs are grouped per track into workgroups).
    envs_per_block / beam_cell: scheduling and memory choices with identical results (set_envs_per_block;
    nascar_set_beam_cell: the distance sensors' beam-list cell size in m, default 1).
    """

    def __init__(self, num_envs: int, num_cars: int = 1, track_file: Union[str, Sequence[str]] = "daytona",
                 reset_on_lap: bool = False, device: Union[str, int, torch.device] = "cuda",
                 start_position=None, start_angle: float = 0.0, perf_history: bool = False,
                 envs_per_block: Optional[int] = None, beam_cell: Optional[float] = None):
        if not torch.cuda.is_available():
            raise RuntimeError("BatchedCarEnv needs a HIP device (torch.cuda.is_available() is False); "
                               "the product path has no CPU fallback")
        if num_cars < 1 or num_cars > 64:
            raise ValueError("num_cars must be in [1, 64]")
        self.E, self.C, self.N = int(num_envs), int(num_cars), int(num_envs) * int(num_cars)
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.L = _lib.lib()
        files = [track_file] * self.E if isinstance(track_file, str) else list(track_file)
        if len(files) != self.E:
            raise ValueError("need one track per env")
        uniq = sorted(set(track_path(f) for f in files))
        first = load_track(track_path(files[0]))
        sx, sy = start_position if start_position is not None else first.start_position
        cfg = _lib.NascarConfig(self.E, self.C, int(reset_on_lap), self.device.index, float(sx), float(sy),
                                float(start_angle))
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.L.nascar_create(ctypes.byref(cfg), ctypes.byref(h)))
        self.h = h
        if envs_per_block is not None:
            self.set_envs_per_block(envs_per_block)
        if beam_cell is not None:     # before the tracks are added: their beam lists are built at this cell size
            _lib.check(self.L.nascar_set_beam_cell(self.h, float(beam_cell)))
        self.tracks, self._track_id, self._track_files_by_id = [], {}, {}
        self.random_track_ids = None
        for p in uniq:
            self._add_track(p)
        self.set_env_tracks(files)
        dev = self.device
        self.obs = torch.zeros(self.E, self.C, _lib.OBS_DIM, dtype=torch.float32, device=dev)
        self.reward = torch.zeros(self.E, self.C, dtype=torch.float32, device=dev)
        self.car_flags = torch.zeros(self.E, self.C, dtype=torch.uint8, device=dev)
        self.env_flags = torch.zeros(self.E, dtype=torch.uint8, device=dev)
        self.terminal_obs = torch.zeros_like(self.obs)
        self._info = torch.zeros(self.E, self.C, _lib.N_INFO, dtype=torch.float64, device=dev)
        self._actions = torch.zeros(self.E, self.C, 2, dtype=torch.float32, device=dev)
        self.normalize = None       # set_normalize: the settings while normalisation is on
        self._norm_obs = self._norm_reward = self._norm_terminal_obs = None
        if perf_history:
            self.set_perf_history(True)

    def set_car_contact(self, enable: bool = True):
        """BUILD-ONLY EXTENSION (no reference counterpart): cars of an env collide with each other (staggered start
        grid; after each Box2D step the env's touching car pairs are solved with b2CollidePolygons manifolds and
        b2ContactSolver's sequential friction and normal impulses, see include/nascar.h).  Off by default; parity holds
        only when off."""
        _lib.check(self.L.nascar_set_car_contact(self.h, int(bool(enable))))

    def set_car_visibility(self, enable: bool = True):
        """BUILD-ONLY EXTENSION (no reference counterpart): the 16 distance sensors of a car also see the other cars
        of its env -- each ray's hit fraction is the minimum of the wall hit and b2PolygonShape::RayCast against the
        other cars' boxes at the poses the same observation is taken from (include/nascar.h).  Independent of
        set_car_contact; off by default, and off is bit-identical to the reference.  Not supported with random-track
        mode or the fused single-launch rollout (`set_rollout_streams(0)`): those calls raise."""
        _lib.check(self.L.nascar_set_car_visibility(self.h, int(bool(enable))))

    @property
    def car_visibility(self) -> bool:
        return bool(self.L.nascar_get_car_visibility(self.h))

    def set_rollout_streams(self, streams: int = 4):
        """How `rollout` schedules its steps (identical results either way): streams >= 1 splits the envs into that
        many shards, each stepped on its own stream (shard 0 on the current one), so one shard's slow cars (Box2D
        TOI chains) overlap the other shards' work (default 4, or GPU_MAX_HW_QUEUES if fewer); 0 runs all steps in
        one fused launch."""
        _lib.check(self.L.nascar_set_rollout_streams(self.h, int(streams)))

    @property
    def rollout_streams(self) -> int:
        return int(self.L.nascar_get_rollout_streams(self.h))

    def set_rollout_pipe(self, sensor_workgroups: int = 0):
        """Pipelined `rollout` (identical results): each workgroup of envs goes on to its next step as soon as its own
        sensors are done, with the sensors in a second persistent kernel of `sensor_workgroups` workgroups fed from a
        device queue, so a slow car delays only its own envs (not the batch's step).  0 turns it off.  Used by
        `rollout` for policies 0 / 1 / 3 (not 2 or 4) without random tracks, car contact or obs trajectories (else the setting of
        set_rollout_streams applies)."""
        _lib.check(self.L.nascar_set_rollout_pipe(self.h, int(sensor_workgroups)))
        self.rollout_pipe = int(sensor_workgroups)

    def rollout_pipe_status(self) -> int:
        """Waits for the current stream and reports whether a pipelined rollout since the last call gave up on a
        clock-bounded wait (1; its results are not valid) or not (0)."""
        import torch
        r = int(self.L.nascar_rollout_pipe_status(self.h, ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        if r < 0:
            _lib.check(r)
        return r

    def set_envs_per_block(self, epb: int = 0):
        """Workgroup layout of the one-lane-per-car step kernels: `epb` whole envs per 128-lane workgroup, in
        [1, 128 // C]; 0 restores the automatic choice.  Results do not depend on it (tests pin every layout the
        bench runs against the oracle); it changes only which cars share a wave."""
        _lib.check(self.L.nascar_set_envs_per_block(self.h, int(epb)))

    @property
    def envs_per_block(self) -> int:
        return int(self.L.nascar_get_envs_per_block(self.h))

    def set_fused_logic(self, enable: bool = True):
        """One launch per step for the vehicle model + Box2D step and the env logic (each workgroup runs its envs'
        logic once its own cars' physics is done; the default) or two (False); identical results."""
        _lib.check(self.L.nascar_set_fused_logic(self.h, int(bool(enable))))

    @property
    def fused_logic(self) -> bool:
        return bool(self.L.nascar_get_fused_logic(self.h))

    def set_sensor_lanes(self, lanes: int = 0):
        """Lanes per car of the distance-sensor kernel: 4 or 16 (one ray per lane), 0 automatic (16).  Identical
        results; a scheduling choice."""
        _lib.check(self.L.nascar_set_sensor_lanes(self.h, int(lanes)))

    def set_sensor_block(self, threads: int = 0):
        """threads per workgroup of the 16-lane sensor kernel: 64 / 128 (walls read from global memory) or 256 / 512 /
        1024 (walls staged in LDS per workgroup); 0: automatic (128); identical results"""
        _lib.check(self.L.nascar_set_sensor_block(self.h, int(threads)))

    def set_perf_history(self, enable: bool = True):
        """Keep Car.velocity_history on the device so the info's `performance` dict is Car.validate_performance
        (src/car.py:1060-1098); a 640-sample float32 ring per car, one 4-byte store per car-step.  Enabled before the
        first reset (as CarEnv does) it covers every episode; enabled mid-episode, an env's window holds steps taken
        before the enable, so its info reports perf_count -1 ("history not kept") until its next reset or until
        600 steps have been recorded since the enable."""
        with torch.cuda.device(self.device):
            _lib.check(self.L.nascar_set_perf_history(self.h, int(bool(enable)), _stream()))

    def _add_track(self, path: str) -> int:
        """Load a .track file into the handle (TrackLoader + _create_track_walls tables); returns its id."""
        path = track_path(path)
        if path in self._track_id:
            return self._track_id[path]
        t = load_track(path)
        seg = np.ascontiguousarray(t.segment_table())
        walls = np.ascontiguousarray(build_walls(t)[:, :4])
        dp = ctypes.POINTER(ctypes.c_double)
        with torch.cuda.device(self.device):   # (the library also brackets its device work with the handle's device)
            tid = _lib.check(self.L.nascar_add_track(self.h, seg.ctypes.data_as(dp), seg.shape[0], float(t.total_length),
                                                     walls.ctypes.data_as(dp), walls.shape[0]))
        self.tracks.append(t)
        self._track_id[path] = tid
        self._track_files_by_id[tid] = path
        return tid

    def set_env_tracks(self, files: Sequence[str]):
        """Per-env track (name or path), applied by the next reset of each env (fresh worlds on the new track, as
        CarEnv.reset rebuilds CarPhysics, src/car_env.py:375-394); until then an env steps on its old track.  New
        tracks are loaded on demand.  The start pose is the handle's (every bundled track starts its GRID at (0, 0),
        heading 0)."""
        if isinstance(files, str):
            files = [files] * self.E
        if len(files) != self.E:
            raise ValueError("need one track per env")
        env_track = np.array([self._add_track(f) for f in files], np.int32)
        _lib.check(self.L.nascar_set_env_tracks(self.h, env_track.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        self.env_track = env_track
        self.track_files = [track_path(f) for f in files]

    # ------------------------------------------------------------------ random-track mode (src/car_env.py:243-303)
    def set_random_tracks(self, files: Sequence[str], seeds, draws=None):
        """Random-track mode on the device (CarEnv(track_file=None), src/car_env.py:243-303, 331-398; learn/ppo.py:65-78
        trains every env this way): every reset of an env -- `reset(mask)` or the auto-reset inside a step -- first draws
        its next track from `files` (any but its current one, CarEnv._select_random_track) and a changed track gets fresh
        worlds; the block map is rebuilt on the device, so a step makes no host round trip.  Draw k of env e is
        `_lib.track_draw(seeds[e], k, current, ids)`; `draws` (default 0) are the per-env draw counters to continue from.
        Files not loaded yet are loaded here.  While the mode is on, `set_env_tracks` raises; `clear_random_tracks` ends
        it (the envs keep their current tracks)."""
        ids = np.array([self._add_track(f) for f in files], np.int32)
        seeds = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).ravel())
        if seeds.size != self.E:
            raise ValueError(f"need one seed per env ({self.E}), got {seeds.size}")
        dr = None
        if draws is not None:
            dr = np.ascontiguousarray(np.broadcast_to(np.asarray(draws, np.int32), (self.E,)))
        i32p, u64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64)
        with torch.cuda.device(self.device):
            _lib.check(self.L.nascar_set_random_tracks(self.h, ids.ctypes.data_as(i32p), int(ids.size),
                                                       seeds.ctypes.data_as(u64p),
                                                       dr.ctypes.data_as(i32p) if dr is not None else None, _stream()))
        self.random_track_ids = ids
        self.random_track_files = [track_path(f) for f in files]

    def clear_random_tracks(self):
        """End random-track mode: the envs keep the tracks they are on, managed by `set_env_tracks` again."""
        with torch.cuda.device(self.device):
            _lib.check(self.L.nascar_set_random_tracks(self.h, None, 0, None, None, _stream()))
        self.random_track_ids = None
        ids, _ = self.env_track_ids()
        self.env_track = ids
        self.track_files = [self._track_files_by_id[i] for i in ids]

    def env_track_ids(self):
        """(track id per env, draws taken per env) as numpy int32 arrays -- the device's in random-track mode (one host
        synchronisation), else the host's assignment and zeros."""
        t = torch.empty(2, self.E, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.L.nascar_get_env_tracks(self.h, _ptr(t[0]), _ptr(t[1]), _stream()))
        a = t.cpu().numpy()
        return a[0].copy(), a[1].copy()

    def env_track_files(self):
        """the .track path each env is on now"""
        ids, _ = self.env_track_ids()
        return [self._track_files_by_id[i] for i in ids]

    def block_map(self):
        """(blk_track [nb], blk_env [nb, envs_per_block]) numpy int32: the workgroup layout of the next launch (test hook,
        nascar_debug_block_map; one host synchronisation)"""
        cap = self.E + 128
        bt = torch.empty(cap, dtype=torch.int32, device=self.device)
        be = torch.empty(cap * max(1, self.envs_per_block), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            nb = _lib.check(self.L.nascar_debug_block_map(self.h, _ptr(bt), _ptr(be), cap, _stream()))
        epb = self.envs_per_block
        return bt[:nb].cpu().numpy(), be[:nb * epb].cpu().numpy().reshape(nb, epb)

    @staticmethod
    def debug_car_contact(bodies: torch.Tensor, num_cars: int):
        """nascar_debug_car_contact (test hook, no engine state): the car-car contact solver on bodies [E * num_cars, 7]
        float32 on the device (x y qs qc vx vy w).  Returns (out [E, num_cars, 4] float32: vx vy w and the car's largest
        normal impulse, env_out [E, 2] int32: pairs solved, pairs dropped at the cap) as device tensors."""
        b = bodies.to(torch.float32).contiguous().reshape(-1, 7)
        C = int(num_cars)
        if C < 1 or b.shape[0] % C:
            raise ValueError(f"{b.shape[0]} bodies are no whole envs of {C} cars")
        E = b.shape[0] // C
        out = torch.zeros(E, C, 4, dtype=torch.float32, device=b.device)
        env_out = torch.zeros(E, 2, dtype=torch.int32, device=b.device)
        with torch.cuda.device(b.device):
            _lib.check(_lib.lib().nascar_debug_car_contact(_ptr(b), E, C, _ptr(out), _ptr(env_out), _stream()))
        return out, env_out

    # ------------------------------------------------------------------ core API
    def reset(self, env_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """CarEnv.reset for all envs (or those with env_mask[e] != 0, uint8[E] on device).  Under set_normalize a full
        reset also performs VecNormalize.reset and returns the normalised observation (`norm_obs`); a masked reset does
        not (SB3's in-step resets are ordinary steps)."""
        with torch.cuda.device(self.device):
            m = None if env_mask is None else env_mask.to(self.device, torch.uint8).contiguous()
            _lib.check(self.L.nascar_reset(self.h, _ptr(m), _ptr(self.obs), _stream()))
            if m is None and self.normalize is not None:
                _lib.check(self.L.nascar_normalize_reset(self.h, _ptr(self.obs), _ptr(self._norm_buffers()[0]), _stream()))
                return self._norm_obs
        return self.obs

    def step(self, actions: torch.Tensor, auto_reset: bool = False, terminal_obs: bool = False):
        """CarEnv.step for all envs.  actions: float32 [E, C, 2] (continuous) or int32 [E, C] (discrete)."""
        self.launch_step(actions, auto_reset, terminal_obs)
        terminated = (self.env_flags & _lib.EF_TERMINATED) != 0
        truncated = (self.env_flags & _lib.EF_TRUNCATED) != 0
        return self.obs, self.reward, terminated, truncated

    def launch_step(self, actions: torch.Tensor, auto_reset: bool = False, terminal_obs: bool = False):
        """Enqueue exactly one env step (model, logic and sensor kernels) on the current stream (no other device work when
        `actions` is already a contiguous float32/int32 tensor on this device)."""
        discrete = not actions.is_floating_point()
        a = actions.to(self.device, torch.int32 if discrete else torch.float32).contiguous()
        if a.numel() != self.N * (1 if discrete else 2):
            raise ValueError(f"actions must have {self.N * (1 if discrete else 2)} elements, got {tuple(a.shape)}")
        with torch.cuda.device(self.device):
            _lib.check(self.L.nascar_step(self.h, _ptr(a), int(discrete), _ptr(self.obs), _ptr(self.reward),
                                          _ptr(self.car_flags), _ptr(self.env_flags), int(auto_reset),
                                          _ptr(self.terminal_obs) if terminal_obs else None, _stream()))

    def step_driven(self, policy: int, seed: int = 0, step: int = 0, auto_reset: bool = True, terminal_obs: bool = False):
        """One env step whose actions come from device action source `policy` (0 uniform, 1 rule driver, 3 noisy rule
        driver) on the current obs, computed inside the step launch; equals policy_actions(policy, seed, step) +
        step(...).  Policies 2 and 4 (MLP controllers) raise: use policy_actions + step, or rollout."""
        with torch.cuda.device(self.device):
            _lib.check(self.L.nascar_step_driven(self.h, int(policy), int(seed), int(step), _ptr(self.obs), _ptr(self.reward),
                                                 _ptr(self.car_flags), _ptr(self.env_flags), int(auto_reset),
                                                 _ptr(self.terminal_obs) if terminal_obs else None, _stream()))
        return self.obs, self.reward

    def rollout(self, policy: int, steps: int, seed: int = 0, step0: int = 0, auto_reset: bool = True,
                trajectory: bool = False, out=None, obs_trajectory: bool = False):
        """`steps` env steps in one call (sharded over streams, or one fused launch: set_rollout_streams), actions
        from device action source `policy` (0 uniform, 1 rule driver, 2 the SAC actor -- sharded only, 3 noisy rule
        driver, 4 the field of per-car controllers, set_car_controllers -- sharded only, 5 the genome drivers,
        set_genomes -- sharded only, not with set_rollout_pipe) on the previous observation; equals `steps` x
        (policy_actions(policy, seed, step0 + k) + step(..., auto_reset)).  With set_fitness on, every step also updates
        the per-car fitness accumulators (auto_reset must be False).  Returns (obs, reward, car_flags, env_flags): the last step's, or with
        trajectory=True the per-step records [steps, E, C] / [steps, E] (obs the last step's).  obs_trajectory=True
        (with trajectory=True, sharded rollout only) also records every step's observation: obs [steps + 1, E, C, 38],
        record 0 the observation before the rollout, record k + 1 the one after step k (a learner's rollout buffer,
        written by the kernels in place).  `out`: caller-owned buffers (reward, car_flags, env_flags), preceded by
        obs when obs_trajectory, each with at least the records this call writes."""
        steps = int(steps)
        if out is not None and not trajectory:
            raise ValueError("`out` buffers are written only with trajectory=True")
        if obs_trajectory and not trajectory:
            raise ValueError("obs_trajectory needs trajectory=True")
        if trajectory and out is not None:      # caller-owned per-step buffers (at least `steps` records)
            n_out = 4 if obs_trajectory else 3
            if len(out) != n_out:
                raise ValueError("out must be (" + ("obs, " if obs_trajectory else "") + "reward, car_flags, env_flags)")
            ot = out[0] if obs_trajectory else None
            rew, cf, ef = out[n_out - 3:]
            checks = [("reward", rew, torch.float32, (self.E, self.C), steps),
                      ("car_flags", cf, torch.uint8, (self.E, self.C), steps),
                      ("env_flags", ef, torch.uint8, (self.E,), steps)]
            if obs_trajectory:
                checks.append(("obs", ot, torch.float32, (self.E, self.C, _lib.OBS_DIM), steps + 1))
            for name, t, dt, inner, n in checks:
                self._check_record_buffer(name, t, dt, inner, n)
        elif trajectory:
            rew = torch.empty(steps, self.E, self.C, dtype=torch.float32, device=self.device)
            cf = torch.empty(steps, self.E, self.C, dtype=torch.uint8, device=self.device)
            ef = torch.empty(steps, self.E, dtype=torch.uint8, device=self.device)
            ot = (torch.empty(steps + 1, self.E, self.C, _lib.OBS_DIM, dtype=torch.float32, device=self.device)
                  if obs_trajectory else None)
        else:
            rew, cf, ef, ot = self.reward, self.car_flags, self.env_flags, None
        traj = (_lib.TRAJ_RECORDS if trajectory else 0) | (_lib.TRAJ_OBS if obs_trajectory else 0)
        with torch.cuda.device(self.device):
            if ot is not None:
                ot[0].copy_(self.obs)
            _lib.check(self.L.nascar_rollout(self.h, int(policy), int(seed), int(step0), steps,
                                             _ptr(ot if ot is not None else self.obs), _ptr(rew), _ptr(cf), _ptr(ef),
                                             int(auto_reset), traj, _stream()))
            if trajectory and steps > 0:
                self.reward.copy_(rew[steps - 1]); self.car_flags.copy_(cf[steps - 1]); self.env_flags.copy_(ef[steps - 1])
                if ot is not None:
                    self.obs.copy_(ot[steps])
        return (ot if ot is not None else self.obs), rew, cf, ef

    def _check_record_buffer(self, name, t, dtype, inner, steps):
        """the kernels write record k at data_ptr + k * prod(inner) elements: anything but a contiguous tensor of
        this dtype on this device with shape [>= steps, *inner] would be written out of bounds (steps: the records
        this call writes)"""
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"out {name}: expected a torch.Tensor, got {type(t).__name__}")
        if t.device != self.device:
            raise ValueError(f"out {name}: on {t.device}, the env is on {self.device}")
        if t.dtype != dtype:
            raise ValueError(f"out {name}: dtype {t.dtype}, expected {dtype}")
        if tuple(t.shape[1:]) != inner or t.dim() != len(inner) + 1:
            raise ValueError(f"out {name}: shape {tuple(t.shape)}, expected [>= {steps}, {', '.join(map(str, inner))}]")
        if t.shape[0] < steps:
            raise ValueError(f"out {name}: holds {t.shape[0]} records, fewer than steps = {steps}")
        if not t.is_contiguous():
            raise ValueError(f"out {name}: must be contiguous")

    def set_step_events(self, events=None):
        """Profiling hook (nascar_set_step_events): 4 torch.cuda.Event(enable_timing=True) recorded by every following
        whole-grid step on its stream -- before model_kernel, after model_kernel, after logic_kernel, after the
        sensor launch -- so their elapsed times are the three kernels' durations; None switches it off."""
        if events is None:
            _lib.check(self.L.nascar_set_step_events(self.h, None, 0))
            self._step_events = None
            return
        if len(events) != 4:
            raise ValueError("need 4 events")
        with torch.cuda.device(self.device):
            for e in events:
                if not e.cuda_event:   # torch creates the HIP event at its first record
                    e.record()
            arr = (ctypes.c_void_p * 4)(*[ctypes.c_void_p(e.cuda_event) for e in events])
            _lib.check(self.L.nascar_set_step_events(self.h, arr, 4))
        self._step_events = list(events)    # kept alive while the engine may record them

    def info_tensor(self) -> torch.Tensor:
        """per-car info [E, C, N_INFO] float64 (fields: _lib.INFO_FIELDS)."""
        with torch.cuda.device(self.device):
            _lib.check(self.L.nascar_get_info(self.h, _ptr(self._info), _stream()))
        return self._info

    def termination_reason(self) -> torch.Tensor:
        return (self.env_flags >> 4) & 7

    def set_actor(self, weights, precision: str = "fp32"):
        """Load an SB3 SAC MlpPolicy actor: a dict from nascargymnasium_amd.policy.load_sb3_actor / random_actor.
        precision "fp32" (default): float32 throughout, the reference's model.predict precision (<= 1e-5 on the
        reference's sac_1235 checkpoint); "bf16": the MFMA kernel (bf16 operands, fp32 accumulation), ~8x faster but
        NOT faithful for trained policies (max |delta action| 0.40 on sac_1235)."""
        from .policy import actor_arrays
        if precision not in ("bf16", "fp32"):
            raise ValueError("precision must be 'bf16' or 'fp32'")
        arrs = actor_arrays(weights)
        fp = ctypes.POINTER(ctypes.c_float)
        _lib.check(self.L.nascar_set_actor(self.h, *[a.ctypes.data_as(fp) for a in arrs], 38, 256, 2))
        _lib.check(self.L.nascar_set_actor_precision(self.h, int(precision == "fp32")))
        self._actor_arrays = arrs

    def actor_forward(self, obs: torch.Tensor) -> torch.Tensor:
        """The loaded actor on a device batch of observations [..., 38] -> actions [..., 2]."""
        o = obs.to(self.device, torch.float32).contiguous()
        n = o.numel() // 38
        out = torch.empty(o.shape[:-1] + (2,), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.L.nascar_actor_forward(self.h, _ptr(o), n, _ptr(out), _stream()))
        return out

    # ------------------------------------------------------------------ per-car controllers (policy 4, "the field")
    def add_controller(self, ctrl) -> int:
        """Load one MLP controller (nascargymnasium_amd.policy.Controller: load_sb3_policy for the reference's SAC /
        PPO / A2C checkpoints, random_mlp) onto the device; returns its id for set_car_controllers /
        controller_forward.  At most 16 per env; shapes the kernels do not hold (_lib.check_controller) raise."""
        m, _keep = _lib.mlp_struct(ctrl)
        with torch.cuda.device(self.device):
            return _lib.check(self.L.nascar_add_controller(self.h, ctypes.byref(m)))

    def controller_forward(self, cid: int, obs: torch.Tensor) -> torch.Tensor:
        """Controller `cid` on a device batch of observations [..., 38] -> actions [..., 2] (float32 MFMA kernel)."""
        o = obs.to(self.device, torch.float32).contiguous()
        n = o.numel() // 38
        out = torch.empty(o.shape[:-1] + (2,), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.L.nascar_controller_forward(self.h, int(cid), _ptr(o), n, _ptr(out), _stream()))
        return out

    def set_car_controllers(self, ctrl=None):
        """The field: the car in slot c of every env is driven by ctrl[c] -- a controller id from add_controller, or
        "rule" (policy 1), "uniform" (policy 0), "noisy" (policy 3), "genome" (policy 5: the slot's cars run their genomes
        of set_genomes, which comes first) -- as the reference's race modes build one controller per car (game/competition.py:150-212).  policy_actions(4) and rollout(4, ...) then run it.  None clears it."""
        if ctrl is None:
            _lib.check(self.L.nascar_set_car_controllers(self.h, None))
            return
        ctrl = list(ctrl)
        if len(ctrl) != self.C:
            raise ValueError(f"need one controller per car slot ({self.C}), got {len(ctrl)}")
        codes = []
        for c in ctrl:
            if isinstance(c, str):
                if c not in _lib.CTRL_BUILTIN:
                    raise ValueError(f"unknown built-in controller {c!r} (one of {sorted(_lib.CTRL_BUILTIN)})")
                c = _lib.CTRL_BUILTIN[c]
            codes.append(int(c))
        arr = (ctypes.c_int32 * self.C)(*codes)
        _lib.check(self.L.nascar_set_car_controllers(self.h, arr))

    # ------------------------------------------------------------------ genome drivers and on-device fitness (policy 5)
    FITNESS_FIELDS = _lib.FITNESS_FIELDS

    def set_genomes(self, genomes=None):
        """One 12-gene genome per car for the genome driver (policy 5, and "genome" slots of set_car_controllers): an
        array [E, C, 12] or [E * C, 12] of Python-float (float64) genes in GeneticController.default_genome's order
        (nascargymnasium_amd.genetic.GENOME_NAMES); None clears the table.  The driver is
        BaseController._fallback_control with its constants replaced by the genes (include/nascar.h).  Every gene
        must be finite.  The upload is ordered on the current stream."""
        if genomes is None:
            _lib.check(self.L.nascar_set_genomes(self.h, None, _stream()))
            return
        g = np.ascontiguousarray(np.asarray(genomes, dtype=np.float64))
        if g.shape not in ((self.E, self.C, _lib.N_GENES), (self.N, _lib.N_GENES)):
            raise ValueError(f"genomes must be [{self.E}, {self.C}, {_lib.N_GENES}] or [{self.N}, {_lib.N_GENES}], "
                             f"got {tuple(g.shape)}")
        with torch.cuda.device(self.device):
            _lib.check(self.L.nascar_set_genomes(self.h, g.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), _stream()))

    def set_fitness(self, enable: bool = True):
        """On-device fitness accumulators (learn/genetic_trainer.py:253-285 per car, float64): while enabled, every
        `step` / `step_driven` and every step of the sharded `rollout` adds the step's reward, speed, distance, time on
        track, lap and disable records of each car whose env has not ended; an env's terminal step is counted, then its
        cars freeze.  Enabling (again) zeroes them.  Steps must run with auto_reset=False while it is on."""
        with torch.cuda.device(self.device):
            _lib.check(self.L.nascar_set_fitness(self.h, int(bool(enable)), _stream()))

    def fitness(self) -> torch.Tensor:
        """The accumulators as an [E, C, 8] float64 device tensor (fields: FITNESS_FIELDS; lap_time NaN without a lap,
        disabled_at_step -1 for a car that was never disabled)."""
        out = torch.empty(self.E, self.C, _lib.N_FITNESS, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.L.nascar_get_fitness(self.h, _ptr(out), _stream()))
        return out

    # ------------------------------------------------------------------ race modes (game/competition.py, game/time_trial.py)
    RACE_FIELDS = _lib.RACE_FIELDS

    def set_race(self, mode, laps_per_attempt: int = 2):
        """The race ledger (include/nascar.h): mode 0 / None off, 1 / "competition", 2 / "time_trial".  While on, every
        `step` / `step_driven` and every step of the sharded `rollout` updates, per car of an env that has not ended, the
        float32 reward sum, the lap events (best and last lap, finishing time, the env's fastest lap and its car) and, in
        the time trial, the parked flag: a car that has timed `laps_per_attempt` laps, or is disabled, is parked -- it
        takes action (0, 0) from then on and its controller is not run (rollout policies 2, 4, 5 and policy_actions).
        Steps must run with auto_reset=False while it is on.  The first call initialises the ledger; `race_begin`
        starts a new race or attempt."""
        mode = {None: 0, "off": 0, "competition": 1, "time_trial": 2}.get(mode, mode)
        if mode not in (0, 1, 2):
            raise ValueError(f"race mode must be 0 / None, 1 / 'competition' or 2 / 'time_trial', got {mode!r}")
        r = _lib.NascarRace(int(mode), int(laps_per_attempt))
        with torch.cuda.device(self.device):
            _lib.check(self.L.nascar_set_race(self.h, ctypes.byref(r), _stream()))
        self._race = (int(mode), int(laps_per_attempt))

    def race_mode(self):
        """(mode, laps_per_attempt) as the last set_race left them; (0, 2) before any"""
        return getattr(self, "_race", (0, 2))

    def race_begin(self, keep_records: bool = False):
        """A new race or attempt: clears the ledger's per-attempt fields, the parked flags and the envs' ended bytes;
        keep_records=True keeps best laps, timed-lap totals and the envs' fastest laps (the time trial across attempts).
        The envs are not reset: call `reset`."""
        with torch.cuda.device(self.device):
            _lib.check(self.L.nascar_race_begin(self.h, int(bool(keep_records)), _stream()))

    def race(self) -> "RaceLedger":
        """The ledger: RaceLedger(ledger [E, C, 10] float64 (fields: RACE_FIELDS; best_lap, last_lap, finish_time NaN
        where there is none), fastest_car [E] int32 (-1: none), ended [E] uint8), device tensors."""
        led = torch.empty(self.E, self.C, _lib.N_RACE, dtype=torch.float64, device=self.device)
        fc = torch.empty(self.E, dtype=torch.int32, device=self.device)
        ended = torch.empty(self.E, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.L.nascar_get_race(self.h, _ptr(led), _ptr(fc), _ptr(ended), _stream()))
        return RaceLedger(led, fc, ended)

    def race_racing(self) -> int:
        """How many envs have not ended their race or attempt (one device count, read to the host)."""
        ended = torch.empty(self.E, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.L.nascar_get_race(self.h, None, None, _ptr(ended), _stream()))
        return int((ended == 0).sum().item())

    def race_rank(self, mode: int, ledger: torch.Tensor = None, fastest_car: torch.Tensor = None) -> "RaceRank":
        """Finishing order and points (mode 1 competition, 2 time trial) of the handle's own ledger, or of a given
        `ledger` [n_env, n_cars, 10] float64 (and `fastest_car` [n_env] int32, None: no fastest-lap bonus) in `race`'s
        layout: RaceRank(order [n_env, n_cars] (the car at position p), position, points [n_env, n_cars]), int32 device
        tensors -- Python's stable sorted() on the reference's key tuples and its two points tables."""
        if ledger is None:
            if fastest_car is not None:
                raise ValueError("fastest_car is given with a ledger")
            E, C, lp, fp = self.E, self.C, None, None
        else:
            if ledger.dim() != 3 or ledger.shape[2] != _lib.N_RACE or not 1 <= ledger.shape[1] <= 64:
                raise ValueError(f"ledger must be [n_env, n_cars <= 64, {_lib.N_RACE}], got {tuple(ledger.shape)}")
            ledger = ledger.to(self.device, torch.float64).contiguous()
            E, C = int(ledger.shape[0]), int(ledger.shape[1])
            if fastest_car is not None:
                fastest_car = fastest_car.to(self.device, torch.int32).contiguous()
                if tuple(fastest_car.shape) != (E,):
                    raise ValueError(f"fastest_car must be [{E}], got {tuple(fastest_car.shape)}")
            lp, fp = _ptr(ledger), (_ptr(fastest_car) if fastest_car is not None else None)
        out = [torch.empty(E, C, dtype=torch.int32, device=self.device) for _ in range(3)]
        with torch.cuda.device(self.device):
            _lib.check(self.L.nascar_race_rank(self.h, lp, fp, E, C, int(mode), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                                               _stream()))
        return RaceRank(*out)

    # ------------------------------------------------------------------ on-policy collection (policy 6)
    def set_actor_critic(self, ac):
        """Load a nascargymnasium_amd.policy.ActorCritic (load_sb3_actor_critic for the reference's PPO / A2C checkpoints,
        random_actor_critic, ActorCriticNet.export) as the handle's sampled actor-critic: policy 6 of policy_actions, and
        what `collect` runs.  Takes two of the handle's 16 controller ids; `update_actor_critic` replaces the weights
        without taking more.  A policy.DiscreteActorCritic (load_sb3_discrete_actor_critic,
        random_discrete_actor_critic, CategoricalActorCriticNet.export) loads the categorical actor of the env's
        Discrete(5) the same way: `collect` then returns a DiscreteRolloutBatch."""
        mp, mv, ls, _keep = self._ac_structs(ac)
        with torch.cuda.device(self.device):
            pi_id = _lib.check(self.L.nascar_add_controller(self.h, ctypes.byref(mp)))
            vf_id = _lib.check(self.L.nascar_add_controller(self.h, ctypes.byref(mv)))
        _lib.check(self.L.nascar_set_actor_critic(self.h, pi_id, vf_id, ls.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
        self._ac_ids = (pi_id, vf_id)
        self._ac_discrete = not hasattr(ac, "log_std")

    @staticmethod
    def _ac_structs(ac):
        """(actor NascarMlp, critic NascarMlp, log_std, the arrays they point to) of an ActorCritic or a
        DiscreteActorCritic (no log_std: the library reads none for a categorical actor, but NULL would clear)"""
        from .policy import OUT_CATEGORICAL, OUT_SAMPLE
        discrete = not hasattr(ac, "log_std")
        mp, kp = _lib.mlp_struct(ac.pi, OUT_CATEGORICAL if discrete else OUT_SAMPLE)
        mv, kv = _lib.mlp_struct(ac.vf)
        ls = np.zeros(2, np.float32) if discrete else np.ascontiguousarray(ac.log_std, np.float32)
        return mp, mv, ls, (kp, kv)

    def update_actor_critic(self, ac):
        """New weights and log_std of the same shapes and activations into the loaded actor-critic, ordered on the
        current stream: a learner's per-iteration update.  Another shape, activation or kind (a DiscreteActorCritic into
        a Gaussian-loaded handle, or the reverse) raises."""
        if getattr(self, "_ac_ids", None) is None:
            raise RuntimeError("update_actor_critic: no actor-critic loaded (set_actor_critic first)")
        mp, mv, ls, _keep = self._ac_structs(ac)
        with torch.cuda.device(self.device):
            _lib.check(self.L.nascar_update_controller(self.h, self._ac_ids[0], ctypes.byref(mp), _stream()))
            _lib.check(self.L.nascar_update_controller(self.h, self._ac_ids[1], ctypes.byref(mv), _stream()))
        _lib.check(self.L.nascar_set_actor_critic(self.h, self._ac_ids[0], self._ac_ids[1],
                                                  ls.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))

    def collect(self, steps: int, seed: int = 0, step0: int = 0, gamma: float = 0.99, gae_lambda: float = 0.95, out=None):
        """One on-policy rollout of `steps` steps on the device, SB3's OnPolicyAlgorithm.collect_rollouts followed by
        RolloutBuffer.compute_returns_and_advantage: per step the loaded actor-critic samples a ~ N(mu(obs), exp(log_std)),
        records a, its log-probability and V(obs), and clip(a, -1, 1) steps the envs with auto-reset; envs that a time
        limit cut (truncated, not terminated) record V(terminal obs) for the reward bootstrap.  Runs on the sharded
        rollout's streams; equals `steps` x (policy_actions(6, seed, step0 + k) + step(auto_reset=True)).  Returns a
        nascargymnasium_amd.onpolicy.RolloutBatch; `out`: a RolloutBatch of caller-owned buffers with at least `steps`
        records (steps + 1 of obs and values) to write into.
        Under set_normalize the loop is the one SB3 runs around a VecNormalize: the actor-critic sees `norm_obs`, every
        step ends with `normalize_step`, GAE takes the normalised rewards, and the batch is a NormalizedRolloutBatch
        (obs and rewards normalised, raw_rewards beside them; `out` then is one too); equals `steps` x
        (policy_actions(6, obs=norm_obs) + step(auto_reset=True, terminal_obs=True) + normalize_step(terminal_obs=True)).
        With a DiscreteActorCritic loaded the actor is the categorical one: the batch is a DiscreteRolloutBatch (under
        set_normalize a NormalizedDiscreteRolloutBatch) whose actions are the sampled int32 indices [K, E, C], which step
        the envs as step()'s discrete actions do; `out` then is of that kind."""
        from .onpolicy import DiscreteRolloutBatch, NormalizedDiscreteRolloutBatch, NormalizedRolloutBatch, RolloutBatch
        K = int(steps)
        if K < 1:
            raise ValueError("collect needs steps >= 1")
        E, C = self.E, self.C
        if getattr(self, "_ac_discrete", False):
            Batch = DiscreteRolloutBatch if self.normalize is None else NormalizedDiscreteRolloutBatch
        else:
            Batch = RolloutBatch if self.normalize is None else NormalizedRolloutBatch
        spec = Batch.spec(E, C)
        if out is None:
            out = Batch(*[torch.empty((K + extra, *inner), dtype=dt, device=self.device)
                          for _name, dt, inner, extra in spec])
        else:
            if len(out) != len(spec) or (type(out).__name__.endswith("RolloutBatch") and not isinstance(out, Batch)):
                raise ValueError(f"out must be a {Batch.__name__} ({len(spec)} buffers), got " +
                                 (f"a {type(out).__name__}" if len(out) == len(spec) else str(len(out))))
            for (name, dt, inner, extra), t in zip(spec, out):
                self._check_record_buffer(name, t, dt, inner, K + extra)
        with torch.cuda.device(self.device):
            if self.normalize is None:
                out.obs[0].copy_(self.obs)
                _lib.check(self.L.nascar_collect(self.h, int(seed), int(step0), K, _ptr(out.obs), _ptr(out.rewards),
                                                 _ptr(out.car_flags), _ptr(out.env_flags), _ptr(out.actions),
                                                 _ptr(out.log_probs), _ptr(out.values), _ptr(out.timeout_values), _stream()))
            else:
                nobs, nrew, _nterm = self._norm_buffers()
                out.obs[0].copy_(nobs)
                _lib.check(self.L.nascar_collect_normalized(
                    self.h, int(seed), int(step0), K, _ptr(self.obs), _ptr(out.obs), _ptr(out.rewards), _ptr(out.raw_rewards),
                    _ptr(out.car_flags), _ptr(out.env_flags), _ptr(out.actions), _ptr(out.log_probs), _ptr(out.values),
                    _ptr(out.timeout_values), _stream()))
            _lib.check(self.L.nascar_gae(self.h, _ptr(out.rewards), _ptr(out.values), _ptr(out.timeout_values),
                                         _ptr(out.env_flags), K, float(gamma), float(gae_lambda), _ptr(out.advantages),
                                         _ptr(out.returns), _stream()))
            self.car_flags.copy_(out.car_flags[K - 1]); self.env_flags.copy_(out.env_flags[K - 1])
            if self.normalize is None:
                self.reward.copy_(out.rewards[K - 1]); self.obs.copy_(out.obs[K])
            else:                                   # (self.obs, raw, was stepped in place)
                self.reward.copy_(out.raw_rewards[K - 1]); nrew.copy_(out.rewards[K - 1]); nobs.copy_(out.obs[K])
        if any(t.shape[0] != K + extra for (_n, _d, _i, extra), t in zip(spec, out)):   # larger caller buffers: this call's records
            out = Batch(*[t[:K + extra] for (_n, _d, _i, extra), t in zip(spec, out)])
        return out

    # ------------------------------------------------------------------ running normalisation (SB3's VecNormalize)
    def set_normalize(self, norm_obs: bool = True, norm_reward: Optional[bool] = None, clip_obs: float = 10.0, clip_reward: float = 10.0,
                      gamma: float = 0.99, epsilon: float = 1e-8, training: bool = True, stats=None):
        """SB3's VecNormalize on the device (the reference trains A2C under VecNormalize(norm_obs=True, norm_reward=True,
        clip_obs=1.0, gamma=0.99), learn/a2c.py:94-100): running float64 mean / variance of the 38 observation columns
        and of the discounted returns over the N = E * C car slots (each is one of SB3's envs), updated from every
        step's batch while `training`, frozen otherwise.  `collect` then runs its loop under it, `normalize_step` /
        `norm_obs` serve a per-step loop, and a full `reset()` performs VecNormalize.reset.  The batch moments are taken
        in float64 over the float32 rows (SB3's NumPy takes them in float32).  `stats`: a NormStats to start from
        (default: fresh ones when normalisation was off, the current ones when only the settings change).
        `set_normalize(False)` switches it off (rewards alone: `set_normalize(norm_obs=False, norm_reward=True)`; norm_reward
        left out means True).  While it is on `collect_transitions` raises, and the state snapshot
        (get_state / set_state) does not carry the statistics: norm_stats() / load_norm_stats() do."""
        with torch.cuda.device(self.device):
            if not norm_obs and not norm_reward:
                _lib.check(self.L.nascar_set_normalize(self.h, None, _stream()))
                self.normalize = None
                return
            norm_reward = True if norm_reward is None else norm_reward
            cfg = _lib.NascarNormalize(int(bool(norm_obs)), int(bool(norm_reward)), int(bool(training)), 0, float(clip_obs),
                                       float(clip_reward), float(gamma), float(epsilon))
            _lib.check(self.L.nascar_set_normalize(self.h, ctypes.byref(cfg), _stream()))
        self.normalize = dict(norm_obs=bool(norm_obs), norm_reward=bool(norm_reward), clip_obs=float(clip_obs),
                              clip_reward=float(clip_reward), gamma=float(gamma), epsilon=float(epsilon),
                              training=bool(training))
        if stats is not None:
            self.load_norm_stats(stats)

    def _norm_buffers(self):
        if self.normalize is None:
            raise RuntimeError("normalisation is off (set_normalize)")
        if self._norm_obs is None:
            self._norm_obs = torch.zeros_like(self.obs)
            self._norm_reward = torch.zeros_like(self.reward)
            self._norm_terminal_obs = torch.zeros_like(self.obs)
        return self._norm_obs, self._norm_reward, self._norm_terminal_obs

    @property
    def norm_obs(self) -> torch.Tensor:
        """the normalised current observation [E, C, 38], as the last full reset(), normalize_step() or collect() left it"""
        return self._norm_buffers()[0]

    @property
    def norm_reward(self) -> torch.Tensor:
        """the normalised reward [E, C] of the last normalize_step() or collect()"""
        return self._norm_buffers()[1]

    @property
    def norm_terminal_obs(self) -> torch.Tensor:
        """normalize_step(terminal_obs=True): the normalised terminal observation of the cars of envs that ended (other
        rows are stale)"""
        return self._norm_buffers()[2]

    def normalize_step(self, terminal_obs: bool = False):
        """VecNormalize.step_wait on the outputs of the last step (`obs`, `reward`, `env_flags`, and `terminal_obs` when
        asked: that step must have been taken with terminal_obs=True): updates the statistics while training, then
        returns (norm_obs, norm_reward); `norm_terminal_obs` holds the normalised terminal rows of the envs that ended."""
        nobs, nrew, nterm = self._norm_buffers()
        with torch.cuda.device(self.device):
            _lib.check(self.L.nascar_normalize_step(self.h, _ptr(self.obs), _ptr(self.reward), _ptr(self.env_flags),
                                                    _ptr(self.terminal_obs) if terminal_obs else None, _ptr(nobs), _ptr(nrew),
                                                    _ptr(nterm) if terminal_obs else None, _stream()))
        return nobs, nrew

    def norm_stats(self):
        """the running statistics and returns as a nascargymnasium_amd.normalize.NormStats (one host synchronisation)"""
        from .normalize import NormStats
        buf = torch.empty(_lib.NORM_STATS + self.N, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.L.nascar_get_norm_stats(self.h, _ptr(buf), _ptr(buf[_lib.NORM_STATS:]), _stream()))
        a = buf.cpu().numpy()
        return NormStats.from_record(a[:_lib.NORM_STATS], returns=a[_lib.NORM_STATS:].copy())

    def load_norm_stats(self, stats):
        """Upload a NormStats (its `returns`, when it has them, must hold one entry per car slot)."""
        stats.validate()
        rec = np.ascontiguousarray(stats.record())
        ret = None
        if stats.returns is not None:
            ret = np.ascontiguousarray(stats.returns, np.float64)
            if ret.size != self.N:
                raise ValueError(f"NormStats.returns holds {ret.size} entries, the env has {self.N} car slots")
        dp = ctypes.POINTER(ctypes.c_double)
        with torch.cuda.device(self.device):
            _lib.check(self.L.nascar_set_norm_stats(self.h, rec.ctypes.data_as(dp),
                                                    ret.ctypes.data_as(dp) if ret is not None else None, _stream()))

    def gae(self, rewards, values, timeout_values, env_flags, gamma: float = 0.99, gae_lambda: float = 0.95):
        """(advantages, returns) [K, E, C] of SB3's RolloutBuffer.compute_returns_and_advantage, float32 in its operation
        order (gae_kernel): rewards [K, E, C] (raw; gamma * timeout_values is added here), values [K + 1, E, C],
        timeout_values [K, E, C], env_flags [K, E] uint8 (done = terminated | truncated)."""
        K = int(rewards.shape[0])
        for name, t, dt, inner, n in (("rewards", rewards, torch.float32, (self.E, self.C), K),
                                      ("values", values, torch.float32, (self.E, self.C), K + 1),
                                      ("timeout_values", timeout_values, torch.float32, (self.E, self.C), K),
                                      ("env_flags", env_flags, torch.uint8, (self.E,), K)):
            self._check_record_buffer(name, t, dt, inner, n)
        adv = torch.empty(K, self.E, self.C, dtype=torch.float32, device=self.device)
        ret = torch.empty_like(adv)
        with torch.cuda.device(self.device):
            _lib.check(self.L.nascar_gae(self.h, _ptr(rewards), _ptr(values), _ptr(timeout_values), _ptr(env_flags), K,
                                         float(gamma), float(gae_lambda), _ptr(adv), _ptr(ret), _stream()))
        return adv, ret

    # ------------------------------------------------------------------ off-policy collection (policy 7)
    def set_explorer(self, actor_or_controller=None, sigma=None):
        """The exploring action source of SB3's off-policy algorithms (policy 7 of policy_actions, source 7 of
        collect_transitions): a nascargymnasium_amd.policy.SquashedActor (load_sb3_sac_actor, random_squashed_actor,
        SquashedActorNet.export) -- SAC's actor sampled, a = tanh(mu + exp(log_std) * eps) -- or an OUT_SQUASH Controller
        with `sigma` = (s0, s1) >= 0, TD3 / DDPG's NormalActionNoise on the deterministic action, clipped to the Box
        (sigma None = zeros: the controller's own action).  Takes one of the handle's 16 controller ids; `update_explorer`
        replaces weights and sigma without taking more.  None clears it."""
        from .policy import OUT_SQUASH, OUT_SQUASH_SAMPLE
        if actor_or_controller is None:
            _lib.check(self.L.nascar_set_explorer(self.h, -1, None))
            self._explorer = None
            return
        a = actor_or_controller
        if a.output not in (OUT_SQUASH, OUT_SQUASH_SAMPLE):
            raise ValueError(f"the explorer is a SquashedActor or an OUT_SQUASH Controller, not output {a.output}")
        if a.output == OUT_SQUASH_SAMPLE and sigma is not None:
            raise ValueError("a SquashedActor samples from its own log_std head: it takes no noise sigma")
        m, _keep = _lib.mlp_struct(a)
        with torch.cuda.device(self.device):
            cid = _lib.check(self.L.nascar_add_controller(self.h, ctypes.byref(m)))
        self._explorer = (cid, int(a.output))
        self._set_explorer_sigma(sigma)

    def _set_explorer_sigma(self, sigma):
        s = None if sigma is None else np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, np.float32), (2,)))
        _lib.check(self.L.nascar_set_explorer(self.h, self._explorer[0],
                                              None if s is None else s.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))

    def update_explorer(self, actor_or_controller=None, sigma=None):
        """New weights of the same shape, activation and kind into the loaded explorer, ordered on the current stream (a
        learner's per-iteration update), and / or a new noise sigma; takes no controller id."""
        if getattr(self, "_explorer", None) is None:
            raise RuntimeError("update_explorer: no explorer loaded (set_explorer first)")
        if actor_or_controller is not None:
            m, _keep = _lib.mlp_struct(actor_or_controller)
            with torch.cuda.device(self.device):
                _lib.check(self.L.nascar_update_controller(self.h, self._explorer[0], ctypes.byref(m), _stream()))
        if sigma is not None:
            self._set_explorer_sigma(sigma)

    def collect_transitions(self, replay, steps: int, seed: int = 0, step0: int = 0, source: int = 7):
        """`steps` steps of SB3's OffPolicyAlgorithm.collect_rollouts on the device: per step the explorer (source 7) or
        the uniform policy (source 0: the learning_starts warm-up) acts on the current observation, the envs step with
        auto-reset, and the transition -- obs, next_obs (the terminal observation where the env ended), the scaled action,
        reward, done, timeout, live -- goes into slot (replay.pos + k) % capacity of `replay`
        (nascargymnasium_amd.offpolicy.ReplayBuffer), whose pos / size advance.  Runs on the sharded rollout's streams, no
        host synchronisation; equals `steps` x (policy_actions(source, seed, step0 + k) + step(auto_reset=True,
        terminal_obs=True)) with the buffer filled on the host.  Returns the observation after the last step."""
        K = int(steps)
        if replay.E != self.E or replay.C != self.C or replay.device != self.device:
            raise ValueError("the replay buffer belongs to another env shape or device")
        with torch.cuda.device(self.device):
            r = replay.struct()
            _lib.check(self.L.nascar_collect_transitions(self.h, int(source), int(seed), int(step0), K, _ptr(self.obs),
                                                         ctypes.byref(r), int(replay.pos), _stream()))
        replay.advance(K)
        return self.obs

    def policy_actions(self, policy: int, seed: int = 0, step: int = 0, obs: Optional[torch.Tensor] = None):
        """device-generated actions: 0 uniform U[-1,1]^2, 1 BaseController fallback driver, 2 the SAC actor, 3 the noisy
        rule driver, 4 the field of per-car controllers (set_car_controllers), 5 the genome drivers (set_genomes: the
        rule driver with per-car evolved constants; shares the rule driver's per-car state), 6 the sampled actor-critic
        (set_actor_critic): clip(a, -1, 1) of the draw a ~ N(mu(obs), exp(log_std)) of (seed, car, step) -- with a
        DiscreteActorCritic the (throttle, steering) pair of the sampled action index (policy.DISCRETE_PAIRS) --, 7 the explorer
        (set_explorer): the sampled SAC actor, or a squashed actor with exploration noise -- the action that steps the env."""
        o = self.obs if obs is None else obs
        with torch.cuda.device(self.device):
            _lib.check(self.L.nascar_policy_actions(self.h, int(policy), int(seed), int(step), _ptr(o),
                                                    _ptr(self._actions), _stream()))
        return self._actions

    # ------------------------------------------------------------------ checkpointing
    def state_bytes(self) -> int:
        return int(self.L.nascar_state_bytes(self.h))

    def get_state(self) -> torch.Tensor:
        buf = torch.empty(self.state_bytes(), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.L.nascar_get_state(self.h, _ptr(buf), _stream()))
        return buf

    def set_state(self, buf: torch.Tensor):
        if buf.numel() != self.state_bytes():
            raise ValueError("state blob size mismatch")
        with torch.cuda.device(self.device):
            _lib.check(self.L.nascar_set_state(self.h, _ptr(buf.to(self.device).contiguous()), _stream()))

    def close(self):
        if getattr(self, "h", None):
            torch.cuda.synchronize(self.device)
            self.L.nascar_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
