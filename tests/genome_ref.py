"""Host oracles of the genome driver and the on-device fitness accumulators -- TEST INFRASTRUCTURE ONLY.

GenomeDriver is a literal restatement of the driver include/nascar.h documents: BaseController._fallback_control
(game/control/base_controller.py:64-103) with its constants replaced by genes, i.e. GeneticController.control
(game/control/genetic_controller.py:64-119) without its lines 81-82 (line 81 reads an attribute that is defined
nowhere).  It operates on np.float32 observation ELEMENTS with Python-float genes and a Python-dict state, exactly as
the reference's controllers do, so NumPy (NEP 50) decides every promotion: it is the oracle for the device's casts.

FitnessLoop accumulates what learn/genetic_trainer.py:253-285 accumulates, in Python floats, from the step's rewards and
the info tensor.
"""
import numpy as np


class GenomeDriver:
    def __init__(self, genome):
        self.g = [float(x) for x in genome]
        assert len(self.g) == 12
        self.control_state = {"throttle_brake": 0.0, "steering": 0.0, "last_forward": 0.0, "speed_limit": 0.0}

    def control(self, observation):
        g, s = self.g, self.control_state
        sensors = observation[22:38]
        right_sensors = sensors[15]
        left_sensors = sensors[1]
        forward = sensors[0]
        current_speed = observation[4]

        if s["last_forward"] >= forward:
            s["speed_limit"] = forward * g[10]
        if s["last_forward"] < forward:
            s["speed_limit"] = 1.0

        if current_speed < s["speed_limit"] * g[0]:
            s["throttle_brake"] += g[2]
        if current_speed > s["speed_limit"] * g[1]:
            s["throttle_brake"] -= g[3]

        with np.errstate(divide="ignore", invalid="ignore"):
            if right_sensors > left_sensors:
                s["steering"] = (1 - (left_sensors / right_sensors)) * g[4]
            elif left_sensors > right_sensors:
                s["steering"] = ((1 - (right_sensors / left_sensors)) * -1) * g[4]
            else:
                s["steering"] *= g[6]

        if abs(s["steering"]) > g[7]:
            s["throttle_brake"] *= g[5]

        s["throttle_brake"] = max(min(s["throttle_brake"], 1), -1)
        s["steering"] = max(min(s["steering"], 1), -1)
        s["last_forward"] = forward

        return np.array([s["throttle_brake"], s["steering"]], dtype=np.float32)

    def ctl(self):
        """the state as the device keeps it: four float64 (throttle_brake, steering, last_forward, speed_limit)"""
        s = self.control_state
        return np.array([float(s["throttle_brake"]), float(s["steering"]), float(s["last_forward"]),
                         float(s["speed_limit"])], np.float64)

    def steering_is_python_number(self):
        return not isinstance(self.control_state["steering"], np.floating)


class Float32GenomeDriver(GenomeDriver):
    """The same driver with the steering ALWAYS a numpy float32 (what a device without the per-car Python-number flag
    would compute): the clamp's int +-1 is cast back to float32."""

    def control(self, observation):
        a = super().control(observation)
        self.control_state["steering"] = np.float32(self.control_state["steering"])
        return a


def drive(drivers, obs):
    """controller.control(obs[i]) for every car: obs [N, 38] float32 -> actions [N, 2] float32"""
    return np.stack([d.control(obs[i]) for i, d in enumerate(drivers)])


FITNESS_FIELDS = ["total_reward", "distance_traveled", "max_speed", "time_on_track", "lap_completed", "lap_time",
                  "steps", "disabled_at_step"]


class FitnessLoop:
    """The trainer's metrics loop over N cars of E envs (C cars each) in Python floats; an env that has terminated or
    truncated is counted for that step and then stops, as the trainer's loop breaks."""

    def __init__(self, E, C):
        self.E, self.C = E, C
        self.m = [{"total_reward": 0.0, "distance_traveled": 0.0, "max_speed": 0.0, "time_on_track": 0.0,
                   "lap_completed": False, "lap_time": None, "steps": 0, "disabled_at_step": None}
                  for _ in range(E * C)]
        self.ended = [False] * E

    def update(self, rewards, info, done, idx):
        """rewards [N] float32, info [N, N_INFO] float64 (numpy), done [E] bool (terminated | truncated of this step);
        idx: the info tensor's field -> column map"""
        rew = [np.float32(x) for x in rewards.reshape(-1)]
        rows = info.reshape(self.E * self.C, -1).tolist()
        for e in range(self.E):
            if self.ended[e]:
                continue
            for n in range(e * self.C, (e + 1) * self.C):
                m, r = self.m[n], rows[n]
                m["total_reward"] += float(rew[n])
                speed = r[idx["speed"]]
                m["max_speed"] = max(m["max_speed"], speed)
                m["distance_traveled"] += speed * (1 / 60)
                if r[idx["on_track"]] != 0.0:
                    m["time_on_track"] += 1 / 60
                if r[idx["lap_count"]] > 0 and not m["lap_completed"]:
                    m["lap_completed"] = True
                    m["lap_time"] = r[idx["last_lap_time"]]
                m["steps"] += 1
                if r[idx["disabled"]] != 0.0 and m["disabled_at_step"] is None:
                    m["disabled_at_step"] = m["steps"]
            if done[e]:
                self.ended[e] = True

    def rows(self):
        """[N, 8] float64 in FITNESS_FIELDS order (lap_time NaN when None, disabled_at_step -1 when None)"""
        out = np.empty((len(self.m), 8), np.float64)
        for n, m in enumerate(self.m):
            out[n] = [m["total_reward"], m["distance_traveled"], m["max_speed"], m["time_on_track"],
                      float(m["lap_completed"]), np.nan if m["lap_time"] is None else m["lap_time"], float(m["steps"]),
                      -1.0 if m["disabled_at_step"] is None else float(m["disabled_at_step"])]
        return out


def synthetic_case(n_cars, steps, seed, bounds):
    """Genomes drawn from `bounds` ([12, 2]) and an observation sequence [steps, n_cars, 38] float32 (only speed,
    forward, left and right are non-zero) directed at the driver's edges.  Per car and step one of: an exact left /
    right tie (also right after a step that saturated the steering clamp), a pair that saturates the clamp when
    g[4] > 1, `forward` equal to the previous step's, `speed` exactly on speed_limit * g[0] or * g[1] (float32
    products, as the driver forms them), and -- for every 7th car, whose g[7] is set to it -- a steering exactly on
    g[7].  Returns (genomes [n_cars, 12] float64, obs, counts of the edges hit)."""
    rng = np.random.default_rng(seed)
    g = rng.uniform(bounds[:, 0], bounds[:, 1], size=(n_cars, 12))
    f32 = np.float32
    L7, R7 = f32(0.6), f32(0.8)
    for n in range(0, n_cars, 7):      # steering exactly on g[7] for the pair (L7, R7)
        g[n, 4] = rng.uniform(0.5, 1.9)
        g[n, 7] = float((1 - (L7 / R7)) * f32(g[n, 4]))
        assert bounds[7, 0] <= g[n, 7] <= bounds[7, 1]
    drivers = [GenomeDriver(g[n]) for n in range(n_cars)]
    obs = np.zeros((steps, n_cars, 38), np.float32)
    counts = dict(tie=0, tie_after_saturation=0, saturated=0, same_forward=0, on_lower=0, on_upper=0, on_g7=0,
                  python_number_tie=0)
    last_fwd = np.zeros(n_cars, np.float32)
    for k in range(steps):
        for n in range(n_cars):
            d = drivers[n]
            was_py = k > 0 and d.steering_is_python_number()
            u = rng.random(4)
            fwd = last_fwd[n] if (k > 0 and u[0] < 0.25) else f32(rng.uniform(0.02, 1.0))
            counts["same_forward"] += int(k > 0 and fwd == last_fwd[n])
            if was_py and u[1] < 0.7 or u[1] < 0.15:
                l = r = f32(rng.uniform(0.05, 1.0))
            elif u[1] < 0.45:                       # small ratio: (1 - l/r) * g[4] > 1 when g[4] is large enough
                a, b = f32(rng.uniform(0.005, 0.05)), f32(rng.uniform(0.5, 1.0))
                l, r = (a, b) if u[2] < 0.5 else (b, a)
            elif n % 7 == 0 and u[1] < 0.7:
                l, r = L7, R7
            else:
                l, r = f32(rng.uniform(0.05, 1.0)), f32(rng.uniform(0.05, 1.0))
            lim = fwd * f32(g[n, 10]) if d.control_state["last_forward"] >= fwd else f32(1.0)
            if u[3] < 0.2:
                spd = lim * f32(g[n, 0]); counts["on_lower"] += 1
            elif u[3] < 0.4:
                spd = lim * f32(g[n, 1]); counts["on_upper"] += 1
            else:
                spd = f32(rng.uniform(0.0, 1.3))
            o = obs[k, n]
            o[4], o[22], o[23], o[37] = spd, fwd, l, r
            d.control(o)
            tie = l == r
            counts["tie"] += int(tie)
            counts["tie_after_saturation"] += int(tie and was_py)
            counts["python_number_tie"] += int(tie and d.steering_is_python_number())
            counts["saturated"] += int(not tie and d.steering_is_python_number())
            counts["on_g7"] += int(not tie and abs(np.float32(d.control_state["steering"])) == f32(g[n, 7]))
            last_fwd[n] = fwd
    return g, obs, counts
