/*
 * include/nascar.h -- C ABI of the MI355X-native batched CarEnv (libnascar.so).
 *
 * Drop-in boundary for the reference's hot path: the Gymnasium CarEnv
 * step()/reset() of heihachi78/NascarGymnasium (src/car_env.py:678-803,
 * :316-535), whose per-car internals -- CarPhysics (src/car_physics.py),
 * Car/TyreManager/Tyre (src/car.py, src/tyre_manager.py, src/tyre.py),
 * DistanceSensor (src/distance_sensor.py), LapTimer (src/lap_timer.py) and the
 * Box2D calls they make through box2d-py SWIG -- run here as one fused HIP
 * kernel over E envs x C cars.  The Python CarEnv / batched VecEnv in
 * nascargymnasium_amd/ binds these entry points with ctypes.
 *
 * Conventions: every buffer argument of nascar_step/nascar_reset is a
 * caller-owned DEVICE pointer (e.g. torch tensor .data_ptr()); launches are
 * asynchronous on the caller's HIP stream (hipStream_t passed as void*).
 * Return code 0 = ok, negative = error; nascar_last_error() has the text.
 * No C++ exception crosses the ABI.  A handle is not thread-safe.
 */
#ifndef NASCAR_H
#define NASCAR_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct NascarHandle NascarHandle;

typedef struct NascarConfig {
    int32_t num_envs;        /* E */
    int32_t num_cars;        /* C in [1, 10] (src/constants/car_specs.py:50 MAX_CARS); up to 64 allowed */
    int32_t reset_on_lap;    /* CarEnv(reset_on_lap=...) (src/car_env.py:84) */
    int32_t device;          /* HIP device ordinal */
    double start_x, start_y, start_angle;   /* CarEnv start pose (src/car_env.py:114-115, 235-241) */
} NascarConfig;

/* CarEnv.__init__ (src/car_env.py:79-219): allocate E*C cars of device state. */
int nascar_create(const NascarConfig* cfg, NascarHandle** out);
void nascar_destroy(NascarHandle* h);
const char* nascar_last_error(void);

/* TrackLoader.load_track + CarPhysics._create_track_walls (src/track_generator.py:305-405,
 * src/car_physics.py:118-339).  Host arrays:
 *   segments: nseg x 13 float64 [type, length, sx, sy, ex, ey, width, curve_angle, curve_radius,
 *             left, start_heading, end_heading, banking]   (type: 0 GRID 1 STARTLINE 2 STRAIGHT 3 FINISHLINE 4 CURVE)
 *   walls:    nwall x 4 float64 [center_x, center_y, angle, half_length] as passed to Box2D
 * The float32 Box2D body transforms (glibc sinf/cosf), fat AABBs and listener keys
 * are derived on the host here.  Returns the track id (>= 0). */
int nascar_add_track(NascarHandle* h, const double* segments, int32_t nseg, double total_length,
                     const double* walls, int32_t nwall);
/* Track build cache (no reference counterpart: the reference rebuilds its walls per CarPhysics, src/car_physics.py:118,
 * and each SubprocVecEnv worker does so on its own, learn/ppo.py:77).  A track's tables (walls, grids and ~0.8 GB of
 * beam lists at 1 m cells, ~2 s of 16 host threads) are shared by every handle of the process; `retain` (default 8)
 * builds stay alive after their last handle closes, most recently used first (0: freed with the last handle).  `dir`
 * (NULL or "" = none, the default) holds on-disk copies of the host tables keyed by the track's arrays and cell size:
 * a process finding one loads it instead of building, one that builds writes it (temporary file + rename), and the
 * processes building one key serialise on a lock file, so the ranks of a node build each track once. */
int nascar_set_track_cache(int32_t retain, const char* dir);
/* Host only (no device): the host tables of one track (arguments as nascar_add_track, plus the beam-list cell size)
 * into the disk cache -- returns 1 if they were already there, 0 if built and written now, < 0 on error (no cache
 * directory set included).  A launcher prebuilds a job's tracks once before its ranks start. */
int nascar_prebuild_track(const double* segments, int32_t nseg, double total_length, const double* walls, int32_t nwall,
                          float beam_cell);

/* per-env track ids (host array of E ints); envs are grouped per track into workgroups (each track's workgroups spread
 * evenly over the workgroup order, so every shard of the sharded rollout holds a share of every track).  A changed id takes
 * effect at that env's next nascar_reset (fresh physics worlds on the new track, as CarEnv.reset recreates
 * CarPhysics, src/car_env.py:375-394); until then the env keeps stepping on its old track.  On a handle that has
 * not been reset, stepped or restored yet the ids apply at once. */
int nascar_set_env_tracks(NascarHandle* h, const int32_t* env_track);

/* Random-track mode, CarEnv(track_file=None) (src/car_env.py:243-303 _select_random_track / _load_random_track,
 * :331-333 and :375-394 in reset; learn/ppo.py:65-78 builds every training env this way).  With ntracks > 0, every
 * reset of an env -- nascar_reset of its mask bit, or the auto-reset inside nascar_step / nascar_step_driven /
 * nascar_rollout -- first draws its next track from the `ntracks` distinct track ids in `tracks` (nascar_add_track ids),
 * uniformly among those that are not its current track (all of them when it is not in the set), and an env whose
 * track changes gets fresh physics worlds there.  Draw k of env e (k counts its draws since seeding, starting at
 * draws[e], NULL = 0) is nascar_track_draw(seeds[e], k, current): a counter hash, reproducible on the host (the
 * reference re-seeds Python's `random` from pid + clock per draw).  The env -> track map, the counters and the
 * workgroup layout live on the device and are updated there (no host synchronisation per step).  ntracks = 0 ends
 * the mode (envs keep their current tracks).  While it is on, nascar_set_env_tracks fails, nascar_rollout runs one
 * shard, and the state snapshot (nascar_get_state) does not carry the env -> track map.  Host arrays; synchronises
 * `stream` once. */
int nascar_set_random_tracks(NascarHandle* h, const int32_t* tracks, int32_t ntracks, const uint64_t* seeds,
                             const int32_t* draws, void* stream);
/* The env -> track ids and the draws taken per env (device int32 [E] each, either may be NULL), on `stream`: the
 * device's in random-track mode, otherwise the host's assignment and zeros. */
int nascar_get_env_tracks(NascarHandle* h, int32_t* env_track, int32_t* draws, void* stream);
/* Host function (no device): the random-track draw for n envs -- out[i] = draw k[i] of seed seeds[i] from an env on
 * track current[i] (-1: none) over tracks[0 .. ntracks). */
int nascar_track_draw(int32_t n, const uint64_t* seeds, const int32_t* k, const int32_t* current, const int32_t* tracks,
                      int32_t ntracks, int32_t* out);

/* SB3 VecEnv glue of the drop-in VecCarEnv (stable_baselines3 Monitor + VecEnv around CarEnv.step, learn/ppo.py:65-78),
 * one launch per step on device buffers:
 * nascar_vec_post: done[e] = terminated | truncated (from env_flags); ep_ret [E*C] float64 += reward, ep_len [E] int64
 *   += 1, their new values copied to snap_ret / snap_len (Monitor's info["episode"] r / l for an env that just ended),
 *   then zeroed for the done envs.
 * nascar_check_actions: *bad (device int32) = 1 if any action is outside the action space (continuous: not in
 *   [-1, 1] or NaN; discrete int32: not in {0..4}) -- CarEnv.step's assert self.action_space.contains(action)
 *   (src/car_env.py:694), read by the caller when it next synchronises. */
int nascar_vec_post(NascarHandle* h, const float* reward, const uint8_t* env_flags, double* ep_ret, int64_t* ep_len,
                    uint8_t* done, double* snap_ret, int64_t* snap_len, void* stream);
int nascar_check_actions(NascarHandle* h, const void* actions, int32_t discrete, int32_t* bad, void* stream);

/* CarEnv.reset (src/car_env.py:316-535) for the envs whose env_mask[e] != 0 (device uint8[E];
 * NULL = all envs).  Writes obs [E*C*38] float32 of the reset envs. */
int nascar_reset(NascarHandle* h, const uint8_t* env_mask, float* obs, void* stream);

/* CarEnv.step (src/car_env.py:678-803) for all E envs.
 *   actions:   continuous: [E*C*2] float32 [throttle_brake, steering] (BaseEnv action space);
 *              discrete:   [E*C] int32 in {0..4} (BaseEnv._discrete_to_continuous, src/base_env.py:227-252)
 *   obs:       [E*C*38] float32 (src/car_env.py:935-946 layout)
 *   reward:    [E*C] float32
 *   car_flags: [E*C] uint8 (bit0 disabled, bit1 just disabled, bit2 collision impulse > 0, bit3 lap completed,
 *              bit7 engine overflow/error)
 *   env_flags: [E] uint8 (bit0 terminated, bit1 truncated, bit3 auto-reset done, bits4-6 termination reason)
 *   auto_reset != 0: envs that terminate/truncate are reset in the same launch; obs then holds the reset
 *              observation and terminal_obs (if non-NULL, [E*C*38]) the final one (SB3 VecEnv convention). */
int nascar_step(NascarHandle* h, const void* actions, int32_t discrete, float* obs, float* reward,
                uint8_t* car_flags, uint8_t* env_flags, int32_t auto_reset, float* terminal_obs, void* stream);

/* nascar_step with the actions of device action source `policy` (0, 1, 3: see nascar_policy_actions) computed on
 * the current obs inside the step launch -- one closed-loop driver step (game/control drivers' loop) without a
 * separate action launch; identical results to nascar_policy_actions(policy, seed, step) + nascar_step.  Policies 2
 * and 4 (the MLP controllers), 5 (the genome drivers) and 6 (the sampled actor-critic) are not available here: use
 * nascar_policy_actions + nascar_step, or nascar_rollout (policy 6: nascar_collect). */
int nascar_step_driven(NascarHandle* h, int32_t policy, uint64_t seed, int64_t step, float* obs, float* reward,
                       uint8_t* car_flags, uint8_t* env_flags, int32_t auto_reset, float* terminal_obs, void* stream);

/* Multi-step rollout: `steps` x (device action source on the current obs + CarEnv.step), i.e. the loop
 * of game/control drivers / learn/genetic_trainer.py:225-283 evaluation rollouts (actions from a policy on the
 * previous observation, src/car_env.py:678-803 per step), enqueued in one call with no host synchronisation.
 * Identical results to `steps` calls of nascar_policy_actions(policy, seed, step0 + k) + nascar_step(auto_reset).
 * Default implementation: the envs split into shards stepped on internal streams, forked from `stream` at the
 * start and joined into it at the end (nascar_set_rollout_streams); streams = 0 selects one fused launch.
 *   policy:  0 uniform, 1 BaseController._fallback_control, 3 noisy rule driver (policy 1 with 15 % of the
 *            car-steps uniform) -- see nascar_policy_actions; 2 the SAC actor (nascar_set_actor; sharded
 *            rollout only: each shard runs the actor on its own cars, one shard unless the envs sit in one
 *            track's workgroups in order); 4 the field of nascar_set_car_controllers (sharded rollout only, as
 *            policy 2: each shard runs the field on its own envs, one shard when the envs do not sit in one track's
 *            workgroups in order or random tracks are on; streams = 0 fails, and under nascar_set_rollout_pipe the
 *            streams setting applies); 5 the genome drivers of nascar_set_genomes (sharded rollout only: each shard
 *            runs the driver on the cars of its own workgroups, whatever the tracks; streams = 0 and the pipelined
 *            rollout fail, as does a handle without a genome table)
 *   obs:     [E*C*38] float32, in: the current observation, out: the last step's
 *   traj & NASCAR_TRAJ_RECORDS: reward [steps][E*C], car_flags [steps][E*C], env_flags [steps][E] (per-step records);
 *   traj == 0: reward [E*C], car_flags [E*C], env_flags [E] hold the last step's values.
 *   traj & NASCAR_TRAJ_OBS (with NASCAR_TRAJ_RECORDS; sharded rollout only): obs is [steps + 1][E*C*38]; record 0
 *            holds the current observation on entry (read by the action source of step 0) and step k writes
 *            record k + 1 (read by step k + 1) -- a learner's per-step observation buffer, no copies in between.
 * car_flags / env_flags may be NULL.  No terminal observations (auto-reset obs overwrite the final ones). */
#define NASCAR_TRAJ_RECORDS 1
#define NASCAR_TRAJ_OBS 2
int nascar_rollout(NascarHandle* h, int32_t policy, uint64_t seed, int64_t step0, int32_t steps, float* obs,
                   float* reward, uint8_t* car_flags, uint8_t* env_flags, int32_t auto_reset, int32_t traj, void* stream);

/* Rollout implementation (no reference counterpart: a scheduling choice with identical results).
 * streams >= 1: the envs split into `streams` shards of contiguous workgroups, each stepped by per-step launches
 * on its own stream (shard 0 on the caller's), so one shard's slow cars overlap the other shards' work; default:
 * 4, or the process's hardware queues if fewer (GPU_MAX_HW_QUEUES; two shards on one queue run back to back);
 * streams = 0: the fused rollout kernel (all steps in one launch, block barriers between the phases).
 * nascar_get_rollout_streams returns the current setting (-1 for a NULL handle). */
int nascar_set_rollout_streams(NascarHandle* h, int32_t streams);
int nascar_get_rollout_streams(NascarHandle* h);

/* Pipelined rollout (no reference counterpart: a scheduling choice with identical results).  sensor_workgroups > 0:
 * nascar_rollout runs its steps as two persistent kernels -- one workgroup per env group doing the vehicle model, the
 * Box2D step and the env logic K times, and `sensor_workgroups` sensor workgroups taking each group's sensor work from
 * a device queue as the group publishes it -- so every group goes on to its next step as soon as its own sensors are
 * done instead of waiting for the batch's slowest car.  Applies to policies 0, 1, 3 without random tracks, car
 * contact or obs trajectories (the streams setting applies otherwise, so to policies 2 and 4); 0 turns it off (default).  Every device wait
 * is clock-bounded: nascar_rollout_pipe_status waits for `stream` and returns 1 if a pipelined rollout since the
 * last status call gave up (its results are not valid), 0 if not, -1 on error. */
int nascar_set_rollout_pipe(NascarHandle* h, int32_t sensor_workgroups);
int nascar_rollout_pipe_status(NascarHandle* h, void* stream);

/* Workgroup layout (no reference counterpart: the reference loops over envs and cars one at a time,
 * learn/ppo.py:77 SubprocVecEnv and src/car_env.py:567-570; a scheduling choice with identical results).
 * The one-lane-per-car step kernels run 128-lane workgroups of `epb` whole envs each, epb in [1, 128 / C];
 * epb = 0 restores the automatic choice (128 / C, or fewer envs per workgroup when that leaves fewer than 2
 * workgroups per CU).  May be called at any time; the next launch uses the new layout.
 * nascar_get_envs_per_block returns the current value (-1 for a NULL handle). */
int nascar_set_envs_per_block(NascarHandle* h, int32_t epb);
int nascar_get_envs_per_block(NascarHandle* h);

/* Lanes per car of the distance-sensor kernel (no reference counterpart: DistanceSensor casts its 16 rays one after
 * another, src/distance_sensor.py:93-115): 4 (each lane walks rays r, r + 4, r + 8, r + 12) or 16 (one ray per
 * lane); 0 = automatic (16).  Identical results either way. */
int nascar_set_sensor_lanes(NascarHandle* h, int32_t lanes);

/* Threads per workgroup of the 16-lane distance-sensor kernel (no reference counterpart; src/distance_sensor.py:93-115
 * casts one ray at a time): 64 or 128 (the walks read the track's wall image from global memory; no LDS), 256, 512
 * or 1024 (each workgroup stages the wall image in LDS once for threads / 16 cars); 0 = automatic (128).  Identical
 * results at any size. */
int nascar_set_sensor_block(NascarHandle* h, int32_t threads);

/* Cell size (m) of the distance sensors' beam lists for the tracks added to this handle AFTER the call (host-built
 * per track in nascar_add_track; no reference counterpart -- DistanceSensor ray-casts against every wall,
 * src/distance_sensor.py:93-115).  Default 1 m: ~0.8 GB of device lists and ~2 s of host build
 * per track; 2 m quarters both for slightly longer list walks.  Range [0.5, 8].  Identical results at any size. */
int nascar_set_beam_cell(NascarHandle* h, float meters);

/* Step kernels (no reference counterpart; identical results): enable != 0 (default) runs the vehicle model + Box2D
 * step and the env logic (disable rules, lap timer, obs[0:22], rewards, termination, auto-reset;
 * src/car_env.py:537-803, 805-1158) as one launch per step, each workgroup starting its envs' logic when its own cars'
 * Box2D steps are done; 0 runs them as two launches (model_kernel, logic_kernel).  nascar_get_fused_logic returns the
 * current setting (-1 for a NULL handle). */
int nascar_set_fused_logic(NascarHandle* h, int32_t enable);
int nascar_get_fused_logic(NascarHandle* h);

/* Profiling hook (no reference counterpart; bench.py's per-kernel roofline): events = 4 caller-created timing
 * events (hipEvent_t), recorded by every following whole-grid step (nascar_step / nascar_step_driven) on its
 * stream before model_kernel, after model_kernel, after logic_kernel and after the sensor launch; n = 0 stops.
 * The events stay owned by the caller and must outlive their use. */
int nascar_set_step_events(NascarHandle* h, void* const* events, int32_t n);

/* Info builder (src/car_env.py:1160-1227, src/lap_timer.py:354-372): per-car float64 [E*C*N_INFO]
 * (field order: nascargymnasium_amd/_lib.py INFO_FIELDS) written to a device buffer. */
int nascar_get_info(NascarHandle* h, double* info, void* stream);

/* BUILD-ONLY EXTENSION, no reference counterpart (each reference car has its own b2World, so cars never touch):
 * enable != 0 makes the cars of an env collide -- staggered start grid (rows of 2, 8 m apart), and after the cars'
 * Box2D steps the env's car pairs within two circumradii are solved with Box2D's own contact algorithms for two dynamic
 * bodies: b2CollidePolygons manifolds of the car boxes (1-2 clip points, face normal, world points from
 * b2WorldManifold), then b2ContactSolver's sequential impulses -- per velocity iteration (6) and contact the tangent
 * impulses clamped by friction x normal impulse, then the accumulated normal impulses clamped at >= 0, with the angular
 * terms in the normal / tangent masses; fixture mixing of two car fixtures (friction sqrt(0.7 * 0.7), restitution
 * max(0.1, 0.1) as a velocity bias below -1 m/s), applied to both cars' linear and angular velocity.  Solved after (not
 * interleaved with) each car's wall island, point by point (no 2-point block solver), without warm start or position
 * correction.  The relative velocity at a contact point is formed in b2ContactSolver's association,
 * vB + wB x rB - vA - wA x rA, left to right.  The normal impulses count in the cars' collision impulse (damage / impact
 * disables).  WRITE-BACK: every car that a solved pair holds takes the solved velocity (the last normal pass can bring a
 * pair's normal impulse back to 0 after its friction, clamped by the iteration before, has moved both cars); a car whose
 * largest accumulated normal impulse is > 0 is also woken and reports the impulse (car flag bit 2); every other car keeps
 * the velocity its own Box2D step gave it.
 * CAPACITY: an env keeps at most num_cars touching pairs per step, taken in (i, j) order, i < j (num_cars * (num_cars -
 * 1) / 2 can touch in a pile of >= 4 cars, since overlap is not corrected).  Further touching pairs are not solved that
 * step; both cars of such a pair get the error flag (car flag bit 7, info's `error`), as after a wall-contact overflow,
 * until the env is reset.
 * Default 0 (reference behaviour); parity runs with 0.  Takes effect from the next reset (start grid) and step. */
int nascar_set_car_contact(NascarHandle* h, int32_t enable);

/* BUILD-ONLY EXTENSION, no reference counterpart (the reference's ray-cast callback drops every fixture that is not a
 * track wall, src/distance_sensor.py:45-47: its cars live in separate worlds): enable != 0 makes the 16 distance
 * sensors of a car see the other cars of its env.  Ray i of car n is the ray cast without the extension (same p1, same
 * float32 end point); its hit fraction becomes the minimum of the wall fraction and b2PolygonShape::RayCast against
 * the box of every other car of the env, taken from the poses the same sensor pass reads (the step's pose for obs and
 * terminal_obs, the auto-reset pose for the reset envs' obs): centre the body origin, rotation b2Rot::Set of the
 * float32 body angle, half extents of the car fixture, lower = 0 / upper = 1.  A ray that starts inside another
 * car's box reports no hit from it; a car never tests itself; disabled cars stay visible.  The value reaches
 * obs[22:38], terminal_obs[22:38], the rollout's obs trajectory and everything read from them; rewards, flags and
 * termination do not read the sensors and stay the reference's.  Independent of nascar_set_car_contact (with contact
 * off the cars are ghosts that are seen but not touched); not part of the state arena.  Default 0: every output is
 * the one without the extension, bit for bit.  Takes effect from the next reset / step / rollout.
 * Refused, with an error naming the combination, by reset / step / rollout in random-track mode and by the fused
 * single-launch rollout (rollout streams 0); the pipelined rollout falls back to the streams schedule.
 * nascar_get_car_visibility returns the current setting (-1 for a NULL handle). */
int nascar_set_car_visibility(NascarHandle* h, int32_t enable);
int nascar_get_car_visibility(NascarHandle* h);

/* Car.velocity_history for Car.validate_performance (src/car.py:173, 384-386, 1060-1098): enable != 0 keeps
 * every car's speed after each step in a 600-sample window on the device (VH_RING x N float32, outside the
 * state arena, so snapshots do not carry it) and nascar_get_info reports perf_count / perf_max_speed /
 * perf_first_fast; 0 frees it (the info fields then read -1 / 0 / -1).  Off by default. */
int nascar_set_perf_history(NascarHandle* h, int32_t enable, void* stream);

/* Raw state snapshot / restore (checkpointing and state-injection parity tests).  The snapshot does not carry the
 * random-track map (nascar_set_random_tracks) nor the running normalisation's statistics and returns
 * (nascar_get_norm_stats / nascar_set_norm_stats carry those). */
int64_t nascar_state_bytes(NascarHandle* h);
int nascar_get_state(NascarHandle* h, void* dst_device, void* stream);
int nascar_set_state(NascarHandle* h, const void* src_device, void* stream);

/* Device action sources:
 *   policy 0: counter-based uniform U[-1,1]^2 (key = seed, car, step)
 *   policy 1: BaseController._fallback_control (game/control/base_controller.py:39-103) from obs
 *   policy 2: the SAC actor loaded with nascar_set_actor, deterministic (SACController.control,
 *             game/control/sac_control_class.py:80-115) from obs
 *   policy 3: policy 1 with its action replaced by policy 0's draw on 15 % of the car-steps (counter hash)
 *   policy 4: "the field" -- the car in slot c of every env takes its action from ctrl[c] of
 *             nascar_set_car_controllers: a controller (nascar_add_controller) on that car's obs, or a built-in source,
 *             which produces exactly what policy 0, 1 or 3 produces for that car at the same (seed, step), the rule
 *             driver's per-car control state included; slots driven by a controller leave that state untouched.  One
 *             launch per distinct (h1, h2, activation) among the field's controllers plus one for the built-in slots,
 *             however many controllers are loaded.  Fails without a table.  actions 8-byte aligned.
 *   policy 5: the genome driver -- every car runs BaseController._fallback_control with its constants replaced by the
 *             car's 12 genes (nascar_set_genomes), one launch of its own (genome_policy_kernel); it shares the per-car
 *             control state with policies 1 and 3.  Fails without a genome table.
 *   policy 6: the sampled actor-critic of nascar_set_actor_critic -- every car draws a ~ N(mu(obs), exp(log_std)^2)
 *             from the Gaussian actor and takes min(max(a, -1), 1), the action SB3's collect_rollouts steps the env with;
 *             the draw is the one of (seed, car, step), see nascar_collect.  Fails without an actor-critic.  actions
 *             8-byte aligned.  With a categorical actor (output 6) every car draws an action index of the env's
 *             Discrete(5) and takes its (throttle, steering) pair, the one nascar_step(discrete = 1) steps the index with.
 *   policy 7: the explorer of nascar_set_explorer -- the sampled SAC actor, or a deterministic squashed actor with
 *             exploration noise; returns the action that steps the env.  Fails without an explorer.  actions 8-byte
 *             aligned. */
int nascar_policy_actions(NascarHandle* h, int32_t policy, uint64_t seed, int64_t step, const float* obs,
                          float* actions, void* stream);

/* SB3 SAC MlpPolicy actor weights (PyTorch layouts, host float32): w1 [256][38], b1 [256],
 * w2 [256][256], b2 [256], w3 = mu.weight [2][256], b3 = mu.bias [2]  (obs_dim 38, hidden 256,
 * act_dim 2; other shapes are rejected).  Replaces SAC.load + policy.predict
 * (game/control/sac_control_class.py:48-115) with one fused actor kernel: float32 by default, the bf16-operand
 * MFMA kernel on request (nascar_set_actor_precision). */
int nascar_set_actor(NascarHandle* h, const float* w1, const float* b1, const float* w2, const float* b2,
                     const float* w3, const float* b3, int32_t obs_dim, int32_t hidden, int32_t act_dim);
/* Actor arithmetic for policy 2 and nascar_actor_forward: 1 (default) = float32 throughout (the reference's
 * model.predict precision; <= 1e-5 on the reference's sac_1235 checkpoint, tests/test_gpu_actor.py), 0 = the
 * bf16-operand MFMA kernel (fp32 accumulation; ~8x faster: 16.2 vs 135 us at 81 920 observations, max |delta action|
 * 0.40 on sac_1235). */
int nascar_set_actor_precision(NascarHandle* h, int32_t fp32);
/* The loaded actor on any device batch: obs [n][38] float32 -> actions [n][2] float32 (both 8-byte aligned).  n = 0
 * launches nothing and returns 0; the pointers of an empty batch may be null (nascar_controller_forward likewise). */
int nascar_actor_forward(NascarHandle* h, const float* obs, int32_t n, float* actions, void* stream);

/* Per-car controllers: the reference's race modes put a different controller in every car of an env
 * (game/competition.py:150-212, 285-307; game/championship.py and game/time_trial.py likewise: one controller per car,
 * controller.control(obs[car_idx]) for each car before every env.step).  A controller here is a float32 MLP
 * obs[38] -> h1 -> h2 -> 2 actions run on the f32 MFMA (mlp_field_kernel, csrc/nascar_actor.h), covering every SB3
 * checkpoint kind the reference ships (game/control/models/):
 *   sac_*.zip             256-256, ReLU, output 2 (tanh-squashed, then unscale_action)   SACController.control
 *   ppo_789 / ppo_849     64-64, Tanh, output 1 (the mean clipped to the Box)            PPOController.control
 *   a2c_best_model3.zip   256-128, ReLU, output 1                                        A2CController.control
 * (A2CController predicts on the raw observation although the checkpoint was trained under VecNormalize,
 * game/control/a2c_control_class.py:104-111; this library does what the controller does.)
 * NascarMlp: host float32 arrays in PyTorch layouts, w1 [h1][38], b1 [h1], w2 [h2][h1], b2 [h2], w3 [2][h2], b3 [2];
 *   activation 0 ReLU, 1 Tanh (tanhf in float32), on both hidden layers;
 *   output 0 raw: mu = W3 h + b3;  1 clip: min(max(mu, -1), 1), SB3 predict for an unsquashed Box policy;
 *          2 squash: tanh(mu) followed by BasePolicy.unscale_action for the Box(-1, 1), as policy 2.
 * Shapes: obs_dim 38, act_dim 2 and (h1, h2) one of 256-256, 256-128, 256-32, 128-128, 64-64, 32-256; every other
 * shape is rejected with a message naming it -- TD3's SB3 default [400, 300] included (the reference ships no TD3
 * checkpoint; nor is the genetic controller covered: GeneticController.control raises).
 * The wide shape 512-512 with ReLU (learn/a2c.py:129: net_arch [512, 512], activation_fn ReLU) runs on a kernel of its own
 *   (mlp_wide_kernel: layer 2 in chunks of four output tiles under the sixteen layer-1 tiles) for every output but 5:
 *   nascar_set_explorer and the four-row head refuse it, and 512-512 Tanh is rejected by name.
 * Discrete(5) (CarEnv(discrete_action_space = True)): act_dim 5, w3 [5][h2], b3 [5], the logits l of SB3's categorical
 *   policy, with one of two outputs:
 *          6 categorical sample: CategoricalDistribution with deterministic = False, serving nascar_set_actor_critic like
 *            output 4 (the draw: below, with nascar_collect);
 *          7 categorical mode: the first maximum of the logits (strict > in index order), deterministic = True; a driver
 *            of the field like outputs 0-2 (nascar_set_car_controllers, nascar_controller_forward).
 *   Either writes the action as the (throttle / brake, steering) pair of nascar_step's discrete path: 0 -> (0, 0),
 *   1 -> (1, 0), 2 -> (-1, 0), 3 -> (0, -1), 4 -> (0, 1).  act_dim 5 with outputs 0-5, and outputs 6 / 7 with another
 *   act_dim, are errors.
 * nascar_check_controller (host only, no device, h not needed): 0 if nascar_add_controller would accept the shape,
 *   activation and output, < 0 with the message otherwise.
 * nascar_add_controller: copies the weights to the device; returns the controller's id >= 0 (at most 16 per handle;
 *   ids stay valid for the handle's life).  Two more kinds serve nascar_set_actor_critic and drive no car of the field
 *   (nascar_set_car_controllers and nascar_controller_forward refuse them): output 4, the sampled Gaussian actor (w3 / b3
 *   give the mean), and act_dim 1 with output 3, a critic (w3 [1][h2], b3 [1]: the value head).
 * nascar_update_controller: same-shape weights into a loaded controller, by an upload ordered on `stream` (launches
 *   enqueued before it on that stream run the old weights, later ones the new); h1, h2, activation, act_dim and output
 *   must be the loaded controller's, anything else is an error naming both.  A learner updates its nets every
 *   iteration, and a handle holds 16 ids.
 * nascar_controller_forward: controller `id` on any device batch, obs [n][38] -> actions [n][2] float32 (actions
 *   8-byte aligned).  256-256 ReLU with output 2 performs the float32 policy-2 kernel's operations in its order: the
 *   results are equal bit for bit.
 * nascar_set_car_controllers: ctrl is a host array [C]: the car in slot c of every env is driven by ctrl[c], a
 *   controller id or one of the built-in sources below; NULL clears the table.  The table is what policy 4 ("the
 *   field") of nascar_policy_actions and nascar_rollout runs; an id that was never returned by nascar_add_controller,
 *   or a negative value other than the four below, is an error.  NASCAR_CTRL_GENOME is accepted once a genome table
 *   is set (nascar_set_genomes first; without one the id is unknown, and a table cleared later fails the field's next
 *   run); the slot produces exactly what policy 5 produces for that car, sharing the rule sources' control state. */
typedef struct NascarMlp {
    int32_t obs_dim, h1, h2, act_dim;
    int32_t activation;      /* 0 ReLU, 1 Tanh */
    int32_t output;          /* 0 raw, 1 clip, 2 squash; 3 value (act_dim 1), 4 sampled: nascar_set_actor_critic;
                                5 squashed sample (act_dim 4): nascar_set_explorer; 6 categorical sample (act_dim 5):
                                nascar_set_actor_critic; 7 categorical mode (act_dim 5) */
    const float *w1, *b1, *w2, *b2, *w3, *b3;   /* PyTorch layouts, host */
} NascarMlp;
#define NASCAR_CTRL_RULE (-1)      /* policy 1 */
#define NASCAR_CTRL_UNIFORM (-2)   /* policy 0 */
#define NASCAR_CTRL_NOISY (-3)     /* policy 3 */
#define NASCAR_CTRL_GENOME (-4)    /* policy 5: the slot's cars run their genomes (nascar_set_genomes) */
int nascar_check_controller(const NascarMlp* mlp);
int nascar_add_controller(NascarHandle* h, const NascarMlp* mlp);
int nascar_controller_forward(NascarHandle* h, int32_t id, const float* obs, int32_t n, float* actions, void* stream);
int nascar_set_car_controllers(NascarHandle* h, const int32_t* ctrl);
int nascar_update_controller(NascarHandle* h, int32_t id, const NascarMlp* mlp, void* stream);

/* On-policy collection: the loop of SB3's on-policy algorithms, as learn/ppo.py:65-107 and learn/a2c.py run it
 * (OnPolicyAlgorithm.collect_rollouts, then RolloutBuffer.compute_returns_and_advantage), on the device.
 * nascar_set_actor_critic: the handle's actor-critic -- pi_id a sampled actor (output 4) and vf_id a critic (act_dim 1,
 *   output 3) from nascar_add_controller, and log_std [2] (host, finite; ActorCriticPolicy's state-independent log_std).
 *   log_std NULL clears it.  Calling it again with the same ids sets a new log_std (with nascar_update_controller: a
 *   learner's update).  pi_id may be a categorical actor (act_dim 5, output 6) instead: it has no log_std, and log_std is
 *   not read -- but must not be NULL, which clears: pass any two floats.
 * The draw of car n at (seed, step): with key the counter key of policy 0 (seed, n, step) and mix32 its hash,
 *     u0 = ((mix32(key ^ 0x5A4D504C45) >> 8) + 1) * 2^-24  in (0, 1]
 *     u1 = (mix32(key ^ 0x3C6EF372FE94F82B) >> 8) * 2^-24   in [0, 1)
 *     r = sqrtf(-2 logf(u0)),  eps = (r cosf(2 pi u1), r sinf(2 pi u1))          (Box-Muller, float32)
 *   a_j = mu_j + expf(log_std_j) * eps_j is the recorded action (unclipped, as SB3's buffer keeps it), min(max(a, -1), 1)
 *   steps the env, and logp = sum_j (-(a_j - mu_j)^2 / (2 std_j^2) - log_std_j - log sqrt(2 pi)) is
 *   DiagGaussianDistribution.log_prob.  It depends on (seed, car index, step) alone, never on the shard, tile or lane
 *   that computes it; the two salts are used by no other action source.
 * The draw of car n at (seed, step) of a categorical actor (output 6) with logits l_0 .. l_4: torch.multinomial cannot be
 *   restated bit for bit, so it is an inverse CDF on one uniform of the same counter key, float32 throughout:
 *     u = (mix32(key ^ 0x4341545F44524157) >> 8) * 2^-24  in [0, 1)         (CAT_SALT, used by no other source)
 *     m = max_j l_j (fmaxf, index order),  e_j = expf(l_j - m),  P_0 = e_0,  P_j = P_{j-1} + e_j,  S = P_4,  t = u * S
 *     a = the number of j in 0..3 with t >= P_j     (category 4 is the fall-through: nothing is compared with P_4)
 *     logp = (l_a - m) - logf(S)                    Categorical(logits = l).log_prob(a)
 *   a is the recorded action, its pair (above) steps the env: bit-identical to nascar_step(discrete = 1) on a.  It
 *   depends on (seed, car index, step) alone.
 * nascar_collect: `steps` x (policy 6 on the current obs + CarEnv.step with auto-reset) as policy 6 of the sharded
 *   rollout, always with the per-step records and the obs trajectory of nascar_rollout (obs [steps + 1][E*C*38], record 0
 *   the current observation on entry; reward, car_flags [steps][E*C]; env_flags [steps][E]; none may be NULL), plus
 *     actions [steps][E*C][2], logp [steps][E*C]   the draws above (actions and obs 8-byte aligned).  With a categorical
 *                                                  actor `actions` points at int32 [steps][E*C], the action index a:
 *                                                  the parameter keeps its declared type and callers cast (4-byte
 *                                                  alignment suffices); nascar_collect_normalized likewise
 *     values [steps + 1][E*C]                      the critic on obs record k
 *     timeout_values [steps][E*C]                  the critic on the TERMINAL observation of step k for the cars of envs
 *                                                  that were truncated and not terminated there, 0 everywhere else: SB3
 *                                                  bootstraps a time limit with reward += gamma * V(terminal_observation)
 *   Identical results to `steps` calls of nascar_policy_actions(6, seed, step0 + k) + nascar_step(auto_reset).  Every car
 *   slot runs the one actor-critic; actor and critic ride in one launch when they share (h1, h2, activation).  Fails
 *   with rollout streams 0, under nascar_set_rollout_pipe, with fitness accumulation on and without an actor-critic;
 *   nascar_step_driven and nascar_rollout refuse policy 6.  Random-track mode and envs that do not sit in one track's
 *   workgroups in order run as one shard, as policy 4 does.
 * nascar_gae: generalised advantage estimation over `steps` records of any device buffers of the handle's E x C shape
 *   (reward, timeout_values, adv, ret [steps][E*C]; values [steps + 1][E*C]; env_flags [steps][E]), float32 throughout in
 *   the operation order of RolloutBuffer.compute_returns_and_advantage under NumPy 2 promotion:
 *     r' = reward + g * timeout_value,  g = (float)gamma;   nnt = 1 - (terminated | truncated of the car's env at step k)
 *     delta = (r' + (g * V[k+1]) * nnt) - V[k];   A[k] = delta + ((float)(gamma * lambda) * nnt) * A[k+1],  A[steps] = 0
 *     ret[k] = A[k] + V[k]
 *   reproducible bit for bit (no fused multiply-adds). */
int nascar_set_actor_critic(NascarHandle* h, int32_t pi_id, int32_t vf_id, const float* log_std);
int nascar_collect(NascarHandle* h, uint64_t seed, int64_t step0, int32_t steps, float* obs, float* reward,
                   uint8_t* car_flags, uint8_t* env_flags, float* actions, float* logp, float* values, float* timeout_values,
                   void* stream);
int nascar_gae(NascarHandle* h, const float* reward, const float* values, const float* timeout_values,
               const uint8_t* env_flags, int32_t steps, double gamma, double lambda, float* adv, float* ret, void* stream);

/* Running normalisation: Stable-Baselines3's VecNormalize (common/vec_env/vec_normalize.py, common/running_mean_std.py
 * of SB3 2.7.0), which the reference wraps its A2C training envs in (learn/a2c.py:94-100: norm_obs, norm_reward,
 * clip_obs = 1.0, gamma = 0.99) and which usually accompanies SB3's PPO, on the device.  Every car slot is one of SB3's
 * envs: a batch is the N = E * C rows of a step, disabled cars' rows included, and an env's done flag applies to the
 * returns of all its cars.
 * Statistics (float64, on the device, outside the state arena: nascar_get_state / nascar_set_state do not carry them, as
 * they do not carry the random-track map): obs_mean [38], obs_var [38], obs_count, ret_mean, ret_var, ret_count -- 80
 * doubles in this order, the `stats` record below -- and returns [N].  Fresh: mean 0, var 1, count 1e-4, returns 0.
 * RunningMeanStd.update(batch), every expression left to right in float64:
 *     bm, bv = batch mean and population variance per column, bc = N
 *     delta = bm - mean;  tot = count + bc;  new_mean = mean + delta * bc / tot
 *     m2 = var * count + bv * bc + delta^2 * count * bc / (count + bc);  new_var = m2 / (count + bc);  new_count = bc + count
 *   ONE DEVIATION: the batch moments are taken in float64 over the float32 rows (SB3 lets NumPy accumulate them in
 *   float32; this is the quantity that approximates).  Each workgroup of 256 rows (a rule of N alone) takes its mean and
 *   its sum of squares about that mean; the workgroups' (count, mean, M2) are merged in workgroup order.  No atomics:
 *   the statistics are the same bits from run to run and whatever the rollout streams.
 * normalize_obs(x) = (float)clip(((double)x - mean) / sqrt(var + epsilon), -clip_obs, clip_obs), normalize_reward(r) =
 *   (float)clip((double)r / sqrt(ret_var + epsilon), -clip_reward, clip_reward): a float64 subtract, divide, clip, one cast.
 * nascar_set_normalize: cfg NULL switches normalisation off (the statistics are kept until it is switched on again,
 *   which starts from fresh ones); otherwise the settings, which may change while it is on (training = 0 freezes the
 *   statistics).  clip_obs, clip_reward and epsilon must be finite and positive, gamma finite and >= 0.  Synchronises
 *   `stream` when it switches on.  nascar_get_normalize returns 1 / 0 for on / off and the settings.
 * nascar_get_norm_stats: the statistics into device buffers stats [80] and returns [N] (either may be NULL).
 * nascar_set_norm_stats: host arrays stats [80] and returns [N] (NULL: kept); every entry finite, no negative variance,
 *   both counts positive.  Synchronises `stream`.
 * nascar_normalize_reset: VecNormalize.reset on the observation a full nascar_reset wrote: returns = 0, the obs update
 *   when training, obs_out = normalize_obs(obs_raw).
 * nascar_normalize_step: VecNormalize.step_wait on one step's outputs, in SB3's order: the obs update (training and
 *   norm_obs), obs_out = normalize_obs(obs_raw), returns = returns * gamma + reward and the returns update (training and
 *   norm_reward), reward_out = normalize_reward(reward_raw), term_out = normalize_obs(term_obs) for the cars of done envs
 *   (terminated | truncated in env_flags) under the statistics as they now stand -- other rows of term_out are left as
 *   they are, term_obs / term_out NULL: none, and they may be one buffer -- and returns = 0 for the cars of done envs
 *   last.  obs_raw holds the reset observation of auto-reset envs: SB3 includes it in the update, and so does this.
 *   A flag that is off copies its input.  obs_raw 8-byte aligned; all buffers device pointers, [N][38] / [N] / [E].
 * nascar_collect_normalized: nascar_collect under normalisation.  obs_raw [N][38] is the engine's raw observation, in /
 *   out (the step and random-track mode read and write it; it stays raw); obs record 0 holds the NORMALISED current
 *   observation on entry (what nascar_normalize_reset / _step wrote) and record k + 1 the normalised one after step k;
 *   the actor samples on and the critic values record k; reward [steps][N] takes the normalised rewards and raw_reward
 *   [steps][N] the raw ones; timeout_values are V of the normalised terminal observation under the statistics after step
 *   k's update.  Identical, bit for bit and in the final statistics, to `steps` x (nascar_policy_actions(6) on the
 *   normalised observation + nascar_step(auto_reset, terminal_obs) + nascar_normalize_step).  While the statistics are
 *   updated (training with either flag) step k + 1 needs every env's step-k observation: the call runs as one shard;
 *   with frozen statistics the work is row-local and the shards run on unsynchronised.  Either way the results do not
 *   depend on the rollout streams.  Refusals as nascar_collect's (rollout streams 0 and the pipelined rollout among them).
 * While normalisation is on, nascar_collect (use nascar_collect_normalized) and nascar_collect_transitions (off-policy
 *   normalisation happens at sample time and is not provided) fail. */
typedef struct NascarNormalize {
    int32_t norm_obs, norm_reward, training;
    int32_t pad_;
    double clip_obs, clip_reward, gamma, epsilon;
} NascarNormalize;
int nascar_set_normalize(NascarHandle* h, const NascarNormalize* cfg, void* stream);
int nascar_get_normalize(NascarHandle* h, NascarNormalize* cfg);
int nascar_get_norm_stats(NascarHandle* h, double* stats, double* returns, void* stream);
int nascar_set_norm_stats(NascarHandle* h, const double* stats, const double* returns, void* stream);
int nascar_normalize_reset(NascarHandle* h, const float* obs_raw, float* obs_out, void* stream);
int nascar_normalize_step(NascarHandle* h, const float* obs_raw, const float* reward_raw, const uint8_t* env_flags,
                          const float* term_obs, float* obs_out, float* reward_out, float* term_out, void* stream);
int nascar_collect_normalized(NascarHandle* h, uint64_t seed, int64_t step0, int32_t steps, float* obs_raw, float* obs,
                              float* reward, float* raw_reward, uint8_t* car_flags, uint8_t* env_flags, float* actions,
                              float* logp, float* values, float* timeout_values, void* stream);

/* Off-policy collection: the loop of SB3's off-policy algorithms, as learn/sac.py, learn/td3.py, learn/td3_n.py and
 * learn/ddpg.py run it (OffPolicyAlgorithm.collect_rollouts, off_policy_algorithm.py: _sample_action, env.step,
 * _store_transition -> ReplayBuffer.add, then ReplayBuffer.sample for the learner), on the device.
 * With scale(u) = 2 * ((u + 1) / 2) - 1 (BasePolicy.scale_action: what the replay buffer keeps, SB3's buffer_action) and
 * unscale(a) = -1 + (0.5 * (a + 1)) * 2 (unscale_action: what steps the env), both float32 for the Box(-1, 1):
 * Controller output 5 (act_dim 4): SB3's SAC Actor with deterministic = False (sac/policies.py Actor.forward /
 *   action_log_prob, SquashedDiagGaussianDistribution).  w3 is [4][h2], rows 0-1 actor.mu.weight, rows 2-3
 *   actor.log_std.weight, b3 [4] likewise.  Per car in float32: mu_j = W3[j].h + b3[j], ls_j = min(max(W3[2 + j].h +
 *   b3[2 + j], -20), 2) (LOG_STD_MIN / LOG_STD_MAX), g_j = mu_j + expf(ls_j) * eps_j, t_j = tanhf(g_j); the env is stepped
 *   with u_j = unscale(t_j) and the replay keeps s_j = scale(u_j).  It runs as the explorer only (the field,
 *   nascar_controller_forward and nascar_set_actor_critic refuse it); nascar_update_controller takes new weights.
 * Exploration noise on a deterministic actor (TD3 / DDPG with NormalActionNoise, _sample_action; the reference uses
 *   sigma 0.15 in learn/ddpg.py:93 and 0.75 in learn/td3_n.py:94): an output-2 controller with sigma [2]:
 *   s_j = min(max(scale(u_det_j) + sigma_j * eps_j, -1), 1), the env is stepped with unscale(s_j), the replay keeps s_j.
 *   sigma = 0 reproduces the controller's output-2 action bit for bit.
 * eps is the Box-Muller pair of nascar_collect's draw (same formula, same counter key of (seed, car, step)) with the salts
 *   0x4F46465F504F4C31 (u0) and 0x7F4A7C15D1B54A33 (u1), used by no other action source: it depends on (seed, car index,
 *   step) alone, never on the shard, tile or lane that computes it.
 * nascar_set_explorer: policy 7 of nascar_policy_actions (which returns u, the action that steps the env; actions 8-byte
 *   aligned) and source 7 of nascar_collect_transitions.  id: an output-5 controller (sigma must be NULL) or an output-2
 *   controller with sigma [2] (host, finite, >= 0; NULL = zeros); id < 0 clears it.  nascar_step_driven and nascar_rollout
 *   refuse policy 7 (use nascar_collect_transitions).
 * NascarReplay: caller-owned device buffers, `capacity` step slots of N = E * C cars: 319 bytes per transition (2 x 152
 *   obs, 8 action, 4 reward, 3 flag bytes), i.e. 319 * N bytes per step slot.  obs, next_obs and actions 8-byte aligned.
 * nascar_collect_transitions: `steps` x (source on the current obs + CarEnv.step with auto-reset) on the sharded rollout,
 *   no host synchronisation; step k writes slot (pos + k) % capacity (a call may wrap the ring any number of times):
 *     obs       the observation the action was computed on
 *     actions   s, the scaled buffer action
 *     reward    the step's reward
 *     done      terminated | truncated of the car's env
 *     timeout   truncated & !terminated (TimeLimit.truncated under handle_timeout_termination)
 *     next_obs  the terminal observation for the cars of done envs, else the new observation (_store_transition)
 *     live      1 unless the car was already disabled before the step (car flag bit 0 without bit 1): a learner masks
 *               dead cars with it (the reference trains at 1 car, where it is always 1)
 *   source: 7 the explorer, or 0 the uniform policy (SB3's learning_starts warm-up, action_space.sample(): policy 0's
 *   draw u, stored as scale(u)).  obs [N][38] is in/out (8-byte aligned): the current observation on entry, the last
 *   step's on return; pos in [0, capacity).  Identical, bit for bit, to `steps` x (nascar_policy_actions(source) +
 *   nascar_step(auto_reset, terminal_obs)) with the buffer assembled on the host.  Each shard writes its own cars' rows
 *   after its sensor launch (one small kernel; no batch-wide staging copy beyond nascar_collect's terminal observations).
 *   Fails with rollout streams 0, under nascar_set_rollout_pipe and with fitness accumulation on, as nascar_collect does;
 *   random-track mode and envs that do not sit in one track's workgroups in order run as one shard.
 * nascar_replay_sample: ReplayBuffer.sample (buffers.py _get_samples) as one launch, uniform over `size` filled step
 *   slots x N cars.  Sample i of (seed, draw): key = the counter key of (seed, car = i, step = draw),
 *     slot = ((uint64)mix32(key ^ 0x5245504C5F534C54) * size) >> 32,  car = ((uint64)mix32(key ^ 0x2545F4914F6CDD1D) * N) >> 32
 *   gathered into contiguous outputs obs / next_obs [batch][38], actions [batch][2], reward [batch], done [batch] float32 =
 *   done * (1 - timeout) (what SB3 hands the learner), live [batch] uint8.  batch = 0 launches nothing; size < 1,
 *   size > capacity and batch < 0 are errors.  obs / next_obs / actions outputs 8-byte aligned. */
typedef struct NascarReplay {
    float *obs, *next_obs;            /* [capacity][N][38] */
    float *actions;                   /* [capacity][N][2]   the scaled buffer action s */
    float *reward;                    /* [capacity][N] */
    uint8_t *done, *timeout, *live;   /* [capacity][N] */
    int32_t capacity;
} NascarReplay;
int nascar_set_explorer(NascarHandle* h, int32_t id, const float* sigma);
int nascar_collect_transitions(NascarHandle* h, int32_t source, uint64_t seed, int64_t step0, int32_t steps, float* obs,
                               const NascarReplay* replay, int32_t pos, void* stream);
int nascar_replay_sample(NascarHandle* h, const NascarReplay* replay, int32_t size, uint64_t seed, int64_t draw,
                         int32_t batch, float* obs, float* next_obs, float* actions, float* reward, float* done,
                         uint8_t* live, void* stream);

/* Genome drivers: the rule driver of the reference's genetic trainer (game/control/genetic_controller.py,
 * learn/genetic_trainer.py), one genome per car.  GeneticController.control cannot run as written (its line 81 reads an
 * attribute that is defined nowhere, and the trainer turns the exception into fitness -1000), so the semantics are those
 * of the class's docstring -- BaseController._fallback_control (game/control/base_controller.py:64-103) with its
 * constants replaced by genes, i.e. control() without lines 81-82:
 *   if last_forward >= forward: speed_limit = forward * g[10]      if last_forward < forward: speed_limit = 1.0
 *   if speed < speed_limit * g[0]: tb += g[2]                      if speed > speed_limit * g[1]: tb -= g[3]
 *   if r > l: steering = (1 - l/r) * g[4]   elif l > r: steering = ((1 - r/l) * -1) * g[4]   else: steering *= g[6]
 *   if abs(steering) > g[7]: tb *= g[5];    both clamped to [-1, 1];    last_forward = forward
 * in the order of GeneticController.default_genome; g[8], g[9] and g[11] are carried and unused (only the omitted lines
 * read 8 and 9, nothing reads 11).  NumPy 2 promotion: g[0], g[1], g[4], g[6], g[7], g[10] meet float32 values and are
 * rounded to float32 first; g[2], g[3], g[5] meet throttle_brake, a Python float, and stay float64.  A steering that
 * the clamp saturated is the Python int +-1, and stays a float64 Python number through the exact left / right ties that
 * follow it; the table keeps that flag per car.  The genome (0.95, 1.05, 0.1, 0.1, 1, 0.5, 0.9, 0.25, 1, 1, 1, 0.3)
 * reproduces policy 1 bit for bit.
 * nascar_set_genomes: genomes is a host array [E*C][12] float64 (NULL clears the table), copied to a device table
 *   outside the state arena (nascar_state_bytes and the snapshot do not change) by an upload ordered on `stream`; every
 *   gene must be finite.  A new table is a new set of controllers: it also zeroes every car's control state (the state
 *   the rule sources share, as GeneticController.__init__ starts from a zero control_state) and the per-car
 *   Python-number flags. */
int nascar_set_genomes(NascarHandle* h, const double* genomes, void* stream);

/* On-device fitness accumulators: what the trainer's evaluation loop gathers per individual from rewards[i] and
 * info['cars'][i] after every step (learn/genetic_trainer.py:253-285), in float64.
 * nascar_set_fitness: enable != 0 allocates (first time) and zeroes the per-car accumulators and a per-env "ended"
 *   byte, on `stream`; 0 stops the accumulation.  While enabled, every step of nascar_step / nascar_step_driven and of the
 *   sharded nascar_rollout enqueues fitness_kernel after its sensor launch (per shard in the rollout).  For an env that
 *   has not ended, per car: total_reward += (double)reward; max_speed = max(max_speed, speed) with the speed of
 *   nascar_get_info; distance += speed * (1.0 / 60.0); time_on_track += 1.0 / 60.0 when on track; steps += 1;
 *   lap_completed and lap_time = last_lap_time at the first step with lap_count > 0 (the trainer's own lap-time lines
 *   leave it None for ever; this is their evident intent); disabled_at_step = steps at the first step that left the car
 *   disabled.  The step whose env flags carry terminated or truncated is included, then the env's cars stop
 *   accumulating.  Needs auto_reset = 0 (CarEnv.step keeps stepping a finished env, and so does this engine); steps
 *   with auto_reset, the fused and the pipelined rollout and random-track mode fail while it is on.  Off by default.
 * nascar_get_fitness: out is a device buffer [E*C][8] float64: total_reward, distance_traveled, max_speed,
 *   time_on_track, lap_completed, lap_time (NaN: none), steps, disabled_at_step (-1: never). */
int nascar_set_fitness(NascarHandle* h, int32_t enable, void* stream);
int nascar_get_fitness(NascarHandle* h, double* out, void* stream);

/* Race modes: what game/competition.py:239-424, game/time_trial.py:222-420 and the stages of game/championship.py:264-607
 * keep per car while they step a field, as a per-step ledger kernel (race_step_kernel, enqueued where fitness_kernel is),
 * and their finishing order and points (competition.py:37-81, championship.py:28-29, 65-120).  Lap times and
 * simulation_time are float64 (Python floats); the per-car reward is a float32 running sum in step order
 * (car_rewards[i] = 0.0; car_rewards[i] += reward[i] is np.float32 from the first add under NumPy 2).
 * NascarRace.mode: 0 off, 1 competition, 2 time trial; laps_per_attempt (>= 1) is the time trial's LAPS_PER_ATTEMPT.
 * Per step, for an env that has not ended, for every car: total_reward += reward, steps += 1.  Then, for every car
 * (mode 2: every car that is not parked): lap_count and disabled are taken from the car's info; if lap_count >
 * prev_lap_count: with a truthy last_lap_time (not None, not 0.0) last_lap = it, laps_timed += 1, attempt_laps += 1,
 * finish_time = simulation_time (overwritten on every lap), best_lap = it where there is none or it is lower, and the env's
 * fastest lap and fastest_car become this car's where there is none or it is strictly lower (cars in index order, so the
 * first car in (step, car) order to reach the minimum keeps it); then prev_lap_count = lap_count either way.
 * Mode 1: the env ends after the step whose env flags carry terminated or truncated (that step is counted).
 * Mode 2: a car with attempt_laps >= laps_per_attempt, and then every disabled car, is parked; the env's flags are
 *   ignored and the env ends after the step that parked its last car.  A parked car's lap_count and disabled stay what
 *   they were at the step that parked it.  Parking acts on action buffers: for nascar_rollout policies 2, 4 and 5 and for
 *   nascar_policy_actions (policies 0 to 5; 6 and 7, the learners' sampling sources, are not masked), a car whose parked field was set by an earlier step takes action (0, 0) and
 *   its controller is not run -- a rule, noisy or genome source skips the car, whose control state stays what it was
 *   when it parked, and an MLP source's row is overwritten.  Policies 0, 1 and 3 of nascar_rollout and
 *   nascar_step_driven run inside the step launch and fail in mode 2.
 * nascar_reset does not touch the rule / genome sources' control state (only nascar_set_genomes and nascar_set_state
 *   write it): a time trial's attempts carry it over a reset, and the caller resets the envs between attempts.
 * nascar_set_race: allocates (first time) and initialises the ledger on `stream`; NULL or mode 0 switches it off (the
 *   ledger stays readable).  Switching modes keeps the ledger: call nascar_race_begin.  While on, every step of
 *   nascar_step / nascar_step_driven and of the sharded nascar_rollout enqueues race_step_kernel after its sensor launch
 *   (per shard in the rollout).  Like the fitness accumulators it needs auto_reset = 0 and fails in the fused and the
 *   pipelined rollout, in random-track mode and under nascar_collect / nascar_collect_transitions; both may be on.
 * nascar_race_begin: a new race or attempt: zeroes lap_count, attempt_laps, prev_lap_count, total_reward, disabled,
 *   parked, steps and the ended bytes and clears last_lap and finish_time; keep_records != 0 keeps best_lap, laps_timed
 *   and the env's fastest lap and its car (the time trial across attempts), 0 clears them too.
 * nascar_get_race (device buffers, any may be NULL): ledger [E*C][10] float64: lap_count, laps_timed, attempt_laps,
 *   best_lap (NaN: none), last_lap (NaN: none), finish_time (NaN: none), total_reward (the float32 sum, widened),
 *   disabled, parked, steps; fastest_car [E] int32 (-1: none); ended [E] uint8.
 * nascar_race_rank (device buffers): order [n_env][n_cars] (the car at position p), position and points [n_env][n_cars]
 *   int32 (any may be NULL) of the handle's own ledger (ledger NULL; n_env, n_cars must be the handle's) or of caller
 *   buffers in nascar_get_race's layout (fastest_car may be NULL: no bonus); n_cars <= 64.  mode 1: Python's stable sorted() by
 *   (-lap_count, finish_time or 999999, best_lap or 999999, -total_reward, disabled) -- `x or 999999` maps None and 0.0
 *   -- then COMPETITION_POINTS[-(min(p, 9) + 1)] of [0, 1, 2, 3, 5, 8, 13, 21, 24, 45] and +15 for fastest_car.
 *   mode 2: stable by best_lap or 999999, then [15, 7, 3] for positions 0-2 that have a best lap. */
typedef struct NascarRace { int32_t mode; int32_t laps_per_attempt; } NascarRace;
int nascar_set_race(NascarHandle* h, const NascarRace* race, void* stream);
int nascar_race_begin(NascarHandle* h, int32_t keep_records, void* stream);
int nascar_get_race(NascarHandle* h, double* ledger, int32_t* fastest_car, uint8_t* ended, void* stream);
int nascar_race_rank(NascarHandle* h, const double* ledger, const int32_t* fastest_car, int32_t n_env, int32_t n_cars,
                     int32_t mode, int32_t* order, int32_t* position, int32_t* points, void* stream);

/* Test hook: the device re-implementation of glibc sinf/cosf used for b2Rot::Set
 * (device pointers, n floats).  Parity tests compare it with the host libm. */
int nascar_debug_sincosf(const float* x, float* s, float* c, int32_t n, void* stream);

/* Test hook: the float64 library functions of the vehicle model, as the step kernels' build compiles them (device
 * pointers, n doubles).  fn 0: exp(-2 x); 1: atan2(|x|, y); 2: tan(x); 3: sqrt(x*x + y*y) as the model writes Python's
 * (x**2 + y**2) ** 0.5; 4: x*x as it writes x ** 2.  y may be null for fn 0, 2 and 4. */
int nascar_debug_f64math(const double* x, const double* y, double* out, int32_t n, int32_t fn, void* stream);

/* Test hooks: the Box2D step's primitives on caller-given cases, one lane per case (device pointers).
 * nascar_debug_toi: b2TimeOfImpact of a car sweep against a static wall box and the exact TOI cull's decision on the
 *   same pair.  cases [n][12] float32: c0.x c0.y c.x c.y a0 a alpha0 | wall x y angle hx hy.  beta [n] float32 and
 *   state [n] int32 are b2TOIOutput's t and state (1 failed, 2 overlapped, 3 touching, 4 separated); far [n] int32 is
 *   1 where the step would skip the call.
 * nascar_debug_collide: b2CollidePolygons of the car box at a pose against a wall box.  cases [n][8] float32:
 *   x y angle | wall x y angle hx hy.  out [n][12] 32-bit words: word 0 = stage | point count << 2 | type << 4
 *   (stage 0: only the point count was written, 1: + type, 2: + everything else), then local normal x y, local point
 *   x y, point 0 x y id, point 1 x y id, 0. */
int nascar_debug_toi(const float* cases, int32_t n, float* beta, int32_t* state, int32_t* far, void* stream);
int nascar_debug_collide(const float* cases, int32_t n, float* out, void* stream);

/* Test hook: the car-car contact solver of nascar_set_car_contact alone, on caller-given bodies (device pointers, no
 * engine state), in the step's lane layout: lane el * num_cars + car, 128 / num_cars envs per 128-lane workgroup, the
 * env's car-0 lane solving it with the step's own function.  bodies [num_envs * num_cars][7] float32: x y qs qc vx vy w
 * (body centre, the rotation's sine and cosine, linear and angular velocity).  out [num_envs * num_cars][4] float32:
 * vx vy w after the solve and the car's largest accumulated normal impulse, before the step's write-back rule (above).
 * env_out [num_envs][2] int32: touching pairs solved, touching pairs dropped at the cap of num_cars.
 * num_cars in [1, 64]; with 1 car nothing is solved. */
int nascar_debug_car_contact(const float* bodies, int32_t num_envs, int32_t num_cars, float* out, int32_t* env_out,
                             void* stream);

/* Test hook: sensors only.  poses: device float32 [E*C*3] (x, y, angle) per car, written into the sensor
 * hand-off; impl 1 = beam-list ray kernel (the step's default), 0 = wall-group kernel; writes the 16
 * DistanceSensor values obs[n*38 + 22 .. 37] (src/distance_sensor.py:71-117, src/car_env.py:946). */
int nascar_debug_sensors(NascarHandle* h, const float* poses, float* obs, int32_t impl, void* stream);

/* Test hook: the workgroup layout the next launch uses (block map; prepare()d first) copied into caller device buffers,
 * blk_track [cap_blocks] and blk_env [cap_blocks * envs per workgroup] int32; returns the number of workgroups launched
 * (random-track mode: those past the last track's are empty, track -1), or < 0 on error. */
int nascar_debug_block_map(NascarHandle* h, int32_t* blk_track, int32_t* blk_env, int32_t cap_blocks, void* stream);

#ifdef __cplusplus
}
#endif
#endif
