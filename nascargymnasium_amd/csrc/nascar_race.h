// Race modes on the device (nascar_set_race): the per-step ledger of game/competition.py:239-424 and
// game/time_trial.py:222-420 (as game/championship.py:264-607 runs them per stage) and their finishing order and points
// (competition.py:37-81, championship.py:65-120).  Included by nascar_kernels.hip after info_core / fitness_kernel.
#pragma once

// The ledger is SoA [RL_N][N] float64 (a wave's lanes touch contiguous lines).  The first RACE_N fields are the rows of
// nascar_get_race, in its order; RL_PREV is the reference's previous_lap_count.  best_lap / finish_time hold NaN for
// Python's None.  total_reward holds a float32 value: car_rewards[i] becomes np.float32 at its first += (NumPy 2
// promotion: python float + np.float32 is float32), so the sum is rounded to float32 after every step.
enum { RACE_LAP_COUNT, RACE_LAPS_TIMED, RACE_ATTEMPT_LAPS, RACE_BEST_LAP, RACE_LAST_LAP, RACE_FINISH_TIME, RACE_REWARD,
       RACE_DISABLED, RACE_PARKED, RACE_STEPS, RACE_N, RL_PREV = RACE_N, RL_N };
enum { RACE_OFF = 0, RACE_COMPETITION = 1, RACE_TIME_TRIAL = 2 };
// per env: the overall best lap (NaN: none) and its car (-1), and the ended byte -- competition: after the step whose env
// flags carry terminated or truncated; time trial: after the step that parked the env's last car
struct RaceEnv { double* fastest; int32_t* fastest_car; uint8_t* ended; };

// Python truthiness of an Optional[float]: None (NaN here) and 0.0 are false
__device__ __forceinline__ bool race_truthy(double x) { return x == x && x != 0.0; }

// nascar_race_begin: a new race or attempt.  keep != 0 keeps best lap, total timed laps and the env's fastest lap, as the
// time trial keeps best_lap_times / all_lap_times / overall_best_lap_time across attempts (time_trial.py:223-232, 246-263)
__global__ void __launch_bounds__(256) race_begin_kernel(int N, int E, int keep, double* led, RaceEnv V) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const size_t S = (size_t)N;
  led[RACE_LAP_COUNT * S + n] = 0.0; led[RACE_ATTEMPT_LAPS * S + n] = 0.0; led[RACE_LAST_LAP * S + n] = NAN;
  led[RACE_FINISH_TIME * S + n] = NAN; led[RACE_REWARD * S + n] = 0.0; led[RACE_DISABLED * S + n] = 0.0;
  led[RACE_PARKED * S + n] = 0.0; led[RACE_STEPS * S + n] = 0.0; led[RL_PREV * S + n] = 0.0;
  if (!keep) { led[RACE_LAPS_TIMED * S + n] = 0.0; led[RACE_BEST_LAP * S + n] = NAN; }
  if (n < E) {
    V.ended[n] = 0;
    if (!keep) { V.fastest[n] = NAN; V.fastest_car[n] = -1; }
  }
}

// One step of the ledger for the env slots [slot0, slot0 + nslot) of the block map (a shard's, or all), after their
// sensor launch.  Laid out as fitness_kernel: one lane per car, 256 / C whole envs per block, so the env-level fields
// (fastest lap, ended) are decided inside the block: every lane publishes its step's timed lap in LDS, and after the
// barrier the env's car-0 lane walks the env's C entries in car order with a strict <, which is the reference's
// "if overall_best is None or last < overall_best" over cars in index order (competition.py:381, championship.py:555-557);
// an earlier step's holder keeps the lap on a tie for the same reason.  The ended byte is read by every lane before the
// barrier and written after it.
__global__ void __launch_bounds__(256) race_step_kernel(Params P, int slot0, int nslot, int mode, int laps_per_attempt,
                                                        const float* reward, const uint8_t* env_flags, double* led,
                                                        RaceEnv V) {
  __shared__ double s_lap[256];
  __shared__ uint8_t s_parked[256];
  const int C = P.C, epw = 256 / C;
  const int el = threadIdx.x / C, car = threadIdx.x - el * C, sl = blockIdx.x * epw + el;
  int env = -1, b = 0;
  if (el < epw && sl < nslot) {
    b = (slot0 + sl) / P.epb;
    if (!blk_empty(P, b)) env = blk_env_of(P, 0, slot0 + sl);
  }
  const bool live = env >= 0 && !V.ended[env];
  double lap = NAN;      // this step's timed lap of this car
  bool parked = true;
  if (live) {
    const TrackDev T = P.tracks[blk_track_of(P, b)];
    const WallSet S{T.walls, T.nwall, T.bp, T.sn, T.wfat};
    const int n = env * C + car;
    const size_t N = (size_t)P.N;
    Car c;
    car_load(P, n, c);
    const InfoCore ic = info_core(S, c);
    // car_rewards[i] += reward[i]: every car, disabled and parked ones included (competition.py:319-321, time_trial.py:304-306)
    led[RACE_REWARD * N + n] = (double)((float)led[RACE_REWARD * N + n] + reward[n]);
    led[RACE_STEPS * N + n] += 1.0;
    parked = led[RACE_PARKED * N + n] != 0.0;
    // the time trial skips the lap loop for cars_finished_attempt (time_trial.py:316-318); the competition has no such set
    if (mode == RACE_COMPETITION || !parked) {
      led[RACE_LAP_COUNT * N + n] = (double)ic.laps;
      led[RACE_DISABLED * N + n] = (double)ic.disabled;
      if ((double)ic.laps > led[RL_PREV * N + n]) {
        if (race_truthy(ic.last_lap)) {
          lap = ic.last_lap;
          led[RACE_LAST_LAP * N + n] = lap;
          led[RACE_LAPS_TIMED * N + n] += 1.0;
          const double al = led[RACE_ATTEMPT_LAPS * N + n] + 1.0;
          led[RACE_ATTEMPT_LAPS * N + n] = al;
          led[RACE_FINISH_TIME * N + n] = P.env_time[env];
          const double best = led[RACE_BEST_LAP * N + n];
          if (!(best == best) || lap < best) led[RACE_BEST_LAP * N + n] = lap;
          if (mode == RACE_TIME_TRIAL && al >= (double)laps_per_attempt) parked = true;
        }
        led[RL_PREV * N + n] = (double)ic.laps;
      }
      // "for car_idx in env.disabled_cars: cars_finished_attempt.add" after the lap loop (time_trial.py:371-373)
      if (mode == RACE_TIME_TRIAL && ic.disabled) parked = true;
      if (mode == RACE_TIME_TRIAL && parked) led[RACE_PARKED * N + n] = 1.0;
    }
  }
  s_lap[threadIdx.x] = lap;
  s_parked[threadIdx.x] = parked;
  __syncthreads();
  if (live && car == 0) {
    double fast = V.fastest[env];
    int who = V.fastest_car[env];
    bool all_parked = true, changed = false;
    for (int j = 0; j < C; ++j) {
      const double t = s_lap[threadIdx.x + j];
      if (t == t && (!(fast == fast) || t < fast)) { fast = t; who = j; changed = true; }
      all_parked = all_parked && s_parked[threadIdx.x + j];
    }
    if (changed) { V.fastest[env] = fast; V.fastest_car[env] = who; }
    const bool end = mode == RACE_TIME_TRIAL ? all_parked : (env_flags[env] & (EF_TERMINATED | EF_TRUNCATED)) != 0;
    if (end) V.ended[env] = 1;
  }
}

// nascar_get_race: the ledger as [N][RACE_N] rows
__global__ void __launch_bounds__(256) race_read_kernel(int N, const double* led, double* out) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  for (int f = 0; f < RACE_N; ++f) out[(size_t)n * RACE_N + f] = led[(size_t)f * N + n];
}

// The time trial's parking for the action sources that write a whole row per car (the MLP launches): cars [n0, n1) whose
// parked field is set take the action (0, 0) (time_trial.py:278-280).  The built-in and genome kernels apply the same
// test themselves, before they touch the car's control state.
__global__ void __launch_bounds__(256) race_park_kernel(int n0, int n1, const double* parked, float* act) {
  const int n = n0 + blockIdx.x * 256 + threadIdx.x;
  if (n >= n1) return;
  if (parked[n] != 0.0) { act[2 * n] = 0.0f; act[2 * n + 1] = 0.0f; }
}

// Finishing order and points of n_env envs of C cars: one lane per car, 256 / C envs per block, the env's sort keys in
// LDS, rank by counting -- position[i] = #{ j : key_j < key_i, or key_j == key_i and j < i }, which is the order of
// Python's stable sorted() on the key tuples with no data-dependent loop.  Competition keys (competition.py:68-76):
// (-laps, finish_time or 999999, best or 999999, -reward, disabled); time trial (championship.py:68): best or 999999.
// All keys are numbers, compared in float64 as Python compares an int with a float.  Field f of car n is at
// led[n * sn + f * sf]: the handle's SoA ledger (sn 1, sf N) or nascar_get_race rows (sn RACE_N, sf 1).
// Points (championship.py:28-29, 65-120): competition COMPETITION_POINTS[-(min(p, 9) + 1)] and FASTEST_LAP_BONUS for the
// env's fastest_car; time trial TIME_TRIAL_POINTS[p] for p < 3 with a best lap.
#define RACE_KEYS 5
__device__ __forceinline__ bool race_key_less(const double* a, const double* b, int ia, int ib) {
#pragma unroll
  for (int k = 0; k < RACE_KEYS; ++k) {
    if (a[k] < b[k]) return true;
    if (a[k] > b[k]) return false;
  }
  return ia < ib;
}
__global__ void __launch_bounds__(256) race_rank_kernel(int n_env, int C, int mode, const double* led, size_t sn, size_t sf,
                                                        const int32_t* fastest_car, int32_t* order, int32_t* position,
                                                        int32_t* points) {
  __shared__ double s_key[256][RACE_KEYS];
  const int epw = 256 / C;
  const int el = threadIdx.x / C, car = threadIdx.x - el * C, env = blockIdx.x * epw + el;
  const bool on = el < epw && env < n_env;
  bool has_best = false;
  if (on) {
    const size_t n = (size_t)env * C + car;
    const double best = led[n * sn + RACE_BEST_LAP * sf];
    has_best = race_truthy(best);
    double* k = s_key[threadIdx.x];
    if (mode == RACE_COMPETITION) {
      const double fin = led[n * sn + RACE_FINISH_TIME * sf];
      k[0] = -led[n * sn + RACE_LAP_COUNT * sf];
      k[1] = race_truthy(fin) ? fin : 999999.0;
      k[2] = has_best ? best : 999999.0;
      k[3] = -led[n * sn + RACE_REWARD * sf];
      k[4] = led[n * sn + RACE_DISABLED * sf] != 0.0 ? 1.0 : 0.0;
    } else {
      k[0] = has_best ? best : 999999.0;
      k[1] = k[2] = k[3] = k[4] = 0.0;
    }
  }
  __syncthreads();
  if (!on) return;
  const int base = el * C;
  int pos = 0;
  for (int j = 0; j < C; ++j) pos += race_key_less(s_key[base + j], s_key[threadIdx.x], j, car) ? 1 : 0;
  const size_t n = (size_t)env * C + car;
  int pts;
  if (mode == RACE_COMPETITION) {
    const int table[10] = {0, 1, 2, 3, 5, 8, 13, 21, 24, 45};
    pts = table[9 - (pos < 9 ? pos : 9)];
    if (fastest_car && fastest_car[env] == car) pts += 15;
  } else {
    pts = !has_best ? 0 : pos == 0 ? 15 : pos == 1 ? 7 : pos == 2 ? 3 : 0;
  }
  if (order) order[(size_t)env * C + pos] = car;
  if (position) position[n] = pos;
  if (points) points[n] = pts;
}
