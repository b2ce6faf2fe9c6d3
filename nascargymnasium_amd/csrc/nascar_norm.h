// nascar_norm.h -- running observation / return normalisation on the device (nascar_set_normalize,
// nascar_normalize_reset, nascar_normalize_step, nascar_collect_normalized; include/nascar.h).
//
// The reference wraps its A2C training envs in Stable-Baselines3's VecNormalize (learn/a2c.py:94-100), the usual
// companion of SB3's PPO too: a RunningMeanStd over the 38 observation columns and one over the discounted returns,
// updated from every step's batch, and (x - mean) / sqrt(var + epsilon) clipped for observations, r / sqrt(ret_var +
// epsilon) clipped for rewards.  Every car slot is one of SB3's envs: a batch is the N = E * C rows of a step.
//
// One step_wait is three launches on one stream (kernel boundaries are the only inter-workgroup hand-off: no atomics,
// no flags):
//   norm_moments_kernel  per workgroup of NORM_ROWS rows (a rule of N alone), the float64 mean and M2 = sum (x - mean)^2
//                        of its rows' 38 columns and of returns = returns * gamma + reward, which it also stores;
//   norm_update_kernel   one lane per column merges the workgroups' (count, mean, M2) in workgroup order (the
//                        count-weighted mean, then M2_b + count_b (mean_b - mean)^2) and applies
//                        RunningMeanStd.update_from_moments;
//   norm_apply_kernel    row-local: normalize_obs on the observation and, for the cars of done envs, on the terminal
//                        observation, normalize_reward, then returns = 0 for the cars of done envs.
// The order of every sum is fixed by N, so the statistics are the same bits from run to run and whatever the rollout's
// shard count.  Built with -ffp-contract=off: the formulas are evaluated operation by operation, left to right.
#pragma once
#include "nascar_device.h"
#include "nascar_actor.h"   // f32x2

namespace nascar {

#define NORM_OBS 38
#define NORM_COLS 39        // the observation columns and the returns column
#define NORM_ROWS 256       // rows per norm_moments_kernel workgroup
#define NORM_UNROLL 4       // row loads in flight per lane: a lane's sum stays in row order
#define NORM_PAIRS 19       // float2 per observation row
#define NORM_SUB 13         // row lanes of a workgroup: 13 x 19 = 247 lanes load 13 whole rows, 8 bytes each, contiguous
#define NORM_RSUB 9         // the other 9 lanes walk the returns column
// statistics record, float64: obs_mean [38], obs_var [38], obs_count, ret_mean, ret_var, ret_count
#define NORM_ST_VAR 38
#define NORM_ST_COUNT 76
#define NORM_ST_RMEAN 77
#define NORM_ST_RVAR 78
#define NORM_ST_RCOUNT 79
#define NORM_STATS 80

// lane roles of norm_moments_kernel: (pair, sub) for the observation lanes, sub alone for the returns lanes
struct NormLane { bool obs; int pair, sub; };
static __device__ __forceinline__ NormLane norm_lane(int t) {
  const bool o = t < NORM_PAIRS * NORM_SUB;
  return {o, o ? t % NORM_PAIRS : 0, o ? t / NORM_PAIRS : t - NORM_PAIRS * NORM_SUB};
}
// column c's sum over the row lanes, in lane order
static __device__ __forceinline__ double norm_col_sum(const double (*red)[256], int c) {
  double a = 0.0;
  if (c < NORM_OBS) {
    for (int k = 0; k < NORM_SUB; ++k) a += red[c & 1][k * NORM_PAIRS + (c >> 1)];
  } else {
    for (int k = 0; k < NORM_RSUB; ++k) a += red[0][NORM_PAIRS * NORM_SUB + k];
  }
  return a;
}

// obs null: no observation columns; reward null: no returns column.  part [gridDim.x][39][2]: mean, M2.
__global__ void __launch_bounds__(256) norm_moments_kernel(int N, const float* __restrict__ obs,
                                                           const float* __restrict__ reward, double* __restrict__ returns,
                                                           double gamma, double* __restrict__ part) {
  __shared__ double red[2][256];
  __shared__ double cmean[NORM_COLS + 1];
  const int t = threadIdx.x, r0 = blockIdx.x * NORM_ROWS, rows = min(NORM_ROWS, N - r0);
  const NormLane L = norm_lane(t);
  const f32x2* orow = obs ? (const f32x2*)(obs + (size_t)r0 * NORM_OBS) + L.pair : nullptr;
  // NORM_UNROLL loads are issued before their values are added, in row order (a row past the end adds nothing)
  double s0 = 0.0, s1 = 0.0;
  if (L.obs) {
    if (obs)
      for (int r = L.sub; r < rows; r += NORM_UNROLL * NORM_SUB) {
        f32x2 v[NORM_UNROLL];
#pragma unroll
        for (int j = 0; j < NORM_UNROLL; ++j) {
          const int rj = r + j * NORM_SUB;
          v[j] = rj < rows ? orow[(size_t)rj * NORM_PAIRS] : (f32x2){0.0f, 0.0f};
        }
#pragma unroll
        for (int j = 0; j < NORM_UNROLL; ++j)
          if (r + j * NORM_SUB < rows) { s0 += (double)v[j].x; s1 += (double)v[j].y; }
      }
  } else if (reward) {
    for (int r = L.sub; r < rows; r += NORM_UNROLL * NORM_RSUB) {
      double v[NORM_UNROLL];
#pragma unroll
      for (int j = 0; j < NORM_UNROLL; ++j) {
        const int rj = r + j * NORM_RSUB;
        v[j] = rj < rows ? returns[r0 + rj] * gamma + (double)reward[r0 + rj] : 0.0;
      }
#pragma unroll
      for (int j = 0; j < NORM_UNROLL; ++j) {
        const int rj = r + j * NORM_RSUB;
        if (rj < rows) { returns[r0 + rj] = v[j]; s0 += v[j]; }
      }
    }
  }
  red[0][t] = s0; red[1][t] = s1;
  __syncthreads();
  if (t < NORM_COLS) cmean[t] = norm_col_sum(red, t) / (double)rows;
  __syncthreads();
  // second pass about the workgroup's mean (its rows, 39 KB, are still on chip)
  double q0 = 0.0, q1 = 0.0;
  if (L.obs) {
    if (obs) {
      const double m0 = cmean[2 * L.pair], m1 = cmean[2 * L.pair + 1];
      for (int r = L.sub; r < rows; r += NORM_UNROLL * NORM_SUB) {
        f32x2 v[NORM_UNROLL];
#pragma unroll
        for (int j = 0; j < NORM_UNROLL; ++j) {
          const int rj = r + j * NORM_SUB;
          v[j] = rj < rows ? orow[(size_t)rj * NORM_PAIRS] : (f32x2){0.0f, 0.0f};
        }
#pragma unroll
        for (int j = 0; j < NORM_UNROLL; ++j)
          if (r + j * NORM_SUB < rows) {
            const double d0 = (double)v[j].x - m0, d1 = (double)v[j].y - m1;
            q0 += d0 * d0; q1 += d1 * d1;
          }
      }
    }
  } else if (reward) {
    const double m = cmean[NORM_OBS];
    for (int r = L.sub; r < rows; r += NORM_RSUB) {   // (the lane's own stores of the first pass)
      const double d = returns[r0 + r] - m;
      q0 += d * d;
    }
  }
  red[0][t] = q0; red[1][t] = q1;
  __syncthreads();
  if (t < NORM_COLS) {
    double* p = part + ((size_t)blockIdx.x * NORM_COLS + t) * 2;
    p[0] = cmean[t];
    p[1] = norm_col_sum(red, t);
  }
}

// One workgroup, one lane per column: the batch moments from the G workgroups' partials, then
// RunningMeanStd.update_from_moments on the column's statistics (SB3 common/running_mean_std.py).
__global__ void __launch_bounds__(64) norm_update_kernel(int N, int G, const double* __restrict__ part, int do_obs,
                                                         int do_ret, double* __restrict__ stats) {
  const int c = threadIdx.x;
  const bool active = c < NORM_COLS && (c < NORM_OBS ? do_obs : do_ret) != 0;
  double* mean_p = c < NORM_OBS ? stats + c : stats + NORM_ST_RMEAN;
  double* var_p = c < NORM_OBS ? stats + NORM_ST_VAR + c : stats + NORM_ST_RVAR;
  double* count_p = stats + (c < NORM_OBS ? NORM_ST_COUNT : NORM_ST_RCOUNT);
  double new_mean = 0.0, new_var = 0.0, new_count = 0.0;
  if (active) {
    // the batch mean is the count-weighted mean of the workgroups' means; the batch M2 their M2 plus each one's
    // count x (mean_b - mean)^2 (the parallel-axis form), both summed in workgroup order
    double sm = 0.0;
    for (int b = 0; b < G; ++b)
      sm += (double)min(NORM_ROWS, N - b * NORM_ROWS) * part[((size_t)b * NORM_COLS + c) * 2];
    const double bm = sm / (double)N;
    double m2 = 0.0;
    for (int b = 0; b < G; ++b) {
      const double d = part[((size_t)b * NORM_COLS + c) * 2] - bm;
      m2 += part[((size_t)b * NORM_COLS + c) * 2 + 1] + (double)min(NORM_ROWS, N - b * NORM_ROWS) * (d * d);
    }
    const double bv = m2 / (double)N, bc = (double)N;
    const double mean = *mean_p, var = *var_p, count = *count_p;
    const double delta = bm - mean, tot = count + bc;
    new_mean = mean + delta * bc / tot;
    const double M2 = var * count + bv * bc + delta * delta * count * bc / (count + bc);
    new_var = M2 / (count + bc);
    new_count = bc + count;
  }
  __syncthreads();   // the observation columns share one count: every lane has read it before lane 0 writes it
  if (active) {
    *mean_p = new_mean;
    *var_p = new_var;
    if (c == 0 || c == NORM_OBS) *count_p = new_count;
  }
}

struct NormApply {
  int norm_obs, norm_reward, zero_returns;
  double clip_obs, clip_reward, eps;
};
static __device__ __forceinline__ float norm_clip(double v, double c) {
  return (float)(v < -c ? -c : v > c ? c : v);   // np.clip: a NaN passes
}
// The cars [c0, c1): one lane per observation element.  obs_out / term_out may be their inputs (each element is read
// and written by one lane); term / term_out null: no terminal observations; reward null: observations only
// (VecNormalize.reset).  The rows of term_out of envs that did not end are left as they are.
__global__ void __launch_bounds__(256) norm_apply_kernel(int c0, int c1, int C, NormApply A, const double* __restrict__ stats,
                                                         const float* obs, float* obs_out, const float* term, float* term_out,
                                                         const float* reward, float* reward_out,
                                                         const uint8_t* __restrict__ env_flags, double* __restrict__ returns) {
  __shared__ double mean[NORM_OBS], den[NORM_OBS];
  const int t = threadIdx.x;
  if (t < NORM_OBS) {
    mean[t] = stats[t];
    den[t] = sqrt(stats[NORM_ST_VAR + t] + A.eps);
  }
  __syncthreads();
  const long long i = (long long)blockIdx.x * 256 + t;
  const long long rel = i / NORM_OBS;
  if (rel >= c1 - c0) return;
  const int col = (int)(i - rel * NORM_OBS);
  const size_t car = (size_t)c0 + (size_t)rel, at = car * NORM_OBS + col;
  const bool done = env_flags && (env_flags[car / C] & 3) != 0;
  const float x = obs[at];
  obs_out[at] = A.norm_obs ? norm_clip(((double)x - mean[col]) / den[col], A.clip_obs) : x;
  if (term && done) {
    const float y = term[at];
    term_out[at] = A.norm_obs ? norm_clip(((double)y - mean[col]) / den[col], A.clip_obs) : y;
  }
  if (col == 0 && reward) {
    const float r = reward[car];
    reward_out[car] = A.norm_reward ? norm_clip((double)r / sqrt(stats[NORM_ST_RVAR] + A.eps), A.clip_reward) : r;
    if (A.zero_returns && done) returns[car] = 0.0;
  }
}

}  // namespace nascar
