// nascar_replay.h -- the device replay ring of the off-policy collection (nascar_collect_transitions,
// nascar_replay_sample; include/nascar.h).  Included by nascar_kernels.hip after policy_car.
//
// SB3's off-policy algorithms (learn/sac.py, learn/td3.py, learn/td3_n.py, learn/ddpg.py of the reference) run
// OffPolicyAlgorithm.collect_rollouts: sample an exploring action, step the env, ReplayBuffer.add the transition
// (_store_transition), and later ReplayBuffer.sample uniform minibatches.  The ring is caller-owned: `capacity` step
// slots of N = E * C cars, 319 bytes per transition (obs and next_obs 152 each, the action 8, the reward 4, done,
// timeout and live one byte each).
#pragma once

// One step's transition for the cars [c0, c1) (a shard's, contiguous), after the step's sensor launch (and, in
// random-track mode, after the track switch): _store_transition's choice of next_obs where the row is written -- the
// terminal observation for the cars of done envs, else the new one -- plus the done / timeout / live bytes, the uniform
// source's scaled action (source 0: the draw of policy 0 that the step kernel took, recomputed: scale(u)) and, when
// another step of the call follows, the new observation as that step's `obs` row (obs_next; null after the last step).
// One 152-byte row over 19 lanes (8-byte accesses); a row's lane 0 writes the car's scalars.
#define RP_ROW 19   // float2 per observation row
__global__ void __launch_bounds__(256) replay_store_kernel(int c0, int c1, int C, const float* __restrict__ obs,
                                                           const float* __restrict__ term, const uint8_t* __restrict__ car_flags,
                                                           const uint8_t* __restrict__ env_flags, float* __restrict__ next_obs,
                                                           float* __restrict__ obs_next, uint8_t* __restrict__ done,
                                                           uint8_t* __restrict__ timeout, uint8_t* __restrict__ live,
                                                           float* __restrict__ actions, int source, uint64_t seed, int64_t step) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long rel = t / RP_ROW;
  const int j = (int)(t - rel * RP_ROW);
  if (rel >= c1 - c0) return;
  const size_t car = (size_t)c0 + (size_t)rel;
  const uint8_t ef = env_flags[car / C];
  const bool d = (ef & 3) != 0;
  const f32x2 cur = ((const f32x2*)(obs + car * ACT_OBS))[j];
  f32x2 nxt = cur;
  if (d) nxt = ((const f32x2*)(term + car * ACT_OBS))[j];
  ((f32x2*)(next_obs + car * ACT_OBS))[j] = nxt;
  if (obs_next) ((f32x2*)(obs_next + car * ACT_OBS))[j] = cur;
  if (j == 0) {
    const uint8_t cf = car_flags[car];
    done[car] = d ? 1 : 0;
    timeout[car] = (ef & 2) && !(ef & 1) ? 1 : 0;
    live[car] = !(cf & 1) || (cf & 2) ? 1 : 0;   // disabled before this step: disabled and not just disabled
    if (source == 0) {
      float a0, a1;
      policy_car(0, seed, step, (int)car, nullptr, nullptr, a0, a1);
      *(f32x2*)&actions[2 * car] = (f32x2){scale_action(a0), scale_action(a1)};
    }
  }
}

// ReplayBuffer.sample as one launch: sample i of (seed, draw) is the transition (slot, car) of key = policy_key(seed,
// draw, i), slot = (mix32(key ^ REPLAY_SALT_SLOT) * size) >> 32, car = (mix32(key ^ REPLAY_SALT_CAR) * N) >> 32 --
// uniform over the `size` filled step slots x N cars -- gathered into contiguous [batch] rows.  32 lanes per sample:
// lanes 0-18 copy the two observation rows (8-byte accesses, coalesced per row), lane 19 the action, lanes 20-22 the
// reward, done * (1 - timeout) as float32 (what SB3 hands the learner) and the live byte.
struct ReplayDev {
  const float *obs, *next_obs, *actions, *reward;
  const uint8_t *done, *timeout, *live;
};
__global__ void __launch_bounds__(256) replay_sample_kernel(ReplayDev R, int N, int size, uint64_t seed, int64_t draw,
                                                            int batch, float* __restrict__ obs, float* __restrict__ next_obs,
                                                            float* __restrict__ actions, float* __restrict__ reward,
                                                            float* __restrict__ done, uint8_t* __restrict__ live) {
  const int i = blockIdx.x * 8 + (threadIdx.x >> 5), j = threadIdx.x & 31;
  if (i >= batch) return;
  const uint64_t key = policy_key(seed, draw, (size_t)i);
  const uint32_t slot = (uint32_t)(((uint64_t)mix32(key ^ REPLAY_SALT_SLOT) * (uint64_t)size) >> 32);
  const uint32_t car = (uint32_t)(((uint64_t)mix32(key ^ REPLAY_SALT_CAR) * (uint64_t)N) >> 32);
  const size_t at = (size_t)slot * N + car;
  if (j < RP_ROW) {
    ((f32x2*)(obs + (size_t)i * ACT_OBS))[j] = ((const f32x2*)(R.obs + at * ACT_OBS))[j];
    ((f32x2*)(next_obs + (size_t)i * ACT_OBS))[j] = ((const f32x2*)(R.next_obs + at * ACT_OBS))[j];
  } else if (j == 19) {
    *(f32x2*)&actions[2 * (size_t)i] = *(const f32x2*)&R.actions[2 * at];
  } else if (j == 20) {
    reward[i] = R.reward[at];
  } else if (j == 21) {
    done[i] = (float)R.done[at] * (1.0f - (float)R.timeout[at]);
  } else if (j == 22) {
    live[i] = R.live[at];
  }
}
