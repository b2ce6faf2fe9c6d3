// nascar_actor.h -- fused SAC actor inference on MFMA.
//
// The reference's closed-loop drivers run Stable-Baselines3 SAC policies
// (game/control/sac_control_class.py:80-115: model.predict(obs, deterministic=True)):
// MlpPolicy actor  latent = ReLU(W2 ReLU(W1 obs + b1) + b2),  mu = W3 latent + b3,
// action = unscale_action(tanh(mu))  with the Box(-1, 1) action space.
//
// One wave = 32 observations; all three layers run on the MFMA with the batch on the lanes:
//   layer 1  H1^T[256 x 32] = [W1 | b1_hi | b1_lo][256 x 40] . [X | 1 | 1]^T   (bf16 MFMA 32x32x16, fp32
//            acc; 8 tiles x 3 k-steps -- the bias rides in two extra K columns, hi + lo bf16 halves)
//   layer 2  H2^T[256 x 32] = W2[256 x 256] . relu(H1^T) + b2   (the layer-1 accumulator tiles, ReLU'd
//            and packed to bf16 in registers, are the B operands directly -- hidden units sit in the
//            registers -- with W2 pre-permuted on the host into the matching k order; b2 is the
//            accumulator's initial value; W2 staged in LDS per workgroup)
//   layer 3  mu^T[32 x 32] = W3'[32 x 256] . relu(H2^T)  with the same register trick; W3' rows 0-3 are
//            bf16 hi(w3[0]), hi(w3[1]), lo(w3[0]), lo(w3[1]) (rows 4-31 zero), so mu_i = row i + row i+2
//            carries W3 to ~2^-16 relative
// Numerics: bf16 operands X, W1, relu(H1), W2, relu(H2); b1 and W3 as bf16 hi + lo pairs; fp32
// accumulation, b2 and tanh in fp32.  Tolerance vs a PyTorch fp32 forward: tests/test_gpu_actor.py.
#pragma once
#include "nascar_device.h"

namespace nascar {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) short i16x8;
typedef __attribute__((ext_vector_type(2))) float f32x2;

typedef __attribute__((ext_vector_type(2))) short i16x2;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

// two floats -> packed bf16 pair, round-to-nearest-even: one v_cvt_pk_bf16_f32 (converted pairwise --
// hipcc splits wider vector truncations that feed integer ops into per-element converts + v_perm)
__device__ __forceinline__ unsigned cvt_pk_bf16(float a, float b) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector(((f32x2){a, b}), bf16x2));
}
// ReLU on a packed bf16 pair's bits (v_pk_max_i16: a negative bf16 is a negative int16)
__device__ __forceinline__ unsigned relu_pk(unsigned p) {
  return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(i16x2, p), (i16x2){}));
}
// relu of registers 8S .. 8S+7 of an accumulator tile as one bf16 B fragment
template <int S>
__device__ __forceinline__ bf16x8 relu_bf16x8(const f32x16& a) {
  const u32x4 u = {relu_pk(cvt_pk_bf16(a[8 * S], a[8 * S + 1])), relu_pk(cvt_pk_bf16(a[8 * S + 2], a[8 * S + 3])),
                   relu_pk(cvt_pk_bf16(a[8 * S + 4], a[8 * S + 5])), relu_pk(cvt_pk_bf16(a[8 * S + 6], a[8 * S + 7]))};
  return __builtin_bit_cast(bf16x8, u);
}

#define ACT_OBS 38
#define ACT_K 40          // layer-1 K: 38 features + the b1 hi/lo columns (row stride of w1p)
#define ACT_H 256
#define ACT_OUT 2
#define ACT_WAVES 8       // waves per workgroup (2 per SIMD); each walks its own 32-observation tiles

struct ActorDev {
  const bf16x8* w1p;   // [256][40] bf16: W1 row | bf16(b1) | bf16(b1 - bf16(b1)), read as 16-B fragments
  const bf16x8* w2p;   // [8 o][8 q][2 s][2 h][32 r] x 8 bf16: W2[32o + r][32q + 16s + 8(j>>2) + 4h + (j&3)]
                       // (lane l = 32h + r reads fragment l of a 1 KB block: conflict-free ds_read_b128)
  const float* b2;     // [256]
  const bf16x8* w3p;   // [8 o][2 s][2 h][4 r] x 8 bf16: W3'[r][32o + 16s + 8(j>>2) + 4h + (j&3)], rows 0-3
  const float* b3;     // [2]
};

// The observations of one 32-row wave tile in the layer-1 B layout: lane (r, h) holds
// obs[row r][16s + 8h .. +7] for s = 0, 1 and, on h = 0 lanes, obs[row r][32 .. 37] (s = 2).
struct ObsFrag { f32x2 v[11]; };

__device__ __forceinline__ void actor_fetch(ObsFrag& f, const float* __restrict__ obs, int N, int tile, int r, int h) {
  // branch-free: the row is clamped (a ragged tile's extra lanes are never stored) and the s = 2
  // loads of h = 1 lanes repeat the h = 0 columns (zeroed at conversion); 8-B aligned float2 loads
  const int row = min(tile * 32 + r, N - 1);
  const f32x2* p = (const f32x2*)(obs + (size_t)row * ACT_OBS);
#pragma unroll
  for (int i = 0; i < 4; ++i) f.v[i] = p[4 * h + i];            // columns 8h .. 8h + 7
#pragma unroll
  for (int i = 0; i < 4; ++i) f.v[4 + i] = p[8 + 4 * h + i];    // columns 16 + 8h .. 23 + 8h
#pragma unroll
  for (int i = 0; i < 3; ++i) f.v[8 + i] = p[16 + i];           // columns 32 .. 37
}

__device__ __forceinline__ bf16x8 to_bf16x8(f32x2 a, f32x2 b, f32x2 c, f32x2 d) {
  const u32x4 u = {cvt_pk_bf16(a.x, a.y), cvt_pk_bf16(b.x, b.y), cvt_pk_bf16(c.x, c.y), cvt_pk_bf16(d.x, d.y)};
  return __builtin_bit_cast(bf16x8, u);
}

// Persistent: one workgroup per CU stages W2 (128 KB), W1' (20 KB), b2 and W3 in LDS once; then each
// wave independently walks 32-observation tiles (no block barriers in the loop), fetching the next
// tile's observations into registers while the current tile computes.  The LDS weight fragments are
// double-buffered in registers one k-step (4 MFMAs) ahead of their use.
__global__ void __launch_bounds__(64 * ACT_WAVES) __attribute__((amdgpu_waves_per_eu(2, 2))) actor_kernel(int N, const float* __restrict__ obs,
                                                               float* __restrict__ act, ActorDev A) {
  __shared__ bf16x8 s_w2[ACT_H * ACT_H / 8];   // 128 KB: the permuted W2 fragments
  __shared__ bf16x8 s_w1[ACT_H * ACT_K / 8];   // 20 KB
  __shared__ float4 s_b2[ACT_H / 4];
  __shared__ bf16x8 s_w3[3 * 8 * 2 * 2 * 4];   // 1 KB of W3' rows 0-3, then 2 KB of zeros read by rows 4-31
  const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, r = l & 31, h = l >> 5;
  APROF_RT(14);
  APROF(0);
  // W2 and W1' straight into LDS (global_load_lds, 16 B per lane = 1 KB per wave-instruction, all of a
  // wave's in flight together; the barrier below drains them)
#pragma unroll
  for (int i = 0; i < ACT_H * ACT_K / 8 / 64; i += ACT_WAVES) {
    const int chunk = i + wave;
    if (chunk < ACT_H * ACT_K / 8 / 64)
      __builtin_amdgcn_global_load_lds((const void*)(A.w1p + 64 * chunk + l),
                                       (__attribute__((address_space(3))) void*)(s_w1 + 64 * chunk), 16, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < ACT_H * ACT_H / 8 / 64; i += ACT_WAVES) {
    const int chunk = i + wave;
    __builtin_amdgcn_global_load_lds((const void*)(A.w2p + 64 * chunk + l),
                                     (__attribute__((address_space(3))) void*)(s_w2 + 64 * chunk), 16, 0, 0);
  }
  for (int i = tid; i < ACT_H / 4; i += 64 * ACT_WAVES) s_b2[i] = ((const float4*)A.b2)[i];
  for (int i = tid; i < 3 * 8 * 2 * 2 * 4; i += 64 * ACT_WAVES) s_w3[i] = i < 8 * 2 * 2 * 4 ? A.w3p[i] : (bf16x8){};
  const float b30 = A.b3[0], b31 = A.b3[1];
  // contiguous tile ranges per workgroup (the split stays within one tile per CU), round-robin over waves
  const int ntile = (N + 31) / 32;
  const int t_end = (int)((long long)ntile * (blockIdx.x + 1) / gridDim.x);
  int tile = (int)((long long)ntile * blockIdx.x / gridDim.x) + wave;
  ObsFrag cur;
  if (tile < t_end) actor_fetch(cur, obs, N, tile, r, h);
  __syncthreads();
  APROF(1);
  int ntiles_done = 0;
  // lane (r, h)'s A-fragment addresses: W1' row 32p + r (stride 5 fragments), W2 (o, q, s2) blocks
  const bf16x8* w1_lane = s_w1 + r * (ACT_K / 8);
  const bf16x8* w2_lane = s_w2 + l;
  // W3' fragment (o, s2) of lane (r, h) at [8(2o + s2) + 4h + r]; rows 4-31 read the zero block instead
  const bf16x8* w3_lane = s_w3 + (r < 4 ? 4 * h + r : 8 * 2 * 2 * 4);
  for (; tile < t_end; tile += ACT_WAVES) {
    // the LDS weight fragments are tile-invariant: without this clobber LICM hoists them all out of
    // the loop (hundreds of registers) and the kernel spills
    asm volatile("" ::: "memory");
    bf16x8 xf[3];
    xf[0] = to_bf16x8(cur.v[0], cur.v[1], cur.v[2], cur.v[3]);
    xf[1] = to_bf16x8(cur.v[4], cur.v[5], cur.v[6], cur.v[7]);
    xf[2] = to_bf16x8(cur.v[8], cur.v[9], cur.v[10], (f32x2){1.0f, 1.0f});
    if (h) xf[2] = (bf16x8){};
    if (tile + ACT_WAVES < t_end) actor_fetch(cur, obs, N, tile + ACT_WAVES, r, h);   // lands during this tile
    // layer 1 in two halves of 4 accumulator tiles (64 registers live) over 3 k-steps, A fragments
    // one k-step ahead; each half's ReLU output is converted in registers to layer-2 B fragments
    // (register 8 s2 + j of tile p is hidden unit 32p + 16 s2 + 8(j>>2) + 4h + (j&3), the k order w2p
    // was permuted into); the ReLU runs on the packed bf16 bits (v_pk_max_i16: a negative bf16 is a
    // negative int16)
    bf16x8 hf[8][2];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      f32x16 acc[4];
      bf16x8 a1[2][4];
#pragma unroll
      for (int p = 0; p < 4; ++p) a1[0][p] = w1_lane[32 * (4 * half + p) * (ACT_K / 8) + h];
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        if (s < 2) {
#pragma unroll
          for (int p = 0; p < 4; ++p)
            a1[(s + 1) & 1][p] = w1_lane[32 * (4 * half + p) * (ACT_K / 8) + (s == 0 ? 2 + h : 4)];
        }
#pragma unroll
        for (int p = 0; p < 4; ++p)
          acc[p] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[s & 1][p], xf[s], s == 0 ? (f32x16){} : acc[p], 0, 0, 0);
      }
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        hf[4 * half + p][0] = relu_bf16x8<0>(acc[p]);
        hf[4 * half + p][1] = relu_bf16x8<1>(acc[p]);
      }
    }
    // layer 2 in two halves of 4 output tiles (64 accumulator registers live, not 128), 16 k-steps
    // each with the next k-step's 4 A fragments in flight, the accumulators starting from b2; each
    // half's relu(H2) is packed to bf16 B fragments and fed straight into layer 3
    f32x16 acc3 = {};
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      f32x16 acc2[4];
#pragma unroll
      for (int o = 0; o < 4; ++o) {   // register reg of tile o is hidden unit 32o + (reg&3) + 8(reg>>2) + 4h
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          const float4 b = s_b2[(32 * (4 * half + o) + 8 * q4 + 4 * h) / 4];
          acc2[o][4 * q4] = b.x; acc2[o][4 * q4 + 1] = b.y; acc2[o][4 * q4 + 2] = b.z; acc2[o][4 * q4 + 3] = b.w;
        }
      }
      bf16x8 a2[2][4];
#pragma unroll
      for (int o = 0; o < 4; ++o) a2[0][o] = w2_lane[(4 * half + o) * 8 * 2 * 64];
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {   // ks = 2q + s2
        if (ks < 15) {
#pragma unroll
          for (int o = 0; o < 4; ++o) a2[(ks + 1) & 1][o] = w2_lane[((4 * half + o) * 16 + ks + 1) * 64];
        }
#pragma unroll
        for (int o = 0; o < 4; ++o)
          acc2[o] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2[ks & 1][o], hf[ks >> 1][ks & 1], acc2[o], 0, 0, 0);
      }
      // layer 3 over this half's 128 hidden units (8 k-steps); W3' fragments are zero past row 3
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        acc3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w3_lane[((4 * half + o) * 2 + 0) * 8], relu_bf16x8<0>(acc2[o]), acc3, 0, 0, 0);
        acc3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w3_lane[((4 * half + o) * 2 + 1) * 8], relu_bf16x8<1>(acc2[o]), acc3, 0, 0, 0);
      }
    }
    // mu^T rows 0-3 sit in registers 0-3 of the h = 0 lanes (column r = this lane's observation)
    const int row = tile * 32 + r;
    if (row < N && h == 0) {
      // deterministic SAC action tanh(mu), then BasePolicy.unscale_action for Box(-1, 1) in float32:
      // low + 0.5 * (a + 1) * (high - low)
      const float m0 = acc3[0] + acc3[2], m1 = acc3[1] + acc3[3];
      const float a0 = tanhf(m0 + b30), a1v = tanhf(m1 + b31);
      *(f32x2*)&act[2 * (size_t)row] = (f32x2){-1.0f + ((0.5f * (a0 + 1.0f)) * 2.0f), -1.0f + ((0.5f * (a1v + 1.0f)) * 2.0f)};
    }
    ++ntiles_done;
    if (ntiles_done < 6) APROF(1 + ntiles_done);
  }
  APROF_RT(15);
  (void)ntiles_done;
}

// ------------------------------------------------------------------ reference-precision (fp32) actor
// The same SB3 MlpPolicy actor in float32 throughout (fp32 FMAs, fp32 tanh): the precision of the reference's
// model.predict (PyTorch fp32), up to summation order -- |delta action| ~1e-6 against a PyTorch fp32 forward.
// One 256-thread workgroup per 32-observation tile: thread t owns hidden unit t for the tile's 32 rows (32
// accumulators), the tile's observations / ReLU'd activations sit in LDS and are read as broadcasts, the
// weights are read transposed ([k][unit], one coalesced 1 KB row per k, L2-resident), layer 3 on 64 lanes.
// VALU-bound: 151 kFLOP per observation (~2x the bf16 MFMA kernel's time at the fp32 vector peak).
struct ActorF32 {
  const float* w1t;   // [38][256]  W1 transposed
  const float* b1;    // [256]
  const float* w2t;   // [256][256] W2 transposed
  const float* b2;    // [256]
  const float* w3;    // [2][256]   mu.weight
  const float* b3;    // [2]
};
// ------------------------------------------------------------------ reference-precision actor on the f32 MFMA
// The float32 actor (SB3 MlpPolicy: ReLU(W2 ReLU(W1 x + b1) + b2), mu = W3 h + b3, tanh, unscale_action) on
// v_mfma_f32_32x32x2_f32: exact f32 products accumulated as an fmaf chain (bitwise, MI355X_MICROARCH.md
// "FP32-input MFMA"), so the result is the fp32 kernel's up to summation order.  One wave = 32 observations
// (batch on the MFMA N dimension, lane r = l & 31 owns observation r, lane half h = l >> 5):
//   layer 1  H1^T[256 x 32] = W1[256 x 38] . X^T: 8 unit tiles x 19 k-steps; A = W1^T[2s + h][32t + r] (global,
//            coalesced per half), B = X[row r][2s + h] (global);
//   layer 2  H2^T = W2 . relu(H1^T + b1): the layer-1 accumulators are the B operands in place -- k-step
//            (t, q) takes register q of tile t, i.e. hidden unit u = 32t + (q & 3) + 8(q >> 2) + 4h on half h
//            (the 32x32 C/D map) -- and A = W2^T[u][32t' + r] is read from global (L2-resident, coalesced per
//            half): 128 k-steps x 8 output tiles;
//   layer 3  mu_i = W3[i] . relu(H2^T + b2) + b3: per-lane partial sums over the lane's 128 hidden values, the
//            two lane halves added with a cross-half swap, then tanh / unscale_action in f32.
// 1024 + 152 MFMAs of 64 cycles per 32 observations: the f32 matrix rate is the f32 vector rate, and
// the MFMA needs one VGPR per operand where the VALU kernel re-read every activation from LDS.
#define AM_WAVES 4
__global__ void __launch_bounds__(64 * AM_WAVES) __attribute__((amdgpu_waves_per_eu(1)))
actor_mfma32_kernel(int N, const float* __restrict__ obs, float* __restrict__ act, ActorF32 A) {
  __shared__ float s_b1[ACT_H], s_b2[ACT_H], s_w3[2 * ACT_H];
  for (int i = threadIdx.x; i < ACT_H; i += 64 * AM_WAVES) { s_b1[i] = A.b1[i]; s_b2[i] = A.b2[i]; }
  for (int i = threadIdx.x; i < 2 * ACT_H; i += 64 * AM_WAVES) s_w3[i] = A.w3[i];
  __syncthreads();
  const int l = threadIdx.x & 63, r = l & 31, h = l >> 5;
  const int tile = blockIdx.x * AM_WAVES + (threadIdx.x >> 6);
  const int row0 = tile * 32;
  if (row0 >= N) return;
  const int row = row0 + r;
  const float* xr = obs + (size_t)(row < N ? row : N - 1) * ACT_OBS;
  f32x16 acc[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) acc[t] = (f32x16){};
  // layer 1
#pragma unroll
  for (int s = 0; s < ACT_OBS / 2; ++s) {
    const float b = xr[2 * s + h];
    const float* w = A.w1t + (size_t)(2 * s + h) * ACT_H + r;
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[32 * t], b, acc[t], 0, 0, 0);
  }
  f32x16 hid[8];   // relu(H1 + b1) as layer 2's B operands
#pragma unroll
  for (int t = 0; t < 8; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int u = 32 * t + (q & 3) + 8 * (q >> 2) + 4 * h;
      hid[t][q] = fmaxf(acc[t][q] + s_b1[u], 0.0f);
    }
#pragma unroll
  for (int t = 0; t < 8; ++t) acc[t] = (f32x16){};
  // layer 2
#pragma unroll
  for (int t = 0; t < 8; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int u = 32 * t + (q & 3) + 8 * (q >> 2) + 4 * h;
      const float* w = A.w2t + (size_t)u * ACT_H + r;
      const float b = hid[t][q];
#pragma unroll
      for (int o = 0; o < 8; ++o) acc[o] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[32 * o], b, acc[o], 0, 0, 0);
    }
  // layer 3: partial sums of this lane's half, then the two halves of the observation added
  float m0 = 0.0f, m1 = 0.0f;
#pragma unroll
  for (int t = 0; t < 8; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int u = 32 * t + (q & 3) + 8 * (q >> 2) + 4 * h;
      const float v = fmaxf(acc[t][q] + s_b2[u], 0.0f);
      m0 = fmaf(s_w3[u], v, m0);
      m1 = fmaf(s_w3[ACT_H + u], v, m1);
    }
  m0 += __shfl_xor(m0, 32);
  m1 += __shfl_xor(m1, 32);
  if (h == 0 && row < N) {
    const float a0 = tanhf(m0 + A.b3[0]), a1 = tanhf(m1 + A.b3[1]);
    *(f32x2*)&act[2 * (size_t)row] = (f32x2){-1.0f + ((0.5f * (a0 + 1.0f)) * 2.0f), -1.0f + ((0.5f * (a1 + 1.0f)) * 2.0f)};
  }
}

// ------------------------------------------------------------------ per-car controllers (policy 4): the general f32 MLP
// The reference's race modes put a different controller in every car of an env (game/competition.py:150-212, 285-307:
// one controller per car, controller.control(obs[car_idx]) before every env.step): SB3 SAC, PPO and A2C checkpoints
// beside the rule driver.  mlp_field_kernel is actor_mfma32_kernel generalised to every model the reference ships
// (game/control/models/): a float32 MLP  obs[38] -> h1 -> h2 -> 2  on v_mfma_f32_32x32x2_f32, templated on the hidden
// tile counts T1 = h1 / 32 and T2 = h2 / 32 and on the activation; the output transform is a template of the epilogue
// (mlp_out<OUT>), chosen per controller by a wave-uniform switch, so that controllers that differ only in it share a
// launch.
//   activation  MLP_RELU, or MLP_TANH with tanhf in f32 (SB3's ActorCriticPolicy default, the PPO checkpoints)
//   output      MLP_OUT_RAW    mu = W3 h + b3
//               MLP_OUT_CLIP   min(max(mu, -1), 1): SB3 predict for an unsquashed Box policy (PPO, A2C)
//               MLP_OUT_SQUASH tanh(mu), then unscale_action for the Box(-1, 1) (SAC; actor_mfma32_kernel's expression)
//               MLP_OUT_VALUE  a critic: w3 is the value head padded to [2][h2] (second row zero); m0 + b3[0] goes to
//                              values[row] (4-byte stores), nothing to act
//               MLP_OUT_SAMPLE the Gaussian actor of SB3's on-policy algorithms, sampled: see mlp_sample below
//               MLP_OUT_SQUASH_SAMPLE  SB3's SAC actor, sampled (a four-row head: mu and log_std): see mlp_explore below;
//                              only the explorer's instantiations (EXPL) hold it
//               MLP_OUT_CATEGORICAL  SB3's categorical actor for Discrete(5), sampled (a five-row head: the logits): see
//                              mlp_categorical below; MLP_OUT_MODE its arg max (deterministic = True), a driver of the field.
//                              The five-row instantiations (CAT) and mlp_wide_kernel hold them, beside outputs 0-4
// Shapes: obs_dim 38 and act_dim 2; (h1, h2) one of MLP_SHAPES below -- 256-256 (the SAC checkpoints), 64-64 (ppo_789,
// ppo_849), 256-128 (a2c_best_model3), and 128-128, 256-32, 32-256 for other nets; every other shape is rejected when the
// controller is loaded (mlp_shape_ok), with a message naming it.  That includes TD3's SB3 default [400, 300]: no multiple
// of 32, and the reference ships no TD3 checkpoint.  512-512 ReLU (MLP_WIDE_SHAPES) runs on mlp_wide_kernel below; a five-row
// head (act_dim 5: outputs 6 and 7) on the CAT instantiations or on the wide kernel.
// Addressing: one wave = one tile = 32 consecutive envs at ONE car slot c, so the controller is wave-uniform: row i of
// the tile is car (env0 + i) * C + c, its observation C * 38 floats after row i - 1's, its action at [car][2].  The
// kernel covers the env range [env0, env0 + nenv) (a rollout shard runs it on its own envs); the last tile of the range
// may be ragged: its extra lanes load the range's last row and store nothing.  blockIdx.y picks the (slot, controller)
// pair of the launch; the weights come from the device table of controllers (scalar loads: the index is uniform).
// With C = 1 and c = 0 the rows are a flat batch: nascar_controller_forward.
// Launches: one per distinct (T1, T2, activation) among a field's controllers (at most the instantiations below,
// however many controllers are loaded) -- not one kernel with a switch over the instantiations, which would run the
// 64-64 nets at the 256-256 net's one wave per SIMD.
// <8, 8, MLP_RELU> with MLP_OUT_SQUASH performs actor_mfma32_kernel's operations in its order (k order of all three
// layers, bias after the accumulation, the lane-half add, tanhf, unscale_action): an all-SAC field equals policy 2 in
// fp32 bit for bit (tests/test_gpu_field.py).  Register budget: 16 (T1 + T2) accumulator / operand VGPRs.
#define MLP_MAX_CTRL 16    // controllers per handle
#define MLP_MAX_CARS 64    // car slots per env (nascar_create's limit)
enum { MLP_RELU = 0, MLP_TANH = 1 };
enum { MLP_OUT_RAW = 0, MLP_OUT_CLIP = 1, MLP_OUT_SQUASH = 2, MLP_OUT_VALUE = 3, MLP_OUT_SAMPLE = 4, MLP_OUT_SQUASH_SAMPLE = 5,
       MLP_OUT_CATEGORICAL = 6, MLP_OUT_MODE = 7 };
#define MLP_SHAPES(X) X(8, 8) X(8, 4) X(8, 1) X(4, 4) X(2, 2) X(1, 8)
// the wide shapes (mlp_wide_kernel below; ReLU only) -- a list of their own: MLP_SHAPES is every shape that holds every head
#define MLP_WIDE_SHAPES(X) X(16, 16)
#define MLP_WIDE_CHUNK 4   // layer-2 output tiles per chunk of mlp_wide_kernel
#define MLP_WIDE_KB 8      // ... and the k steps per block of its weight prefetch
struct MlpDev {        // one loaded controller (device pointers)
  const float* w1t;    // [38][h1]  W1 transposed
  const float* b1;     // [h1]
  const float* w2t;    // [h1][h2]  W2 transposed
  const float* b2;     // [h2]
  const float* w3;     // [2][h2]; MLP_OUT_SQUASH_SAMPLE: [4][h2], rows 0-1 mu.weight, rows 2-3 log_std.weight;
                       //   MLP_OUT_CATEGORICAL / MLP_OUT_MODE: [5][h2], the logit rows
  const float* b3;     // [2]; MLP_OUT_SQUASH_SAMPLE: [4]; MLP_OUT_CATEGORICAL / MLP_OUT_MODE: [5]
  int h1, h2, activation, output;
};
struct MlpLaunch {
  const MlpDev* table;         // [MLP_MAX_CTRL]
  const float* obs;            // [E][C][38]
  float* act;                  // [E][C][2]
  int env0, nenv, C;
  int slot_id[MLP_MAX_CARS];   // blockIdx.y -> car slot c | controller id << 8
  // the on-policy outputs (nascar_collect, policy 6); rows are indexed like act, by car
  float* values;               // MLP_OUT_VALUE: [E][C]
  float* actions;              // MLP_OUT_SAMPLE: the unclipped action [E][C][2] (null: not kept); the explorer (EXPL):
                               //   the scaled buffer action s [E][C][2] (null: not kept); MLP_OUT_CATEGORICAL: the action
                               //   index, int32 [E][C] behind this pointer (null: not kept)
  float* logp;                 // MLP_OUT_SAMPLE, MLP_OUT_CATEGORICAL: [E][C] (null: not kept)
  const uint8_t* tflags;       // non-null: env_flags [E] of the step; only the cars of truncated, not terminated envs
  int tcars;                   //   are computed (env = car / tcars), and a tile or workgroup without one returns at once
  float log_std[2];            // MLP_OUT_SAMPLE; the explorer on an MLP_OUT_SQUASH controller: the noise sigma [2]
  uint64_t seed;
  int64_t step;
};
__device__ __forceinline__ uint32_t mix32(uint64_t x) {   // splitmix64 finaliser
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  x ^= x >> 31;
  return (uint32_t)(x >> 32);
}
// the counter key of car n at (seed, step): every device action source hashes it, each with salts of its own
__device__ __forceinline__ uint64_t policy_key(uint64_t seed, int64_t step, size_t n) {
  return (seed * 0x100000001B3ull) ^ ((uint64_t)n << 24) ^ (uint64_t)step * 0x9E3779B1ull;
}
// MLP_OUT_SAMPLE: a ~ N(mu, diag(exp(log_std))^2) as SB3's DiagGaussianDistribution samples and scores it, the noise a
// Box-Muller pair of two mix32 draws on the car's key (salts SAMPLE_SALT0 / SAMPLE_SALT1, include/nascar.h): u0 in (0, 1],
// u1 in [0, 1).  The draw depends on (seed, car, step) alone -- not on the shard, tile or lane that computes it.
// a is what the rollout buffer keeps (unclipped), clip(a, -1, 1) what drives the env (OnPolicyAlgorithm.collect_rollouts),
// logp = sum_j (-(a_j - mu_j)^2 / (2 std_j^2) - log_std_j - log(sqrt(2 pi))) as torch's Normal.log_prob writes it.
#define SAMPLE_SALT0 0x5A4D504C45ull
#define SAMPLE_SALT1 0x3C6EF372FE94F82Bull
#define HALF_LOG_2PI 0.918938533204672742f
__device__ __forceinline__ void mlp_sample(const MlpLaunch& L, size_t car, float mu0, float mu1, f32x2& a, float& logp) {
  const uint64_t key = policy_key(L.seed, L.step, car);
  const float u0 = (float)((mix32(key ^ SAMPLE_SALT0) >> 8) + 1u) * (1.0f / 16777216.0f);
  const float u1 = (float)(mix32(key ^ SAMPLE_SALT1) >> 8) * (1.0f / 16777216.0f);
  const float r = sqrtf(-2.0f * logf(u0)), th = 6.283185307179586f * u1;
  const float e0 = r * cosf(th), e1 = r * sinf(th);
  const float s0 = expf(L.log_std[0]), s1 = expf(L.log_std[1]);
  a = (f32x2){mu0 + s0 * e0, mu1 + s1 * e1};
  const float d0 = a.x - mu0, d1 = a.y - mu1;
  const float l0 = (-(d0 * d0) / (2.0f * (s0 * s0)) - L.log_std[0]) - HALF_LOG_2PI;
  const float l1 = (-(d1 * d1) / (2.0f * (s1 * s1)) - L.log_std[1]) - HALF_LOG_2PI;
  logp = l0 + l1;
}
// tanhf as a call: inlined, its divergent branch (small / large |x|) cuts the unrolled activation loops into 16 (T1 + T2)
// blocks, the accumulators are copied out of the AGPRs wholesale and the 256-wide nets spill (52 dwords at <8, 8>, 134
// VGPRs at <2, 2>); called, <2, 2> holds 54 VGPRs + 32 AGPRs (5 waves per SIMD) and nothing spills
__device__ __attribute__((noinline)) float mlp_tanh(float x) { return tanhf(x); }
template <int ACT>
__device__ __forceinline__ float mlp_act(float v) { return ACT == MLP_RELU ? fmaxf(v, 0.0f) : mlp_tanh(v); }
template <int OUT>
__device__ __forceinline__ f32x2 mlp_out(float mu0, float mu1) {
  if (OUT == MLP_OUT_CLIP) return (f32x2){fminf(fmaxf(mu0, -1.0f), 1.0f), fminf(fmaxf(mu1, -1.0f), 1.0f)};
  if (OUT == MLP_OUT_SQUASH) {
    const float a0 = tanhf(mu0), a1 = tanhf(mu1);
    return (f32x2){-1.0f + ((0.5f * (a0 + 1.0f)) * 2.0f), -1.0f + ((0.5f * (a1 + 1.0f)) * 2.0f)};
  }
  return (f32x2){mu0, mu1};
}
// The explorer (policy 7, nascar_set_explorer): the two exploring epilogues of SB3's off-policy algorithms, on the
// Box-Muller pair of mlp_sample with salts of their own (EXPLORE_SALT0 / EXPLORE_SALT1, include/nascar.h) -- the draw
// depends on (seed, car, step) alone.  With scale(u) = 2 * ((u + 1) / 2) - 1 (scale_action, what the replay buffer keeps)
// and unscale(a) = -1 + (0.5 * (a + 1)) * 2 (unscale_action, what steps the env; mlp_out<MLP_OUT_SQUASH>'s expression):
//   MLP_OUT_SQUASH_SAMPLE  SquashedDiagGaussianDistribution, SAC's Actor with deterministic = False: m2 / m3 are the
//     log_std rows, ls = min(max(ls, -20), 2), g = mu + expf(ls) * eps, u = unscale(tanhf(g)), s = scale(u)
//   MLP_OUT_SQUASH with sigma  NormalActionNoise on a deterministic actor (TD3 / DDPG, OffPolicyAlgorithm._sample_action):
//     s = min(max(scale(u_det) + sigma * eps, -1), 1), u = unscale(s); sigma = 0 gives u_det back bit for bit
//     (scale and unscale are exact on an unscale's result)
#define EXPLORE_SALT0 0x4F46465F504F4C31ull
#define EXPLORE_SALT1 0x7F4A7C15D1B54A33ull
#define REPLAY_SALT_SLOT 0x5245504C5F534C54ull
#define REPLAY_SALT_CAR 0x2545F4914F6CDD1Dull
__device__ __forceinline__ float scale_action(float u) { return 2.0f * ((u + 1.0f) / 2.0f) - 1.0f; }
__device__ __forceinline__ float unscale_action(float a) { return -1.0f + ((0.5f * (a + 1.0f)) * 2.0f); }
__device__ __forceinline__ void mlp_explore(const MlpLaunch& L, const MlpDev& W, size_t car, float m0, float m1, float m2,
                                            float m3, f32x2& u, f32x2& s) {
  const uint64_t key = policy_key(L.seed, L.step, car);
  const float u0 = (float)((mix32(key ^ EXPLORE_SALT0) >> 8) + 1u) * (1.0f / 16777216.0f);
  const float u1 = (float)(mix32(key ^ EXPLORE_SALT1) >> 8) * (1.0f / 16777216.0f);
  const float r = sqrtf(-2.0f * logf(u0)), th = 6.283185307179586f * u1;
  const float e0 = r * cosf(th), e1 = r * sinf(th);
  const float mu0 = m0 + W.b3[0], mu1 = m1 + W.b3[1];
  if (W.output == MLP_OUT_SQUASH_SAMPLE) {   // wave-uniform
    const float l0 = fminf(fmaxf(m2 + W.b3[2], -20.0f), 2.0f), l1 = fminf(fmaxf(m3 + W.b3[3], -20.0f), 2.0f);
    const float g0 = mu0 + expf(l0) * e0, g1 = mu1 + expf(l1) * e1;
    u = (f32x2){unscale_action(tanhf(g0)), unscale_action(tanhf(g1))};
    s = (f32x2){scale_action(u.x), scale_action(u.y)};
  } else {
    const f32x2 d = mlp_out<MLP_OUT_SQUASH>(mu0, mu1);
    s = (f32x2){fminf(fmaxf(scale_action(d.x) + L.log_std[0] * e0, -1.0f), 1.0f),
                fminf(fmaxf(scale_action(d.y) + L.log_std[1] * e1, -1.0f), 1.0f)};
    u = (f32x2){unscale_action(s.x), unscale_action(s.y)};
  }
}
// MLP_OUT_CATEGORICAL: SB3's CategoricalDistribution over the five actions of the env's Discrete(5), sampled by an inverse
// CDF on one mix32 draw on the car's key (salt CAT_SALT, include/nascar.h): u in [0, 1).  With l the five logits,
//   m = max_j l_j (fmaxf, index order), e_j = expf(l_j - m), P_0 = e_0, P_j = P_{j-1} + e_j, S = P_4, t = u * S,
//   a = #{j in 0..3 : t >= P_j}   (category 4 is the fall-through: nothing is compared with P_4)
//   logp = (l_a - m) - logf(S)    Categorical(logits = l).log_prob(a)
// The draw depends on (seed, car, step) alone.  MLP_OUT_MODE: the first maximum of the logits (strict > in index order).
// Either index goes to the env as the pair of nascar_step's discrete path (model_block: _discrete_to_continuous).
#define CAT_SALT 0x4341545F44524157ull
__device__ __forceinline__ f32x2 discrete_pair(int a) {
  return (f32x2){a == 1 ? 1.0f : (a == 2 ? -1.0f : 0.0f), a == 3 ? -1.0f : (a == 4 ? 1.0f : 0.0f)};
}
__device__ __forceinline__ void mlp_categorical(const MlpLaunch& L, size_t car, const float (&l)[5], int& a, float& logp) {
  const float u = (float)(mix32(policy_key(L.seed, L.step, car) ^ CAT_SALT) >> 8) * (1.0f / 16777216.0f);
  float m = l[0];
#pragma unroll
  for (int j = 1; j < 5; ++j) m = fmaxf(m, l[j]);
  float d[5], P[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    d[j] = l[j] - m;
    P[j] = j ? P[j - 1] + expf(d[j]) : expf(d[j]);
  }
  const float t = u * P[4];
  a = 0;
  float da = d[0];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (t >= P[j]) { a = j + 1; da = d[j + 1]; }   // (P is non-decreasing: the passed thresholds are a prefix)
  logp = da - logf(P[4]);
}
__device__ __forceinline__ int mlp_mode(const float (&l)[5]) {
  int a = 0;
  float best = l[0];
#pragma unroll
  for (int j = 1; j < 5; ++j)
    if (l[j] > best) { best = l[j]; a = j; }
  return a;
}
// The epilogues of a five-sum head (the CAT instantiations of mlp_field_kernel, and mlp_wide_kernel): m the layer-3 sums
// after the lane-half add; a two-row controller's rows 2-4 were zeroed in LDS and its b3 [2] is read no further.
__device__ __forceinline__ void mlp_head5(const MlpLaunch& L, const MlpDev& W, size_t car, bool wanted, const float (&m)[5]) {
  const float mu0 = m[0] + W.b3[0], mu1 = m[1] + W.b3[1];
  f32x2* out = (f32x2*)&L.act[2 * car];
  switch (W.output) {   // wave-uniform
    case MLP_OUT_CATEGORICAL: case MLP_OUT_MODE: {
      const float l[5] = {mu0, mu1, m[2] + W.b3[2], m[3] + W.b3[3], m[4] + W.b3[4]};
      int a;
      if (W.output == MLP_OUT_CATEGORICAL) {
        float lp;
        mlp_categorical(L, car, l, a, lp);
        if (L.actions) ((int*)L.actions)[car] = a;
        if (L.logp) L.logp[car] = lp;
      } else {
        a = mlp_mode(l);
      }
      *out = discrete_pair(a);
      break;
    }
    case MLP_OUT_VALUE:
      if (wanted) L.values[car] = mu0;
      break;
    case MLP_OUT_SAMPLE: {
      f32x2 a; float lp;
      mlp_sample(L, car, mu0, mu1, a, lp);
      if (L.actions) *(f32x2*)&L.actions[2 * car] = a;
      if (L.logp) L.logp[car] = lp;
      *out = mlp_out<MLP_OUT_CLIP>(a.x, a.y);
      break;
    }
    case MLP_OUT_SQUASH: *out = mlp_out<MLP_OUT_SQUASH>(mu0, mu1); break;
    case MLP_OUT_CLIP: *out = mlp_out<MLP_OUT_CLIP>(mu0, mu1); break;
    default: *out = mlp_out<MLP_OUT_RAW>(mu0, mu1); break;
  }
}
// EXPL: the explorer's instantiations (policy 7), separate so that the others compile to what they were: a four-row w3 in
// LDS and four layer-3 sums (rows 2-3 zero for a two-row controller), and mlp_explore as the only epilogue.
// CAT: the five-row instantiations, separate for the same reason: a five-row w3 in LDS (rows 2-4 zero for a two-row
// controller: a critic or a Gaussian actor that shares the launch), five layer-3 sums and mlp_head5's epilogues.
template <int T1, int T2, int ACT, bool EXPL = false, bool CAT = false>
__global__ void __launch_bounds__(64 * AM_WAVES) mlp_field_kernel(MlpLaunch L) {
  constexpr int H1 = 32 * T1, H2 = 32 * T2;
  static_assert(!(EXPL && CAT), "one head kind per instantiation");
  __shared__ float s_b1[H1], s_b2[H2], s_w3[(EXPL ? 4 : CAT ? 5 : 2) * H2];
  const int c = L.slot_id[blockIdx.y] & 255;
  bool wanted = true;
  if (L.tflags) {   // timeout values: only the cars of envs that were truncated and not terminated at this step
    const int it = (blockIdx.x * AM_WAVES + (threadIdx.x >> 6)) * 32 + (threadIdx.x & 31);
    wanted = false;
    if (it < L.nenv) {
      const uint8_t f = L.tflags[((size_t)(L.env0 + it) * L.C + c) / L.tcars];
      wanted = (f & 2) && !(f & 1);
    }
    if (!__syncthreads_or(wanted)) return;   // block-uniform: nothing has been loaded yet
  }
  const MlpDev W = L.table[L.slot_id[blockIdx.y] >> 8];
  for (int i = threadIdx.x; i < H1; i += 64 * AM_WAVES) s_b1[i] = W.b1[i];
  for (int i = threadIdx.x; i < H2; i += 64 * AM_WAVES) s_b2[i] = W.b2[i];
  if (EXPL) {
    const int n3 = (W.output == MLP_OUT_SQUASH_SAMPLE ? 4 : 2) * H2;
    for (int i = threadIdx.x; i < 4 * H2; i += 64 * AM_WAVES) s_w3[i] = i < n3 ? W.w3[i] : 0.0f;
  } else if (CAT) {
    const int n3 = (W.output >= MLP_OUT_CATEGORICAL ? 5 : 2) * H2;
    for (int i = threadIdx.x; i < 5 * H2; i += 64 * AM_WAVES) s_w3[i] = i < n3 ? W.w3[i] : 0.0f;
  } else {
    for (int i = threadIdx.x; i < 2 * H2; i += 64 * AM_WAVES) s_w3[i] = W.w3[i];
  }
  __syncthreads();
  const int l = threadIdx.x & 63, r = l & 31, h = l >> 5;
  const int tile = blockIdx.x * AM_WAVES + (threadIdx.x >> 6);
  const int i0 = tile * 32;
  if (i0 >= L.nenv) return;
  if (L.tflags && !__any(wanted)) return;   // wave-uniform
  const int i = i0 + r;
  const size_t car = (size_t)(L.env0 + (i < L.nenv ? i : L.nenv - 1)) * L.C + c;
  const float* xr = L.obs + car * ACT_OBS;
  f32x16 hid[T1];   // layer-1 accumulators, then act(H1 + b1) in place: layer 2's B operands
#pragma unroll
  for (int t = 0; t < T1; ++t) hid[t] = (f32x16){};
#pragma unroll
  for (int s = 0; s < ACT_OBS / 2; ++s) {
    const float b = xr[2 * s + h];
    const float* w = W.w1t + (size_t)(2 * s + h) * H1 + r;
#pragma unroll
    for (int t = 0; t < T1; ++t) hid[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[32 * t], b, hid[t], 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < T1; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int u = 32 * t + (q & 3) + 8 * (q >> 2) + 4 * h;   // the 32x32 C/D map: register q of tile t on half h
      hid[t][q] = mlp_act<ACT>(hid[t][q] + s_b1[u]);
    }
  f32x16 acc[T2];
#pragma unroll
  for (int o = 0; o < T2; ++o) acc[o] = (f32x16){};
#pragma unroll
  for (int t = 0; t < T1; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int u = 32 * t + (q & 3) + 8 * (q >> 2) + 4 * h;
      const float* w = W.w2t + (size_t)u * H2 + r;
      const float b = hid[t][q];
#pragma unroll
      for (int o = 0; o < T2; ++o) acc[o] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[32 * o], b, acc[o], 0, 0, 0);
    }
  // layer 3: partial sums over this lane's half of the hidden units, then the two halves of the observation added
  float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f, m3 = 0.0f, m4 = 0.0f;
#pragma unroll
  for (int t = 0; t < T2; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int u = 32 * t + (q & 3) + 8 * (q >> 2) + 4 * h;
      const float v = mlp_act<ACT>(acc[t][q] + s_b2[u]);
      m0 = fmaf(s_w3[u], v, m0);
      m1 = fmaf(s_w3[H2 + u], v, m1);
      if (EXPL || CAT) {
        m2 = fmaf(s_w3[2 * H2 + u], v, m2);
        m3 = fmaf(s_w3[3 * H2 + u], v, m3);
      }
      if (CAT) m4 = fmaf(s_w3[4 * H2 + u], v, m4);
    }
  m0 += __shfl_xor(m0, 32);
  m1 += __shfl_xor(m1, 32);
  if (CAT) {
    m2 += __shfl_xor(m2, 32);
    m3 += __shfl_xor(m3, 32);
    m4 += __shfl_xor(m4, 32);
    if (h == 0 && i < L.nenv) mlp_head5(L, W, car, wanted, {m0, m1, m2, m3, m4});
    return;
  }
  if (EXPL) {
    m2 += __shfl_xor(m2, 32);
    m3 += __shfl_xor(m3, 32);
    if (h == 0 && i < L.nenv) {
      f32x2 u, s;
      mlp_explore(L, W, car, m0, m1, m2, m3, u, s);
      *(f32x2*)&L.act[2 * car] = u;
      if (L.actions) *(f32x2*)&L.actions[2 * car] = s;
    }
    return;
  }
  if (h == 0 && i < L.nenv) {
    const float mu0 = m0 + W.b3[0], mu1 = m1 + W.b3[1];
    f32x2* out = (f32x2*)&L.act[2 * car];
    switch (W.output) {   // wave-uniform
      case MLP_OUT_VALUE:
        if (wanted) L.values[car] = mu0;
        break;
      case MLP_OUT_SAMPLE: {
        f32x2 a; float lp;
        mlp_sample(L, car, mu0, mu1, a, lp);
        if (L.actions) *(f32x2*)&L.actions[2 * car] = a;
        if (L.logp) L.logp[car] = lp;
        *out = mlp_out<MLP_OUT_CLIP>(a.x, a.y);
        break;
      }
      case MLP_OUT_SQUASH: *out = mlp_out<MLP_OUT_SQUASH>(mu0, mu1); break;
      case MLP_OUT_CLIP: *out = mlp_out<MLP_OUT_CLIP>(mu0, mu1); break;
      default: *out = mlp_out<MLP_OUT_RAW>(mu0, mu1); break;
    }
  }
}

// ------------------------------------------------------------------ the wide MLP: 512-512 ReLU (learn/a2c.py's net_arch)
// mlp_field_kernel<T1, T2> keeps 16 (T1 + T2) accumulator registers: 512 at 16 + 16, the whole register file of a lane.
// mlp_wide_kernel holds the 16 layer-1 tiles (256 registers: layer 2's B operands) and runs layer 2 in chunks of TC output
// tiles, folding each chunk's layer-3 partial sums into the five sums before the next chunk reuses the accumulators.  The
// result is what a monolithic <16, 16> would compute: a chunk's accumulators see their k steps in the same order (t, then
// q), the bias is added after the accumulation, and the chunks are folded in ascending order, so each sum's fmaf chain
// runs over ascending u per lane half.  Addressing, the ragged last tile and the tflags early-out are mlp_field_kernel's.
// Heads: every epilogue of mlp_head5 (outputs 0-4, 6, 7); no explorer, no Tanh (tanhf as a call under ~330 live registers).
template <int T1, int T2, int TC>
__global__ void __launch_bounds__(64 * AM_WAVES) mlp_wide_kernel(MlpLaunch L) {
  constexpr int H1 = 32 * T1, H2 = 32 * T2;
  static_assert(T2 % TC == 0, "whole chunks");
  __shared__ float s_b1[H1], s_b2[H2], s_w3[5 * H2];
  const int c = L.slot_id[blockIdx.y] & 255;
  bool wanted = true;
  if (L.tflags) {   // timeout values: only the cars of envs that were truncated and not terminated at this step
    const int it = (blockIdx.x * AM_WAVES + (threadIdx.x >> 6)) * 32 + (threadIdx.x & 31);
    wanted = false;
    if (it < L.nenv) {
      const uint8_t f = L.tflags[((size_t)(L.env0 + it) * L.C + c) / L.tcars];
      wanted = (f & 2) && !(f & 1);
    }
    if (!__syncthreads_or(wanted)) return;   // block-uniform: nothing has been loaded yet
  }
  const MlpDev W = L.table[L.slot_id[blockIdx.y] >> 8];
  for (int i = threadIdx.x; i < H1; i += 64 * AM_WAVES) s_b1[i] = W.b1[i];
  for (int i = threadIdx.x; i < H2; i += 64 * AM_WAVES) s_b2[i] = W.b2[i];
  const int n3 = (W.output >= MLP_OUT_CATEGORICAL ? 5 : 2) * H2;   // a two-row head is not read past its rows
  for (int i = threadIdx.x; i < 5 * H2; i += 64 * AM_WAVES) s_w3[i] = i < n3 ? W.w3[i] : 0.0f;
  __syncthreads();
  const int l = threadIdx.x & 63, r = l & 31, h = l >> 5;
  const int tile = blockIdx.x * AM_WAVES + (threadIdx.x >> 6);
  const int i0 = tile * 32;
  if (i0 >= L.nenv) return;
  if (L.tflags && !__any(wanted)) return;   // wave-uniform
  const int i = i0 + r;
  const size_t car = (size_t)(L.env0 + (i < L.nenv ? i : L.nenv - 1)) * L.C + c;
  const float* xr = L.obs + car * ACT_OBS;
  f32x16 hid[T1];   // layer-1 accumulators, then relu(H1 + b1) in place: layer 2's B operands, live through every chunk
  // in two halves of T1 / 2 tiles (each tile's k order is unchanged): 16 T1 accumulators at once fill the accumulator
  // file, and their activation in place then costs spills
#pragma unroll
  for (int half = 0; half < 2; ++half) {
#pragma unroll
    for (int t = half * (T1 / 2); t < (half + 1) * (T1 / 2); ++t) hid[t] = (f32x16){};
#pragma unroll
    for (int s = 0; s < ACT_OBS / 2; ++s) {
      const float b = xr[2 * s + h];
      const float* w = W.w1t + (size_t)(2 * s + h) * H1 + r;
#pragma unroll
      for (int t = half * (T1 / 2); t < (half + 1) * (T1 / 2); ++t)
        hid[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[32 * t], b, hid[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = half * (T1 / 2); t < (half + 1) * (T1 / 2); ++t)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int u = 32 * t + (q & 3) + 8 * (q >> 2) + 4 * h;
        hid[t][q] = fmaxf(hid[t][q] + s_b1[u], 0.0f);
      }
    __builtin_amdgcn_sched_barrier(0);
  }
  float m[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
  for (int ch = 0; ch < T2 / TC; ++ch) {   // a real loop: one chunk's code (16 T1 TC MFMAs), not T2 / TC copies of it
    f32x16 acc[TC];
#pragma unroll
    for (int o = 0; o < TC; ++o) acc[o] = (f32x16){};
    // k step k = 16 t + q takes hid[t][q], hidden unit u(k), in mlp_field_kernel's order.  The A operands (W2^T rows,
    // L2-resident) are fetched one block of KB k steps ahead of their use, and nothing is scheduled across a block's end:
    // with hid filling the vector registers the scheduler left to itself hoists no load, and every k step waits a full
    // L2 latency (measured at 8192 x 10: collect 3.79 ms per step with the plain loop, 0.99 ms with this one; KB = 16
    // measured the same as 8)
    const float* wc = W.w2t + 32 * TC * ch + r;
    constexpr int KB = MLP_WIDE_KB, NB = 16 * T1 / KB;
#define WIDE_U(k) (32 * ((k) >> 4) + ((k) & 3) + 8 * (((k) & 15) >> 2) + 4 * h)
    float wn[KB * TC];
#pragma unroll
    for (int j = 0; j < KB; ++j)
#pragma unroll
      for (int o = 0; o < TC; ++o) wn[j * TC + o] = wc[(size_t)WIDE_U(j) * H2 + 32 * o];
#pragma unroll
    for (int blk = 0; blk < NB; ++blk) {
      float wcur[KB * TC];
#pragma unroll
      for (int j = 0; j < KB * TC; ++j) wcur[j] = wn[j];
      if (blk + 1 < NB) {
#pragma unroll
        for (int j = 0; j < KB; ++j)
#pragma unroll
          for (int o = 0; o < TC; ++o) wn[j * TC + o] = wc[(size_t)WIDE_U(KB * (blk + 1) + j) * H2 + 32 * o];
      }
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        const float b = hid[(KB * blk + j) >> 4][(KB * blk + j) & 15];
#pragma unroll
        for (int o = 0; o < TC; ++o) acc[o] = __builtin_amdgcn_mfma_f32_32x32x2f32(wcur[j * TC + o], b, acc[o], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#undef WIDE_U
#pragma unroll
    for (int o = 0; o < TC; ++o)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int u = 32 * (TC * ch + o) + (q & 3) + 8 * (q >> 2) + 4 * h;
        const float v = fmaxf(acc[o][q] + s_b2[u], 0.0f);
#pragma unroll
        for (int j = 0; j < 5; ++j) m[j] = fmaf(s_w3[j * H2 + u], v, m[j]);
      }
  }
#pragma unroll
  for (int j = 0; j < 5; ++j) m[j] += __shfl_xor(m[j], 32);
  if (h == 0 && i < L.nenv) mlp_head5(L, W, car, wanted, m);
}

// ------------------------------------------------------------------ GAE (nascar_gae, nascar_collect)
// Generalised advantage estimation over K records of N = E * C cars, one lane per car walking the records backwards
// (every load and store coalesced across cars), float32 throughout in the operation order of SB3's
// RolloutBuffer.compute_returns_and_advantage under NumPy 2 promotion (float32 arrays, Python-float gamma / lambda):
//   r' = reward + g * tv               g = (float)gamma; tv the time-limit bootstrap V(terminal obs), 0 elsewhere
//   nnt = 1 - done[k]                  done = terminated | truncated of the car's env (episode_starts[k + 1] == dones[k])
//   delta = (r' + (g * V[k+1]) * nnt) - V[k]
//   A[k] = delta + (gl * nnt) * A[k+1] gl = (float)((double)gamma * (double)lambda), A[K] = 0
//   returns[k] = A[k] + V[k]
// Built with -ffp-contract=off: no product is fused into a sum, so the result is reproducible bit for bit.
__global__ void __launch_bounds__(256) gae_kernel(int N, int C, int K, const float* __restrict__ reward,
                                                  const float* __restrict__ values, const float* __restrict__ tv,
                                                  const uint8_t* __restrict__ env_flags, float g, float gl,
                                                  float* __restrict__ adv, float* __restrict__ ret) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int E = N / C, env = n / C;
  float a = 0.0f, vnext = values[(size_t)K * N + n];
  for (int k = K - 1; k >= 0; --k) {
    const size_t at = (size_t)k * N + n;
    const float v = values[at];
    const float rp = reward[at] + g * tv[at];
    const float nnt = 1.0f - ((env_flags[(size_t)k * E + env] & 3) ? 1.0f : 0.0f);
    const float delta = (rp + (g * vnext) * nnt) - v;
    a = delta + (gl * nnt) * a;
    adv[at] = a;
    ret[at] = a + v;
    vnext = v;
  }
}

#define AF_TILE 32
__global__ void __launch_bounds__(256) actor_fp32_kernel(int N, const float* __restrict__ obs, float* __restrict__ act,
                                                         ActorF32 A) {
  __shared__ float4 xs[ACT_OBS][AF_TILE / 4];   // observations, [feature][row]
  __shared__ float4 hs[ACT_H][AF_TILE / 4];     // relu(H1) then relu(H2), [unit][row]
  const int t = threadIdx.x;
  const float b1 = A.b1[t], b2 = A.b2[t];
  for (int tile = blockIdx.x; tile * AF_TILE < N; tile += gridDim.x) {
    const int row0 = tile * AF_TILE;
    float* xf = (float*)xs;
    for (int i = t; i < AF_TILE * ACT_OBS; i += 256) {
      const int o = i / ACT_OBS, k = i - o * ACT_OBS;
      xf[k * AF_TILE + o] = row0 + o < N ? obs[(size_t)row0 * ACT_OBS + i] : 0.0f;
    }
    __syncthreads();
    float acc[AF_TILE];
#pragma unroll
    for (int o = 0; o < AF_TILE; ++o) acc[o] = 0.0f;
#pragma unroll 2
    for (int k = 0; k < ACT_OBS; ++k) {
      const float w = A.w1t[k * ACT_H + t];
#pragma unroll
      for (int q = 0; q < AF_TILE / 4; ++q) {
        const float4 x = xs[k][q];
        acc[4 * q] = fmaf(x.x, w, acc[4 * q]); acc[4 * q + 1] = fmaf(x.y, w, acc[4 * q + 1]);
        acc[4 * q + 2] = fmaf(x.z, w, acc[4 * q + 2]); acc[4 * q + 3] = fmaf(x.w, w, acc[4 * q + 3]);
      }
    }
#pragma unroll
    for (int q = 0; q < AF_TILE / 4; ++q)
      hs[t][q] = make_float4(fmaxf(acc[4 * q] + b1, 0.0f), fmaxf(acc[4 * q + 1] + b1, 0.0f),
                             fmaxf(acc[4 * q + 2] + b1, 0.0f), fmaxf(acc[4 * q + 3] + b1, 0.0f));
    __syncthreads();
#pragma unroll
    for (int o = 0; o < AF_TILE; ++o) acc[o] = 0.0f;
#pragma unroll 4
    for (int k = 0; k < ACT_H; ++k) {
      const float w = A.w2t[k * ACT_H + t];
#pragma unroll
      for (int q = 0; q < AF_TILE / 4; ++q) {
        const float4 x = hs[k][q];
        acc[4 * q] = fmaf(x.x, w, acc[4 * q]); acc[4 * q + 1] = fmaf(x.y, w, acc[4 * q + 1]);
        acc[4 * q + 2] = fmaf(x.z, w, acc[4 * q + 2]); acc[4 * q + 3] = fmaf(x.w, w, acc[4 * q + 3]);
      }
    }
    __syncthreads();   // every lane has read relu(H1)
#pragma unroll
    for (int q = 0; q < AF_TILE / 4; ++q)
      hs[t][q] = make_float4(fmaxf(acc[4 * q] + b2, 0.0f), fmaxf(acc[4 * q + 1] + b2, 0.0f),
                             fmaxf(acc[4 * q + 2] + b2, 0.0f), fmaxf(acc[4 * q + 3] + b2, 0.0f));
    __syncthreads();
    if (t < 2 * AF_TILE) {
      const int o = t >> 1, i = t & 1;
      const float* hf = (const float*)hs;
      float m = 0.0f;
      for (int k = 0; k < ACT_H; ++k) m = fmaf(A.w3[i * ACT_H + k], hf[k * AF_TILE + o], m);
      const float a = tanhf(m + A.b3[i]);
      if (row0 + o < N) act[2 * (size_t)(row0 + o) + i] = -1.0f + ((0.5f * (a + 1.0f)) * 2.0f);   // unscale_action
    }
    __syncthreads();   // xs / hs are reused by the next tile
  }
}

}  // namespace nascar
