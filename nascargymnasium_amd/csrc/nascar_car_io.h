// nascar_car_io.h -- load / store of one car between the SoA state arrays (nascar_layout.h) and struct Car: one field
// table (layout field, Car member, group), car_load, car_store and the staged subsets the step kernels use as
// compositions of its groups.  Needs nascar_params.h.
#pragma once
#include "nascar_params.h"

// ------------------------------------------------------------------ load / store of one car
// Every field of nascar_layout.h, in its order: (storage type, layout field, Car member, group).  A group is a set of
// fields the step kernels always move together; the functions below are unions of groups.
enum {
  G_BODY = 1,     // b2Body, its contact-list counts and the listener's count
  G_IMP = 2,      // CarCollisionListener impulse
  G_MODEL = 4,    // vehicle-model scalars
  G_BANK = 8,
  G_TYRES = 16,
  G_ACC = 32,     // acceleration-history ring position
  G_DIS = 64,
  G_LOGIC = 128,  // rewards, lap timer, CarEnv bookkeeping
  G_ALL = 255
};
#define CAR_F32_TABLE(X) \
  X(F32, cx, c.c.x, G_BODY) X(F32, cy, c.c.y, G_BODY) X(F32, a, c.a, G_BODY) \
  X(F32, vx, c.v.x, G_BODY) X(F32, vy, c.v.y, G_BODY) X(F32, w, c.w, G_BODY) \
  X(F32, qs, c.xf.q.s, G_BODY) X(F32, qc, c.xf.q.c, G_BODY) X(F32, xpx, c.xf.p.x, G_BODY) X(F32, xpy, c.xf.p.y, G_BODY) \
  X(F32, sleep, c.sleep, G_BODY) X(F32, invdt0, c.invdt0, G_BODY) \
  X(F32, flox, c.fat.lo.x, G_BODY) X(F32, floy, c.fat.lo.y, G_BODY) X(F32, fhix, c.fat.hi.x, G_BODY) X(F32, fhiy, c.fat.hi.y, G_BODY) \
  X(F32, cum_reward, c.cum_reward, G_LOGIC) X(F32, cum_reward_info, c.cum_reward_info, G_LOGIC)
#define CAR_F64_TABLE(X) \
  X(F64, rpm, c.rpm, G_MODEL) X(F64, pvx, c.pvx, G_MODEL) X(F64, pvy, c.pvy, G_MODEL) \
  X(F64, lfm, c.lfm, G_MODEL) X(F64, slip, c.slip, G_MODEL) X(F64, bank, c.bank, G_BANK) \
  X(F64, load0, c.load[0], G_TYRES) X(F64, load1, c.load[1], G_TYRES) X(F64, load2, c.load[2], G_TYRES) X(F64, load3, c.load[3], G_TYRES) \
  X(F64, temp0, c.temp[0], G_TYRES) X(F64, temp1, c.temp[1], G_TYRES) X(F64, temp2, c.temp[2], G_TYRES) X(F64, temp3, c.temp[3], G_TYRES) \
  X(F64, wear0, c.wear[0], G_TYRES) X(F64, wear1, c.wear[1], G_TYRES) X(F64, wear2, c.wear[2], G_TYRES) X(F64, wear3, c.wear[3], G_TYRES) \
  X(F64, imp, c.imp, G_IMP) \
  X(F64, lt_start, c.lt_start, G_LOGIC) X(F64, lt_cur, c.lt_cur, G_LOGIC) X(F64, lt_last, c.lt_last, G_LOGIC) \
  X(F64, lt_best, c.lt_best, G_LOGIC) X(F64, lt_px, c.lt_px, G_LOGIC) X(F64, lt_py, c.lt_py, G_LOGIC) X(F64, lt_dist, c.lt_dist, G_LOGIC) \
  X(F64, cum_impact, c.cum_impact, G_LOGIC) X(F64, stuck_dur, c.stuck_dur, G_LOGIC) \
  X(F64, stuck_sx, c.stuck_sx, G_LOGIC) X(F64, stuck_sy, c.stuck_sy, G_LOGIC) \
  X(F64, prev_px, c.prev_px, G_LOGIC) X(F64, prev_py, c.prev_py, G_LOGIC) \
  X(F64, prog_hist, c.prog_hist, G_LOGIC) X(F64, back, c.back, G_LOGIC) X(F64, prev_back, c.prev_back, G_LOGIC) \
  X(F64, imp_at_obs, c.imp_at_obs, G_LOGIC)
#define CAR_I32_TABLE(X) \
  X(I32, awake, c.awake, G_BODY) X(I32, nct, c.nct, G_BODY) X(I32, overflow, c.overflow, G_BODY) \
  X(I32, acc_len, c.acc_len, G_ACC) X(I32, acc_head, c.acc_head, G_ACC) \
  X(I32, imp_present, c.imp_present, G_IMP) X(I32, nact, c.nact, G_BODY) \
  X(I32, lt_timing, c.lt_timing, G_LOGIC) X(I32, lt_has_last, c.lt_has_last, G_LOGIC) X(I32, lt_has_best, c.lt_has_best, G_LOGIC) \
  X(I32, lt_crossed, c.lt_crossed, G_LOGIC) X(I32, lt_has_pos, c.lt_has_pos, G_LOGIC) X(I32, lt_laps, c.lt_laps, G_LOGIC) \
  X(I32, disabled, c.disabled, G_DIS) X(I32, has_stuck_start, c.has_stuck_start, G_LOGIC) \
  X(I32, first_step, c.first_step, G_LOGIC) X(I32, prev_laps, c.prev_laps, G_LOGIC)

// the tables list exactly the fields of NASCAR_*_FIELDS, in the same order: a field added to the layout without a row
// here (or a row out of place) fails the build.  A row's Car member and group are not checked here: a wrong one shows
// in the GPU state-parity tests (tests/test_gpu_state_parity.py)
#define CAR_ROW_ENUM(T, f, m, g) CAR_ROW_##T##_##f,
#define CAR_ROW_CHECK(T, f, m, g) \
  static_assert((int)CAR_ROW_##T##_##f == (int)T##_##f, "car field table: row " #f " is not at its nascar_layout.h index");
enum { CAR_F32_TABLE(CAR_ROW_ENUM) CAR_ROWS_F32 };
enum { CAR_F64_TABLE(CAR_ROW_ENUM) CAR_ROWS_F64 };
enum { CAR_I32_TABLE(CAR_ROW_ENUM) CAR_ROWS_I32 };
CAR_F32_TABLE(CAR_ROW_CHECK) CAR_F64_TABLE(CAR_ROW_CHECK) CAR_I32_TABLE(CAR_ROW_CHECK)
static_assert((int)CAR_ROWS_F32 == (int)N_F32 && (int)CAR_ROWS_F64 == (int)N_F64 && (int)CAR_ROWS_I32 == (int)N_I32,
              "car field table: row count differs from nascar_layout.h");

// the rows whose group is in MASK, in layout order (the statement order the hand-written lists had: the step kernels
// are tuned to their register budget with it)
template <int MASK>
__device__ __forceinline__ void car_load_groups(const Params& P, int n, Car& c) {
#define CAR_ROW_LOAD(T, f, m, g) if (MASK & (g)) m = T##P(P, f)[n];
  CAR_F32_TABLE(CAR_ROW_LOAD) CAR_F64_TABLE(CAR_ROW_LOAD) CAR_I32_TABLE(CAR_ROW_LOAD)
#undef CAR_ROW_LOAD
}
template <int MASK>
__device__ __forceinline__ void car_store_groups(const Params& P, int n, const Car& c) {
#define CAR_ROW_STORE(T, f, m, g) if (MASK & (g)) T##P(P, f)[n] = m;
  CAR_F32_TABLE(CAR_ROW_STORE) CAR_F64_TABLE(CAR_ROW_STORE) CAR_I32_TABLE(CAR_ROW_STORE)
#undef CAR_ROW_STORE
}
// the per-step members no array holds, set after a load that starts a car's step
__device__ __forceinline__ void car_init_step(const Params& P, int n, Car& c) {
  c.just_disabled = 0;
  c.force = zero2(); c.torque = 0.0f; c.c0 = c.c; c.a0 = c.a; c.alpha0 = 0.0f; c.moved = 0;
  c.ct = P.ct + (size_t)n * MAXC; c.act_key = P.act_key + (size_t)n * MAXC; c.act_n = P.act_n + (size_t)n * MAXC * 2;
  c.acc = nullptr;
}

__device__ inline void car_load(const Params& P, int n, Car& c) { car_load_groups<G_ALL>(P, n, c); car_init_step(P, n, c); }
__device__ inline void car_store(const Params& P, int n, const Car& c) { car_store_groups<G_ALL>(P, n, c); }

// Staged load/store for model_kernel: only the body, vehicle-model and listener fields are
// live through update_physics + the Box2D step; the model fields are written back right
// after update_physics (a compiler memory barrier stops the reload being forwarded) and the
// lap-timer / bookkeeping fields are loaded after the Box2D step.  Register pressure, not
// traffic, is what this buys (the re-read hits L2).
__device__ inline void car_load_phys(const Params& P, int n, Car& c) {
  car_load_groups<G_BODY | G_IMP | G_MODEL | G_BANK | G_TYRES | G_ACC | G_DIS>(P, n, c);
  car_init_step(P, n, c);
}
__device__ inline void car_store_model(const Params& P, int n, const Car& c) { car_store_groups<G_MODEL | G_TYRES | G_ACC>(P, n, c); }
__device__ inline void car_reload_tyres(const Params& P, int n, Car& c) { car_load_groups<G_TYRES>(P, n, c); }
__device__ inline void car_load_logic(const Params& P, int n, Car& c) { car_load_groups<G_LOGIC>(P, n, c); }

// model_kernel -> logic_kernel hand-off: the body / listener fields the Box2D step produced
__device__ inline void car_store_body(const Params& P, int n, const Car& c) { car_store_groups<G_BODY | G_IMP>(P, n, c); }
__device__ inline void car_load_body(const Params& P, int n, Car& c) {
  car_load_groups<G_BODY | G_IMP | G_DIS>(P, n, c);
  car_init_step(P, n, c);
}
// logic_kernel's write-back: every field but the vehicle-model ones (car_store_model) and the body
// ones only the model kernel changes
__device__ inline void car_store_logic(const Params& P, int n, const Car& c) {
  car_store_groups<G_LOGIC | G_BANK | G_IMP | G_DIS>(P, n, c);
}
