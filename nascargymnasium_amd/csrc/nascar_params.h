// nascar_params.h -- device-side tables of one track (DSeg, BeamGrid, TrackDev), the kernels' Params, the block-map
// helpers (blk_env_of, blk_track_of, blk_empty, wg_block, car_slot), beam_cell and the field pointer macros F32P /
// F64P / I32P. nascar_car_io.h and nascar_kernels.hip build on it: it switches fp contraction off and opens namespace
// nascar for what follows it. Needs nascar_device.h.
#pragma once
#include "nascar_device.h"

#pragma clang fp contract(off)

using namespace nascar;

#define MAX_SEG 64

#ifdef NASCAR_DEBUG
__device__ double* g_dbg = nullptr;   // debug build only: intermediate taps of one car
__device__ int g_dbg_car = -1;
#define DBG(n, slot, val) do { if ((n) == g_dbg_car && g_dbg) g_dbg[slot] = (double)(val); } while (0)
#else
#define DBG(n, slot, val) do { } while (0)
#endif


// ------------------------------------------------------------------ device-side tables
struct DSeg {   // per segment, float64 (src/track_generator.py TrackSegment)
  double sx, sy, ex, ey, width, banking, la, chord;  // la: banking lateral assist (src/car.py:527-533)
};
// Ray-candidate lists ("beams"), built on the host (build_beams): for every cell (nascar_set_beam_cell) near the
// walls and every one of BEAM_NB direction bins, the walls that a ray starting anywhere in the cell with a
// direction in the bin can reach within 250 m, sorted by a lower bound of their distance from the cell.
// Entry (16 bits) = bound code << wbits | wall index (wbits = 10 up to 1024 walls, up to 13 for 8192): code c stands
// for the bound c^2 * kq m, rounded down from the wall's exact bound (c < cmax = 2^(16 - wbits) - 1, the sentinel's
// code, past every hit), so the codes are conservative and ascend along a list.  A ray walks its list and stops at the first entry whose bound exceeds its best hit so far: the minimum exact
// fraction over the walls visited is the minimum over all walls, i.e. the reference's Box2D RayCast result.
#define BEAM_NB 256       // direction bins (measured 64: 44.2 us, 128: 41.7, 256: 38.7, 512: 39.1) (a multiple of 16: ray i is BEAM_NB / 16 bins from ray i + 1)
#define BEAM_STRIDE (BEAM_NB / 16)
// list slot of a bin: the 16 bins of one residue mod BEAM_STRIDE are adjacent, so a car's 16 rays read
// 16 adjacent lists
__host__ __device__ __forceinline__ int beam_slot(int bin) { return (bin % BEAM_STRIDE) * 16 + bin / BEAM_STRIDE; }
__host__ __device__ __forceinline__ int beam_bin(int slot) { return (slot % 16) * BEAM_STRIDE + slot / 16; }
#define BEAM_MAX_WALL_BITS 13                  // tracks with more than 8192 walls get no lists (the wall-group walk)
#define BEAM_PAD 0xFFFFu                       // sentinel: the largest code, stops every walk
#define BEAM_CONT_MAX 0xFFFFu                  // continuation entries of one cell (16-bit offsets from the cell's base)
struct BeamGrid {
  float ox, oy, inv_cell; int nx, ny;
  uint32_t wbits, wmask, cmax; float kq;   // entry layout: wall index bits, their mask, sentinel code, bound scale (m)
  // the cell map in chunks of BEAM_CHUNK cells along x, [ny][nxc]: (first list of the chunk's first built cell = its
  // id * BEAM_NB, the chunk's first ent[] index, the mask of its built cells, 0) -- the built cells of a chunk have
  // consecutive ids, so a cell's list base is the chunk's plus BEAM_NB per built cell below it.  ~0.5 MB per track
  // (a dense int2 per cell was ~9 MB, a random 128-byte line per car that no L2 held; this table stays cached)
  const int4* chunk; int nxc;
  const uint16_t* ent;      // list continuations, each closed by a BEAM_PAD sentinel
  // [built cells * BEAM_NB] 8-byte head records: the first BEAM_HEAD entries of each list (padded with BEAM_PAD) and
  // the offset + 1 of the list's continuation from its chunk's first ent[] index (0: none), so a walk starts with one
  // 8-byte load and reads the rest in chunks of RAY_CHUNK entries up to the sentinel.  (Round 5's 16-byte heads held
  // three 32-bit entries and an absolute index: 256 B of heads per car and step against 128.)
  const uint2* head;
};
#define BEAM_HEAD 3
#define RAY_CHUNK 4    // list entries past the head requested together
// an entry's distance bound in m (the sentinel's: beyond every hit) and its wall
__device__ __forceinline__ float beam_bound(const BeamGrid& G, uint32_t v) {
  const uint32_t c = v >> G.wbits;
  return c >= G.cmax ? 1e30f : (float)(c * c) * G.kq;
}
__device__ __forceinline__ int beam_wall(const BeamGrid& G, uint32_t v) { return (int)(v & G.wmask); }
// a walk goes on past an entry while its bound is within the best hit (fraction bi of the 250 m ray), with margin
__device__ __forceinline__ bool beam_beyond(const BeamGrid& G, uint32_t v, float bi) {
  return beam_bound(G, v) > bi * 250.0f * 1.00001f + 0.01f;
}
#define BEAM_CHUNK 32
struct BeamHead { uint2 w; uint32_t cb; };   // the head record and its chunk's first ent[] index
__device__ __forceinline__ BeamHead beam_head(const BeamGrid& G, int2 cell, int li) {
  BeamHead h;
  h.w = ldg(G.head + li);
  h.cb = (uint32_t)cell.y;
  return h;
}
#define LDS_PER_CU ((size_t)160 * 1024)   // gfx950: 160 KiB of LDS per CU, all of which one workgroup may declare
struct TrackDev {
  LWall* walls; int nwall;
  const float4* wfat;  // [nwall] broadphase fat AABBs
  DSeg* segs; int nseg;
  double* prefix;      // cumulative chord length before segment k (src/car_env.py:1593-1600)
  double total_length; int startline; int has_banking;
  WallGrid bp, sn;
  const float4* groups; int ngroup;   // sensor wall groups: (cx, cy, radius incl. margin, first | count << 16)
  const float4* swall;                // [2 * nwall] sensor image: (px, py, rad + 0.25, hx), (qs, qc, hy, 0)
  BeamGrid beam;                      // per (cell, direction bin) candidate walls of one ray (ray_sensor_kernel)
};

struct Params {
  int E, C, N, epb, nblocks, reset_on_lap;
  float dt_f; double dt_d; float friction;
  double start_x, start_y; float start_angle;
  float* f32; double* f64; int* i32; double* acc;
  DContact* ct; int* act_key; float* act_n;
  double* env_time; int* env_i32;
  const int* blk_track; const int* blk_env;
  const TrackDev* tracks;
  float4* pose;        // [2][N] sensor hand-off: (x, y, angle, mode) -- see sensor_kernel
  // [E] this step's auto-reset envs (the logic writes every env's byte): the step's sensor passes read an env's pass-B
  // pose only when its byte is set, so the pass-B records of the other cars are neither cleared nor read every step
  uint8_t* reset_env;
  double2* pose_cs;    // [2][N] cos, sin of (double)angle for the ray end points (computed once per car)
  const double2* ray_cs;   // [16] cos, sin of the ray offsets radians(22.5 i) (nascar_rays.h)
  double* ctl;         // [N][4] rule-driver state of the device action sources (policy_car)
  float* vhist;        // [VH_RING][N] speed history for validate_performance, or null (nascar_set_perf_history)
  int car_contact;     // build-only extension (nascar_set_car_contact): car-car contact inside each env; 0 = reference
  // block map shortcuts (prepare()): map_identity = blk_env[s] is s (< E) or -1, one_track >= 0 = every
  // block's track; they spare each kernel's first dependent load
  int map_identity, one_track;
  int blk0;            // first step-kernel workgroup of this launch (sharded rollout, nascar_set_rollout_streams); else 0
};
__device__ __forceinline__ int blk_env_of(const Params& P, int el, int s) {
  if (el >= P.epb) return -1;
  if (P.map_identity) return s < P.E ? s : -1;
  return P.blk_env[s];
}
__device__ __forceinline__ int blk_track_of(const Params& P, int b) { return P.one_track >= 0 ? P.one_track : P.blk_track[b]; }
// a workgroup of no track: the device-built block map's workgroups past the last track's (random-track mode); every
// kernel returns first for them (never taken with the host-built map, whose workgroups all hold envs)
__device__ __forceinline__ bool blk_empty(const Params& P, int b) { return P.one_track < 0 && P.blk_track[b] < 0; }
// The step kernels' workgroup (block-map index) of this dispatch slot.  The dispatcher deals a launch's workgroups
// round-robin over the 8 XCDs (slot b on XCD b % 8), each with its own L2; remapped here, each XCD takes a contiguous
// run of the launch's workgroups instead, so the state cache lines two neighbouring workgroups share (a workgroup's
// SoA run of cars rarely ends on a 128-B line) are fetched into one L2, not two.
__device__ __forceinline__ int wg_block(const Params& P) {
  const int nb = gridDim.x, b = blockIdx.x, q = nb >> 3, r = nb & 7, x = b & 7;
  return P.blk0 + x * q + min(x, r) + (b >> 3);
}
// This lane's car in the one-lane-per-car kernels, for workgroup (block-map index) b: its env of the block (el), car of
// the env, env (-1: none) and car index n (0 without an env)
struct CarSlot { int tid, el, car, env, n; };
__device__ __forceinline__ CarSlot car_slot(const Params& P, int b) {
  CarSlot r;
  r.tid = threadIdx.x;
  r.el = r.tid / P.C; r.car = r.tid - r.el * P.C;
  r.env = blk_env_of(P, r.el, b * P.epb + r.el);
  r.n = r.env >= 0 ? r.env * P.C + r.car : 0;
  return r;
}
// BeamGrid record of the cell holding (x, y): (list base = built cell id * BEAM_NB, its chunk's first ent[] index);
// list base -1 outside the built cells
__device__ __forceinline__ int2 beam_cell(const BeamGrid& G, float x, float y) {
  const float fx = (x - G.ox) * G.inv_cell, fy = (y - G.oy) * G.inv_cell;
  if (!(fx >= 0.0f && fy >= 0.0f && fx < (float)G.nx && fy < (float)G.ny)) return make_int2(-1, 0);
  const int cx = (int)fx;
  const int4 ch = ldg(G.chunk + (int)fy * G.nxc + cx / BEAM_CHUNK);
  const uint32_t bit = 1u << (cx % BEAM_CHUNK), m = (uint32_t)ch.z;
  if (!(m & bit)) return make_int2(-1, 0);
  return make_int2(ch.x + __popc(m & (bit - 1u)) * BEAM_NB, ch.y);
}

#define F32P(P, f) ((P).f32 + (size_t)F32_##f * (P).N)
#define F64P(P, f) ((P).f64 + (size_t)F64_##f * (P).N)
#define I32P(P, f) ((P).i32 + (size_t)I32_##f * (P).N)
