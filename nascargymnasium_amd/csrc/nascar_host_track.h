// nascar_host_track.h -- the host side of one track: its tables built from the segment and wall arrays (wall grids,
// beam lists, wall groups), their upload, the process-wide cache of built tracks and the track files of the disk
// cache.  Host code only; included by nascar_kernels.hip after the kernels (it needs fail / HIPCHK, the device structs
// and, for sensor_lds_reserve, the sensor and rollout kernels).
#pragma once

struct HostGrid {
  WallGrid g{};
  std::vector<int> start; std::vector<uint16_t> idx;
  int* d_start = nullptr; uint16_t* d_idx = nullptr;
  std::vector<float4> box; float4* d_box = nullptr;
};
// host-side wall record: the device's LWall plus the values only the host builders use
struct HWall : LWall {
  float rad;                 // bounding radius + culling margin (sensor wall image)
  float flx, fly, fhx, fhy;  // broadphase fat AABB
};
struct HostTrack {
  std::vector<HWall> walls; std::vector<DSeg> segs; std::vector<double> prefix;
  double total_length; int startline, has_banking;
  LWall* d_walls = nullptr; float4* d_wfat = nullptr; DSeg* d_segs = nullptr; double* d_prefix = nullptr;
  HostGrid bp, sn;
  struct {
    BeamGrid g{};
    std::vector<int4> chunk; std::vector<uint16_t> ent; std::vector<uint2> head;
    int4* d_chunk = nullptr; uint16_t* d_ent = nullptr; uint2* d_head = nullptr;
    int nxc = 0;
    size_t entries = 0, nlist = 0, dropped = 0;   // dropped: cells whose continuations overflow the 16-bit offsets
    double build_s = 0.0;
  } beam;
  std::vector<float4> groups; float4* d_groups = nullptr;
  float4* d_swall = nullptr;
};

// Wall grids (see WallGrid in nascar_device.h).  Conservative by construction: the
// broadphase list of a cell holds every wall whose fat AABB overlaps the cell grown by
// reach (+5 cm); the sensor list every wall whose culling circle (rad + 0.25 m) comes
// within 251 m of the cell, nearest first.
static const float BP_CELL = 4.0f, BP_REACH = 7.0f, SN_CELL = 16.0f, SN_PAD = 20.0f;
static const double SN_GROUP_R = 12.0; static const int SN_GROUP_N = 8;
static void build_grids(HostTrack& t) {
  double lx = 1e30, ly = 1e30, hx = -1e30, hy = -1e30;
  for (auto& w : t.walls) { lx = std::min(lx, (double)w.flx); ly = std::min(ly, (double)w.fly);
                            hx = std::max(hx, (double)w.fhx); hy = std::max(hy, (double)w.fhy); }
  auto setup = [&](HostGrid& G, float cell, float pad, float reach) {
    G.g.ox = (float)(lx - pad); G.g.oy = (float)(ly - pad); G.g.inv_cell = 1.0f / cell; G.g.reach = reach;
    G.g.nx = (int)std::ceil((hx + pad - G.g.ox) / cell) + 1; G.g.ny = (int)std::ceil((hy + pad - G.g.oy) / cell) + 1;
    G.start.assign((size_t)G.g.nx * G.g.ny + 1, 0);
  };
  setup(t.bp, BP_CELL, BP_REACH + 4.0f, BP_REACH);
  setup(t.sn, SN_CELL, SN_PAD, 0.0f);
  const int nw = (int)t.walls.size();
  for (int cy = 0; cy < t.bp.g.ny; ++cy)
    for (int cx = 0; cx < t.bp.g.nx; ++cx) {
      const double x0 = t.bp.g.ox + (double)cx * BP_CELL - BP_REACH - 0.05, x1 = t.bp.g.ox + (double)(cx + 1) * BP_CELL + BP_REACH + 0.05;
      const double y0 = t.bp.g.oy + (double)cy * BP_CELL - BP_REACH - 0.05, y1 = t.bp.g.oy + (double)(cy + 1) * BP_CELL + BP_REACH + 0.05;
      t.bp.start[(size_t)cy * t.bp.g.nx + cx] = (int)t.bp.idx.size();
      for (int j = 0; j < nw; ++j) {
        const HWall& w = t.walls[j];
        if (w.flx > x1 || w.fhx < x0 || w.fly > y1 || w.fhy < y0) continue;
        t.bp.idx.push_back((uint16_t)j);
        t.bp.box.push_back(make_float4(w.flx, w.fly, w.fhx, w.fhy));
      }
    }
  t.bp.start.back() = (int)t.bp.idx.size();
  for (int k = 0; k < std::max(BP_BATCH, 1); ++k) t.bp.box.push_back(make_float4(1e30f, 1e30f, -1e30f, -1e30f));
  // sensor wall groups: runs of consecutive walls (index order follows each boundary through
  // the curves) whose corners fit in a circle of radius <= SN_GROUP_R, at most SN_GROUP_N walls
  {
    auto corners = [&](int j, double* xs, double* ys) {
      const LWall& w = t.walls[j];
      const float vx[4] = {-w.hx, w.hx, w.hx, -w.hx}, vy[4] = {-w.hy, -w.hy, w.hy, w.hy};
      for (int i = 0; i < 4; ++i) { xs[i] = (w.qc * vx[i] - w.qs * vy[i]) + w.px; ys[i] = (w.qs * vx[i] + w.qc * vy[i]) + w.py; }
    };
    auto circle = [&](int first, int count, double& cx, double& cy) {
      double lx = 1e30, ly = 1e30, ux = -1e30, uy = -1e30, xs[4], ys[4];
      for (int j = first; j < first + count; ++j) {
        corners(j, xs, ys);
        for (int i = 0; i < 4; ++i) { lx = std::min(lx, xs[i]); ux = std::max(ux, xs[i]); ly = std::min(ly, ys[i]); uy = std::max(uy, ys[i]); }
      }
      cx = 0.5 * (lx + ux); cy = 0.5 * (ly + uy);
      double r = 0.0;
      for (int j = first; j < first + count; ++j) {
        corners(j, xs, ys);
        for (int i = 0; i < 4; ++i) r = std::max(r, std::hypot(xs[i] - cx, ys[i] - cy));
      }
      return r;
    };
    t.groups.clear();
    int first = 0;
    while (first < nw) {
      int count = 1;
      while (first + count < nw && count < SN_GROUP_N) {
        double cx, cy;
        if (circle(first, count + 1, cx, cy) > SN_GROUP_R) break;
        ++count;
      }
      double cx, cy, r = circle(first, count, cx, cy);
      const int packed = first | (count << 16);
      float pf; memcpy(&pf, &packed, sizeof pf);
      t.groups.push_back(make_float4((float)cx, (float)cy, (float)(r + 0.3), pf));
      first += count;
    }
  }
  std::vector<std::pair<double, int>> cand;
  const int ng = (int)t.groups.size();
  for (int cy = 0; cy < t.sn.g.ny; ++cy)
    for (int cx = 0; cx < t.sn.g.nx; ++cx) {
      const double x0 = t.sn.g.ox + (double)cx * SN_CELL, x1 = x0 + SN_CELL;
      const double y0 = t.sn.g.oy + (double)cy * SN_CELL, y1 = y0 + SN_CELL;
      const double mx = 0.5 * (x0 + x1), my = 0.5 * (y0 + y1);
      t.sn.start[(size_t)cy * t.sn.g.nx + cx] = (int)t.sn.idx.size();
      cand.clear();
      for (int g = 0; g < ng; ++g) {
        const float4 G = t.groups[g];
        const double dx = std::max(std::max(x0 - G.x, 0.0), G.x - x1), dy = std::max(std::max(y0 - G.y, 0.0), G.y - y1);
        if (std::sqrt(dx * dx + dy * dy) > 251.0 + G.z) continue;
        cand.push_back({std::hypot(G.x - mx, G.y - my) - G.z, g});
      }
      std::sort(cand.begin(), cand.end());
      for (auto& c : cand) t.sn.idx.push_back((uint16_t)c.second);
    }
  t.sn.start.back() = (int)t.sn.idx.size();
}
// Beam lists (BeamGrid).  Cells of `cell` m (BEAM_CELL_M by default) over the walls' extent; a cell gets lists when its centre is
// within (largest half width + BEAM_BAND) of a wall centre line -- the corridor and a band outside each wall.
// Per cell (centre c, disk radius rc = half diagonal + 5 cm) and wall j (centre line AB, capsule radius
// rr = half thickness + 10 cm, which holds the box and the f32 rounding of the device's ray cast):
//  * lb = dist(c, AB) - rr - rc bounds the distance from any ray origin in the cell to any point of the box;
//    walls with lb > 251 m are out of the 250 m ray's reach;
//  * the directions from the disk to the capsule lie in the arc between the directions from c to A and to
//    B, widened by asin((rr + rc) / dist(c, AB)) (all bins when c is inside the grown capsule), plus a
//    2e-3 rad guard for the f32 ray end points; every bin that arc touches lists the wall.
// Both are conservative, so the walk in ray_sensor_kernel visits every wall that can be the first hit.
// Cell size: the cell's disk widens every wall's angular arc and lowers its distance bound, so smaller cells give
// shorter walks (steady-state sensor tails; bench step 191 -> 178 / 174 / 168 / 167 us at 2 / 1.5 / 1 / 0.75 m,
// round 4) at 0.2-0.5 GB of lists per track at 1 m (8-byte heads + sentinel-terminated continuations).
#define BEAM_CELL_M 1.0f
#define BEAM_CELL_MIN 0.5f    // nascar_set_beam_cell range (heads: cell count x 4 KB; walks: longer above ~2 m)
#define BEAM_CELL_MAX 8.0f
static const double BEAM_BAND = 8.0;
static void build_beams(HostTrack& t, const float cell) {
  auto t0 = std::chrono::steady_clock::now();
  auto& B = t.beam;
  const int nw = (int)t.walls.size();
  std::vector<double> ax(nw), ay(nw), bx(nw), by(nw), rr(nw);
  double lx = 1e30, ly = 1e30, ux = -1e30, uy = -1e30, hwmax = 0.0;
  for (int j = 0; j < nw; ++j) {
    const LWall& w = t.walls[j];
    const double ex = (double)w.hx * w.qc, ey = (double)w.hx * w.qs;
    ax[j] = w.px - ex; ay[j] = w.py - ey; bx[j] = w.px + ex; by[j] = w.py + ey;
    rr[j] = (double)w.hy + 0.1;
    lx = std::min({lx, ax[j], bx[j]}); ux = std::max({ux, ax[j], bx[j]});
    ly = std::min({ly, ay[j], by[j]}); uy = std::max({uy, ay[j], by[j]});
  }
  for (auto& s : t.segs) hwmax = std::max(hwmax, s.width / 2.0);
  const double D = hwmax + BEAM_BAND, pad = D + 2.0 * cell;
  B.g.ox = (float)(lx - pad); B.g.oy = (float)(ly - pad); B.g.inv_cell = 1.0f / cell;
  B.g.nx = (int)std::ceil((ux + pad - B.g.ox) / cell) + 1;
  B.g.ny = (int)std::ceil((uy + pad - B.g.oy) / cell) + 1;
  const int nx = B.g.nx, ny = B.g.ny;
  auto segdist = [&](int j, double x, double y) {
    const double sx = bx[j] - ax[j], sy = by[j] - ay[j], ll = sx * sx + sy * sy;
    double tt = ll > 0 ? ((x - ax[j]) * sx + (y - ay[j]) * sy) / ll : 0.0;
    tt = std::min(1.0, std::max(0.0, tt));
    return std::hypot(x - (ax[j] + tt * sx), y - (ay[j] + tt * sy));
  };
  auto centre = [&](int cx, int cy, double& x, double& y) {
    x = (double)B.g.ox + (cx + 0.5) * (double)cell; y = (double)B.g.oy + (cy + 0.5) * (double)cell;
  };
  // cells near a wall
  std::vector<uint8_t> mark((size_t)nx * ny, 0);
  for (int j = 0; j < nw; ++j) {
    const int x0 = std::max(0, (int)std::floor((std::min(ax[j], bx[j]) - D - B.g.ox) / cell) - 1);
    const int x1 = std::min(nx - 1, (int)std::floor((std::max(ax[j], bx[j]) + D - B.g.ox) / cell) + 1);
    const int y0 = std::max(0, (int)std::floor((std::min(ay[j], by[j]) - D - B.g.oy) / cell) - 1);
    const int y1 = std::min(ny - 1, (int)std::floor((std::max(ay[j], by[j]) + D - B.g.oy) / cell) + 1);
    for (int cy = y0; cy <= y1; ++cy)
      for (int cx = x0; cx <= x1; ++cx) {
        double x, y;
        centre(cx, cy, x, y);
        if (segdist(j, x, y) <= D) mark[(size_t)cy * nx + cx] = 1;
      }
  }
  // entry layout: 10 wall bits up to 1024 walls (6-bit codes of c^2 / 16 m), then one more per doubling; the code scale
  // keeps the largest non-sentinel code near 240 m (a 250 m ray)
  uint32_t wb = 10;
  while (wb < BEAM_MAX_WALL_BITS && nw > (1 << wb)) ++wb;
  B.g.wbits = wb; B.g.wmask = (1u << wb) - 1u; B.g.cmax = (1u << (16 - wb)) - 1u;
  B.g.kq = (float)(0.0625 * std::pow(62.0 / (double)(B.g.cmax - 1), 2.0));
  std::vector<int> cells;   // the marked cells, row-major
  if (nw <= (1 << BEAM_MAX_WALL_BITS))   // (more walls than the entries address: no lists, the wall-group walk)
    for (size_t k = 0; k < mark.size(); ++k)
      if (mark[k]) cells.push_back((int)k);
  const int ncell = (int)cells.size();
  const double rc = cell * 0.70710678 + 0.05, two_pi = 2.0 * M_PI, dbin = two_pi / BEAM_NB;
  std::vector<std::vector<uint32_t>> lists((size_t)ncell * BEAM_NB);
  auto work = [&](int c0, int c1) {
    for (int ci = c0; ci < c1; ++ci) {
      double x, y;
      centre(cells[ci] % nx, cells[ci] / nx, x, y);
      std::vector<uint32_t>* L = &lists[(size_t)ci * BEAM_NB];
      for (int j = 0; j < nw; ++j) {
        const double d = segdist(j, x, y), R = rr[j] + rc, lb = d - R;
        if (lb > 251.0) continue;
        const uint32_t q = (uint32_t)std::min(65535.0, std::floor(std::max(lb, 0.0) * 100.0));
        const uint32_t e = (q << 16) | (uint32_t)j;
        if (d <= R * 1.0001 + 1e-3) { for (int k = 0; k < BEAM_NB; ++k) L[k].push_back(e); continue; }
        const double aA = std::atan2(ay[j] - y, ax[j] - x), aB = std::atan2(by[j] - y, bx[j] - x);
        double dl = aB - aA;
        while (dl > M_PI) dl -= two_pi;
        while (dl <= -M_PI) dl += two_pi;
        const double a0 = dl >= 0 ? aA : aB, span = std::fabs(dl);
        const double wid = std::asin(std::min(1.0, R / d)) + 2e-3;
        const long k0 = (long)std::floor((a0 - wid) / dbin), k1 = (long)std::floor((a0 + span + wid) / dbin);
        if (k1 - k0 + 1 >= BEAM_NB) { for (int k = 0; k < BEAM_NB; ++k) L[k].push_back(e); continue; }
        for (long k = k0; k <= k1; ++k) L[((k % BEAM_NB) + BEAM_NB) % BEAM_NB].push_back(e);
      }
      for (int k = 0; k < BEAM_NB; ++k) std::sort(L[k].begin(), L[k].end());
    }
  };
  const int nth = std::max(1, std::min(16, (int)std::thread::hardware_concurrency()));
  std::vector<std::thread> th;
  for (int k = 0; k < nth; ++k) th.emplace_back(work, (int)((long)ncell * k / nth), (int)((long)ncell * (k + 1) / nth));
  for (auto& x : th) x.join();
  // 16-bit entries: the bound code c = floor(sqrt(bound / kq)), so c^2 kq <= the wall's bound (rounded down again where
  // the double sqrt rounded up onto an integer), at most cmax - 1; each list sorted by entry, so the codes ascend
  const uint32_t cmax = B.g.cmax;
  const double kq = (double)B.g.kq;
  auto code_of = [&](uint32_t e) {
    const double lb = (double)(e >> 16) * 0.01;   // the cm bound, itself rounded down
    int c = (int)std::min<double>((double)cmax - 1.0, std::floor(std::sqrt(lb / kq)));
    while (c > 0 && (double)(c * c) * kq > lb) --c;
    return (uint16_t)(((uint32_t)c << wb) | (e & 0xFFFFu));
  };
  // per list (cell-major, slot order, beam_slot): the head record holds its first BEAM_HEAD entries (BEAM_PAD filled)
  // and, when the list is longer, 1 + the offset of its continuation -- the remaining entries followed by one BEAM_PAD
  // sentinel, so a walk needs no list end -- from its chunk's first ent[] index.  ent[0] is a sentinel; BEAM_COOP_PAD
  // sentinels close the array (the chunked and the wave-cooperative walks read past a list's sentinel).  A cell whose
  // continuations would overflow its chunk's 16-bit offsets keeps no lists (its rays take the wall-group walk).
  B.nxc = (nx + BEAM_CHUNK - 1) / BEAM_CHUNK;
  B.chunk.assign((size_t)B.nxc * ny, make_int4(-1, 0, 0, 0));
  std::vector<uint8_t> keep(ncell, 1);
  B.dropped = 0;
  for (int c0 = 0, c1; c0 < ncell; c0 = c1) {   // cells of one chunk: consecutive in row-major order
    const int key = cells[c0] / nx * B.nxc + cells[c0] % nx / BEAM_CHUNK;
    for (c1 = c0; c1 < ncell && cells[c1] / nx * B.nxc + cells[c1] % nx / BEAM_CHUNK == key; ++c1) {}
    size_t used = 0;
    for (int ci = c0; ci < c1; ++ci) {
      size_t cont = 0;
      for (int slot = 0; slot < BEAM_NB; ++slot) {
        const size_t len = lists[(size_t)ci * BEAM_NB + slot].size();
        if (len > (size_t)BEAM_HEAD) cont += len - BEAM_HEAD + 1;
      }
      if (used + cont >= BEAM_CONT_MAX) { keep[ci] = 0; ++B.dropped; } else used += cont;
    }
  }
  const size_t nkept = (size_t)ncell - B.dropped, nlist = nkept * BEAM_NB;
  B.head.assign(nlist, make_uint2(BEAM_PAD | (BEAM_PAD << 16), BEAM_PAD));
  B.ent.assign(1, (uint16_t)BEAM_PAD);
  B.entries = 0;
  std::vector<uint16_t> L16;
  int id = 0, cur = -1;
  size_t cb = 0;
  for (int ci = 0; ci < ncell; ++ci) {
    if (!keep[ci]) continue;
    const int cx = cells[ci] % nx, cy = cells[ci] / nx, key = cy * B.nxc + cx / BEAM_CHUNK;
    int4& ch = B.chunk[key];
    if (key != cur) { cur = key; cb = B.ent.size(); ch = make_int4(id * BEAM_NB, (int)cb, 0, 0); }
    ch.z = (int)((uint32_t)ch.z | (1u << (cx % BEAM_CHUNK)));
    for (int slot = 0; slot < BEAM_NB; ++slot) {
      const auto& L = lists[(size_t)ci * BEAM_NB + beam_bin(slot)];
      B.entries += L.size();
      L16.resize(L.size());
      for (size_t k = 0; k < L.size(); ++k) L16[k] = code_of(L[k]);
      std::sort(L16.begin(), L16.end());
      uint32_t h[4];
      for (int k = 0; k < BEAM_HEAD; ++k) h[k] = (size_t)k < L16.size() ? L16[k] : BEAM_PAD;
      h[3] = 0u;
      if (L16.size() > (size_t)BEAM_HEAD) {
        h[3] = (uint32_t)(B.ent.size() - cb) + 1u;
        B.ent.insert(B.ent.end(), L16.begin() + BEAM_HEAD, L16.end());
        B.ent.push_back((uint16_t)BEAM_PAD);
      }
      B.head[(size_t)id * BEAM_NB + slot] = make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
    }
    ++id;
  }
  for (int k = 0; k < (RAY_CHUNK > BEAM_COOP_PAD ? RAY_CHUNK : BEAM_COOP_PAD); ++k) B.ent.push_back((uint16_t)BEAM_PAD);
  if (getenv("NASCAR_VERBOSE"))
    fprintf(stderr, "build_beams: %d walls (%u-bit wall indices, bound codes of %.4f m x c^2), %d cells with lists, %zu "
            "dropped (continuation offsets), %zu entries, heads %.1f MB + continuations %.1f MB\n", nw, B.g.wbits,
            (double)B.g.kq, ncell - (int)B.dropped, B.dropped, B.entries, 8.0 * B.head.size() / 1e6, 2.0 * B.ent.size() / 1e6);
  B.nlist = nlist;
  B.build_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
static int upload_beams(HostTrack& t) {
  auto& B = t.beam;
  if (B.ent.size() >= 0x7FFFFFF0u) return fail("beam list continuations hold %zu entries (31-bit cell offsets)", B.ent.size());
  HIPCHK(hipMalloc(&B.d_chunk, sizeof(int4) * std::max<size_t>(B.chunk.size(), 1)));
  if (!B.chunk.empty()) HIPCHK(hipMemcpy(B.d_chunk, B.chunk.data(), sizeof(int4) * B.chunk.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMalloc(&B.d_ent, sizeof(uint16_t) * std::max<size_t>(B.ent.size(), 1)));
  if (!B.ent.empty()) HIPCHK(hipMemcpy(B.d_ent, B.ent.data(), sizeof(uint16_t) * B.ent.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMalloc(&B.d_head, sizeof(uint2) * std::max<size_t>(B.head.size(), 1)));
  if (!B.head.empty()) HIPCHK(hipMemcpy(B.d_head, B.head.data(), sizeof(uint2) * B.head.size(), hipMemcpyHostToDevice));
  B.g.chunk = B.d_chunk; B.g.nxc = B.nxc; B.g.ent = B.d_ent; B.g.head = B.d_head;
  return 0;
}

static int upload_grid(HostGrid& G) {
  HIPCHK(hipMalloc(&G.d_start, sizeof(int) * G.start.size()));
  HIPCHK(hipMemcpy(G.d_start, G.start.data(), sizeof(int) * G.start.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMalloc(&G.d_idx, sizeof(uint16_t) * std::max<size_t>(G.idx.size(), 1)));
  if (!G.idx.empty()) HIPCHK(hipMemcpy(G.d_idx, G.idx.data(), sizeof(uint16_t) * G.idx.size(), hipMemcpyHostToDevice));
  G.g.start = G.d_start; G.g.idx = G.d_idx; G.g.box = nullptr;
  if (!G.box.empty()) {
    HIPCHK(hipMalloc(&G.d_box, sizeof(float4) * G.box.size()));
    HIPCHK(hipMemcpy(G.d_box, G.box.data(), sizeof(float4) * G.box.size(), hipMemcpyHostToDevice));
    G.g.box = G.d_box;
  }
  return 0;
}

// A built track: the device tables of one .track (walls, segments, grids, beam lists, sensor image), read-only
// once built.  Handles share them through a process-wide cache keyed by the track's input arrays and the device:
// every env of a batch, every VecEnv sub-engine and every later handle on the same track uses one copy (the beam
// lists are 0.2-0.5 GB per track at 1 m cells and take ~2 s of host time to build).  The last handle to drop a
// build frees its device memory.
struct TrackBuild {
  int device = 0;
  HostTrack t;
  size_t lds = 0;   // model_kernel's LDS wall table
  ~TrackBuild() {
    DeviceGuard on(device);
    hipFree(t.d_walls); hipFree(t.d_wfat); hipFree(t.d_segs); hipFree(t.d_prefix);
    hipFree(t.bp.d_start); hipFree(t.bp.d_idx); hipFree(t.bp.d_box); hipFree(t.sn.d_start); hipFree(t.sn.d_idx);
    hipFree(t.d_groups); hipFree(t.d_swall);
    hipFree(t.beam.d_chunk); hipFree(t.beam.d_ent); hipFree(t.beam.d_head);
  }
};
static std::mutex g_track_mu;
static std::unordered_map<std::string, std::weak_ptr<TrackBuild>> g_track_cache;

// The sensor wall image (2 float4 per wall + 1 per wall group) lives in the dynamic LDS of the kernels that stage it
// (ray_sensor_kernel, the fused rollout_kernel); with their static LDS it must fit the CU's 160 KiB, so that bounds
// the walls a track may have (~4 000 with the fused rollout's static LDS, ~4 900 for the sensor kernel alone; the
// bundled tracks have 730-732).  Images beyond 64 KiB are declared to the runtime first.
static int sensor_lds_reserve(size_t need) {
  const void* kern[] = {(const void*)ray_sensor_kernel<4>, (const void*)ray_sensor_kernel<16>,
                        (const void*)ray_sensor_kernel<16, 512>, (const void*)ray_sensor_kernel<16, 1024>,
                        (const void*)ray_sensor_kernel<4, BLOCK, false, true>, (const void*)ray_sensor_kernel<16, BLOCK, false, true>,
                        (const void*)ray_sensor_kernel<16, 512, false, true>, (const void*)ray_sensor_kernel<16, 1024, false, true>,
                        (const void*)rollout_kernel};
  for (const void* k : kern) {
    hipFuncAttributes a;
    if (hipFuncGetAttributes(&a, k) != hipSuccess) return fail("hipFuncGetAttributes failed");
    // the fused rollout kernel also holds the car-car extension's scratch after the wall image
    const size_t n2 = k == (const void*)rollout_kernel ? ((need + 15) & ~(size_t)15) + CC_LDS_BYTES : need;
    if (a.sharedSizeBytes + n2 > LDS_PER_CU)
      return fail("track needs %zu B of LDS for its sensor wall image; with %zu B of static LDS a workgroup has %zu",
                  need, (size_t)a.sharedSizeBytes, LDS_PER_CU - (size_t)a.sharedSizeBytes);
    if (n2 > 64 * 1024) HIPCHK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)n2));
  }
  return 0;
}
// the host tables of one track (nascar_add_track): walls as Box2D sees them, segments, grids, beam lists, wall groups
static int host_build_track(HostTrack& t, const double* segments, int32_t nseg, double total_length,
                            const double* walls, int32_t nwall, float beam_cell) {
  t.total_length = total_length;
  t.startline = -1; t.has_banking = 0;
  double pre = 0.0;
  for (int k = 0; k < nseg; ++k) {
    const double* s = segments + 13 * k;
    DSeg d;
    d.sx = s[2]; d.sy = s[3]; d.ex = s[4]; d.ey = s[5]; d.width = s[6]; d.banking = s[12];
    double br = d.banking * (M_PI / 180.0);
    d.la = (1500.0 * 9.81) * sin(fabs(br)) * 0.3;     // src/car.py:527-533
    d.chord = sqrt(pow(d.ex - d.sx, 2.0) + pow(d.ey - d.sy, 2.0));
    t.prefix.push_back(pre);
    pre += d.chord;
    t.segs.push_back(d);
    if (t.startline < 0 && (int)s[0] == 1) t.startline = k;
    if (fabs(d.banking) >= 0.1) t.has_banking = 1;
  }
  std::unordered_map<std::string, int> keys;
  for (int j = 0; j < nwall; ++j) {
    const double* w = walls + 4 * j;
    HWall L;
    memset(&L, 0, sizeof L);
    L.px = (float)w[0]; L.py = (float)w[1]; L.ang = (float)w[2];
    L.qs = sinf(L.ang); L.qc = cosf(L.ang);
    L.hx = (float)w[3]; L.hy = (float)(1.0 / 2);
    L.rad = sqrtf(L.hx * L.hx + L.hy * L.hy) + 0.02f;
    float lx = 0, ly = 0, ux = 0, uy = 0;
    const float vx[4] = {-L.hx, L.hx, L.hx, -L.hx}, vy[4] = {-L.hy, -L.hy, L.hy, L.hy};
    for (int i = 0; i < 4; ++i) {
      float x = (L.qc * vx[i] - L.qs * vy[i]) + L.px;
      float y = (L.qs * vx[i] + L.qc * vy[i]) + L.py;
      if (i == 0) { lx = ux = x; ly = uy = y; }
      else { lx = x < lx ? x : lx; ly = y < ly ? y : ly; ux = ux > x ? ux : x; uy = uy > y ? uy : y; }
    }
    const float r = 2.0f * 0.005f;
    L.flx = (lx - r) - 0.1f; L.fly = (ly - r) - 0.1f; L.fhx = (ux + r) + 0.1f; L.fhy = (uy + r) + 0.1f;
    char kbuf[96];
    snprintf(kbuf, sizeof kbuf, "wall_%.1f_%.1f", (double)L.px, (double)L.py);
    auto it = keys.find(kbuf);
    if (it == keys.end()) { int id = (int)keys.size(); keys.emplace(kbuf, id); L.key = id; }
    else L.key = it->second;
    t.walls.push_back(L);
  }
  if (nwall > 65535) return fail("track has %d walls (grid and beam-list indices are 16-bit)", nwall);
  build_grids(t);
  build_beams(t, beam_cell);
  return 0;
}
// the device tables of a host-built (or cache-loaded) track, on the current device; lds: model_kernel's wall table bytes.
// The beam lists' host copies are released afterwards (the device copies are all the kernels use).
static int upload_track(HostTrack& t, size_t& lds_out) {
  {
    std::vector<LWall> dw(t.walls.begin(), t.walls.end());
    std::vector<float4> fat(t.walls.size());
    for (size_t j = 0; j < t.walls.size(); ++j) fat[j] = make_float4(t.walls[j].flx, t.walls[j].fly, t.walls[j].fhx, t.walls[j].fhy);
    HIPCHK(hipMalloc(&t.d_walls, sizeof(LWall) * dw.size()));
    HIPCHK(hipMemcpy(t.d_walls, dw.data(), sizeof(LWall) * dw.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMalloc(&t.d_wfat, sizeof(float4) * fat.size()));
    HIPCHK(hipMemcpy(t.d_wfat, fat.data(), sizeof(float4) * fat.size(), hipMemcpyHostToDevice));
  }
  HIPCHK(hipMalloc(&t.d_segs, sizeof(DSeg) * t.segs.size()));
  HIPCHK(hipMemcpy(t.d_segs, t.segs.data(), sizeof(DSeg) * t.segs.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMalloc(&t.d_prefix, sizeof(double) * t.prefix.size()));
  HIPCHK(hipMemcpy(t.d_prefix, t.prefix.data(), sizeof(double) * t.prefix.size(), hipMemcpyHostToDevice));
  if (upload_grid(t.bp) < 0 || upload_grid(t.sn) < 0) return -1;
  if (upload_beams(t) < 0) return -1;
  HIPCHK(hipMalloc(&t.d_groups, sizeof(float4) * t.groups.size()));
  HIPCHK(hipMemcpy(t.d_groups, t.groups.data(), sizeof(float4) * t.groups.size(), hipMemcpyHostToDevice));
  {   // the sensor kernel's wall image (same f32 values it would stage: rad + 0.25 rounded once)
    std::vector<float4> sw(2 * t.walls.size());
    for (size_t j = 0; j < t.walls.size(); ++j) {
      const HWall& w = t.walls[j];
      sw[2 * j] = make_float4(w.px, w.py, w.rad + 0.25f, w.hx);
      sw[2 * j + 1] = make_float4(w.qs, w.qc, w.hy, 0.0f);
    }
    HIPCHK(hipMalloc(&t.d_swall, sizeof(float4) * sw.size()));
    HIPCHK(hipMemcpy(t.d_swall, sw.data(), sizeof(float4) * sw.size(), hipMemcpyHostToDevice));
  }
  if (getenv("NASCAR_VERBOSE"))
    fprintf(stderr, "nascar_add_track: %zu walls, %zu groups; broadphase grid %dx%d (%zu entries), sensor grid %dx%d "
            "(%zu entries, mean %.1f per cell)\n", t.walls.size(), t.groups.size(), t.bp.g.nx, t.bp.g.ny, t.bp.idx.size(),
            t.sn.g.nx, t.sn.g.ny, t.sn.idx.size(), (double)t.sn.idx.size() / ((double)t.sn.g.nx * t.sn.g.ny));
  if (getenv("NASCAR_VERBOSE"))
    fprintf(stderr, "nascar_add_track: beam grid %dx%d (%.2f m cells), %zu cells with lists (%zu dropped: continuation "
            "offsets), %zu entries (mean %.2f per list), heads %.1f MB + continuations %.1f MB + cell chunks %.1f MB, built in "
            "%.2f s\n", t.beam.g.nx, t.beam.g.ny, 1.0 / (double)t.beam.g.inv_cell, t.beam.nlist / BEAM_NB,
            t.beam.dropped, t.beam.entries, (double)t.beam.entries / std::max<size_t>(1, t.beam.nlist),
            8.0 * t.beam.head.size() / 1e6, 2.0 * t.beam.ent.size() / 1e6, 16.0 * t.beam.chunk.size() / 1e6, t.beam.build_s);
  t.beam.chunk.clear(); t.beam.ent.clear(); t.beam.head.clear();
  t.beam.chunk.shrink_to_fit(); t.beam.ent.shrink_to_fit(); t.beam.head.shrink_to_fit();
  lds_out = sizeof(LWall) * t.walls.size();
  return 0;
}

// ------------------------------------------------------------------ track cache on disk (nascar_set_track_cache)
// A host build (walls, grids and 0.2-0.5 GB of beam lists per track at 1 m cells: ~2 s of 16 threads) written once and read
// by every later process: ranks of one node (bench.py --gpus N, learn/ppo.py-style SubprocVecEnv runs) share one build
// per track.  File = magic, format version, the full key (segments, walls, total length, cell size: compared byte for
// byte on load, so a hash collision can only miss), then the host tables.  Written to a temporary name and renamed; the
// builders of one key serialise on an flock'ed lock file, so concurrent ranks build each track once and the others load.
static const uint32_t TRACK_FILE_VERSION = 4;   // 4: 8-byte heads, 16-bit entries, per-track wall bits, chunked cell map
static std::string g_cache_dir;                       // "" = no disk cache (default)
static int g_retain = 8;                              // builds kept alive after their last handle (most recent first)
static std::deque<std::shared_ptr<TrackBuild>>* g_retained = new std::deque<std::shared_ptr<TrackBuild>>();
// (never destroyed: freeing device memory from a static destructor would run after the HIP runtime's own teardown)
static void retain_build(const std::shared_ptr<TrackBuild>& tb) {   // (g_track_mu held) most recently used first
  if (g_retain <= 0) return;
  auto& R = *g_retained;
  for (auto it = R.begin(); it != R.end(); ++it)
    if (*it == tb) { R.erase(it); break; }
  R.push_front(tb);
  while ((int)R.size() > g_retain) R.pop_back();
}

static uint64_t fnv1a64(const std::string& s, uint64_t h) {
  for (unsigned char c : s) { h ^= c; h *= 0x100000001B3ull; }
  return h;
}
struct Sink {
  FILE* f; bool ok = true;
  void raw(const void* p, size_t n) { if (ok && n && fwrite(p, 1, n, f) != n) ok = false; }
  template <class T> void pod(const T& v) { raw(&v, sizeof v); }
  template <class T> void vec(const std::vector<T>& v) { const uint64_t n = v.size(); pod(n); raw(v.data(), n * sizeof(T)); }
};
struct Source {
  FILE* f; bool ok = true;
  void raw(void* p, size_t n) { if (ok && n && fread(p, 1, n, f) != n) ok = false; }
  template <class T> void pod(T& v) { raw(&v, sizeof v); }
  template <class T> void vec(std::vector<T>& v) {
    uint64_t n = 0; pod(n);
    if (!ok || n > ((uint64_t)1 << 40) / sizeof(T)) { ok = false; return; }
    v.resize(n); raw(v.data(), n * sizeof(T));
  }
};
template <class IO, class HT> static void track_io(IO& io, HT& t) {   // the host tables, in file order
  io.vec(t.walls); io.vec(t.segs); io.vec(t.prefix);
  io.pod(t.total_length); io.pod(t.startline); io.pod(t.has_banking);
  io.pod(t.bp.g); io.vec(t.bp.start); io.vec(t.bp.idx); io.vec(t.bp.box);
  io.pod(t.sn.g); io.vec(t.sn.start); io.vec(t.sn.idx); io.vec(t.sn.box);
  io.pod(t.beam.g); io.vec(t.beam.chunk); io.pod(t.beam.nxc); io.vec(t.beam.ent); io.vec(t.beam.head);
  io.pod(t.beam.entries); io.pod(t.beam.nlist); io.pod(t.beam.dropped); io.pod(t.beam.build_s);
  io.vec(t.groups);
}
static bool load_track_file(const std::string& path, const std::string& key, HostTrack& t) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  Source in{f};
  char magic[8] = {0}; uint32_t ver = 0; std::string k;
  in.raw(magic, 8); in.pod(ver);
  std::vector<char> kb; in.vec(kb);
  bool ok = in.ok && !memcmp(magic, "NASCARTK", 8) && ver == TRACK_FILE_VERSION && kb.size() == key.size() &&
            !memcmp(kb.data(), key.data(), key.size());
  if (ok) { track_io(in, t); ok = in.ok; }
  fclose(f);
  if (!ok) t = HostTrack();
  return ok;
}
static void save_track_file(const std::string& path, const std::string& key, HostTrack& t) {
  const std::string tmp = path + ".tmp." + std::to_string((long)getpid());
  FILE* f = fopen(tmp.c_str(), "wb");
  if (!f) return;                        // (a cache that cannot be written is only slower)
  Sink out{f};
  out.raw("NASCARTK", 8); out.pod(TRACK_FILE_VERSION);
  std::vector<char> kb(key.begin(), key.end()); out.vec(kb);
  track_io(out, t);
  const bool ok = out.ok && fclose(f) == 0;
  if (ok) rename(tmp.c_str(), path.c_str());
  else unlink(tmp.c_str());
}
// the track's inputs and the beam-list cell size (builds at different cell sizes differ): the disk cache's key
static std::string track_key(const double* segments, int32_t nseg, double total_length, const double* walls,
                             int32_t nwall, float beam_cell) {
  std::string k;
  const int32_t dims[2] = {nseg, nwall};
  k.append((const char*)dims, sizeof dims);
  k.append((const char*)&total_length, sizeof total_length);
  k.append((const char*)&beam_cell, sizeof beam_cell);
  k.append((const char*)segments, sizeof(double) * 13 * (size_t)nseg);
  k.append((const char*)walls, sizeof(double) * 4 * (size_t)nwall);
  return k;
}
// host tables of a track: from the disk cache when it holds this key (*loaded = 1), else built (and written there)
static int host_track(HostTrack& t, const std::string& key, const double* segments, int32_t nseg, double total_length,
                      const double* walls, int32_t nwall, float beam_cell, int* loaded = nullptr) {
  if (loaded) *loaded = 0;
  if (g_cache_dir.empty()) return host_build_track(t, segments, nseg, total_length, walls, nwall, beam_cell);
  char name[64];
  snprintf(name, sizeof name, "track_%016llx%016llx.nbt", (unsigned long long)fnv1a64(key, 0xCBF29CE484222325ull),
           (unsigned long long)fnv1a64(key, 0x84222325CBF29CE4ull));
  const std::string path = g_cache_dir + "/" + name;
  if (load_track_file(path, key, t)) { if (loaded) *loaded = 1; return 0; }
  mkdir(g_cache_dir.c_str(), 0777);       // (one level; an existing directory is fine)
  const int lk = open((path + ".lock").c_str(), O_CREAT | O_RDWR, 0666);
  if (lk >= 0) flock(lk, LOCK_EX);       // another process may be building this key: wait for it, then load
  int rc = 0;
  if (lk >= 0 && load_track_file(path, key, t)) {
    if (loaded) *loaded = 1;
  } else {
    rc = host_build_track(t, segments, nseg, total_length, walls, nwall, beam_cell);
    if (rc == 0) save_track_file(path, key, t);
  }
  if (lk >= 0) { flock(lk, LOCK_UN); close(lk); }
  return rc;
}
