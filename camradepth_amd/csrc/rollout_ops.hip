// Local planner on the device: K velocity candidates rolled out over P poses from the vehicle's pose, tested against the costmap and
// against the predicted positions of the object tracks, scored and picked (include/camradepth_hip.h, crd_plan_rollouts).  The arcs, the
// velocities and the horizon in track updates are tables made on the host, so the device adds, subtracts, multiplies, divides, floors and
// compares.  Two launches on the caller's stream:
//   rollouts  one wave per (candidate, map), four waves to a workgroup, the lanes over the poses (up to four a lane).  The workgroup first
//             compacts the counting tracks of its map into LDS by ballot, in slot order (pos, vel: 32 bytes a track, 32 KiB at 1,024);
//             every lane then walks that list for its poses, every lane reading the same track (an LDS broadcast).  Integer minimum,
//             maximum and add over the wave; lane 0 writes the candidate's record and its rows of the tables with plain stores.
//   pick      one workgroup per map: the counts of info, the least record in rp_better's order by a strided scan and a tree over LDS.
// No global atomic, and the pick is the least element of a total order: the same bits every run.  No workgroup waits for another; every
// loop's bound is an argument of the launch (the poses a lane owns, 1, 2 or 4, pick the instantiation).
#include "raster.h"       // finite_d, aligned16
#include "rollout_pick.h"
#include <string.h>

// the results are specified operation by operation (include/camradepth_hip.h) and compared bit for bit with NumPy, which never fuses
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256, WAVES = TPB / CRD_WAVE;
constexpr int PICK_TPB = 256;                                           // at most 16 records a thread, a tree of eight levels
constexpr int SEGS = RP_MAX_T / CRD_WAVE;                               // runs of 64 slots
constexpr int NO_POSE = 0x7fffffff;

struct Roll {
  const double *pose, *vw, *arc, *tau;
  int M, n_v, n_w, K, P, nx, ny, blocked_at, outside_blocks;
  const long long* origin;
  double cell;
  const unsigned char* cost;
  const int32_t* togo;                                                  // may be NULL
  const int32_t* tracks;                                                // may be NULL: then T is 0
  const double *pos, *vel;
  int T, min_status, max_object_cells;
  double min_speed2, keep_out2;
  const double* twist;                                                  // may be NULL
  double a_v_dt, a_w_dt;
  RpWeights w;
  RpRecord* records;                                                    // the workspace
  int32_t *best, *info;                                                 // the outputs
  double* command;
  long long *score, *scores;                                            // the tables and xy may be NULL
  int32_t *first_blocked, *first_track, *max_cost, *end_togo;
  double* xy;
};

// whether slot s of map m counts; its pos and vel
__device__ __forceinline__ bool counting(const Roll& a, int m, int s, double& px, double& py, double& vx, double& vy) {
  if (s >= a.T) return false;
  const long long at = (long long)m * a.T + s;
  const int32_t* row = a.tracks + at * 8;
  px = a.pos[at * 2]; py = a.pos[at * 2 + 1]; vx = a.vel[at * 2]; vy = a.vel[at * 2 + 1];
  if (!(row[0] >= a.min_status && row[5] <= a.max_object_cells)) return false;
  if (!(finite_d(px) && finite_d(py) && finite_d(vx) && finite_d(vy))) return false;
  return vx * vx + vy * vy >= a.min_speed2;
}

// Launch 1: blockIdx = (group of WAVES candidates, map).  NJ: the poses a lane owns, cdiv(P, 64) rounded up to 1, 2 or 4.
template <int NJ>
__global__ __launch_bounds__(TPB) void k_rollouts(Roll a) {
  __shared__ double trk[RP_MAX_T * 4];
  __shared__ short slot_of[RP_MAX_T];
  __shared__ int seg_count[SEGS];
  const int tid = threadIdx.x, lane = tid & (CRD_WAVE - 1), wave = tid >> 6, m = blockIdx.y;
  const int chunks = (a.T + TPB - 1) / TPB;                             // 0 without tracks
  for (int c = 0; c < chunks; ++c) {
    double px, py, vx, vy;
    const unsigned long long word = __ballot(counting(a, m, c * TPB + tid, px, py, vx, vy));
    if (lane == 0) seg_count[c * WAVES + wave] = __popcll(word);
  }
  __syncthreads();
  int n_list = 0;
  for (int c = 0; c < chunks; ++c) {
    double px = 0.0, py = 0.0, vx = 0.0, vy = 0.0;
    const int s = c * TPB + tid, seg = c * WAVES + wave;
    const bool ok = counting(a, m, s, px, py, vx, vy);
    const unsigned long long word = __ballot(ok);
    int base = 0;
    for (int q = 0; q < seg; ++q) base += seg_count[q];
    if (ok) {
      const int at = base + __popcll(word & ((1ull << lane) - 1ull));   // the slots that count, in slot order
      trk[at * 4] = px; trk[at * 4 + 1] = py; trk[at * 4 + 2] = vx; trk[at * 4 + 3] = vy;
      slot_of[at] = (short)s;
    }
    for (int q = 0; q < WAVES; ++q) n_list += seg_count[c * WAVES + q];
  }
  __syncthreads();
  const int k = blockIdx.x * WAVES + wave;
  if (k >= a.K) return;                                                 // the whole wave, behind the barriers
  const double* T = a.pose + (long long)m * 12;
  const double t00 = T[0], t01 = T[1], t03 = T[3], t10 = T[4], t11 = T[5], t13 = T[7];
  const long long ox = a.origin[m * 2], oy = a.origin[m * 2 + 1];
  const double x_lo = (double)ox, x_hi = (double)(long long)((unsigned long long)ox + (unsigned long long)a.nx);
  const double y_lo = (double)oy, y_hi = (double)(long long)((unsigned long long)oy + (unsigned long long)a.ny);
  double X[NJ], Y[NJ], tau[NJ];
  int hit[NJ];
  int first = NO_POSE, worst = 0, sum = 0, end = RP_UNREACHED;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int p = lane + j * CRD_WAVE;
    hit[j] = NO_POSE;
    X[j] = Y[j] = tau[j] = __longlong_as_double(0x7ff8000000000000ll);  // a pose beyond P meets nothing
    if (p >= a.P) continue;
    const long long at = (long long)k * a.P + p;
    const double x = a.arc[at * 2], y = a.arc[at * 2 + 1];
    X[j] = t00 * x + t01 * y + t03;
    Y[j] = t10 * x + t11 * y + t13;
    tau[j] = a.tau[p];
    if (a.xy) {
      const long long to = ((long long)m * a.K + k) * a.P + p;
      a.xy[to * 2] = X[j]; a.xy[to * 2 + 1] = Y[j];
    }
    // crd_field_paths' INSIDE and BLOCKED
    const double wx = floor(X[j] / a.cell), wy = floor(Y[j] / a.cell);
    int c = -1;
    if (finite_d(X[j]) && finite_d(Y[j]) && wx >= x_lo && wx < x_hi && wy >= y_lo && wy < y_hi) {            // on the doubles
      const long long i = (long long)wx - ox, jj = (long long)wy - oy;
      if (i >= 0 && i < a.nx && jj >= 0 && jj < a.ny) c = (int)i * a.ny + (int)jj;
    }
    bool blocked;
    if (c >= 0) {
      const long long idx = (long long)m * a.nx * a.ny + c;
      const int cost = a.cost[idx];
      worst = cost > worst ? cost : worst;
      sum += cost;
      blocked = cost >= a.blocked_at;
      if (p == a.P - 1 && a.togo) end = a.togo[idx];
    } else {
      blocked = a.outside_blocks != 0;
    }
    if (blocked && p < first) first = p;
  }
  // the walk: entry i of the list is the i-th counting slot, so the first hit of a pose is its lowest slot
  for (int i = 0; i < n_list; ++i) {
    const double px = trk[i * 4], py = trk[i * 4 + 1], vx = trk[i * 4 + 2], vy = trk[i * 4 + 3];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const double qx = px + vx * tau[j], qy = py + vy * tau[j];
      const double dx = X[j] - qx, dy = Y[j] - qy;
      const double d2 = dx * dx + dy * dy;
      if (d2 <= a.keep_out2 && i < hit[j]) hit[j] = i;                  // a NaN compares false
    }
  }
  int track_key = NO_POSE;                                              // pose * 1024 + slot: the lowest hit pose, its lowest slot
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    if (hit[j] == NO_POSE) continue;
    const int key = (lane + j * CRD_WAVE) * RP_MAX_T + slot_of[hit[j]];
    track_key = key < track_key ? key : track_key;
  }
  const int first_static = first;
  if (track_key != NO_POSE && track_key / RP_MAX_T < first) first = track_key / RP_MAX_T;
  int clear_static = first_static == NO_POSE ? 1 : 0;
#pragma unroll
  for (int d = CRD_WAVE / 2; d > 0; d >>= 1) {
    const int f = __shfl_xor(first, d), t = __shfl_xor(track_key, d), w = __shfl_xor(worst, d), e = __shfl_xor(end, d);
    first = f < first ? f : first;
    track_key = t < track_key ? t : track_key;
    worst = w > worst ? w : worst;
    end = e < end ? e : end;
    sum += __shfl_xor(sum, d);
    clear_static &= __shfl_xor(clear_static, d);
  }
  if (lane != 0) return;
  bool admissible = true;
  if (a.twist) {
    const double dv = fabs(a.vw[k * 2] - a.twist[m * 2]), dw = fabs(a.vw[k * 2 + 1] - a.twist[m * 2 + 1]);
    admissible = dv <= a.a_v_dt && dw <= a.a_w_dt;                      // a NaN compares false
  }
  const bool clear = first == NO_POSE;
  const bool valid = admissible && clear && !(a.togo && a.w.togo > 0 && end == RP_UNREACHED);
  RpRecord r;
  r.score = rp_score(a.w, a.togo != nullptr, end, worst, sum, k, a.n_v, a.n_w);
  r.first_blocked = clear ? -1 : first;
  r.first_track = track_key == NO_POSE ? -1 : track_key % RP_MAX_T;
  r.max_cost = worst; r.end_togo = end; r.sum_cost = sum;
  r.flags = (admissible ? RP_ADMISSIBLE : 0) | (clear_static ? RP_CLEAR_STATIC : 0) | (clear ? RP_CLEAR : 0) | (valid ? RP_VALID : 0);
  const long long at = (long long)m * a.K + k;
  a.records[at] = r;
  if (a.scores) {
    a.scores[at] = r.score; a.first_blocked[at] = r.first_blocked; a.first_track[at] = r.first_track; a.max_cost[at] = r.max_cost;
    a.end_togo[at] = r.end_togo;
  }
}

// Launch 2: one workgroup per map
__global__ __launch_bounds__(PICK_TPB) void k_rollout_pick(Roll a) {
  __shared__ RpCandidate best[PICK_TPB];
  __shared__ int counts[4], bad;
  const int tid = threadIdx.x, m = blockIdx.x;
  const RpRecord* records = a.records + (long long)m * a.K;
  if (tid < 4) counts[tid] = 0;
  if (tid == 0) bad = 0;
  __syncthreads();
  RpCandidate mine = rp_at(records, tid < a.K ? tid : 0, a.n_w);
  int n[4] = {0, 0, 0, 0};
  for (int k = tid; k < a.K; k += PICK_TPB) {
    const RpCandidate c = rp_at(records, k, a.n_w);
    if (rp_better(c, mine)) mine = c;
    const int flags = records[k].flags;
    n[0] += flags & RP_ADMISSIBLE ? 1 : 0; n[1] += flags & RP_CLEAR_STATIC ? 1 : 0; n[2] += flags & RP_CLEAR ? 1 : 0;
    n[3] += flags & RP_VALID ? 1 : 0;
  }
  best[tid] = mine;
  for (int q = 0; q < 4; ++q)
    if (n[q]) atomicAdd(&counts[q], n[q]);                              // integers in LDS: no order changes the sum
  if (tid < 12 && !finite_d(a.pose[(long long)m * 12 + tid])) atomicOr(&bad, 1);
  if (tid < 2 && a.twist && !finite_d(a.twist[m * 2 + tid])) atomicOr(&bad, 1);
  __syncthreads();
  for (int d = PICK_TPB / 2; d > 0; d >>= 1) {
    if (tid < d && rp_better(best[tid + d], best[tid])) best[tid] = best[tid + d];
    __syncthreads();
  }
  if (tid != 0) return;
  const RpCandidate win = best[0];
  const int status = (bad ? RP_NOT_FINITE : 0) | (counts[3] == 0 ? RP_NO_CANDIDATE : 0);
  const bool picked = status == 0;                                      // then win is valid
  a.best[m] = picked ? win.k : -1;
  a.score[m] = picked ? win.score : 0ll;
  a.command[m * 2] = picked ? a.vw[win.k * 2] : 0.0;
  a.command[m * 2 + 1] = picked ? a.vw[win.k * 2 + 1] : 0.0;
  int32_t* info = a.info + m * 8;
  info[0] = counts[0]; info[1] = counts[1]; info[2] = counts[2]; info[3] = counts[3]; info[4] = status; info[5] = 0; info[6] = 0; info[7] = 0;
}

inline bool aligned_to(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }
inline double from_bits(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }
inline bool finite_h(double v) { return v - v == 0.0; }                  // false for NaN and +-inf
inline bool weight_ok(int32_t w) { return w >= 0 && w <= RP_MAX_WEIGHT; }

}  // namespace

extern "C" int crd_plan_rollouts(const double* pose, const double* vw, const double* arc, const double* tau, int32_t M, int32_t n_v, int32_t n_w,
                                 int32_t P, const int64_t* origin, uint64_t cell_f64_bits, const uint8_t* cost, const int32_t* togo, int32_t nx,
                                 int32_t ny, int32_t blocked_at, int32_t outside_blocks, const int32_t* tracks, const double* pos,
                                 const double* vel, int32_t T, int32_t min_status, int32_t max_object_cells, uint64_t min_speed2_f64_bits,
                                 uint64_t keep_out2_f64_bits, const double* twist, uint64_t a_v_dt_f64_bits, uint64_t a_w_dt_f64_bits,
                                 int32_t w_togo, int32_t w_max_cost, int32_t w_sum_cost, int32_t w_slow, int32_t w_turn, void* workspace,
                                 int64_t workspace_bytes, int32_t* best, double* command, int64_t* score, int32_t* info, int64_t* scores,
                                 int32_t* first_blocked, int32_t* first_track, int32_t* max_cost, int32_t* end_togo, double* xy,
                                 crd_stream_t stream) {
  const char* name = "crd_plan_rollouts";
  CRD_CHECK_ARG(M >= 1 && M <= 65535, "%s: bad argument (M %d maps; 1 .. 65535)", name, M);
  CRD_CHECK_ARG(n_v >= 1 && n_v <= RP_MAX_V, "%s: bad argument (n_v %d; 1 .. 64)", name, n_v);
  CRD_CHECK_ARG(n_w >= 1 && n_w <= RP_MAX_W && (n_w & 1), "%s: bad argument (n_w %d; odd, 1 .. 129)", name, n_w);
  const int K = n_v * n_w;
  CRD_CHECK_ARG(K <= RP_MAX_K, "%s: bad argument (K = n_v * n_w = %d candidates; at most 4096)", name, K);
  CRD_CHECK_ARG(P >= 1 && P <= RP_MAX_P, "%s: bad argument (P %d poses; 1 .. 256)", name, P);
  CRD_CHECK_ARG(nx >= 1 && nx <= 65535 && ny >= 1 && ny <= 65535, "%s: bad argument (a map of nx %d x ny %d cells; each is 1 .. 65535)", name,
                nx, ny);
  CRD_CHECK_ARG((long long)M * nx * ny < 0x80000000ll, "%s: bad argument (M * nx * ny = %lld cells are more than the 32-bit indices hold)", name,
                (long long)M * nx * ny);
  CRD_CHECK_ARG(blocked_at >= 1 && blocked_at <= 255, "%s: bad argument (blocked_at %d is not in 1 .. 255)", name, blocked_at);
  CRD_CHECK_ARG(outside_blocks == 0 || outside_blocks == 1, "%s: bad argument (outside_blocks %d is neither 0 nor 1)", name, outside_blocks);
  const double cell = from_bits(cell_f64_bits), min_speed2 = from_bits(min_speed2_f64_bits), keep_out2 = from_bits(keep_out2_f64_bits);
  const double a_v_dt = from_bits(a_v_dt_f64_bits), a_w_dt = from_bits(a_w_dt_f64_bits);
  CRD_CHECK_ARG(cell > 0.0 && finite_h(cell), "%s: bad argument (cell %g is not a finite positive size)", name, cell);
  CRD_CHECK_ARG(min_speed2 >= 0.0 && finite_h(min_speed2), "%s: bad argument (min_speed2 %g is negative or not finite)", name, min_speed2);
  CRD_CHECK_ARG(keep_out2 >= 0.0 && finite_h(keep_out2), "%s: bad argument (keep_out2 %g is negative or not finite)", name, keep_out2);
  CRD_CHECK_ARG(!twist || (a_v_dt >= 0.0 && a_w_dt >= 0.0), "%s: bad argument (a_v_dt %g, a_w_dt %g: with a twist neither is negative or NaN)",
                name, a_v_dt, a_w_dt);
  CRD_CHECK_ARG(T >= 0 && T <= RP_MAX_T && (tracks != nullptr) == (T > 0),
                "%s: bad argument (T %d slots with tracks %s: T is 1 .. 1024 with tracks and 0 without)", name, T, tracks ? "given" : "NULL");
  CRD_CHECK_ARG(!tracks || (pos && vel), "%s: null pointer (pos, vel: they go with tracks)", name);
  CRD_CHECK_ARG(min_status >= 0 && min_status <= 2, "%s: bad argument (min_status %d is not in 0 .. 2)", name, min_status);
  CRD_CHECK_ARG(max_object_cells >= 0, "%s: bad argument (max_object_cells %d is negative)", name, max_object_cells);
  CRD_CHECK_ARG(weight_ok(w_togo) && weight_ok(w_max_cost) && weight_ok(w_sum_cost) && weight_ok(w_slow) && weight_ok(w_turn),
                "%s: bad argument (weights togo %d, max_cost %d, sum_cost %d, slow %d, turn %d; each is 0 .. 32767)", name, w_togo, w_max_cost,
                w_sum_cost, w_slow, w_turn);
  CRD_CHECK_ARG(pose && vw && arc && tau && origin && cost && workspace && best && command && score && info,
                "%s: null pointer (pose, vw, arc, tau, origin, cost, workspace, best, command, score, info)", name);
  const bool all_tables = scores && first_blocked && first_track && max_cost && end_togo;
  const bool no_table = !scores && !first_blocked && !first_track && !max_cost && !end_togo;
  CRD_CHECK_ARG(all_tables || no_table, "%s: bad argument (the tables scores, first_blocked, first_track, max_cost and end_togo: all or none)",
                name);
  const long long need = 32ll * M * K;
  CRD_CHECK_ARG(workspace_bytes >= need, "%s: the workspace holds %lld bytes, %lld are needed", name, (long long)workspace_bytes, need);
  CRD_CHECK_ARG(aligned16(workspace), "%s: bad argument (the workspace must be 16-byte aligned)", name);
  CRD_CHECK_ARG(aligned_to(pose, 8) && aligned_to(vw, 8) && aligned_to(arc, 8) && aligned_to(tau, 8) && aligned_to(origin, 8) && aligned_to(pos, 8) &&
                    aligned_to(vel, 8) && aligned_to(twist, 8) && aligned_to(command, 8) && aligned_to(score, 8) && aligned_to(scores, 8) &&
                    aligned_to(xy, 8) && aligned_to(togo, 4) && aligned_to(tracks, 4) && aligned_to(best, 4) && aligned_to(info, 4) &&
                    aligned_to(first_blocked, 4) && aligned_to(first_track, 4) && aligned_to(max_cost, 4) && aligned_to(end_togo, 4),
                "%s: bad argument (pose, vw, arc, tau, origin, pos, vel, twist, command, score, scores and xy must be 8-byte aligned, togo, "
                "tracks, best, info, first_blocked, first_track, max_cost and end_togo 4-byte)", name);
  static_assert(sizeof(RpRecord) == 32, "the workspace formula counts 32 bytes a record");
  Roll a;
  a.pose = pose; a.vw = vw; a.arc = arc; a.tau = tau; a.M = M; a.n_v = n_v; a.n_w = n_w; a.K = K; a.P = P; a.nx = nx; a.ny = ny;
  a.blocked_at = blocked_at; a.outside_blocks = outside_blocks; a.origin = reinterpret_cast<const long long*>(origin); a.cell = cell;
  a.cost = cost; a.togo = togo; a.tracks = tracks; a.pos = pos; a.vel = vel; a.T = T; a.min_status = min_status;
  a.max_object_cells = max_object_cells; a.min_speed2 = min_speed2; a.keep_out2 = keep_out2; a.twist = twist; a.a_v_dt = a_v_dt;
  a.a_w_dt = a_w_dt; a.w.togo = w_togo; a.w.max_cost = w_max_cost; a.w.sum_cost = w_sum_cost; a.w.slow = w_slow; a.w.turn = w_turn;
  a.records = reinterpret_cast<RpRecord*>(workspace); a.best = best; a.info = info; a.command = command;
  a.score = reinterpret_cast<long long*>(score); a.scores = reinterpret_cast<long long*>(scores); a.first_blocked = first_blocked;
  a.first_track = first_track; a.max_cost = max_cost; a.end_togo = end_togo; a.xy = xy;
  hipStream_t st = as_stream(stream);
  const dim3 grid(cdiv(K, WAVES), M), block(TPB);
  if (P <= CRD_WAVE) hipLaunchKernelGGL(k_rollouts<1>, grid, block, 0, st, a);
  else if (P <= 2 * CRD_WAVE) hipLaunchKernelGGL(k_rollouts<2>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(k_rollouts<4>, grid, block, 0, st, a);
  hipLaunchKernelGGL(k_rollout_pick, dim3(M), dim3(PICK_TPB), 0, st, a);
  CRD_LAUNCH_CHECK(name);
  return CRD_OK;
}
