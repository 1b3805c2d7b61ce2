// Object tracks on the device: the object table of one frame (object_ops.hip's `objects`, `centre` and `info`) and the tracks kept
// over the frames -> the table's rows associated with the tracks, the tracks moved on, dropped and born, every row's track slot and id
// (include/camradepth_hip.h, crd_track_objects).  One launch, one workgroup per map, one thread per track slot and per table row (both at
// most 1024): the stage is a few kilobytes and launch-bound, and the assignment needs barriers, which one workgroup has.
//   load      a slot's state into registers, its prediction pos + vel and the rows' centres into LDS
//   associate rounds of mutual best choices (track_assoc.h) over LDS, two barriers a round; in a round every open row scans the
//             predictions up to the highest live slot and every open slot the n centres, without a branch in the loop
//   update    a matched slot moves towards its row, an unmatched one coasts; too many misses or a position off the window free it
//   births    the unmatched rows take the free slots, rank to rank: two ballot scans, no ticket
// No atomic at all and no workgroup reads what another wrote, so the bits are the same every run.  The round loop is capped at
// min(N, T) + 1, which it cannot pass (every round but the last takes a pair); leaving by the cap raises info's guard.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): k_track_objects 86 VGPRs, 49472 bytes of LDS (one workgroup of up to
// 16 waves on a CU), no scratch.
#include "raster.h"       // finite_d
#include "track_assoc.h"
#include <string.h>

// pos, vel and the squared distance are specified operation by operation (include/camradepth_hip.h) and compared bit for bit with
// NumPy, which never fuses
#pragma clang fp contract(off)

namespace {

constexpr int MAX_ITEMS = 1024;                                         // slots and rows of one map: one thread each
constexpr int MAX_WAVES = MAX_ITEMS / CRD_WAVE;
constexpr int FREE = 0, TENTATIVE = 1, CONFIRMED = 2;
constexpr int INT_MAX_ = 0x7fffffff;
constexpr long long NAN_BITS = 0x7ff8000000000000ll;

struct Trk {
  const int32_t *objects, *obj_info;
  const double* centre;
  const long long* origin;
  int M, N, T, nx, ny;
  double cell, gate2, alpha, beta;
  int confirm_hits, max_misses;
  long long *ids, *box, *next_id, *id_of;
  int32_t *tracks, *track_of, *info;
  double *pos, *vel;
};

__device__ __forceinline__ int up(int v) { return v < INT_MAX_ ? v + 1 : v; }

// The rank of this thread among the threads with f set, and their number, in every thread.  red holds MAX_WAVES ints.
__device__ __forceinline__ int block_rank(bool f, int* red, int& total) {
  const int lane = threadIdx.x & (CRD_WAVE - 1), wave = threadIdx.x >> 6, waves = (blockDim.x + CRD_WAVE - 1) >> 6;
  const unsigned long long word = __ballot(f);
  __syncthreads();                                                      // red may still be read from the call before
  if (lane == 0) red[wave] = __popcll(word);
  __syncthreads();
  int rank = __popcll(word & ((1ull << lane) - 1ull));
  total = 0;
  for (int q = 0; q < waves; ++q) {
    const int c = red[q];
    if (q < wave) rank += c;
    total += c;
  }
  return rank;
}

// crd_field_paths' INSIDE rule
__device__ __forceinline__ bool inside(const Trk& a, double X, double Y, long long ox, long long oy) {
  const double x_lo = (double)ox, x_hi = (double)(long long)((unsigned long long)ox + (unsigned long long)a.nx);
  const double y_lo = (double)oy, y_hi = (double)(long long)((unsigned long long)oy + (unsigned long long)a.ny);
  const double wx = floor(X / a.cell), wy = floor(Y / a.cell);
  return finite_d(X) && finite_d(Y) && wx >= x_lo && wx < x_hi && wy >= y_lo && wy < y_hi;
}

__device__ __forceinline__ void box_of(const int32_t* row, long long ox, long long oy, long long* b) {
  b[0] = (long long)((unsigned long long)ox + (unsigned long long)(long long)row[2]);
  b[1] = (long long)((unsigned long long)ox + (unsigned long long)(long long)row[3]);
  b[2] = (long long)((unsigned long long)oy + (unsigned long long)(long long)row[4]);
  b[3] = (long long)((unsigned long long)oy + (unsigned long long)(long long)row[5]);
}

// One workgroup per map; blockDim.x = max(N, T) up to a multiple of 64.  Thread tid owns slot tid (tid < T) and row tid (tid < N).
__global__ __launch_bounds__(MAX_ITEMS) void k_track_objects(Trk a) {
  __shared__ double zx[MAX_ITEMS], zy[MAX_ITEMS], px[MAX_ITEMS], py[MAX_ITEMS];
  __shared__ int trk_obj[MAX_ITEMS], obj_trk[MAX_ITEMS], obj_pick[MAX_ITEMS], trk_pick[MAX_ITEMS];
  __shared__ int red[MAX_WAVES];
  const long long m = blockIdx.x;
  const int tid = threadIdx.x;
  const bool slot = tid < a.T, row = tid < a.N;
  const long long id0 = a.next_id[m], ox = a.origin[m * 2], oy = a.origin[m * 2 + 1];
  int n = a.obj_info[m * 4];
  n = n < 0 ? 0 : (n > a.N ? a.N : n);
  const long long st = m * a.T + tid, rt = m * a.N + tid;      // this thread's slot and row

  // load
  int status = FREE, age = 0, hits = 0, misses = 0, object = -1, n_cells = 0, flags = 0;
  double pos_x = 0.0, pos_y = 0.0, vel_x = 0.0, vel_y = 0.0;
  long long box[4] = {0, 0, 0, 0};
  if (slot) {
    const int32_t* s = a.tracks + st * 8;
    status = s[0]; age = s[1]; hits = s[2]; misses = s[3]; object = s[4]; n_cells = s[5]; flags = s[6];
  }
  bool live = slot && status != FREE;
  if (live) {
    pos_x = a.pos[st * 2]; pos_y = a.pos[st * 2 + 1]; vel_x = a.vel[st * 2]; vel_y = a.vel[st * 2 + 1];
    for (int q = 0; q < 4; ++q) box[q] = a.box[st * 4 + q];
  }
  const double pred_x = pos_x + vel_x, pred_y = pos_y + vel_y;
  if (slot) {
    px[tid] = pred_x; py[tid] = pred_y;
    trk_obj[tid] = live ? TA_OPEN : TA_NOT;
    trk_pick[tid] = TA_NONE;
  }
  double z_x = 0.0, z_y = 0.0;
  bool candidate = false;
  if (row) {
    z_x = a.centre[rt * 2]; z_y = a.centre[rt * 2 + 1];
    candidate = tid < n && finite_d(z_x) && finite_d(z_y);
    zx[tid] = z_x; zy[tid] = z_y;
    obj_trk[tid] = candidate ? TA_OPEN : TA_NOT;
    obj_pick[tid] = TA_NONE;
  }
  // the slots above the highest live one take no part: births fill the lowest free slots, so the live ones sit at the bottom
  const unsigned long long live_word = __ballot(live);
  if ((tid & (CRD_WAVE - 1)) == 0) red[tid >> 6] = live_word ? tid + CRD_WAVE - __clzll((long long)live_word) : 0;
  __syncthreads();
  int t_hi = 0;
  for (int q = 0; q < (int)((blockDim.x + CRD_WAVE - 1) >> 6); ++q) t_hi = red[q] > t_hi ? red[q] : t_hi;

  // associate
  const int cap = (a.N < a.T ? a.N : a.T) + 1;
  int rounds = 0, any = 1;
  while (rounds < cap) {                                                // rounds and any are the same in every thread
    if (row) ta_object_pick(tid, t_hi, zx, zy, px, py, a.gate2, trk_obj, obj_trk, obj_pick);
    if (slot) ta_track_pick(tid, n, zx, zy, px, py, a.gate2, trk_obj, obj_trk, trk_pick);
    __syncthreads();
    const bool took = row && ta_take(tid, obj_pick, trk_pick, trk_obj, obj_trk);
    ++rounds;
    any = __syncthreads_or(took ? 1 : 0);
    if (!any) break;
  }
  const int guard = any ? 1 : 0;                                        // left by the cap with a pair just taken: never

  // update
  const int k = live ? trk_obj[tid] : TA_NOT;                           // the row that took this slot
  const bool matched = k >= 0;
  bool missed_out = false, left = false;
  if (live) {
    if (matched) {
      const double r_x = zx[k] - pred_x, r_y = zy[k] - pred_y;
      pos_x = pred_x + a.alpha * r_x; pos_y = pred_y + a.alpha * r_y;
      vel_x = vel_x + a.beta * r_x; vel_y = vel_y + a.beta * r_y;
      const int32_t* o = a.objects + (m * a.N + k) * 8;
      hits = up(hits); misses = 0; age = up(age); object = k; n_cells = o[1]; flags = o[6];
      box_of(o, ox, oy, box);
      if (hits >= a.confirm_hits) status = CONFIRMED;
    } else {
      pos_x = pred_x; pos_y = pred_y;
      misses = up(misses); age = up(age); object = -1;
      if (misses > a.max_misses) { live = false; missed_out = true; }
    }
    if (live && !inside(a, pos_x, pos_y, ox, oy)) {
      live = false; left = true;
      if (matched) obj_trk[k] = TA_NOT;                                 // the row keeps no track and is not born again either
    }
  }
  const int n_matched = __syncthreads_count(matched);
  const int n_missed_out = __syncthreads_count(missed_out);
  const int n_left = __syncthreads_count(left);
  const int n_kept = __syncthreads_count(live);

  // births: free slot of rank r <- unmatched row of rank r
  int* free_slot = trk_pick;                                            // not read any more (a barrier since)
  int n_free, n_new;
  const bool free_now = slot && !live;
  const int free_rank = block_rank(free_now, red, n_free);
  if (free_now) free_slot[free_rank] = tid;
  const int mine = row ? obj_trk[tid] : TA_NOT;                         // after the barriers above: a slot that left is seen
  const bool unmatched = mine == TA_OPEN;
  const int new_rank = block_rank(unmatched, red, n_new);               // its barriers also publish free_slot
  const int births = n_new < n_free ? n_new : n_free;

  // write the slot
  if (live) {
    int32_t* s = a.tracks + st * 8;
    s[0] = status; s[1] = age; s[2] = hits; s[3] = misses; s[4] = object; s[5] = n_cells; s[6] = flags; s[7] = 0;
    a.pos[st * 2] = pos_x; a.pos[st * 2 + 1] = pos_y; a.vel[st * 2] = vel_x; a.vel[st * 2 + 1] = vel_y;
    for (int q = 0; q < 4; ++q) a.box[st * 4 + q] = box[q];
  } else if (slot && free_rank >= births) {                             // stays free; a slot that is refilled is written by its row
    int32_t* s = a.tracks + st * 8;
    s[0] = FREE; s[1] = 0; s[2] = 0; s[3] = 0; s[4] = -1; s[5] = 0; s[6] = 0; s[7] = 0;
    a.ids[st] = -1;
    long long* p = reinterpret_cast<long long*>(a.pos) + st * 2;
    long long* v = reinterpret_cast<long long*>(a.vel) + st * 2;
    p[0] = NAN_BITS; p[1] = NAN_BITS; v[0] = NAN_BITS; v[1] = NAN_BITS;
    for (int q = 0; q < 4; ++q) a.box[st * 4 + q] = 0;
  }
  // write the row
  if (row) {
    int slot_of = -1;
    long long id = -1;
    if (mine >= 0) {                                                    // matched, and the slot is still live: no one writes its id
      slot_of = mine;
      id = a.ids[m * a.T + mine];
    } else if (unmatched && new_rank < births) {
      slot_of = free_slot[new_rank];
      id = (long long)((unsigned long long)id0 + (unsigned long long)new_rank);
      const long long bt = m * a.T + slot_of;
      const int32_t* o = a.objects + rt * 8;
      int32_t* s = a.tracks + bt * 8;
      s[0] = a.confirm_hits <= 1 ? CONFIRMED : TENTATIVE; s[1] = 1; s[2] = 1; s[3] = 0; s[4] = tid; s[5] = o[1]; s[6] = o[6]; s[7] = 0;
      a.ids[bt] = id;
      a.pos[bt * 2] = z_x; a.pos[bt * 2 + 1] = z_y; a.vel[bt * 2] = 0.0; a.vel[bt * 2 + 1] = 0.0;
      long long b[4];
      box_of(o, ox, oy, b);
      for (int q = 0; q < 4; ++q) a.box[bt * 4 + q] = b[q];
    }
    a.track_of[rt] = slot_of;
    a.id_of[rt] = id;
  }
  if (tid == 0) {
    a.next_id[m] = (long long)((unsigned long long)id0 + (unsigned long long)births);
    int32_t* o = a.info + m * 8;
    o[0] = n_kept + births; o[1] = n_matched; o[2] = births; o[3] = n_missed_out; o[4] = n_left; o[5] = n_new - births; o[6] = rounds;
    o[7] = guard;
  }
}

inline bool aligned_to(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }
inline double from_bits(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }
inline bool finite_h(double v) { return v - v == 0.0; }                  // false for NaN and +-inf

}  // namespace

extern "C" int crd_track_objects(const int32_t* objects, const double* centre, const int32_t* objects_info, const int64_t* origin, int32_t M,
                                 int32_t N, int32_t T, int32_t nx, int32_t ny, uint64_t cell_f64_bits, uint64_t gate_f64_bits,
                                 uint64_t alpha_f64_bits, uint64_t beta_f64_bits, int32_t confirm_hits, int32_t max_misses, int64_t* ids,
                                 int32_t* tracks, double* pos, double* vel, int64_t* box, int64_t* next_id, int32_t* track_of, int64_t* id_of,
                                 int32_t* info, crd_stream_t stream) {
  const char* name = "crd_track_objects";
  CRD_CHECK_ARG(M >= 1, "%s: bad argument (M %d maps)", name, M);
  CRD_CHECK_ARG(N >= 1 && N <= MAX_ITEMS, "%s: bad argument (N %d table rows; 1 .. 1024)", name, N);
  CRD_CHECK_ARG(T >= 1 && T <= MAX_ITEMS, "%s: bad argument (T %d track slots; 1 .. 1024)", name, T);
  CRD_CHECK_ARG(nx >= 1 && nx <= 65535 && ny >= 1 && ny <= 65535, "%s: bad argument (a map of nx %d x ny %d cells; each is 1 .. 65535)", name,
                nx, ny);
  const double cell = from_bits(cell_f64_bits), gate = from_bits(gate_f64_bits), alpha = from_bits(alpha_f64_bits),
               beta = from_bits(beta_f64_bits);
  CRD_CHECK_ARG(cell > 0.0 && finite_h(cell), "%s: bad argument (cell %g is not a finite positive size)", name, cell);
  CRD_CHECK_ARG(gate > 0.0 && finite_h(gate) && finite_h(gate * gate), "%s: bad argument (gate %g is not finite and positive with a finite square)",
                name, gate);
  CRD_CHECK_ARG(alpha > 0.0 && alpha <= 1.0, "%s: bad argument (alpha %g is not in (0, 1])", name, alpha);
  CRD_CHECK_ARG(beta >= 0.0 && beta <= 2.0, "%s: bad argument (beta %g is not in [0, 2])", name, beta);
  CRD_CHECK_ARG(confirm_hits >= 1, "%s: bad argument (confirm_hits %d is below 1)", name, confirm_hits);
  CRD_CHECK_ARG(max_misses >= 0, "%s: bad argument (max_misses %d is below 0)", name, max_misses);
  CRD_CHECK_ARG(objects && centre && objects_info && origin && ids && tracks && pos && vel && box && next_id && track_of && id_of && info,
                "%s: null pointer (objects, centre, objects_info, origin, ids, tracks, pos, vel, box, next_id, track_of, id_of, info)", name);
  CRD_CHECK_ARG(aligned_to(objects, 4) && aligned_to(objects_info, 4) && aligned_to(tracks, 4) && aligned_to(track_of, 4) && aligned_to(info, 4) &&
                    aligned_to(centre, 8) && aligned_to(origin, 8) && aligned_to(ids, 8) && aligned_to(pos, 8) && aligned_to(vel, 8) &&
                    aligned_to(box, 8) && aligned_to(next_id, 8) && aligned_to(id_of, 8),
                "%s: bad argument (objects, objects_info, tracks, track_of and info must be 4-byte aligned, centre, origin, ids, pos, vel, box, "
                "next_id and id_of 8-byte)", name);
  Trk a;
  a.objects = objects; a.obj_info = objects_info; a.centre = centre; a.origin = reinterpret_cast<const long long*>(origin);
  a.M = M; a.N = N; a.T = T; a.nx = nx; a.ny = ny; a.cell = cell; a.gate2 = gate * gate; a.alpha = alpha; a.beta = beta;
  a.confirm_hits = confirm_hits; a.max_misses = max_misses;
  a.ids = reinterpret_cast<long long*>(ids); a.box = reinterpret_cast<long long*>(box); a.next_id = reinterpret_cast<long long*>(next_id);
  a.id_of = reinterpret_cast<long long*>(id_of); a.tracks = tracks; a.track_of = track_of; a.info = info; a.pos = pos; a.vel = vel;
  const int items = N > T ? N : T;
  hipLaunchKernelGGL(k_track_objects, dim3(M), dim3(cdiv(items, CRD_WAVE) * CRD_WAVE), 0, as_stream(stream), a);
  CRD_LAUNCH_CHECK(name);
  return CRD_OK;
}
