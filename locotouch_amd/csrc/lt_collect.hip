// lt_collect.hip - the tactile delay line and the per-step recording of the student-driven collection loop (include/lt_collect.h).
//
// The reference's TactileRecorder (locotouch/distill/tactile_recorder.py:4-34) is a physically shifted [n][max_delay][d] register:
// every step reads and rewrites all of it (cat + where), gathers the delayed rows, and a reset multiplies the whole register by a
// mask.  Here the register is a ring with a head, a count and a delay per env (the rules: lt_collect.h), so a step moves one row in
// and one row out per env and a reset touches three ints:
//   lt_delay_push_kernel         : a wave per env walks along the row (lane l owns floats [l * VEC, l * VEC + VEC) of every 64 * VEC
//                                  chunk: one coalesced load instruction per chunk).  It loads the new row, stores it into the ring
//                                  slot behind the head, takes the delayed row - from the ring, or, when the delay reaches no further
//                                  back than this push, from the value just loaded - and stores it to one or two destinations; the
//                                  same wave copies the env's policy row to its store slot.  With rows = NULL it only reads
//                                  (lt_delay_read).  The env's three ints are one wave-uniform load each; lane 0 writes them back.
//   lt_collect_after_step_kernel : a lane per env: reward and done mask to their store slots, count = 0 and a fresh delay for the
//                                  finished envs.  With reward = NULL it is lt_delay_reset.
// THE ONE HAZARD of the in-place form: the push writes slot (head + 1) mod depth and the delayed row lies min(delay, count - 1) slots
// behind it.  delay < depth, so that is another slot - unless it is 0, when the delayed row IS the row being pushed: then it is taken
// from the registers that hold the loaded value and the ring is not read at all.  A wave owns its env's ring and ints alone, so
// there is no other reader or writer of them in the launch.
// VEC (4, 2 or 1 floats per lane: 16, 8 or 4 bytes) is chosen per launch on the host from d, the row strides and the pointers; since
// d is then a multiple of VEC, the only tail is the last, partly filled chunk of a row, which the chunk loop's bound handles.
// No LDS, no atomics, no arithmetic on the data: every output is bit for bit an input row or zeros.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "lt_host_check.h"
#include "lt_internal.h"

namespace {

constexpr int TPB = 256;    // four waves: four envs per workgroup
constexpr int WAVE = 64;
constexpr int STEP_TPB = 256;

struct PushArgs {
  float* ring;
  int *head, *count;
  const int* delay;
  const float* rows;  // NULL: read only
  float *out0, *out1;
  const float* copy_src;
  float* copy_dst;
  long long n, d, depth, rows_stride, out0_stride, out1_stride, copy_src_stride, copy_dst_stride, copy_d;
  int copy_vec;
};

template <int VEC>
struct Vec { float v[VEC]; };

template <int VEC>
__device__ __forceinline__ Vec<VEC> ldv(const float* p) {
  Vec<VEC> r;
  if constexpr (VEC == 4) { const float4 t = *(const float4*)p; r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w; }
  else if constexpr (VEC == 2) { const float2 t = *(const float2*)p; r.v[0] = t.x; r.v[1] = t.y; }
  else r.v[0] = *p;
  return r;
}
template <int VEC>
__device__ __forceinline__ void stv(float* p, const Vec<VEC>& r) {
  if constexpr (VEC == 4) *(float4*)p = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  else if constexpr (VEC == 2) *(float2*)p = make_float2(r.v[0], r.v[1]);
  else *p = r.v[0];
}

template <int VEC>
__device__ __forceinline__ void copy_row(const float* src, float* dst, long long d, int lane) {
  for (long long c = (long long)lane * VEC; c < d; c += WAVE * VEC) stv<VEC>(dst + c, ldv<VEC>(src + c));
}

template <int VEC>
__global__ __launch_bounds__(TPB) void lt_delay_push_kernel(const PushArgs a) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long long e = (long long)blockIdx.x * (TPB / WAVE) + (threadIdx.x >> 6);  // wave-uniform
  if (e >= a.n) return;
  const int depth = (int)a.depth;
  // (the clamps cost nothing and keep every access inside the env's ring whatever the ints hold: a state that was never zeroed, or
  // a delay the caller did not keep below depth, gives wrong rows, not a wild address)
  int head = a.head[e], count = a.count[e];
  int delay = a.delay[e];
  head = head >= 0 && head < depth ? head : 0;
  count = count < 0 ? 0 : count > depth ? depth : count;
  delay = delay < 0 ? 0 : delay;
  const bool push = a.rows != nullptr;
  if (push) {
    head = head + 1 < depth ? head + 1 : 0;
    count = count < depth ? count + 1 : depth;
  }
  const int back = delay < count - 1 ? delay : count - 1;  // -1: nothing pushed since the reset -> zeros
  const bool from_ring = back > 0 || (back == 0 && !push);
  float* const ring = a.ring + e * a.depth * a.d;
  float* const slot_in = ring + (long long)head * a.d;
  const float* const slot_out = ring + (long long)(head - back < 0 ? head - back + depth : head - back) * a.d;  // != slot_in when read
  const float* const row = push ? a.rows + e * a.rows_stride : nullptr;
  float* const o0 = a.out0 + e * a.out0_stride;
  float* const o1 = a.out1 ? a.out1 + e * a.out1_stride : nullptr;
  for (long long c = (long long)lane * VEC; c < a.d; c += WAVE * VEC) {
    Vec<VEC> x, y;
    for (int v = 0; v < VEC; ++v) x.v[v] = y.v[v] = 0.0f;
    if (push) {
      x = ldv<VEC>(row + c);
      stv<VEC>(slot_in + c, x);
    }
    if (from_ring) y = ldv<VEC>(slot_out + c);
    else if (back == 0) y = x;
    stv<VEC>(o0 + c, y);
    if (o1) stv<VEC>(o1 + c, y);
  }
  if (push && lane == 0) {
    a.head[e] = head;
    a.count[e] = count;
  }
  if (a.copy_src) {
    const float* const s = a.copy_src + e * a.copy_src_stride;
    float* const t = a.copy_dst + e * a.copy_dst_stride;
    if (a.copy_vec == 4) copy_row<4>(s, t, a.copy_d, lane);
    else if (a.copy_vec == 2) copy_row<2>(s, t, a.copy_d, lane);
    else copy_row<1>(s, t, a.copy_d, lane);
  }
}

struct StepArgs {
  int *count, *delay;  // NULL: no delay line
  const unsigned char* mask;  // reset form: NULL = every env
  const float* reward;        // NULL: the reset form (mask instead of dones, nothing recorded)
  const long long* dones;
  const long long* fresh;
  float* reward_out;
  unsigned char* done_out;
  long long n;
};

__global__ __launch_bounds__(STEP_TPB) void lt_collect_after_step_kernel(const StepArgs a) {
  const long long e = (long long)blockIdx.x * STEP_TPB + threadIdx.x;
  if (e >= a.n) return;
  bool done;
  if (a.reward) {
    done = a.dones[e] != 0;
    a.reward_out[e] = a.reward[e];
    a.done_out[e] = done ? 1 : 0;
  } else {
    done = !a.mask || a.mask[e] != 0;
  }
  if (done && a.count) {
    a.count[e] = 0;
    a.delay[e] = (int)a.fresh[e];
  }
}

size_t ring_bytes(int64_t n, int64_t d, int64_t depth) { return ((size_t)4 * (size_t)n * (size_t)depth * (size_t)d + 15) & ~(size_t)15; }

// n, d, depth >= 1, the products in range (the ring below 2^62 bytes, the grids below 2^31 workgroups)
const char* bad_shape(int64_t n, int64_t d, int64_t depth) {
  if (n < 1 || n > INT32_MAX) return "n must be in [1, 2^31)";
  if (d < 1 || d > INT32_MAX) return "d must be in [1, 2^31)";
  if (depth < 1 || depth > INT32_MAX) return "depth must be in [1, 2^31)";
  if ((double)n * (double)d * (double)depth > 1e18) return "n * d * depth is out of range";
  return nullptr;
}

struct Span { uintptr_t lo, hi; };
Span span_of(const void* p, int64_t n, int64_t stride, int64_t d) {
  const int64_t first = stride < 0 ? (n - 1) * stride : 0, last = stride < 0 ? 0 : (n - 1) * stride;
  return {(uintptr_t)p + (uintptr_t)(first * 4), (uintptr_t)p + (uintptr_t)((last + d) * 4)};
}
bool overlap(Span a, Span b) { return a.lo < b.hi && b.lo < a.hi; }

// floats per lane: the widest of 4, 2, 1 that divides d and every row stride and to whose bytes every pointer is aligned
struct VecPick {
  int64_t d;
  uintptr_t bits = 0;
  void add(const void* p, int64_t stride) { bits |= (uintptr_t)p | ((uintptr_t)stride * 4); }
  int vec() const {
    if (d % 4 == 0 && bits % 16 == 0) return 4;
    if (d % 2 == 0 && bits % 8 == 0) return 2;
    return 1;
  }
};

void split_state(void* state, int64_t n, int64_t d, int64_t depth, float** ring, int** head, int** count, int** delay) {
  *ring = (float*)state;
  *head = (int*)((char*)state + ring_bytes(n, d, depth));
  *count = *head + n;
  *delay = *count + n;
}

int push_or_read(const char* fn, void* state, int64_t n, int64_t d, int64_t depth, const float* rows, int64_t rows_stride, float* out0,
                 int64_t out0_stride, float* out1, int64_t out1_stride, const float* copy_src, int64_t copy_src_stride, float* copy_dst,
                 int64_t copy_dst_stride, int64_t copy_d, void* stream) {
  if (const char* why = bad_shape(n, d, depth)) return refuse(fn, why);
  if (!state || (uintptr_t)state % 4) return refuse(fn, "state must be non-null and 4-byte aligned");
  if (!out0) return refuse(fn, "out0 must be non-null");
  if (copy_src && !copy_dst) return refuse(fn, "copy_dst must be non-null when copy_src is given");
  if (copy_dst && !copy_src) return refuse(fn, "copy_src must be non-null when copy_dst is given");
  if (copy_src && (copy_d < 1 || copy_d > INT32_MAX)) return refuse(fn, "copy_d must be in [1, 2^31) when copy_src is given");
  for (const void* p : {(const void*)rows, (const void*)out0, (const void*)out1, (const void*)copy_src, (const void*)copy_dst})
    if ((uintptr_t)p % 4) return refuse(fn, "rows, out0, out1, copy_src and copy_dst must be 4-byte aligned");
  const Span st = {(uintptr_t)state, (uintptr_t)state + ring_bytes(n, d, depth) + (size_t)12 * (size_t)n};
  const struct { const char* name; const void* p; int64_t stride, width; } dsts[3] = {
      {"out0", out0, out0_stride, d}, {"out1", out1, out1_stride, d}, {"copy_dst", copy_dst, copy_dst_stride, copy_d}};
  for (const auto& t : dsts) {
    if (!t.p) continue;
    const Span s = span_of(t.p, n, t.stride, t.width);
    char why[96];
    if (rows && overlap(s, span_of(rows, n, rows_stride, d))) { snprintf(why, sizeof why, "%s overlaps the input rows", t.name); return refuse(fn, why); }
    if (copy_src && overlap(s, span_of(copy_src, n, copy_src_stride, copy_d))) { snprintf(why, sizeof why, "%s overlaps copy_src", t.name); return refuse(fn, why); }
    if (overlap(s, st)) { snprintf(why, sizeof why, "%s lies inside the state", t.name); return refuse(fn, why); }
  }
  PushArgs a;
  split_state(state, n, d, depth, &a.ring, &a.head, &a.count, (int**)&a.delay);
  a.rows = rows; a.out0 = out0; a.out1 = out1; a.copy_src = copy_src; a.copy_dst = copy_dst;
  a.n = n; a.d = d; a.depth = depth; a.rows_stride = rows_stride; a.out0_stride = out0_stride; a.out1_stride = out1_stride;
  a.copy_src_stride = copy_src_stride; a.copy_dst_stride = copy_dst_stride; a.copy_d = copy_src ? copy_d : 0;
  VecPick row{d}, cp{a.copy_d};
  row.add(state, 0);  // the ring's rows are d floats apart: covered by d itself
  if (rows) row.add(rows, rows_stride);
  row.add(out0, out0_stride);
  if (out1) row.add(out1, out1_stride);
  if (copy_src) { cp.add(copy_src, copy_src_stride); cp.add(copy_dst, copy_dst_stride); }
  a.copy_vec = copy_src ? cp.vec() : 1;
  const dim3 grid((unsigned)((n + TPB / WAVE - 1) / (TPB / WAVE)));
  const int vec = row.vec();
  if (vec == 4) hipLaunchKernelGGL(lt_delay_push_kernel<4>, grid, dim3(TPB), 0, (hipStream_t)stream, a);
  else if (vec == 2) hipLaunchKernelGGL(lt_delay_push_kernel<2>, grid, dim3(TPB), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(lt_delay_push_kernel<1>, grid, dim3(TPB), 0, (hipStream_t)stream, a);
  return launch_status(fn);
}

}  // namespace

extern "C" {

int lt_delay_state_bytes(int64_t n, int64_t d, int64_t depth, size_t* bytes) {
  if (const char* why = bad_shape(n, d, depth)) return refuse("lt_delay_state_bytes", why);
  if (!bytes) return refuse("lt_delay_state_bytes", "bytes must be non-null");
  *bytes = ring_bytes(n, d, depth) + (size_t)12 * (size_t)n;
  return LT_OK;
}

int lt_delay_reset(void* state, int64_t n, int64_t d, int64_t depth, const uint8_t* mask_or_null, const int64_t* fresh_delays, void* stream) {
  if (const char* why = bad_shape(n, d, depth)) return refuse("lt_delay_reset", why);
  if (!state || (uintptr_t)state % 4) return refuse("lt_delay_reset", "state must be non-null and 4-byte aligned");
  if (!fresh_delays || (uintptr_t)fresh_delays % 8) return refuse("lt_delay_reset", "fresh_delays must be non-null and 8-byte aligned");
  StepArgs a = {};
  float* ring;
  int* head;
  split_state(state, n, d, depth, &ring, &head, &a.count, &a.delay);
  a.mask = mask_or_null; a.fresh = (const long long*)fresh_delays; a.n = n;
  hipLaunchKernelGGL(lt_collect_after_step_kernel, dim3((unsigned)((n + STEP_TPB - 1) / STEP_TPB)), dim3(STEP_TPB), 0, (hipStream_t)stream, a);
  return launch_status("lt_delay_reset");
}

int lt_delay_push(void* state, int64_t n, int64_t d, int64_t depth, const float* rows, int64_t rows_stride, float* out0, int64_t out0_stride,
                  float* out1, int64_t out1_stride, const float* copy_src, int64_t copy_src_stride, float* copy_dst, int64_t copy_dst_stride,
                  int64_t copy_d, void* stream) {
  if (!rows) return refuse("lt_delay_push", "rows must be non-null");
  return push_or_read("lt_delay_push", state, n, d, depth, rows, rows_stride, out0, out0_stride, out1, out1_stride, copy_src, copy_src_stride,
                      copy_dst, copy_dst_stride, copy_d, stream);
}

int lt_delay_read(const void* state, int64_t n, int64_t d, int64_t depth, float* out, int64_t out_stride, void* stream) {
  return push_or_read("lt_delay_read", (void*)state, n, d, depth, nullptr, 0, out, out_stride, nullptr, 0, nullptr, 0, nullptr, 0, 0, stream);
}

int lt_collect_after_step(void* state_or_null, int64_t n, int64_t d, int64_t depth, const float* reward, const int64_t* dones,
                          const int64_t* fresh_delays, float* reward_out, uint8_t* done_mask_out, void* stream) {
  const char* fn = "lt_collect_after_step";
  if (n < 1 || n > INT32_MAX) return refuse(fn, "n must be in [1, 2^31)");
  if (!reward || (uintptr_t)reward % 4) return refuse(fn, "reward must be non-null and 4-byte aligned");
  if (!dones || (uintptr_t)dones % 8) return refuse(fn, "dones must be non-null and 8-byte aligned");
  if (!reward_out || (uintptr_t)reward_out % 4) return refuse(fn, "reward_out must be non-null and 4-byte aligned");
  if (!done_mask_out) return refuse(fn, "done_mask_out must be non-null");
  StepArgs a = {};
  if (state_or_null) {
    if (const char* why = bad_shape(n, d, depth)) return refuse(fn, why);
    if ((uintptr_t)state_or_null % 4) return refuse(fn, "state must be 4-byte aligned");
    if (!fresh_delays || (uintptr_t)fresh_delays % 8) return refuse(fn, "fresh_delays must be non-null and 8-byte aligned when state is given");
    float* ring;
    int* head;
    split_state(state_or_null, n, d, depth, &ring, &head, &a.count, &a.delay);
  }
  a.reward = reward; a.dones = (const long long*)dones; a.fresh = (const long long*)fresh_delays;
  a.reward_out = reward_out; a.done_out = done_mask_out; a.n = n;
  hipLaunchKernelGGL(lt_collect_after_step_kernel, dim3((unsigned)((n + STEP_TPB - 1) / STEP_TPB)), dim3(STEP_TPB), 0, (hipStream_t)stream, a);
  return launch_status(fn);
}

}  // extern "C"
