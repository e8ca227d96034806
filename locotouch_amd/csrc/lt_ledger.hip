// lt_ledger.hip - the episode ledger of DAgger collection and evaluation (include/lt_ledger.h).
//
// The host loops of locotouch_amd/distill/replay_buffer.py copy [check_every][n] rewards and dones to the host and replay the
// reference's per-step bookkeeping there: f64 reward sums, the finished episodes in step order then env-id order, and the rule that
// keeps trajectories until the kept steps reach a target - a rule that can stop in the middle of one step's done list.  Here one launch
// behind each env step applies the same rules to the step's reward and done rows (the rules: lt_ledger.h):
//   lt_ledger_step_kernel : ONE workgroup of 1024 lanes (16 waves) walks the envs in chunks of 1024.  Per chunk a lane adds its env's
//                           reward to the f64 sum; the done flags of a wave are one ballot, the popcount of the bits below the lane is
//                           the lane's place in the wave's part of the done list, and an inclusive shuffle scan over the wave gives
//                           the int64 lengths' prefix.  The 16 per-wave totals go through LDS (two barriers per chunk), every lane
//                           adds those of the waves below its own, and both running totals are carried from chunk to chunk in
//                           registers.  A done lane then knows its episode's number and the kept steps in front of it, which is all
//                           the rules ask: it writes its own list slots, so every list has one order whatever the waves' schedule.
//                           The counters a step adds to the head (kept envs, kept steps, overflow) are summed by a shuffle + LDS
//                           reduction at the end and lane 0 writes the head - the head is read by every lane before the first barrier
//                           and written behind the last, so no lane sees the new one.
//   lt_ledger_begin_kernel, lt_ledger_end_kernel : a lane per env.
// No atomics, no float arithmetic other than the one f64 add per env and the f32 <-> f64 conversions at the two ends.
#include <hip/hip_runtime.h>

#include "lt_host_check.h"
#include "lt_internal.h"

namespace {

constexpr int TPB = 1024;  // the step kernel's one workgroup
constexpr int WAVE = 64;
constexpr int NW = TPB / WAVE;
constexpr int ROW_TPB = 256;  // begin / end: a lane per env
constexpr size_t HEAD_BYTES = 8 * LT_LEDGER_HEAD_FIELDS;

struct StepArgs {
  long long* head;
  double* sum;
  long long* start;
  const float* reward;
  const unsigned char* done;
  double* ep_reward;
  long long* ep_length;
  long long* traj;
  long long n, ep_first, ep_cap, traj_first, traj_cap;
};

__device__ __forceinline__ long long wave_sum(long long v) {
  for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

__global__ __launch_bounds__(TPB) void lt_ledger_step_kernel(const StepArgs a) {
  __shared__ int s_cnt[NW];
  __shared__ long long s_len[NW];
  __shared__ long long s_red[3][NW];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
  if (a.head[LT_LEDGER_STOPPED_AT] != 0) return;  // (uniform: the whole workgroup leaves)
  const long long s = a.head[LT_LEDGER_STEP] + 1;
  const long long kept0 = a.head[LT_LEDGER_KEPT_STEPS], ep0 = a.head[LT_LEDGER_EPISODES], tr0 = a.head[LT_LEDGER_TRAJS];
  const long long ovf0 = a.head[LT_LEDGER_OVERFLOW];
  const long long keep_target = a.head[LT_LEDGER_KEEP_TARGET], episode_target = a.head[LT_LEDGER_EPISODE_TARGET];
  long long done_before = 0, len_before = 0;       // this step's done envs / their lengths in the chunks walked so far
  long long my_kept = 0, my_kept_len = 0, my_ovf = 0;  // this lane's share of what the step adds to the head
  for (long long base = 0; base < a.n; base += TPB) {
    const long long e = base + tid;
    const bool in = e < a.n;
    double sum = 0.0;
    long long st = 0;
    bool d = false;
    if (in) {
      sum = a.sum[e] + (double)a.reward[e];
      st = a.start[e];
      d = a.done[e] != 0;
    }
    const long long len = d ? s - st : 0;
    const unsigned long long ballot = __ballot(d);
    const int below = __popcll(ballot & ((1ull << lane) - 1ull));
    long long incl = len;  // inclusive scan of the lengths over the wave
    for (int off = 1; off < WAVE; off <<= 1) {
      const long long up = __shfl_up(incl, off, WAVE);
      if (lane >= off) incl += up;
    }
    if (lane == WAVE - 1) {
      s_cnt[wave] = __popcll(ballot);
      s_len[wave] = incl;
    }
    __syncthreads();
    long long cnt_lo = 0, len_lo = 0, cnt_all = 0, len_all = 0;
    for (int w = 0; w < NW; ++w) {
      const long long c = s_cnt[w], l = s_len[w];
      if (w < wave) { cnt_lo += c; len_lo += l; }
      cnt_all += c;
      len_all += l;
    }
    __syncthreads();  // (the next chunk overwrites s_cnt / s_len)
    if (in) {
      if (d) {
        const long long k = done_before + cnt_lo + below;           // the env's place in this step's done list
        const long long in_front = len_before + len_lo + incl - len;  // the lengths of the done envs below it
        const long long slot = ep0 + k - a.ep_first;
        if (slot >= 0 && slot < a.ep_cap) {
          a.ep_reward[slot] = sum;
          a.ep_length[slot] = len;
        } else {
          ++my_ovf;
        }
        sum = 0.0;
        if (keep_target < 0 || kept0 + in_front < keep_target) {  // kept: a prefix of the done list, so its place among the kept is k too
          if (a.traj) {
            const long long tslot = tr0 + k - a.traj_first;
            if (tslot >= 0 && tslot < a.traj_cap) {
              a.traj[3 * tslot + 0] = e;
              a.traj[3 * tslot + 1] = st;
              a.traj[3 * tslot + 2] = s;
            } else {
              ++my_ovf;
            }
          }
          ++my_kept;
          my_kept_len += len;
          a.start[e] = s;
        }
      }
      a.sum[e] = sum;
    }
    done_before += cnt_all;
    len_before += len_all;
  }
  const long long r0 = wave_sum(my_kept), r1 = wave_sum(my_kept_len), r2 = wave_sum(my_ovf);
  if (lane == 0) {
    s_red[0][wave] = r0;
    s_red[1][wave] = r1;
    s_red[2][wave] = r2;
  }
  __syncthreads();
  if (tid == 0) {
    long long kept = 0, kept_len = 0, ovf = 0;
    for (int w = 0; w < NW; ++w) {
      kept += s_red[0][w];
      kept_len += s_red[1][w];
      ovf += s_red[2][w];
    }
    const long long kept_steps = kept0 + kept_len, episodes = ep0 + done_before;
    a.head[LT_LEDGER_STEP] = s;
    a.head[LT_LEDGER_KEPT_STEPS] = kept_steps;
    a.head[LT_LEDGER_EPISODES] = episodes;
    a.head[LT_LEDGER_TRAJS] = tr0 + kept;
    a.head[LT_LEDGER_OVERFLOW] = ovf0 + ovf;
    if ((keep_target >= 0 && kept_steps >= keep_target) || (episode_target >= 0 && episodes >= episode_target)) a.head[LT_LEDGER_STOPPED_AT] = s;
  }
}

__global__ __launch_bounds__(ROW_TPB) void lt_ledger_begin_kernel(long long* head, double* sum, long long* start, const float* sums_in,
                                                                   long long n, long long keep_target, long long episode_target) {
  const long long e = (long long)blockIdx.x * ROW_TPB + threadIdx.x;
  if (e < LT_LEDGER_HEAD_FIELDS)
    head[e] = e == LT_LEDGER_KEEP_TARGET ? keep_target : e == LT_LEDGER_EPISODE_TARGET ? episode_target : 0;
  if (e >= n) return;
  sum[e] = sums_in ? (double)sums_in[e] : 0.0;
  start[e] = 0;
}

__global__ __launch_bounds__(ROW_TPB) void lt_ledger_end_kernel(const double* sum, float* out, long long n) {
  const long long e = (long long)blockIdx.x * ROW_TPB + threadIdx.x;
  if (e < n) out[e] = (float)sum[e];
}

const char* bad_state(const void* state, int64_t n) {
  if (n < 1 || n > INT32_MAX) return "n must be in [1, 2^31)";
  if (!state || (uintptr_t)state % 16) return "state must be non-null and 16-byte aligned";
  return nullptr;
}

void split_state(void* state, int64_t n, long long** head, double** sum, long long** start) {
  *head = (long long*)state;
  *sum = (double*)((char*)state + HEAD_BYTES);
  *start = (long long*)(*sum + n);
}

unsigned row_grid(int64_t n) {  // at least the lanes that write the head
  const int64_t lanes = n > LT_LEDGER_HEAD_FIELDS ? n : LT_LEDGER_HEAD_FIELDS;
  return (unsigned)((lanes + ROW_TPB - 1) / ROW_TPB);
}

}  // namespace

extern "C" {

int lt_ledger_state_bytes(int64_t n, size_t* bytes) {
  if (n < 1 || n > INT32_MAX) return refuse("lt_ledger_state_bytes", "n must be in [1, 2^31)");
  if (!bytes) return refuse("lt_ledger_state_bytes", "bytes must be non-null");
  *bytes = HEAD_BYTES + (size_t)16 * (size_t)n;
  return LT_OK;
}

int lt_ledger_begin(void* state, int64_t n, const float* reward_sums_in_or_null, int64_t keep_target, int64_t episode_target, void* stream) {
  const char* fn = "lt_ledger_begin";
  if (const char* why = bad_state(state, n)) return refuse(fn, why);
  if ((uintptr_t)reward_sums_in_or_null % 4) return refuse(fn, "reward_sums_in must be 4-byte aligned");
  long long *head, *start;
  double* sum;
  split_state(state, n, &head, &sum, &start);
  hipLaunchKernelGGL(lt_ledger_begin_kernel, dim3(row_grid(n)), dim3(ROW_TPB), 0, (hipStream_t)stream, head, sum, start, reward_sums_in_or_null,
                     (long long)n, (long long)(keep_target < 0 ? -1 : keep_target), (long long)(episode_target < 0 ? -1 : episode_target));
  return launch_status(fn);
}

int lt_ledger_step(void* state, int64_t n, const float* reward, const uint8_t* done, double* ep_reward, int64_t* ep_length, int64_t ep_first,
                   int64_t ep_cap, int64_t* traj, int64_t traj_first, int64_t traj_cap, void* stream) {
  const char* fn = "lt_ledger_step";
  if (const char* why = bad_state(state, n)) return refuse(fn, why);
  if (!reward || (uintptr_t)reward % 4) return refuse(fn, "reward must be non-null and 4-byte aligned");
  if (!done) return refuse(fn, "done must be non-null");
  if (ep_cap < 0) return refuse(fn, "ep_cap must not be negative");
  if (traj_cap < 0) return refuse(fn, "traj_cap must not be negative");
  if (ep_first < 0) return refuse(fn, "ep_first must not be negative");
  if (traj_first < 0) return refuse(fn, "traj_first must not be negative");
  if ((ep_cap > 0 && !ep_reward) || (uintptr_t)ep_reward % 8) return refuse(fn, "ep_reward must be 8-byte aligned, and non-null when ep_cap is not 0");
  if ((ep_cap > 0 && !ep_length) || (uintptr_t)ep_length % 8) return refuse(fn, "ep_length must be 8-byte aligned, and non-null when ep_cap is not 0");
  if ((traj_cap > 0 && !traj) || (uintptr_t)traj % 8) return refuse(fn, "traj must be 8-byte aligned, and non-null when traj_cap is not 0");
  StepArgs a;
  split_state(state, n, &a.head, &a.sum, &a.start);
  a.reward = reward; a.done = done; a.ep_reward = ep_reward; a.ep_length = (long long*)ep_length; a.traj = (long long*)traj;
  a.n = n; a.ep_first = ep_first; a.ep_cap = ep_reward && ep_length ? ep_cap : 0; a.traj_first = traj_first; a.traj_cap = traj_cap;
  hipLaunchKernelGGL(lt_ledger_step_kernel, dim3(1), dim3(TPB), 0, (hipStream_t)stream, a);
  return launch_status(fn);
}

int lt_ledger_end(const void* state, int64_t n, float* reward_sums_out, void* stream) {
  const char* fn = "lt_ledger_end";
  if (const char* why = bad_state(state, n)) return refuse(fn, why);
  if (!reward_sums_out || (uintptr_t)reward_sums_out % 4) return refuse(fn, "reward_sums_out must be non-null and 4-byte aligned");
  long long *head, *start;
  double* sum;
  split_state((void*)state, n, &head, &sum, &start);
  hipLaunchKernelGGL(lt_ledger_end_kernel, dim3(row_grid(n)), dim3(ROW_TPB), 0, (hipStream_t)stream, (const double*)sum, reward_sums_out, (long long)n);
  return launch_status(fn);
}

}  // extern "C"
