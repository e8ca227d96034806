// lt_obs_norm.hip - the running observation normaliser of the trainer on the device (include/lt_obs_norm.h).
//
// The reference's EmpiricalNormalization (loco_rl/loco_rl/modules/normalizer.py:42-72) is, per rollout step and per network, six
// small torch ops behind a host read of `count` (normalizer.py:60).  Here it is two launches that serve BOTH networks, on the
// rollout's stream, with no host read and no float atomics (every sum has one fixed order: runs are bit-reproducible):
//   launch 1  lt_obs_norm_stats_kernel : column statistics of the [n][d] row block as per-workgroup partials (mean, M2) over 128
//             rows each.  A lane owns VEC adjacent columns, a wave walks one row (64 x VEC consecutive floats per load
//             instruction), 8 rows are held in registers at a time and reduced in two passes; sub-blocks, row lanes and partials
//             are merged with Chan's formula.  All of it in f64: the kernel is bound by its loads, and an f32 merge chain carried
//             the rounding of every partial mean into the result (a column of mean 1e3 and spread 1e-2 must keep its variance).
//             The first row block also copies what launch 2 must see as "before" into the workspace.
//   launch 2  lt_obs_norm_finish_kernel: EVERY workgroup merges the partials of its own columns in the same fixed order (so all
//             of them hold the same bits), applies the running recurrence (normalizer.py:63-72, with the `until` test of :60 on the
//             device) and normalises its rows through (mean, 1 / (std + eps)); the first row block writes the running buffers, the
//             count and the snapshot.  Nothing this launch writes is read by it: the "before" values come from the workspace.
// The recurrence runs on f64 copies of mean and var that live in the workspace; the module's f32 buffers receive their roundings.
// An f32 `_mean` that is read back, updated and rounded at every step walks away from the recurrence by half an ulp per step (the
// torch class does); rounded once from the f64 state it stays within half an ulp.  The f64 state is used only while the f32 buffers
// still hold exactly what the kernel last wrote (else - first use, a loaded checkpoint - it restarts from the f32 values).
// In evaluation mode (merge = 0) launch 1 is skipped and launch 2 reads the running buffers, writing only snapshot and rows.
// lt_obs_norm_apply normalises rows through stored snapshots (one per `rows_per_snap` rows): the whole [T][n][d] storage at once.
#include <hip/hip_runtime.h>

#include "lt_device_prims.h"
#include "lt_host_check.h"
#include "lt_internal.h"

namespace {

constexpr int TPB = 256;         // 64 column groups x 4 row lanes (one wave per row lane)
constexpr int CG = 64;           // column groups of a chunk
constexpr int RL = 4;            // row lanes
constexpr int SUB = 8;           // rows a lane reduces in registers at a time
constexpr int STAT_ROWS = 128;   // rows of one partial (32 per row lane)
constexpr int APPLY_ROWS = 64;   // rows of one workgroup of lt_obs_norm_apply
constexpr int WS_HEAD = 4;       // floats in front of a network's workspace: the int64 count before the merge, padded to 16 bytes
constexpr int WS_FIXED = 12;     // regions of dpad floats behind it (below), then 4 per partial
constexpr int MAX_D = 1024;

struct Net {
  const float* x;
  int d, dpad, vec;
  float *mean, *var, *stdv;
  long long* count;
  float *snap, *out, *ws;
};
struct Args {
  Net net[2];
  long long n, until;
  double eps;
  int merge, nparts, finish_rows;
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

// Chan et al.: (na, ma, qa) <- (na, ma, qa) + (nb, mb, qb), q = sum of squared deviations.  na = 0 needs ma = qa = 0.
__device__ __forceinline__ void chan(double na, double& ma, double& qa, double nb, double mb, double qb) {
  if (nb <= 0.0) return;
  const double f = nb / (na + nb), dlt = mb - ma;
  ma += dlt * f;
  qa += qb + dlt * dlt * (na * f);
}

// Workspace of a network, in units of dpad floats behind the header: the f64 state [0,2) mean [2,4) var, the f32 values last written
// [4] mean [5] var; what launch 2 reads as "before": [6,8) mean f64 [8,10) var f64 [10] mean f32 [11] std f32; then per partial
// [0,2) mean f64 [2,4) M2 f64.
__device__ __forceinline__ float* ws_at(const Net& nt, long long unit) { return nt.ws + WS_HEAD + unit * nt.dpad; }
__device__ __forceinline__ double* ws_part(const Net& nt, long long p, int which) { return (double*)ws_at(nt, WS_FIXED + 4 * p + 2 * which); }

template <int VEC>
__device__ void stats_body(const Net& nt, long long n, int chunk, long long blk, double (*sh_m)[CG * 4], double (*sh_q)[CG * 4]) {
  const int tid = threadIdx.x, cg = tid & (CG - 1), rl = tid >> 6;
  const int col = (chunk * CG + cg) * VEC;
  const bool colok = col < nt.d;
  if (blk == 0 && rl == 0 && colok) {
    for (int v = 0; v < VEC; ++v) {
      const int c = col + v;
      const float mean = nt.mean[c], var = nt.var[c];
      const bool live = ws_at(nt, 4)[c] == mean && ws_at(nt, 5)[c] == var;  // the f32 buffers are what the f64 state was rounded to
      ((double*)ws_at(nt, 6))[c] = live ? ((const double*)ws_at(nt, 0))[c] : (double)mean;
      ((double*)ws_at(nt, 8))[c] = live ? ((const double*)ws_at(nt, 2))[c] : (double)var;
      ws_at(nt, 10)[c] = mean;
      ws_at(nt, 11)[c] = nt.stdv[c];
    }
  }
  if (blk == 0 && chunk == 0 && tid == 0) *(long long*)nt.ws = *nt.count;
  const long long row0 = blk * STAT_ROWS + rl * (STAT_ROWS / RL);
  double cn = 0.0, m[VEC], q[VEC];
  for (int v = 0; v < VEC; ++v) m[v] = q[v] = 0.0;
  if (colok) {
    for (int s = 0; s < STAT_ROWS / RL / SUB; ++s) {
      const long long r0 = row0 + s * SUB;
      if (r0 >= n) break;
      const int k = (n - r0) < SUB ? (int)(n - r0) : SUB;
      Vec<VEC> x[SUB];
#pragma unroll
      for (int i = 0; i < SUB; ++i) x[i] = ldv<VEC>(nt.x + (r0 + (i < k ? i : 0)) * nt.d + col);
      const double kf = (double)k;
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        double s1 = 0.0;
#pragma unroll
        for (int i = 0; i < SUB; ++i) s1 += i < k ? (double)x[i].v[v] : 0.0;
        const double mu = s1 / kf;
        double s2 = 0.0;
#pragma unroll
        for (int i = 0; i < SUB; ++i) { const double e = i < k ? (double)x[i].v[v] - mu : 0.0; s2 += e * e; }
        chan(cn, m[v], q[v], kf, mu, s2);
      }
      cn += kf;
    }
    for (int v = 0; v < VEC; ++v) { sh_m[rl][cg * VEC + v] = m[v]; sh_q[rl][cg * VEC + v] = q[v]; }
  }
  __syncthreads();
  if (colok && rl == 0) {
    for (int l = 1; l < RL; ++l) {  // the row lanes in order; a lane past the last row holds nothing
      const long long lr = n - (blk * STAT_ROWS + l * (STAT_ROWS / RL));
      const double ln = lr <= 0 ? 0.0 : lr < STAT_ROWS / RL ? (double)lr : (double)(STAT_ROWS / RL);
      for (int v = 0; v < VEC; ++v) chan(cn, m[v], q[v], ln, sh_m[l][cg * VEC + v], sh_q[l][cg * VEC + v]);
      cn += ln;
    }
    for (int v = 0; v < VEC; ++v) { ws_part(nt, blk, 0)[col + v] = m[v]; ws_part(nt, blk, 1)[col + v] = q[v]; }
  }
}

__global__ __launch_bounds__(TPB) void lt_obs_norm_stats_kernel(const Args a) {
  __shared__ double sh_m[RL][CG * 4], sh_q[RL][CG * 4];
  const Net& nt = a.net[blockIdx.z];
  const int chunk = blockIdx.y;
  if (chunk * CG * nt.vec >= nt.d) return;  // (uniform over the workgroup)
  if (nt.vec == 4) stats_body<4>(nt, a.n, chunk, blockIdx.x, sh_m, sh_q);
  else if (nt.vec == 2) stats_body<2>(nt, a.n, chunk, blockIdx.x, sh_m, sh_q);
  else stats_body<1>(nt, a.n, chunk, blockIdx.x, sh_m, sh_q);
}

template <int VEC>
__device__ void finish_body(const Net& nt, const Args& a, int chunk, long long blk, double (*sh_m)[CG * 4], double (*sh_q)[CG * 4],
                            float* sh_mean, float* sh_inv) {
  const int tid = threadIdx.x, cg = tid & (CG - 1), rl = tid >> 6;
  const int col = (chunk * CG + cg) * VEC;
  const bool colok = col < nt.d;
  const long long n = a.n;
  const int per = (a.nparts + RL - 1) / RL;  // partials per row lane, contiguous: the merge order is the row order
  double cn = 0.0, m[VEC], q[VEC];
  for (int v = 0; v < VEC; ++v) m[v] = q[v] = 0.0;
  if (a.merge) {
    if (colok) {
      const int p1 = (rl + 1) * per < a.nparts ? (rl + 1) * per : a.nparts;
      for (int p = rl * per; p < p1; ++p) {
        const long long left = n - (long long)p * STAT_ROWS;
        const double nb = left < STAT_ROWS ? (double)left : (double)STAT_ROWS;
        for (int v = 0; v < VEC; ++v) chan(cn, m[v], q[v], nb, ws_part(nt, p, 0)[col + v], ws_part(nt, p, 1)[col + v]);
        cn += nb;
      }
      for (int v = 0; v < VEC; ++v) { sh_m[rl][cg * VEC + v] = m[v]; sh_q[rl][cg * VEC + v] = q[v]; }
    }
    __syncthreads();
  }
  if (colok && rl == 0) {
    bool upd = false;
    long long cnt = 0;
    if (a.merge) {
      for (int l = 1; l < RL; ++l) {
        long long lo = (long long)l * per * STAT_ROWS, hi = (long long)(l + 1) * per * STAT_ROWS;
        lo = lo < n ? lo : n;
        hi = hi < n ? hi : n;
        const double ln = (double)(hi - lo);
        for (int v = 0; v < VEC; ++v) chan(cn, m[v], q[v], ln, sh_m[l][cg * VEC + v], sh_q[l][cg * VEC + v]);
        cn += ln;
      }
      const long long before = *(const long long*)nt.ws;
      upd = a.until < 0 || before < a.until;  // normalizer.py:60
      cnt = before + n;
    }
    const double w = upd ? (double)n / (double)cnt : 0.0;  // normalizer.py:65
    for (int v = 0; v < VEC; ++v) {
      const int c = col + v;
      float mean = a.merge ? ws_at(nt, 10)[c] : nt.mean[c];
      double den = (double)(a.merge ? ws_at(nt, 11)[c] : nt.stdv[c]) + a.eps;  // normalizer.py:54
      if (upd) {
        double mean64 = ((const double*)ws_at(nt, 6))[c], var64 = ((const double*)ws_at(nt, 8))[c];
        const double bm = m[v], bv = q[v] / (double)n;
        const double shift = bm - mean64;                   // normalizer.py:69-72
        mean64 += w * shift;
        var64 += w * (bv - var64 + shift * (bm - mean64));
        var64 = var64 > 0.0 ? var64 : 0.0;
        const double sd64 = sqrt(var64);
        mean = (float)mean64;
        den = sd64 + a.eps;
        if (blk == 0) {
          const float var = (float)var64;
          nt.mean[c] = mean; nt.var[c] = var; nt.stdv[c] = (float)sd64;
          ((double*)ws_at(nt, 0))[c] = mean64; ((double*)ws_at(nt, 2))[c] = var64;
          ws_at(nt, 4)[c] = mean; ws_at(nt, 5)[c] = var;
        }
      }
      const float inv = (float)(1.0 / den);
      sh_mean[cg * VEC + v] = mean;
      sh_inv[cg * VEC + v] = inv;
      if (blk == 0) { nt.snap[c] = mean; nt.snap[nt.d + c] = inv; }
    }
    if (upd && blk == 0 && chunk == 0 && tid == 0) *nt.count = cnt;
  }
  __syncthreads();
  if (!colok || !nt.out) return;
  Vec<VEC> mu, iv;
  for (int v = 0; v < VEC; ++v) { mu.v[v] = sh_mean[cg * VEC + v]; iv.v[v] = sh_inv[cg * VEC + v]; }
  const long long r1 = (blk + 1) * a.finish_rows < n ? (blk + 1) * a.finish_rows : n;
#pragma unroll 4
  for (long long r = blk * a.finish_rows + rl; r < r1; r += RL) {
    Vec<VEC> x = ldv<VEC>(nt.x + r * nt.d + col);
    for (int v = 0; v < VEC; ++v) x.v[v] = (x.v[v] - mu.v[v]) * iv.v[v];
    stv<VEC>(nt.out + r * nt.d + col, x);
  }
}

__global__ __launch_bounds__(TPB) void lt_obs_norm_finish_kernel(const Args a) {
  __shared__ double sh_m[RL][CG * 4], sh_q[RL][CG * 4];
  __shared__ float sh_mean[CG * 4], sh_inv[CG * 4];
  const Net& nt = a.net[blockIdx.z];
  const int chunk = blockIdx.y;
  if (chunk * CG * nt.vec >= nt.d) return;
  if (blockIdx.x > 0 && !nt.out) return;
  if (nt.vec == 4) finish_body<4>(nt, a, chunk, blockIdx.x, sh_m, sh_q, sh_mean, sh_inv);
  else if (nt.vec == 2) finish_body<2>(nt, a, chunk, blockIdx.x, sh_m, sh_q, sh_mean, sh_inv);
  else finish_body<1>(nt, a, chunk, blockIdx.x, sh_m, sh_q, sh_mean, sh_inv);
}

struct ApplyArgs {
  const float* x;
  float* out;
  const float* snaps;
  long long nrows, snap_stride, rows_per_snap;
  int d;
};

template <int VEC>
__global__ __launch_bounds__(TPB) void lt_obs_norm_apply_kernel(const ApplyArgs a) {
  const int tid = threadIdx.x, cg = tid & (CG - 1), rl = tid >> 6;
  const int col = ((int)blockIdx.y * CG + cg) * VEC;
  if (col >= a.d) return;
  const long long rb = (long long)blockIdx.x * APPLY_ROWS;
  const long long r1 = rb + APPLY_ROWS < a.nrows ? rb + APPLY_ROWS : a.nrows;
  long long s_have = -1;
  Vec<VEC> mu, iv;
  const bool one = rb / a.rows_per_snap == (r1 - 1) / a.rows_per_snap;  // the usual case: the block lies inside one snapshot
  long long s = rb / a.rows_per_snap;
#pragma unroll 4
  for (long long r = rb + rl; r < r1; r += RL) {
    if (!one) s = r / a.rows_per_snap;
    if (s != s_have) {
      const float* sn = a.snaps + s * a.snap_stride;
      for (int v = 0; v < VEC; ++v) { mu.v[v] = sn[col + v]; iv.v[v] = sn[a.d + col + v]; }
      s_have = s;
    }
    Vec<VEC> x = ldv<VEC>(a.x + r * a.d + col);
    for (int v = 0; v < VEC; ++v) x.v[v] = (x.v[v] - mu.v[v]) * iv.v[v];
    stv<VEC>(a.out + r * a.d + col, x);
  }
}

int vec_of(int d, const void* p, const void* q) {
  const uintptr_t bits = (uintptr_t)p | (uintptr_t)q;
  if (d % 4 == 0 && bits % 16 == 0) return 4;
  if (d % 2 == 0 && bits % 8 == 0) return 2;
  return 1;
}

int dpad_of(int d) { return (d + 3) & ~3; }
int nparts_of(int64_t n) { return (int)((n + STAT_ROWS - 1) / STAT_ROWS); }

}  // namespace

extern "C" {

int lt_obs_norm_ws_floats(int64_t n, int d, size_t* floats) {
  if (n <= 0 || n > INT32_MAX || d <= 0 || d > MAX_D || !floats) return einval("lt_obs_norm_ws_floats: n must be in [1, 2^31) and d in [1, 1024]");
  *floats = (size_t)WS_HEAD + ((size_t)WS_FIXED + 4 * (size_t)nparts_of(n)) * dpad_of(d);
  return LT_OK;
}

int lt_obs_norm_update(int64_t n, int merge, int64_t until, double eps,
                       const float* rows0, int d0, float* mean0, float* var0, float* std0, int64_t* count0, float* snap0, float* out0, float* ws0,
                       const float* rows1, int d1, float* mean1, float* var1, float* std1, int64_t* count1, float* snap1, float* out1, float* ws1,
                       void* stream) {
  const int nets = d1 ? 2 : 1;
  if (n <= 0 || n > INT32_MAX || !(eps > 0.0)) return einval("lt_obs_norm_update: n must be in [1, 2^31) and eps positive");
  Args a;
  a.n = n; a.until = until; a.eps = eps; a.merge = merge ? 1 : 0; a.nparts = nparts_of(n);
  const int64_t fr = (n + 63) / 64;  // at most 64 row blocks merge the partials again
  a.finish_rows = fr < 64 ? 64 : (int)((fr + RL - 1) / RL * RL);
  const float* rows[2] = {rows0, rows1};
  const int d[2] = {d0, d1};
  float* const mean[2] = {mean0, mean1}; float* const var[2] = {var0, var1}; float* const sd[2] = {std0, std1};
  int64_t* const count[2] = {count0, count1};
  float* const snap[2] = {snap0, snap1}; float* const out[2] = {out0, out1}; float* const ws[2] = {ws0, ws1};
  int chunks = 0;
  bool any_out = false;
  for (int i = 0; i < 2; ++i) {
    Net& t = a.net[i];
    if (i >= nets) { t = a.net[0]; continue; }
    if (d[i] <= 0 || d[i] > MAX_D || !rows[i] || !mean[i] || !var[i] || !sd[i] || !count[i] || !snap[i] || (merge && !ws[i]) ||
        (merge && (uintptr_t)ws[i] % 16))
      return einval("lt_obs_norm_update: d must be in [1, 1024]; rows, mean, var, std, count and snapshot non-null; the workspace "
                    "non-null and 16-byte aligned when merging");
    t.x = rows[i]; t.d = d[i]; t.dpad = dpad_of(d[i]); t.vec = vec_of(d[i], rows[i], out[i]);
    t.mean = mean[i]; t.var = var[i]; t.stdv = sd[i]; t.count = (long long*)count[i]; t.snap = snap[i]; t.out = out[i]; t.ws = ws[i];
    const int c = (d[i] / t.vec + CG - 1) / CG;
    chunks = c > chunks ? c : chunks;
    any_out = any_out || out[i];
  }
  if (a.merge)
    hipLaunchKernelGGL(lt_obs_norm_stats_kernel, dim3((unsigned)a.nparts, (unsigned)chunks, (unsigned)nets), dim3(TPB), 0, (hipStream_t)stream, a);
  const unsigned row_blocks = any_out ? (unsigned)((n + a.finish_rows - 1) / a.finish_rows) : 1u;
  hipLaunchKernelGGL(lt_obs_norm_finish_kernel, dim3(row_blocks, (unsigned)chunks, (unsigned)nets), dim3(TPB), 0, (hipStream_t)stream, a);
  return launch_status();
}

int lt_obs_norm_apply(const float* rows, int64_t nrows, int d, const float* snaps, int64_t snap_stride, int64_t rows_per_snap, float* out,
                      void* stream) {
  if (!rows || !out || !snaps || nrows <= 0 || d <= 0 || d > MAX_D || rows_per_snap <= 0 || snap_stride < 0 ||
      (nrows + APPLY_ROWS - 1) / APPLY_ROWS > INT32_MAX)
    return einval("lt_obs_norm_apply: rows, snapshots and out non-null; nrows, rows_per_snap positive; d in [1, 1024]");
  ApplyArgs a;
  a.x = rows; a.out = out; a.snaps = snaps; a.nrows = nrows; a.snap_stride = snap_stride; a.rows_per_snap = rows_per_snap; a.d = d;
  const int vec = vec_of(d, rows, out);
  const dim3 grid((unsigned)((nrows + APPLY_ROWS - 1) / APPLY_ROWS), (unsigned)((d / vec + CG - 1) / CG));
  if (vec == 4) hipLaunchKernelGGL(lt_obs_norm_apply_kernel<4>, grid, dim3(TPB), 0, (hipStream_t)stream, a);
  else if (vec == 2) hipLaunchKernelGGL(lt_obs_norm_apply_kernel<2>, grid, dim3(TPB), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(lt_obs_norm_apply_kernel<1>, grid, dim3(TPB), 0, (hipStream_t)stream, a);
  return launch_status();
}

}  // extern "C"
