// lt_render.hip - batched ray caster over the analytic collision primitives (include/lt_env.h, lt_env_render).
//
// One launch renders up to LT_RENDER_VIEWS_PER_LAUNCH views (blockIdx.z = view).  A workgroup (256 threads = 4 wave64) owns a
// 64 x 16 pixel tile of one view; each wave walks 4 strips of 64 x 1 pixels (rows w, w + 4, w + 8, w + 12 of the tile), so every
// output store of a wave is 64 consecutive dwords - one 256-byte coalesced access.
//
// Prologue (per workgroup, DESIGN.md "Renderer"): 6 threads read the env's root pose, joint angles, object pose and foot forces through
// the quad-array pointers the host resolved (lt_env_render, the logic of lt_env_get_view), run the forward kinematics of the 4 legs
// and build the primitive table (world -> local rigid transform, extents, bounding sphere) and the camera basis in LDS.  Recomputing
// it per workgroup costs a few hundred FLOPs and saves a second launch plus a device scratch buffer.
//
// Per strip: lane i < LT_RENDER_NUM_PRIMS tests primitive i's bounding sphere against the strip's 4 frustum planes; the ballot is a
// wave-uniform bitmask and the per-pixel loop runs over its set bits (scalar loop, no divergence between lanes of a strip).  Nearest
// hit -> ambient + Lambert from one directional light, one shadow ray against the whole table (flag), a fixed palette with foot
// contact tint and the taxel grid on the plate.  No atomics: the output is a pure function of the inputs.
//
// Built with -ffinite-math-only: "no hit" is a large finite distance, every 1/d is guarded for axis-parallel rays.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lt_internal.h"
#include "../../include/lt_go1_model.h"

namespace {

constexpr int NPRIM = LT_RENDER_NUM_PRIMS;
constexpr int TILE_W = 64, TILE_H = 16;
constexpr float T_MISS = (float)LT_RENDER_FAR;
constexpr float EPS_D = 1e-12f;  // |d| component below which a ray counts as parallel to a slab / cap
constexpr float AMBIENT = 0.3f;
constexpr float CONTACT_N = 1.0f;  // foot contact threshold (N), the reference's contact-sensor threshold

enum { P_BOX = 0, P_CYL = 1, P_SPHERE = 2, P_PLANE = 3, P_NONE = 4 };

struct Prim {
  float R[9];   // local -> world rotation, row-major (world = R * local + c)
  float c[3];
  float e[3];   // box: half extents; cylinder (axis = local y): radius, half length; sphere: radius
  float bs[4];  // bounding sphere (centre, radius)
  int type;
};

struct RenderArgs {
  const float* root_pos;   // quad arrays [q][npad][4]: component c of env e at (c / 4) * qstride + e * 4 + c % 4
  const float* root_quat;
  const float* joint_pos;  // 3 quads: joint (type, leg) at type * qstride + e * 4 + leg
  const float* obj_pos;
  const float* obj_quat;
  const float* obj_params; // (radius, length, mass, mu)
  const float* force_hist; // [slot 3][type 4] quads, slot 0 newest
  const float* tactile;    // `tactile` observation rows (channel 0 = contact of taxel row * 13 + col); null without tactile
  long long qstride;       // npad * 4
  long long tactile_stride;
  int width, height, flags, has_obj, view0, nview;
  float light[3];
  uint32_t* rgba;
  float* depth;
  int* ids;
  float* poses;
  lt_render_view views[LT_RENDER_VIEWS_PER_LAUNCH];
};

// ---- small vector helpers (plain C++; this file does not include the step kernel's math headers) ----
struct F3 { float x, y, z; };
__device__ __forceinline__ F3 f3(float x, float y, float z) { return {x, y, z}; }
__device__ __forceinline__ F3 operator+(F3 a, F3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ F3 operator-(F3 a, F3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ F3 operator*(float s, F3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ float dot(F3 a, F3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ F3 cross(F3 a, F3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ F3 normalize(F3 a) {
  const float l2 = dot(a, a);
  return (l2 > 0.f ? 1.f / sqrtf(l2) : 0.f) * a;
}

struct Q4 { float w, x, y, z; };
__device__ __forceinline__ Q4 qmul(Q4 a, Q4 b) {
  return {a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
          a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x, a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w};
}
// v rotated by q (the form of compat/math.py quat_apply)
__device__ __forceinline__ F3 qrot(Q4 q, F3 v) {
  const F3 u = f3(q.x, q.y, q.z);
  const F3 t = 2.f * cross(u, v);
  return v + q.w * t + cross(u, t);
}
__device__ __forceinline__ void qmat(Q4 q, float* R) {
  const float n = q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z;
  const float s = n > 0.f ? 2.f / n : 0.f;
  const float xx = q.x * q.x * s, yy = q.y * q.y * s, zz = q.z * q.z * s, xy = q.x * q.y * s, xz = q.x * q.z * s, yz = q.y * q.z * s,
              wx = q.w * q.x * s, wy = q.w * q.y * s, wz = q.w * q.z * s;
  R[0] = 1.f - yy - zz; R[1] = xy - wz;       R[2] = xz + wy;
  R[3] = xy + wz;       R[4] = 1.f - xx - zz; R[5] = yz - wx;
  R[6] = xz - wy;       R[7] = yz + wx;       R[8] = 1.f - xx - yy;
}

__device__ __forceinline__ float quad(const float* f, long long qs, int e, int c) { return f[(c >> 2) * qs + (long long)e * 4 + (c & 3)]; }

// primitive owned by a body with pose (p, q): local frame = body frame * (offset, rotation `rot`: 0 none, 1 local y -> body x)
__device__ void make_prim(Prim& P, int type, F3 p, Q4 q, F3 off, int rot, float e0, float e1, float e2) {
  float B[9];
  qmat(q, B);
  if (rot == 1) {  // local axes in body axes: x_l = -y_b, y_l = x_b, z_l = z_b (R = B * M, M's columns those axes)
    for (int r = 0; r < 3; ++r) {
      const float bx = B[r * 3 + 0], by = B[r * 3 + 1], bz = B[r * 3 + 2];
      P.R[r * 3 + 0] = -by; P.R[r * 3 + 1] = bx; P.R[r * 3 + 2] = bz;
    }
  } else {
    for (int k = 0; k < 9; ++k) P.R[k] = B[k];
  }
  const F3 c = p + qrot(q, off);
  P.c[0] = c.x; P.c[1] = c.y; P.c[2] = c.z;
  P.e[0] = e0; P.e[1] = e1; P.e[2] = e2;
  P.bs[0] = c.x; P.bs[1] = c.y; P.bs[2] = c.z;
  P.bs[3] = type == P_BOX ? sqrtf(e0 * e0 + e1 * e1 + e2 * e2) : (type == P_CYL ? sqrtf(e0 * e0 + e1 * e1) : e0);
  P.type = type;
}

// nearest hit t in (tmin, tmax0) of a ray (o, d) with primitive P; n = world normal at the hit.  Returns tmax0 exactly when there is none.
__device__ __forceinline__ float intersect(const Prim& P, F3 o, F3 d, float tmin, const float tmax0, F3& n) {
  float tmax = tmax0;
  if (P.type == P_PLANE) {  // ground z = 0, seen from above
    if (d.z < -EPS_D && o.z > 0.f) {
      const float t = -o.z / d.z;
      if (t > tmin && t < tmax) { n = f3(0.f, 0.f, 1.f); return t; }
    }
    return tmax0;
  }
  const float* R = P.R;
  const F3 w = o - f3(P.c[0], P.c[1], P.c[2]);
  // local = R^T * world
  F3 lo = f3(R[0] * w.x + R[3] * w.y + R[6] * w.z, R[1] * w.x + R[4] * w.y + R[7] * w.z, R[2] * w.x + R[5] * w.y + R[8] * w.z);
  const F3 ld = f3(R[0] * d.x + R[3] * d.y + R[6] * d.z, R[1] * d.x + R[4] * d.y + R[7] * d.z, R[2] * d.x + R[5] * d.y + R[8] * d.z);
  // round shapes: solve from the ray point closest to the centre (t = tc), so that the quadratics do not cancel in f32 at distance
  const float tc = P.type == P_BOX ? 0.f : -dot(lo, ld);
  lo = lo + tc * ld;
  tmin -= tc;
  tmax -= tc;
  F3 ln = f3(0.f, 0.f, 0.f);
  float best = tmax;
  if (P.type == P_BOX) {
    float tn = -T_MISS, tf = T_MISS;
    int ax = -1;
    float sgn = 0.f;
    const float oo[3] = {lo.x, lo.y, lo.z}, dd[3] = {ld.x, ld.y, ld.z};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (fabsf(dd[k]) < EPS_D) {
        if (fabsf(oo[k]) > P.e[k]) return tmax0;
      } else {
        const float inv = 1.f / dd[k];
        float ta = (-P.e[k] - oo[k]) * inv, tb = (P.e[k] - oo[k]) * inv;
        if (ta > tb) { const float t = ta; ta = tb; tb = t; }
        if (ta > tn) { tn = ta; ax = k; sgn = dd[k] > 0.f ? -1.f : 1.f; }
        tf = tb < tf ? tb : tf;
      }
    }
    if (ax < 0 || !(tn <= tf) || !(tn > tmin) || !(tn < tmax)) return tmax0;
    best = tn;
    ln = ax == 0 ? f3(sgn, 0.f, 0.f) : (ax == 1 ? f3(0.f, sgn, 0.f) : f3(0.f, 0.f, sgn));
  } else if (P.type == P_CYL) {
    const float r = P.e[0], h = P.e[1];
    const float a = ld.x * ld.x + ld.z * ld.z;
    if (a > EPS_D) {
      const float b = lo.x * ld.x + lo.z * ld.z, cc = lo.x * lo.x + lo.z * lo.z - r * r;
      const float disc = b * b - a * cc;
      if (disc >= 0.f) {
        const float t = (-b - sqrtf(disc)) / a;
        const float y = lo.y + t * ld.y;
        if (t > tmin && t < best && fabsf(y) <= h) { best = t; ln = (1.f / r) * f3(lo.x + t * ld.x, 0.f, lo.z + t * ld.z); }
      }
    }
    if (fabsf(ld.y) > EPS_D) {
      const float inv = 1.f / ld.y;
#pragma unroll
      for (int s = -1; s <= 1; s += 2) {
        const float t = ((float)s * h - lo.y) * inv;
        const float x = lo.x + t * ld.x, z = lo.z + t * ld.z;
        if (t > tmin && t < best && x * x + z * z <= r * r && (float)s * ld.y < 0.f) { best = t; ln = f3(0.f, (float)s, 0.f); }
      }
    }
    if (!(best < tmax)) return tmax0;
  } else {  // sphere
    const float r = P.e[0];
    const float b = dot(lo, ld), cc = dot(lo, lo) - r * r;
    const float disc = b * b - cc;
    if (disc < 0.f) return tmax0;
    const float t = -b - sqrtf(disc);
    if (!(t > tmin) || !(t < tmax)) return tmax0;
    best = t;
    ln = (1.f / r) * (lo + t * ld);
  }
  n = f3(R[0] * ln.x + R[1] * ln.y + R[2] * ln.z, R[3] * ln.x + R[4] * ln.y + R[5] * ln.z, R[6] * ln.x + R[7] * ln.y + R[8] * ln.z);
  return best + tc < tmax0 ? best + tc : tmax0;
}

// palette (linear 0..1 RGB) per primitive id
__device__ __forceinline__ F3 albedo(int id) {
  if (id == LT_PRIM_TRUNK || id == LT_PRIM_BACK_MID) return f3(0.25f, 0.27f, 0.30f);
  if (id == LT_PRIM_PLATE) return f3(0.80f, 0.80f, 0.78f);
  if (id == LT_PRIM_RAIL_LEFT || id == LT_PRIM_RAIL_RIGHT) return f3(0.55f, 0.55f, 0.58f);
  if (id < LT_PRIM_THIGH) return f3(0.35f, 0.35f, 0.38f);  // hips
  if (id < LT_PRIM_CALF) return f3(0.85f, 0.55f, 0.15f);   // thighs
  if (id < LT_PRIM_FOOT) return f3(0.20f, 0.20f, 0.22f);   // calves
  if (id < LT_PRIM_OBJECT) return f3(0.10f, 0.10f, 0.10f); // feet
  return f3(0.15f, 0.45f, 0.85f);                           // object
}

__device__ __forceinline__ uint32_t pack(F3 c) {
  auto u8 = [](float v) -> uint32_t {
    v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
    return (uint32_t)(v * 255.f + 0.5f);
  };
  return u8(c.x) | (u8(c.y) << 8) | (u8(c.z) << 16) | (255u << 24);
}

__global__ __launch_bounds__(256) void lt_render_kernel(const RenderArgs a) {
  __shared__ Prim s_prim[NPRIM];
  __shared__ float s_pose[LT_NUM_SENSOR_BODIES * 7];
  __shared__ float s_cam[13];         // eye, forward, right, up, tan(fov / 2)
  __shared__ int s_contact[4];        // feet with |F| above the contact threshold
  const lt_render_view& V = a.views[blockIdx.z];
  const int e = V.env_id;
  const long long qs = a.qstride;
  const int tid = threadIdx.x;
  const F3 p0 = f3(quad(a.root_pos, qs, e, 0), quad(a.root_pos, qs, e, 1), quad(a.root_pos, qs, e, 2));
  const Q4 q0 = {quad(a.root_quat, qs, e, 0), quad(a.root_quat, qs, e, 1), quad(a.root_quat, qs, e, 2), quad(a.root_quat, qs, e, 3)};
  // ---- prologue: forward kinematics and the primitive table ----
  if (tid < 4) {  // leg `tid`: hip (about x), thigh, calf (about y), foot fixed to the calf (compat/scene_views.py link_kinematics)
    const int leg = tid;
    const float offs[LT_NUM_LEGS][LT_LINKS_PER_LEG][3] = LT_JOINT_OFFSET_INIT;
    const float foot[3] = LT_FOOT_OFFSET_INIT;
    const float hip_y[4] = LT_HIP_CYL_Y_INIT;
    const float thigh[3] = LT_THIGH_BOX_INIT, calf[3] = LT_CALF_BOX_INIT;
    F3 p = p0;
    Q4 q = q0;
    for (int k = 0; k < 3; ++k) {
      p = p + qrot(q, f3(offs[leg][k][0], offs[leg][k][1], offs[leg][k][2]));
      const float h = 0.5f * a.joint_pos[k * qs + (long long)e * 4 + leg];
      const float c = cosf(h), s = sinf(h);
      q = qmul(q, k == 0 ? Q4{c, s, 0.f, 0.f} : Q4{c, 0.f, s, 0.f});
      float* P = s_pose + (1 + k * 4 + leg) * 7;
      P[0] = p.x; P[1] = p.y; P[2] = p.z; P[3] = q.w; P[4] = q.x; P[5] = q.y; P[6] = q.z;
      if (k == 0) make_prim(s_prim[LT_PRIM_HIP + leg], P_CYL, p, q, f3(0.f, hip_y[leg], 0.f), 0, LT_HIP_CYL_RADIUS, 0.5f * LT_HIP_CYL_LENGTH, 0.f);
      // thigh / calf boxes: URDF size (length, width, depth) turned about y by 90 deg, centred half a length below the joint
      if (k == 1) make_prim(s_prim[LT_PRIM_THIGH + leg], P_BOX, p, q, f3(0.f, 0.f, -0.5f * thigh[0]), 0, 0.5f * thigh[2], 0.5f * thigh[1], 0.5f * thigh[0]);
      if (k == 2) make_prim(s_prim[LT_PRIM_CALF + leg], P_BOX, p, q, f3(0.f, 0.f, -0.5f * calf[0]), 0, 0.5f * calf[2], 0.5f * calf[1], 0.5f * calf[0]);
    }
    const F3 pf = p + qrot(q, f3(foot[0], foot[1], foot[2]));
    float* P = s_pose + (1 + 12 + leg) * 7;
    P[0] = pf.x; P[1] = pf.y; P[2] = pf.z; P[3] = q.w; P[4] = q.x; P[5] = q.y; P[6] = q.z;
    make_prim(s_prim[LT_PRIM_FOOT + leg], P_SPHERE, pf, q, f3(0.f, 0.f, 0.f), 0, LT_FOOT_RADIUS, 0.f, 0.f);
    s_contact[leg] = (a.flags & LT_RENDER_CONTACT_TINT) && a.force_hist[3 * qs + (long long)e * 4 + leg] > CONTACT_N;
  } else if (tid == 4) {  // trunk and what is fixed to it (URDF `trunk`, `back_mid`, `back`, rail cylinders along x)
    const float th[3] = LT_TRUNK_BOX_HALF_INIT;
    s_pose[0] = p0.x; s_pose[1] = p0.y; s_pose[2] = p0.z; s_pose[3] = q0.w; s_pose[4] = q0.x; s_pose[5] = q0.y; s_pose[6] = q0.z;
    make_prim(s_prim[LT_PRIM_TRUNK], P_BOX, p0, q0, f3(0.f, 0.f, 0.f), 0, th[0], th[1], th[2]);
    // back_mid: box 0.25 x 0.194 x 0.083 centred 0.0415 above the trunk origin; its top meets the plate's underside
    make_prim(s_prim[LT_PRIM_BACK_MID], P_BOX, p0, q0, f3(0.f, 0.f, 0.5f * LT_RAIL_Z), 0, LT_BACK_HALF_X, LT_RAIL_Y + LT_RAIL_RADIUS, 0.5f * LT_RAIL_Z);
    make_prim(s_prim[LT_PRIM_PLATE], P_BOX, p0, q0, f3(0.f, 0.f, 0.5f * (LT_BACK_TOP_Z + LT_RAIL_Z)), 0, LT_BACK_HALF_X, LT_BACK_HALF_Y,
              0.5f * (LT_BACK_TOP_Z - LT_RAIL_Z));
    make_prim(s_prim[LT_PRIM_RAIL_LEFT], P_CYL, p0, q0, f3(0.f, LT_RAIL_Y, LT_RAIL_Z), 1, LT_RAIL_RADIUS, LT_BACK_HALF_X, 0.f);
    make_prim(s_prim[LT_PRIM_RAIL_RIGHT], P_CYL, p0, q0, f3(0.f, -LT_RAIL_Y, LT_RAIL_Z), 1, LT_RAIL_RADIUS, LT_BACK_HALF_X, 0.f);
  } else if (tid == 5) {  // object cylinder (axis = object y) and the ground
    if (a.has_obj) {
      const F3 po = f3(quad(a.obj_pos, qs, e, 0), quad(a.obj_pos, qs, e, 1), quad(a.obj_pos, qs, e, 2));
      const Q4 qo = {quad(a.obj_quat, qs, e, 0), quad(a.obj_quat, qs, e, 1), quad(a.obj_quat, qs, e, 2), quad(a.obj_quat, qs, e, 3)};
      make_prim(s_prim[LT_PRIM_OBJECT], P_CYL, po, qo, f3(0.f, 0.f, 0.f), 0, quad(a.obj_params, qs, e, 0), 0.5f * quad(a.obj_params, qs, e, 1), 0.f);
    } else {
      s_prim[LT_PRIM_OBJECT].type = P_NONE;
    }
    s_prim[LT_PRIM_GROUND].type = P_PLANE;
  } else if (tid == 6) {  // camera basis: forward, right = forward x z (x y when looking straight up / down), up = right x forward
    F3 eye = f3(V.eye[0], V.eye[1], V.eye[2]), at = f3(V.lookat[0], V.lookat[1], V.lookat[2]);
    if (V.origin == LT_RENDER_ORIGIN_ASSET_ROOT) { eye = eye + p0; at = at + p0; }
    const F3 fw = normalize(at - eye);
    F3 rt = cross(fw, f3(0.f, 0.f, 1.f));
    if (dot(rt, rt) < 1e-12f) rt = cross(fw, f3(0.f, 1.f, 0.f));
    rt = normalize(rt);
    const F3 up = cross(rt, fw);
    const float v[13] = {eye.x, eye.y, eye.z, fw.x, fw.y, fw.z, rt.x, rt.y, rt.z, up.x, up.y, up.z, tanf(0.5f * V.fov_y_deg * 0.017453292519943295f)};
    for (int k = 0; k < 13; ++k) s_cam[k] = v[k];
  }
  __syncthreads();
  const int view = a.view0 + (int)blockIdx.z;
  if (a.poses && blockIdx.x == 0 && blockIdx.y == 0 && tid < LT_NUM_SENSOR_BODIES * 7) a.poses[(long long)view * LT_NUM_SENSOR_BODIES * 7 + tid] = s_pose[tid];

  const F3 eye = f3(s_cam[0], s_cam[1], s_cam[2]), fw = f3(s_cam[3], s_cam[4], s_cam[5]), rt = f3(s_cam[6], s_cam[7], s_cam[8]),
           up = f3(s_cam[9], s_cam[10], s_cam[11]);
  const float W = (float)a.width, H = (float)a.height, tanh_ = s_cam[12], aspect = W / H;
  auto ray = [&](float sx, float sy) {  // direction through continuous pixel coordinates (sx, sy), y down
    return normalize(fw + ((sx * 2.f / W - 1.f) * tanh_ * aspect) * rt + ((1.f - sy * 2.f / H) * tanh_) * up);
  };
  F3 L = normalize(f3(a.light[0], a.light[1], a.light[2]));
  const int lane = tid & 63, wave = tid >> 6;
  const int px = (int)blockIdx.x * TILE_W + lane;
  const int x0 = (int)blockIdx.x * TILE_W, x1 = min(x0 + TILE_W, a.width);
  for (int r = wave; r < TILE_H; r += 4) {
    const int py = (int)blockIdx.y * TILE_H + r;
    if (py >= a.height) break;  // wave-uniform
    // strip frustum: planes through the eye and the strip's corner rays; lane i tests primitive i's bounding sphere
    const F3 c00 = ray((float)x0, (float)py), c10 = ray((float)x1, (float)py), c01 = ray((float)x0, (float)py + 1.f),
             c11 = ray((float)x1, (float)py + 1.f);
    const F3 mid = normalize(c00 + c10 + c01 + c11);
    bool keep = false;
    if (lane < NPRIM) {
      const Prim& P = s_prim[lane];
      if (P.type == P_PLANE) keep = true;
      else if (P.type != P_NONE) {
        const F3 cv = f3(P.bs[0], P.bs[1], P.bs[2]) - eye;
        const F3 pl[4] = {cross(c00, c01), cross(c11, c10), cross(c10, c00), cross(c01, c11)};
        keep = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          F3 nrm = normalize(pl[k]);
          if (dot(nrm, mid) < 0.f) nrm = -1.f * nrm;
          if (dot(nrm, cv) < -P.bs[3]) keep = false;
        }
      }
    }
    uint64_t mask = __ballot(keep);
    if (px >= a.width) continue;
    const F3 d = ray((float)px + 0.5f, (float)py + 0.5f);
    float tbest = T_MISS;
    int id = -1;
    F3 nbest = f3(0.f, 0.f, 1.f);
    while (mask) {
      const int i = __builtin_ctzll(mask);
      mask &= mask - 1;
      F3 n;
      const float t = intersect(s_prim[i], eye, d, 0.f, tbest, n);
      if (t < tbest) { tbest = t; id = i; nbest = n; }
    }
    F3 col = f3(0.55f, 0.70f, 0.90f);  // sky
    if (id >= 0) {
      const F3 ph = eye + tbest * d;
      F3 base;
      if (id == LT_PRIM_GROUND) {
        const int parity = ((int)floorf(ph.x * 2.f) + (int)floorf(ph.y * 2.f)) & 1;
        base = parity ? f3(0.62f, 0.62f, 0.60f) : f3(0.42f, 0.42f, 0.40f);
      } else {
        base = albedo(id);
        if (id >= LT_PRIM_FOOT && id < LT_PRIM_OBJECT && s_contact[id - LT_PRIM_FOOT]) base = f3(0.95f, 0.15f, 0.10f);
        if (id == LT_PRIM_PLATE && (a.flags & LT_RENDER_TAXELS)) {  // taxel grid on the top face (trunk frame x, y)
          const Prim& P = s_prim[LT_PRIM_PLATE];
          const F3 w = ph - f3(P.c[0], P.c[1], P.c[2]);
          const float lx = P.R[0] * w.x + P.R[3] * w.y + P.R[6] * w.z, ly = P.R[1] * w.x + P.R[4] * w.y + P.R[7] * w.z;
          const float lnz = P.R[2] * nbest.x + P.R[5] * nbest.y + P.R[8] * nbest.z;
          if (lnz > 0.5f) {
            const int row = (int)rintf((LT_TAXEL_X0 - lx) * (1.f / LT_TAXEL_DX)), cl = (int)rintf((LT_TAXEL_Y0 - ly) * (1.f / LT_TAXEL_DY));
            if (row >= 0 && row < LT_TAXEL_ROWS && cl >= 0 && cl < LT_TAXEL_COLS &&
                fabsf(lx - (LT_TAXEL_X0 - LT_TAXEL_DX * (float)row)) <= 0.4f * LT_TAXEL_DX &&
                fabsf(ly - (LT_TAXEL_Y0 - LT_TAXEL_DY * (float)cl)) <= 0.4f * LT_TAXEL_DY) {
              const bool on = a.tactile && a.tactile[(long long)e * a.tactile_stride + row * LT_TAXEL_COLS + cl] > 0.5f;
              base = on ? f3(0.95f, 0.20f, 0.55f) : f3(0.62f, 0.64f, 0.66f);
            }
          }
        }
      }
      float ndl = dot(nbest, L);
      ndl = ndl > 0.f ? ndl : 0.f;
      if (ndl > 0.f && (a.flags & LT_RENDER_SHADOWS)) {  // one shadow ray towards the light, against every primitive but the ground
        const F3 so = ph + 1e-4f * nbest;
        for (int i = 0; i < LT_PRIM_GROUND; ++i) {
          F3 n;
          if (s_prim[i].type != P_NONE && intersect(s_prim[i], so, L, 0.f, T_MISS, n) < T_MISS) { ndl = 0.f; break; }
        }
      }
      col = (AMBIENT + (1.f - AMBIENT) * ndl) * base;
    }
    const long long o = ((long long)view * a.height + py) * a.width + px;
    a.rgba[o] = pack(col);
    if (a.depth) a.depth[o] = id >= 0 ? tbest : (float)LT_RENDER_DEPTH_MISS;
    if (a.ids) a.ids[o] = id;
  }
}

}  // namespace

int lt_launch_render(const lt_env* env, const lt_render_desc* desc, const lt_render_view* views, int nviews, uint32_t* rgba, float* depth,
                     int32_t* ids, float* poses, void* stream) {
  static_assert(sizeof(RenderArgs) <= 4096, "kernel arguments too large");
  const lt_layout& L = env->layout;
  const char* base = (const char*)env->arena;
  RenderArgs a = {};
  auto q = [&](int f) { return (const float*)(base + L.quad_off[f]); };  // == lt_env_get_view(f).ptr
  a.root_pos = q(LT_F_ROOT_POS); a.root_quat = q(LT_F_ROOT_QUAT); a.joint_pos = q(LT_F_JOINT_POS);
  a.obj_pos = q(LT_F_OBJ_POS); a.obj_quat = q(LT_F_OBJ_QUAT); a.obj_params = q(LT_F_OBJ_PARAMS); a.force_hist = q(LT_F_FORCE_HIST);
  a.qstride = L.npad * 4;
  a.has_obj = env->cfg.task == LT_TASK_TRANSPORT_TEACHER;
  if (L.tactile) {  // == lt_env_get_view(LT_F_OBS_TACTILE): [N][lt_cfg_tactile_dim]
    a.tactile = (const float*)(base + L.off_obs_tactile);
    a.tactile_stride = lt_cfg_tactile_dim(&env->cfg);
  }
  a.width = desc->width; a.height = desc->height; a.flags = desc->flags;
  for (int k = 0; k < 3; ++k) a.light[k] = desc->light_dir[k];
  a.rgba = rgba; a.depth = depth; a.ids = ids; a.poses = poses;
  const dim3 grid((unsigned)((desc->width + TILE_W - 1) / TILE_W), (unsigned)((desc->height + TILE_H - 1) / TILE_H), 1);
  for (int v0 = 0; v0 < nviews; v0 += LT_RENDER_VIEWS_PER_LAUNCH) {
    const int nv = min(LT_RENDER_VIEWS_PER_LAUNCH, nviews - v0);
    a.view0 = v0; a.nview = nv;
    for (int k = 0; k < nv; ++k) a.views[k] = views[v0 + k];
    hipLaunchKernelGGL(lt_render_kernel, dim3(grid.x, grid.y, (unsigned)nv), dim3(256), 0, (hipStream_t)stream, a);
    const int err = (int)hipGetLastError();
    if (err) return err;
  }
  return 0;
}
