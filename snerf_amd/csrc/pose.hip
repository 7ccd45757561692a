// Learned camera pose on the device (pose_refine = True of both shipped S-NeRF configs): the pose branch of sample_rays
// (s-nerf/utils/sample_utils.py:421-435) on one row of the LearnPose table (model/poses.py:6-36, utils/lie_group_helper.py:47-81),
// and the reduction of the step's ray gradients to that row's gradient.
//
//   R = I + (sin th / th) K + ((1 - cos th) / th^2) K^2,   K = skew(r),   th = |r| + 1e-15        (lie_group_helper.py:60-70, as written)
//   directions' = R d,   viewdirs' = R v,   origins' = o + t                                     (the origins are shifted, not rotated)
//
// R is formed in double from the fp32 row and rounded once; the per-ray products are separate fp32 ops (this unit is built with
// -ffp-contract=off).  At r = 0 every entry of K is a zero, so R = I exactly and the transformed rays are the inputs bit for bit.
// The camera index comes from device memory (int64 [1], the batchers' `img` output: no host read) or from the host; an index outside the
// table makes the kernels return without a store.
//
// The COMPOSED form (test-time pose refinement, s-nerf/eval.py:77-114: rays generated from make_c2w(r, t) @ init_c2w[img]) turns the
// camera centre as well: origins' = (R o) + t on the rays of the initial pose, and the rotation's gradient gains sum g_o o^T
// (snerf_pose_compose_apply / snerf_pose_compose_grad: the same kernels, instantiated with COMPOSE).
#include "common.h"
#include <math.h>

// the [3,3] rotation of an axis-angle row, in double
__device__ __forceinline__ void pose_rotation(const float* __restrict__ r, double R[9]) {
  const double x = (double)r[0], y = (double)r[1], z = (double)r[2];
  const double th = sqrt((x * x + y * y) + z * z) + 1e-15;
  const double A = sin(th) / th, B = (1.0 - cos(th)) / (th * th);
  const double K[9] = {0.0, -z, y, z, 0.0, -x, -y, x, 0.0};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double k2 = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
      R[3 * i + j] = (i == j ? 1.0 : 0.0) + A * K[3 * i + j] + B * k2;
    }
}

struct PoseApply {
  const float *r, *t;               // [n_cams,3]; t nullable
  int n_cams;
  const long* cam_dev; int cam_host;
  const float *o, *d, *v;           // [n,3]
  long n;
  float *o_out, *d_out, *v_out;     // [n,3]
  float* pose_out;                  // [3,4], nullable
};

template <bool COMPOSE>
__global__ __launch_bounds__(256) void pose_apply_kernel(PoseApply a) {
  __shared__ float s_R[9], s_t[3];
  __shared__ int s_ok;
  if (threadIdx.x == 0) {
    const long cam = a.cam_dev != nullptr ? a.cam_dev[0] : (long)a.cam_host;
    s_ok = cam >= 0 && cam < a.n_cams;
    if (s_ok) {
      double R[9];
      pose_rotation(a.r + 3 * cam, R);
#pragma unroll
      for (int k = 0; k < 9; ++k) s_R[k] = (float)R[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) s_t[k] = a.t != nullptr ? a.t[3 * cam + k] : 0.f;
      if (blockIdx.x == 0 && a.pose_out != nullptr) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
          for (int j = 0; j < 3; ++j) a.pose_out[4 * i + j] = s_R[3 * i + j];
          a.pose_out[4 * i + 3] = s_t[i];
        }
      }
    }
  }
  __syncthreads();
  if (!s_ok) return;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const float d0 = a.d[3 * i], d1 = a.d[3 * i + 1], d2 = a.d[3 * i + 2];
  const float v0 = a.v[3 * i], v1 = a.v[3 * i + 1], v2 = a.v[3 * i + 2];
  if constexpr (COMPOSE) {
    const float o0 = a.o[3 * i], o1 = a.o[3 * i + 1], o2 = a.o[3 * i + 2];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float r0 = s_R[3 * c], r1 = s_R[3 * c + 1], r2 = s_R[3 * c + 2];
      a.d_out[3 * i + c] = (r0 * d0 + r1 * d1) + r2 * d2;
      a.v_out[3 * i + c] = (r0 * v0 + r1 * v1) + r2 * v2;
      const float ro = (r0 * o0 + r1 * o1) + r2 * o2;
      a.o_out[3 * i + c] = a.t != nullptr ? ro + s_t[c] : ro;
    }
    return;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float r0 = s_R[3 * c], r1 = s_R[3 * c + 1], r2 = s_R[3 * c + 2];
    a.d_out[3 * i + c] = (r0 * d0 + r1 * d1) + r2 * d2;
    a.v_out[3 * i + c] = (r0 * v0 + r1 * v1) + r2 * v2;
    a.o_out[3 * i + c] = a.t != nullptr ? a.o[3 * i + c] + s_t[c] : a.o[3 * i + c];
  }
}

// do [a, a + la) and [b, b + lb) (bytes) share memory?
static inline bool pose_overlap(const float* a, uintptr_t la, const float* b, uintptr_t lb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a != nullptr && b != nullptr && x < y + lb && y < x + la;
}

template <bool COMPOSE>
static int pose_apply_go(const float* r, const float* t, int n_cams, const long* cam_dev, int cam_host, const float* origins,
                         const float* directions, const float* viewdirs, long n, float* origins_out, float* directions_out,
                         float* viewdirs_out, float* pose_out, void* stream) {
  if (n == 0) return SNERF_OK;
  if (n < 0 || n_cams < 1 || r == nullptr) return SNERF_ERR_ARG;
  if (cam_dev == nullptr && (cam_host < 0 || cam_host >= n_cams)) return SNERF_ERR_ARG;
  if (origins == nullptr || directions == nullptr || viewdirs == nullptr || origins_out == nullptr || directions_out == nullptr ||
      viewdirs_out == nullptr)
    return SNERF_ERR_ARG;
  // the backward needs the untransformed directions / viewdirs: no output may share memory with an input, nor (a race) with another output
  const uintptr_t len = (uintptr_t)n * 12;
  const float* in[3] = {origins, directions, viewdirs};
  const float* out[3] = {origins_out, directions_out, viewdirs_out};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      if (pose_overlap(out[i], len, in[j], len)) return SNERF_ERR_ARG;
    for (int j = i + 1; j < 3; ++j)
      if (pose_overlap(out[i], len, out[j], len)) return SNERF_ERR_ARG;
    if (pose_overlap(out[i], len, pose_out, 48)) return SNERF_ERR_ARG;
  }
  PoseApply a{r, t, n_cams, cam_dev, cam_host, origins, directions, viewdirs, n, origins_out, directions_out, viewdirs_out, pose_out};
  hipLaunchKernelGGL(pose_apply_kernel<COMPOSE>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return snerf_check_launch();
}

extern "C" int snerf_pose_apply(const float* r, const float* t, int n_cams, const long* cam_dev, int cam_host, const float* origins,
                                const float* directions, const float* viewdirs, long n, float* origins_out, float* directions_out,
                                float* viewdirs_out, float* pose_out, void* stream) {
  return pose_apply_go<false>(r, t, n_cams, cam_dev, cam_host, origins, directions, viewdirs, n, origins_out, directions_out, viewdirs_out,
                              pose_out, stream);
}

extern "C" int snerf_pose_compose_apply(const float* r, const float* t, int n_cams, const long* cam_dev, int cam_host, const float* origins,
                                        const float* directions, const float* viewdirs, long n, float* origins_out, float* directions_out,
                                        float* viewdirs_out, float* pose_out, void* stream) {
  return pose_apply_go<true>(r, t, n_cams, cam_dev, cam_host, origins, directions, viewdirs, n, origins_out, directions_out, viewdirs_out,
                             pose_out, stream);
}

// ---------------------------------------------------------------------------
// Pose gradient.  Twelve sums over the rays, g_t = sum g_o and G[i][j] = sum (g_d[i] d[j] + g_v[i] v[j]) = d loss / d R[i][j] with the
// UNtransformed d, v, accumulated in double in an order that depends on n only: ray i belongs to thread i mod (256 blocks(n)) and is
// taken in ascending order, the 64 lanes of a wave fold with shuffles, the 4 waves of a workgroup through LDS in wave order, the
// workgroups' partials (ws[12 b + k]) in block order by the second launch.  No floating-point atomics: the same bits every run.
// The second launch (one wave) chains G to the table row in double, as autograd sees the formula above:
//   dL/dr_k = A <G, E_k> + B <G, E_k K + K E_k> + (A' <G, K> + B' <G, K^2>) r_k / |r|,    E_k = dK/dr_k,
//   A' = (th cos th - sin th) / th^2,   B' = (th sin th - 2 (1 - cos th)) / th^3,
// without the last term at |r| = 0 (the norm's subgradient there is 0: training starts there), rounds once to fp32 and ADDS into row
// `cam` of grad_r / grad_t.
// COMPOSE: the rotation reached the origins too, G[i][j] = sum ((g_d[i] d[j] + g_v[i] v[j]) + g_o[i] o[j]) with the UNtransformed o -- still
// twelve sums, the same scratch, the same fold and chain.
// ---------------------------------------------------------------------------
#define POSE_MAX_BLOCKS 256
static inline int pose_grad_blocks(long n) {
  const long b = (n + 255) / 256;
  return b < 1 ? 1 : (b > POSE_MAX_BLOCKS ? POSE_MAX_BLOCKS : (int)b);
}

extern "C" long snerf_pose_grad_ws(long n) { return n <= 0 ? 0 : 12L * pose_grad_blocks(n); }

struct PoseGrad {
  const float* r; int n_cams;
  const long* cam_dev; int cam_host;
  const float *g_o, *g_d, *g_v, *d, *v;   // [n,3]; g_o nullable (no translation gradient wanted; never in the composed form)
  const float* o;                         // [n,3] untransformed origins: the composed form only
  long n;
  double* ws;                             // [12 blocks]
  int blocks;
  float *grad_r, *grad_t;                 // [n_cams,3], each nullable
};

__device__ __forceinline__ bool pose_cam(const long* cam_dev, int cam_host, int n_cams, long* cam) {
  *cam = cam_dev != nullptr ? cam_dev[0] : (long)cam_host;
  return *cam >= 0 && *cam < n_cams;
}

template <bool COMPOSE>
__global__ __launch_bounds__(256) void pose_grad_partial_kernel(PoseGrad a) {
  __shared__ double red[4][12];
  long cam;
  if (!pose_cam(a.cam_dev, a.cam_host, a.n_cams, &cam)) return;      // (uniform over the grid)
  double acc[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) acc[k] = 0.0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (long)gridDim.x * 256) {
    double d[3], v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { d[c] = (double)a.d[3 * i + c]; v[c] = (double)a.v[3 * i + c]; }
    if constexpr (COMPOSE) {
      double o[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = (double)a.o[3 * i + c];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double gd = (double)a.g_d[3 * i + c], gv = (double)a.g_v[3 * i + c], go = (double)a.g_o[3 * i + c];
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[3 * c + j] += (gd * d[j] + gv * v[j]) + go * o[j];
        acc[9 + c] += go;
      }
      continue;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double gd = (double)a.g_d[3 * i + c], gv = (double)a.g_v[3 * i + c];
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[3 * c + j] += gd * d[j] + gv * v[j];
      if (a.g_o != nullptr) acc[9 + c] += (double)a.g_o[3 * i + c];
    }
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 12; ++k) red[threadIdx.x >> 6][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < 12) a.ws[12 * (long)blockIdx.x + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

__device__ __forceinline__ double dot9(const double* a, const double* b) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) s += a[k] * b[k];
  return s;
}

__device__ __forceinline__ void mul33(const double* a, const double* b, double* c) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}

// G [3,3] = d loss / d R and the table row r -> d loss / d r, in double
__device__ __forceinline__ void pose_chain(const double* G, const float* r, double g[3]) {
  const double x = (double)r[0], y = (double)r[1], z = (double)r[2];
  const double rv[3] = {x, y, z};
  const double nr = sqrt((x * x + y * y) + z * z), th = nr + 1e-15;
  const double sn = sin(th), cs = cos(th);
  const double A = sn / th, B = (1.0 - cs) / (th * th);
  const double dA = (th * cs - sn) / (th * th), dB = (th * sn - 2.0 * (1.0 - cs)) / (th * th * th);
  const double K[9] = {0.0, -z, y, z, 0.0, -x, -y, x, 0.0};
  double K2[9];
  mul33(K, K, K2);
  const double radial = nr > 0.0 ? dA * dot9(G, K) + dB * dot9(G, K2) : 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double E[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int p = (k + 1) % 3, q = (k + 2) % 3;           // E_k[q][p] = 1, E_k[p][q] = -1
    E[3 * q + p] = 1.0; E[3 * p + q] = -1.0;
    double EK[9], KE[9];
    mul33(E, K, EK);
    mul33(K, E, KE);
#pragma unroll
    for (int e = 0; e < 9; ++e) EK[e] += KE[e];
    g[k] = A * dot9(G, E) + B * dot9(G, EK);
    if (nr > 0.0) g[k] += radial * (rv[k] / nr);
  }
}

__global__ __launch_bounds__(64) void pose_grad_finish_kernel(PoseGrad a) {
  __shared__ double s[12];
  long cam;
  if (!pose_cam(a.cam_dev, a.cam_host, a.n_cams, &cam)) return;
  if (threadIdx.x < 12) {
    double acc = 0.0;
    for (int b = 0; b < a.blocks; ++b) acc += a.ws[12 * (long)b + threadIdx.x];
    s[threadIdx.x] = acc;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (a.grad_t != nullptr) {
#pragma unroll
    for (int c = 0; c < 3; ++c) a.grad_t[3 * cam + c] += (float)s[9 + c];
  }
  if (a.grad_r == nullptr) return;
  double g[3];
  pose_chain(s, a.r + 3 * cam, g);
#pragma unroll
  for (int k = 0; k < 3; ++k) a.grad_r[3 * cam + k] += (float)g[k];
}

extern "C" int snerf_pose_grad(const float* r, int n_cams, const long* cam_dev, int cam_host, const float* g_o, const float* g_d,
                               const float* g_v, const float* directions, const float* viewdirs, long n, double* ws, long ws_doubles,
                               float* grad_r, float* grad_t, void* stream) {
  if (n == 0) return SNERF_OK;
  if (n < 0 || n_cams < 1 || r == nullptr) return SNERF_ERR_ARG;
  if (cam_dev == nullptr && (cam_host < 0 || cam_host >= n_cams)) return SNERF_ERR_ARG;
  if (g_d == nullptr || g_v == nullptr || directions == nullptr || viewdirs == nullptr) return SNERF_ERR_ARG;
  if ((grad_r == nullptr && grad_t == nullptr) || (grad_t != nullptr && g_o == nullptr)) return SNERF_ERR_ARG;
  const int blocks = pose_grad_blocks(n);
  if (ws == nullptr || ws_doubles < 12L * blocks) return SNERF_ERR_ARG;
  PoseGrad a{r, n_cams, cam_dev, cam_host, grad_t != nullptr ? g_o : nullptr, g_d, g_v, directions, viewdirs, nullptr, n, ws, blocks, grad_r, grad_t};
  hipLaunchKernelGGL(pose_grad_partial_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(pose_grad_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
  return snerf_check_launch();
}

extern "C" int snerf_pose_compose_grad(const float* r, int n_cams, const long* cam_dev, int cam_host, const float* g_o, const float* g_d,
                                       const float* g_v, const float* origins, const float* directions, const float* viewdirs, long n,
                                       double* ws, long ws_doubles, float* grad_r, float* grad_t, void* stream) {
  if (n == 0) return SNERF_OK;
  if (n < 0 || n_cams < 1 || r == nullptr) return SNERF_ERR_ARG;
  if (cam_dev == nullptr && (cam_host < 0 || cam_host >= n_cams)) return SNERF_ERR_ARG;
  if (g_o == nullptr || g_d == nullptr || g_v == nullptr || origins == nullptr || directions == nullptr || viewdirs == nullptr) return SNERF_ERR_ARG;
  if (grad_r == nullptr && grad_t == nullptr) return SNERF_ERR_ARG;
  const int blocks = pose_grad_blocks(n);
  if (ws == nullptr || ws_doubles < 12L * blocks) return SNERF_ERR_ARG;
  PoseGrad a{r, n_cams, cam_dev, cam_host, g_o, g_d, g_v, directions, viewdirs, origins, n, ws, blocks, grad_r, grad_t};
  hipLaunchKernelGGL(pose_grad_partial_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(pose_grad_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
  return snerf_check_launch();
}

// ---------------------------------------------------------------------------
// Per-ray learned poses (path C: s-nerfpp/zipnerf/train.py:177-213, internal/posenet_v2.py).  A batch mixes cameras: every ray carries
// the row of the table that moves it (batch['glo_idx']), five ray tensors turn -- directions, viewdirs, base_x, base_y get R x, origins
// get + t -- and the translation is t * t_ratio (posenet_v2.py:89,99).  snerf_pose_table forms the [R | t * t_ratio] rows once per
// step, snerf_pose_rays_apply gathers a ray's row, snerf_pose_rays_grad reduces the step's ray gradients camera by camera.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pose_table_kernel(const float* __restrict__ r, const float* __restrict__ t, int n_cams, float t_ratio,
                                                         float* __restrict__ table) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n_cams) return;
  double R[9];
  pose_rotation(r + 3 * (long)c, R);
  float* row = table + 12 * (long)c;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) row[4 * i + j] = (float)R[3 * i + j];
    row[4 * i + 3] = t != nullptr ? t[3 * (long)c + i] * t_ratio : 0.f;
  }
}

extern "C" int snerf_pose_table(const float* r, const float* t, int n_cams, float t_ratio, float* table_out, void* stream) {
  if (n_cams < 1 || r == nullptr || table_out == nullptr) return SNERF_ERR_ARG;
  const uintptr_t len = (uintptr_t)n_cams * 12;
  if (pose_overlap(table_out, 4 * len, r, len) || pose_overlap(table_out, 4 * len, t, len)) return SNERF_ERR_ARG;
  hipLaunchKernelGGL(pose_table_kernel, dim3((unsigned)((n_cams + 255) / 256)), dim3(256), 0, (hipStream_t)stream, r, t, n_cams, t_ratio,
                     table_out);
  return snerf_check_launch();
}

// the row of a ray: its fp32 index truncated toward zero (the reference's .int()); -1 = outside the table (NaN included)
__device__ __forceinline__ int pose_ray_cam(float c, int n_cams) { return (c > -1.f && c < (float)n_cams) ? (int)c : -1; }

struct PoseRays {
  const float* table; int n_cams;   // [n_cams,3,4]
  const float* cam;                 // [n]
  const float* in[5];               // origins, directions, viewdirs, base_x, base_y [n,3]
  float* out[5];
  long n;
};

__global__ __launch_bounds__(256) void pose_rays_apply_kernel(PoseRays a) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const int c = pose_ray_cam(a.cam[i], a.n_cams);
  if (c < 0) {                                          // copied through unchanged
#pragma unroll
    for (int k = 0; k < 5; ++k)
#pragma unroll
      for (int e = 0; e < 3; ++e) a.out[k][3 * i + e] = a.in[k][3 * i + e];
    return;
  }
  float T[12];
  const float4* row = (const float4*)(a.table + 12 * (long)c);     // (rows are 48 bytes: 16-byte aligned with the table)
#pragma unroll
  for (int q = 0; q < 3; ++q) { const float4 w = row[q]; T[4 * q] = w.x; T[4 * q + 1] = w.y; T[4 * q + 2] = w.z; T[4 * q + 3] = w.w; }
#pragma unroll
  for (int e = 0; e < 3; ++e) a.out[0][3 * i + e] = a.in[0][3 * i + e] + T[4 * e + 3];
#pragma unroll
  for (int k = 1; k < 5; ++k) {
    const float x0 = a.in[k][3 * i], x1 = a.in[k][3 * i + 1], x2 = a.in[k][3 * i + 2];
#pragma unroll
    for (int e = 0; e < 3; ++e) a.out[k][3 * i + e] = (T[4 * e] * x0 + T[4 * e + 1] * x1) + T[4 * e + 2] * x2;
  }
}

extern "C" int snerf_pose_rays_apply(const float* table, int n_cams, const float* cam, const float* origins, const float* directions,
                                     const float* viewdirs, const float* base_x, const float* base_y, long n, float* origins_out,
                                     float* directions_out, float* viewdirs_out, float* base_x_out, float* base_y_out, void* stream) {
  if (n == 0) return SNERF_OK;
  if (n < 0 || n_cams < 1 || table == nullptr || cam == nullptr || ((uintptr_t)table & 15)) return SNERF_ERR_ARG;
  PoseRays a{table, n_cams, cam, {origins, directions, viewdirs, base_x, base_y},
             {origins_out, directions_out, viewdirs_out, base_x_out, base_y_out}, n};
  // the backward needs the untransformed rays: no output may share memory with an input, the table or the indices, nor with another output
  const uintptr_t len = (uintptr_t)n * 12;
  for (int i = 0; i < 5; ++i) {
    if (a.in[i] == nullptr || a.out[i] == nullptr) return SNERF_ERR_ARG;
    for (int j = 0; j < 5; ++j)
      if (pose_overlap(a.out[i], len, a.in[j], len)) return SNERF_ERR_ARG;
    for (int j = i + 1; j < 5; ++j)
      if (pose_overlap(a.out[i], len, a.out[j], len)) return SNERF_ERR_ARG;
    if (pose_overlap(a.out[i], len, table, (uintptr_t)n_cams * 48) || pose_overlap(a.out[i], len, cam, (uintptr_t)n * 4)) return SNERF_ERR_ARG;
  }
  hipLaunchKernelGGL(pose_rays_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return snerf_check_launch();
}

// ---------------------------------------------------------------------------
// Gradient of the table under snerf_pose_rays_apply, segmented by camera.  For every camera c that owns a ray
//   G_c[i][j] = sum over its rays of (g_d[i] d[j] + g_v[i] v[j]) + (g_bx[i] bx[j] + g_by[i] by[j]),    g_t,c = t_ratio * sum g_o
// with the UNtransformed d, v, bx, by.  Grid (n_cams, S): workgroup (c, s) walks the rays s 256 + lane, + 256 S, ... in ascending order,
// reads the index of each (coalesced) and loads the 27 floats of the rays of camera c only; 12 sums and the ray count fold in double,
// lane -> wave -> workgroup as in pose_grad_partial_kernel, into ws[(c S + s) 13 + k].  The finish launch, one thread per camera, folds the
// S slices in order, leaves a camera without a ray alone (no store), chains G_c to its row (pose_chain), rounds once and ADDS.  No
// floating-point atomics; S depends on (n, n_cams) only: the same bits every run.  Cost: n_cams n index reads out of L2.
// ---------------------------------------------------------------------------
#define POSE_RAYS_WG 2048            // workgroups aimed at: S = ceil(POSE_RAYS_WG / n_cams), at most one per 256 rays
static inline int pose_rays_slices(long n, int n_cams) {
  const int want = (POSE_RAYS_WG + n_cams - 1) / n_cams, have = pose_grad_blocks(n);
  return want < have ? want : have;
}

extern "C" long snerf_pose_rays_grad_ws(long n, int n_cams) { return (n <= 0 || n_cams < 1) ? 0 : 13L * n_cams * pose_rays_slices(n, n_cams); }

struct PoseRaysGrad {
  const float* r; int n_cams; float t_ratio;
  const float* cam;                                     // [n]
  const float *g_o, *g_d, *g_v, *g_bx, *g_by;           // [n,3]; g_o nullable (no translation gradient wanted)
  const float *d, *v, *bx, *by;                         // [n,3], untransformed
  long n;
  double* ws;                                           // [n_cams, slices, 13]
  int slices;
  float *grad_r, *grad_t;                               // [n_cams,3], each nullable
};

__global__ __launch_bounds__(256) void pose_rays_grad_partial_kernel(PoseRaysGrad a) {
  __shared__ double red[4][13];
  const int c = blockIdx.x;
  double acc[13];
#pragma unroll
  for (int k = 0; k < 13; ++k) acc[k] = 0.0;
  for (long i = (long)blockIdx.y * 256 + threadIdx.x; i < a.n; i += (long)gridDim.y * 256) {
    if (pose_ray_cam(a.cam[i], a.n_cams) != c) continue;
    double d[3], v[3], bx[3], by[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      d[e] = (double)a.d[3 * i + e]; v[e] = (double)a.v[3 * i + e]; bx[e] = (double)a.bx[3 * i + e]; by[e] = (double)a.by[3 * i + e];
    }
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const double gd = (double)a.g_d[3 * i + e], gv = (double)a.g_v[3 * i + e], gx = (double)a.g_bx[3 * i + e], gy = (double)a.g_by[3 * i + e];
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[3 * e + j] += (gd * d[j] + gv * v[j]) + (gx * bx[j] + gy * by[j]);
      if (a.g_o != nullptr) acc[9 + e] += (double)a.g_o[3 * i + e];
    }
    acc[12] += 1.0;
  }
#pragma unroll
  for (int k = 0; k < 13; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 13; ++k) red[threadIdx.x >> 6][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < 13)
    a.ws[13 * ((long)c * a.slices + blockIdx.y) + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

__global__ __launch_bounds__(64) void pose_rays_grad_finish_kernel(PoseRaysGrad a) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= a.n_cams) return;
  double s[13];
#pragma unroll
  for (int k = 0; k < 13; ++k) s[k] = 0.0;
  for (int b = 0; b < a.slices; ++b) {
    const double* w = a.ws + 13 * ((long)c * a.slices + b);
#pragma unroll
    for (int k = 0; k < 13; ++k) s[k] += w[k];
  }
  if (s[12] == 0.0) return;                             // no ray of this camera in the batch: its rows keep their bits
  if (a.grad_t != nullptr) {
#pragma unroll
    for (int e = 0; e < 3; ++e) a.grad_t[3 * (long)c + e] += (float)((double)a.t_ratio * s[9 + e]);
  }
  if (a.grad_r == nullptr) return;
  double g[3];
  pose_chain(s, a.r + 3 * (long)c, g);
#pragma unroll
  for (int k = 0; k < 3; ++k) a.grad_r[3 * (long)c + k] += (float)g[k];
}

extern "C" int snerf_pose_rays_grad(const float* r, int n_cams, float t_ratio, const float* cam, const float* g_o, const float* g_d,
                                    const float* g_v, const float* g_bx, const float* g_by, const float* directions, const float* viewdirs,
                                    const float* base_x, const float* base_y, long n, double* ws, long ws_doubles, float* grad_r,
                                    float* grad_t, void* stream) {
  if (n == 0) return SNERF_OK;
  if (n < 0 || n_cams < 1 || r == nullptr || cam == nullptr) return SNERF_ERR_ARG;
  if (g_d == nullptr || g_v == nullptr || g_bx == nullptr || g_by == nullptr || directions == nullptr || viewdirs == nullptr ||
      base_x == nullptr || base_y == nullptr)
    return SNERF_ERR_ARG;
  if ((grad_r == nullptr && grad_t == nullptr) || (grad_t != nullptr && g_o == nullptr)) return SNERF_ERR_ARG;
  const int slices = pose_rays_slices(n, n_cams);
  if (ws == nullptr || ws_doubles < 13L * n_cams * slices) return SNERF_ERR_ARG;
  PoseRaysGrad a{r, n_cams, t_ratio, cam, grad_t != nullptr ? g_o : nullptr, g_d, g_v, g_bx, g_by, directions, viewdirs, base_x, base_y, n, ws,
                 slices, grad_r, grad_t};
  hipLaunchKernelGGL(pose_rays_grad_partial_kernel, dim3((unsigned)n_cams, (unsigned)slices), dim3(256), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(pose_rays_grad_finish_kernel, dim3((unsigned)((n_cams + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
  return snerf_check_launch();
}
