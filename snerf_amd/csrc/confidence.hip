// Learned depth confidence on the device (depth_conf = True, precompute_conf = True of both shipped S-NeRF configs): the precomputed branch
// of calc_final_confidence (s-nerf/model/confidence.py:193-206) on the rays of one batch, and the reduction of the step's d loss / d conf
// to the gradient of one column of the Confidence.lambdas table (confidence.py:69).
//
//   w_k = sigmoid(lambdas[k, i]),   conf_r = (sum_k w_k maps[k, slot(i), row_r, col_r]) / (sum_k w_k),   conf_r = 1 on sky pixels
//
// The reference indexes the maps by the image's position in i_train and lambdas by the image index (confidence.py:193,196):
// slot_of_image carries the first, -1 for an image without maps.  w_k is formed in double from the fp32 table entry and rounded once; the
// sums run in the reference's mode order (final_conf_map = 0; += w_k map_k; /= w.sum()) as separate fp32 ops (this unit is built with
// -ffp-contract=off).  The image index comes from device memory (int64 [1], the batchers' `img` output: no host read) or from the host.
// An image outside the table or without maps gives conf = 1 on every ray and no gradient (the reference raises there); so does a ray
// whose (row, col) lies outside the H x W image, which the reference's indexing would refuse.
#include "common.h"
#include <math.h>

#define CONF_MAX_MODES 8

struct ConfArgs {
  const float* maps;                // [M,P,H,W]
  int M, P, H, W;
  const int* slot_of_image;         // [n_images]
  const float* lambdas;             // [M,n_images]
  int n_images;
  const unsigned char* sky;         // [n_images,H,W], nullable
  const long* img_dev; int img_host;
  const long* coords;               // [n,2] = (row, col)
  long n;
  float* conf;                      // [n]            (apply)
  const float* g_conf;              // [n]            (grad)
  double* ws;                       // [8 blocks]     (grad)
  int blocks;
  float* grad_lambdas;              // [M,n_images]   (grad)
};

// the image of the batch and its map slot; false = no maps for it (outside the table, slot -1, or a slot past the maps)
__device__ __forceinline__ bool conf_image(const ConfArgs& a, long* img, int* slot) {
  *img = a.img_dev != nullptr ? a.img_dev[0] : (long)a.img_host;
  if (*img < 0 || *img >= a.n_images) return false;
  *slot = a.slot_of_image[*img];
  return *slot >= 0 && *slot < a.P;
}

__device__ __forceinline__ double conf_sigmoid(float x) { return 1.0 / (1.0 + exp(-(double)x)); }

// offset of ray r's pixel inside one [H,W] map, or -1 when the ray takes no part (coordinates outside the image, sky)
__device__ __forceinline__ long conf_pixel(const ConfArgs& a, long img, long r) {
  const long row = a.coords[2 * r], col = a.coords[2 * r + 1];
  if (row < 0 || row >= a.H || col < 0 || col >= a.W) return -1;
  const long px = row * a.W + col;
  if (a.sky != nullptr && a.sky[(img * a.H) * a.W + px] != 0) return -1;
  return px;
}

__global__ __launch_bounds__(256) void conf_apply_kernel(ConfArgs a) {
  __shared__ float s_w[CONF_MAX_MODES], s_S;
  __shared__ long s_img;
  __shared__ int s_slot, s_ok;
  if (threadIdx.x == 0) {
    long img; int slot = 0;
    s_ok = conf_image(a, &img, &slot);
    s_img = img; s_slot = slot;
    if (s_ok) {
      float S = 0.f;
      for (int k = 0; k < a.M; ++k) {
        s_w[k] = (float)conf_sigmoid(a.lambdas[(long)k * a.n_images + img]);
        S = k == 0 ? s_w[0] : S + s_w[k];
      }
      s_S = S;
    }
  }
  __syncthreads();
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.n) return;
  float c = 1.f;
  if (s_ok) {
    const long px = conf_pixel(a, s_img, r);
    if (px >= 0) {
      const long HW = (long)a.H * a.W;
      const float* m = a.maps + (long)s_slot * HW + px;
      float acc = s_w[0] * m[0];
      for (int k = 1; k < a.M; ++k) acc = acc + s_w[k] * m[(long)k * a.P * HW];
      c = acc / s_S;
    }
  }
  a.conf[r] = c;
}

static inline bool conf_bad_common(const float* maps, int M, int P, int H, int W, const int* slot_of_image, const float* lambdas, int n_images,
                                   const long* img_dev, int img_host, const long* coords, long n) {
  if (n < 0 || M < 1 || M > CONF_MAX_MODES || P < 1 || H < 1 || W < 1 || n_images < 1) return true;
  if (maps == nullptr || slot_of_image == nullptr || lambdas == nullptr || coords == nullptr) return true;
  return img_dev == nullptr && (img_host < 0 || img_host >= n_images);
}

extern "C" int snerf_conf_apply(const float* maps, int M, int P, int H, int W, const int* slot_of_image, const float* lambdas, int n_images,
                                const unsigned char* sky, const long* img_dev, int img_host, const long* coords, long n, float* conf,
                                void* stream) {
  if (n == 0) return SNERF_OK;
  if (conf_bad_common(maps, M, P, H, W, slot_of_image, lambdas, n_images, img_dev, img_host, coords, n) || conf == nullptr) return SNERF_ERR_ARG;
  ConfArgs a{maps, M, P, H, W, slot_of_image, lambdas, n_images, sky, img_dev, img_host, coords, n, conf, nullptr, nullptr, 0, nullptr};
  hipLaunchKernelGGL(conf_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return snerf_check_launch();
}

// ---------------------------------------------------------------------------
// Gradient of the table column.  M sums over the rays that took part in the forward (not sky, inside the image),
//   A_k = sum_r g_conf_r maps[k, slot, row_r, col_r],
// accumulated in double in an order that depends on n only: ray r belongs to thread r mod (256 blocks(n)) and is taken in ascending
// order, the 64 lanes of a wave fold with shuffles, the 4 waves of a workgroup through LDS in wave order, the workgroups' partials
// (ws[8 b + k]) in block order by the second launch.  No floating-point atomics: the same bits every run.  The second launch (one lane)
// chains them to the column in double, with s_k = sigmoid(lambdas[k, i]) and S = sum_k s_k:
//   d conf_r / d lambda_k = s_k (1 - s_k) (map_k - conf_r) / S    =>    d loss / d lambda_k = s_k (1 - s_k) / S (A_k - sum_j s_j A_j / S),
// rounds once to fp32 and ADDS into column i of grad_lambdas.
// ---------------------------------------------------------------------------
#define CONF_MAX_BLOCKS 256
static inline int conf_grad_blocks(long n) {
  const long b = (n + 255) / 256;
  return b < 1 ? 1 : (b > CONF_MAX_BLOCKS ? CONF_MAX_BLOCKS : (int)b);
}

extern "C" long snerf_conf_grad_ws(long n) { return n <= 0 ? 0 : (long)CONF_MAX_MODES * conf_grad_blocks(n); }

__global__ __launch_bounds__(256) void conf_grad_partial_kernel(ConfArgs a) {
  __shared__ double red[4][CONF_MAX_MODES];
  long img; int slot = 0;
  if (!conf_image(a, &img, &slot)) return;                           // (uniform over the grid)
  const long HW = (long)a.H * a.W;
  double acc[CONF_MAX_MODES];
#pragma unroll
  for (int k = 0; k < CONF_MAX_MODES; ++k) acc[k] = 0.0;
  for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < a.n; r += (long)gridDim.x * 256) {
    const long px = conf_pixel(a, img, r);
    if (px < 0) continue;
    const double g = (double)a.g_conf[r];
    const float* m = a.maps + (long)slot * HW + px;
#pragma unroll
    for (int k = 0; k < CONF_MAX_MODES; ++k)
      if (k < a.M) acc[k] += g * (double)m[(long)k * a.P * HW];
  }
#pragma unroll
  for (int k = 0; k < CONF_MAX_MODES; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < CONF_MAX_MODES; ++k) red[threadIdx.x >> 6][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < CONF_MAX_MODES)
    a.ws[CONF_MAX_MODES * (long)blockIdx.x + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

__global__ __launch_bounds__(64) void conf_grad_finish_kernel(ConfArgs a) {
  __shared__ double s_A[CONF_MAX_MODES];
  long img; int slot = 0;
  if (!conf_image(a, &img, &slot)) return;
  if (threadIdx.x < CONF_MAX_MODES) {
    double acc = 0.0;
    for (int b = 0; b < a.blocks; ++b) acc += a.ws[CONF_MAX_MODES * (long)b + threadIdx.x];
    s_A[threadIdx.x] = acc;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double s[CONF_MAX_MODES], S = 0.0, sA = 0.0;
  for (int k = 0; k < a.M; ++k) {
    s[k] = conf_sigmoid(a.lambdas[(long)k * a.n_images + img]);
    S += s[k];
    sA += s[k] * s_A[k];
  }
  for (int k = 0; k < a.M; ++k) a.grad_lambdas[(long)k * a.n_images + img] += (float)(s[k] * (1.0 - s[k]) / S * (s_A[k] - sA / S));
}

extern "C" int snerf_conf_grad(const float* maps, int M, int P, int H, int W, const int* slot_of_image, const float* lambdas, int n_images,
                               const unsigned char* sky, const long* img_dev, int img_host, const long* coords, const float* g_conf, long n,
                               double* ws, long ws_doubles, float* grad_lambdas, void* stream) {
  if (n == 0) return SNERF_OK;
  if (conf_bad_common(maps, M, P, H, W, slot_of_image, lambdas, n_images, img_dev, img_host, coords, n)) return SNERF_ERR_ARG;
  if (g_conf == nullptr || grad_lambdas == nullptr) return SNERF_ERR_ARG;
  const int blocks = conf_grad_blocks(n);
  if (ws == nullptr || ws_doubles < (long)CONF_MAX_MODES * blocks) return SNERF_ERR_ARG;
  ConfArgs a{maps, M, P, H, W, slot_of_image, lambdas, n_images, sky, img_dev, img_host, coords, n, nullptr, g_conf, ws, blocks, grad_lambdas};
  hipLaunchKernelGGL(conf_grad_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(conf_grad_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
  return snerf_check_launch();
}
