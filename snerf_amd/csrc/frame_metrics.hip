// Frame metrics on the device: the two numbers of image.MetricHarness (s-nerfpp/zipnerf/internal/image.py:110-125: skimage's PSNR of the
// uint8 RGB images and its SSIM of their 8-bit grey images) and eval.py's float PSNR (s-nerf/eval.py:152), F frames per call:
//
//   quantise    q(x) = trunc(x * 255.f): one fp32 product, truncated toward zero; a product below 0 gives 0, above 255 gives 255, NaN
//               gives 0 (numpy's cast is undefined outside (-1, 256): a stated deviation).  A uint8 ground truth is used as it is.
//   float       d = pred - g and d * d as separate fp32 ops (this unit is built with -ffp-contract=off), g = gt or, for a uint8 ground
//               truth, float32(k / 255.0) (the batchers' decode); the squares are summed in double.  mse_f = sum / (3 H W),
//               psnr_f = -10 / ln 10 * ln(mse_f).
//   uint8       the squared differences of the quantised samples summed as an integer (exact); mse_u8 = sse / (3 H W),
//               psnr_u8 = 10 log10(255^2 / mse_u8): +inf for equal images.
//   grey        (r wr + g wg + b wb + (1 << (shift - 1))) >> shift on the quantised channels (FM_GRAY_CV4: OpenCV 4's 8-bit RGB2GRAY).
//   ssim        structural_similarity(grey_pred, grey_gt, data_range = 255) with skimage's defaults: 7 x 7 uniform window, K1 = 0.01,
//               K2 = 0.03, sample covariance, a border of 3 cropped.  The five window sums are exact in int32 (49 * 255^2 at most), the
//               rest is double: ux = Sx / 49, vx = 49/48 (Sxx / 49 - ux^2), vxy = 49/48 (Sxy / 49 - ux uy), S = (2 ux uy + C1)
//               (2 vxy + C2) / ((ux^2 + uy^2 + C1) (vx + vy + C2)); ssim = the mean of S over the (H - 6) (W - 6) cropped pixels.
//
// Two launches: one workgroup per 32 x 32 tile of cropped outputs and frame writes its three partial sums to the workspace, then one
// workgroup per frame folds them in tile order.  Every sum runs in an order that depends on the shape only and there are no
// floating-point atomics: the same bits every run.  Nothing is read back; the call can be captured in a graph.
#include "common.h"
#include <math.h>

#define FM_TILE 32              // cropped SSIM outputs per workgroup: 32 x 32
#define FM_WIN 7
#define FM_IN (FM_TILE + FM_WIN - 1)
#define FM_MAX_FRAMES 65535     // the frame rides on grid.z

// the grey weights {wr, wg, wb, shift} of the call when gray_w is NULL: OpenCV 4's 8-bit RGB2GRAY ({4899, 9617, 1868, 14} is OpenCV 3's)
static const int FM_GRAY_CV4[4] = {9798, 19235, 3735, 15};

struct FrameMetricArgs {
  const float* pred; const void* gt;
  int H, W, n_tiles;
  int wr, wg, wb, shift;
  double* part_d;                                  // [F][n_tiles][2]: sum of S, sum of the fp32 squares
  long long* part_i;                               // [F][n_tiles]: sum of the squared uint8 differences
  double* out;                                     // [F][5]
};

static inline long fm_tiles(int H, int W) { return (long)((W - 6 + FM_TILE - 1) / FM_TILE) * ((H - 6 + FM_TILE - 1) / FM_TILE); }
static inline bool fm_shape_ok(int F, int H, int W) { return F >= 1 && F <= FM_MAX_FRAMES && H >= FM_WIN && W >= FM_WIN; }

extern "C" long snerf_frame_metrics_ws(int F, int H, int W) {
  if (!fm_shape_ok(F, H, W)) return 0;
  return ((long)F * fm_tiles(H, W) * 24 + 255) / 256 * 256;
}

__device__ __forceinline__ int fm_quant(float x) {
  const float p = x * 255.f;
  return p >= 255.f ? 255 : (p > 0.f ? (int)p : 0);                           // NaN fails both comparisons: 0
}

// sums of the workgroup's 256 values in a fixed order (xor tree in the wave, then waves 0..3); valid in thread 0
__device__ __forceinline__ void fm_block_sum(double& a, double& b, long long& c, double* red /*[8]*/, long long* redi /*[4]*/) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a = a + __shfl_xor(a, o, 64);
    b = b + __shfl_xor(b, o, 64);
    c = c + __shfl_xor(c, o, 64);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = a; red[4 + (threadIdx.x >> 6)] = b; redi[threadIdx.x >> 6] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = ((red[0] + red[1]) + red[2]) + red[3];
    b = ((red[4] + red[5]) + red[6]) + red[7];
    c = redi[0] + redi[1] + redi[2] + redi[3];
  }
}

// One workgroup per 32 x 32 tile of cropped outputs (grid.x, grid.y) and frame (grid.z).  Output (oy, ox) of the cropped image is
// centred on pixel (oy + 3, ox + 3) and its window covers the pixels [oy, oy + 7) x [ox, ox + 7), so the tile at (y0, x0) = 32 (by, bx)
// reads the 38 x 38 pixels from (y0, x0) on: they are quantised and grey-converted on the load (no uint8 or grey image is ever
// materialised) into 2 x 38 x 38 ints of LDS, a horizontal 7-tap pass writes the sums of x, y, x^2, y^2, xy for the 38 rows
// (5 x 38 x 32 ints), a vertical pass finishes the five window sums of 4 outputs per thread: 36 KB of LDS, inside the default limit.
// As in reproj_ssim_kernel, the 32 lanes of a bank group address 32 consecutive dwords of one row in both passes: no bank conflict at
// any row stride, no padding.
// The PSNR sums ride in the same load over the pixels the tile OWNS, so that every pixel of the frame is counted exactly once: the
// first 32 x 32 of its 38 x 38 pixels, and in the last tile column (row) also the columns (rows) from x0 + 32 (y0 + 32) up to W (H).
// Those are at most 6, W <= x0 + 38 there, so they lie inside the loaded region: the image's right and bottom border of 3 and
// whatever the ragged last tile leaves belong to the last column / row of tiles, the top and left border to the tiles that start there.
template <bool U8> __global__ __launch_bounds__(256) void frame_metrics_tile_kernel(FrameMetricArgs a) {
  __shared__ int s_x[FM_IN * FM_IN], s_y[FM_IN * FM_IN], s_h[5][FM_IN * FM_TILE];
  __shared__ double s_red[8];
  __shared__ long long s_redi[4];
  const int H = a.H, W = a.W, tid = threadIdx.x;
  const int x0 = blockIdx.x * FM_TILE, y0 = blockIdx.y * FM_TILE;
  const int own_x1 = blockIdx.x + 1 == gridDim.x ? W : x0 + FM_TILE, own_y1 = blockIdx.y + 1 == gridDim.y ? H : y0 + FM_TILE;
  const long frame = (long)blockIdx.z * H * W;
  const int half = 1 << (a.shift - 1);
  double sq = 0.0;
  long long sse = 0;
  for (int i = tid; i < FM_IN * FM_IN; i += 256) {
    const int ly = i / FM_IN, lx = i - ly * FM_IN, gy = y0 + ly, gx = x0 + lx;
    int xv = 0, yv = 0;
    if (gy < H && gx < W) {
      const long o = (frame + (long)gy * W + gx) * 3;
      const bool own = gy < own_y1 && gx < own_x1;
      int qp[3], qg[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float p = a.pred[o + c];
        float g;
        if (U8) { qg[c] = ((const unsigned char*)a.gt)[o + c]; g = (float)((double)qg[c] / 255.0); }
        else    { g = ((const float*)a.gt)[o + c]; qg[c] = fm_quant(g); }
        qp[c] = fm_quant(p);
        if (own) {
          const float d = p - g;
          sq = sq + (double)(d * d);
          const int e = qp[c] - qg[c];
          sse += e * e;
        }
      }
      xv = (qp[0] * a.wr + qp[1] * a.wg + qp[2] * a.wb + half) >> a.shift;
      yv = (qg[0] * a.wr + qg[1] * a.wg + qg[2] * a.wb + half) >> a.shift;
    }
    s_x[i] = xv; s_y[i] = yv;
  }
  __syncthreads();
  for (int i = tid; i < FM_IN * FM_TILE; i += 256) {
    const int ry = i >> 5, rx = i & 31;
    const int* px = s_x + ry * FM_IN + rx;
    const int* py = s_y + ry * FM_IN + rx;
    int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
    for (int t = 0; t < FM_WIN; ++t) {
      const int xv = px[t], yv = py[t];
      sx += xv; sy += yv; sxx += xv * xv; syy += yv * yv; sxy += xv * yv;
    }
    s_h[0][i] = sx; s_h[1][i] = sy; s_h[2][i] = sxx; s_h[3][i] = syy; s_h[4][i] = sxy;
  }
  __syncthreads();
  const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0), NP = 49.0, COV = 49.0 / 48.0;
  const int col = tid & 31, row0 = tid >> 5;
  double ss = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int row = row0 + 8 * k, o = row * FM_TILE + col;
    int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
    for (int t = 0; t < FM_WIN; ++t) {
      sx += s_h[0][o + t * FM_TILE]; sy += s_h[1][o + t * FM_TILE]; sxx += s_h[2][o + t * FM_TILE];
      syy += s_h[3][o + t * FM_TILE]; sxy += s_h[4][o + t * FM_TILE];
    }
    if (y0 + row < H - 6 && x0 + col < W - 6) {
      const double ux = (double)sx / NP, uy = (double)sy / NP;
      const double vx = COV * ((double)sxx / NP - ux * ux), vy = COV * ((double)syy / NP - uy * uy);
      const double vxy = COV * ((double)sxy / NP - ux * uy);
      const double s = ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
      ss = ss + s;
    }
  }
  fm_block_sum(ss, sq, sse, s_red, s_redi);
  if (tid == 0) {
    const long t = (long)blockIdx.z * a.n_tiles + (long)blockIdx.y * gridDim.x + blockIdx.x;
    a.part_d[2 * t] = ss; a.part_d[2 * t + 1] = sq; a.part_i[t] = sse;
  }
}

// one workgroup per frame: the tiles' partials in tile order -> mse_f, psnr_f, mse_u8, psnr_u8, ssim
__global__ __launch_bounds__(256) void frame_metrics_finish_kernel(FrameMetricArgs a) {
  __shared__ double s_red[8];
  __shared__ long long s_redi[4];
  const long base = (long)blockIdx.x * a.n_tiles;
  double ss = 0.0, sq = 0.0;
  long long sse = 0;
  for (int t = threadIdx.x; t < a.n_tiles; t += 256) {
    ss = ss + a.part_d[2 * (base + t)]; sq = sq + a.part_d[2 * (base + t) + 1]; sse += a.part_i[base + t];
  }
  fm_block_sum(ss, sq, sse, s_red, s_redi);
  if (threadIdx.x == 0) {
    const double n = (double)(3l * a.H * a.W), mse_f = sq / n, mse_u8 = (double)sse / n;
    double* o = a.out + 5l * blockIdx.x;
    o[0] = mse_f;
    o[1] = -10.0 / log(10.0) * log(mse_f);
    o[2] = mse_u8;
    o[3] = 10.0 * log10(255.0 * 255.0 / mse_u8);
    o[4] = ss / (double)((long)(a.H - 6) * (a.W - 6));
  }
}

extern "C" int snerf_frame_metrics(const float* pred, const void* gt, int gt_u8, int F, int H, int W, const int* gray_w, void* ws,
                                   long ws_bytes, double* out, void* stream) {
  if (pred == nullptr || gt == nullptr || out == nullptr || ws == nullptr || !fm_shape_ok(F, H, W)) return SNERF_ERR_ARG;
  if (ws_bytes < snerf_frame_metrics_ws(F, H, W) || ((uintptr_t)ws & 7) != 0) return SNERF_ERR_ARG;
  const int* g = gray_w != nullptr ? gray_w : FM_GRAY_CV4;
  if (g[3] < 1 || g[3] > 20 || g[0] < 0 || g[1] < 0 || g[2] < 0) return SNERF_ERR_ARG;
  if ((long)g[0] + g[1] + g[2] > (1l << g[3])) return SNERF_ERR_ARG;          // grey must stay within 0..255: the window sums are int32
  const long n_tiles = fm_tiles(H, W);
  if (n_tiles > 0x7fffffffl) return SNERF_ERR_ARG;

  FrameMetricArgs a;
  a.pred = pred; a.gt = gt; a.H = H; a.W = W; a.n_tiles = (int)n_tiles;
  a.wr = g[0]; a.wg = g[1]; a.wb = g[2]; a.shift = g[3];
  a.part_d = (double*)ws; a.part_i = (long long*)((double*)ws + 2l * F * n_tiles); a.out = out;

  hipStream_t st = (hipStream_t)stream;
  const dim3 tiles((unsigned)((W - 6 + FM_TILE - 1) / FM_TILE), (unsigned)((H - 6 + FM_TILE - 1) / FM_TILE), (unsigned)F), wg(256);
  if (gt_u8) hipLaunchKernelGGL(frame_metrics_tile_kernel<true>, tiles, wg, 0, st, a);
  else       hipLaunchKernelGGL(frame_metrics_tile_kernel<false>, tiles, wg, 0, st, a);
  hipLaunchKernelGGL(frame_metrics_finish_kernel, dim3((unsigned)F), wg, 0, st, a);
  return snerf_check_launch();
}
