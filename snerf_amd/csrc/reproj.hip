// Reprojection confidence maps on the device: the rgb, ssim and depth modes of Confidence.precompute_conf_map
// (s-nerf/model/confidence.py:78-112) = get_reproj_conf (model/loss.py:271-327) over reproj_err (:218-268), warping (:138-179),
// sample_points (:122-135) and ssim (utils/pytorch_msssim/__init__.py:19-60), one pass per (base image, neighbour):
//
//   warp        one thread per base pixel (x = col, y = row): d = [(x - cx) / f, -(y - cy) / f, -1] depth, c = inverse(tgt_pose) base_pose [d; 1],
//               dep = |c.z|, u = c.x / dep f_t + cx_t, v = -(c.y / dep f_t) + cy_t; in view iff 0 <= rint(v) < H and 0 <= rint(u) < W
//               (compared on the rounded floats: a non-finite u or v is out of view, a point behind the camera is not rejected, a pixel
//               of depth 0 is projected like any other).  fake = grid_sample(neighbour image) at gx = u / ((W-1)//2) - 1,
//               gy = v / ((H-1)//2) - 1 (align_corners = False, zero padding: the sample point is ((gx + 1) W - 1) / 2, not u),
//               tgt_depth = neighbour depth at (rint(v), rint(u)); rgb error = mean_c |base - fake|, depth error = |dep - tgt_depth| /
//               max(tgt_depth, 1e-10), flagged where > tau and then clamped to tau.
//   ssim        1 - mean_c SSIM(base_, fake) of the two FULL masked images (both zero out of view): 11 x 11 Gaussian window of sigma 1.5,
//               zero padding of 5, C1 = 0.01^2, C2 = 0.03^2 (L = 1: images in [0, 1]), tiled through LDS and applied separably.
//   finish      folds the workgroups' min / max partials of each error over the in-view pixels (max and min are order independent; no
//               floating-point atomics: the same bits every run) and the "any pixel in view" flag, all in device memory.
//   accumulate  sum_mode += (emax - err) / (emax - emin), count += 1 on the in-view pixels: the reference's conf = err.max() - err;
//               conf / conf.max() as the same two fp32 subtractions and one division.  A pass with no pixel in view adds nothing and does
//               not become "the last pass" (the reference raises on the empty max); emax == emin gives 0 / 0 = NaN, as the reference's.
//   finalize    sum / max(count, 1); with the depth mode, EVERY mode's map is 0 on the pixels that were in view and over tau in the LAST
//               non-empty pass only (loss.py:323-326 uses the loop's last Mask and depth_mask: a quirk that is part of the contract).
//
// The inverse of the neighbour's pose is the general affine inverse (not R^T), formed once per workgroup in double from the fp32 entries
// and rounded to fp32; everything per pixel is fp32 as separate ops (this unit is built with -ffp-contract=off).  Nothing is read back
// and nothing depends on host state between the launches: the whole call can be captured in a graph.  Inputs are expected finite.
#include "common.h"
#include <math.h>

#define RP_RGB 1
#define RP_SSIM 2
#define RP_DEPTH 4
#define RP_WARP_PART 5          // per warp workgroup: rgb min, rgb max, depth min, depth max, any-in-view
#define RP_TILE 32              // SSIM outputs per workgroup: 32 x 32
#define RP_HALO 5
#define RP_IN (RP_TILE + 2 * RP_HALO)

struct ReprojArgs {
  const void* images; const float* depths; const float* poses; const float* intrinsics;
  int H, W, base, tgt, modes;
  float tau;
  float g[11];                                     // the normalised fp32 1-D window
  float* fake;                                     // [H,W,3]
  float* err[3];                                   // [H,W] each: rgb, ssim, depth (clamped)
  float* count;                                    // [H,W]
  unsigned char *mask, *dmask, *last_mask, *last_dmask;
  float* part_warp; float* part_ssim;              // [warp workgroups][5], [tiles][2]
  int n_warp, n_tiles;
  float* stats;                                    // emax, emin of rgb, ssim, depth; [6] = 1 when any pixel of the pass is in view
  float* out[3];
};

struct ReprojLayout { long fake, err, count, bytes4, part_warp, part_ssim, stats, total; int n_warp, n_tiles; };
static inline long rp_align(long b) { return (b + 255) / 256 * 256; }
static inline ReprojLayout rp_layout(int H, int W) {
  ReprojLayout l;
  const long HW = (long)H * W;
  l.n_warp = (int)((HW + 255) / 256);
  l.n_tiles = ((W + RP_TILE - 1) / RP_TILE) * ((H + RP_TILE - 1) / RP_TILE);
  long o = 0;
  l.fake = o;      o += rp_align(HW * 3 * 4);
  l.err = o;       o += 3 * rp_align(HW * 4);
  l.count = o;     o += rp_align(HW * 4);
  l.bytes4 = o;    o += 4 * rp_align(HW);
  l.part_warp = o; o += rp_align((long)l.n_warp * RP_WARP_PART * 4);
  l.part_ssim = o; o += rp_align((long)l.n_tiles * 2 * 4);
  l.stats = o;     o += 256;
  l.total = o;
  return l;
}

extern "C" long snerf_reproj_conf_ws(int H, int W) { return H < 1 || W < 1 ? 0 : rp_layout(H, W).total; }

template <bool U8> __device__ __forceinline__ float rp_pixel(const void* images, long i) {
  if (U8) return (float)((double)((const unsigned char*)images)[i] / 255.0);
  return ((const float*)images)[i];
}

// min / max of the workgroup's 256 values; valid in thread 0
__device__ __forceinline__ void rp_block_minmax(float& lo, float& hi, float* red /*[8]*/) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o, 64));
    hi = fmaxf(hi, __shfl_xor(hi, o, 64));
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = lo; red[4 + (threadIdx.x >> 6)] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    lo = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
    hi = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
  }
}

__global__ __launch_bounds__(256) void reproj_init_kernel(ReprojArgs a) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long)a.H * a.W) return;
#pragma unroll
  for (int m = 0; m < 3; ++m)
    if (a.modes >> m & 1) a.out[m][p] = 0.f;
  a.count[p] = 0.f;
  a.last_mask[p] = 0; a.last_dmask[p] = 0;
}

template <bool U8> __global__ __launch_bounds__(256) void reproj_warp_kernel(ReprojArgs a) {
  __shared__ float s_cam[24];                      // base pose [12], inverse of the neighbour's pose [12]
  __shared__ float s_red[8];
  if (threadIdx.x == 0) {
    const float* B = a.poses + 12l * a.base;
    const float* T = a.poses + 12l * a.tgt;
    for (int i = 0; i < 12; ++i) s_cam[i] = B[i];
    // inverse of [R t; 0 0 0 1] = [R^-1, -R^-1 t] with R^-1 = adj(R) / det(R), in double
    const double r00 = T[0], r01 = T[1], r02 = T[2], t0 = T[3], r10 = T[4], r11 = T[5], r12 = T[6], t1 = T[7], r20 = T[8], r21 = T[9],
                 r22 = T[10], t2 = T[11];
    const double c00 = r11 * r22 - r12 * r21, c01 = r02 * r21 - r01 * r22, c02 = r01 * r12 - r02 * r11;
    const double c10 = r12 * r20 - r10 * r22, c11 = r00 * r22 - r02 * r20, c12 = r02 * r10 - r00 * r12;
    const double c20 = r10 * r21 - r11 * r20, c21 = r01 * r20 - r00 * r21, c22 = r00 * r11 - r01 * r10;
    const double det = r00 * c00 + r01 * c10 + r02 * c20;
    const double i00 = c00 / det, i01 = c01 / det, i02 = c02 / det, i10 = c10 / det, i11 = c11 / det, i12 = c12 / det, i20 = c20 / det,
                 i21 = c21 / det, i22 = c22 / det;
    float* I = s_cam + 12;
    I[0] = (float)i00; I[1] = (float)i01; I[2] = (float)i02;  I[3] = (float)-(i00 * t0 + i01 * t1 + i02 * t2);
    I[4] = (float)i10; I[5] = (float)i11; I[6] = (float)i12;  I[7] = (float)-(i10 * t0 + i11 * t1 + i12 * t2);
    I[8] = (float)i20; I[9] = (float)i21; I[10] = (float)i22; I[11] = (float)-(i20 * t0 + i21 * t1 + i22 * t2);
  }
  __syncthreads();
  const int H = a.H, W = a.W;
  const long HW = (long)H * W, p = (long)blockIdx.x * 256 + threadIdx.x;
  float lo_rgb = INFINITY, hi_rgb = -INFINITY, lo_d = INFINITY, hi_d = -INFINITY, none = 0.f, any = 0.f;
  if (p < HW) {
    const float* kb = a.intrinsics + 4l * a.base;   // cx, cy, fx, fy
    const float* kt = a.intrinsics + 4l * a.tgt;
    const float focal = (kb[2] + kb[3]) / 2.f, tgt_focal = (kt[2] + kt[3]) / 2.f;
    const int y = (int)(p / W), x = (int)(p - (long)y * W);
    const float depth = a.depths[(long)a.base * HW + p];
    const float dx = ((float)x - kb[0]) / focal * depth, dy = -(((float)y - kb[1]) / focal) * depth, dz = -depth;
    const float* B = s_cam;
    const float* I = s_cam + 12;
    const float px = ((B[0] * dx + B[1] * dy) + B[2] * dz) + B[3];
    const float py = ((B[4] * dx + B[5] * dy) + B[6] * dz) + B[7];
    const float pz = ((B[8] * dx + B[9] * dy) + B[10] * dz) + B[11];
    const float cx = ((I[0] * px + I[1] * py) + I[2] * pz) + I[3];
    const float cy = ((I[4] * px + I[5] * py) + I[6] * pz) + I[7];
    const float cz = ((I[8] * px + I[9] * py) + I[10] * pz) + I[11];
    const float dep = fabsf(cz);
    const float u = cx / dep * tgt_focal + kt[0];
    const float v = -(cy / dep * tgt_focal) + kt[1];
    const float r = rintf(v), q = rintf(u);
    const bool in_view = r >= 0.f && r < (float)H && q >= 0.f && q < (float)W;
    float f[3] = {0.f, 0.f, 0.f}, e_rgb = 0.f, e_d = 0.f;
    bool over = false;
    if (in_view) {
      // grid_sample(align_corners = False, padding_mode = 'zeros'), bilinear
      const float gx = u / (float)((W - 1) / 2) - 1.f, gy = v / (float)((H - 1) / 2) - 1.f;
      const float ix = ((gx + 1.f) * (float)W - 1.f) / 2.f, iy = ((gy + 1.f) * (float)H - 1.f) / 2.f;
      if (ix > -1.f && ix < (float)W && iy > -1.f && iy < (float)H) {      // (else all four taps fall in the padding, or ix / iy is not finite)
        const float x0f = floorf(ix), y0f = floorf(iy);
        const int x0 = (int)x0f, y0 = (int)y0f;
        const float wx1 = ix - x0f, wx0 = (x0f + 1.f) - ix, wy1 = iy - y0f, wy0 = (y0f + 1.f) - iy;
        const float w_nw = wx0 * wy0, w_ne = wx1 * wy0, w_sw = wx0 * wy1, w_se = wx1 * wy1;
        const bool xl = x0 >= 0, xr = x0 + 1 < W, yt = y0 >= 0, yb = y0 + 1 < H;
        const long o = ((long)a.tgt * HW + (long)y0 * W + x0) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          float s = 0.f;
          if (xl && yt) s = s + rp_pixel<U8>(a.images, o + c) * w_nw;
          if (xr && yt) s = s + rp_pixel<U8>(a.images, o + 3 + c) * w_ne;
          if (xl && yb) s = s + rp_pixel<U8>(a.images, o + 3l * W + c) * w_sw;
          if (xr && yb) s = s + rp_pixel<U8>(a.images, o + 3l * W + 3 + c) * w_se;
          f[c] = s;
        }
      }
      const long ob = ((long)a.base * HW + p) * 3;
      e_rgb = ((fabsf(rp_pixel<U8>(a.images, ob) - f[0]) + fabsf(rp_pixel<U8>(a.images, ob + 1) - f[1])) +
               fabsf(rp_pixel<U8>(a.images, ob + 2) - f[2])) / 3.f;
      const float td = a.depths[(long)a.tgt * HW + (long)r * W + (long)q];
      e_d = fabsf(dep - td) / fmaxf(td, 1e-10f);
      over = e_d > a.tau;
      e_d = fminf(e_d, a.tau);
      lo_rgb = hi_rgb = e_rgb;
      lo_d = hi_d = e_d;
      any = 1.f;
    }
    a.fake[3 * p] = f[0]; a.fake[3 * p + 1] = f[1]; a.fake[3 * p + 2] = f[2];
    a.mask[p] = in_view; a.dmask[p] = over;
    a.err[0][p] = e_rgb; a.err[2][p] = e_d;
  }
  rp_block_minmax(lo_rgb, hi_rgb, s_red);
  rp_block_minmax(lo_d, hi_d, s_red);
  rp_block_minmax(none, any, s_red);
  if (threadIdx.x == 0) {
    float* o = a.part_warp + (long)blockIdx.x * RP_WARP_PART;
    o[0] = lo_rgb; o[1] = hi_rgb; o[2] = lo_d; o[3] = hi_d; o[4] = any;
  }
}

// One workgroup per 32 x 32 tile of outputs, one channel at a time: the tile and its halo of 5 of base_ (the image under the mask byte:
// never materialised) and fake_img go to LDS (2 x 42 x 42 floats), a horizontal 11-tap pass writes x, y, x^2, y^2, xy for the 42 rows
// (5 x 42 x 32 floats), a vertical pass finishes the five window sums of 4 outputs per thread: 41 KB of LDS, inside the default limit.
// In both passes the 32 lanes of a bank group (ds_read_b32 / ds_write_b32 bank over 32 dwords per 32-lane half) address 32 consecutive
// dwords of one row, so neither pass has a bank conflict at any row stride and the rows need no padding.
template <bool U8> __global__ __launch_bounds__(256) void reproj_ssim_kernel(ReprojArgs a) {
  __shared__ float s_x[RP_IN * RP_IN], s_y[RP_IN * RP_IN], s_h[5][RP_IN * RP_TILE];
  __shared__ float s_red[8];
  const int H = a.H, W = a.W, tid = threadIdx.x;
  const long HW = (long)H * W;
  const int x0 = blockIdx.x * RP_TILE, y0 = blockIdx.y * RP_TILE;
  const float C1 = (float)(0.01 * 0.01), C2 = (float)(0.03 * 0.03);
  const int col = tid & 31, row0 = tid >> 5;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < 3; ++c) {
    __syncthreads();                                                          // the previous channel's passes are done with s_x, s_y, s_h
    for (int i = tid; i < RP_IN * RP_IN; i += 256) {
      const int ly = i / RP_IN, lx = i - ly * RP_IN, gy = y0 + ly - RP_HALO, gx = x0 + lx - RP_HALO;
      float xv = 0.f, yv = 0.f;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        const long p = (long)gy * W + gx;
        if (a.mask[p]) xv = rp_pixel<U8>(a.images, ((long)a.base * HW + p) * 3 + c);
        yv = a.fake[3 * p + c];
      }
      s_x[i] = xv; s_y[i] = yv;
    }
    __syncthreads();
    for (int i = tid; i < RP_IN * RP_TILE; i += 256) {
      const int ry = i >> 5, rx = i & 31;
      const float* px = s_x + ry * RP_IN + rx;
      const float* py = s_y + ry * RP_IN + rx;
      float sx = 0.f, sy = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
#pragma unroll
      for (int t = 0; t < 11; ++t) {
        const float xv = px[t], yv = py[t], w = a.g[t];
        sx = sx + w * xv; sy = sy + w * yv; sxx = sxx + w * (xv * xv); syy = syy + w * (yv * yv); sxy = sxy + w * (xv * yv);
      }
      s_h[0][i] = sx; s_h[1][i] = sy; s_h[2][i] = sxx; s_h[3][i] = syy; s_h[4][i] = sxy;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int o = (row0 + 8 * k) * RP_TILE + col;
      float mu1 = 0.f, mu2 = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
#pragma unroll
      for (int t = 0; t < 11; ++t) {
        const float w = a.g[t];
        mu1 = mu1 + w * s_h[0][o + t * RP_TILE]; mu2 = mu2 + w * s_h[1][o + t * RP_TILE]; xx = xx + w * s_h[2][o + t * RP_TILE];
        yy = yy + w * s_h[3][o + t * RP_TILE];   xy = xy + w * s_h[4][o + t * RP_TILE];
      }
      const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
      const float sigma1_sq = xx - mu1_sq, sigma2_sq = yy - mu2_sq, sigma12 = xy - mu1_mu2;
      const float v1 = 2.f * sigma12 + C2, v2 = (sigma1_sq + sigma2_sq) + C2;
      const float s = ((2.f * mu1_mu2 + C1) * v1) / (((mu1_sq + mu2_sq) + C1) * v2);
      acc[k] = c == 0 ? s : acc[k] + s;
    }
  }
  float lo = INFINITY, hi = -INFINITY;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int gy = y0 + row0 + 8 * k, gx = x0 + col;
    if (gy < H && gx < W) {
      const long p = (long)gy * W + gx;
      const bool in_view = a.mask[p] != 0;
      const float e = in_view ? 1.f - acc[k] / 3.f : 0.f;
      a.err[1][p] = e;
      if (in_view) { lo = fminf(lo, e); hi = fmaxf(hi, e); }
    }
  }
  rp_block_minmax(lo, hi, s_red);
  if (tid == 0) {
    float* o = a.part_ssim + 2l * (blockIdx.y * gridDim.x + blockIdx.x);
    o[0] = lo; o[1] = hi;
  }
}

// one workgroup: the partials of the pass -> stats
__global__ __launch_bounds__(256) void reproj_finish_kernel(ReprojArgs a) {
  __shared__ float s_red[8];
  float lo_rgb = INFINITY, hi_rgb = -INFINITY, lo_d = INFINITY, hi_d = -INFINITY, lo_s = INFINITY, hi_s = -INFINITY, any = 0.f, none = 0.f;
  for (int b = threadIdx.x; b < a.n_warp; b += 256) {
    const float* q = a.part_warp + (long)b * RP_WARP_PART;
    lo_rgb = fminf(lo_rgb, q[0]); hi_rgb = fmaxf(hi_rgb, q[1]); lo_d = fminf(lo_d, q[2]); hi_d = fmaxf(hi_d, q[3]); any = fmaxf(any, q[4]);
  }
  if (a.modes & RP_SSIM)
    for (int b = threadIdx.x; b < a.n_tiles; b += 256) { lo_s = fminf(lo_s, a.part_ssim[2l * b]); hi_s = fmaxf(hi_s, a.part_ssim[2l * b + 1]); }
  rp_block_minmax(lo_rgb, hi_rgb, s_red);
  rp_block_minmax(lo_s, hi_s, s_red);
  rp_block_minmax(lo_d, hi_d, s_red);
  rp_block_minmax(none, any, s_red);
  if (threadIdx.x == 0) {
    a.stats[0] = hi_rgb; a.stats[1] = lo_rgb; a.stats[2] = hi_s; a.stats[3] = lo_s; a.stats[4] = hi_d; a.stats[5] = lo_d; a.stats[6] = any;
  }
}

__global__ __launch_bounds__(256) void reproj_accumulate_kernel(ReprojArgs a) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long)a.H * a.W || a.stats[6] == 0.f) return;            // a pass with nothing in view: no sum, no count, not "the last pass"
  const unsigned char m = a.mask[p];
  a.last_mask[p] = m; a.last_dmask[p] = a.dmask[p];
  if (!m) return;
  a.count[p] = a.count[p] + 1.f;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (a.modes >> k & 1) {
      const float emax = a.stats[2 * k], emin = a.stats[2 * k + 1];
      a.out[k][p] = a.out[k][p] + (emax - a.err[k][p]) / (emax - emin);
    }
}

__global__ __launch_bounds__(256) void reproj_finalize_kernel(ReprojArgs a) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long)a.H * a.W) return;
  const float n = fmaxf(a.count[p], 1.f);
  const bool zero = (a.modes & RP_DEPTH) && a.last_mask[p] && a.last_dmask[p];
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (a.modes >> k & 1) a.out[k][p] = zero ? 0.f : a.out[k][p] / n;
}

extern "C" int snerf_reproj_conf(const void* images, int images_u8, const float* depths, const float* poses, const float* intrinsics, int N,
                                 int H, int W, int base, const int* neighbours, int n_neighbours, int modes, float tau, void* ws,
                                 long ws_bytes, float* out_rgb, float* out_ssim, float* out_depth, void* stream) {
  if (images == nullptr || depths == nullptr || poses == nullptr || intrinsics == nullptr || N < 1 || H < 1 || W < 1) return SNERF_ERR_ARG;
  if (base < 0 || base >= N || n_neighbours < 0 || (n_neighbours > 0 && neighbours == nullptr)) return SNERF_ERR_ARG;
  for (int i = 0; i < n_neighbours; ++i)
    if (neighbours[i] < 0 || neighbours[i] >= N) return SNERF_ERR_ARG;
  if (modes < 1 || modes > 7 || !isfinite(tau)) return SNERF_ERR_ARG;
  float* out[3] = {out_rgb, out_ssim, out_depth};
  for (int k = 0; k < 3; ++k)
    if ((modes >> k & 1) && out[k] == nullptr) return SNERF_ERR_ARG;
  const ReprojLayout l = rp_layout(H, W);
  if (ws == nullptr || ws_bytes < l.total) return SNERF_ERR_ARG;

  ReprojArgs a;
  a.images = images; a.depths = depths; a.poses = poses; a.intrinsics = intrinsics;
  a.H = H; a.W = W; a.base = base; a.tgt = base; a.modes = modes; a.tau = tau;
  {  // pytorch_msssim's gaussian(11, 1.5): fp32 entries of the double exponentials, divided by their fp32 sum
    float s = 0.f;
    for (int t = 0; t < 11; ++t) { a.g[t] = (float)exp(-(double)((t - 5) * (t - 5)) / (2.0 * 1.5 * 1.5)); s += a.g[t]; }
    for (int t = 0; t < 11; ++t) a.g[t] /= s;
  }
  char* w = (char*)ws;
  const long HW = (long)H * W;
  a.fake = (float*)(w + l.fake);
  for (int k = 0; k < 3; ++k) { a.err[k] = (float*)(w + l.err + k * rp_align(HW * 4)); a.out[k] = out[k]; }
  a.count = (float*)(w + l.count);
  unsigned char* b4 = (unsigned char*)(w + l.bytes4);
  a.mask = b4; a.dmask = b4 + rp_align(HW); a.last_mask = b4 + 2 * rp_align(HW); a.last_dmask = b4 + 3 * rp_align(HW);
  a.part_warp = (float*)(w + l.part_warp); a.part_ssim = (float*)(w + l.part_ssim); a.stats = (float*)(w + l.stats);
  a.n_warp = l.n_warp; a.n_tiles = l.n_tiles;

  hipStream_t st = (hipStream_t)stream;
  const dim3 px((unsigned)l.n_warp), wg(256), tiles((unsigned)((W + RP_TILE - 1) / RP_TILE), (unsigned)((H + RP_TILE - 1) / RP_TILE));
  hipLaunchKernelGGL(reproj_init_kernel, px, wg, 0, st, a);
  for (int i = 0; i < n_neighbours; ++i) {
    a.tgt = neighbours[i];
    if (images_u8) hipLaunchKernelGGL(reproj_warp_kernel<true>, px, wg, 0, st, a);
    else           hipLaunchKernelGGL(reproj_warp_kernel<false>, px, wg, 0, st, a);
    if (modes & RP_SSIM) {
      if (images_u8) hipLaunchKernelGGL(reproj_ssim_kernel<true>, tiles, wg, 0, st, a);
      else           hipLaunchKernelGGL(reproj_ssim_kernel<false>, tiles, wg, 0, st, a);
    }
    hipLaunchKernelGGL(reproj_finish_kernel, dim3(1), wg, 0, st, a);
    hipLaunchKernelGGL(reproj_accumulate_kernel, px, wg, 0, st, a);
  }
  hipLaunchKernelGGL(reproj_finalize_kernel, px, wg, 0, st, a);
  return snerf_check_launch();
}
