// Projected mesh shadows of S-NeRF++ stage 3 (s-nerfpp/stage3_code/mesh_shadow.py:21-113 generate_one_shadow, helpers in stage3_code/utils.py).
//   snerf_shadow_project  <- utils.py:339-354 process_mesh (given as a 3 x 4 placement), :130-154 project_to_ground, :157-168 project,
//                            :171-192 points_to_mask: all in float64, one lane per vertex, plain byte stores of 255 into a zeroed plane
//   snerf_shadow_close    <- utils.py:195-211 interpolate: cv2.morphologyEx(MORPH_CLOSE, rect (r, r), iterations) on the zero-padded mask,
//                            on bit-packed rows (64 pixels per word): dilation = OR of shifted words, erosion = AND, rows then columns
//   snerf_shadow_fuse     <- mesh_shadow.py:89-107 blur_shadow (bounding box -> box filter -> check_the_occlusion -> darken) and, with
//                            check, utils.py:248-269 shadow_fuse(im, mask, 1, blur=None)
// cv2 is not available where this was written: the closing and the box filter follow OpenCV's published definitions (PARITY UNPINNED,
// include/snerf_hip.h); the geometry, the occlusion test and the fuse arithmetic are pinned against the reference's own functions.
// No kernel synchronises, allocates or hands a value to the host: the blur's kernel size lives in device scratch.
#include "common.h"

typedef unsigned long long u64;

// ---- project and splat ---------------------------------------------------------------------------------------------------------------
struct ShadowXf {
  double A[12];      // placement, row-major 3 x 4: Rz(theta) | bbox_center + Rz mesh_bias
  double L[3];       // light vector
  double g;          // ground height (mode 0)
  double M[12];      // world -> pixel, row-major 3 x 4: P (c2w^-1)[:3]
  int mode;          // 0: the ground is g; 1: the reference's `if not ground_height`, the smallest z of the placed points; 2: no ground projection (check)
};
#define SHADOW_PARTS 1024    // blocks of the first reduction stage = doubles of its scratch

__device__ __forceinline__ void shadow_place(const ShadowXf& t, const void* v, int f64, long i, double& x, double& y, double& z) {
  double a, b, c;
  if (f64) {
    const double* p = (const double*)v + 3 * i;
    a = p[0]; b = p[1]; c = p[2];
  } else {
    const float* p = (const float*)v + 3 * i;
    a = p[0]; b = p[1]; c = p[2];
  }
  x = ((t.A[0] * a + t.A[1] * b) + t.A[2] * c) + t.A[3];
  y = ((t.A[4] * a + t.A[5] * b) + t.A[6] * c) + t.A[7];
  z = ((t.A[8] * a + t.A[9] * b) + t.A[10] * c) + t.A[11];
}

// min over the block (fmin: a NaN never wins, as it sorts last in the reference's np.sort); sh: 4 doubles of LDS
__device__ __forceinline__ double shadow_block_min(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  v = fmin(fmin(sh[0], sh[1]), fmin(sh[2], sh[3]));
  __syncthreads();
  return v;
}

__global__ __launch_bounds__(256) void shadow_zmin_kernel(ShadowXf t, const void* __restrict__ v, int f64, long N, double* __restrict__ partial) {
  __shared__ double sh[4];
  double m = INFINITY;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long)gridDim.x * 256) {
    double x, y, z;
    shadow_place(t, v, f64, i, x, y, z);
    m = fmin(m, z);
  }
  m = shadow_block_min(m, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = m;
}

__global__ __launch_bounds__(256) void shadow_splat_kernel(ShadowXf t, const void* __restrict__ v, int f64, long N, const double* __restrict__ partial,
                                                           int n_parts, unsigned char* __restrict__ plane, int H, int W) {
  __shared__ double sh[4];
  double g = t.g;
  if (t.mode == 1) {                                       // second stage: every block reduces the partial minima in the same order
    double m = INFINITY;
    for (int k = threadIdx.x; k < n_parts; k += 256) m = fmin(m, partial[k]);
    g = shadow_block_min(m, sh);
  }
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  double x, y, z;
  shadow_place(t, v, f64, i, x, y, z);
  if (t.mode != 2) {
    const double coef = (z - g) / t.L[2];
    x = x - t.L[0] * coef; y = y - t.L[1] * coef; z = z - t.L[2] * coef;
  }
  const double c0 = ((t.M[0] * x + t.M[1] * y) + t.M[2] * z) + t.M[3];
  const double c1 = ((t.M[4] * x + t.M[5] * y) + t.M[6] * z) + t.M[7];
  const double c2 = ((t.M[8] * x + t.M[9] * y) + t.M[10] * z) + t.M[11];
  const double qx = c0 / c2, qy = c1 / c2;                  // no test of c2's sign, as in the reference
  // not finite, negative or >= 65536: dropped (the reference's float -> uint16 cast wraps those; documented divergence)
  if (!(qx >= 0. && qx < 65536. && qy >= 0. && qy < 65536.)) return;
  const int xi = (int)qx, yi = (int)qy;
  if (xi > 0 && xi < W && yi > 0 && yi < H) plane[(long)yi * W + xi] = 255;      // strict: column 0 and row 0 are never set
}

// single-channel plane -> [H,W,3]
__global__ __launch_bounds__(256) void shadow_plane_expand_kernel(const unsigned char* __restrict__ plane, long P, unsigned char* __restrict__ out) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const unsigned char v = plane[p] ? 255 : 0;
  out[3 * p] = v; out[3 * p + 1] = v; out[3 * p + 2] = v;
}

// ---- bit-packed closing --------------------------------------------------------------------------------------------------------------
// Domain: the image extended by (Ex, Ey) = min(iterations * (r / 2), pad) on every side, Hd x Wd pixels, nwd words per row, bit b of
// word j = pixel 64 j + b; bits past Wd in the last word are kept 0 in memory.  Outside the domain a pixel never wins: 0 for the
// dilation, 1 for the erosion.  Where the extension is the reach and not the pad, what lies outside cannot influence the cropped image.

// one wave per domain word: src = bytes with `stride` (1: plane, 3: channel 0 of an [H,W,3] mask), > 0 = set
__global__ __launch_bounds__(256) void shadow_pack_kernel(const unsigned char* __restrict__ src, int stride, int H, int W, int Ex, int Ey, long n_words,
                                                          int nwd, u64* __restrict__ dst) {
  const long wid = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wid >= n_words) return;                                       // wave-uniform
  const long y = wid / nwd - Ey, x = (wid % nwd) * 64 + (threadIdx.x & 63) - Ex;
  const int set = y >= 0 && y < H && x >= 0 && x < W && src[(y * W + x) * stride] > 0;
  const u64 bits = __ballot(set);
  if ((threadIdx.x & 63) == 0) dst[wid] = bits;
}

__device__ __forceinline__ u64 shadow_word(const u64* __restrict__ src, long y, long j, int Hd, int nwd, u64 tailmask, int erode) {
  if (y < 0 || y >= Hd || j < 0 || j >= nwd) return erode ? ~0ull : 0ull;
  u64 w = src[y * nwd + j];
  if (erode && j == nwd - 1) w |= tailmask;
  return w;
}

// One dilation or erosion by the window [-a, b] x [-a, b] (a = r / 2, b = r - 1 - a, both clamped to the domain): the tile and its halo
// are staged in LDS, the row pass runs LDS -> LDS, the column pass LDS -> global.
#define SH_TH 32
#define SH_TW 4
__global__ __launch_bounds__(256) void shadow_close_tile_kernel(const u64* __restrict__ src, u64* __restrict__ dst, int Hd, int nwd, u64 tailmask, int a,
                                                                int b, int erode, int tiles_x) {
  extern __shared__ u64 shadow_lds[];
  const int hwl = (a + 63) >> 6, hwr = (b + 63) >> 6, WA = SH_TW + hwl + hwr, RA = SH_TH + a + b;
  u64* A = shadow_lds;
  u64* B = shadow_lds + RA * WA;
  const int y0 = (blockIdx.x / tiles_x) * SH_TH, j0 = (blockIdx.x % tiles_x) * SH_TW;
  const u64 fill = erode ? ~0ull : 0ull;
  for (int i = threadIdx.x; i < RA * WA; i += 256) A[i] = shadow_word(src, (long)y0 - a + i / WA, (long)j0 - hwl + i % WA, Hd, nwd, tailmask, erode);
  __syncthreads();
  for (int i = threadIdx.x; i < RA * SH_TW; i += 256) {
    const u64* row = A + (i / SH_TW) * WA;
    u64 acc = fill;
    int p = 64 * (i % SH_TW + hwl) - a;
    for (int d = 0; d <= a + b; ++d, ++p) {
      const int w = p >> 6, s = p & 63;
      u64 v = row[w] >> s;
      if (s) v |= row[w + 1] << (64 - s);
      acc = erode ? acc & v : acc | v;
    }
    B[i] = acc;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < SH_TH * SH_TW; i += 256) {
    const int rr = i / SH_TW, jj = i % SH_TW, y = y0 + rr, j = j0 + jj;
    if (y >= Hd || j >= nwd) continue;
    u64 acc = fill;
    for (int d = 0; d <= a + b; ++d) {
      const u64 v = B[(rr + d) * SH_TW + jj];
      acc = erode ? acc & v : acc | v;
    }
    if (j == nwd - 1) acc &= ~tailmask;
    dst[(long)y * nwd + j] = acc;
  }
}

// The same two passes through global memory, for windows whose tile does not fit in LDS: one lane per word.
__global__ __launch_bounds__(256) void shadow_close_row_kernel(const u64* __restrict__ src, u64* __restrict__ dst, int Hd, int nwd, u64 tailmask, int a,
                                                               int b, int erode) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)Hd * nwd) return;
  const long y = i / nwd, j = i % nwd;
  u64 acc = erode ? ~0ull : 0ull;
  long p = 64 * j - a;
  for (long d = 0; d <= (long)a + b; ++d, ++p) {
    const long w = p >> 6;
    const int s = (int)(p & 63);
    u64 v = shadow_word(src, y, w, Hd, nwd, tailmask, erode) >> s;
    if (s) v |= shadow_word(src, y, w + 1, Hd, nwd, tailmask, erode) << (64 - s);
    acc = erode ? acc & v : acc | v;
  }
  if (j == nwd - 1) acc &= ~tailmask;
  dst[i] = acc;
}

__global__ __launch_bounds__(256) void shadow_close_col_kernel(const u64* __restrict__ src, u64* __restrict__ dst, int Hd, int nwd, u64 tailmask, int a,
                                                               int b, int erode) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)Hd * nwd) return;
  const long y = i / nwd, j = i % nwd;
  u64 acc = erode ? ~0ull : 0ull;
  for (long d = -(long)a; d <= b; ++d) {
    const u64 v = shadow_word(src, y + d, j, Hd, nwd, tailmask, erode);
    acc = erode ? acc & v : acc | v;
  }
  if (j == nwd - 1) acc &= ~tailmask;
  dst[i] = acc;
}

// domain -> the image's own packed rows (nwc words per row, bits past W are 0)
__global__ __launch_bounds__(256) void shadow_crop_kernel(const u64* __restrict__ src, int Hd, int nwd, int Ex, int Ey, int H, int W, int nwc,
                                                          u64* __restrict__ crop) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)H * nwc) return;
  const long y = i / nwc, j = i % nwc, p = 64 * j + Ex;
  const long w = p >> 6;
  const int s = (int)(p & 63);
  u64 v = shadow_word(src, y + Ey, w, Hd, nwd, 0, 0) >> s;
  if (s) v |= shadow_word(src, y + Ey, w + 1, Hd, nwd, 0, 0) << (64 - s);
  if (j == nwc - 1 && (W & 63)) v &= ~(~0ull << (W & 63));
  crop[i] = v;
}

__global__ __launch_bounds__(256) void shadow_expand_kernel(const u64* __restrict__ crop, int H, int W, int nwc, unsigned char* __restrict__ out) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long)H * W) return;
  const long y = p / W, x = p % W;
  const unsigned char v = ((crop[y * nwc + (x >> 6)] >> (x & 63)) & 1) ? 255 : 0;
  out[3 * p] = v; out[3 * p + 1] = v; out[3 * p + 2] = v;
}

// ---- bounding box, box counts, fuse --------------------------------------------------------------------------------------------------
// info (int32): 0 any, 1 kw, 2 kh, 3 xmin, 4 xmax, 5 ymin, 6 ymax, 7 unused
// first stage, one lane per row: the row's first and last set column (INT_MAX, -1 for an empty row) and the exclusive prefix counts of
// its words, wprefix[y][0 .. nwc]
__global__ __launch_bounds__(256) void shadow_rows_kernel(const u64* __restrict__ crop, int H, int nwc, int* __restrict__ wprefix, int* __restrict__ rowinfo) {
  const int y = blockIdx.x * 256 + threadIdx.x;
  if (y >= H) return;
  int xmin = 0x7fffffff, xmax = -1, run = 0;
  for (int j = 0; j < nwc; ++j) {
    const u64 w = crop[(long)y * nwc + j];
    wprefix[(long)y * (nwc + 1) + j] = run;
    if (w) {
      if (xmax < 0) xmin = 64 * j + __builtin_ctzll(w);
      xmax = 64 * j + 63 - __builtin_clzll(w);
    }
    run += __popcll(w);
  }
  wprefix[(long)y * (nwc + 1) + nwc] = run;
  rowinfo[2 * y] = xmin; rowinfo[2 * y + 1] = xmax;
}

// second stage, one block: the box and kw = max(1, (xmax - xmin) / 5), kh likewise (mesh_shadow.py:94-97)
__global__ __launch_bounds__(256) void shadow_bbox_kernel(const int* __restrict__ rowinfo, int H, int* __restrict__ info) {
  __shared__ int sh[4][256];
  int xmin = 0x7fffffff, xmax = -1, ymin = 0x7fffffff, ymax = -1;
  for (int y = threadIdx.x; y < H; y += 256) {
    const int a = rowinfo[2 * y], b = rowinfo[2 * y + 1];
    if (b >= 0) { xmin = min(xmin, a); xmax = max(xmax, b); ymin = min(ymin, y); ymax = max(ymax, y); }
  }
  sh[0][threadIdx.x] = xmin; sh[1][threadIdx.x] = xmax; sh[2][threadIdx.x] = ymin; sh[3][threadIdx.x] = ymax;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      sh[0][threadIdx.x] = min(sh[0][threadIdx.x], sh[0][threadIdx.x + o]); sh[1][threadIdx.x] = max(sh[1][threadIdx.x], sh[1][threadIdx.x + o]);
      sh[2][threadIdx.x] = min(sh[2][threadIdx.x], sh[2][threadIdx.x + o]); sh[3][threadIdx.x] = max(sh[3][threadIdx.x], sh[3][threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int any = sh[1][0] >= 0;
    info[0] = any;
    info[1] = any ? max(1, (sh[1][0] - sh[0][0]) / 5) : 1;
    info[2] = any ? max(1, (sh[3][0] - sh[2][0]) / 5) : 1;
    info[3] = sh[0][0]; info[4] = sh[1][0]; info[5] = sh[2][0]; info[6] = sh[3][0]; info[7] = 0;
  }
}

// set pixels of row y in [0, x), 0 <= x <= W
__device__ __forceinline__ int shadow_row_prefix(const u64* __restrict__ row, const int* __restrict__ wp, int x) {
  const int j = x >> 6, b = x & 63;
  int c = wp[j];
  if (b) c += __popcll(row[j] & ~(~0ull << b));
  return c;
}

// sum of f over the window [x0, x0 + k) of an axis of length n under BORDER_REFLECT_101 (index -t -> t, n - 1 + t -> n - 1 - t), given
// F(i) = sum of f over [0, i); the window leaves the axis by less than n on either side, so it reflects at most once
#define SHADOW_WINDOW(F, x0, k, n, out)                                  \
  {                                                                      \
    const int x1_ = (x0) + (k);                                          \
    out = F(min(x1_, (n))) - F(max((x0), 0));                            \
    if ((x0) < 0) out += F(1 - (x0)) - F(1);                             \
    if (x1_ > (n)) out += F((n) - 1) - F(2 * (n) - 1 - x1_);             \
  }

// Column prefix of the row counts in two levels, rows in chunks of SHADOW_CH.  First level, one lane per (chunk, column):
// colprefix[y][x] = sum over the rows of y's chunk above y of the kw-window count of that row at x, chunksum[c][x] = the chunk's total.
#define SHADOW_CH 32
__global__ __launch_bounds__(256) void shadow_colprefix_kernel(const u64* __restrict__ crop, const int* __restrict__ wprefix, const int* __restrict__ info,
                                                               int H, int W, int nwc, long n, int* __restrict__ colprefix, int* __restrict__ chunksum) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n || !info[0]) return;
  const int x = (int)(t % W), c = (int)(t / W);
  const int kw = info[1], x0 = x - kw / 2, y_end = min(H, (c + 1) * SHADOW_CH);
  int run = 0;
  for (int y = c * SHADOW_CH; y < y_end; ++y) {
    colprefix[(long)y * W + x] = run;
    const u64* row = crop + (long)y * nwc;
    const int* wp = wprefix + (long)y * (nwc + 1);
#define SHADOW_FROW(i) shadow_row_prefix(row, wp, (i))
    int cnt;
    SHADOW_WINDOW(SHADOW_FROW, x0, kw, W, cnt)
#undef SHADOW_FROW
    run += cnt;
  }
  chunksum[(long)c * W + x] = run;
}

// second level, one lane per column: chunksum -> the exclusive prefix over the chunks, in place; entry n_chunks = the column's total
__global__ __launch_bounds__(256) void shadow_chunkscan_kernel(const int* __restrict__ info, int W, int n_chunks, int* __restrict__ chunksum) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= W || !info[0]) return;
  int run = 0;
  for (int c = 0; c < n_chunks; ++c) {
    const int v = chunksum[(long)c * W + x];
    chunksum[(long)c * W + x] = run;
    run += v;
  }
  chunksum[(long)n_chunks * W + x] = run;
}

// per pixel and channel, each line one rounded float64 operation (mesh_shadow.py:98-105):
//   b = count * (1.0 / (kw kh)); occ = 255 where b > 0 and not total_mask > 0; m = (b * occ) / 255; v = im * (1 - light_scale * m)
__global__ __launch_bounds__(256) void shadow_fuse_kernel(unsigned char* __restrict__ im, const unsigned char* __restrict__ total, const int* __restrict__ colprefix,
                                                          const int* __restrict__ chunkbase, const int* __restrict__ info, int* __restrict__ counts, int H, int W,
                                                          int n_chunks, double light_scale) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long)H * W || !info[0]) return;                                      // an empty mask: the image is left untouched
  const int y = (int)(p / W), x = (int)(p % W), kw = info[1], kh = info[2], y0 = y - kh / 2;
// rows above row i: the chunk's base plus the prefix inside it (i = H: the total)
#define SHADOW_FCOL(i) ((i) == H ? chunkbase[(long)n_chunks * W + x] : chunkbase[(long)((i) / SHADOW_CH) * W + x] + colprefix[(long)(i) * W + x])
  int cnt;
  SHADOW_WINDOW(SHADOW_FCOL, y0, kh, H, cnt)
#undef SHADOW_FCOL
  counts[p] = cnt;
  if (cnt == 0) return;                                                          // b = 0: every channel would be stored back as it is
  const double scale = 1.0 / (double)(kw * kh);
  const double b = (double)cnt * scale;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double occ = (b > 0. && !(total[3 * p + c] > 0)) ? 255. : 0.;
    const double m = (b * occ) / 255.;
    const double w = light_scale * m;
    const double v = (double)im[3 * p + c] * (1.0 - w);
    im[3 * p + c] = (unsigned char)v;
  }
}

// check = True: im[mask > 0] = 0
__global__ __launch_bounds__(256) void shadow_blank_kernel(unsigned char* __restrict__ im, const u64* __restrict__ crop, int H, int W, int nwc) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long)H * W) return;
  const long y = p / W, x = p % W;
  if ((crop[y * nwc + (x >> 6)] >> (x & 63)) & 1) { im[3 * p] = 0; im[3 * p + 1] = 0; im[3 * p + 2] = 0; }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
struct ShadowWs {
  long info, partial, plane, crop, wprefix, rowinfo, colprefix, chunks, counts, fixed_end, bits_a, bits_b, total;
  long Hd, Wd, nwd, nwc;
  int Ex, Ey, a, b;
};

static inline long shadow_up(long x) { return (x + 255) & ~255l; }

// false: a shape the index types do not hold, or a bad parameter
static bool shadow_layout(int H, int W, long N, int r, int iter, ShadowWs& L) {
  if (H < 1 || W < 1 || N < 0 || N > 0x7fffffffl || r < 1 || iter < 0 || (long)H * W > 0x7fffffffl) return false;
  const long P = (long)H * W;
  L.nwc = ((long)W + 63) / 64;
  const long reach = (long)iter * (r / 2);
  L.Ex = (int)(reach < W ? reach : W); L.Ey = (int)(reach < H ? reach : H);
  L.Wd = (long)W + 2 * L.Ex; L.Hd = (long)H + 2 * L.Ey; L.nwd = (L.Wd + 63) / 64;
  if (L.Hd > 0x7fffffffl || L.Wd > 0x7fffffffl || L.Hd * L.nwd > 0x7fffffffl) return false;
  const long dmax = L.Hd > L.Wd ? L.Hd : L.Wd;
  L.a = (int)(r / 2 < dmax ? r / 2 : dmax);
  L.b = (int)(r - 1 - r / 2 < dmax ? r - 1 - r / 2 : dmax);
  long o = 0;
  L.info = o; o += 256;
  L.partial = o; o += SHADOW_PARTS * 8;
  L.plane = o; o = shadow_up(o + P);
  L.crop = o; o = shadow_up(o + (long)H * L.nwc * 8);
  L.wprefix = o; o = shadow_up(o + (long)H * (L.nwc + 1) * 4);
  L.rowinfo = o; o = shadow_up(o + (long)H * 8);
  L.colprefix = o; o = shadow_up(o + P * 4);
  L.chunks = o; o = shadow_up(o + (((long)H + SHADOW_CH - 1) / SHADOW_CH + 1) * W * 4);
  L.counts = o; o = shadow_up(o + P * 4);
  L.fixed_end = o;
  L.bits_a = o; o = shadow_up(o + L.Hd * L.nwd * 8);
  L.bits_b = o; o = shadow_up(o + L.Hd * L.nwd * 8);
  L.total = o;
  return true;
}

static inline bool shadow_overlap(const void* p, long n, const void* q, long m) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return p != nullptr && q != nullptr && a < b + (uintptr_t)m && b < a + (uintptr_t)n;
}

static inline unsigned shadow_blocks(long n) { return (unsigned)((n + 255) / 256); }

extern "C" long snerf_shadow_ws_bytes(int H, int W, long N, int r, int iter) {
  ShadowWs L;
  return shadow_layout(H, W, N, r, iter, L) ? L.total : 0;
}

extern "C" long snerf_shadow_ws_offset(int H, int W, int which) {
  ShadowWs L;
  if (!shadow_layout(H, W, 0, 1, 0, L) || which < 0 || which > 1) return -1;
  return which == 0 ? L.info : L.counts;
}

extern "C" int snerf_shadow_project(const void* vertices, int vertices_f64, long N, const double* xf, int ground_mode, int H, int W, void* mask_out,
                                    void* ws, long ws_bytes, void* stream) {
  ShadowWs L;
  if (!shadow_layout(H, W, N, 1, 0, L) || xf == nullptr || ws == nullptr || ((uintptr_t)ws & 7) || ws_bytes < L.total || (vertices == nullptr && N > 0) ||
      (vertices_f64 != 0 && vertices_f64 != 1) || ground_mode < 0 || ground_mode > 2)
    return SNERF_ERR_ARG;
  const long P = (long)H * W;
  if (shadow_overlap(mask_out, 3 * P, ws, ws_bytes) || shadow_overlap(mask_out, 3 * P, vertices, N * (vertices_f64 ? 24 : 12))) return SNERF_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  char* base = (char*)ws;
  unsigned char* plane = (unsigned char*)(base + L.plane);
  hipMemsetAsync(plane, 0, P, s);
  if (N > 0) {
    ShadowXf t;
    for (int i = 0; i < 12; ++i) t.A[i] = xf[i];
    for (int i = 0; i < 3; ++i) t.L[i] = xf[12 + i];
    t.g = xf[15];
    for (int i = 0; i < 12; ++i) t.M[i] = xf[16 + i];
    t.mode = ground_mode;
    const long nb = (N + 255) / 256;
    const int parts = (int)(nb < SHADOW_PARTS ? nb : SHADOW_PARTS);
    double* partial = (double*)(base + L.partial);
    if (ground_mode == 1) hipLaunchKernelGGL(shadow_zmin_kernel, dim3(parts), dim3(256), 0, s, t, vertices, vertices_f64, N, partial);
    hipLaunchKernelGGL(shadow_splat_kernel, dim3((unsigned)nb), dim3(256), 0, s, t, vertices, vertices_f64, N, (const double*)partial, parts, plane, H, W);
  }
  if (mask_out != nullptr) hipLaunchKernelGGL(shadow_plane_expand_kernel, dim3(shadow_blocks(P)), dim3(256), 0, s, (const unsigned char*)plane, P, (unsigned char*)mask_out);
  return snerf_check_launch();
}

extern "C" int snerf_shadow_close(const void* mask_in, int H, int W, int r, int iter, void* mask_out, void* ws, long ws_bytes, void* stream) {
  ShadowWs L;
  if (!shadow_layout(H, W, 0, r, iter, L) || ws == nullptr || ((uintptr_t)ws & 7) || ws_bytes < L.total) return SNERF_ERR_ARG;
  const long P = (long)H * W;
  // mask_out == mask_in is safe (the input is packed before anything is written); a partial overlap is not
  if ((mask_in != mask_out && shadow_overlap(mask_in, 3 * P, mask_out, 3 * P)) || shadow_overlap(mask_in, 3 * P, ws, ws_bytes) ||
      shadow_overlap(mask_out, 3 * P, ws, ws_bytes))
    return SNERF_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  char* base = (char*)ws;
  u64* bits[2] = {(u64*)(base + L.bits_a), (u64*)(base + L.bits_b)};
  u64* crop = (u64*)(base + L.crop);
  const unsigned char* src = mask_in != nullptr ? (const unsigned char*)mask_in : (const unsigned char*)(base + L.plane);
  const int stride = mask_in != nullptr ? 3 : 1;
  if (iter == 0) {
    const long nw = (long)H * L.nwc;
    hipLaunchKernelGGL(shadow_pack_kernel, dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, s, src, stride, H, W, 0, 0, nw, (int)L.nwc, crop);
  } else {
    const int Hd = (int)L.Hd, nwd = (int)L.nwd;
    const long nw = L.Hd * L.nwd;
    const u64 tailmask = (L.Wd & 63) ? ~0ull << (L.Wd & 63) : 0ull;
    hipLaunchKernelGGL(shadow_pack_kernel, dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, s, src, stride, H, W, L.Ex, L.Ey, nw, nwd, bits[0]);
    const long RA = (long)SH_TH + L.a + L.b, WA = SH_TW + (L.a + 63) / 64 + (L.b + 63) / 64, lds = RA * (WA + SH_TW) * 8;
    const long tiles_x = (L.nwd + SH_TW - 1) / SH_TW, tiles = tiles_x * ((L.Hd + SH_TH - 1) / SH_TH);
    for (int k = 0; k < 2 * iter; ++k) {                                          // dilations first, then erosions; the result ends in bits[0]
      const int erode = k >= iter;
      if (lds <= 65536) {
        hipLaunchKernelGGL(shadow_close_tile_kernel, dim3((unsigned)tiles), dim3(256), (size_t)lds, s, (const u64*)bits[k & 1], bits[(k & 1) ^ 1], Hd, nwd,
                           tailmask, L.a, L.b, erode, (int)tiles_x);
      } else {
        hipLaunchKernelGGL(shadow_close_row_kernel, dim3(shadow_blocks(nw)), dim3(256), 0, s, (const u64*)bits[0], bits[1], Hd, nwd, tailmask, L.a, L.b, erode);
        hipLaunchKernelGGL(shadow_close_col_kernel, dim3(shadow_blocks(nw)), dim3(256), 0, s, (const u64*)bits[1], bits[0], Hd, nwd, tailmask, L.a, L.b, erode);
      }
    }
    // an even number of tile launches swaps back to bits[0]; a row + column pair never leaves it
    hipLaunchKernelGGL(shadow_crop_kernel, dim3(shadow_blocks((long)H * L.nwc)), dim3(256), 0, s, (const u64*)bits[0], Hd, nwd, L.Ex, L.Ey, H, W, (int)L.nwc,
                       crop);
  }
  if (mask_out != nullptr) hipLaunchKernelGGL(shadow_expand_kernel, dim3(shadow_blocks(P)), dim3(256), 0, s, (const u64*)crop, H, W, (int)L.nwc, (unsigned char*)mask_out);
  return snerf_check_launch();
}

extern "C" int snerf_shadow_fuse(void* im, const void* total_mask, const void* shadow_mask, int H, int W, double light_scale, int check, void* ws,
                                 long ws_bytes, void* stream) {
  ShadowWs L;
  if (!shadow_layout(H, W, 0, 1, 0, L) || im == nullptr || ws == nullptr || ((uintptr_t)ws & 7) || ws_bytes < L.total || (check != 0 && check != 1) ||
      (!check && (total_mask == nullptr || !(light_scale >= 0. && light_scale <= 1.))))
    return SNERF_ERR_ARG;
  const long P = (long)H * W;
  if (shadow_overlap(im, 3 * P, total_mask, 3 * P) || shadow_overlap(im, 3 * P, shadow_mask, 3 * P) || shadow_overlap(im, 3 * P, ws, ws_bytes) ||
      shadow_overlap(shadow_mask, 3 * P, ws, ws_bytes) || shadow_overlap(total_mask, 3 * P, ws, ws_bytes))
    return SNERF_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  char* base = (char*)ws;
  u64* crop = (u64*)(base + L.crop);
  const int nwc = (int)L.nwc;
  if (shadow_mask != nullptr) {
    const long nw = (long)H * nwc;
    hipLaunchKernelGGL(shadow_pack_kernel, dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, s, (const unsigned char*)shadow_mask, 3, H, W, 0, 0, nw, nwc, crop);
  }
  if (check) {
    hipLaunchKernelGGL(shadow_blank_kernel, dim3(shadow_blocks(P)), dim3(256), 0, s, (unsigned char*)im, (const u64*)crop, H, W, nwc);
    return snerf_check_launch();
  }
  int* info = (int*)(base + L.info);
  int* wprefix = (int*)(base + L.wprefix);
  int* rowinfo = (int*)(base + L.rowinfo);
  int* colprefix = (int*)(base + L.colprefix);
  hipLaunchKernelGGL(shadow_rows_kernel, dim3(shadow_blocks(H)), dim3(256), 0, s, (const u64*)crop, H, nwc, wprefix, rowinfo);
  hipLaunchKernelGGL(shadow_bbox_kernel, dim3(1), dim3(256), 0, s, (const int*)rowinfo, H, info);
  int* chunks = (int*)(base + L.chunks);
  const int n_chunks = (H + SHADOW_CH - 1) / SHADOW_CH;
  const long n_lanes = (long)n_chunks * W;
  hipLaunchKernelGGL(shadow_colprefix_kernel, dim3(shadow_blocks(n_lanes)), dim3(256), 0, s, (const u64*)crop, (const int*)wprefix, (const int*)info, H, W, nwc,
                     n_lanes, colprefix, chunks);
  hipLaunchKernelGGL(shadow_chunkscan_kernel, dim3(shadow_blocks(W)), dim3(256), 0, s, (const int*)info, W, n_chunks, chunks);
  hipLaunchKernelGGL(shadow_fuse_kernel, dim3(shadow_blocks(P)), dim3(256), 0, s, (unsigned char*)im, (const unsigned char*)total_mask, (const int*)colprefix,
                     (const int*)chunks, (const int*)info, (int*)(base + L.counts), H, W, n_chunks, light_scale);
  return snerf_check_launch();
}
