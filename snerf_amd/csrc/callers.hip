// The two steps either side of the render path: ray generation (before) and the per-ray loss tail
// (after).  Compiled with -ffp-contract=off: every operation rounds like the reference's separate fp32 torch ops.
#include "common.h"

// ---------------------------------------------------------------------------
// Pinhole rays.  s-nerf/utils/sample_utils.py:286-345 (get_rays_single_img: whole frame, half-pixel centres) and :92-211
// (sample_single_img: selected pixels; directions from run_nerf_helpers.get_rays_by_coord :300-312, i.e. WITHOUT the
// half-pixel offset, radii still from the half-pixel grid), no-NDC branch.  One lane per ray.
// ---------------------------------------------------------------------------
struct RayGen {
  const int* coords;      // [N,2] (row, col) or null: pixel index first + n, row-major over W
  long first;
  int W, H, training;
  float p[12];            // pose [3,4] row-major
  float cx, cy, fx, fy, near, far;
  long N;
  float *origins, *directions, *viewdirs, *radii, *near_out, *far_out;
};

__device__ __forceinline__ void cam_dir(const float* p, float cx, float cy, float jj, float ii, float f, float off, float* d) {
  const float c0 = (ii - cx + off) / f, c1 = -((jj - cy + off) / f), c2 = -1.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) d[c] = (c0 * p[4 * c + 0] + c1 * p[4 * c + 1]) + c2 * p[4 * c + 2];
}

// the ray of pixel (row, col): direction d, unit view direction v, radius; the origin is p[3], p[7], p[11].  Shared by the pixel
// list launch below and the training batcher (snerf_mip_image_batch), which must agree with it bit for bit.
__device__ __forceinline__ void pinhole_ray(const float* p, float cx, float cy, float fx, float fy, int H, int row, int col, int training,
                                            float* d, float* v, float* radius) {
  const float f = (fx + fy) / 2.f;
  const float jj = (float)row, ii = (float)col;
  if (training) {
    // get_rays_by_coord: i = (col - cx) / focal, j = -(row - cy) / focal
    const float c0 = (ii - cx) / f, c1 = -((jj - cy) / f);
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = (c0 * p[4 * c + 0] + c1 * p[4 * c + 1]) + (-1.f) * p[4 * c + 2];
  } else {
    cam_dir(p, cx, cy, jj, ii, f, 0.5f, d);
  }
  // radius: distance to the neighbour one row down on the half-pixel grid; the reference appends dx[-2:-1] for the last image
  // row, i.e. the value of row H-3 (sample_utils.py:309-310), not that of row H-2
  const float ja = row >= H - 1 ? (float)(H - 3) : jj;
  float d0[3], d1[3];
  cam_dir(p, cx, cy, ja, ii, f, 0.5f, d0);
  cam_dir(p, cx, cy, ja + 1.f, ii, f, 0.5f, d1);
  const float e0 = d0[0] - d1[0], e1 = d0[1] - d1[1], e2 = d0[2] - d1[2];
  const float dx = sqrtf((e0 * e0 + e1 * e1) + e2 * e2);
  const float nrm = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = d[c] / nrm;
  *radius = dx * 2.f / 3.4641016151377544f;            // dx[..., None] * 2 / np.sqrt(12)
}

__global__ __launch_bounds__(256) void pinhole_rays_kernel(RayGen a) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.N) return;
  int row, col;
  if (a.coords != nullptr) { row = a.coords[2 * r]; col = a.coords[2 * r + 1]; }
  else { const long pix = a.first + r; row = (int)(pix / a.W); col = (int)(pix - (long)row * a.W); }
  float d[3], v[3], rad;
  pinhole_ray(a.p, a.cx, a.cy, a.fx, a.fy, a.H, row, col, a.training, d, v, &rad);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    a.origins[3 * r + c] = a.p[4 * c + 3];
    a.directions[3 * r + c] = d[c];
    a.viewdirs[3 * r + c] = v[c];
  }
  a.radii[r] = rad;
  a.near_out[r] = a.near;
  a.far_out[r] = a.far;
}

extern "C" int snerf_pinhole_rays(const int* coords, long first_pixel, int W, int H, const float* pose_host, float cx, float cy, float fx,
                                  float fy, int training, float near, float far, long N, float* origins, float* directions,
                                  float* viewdirs, float* radii, float* near_out, float* far_out, void* stream) {
  if (N <= 0) return SNERF_OK;
  if (pose_host == nullptr || W <= 0 || H < 3) return SNERF_ERR_ARG;
  RayGen a{coords, first_pixel, W, H, training, {}, cx, cy, fx, fy, near, far, N, origins, directions, viewdirs, radii, near_out, far_out};
  for (int k = 0; k < 12; ++k) a.p[k] = pose_host[k];
  hipLaunchKernelGGL(pinhole_rays_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return snerf_check_launch();
}

// ---------------------------------------------------------------------------
// Classic-path ray front end: get_rays (s-nerf/model/run_nerf_helpers.py:247-258), ndc_rays (:314-332) and the
// ray-batch assembly of render() (s-nerf/model/render.py:50-77) -- pinhole directions or given rays, unit view directions from
// the PRE-NDC directions, the optional static camera that replaces the rays but not the view directions, the NDC warp, and the
// row layout [o3, d3, near, far, (depth), (viewdir3)] -- as ONE lane-per-ray launch writing the [N, ld] rows render_rays reads.
// Every operation rounds like the reference's separate fp32 torch ops (-ffp-contract=off, explicit association).
// ---------------------------------------------------------------------------
struct ClassicRays {
  const float *rays_o, *rays_d;   // given rays [n,3] (contiguous) or null: pinhole rays of the H x W frame from c2w
  long n;
  int H, W;
  float focal, cx, cy;            // fp32 roundings of the reference's python scalars
  float c2w[12], c2w_static[12];  // [3,4] row-major
  int has_c2w, has_static, ndc, use_viewdirs;
  float ndc_near, near, far;
  float ndc_cw, ndc_ch;           // -1/(W/(2 focal)), -1/(H/(2 focal)) computed in double on the host like the python scalars
  const float* depths;            // optional extra column
  float* rows; int ld;            // ray batch rows, or null
  float *o_out, *d_out;           // separate [n,3] outputs (get_rays / ndc_rays), or null
};

__device__ __forceinline__ void classic_pinhole(const float* c2w, int row, int col, float focal, float cx, float cy, float* o, float* d) {
  // dirs = [((i + 0.5) - cx) / focal, -((j + 0.5) - cy) / focal, -1];  rays_d = sum(dirs[None, :] * c2w[:3, :3], -1)
  const float c0 = (((float)col + 0.5f) - cx) / focal, c1 = -((((float)row + 0.5f) - cy) / focal), c2 = -1.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    d[c] = (c0 * c2w[4 * c + 0] + c1 * c2w[4 * c + 1]) + c2 * c2w[4 * c + 2];
    o[c] = c2w[4 * c + 3];
  }
}

// (ndc_cw, ndc_ch) = (-1/(W/(2 focal)), -1/(H/(2 focal))), computed in double like the python scalars and rounded once
__device__ __forceinline__ void classic_ndc(float ndc_near, float ndc_cw, float ndc_ch, float* o, float* d) {
  const float t = -(ndc_near + o[2]) / d[2];
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = o[c] + t * d[c];
  const float o0 = ndc_cw * o[0] / o[2], o1 = ndc_ch * o[1] / o[2], o2 = 1.f + (2.f * ndc_near) / o[2];
  const float d0 = ndc_cw * (d[0] / d[2] - o[0] / o[2]), d1 = ndc_ch * (d[1] / d[2] - o[1] / o[2]), d2 = (-2.f * ndc_near) / o[2];
  o[0] = o0; o[1] = o1; o[2] = o2;
  d[0] = d0; d[1] = d1; d[2] = d2;
}

// viewdirs = rays_d / norm(rays_d) (render.py:52-53), from the PRE-NDC directions
__device__ __forceinline__ void classic_unit(const float* d, float* v) {
  const float nrm = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = d[c] / nrm;
}

// one row [o3, d3, near, far, (depth), (viewdir3)] of the ray batch (render.py:70-77)
__device__ __forceinline__ void classic_store_row(float* q, const float* o, const float* d, float near, float far, const float* depth,
                                                  int use_viewdirs, const float* v) {
  q[0] = o[0]; q[1] = o[1]; q[2] = o[2]; q[3] = d[0]; q[4] = d[1]; q[5] = d[2];
  q[6] = near; q[7] = far;                             // near * ones_like(d[..., :1]): exact
  int k = 8;
  if (depth != nullptr) q[k++] = *depth;
  if (use_viewdirs) { q[k] = v[0]; q[k + 1] = v[1]; q[k + 2] = v[2]; }
}

__global__ __launch_bounds__(256) void classic_rays_kernel(ClassicRays a) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.n) return;
  const int row = (int)(r / a.W), col = (int)(r - (long)row * a.W);
  float o[3], d[3], v[3];
  if (a.has_c2w) classic_pinhole(a.c2w, row, col, a.focal, a.cx, a.cy, o, d);
  else {
#pragma unroll
    for (int c = 0; c < 3; ++c) { o[c] = a.rays_o[3 * r + c]; d[c] = a.rays_d[3 * r + c]; }
  }
  if (a.use_viewdirs) {
    classic_unit(d, v);
    // c2w_staticcam: the rays come from the static camera (principal point at the image centre: render.py:59 passes no
    // ori_points), the view directions stay those of c2w
    if (a.has_static) classic_pinhole(a.c2w_static, row, col, a.focal, (float)(a.W * 0.5), (float)(a.H * 0.5), o, d);
  }
  if (a.ndc) classic_ndc(a.ndc_near, a.ndc_cw, a.ndc_ch, o, d);
  if (a.o_out != nullptr) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { a.o_out[3 * r + c] = o[c]; a.d_out[3 * r + c] = d[c]; }
  }
  if (a.rows != nullptr)
    classic_store_row(a.rows + r * a.ld, o, d, a.near, a.far, a.depths != nullptr ? a.depths + r : nullptr, a.use_viewdirs, v);
}

static int classic_rays_launch(ClassicRays& a, void* stream) {
  if (a.n <= 0) return SNERF_OK;
  hipLaunchKernelGGL(classic_rays_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return snerf_check_launch();
}

extern "C" int snerf_classic_get_rays(int H, int W, double focal, double cx, double cy, const float* c2w_host, float* rays_o, float* rays_d,
                                      void* stream) {
  if (H <= 0 || W <= 0 || c2w_host == nullptr || rays_o == nullptr || rays_d == nullptr) return SNERF_ERR_ARG;
  ClassicRays a{};
  a.n = (long)H * W; a.H = H; a.W = W; a.focal = (float)focal; a.cx = (float)cx; a.cy = (float)cy; a.has_c2w = 1;
  for (int k = 0; k < 12; ++k) a.c2w[k] = c2w_host[k];
  a.o_out = rays_o; a.d_out = rays_d;
  return classic_rays_launch(a, stream);
}

extern "C" int snerf_classic_ndc_rays(int H, int W, double focal, float near, const float* rays_o, const float* rays_d, long n, float* o_out,
                                      float* d_out, void* stream) {
  if (H <= 0 || W <= 0 || rays_o == nullptr || rays_d == nullptr || o_out == nullptr || d_out == nullptr) return SNERF_ERR_ARG;
  ClassicRays a{};
  a.n = n; a.H = H; a.W = W; a.rays_o = rays_o; a.rays_d = rays_d; a.ndc = 1; a.ndc_near = near;
  a.ndc_cw = (float)(-1.0 / ((double)W / (2.0 * focal))); a.ndc_ch = (float)(-1.0 / ((double)H / (2.0 * focal)));
  a.o_out = o_out; a.d_out = d_out;
  return classic_rays_launch(a, stream);
}

extern "C" int snerf_classic_ray_batch(int H, int W, double focal, double cx, double cy, const float* c2w_host, const float* c2w_static_host,
                                       const float* rays_o, const float* rays_d, long n, int ndc, float near, float far,
                                       const float* depths, int use_viewdirs, float* rows, int ld, void* stream) {
  const int need = 8 + (depths != nullptr ? 1 : 0) + (use_viewdirs ? 3 : 0);
  if (H <= 0 || W <= 0 || rows == nullptr || ld < need) return SNERF_ERR_ARG;
  if (c2w_host == nullptr && (rays_o == nullptr || rays_d == nullptr)) return SNERF_ERR_ARG;
  if (c2w_host != nullptr && n != (long)H * W) return SNERF_ERR_ARG;
  if (c2w_static_host != nullptr && n != (long)H * W) return SNERF_ERR_ARG;
  ClassicRays a{};
  a.n = n; a.H = H; a.W = W; a.focal = (float)focal; a.cx = (float)cx; a.cy = (float)cy;
  a.rays_o = rays_o; a.rays_d = rays_d;
  if (c2w_host != nullptr) { a.has_c2w = 1; for (int k = 0; k < 12; ++k) a.c2w[k] = c2w_host[k]; }
  if (c2w_static_host != nullptr) { a.has_static = 1; for (int k = 0; k < 12; ++k) a.c2w_static[k] = c2w_static_host[k]; }
  a.ndc = ndc; a.ndc_near = 1.f;                       // render.py:66 passes near = 1. to ndc_rays
  a.ndc_cw = (float)(-1.0 / ((double)W / (2.0 * focal))); a.ndc_ch = (float)(-1.0 / ((double)H / (2.0 * focal)));
  a.near = near; a.far = far; a.depths = depths; a.use_viewdirs = use_viewdirs; a.rows = rows; a.ld = ld;
  return classic_rays_launch(a, stream);
}

// ---------------------------------------------------------------------------
// Per-ray loss tail of the mip path (s-nerf/train.py:150-208): RgbLoss (loss_factory.py:5-11), calc_depth_loss with DepthLoss
// and per-ray confidence (confidence.py:209-224, loss_factory.py:26-37) and ProposalLoss (loss_factory.py:59-74), forward
// value AND the gradients w.r.t. the renderer outputs in one pass.  One lane per ray; prefix sums in the canonical order
// (fp64 accumulate, one rounding per emitted fp32 value), which is what torch.cumsum does on the CPU.
// out[0..3] = {#valid depth rays, rgb loss, depth loss (x depth_lambda), proposal loss (x proposal_lambda)}.
// ---------------------------------------------------------------------------
struct LossTail {
  const float *rgb, *tgt, *dist1, *dist0, *tdepth, *conf;
  const float *s_f, *w_f, *s_c, *w_c;
  long N;
  int Pf, Sc, disparity;
  float depth_lambda, coarse_mult, prop_lambda;
  float* out;
  float *g_rgb, *g_dist1, *g_dist0, *g_wc;
};

__global__ __launch_bounds__(1024) void loss_prepare_kernel(const float* __restrict__ tdepth, long N, float* __restrict__ out) {
  __shared__ int part[16];
  int cnt = 0;
  if (tdepth != nullptr)
    for (long r = threadIdx.x; r < N; r += 1024) cnt += tdepth[r] != 0.f;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < 16; ++w) t += part[w];
    out[0] = (float)t; out[1] = 0.f; out[2] = 0.f; out[3] = 0.f; out[4] = 0.f;
  }
}

// (loss_tail_proposal / loss_tail_depth below restate the depth and proposal blocks of this kernel for the masked tail: an edit to
// either side must be mirrored on the other; tests/test_mip_semantic_step.py compares the two entries' gradients bit for bit.)
__global__ __launch_bounds__(64) void loss_tail_kernel(LossTail a) {
  const long r = (long)blockIdx.x * 64 + threadIdx.x;
  float l_rgb = 0.f, l_dep = 0.f, l_prop = 0.f;
  if (r < a.N) {
    // ---- RGB: mean over N*3 of (pred - tgt)^2
    const float inv = 1.f / (3.f * (float)a.N);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float d = a.rgb[3 * r + c] - a.tgt[3 * r + c];
      l_rgb += d * d;
      a.g_rgb[3 * r + c] = d * (2.f * inv);
    }
    l_rgb *= inv;
    // ---- depth: masked mean over the rays with a LiDAR target
    if (a.tdepth != nullptr) {
      const float t = a.tdepth[r];
      float g1 = 0.f, g0 = 0.f;
      if (t != 0.f) {
        const float nv = a.out[0];
        const float cw = (a.conf != nullptr ? a.conf[r] : 1.f);
        const float d1 = a.dist1[r], d0 = a.dist0[r];
        float e1, e0, s1, s0;
        if (a.disparity) { e1 = 1.f / d1 - 1.f / t; e0 = 1.f / d0 - 1.f / t; s1 = -1.f / (d1 * d1); s0 = -1.f / (d0 * d0); }
        else { e1 = d1 - t; e0 = d0 - t; s1 = 1.f; s0 = 1.f; }
        const float k = cw * a.depth_lambda / nv;
        l_dep = (fabsf(e1) + a.coarse_mult * fabsf(e0)) * k;
        g1 = (e1 > 0.f ? 1.f : (e1 < 0.f ? -1.f : 0.f)) * s1 * k;
        g0 = (e0 > 0.f ? 1.f : (e0 < 0.f ? -1.f : 0.f)) * s0 * k * a.coarse_mult;
      }
      a.g_dist1[r] = g1;
      a.g_dist0[r] = g0;
    }
    // ---- proposal: the coarse histogram must bound the (detached) fine weights from above
    if (a.s_c != nullptr) {
      const float* sf = a.s_f + r * a.Pf;
      const float* wf = a.w_f + r * (a.Pf - 1);
      const float* sc = a.s_c + r * (a.Sc + 1);
      const float* wc = a.w_c + r * a.Sc;
      float* g = a.g_wc + r * a.Sc;
      for (int j = 0; j < a.Sc; ++j) g[j] = 0.f;
      const int cap = min(a.Pf - 2, a.Sc - 1);          // the reference clamps `right` with the FINE interval count
      const float scale = a.prop_lambda / (float)a.N;
      // walk both sorted fence-post lists once; p = #(s_c <= s_f[k]) (searchsorted right=True); C = cumsum(w_c)
      int p = 0;
      double cum = 0.0;
      float Wlast = 0.f;                                 // C[min(p-1, Sc-1)]
      float Wcap = 0.f;                                  // C[cap], known once p-1 >= cap
      const float W0 = wc[0];                            // C[0]: the reference clamps the left index at 0 (not "empty prefix")
      float left = 0.f;
      int li = 0;
      for (int k = 0; k < a.Pf; ++k) {
        const float s = sf[k];
        while (p <= a.Sc && sc[p] <= s) {
          if (p < a.Sc) { cum += (double)wc[p]; Wlast = (float)cum; if (p == cap) Wcap = Wlast; }
          ++p;
        }
        const int idx = p - 1;                           // inds - 1 of this fence post
        if (k > 0) {
          const int ri = idx > cap ? cap : max(idx, 0);
          const float right = idx > cap ? Wcap : (idx <= 0 ? W0 : Wlast);
          const float w = wf[k - 1];
          const float over = w - (right - left);
          if (over > 0.f) {
            l_prop += over * over / (w + 1e-8f);
            const float gb = -2.f * over / (w + 1e-8f) * scale;
            g[ri] += gb;
            g[li] -= gb;
          }
        }
        li = idx <= 0 ? 0 : min(idx, a.Sc - 1);          // (an index past the last interval raises in the reference)
        left = idx <= 0 ? W0 : Wlast;
      }
      l_prop *= scale;
      // d/dw_c[j] = sum_{k >= j} dW[k]
      double acc = 0.0;
      for (int j = a.Sc - 1; j >= 0; --j) { acc += (double)g[j]; g[j] = (float)acc; }
    }
  }
  l_rgb = wave_sum(l_rgb); l_dep = wave_sum(l_dep); l_prop = wave_sum(l_prop);
  if (threadIdx.x == 0) {
    atomicAdd(a.out + 1, l_rgb);
    if (a.tdepth != nullptr) atomicAdd(a.out + 2, l_dep);
    if (a.s_c != nullptr) atomicAdd(a.out + 3, l_prop);
    atomicAdd(a.out + 4, (l_rgb + l_dep) + l_prop);     // the total: the step's loss scalar without a fold launch behind the tail
  }
}

extern "C" int snerf_mip_loss_tail(const float* rgb, const float* tgt, const float* dist1, const float* dist0, const float* tdepth,
                                   const float* conf, const float* s_f, const float* w_f, const float* s_c, const float* w_c, long N,
                                   int Pf, int Sc, int disparity, float depth_lambda, float coarse_mult, float prop_lambda, float* out,
                                   float* g_rgb, float* g_dist1, float* g_dist0, float* g_wc, void* stream) {
  if (N <= 0) return SNERF_OK;
  if (rgb == nullptr || tgt == nullptr || out == nullptr || g_rgb == nullptr) return SNERF_ERR_ARG;
  if (tdepth != nullptr && (dist1 == nullptr || dist0 == nullptr || g_dist1 == nullptr || g_dist0 == nullptr)) return SNERF_ERR_ARG;
  if (s_c != nullptr && (s_f == nullptr || w_f == nullptr || w_c == nullptr || g_wc == nullptr || Pf < 2 || Sc < 1)) return SNERF_ERR_ARG;
  hipLaunchKernelGGL(loss_prepare_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, tdepth, N, out);
  LossTail a{rgb, tgt, dist1, dist0, tdepth, conf, s_f, w_f, s_c, w_c, N, Pf, Sc, disparity, depth_lambda, coarse_mult, prop_lambda, out,
             g_rgb, g_dist1, g_dist0, g_wc};
  hipLaunchKernelGGL(loss_tail_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
  return snerf_check_launch();
}

// ---------------------------------------------------------------------------
// Loss tail of the classic path: the stock training loop around render_rays, img2mse / mse2psnr (s-nerf/model/run_nerf_helpers.py:16-17)
// on the fine and the coarse colour map, value and gradients in two launches.
//   img_loss = mean((rgb - tgt)^2), img_loss0 = mean((rgb0 - tgt)^2) (rgb0 null: 0), loss = img_loss + img_loss0,
//   psnr = -10 ln(img_loss) / ln 10;  out[4] = {loss, img_loss, img_loss0, psnr}
//   g_rgb[i] = inv (2 (rgb[i] - tgt[i])), inv = 1.f / (float)(3 N): what torch's mean / pow backward evaluate, in fp32
// The sums are taken in double (the differences too: the squares are exact to double rounding) in an order that depends on N only:
// ray r belongs to thread r mod (256 blocks(N)) and is taken in ascending order, the 64 lanes of a wave fold with shuffles, the 4
// waves of a workgroup through LDS in wave order, the workgroups' partials (ws[2 b + k]) in block order by the finish launch, which
// forms the four scalars in double and rounds each once.  No floating-point atomics: the same bits every run, graph-safe.
// ---------------------------------------------------------------------------
#define CLASSIC_TAIL_MAX_BLOCKS 256
static inline int classic_tail_blocks(long N) {
  const long b = (N + 255) / 256;
  return b < 1 ? 1 : (b > CLASSIC_TAIL_MAX_BLOCKS ? CLASSIC_TAIL_MAX_BLOCKS : (int)b);
}

struct ClassicTail {
  const float *rgb, *rgb0, *tgt;
  long N;
  double* ws; int blocks;
  float *out, *g_rgb, *g_rgb0;
};

__global__ __launch_bounds__(256) void classic_tail_partial_kernel(ClassicTail a) {
  __shared__ double red[4][2];
  const float inv = 1.0f / (float)(3 * a.N);
  double s1 = 0.0, s0 = 0.0;
  for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < a.N; r += (long)gridDim.x * 256) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float t = a.tgt[3 * r + c], x = a.rgb[3 * r + c];
      const double e = (double)x - (double)t;
      s1 += e * e;
      a.g_rgb[3 * r + c] = inv * (2.f * (x - t));
      if (a.rgb0 != nullptr) {
        const float y = a.rgb0[3 * r + c];
        const double e0 = (double)y - (double)t;
        s0 += e0 * e0;
        a.g_rgb0[3 * r + c] = inv * (2.f * (y - t));
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s0 += __shfl_xor(s0, o, 64); }
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = s1; red[threadIdx.x >> 6][1] = s0; }
  __syncthreads();
  if (threadIdx.x < 2) a.ws[2 * (long)blockIdx.x + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

__global__ __launch_bounds__(64) void classic_tail_finish_kernel(ClassicTail a) {
  if (threadIdx.x != 0) return;
  double s1 = 0.0, s0 = 0.0;
  for (int b = 0; b < a.blocks; ++b) { s1 += a.ws[2 * (long)b]; s0 += a.ws[2 * (long)b + 1]; }
  const double cnt = 3.0 * (double)a.N;
  const double l1 = s1 / cnt, l0 = a.rgb0 != nullptr ? s0 / cnt : 0.0;
  a.out[0] = (float)(l1 + l0);
  a.out[1] = (float)l1;
  a.out[2] = (float)l0;
  a.out[3] = (float)(-10.0 * log(l1) / log(10.0));
}

extern "C" long snerf_classic_loss_tail_ws(long N) { return N <= 0 ? 0 : 16L * classic_tail_blocks(N); }

extern "C" int snerf_classic_loss_tail(const float* rgb, const float* rgb0, const float* tgt, long N, void* ws, float* out, float* g_rgb,
                                       float* g_rgb0, void* stream) {
  if (N <= 0 || rgb == nullptr || tgt == nullptr || ws == nullptr || out == nullptr || g_rgb == nullptr) return SNERF_ERR_ARG;
  if ((rgb0 == nullptr) != (g_rgb0 == nullptr)) return SNERF_ERR_ARG;
  if ((((uintptr_t)rgb | (uintptr_t)rgb0 | (uintptr_t)tgt | (uintptr_t)out | (uintptr_t)g_rgb | (uintptr_t)g_rgb0) & 3) != 0 ||
      ((uintptr_t)ws & 7) != 0)
    return SNERF_ERR_ARG;
  ClassicTail a{rgb, rgb0, tgt, N, (double*)ws, classic_tail_blocks(N), out, g_rgb, g_rgb0};
  hipLaunchKernelGGL(classic_tail_partial_kernel, dim3((unsigned)a.blocks), dim3(256), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(classic_tail_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
  return snerf_check_launch();
}

// ---------------------------------------------------------------------------
// The same tail with the per-image rules of s-nerf/train.py:131-209: the semantic cross-entropy (SemanticLoss,
// loss_factory.py:13-24 = nn.CrossEntropyLoss, ignore_index -100, times semantic_lambda; only for images with labels), the Waymo
// side-camera mask (:137-144: rays of pixel rows >= a limit leave the RGB and the semantic mean) and the back-camera mask
// (:165-170, loss.py:344-346: rays of rows >= a limit, or with seg_mask != 0, leave the depth mean -- and only that).  The image
// is the device word *img_i, never read on the host; its rules come from three tables with one entry per image.  Per ray r:
//   Wr = rows[2 r] < rgb_row_limit[i];  Br = rows[2 r] < depth_row_limit[i] and depth_keep[r] == 0  (absent = true)
//   rgb       sum_{Wr} |rgb - tgt|^2 / (3 #W), gradient 0 where !Wr
//   depth     the plain tail's expression over the rays with tdepth != 0 and Br, divided by their number
//   semantic  sem_valid[i] != 0: semantic_lambda * mean over the rays with Wr and a label in [0, C) of -log softmax(sem_r)[label_r]
//             (float64 log-sum-exp after subtracting the row maximum, one rounding per emitted value); g_sem is written in full
//   proposal  every ray, as in the plain tail
// A term whose count is 0 is 0 and so are its gradients (the reference's empty mean is NaN); an image index outside the tables
// counts no ray for the rgb, depth and semantic terms.  The prepare launch forms the three counts and zeroes the sums.
// out[0..7] = {#depth rays, rgb, depth, proposal, total, semantic, #rgb rays, #semantic rays}: out[0..4] as in the plain tail.
// With every new pointer null the lanes do the plain tail's arithmetic in the plain tail's order.
// ---------------------------------------------------------------------------
// The proposal and depth terms of loss_tail_kernel as functions, statement for statement.  (The plain kernel keeps its inline text:
// routed through these functions it computed the same bits on another instruction schedule, 2 % slower -- 294 -> 300 us at 4096 rays
// on the MI355X.)
// ProposalLoss of ray r: the coarse histogram must bound the (detached) fine weights from above.  -> the ray's term (times
// prop_lambda / N); writes g_wc[r] = d term / d w_c[r].
__device__ __forceinline__ float loss_tail_proposal(const LossTail& a, long r) {
  float l_prop = 0.f;
  const float* sf = a.s_f + r * a.Pf;
  const float* wf = a.w_f + r * (a.Pf - 1);
  const float* sc = a.s_c + r * (a.Sc + 1);
  const float* wc = a.w_c + r * a.Sc;
  float* g = a.g_wc + r * a.Sc;
  for (int j = 0; j < a.Sc; ++j) g[j] = 0.f;
  const int cap = min(a.Pf - 2, a.Sc - 1);          // the reference clamps `right` with the FINE interval count
  const float scale = a.prop_lambda / (float)a.N;
  // walk both sorted fence-post lists once; p = #(s_c <= s_f[k]) (searchsorted right=True); C = cumsum(w_c)
  int p = 0;
  double cum = 0.0;
  float Wlast = 0.f;                                 // C[min(p-1, Sc-1)]
  float Wcap = 0.f;                                  // C[cap], known once p-1 >= cap
  const float W0 = wc[0];                            // C[0]: the reference clamps the left index at 0 (not "empty prefix")
  float left = 0.f;
  int li = 0;
  for (int k = 0; k < a.Pf; ++k) {
    const float s = sf[k];
    while (p <= a.Sc && sc[p] <= s) {
      if (p < a.Sc) { cum += (double)wc[p]; Wlast = (float)cum; if (p == cap) Wcap = Wlast; }
      ++p;
    }
    const int idx = p - 1;                           // inds - 1 of this fence post
    if (k > 0) {
      const int ri = idx > cap ? cap : max(idx, 0);
      const float right = idx > cap ? Wcap : (idx <= 0 ? W0 : Wlast);
      const float w = wf[k - 1];
      const float over = w - (right - left);
      if (over > 0.f) {
        l_prop += over * over / (w + 1e-8f);
        const float gb = -2.f * over / (w + 1e-8f) * scale;
        g[ri] += gb;
        g[li] -= gb;
      }
    }
    li = idx <= 0 ? 0 : min(idx, a.Sc - 1);          // (an index past the last interval raises in the reference)
    left = idx <= 0 ? W0 : Wlast;
  }
  l_prop *= scale;
  // d/dw_c[j] = sum_{k >= j} dW[k]
  double acc = 0.0;
  for (int j = a.Sc - 1; j >= 0; --j) { acc += (double)g[j]; g[j] = (float)acc; }
  return l_prop;
}

// the depth term of ray r, which has a LiDAR target t != 0 and is one of the out[0] counted rays.  -> the term; *g1 / *g0 = d term /
// d (dist1[r], dist0[r]).
__device__ __forceinline__ float loss_tail_depth(const LossTail& a, long r, float t, float* g1, float* g0, float* gc = nullptr) {
  const float nv = a.out[0];
  const float cw = (a.conf != nullptr ? a.conf[r] : 1.f);
  const float d1 = a.dist1[r], d0 = a.dist0[r];
  float e1, e0, s1, s0;
  if (a.disparity) { e1 = 1.f / d1 - 1.f / t; e0 = 1.f / d0 - 1.f / t; s1 = -1.f / (d1 * d1); s0 = -1.f / (d0 * d0); }
  else { e1 = d1 - t; e0 = d0 - t; s1 = 1.f; s0 = 1.f; }
  const float k = cw * a.depth_lambda / nv;
  *g1 = (e1 > 0.f ? 1.f : (e1 < 0.f ? -1.f : 0.f)) * s1 * k;
  *g0 = (e0 > 0.f ? 1.f : (e0 < 0.f ? -1.f : 0.f)) * s0 * k * a.coarse_mult;
  if (gc != nullptr) *gc = (fabsf(e1) + a.coarse_mult * fabsf(e0)) * (a.depth_lambda / nv);      // d term / d conf[r]
  return (fabsf(e1) + a.coarse_mult * fabsf(e0)) * k;
}

struct LossTailMasked {
  LossTail t;
  const float* sem; const void* labels; int labels_f32, C;
  const long *rows, *img_i;
  const int *rgb_row_limit, *depth_row_limit, *sem_valid;
  int n_images;
  const float* depth_keep;
  float sem_lambda;
  float* g_sem;
};

// label of ray r, or -1 for a ray the semantic mean leaves out (ignore_index -100, and any other value outside [0, C))
__device__ __forceinline__ int loss_tail_label(const LossTailMasked& a, long r) {
  int l;
  if (a.labels_f32) {
    const float f = ((const float*)a.labels)[r];
    l = (f >= 0.f && f < 32.f) ? (int)f : -1;          // (NaN fails both comparisons)
    if ((float)l != f) l = -1;
  } else {
    l = ((const int*)a.labels)[r];
  }
  return (l >= 0 && l < a.C) ? l : -1;
}

// which means ray r enters: bit 0 = rgb (and semantic) mask Wr, bit 1 = depth mask Br
__device__ __forceinline__ int loss_tail_masks(const LossTailMasked& a, long r) {
  int W = 1, B = 1;
  if (a.rows != nullptr) {
    const long i = a.img_i[0];
    if (i < 0 || i >= a.n_images) return 0;
    const long row = a.rows[2 * r];
    W = row < a.rgb_row_limit[i];
    B = row < a.depth_row_limit[i];
  }
  if (a.depth_keep != nullptr) B = B && a.depth_keep[r] == 0.f;
  return W | B << 1;
}

__device__ __forceinline__ bool loss_tail_sem_active(const LossTailMasked& a) {
  if (a.sem == nullptr) return false;
  if (a.rows == nullptr) return true;
  const long i = a.img_i[0];
  return i >= 0 && i < a.n_images && a.sem_valid[i] != 0;
}

__global__ __launch_bounds__(1024) void loss_prepare_masked_kernel(LossTailMasked a) {
  __shared__ int part[3][16];
  int cnt[3] = {0, 0, 0};                              // depth, rgb, semantic
  const bool sem_on = loss_tail_sem_active(a);
  for (long r = threadIdx.x; r < a.t.N; r += 1024) {
    const int m = loss_tail_masks(a, r);
    if (a.t.tdepth != nullptr) cnt[0] += a.t.tdepth[r] != 0.f && (m & 2);
    cnt[1] += m & 1;
    if (sem_on) cnt[2] += (m & 1) && loss_tail_label(a, r) >= 0;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt[k] += __shfl_xor(cnt[k], o, 64);
    if ((threadIdx.x & 63) == 0) part[k][threadIdx.x >> 6] = cnt[k];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    int t = 0;
    for (int w = 0; w < 16; ++w) t += part[threadIdx.x][w];
    a.t.out[threadIdx.x == 0 ? 0 : 5 + threadIdx.x] = (float)t;
  }
  if (threadIdx.x >= 3 && threadIdx.x < 8) a.t.out[threadIdx.x - 2] = 0.f;      // out[1..5]
}

// GCONF: also write g_conf[r] = d total / d conf[r] (the learned confidence, confidence.hip); the other outputs keep their bits (this
// unit is built without fp contraction, so the extra statement cannot fuse into theirs)
template <bool GCONF>
__global__ __launch_bounds__(64) void loss_tail_masked_kernel(LossTailMasked a, float* __restrict__ g_conf) {
  const LossTail& t = a.t;
  const long r = (long)blockIdx.x * 64 + threadIdx.x;
  float l_rgb = 0.f, l_dep = 0.f, l_prop = 0.f;
  double l_sem = 0.0;
  if (r < t.N) {
    const int m = loss_tail_masks(a, r);
    // ---- RGB: mean over the #W * 3 values of the rays inside the mask
    const float nW = t.out[6];
    const float inv = nW > 0.f ? 1.f / (3.f * nW) : 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float d = t.rgb[3 * r + c] - t.tgt[3 * r + c];
      if (m & 1) l_rgb += d * d;
      t.g_rgb[3 * r + c] = (m & 1) ? d * (2.f * inv) : 0.f;
    }
    l_rgb *= inv;
    // ---- depth: mean over the rays with a LiDAR target inside the depth mask
    if (t.tdepth != nullptr) {
      const float td = t.tdepth[r];
      float g1 = 0.f, g0 = 0.f, gc = 0.f;
      if (td != 0.f && (m & 2)) l_dep = loss_tail_depth(t, r, td, &g1, &g0, GCONF ? &gc : nullptr);
      t.g_dist1[r] = g1;
      t.g_dist0[r] = g0;
      if (GCONF) g_conf[r] = gc;
    }
    // ---- proposal: every ray
    if (t.s_c != nullptr) l_prop = loss_tail_proposal(t, r);
    // ---- semantic: cross-entropy of the composited logits
    if (a.sem != nullptr) {
      const float* x = a.sem + r * a.C;
      float* g = a.g_sem + r * a.C;
      const int lab = (loss_tail_sem_active(a) && (m & 1)) ? loss_tail_label(a, r) : -1;
      if (lab < 0) {
        for (int c = 0; c < a.C; ++c) g[c] = 0.f;
      } else {
        float mx = x[0];
        for (int c = 1; c < a.C; ++c) mx = fmaxf(mx, x[c]);
        double se = 0.0;
        for (int c = 0; c < a.C; ++c) se += exp((double)x[c] - (double)mx);
        const double lse = log(se);
        const double k = (double)a.sem_lambda / (double)t.out[7];      // (this ray is counted: out[7] >= 1)
        l_sem = (lse - ((double)x[lab] - (double)mx)) * k;
        for (int c = 0; c < a.C; ++c) {
          const double p = exp(((double)x[c] - (double)mx) - lse);
          g[c] = (float)((p - (c == lab ? 1.0 : 0.0)) * k);
        }
      }
    }
  }
  l_rgb = wave_sum(l_rgb); l_dep = wave_sum(l_dep); l_prop = wave_sum(l_prop);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) l_sem += __shfl_xor(l_sem, o, 64);
  if (threadIdx.x == 0) {
    const float ls = (float)l_sem;
    atomicAdd(t.out + 1, l_rgb);
    if (t.tdepth != nullptr) atomicAdd(t.out + 2, l_dep);
    if (t.s_c != nullptr) atomicAdd(t.out + 3, l_prop);
    if (a.sem != nullptr) atomicAdd(t.out + 5, ls);
    atomicAdd(t.out + 4, ((l_rgb + l_dep) + l_prop) + ls);
  }
}

// snerf_mip_loss_tail_masked that also returns g_conf [N] (nullable) = d total / d conf[r] = (|e1| + coarse_mult |e0|) depth_lambda / #depth
// on the rays the depth mean counts and 0 elsewhere, for the learned confidence (confidence.hip)
extern "C" int snerf_mip_loss_tail_gconf(const float* rgb, const float* tgt, const float* dist1, const float* dist0, const float* tdepth,
                                         const float* conf, const float* s_f, const float* w_f, const float* s_c, const float* w_c,
                                         const float* sem, const void* labels, int labels_f32, int C, const long* rows, const long* img_i,
                                         const int* rgb_row_limit, const int* depth_row_limit, const int* sem_valid, int n_images,
                                         const float* depth_keep, long N, int Pf, int Sc, int disparity, float depth_lambda, float coarse_mult,
                                         float prop_lambda, float semantic_lambda, float* out, float* g_rgb, float* g_dist1, float* g_dist0,
                                         float* g_wc, float* g_sem, float* g_conf, void* stream) {
  if (N <= 0) return SNERF_OK;
  if (rgb == nullptr || tgt == nullptr || out == nullptr || g_rgb == nullptr) return SNERF_ERR_ARG;
  if (tdepth != nullptr && (dist1 == nullptr || dist0 == nullptr || g_dist1 == nullptr || g_dist0 == nullptr)) return SNERF_ERR_ARG;
  if (s_c != nullptr && (s_f == nullptr || w_f == nullptr || w_c == nullptr || g_wc == nullptr || Pf < 2 || Sc < 1)) return SNERF_ERR_ARG;
  const int n_sem = (sem != nullptr) + (labels != nullptr) + (g_sem != nullptr);
  if (n_sem != 0 && n_sem != 3) return SNERF_ERR_ARG;
  if (sem != nullptr && (C < 1 || C > 32 || (labels_f32 != 0 && labels_f32 != 1))) return SNERF_ERR_ARG;
  const int n_rule = (rows != nullptr) + (img_i != nullptr) + (rgb_row_limit != nullptr) + (depth_row_limit != nullptr) + (sem_valid != nullptr);
  if (n_rule != 0 && n_rule != 5) return SNERF_ERR_ARG;
  if (rows != nullptr && n_images < 1) return SNERF_ERR_ARG;
  if (depth_keep != nullptr && tdepth == nullptr) return SNERF_ERR_ARG;
  if (g_conf != nullptr && tdepth == nullptr) return SNERF_ERR_ARG;      // (g_conf is a by-product of the depth term)
  LossTailMasked a{{rgb, tgt, dist1, dist0, tdepth, conf, s_f, w_f, s_c, w_c, N, Pf, Sc, disparity, depth_lambda, coarse_mult, prop_lambda, out,
                    g_rgb, g_dist1, g_dist0, g_wc},
                   sem, labels, labels_f32, C, rows, img_i, rgb_row_limit, depth_row_limit, sem_valid, n_images, depth_keep, semantic_lambda, g_sem};
  hipLaunchKernelGGL(loss_prepare_masked_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
  const dim3 grid((unsigned)((N + 63) / 64));
  if (g_conf != nullptr) hipLaunchKernelGGL(loss_tail_masked_kernel<true>, grid, dim3(64), 0, (hipStream_t)stream, a, g_conf);
  else hipLaunchKernelGGL(loss_tail_masked_kernel<false>, grid, dim3(64), 0, (hipStream_t)stream, a, g_conf);
  return snerf_check_launch();
}

extern "C" int snerf_mip_loss_tail_masked(const float* rgb, const float* tgt, const float* dist1, const float* dist0, const float* tdepth,
                                          const float* conf, const float* s_f, const float* w_f, const float* s_c, const float* w_c,
                                          const float* sem, const void* labels, int labels_f32, int C, const long* rows, const long* img_i,
                                          const int* rgb_row_limit, const int* depth_row_limit, const int* sem_valid, int n_images,
                                          const float* depth_keep, long N, int Pf, int Sc, int disparity, float depth_lambda, float coarse_mult,
                                          float prop_lambda, float semantic_lambda, float* out, float* g_rgb, float* g_dist1, float* g_dist0,
                                          float* g_wc, float* g_sem, void* stream) {
  return snerf_mip_loss_tail_gconf(rgb, tgt, dist1, dist0, tdepth, conf, s_f, w_f, s_c, w_c, sem, labels, labels_f32, C, rows, img_i, rgb_row_limit,
                                   depth_row_limit, sem_valid, n_images, depth_keep, N, Pf, Sc, disparity, depth_lambda, coarse_mult, prop_lambda,
                                   semantic_lambda, out, g_rgb, g_dist1, g_dist0, g_wc, g_sem, nullptr, stream);
}

// ---------------------------------------------------------------------------
// Edge-aware smoothness of depth patches (--smooth_loss; s-nerf/train.py:154-177): SmoothLoss (model/loss_factory.py:39-57) over
// edge_aware_loss_v2 (model/loss.py:14-34), value and gradient w.r.t. the distances in one pass.  Per patch of p x p pixels:
//   disp = 1 / max(dist, 1e-5), u = disp / (mean(disp) + 1e-7),
//   x-edge (a = left, b = right neighbour): |u_a - u_b| exp(-mean_c |rgb_a - rgb_b|) (1 + sky_a); y-edges alike with a = top;
//   loss = weight (sum over x-edges / (P p (p - 1)) + the same for the y-edges).
// One workgroup per patch, one lane per pixel (p^2 lanes rounded up to whole waves; p = 8 is one wave).  Everything is float64: the
// fp32 inputs convert exactly and every output is rounded to fp32 once.  u goes through LDS to the neighbours; each lane owns the edge
// to its right and the edge below it and leaves their signed weights in LDS, from which every lane collects q = d (edge sums) / d u
// of its pixel.  With M = mean + 1e-7 and S = sum_i q_i disp_i:  d / d disp_j = q_j / M - S / (M^2 p^2), times -1 / dist^2 where
// dist >= 1e-5 (torch's clamp passes no gradient below its bound; such a pixel still enters the mean), sign(0) = 0.  The gradient of a
// patch needs only that patch, so it leaves in this launch; the patch's two edge sums go to ws and a one-wave finish launch adds them
// in a fixed order: no floating-point atomics, two calls give the same bits.
// ---------------------------------------------------------------------------
struct SmoothArgs {
  const float *rgb, *dist, *sky;    // [P,p,p,3], [P,p,p], [P,p,p] nullable
  long P; int p;
  double weight;
  double* ws;                       // [P,2] = each patch's {x-edge sum, y-edge sum}
  float *out, *total, *g_dist;
  int accumulate;
};

// sum over the workgroup, the same bits in every lane: xor butterfly inside the waves, then the waves' values in wave order
__device__ __forceinline__ double smooth_block_sum(double v, double* s_part) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();                                   // (the previous sum's readers are done with s_part)
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += s_part[w];
  return s;
}

__global__ __launch_bounds__(1024) void smooth_loss_kernel(SmoothArgs a) {
  __shared__ double s_u[1024], s_gx[1024], s_gy[1024], s_part[16];
  const int p = a.p, pp = p * p, t = (int)threadIdx.x;
  const bool live = t < pp;
  const long base = (long)blockIdx.x * pp;
  const int y = t / p, x = t - y * p;
  const float df = live ? a.dist[base + t] : 1.f;
  const bool clamped = df < 1e-5f;                   // (a NaN distance is not clamped, as in torch)
  const double d = clamped ? (double)1e-5f : (double)df;
  const double disp = live ? 1.0 / d : 0.0;
  const double M = smooth_block_sum(disp, s_part) / (double)pp + 1e-7;
  const double u = disp / M;
  s_u[t] = u;
  __syncthreads();
  double ex = 0.0, ey = 0.0, gx = 0.0, gy = 0.0;     // this lane's two edges: value, and signed weight = d value / d u of this pixel
  if (live) {
    const float* c0 = a.rgb + 3 * (base + t);
    const double k = a.sky != nullptr ? 1.0 + (double)a.sky[base + t] : 1.0;
    if (x + 1 < p) {
      const float* c1 = c0 + 3;
      const double w = exp(-((fabs((double)c0[0] - (double)c1[0]) + fabs((double)c0[1] - (double)c1[1])) + fabs((double)c0[2] - (double)c1[2])) / 3.0) * k;
      const double du = u - s_u[t + 1];
      ex = fabs(du) * w;
      gx = du > 0.0 ? w : (du < 0.0 ? -w : 0.0);
    }
    if (y + 1 < p) {
      const float* c1 = c0 + 3 * p;
      const double w = exp(-((fabs((double)c0[0] - (double)c1[0]) + fabs((double)c0[1] - (double)c1[1])) + fabs((double)c0[2] - (double)c1[2])) / 3.0) * k;
      const double du = u - s_u[t + p];
      ey = fabs(du) * w;
      gy = du > 0.0 ? w : (du < 0.0 ? -w : 0.0);
    }
  }
  s_gx[t] = gx;
  s_gy[t] = gy;
  __syncthreads();
  double q = 0.0;
  if (live) {
    q = gx + gy;
    if (x > 0) q -= s_gx[t - 1];
    if (y > 0) q -= s_gy[t - p];
  }
  const double S = smooth_block_sum(q * disp, s_part);
  const double sx = smooth_block_sum(ex, s_part), sy = smooth_block_sum(ey, s_part);
  if (t == 0) { a.ws[2 * blockIdx.x] = sx; a.ws[2 * blockIdx.x + 1] = sy; }
  if (live) {
    const double scale = a.weight / ((double)a.P * p * (p - 1));
    const double g_disp = (q / M - S / (M * M * (double)pp)) * scale;
    const float g = clamped ? 0.f : (float)(g_disp * (-1.0 / (d * d)));
    a.g_dist[base + t] = a.accumulate ? a.g_dist[base + t] + g : g;
  }
}

__global__ __launch_bounds__(64) void smooth_loss_finish_kernel(SmoothArgs a) {
  double sx = 0.0, sy = 0.0;
  for (long k = threadIdx.x; k < a.P; k += 64) { sx += a.ws[2 * k]; sy += a.ws[2 * k + 1]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { sx += __shfl_xor(sx, o, 64); sy += __shfl_xor(sy, o, 64); }
  if (threadIdx.x == 0) {
    const double edges = (double)a.P * a.p * (a.p - 1);
    const float loss = (float)(a.weight * (sx / edges + sy / edges));
    a.out[0] = loss;
    a.out[1] = (float)(sx / edges);
    a.out[2] = (float)(sy / edges);
    if (a.total != nullptr) *a.total = *a.total + loss;
  }
}

extern "C" long snerf_smooth_loss_ws(long P) { return P <= 0 ? 0 : 2 * P; }

extern "C" int snerf_smooth_loss(const float* rgb, const float* dist, const float* sky, long P, int p, float weight, double* ws, long ws_doubles,
                                 float* out, float* total, float* g_dist, int accumulate, void* stream) {
  if (P == 0) return SNERF_OK;
  if (P < 0 || P > 0x7FFFFFFFL || p < 2 || p > 32 || (accumulate != 0 && accumulate != 1)) return SNERF_ERR_ARG;
  if (rgb == nullptr || dist == nullptr || out == nullptr || g_dist == nullptr || ws == nullptr || ws_doubles < 2 * P) return SNERF_ERR_ARG;
  SmoothArgs a{rgb, dist, sky, P, p, (double)weight, ws, out, total, g_dist, accumulate};
  hipLaunchKernelGGL(smooth_loss_kernel, dim3((unsigned)P), dim3((unsigned)((p * p + 63) / 64 * 64)), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(smooth_loss_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
  return snerf_check_launch();
}

// ---------------------------------------------------------------------------
// The patch terms of the zipnerf loop (s-nerfpp/zipnerf/train.py:280-293): d_smo = edge_aware_loss_v2 on the rendered disparity,
// s_smo = edge_aware_loss_for_semantic on the rendered class probabilities (internal/train_utils.py:297-315, 337-359, both in their
// `mask is not None` branch), values and gradients in one pass.  Per patch of p x p pixels (layout [dy][dx]), valid = !(mask > 0):
//   disp = 1 / (depth + 1e-5), u = disp / (mean(disp) + 1e-7);  v_c = sem_c / (mean(sem_c) + 1e-5)  (means over all p^2 pixels);
//   w(a, b) = exp(-mean_c |rgb_a - rgb_b|);  x-edge (a, b = right neighbour), y-edge (a, b = lower neighbour), counted when both
//   pixels are valid:  depth |u_a - u_b| w,  semantic (sum_c |v_c,a - v_c,b|) w;
//   term = mult (sum of the valid x-edge values / Nx + the same for y / Ny), Nx / Ny = the valid edges of ALL patches.
// Nx and Ny scale every gradient, so they are counted first: zip_smooth_count_kernel (one workgroup per patch, wave ballots, one
// integer atomic per wave into the two counters at the head of ws, zeroed by a memset node ahead of it).  Then one workgroup per
// patch, one lane per pixel, float64 throughout (the fp32 inputs convert exactly, every output is rounded once): u goes through LDS
// to the neighbours, each lane owns the edge to its right and the edge below it and leaves their signed, 1/N-scaled weights in LDS,
// from which every lane collects q = d (sum_x / Nx + sum_y / Ny) / d u of its pixel.  With M = mean + eps and S = sum_i q_i disp_i:
// d / d disp_j = q_j / M - S / (M^2 p^2) (a masked pixel has q = 0 and keeps the second part), times -1 / (depth + 1e-5)^2 for the
// depth; sign(0) = 0.  The classes of the semantic term run one after the other through the same LDS arrays.  The patch's four edge
// sums go to ws and a one-wave finish launch adds them in a fixed order: no floating-point atomics, two calls give the same bits.
// Nx = 0 or Ny = 0: both terms and every gradient are exactly 0 (torch.nan_to_num of the empty mean, whose gradient is 0).
// ---------------------------------------------------------------------------
struct ZipSmoothArgs {
  const float *rgb, *depth, *sem, *mask;   // [P,p,p,3], [P,p,p], [P,p,p,ld] nullable, [P,p,p] nullable
  long ld; int C;
  long P; int p;
  double d_mult, s_mult, grad_mult;
  unsigned long long* cnt;                 // ws[0..1] as integers: {Nx, Ny}
  double* sums;                            // ws + 2: [P,4] = each patch's {depth x, depth y, semantic x, semantic y} edge sums
  float *out, *total, *g_depth, *g_sem;
  int accumulate;
};

__device__ __forceinline__ bool zip_smooth_valid(const ZipSmoothArgs& a, long i) { return a.mask == nullptr || !(a.mask[i] > 0.f); }

__global__ __launch_bounds__(1024) void zip_smooth_count_kernel(ZipSmoothArgs a) {
  const int p = a.p, pp = p * p, t = (int)threadIdx.x;
  const long base = (long)blockIdx.x * pp;
  bool ex = false, ey = false;
  if (t < pp && zip_smooth_valid(a, base + t)) {
    const int y = t / p, x = t - y * p;
    ex = x + 1 < p && zip_smooth_valid(a, base + t + 1);
    ey = y + 1 < p && zip_smooth_valid(a, base + t + p);
  }
  const unsigned long long bx = __ballot(ex), by = __ballot(ey);
  if ((t & 63) == 0) {
    if (bx != 0ull) atomicAdd(a.cnt, (unsigned long long)__popcll(bx));
    if (by != 0ull) atomicAdd(a.cnt + 1, (unsigned long long)__popcll(by));
  }
}

// one normalised channel of a patch (disparity, or one class): z = the lane's value, ex / ey = its edges' 1/N-scaled exp weights (0
// where the edge is missing or masked).  -> d (sum_x / Nx + sum_y / Ny) / d z of this pixel; the edges' |du| w / N are added to vx, vy
__device__ __forceinline__ double zip_smooth_channel(double z, double eps, bool live, int t, int x, int y, int p, double ex, double ey,
                                                     double* s_u, double* s_gx, double* s_gy, double* s_part, double& vx, double& vy) {
  const int pp = p * p;
  const double M = smooth_block_sum(z, s_part) / (double)pp + eps;
  const double u = z / M;
  s_u[t] = u;
  __syncthreads();
  double gx = 0.0, gy = 0.0;
  if (live && x + 1 < p) {
    const double du = u - s_u[t + 1];
    vx += fabs(du) * ex;
    gx = du > 0.0 ? ex : (du < 0.0 ? -ex : 0.0);
  }
  if (live && y + 1 < p) {
    const double du = u - s_u[t + p];
    vy += fabs(du) * ey;
    gy = du > 0.0 ? ey : (du < 0.0 ? -ey : 0.0);
  }
  s_gx[t] = gx;
  s_gy[t] = gy;
  __syncthreads();
  double q = 0.0;
  if (live) {
    q = gx + gy;
    if (x > 0) q -= s_gx[t - 1];
    if (y > 0) q -= s_gy[t - p];
  }
  const double S = smooth_block_sum(q * z, s_part);
  return q / M - S / (M * M * (double)pp);
}

__global__ __launch_bounds__(1024) void zip_smooth_loss_kernel(ZipSmoothArgs a) {
  __shared__ double s_u[1024], s_gx[1024], s_gy[1024], s_part[16];
  const int p = a.p, pp = p * p, t = (int)threadIdx.x;
  const bool live = t < pp;
  const long base = (long)blockIdx.x * pp;
  const int y = t / p, x = t - y * p;
  const long full = a.P * p * (p - 1);
  const long Nx = a.mask != nullptr ? (long)a.cnt[0] : full, Ny = a.mask != nullptr ? (long)a.cnt[1] : full;
  if (Nx == 0 || Ny == 0) {                           // the same in every lane of every workgroup
    if (live && !a.accumulate) {
      a.g_depth[base + t] = 0.f;
      if (a.sem != nullptr)
        for (int c = 0; c < a.C; ++c) a.g_sem[(base + t) * a.ld + c] = 0.f;
    }
    if (t < 4) a.sums[4 * blockIdx.x + t] = 0.0;
    return;
  }
  double ex = 0.0, ey = 0.0;                          // exp weight / N of the lane's two edges, 0 where there is none
  if (live && zip_smooth_valid(a, base + t)) {
    const float* c0 = a.rgb + 3 * (base + t);
    if (x + 1 < p && zip_smooth_valid(a, base + t + 1)) {
      const float* c1 = c0 + 3;
      ex = exp(-((fabs((double)c0[0] - (double)c1[0]) + fabs((double)c0[1] - (double)c1[1])) + fabs((double)c0[2] - (double)c1[2])) / 3.0) / (double)Nx;
    }
    if (y + 1 < p && zip_smooth_valid(a, base + t + p)) {
      const float* c1 = c0 + 3 * p;
      ey = exp(-((fabs((double)c0[0] - (double)c1[0]) + fabs((double)c0[1] - (double)c1[1])) + fabs((double)c0[2] - (double)c1[2])) / 3.0) / (double)Ny;
    }
  }
  double dx = 0.0, dy = 0.0, sx = 0.0, sy = 0.0;
  {
    const double dd = live ? (double)a.depth[base + t] + 1e-5 : 1.0;
    const double disp = live ? 1.0 / dd : 0.0;
    const double g_disp = zip_smooth_channel(disp, 1e-7, live, t, x, y, p, ex, ey, s_u, s_gx, s_gy, s_part, dx, dy);
    if (live) {
      const float g = (float)(g_disp * (-1.0 / (dd * dd)) * (a.d_mult * a.grad_mult));
      a.g_depth[base + t] = a.accumulate ? a.g_depth[base + t] + g : g;
    }
  }
  if (a.sem != nullptr) {
    for (int c = 0; c < a.C; ++c) {
      const long i = (base + t) * a.ld + c;
      const double z = live ? (double)a.sem[i] : 0.0;
      const double g_z = zip_smooth_channel(z, 1e-5, live, t, x, y, p, ex, ey, s_u, s_gx, s_gy, s_part, sx, sy);
      if (live) {
        const float g = (float)(g_z * (a.s_mult * a.grad_mult));
        a.g_sem[i] = a.accumulate ? a.g_sem[i] + g : g;
      }
    }
  }
  dx = smooth_block_sum(dx, s_part); dy = smooth_block_sum(dy, s_part);
  sx = smooth_block_sum(sx, s_part); sy = smooth_block_sum(sy, s_part);
  if (t == 0) {
    double* o = a.sums + 4 * blockIdx.x;
    o[0] = dx; o[1] = dy; o[2] = sx; o[3] = sy;
  }
}

__global__ __launch_bounds__(64) void zip_smooth_finish_kernel(ZipSmoothArgs a) {
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (long k = threadIdx.x; k < a.P; k += 64) {
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] += a.sums[4 * k + j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    for (int o = 32; o > 0; o >>= 1) s[j] += __shfl_xor(s[j], o, 64);
  if (threadIdx.x == 0) {
    const long full = a.P * a.p * (a.p - 1);
    const long Nx = a.mask != nullptr ? (long)a.cnt[0] : full, Ny = a.mask != nullptr ? (long)a.cnt[1] : full;
    const float d_smo = (float)(a.d_mult * (s[0] + s[1])), s_smo = (float)(a.s_mult * (s[2] + s[3]));    // (the 1 / N are in the sums)
    a.out[0] = d_smo;
    a.out[1] = s_smo;
    a.out[2] = (float)Nx;
    a.out[3] = (float)Ny;
    if (a.total != nullptr) *a.total = (*a.total + d_smo) + s_smo;
  }
}

extern "C" long snerf_zip_smooth_loss_ws(long P) { return P <= 0 ? 0 : 2 + 4 * P; }

extern "C" int snerf_zip_smooth_loss(const float* rgb, const float* depth, const float* sem, long ld_sem, int C, const float* mask, long P, int p,
                                     float d_mult, float s_mult, float grad_mult, double* ws, long ws_doubles, float* out, float* total,
                                     float* g_depth, float* g_sem, int accumulate, void* stream) {
  if (P == 0) return SNERF_OK;
  if (P < 0 || P > 0x7FFFFFFFL || p < 2 || p > 32 || (accumulate != 0 && accumulate != 1)) return SNERF_ERR_ARG;
  if (rgb == nullptr || depth == nullptr || out == nullptr || g_depth == nullptr || ws == nullptr || ws_doubles < 2 + 4 * P) return SNERF_ERR_ARG;
  if (sem != nullptr && (C < 1 || C > 32 || ld_sem < C || g_sem == nullptr)) return SNERF_ERR_ARG;
  ZipSmoothArgs a{rgb, depth, sem, mask, ld_sem, C, P, p, (double)d_mult, (double)s_mult, (double)grad_mult, (unsigned long long*)ws, ws + 2,
                  out, total, g_depth, g_sem, accumulate};
  const dim3 grid((unsigned)P), block((unsigned)((p * p + 63) / 64 * 64));
  if (mask != nullptr) {
    if (hipMemsetAsync(ws, 0, 2 * sizeof(double), (hipStream_t)stream) != hipSuccess) return snerf_check_launch();   // (no count on stale counters)
    hipLaunchKernelGGL(zip_smooth_count_kernel, grid, block, 0, (hipStream_t)stream, a);
  }
  hipLaunchKernelGGL(zip_smooth_loss_kernel, grid, block, 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(zip_smooth_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
  return snerf_check_launch();
}

// ---------------------------------------------------------------------------
// zipnerf (path C) ray generation: s-nerfpp/zipnerf/internal/camera_utils.py:453-563 (pixels_to_rays), perspective camera, no
// distortion, no NDC.  numpy promotes to float64 there (integer pixels + .5); the dataset casts the result to fp32.  One lane
// per ray, float64 arithmetic, one rounding per emitted value.
// ---------------------------------------------------------------------------
struct ZipRayGen {
  const int *pix_x, *pix_y, *cam_idx;
  const float *pixtocams, *camtoworlds;          // [ncam,3,3], [ncam,3,4]
  long N;
  int ncam;
  float *origins, *directions, *viewdirs, *radii, *imageplane, *base_x, *base_y;
};

__device__ __forceinline__ void zip_cast(const double* k, const double* p, double x, double y, double* cam, double* d) {
  const double px = x + .5, py = y + .5;
#pragma unroll
  for (int c = 0; c < 3; ++c) cam[c] = (k[3 * c] * px + k[3 * c + 1] * py) + k[3 * c + 2];
  cam[1] = -cam[1]; cam[2] = -cam[2];                 // OpenCV -> OpenGL (:527)
#pragma unroll
  for (int c = 0; c < 3; ++c) d[c] = (p[4 * c] * cam[0] + p[4 * c + 1] * cam[1]) + p[4 * c + 2] * cam[2];
}

// the ray of pixel (x, y) of camera (K = pixtocam [3,3], P = camtoworld [3,4]), stored at row r of the outputs (imageplane nullable).
// Shared by the pixel list launch below and the training batcher (snerf_zip_ray_batch), which must agree with it bit for bit.
__device__ __forceinline__ void zip_ray(const float* K, const float* P, int xi, int yi, long r, float* origins, float* directions, float* viewdirs,
                                        float* radii, float* imageplane, float* base_x, float* base_y) {
  double k[9], p[12];
#pragma unroll
  for (int i = 0; i < 9; ++i) k[i] = (double)K[i];
#pragma unroll
  for (int i = 0; i < 12; ++i) p[i] = (double)P[i];
  const double x = (double)xi, y = (double)yi;
  double c0[3], cx[3], cy[3], d[3], dx[3], dy[3];
  zip_cast(k, p, x, y, c0, d);
  zip_cast(k, p, x + 1.0, y, cx, dx);
  zip_cast(k, p, x, y + 1.0, cy, dy);
  double nd = 0, nx = 0, ny = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) { dx[c] -= d[c]; dy[c] -= d[c]; nd += d[c] * d[c]; nx += dx[c] * dx[c]; ny += dy[c] * dy[c]; }
  nd = sqrt(nd); nx = sqrt(nx); ny = sqrt(ny);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    origins[3 * r + c] = (float)p[4 * c + 3];
    directions[3 * r + c] = (float)d[c];
    viewdirs[3 * r + c] = (float)(d[c] / nd);
    base_x[3 * r + c] = (float)(dx[c] / nx);
    base_y[3 * r + c] = (float)(dy[c] / ny);
  }
  radii[r] = (float)((0.5 * (nx + ny)) * 2.0 / 3.4641016151377544);
  if (imageplane != nullptr) { imageplane[2 * r] = (float)c0[0]; imageplane[2 * r + 1] = (float)c0[1]; }
}

__global__ __launch_bounds__(256) void zip_rays_kernel(ZipRayGen a) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.N) return;
  int cam = a.cam_idx != nullptr ? a.cam_idx[r] : 0;
  cam = min(max(cam, 0), a.ncam - 1);
  zip_ray(a.pixtocams + 9 * cam, a.camtoworlds + 12 * cam, a.pix_x[r], a.pix_y[r], r, a.origins, a.directions, a.viewdirs, a.radii, a.imageplane,
          a.base_x, a.base_y);
}

extern "C" int snerf_zip_pixels_to_rays(const int* pix_x, const int* pix_y, const int* cam_idx, const float* pixtocams, const float* camtoworlds,
                                        int ncam, long N, float* origins, float* directions, float* viewdirs, float* radii, float* imageplane,
                                        float* base_x, float* base_y, void* stream) {
  if (N <= 0) return SNERF_OK;
  if (pix_x == nullptr || pix_y == nullptr || pixtocams == nullptr || camtoworlds == nullptr || ncam < 1 || origins == nullptr ||
      directions == nullptr || viewdirs == nullptr || radii == nullptr || base_x == nullptr || base_y == nullptr)
    return SNERF_ERR_ARG;
  ZipRayGen a{pix_x, pix_y, cam_idx, pixtocams, camtoworlds, N, ncam, origins, directions, viewdirs, radii, imageplane, base_x, base_y};
  hipLaunchKernelGGL(zip_rays_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return snerf_check_launch();
}

// ---------------------------------------------------------------------------
// Device-resident training batchers (the step before the render paths): the training set stays in HBM and one launch draws, casts
// and gathers a batch, with no host work and no sync.  Only the draw differs from the reference (numpy's RNG there); given the drawn
// pixels, rays and targets are those of pinhole_ray / zip_ray above, bit for bit.
//
// Generator: Philox4x32-10 (Salmon et al., SC'11; the Random123 constants), key (k0, k1) = (low, high 32 bits of the seed):
//   round: (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), M0 = 0xD2511F53, M1 = 0xCD9E8D57,
//   then (k0, k1) += (0x9E3779B9, 0xBB67AE85); ten rounds.  philox(c0, c1, c2, c3) below is the first output word.
// Keyed permutation perm(tag, t, M) of [0, M): a balanced Feistel network over b bits (b = the bit length of M - 1, rounded up to
// an even number, at least 2; h = b / 2), four rounds j = 0..3 on v = (L << h) | R:
//   F = philox(R, tag << 16 | j, lo32(t), hi32(t)) & (2^h - 1);  (L, R) <- (R, L ^ F)
// applied again to its own output ("cycle walking") until the value is below M: a bijection of [0, M) with O(1) expected passes.
//   snerf_mip_image_batch, step s over n_train training images:  image = i_train[perm(1, s / n_train, n_train)(s % n_train)] (each
//   training image once per epoch); ray i (global batch position) -> pixel q = perm(2, s, H W)(i), row = q / W, col = q % W:
//   n distinct pixels without a sort.
//   snerf_zip_ray_batch, step s, ray i, value v (0 = camera, 1 = x, 2 = y) drawn uniformly from [lo, lo + range): attempts
//   a = 0, 1, ...: u = philox(i, 3 << 16 | v << 8 | a, lo32(s), hi32(s)), m = u * range (64 bits); accepted when lo32(m) >=
//   2^32 mod range (Lemire's unbiased bounded integers); value = lo + hi32(m).  Attempt 255 is accepted as it is (a rejection has
//   probability range / 2^32).  batching 'single_image': every ray takes the camera of ray 0.
//   snerf_mip_image_patch_batch, step s, patch k: the same bounded draw with (i, v) = (k, 3) over the patch-centre window (below).
//   snerf_zip_ray_patch_batch, step s, patch k of p x p pixels: camera, x0, y0 = the same draw with (i, v) = (k p^2, 0 / 1 / 2).
// A ray's draws depend on (seed, step, i) only: not on the rank slice [i0, i1) a launch writes, nor on the launch geometry.
// Step counter ctr[2] (int64, device): ctr[0] = step.  Every workgroup reads it and takes a ticket (ctr[1]); the last one stores
// step + 1 and resets the ticket: a replayed graph launch draws a new batch every time.
// ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c0;
}

__device__ __forceinline__ unsigned long long keyed_perm(unsigned long long v, unsigned long long M, unsigned tag, long t, unsigned k0, unsigned k1) {
  int b = 64 - __clzll(M - 1);
  b = b < 2 ? 2 : b + (b & 1);
  const int h = b >> 1;
  const unsigned long long mask = (1ull << h) - 1;
  const unsigned t0 = (unsigned)(unsigned long long)t, t1 = (unsigned)((unsigned long long)t >> 32);
  do {
#pragma unroll
    for (unsigned j = 0; j < 4; ++j) {
      const unsigned long long L = v >> h, R = v & mask;
      const unsigned long long F = philox((unsigned)R, tag << 16 | j, t0, t1, k0, k1) & mask;
      v = (R << h) | (L ^ F);
    }
  } while (v >= M);
  return v;
}

__device__ __forceinline__ int bounded_draw(unsigned i, unsigned v, long s, unsigned range, unsigned k0, unsigned k1) {
  const unsigned thresh = (0u - range) % range;
  const unsigned s0 = (unsigned)(unsigned long long)s, s1 = (unsigned)((unsigned long long)s >> 32);
  unsigned long long m = 0;
  for (unsigned a = 0; a < 256; ++a) {
    m = (unsigned long long)philox(i, 3u << 16 | v << 8 | a, s0, s1, k0, k1) * range;
    if ((unsigned)m >= thresh) break;
  }
  return (int)(m >> 32);
}

// workgroup start: the step of this launch (LDS broadcast); the last workgroup to take a ticket advances the counter
__device__ __forceinline__ long batch_step(long* ctr) {
  __shared__ long s_step;
  if (threadIdx.x == 0) {
    const long s = __hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_step = s;
    __threadfence();
    const unsigned long long ticket = atomicAdd((unsigned long long*)(ctr + 1), 1ull);
    if (ticket == gridDim.x - 1) {
      __hip_atomic_store(ctr + 1, 0L, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(ctr, s + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __syncthreads();
  return s_step;
}

// uint8 storage decodes to float32(k / 255.0) computed in double (numpy's `image / 255.` before its cast to float32)
__device__ __forceinline__ float texel(const void* img, int u8, long idx) {
  return u8 ? (float)((double)((const unsigned char*)img)[idx] / 255.0) : ((const float*)img)[idx];
}

struct MipBatch {
  const void* images; int u8;                     // [N,H,W,3]
  const float *depths, *poses, *intr, *near, *far, *app, *extras;   // [N,H,W] / [N,3,4] / [N,4] = (cx, cy, fx, fy) / [N] x 3 / [k,N,H,W]
  int n_extra;
  const int* i_train; int n_train;
  int N, H, W;
  unsigned k0, k1;
  long* ctr;
  long n, i0, i1;
  float *origins, *directions, *viewdirs, *radii, *lossmult, *near_out, *far_out, *app_out, *rgb, *depth, *extras_out;
  long *sel_coords, *img_out;
  int patch_sz, pk0, pk1;                         // snerf_mip_image_patch_batch: patches [pk0, pk1) of patch_sz^2 pixels behind the pixel rows
};

// Patch rows (snerf_mip_image_patch_batch; sample_utils.py:68-89 sample_patches_pt): centre k of step s = bounded_draw(k, 3, s, hr wc)
// over the hr x wc = (H - 2p - 1)(W - 2p - 1) pixels strictly more than p = patch_sz from every border, row-major: WITH replacement,
// like np.random.randint; its p^2 pixels are [c - p/2, c + p/2) in both axes, rows outer.
__global__ __launch_bounds__(256) void mip_image_batch_kernel(MipBatch a) {
  const long s = batch_step(a.ctr);
  const long e = s / a.n_train, pos = s - e * a.n_train;
  const int img = a.i_train[keyed_perm((unsigned long long)pos, (unsigned long long)a.n_train, 1u, e, a.k0, a.k1)];
  if (blockIdx.x == 0 && threadIdx.x == 0) a.img_out[0] = img;
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  const long npix = a.i1 - a.i0, pp = (long)a.patch_sz * a.patch_sz, nl = npix + (long)(a.pk1 - a.pk0) * pp;
  if (r >= nl) return;
  const long HW = (long)a.H * a.W;
  int row, col;
  if (r < npix) {
    const long q = (long)keyed_perm((unsigned long long)(a.i0 + r), (unsigned long long)HW, 2u, s, a.k0, a.k1);
    row = (int)(q / a.W); col = (int)(q - (long)row * a.W);
  } else {
    const long j = r - npix, k = a.pk0 + j / pp;
    const int t = (int)(j - (k - a.pk0) * pp), p = a.patch_sz, wc = a.W - 2 * p - 1;
    const unsigned idx = (unsigned)bounded_draw((unsigned)k, 3u, s, (unsigned)(a.H - 2 * p - 1) * (unsigned)wc, a.k0, a.k1);
    row = p + 1 + (int)(idx / (unsigned)wc) - p / 2 + t / p;
    col = p + 1 + (int)(idx % (unsigned)wc) - p / 2 + t % p;
  }
  const long q = (long)row * a.W + col;
  const float* p = a.poses + 12 * (long)img;
  const float* k = a.intr + 4 * (long)img;
  float d[3], v[3], rad;
  pinhole_ray(p, k[0], k[1], k[2], k[3], a.H, row, col, 1, d, v, &rad);
  const long pix = (long)img * HW + q;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    a.origins[3 * r + c] = p[4 * c + 3];
    a.directions[3 * r + c] = d[c];
    a.viewdirs[3 * r + c] = v[c];
    a.rgb[3 * r + c] = texel(a.images, a.u8, 3 * pix + c);
  }
  a.radii[r] = rad;
  a.lossmult[r] = 1.f;
  a.near_out[r] = a.near[img];
  a.far_out[r] = a.far[img];
  a.app_out[r] = a.app[img];
  if (a.depth != nullptr) a.depth[r] = a.depths[pix];
  for (int x = 0; x < a.n_extra; ++x) a.extras_out[x * nl + r] = a.extras[(long)x * a.N * HW + pix];
  a.sel_coords[2 * r] = row;
  a.sel_coords[2 * r + 1] = col;
}

// checks shared by the two path A entries; n == 0 is handled by the callers
static int mip_batch_bad(const void* images, int images_u8, const float* depths, const float* poses, const float* intrinsics, const float* near,
                         const float* far, const float* app, const float* extras, int n_extra, const int* i_train, int n_train, int N, int H,
                         int W, const long* counter, long n, long i0, long i1, const float* origins, const float* directions,
                         const float* viewdirs, const float* radii, const float* lossmult, const float* near_out, const float* far_out,
                         const float* app_out, const float* rgb, const float* depth, const float* extras_out, const long* sel_coords,
                         const long* img_out) {
  if (n < 0 || N < 1 || n_train < 1 || H < 3 || W < 1 || n > (long)H * W || i0 < 0 || i1 < i0 || i1 > n || n_extra < 0) return 1;
  if (images == nullptr || poses == nullptr || intrinsics == nullptr || near == nullptr || far == nullptr || app == nullptr ||
      i_train == nullptr || counter == nullptr || img_out == nullptr || (images_u8 != 0 && images_u8 != 1))
    return 1;
  if (origins == nullptr || directions == nullptr || viewdirs == nullptr || radii == nullptr || lossmult == nullptr || near_out == nullptr ||
      far_out == nullptr || app_out == nullptr || rgb == nullptr || sel_coords == nullptr)
    return 1;
  if ((depth != nullptr && depths == nullptr) || (n_extra > 0 && (extras == nullptr || extras_out == nullptr))) return 1;
  return 0;
}

extern "C" int snerf_mip_image_patch_batch(const void* images, int images_u8, const float* depths, const float* poses, const float* intrinsics,
                                           const float* near, const float* far, const float* app, const float* extras, int n_extra,
                                           const int* i_train, int n_train, int N, int H, int W, long seed, long* counter, long n, long i0,
                                           long i1, float* origins, float* directions, float* viewdirs, float* radii, float* lossmult,
                                           float* near_out, float* far_out, float* app_out, float* rgb, float* depth, float* extras_out,
                                           long* sel_coords, long* img_out, int n_patch, int patch_sz, int k0, int k1, void* stream) {
  if (n_patch < 0 || k0 < 0 || k1 < k0 || k1 > n_patch) return SNERF_ERR_ARG;
  if (n_patch == 0) {
    if (n == 0) return SNERF_OK;
    patch_sz = 0;
  } else {
    if (patch_sz < 2 || patch_sz > 32 || (patch_sz & 1) != 0) return SNERF_ERR_ARG;
    const long hr = (long)H - 2L * patch_sz - 1, wc = (long)W - 2L * patch_sz - 1;
    if (hr < 1 || wc < 1 || hr * wc > 0xFFFFFFFFL) return SNERF_ERR_ARG;
  }
  if (mip_batch_bad(images, images_u8, depths, poses, intrinsics, near, far, app, extras, n_extra, i_train, n_train, N, H, W, counter, n, i0, i1,
                    origins, directions, viewdirs, radii, lossmult, near_out, far_out, app_out, rgb, depth, extras_out, sel_coords, img_out))
    return SNERF_ERR_ARG;
  MipBatch a{images, images_u8, depths, poses, intrinsics, near, far, app, extras, n_extra, i_train, n_train, N, H, W,
             (unsigned)(unsigned long)seed, (unsigned)((unsigned long)seed >> 32), counter, n, i0, i1, origins, directions, viewdirs, radii,
             lossmult, near_out, far_out, app_out, rgb, depth, extras_out, sel_coords, img_out, patch_sz, k0, k1};
  const long nl = (i1 - i0) + (long)(k1 - k0) * patch_sz * patch_sz;
  hipLaunchKernelGGL(mip_image_batch_kernel, dim3((unsigned)(nl > 0 ? (nl + 255) / 256 : 1)), dim3(256), 0, (hipStream_t)stream, a);
  return snerf_check_launch();
}

extern "C" int snerf_mip_image_batch(const void* images, int images_u8, const float* depths, const float* poses, const float* intrinsics,
                                     const float* near, const float* far, const float* app, const float* extras, int n_extra, const int* i_train,
                                     int n_train, int N, int H, int W, long seed, long* counter, long n, long i0, long i1, float* origins,
                                     float* directions, float* viewdirs, float* radii, float* lossmult, float* near_out, float* far_out,
                                     float* app_out, float* rgb, float* depth, float* extras_out, long* sel_coords, long* img_out, void* stream) {
  return snerf_mip_image_patch_batch(images, images_u8, depths, poses, intrinsics, near, far, app, extras, n_extra, i_train, n_train, N, H, W, seed,
                                     counter, n, i0, i1, origins, directions, viewdirs, radii, lossmult, near_out, far_out, app_out, rgb, depth,
                                     extras_out, sel_coords, img_out, 0, 0, 0, 0, stream);
}

// ---------------------------------------------------------------------------
// Training batch of the classic path: the device-resident form of the stock `use_batching` loader (every ray of the training images,
// shuffled, N_rand at a time).  T = n_train H W rays; row r of step s sits at global position p = s N_rand + r, in epoch e = p / T, and
// is ray q = perm(4, e, T)(p mod T) -> image i_train[q / (H W)], pixel (q mod (H W)) / W, (q mod (H W)) mod W: every ray exactly once
// per epoch, a new order every epoch, batches of constant size that may straddle an epoch boundary.  Given the pixel, the row is what
// classic_rays_kernel writes for that pixel of that camera (the same device functions, the same fp32 roundings of focal / cx / cy and
// of the NDC constants), the target the pixel's colour (texel).  One lane per row; rows [i0, i1) of the global batch: a rank's slice.
// ---------------------------------------------------------------------------
struct ClassicBatch {
  const void* images; int u8;                     // [n_img,H,W,3]
  const float* c2w;                               // [n_img,3,4]
  const double* intr;                             // [n_img,3] = (focal, cx, cy)
  const int* i_train; int n_train, n_img, H, W;
  unsigned k0, k1;
  long* ctr;
  long n, i0, i1;
  int ndc, use_viewdirs;
  float near, far;
  float* rows; int ld;
  float* rgb;
};

__global__ __launch_bounds__(256) void classic_train_batch_kernel(ClassicBatch a) {
  const long s = batch_step(a.ctr);
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.i1 - a.i0) return;
  const unsigned long long HW = (unsigned long long)a.H * a.W, T = HW * (unsigned long long)a.n_train;
  const unsigned long long p = (unsigned long long)s * (unsigned long long)a.n + (unsigned long long)(a.i0 + r);
  const unsigned long long e = p / T;
  const unsigned long long q = keyed_perm(p - e * T, T, 4u, (long)e, a.k0, a.k1);
  const unsigned long long slot = q / HW, pixel = q - slot * HW;
  const int img = a.i_train[slot];
  if (img < 0 || img >= a.n_img) return;          // (RayBatcher checks i_train on the host; never read past the tables)
  const int row = (int)(pixel / (unsigned)a.W), col = (int)(pixel - (unsigned long long)row * a.W);
  const double* k = a.intr + 3 * (long)img;
  float o[3], d[3], v[3] = {0.f, 0.f, 0.f};
  classic_pinhole(a.c2w + 12 * (long)img, row, col, (float)k[0], (float)k[1], (float)k[2], o, d);
  if (a.use_viewdirs) classic_unit(d, v);
  if (a.ndc) classic_ndc(1.f, (float)(-1.0 / ((double)a.W / (2.0 * k[0]))), (float)(-1.0 / ((double)a.H / (2.0 * k[0]))), o, d);
  classic_store_row(a.rows + r * a.ld, o, d, a.near, a.far, nullptr, a.use_viewdirs, v);
  const long pix = (long)img * (long)HW + (long)pixel;
#pragma unroll
  for (int c = 0; c < 3; ++c) a.rgb[3 * r + c] = texel(a.images, a.u8, 3 * pix + c);
}

extern "C" int snerf_classic_train_batch(const void* images, int images_u8, const float* c2w, const double* intrinsics, const int* i_train,
                                         int n_train, int n_images, int H, int W, long seed, long* counter, long n, long i0, long i1,
                                         int ndc, float near, float far, int use_viewdirs, float* rows, int ld, float* rgb, void* stream) {
  if (n <= 0 || n_images < 1 || n_train < 1 || H < 1 || W < 1 || i0 < 0 || i1 < i0 || i1 > n || seed < 0) return SNERF_ERR_ARG;
  if (images == nullptr || c2w == nullptr || intrinsics == nullptr || i_train == nullptr || counter == nullptr || rows == nullptr ||
      rgb == nullptr || (images_u8 != 0 && images_u8 != 1) || ld < (use_viewdirs ? 11 : 8))
    return SNERF_ERR_ARG;
  if ((((uintptr_t)c2w | (uintptr_t)i_train | (uintptr_t)rows | (uintptr_t)rgb) & 3) != 0 || (((uintptr_t)intrinsics | (uintptr_t)counter) & 7) != 0 ||
      (images_u8 == 0 && ((uintptr_t)images & 3) != 0))
    return SNERF_ERR_ARG;
  ClassicBatch a{images, images_u8, c2w, intrinsics, i_train, n_train, n_images, H, W, (unsigned)(unsigned long)seed,
                 (unsigned)((unsigned long)seed >> 32), counter, n, i0, i1, ndc ? 1 : 0, use_viewdirs ? 1 : 0, near, far, rows, ld, rgb};
  const long m = i1 - i0;
  hipLaunchKernelGGL(classic_train_batch_kernel, dim3((unsigned)(m > 0 ? (m + 255) / 256 : 1)), dim3(256), 0, (hipStream_t)stream, a);
  return snerf_check_launch();
}

struct ZipBatch {
  const void* images; int u8;                     // [N,H,W,3]
  const float* depths; const int* semantics; const float* masks;  // [N,H,W], nullable
  const float *pixtocams, *camtoworlds;           // [N,3,3], [N,3,4]
  const int* local2global;                        // [N], nullable
  int N, H, W, border, single_image;
  float near, far;
  unsigned k0, k1;
  long* ctr;
  long n, i0, i1;
  float *origins, *directions, *viewdirs, *radii, *imageplane, *base_x, *base_y, *lossmult, *near_out, *far_out, *cam_out, *glo_out;
  float *rgb, *depth; int* semantic; float* mask;
  int *pix_x, *pix_y;
  int patch; long pk0, pk1;                         // snerf_zip_ray_patch_batch: patches [pk0, pk1) of patch^2 pixels ahead of the pixel rows
};

// one row of a path C batch: the ray and the gathered targets of pixel (x, y) of camera cam into row r
__device__ __forceinline__ void zip_batch_row(const ZipBatch& a, int cam, int x, int y, long r) {
  zip_ray(a.pixtocams + 9 * (long)cam, a.camtoworlds + 12 * (long)cam, x, y, r, a.origins, a.directions, a.viewdirs, a.radii, a.imageplane,
          a.base_x, a.base_y);
  const long pix = ((long)cam * a.H + y) * a.W + x;
#pragma unroll
  for (int c = 0; c < 3; ++c) a.rgb[3 * r + c] = texel(a.images, a.u8, 3 * pix + c);
  a.lossmult[r] = 1.f;
  a.near_out[r] = a.near;
  a.far_out[r] = a.far;
  a.cam_out[r] = (float)cam;
  if (a.glo_out != nullptr) a.glo_out[r] = (float)a.local2global[cam];
  if (a.depth != nullptr) a.depth[r] = a.depths[pix];
  if (a.semantic != nullptr) a.semantic[r] = a.semantics[pix];
  if (a.mask != nullptr) a.mask[r] = a.masks[pix];
  a.pix_x[r] = x;
  a.pix_y[r] = y;
}

__global__ __launch_bounds__(256) void zip_ray_batch_kernel(ZipBatch a) {
  const long s = batch_step(a.ctr);
  const long i = a.i0 + (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.i1) return;
  const int cam = bounded_draw(a.single_image ? 0u : (unsigned)i, 0u, s, (unsigned)a.N, a.k0, a.k1);
  const int x = a.border + bounded_draw((unsigned)i, 1u, s, (unsigned)(a.W - 2 * a.border), a.k0, a.k1);
  const int y = a.border + bounded_draw((unsigned)i, 2u, s, (unsigned)(a.H - 2 * a.border), a.k0, a.k1);
  zip_batch_row(a, cam, x, y, i - a.i0);
}

// Patch batches (datasets.py:397-414, 508-541): the first n_patch p^2 positions of the global batch are n_patch whole patches of p x p
// pixels, rows [dy][dx]; patch k draws its camera and its corner (x0, y0) in [border, W - border - p] x [border, H - border - p] with
// the bounded draw of its first position, (i, v) = (k p^2, 0 / 1 / 2).  The positions behind them are single pixels with the draw
// they have in snerf_zip_ray_batch.  A launch writes patches [pk0, pk1) followed by positions [i0, i1).
__global__ __launch_bounds__(256) void zip_ray_patch_batch_kernel(ZipBatch a) {
  const long s = batch_step(a.ctr);
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  const long pp = (long)a.patch * a.patch, npr = (a.pk1 - a.pk0) * pp;
  if (r >= npr + (a.i1 - a.i0)) return;
  if (r < npr) {
    const long k = a.pk0 + r / pp;
    const int t = (int)(r % pp), dy = t / a.patch, dx = t - dy * a.patch;
    const unsigned i = (unsigned)(k * pp);
    const int cam = bounded_draw(a.single_image ? 0u : i, 0u, s, (unsigned)a.N, a.k0, a.k1);
    const int x0 = a.border + bounded_draw(i, 1u, s, (unsigned)(a.W - 2 * a.border - a.patch + 1), a.k0, a.k1);
    const int y0 = a.border + bounded_draw(i, 2u, s, (unsigned)(a.H - 2 * a.border - a.patch + 1), a.k0, a.k1);
    zip_batch_row(a, cam, x0 + dx, y0 + dy, r);
  } else {
    const long i = a.i0 + (r - npr);
    const int cam = bounded_draw(a.single_image ? 0u : (unsigned)i, 0u, s, (unsigned)a.N, a.k0, a.k1);
    const int x = a.border + bounded_draw((unsigned)i, 1u, s, (unsigned)(a.W - 2 * a.border), a.k0, a.k1);
    const int y = a.border + bounded_draw((unsigned)i, 2u, s, (unsigned)(a.H - 2 * a.border), a.k0, a.k1);
    zip_batch_row(a, cam, x, y, r);
  }
}

extern "C" int snerf_zip_ray_batch(const void* images, int images_u8, const float* depths, const int* semantics, const float* masks,
                                   const float* pixtocams, const float* camtoworlds, const int* local2global, int N, int H, int W, float near,
                                   float far, int border, int patch_size, int single_image, long seed, long* counter, long n, long i0, long i1,
                                   float* origins, float* directions, float* viewdirs, float* radii, float* imageplane, float* base_x,
                                   float* base_y, float* lossmult, float* near_out, float* far_out, float* cam_idx, float* glo_idx, float* rgb,
                                   float* depth, int* semantic, float* mask, int* pix_x, int* pix_y, void* stream) {
  if (n == 0) return SNERF_OK;
  if (n < 0 || N < 1 || H < 1 || W < 1 || border < 0 || 2L * border >= W || 2L * border >= H || patch_size != 1 || i0 < 0 || i1 < i0 ||
      i1 > n || n > 0xFFFFFFFFL || (single_image != 0 && single_image != 1) || (images_u8 != 0 && images_u8 != 1))
    return SNERF_ERR_ARG;
  if (images == nullptr || pixtocams == nullptr || camtoworlds == nullptr || counter == nullptr || origins == nullptr || directions == nullptr ||
      viewdirs == nullptr || radii == nullptr || base_x == nullptr || base_y == nullptr || lossmult == nullptr || near_out == nullptr ||
      far_out == nullptr || cam_idx == nullptr || rgb == nullptr || pix_x == nullptr || pix_y == nullptr)
    return SNERF_ERR_ARG;
  if ((depth != nullptr && depths == nullptr) || (semantic != nullptr && semantics == nullptr) || (mask != nullptr && masks == nullptr) ||
      (glo_idx != nullptr && local2global == nullptr))
    return SNERF_ERR_ARG;
  ZipBatch a{images, images_u8, depths, semantics, masks, pixtocams, camtoworlds, local2global, N, H, W, border, single_image, near, far,
             (unsigned)(unsigned long)seed, (unsigned)((unsigned long)seed >> 32), counter, n, i0, i1, origins, directions, viewdirs, radii,
             imageplane, base_x, base_y, lossmult, near_out, far_out, cam_idx, glo_idx, rgb, depth, semantic, mask, pix_x, pix_y};
  const long nl = i1 - i0;
  hipLaunchKernelGGL(zip_ray_batch_kernel, dim3((unsigned)(nl > 0 ? (nl + 255) / 256 : 1)), dim3(256), 0, (hipStream_t)stream, a);
  return snerf_check_launch();
}

extern "C" int snerf_zip_ray_patch_batch(const void* images, int images_u8, const float* depths, const int* semantics, const float* masks,
                                         const float* pixtocams, const float* camtoworlds, const int* local2global, int N, int H, int W,
                                         float near, float far, int border, int patch_size, int single_image, long seed, long* counter, long n,
                                         long k0, long k1, long i0, long i1, float* origins, float* directions, float* viewdirs, float* radii,
                                         float* imageplane, float* base_x, float* base_y, float* lossmult, float* near_out, float* far_out,
                                         float* cam_idx, float* glo_idx, float* rgb, float* depth, int* semantic, float* mask, int* pix_x,
                                         int* pix_y, void* stream) {
  if (n == 0) return SNERF_OK;
  if (n < 0 || N < 1 || H < 1 || W < 1 || border < 0 || patch_size < 2 || patch_size > 32 || n > 0xFFFFFFFFL ||
      (single_image != 0 && single_image != 1) || (images_u8 != 0 && images_u8 != 1))
    return SNERF_ERR_ARG;
  const long pp = (long)patch_size * patch_size, n_patch = n / 4 / pp;
  if (n % (4 * pp) != 0 || 2L * border + patch_size > W || 2L * border + patch_size > H) return SNERF_ERR_ARG;
  if (k0 < 0 || k1 < k0 || k1 > n_patch || i0 < n_patch * pp || i1 < i0 || i1 > n) return SNERF_ERR_ARG;
  if (images == nullptr || pixtocams == nullptr || camtoworlds == nullptr || counter == nullptr || origins == nullptr || directions == nullptr ||
      viewdirs == nullptr || radii == nullptr || base_x == nullptr || base_y == nullptr || lossmult == nullptr || near_out == nullptr ||
      far_out == nullptr || cam_idx == nullptr || rgb == nullptr || pix_x == nullptr || pix_y == nullptr)
    return SNERF_ERR_ARG;
  if ((depth != nullptr && depths == nullptr) || (semantic != nullptr && semantics == nullptr) || (mask != nullptr && masks == nullptr) ||
      (glo_idx != nullptr && local2global == nullptr))
    return SNERF_ERR_ARG;
  ZipBatch a{images, images_u8, depths, semantics, masks, pixtocams, camtoworlds, local2global, N, H, W, border, single_image, near, far,
             (unsigned)(unsigned long)seed, (unsigned)((unsigned long)seed >> 32), counter, n, i0, i1, origins, directions, viewdirs, radii,
             imageplane, base_x, base_y, lossmult, near_out, far_out, cam_idx, glo_idx, rgb, depth, semantic, mask, pix_x, pix_y, patch_size, k0, k1};
  const long nl = (k1 - k0) * pp + (i1 - i0);
  hipLaunchKernelGGL(zip_ray_patch_batch_kernel, dim3((unsigned)(nl > 0 ? (nl + 255) / 256 : 1)), dim3(256), 0, (hipStream_t)stream, a);
  return snerf_check_launch();
}

// ---------------------------------------------------------------------------
// Per-ray loss tail of the zipnerf training step (s-nerfpp/zipnerf/train.py:250-311), value AND gradients w.r.t. the renderer
// outputs in one pass:
//   data        train_utils.py:62-90   sum(lossmult * sqrt(resid^2 + pad^2)) / sum(lossmult)   ('charb'; 'mse' = resid^2)
//   depth       train.py:252-255,277   depth_lambda * masked mean |1/(depth+1e-5) - 1/(1e-5+target)|
//   d_complete  train.py:260-272       the same under the second mask, x 0.2
//   sem         train.py:294-298       -sem_mult * masked mean log(semantic[r, label] + 1e-6)
//   interlevel  train_utils.py:132-164 (anti_interlevel_loss): NeRF histogram blurred by the level's pulse width
//               (stepfun.py:425-433), integrated to a piecewise-quadratic CDF, resampled on the proposal intervals
//               (math.py:133-156); mean(clamp(w_s - wp, 0)^2 / (wp + 1e-5)); gradient reaches the proposal weights only
//   distortion  stepfun.py:297-307     mean_r [sum_ij w_i w_j |u_i - u_j| + sum_i w_i^2 d_i / 3]; gradient w.r.t. the NeRF weights
// grid = (ceil(R/64), 3): y = 0 per-ray terms + distortion, y = 1, 2 the two proposal levels.  One lane per ray.  The blurred
// histogram is never materialised: its 2(S+1) knots are the merge of the two sorted lists {c - r} and {c + r}, walked once
// together with the (sorted) proposal fence posts; prefix sums run in float64 (the reference's fp32 cumsum of the +/- steps
// carries ~1e-4 relative noise, tests/test_oracle_callers_golden.py) and every emitted value is rounded once.
// out[0..3] = {3 sum lossmult, sum depth mask, sum complete mask, sum semantic mask};
// out[4..10] = {data, mse, depth, d_complete, sem, interlevel, distortion} (already multiplied by their weights).
// ---------------------------------------------------------------------------
struct ZipLoss {
  const float *rgb, *tgt, *lossmult;
  const float *depth, *tdepth, *dmask, *cmask;
  const float* sem; const int* labels; const float* smask;
  const float *s0, *w0, *s1, *w1, *s2, *w2;
  long R;
  int C, S0, S1, S2, mse;
  float pad, data_mult, depth_lambda, com_mult, sem_mult, pw0, pw1, inter_mult, dist_mult;
  float* out;
  float *g_rgb, *g_depth, *g_sem, *g_w0, *g_w1, *g_w2;
};

__global__ __launch_bounds__(1024) void zip_loss_prepare_kernel(ZipLoss a) {
  __shared__ float part[4][16];
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (long r = threadIdx.x; r < a.R; r += 1024) {
    s[0] += a.lossmult != nullptr ? a.lossmult[r] : 1.f;
    if (a.depth != nullptr && a.dmask != nullptr) s[1] += a.dmask[r];
    if (a.depth != nullptr && a.cmask != nullptr) s[2] += a.cmask[r];
    if (a.sem != nullptr) s[3] += a.smask != nullptr ? a.smask[r] : 1.f;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    s[k] = wave_sum(s[k]);
    if ((threadIdx.x & 63) == 0) part[k][threadIdx.x >> 6] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    float t = 0.f;
    for (int w = 0; w < 16; ++w) t += part[threadIdx.x][w];
    a.out[threadIdx.x] = threadIdx.x == 0 ? 3.f * t : t;
  }
  if (threadIdx.x >= 4 && threadIdx.x < 11) a.out[threadIdx.x] = 0.f;
}

// anti-interlevel term of one ray against one proposal level -> sum_j clamp(w_s - wp, 0)^2 / (wp + 1e-5); writes d/d wp
// (`g` may be `wp` itself: g[j] is written after the last read of wp[j] -- the LDS-staged caller overwrites the weights in place)
__device__ __forceinline__ float zip_interlevel_ray(const float* __restrict__ c, const float* __restrict__ w, int S, const float* __restrict__ cp,
                                                    const float* wp, int Sp, float r, float gscale, float* g) {
  const int n = S + 1;
  const double r2 = 2.0 * (double)r;
  // y1[k] = (wn[k] - wn[k-1]) / (2r) with wn = w / (c[k+1] - c[k]) and zeros outside (stepfun.py:427-428); each of the two knot streams
  // visits k = 0 .. S in order, so wn[k-1] is the value its previous visit computed (`last`): one division per knot
  auto y1 = [&](int k, double& last) __attribute__((always_inline)) {
    const double hi = k < S ? (double)w[k] / ((double)c[k + 1] - (double)c[k]) : 0.0;
    const double v = (hi - last) / r2;
    last = hi;
    return v;
  };
  double wn_a = 0.0, wn_b = 0.0;
  int ia = 0, ib = 0, q = 0;
  float xa = c[0] - r, xb = c[0] + r;
  double inner = 0.0, yrun = 0.0, cdf = 0.0;
  double xprev = 0.0, yprev = 0.0, cprev = 0.0;
  double ci_prev = 0.0;
  double loss = 0.0;
  auto emit = [&](double ci) __attribute__((always_inline)) {
    if (q > 0) {
      const double ws = ci - ci_prev;
      const double p = (double)wp[q - 1];
      const double over = ws > p ? ws - p : 0.0;
      const double den = p + 1e-5;
      loss += over * over / den;
      g[q - 1] = (float)((double)gscale * (-2.0 * over / den - over * over / (den * den)));
    }
    ci_prev = ci;
    ++q;
  };
  float xq = cp[0];
  for (int k = 0; k < 2 * n; ++k) {
    double xk, val;
    if (ib >= n || (ia < n && xa <= xb)) { xk = (double)xa; val = y1(ia, wn_a); ++ia; xa = ia < n ? c[ia] - r : 0.f; }
    else { xk = (double)xb; val = -y1(ib, wn_b); ++ib; xb = ib < n ? c[ib] + r : 0.f; }
    double yk = 0.0;
    if (k > 0) {
      const double dx = xk - xprev;
      yrun += dx * inner;
      yk = yrun > 0.0 ? yrun : 0.0;
      cdf += 0.5 * (yk + yprev) * dx;
    }
    // proposal fence posts in [x_{k-1}, x_k): idx = k knots are <= x (math.py:141-148)
    while (q <= Sp && (double)xq < xk) {
      double ci = 0.0;
      if (k > 0) {
        const double t = (double)xq - xprev;
        double off = t / (xk - xprev);
        off = off < 0.0 ? 0.0 : (off > 1.0 ? 1.0 : off);
        ci = cprev + t * (yprev + yk * off + yprev * (1.0 - off)) / 2.0;
      }
      emit(ci);
      xq = q <= Sp ? cp[q] : 0.f;
    }
    xprev = xk; yprev = yk; cprev = cdf;
    inner += val;
  }
  while (q <= Sp) {                                   // at or past the last knot: offset = 1 (or nan -> 0 when equal), both give this
    emit(cprev + ((double)xq - xprev) * yprev);
    xq = q <= Sp ? cp[q] : 0.f;
  }
  return (float)loss;
}

// The anti-interlevel term with a workgroup's 64 rays staged in LDS: the per-lane walks over (c, w, cp, wp) are 130 dependent steps of
// row-strided reads -- from global memory every one of them is 64 cache lines per wave instruction (573 us for 65 536 rays x 2 levels);
// staged through coalesced loads into odd-strided LDS rows (conflict-free for lane = ray) they are LDS latency.  The gradient overwrites
// the staged proposal weights in place and leaves through coalesced stores.  grid = (ceil(R / 64), 2 levels); same arithmetic, same
// order, same results as the global-memory walk (which stays for interval counts whose rows do not fit 160 KB).
__global__ __launch_bounds__(64) void zip_interlevel_lds_kernel(ZipLoss a) {
  extern __shared__ float zil_sm[];
  const int lvl = blockIdx.y;
  const float* sp = lvl == 0 ? a.s0 : a.s1;
  if (sp == nullptr) return;
  const int Sp = lvl == 0 ? a.S0 : a.S1, S = a.S2;
  const int stc = (S + 1) | 1, stw = S | 1, stp = (Sp + 1) | 1, stq = Sp | 1;
  float* sc = zil_sm;
  float* sw = sc + 64 * stc;
  float* scp = sw + 64 * stw;
  float* swp = scp + 64 * stp;
  const long r0 = (long)blockIdx.x * 64;
  const int nr = (int)(a.R - r0 < 64 ? a.R - r0 : 64);
  const int tid = threadIdx.x;
  auto stage = [&](const float* __restrict__ src, int len, float* dst, int stride) __attribute__((always_inline)) {
    for (int i = tid; i < nr * len; i += 64) { const int ray = i / len; dst[ray * stride + (i - ray * len)] = src[i]; }
  };
  stage(a.s2 + r0 * (S + 1), S + 1, sc, stc);
  stage(a.w2 + r0 * S, S, sw, stw);
  stage(sp + r0 * (Sp + 1), Sp + 1, scp, stp);
  stage((lvl == 0 ? a.w0 : a.w1) + r0 * Sp, Sp, swp, stq);
  __syncthreads();
  float l = 0.f;
  const float scale = a.inter_mult / ((float)a.R * (float)Sp);
  if (tid < nr)
    l = zip_interlevel_ray(sc + tid * stc, sw + tid * stw, S, scp + tid * stp, swp + tid * stq, Sp, lvl == 0 ? a.pw0 : a.pw1, scale, swp + tid * stq) * scale;
  __syncthreads();
  float* g = (lvl == 0 ? a.g_w0 : a.g_w1) + r0 * Sp;
  for (int i = tid; i < nr * Sp; i += 64) { const int ray = i / Sp; g[i] = swp[ray * stq + (i - ray * Sp)]; }
  l = wave_sum(l);
  if (tid == 0) atomicAdd(a.out + 9, l);
}

__global__ __launch_bounds__(64) void zip_loss_tail_kernel(ZipLoss a) {
  const long r = (long)blockIdx.x * 64 + threadIdx.x;
  const int task = blockIdx.y;
  const bool on = r < a.R;
  if (task > 0) {
    if (a.s2 == nullptr || a.inter_mult <= 0.f) return;
    const int lvl = task - 1;
    const float* sp = lvl == 0 ? a.s0 : a.s1;
    if (sp == nullptr) return;
    const int Sp = lvl == 0 ? a.S0 : a.S1;
    float l = 0.f;
    if (on) {
      const float* wp = (lvl == 0 ? a.w0 : a.w1) + r * Sp;
      float* g = (lvl == 0 ? a.g_w0 : a.g_w1) + r * Sp;
      const float sc = a.inter_mult / ((float)a.R * (float)Sp);
      l = zip_interlevel_ray(a.s2 + r * (a.S2 + 1), a.w2 + r * a.S2, a.S2, sp + r * (Sp + 1), wp, Sp, lvl == 0 ? a.pw0 : a.pw1, sc, g) * sc;
    }
    l = wave_sum(l);
    if (threadIdx.x == 0) atomicAdd(a.out + 9, l);
    return;
  }
  float l_data = 0.f, l_mse = 0.f, l_dep = 0.f, l_com = 0.f, l_sem = 0.f, l_dist = 0.f;
  if (on) {
    // ---- data term
    const float lm = a.lossmult != nullptr ? a.lossmult[r] : 1.f;
    const float inv = 1.f / a.out[0];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float d = a.rgb[3 * r + c] - a.tgt[3 * r + c];
      const float r2 = d * d;
      l_mse += lm * r2;
      if (a.mse) { l_data += lm * r2; a.g_rgb[3 * r + c] = a.data_mult * lm * 2.f * d * inv; }
      else {
        const float root = sqrtf(r2 + a.pad * a.pad);
        l_data += lm * root;
        a.g_rgb[3 * r + c] = a.data_mult * lm * (d / root) * inv;
      }
    }
    l_data *= a.data_mult * inv; l_mse *= inv;
    // ---- disparity L1 under the two masks
    if (a.depth != nullptr) {
      const float dp = a.depth[r] + 1e-5f;
      const float e = 1.f / dp - 1.f / (1e-5f + a.tdepth[r]);
      const float sg = (e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f)) * (-1.f / (dp * dp));
      float g = 0.f;
      if (a.dmask != nullptr && a.out[1] > 0.f) { const float k = a.depth_lambda * a.dmask[r] / a.out[1]; l_dep = k * fabsf(e); g += k * sg; }
      if (a.cmask != nullptr && a.out[2] > 0.f) { const float k = a.depth_lambda * a.com_mult * a.cmask[r] / a.out[2]; l_com = k * fabsf(e); g += k * sg; }
      a.g_depth[r] = g;
    }
    // ---- semantic NLL
    if (a.sem != nullptr) {
      const int lab = min(max(a.labels[r], 0), a.C - 1);
      const float m = a.smask != nullptr ? a.smask[r] : 1.f;
      const float p = a.sem[r * a.C + lab] + 1e-6f;
      const float k = a.out[3] > 0.f ? a.sem_mult * m / a.out[3] : 0.f;
      l_sem = -k * logf(p);
      for (int c = 0; c < a.C; ++c) a.g_sem[r * a.C + c] = c == lab ? -k / p : 0.f;
    }
    // ---- distortion: sum_ij w_i w_j |u_i - u_j| through prefix sums over the sorted midpoints
    if (a.s2 != nullptr && a.dist_mult > 0.f) {
      const float* c = a.s2 + r * (a.S2 + 1);
      const float* w = a.w2 + r * a.S2;
      float* g = a.g_w2 + r * a.S2;
      double W = 0.0, WU = 0.0;
      for (int k = 0; k < a.S2; ++k) { const double u = (double)((c[k + 1] + c[k]) / 2.f); W += (double)w[k]; WU += (double)w[k] * u; }
      double Wl = 0.0, WUl = 0.0, acc = 0.0;
      const float sc = a.dist_mult / (float)a.R;
      for (int k = 0; k < a.S2; ++k) {
        const double u = (double)((c[k + 1] + c[k]) / 2.f), wk = (double)w[k], dk = (double)(c[k + 1] - c[k]);
        const double Wg = W - Wl - wk, WUg = WU - WUl - wk * u;
        const double inner = u * (Wl - Wg) - (WUl - WUg);
        acc += wk * inner + wk * wk * dk / 3.0;
        g[k] = sc * (float)(2.0 * inner + 2.0 * wk * dk / 3.0);
        Wl += wk; WUl += wk * u;
      }
      l_dist = sc * (float)acc;
    }
  }
  l_data = wave_sum(l_data); l_mse = wave_sum(l_mse); l_dep = wave_sum(l_dep); l_com = wave_sum(l_com); l_sem = wave_sum(l_sem);
  l_dist = wave_sum(l_dist);
  if (threadIdx.x == 0) {
    atomicAdd(a.out + 4, l_data); atomicAdd(a.out + 5, l_mse);
    if (a.depth != nullptr) { atomicAdd(a.out + 6, l_dep); atomicAdd(a.out + 7, l_com); }
    if (a.sem != nullptr) atomicAdd(a.out + 8, l_sem);
    if (a.s2 != nullptr && a.dist_mult > 0.f) atomicAdd(a.out + 10, l_dist);
  }
}

extern "C" int snerf_zip_loss_tail(const float* rgb, const float* tgt, const float* lossmult, const float* depth, const float* tdepth,
                                   const float* dmask, const float* cmask, const float* sem, const int* labels, const float* smask, int C,
                                   const float* s0, const float* w0, int S0, const float* s1, const float* w1, int S1, const float* s2,
                                   const float* w2, int S2, long R, int mse, float pad, float data_mult, float depth_lambda, float com_mult,
                                   float sem_mult, float pw0, float pw1, float inter_mult, float dist_mult, float* out, float* g_rgb,
                                   float* g_depth, float* g_sem, float* g_w0, float* g_w1, float* g_w2, void* stream) {
  if (R <= 0) return SNERF_OK;
  if (rgb == nullptr || tgt == nullptr || out == nullptr || g_rgb == nullptr) return SNERF_ERR_ARG;
  if (depth != nullptr && (tdepth == nullptr || g_depth == nullptr)) return SNERF_ERR_ARG;
  if (sem != nullptr && (labels == nullptr || g_sem == nullptr || C < 1)) return SNERF_ERR_ARG;
  if (s2 != nullptr) {
    if (w2 == nullptr || S2 < 1) return SNERF_ERR_ARG;
    if (dist_mult > 0.f && g_w2 == nullptr) return SNERF_ERR_ARG;
    if (inter_mult > 0.f) {
      if (s0 != nullptr && (w0 == nullptr || g_w0 == nullptr || S0 < 1 || !(pw0 > 0.f))) return SNERF_ERR_ARG;
      if (s1 != nullptr && (w1 == nullptr || g_w1 == nullptr || S1 < 1 || !(pw1 > 0.f))) return SNERF_ERR_ARG;
    }
  }
  ZipLoss a{rgb, tgt, lossmult, depth, tdepth, dmask, cmask, sem, labels, smask, s0, w0, s1, w1, s2, w2, R, C, S0, S1, S2, mse,
            pad, data_mult, depth_lambda, com_mult, sem_mult, pw0, pw1, inter_mult, dist_mult, out, g_rgb, g_depth, g_sem, g_w0, g_w1, g_w2};
  hipLaunchKernelGGL(zip_loss_prepare_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
  const bool inter = s2 != nullptr && inter_mult > 0.f && (s0 != nullptr || s1 != nullptr);
  // the interlevel walks from LDS when a workgroup's rows fit (the shipped interval counts: 49 KB); else from global memory (y = 1, 2)
  const int Spm = (s0 != nullptr ? S0 : 0) > (s1 != nullptr ? S1 : 0) ? S0 : S1;
  const size_t lds = (size_t)64 * 4 * (((S2 + 1) | 1) + (S2 | 1) + ((Spm + 1) | 1) + (Spm | 1));
  const bool staged = inter && lds <= 160 * 1024;
  hipLaunchKernelGGL(zip_loss_tail_kernel, dim3((unsigned)((R + 63) / 64), inter && !staged ? 3 : 1), dim3(64), 0, (hipStream_t)stream, a);
  if (staged) snerf_launch<zip_interlevel_lds_kernel>(dim3((unsigned)((R + 63) / 64), 2), dim3(64), lds, 160 * 1024, (hipStream_t)stream, a);
  return snerf_check_launch();
}

// ---------------------------------------------------------------------------
// Frame quantisation for the S-NeRF++ wire format (s-nerfpp/zipnerf/random_render_waymo_seq.py:214-227):
//   rgb    u8  = trunc(clip(nan_to_num(rgb), 0, 1) * 255)                       internal/utils.py:111-116 (save_img_u8)
//   depth  u16 = (depth * 256 / scale_factor).astype(uint16)                    :218-219 (float32 product and quotient, truncation;
//                                                                                values past 65535 wrap like the x86 int32 cast numpy emits)
//   label  u8  = argmax_c semantic[., c] (first maximum)                        :222-223
//   paint  u8x3 = color_map[label]                                              :225
// One pass over the rendered buffers on the device: the host copy shrinks from (3 + 1 + C) floats to 9 bytes per pixel.
// ---------------------------------------------------------------------------
struct FrameQ {
  const float *rgb, *depth, *sem; long ld_sem; int C; const unsigned char* cmap; long P; float scale_factor;
  unsigned char* rgb8; unsigned short* depth16; unsigned char* label8; unsigned char* paint8;
};

__global__ __launch_bounds__(256) void frame_quantize_kernel(FrameQ a) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.P) return;
  if (a.rgb != nullptr) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = a.rgb[3 * p + c];
      v = v != v ? 0.f : v;                                   // nan_to_num: nan -> 0, +/-inf -> +/-max (then clipped)
      v = fminf(fmaxf(v, 0.f), 1.f) * 255.f;
      a.rgb8[3 * p + c] = (unsigned char)(int)v;
    }
  }
  if (a.depth != nullptr) {
    const float v = a.depth[p] * 256.f / a.scale_factor;
    int q;
    if (!(v == v)) q = (int)0x80000000;                       // cvttss2si's "integer indefinite" for nan / out-of-range
    else if (v >= 2147483648.f || v < -2147483648.f) q = (int)0x80000000;
    else q = (int)v;
    a.depth16[p] = (unsigned short)(q & 0xFFFF);
  }
  if (a.sem != nullptr) {
    const float* s = a.sem + p * a.ld_sem;
    int best = 0;
    float bv = s[0];
    for (int c = 1; c < a.C; ++c) {
      const float v = s[c];
      if (v > bv || (v != v && bv == bv)) { bv = v; best = c; }   // np.argmax: first maximum; a nan is a maximum
    }
    a.label8[p] = (unsigned char)best;
    if (a.paint8 != nullptr) {
#pragma unroll
      for (int c = 0; c < 3; ++c) a.paint8[3 * p + c] = a.cmap[3 * best + c];
    }
  }
}

extern "C" int snerf_frame_quantize(const float* rgb, const float* depth, const float* sem, long ld_sem, int C, const void* color_map, long P,
                                    float scale_factor, void* rgb_u8, void* depth_u16, void* label_u8, void* paint_u8, void* stream) {
  if (P <= 0) return SNERF_OK;
  if (rgb != nullptr && rgb_u8 == nullptr) return SNERF_ERR_ARG;
  if (depth != nullptr && (depth_u16 == nullptr || !(scale_factor != 0.f))) return SNERF_ERR_ARG;
  if (sem != nullptr && (label_u8 == nullptr || C < 1 || C > 256 || ld_sem < C)) return SNERF_ERR_ARG;
  if (sem != nullptr && paint_u8 != nullptr && color_map == nullptr) return SNERF_ERR_ARG;
  FrameQ a{rgb, depth, sem, ld_sem, C, (const unsigned char*)color_map, P, scale_factor, (unsigned char*)rgb_u8, (unsigned short*)depth_u16,
           (unsigned char*)label_u8, (unsigned char*)paint_u8};
  hipLaunchKernelGGL(frame_quantize_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return snerf_check_launch();
}

// ---------------------------------------------------------------------------
// Hash-grid weight decay of the zipnerf training step (s-nerfpp/zipnerf/internal/train_utils.py:184-203, hash_decay_loss, on by default:
// configs.py:74 hash_decay_mults = 0.1): per encoder, mult * mean_{l,c}( mean over the rows of level l of table[row, c]^2 ) -- the
// reference computes the per-level means with torch_scatter.segment_coo(param ** 2, idx, reduce='mean').  Value and gradient
// (grad += 2 mult p / (rows_l L C)) in one pass over the table; grid.y = level.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hash_decay_kernel(const float* __restrict__ table, float* __restrict__ grad, const int* __restrict__ offsets,
                                                         int L, int C, float mult, float* __restrict__ loss) {
  const int level = blockIdx.y;
  const long b = (long)offsets[level] * C, e = (long)offsets[level + 1] * C;
  const float k = mult / ((float)(offsets[level + 1] - offsets[level]) * (float)L * (float)C);
  float part = 0.f;
  for (long i = b + (long)blockIdx.x * 256 + threadIdx.x; i < e; i += (long)gridDim.x * 256) {
    const float p = table[i];
    part += p * p;
    grad[i] += 2.f * k * p;
  }
  part = wave_sum(part);
  __shared__ float ws[4];
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = part;
  __syncthreads();
  if (threadIdx.x == 0 && loss != nullptr) atomicAdd(loss, k * (ws[0] + ws[1] + ws[2] + ws[3]));
}

extern "C" int snerf_hash_decay(const float* table, float* grad, const int* offsets, int L, int C, float mult, float* loss, void* stream) {
  if (L <= 0 || mult == 0.f) return SNERF_OK;
  if (table == nullptr || grad == nullptr || offsets == nullptr || C < 1) return SNERF_ERR_ARG;
  hipLaunchKernelGGL(hash_decay_kernel, dim3(512, L), dim3(256), 0, (hipStream_t)stream, table, grad, offsets, L, C, mult, loss);
  return snerf_check_launch();
}
