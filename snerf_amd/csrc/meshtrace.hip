// First-hit ray / triangle-mesh tracer: the mesh depth and hit masks of the S-NeRF++ foreground stages on the device.
//
// Reference counterpart: `raytracing.RayTracer(vertices, faces).trace(ray_o, ray_d)` as called by s-nerfpp/stage1_code/utils_render.py:839-868
// (the mesh depth along every masked pixel's ray; `depth[depth >= 99.] = .1`) and s-nerfpp/stage0_code/utils_render.py:755-776 (the instance
// mask `depth < 100.`).  That library is not part of the reference tree, so what it does at an edge, its normal orientation and whether it
// reports hits beyond its max depth of 100 cannot be pinned; defined here: a hit needs 0 < t < t_max, the nearest one wins, a miss
// returns t_max (pinhole entry: miss_value) with zero position and normal and face id -1.
//
// Structure: flat and two-level, no tree and no per-lane stack.  The caller orders the triangles once by the Morton code of their
// object-space centroids (an affine map keeps neighbours neighbours, so the order serves every frame); 64 consecutive triangles are a
// chunk, 64 consecutive chunks a group.  Per call, mesh_prepare_kernel applies the 3 x 4 transform, writes one 48-byte record per
// triangle (three vertices + the caller's face id) and the chunks' boxes, mesh_group_box_kernel the groups' boxes.  The trace kernels
// run one wave per workgroup and one lane per ray (an 8 x 8 pixel tile, or 64 consecutive rays): the group and the chunk loop are
// wave-uniform -- every lane tests its ray against the box, clipped to its nearest hit so far, and a ballot decides whether the wave
// enters -- and inside a chunk all lanes walk the same 64 records, which the wave has staged in LDS (48 bytes per lane, read back as
// broadcasts; MT_UNIFORM reads them through wave-uniform global loads instead: measured 4 % slower on the culled 1920 x 1280 shape of
// tools/bench_mesh_trace.py and 4 % faster with culling off, profiles/r22_a_mesh_trace.txt, so staging is what ships).
// No recursion, no atomics, plain vector stores.
//
// Watertightness: the intersection is Woop, Benthin and Wald's (JCGT 2013) in plain fp32 without their double fallback.  The vertices
// are moved to the ray's origin and sheared so that the ray becomes the axis of its largest direction component; the sheared x, y of a
// vertex depend on the vertex and the ray only, never on the triangle.  The three edge functions are e(P, Q) = Qx Py - Qy Px with two
// rounded products and one subtraction (this unit is built with -ffp-contract=off): e(Q, P) is exactly -e(P, Q), so the two triangles
// of an edge see the same number, and because rounding is monotonic its sign is the exact sign or zero.  A triangle is hit when no two
// of its edge functions have opposite signs (zero sides with both), so the triangle that really contains the ray's foot point is
// always accepted: no ray slips between two triangles.  The boxes are padded by 1e-5 of their coordinates and the slab test by 1e-5 of
// t, far more than the shear's rounding.  Degenerate faces (an index outside [0, V), a non-finite vertex, a zero cross product) are
// stored as zero records that no ray hits and are left out of the boxes; a ray with a non-finite component or a zero direction hits
// nothing.
//
// The renderer at the end of the file (snerf_mesh_render_pinhole: the instance image and mask of api_code/mesh_renderer.py) shades the
// pinhole entry's first hit; it shares the walk and the intersection routine, so its visibility is the tracer's bit for bit.
#include "common.h"
#include <float.h>
#include <math.h>

#define MT_CHUNK 64
#define MT_GROUP 64
#define MT_TRI_BYTES 48
#define MT_BOX_BYTES 32
#define MT_NO_CULL 1            // flags bit 0: enter every chunk (the all-pairs flavour of the same kernel, for measurements)
#define MT_UNIFORM 2            // flags bit 1: read each entered chunk through wave-uniform loads instead of staging it in LDS

static inline long mt_chunks(long F) { return (F + MT_CHUNK - 1) / MT_CHUNK; }
static inline long mt_groups(long F) { return (mt_chunks(F) + MT_GROUP - 1) / MT_GROUP; }

extern "C" long snerf_mesh_ws_bytes(int F) {
  if (F <= 0) return 0;
  const long nc = mt_chunks(F), ng = mt_groups(F);
  return (nc * MT_CHUNK * MT_TRI_BYTES + ng * MT_GROUP * MT_BOX_BYTES + ng * MT_BOX_BYTES + 255) / 256 * 256;
}

struct MtMesh {                 // views into the workspace
  const float4* tri;            // [n_chunks * 64][3]: (a.xyz, face id), (b.xyz, 0), (c.xyz, 0); zero records behind F and for degenerate faces
  const float4* cbox;           // [n_groups * 64][2]: (lo.xyz, 0), (hi.xyz, 0); lo.x > hi.x = empty
  const float4* gbox;           // [n_groups][2]
  int F, n_chunks, n_groups;
};

static inline MtMesh mt_views(void* ws, int F) {
  MtMesh m;
  const long nc = mt_chunks(F), ng = mt_groups(F);
  m.tri = (const float4*)ws;
  m.cbox = (const float4*)((char*)ws + nc * MT_CHUNK * MT_TRI_BYTES);
  m.gbox = (const float4*)((char*)ws + nc * MT_CHUNK * MT_TRI_BYTES + ng * MT_GROUP * MT_BOX_BYTES);
  m.F = F; m.n_chunks = (int)nc; m.n_groups = (int)ng;
  return m;
}

__device__ __forceinline__ bool mt_finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

__device__ __forceinline__ void mt_write_box(float4* box, float lx, float ly, float lz, float hx, float hy, float hz) {
  if (lx <= hx) {               // not empty: pad by 1e-5 of the coordinates
    const float px = 1e-5f * fmaxf(fabsf(lx), fabsf(hx)) + FLT_MIN, py = 1e-5f * fmaxf(fabsf(ly), fabsf(hy)) + FLT_MIN,
                pz = 1e-5f * fmaxf(fabsf(lz), fabsf(hz)) + FLT_MIN;
    lx = lx - px; ly = ly - py; lz = lz - pz; hx = hx + px; hy = hy + py; hz = hz + pz;
  }
  box[0] = make_float4(lx, ly, lz, 0.f);
  box[1] = make_float4(hx, hy, hz, 0.f);
}

__device__ __forceinline__ void mt_wave_box(float& lx, float& ly, float& lz, float& hx, float& hy, float& hz) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lx = fminf(lx, __shfl_xor(lx, o, 64)); ly = fminf(ly, __shfl_xor(ly, o, 64)); lz = fminf(lz, __shfl_xor(lz, o, 64));
    hx = fmaxf(hx, __shfl_xor(hx, o, 64)); hy = fmaxf(hy, __shfl_xor(hy, o, 64)); hz = fmaxf(hz, __shfl_xor(hz, o, 64));
  }
}

// One wave per chunk slot (n_groups * 64 of them; the slots behind the last chunk get empty boxes), one lane per ordered triangle.
__global__ __launch_bounds__(64) void mesh_prepare_kernel(const float* __restrict__ vertices, int V, const int* __restrict__ faces,
                                                          const int* __restrict__ face_ids, const float* __restrict__ xf, float4* tri,
                                                          float4* cbox, int F, int n_chunks) {
  const int c = blockIdx.x, lane = threadIdx.x;
  float lx = FLT_MAX, ly = FLT_MAX, lz = FLT_MAX, hx = -FLT_MAX, hy = -FLT_MAX, hz = -FLT_MAX;
  if (c < n_chunks) {
    const long k = (long)c * MT_CHUNK + lane;
    float p[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    int id = -1;
    bool good = false;
    if (k < F) {
      const int i0 = faces[3 * k], i1 = faces[3 * k + 1], i2 = faces[3 * k + 2];
      if (i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V) {      // checked before any vertex is read
        const int idx[3] = {i0, i1, i2};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const float x = vertices[3l * idx[j]], y = vertices[3l * idx[j] + 1], z = vertices[3l * idx[j] + 2];
          if (xf != nullptr) {
            p[j][0] = ((xf[0] * x + xf[1] * y) + xf[2] * z) + xf[3];
            p[j][1] = ((xf[4] * x + xf[5] * y) + xf[6] * z) + xf[7];
            p[j][2] = ((xf[8] * x + xf[9] * y) + xf[10] * z) + xf[11];
          } else {
            p[j][0] = x; p[j][1] = y; p[j][2] = z;
          }
        }
        const float e1x = p[1][0] - p[0][0], e1y = p[1][1] - p[0][1], e1z = p[1][2] - p[0][2];
        const float e2x = p[2][0] - p[0][0], e2y = p[2][1] - p[0][1], e2z = p[2][2] - p[0][2];
        const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
        good = mt_finite3(p[0][0], p[0][1], p[0][2]) && mt_finite3(p[1][0], p[1][1], p[1][2]) && mt_finite3(p[2][0], p[2][1], p[2][2])
               && mt_finite3(nx, ny, nz) && (nx != 0.f || ny != 0.f || nz != 0.f);
      }
    }
    if (good) {
      id = face_ids != nullptr ? face_ids[k] : (int)k;
      lx = fminf(p[0][0], fminf(p[1][0], p[2][0])); hx = fmaxf(p[0][0], fmaxf(p[1][0], p[2][0]));
      ly = fminf(p[0][1], fminf(p[1][1], p[2][1])); hy = fmaxf(p[0][1], fmaxf(p[1][1], p[2][1]));
      lz = fminf(p[0][2], fminf(p[1][2], p[2][2])); hz = fmaxf(p[0][2], fmaxf(p[1][2], p[2][2]));
    } else {
#pragma unroll
      for (int j = 0; j < 3; ++j) { p[j][0] = 0.f; p[j][1] = 0.f; p[j][2] = 0.f; }
    }
    tri[3 * k] = make_float4(p[0][0], p[0][1], p[0][2], __int_as_float(id));
    tri[3 * k + 1] = make_float4(p[1][0], p[1][1], p[1][2], 0.f);
    tri[3 * k + 2] = make_float4(p[2][0], p[2][1], p[2][2], 0.f);
  }
  mt_wave_box(lx, ly, lz, hx, hy, hz);
  if (lane == 0) mt_write_box(cbox + 2l * c, lx, ly, lz, hx, hy, hz);
}

// One wave per group, one lane per chunk slot (all 64 exist).  The chunks' boxes are padded already; the union is padded once more.
__global__ __launch_bounds__(64) void mesh_group_box_kernel(const float4* __restrict__ cbox, float4* gbox) {
  const long s = (long)blockIdx.x * MT_GROUP + threadIdx.x;
  const float4 lo = cbox[2 * s], hi = cbox[2 * s + 1];
  float lx = lo.x, ly = lo.y, lz = lo.z, hx = hi.x, hy = hi.y, hz = hi.z;
  if (lx > hx) { lx = FLT_MAX; ly = FLT_MAX; lz = FLT_MAX; hx = -FLT_MAX; hy = -FLT_MAX; hz = -FLT_MAX; }
  mt_wave_box(lx, ly, lz, hx, hy, hz);
  if (threadIdx.x == 0) mt_write_box(gbox + 2l * blockIdx.x, lx, ly, lz, hx, hy, hz);
}

extern "C" int snerf_mesh_prepare(const float* vertices, int V, const int* faces, const int* face_ids, int F, const float* transform,
                                  void* ws, long ws_bytes, void* stream) {
  if (F < 0 || V < 0) return SNERF_ERR_ARG;
  if (F == 0) return SNERF_OK;
  if (faces == nullptr || (vertices == nullptr && V > 0) || ws == nullptr || ((uintptr_t)ws & 15) != 0) return SNERF_ERR_ARG;
  if (ws_bytes < snerf_mesh_ws_bytes(F)) return SNERF_ERR_ARG;
  const MtMesh m = mt_views(ws, F);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mesh_prepare_kernel, dim3((unsigned)(m.n_groups * MT_GROUP)), dim3(64), 0, st, vertices, V, faces, face_ids, transform,
                     (float4*)m.tri, (float4*)m.cbox, F, m.n_chunks);
  hipLaunchKernelGGL(mesh_group_box_kernel, dim3((unsigned)m.n_groups), dim3(64), 0, st, m.cbox, (float4*)m.gbox);
  return snerf_check_launch();
}

// ---- the trace --------------------------------------------------------------------------------------------------------------------------
struct MtRay {
  float ox, oy, oz;             // origin
  float ix, iy, iz;             // 1 / d per axis for the slab test (1e30 where |d| < 1e-30: the slab then only asks whether o lies inside)
  float sx, sy, sz;             // the shear: d[kx] / d[kz], d[ky] / d[kz], 1 / d[kz]
  int kz;                       // axis of the largest |d|; kx = kz + 1, ky = kz + 2 (mod 3)
  bool ok;                      // a ray that can hit: every component finite, d != 0
};

__device__ __forceinline__ MtRay mt_ray(float ox, float oy, float oz, float dx, float dy, float dz, bool ok) {
  MtRay r;
  r.ok = ok && mt_finite3(ox, oy, oz) && mt_finite3(dx, dy, dz) && (dx != 0.f || dy != 0.f || dz != 0.f);
  if (!r.ok) { ox = 0.f; oy = 0.f; oz = 0.f; dx = 0.f; dy = 0.f; dz = -1.f; }
  r.ox = ox; r.oy = oy; r.oz = oz;
  const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
  r.kz = (az >= ax && az >= ay) ? 2 : (ax >= ay ? 0 : 1);
  const float dkz = r.kz == 2 ? dz : (r.kz == 0 ? dx : dy);
  const float dkx = r.kz == 2 ? dx : (r.kz == 0 ? dy : dz);
  const float dky = r.kz == 2 ? dy : (r.kz == 0 ? dz : dx);
  r.sx = dkx / dkz; r.sy = dky / dkz; r.sz = 1.f / dkz;
  r.ix = ax > 1e-30f ? 1.f / dx : 1e30f; r.iy = ay > 1e-30f ? 1.f / dy : 1e30f; r.iz = az > 1e-30f ? 1.f / dz : 1e30f;
  return r;
}

// does the ray meet the box within [0, t_best]?  (1e-5 of slack on both ends; the boxes are padded too)
__device__ __forceinline__ bool mt_slab(const float4 lo, const float4 hi, const MtRay& r, float t_best) {
  const float x1 = (lo.x - r.ox) * r.ix, x2 = (hi.x - r.ox) * r.ix;
  const float y1 = (lo.y - r.oy) * r.iy, y2 = (hi.y - r.oy) * r.iy;
  const float z1 = (lo.z - r.oz) * r.iz, z2 = (hi.z - r.oz) * r.iz;
  const float tn = fmaxf(fmaxf(fminf(x1, x2), fminf(y1, y2)), fmaxf(fminf(z1, z2), 0.f));
  const float tf = fminf(fminf(fmaxf(x1, x2), fmaxf(y1, y2)), fminf(fmaxf(z1, z2), t_best));
  return r.ok && tn * 0.99999f <= tf * 1.00001f;
}

// (x, y, z) -> (v[kx], v[ky], v[kz]); KZ >= 0: the axis is a compile-time constant (no selects)
template <int KZ> __device__ __forceinline__ void mt_perm(int kz, float x, float y, float z, float& px, float& py, float& pz) {
  const int k = KZ >= 0 ? KZ : kz;
  px = k == 2 ? x : (k == 0 ? y : z);
  py = k == 2 ? y : (k == 0 ? z : x);
  pz = k == 2 ? z : (k == 0 ? x : y);
}

// The one intersection routine of both entries: record k against the lane's ray; a nearer hit replaces (t_best, k_best).
template <int KZ> __device__ __forceinline__ void mt_hit(const float4 a, const float4 b, const float4 c, const MtRay& r, bool live, int k,
                                                         float& t_best, int& k_best) {
  float ax, ay, az, bx, by, bz, cx, cy, cz;
  mt_perm<KZ>(r.kz, a.x - r.ox, a.y - r.oy, a.z - r.oz, ax, ay, az);
  mt_perm<KZ>(r.kz, b.x - r.ox, b.y - r.oy, b.z - r.oz, bx, by, bz);
  mt_perm<KZ>(r.kz, c.x - r.ox, c.y - r.oy, c.z - r.oz, cx, cy, cz);
  ax = ax - r.sx * az; ay = ay - r.sy * az;
  bx = bx - r.sx * bz; by = by - r.sy * bz;
  cx = cx - r.sx * cz; cy = cy - r.sy * cz;
  const float u = cx * by - cy * bx, v = ax * cy - ay * cx, w = bx * ay - by * ax;     // e(B, C), e(C, A), e(A, B)
  const bool neg = u < 0.f || v < 0.f || w < 0.f, pos = u > 0.f || v > 0.f || w > 0.f;
  const float det = (u + v) + w;
  const float t = ((u * (r.sz * az) + v * (r.sz * bz)) + w * (r.sz * cz)) / det;
  if (live && !(neg && pos) && det != 0.f && t > 0.f && t < t_best) { t_best = t; k_best = k; }   // a NaN t fails both comparisons
}

// `live`: the lane's own ray met the chunk's box (or culling is off).  A lane that rides along because a neighbour's ray met it takes no hit,
// so what a ray returns never depends on the rays that share its wave.
template <int KZ, bool LDS> __device__ __forceinline__ void mt_chunk(const MtMesh& m, int c, const MtRay& r, bool live, float4* s_tri, float& t_best,
                                                                     int& k_best) {
  const int k0 = c * MT_CHUNK, n = min(MT_CHUNK, m.F - k0);
  if (LDS) {
    __syncthreads();                                                            // (one wave per workgroup: the previous chunk's reads are done)
    const float4* src = m.tri + 3l * (k0 + threadIdx.x);                       // the records behind F exist (zeros)
    s_tri[3 * threadIdx.x] = src[0]; s_tri[3 * threadIdx.x + 1] = src[1]; s_tri[3 * threadIdx.x + 2] = src[2];
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < n; ++i) mt_hit<KZ>(s_tri[3 * i], s_tri[3 * i + 1], s_tri[3 * i + 2], r, live, k0 + i, t_best, k_best);
  } else {
    const float4* src = m.tri + 3l * k0;
#pragma unroll 4
    for (int i = 0; i < n; ++i) mt_hit<KZ>(src[3 * i], src[3 * i + 1], src[3 * i + 2], r, live, k0 + i, t_best, k_best);
  }
}

// The wave's walk over groups and chunks.  Everything that steers a loop (m, flags, the ballots) is wave-uniform.
template <bool LDS> __device__ __forceinline__ void mt_walk(const MtMesh& m, const MtRay& r, int flags, float4* s_tri, float& t_best, int& k_best) {
  const bool cull = (flags & MT_NO_CULL) == 0;
  const bool z_major = __all(r.kz == 2);                                        // every pinhole tile narrower than 90 degrees
  for (int g = 0; g < m.n_groups; ++g) {
    if (cull) {
      const float4 lo = m.gbox[2 * g], hi = m.gbox[2 * g + 1];
      if (lo.x > hi.x || __ballot(mt_slab(lo, hi, r, t_best)) == 0ull) continue;
    }
    const int c1 = min(m.n_chunks, (g + 1) * MT_GROUP);
    for (int c = g * MT_GROUP; c < c1; ++c) {
      bool live = r.ok;
      if (cull) {
        const float4 lo = m.cbox[2 * c], hi = m.cbox[2 * c + 1];
        if (lo.x > hi.x) continue;
        live = mt_slab(lo, hi, r, t_best);
        if (__ballot(live) == 0ull) continue;
      }
      if (z_major) mt_chunk<2, LDS>(m, c, r, live, s_tri, t_best, k_best);
      else         mt_chunk<-1, LDS>(m, c, r, live, s_tri, t_best, k_best);
    }
  }
}

struct MtRaysArgs {
  const float* rays_o; const float* rays_d; long R; float t_max; int flags;
  float* depth; int* face_id; float* positions; float* normals;
};

// 64 consecutive rays per wave
template <bool LDS> __global__ __launch_bounds__(64) void mesh_trace_rays_kernel(MtMesh m, MtRaysArgs a) {
  __shared__ float4 s_tri[LDS ? 3 * MT_CHUNK : 1];
  const long i = (long)blockIdx.x * 64 + threadIdx.x;
  const bool in = i < a.R;
  float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
  if (in) {
#pragma unroll
    for (int j = 0; j < 3; ++j) { o[j] = a.rays_o[3 * i + j]; d[j] = a.rays_d[3 * i + j]; }
  }
  const MtRay r = mt_ray(o[0], o[1], o[2], d[0], d[1], d[2], in);
  float t = a.t_max;
  int k = -1;
  mt_walk<LDS>(m, r, a.flags, s_tri, t, k);
  if (!in) return;
  float pos[3] = {0.f, 0.f, 0.f}, nrm[3] = {0.f, 0.f, 0.f};
  int id = -1;
  if (k >= 0) {
    const float4 va = m.tri[3l * k], vb = m.tri[3l * k + 1], vc = m.tri[3l * k + 2];
    id = __float_as_int(va.w);
    pos[0] = o[0] + t * d[0]; pos[1] = o[1] + t * d[1]; pos[2] = o[2] + t * d[2];
    const float e1x = vb.x - va.x, e1y = vb.y - va.y, e1z = vb.z - va.z, e2x = vc.x - va.x, e2y = vc.y - va.y, e2z = vc.z - va.z;
    float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const float big = fmaxf(fabsf(nx), fmaxf(fabsf(ny), fabsf(nz)));            // > 0: mesh_prepare_kernel dropped the others
    nx = nx / big; ny = ny / big; nz = nz / big;                                // (no underflow in the squares)
    const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
    nrm[0] = nx / len; nrm[1] = ny / len; nrm[2] = nz / len;
  }
  a.depth[i] = t;
  if (a.face_id != nullptr) a.face_id[i] = id;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    if (a.positions != nullptr) a.positions[3 * i + j] = pos[j];
    if (a.normals != nullptr) a.normals[3 * i + j] = nrm[j];
  }
}

struct MtPinholeArgs {
  float fx, fy, cx, cy, off; int H, W; const unsigned char* mask; float t_max, miss_value; int flags;
  float* depth; unsigned char* hit;
};

// one 8 x 8 pixel tile per wave; the ray of pixel (x, y) is d = (((x + off) - cx) / fx, -(((y + off) - cy) / fy), -1) from the origin
template <bool LDS> __global__ __launch_bounds__(64) void mesh_trace_pinhole_kernel(MtMesh m, MtPinholeArgs a) {
  __shared__ float4 s_tri[LDS ? 3 * MT_CHUNK : 1];
  const int x = blockIdx.x * 8 + (threadIdx.x & 7), y = blockIdx.y * 8 + (threadIdx.x >> 3);
  const bool in = x < a.W && y < a.H;
  const long p = (long)y * a.W + x;
  const bool traced = in && (a.mask == nullptr || a.mask[3 * p] > 0);
  const float dx = (((float)x + a.off) - a.cx) / a.fx, dy = -((((float)y + a.off) - a.cy) / a.fy);
  const MtRay r = mt_ray(0.f, 0.f, 0.f, dx, dy, -1.f, traced);
  float t = a.t_max;
  int k = -1;
  if (__ballot(traced) != 0ull) mt_walk<LDS>(m, r, a.flags, s_tri, t, k);
  if (!in) return;
  a.depth[p] = !traced ? 0.f : (k >= 0 ? t : a.miss_value);
  if (a.hit != nullptr) {
    const unsigned char h = k >= 0 ? 255 : 0;
    a.hit[3 * p] = h; a.hit[3 * p + 1] = h; a.hit[3 * p + 2] = h;
  }
}

static inline bool mt_ws_ok(const void* ws, int F) { return F == 0 || (ws != nullptr && ((uintptr_t)ws & 15) == 0); }

extern "C" int snerf_mesh_trace(const void* ws, int F, const float* rays_o, const float* rays_d, long R, float t_max, int flags, float* depth,
                                int* face_id, float* positions, float* normals, void* stream) {
  if (F < 0 || R < 0 || !(t_max > 0.f) || !isfinite(t_max) || (flags & ~(MT_NO_CULL | MT_UNIFORM)) != 0) return SNERF_ERR_ARG;
  if (R == 0) return SNERF_OK;
  if (rays_o == nullptr || rays_d == nullptr || depth == nullptr || !mt_ws_ok(ws, F)) return SNERF_ERR_ARG;
  const long blocks = (R + 63) / 64;
  if (blocks > 0x7fffffffl) return SNERF_ERR_ARG;
  const MtMesh m = mt_views((void*)ws, F);
  MtRaysArgs a;
  a.rays_o = rays_o; a.rays_d = rays_d; a.R = R; a.t_max = t_max; a.flags = flags;
  a.depth = depth; a.face_id = face_id; a.positions = positions; a.normals = normals;
  hipStream_t st = (hipStream_t)stream;
  if (flags & MT_UNIFORM) hipLaunchKernelGGL(mesh_trace_rays_kernel<false>, dim3((unsigned)blocks), dim3(64), 0, st, m, a);
  else                    hipLaunchKernelGGL(mesh_trace_rays_kernel<true>, dim3((unsigned)blocks), dim3(64), 0, st, m, a);
  return snerf_check_launch();
}

extern "C" int snerf_mesh_trace_pinhole(const void* ws, int F, float fx, float fy, float cx, float cy, int pixel_center, int H, int W,
                                        const void* mask, float t_max, float miss_value, int flags, float* depth, void* hit, void* stream) {
  if (F < 0 || H < 0 || W < 0 || !(t_max > 0.f) || !isfinite(t_max) || (flags & ~(MT_NO_CULL | MT_UNIFORM)) != 0) return SNERF_ERR_ARG;
  if ((long)H * W > 0x7fffffffl) return SNERF_ERR_ARG;
  if (!isfinite(fx) || !isfinite(fy) || fx == 0.f || fy == 0.f || !isfinite(cx) || !isfinite(cy)) return SNERF_ERR_ARG;
  if (H == 0 || W == 0) return SNERF_OK;
  if (depth == nullptr || !mt_ws_ok(ws, F)) return SNERF_ERR_ARG;
  const unsigned gx = (unsigned)((W + 7) / 8), gy = (unsigned)((H + 7) / 8);
  if (gy > 65535u) return SNERF_ERR_ARG;
  const MtMesh m = mt_views((void*)ws, F);
  MtPinholeArgs a;
  a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.off = pixel_center ? 0.5f : 0.f; a.H = H; a.W = W; a.mask = (const unsigned char*)mask;
  a.t_max = t_max; a.miss_value = miss_value; a.flags = flags; a.depth = depth; a.hit = (unsigned char*)hit;
  hipStream_t st = (hipStream_t)stream;
  if (flags & MT_UNIFORM) hipLaunchKernelGGL(mesh_trace_pinhole_kernel<false>, dim3(gx, gy), dim3(64), 0, st, m, a);
  else                    hipLaunchKernelGGL(mesh_trace_pinhole_kernel<true>, dim3(gx, gy), dim3(64), 0, st, m, a);
  return snerf_check_launch();
}

// ---- the renderer: instance image and mask of mesh_renderer.py:render ------------------------------------------------------------------------
// Reference counterpart: s-nerfpp/api_code/mesh_renderer.py:36-88 (nvdiffrast rasterize + interpolate, kaolin camera; neither library is in
// the reference tree, so their fill rule at an edge and their near plane are not pinned).  Visibility is mesh_trace_pinhole_kernel's with
// pixel centres: the same ray arithmetic and the same walk, so hit / miss / face are its bits.  The winning record is then intersected
// once more with mt_hit's sheared edge functions; (u, v, w) / ((u + v) + w) are the barycentrics of (a, b, c) at the hit point in 3-D,
// i.e. perspective-correct.  Attributes: vertex colours through the ordered faces, or uvs through face_uvs_idx and one bilinear fetch
// that follows grid_sample(mode = 'bilinear', align_corners = False, padding_mode = 'border') operation by operation.  Every index is
// checked before it is used.  Frame validity (mesh_renderer.py:44-53): one record per wave with plain stores, a one-block reduction in
// a fixed order, a finishing launch that clears an invalid frame: no atomics, no host read.
#define MT_REC_TOP 1
#define MT_REC_BOTTOM 2
#define MT_REC_LEFT 4
#define MT_REC_RIGHT 8
#define MT_SCRATCH_HEAD 16      // bytes in front of the tile records: the verdict (int; 1 = the frame is cleared)

struct MtRenderArgs {
  float fx, fy, cx, cy; int H, W; float t_max, miss_value; int flags;
  const int* faces; const float* vcolor; int V;                               // vertex-colour mode (vcolor != nullptr)
  const float* uvs; int U; const int* face_uvs; const int* face_mat;          // texture mode
  const float4* texels; long n_texels; const int4* mats; int M;               // texels (r, g, b, 0); mats[i] = (texel offset, Hm, Wm, 0)
  int2* records;                                                              // per tile (hit count, border bits), or nullptr
  unsigned char* image; float* image_f; unsigned char* mask; float* depth; int* face_id;
};

// the barycentrics of (a, b, c) for a record the ray has hit: mt_hit's arithmetic, runtime axis
__device__ __forceinline__ void mt_bary(const float4 a, const float4 b, const float4 c, const MtRay& r, float& b0, float& b1, float& b2) {
  float ax, ay, az, bx, by, bz, cx, cy, cz;
  mt_perm<-1>(r.kz, a.x - r.ox, a.y - r.oy, a.z - r.oz, ax, ay, az);
  mt_perm<-1>(r.kz, b.x - r.ox, b.y - r.oy, b.z - r.oz, bx, by, bz);
  mt_perm<-1>(r.kz, c.x - r.ox, c.y - r.oy, c.z - r.oz, cx, cy, cz);
  ax = ax - r.sx * az; ay = ay - r.sy * az;
  bx = bx - r.sx * bz; by = by - r.sy * bz;
  cx = cx - r.sx * cz; cy = cy - r.sy * cz;
  const float u = cx * by - cy * bx, v = ax * cy - ay * cx, w = bx * ay - by * ax;
  const float det = (u + v) + w;                                                // != 0: the record was accepted
  b0 = u / det; b1 = v / det; b2 = w / det;
}

// grid_sample's bilinear fetch with border padding at (u, v) in [0, 1]^2 coordinates: gx = 2u - 1, gy = -(2v - 1)
__device__ __forceinline__ void mt_texture(const float4* __restrict__ tex, int Hm, int Wm, float u, float v, float& cr, float& cg, float& cb) {
  const float gx = u * 2.f - 1.f, gy = -(v * 2.f - 1.f);
  float ix = ((gx + 1.f) * (float)Wm - 1.f) / 2.f, iy = ((gy + 1.f) * (float)Hm - 1.f) / 2.f;
  ix = fminf(fmaxf(ix, 0.f), (float)(Wm - 1)); iy = fminf(fmaxf(iy, 0.f), (float)(Hm - 1));       // (a NaN becomes 0)
  const float fx0 = floorf(ix), fy0 = floorf(iy);
  const int x0 = (int)fx0, y0 = (int)fy0, x1 = x0 + 1, y1 = y0 + 1;
  const float wx1 = ix - fx0, wx0 = (fx0 + 1.f) - ix, wy1 = iy - fy0, wy0 = (fy0 + 1.f) - iy;
  const float wgt[4] = {wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1};           // nw, ne, sw, se: grid_sample's order of accumulation
  const int tx[4] = {x0, x1, x0, x1}, ty[4] = {y0, y0, y1, y1};
  cr = 0.f; cg = 0.f; cb = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (tx[j] >= 0 && tx[j] < Wm && ty[j] >= 0 && ty[j] < Hm) {               // a tap outside the map contributes nothing
      const float4 s = tex[(long)ty[j] * Wm + tx[j]];
      cr = cr + s.x * wgt[j]; cg = cg + s.y * wgt[j]; cb = cb + s.z * wgt[j];
    }
  }
}

__device__ __forceinline__ unsigned char mt_u8(float c) { return (unsigned char)floorf(255.f * c + 0.5f); }   // c in [0, 1]

// one 8 x 8 pixel tile per wave, pixel centres: the rays and the walk of mesh_trace_pinhole_kernel with off = 0.5 and no mask
template <bool LDS> __global__ __launch_bounds__(64) void mesh_render_pinhole_kernel(MtMesh m, MtRenderArgs a) {
  __shared__ float4 s_tri[LDS ? 3 * MT_CHUNK : 1];
  const int x = blockIdx.x * 8 + (threadIdx.x & 7), y = blockIdx.y * 8 + (threadIdx.x >> 3);
  const bool in = x < a.W && y < a.H;
  const long p = (long)y * a.W + x;
  const float dx = (((float)x + 0.5f) - a.cx) / a.fx, dy = -((((float)y + 0.5f) - a.cy) / a.fy);
  const MtRay r = mt_ray(0.f, 0.f, 0.f, dx, dy, -1.f, in);
  float t = a.t_max;
  int k = -1;
  mt_walk<LDS>(m, r, a.flags, s_tri, t, k);                                     // (every tile has a pixel inside the frame)
  const bool hit = in && k >= 0;
  if (a.records != nullptr) {
    const unsigned long long all = __ballot(hit);
    const int bits = (__ballot(hit && y == 0) != 0ull ? MT_REC_TOP : 0) | (__ballot(hit && y == a.H - 1) != 0ull ? MT_REC_BOTTOM : 0)
                     | (__ballot(hit && x == 0) != 0ull ? MT_REC_LEFT : 0) | (__ballot(hit && x == a.W - 1) != 0ull ? MT_REC_RIGHT : 0);
    if (threadIdx.x == 0) a.records[(long)blockIdx.y * gridDim.x + blockIdx.x] = make_int2(__popcll(all), bits);
  }
  if (!in) return;
  float c[3] = {0.f, 0.f, 0.f};
  int id = -1;
  if (hit) {
    const float4 va = m.tri[3l * k], vb = m.tri[3l * k + 1], vc = m.tri[3l * k + 2];
    id = __float_as_int(va.w);
    float b0, b1, b2;
    mt_bary(va, vb, vc, r, b0, b1, b2);
    if (a.vcolor != nullptr) {
      const int i0 = a.faces[3l * k], i1 = a.faces[3l * k + 1], i2 = a.faces[3l * k + 2];
      if (i0 >= 0 && i0 < a.V && i1 >= 0 && i1 < a.V && i2 >= 0 && i2 < a.V) {  // (a hit record passed this check in mesh_prepare_kernel already)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[j] = (b0 * a.vcolor[3l * i0 + j] + b1 * a.vcolor[3l * i1 + j]) + b2 * a.vcolor[3l * i2 + j];
      }
    } else {
      float uv[3][2];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int iu = a.face_uvs[3l * k + j];
        const bool ok = iu >= 0 && iu < a.U;                                    // outside: the reference's appended zero row
        uv[j][0] = ok ? a.uvs[2l * iu] : 0.f; uv[j][1] = ok ? a.uvs[2l * iu + 1] : 0.f;
      }
      const float tu = (b0 * uv[0][0] + b1 * uv[1][0]) + b2 * uv[2][0], tv = (b0 * uv[0][1] + b1 * uv[1][1]) + b2 * uv[2][1];
      const int mi = a.face_mat[k];
      if (mi >= 0 && mi < a.M) {                                                // outside: no material matches, the colour stays 0
        const int4 mt = a.mats[mi];
        if (mt.x >= 0 && mt.y >= 1 && mt.z >= 1 && (long)mt.x + (long)mt.y * mt.z <= a.n_texels)
          mt_texture(a.texels + mt.x, mt.y, mt.z, tu, tv, c[0], c[1], c[2]);
      }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) c[j] = fminf(fmaxf(c[j], 0.f), 1.f);            // clamp(img, 0, 1); a NaN becomes 0
  }
  const unsigned char mk = hit ? 255 : 0;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    a.image[3 * p + j] = mt_u8(c[j]);
    if (a.image_f != nullptr) a.image_f[3 * p + j] = c[j];
    if (a.mask != nullptr) a.mask[3 * p + j] = mk;
  }
  if (a.depth != nullptr) a.depth[p] = hit ? t : a.miss_value;
  if (a.face_id != nullptr) a.face_id[p] = id;
}

// one block: the tile records in a fixed order -> verdict (mesh_renderer.py:44-53; the area rule as the integer 2 count > H W)
__global__ __launch_bounds__(256) void mesh_render_verdict_kernel(const int2* __restrict__ records, long n_tiles, long HW, int* verdict) {
  __shared__ int s_count[256], s_bits[256];
  int count = 0, bits = 0;                                                      // count <= H W < 2^31
  for (long i = threadIdx.x; i < n_tiles; i += 256) { const int2 rec = records[i]; count += rec.x; bits |= rec.y; }
  s_count[threadIdx.x] = count; s_bits[threadIdx.x] = bits;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) { s_count[threadIdx.x] += s_count[threadIdx.x + o]; s_bits[threadIdx.x] |= s_bits[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int b = s_bits[0];
    const bool bad = ((b & MT_REC_TOP) && (b & MT_REC_BOTTOM)) || ((b & MT_REC_LEFT) && (b & MT_REC_RIGHT)) || 2l * s_count[0] > HW;
    *verdict = bad ? 1 : 0;
  }
}

// an invalid frame: every output as if nothing had been hit
__global__ __launch_bounds__(256) void mesh_render_finish_kernel(const int* __restrict__ verdict, long HW, float miss_value, unsigned char* image,
                                                                 float* image_f, unsigned char* mask, float* depth, int* face_id) {
  if (*verdict == 0) return;
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    image[3 * p + j] = 0;
    if (image_f != nullptr) image_f[3 * p + j] = 0.f;
    if (mask != nullptr) mask[3 * p + j] = 0;
  }
  if (depth != nullptr) depth[p] = miss_value;
  if (face_id != nullptr) face_id[p] = -1;
}

extern "C" long snerf_mesh_render_scratch_bytes(int H, int W) {
  if (H <= 0 || W <= 0) return 0;
  return MT_SCRATCH_HEAD + (long)((H + 7) / 8) * ((W + 7) / 8) * (long)sizeof(int2);
}

extern "C" int snerf_mesh_render_pinhole(const void* ws, int F, float fx, float fy, float cx, float cy, int H, int W, float t_max, float miss_value,
                                         int flags, const int* faces, const float* vertex_color, int V, const float* uvs, int U,
                                         const int* face_uvs_idx, const int* face_material_idx, const void* texels, long n_texels,
                                         const int* materials, int M, int validate, void* scratch, long scratch_bytes, void* image,
                                         float* image_f, void* mask, float* depth, int* face_id, void* stream) {
  if (F < 0 || H < 0 || W < 0 || V < 0 || U < 0 || n_texels < 0 || !(t_max > 0.f) || !isfinite(t_max) || (flags & ~(MT_NO_CULL | MT_UNIFORM)) != 0)
    return SNERF_ERR_ARG;
  if ((long)H * W > 0x7fffffffl) return SNERF_ERR_ARG;
  if (!isfinite(fx) || !isfinite(fy) || fx == 0.f || fy == 0.f || !isfinite(cx) || !isfinite(cy)) return SNERF_ERR_ARG;
  if (F > 0) {                                                                  // the attribute source: exactly one mode, complete
    const bool colours = vertex_color != nullptr, textures = face_uvs_idx != nullptr;
    if (colours == textures) return SNERF_ERR_ARG;
    if (colours && faces == nullptr) return SNERF_ERR_ARG;
    if (textures && (M < 1 || materials == nullptr || face_material_idx == nullptr || (uvs == nullptr && U > 0) || (texels == nullptr && n_texels > 0)
                     || ((uintptr_t)texels & 15) != 0 || ((uintptr_t)materials & 15) != 0))
      return SNERF_ERR_ARG;
  }
  if (H == 0 || W == 0) return SNERF_OK;
  if (image == nullptr || !mt_ws_ok(ws, F)) return SNERF_ERR_ARG;
  if (validate && (scratch == nullptr || ((uintptr_t)scratch & 7) != 0 || scratch_bytes < snerf_mesh_render_scratch_bytes(H, W))) return SNERF_ERR_ARG;
  const unsigned gx = (unsigned)((W + 7) / 8), gy = (unsigned)((H + 7) / 8);
  if (gy > 65535u) return SNERF_ERR_ARG;
  const MtMesh m = mt_views((void*)ws, F);
  MtRenderArgs a;
  a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.H = H; a.W = W; a.t_max = t_max; a.miss_value = miss_value; a.flags = flags;
  a.faces = faces; a.vcolor = vertex_color; a.V = V; a.uvs = uvs; a.U = U; a.face_uvs = face_uvs_idx; a.face_mat = face_material_idx;
  a.texels = (const float4*)texels; a.n_texels = n_texels; a.mats = (const int4*)materials; a.M = M;
  a.records = validate ? (int2*)((char*)scratch + MT_SCRATCH_HEAD) : nullptr;
  a.image = (unsigned char*)image; a.image_f = image_f; a.mask = (unsigned char*)mask; a.depth = depth; a.face_id = face_id;
  hipStream_t st = (hipStream_t)stream;
  if (flags & MT_UNIFORM) hipLaunchKernelGGL(mesh_render_pinhole_kernel<false>, dim3(gx, gy), dim3(64), 0, st, m, a);
  else                    hipLaunchKernelGGL(mesh_render_pinhole_kernel<true>, dim3(gx, gy), dim3(64), 0, st, m, a);
  if (validate) {
    const long HW = (long)H * W;
    hipLaunchKernelGGL(mesh_render_verdict_kernel, dim3(1), dim3(256), 0, st, a.records, (long)gx * gy, HW, (int*)scratch);
    hipLaunchKernelGGL(mesh_render_finish_kernel, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, st, (const int*)scratch, HW, miss_value, a.image,
                       image_f, a.mask, depth, face_id);
  }
  return snerf_check_launch();
}
