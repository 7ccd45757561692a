/* libsnerf_hip -- C ABI of the MI355X (gfx950) volumetric-render hot path.
 *
 * Drop-in boundary for the S-NeRF background renderer.
 * The reference has exactly one native interface -- the pybind module of
 * s-nerfpp/zipnerf/gridencoder (src/bindings.cpp:5-9, src/gridencoder.h:12-15)
 * -- and otherwise runs PyTorch eager ops; every entry point below names the
 * reference function (file:line under /root/reference) it replaces.
 *
 * Conventions
 *   - plain C: raw DEVICE pointers, explicit sizes/strides (in elements),
 *     `stream` is a hipStream_t passed as void* (0 = default stream);
 *   - the caller allocates everything, the callee writes in place, nothing is
 *     returned but a status: 0 ok, 1 bad argument, 2 launch failure; no
 *     exceptions cross the ABI, no hidden global state, thread-safe per stream;
 *   - `dtype`: 0 = fp32 activations/weights (exact-parity mode, fp32 MFMA),
 *     1 = bf16 activations/weights with fp32 accumulation;
 *   - all launches are asynchronous on `stream`.
 */
#ifndef SNERF_HIP_H
#define SNERF_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

#define SNERF_DT_F32 0
#define SNERF_DT_BF16 1
#define SNERF_DT_F16 2 /* hash-grid tables; the fp16 compute mode of path C (GEMMs: fp16 operands on the f16 MFMA, fp32 accumulation; features, activations, packed weights) */
#define SNERF_DT_F64 3 /* stand-alone GridEncoder operator only (the reference dispatches float / double / half) */
#define SNERF_DT_BF16X3 4 /* snerf_linear_fwd / snerf_linear_wgrad only: split-bf16 operands (the fp32-parity mode at bf16 MFMA rates) */
#define SNERF_ACT_NONE 0
#define SNERF_ACT_RELU 1
#define SNERF_ACT_MASK 2 /* y = aux > 0 ? y : 0 : ReLU backward fused into the data-gradient GEMM */
#define SNERF_ACT_RELU_BITS 3 /* ReLU; `aux` (uint32 words, OUTPUT) also receives one bit per element (y > 0) */
#define SNERF_ACT_MASK_BITS 4 /* as SNERF_ACT_MASK with `aux` = the words an ACT_RELU_BITS launch of the same [M, N] wrote */

int snerf_version(void);
/* the hipError_t (as int) that the most recent "kernel launch failure" status (2) of any entry stood for; 0 if there was none */
int snerf_last_hip_error(void);
/* Test utility (tests/test_stale_lds.py): fills the LDS of every CU with a seeded pseudo-random pattern.  LDS content survives from one
 * kernel to the next; a kernel that reads LDS before its own write / DMA has landed shows up as a result that depends on `seed`. */
int snerf_debug_lds_scribble(int seed, void* stream);

/* ---- tiny-MLP layers (MFMA GEMMs) ------------------------------------------------------------
 * Y[M, n_store] = act(A[M,K] . W[N,K]^T + bias).  Replaces nn.Linear(+ReLU):
 *   s-nerf/model/models.py:200-214 (DenseBlock), :232-255 (MLP), :307-315 (proposal),
 *   s-nerf/model/run_nerf_helpers.py:86-126 (NeRF), called through run_network :460-474.
 * W is the packed weight [N (multiple of 128), K] in `dtype`; K a multiple of 64 (bf16) / 32 (fp32)
 * with zero padding; lda/ldw multiples of 8/4; Y is `dtype` or fp32 (out_f32).  With W := W^T the
 * same entry computes the data gradient; ACT_MASK applies the ReLU mask from `aux` and `colsum`
 * (fp32 [n_store], accumulated) receives the column sums = bias gradient of the layer below; `colsum_ws`
 * (fp32 [max(2*ceil(M/128), 2*min(ceil(M/256)*(N/256), 1024)), N], contents irrelevant) lets that reduction run without atomics:
 * one partial row per 128-row slab, or -- persistent kernel -- one per (workgroup, wave row), kept in registers across its tiles.
 * The two *_BITS activations carry the ReLU mask of a training step as 1 bit per element (8*ceil(M/256) * N/64 blocks of 64
 * words; word l of block (32-row block, 64-column group) = rows 8*it + l/8, columns 8*(l%8) + e at bit 8*it + e): 1/16 of the
 * bytes of the activation and DMA-able ahead of use.  Only the persistent kernel implements them (bf16, variant 8,
 * N % 256 == 0, K >= 128, 16-byte aligned Y rows); other launches return SNERF_ERR_ARG.
 * variant (low nibble): 0 = 128x128 tile, 1 = 256x256 tile, 4 = 256x256 8-phase, 8 = 256x256 persistent 8-phase (bf16,
 * N % 256 == 0, K >= 128, 16-byte epilogue; other shapes fall back to 4, then 0); higher bits = ablation switches, except
 * bit 14 (0x4000; dtype bf16, ACT_MASK): `aux` is an activation a split-bf16 (SNERF_DT_BF16X3) forward saved -- interleaved hi / lo per 64
 * columns -- while A, W and Y are plain bf16: the single-pass data gradient behind a three-pass forward (compute="bf16x3_fwd"). */
int snerf_linear_fwd(const void* A, long lda, const void* W, long ldw, const float* bias, void* Y, long ldy,
                     const void* aux, long ldaux, float* colsum, float* colsum_ws, int M, int N, int K, int n_store,
                     int act, int dtype, int out_f32, int variant, void* stream);

/* dW[n_valid, k_valid] (fp32, ldw) += dZ[M,N]^T . X[M,K]  -- weight gradient of the same layers
 * (autograd of nn.Linear in the reference; train.py:213 loss.backward()).  `zeros` = >=16 bytes of
 * device zeros (source for rows past M).  variant bit 1 (bf16, N and K multiples of 128): transposing LDS reads; bit 2 (bf16,
 * N % 256 == 0, K >= 256): the 256 x 256 8-phase kernel; bits 16 / 32 / 64: probe only -- 1024 / 2048 / 4096 M-slices for the
 * 128 x 128 kernel instead of its default of about 512 (tools/gemm_tn_slices_probe.py); bit 14 (0x4000; dtype bf16): X is an activation a
 * split-bf16 forward saved ([M, >= 2 K], hi / lo interleaved per 64 columns) and its hi half is multiplied, K = its LOGICAL width, dZ plain bf16. */
int snerf_linear_wgrad(const void* Z, long ldz, const void* X, long ldx, float* dW, long ldw, const void* zeros,
                       int M, int N, int K, int n_valid, int k_valid, int dtype, int variant, void* stream);

/* ---- encoders ---------------------------------------------------------------------------------
 * Classic positional encoding written straight into MLP operand buffers.
 *   run_nerf_helpers.py:22-70 (Embedder.embed: [x, sin(2^k x), cos(2^k x)]_k) and the per-sample
 *   broadcast of the view direction in run_network (:465-469).
 * pts [M,3]; viewdirs [N,3] rows vd_stride apart (NULL = no view branch); S samples per ray.
 * dst1/dst2 (dst2 optional) get w_pts columns (3+6L values + zero pad); dstv gets w_views columns. */
int snerf_classic_embed(const float* pts, const float* viewdirs, int vd_stride, int S, long M, int L, int Lv,
                        void* dst1, long ld1, void* dst2, long ld2, int w_pts, void* dstv, long ldv, int w_views,
                        int dtype, void* stream);

/* mip path: s -> t (mip.py:7-9) -> cast_rays cone/cylinder (mip.py:80-91, 56-77, 31-53) -> contraction
 * fn2 + Jacobi_g (mip.py:343-374) -> diagonal of J diag(c) J^T (mip.py:381-395) -> integrated_pos_enc
 * (mip.py:94-118, 24-28; math_ops.py:6-12), `width` >= 6*max_deg columns (zero padded) into dst1 (and dst2).
 * means_out/covs_out: optional fp32 [N*S,3] copies of the contracted mean / covariance diagonal.
 * `cone`: bit 0 = ray shape (1 cone, 0 cylinder); bit 1 = --disable_integration (models.py:132-133: the covariances are replaced by zeros
 * before the encoding; the backward entries take the same value). */
int snerf_mip_encode(const float* s_vals, const float* origins, const float* directions, const float* radii,
                     const float* near, const float* far, long n_rays, int S, int cone, int transform_idx, int max_deg,
                     void* dst1, long ld1, void* dst2, long ld2, int width, float* means_out, float* covs_out,
                     int dtype, const int* sample_id, long n_rows, void* stream);

/* The same with the warp of sample2enc selected (mip.py:367-378 warp_fn, model argument `fn`): fn_idx 1 = the contraction above,
 * fn_idx 0 = the view-centred warp fn1 (x - viewc) / sqrt(|x - viewc| far) (mip.py:368-369) with Jacobi_f (mip.py:323-340:
 * (l I - x x^T) / l^1.5 / sqrt(max far), l = |x| + 1e-5 at the unshifted mean).  (vx, vy, vz) = viewc, the mean camera centre
 * (train.py:36, eval.py:50); far_max: DEVICE scalar = max over the batch of rays.far (ignored for fn_idx 1). */
int snerf_mip_encode_warp(const float* s_vals, const float* origins, const float* directions, const float* radii,
                          const float* near, const float* far, long n_rays, int S, int cone, int transform_idx, int max_deg,
                          void* dst1, long ld1, void* dst2, long ld2, int width, float* means_out, float* covs_out,
                          int dtype, const int* sample_id, long n_rows, int fn_idx, float vx, float vy, float vz,
                          const float* far_max, void* stream);

/* mip.py:12-21 pos_enc(viewdirs, 0, deg, append_identity) tiled per sample (models.py:285-287). */
int snerf_mip_viewenc(const float* viewdirs, long n_rays, int S, int deg, void* dst, long ld, int width, int dtype,
                      const int* sample_id, long n_rows, void* stream);

/* ---- samplers (bit-exact interval indices; fp64 sequential accumulation per ray) -----------------
 * run_nerf_helpers.py:336-379 sample_pdf.  nc = number of bins = cdf entries, nc-1 weights (rows ld_w apart).
 * mid_mode 1 = the render_rays call (render.py:378-380): `bins` is z_vals [N,nc+1] (bin j = mid of z[j],z[j+1]) and
 * `weights` points at weights[:,1]; mid_mode 0: bins [N,nc] as given.  u [N,Nf] rows u_stride apart (0 = shared row).
 * inds (int32, nullable) = searchsorted(cdf,u,right); z_std (nullable) = std(samples,-1,unbiased=False) (render.py:405). */
int snerf_classic_sample_pdf(const float* bins, long ld_bins, int mid_mode, const float* weights, long ld_w, int nc,
                             const float* u, long u_stride, long N, int Nf, float* samples, int* inds, float* z_std,
                             void* stream);
/* math_ops.py:50-54 (randomized branch of sorted_piecewise_constant_pdf): u = min(arange(P) * s + jit, 1 - eps) in place over the
 * uniform draw jit [N, P] (torch's own RNG launch stays the caller's, so the draws are the reference's); one launch, same roundings. */
int snerf_jitter_u(float* u, long N, int P, float s, void* stream);
/* render.py:354/:385  pts = rays_o[...,None,:] + rays_d[...,None,:] * z_vals[...,:,None]; rays rows = [o3,d3,...]. */
int snerf_classic_points(const float* rays, int ray_stride, const float* z_vals, long N, int S, float* pts, void* stream);
/* render.py:383 torch.sort(torch.cat([z_vals, z_samples], -1), -1) */
int snerf_classic_merge_sort(const float* a, int na, const float* b, int nb, long N, float* out, void* stream);
/* mip.py:294-316 blur-pool + resample_padding, then math_ops.py:19-76 sorted_piecewise_constant_pdf.
 * idx_out (int32, nullable) = #(u >= cdf) - 1. */
int snerf_mip_resample(const float* s_vals, const float* weights, const float* u, long u_stride, long N, int S, int Nf,
                       float resample_padding, float* out, int* idx_out, void* stream);
/* render.py:330-352 (mode 0: z = near(1-t)+far t or disparity) / mip.py:268-288 (mode 1: s = t) with optional
 * stratified jitter rnd [N,P]; base [P] = linspace(0,1,P). */
int snerf_stratified(const float* base, const float* rnd, const float* near, const float* far, int nf_stride, long N,
                     int P, int mode, int lindisp, float* out, void* stream);

/* ---- compositing --------------------------------------------------------------------------------
 * models.py:166-175 activations + mip.py:151-189 real_volumetric_rendering.  raw_rgb NULL = proposal level. 
 * g_dirs (nullable) [N,3] <- d loss / d directions through delta = (t1 - t0) * |d| (mip.py:160-161; the reference's pose refinement). */
int snerf_mip_composite_fwd(const float* raw_rgb, long ld_rgb, const float* raw_density, long ld_den, const float* noise,
                            const float* s_vals, const float* dirs, const float* near, const float* far, long N, int S,
                            int transform_idx, int white, float rgb_padding, float density_bias, float* comp_rgb,
                            float* distance, float* acc, float* weights, const int* row_index, void* stream);
int snerf_mip_composite_bwd(const float* raw_rgb, long ld_rgb, const float* raw_density, long ld_den, const float* noise,
                            const float* s_vals, const float* dirs, const float* near, const float* far, long N, int S,
                            int transform_idx, int white, float rgb_padding, float density_bias, const float* weights,
                            const float* distance, const float* g_rgb, const float* g_dist, const float* g_acc,
                            const float* g_w, float* d_raw_rgb, long ld_drgb, float* d_raw_density, long ld_dden,
                            float* g_dirs, void* stream);
/* run_nerf_helpers.py:381-424 raw2outputs */
int snerf_classic_composite_fwd(const float* raw, long ld, const float* noise, const float* z_vals, const float* rays_d,
                                int rd_stride, long N, int S, int white, float* rgb_map, float* disp_map, float* acc_map,
                                float* weights, float* depth_map, void* stream);
int snerf_classic_composite_bwd(const float* raw, long ld, const float* noise, const float* z_vals, const float* rays_d,
                                int rd_stride, long N, int S, int white, const float* weights, const float* acc_map,
                                const float* depth_map, const float* g_rgb, const float* g_disp, const float* g_acc,
                                const float* g_depth, const float* g_w, float* d_raw, long ld_draw, void* stream);

/* ---- multiresolution hash-grid encoder (S-NeRF++ / zipnerf) ------------------------------------------------------
 * Same entry points and argument order as the reference's pybind module (s-nerfpp/zipnerf/gridencoder/src/bindings.cpp:5-9,
 * src/gridencoder.h:12-15; kernels src/gridencoder.cu:87-245, :248-340, :343-369, :506-610):
 *   grid_encode_forward(inputs, embeddings, offsets, outputs, B, D, C, L, S, H, dy_dx?, gridtype, align_corners, interp)
 *   grid_encode_backward(grad, inputs, embeddings, offsets, grad_embeddings, B, D, C, L, S, H, dy_dx?, grad_inputs?, ...)
 *   grad_total_variation(inputs, embeddings, grad, offsets, weight, B, D, C, L, S, H, gridtype, align_corners)
 * plus `dtype` of the table / outputs / gradients (SNERF_DT_F32, SNERF_DT_F16 or SNERF_DT_F64; the reference dispatches on the
 * tensor dtype, AT_DISPATCH_FLOATING_TYPES_AND_HALF gridencoder.cu:469), the strides (elements) of the level and point axes of `outputs` / `grad` (reference layout [L,B,C]:
 * stride_l = B*C, stride_b = C; [B, L*C] directly: stride_l = C, stride_b = L*C) and the stream (the reference always
 * uses the legacy default stream).  inputs fp32 [B,D] in [0,1] (out-of-bound points -> zeros); D in {2,3,4,5} (gridencoder.cu:376-399); C in {1,2,4,8};
 * gridtype 0 hash / 1 tiled; interp 0 linear / 1 smoothstep.  grad_embeddings / grad_inputs must arrive zeroed. */
int snerf_grid_encode_fwd(const float* inputs, const void* embeddings, const int* offsets, void* outputs, int B, int D, int C,
                          int L, float S, int H, void* dy_dx, int gridtype, int align_corners, int interp, int dtype,
                          long out_stride_l, long out_stride_b, void* stream);
/* snerf_grid_encode_fwd in kernel_grid's own form (one thread per (point, level), eight independent row loads: gridencoder.cu:87-245) for
 * EVERY instantiation -- the A/B partner of the measurement legs and parity tests.  Same arguments, same results bit for bit.  (A second
 * entry instead of a process-wide switch: no hidden state in the library.) */
int snerf_grid_encode_fwd_ref(const float* inputs, const void* embeddings, const int* offsets, void* outputs, int B, int D, int C,
                              int L, float S, int H, void* dy_dx, int gridtype, int align_corners, int interp, int dtype,
                              long out_stride_l, long out_stride_b, void* stream);
int snerf_grid_encode_bwd(const void* grad, const float* inputs, const void* embeddings, const int* offsets, void* grad_embeddings,
                          int B, int D, int C, int L, float S, int H, const void* dy_dx, void* grad_inputs, int gridtype,
                          int align_corners, int interp, int dtype, long grad_stride_l, long grad_stride_b, void* stream);
int snerf_grid_tv_grad(const float* inputs, const void* embeddings, void* grad, const int* offsets, float weight, int B, int D,
                       int C, int L, float S, int H, int gridtype, int align_corners, int dtype, void* stream);
/* The table gradient of grid_encode_backward (gridencoder.cu:248-340, bindings.cpp:7) WITHOUT atomics on the table, for the instantiations
 * zipnerf constructs (internal/models.py:413-421: D = 3, hash, linear, align_corners = False; C in {1, 2, 4, 8}): runs of consecutive points in one
 * cell become records (row, sum of w x grad), binned by destination row range through an LDS stage (full, aligned lines), accumulated per
 * bin in LDS in 64-bit fixed point (bit-reproducible; sums exact to 2^-31 of the largest |grad|).  ONE call, LEVEL by level and CHUNK of
 * points by chunk: count -> scan -> staged write -> accumulate into the level's int64 image, so that the workspace is bounded whatever B
 * is.  `ws`: 256-byte aligned; ANY size from the smallest feasible layout up works -- the call plans its chunks and (for a [B, L*C]
 * gradient) the number of levels it transposes per sweep from `ws_bytes`; snerf_grid_encode_bwd_binned_ws_bytes(...) returns the
 * recommended size: everything in one chunk when that takes less than 1 GB, else 1 GB (-1 = unsupported level layout: more than 1024
 * row ranges per level); snerf_grid_encode_bwd_binned_plan(...) reports what a given size would run (out[6]: chunks per level, points
 * per chunk, levels per transposed group (0 = none), kernel launches, record capacity of a chunk, bytes used).
 * grad [B, L*C] (stride_l = C, stride_b = L*C) or [L, B, C] (stride_l = B*C, stride_b = C: the layout the reference's backward builds,
 * grid.py:74 -- no transposition sweep) in grad_dtype (F32 / F16); grad_embeddings [sO, C] in out_dtype (F32 / F16), += like the reference
 * (arrives zeroed); offsets_host = the same int32 [L + 1] offsets in host memory (the plan is made on the host); half_records != 0
 * (C = 1 / 4 only): contributions rounded once to fp16 (the reference adds __half2 atomics there). */
/* starts[L, 1024] (int64) = exclusive scan of counts[L, 1024] (int32), flat over levels and bins: the record offsets of the binned table
 * gradient (between its count and write passes), on the device. */
int snerf_zip_bin_scan(const int* counts, long* starts, int L, void* stream);
long snerf_grid_encode_bwd_binned_ws_bytes(long B, int C, int L, const int* offsets_host, int half_records);
int snerf_grid_encode_bwd_binned_plan(long B, int C, int L, const int* offsets_host, int half_records, int grad_dtype, int level_major,
                                      long ws_bytes, long* out);
int snerf_grid_encode_bwd_binned(const void* grad, const float* inputs, const int* offsets, const int* offsets_host, void* grad_embeddings,
                                 long B, int C, int L, float S, int H, int grad_dtype, int out_dtype, long grad_stride_l,
                                 long grad_stride_b, int half_records, void* ws, long ws_bytes, void* stream);

/* ---- S-NeRF++ / zipnerf background model (s-nerfpp/zipnerf/internal) --------------------------------------------------
 * One launch per sampling level: stepfun.max_dilate_weights (stepfun.py:75-105; dilate = 0 skips it, level 0) with the
 * caller's [1:-1] trim (models.py:187-188), the annealed logits (models.py:196-203), stepfun.sample_intervals
 * (stepfun.py:251-294 -> 175-218 -> 154-161 -> 108-128, math.sorted_interp math.py:88-107) at the centres `u` [R,n]
 * (rows u_stride apart, 0 = shared) and the power-transformation ray warp s -> t (coord.py:103-162, lam).  sdist [R,S0+1],
 * weights [R,S0] -> sdist_out / tdist_out [R,n+1].  One wave per ray; at most 256 intervals after the dilation (3*S0 - 2 <= 256,
 * i.e. S0 <= 86; undilated S0 <= 256), SNERF_ERR_ARG beyond. */
int snerf_zip_resample(const float* sdist, const float* weights, int S0, const float* u, long u_stride, int n,
                       const float* near, const float* far, long R, float dilation, int dilate, float anneal,
                       float resample_padding, float lam, float dom0, float dom1, float* sdist_out, float* tdist_out,
                       void* stream);
/* render.cast_rays (render.py:129-168; n multisamples on an m-turn helix, deg_jitter [R,S,n] or NULL) + coord.contract_mean_std
 * (coord.py:51-63) + /2 + GridEncoder forward (gridencoder.cu:87-245, hash type, linear) + erf down-weighting and mean over
 * the multisamples (models.py:488-497) -> feat [R*S, ld] (columns level*C + c; feat_dtype fp32/bf16).  table fp32 or fp16
 * (SNERF_DT_F16); grid_sizes = GridEncoder.grid_sizes; Sl = log2(per_level_scale).  levels_per_thread: 0 / 1 = one thread per
 * (interval, level) (best for scattered training rays: most gathers in flight); L = one thread per interval evaluates its multisamples
 * once for all levels (best for the coherent rays of a frame); values in between group the levels.  Same results. */
int snerf_zip_encode_fwd(const float* tdist, const float* origins, const float* directions, const float* radii,
                         const float* base_x, const float* base_y, const float* deg_jitter, const void* table,
                         const int* offsets, const int* grid_sizes, void* feat, long ld, long R, int S, int L, int C, int n,
                         int m, float Sl, int H, float std_scale, int table_dtype, int feat_dtype, int levels_per_thread, void* stream);
/* snerf_zip_encode_fwd for a training step whose table gradient is the binned reduction (snerf_zip_encode_bwd_binned): one thread per
 * (interval, level), and the same sweep also IS that gradient's pass 0 -- it has the 8 rows of every multisample's cell in hand for its
 * gathers and counts the records the backward will emit per bin (counts [L, 1024], zeroed by the caller) and reserves each workgroup's
 * ranges (wg_offsets [L, ceil(R S / 256), 1024]); ksplit_host / level_rows_host as for snerf_zip_encode_bwd_binned.  The backward then
 * starts at its record pass (1 / 3) with these two buffers.  C = 1 or 4, n <= 8 multisamples. */
int snerf_zip_encode_fwd_count(const float* tdist, const float* origins, const float* directions, const float* radii,
                               const float* base_x, const float* base_y, const float* deg_jitter, const void* table,
                               const int* offsets, const int* grid_sizes, void* feat, long ld, long R, int S, int L, int C, int n,
                               int m, float Sl, int H, float std_scale, int table_dtype, int feat_dtype, const int* ksplit_host,
                               const int* level_rows_host, int* counts, void* wg_offsets, void* stream);
/* The proposal MLP of a zipnerf TRAINING step (internal/models.py:425-427, 481-519 with disable_rgb: Linear(L -> hidden) + ReLU +
 * Linear(hidden -> 1) on the grid features) as one launch each way instead of per-layer GEMMs over 64-column padded buffers: F [P, ldf]
 * (feat_dtype fp32 / bf16, L <= 16 feature columns, ldf >= L -- a compact buffer), parameters fp32 in the reference's layouts
 * (density_layer.0.weight [hidden, L], .bias [hidden], density_layer.2.weight [1, hidden], .bias [1]; hidden <= 64), raw [P] fp32.
 * round_bf16: rounding mode = the rounding points of the GEMM route in that compute dtype (weights and stored activations rounded, fp32
 * accumulation): 0 none (fp32), 1 bf16, 2 fp16 (requires feat_dtype SNERF_DT_F16).  The backward
 * recomputes the hidden activations from F, writes dF [P, lddf] (columns L .. lddf - 1 zero; lddf <= 64) and adds the parameter
 * gradients into g_* (fp32, same layouts) by per-workgroup partial sums folded in a fixed order (bit-reproducible);
 * ws: snerf_zip_prop_mlp_ws_floats(L, hidden, P) floats of scratch. */
int snerf_zip_prop_mlp_ws_floats(int L, int hidden, long P);
int snerf_zip_prop_mlp_fwd(const void* F, long ldf, long P, int L, const float* w1, const float* b1, const float* w2, const float* b2,
                           int hidden, int round_bf16, int feat_dtype, float* raw, void* stream);
int snerf_zip_prop_mlp_bwd(const void* F, long ldf, const float* d_raw, long P, int L, const float* w1, const float* b1,
                           const float* w2, const float* b2, int hidden, int round_bf16, int feat_dtype, void* dF, long lddf,
                           float* g_w1, float* g_b1, float* g_w2, float* g_b2, float* ws, long ws_floats, void* stream);
/* matching scatter-add of grad_feat [R*S, ld] into the fp32 table gradient (gridencoder.cu:248-340 composed with the mean /
 * erf weights); grad_table accumulates (fp32 atomics).  The first `lds_levels` levels (small dense tables) are accumulated
 * in LDS by persistent workgroups, in slabs of `lds_cells` rows (lds_cells*C*4 <= 160 KB; lds_slabs = sum of
 * ceil(rows_l / lds_cells) over those levels), and flushed once.  grad_table_bf16 (nullable, C even): a bf16 [entries, C]
 * buffer that receives the contributions of the remaining (hashed) levels as packed bf16-pair atomics instead -- half the
 * atomic operations (what the reference does with __half2 under autocast, gridencoder.cu:300-330); the caller adds it to the
 * fp32 gradient afterwards. */
int snerf_zip_encode_bwd(const float* tdist, const float* origins, const float* directions, const float* radii,
                         const float* base_x, const float* base_y, const float* deg_jitter, const int* offsets,
                         const int* grid_sizes, const void* grad_feat, long ld, float* grad_table, long R, int S, int L, int C,
                         int n, int m, float Sl, int H, float std_scale, int feat_dtype, int lds_levels, long lds_cells,
                         int lds_slabs, void* grad_table_bf16, void* stream);
/* render.compute_alpha_weights (render.py:170-189, opaque_background) + volumetric_rendering (render.py:192-233: rgb with
 * clamped background weight, depth = clip(exp(E_w[log t_mid]))) fused with density = softplus(raw + bias) (models.py:586)
 * and rgb = sigmoid(raw)(1 + 2 pad) - pad (models.py:689-703).  raw_rgb NULL = proposal level (rgb = 0). */
int snerf_zip_composite_fwd(const float* raw_rgb, long ld_rgb, const float* raw_density, long ld_den, const float* tdist,
                            const float* dirs, long R, int S, int opaque, float bg, float rgb_padding, float density_bias,
                            float* rgb, float* depth, float* acc, float* weights, void* stream);
int snerf_zip_composite_bwd(const float* raw_rgb, long ld_rgb, const float* raw_density, long ld_den, const float* tdist,
                            const float* dirs, long R, int S, int opaque, float bg, float rgb_padding, float density_bias,
                            const float* weights, const float* acc, const float* depth, const float* g_rgb, const float* g_depth,
                            const float* g_acc, const float* g_w, float* d_raw_rgb, long ld_drgb, float* d_raw_density,
                            long ld_dden, float* g_dirs, void* stream);

/* ---- training tail ------------------------------------------------------------------------------
 * torch.optim.Adam step over a flat fp32 arena (model_utils.py:23-34 builds Adam); grad_scale folds the
 * data-parallel 1/world_size; zero_grad clears g for the next step. */
int snerf_adam_step(float* p, float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps, int step,
                    float grad_scale, int zero_grad, void* stream);
/* Appearance embedding (--encode_appearance; s-nerf/model/models.py:63-64, 153-159: condition = cat([view encoding, emb(rays.app)])):
 * snerf_app_embed writes emb[(int)app[ray], :dim] (fp32 table [n_vocab, dim], dim = 48 in the reference) into columns [0, dim) of dst
 * rows ray * S + i (dst: the condition block right of the 27 view-encoding columns; dtype fp32 / bf16; sample_id / rows as in
 * snerf_mip_viewenc); indices are clamped to the table.  snerf_app_embed_bwd accumulates d loss / d emb.weight (+=) from the fp32
 * gradient of those columns, dV [n_rays * S, ld]. */
int snerf_app_embed(const float* emb, const float* app, int n_vocab, long n_rays, int S, int dim, void* dst, long ld, int dtype,
                    const int* sample_id, long rows, void* stream);
int snerf_app_embed_bwd(const float* dV, long ld, const float* app, int n_vocab, long n_rays, int S, int dim, float* g_emb, void* stream);
/* the same accumulation in a fixed order (one workgroup per table row, rays in order; no atomics): bit-reproducible run to run */
int snerf_app_embed_bwd_det(const float* dV, long ld, const float* app, int n_vocab, long n_rays, int S, int dim, float* g_emb, void* stream);
/* bad[0] += number of entries of the float index vector idx [n] that torch.nn.Embedding(n_rows, .) would refuse after .long() (outside
 * [0, n_rows) or not finite); the kernels themselves clamp.  The host polls the counter later and raises (no sync inside the step). */
int snerf_index_check(const float* idx, long n, int n_rows, int* bad, void* stream);

/* Split-bf16 operands (dtype SNERF_DT_BF16X3 of snerf_linear_fwd / snerf_linear_wgrad): a value x is carried as hi = bf16(x) and
 * lo = bf16(x - hi) (16 mantissa bits) and a product evaluated as hi.hi + lo.hi + hi.lo on the bf16 MFMA path with fp32 accumulation
 * -- the arithmetic of the reference (fp32, s-nerf/model/models.py) to ~2^-16 relative per product at 1/3 of the bf16 rate instead
 * of 1/16 (the exact-fp32 MFMA).  Layout: activations [M, 2 K] with logical columns [64 j, 64 j + 64) at physical columns
 * [128 j, 128 j + 64) (hi) and [128 j + 64, 128 j + 128) (lo); weights [N, 3 K] = [hi_j | hi_j | lo_j] per 64 columns (built by
 * snerf_gather_pack: index bit 30 = the lo part).  snerf_linear_fwd then takes the LOGICAL K, writes bf16 outputs in the interleaved
 * layout (fp32 outputs plainly), sums hi + lo into the bias gradient; snerf_linear_wgrad takes the PHYSICAL N = dZ columns and
 * K = X columns (n_valid / k_valid logical) and maps its output indices back.  snerf_split_cast converts fp32 rows ([M, C], zero
 * padded to Cpad % 64 == 0 logical columns) into that layout. */
int snerf_split_cast(const float* src, long ld_src, long M, int C, int Cpad, void* dst, long ld_dst, void* stream);

/* fp16 + fp8 split operands (dtype SNERF_DT_F16F8 of snerf_linear_fwd): the same fp32-class contract in TWO pass-equivalents.  x = hi + r,
 * hi = fp16(x); a product is hi.hi on the fp16 MFMA plus the correction r.w + x.(w - fp16(w)), whose factors need 4 significant bits only and run as
 * OCP e4m3 on the block-scaled MFMA (v_mfma_scale_f32_32x32x64_f8f6f4, twice the 16-bit rate; its E8M0 scale bytes undo the operands' power-of-two
 * scales).  Layout per 64 logical columns, 256 bytes: activations [fp16(x) x 64 | e4m3((x - hi) 2^13) x 64 | e4m3(x 2^2) x 64], weights
 * [fp16(w) x 64 | e4m3(w 2^9) x 64 | e4m3((w - hi) 2^20) x 64] (2-byte element strides, K the LOGICAL reduction length; e4m3 saturates at +-448:
 * |x| > 112 or |w| > 0.875 lose the clipped part of the correction only).  Forward activations only: ACT_NONE / ACT_RELU / ACT_RELU_BITS, no column
 * sums; the backward behind it runs on plain fp16 operands (bit 14 of the two GEMM entries' `variant` reads the fp16 halves).  Measured on fitted
 * weights: profiles/r6_c_two_pass_precision_with_split_schemes.txt.  snerf_split8_cast converts fp32 rows into either layout (weight = 0 / 1). */
#define SNERF_DT_F16F8 5
int snerf_split8_cast(const float* src, long ld_src, long M, int C, int Cpad, void* dst, long ld_dst, int weight, void* stream);

int snerf_colsum_f32(const float* x, long ld, long M, int C, float* out, void* stream);
int snerf_cast_pad(const float* src, long ld_src, long M, int C, int Cpad, void* dst, long ld_dst, int dtype, void* stream);
/* Gradient w.r.t. the pre-embedded input x = [embedded pts (ic) | embedded views (icv)] of the classic NeRF (autograd of NeRF.forward(x),
 * s-nerf/model/run_nerf_helpers.py:103-126): g0 [M, ld0] / g5 [M, ld5] = the fp32 data gradients that reach the point block through
 * pts_linears.0 and (skip connection) pts_linears.5, gv [M, ldv] the one through views_linears.0 (null when icv = 0) ->
 * dx [M, ld_dx >= ic + icv] fp32: dx[:, :ic] = g0 + g5, dx[:, ic:] = gv.  Any row strides, 4-byte alignment. */
int snerf_classic_x_grad(const float* g0, long ld0, const float* g5, long ld5, const float* gv, long ldv, long M, int ic, int icv,
                         float* dx, long ld_dx, void* stream);
/* Refresh of the packed GEMM / fused-MLP operands after an optimiser step (the reference has no counterpart: torch.nn.Linear reads its
 * weights in place): dst[i] = flat[idx[i]] rounded to `dtype` (0 = fp32, 1 = bf16); idx -1 -> 0 (padding), -2 -> 1 (identity rows).  flat =
 * the fp32 parameter arena; idx (16-byte aligned) is built once per network by the host from the same slicing code that defines the
 * layouts (snerf_amd/mlp.py: _Net._build_plan). */
int snerf_gather_pack(const float* flat, const int* idx, long n, void* dst, int dtype, void* stream);
/* The same refresh with the transposed images (a packed W^T reads the arena at a stride of one weight row per element: one L2 request per
 * element in the gather) taken as 16 x 64 destination tiles: tiles int32 [n_tiles, 4] = {dst_off, src_base, src_stride, dst_ld} with
 * dst[dst_off + i * dst_ld + j] = flat[src_base + j * src_stride + i], i < 16, j < 64; src_base and src_stride multiples of 4, flat and tiles
 * 16-byte aligned.  The tiles' elements carry idx = -3 (skipped by the gather part of the launch).  One launch. */
int snerf_gather_pack_tiles(const float* flat, const int* idx, long n, void* dst, int dtype, const int* tiles, int n_tiles, void* stream);
/* snerf_gather_pack_tiles of a network's 16-bit operand pool and the plain gather of its (small) fp32 pool -- biases, fused-kernel tables:
 * dst32[i] = flat[idx32[i]], same index codes -- as ONE launch (tiles / n_tiles may be NULL / 0; n32 = 0: the 16-bit pool alone). */
int snerf_gather_pack_pair(const float* flat, const int* idx, long n, void* dst, int dtype, const int* tiles, int n_tiles, const int* idx32,
                           long n32, float* dst32, void* stream);

/* Semantic compositing, both flavours of the reference.  softmax = 1: zipnerf NerfMLP (internal/models.py:594-597) +
 * internal/render.py:237-241: semantic [R,C] = sum_i detach(weights [R,S]) softmax(logits [R*S, ld][:, :C]) (logits = columns
 * 1..C of the density network's output x); backward: d_logits only (g_w_out, if given, is zeroed).  softmax = 0: live mip path
 * (s-nerf/model/mip.py:175-176): semantic = sum_i weights raw_semantic; backward: d_logits [R*S, ld_d][:, :C] = w g and
 * g_w_out [R,S] = sum_c g_c raw (the weights are part of the graph there).  logits fp32 or bf16; gradients fp32.  row_index
 * (forward, may be NULL): int32 [R,S] from snerf_ert_compact -- the logits of sample (r, i) are row row_index[r, i] of `logits`, -1 =
 * sample not evaluated (contributes nothing): semantic rendering on compacted rows (inference extension, not in the reference). */
int snerf_semantic_composite_fwd(const float* weights, const void* logits, long ld, int dtype, long R, int S, int C, int softmax,
                                 const int* row_index, float* sem, void* stream);
int snerf_semantic_composite_bwd(const float* weights, const void* logits, long ld, int dtype, const float* g_sem, long R, int S, int C,
                                 int softmax, float* d_logits, long ld_d, float* g_w_out, void* stream);

/* ---- early ray termination + sample compaction (inference; NOT in the reference: opt-in, error bounded by the proposal) -----
 * From the proposal histogram (s0 [N,S0+1], w0 [N,S0]) and the resampled fence posts s1 [N,S1+1]: W = cumulative proposal
 * weight (piecewise linear), T_i = 1 - W(s1[i]), m_i = W(s1[i+1]) - W(s1[i]); fine interval i is kept iff T_i > eps_t and
 * m_i > eps_w.  Outputs: row_index [N,S1] (row of the kept sample in the compacted arrays, -1 = skipped), sample_id [rows]
 * (= ray * S1 + i of every row, rows in ray-major order) and *total = number of rows (device).  masks (8*N*ceil(S1/64) bytes)
 * and counts (int32 [N]) are scratch.  snerf_mip_encode / snerf_mip_viewenc take `sample_id, n_rows` (NULL = all samples) and
 * snerf_mip_composite_fwd takes `row_index` (NULL = dense rows) to run the fine level on the compacted rows. */
int snerf_ert_compact(const float* s0, const float* w0, const float* s1, long N, int S0, int S1, float eps_t, float eps_w,
                      void* masks, int* counts, int* row_index, int* sample_id, long* total, void* stream);
/* Front-to-back early ray termination on the fine network's OWN densities (inference; exact bound): the fine level is evaluated in groups
 * of consecutive samples.  One call = after group [g0, g0 + G) was evaluated (prev_raw_d: its raw densities, row r of it = row_index -
 * prev_base; G = 0 / NULL for the first call), add its optical depth sum softplus(raw + density_bias) (t1 - t0) |d| to tau [N] (in/out,
 * zeroed by the caller), flag the rays with exp(-tau) > eps_t (flags [N]), and assign the next group [next_g0, next_g0 + next_G):
 * row_index [N, S1] (row_base + running row, or -1 for the rays that left) and sample_id [rows]; counts [N] scratch; total[0] = rows.
 * The samples never assigned keep the -1 the caller initialised row_index with; their weights sum to at most eps_t per ray. */
int snerf_ert_f2b_step(const float* prev_raw_d, long ld_den, long prev_base, const float* s1, const float* dirs, const float* near,
                       const float* far, long N, int S1, int g0, int G, int next_g0, int next_G, int transform_idx, float density_bias,
                       float eps_t, float* tau, int* flags, int* counts, int* row_index, int* sample_id, long row_base, long* total,
                       void* stream);
/* Front-to-back early ray termination of the CLASSIC path's fine pass (render_rays(ert=...), inference extension, not in the reference):
 * after the fine network evaluated the group [g0, g0 + G) of the rays `alive` (int32 [n], NULL = rays 0 .. n-1; rows of raw_g [n*G, C >= 4]
 * in that order), scatter the raw outputs into raw_full [N, S, C], multiply the rays' transmittances T [N] by exp(-sum relu(sigma) dz |d|)
 * (raw2outputs, run_nerf_helpers.py:394-414; rays [N, ld_rays]: o3, d3, ...; z_all [N, S] sorted), and compact the rays with T > eps_t
 * into alive_next (in order; none when g0 + G == S); *total (device) = their number.  keep: int32 [n], offs: int32 [ceil(n / 1024)] scratch. */
int snerf_classic_ert_step(const float* raw_g, int C, const int* alive, long n, const float* z_all, int S, const float* rays, long ld_rays,
                           int g0, int G, float eps_t, float* T, float* raw_full, int* keep, int* offs, int* alive_next, long* total,
                           void* stream);
/* pts [n, G, 3] = o + d z (render.py:354) and viewdirs [n, 3] (columns viewdir_col .. +2 of the ray rows; NULL = none) of the rows
 * (alive[i], g0 + k) -- the compacted rows of the next group. */
int snerf_classic_ert_points(const float* rays, long ld_rays, const float* z_all, int S, const int* alive, long n, int g0, int G,
                             float* pts, float* viewdirs, int viewdir_col, void* stream);

/* ---- the callers either side of the path --------------------------------------------------------
 * Ray generation: s-nerf/utils/sample_utils.py:286-345 get_rays_single_img (training = 0: whole frame / any pixels, half-pixel
 * centres) and :92-211 sample_single_img (training = 1: directions by run_nerf_helpers.get_rays_by_coord :300-312 without the
 * half-pixel offset, radii from the half-pixel grid), no-NDC branch.  coords int32 [N,2] = (row, col), or NULL for the N pixels
 * first_pixel.. in row-major order.  pose_host: HOST pointer to the [3,4] camera-to-world matrix (12 floats, passed by value
 * to the kernel).  near / far are the caller's bounds (the reference scales them by 0.9 / 1.1 before).  Outputs are the Rays
 * fields of sample_utils.py:11-13 (lossmult = 1 and app = 0 are the caller's constants). */
int snerf_pinhole_rays(const int* coords, long first_pixel, int W, int H, const float* pose_host, float cx, float cy, float fx,
                       float fy, int training, float near, float far, long N, float* origins, float* directions, float* viewdirs,
                       float* radii, float* near_out, float* far_out, void* stream);
/* Per-ray loss tail of s-nerf/train.py:150-208, value and gradients w.r.t. the renderer outputs in one pass: RgbLoss
 * (model/loss_factory.py:5-11) on rgb/tgt [N,3]; calc_depth_loss (model/confidence.py:209-224) = DepthLoss
 * (loss_factory.py:26-37; disparity 1: |1/p - 1/t|) on dist1 (fine) + coarse_mult * dist0 (coarse), rays with tdepth == 0 masked
 * out, times conf [N] (nullable), mean over the valid rays, times depth_lambda (tdepth NULL = no depth loss); ProposalLoss
 * (loss_factory.py:59-74) of the detached fine histogram (s_f [N,Pf], w_f [N,Pf-1]) against the coarse one (s_c [N,Sc+1],
 * w_c [N,Sc]) times prop_lambda (s_c NULL = off).  out[5] = {#valid depth rays, rgb loss, depth loss, proposal loss, their sum};
 * g_rgb [N,3], g_dist1 / g_dist0 [N], g_wc [N,Sc] = d(total loss)/d(input). */
int snerf_mip_loss_tail(const float* rgb, const float* tgt, const float* dist1, const float* dist0, const float* tdepth,
                        const float* conf, const float* s_f, const float* w_f, const float* s_c, const float* w_c, long N, int Pf,
                        int Sc, int disparity, float depth_lambda, float coarse_mult, float prop_lambda, float* out, float* g_rgb,
                        float* g_dist1, float* g_dist0, float* g_wc, void* stream);
/* Loss tail of the classic path (path B): the stock training loop around render_rays with img2mse / mse2psnr
 * (s-nerf/model/run_nerf_helpers.py:16-17).  rgb (the fine colour map, or the only one), rgb0 (the coarse map of a two-level render;
 * nullable), tgt, g_rgb, g_rgb0 (nullable iff rgb0 is): fp32 [N,3] contiguous.
 *   img_loss = mean((rgb - tgt)^2), img_loss0 = mean((rgb0 - tgt)^2) (0 without rgb0), loss = img_loss + img_loss0,
 *   psnr = -10 ln(img_loss) / ln 10;  out[4] = {loss, img_loss, img_loss0, psnr}
 *   g_rgb[i] = inv * (2 * (rgb[i] - tgt[i])) with inv = 1.0f / (float)(3 N), an fp32 division: the expression torch's pow / mean
 *   backward evaluates; g_rgb0 alike from rgb0.  Gradients of the LOCAL mean: a data-parallel mean belongs into Adam's grad_scale.
 * The sums are taken in double in an order that depends on N only (a partial launch into ws, a finish launch that adds the partials
 * in block order and rounds each scalar to fp32 once): no floating-point atomics, bit-reproducible, graph-safe.  ws: device scratch of
 * >= snerf_classic_loss_tail_ws(N) BYTES, 8-byte aligned; nothing past that is written.  Bad arguments (N <= 0, a null rgb / tgt / ws /
 * out / g_rgb, rgb0 and g_rgb0 not both null or both given, a pointer off 4-byte alignment, ws off 8-byte alignment) return 1 before
 * any launch. */
int snerf_classic_loss_tail(const float* rgb, const float* rgb0, const float* tgt, long N, void* ws, float* out, float* g_rgb,
                            float* g_rgb0, void* stream);
/* bytes of scratch snerf_classic_loss_tail needs for N rays (0 for N <= 0) */
long snerf_classic_loss_tail_ws(long N);
/* The same tail with the per-image rules of s-nerf/train.py:131-209; the arguments of snerf_mip_loss_tail keep their meaning and,
 * with every new pointer NULL, their results (gradients bit for bit).  New, each nullable = term or mask absent:
 *   sem [N,C] fp32 composited logits, labels [N] (int32, or fp32 holding exact integers when labels_f32 = 1), g_sem [N,C]: all three
 *   or none; C in 1..32.  SemanticLoss (model/loss_factory.py:13-24): semantic_lambda * nn.CrossEntropyLoss()(sem, labels), labels
 *   of -100 (ignore_index) left out.  A label outside [0, C) other than -100 is left out too (the reference raises on one).
 *   rows int64 [N,2] (the batcher's sel_coords: element 2 r = pixel row of ray r), img_i int64 [1] DEVICE word = the image of the
 *   batch (read by the kernels, never on the host), rgb_row_limit / depth_row_limit / sem_valid int32 [n_images] per-image tables:
 *   all five or none.  With i = *img_i: Wr = rows[2 r] < rgb_row_limit[i] (train.py:137-144, the Waymo side cameras),
 *   Br = rows[2 r] < depth_row_limit[i] (train.py:165-170, the back camera), semantic term only where sem_valid[i] != 0
 *   (train.py:131,185).  An i outside [0, n_images) counts no ray for the rgb, depth and semantic terms.
 *   depth_keep [N] fp32 (needs tdepth): Br also needs depth_keep[r] == 0 (train.py:168-170, seg_mask == 0).
 * rgb = sum_{Wr} |rgb - tgt|^2 / (3 #W), g_rgb = 0 where !Wr; depth = the plain expression over the rays with tdepth != 0 and Br,
 * divided by their number; semantic = mean over the rays with Wr and a counted label of -log softmax(sem_r)[label_r] (row maximum
 * subtracted, float64 log-sum-exp) times semantic_lambda, g_sem = semantic_lambda (softmax - onehot) / #sem on those rays and 0
 * elsewhere (always written in full); proposal = every ray.  A term whose count is 0 is 0 with zero gradients (the reference's mean
 * over an empty selection is NaN).
 * out[8] = {#depth rays, rgb, depth, proposal, total, semantic, #rgb rays, #semantic rays} (out[0..4] as snerf_mip_loss_tail). */
int snerf_mip_loss_tail_masked(const float* rgb, const float* tgt, const float* dist1, const float* dist0, const float* tdepth,
                               const float* conf, const float* s_f, const float* w_f, const float* s_c, const float* w_c,
                               const float* sem, const void* labels, int labels_f32, int C, const long* rows, const long* img_i,
                               const int* rgb_row_limit, const int* depth_row_limit, const int* sem_valid, int n_images,
                               const float* depth_keep, long N, int Pf, int Sc, int disparity, float depth_lambda, float coarse_mult,
                               float prop_lambda, float semantic_lambda, float* out, float* g_rgb, float* g_dist1, float* g_dist0,
                               float* g_wc, float* g_sem, void* stream);
/* snerf_mip_loss_tail_masked plus g_conf [N] (needs tdepth) = d total / d conf[r] = (|e1| + coarse_mult |e0|) depth_lambda / #depth on
 * the rays the depth mean counts (e = the depth errors of DepthLoss above) and 0 elsewhere, always written in full: what the learned
 * confidence (snerf_conf_grad) reduces to the gradient of its table.  Every other output keeps the bits snerf_mip_loss_tail_masked
 * gives; with g_conf NULL the entry IS snerf_mip_loss_tail_masked. */
int snerf_mip_loss_tail_gconf(const float* rgb, const float* tgt, const float* dist1, const float* dist0, const float* tdepth,
                              const float* conf, const float* s_f, const float* w_f, const float* s_c, const float* w_c,
                              const float* sem, const void* labels, int labels_f32, int C, const long* rows, const long* img_i,
                              const int* rgb_row_limit, const int* depth_row_limit, const int* sem_valid, int n_images,
                              const float* depth_keep, long N, int Pf, int Sc, int disparity, float depth_lambda, float coarse_mult,
                              float prop_lambda, float semantic_lambda, float* out, float* g_rgb, float* g_dist1, float* g_dist0,
                              float* g_wc, float* g_sem, float* g_conf, void* stream);
/* Edge-aware smoothness of P depth patches of p x p pixels (--smooth_loss, s-nerf/train.py:154-177): SmoothLoss
 * (model/loss_factory.py:39-57) over edge_aware_loss_v2 (model/loss.py:14-34), value and gradient w.r.t. dist in one pass.
 * rgb [P,p,p,3] (the target colours), dist [P,p,p] (the renderer's distances), sky [P,p,p] (nullable = no sky weighting), fp32:
 *   disp = 1 / max(dist, 1e-5); u = disp / (patch mean of disp + 1e-7); every pair of horizontal neighbours (a left, b right) gives
 *   |u_a - u_b| exp(-mean_c |rgb_a - rgb_b|) (1 + sky_a), every vertical pair alike with a on top;
 *   loss = weight (mean over the P p (p - 1) x-edges + mean over the P p (p - 1) y-edges).
 * out[3] = {loss, x mean, y mean}; total (nullable device float) += loss; g_dist [P,p,p] = d loss / d dist, ADDED when
 * accumulate = 1 and stored when 0.  The gradient follows torch's rules: sign(0) = 0 for equal neighbours, no gradient where
 * dist < 1e-5 (such a pixel still enters its patch mean).  One workgroup per patch, float64 throughout, each result rounded to fp32
 * once; the patches' sums pass through ws (>= snerf_smooth_loss_ws(P) doubles of device scratch, ws_doubles = its length) and are added
 * in a fixed order by a second launch: no floating-point atomics, bit-reproducible, graph-safe.  P = 0 is a no-op; bad arguments (a null
 * rgb / dist / out / g_dist / ws, a short ws, P < 0, p outside 2..32, accumulate outside {0, 1}) return 1 before any launch. */
int snerf_smooth_loss(const float* rgb, const float* dist, const float* sky, long P, int p, float weight, double* ws, long ws_doubles,
                      float* out, float* total, float* g_dist, int accumulate, void* stream);
/* doubles of scratch snerf_smooth_loss needs for P patches */
long snerf_smooth_loss_ws(long P);

/* zipnerf (path C) ray generation: s-nerfpp/zipnerf/internal/camera_utils.py:453-563 pixels_to_rays, perspective camera, no
 * distortion, no NDC.  pix_x / pix_y int32 [N] integer pixel coordinates, cam_idx int32 [N] (NULL = camera 0) into pixtocams
 * [ncam,3,3] (inverse intrinsics) and camtoworlds [ncam,3,4], all device pointers.  float64 arithmetic like numpy's there, one
 * rounding per output.  origins / directions / viewdirs / base_x / base_y [N,3], radii [N], imageplane [N,2] (nullable). */
int snerf_zip_pixels_to_rays(const int* pix_x, const int* pix_y, const int* cam_idx, const float* pixtocams, const float* camtoworlds,
                             int ncam, long N, float* origins, float* directions, float* viewdirs, float* radii, float* imageplane,
                             float* base_x, float* base_y, void* stream);
/* Device-resident training batchers: the training set stays in device memory and ONE launch draws, casts and gathers one batch
 * (positions [i0, i1) of a global batch of n rays: a rank's slice), with no host work and no sync.  The draws come from a
 * counter-based generator (Philox4x32-10 keyed by `seed`, counted by the step, the ray's position in the global batch and the draw
 * number; algorithm in csrc/callers.hip) instead of numpy's; given the drawn pixels, everything else is what snerf_pinhole_rays
 * (training = 1) / snerf_zip_pixels_to_rays compute, bit for bit.  `counter` = int64 [2] device words {step, 0}: the launch draws
 * the batch of step counter[0] and advances it by one (graph-safe: a replayed launch draws the next batch).  uint8 images
 * (images_u8 = 1) decode to float32(k / 255.0), computed in double.  n = 0 is a no-op; bad arguments return 1 before any launch.
 *
 * Path A (s-nerf/dataloader/rayset.py:124-151 SingleImage + sample_utils.py:92-211 sample_single_img, no_batching): the image of
 * step s is i_train[perm_epoch(s mod n_train)] (a keyed permutation of the training images per epoch: each once per epoch), its n
 * pixels are the first n outputs of a keyed permutation of [0, H W) (distinct, n <= H W).  images [N,H,W,3] fp32 or uint8,
 * depths [N,H,W] fp32 (nullable with depth), poses [N,3,4], intrinsics [N,4] = (cx, cy, fx, fy), near / far / app [N] per image
 * (the bounds sample_single_img passes on), extras [n_extra,N,H,W] fp32 per-pixel maps (confidence, sky mask), i_train int32
 * [n_train].  Outputs (i1 - i0 rows): origins / directions / viewdirs [.,3], radii / lossmult (= 1) / near / far / app [.],
 * rgb [.,3], depth [.] (nullable), extras_out [n_extra, i1 - i0], sel_coords int64 [.,2] = (row, col), img_out int64 [1]. */
int snerf_mip_image_batch(const void* images, int images_u8, const float* depths, const float* poses, const float* intrinsics,
                          const float* near, const float* far, const float* app, const float* extras, int n_extra, const int* i_train,
                          int n_train, int N, int H, int W, long seed, long* counter, long n, long i0, long i1, float* origins,
                          float* directions, float* viewdirs, float* radii, float* lossmult, float* near_out, float* far_out,
                          float* app_out, float* rgb, float* depth, float* extras_out, long* sel_coords, long* img_out, void* stream);
/* snerf_mip_image_batch followed by the depth patches of --smooth_loss (s-nerf/utils/sample_utils.py:68-89 sample_patches_pt, :102-103,
 * 136-138: the patches lie BEHIND the random pixels).  With n_patch = 0 (then k0 = k1 = 0) it IS snerf_mip_image_batch: every output
 * has the same bits.  Otherwise ONE launch writes (i1 - i0) pixel rows followed by (k1 - k0) patch_sz^2 patch rows, patches [k0, k1) of
 * the step's n_patch (a rank's whole patches); every output has (i1 - i0) + (k1 - k0) patch_sz^2 rows, extras_out that row stride.  The
 * image of the step and the pixel rows are those of snerf_mip_image_batch for the same seed and step: patches do not move the random
 * pixels.  Centre k of step s is drawn WITH replacement (np.random.randint there) over the (H - 2p - 1)(W - 2p - 1) pixels strictly
 * more than p = patch_sz from every border: the bounded draw of snerf_zip_ray_batch with (i, v) = (k, 3), idx -> row p + 1 + idx / wc,
 * column p + 1 + idx % wc, wc = W - 2p - 1 (csrc/callers.hip).  The patch's pixels are [c - p/2, c + p/2) in both axes, rows outer,
 * patches in order k; every field of a patch row is computed as for a pixel row.  One counter advance per launch; graph-safe.
 * n_patch = 0 with n = 0 is a no-op.  Bad arguments (those of snerf_mip_image_batch; n_patch < 0; 0 <= k0 <= k1 <= n_patch not
 * holding; with n_patch > 0: patch_sz odd, below 2 or above 32, fewer than 1 or 2^32 and more interior pixels) return 1 before any
 * launch. */
int snerf_mip_image_patch_batch(const void* images, int images_u8, const float* depths, const float* poses, const float* intrinsics,
                                const float* near, const float* far, const float* app, const float* extras, int n_extra,
                                const int* i_train, int n_train, int N, int H, int W, long seed, long* counter, long n, long i0, long i1,
                                float* origins, float* directions, float* viewdirs, float* radii, float* lossmult, float* near_out,
                                float* far_out, float* app_out, float* rgb, float* depth, float* extras_out, long* sel_coords,
                                long* img_out, int n_patch, int patch_sz, int k0, int k1, void* stream);
/* Path B (the stock `use_batching` loader of the classic training loop: every ray of the training images, shuffled, N_rand per step):
 * T = n_train H W rays.  Row r of step s has global position p = s n + r, epoch e = p / T, and is ray q = perm(4, e, T)(p mod T) (the
 * keyed permutation of csrc/callers.hip with tag 4, keyed by the epoch) -> image i_train[q / (H W)], pixel row (q mod (H W)) / W, column
 * (q mod (H W)) mod W: every ray exactly once per epoch, a new order every epoch; batches have constant size n and may straddle an
 * epoch boundary.  images [n_images,H,W,3] fp32 or uint8, c2w fp32 [n_images,3,4], intrinsics DOUBLE [n_images,3] = (focal, cx, cy)
 * (snerf_classic_get_rays takes doubles; each is rounded to fp32 as there), i_train int32 [n_train] with entries in [0, n_images).
 * Outputs, rows [i0, i1) of the global batch: rows [i1 - i0, ld] = [o3, d3, near, far, (viewdir3)] (ld >= 8, or 11 with use_viewdirs),
 * bit for bit what snerf_classic_ray_batch writes for the same pixel of the same camera (ndc as there, near = 1 in the warp); rgb
 * [i1 - i0, 3] the pixel's colour.  counter as above.  A launch with i0 = i1 still advances the counter.  Bad arguments (n <= 0,
 * n_images / n_train / H / W < 1, 0 <= i0 <= i1 <= n not holding, seed < 0, a null pointer, images_u8 outside {0, 1}, a short ld, a
 * misaligned pointer) return 1 before any launch. */
int snerf_classic_train_batch(const void* images, int images_u8, const float* c2w, const double* intrinsics, const int* i_train,
                              int n_train, int n_images, int H, int W, long seed, long* counter, long n, long i0, long i1, int ndc,
                              float near, float far, int use_viewdirs, float* rows, int ld, float* rgb, void* stream);
/* Path C(s-nerfpp/zipnerf/internal/datasets.py:442-566 Dataset._next_train + _make_ray_batch, patch_size 1; anything else is a
 * bad argument): per ray a camera in [0, N) and x in [border, W - border), y in [border, H - border), uniform WITH replacement like
 * np.random.randint (single_image = 1: one camera per step, batching 'single_image').  images [N,H,W,3] fp32 or uint8, depths
 * [N,H,W] fp32, semantics int32 [N,H,W], masks fp32 [N,H,W] (each nullable with its output), pixtocams [N,3,3], camtoworlds
 * [N,3,4], local2global int32 [N] (nullable with glo_idx).  Outputs (i1 - i0 rows): the rays of snerf_zip_pixels_to_rays
 * (imageplane nullable), lossmult (= 1) / near / far / cam_idx / glo_idx fp32 [.] (as _make_ray_batch's float casts), rgb [.,3],
 * depth [.], semantic int32 [.], mask [.], and the drawn pix_x / pix_y int32 [.]. */
int snerf_zip_ray_batch(const void* images, int images_u8, const float* depths, const int* semantics, const float* masks,
                        const float* pixtocams, const float* camtoworlds, const int* local2global, int N, int H, int W, float near,
                        float far, int border, int patch_size, int single_image, long seed, long* counter, long n, long i0, long i1,
                        float* origins, float* directions, float* viewdirs, float* radii, float* imageplane, float* base_x,
                        float* base_y, float* lossmult, float* near_out, float* far_out, float* cam_idx, float* glo_idx, float* rgb,
                        float* depth, int* semantic, float* mask, int* pix_x, int* pix_y, void* stream);
/* snerf_zip_ray_batch for patch_size = p in 2..32 (datasets.py:397-414 next_train, :508-541 _next_train): n % (4 p^2) = 0; the first
 * n_patch p^2 positions of the global batch, n_patch = (n / 4) / p^2, are whole patches of p x p pixels in order k, rows dy-outer,
 * dx-inner; the other n - n / 4 positions are single pixels.  Patch k draws its camera, x0 in [border, W - border - p] and y0 in
 * [border, H - border - p] with snerf_zip_ray_batch's bounded draw as (i, v) = (k p^2, 0 / 1 / 2); its pixels are (x0 + dx, y0 + dy).
 * A pixel position keeps the draw it has in snerf_zip_ray_batch for the same seed and step; single_image = 1: every row takes the
 * camera of position 0.  ONE launch writes patches [k0, k1) followed by positions [i0, i1), n_patch p^2 <= i0 <= i1 <= n (a rank's
 * whole patches, then its pixels): (k1 - k0) p^2 + (i1 - i0) rows in every output; given (x, y, camera), every field of a row is
 * computed as by snerf_zip_ray_batch.  One counter advance per launch; graph-safe.  n = 0 is a no-op.  Bad arguments (those of
 * snerf_zip_ray_batch; p outside 2..32; n % (4 p^2) != 0; 2 border + p > W or H; 0 <= k0 <= k1 <= n_patch or the bounds of i0, i1 not
 * holding) return 1 before any launch. */
int snerf_zip_ray_patch_batch(const void* images, int images_u8, const float* depths, const int* semantics, const float* masks,
                              const float* pixtocams, const float* camtoworlds, const int* local2global, int N, int H, int W, float near,
                              float far, int border, int patch_size, int single_image, long seed, long* counter, long n, long k0, long k1,
                              long i0, long i1, float* origins, float* directions, float* viewdirs, float* radii, float* imageplane,
                              float* base_x, float* base_y, float* lossmult, float* near_out, float* far_out, float* cam_idx,
                              float* glo_idx, float* rgb, float* depth, int* semantic, float* mask, int* pix_x, int* pix_y, void* stream);
/* The patch terms of s-nerfpp/zipnerf/train.py:280-293 on P patches of p x p rays (p in 2..32, layout [k, dy, dx]), values and gradients
 * in one pass: d_smo = d_mult * edge_aware_loss_v2(rgb, 1 / (depth + 1e-5), mask) and s_smo = s_mult * edge_aware_loss_for_semantic(rgb,
 * sem, mask) (internal/train_utils.py:297-315, 337-359, the `mask is not None` branch).  fp32: rgb [P,p,p,3] target colours, depth
 * [P,p,p] rendered, sem [P,p,p,C] rendered probabilities with row stride ld_sem >= C, C in 1..32 (NULL = no semantic term: s_smo = 0,
 * g_sem not touched, ld_sem / C ignored), mask [P,p,p] in the batch's convention, > 0 = masked out (NULL = every pixel valid).
 *   disp = 1 / (depth + 1e-5) (no clamp), u = disp / (patch mean of disp over all p^2 pixels, masked or not, + 1e-7),
 *   v_c = sem_c / (patch mean of sem_c + 1e-5), w(a, b) = exp(-mean_c |rgb_a - rgb_b|);
 *   x-edges join (dy, dx) and (dy, dx + 1), y-edges (dy, dx) and (dy + 1, dx); an edge is valid when both pixels are unmasked,
 *   Nx / Ny = the valid x- / y-edges of all P patches;
 *   d_smo = d_mult (sum over valid x-edges of |u_a - u_b| w / Nx + the same over y-edges / Ny),
 *   s_smo = s_mult (sum over valid x-edges of (sum_c |v_c,a - v_c,b|) w / Nx + the same over y-edges / Ny).
 * Nx = 0 or Ny = 0: both terms and all gradients are exactly 0, as torch.nan_to_num of the empty mean gives.  Other non-finite values
 * propagate as they are: nan_to_num's mapping of +-inf to the largest float is NOT reproduced.
 * out[4] = {d_smo, s_smo, Nx, Ny} (the counts as floats); total (nullable device float) += d_smo, then += s_smo.
 * g_depth [P p^2] and g_sem [P p^2, ld_sem] = grad_mult * d (d_smo + s_smo) / d (depth, sem), stored when accumulate = 0 and ADDED
 * when 1: grad_mult (the trainer's loss scale) multiplies the gradients and not the values.  The gradients follow torch's rules:
 * through the patch means (a masked pixel of a patch with valid edges has a gradient) and through 1 / (depth + 1e-5); sign(0) = 0.
 * One workgroup per patch, float64 throughout, each output rounded to fp32 once.  With a mask the edge counts come from an integer
 * count launch ahead of the main one (a memset node zeroes the counters); the patches' sums pass through ws (>= snerf_zip_smooth_loss_ws(P)
 * doubles of device scratch, ws_doubles = its length) and are added in a fixed order by a one-wave launch: no floating-point atomics,
 * bit-reproducible, graph-safe, no host read.  P = 0 is a no-op; bad arguments (a null rgb / depth / out / g_depth / ws, a short ws,
 * P < 0, p outside 2..32, accumulate outside {0, 1}; with sem: C outside 1..32, ld_sem < C, a null g_sem) return 1 before any launch. */
int snerf_zip_smooth_loss(const float* rgb, const float* depth, const float* sem, long ld_sem, int C, const float* mask, long P, int p,
                          float d_mult, float s_mult, float grad_mult, double* ws, long ws_doubles, float* out, float* total,
                          float* g_depth, float* g_sem, int accumulate, void* stream);
/* doubles of scratch snerf_zip_smooth_loss needs for P patches */
long snerf_zip_smooth_loss_ws(long P);
/* Per-ray loss tail of s-nerfpp/zipnerf/train.py:250-311, value and gradients w.r.t. the renderer outputs in one pass:
 * data term (internal/train_utils.py:62-90; mse = 0: Charbonnier sqrt(resid^2 + pad^2), 1: resid^2) weighted by lossmult [R]
 * (nullable = 1) and normalised by its sum; disparity L1 |1/(depth+1e-5) - 1/(1e-5+tdepth)| as a masked mean under dmask [R]
 * (x depth_lambda, train.py:252-255,277) and cmask [R] (x depth_lambda * com_mult, :260-272), both nullable, empty mask = 0;
 * semantic NLL -log(sem[r, labels[r]] + 1e-6) as a masked mean under smask (x sem_mult, :294-298; sem NULL = off);
 * anti_interlevel_loss (train_utils.py:132-164: stepfun.blur_stepfun :425-433 with pulse widths pw0 / pw1, math.sorted_interp_quad
 * :133-156) of the NeRF histogram (s2 [R,S2+1], w2 [R,S2], detached) against the proposal levels (s0/w0, s1/w1; either NULL = skip)
 * x inter_mult; lossfun_distortion (stepfun.py:297-307) on the NeRF level x dist_mult (s2 NULL = no regularisers).
 * out[11]: [0..3] = {3 sum lossmult, sum dmask, sum cmask, sum smask}, [4..10] = {data, mse, depth, d_complete, sem, interlevel,
 * distortion}, weights applied.  g_rgb [R,3], g_depth [R], g_sem [R,C], g_w0 [R,S0], g_w1 [R,S1] (interlevel), g_w2 [R,S2]
 * (distortion) = d(sum of the terms)/d(input). */
int snerf_zip_loss_tail(const float* rgb, const float* tgt, const float* lossmult, const float* depth, const float* tdepth,
                        const float* dmask, const float* cmask, const float* sem, const int* labels, const float* smask, int C,
                        const float* s0, const float* w0, int S0, const float* s1, const float* w1, int S1, const float* s2,
                        const float* w2, int S2, long R, int mse, float pad, float data_mult, float depth_lambda, float com_mult,
                        float sem_mult, float pw0, float pw1, float inter_mult, float dist_mult, float* out, float* g_rgb,
                        float* g_depth, float* g_sem, float* g_w0, float* g_w1, float* g_w2, void* stream);

/* Distance percentiles of compute_extras (internal/render.py:255-267 -> stepfun.weighted_percentile :329-339, math.sorted_interp
 * :88-107): tdist [R,S+1], weights [R,S], t_far [R] (the extra fence post that carries the background weight); ps_host: HOST array of
 * np <= 8 percentiles in % (the reference uses 5, 50, 95); out [R,np]. */
int snerf_zip_percentiles(const float* tdist, const float* weights, const float* t_far, long R, int S, const float* ps_host, int np,
                          float* out, void* stream);

/* Frame quantisation for the S-NeRF++ wire format (s-nerfpp/zipnerf/random_render_waymo_seq.py:214-227): rgb [P,3] -> u8 as
 * internal/utils.py:111-116 save_img_u8 (clip(nan_to_num(x), 0, 1) * 255, truncated); depth [P] -> u16 = depth * 256 / scale_factor
 * truncated (:218-219); sem [P, ld_sem >= C] -> label u8 = first argmax over the C classes (:222-223) and paint u8 [P,3] =
 * color_map[label] (color_map: device u8 [C,3]; :225).  Any of rgb / depth / sem may be NULL (skipped); paint_u8 may be NULL. */
int snerf_frame_quantize(const float* rgb, const float* depth, const float* sem, long ld_sem, int C, const void* color_map, long P,
                         float scale_factor, void* rgb_u8, void* depth_u16, void* label_u8, void* paint_u8, void* stream);

/* ---- image-space foreground composite of S-NeRF++ stage 1 (s-nerfpp/stage1_code/) -----------------------
 * All images are device uint8 [H,W,3] (masks / bands hold 0 or 255, tested as > 0), depth float [H,W] (the uint16 depth PNG / 256,
 * exactly representable), semantic uint8 [H,W]; P = H*W.
 * snerf_fg_paste: utils_render.py:826-1005 handle_occlusion_paste given fg_depth [P] = the mesh depth along each pixel's ray (what the
 * reference's ray tracer returns, :913-947; ignored with person = 1, where the reference uses -1 :940-941).  In place: a pixel with
 * mask[...,0] > 0 takes the foreground colour, fg depth and class_id when fg_depth < depth or the background class is 0, 1 or 8;
 * otherwise its mask is cleared.  counters (device int[2]) <- {#masked, #pasted}: occlusion = 1 - pasted / (masked + 1) (:1002-1003). */
int snerf_fg_paste(void* bg_im, const void* fg_im, void* mask_im, float* depth, void* semantic, const float* fg_depth, long P,
                   int class_id, int person, int* counters, void* stream);
/* utils_render.py:306-324 get_bound_im: band = cv2.dilate(mask[...,0]) XOR cv2.erode(mask[...,0]) with the r x r rect kernel (default
 * anchor r/2, border never wins), written to all 3 channels of bound_im as 0 / 255; mask_out (nullable, must not alias mask_im)
 * <- ip_utils.py:10-19 set_diff(mask_im, bound_im) as the caller does next (generate_images.py:152-153). */
int snerf_fg_bound(const void* mask_im, int H, int W, int r, void* bound_im, void* mask_out, void* stream);
/* In place over nbytes bytes: total_bound <- utils_render.py:338-361 fuse_bound(total_mask, total_bound, bound, mask), then
 * total_mask <- (mask | total_mask) * 255 (generate_images.py:160-161). */
int snerf_fg_accumulate(void* total_mask, void* total_bound, const void* bound, const void* mask, long nbytes, void* stream);
/* utils_render.py:327-335 fuse_bound_and_im: im[bound > 0] = 0, per byte, in place. */
int snerf_fg_blank(void* im, const void* bound, long nbytes, void* stream);
/* Pairwise overlap statistics of N masks, the input of utils_render.py:691-808 occlution_order (:745-753).  masks: a HOST array of N
 * DEVICE pointers to [H,W,3] uint8 masks (copied into the kernel arguments: no staging copy, no stacked masks; 16-byte aligned masks
 * are read with 16-byte loads, others byte by byte); stats: device int64 [N,N,3], ZEROED BY THE CALLER, to which the entry adds.  For
 * every pair a < b, stats[a][b] = (count, sum of row, sum of col) over all (row, col, channel) triples with mask_a > 0 and mask_b > 0
 * there: what np.where(intersection_mask > 0) enumerates -- bytes, not pixels, so masks whose channels differ are counted as the
 * reference counts them.  Entries with a >= b are not touched.  Integer sums through 32-bit LDS partials and 64-bit atomics: the result
 * does not depend on their order and is bit-reproducible.  Bad arguments (N outside [2, 32], H or W outside [1, 65535], a null masks,
 * mask or stats pointer) return 1 before any launch. */
int snerf_fg_overlap(const void* const* masks, int N, int H, int W, long* stats, void* stream);
/* The lighting match of stage 1 (utils_render.py:1008-1051 handle_lighting, called by fuse() on the whole frame after every paste, :300;
 * lighting.hip).  Both entries are bit-exact against the numpy model in snerf_amd/foreground.py (rgb_to_hsv_u8_host, hsv_to_rgb_u8_host,
 * handle_lighting_host, lighting_stats_host).
 *
 * snerf_fg_hsv: in place on P packed 3-byte pixels, any byte alignment of px, any P >= 1 (no limit but `long`).  to_rgb = 0 is OpenCV's
 * 8-bit COLOR_RGB2HSV with H range 180, to_rgb = 1 its 8-bit COLOR_HSV2RGB, both restated from the scalar code of OpenCV's imgproc
 * color_hsv (RGB2HSV_b; HSV2RGB_b over HSV2RGB_native):
 *   RGB -> HSV, integers, shift 12: sdiv[i] = rint((255 << 12) / (1.0 i)), hdiv[i] = rint((180 << 12) / (6.0 i)), i = 1 .. 255, double
 *     division, half to even, entry 0 = 0.  v = max(r, g, b), diff = v - min(r, g, b), s = (diff sdiv[v] + 2048) >> 12; h0 = g - b if
 *     v == r, else b - r + 2 diff if v == g, else r - g + 4 diff; h = (h0 hdiv[diff] + 2048) >> 12 (arithmetic shift), + 180 if h < 0.
 *   HSV -> RGB, fp32, every operation rounded on its own: hf = float(h) * (6.f / 180.f), sf = float(s) * (1.f / 255.f), vf = float(v) *
 *     (1.f / 255.f) (the constants are fp32 divisions).  sf == 0: all three channels are vf.  Otherwise hf = fmodf(hf, 6.f), sector =
 *     floor(hf), hf -= sector (a sector outside 0 .. 5 becomes sector 0 with hf = 0); tab = {vf, vf (1 - sf), vf (1 - sf hf),
 *     vf (1 - sf (1 - hf))}; (b, g, r) = tab[{1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0}][sector].  Each channel is
 *     rint(x * 255.f) (half to even) saturated to 0 .. 255.  H = 180 .. 255 is legal input and follows the same formula.
 * Refused (1, before any launch): a null px, P < 1, to_rgb outside 0 / 1.
 *
 * snerf_fg_lighting: im [H,W,3] u8, changed in place; mask [H,W,3] u8 of which only channel 0 is read, as mask[..., 0] > 0 (a 1 counts,
 * channels 1 and 2 do not).  On V = max(r, g, b), the V channel of the frame's HSV image:
 *   fg = the pixels with mask[..., 0] > 0, (i_min, i_max, j_min, j_max) their bounding rows and columns, i_len = i_max - i_min, j_len =
 *     j_max - j_min; the box grows to rows [max(0, i_min - i_len / 2 - 1), min(H - 1, i_max + i_len / 2 + 1)] and the same for the columns
 *     with W; bg = the pixels with mask[..., 0] == 0 inside the grown box, bounds inclusive.
 *   fg_mean = sum_v_fg / n_fg, bg_mean = sum_v_bg / n_bg: double divisions of exact integer sums (numpy's float64 mean of uint8 data).
 *   V' = (uint8) trunc(clip((double(V) - fg_mean) + bg_mean, 0, 255)) on fg, two double additions in this order -- unless all fg V are
 *     equal (`if not fg_var < 1e-7`), decided as n_fg sum_v2_fg == sum_v_fg^2 in int64: then V stays.  The smallest non-zero variance
 *     of n bytes is (n - 1) / n^2 = 1.19e-7 > 1e-7 at n = 2^23, so up to H W = 2^23 the integer test and numpy's agree for every input
 *     and both sides fit in int64; hence the size limit.
 *   keep_background = 0 (the reference): EVERY pixel of the frame is rewritten as hsv2rgb(rgb2hsv(.)) with the V above, also when the
 *     mask is empty (:1018-1019) or no shift applies.  keep_background = 1 (an extension): pixels with mask[..., 0] == 0 keep their
 *     bytes, fg pixels get exactly the keep_background = 0 result.
 *   Deviation: a mask that fills its whole grown box leaves n_bg = 0; the reference then casts the NaN mean of an empty array to uint8
 *     (undefined).  Here V stays unchanged in that case.
 * stats: device long[9], scratch and output, initialised by the entry itself (an init launch on `stream`): {i_min, i_max, j_min,
 * j_max, n_fg, sum_v_fg, sum_v2_fg, n_bg, sum_v_bg}; the box is that of the RAW mask, before it grows.  An empty mask leaves n_fg = 0
 * and the sentinels (i_min, i_max, j_min, j_max) = (H, -1, W, -1); n_bg and sum_v_bg are then 0 too.  The init launch and three
 * kernels (fg statistics; bg statistics, whose workgroups read the box from stats on the device and exit outside its rows; apply); no
 * host read, no sync, capturable in a graph.  Integer sums through wave and workgroup partials and 64-bit integer atomics: no
 * floating-point atomics, the result does not depend on the order.  Any byte alignment of im and mask.
 * Refused (1, before any launch): a null im / mask / stats, H or W < 1, H * W > 2^23, keep_background outside 0 / 1.
 *
 * PARITY: cv2 is installed neither where this was written nor where it was run, so the two conversions follow OpenCV's published scalar
 * code and are UNPINNED against the library -- in particular whether a SIMD build of HSV2RGB fuses v * (1 - s * h).  Everything after
 * the conversions (box, means, shift, clip, cast) is pinned: it is the reference's own numpy. */
int snerf_fg_hsv(void* px, long P, int to_rgb, void* stream);
int snerf_fg_lighting(void* im, const void* mask, int H, int W, int keep_background, long* stats, void* stream);

/* Hash-grid weight decay (s-nerfpp/zipnerf/internal/train_utils.py:184-203 hash_decay_loss; torch_scatter.segment_coo(param**2, idx,
 * reduce='mean').mean() per encoder): table / grad fp32 [rows, C] (grad accumulated: += 2 mult p / (rows_l L C)), offsets device int32
 * [L+1]; *loss (device, nullable) += mult * mean over (l, c) of the per-level mean of table^2. */
int snerf_hash_decay(const float* table, float* grad, const int* offsets, int L, int C, float mult, float* loss, void* stream);

/* Gradients of the encoders w.r.t. the rays (pose refinement, s-nerf/utils/sample_utils.py:410-435: autograd through
 * integrated_pos_enc mip.py:105-118, sample2enc / Jacobi_g / fn2 mip.py:343-395 and cast_rays / lift_gaussian mip.py:31-91).
 * dE fp32 [n_rays*S, ld >= 6*max_deg] = d loss / d IPE features; g_origins / g_directions [n_rays,3] are WRITTEN (one wave per ray,
 * deterministic).  Fence posts carry no ray gradient (level 0 constants; level 1 detached, mip.py:318). */
int snerf_mip_encode_bwd(const float* s_vals, const float* origins, const float* directions, const float* radii, const float* near,
                         const float* far, long n_rays, int S, int cone, int transform_idx, int max_deg, const float* dE, long ld,
                         float* g_origins, float* g_directions, void* stream);
/* snerf_mip_encode_bwd with the warp selected, the backward of snerf_mip_encode_warp: fn_idx 1 = the contraction (above), 0 = the
 * view-centred warp fn1 + Jacobi_f (mip.py:323-341, 367-369) around (vx, vy, vz); far_max = device scalar max(far) of the batch. */
int snerf_mip_encode_warp_bwd(const float* s_vals, const float* origins, const float* directions, const float* radii, const float* near,
                              const float* far, long n_rays, int S, int cone, int transform_idx, int max_deg, const float* dE, long ld,
                              float* g_origins, float* g_directions, int fn_idx, float vx, float vy, float vz, const float* far_max,
                              void* stream);
/* dV fp32 [n_rays*S, ld >= 3 + 6*deg] = d loss / d view-direction encoding (mip.py:12-21) -> g_viewdirs [n_rays,3] (written). */
int snerf_mip_viewenc_bwd(const float* viewdirs, long n_rays, int S, int deg, const float* dV, long ld, float* g_viewdirs, void* stream);

/* Inference of one zipnerf PROPOSAL level in a single launch: snerf_zip_encode_fwd for the single-channel grid (C = 1) followed by the
 * proposal MLP on the features still in registers -- density_layer = Linear(L, hidden) + ReLU + Linear(hidden, 1)
 * (internal/models.py:425-427, 481-519 with disable_rgb).  w1 [hidden, L], b1 [hidden], w2 [hidden], b2 [1]: fp32 device pointers (the
 * state_dict tensors prop_mlp_i.density_layer.{0,2}.{weight,bias}); round_bf16 = 1 (bf16) / 2 (fp16) reproduces that GEMM path's roundings
 * (features, weights, hidden layer), 0 = fp32 throughout.  raw_density [R*S] fp32. */
int snerf_zip_encode_prop_fwd(const float* tdist, const float* origins, const float* directions, const float* radii, const float* base_x,
                              const float* base_y, const float* deg_jitter, const void* table, const int* offsets, const int* grid_sizes,
                              long R, int S, int L, int n, int m, float Sl, int H, float std_scale, int table_dtype, const float* w1,
                              const float* b1, const float* w2, const float* b2, int hidden, int round_bf16, float* raw_density,
                              void* stream);

/* ---- fused register-resident MLPs (csrc/fmlp.hip) ----------------------------------------------------------------------------
 * One launch for a whole 256-wide network; activations stay in registers from the first layer to the heads, the weights stream
 * through LDS as MFMA fragments.  wstream: n_frags x 1 KiB fragments in the kernel's consumption order, bias: n_blocks x 32 floats
 * (both built by snerf_amd.mlp.fmlp_pack from the reference's state_dict tensors; layout in the kernel header).  bf16 operands,
 * fp32 accumulation.
 * snerf_fmlp_classic_fwd  = NeRF.forward behind run_network (s-nerf/model/run_nerf_helpers.py:103-126, 460-474) for D = 8, W = 256,
 *   skips = [4], use_viewdirs: E [M, ldE] = embedded points (63 values, zero padded to 64), VE [M, ldVE] = embedded view directions
 *   (27 -> 32) -> raw [M,4] = (rgb, sigma).  n_frags = 1184, n_blocks = 78.
 * snerf_fmlp_proposal_fwd = proposal.forward (s-nerf/model/models.py:316-325), 4 x 256: E [M, ldE] = IPE (96) -> raw_density [M].
 *   n_frags = 448, n_blocks = 33. */
int snerf_fmlp_classic_fwd(const void* E, long ldE, const void* VE, long ldVE, const void* wstream, long n_frags, const float* bias,
                           int n_blocks, float* raw, long M, void* stream);
int snerf_fmlp_proposal_fwd(const void* E, long ldE, const void* wstream, long n_frags, const float* bias, int n_blocks,
                            float* raw_density, long M, void* stream);
/* snerf_fmlp_classic_fwd with the two positional encodings (Embedder, run_nerf_helpers.py:22-52) computed inside the kernel: the whole
 * run_network (:460-474) is this ONE launch.  pts [M,3] fp32 sample positions (row = ray * S + sample), viewdirs [M / S, ldvd] fp32.
 * sin / cos are evaluated in revolutions (two-term exact-product reduction + v_sin_f32, abs. error a few 1e-7) and rounded to bf16
 * like the output of snerf_classic_embed, which remains the bit-exact fp32 statement of the encoding.  M < 2^31. */
int snerf_fmlp_classic_pts_fwd(const float* pts, const float* viewdirs, long ldvd, int S, const void* wstream, long n_frags,
                               const float* bias, int n_blocks, float* raw, long M, void* stream);
/* snerf_fmlp_classic_fwd on the caller's pre-embedded fp32 rows (NeRF.forward(x), run_nerf_helpers.py:103-126, as batchify(fn, netchunk)
 * calls it, :450-474): x [M, ldx >= 90], columns [0, 63) = embedded points, [63, 90) = embedded view directions, any row stride, 4-byte
 * alignment (a row- or column-sliced view of a wider tensor).  Rounded to bf16 in registers exactly as snerf_cast_pad rounds (nearest
 * even): bit-identical to snerf_cast_pad into E / VE followed by snerf_fmlp_classic_fwd.  M < 2^31. */
int snerf_fmlp_classic_x_fwd(const float* x, long ldx, const void* wstream, long n_frags, const float* bias, int n_blocks, float* raw,
                             long M, void* stream);
/* Its training forward: the stores of snerf_fmlp_classic_train_fwd (acts / act_ld / bits, same layout) plus the rounded inputs where the
 * per-layer backward reads them -- xin / xin_ld: HOST arrays of 3 device pointers / row strides (elements): the operand of pts_linears.0
 * ([M, >= 64] bf16), the head of the skip buffer ([M, >= 64]) and the view tail of [feature | views] ([M, >= 32]); pad columns written
 * as zeros; pointers 16-byte aligned, strides multiples of 8.  Bit-identical to snerf_cast_pad into those three buffers followed by
 * snerf_fmlp_classic_train_fwd.  M < 2^31. */
int snerf_fmlp_classic_x_train_fwd(const float* x, long ldx, const void* wstream, long n_frags, const float* bias, int n_blocks,
                                   float* raw, void* const* xin, const long* xin_ld, void* const* acts, const long* act_ld,
                                   void* const* bits, long M, void* stream);
/* Training forward of the two networks (autograd of NeRF.forward / proposal.forward in the reference): the same launch, which also
 * stores what the backward pass reads -- the bf16 outputs of the hidden layers and the ReLU bit masks of the 256-wide ones.
 * acts / act_ld: HOST arrays of device pointers / row strides (elements) -- classic: 10 = pts_linears.0 .. .7 (256 wide),
 * feature_linear (256), views_linears.0 (128); proposal: 4 = layers.0 .. .3 (256 wide).  Pointers 16-byte aligned, strides multiples
 * of 8.  bits: HOST array of 9 (classic: pts_linears.0 .. .7, then views_linears.0) / 4 (proposal) device pointers to
 * 4 * 8 * ceil(M / 256) * 4 * 64 bytes each (views_linears.0: half that), written in the layout snerf_linear_fwd's act = 4 (mask
 * bits) reads.  The per-layer snerf_linear_fwd (data gradient) /
 * snerf_linear_wgrad consume all of it unchanged. */
int snerf_fmlp_classic_train_fwd(const void* E, long ldE, const void* VE, long ldVE, const void* wstream, long n_frags,
                                 const float* bias, int n_blocks, float* raw, void* const* acts, const long* act_ld,
                                 void* const* bits, long M, void* stream);
int snerf_fmlp_proposal_train_fwd(const void* E, long ldE, const void* wstream, long n_frags, const float* bias, int n_blocks,
                                  float* raw_density, void* const* acts, const long* act_ld, void* const* bits, long M,
                                  void* stream);
/* The seven entries above in either 16-bit flavour (library version >= 2): the same arguments with `int dtype` in front of `stream`.
 * dtype = SNERF_DT_BF16 (what the entries without the suffix run; they forward here) or SNERF_DT_F16: E / VE, the weight stream (packed
 * from fp16 weights), the stored activations and the xin copies are fp16, the products run on the f16 MFMA with fp32 accumulation, the
 * heads leave from the unrounded fp32 accumulator.  pts / x inputs are rounded to fp16 to nearest even, as snerf_classic_embed /
 * snerf_cast_pad round for SNERF_DT_F16, so "x flavour == snerf_cast_pad + rows flavour, bit for bit" holds in fp16 too.  The ReLU bit
 * masks have the same layout and meaning (a 16-bit ReLU output is > 0 iff its bits are not 0).  Any other dtype: SNERF_ERR_ARG, before
 * anything touches a device. */
int snerf_fmlp_classic_fwd_dt(const void* E, long ldE, const void* VE, long ldVE, const void* wstream, long n_frags, const float* bias,
                              int n_blocks, float* raw, long M, int dtype, void* stream);
int snerf_fmlp_proposal_fwd_dt(const void* E, long ldE, const void* wstream, long n_frags, const float* bias, int n_blocks,
                               float* raw_density, long M, int dtype, void* stream);
int snerf_fmlp_classic_pts_fwd_dt(const float* pts, const float* viewdirs, long ldvd, int S, const void* wstream, long n_frags,
                                  const float* bias, int n_blocks, float* raw, long M, int dtype, void* stream);
int snerf_fmlp_classic_x_fwd_dt(const float* x, long ldx, const void* wstream, long n_frags, const float* bias, int n_blocks, float* raw,
                                long M, int dtype, void* stream);
int snerf_fmlp_classic_x_train_fwd_dt(const float* x, long ldx, const void* wstream, long n_frags, const float* bias, int n_blocks,
                                      float* raw, void* const* xin, const long* xin_ld, void* const* acts, const long* act_ld,
                                      void* const* bits, long M, int dtype, void* stream);
int snerf_fmlp_classic_train_fwd_dt(const void* E, long ldE, const void* VE, long ldVE, const void* wstream, long n_frags,
                                    const float* bias, int n_blocks, float* raw, void* const* acts, const long* act_ld,
                                    void* const* bits, long M, int dtype, void* stream);
int snerf_fmlp_proposal_train_fwd_dt(const void* E, long ldE, const void* wstream, long n_frags, const float* bias, int n_blocks,
                                     float* raw_density, void* const* acts, const long* act_ld, void* const* bits, long M,
                                     int dtype, void* stream);

/* NeRF MLP of the zipnerf path at INFERENCE as one launch (s-nerfpp/zipnerf/internal/models.py:462-479, 586-703; waymo.gin branch, no GLO
 * vectors): F [M, ldF >= 64] grid features (columns 40.. zero) and D [M, ldD >= 16] direction encoding (columns 9.. zero) in `dtype`
 * (SNERF_DT_BF16 or SNERF_DT_F16) -> raw_rgb [M, ld_rgb >= 3] and raw_d [M, ld_d >= 1] fp32.  density_layer.0 (+ReLU), density_layer.2 (x;
 * raw density = its output 0 before rounding), lin_second_stage_0 on cat([x, D]) (+ReLU), lin_second_stage_1 on cat([h, x, D]) (+ReLU),
 * rgb_layer -- activations stay in registers.  x32 (optional, [M, ld_x >= 32] in `dtype`): channels 0..31 of x, of which the semantic head
 * reads 1..C (models.py:594-597).  wstream (464 fragments of 1 KiB) / bias (35 blocks of 32 floats): the packing of
 * snerf_amd.mlp.ZipNerfNet._pack_fused_infer. */
int snerf_fmlp_zip_fwd(const void* F, long ldF, const void* D, long ldD, const void* wstream, long n_frags, const float* bias, int n_blocks,
                       float* raw_rgb, long ld_rgb, float* raw_d, long ld_d, void* x32, long ld_x, long M, int dtype, void* stream);
/* ... and as the TRAINING forward: the same outputs plus what the backward reads -- acts[0] = H1 [M, >= 64], acts[1] = x, acts[2] = h
 * (lin_second_stage_0), acts[3] = H3 (lin_second_stage_1) [M, >= 256] each (in `dtype`, row strides act_ld, 16-byte aligned) and bits[0..2] =
 * the ReLU bit masks of H1 ([M, 64]), h and H3 ([M, 256]) in snerf_linear_fwd's SNERF_ACT_RELU_BITS layout. */
int snerf_fmlp_zip_train_fwd(const void* F, long ldF, const void* D, long ldD, const void* wstream, long n_frags, const float* bias, int n_blocks,
                             float* raw_rgb, long ld_rgb, float* raw_d, long ld_d, void* const* acts, const long* act_ld, void* const* bits,
                             long M, int dtype, void* stream);
/* ... and its BACKWARD data-gradient chain in one launch: d_rgb [M, ld_rgb >= 3], d_den [M, ld_den >= den_cols] fp32 (d raw density, then the
 * gradients of the den_cols - 1 <= 31 semantic logits) -> dz[0] = d pre-activation of lin_second_stage_1, dz[1] = of lin_second_stage_0, dz[2] = d x
 * ([M, >= 256] each), dz[3] = d pre-activation of density_layer.0, dz[4] = d grid features ([M, >= 64]) in `dtype` -- the operands of the five
 * weight-gradient GEMMs and of the table gradient; bits[0..2] as written by snerf_fmlp_zip_train_fwd; the bias gradients of lin_second_stage_1,
 * lin_second_stage_0, density_layer.2, density_layer.0 are ADDED to g_bias[0..3] (not bit-reproducible); ws: snerf_fmlp_zip_chain_ws_floats(M)
 * floats.  wstream (448 fragments): snerf_amd.mlp.ZipNerfNet._pack_fused_chain. */
long snerf_fmlp_zip_chain_ws_floats(long M);
int snerf_fmlp_zip_chain_bwd(const float* d_rgb, long ld_rgb, const float* d_den, long ld_den, int den_cols, const void* wstream, long n_frags,
                             void* const* bits, void* const* dz, const long* dz_ld, float* const* g_bias, float* ws, long ws_floats, long M,
                             int dtype, void* stream);
/* Colour head of the live mip path's NeRF MLP, fused (s-nerf/model/models.py:283-296: cat([bottleneck, view encoding]) ->
 * cond_layers.0 .. .2 (Linear 128 + ReLU) -> rgb_layer; hidden 1024, 27 view-encoding columns).  Replaces four snerf_linear_fwd
 * launches forward and the four data-gradient launches backward.
 * snerf_fcolour_fwd: CB [M, ldCB] bf16 = [bottleneck 1024 | view encoding 27 | zeros up to column 1056] -> raw_rgb [M,3] fp32.
 *   wstream (336 fragments; cond_layers.0 in k-major order) / bias (13 blocks) from snerf_amd.mlp.fmlp_pack.  acts / act_ld / bits:
 *   HOST arrays of 3 (or all NULL for inference): the three hidden activations ([M, >= 128] bf16) and their ReLU bit masks
 *   (8 * ceil(M / 256) * 2 * 64 words each, snerf_linear_fwd's mask-bit layout for N = 128), stored for the backward pass.
 *   variant: 0; bit 0 selects the alternative input read-ahead depth (tools/fcolour_probe.py).
 * snerf_fcolour_bwd: d_raw_rgb [M,3] fp32 -> dC[0..2] = d pre-activation of cond_layers.2, .1, .0 ([M, >= 128] bf16; the weight-
 *   gradient GEMMs read them) and dB = d pre-activation of the bottleneck layer [M, >= 1024] bf16.  bits[0..3] = the bit masks of
 *   cond_layers.2, .1, .0 and of the bottleneck (N = 1024); wstream (336 fragments) = fmlp_pack of the TRANSPOSED weights; the four
 *   layers' bias gradients are ADDED to g_bias[0..3] (128, 128, 128, 1024 floats) in a fixed order (bit-reproducible).
 *   ws: snerf_fcolour_bwd_ws_floats(M) floats. */
int snerf_fcolour_fwd(const void* CB, long ldCB, const void* wstream, long n_frags, const float* bias, int n_blocks, float* raw_rgb,
                      void* const* acts, const long* act_ld, void* const* bits, long M, int variant, void* stream);
long snerf_fcolour_bwd_ws_floats(long M);
int snerf_fcolour_bwd(const float* d_raw_rgb, const void* wstream, long n_frags, void* const* bits, void* const* dC, const long* dC_ld,
                      void* dB, long dB_ld, float* const* g_bias, float* ws, long ws_floats, long M, void* stream);
/* ... in either 16-bit flavour (library version >= 3; snerf_fcolour_fwd / snerf_fcolour_bwd forward here with SNERF_DT_BF16): dtype =
 * SNERF_DT_BF16 or SNERF_DT_F16 = the type of CB, of the weight stream, of the stored activations and of dC / dB; d_raw_rgb is rounded
 * to it (nearest even).  Nothing is scaled: under an fp16 loss scale d_raw_rgb arrives multiplied by it and the caller unscales what it
 * reads.  raw_rgb, biases and the bias gradients (fixed-order fp32 sums of the unrounded accumulators, bit-reproducible) are fp32 either
 * way.  Any other dtype: SNERF_ERR_ARG before anything touches a device, also for M = 0. */
int snerf_fcolour_fwd_dt(const void* CB, long ldCB, const void* wstream, long n_frags, const float* bias, int n_blocks, float* raw_rgb,
                         void* const* acts, const long* act_ld, void* const* bits, long M, int variant, int dtype, void* stream);
int snerf_fcolour_bwd_dt(const float* d_raw_rgb, const void* wstream, long n_frags, void* const* bits, void* const* dC, const long* dC_ld,
                         void* dB, long dB_ld, float* const* g_bias, float* ws, long ws_floats, long M, int dtype, void* stream);

/* Data-gradient chains of the two 256-wide networks, fused (autograd of NeRF.forward, run_nerf_helpers.py:83-139, and of the mip
 * path's proposal MLP, s-nerf/model/models.py:237-262): d raw -> d pre-activation of every layer in ONE launch; replaces ten
 * (classic) / four (proposal) snerf_linear_fwd data-gradient launches.  Every step's output is stored for snerf_linear_wgrad.
 * net 0 (classic): d_raw [M,4] fp32 (d rgb, d alpha); dz[0] = d views_linears.0 ([M, >= 128] bf16), dz[1] = d feature_linear output
 *   ([M, >= 256]), dz[2..9] = d pts_linears.7 .. .0; bits[0..7] = masks of pts_linears.0 .. .7, bits[8] = of views_linears.0;
 *   wstream: 1104 fragments.  net 1 (proposal): d_raw [M] (d raw density); dz[0..3] = d layers.3 .. .0; bits[0..3] = masks of
 *   layers.0 .. .3; wstream: 400 fragments.  wstream = snerf_amd.mlp.fmlp_pack of the transposed weights in chain order.
 * The bias gradient of step i is ADDED to g_bias[i] (width of dz[i] floats); the partial sums meet in LDS atomics, so the result is
 * NOT bit-reproducible run to run (the deterministic mode keeps the per-layer launches).  ws: snerf_fchain_bwd_ws_floats(net, M). */
long snerf_fchain_bwd_ws_floats(int net, long M);
int snerf_fchain_bwd(int net, const float* d_raw, const void* wstream, long n_frags, void* const* bits, void* const* dz, const long* dz_ld,
                     float* const* g_bias, float* ws, long ws_floats, long M, void* stream);
/* ... in either 16-bit flavour (library version >= 2; snerf_fchain_bwd forwards here with SNERF_DT_BF16): dtype = SNERF_DT_BF16 or
 * SNERF_DT_F16 = the type of the weight stream and of every dz; d_raw is rounded to it (nearest even).  Nothing is scaled: under an fp16
 * loss scale d_raw arrives multiplied by it and the caller unscales what it reads.  The bias gradients are fp32 sums of the unrounded
 * accumulators either way.  Any other dtype: SNERF_ERR_ARG before anything touches a device. */
int snerf_fchain_bwd_dt(int net, const float* d_raw, const void* wstream, long n_frags, void* const* bits, void* const* dz, const long* dz_ld,
                        float* const* g_bias, float* ws, long ws_floats, long M, int dtype, void* stream);

/* ---- deterministic mode ("deterministic mode for parity tests") ------------------------------------------
 * The weight gradient normally lands in dW by fp32 atomics from the M slices (order varies run to run).  snerf_linear_wgrad_det makes
 * every slice store its partial tile into `ws` (snerf_linear_wgrad_ws_floats(...) floats) and folds them in slice order: bit-identical
 * gradients run to run.  snerf_colsum_f32_det is the single-workgroup form of snerf_colsum_f32; snerf_linear_fwd takes variant bit 8
 * (| 256) to fold its bias-gradient partials in a fixed order. */
long snerf_linear_wgrad_ws_floats(int M, int N, int K, long ldz, long ldx, int dtype, int variant);
int snerf_linear_wgrad_det(const void* Z, long ldz, const void* X, long ldx, float* dW, long ldw, const void* zeros, int M, int N, int K,
                           int n_valid, int k_valid, int dtype, int variant, float* ws, long ws_floats, void* stream);
int snerf_colsum_f32_det(const float* x, long ld, long M, int C, float* out, void* stream);

/* ---- classic-path ray front end ---------------------------------------------------------------------
 * snerf_classic_get_rays  = get_rays (s-nerf/model/run_nerf_helpers.py:247-258): pinhole rays of an H x W frame, pixel centres at
 *   +0.5, principal point (cx, cy) = `ori_points` (default W/2, H/2); c2w_host: HOST pointer to the [3,4] camera-to-world matrix.
 * snerf_classic_ndc_rays  = ndc_rays (:314-332).
 * snerf_classic_ray_batch = the front half of render() (s-nerf/model/render.py:50-77) in one launch: rays from c2w_host (whole
 *   frame, n = H*W) or the given rays_o / rays_d [n,3]; unit view directions from the pre-NDC directions; c2w_static_host
 *   (c2w_staticcam) replaces the rays but not the view directions; NDC warp with near = 1; rows [n, ld] =
 *   [o3, d3, near, far, (depth), (viewdir3)] exactly as render_rays reads them (render.py:326-329). */
int snerf_classic_get_rays(int H, int W, double focal, double cx, double cy, const float* c2w_host, float* rays_o, float* rays_d, void* stream);
int snerf_classic_ndc_rays(int H, int W, double focal, float near, const float* rays_o, const float* rays_d, long n, float* o_out,
                           float* d_out, void* stream);
int snerf_classic_ray_batch(int H, int W, double focal, double cx, double cy, const float* c2w_host, const float* c2w_static_host,
                            const float* rays_o, const float* rays_d, long n, int ndc, float near, float far, const float* depths,
                            int use_viewdirs, float* rows, int ld, void* stream);

/* snerf_zip_encode_bwd without the atomic wall ("binned" table gradient): the contributions of gridencoder.cu:248-340 are written
 * out as records partitioned by destination (level, range of 4096 (C = 4) / 16384 (C = 1) table rows, replica), then one workgroup per
 * bin accumulates its records in LDS with 64-bit fixed-point integer atomics (scale from snerf_zip_bin_scale) and writes its rows back: no L2
 * atomics on the hashed levels, and a gradient that is BIT-IDENTICAL run to run (integer addition is order-independent).
 * Three calls: pass 0 counts (counts [L,1024] int32, zeroed by the caller) and reserves every workgroup's range inside the bins it
 * touches (wg_offsets: uint32 [L, ceil(R*S/256), 1024], need not be initialised); the caller scans the counts into `starts`
 * ([L,1024] int64, exclusive prefix sums over the flattened bins); pass 1 writes the records (rec_row uint16 [capacity], rec_val fp32
 * [capacity, max(C, 2)] -- for C = 1 a record is one 8-byte {row, value} pair in rec_val and rec_row is not touched; capacity >=
 * R*S*n*8*L is always enough) -- staged per workgroup in LDS and written run by run, so that a store instruction covers consecutive
 * records of ONE (workgroup, bin) range instead of 64 different lines (n <= 8; pass 3 is the same write with every thread storing its
 * records where they fall: more than 8 multisamples, A/B probes); pass 2 accumulates into grad_table (fp32, +=).  ksplit_host: HOST int[L],
 * replicas per row range (> 1 for levels with few, hot rows: they meet in g64, an int64 image of table rows [0, g64_rows) zeroed by
 * the caller); level_rows_host: HOST int[L], table rows per level -- a level needs ceil(rows / 4096 or 16384) * ksplit <= 1024 bins,
 * anything larger is refused with a bad-argument status (use snerf_zip_encode_bwd, the atomic scatter). */
int snerf_zip_encode_bwd_binned(int pass, const float* tdist, const float* origins, const float* directions, const float* radii,
                                const float* base_x, const float* base_y, const float* deg_jitter, const int* offsets,
                                const int* grid_sizes, const void* grad_feat, long ld, float* grad_table, long R, int S, int L, int C, int n,
                                int m, float Sl, int H, float std_scale, int feat_dtype, const int* ksplit_host, const int* level_rows_host,
                                int* counts, void* wg_offsets, const long* starts, void* rec_row, float* rec_val, long capacity, void* g64,
                                long g64_rows, const int* scale_exp, void* stream);
/* out[c] += sum over the M rows of x[m, c] (fp32, any number of columns C <= ld): the bias gradients behind the per-ray rows of the GLO
 * branch (snerf_colsum_f32 serves the heads: C <= 8).  deterministic != 0: one fixed summation order. */
int snerf_colsum_wide_f32(const float* x, long ld, long M, int C, float* out, int deterministic, void* stream);
/* GLO modulation of the zipnerf NeRF MLP's bottleneck (internal/models.py:620-630; Model.num_glo_features > 0, configs/360_glo*.gin):
 * out[p, c] = X[p, c] * exp(SS[p / S, c]) + SS[p / S, B + c] for the B bottleneck columns of the R * S samples; SS [R, >= 2 B] fp32 =
 * (scale | shift) per ray, the output of lin_glo_0 / lin_glo_1 on the ray's GLO vector.  X / out in `dtype` (fp32 or bf16).
 * _bwd: dXm = d loss / d out -> dX = dXm * exp(scale) + d_head (fp32 [R * S, >= n_head]: gradients that enter columns < n_head of x
 * directly -- raw density and the semantic logits, models.py:511,594), dSS [R, >= 2 B] = (sum_s dXm * X * exp(scale) | sum_s dXm), and
 * dxsum [R, >= B] = per-ray column sums of the stored dX (their sum over the rays is the bias gradient of density_layer.2).  One
 * workgroup per ray, samples in order: deterministic. */
int snerf_zip_glo_modulate(const void* X, long ldx, const float* SS, long ldss, long R, int S, int B, void* out, long ldo, int dtype, void* stream);
int snerf_zip_glo_modulate_bwd(const void* dXm, long lddxm, const void* X, long ldx, const float* SS, long ldss, const float* d_head, long ldh,
                               int n_head, long R, int S, int B, void* dX, long lddx, float* dSS, long lddss, float* dxsum, long ldsum,
                               int dtype, void* stream);
/* The fixed-point scale of one binned launch: scale_exp (device int[2]) [0] = e such that 2^e * max |grad_feat[:rows, :cols]| lies in
 * [2^33, 2^34) -- the accumulation grid follows the magnitude of the gradient (a loss-scaled 1e-12 gradient keeps 34 bits below its
 * largest entry); pass 2 reads it.  [1] = the bits of that maximum; a NaN / +-Inf in grad_feat (an fp16 overflow) leaves 0x7f800000
 * there and pass 2 then writes a NaN into grad_table[0]: the launch's records are meaningless and a found-inf check must see it. */
int snerf_zip_bin_scale(const void* grad_feat, long ld, long rows, int cols, int feat_dtype, int* scale_exp, void* stream);

/* Featurisation backward to the RAYS -- `cal_input_grad` of the reference (internal/models.py:491 -> gridencoder/grid.py:65-89 ->
 * gridencoder.cu:199-244, 343-369), needed by the pose refinement of zipnerf/train.py:187-197: d loss / d (origins, directions, base_x,
 * base_y) [R,3] each (ACCUMULATED: the caller zeroes them) from grad_feat = d loss / d features [R*S, ld] (feat_dtype), through the
 * trilinear derivative of every level, the erf down-weighting's dependence on the contracted std, the contraction's Jacobian
 * (coord.py:51-63) and the multisample helix (render.py:129-168).  table: the gather table of snerf_zip_encode_fwd (table_dtype 0 =
 * fp32, 2 = fp16).  snerf_zip_composite_bwd's `g_dirs` (optional, [R,3], written) is d loss / d directions through the interval
 * lengths (t1 - t0) |d| (render.py:170-176). */
int snerf_zip_encode_ray_bwd(const float* tdist, const float* origins, const float* directions, const float* radii, const float* base_x,
                             const float* base_y, const float* deg_jitter, const void* table, const int* offsets, const int* grid_sizes,
                             const void* grad_feat, long ld, long R, int S, int L, int C, int n, int m, float Sl, int H, float std_scale,
                             int table_dtype, int feat_dtype, float* g_origins, float* g_directions, float* g_base_x, float* g_base_y,
                             void* stream);

/* snerf_adam_step with the step count t in DEVICE memory: *step_dev is incremented, then used for the bias corrections -- no launch
 * argument depends on host state, so a whole training step can be captured in a hipGraph and replayed. */
int snerf_adam_step_dev(float* p, float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps, int* step_dev,
                        float grad_scale, int zero_grad, void* stream);

/* The Adam step with the gradient hygiene of s-nerfpp/zipnerf/internal/train_utils.py:234-243 (clip_gradients, called every step at
 * zipnerf/train.py:336) folded into the same pass over the arena, in the reference's order: global-norm clip (clip_coef: device
 * scalar from snerf_grad_clip_coef, or NULL), value clip (grad_max_val > 0, torch.clamp semantics: NaN stays NaN), then `nonfinite`:
 * 0 = keep, 1 = NaN / +-Inf -> 0 (a poisoned gradient never reaches m, v or the parameters), 2 = torch.nan_to_num_ exactly (NaN -> 0,
 * +-Inf -> +-FLT_MAX).  step_dev != NULL: step count in device memory (incremented first); lr_dev != NULL: learning rate read from
 * device memory (a captured hipGraph then follows an lr schedule). */
int snerf_adam_step_ex(float* p, float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps, int step,
                       int* step_dev, const float* lr_dev, float grad_scale, int zero_grad, int nonfinite, float grad_max_val,
                       const float* clip_coef, void* stream);
/* snerf_adam_step_ex with a counter: *dropped (device uint64, 8-byte aligned, never reset by the launch; NULL = off) += the number of
 * NaN / +-Inf gradient elements the launch saw, whatever `nonfinite` does with them.  The reference trains fp16 under GradScaler
 * (zipnerf/train.py:44,331), which skips such a step; with a static loss scale the drop would otherwise be silent. */
int snerf_adam_step_cnt(float* p, float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps, int step,
                        int* step_dev, const float* lr_dev, float grad_scale, int zero_grad, int nonfinite, float grad_max_val,
                        const float* clip_coef, void* dropped, void* stream);
/* Plain SGD over a flat fp32 buffer (torch.optim.SGD without momentum or weight decay: the optimiser of the reference's learned camera
 * poses, s-nerfpp/zipnerf/internal/train_utils.py:290, stepped after clip_gradients(posenet), train.py:343):
 * p -= lr * hygiene(g * grad_scale), then g = 0.  The hygiene, its order and the `nonfinite` codes are snerf_adam_step_ex's (clip_coef:
 * nullable device float; grad_max_val > 0: value clip; nonfinite 0 / 1 / 2); the product lr * g and the difference are separate fp32
 * operations.  *dropped (device uint64, 8-byte aligned, nullable) += the NaN / +-Inf gradient elements met.  count = 0 is a no-op; a
 * null p or g, count < 0, a pointer off 4-byte alignment or a nonfinite code outside 0..2 return 1 before any launch. */
int snerf_sgd_step(float* p, float* g, long count, float lr, float grad_scale, float grad_max_val, const float* clip_coef, int nonfinite,
                   void* dropped, void* stream);
/* torch.nn.utils.clip_grad_norm_ coefficient over a flat gradient arena: out[0] = min(1, max_norm / (|grad_scale| * ||g||_2 + 1e-6)),
 * out[1] = the norm.  ws: >= 1024 doubles of device scratch.  Fixed reduction order (deterministic).  A NaN in g gives out[0] = out[1]
 * = NaN (torch's clamp(max=1) keeps the NaN too): snerf_adam_step_ex then sees NaN gradients everywhere and its `nonfinite` policy decides
 * (1 / 2: the step applies an all-zero gradient; 0: parameters poisoned, as torch's are).  +-Inf in g gives out[0] = 0. */
int snerf_grad_clip_coef(const float* g, long n, float grad_scale, float max_norm, void* ws, float* out, void* stream);
/* The found-inf check of a dynamic loss scaler (torch.cuda.amp.GradScaler, which accelerate wraps around the reference's fp16 training:
 * s-nerfpp/zipnerf/train.py:44,215,331): *flag |= 1 when any of the n fp32 gradients is NaN or +-Inf.  The caller zeroes *flag
 * (device int); the binned table gradient marks an overflowed feature gradient by a NaN in its first element (snerf_zip_encode_bwd_binned). */
int snerf_nonfinite_flag(const float* g, long n, int* flag, void* stream);

/* Learned camera pose (pose_refine = True; s-nerf/model/poses.py:6-36 LearnPose, utils/lie_group_helper.py:47-81) applied to a ray
 * batch: the pose branch of sample_rays (utils/sample_utils.py:421-435).  Row `cam` of the table r [n_cams,3] (axis-angle) / t
 * [n_cams,3] (NULL = no translation) gives R = I + (sin th / th) K + ((1 - cos th) / th^2) K^2, K = skew(r), th = |r| + 1e-15, formed
 * in double by every workgroup and rounded once; directions_out = R d, viewdirs_out = R v (fp32, not contracted), origins_out = o + t
 * (one fp32 add: the reference shifts the origins and does not rotate them).  r = 0 gives R = I exactly: the outputs equal the inputs
 * bit for bit.  cam_dev: int64 [1] in device memory (a batcher's img_out as it is: no host read), NULL = use cam_host; a device index
 * outside the table makes the kernel return without a store.  The outputs [n,3] must not overlap the inputs (the backward needs the
 * untransformed d, v), each other or pose_out.  pose_out [3,4] (nullable) = the transform that was applied.  n = 0 is a no-op; bad arguments (a null required
 * pointer, n < 0, n_cams < 1, cam_host outside the table, overlap) return 1 before any launch. */
int snerf_pose_apply(const float* r, const float* t, int n_cams, const long* cam_dev, int cam_host, const float* origins,
                     const float* directions, const float* viewdirs, long n, float* origins_out, float* directions_out,
                     float* viewdirs_out, float* pose_out, void* stream);
/* The ray gradients of a step (g_o, g_d, g_v [n,3] = d loss / d the TRANSFORMED origins / directions / viewdirs) and the untransformed
 * directions / viewdirs [n,3] reduced to the gradient of table row `cam`: g_t = sum g_o and G[i][j] = sum (g_d[i] d[j] + g_v[i] v[j]),
 * summed in double in an order that depends on n only (no floating-point atomics: bit-reproducible), then chained through the formula
 * of snerf_pose_apply as autograd differentiates it (the term through |r| dropped at |r| = 0, torch's subgradient), in double, rounded
 * once and ADDED into row `cam` of grad_r [n_cams,3] / grad_t [n_cams,3] (either nullable, not both; g_o nullable without grad_t);
 * other rows are not touched.  ws: >= snerf_pose_grad_ws(n) doubles of device scratch, ws_doubles = its length (short = bad
 * argument).  Camera index, n = 0 and bad arguments as for snerf_pose_apply.  Linear in the rays: per-slice results add up. */
int snerf_pose_grad(const float* r, int n_cams, const long* cam_dev, int cam_host, const float* g_o, const float* g_d, const float* g_v,
                    const float* directions, const float* viewdirs, long n, double* ws, long ws_doubles, float* grad_r, float* grad_t,
                    void* stream);
/* doubles of scratch snerf_pose_grad needs for n rays */
long snerf_pose_grad_ws(long n);
/* The learned pose COMPOSED with the initial one (test-time pose refinement, s-nerf/eval.py:77-114: rays generated from
 * make_c2w(r, t) @ init_c2w[img]), applied to the rays of the initial pose: R as in snerf_pose_apply (double, rounded once);
 * directions_out = R d, viewdirs_out = R v, origins_out = (R o) + t -- the camera centre turns with the rotation -- as separate fp32
 * operations in a fixed order, not contracted; t NULL: origins_out = R o.  r = 0 with t NULL or zero returns the three inputs bit for
 * bit.  Camera index (device or host; a device index outside the table stores nothing), pose_out, n = 0, the overlap rules and bad
 * arguments as for snerf_pose_apply. */
int snerf_pose_compose_apply(const float* r, const float* t, int n_cams, const long* cam_dev, int cam_host, const float* origins,
                             const float* directions, const float* viewdirs, long n, float* origins_out, float* directions_out,
                             float* viewdirs_out, float* pose_out, void* stream);
/* The gradient of table row `cam` under snerf_pose_compose_apply: g_t = sum g_o and G[i][j] = sum (g_d[i] d[j] + g_v[i] v[j] +
 * g_o[i] o[j]) with the UNtransformed origins / directions / viewdirs [n,3], summed, chained and ADDED into grad_r / grad_t (either
 * nullable, not both) exactly as snerf_pose_grad does: doubles in an order that depends on n only, no floating-point atomics, the
 * same bits every call.  g_o and origins are required, with or without grad_t.  ws: >= snerf_pose_grad_ws(n) doubles (there are
 * still twelve sums).  Camera index, n = 0 and bad arguments as for snerf_pose_grad.  Linear in the rays: per-slice results add up. */
int snerf_pose_compose_grad(const float* r, int n_cams, const long* cam_dev, int cam_host, const float* g_o, const float* g_d,
                            const float* g_v, const float* origins, const float* directions, const float* viewdirs, long n, double* ws,
                            long ws_doubles, float* grad_r, float* grad_t, void* stream);

/* Per-ray learned poses (path C: s-nerfpp/zipnerf/train.py:177-213, internal/posenet_v2.py): a batch mixes cameras, every ray names its
 * row of the table.  snerf_pose_table writes table_out [n_cams,3,4], one thread per camera: the rotation of row c formed in double from
 * the fp32 r [n_cams,3] and rounded once (as snerf_pose_apply does; r = 0 gives I exactly), column 3 = fp32(t[c] * t_ratio)
 * (posenet_v2.py:89,99; zeros when t is NULL).  table_out must not overlap r or t.  Bad arguments (a null r or table_out, n_cams < 1,
 * overlap) return 1 before any launch. */
int snerf_pose_table(const float* r, const float* t, int n_cams, float t_ratio, float* table_out, void* stream);
/* The table of snerf_pose_table (16-byte aligned) applied ray by ray (train.py:186-196): cam [n] fp32 holds each ray's row, truncated
 * toward zero like the reference's .int(); origins_out = o + t_eff (one fp32 add), and for x in (directions, viewdirs, base_x, base_y)
 * x'_i = (R_i0 x_0 + R_i1 x_1) + R_i2 x_2 as separate fp32 operations, not contracted.  A ray whose index is outside [0, n_cams) (or
 * NaN) is copied through unchanged.  The inputs are never written; an output that overlaps an input, the table, cam or another output
 * is a bad argument, like a null pointer, n < 0 or n_cams < 1 (status 1 before any launch).  n = 0 is a no-op. */
int snerf_pose_rays_apply(const float* table, int n_cams, const float* cam, const float* origins, const float* directions,
                          const float* viewdirs, const float* base_x, const float* base_y, long n, float* origins_out,
                          float* directions_out, float* viewdirs_out, float* base_x_out, float* base_y_out, void* stream);
/* doubles of scratch snerf_pose_rays_grad needs for n rays spread over a table of n_cams rows (0 for n <= 0 or n_cams < 1) */
long snerf_pose_rays_grad_ws(long n, int n_cams);
/* The gradient of the table under snerf_pose_rays_apply, segmented by camera: g_o .. g_by [n,3] = d loss / d the TRANSFORMED origins,
 * directions, viewdirs, base_x, base_y, and the UNtransformed directions, viewdirs, base_x, base_y [n,3].  For every camera c that owns
 * at least one ray, G_c[i][j] = sum over its rays of (g_d[i] d[j] + g_v[i] v[j]) + (g_bx[i] bx[j] + g_by[i] by[j]) and g_t,c = t_ratio *
 * sum g_o, summed in double in an order that depends on (n, n_cams) only -- no floating-point atomics, the same bits every call --
 * chained through row c of r as snerf_pose_grad chains, rounded once to fp32 and ADDED into row c of grad_r / grad_t [n_cams,3] (either
 * nullable, not both; g_o nullable without grad_t).  Rows of cameras without a ray in the batch are not stored to; rays with an index
 * outside the table take no part.  ws: >= snerf_pose_rays_grad_ws(n, n_cams) doubles, ws_doubles = its length (short = bad argument).
 * n = 0 is a no-op; a null required pointer, n < 0 or n_cams < 1 return 1 before any launch.  Linear in the rays: per-slice results
 * add up. */
int snerf_pose_rays_grad(const float* r, int n_cams, float t_ratio, const float* cam, const float* g_o, const float* g_d, const float* g_v,
                         const float* g_bx, const float* g_by, const float* directions, const float* viewdirs, const float* base_x,
                         const float* base_y, long n, double* ws, long ws_doubles, float* grad_r, float* grad_t, void* stream);

/* Learned depth confidence (depth_conf = True, precompute_conf = True; s-nerf/model/confidence.py:65-73,193-206) on the rays of one
 * batch: conf[r] = sum_k w_k maps[k, slot, row_r, col_r] / sum_k w_k with w_k = sigmoid(lambdas[k, i]), i the image of the batch and
 * slot = slot_of_image[i] its position among the images with maps (the reference indexes the maps by position in i_train and lambdas
 * by image: confidence.py:193,196), and conf[r] = 1 where sky[i, row_r, col_r] != 0 (confidence.py:202-203).
 * maps fp32 [M,P,H,W] (M modes, 1..8; P images with maps), slot_of_image int32 [n_images] (in [0,P) or -1), lambdas fp32 [M,n_images],
 * sky uint8 [n_images,H,W] (nullable), coords int64 [n,2] = (row, col) (a batcher's sel_coords).  w_k is formed in double and rounded
 * once; the sums run in the reference's mode order as separate fp32 ops, then one fp32 division.  img_dev: int64 [1] in device memory
 * (a batcher's img_out as it is: no host read), NULL = use img_host.  A device index outside the table, a slot of -1 (or past P) and a
 * ray whose (row, col) lies outside the image give conf = 1 (the reference raises).  n = 0 is a no-op; bad arguments (a null required
 * pointer, M outside 1..8, P / H / W / n_images < 1, n < 0, img_host outside the table) return 1 before any launch. */
int snerf_conf_apply(const float* maps, int M, int P, int H, int W, const int* slot_of_image, const float* lambdas, int n_images,
                     const unsigned char* sky, const long* img_dev, int img_host, const long* coords, long n, float* conf, void* stream);
/* g_conf [n] = d loss / d conf (snerf_mip_loss_tail_gconf) reduced to the gradient of column i of lambdas: the M sums
 * A_k = sum_r g_conf[r] maps[k, slot, row_r, col_r] over the rays that are not sky (and inside the image), in double in an order that
 * depends on n only (a partial and a finish launch, no floating-point atomics: bit-reproducible), then
 * d lambda_k = s_k (1 - s_k) / S (A_k - sum_j s_j A_j / S), s = sigmoid(lambdas[:, i]) and S = sum s in double, rounded once and ADDED
 * into grad_lambdas[k, i] (fp32 [M,n_images]); the other columns are not touched.  An index outside the table or a slot of -1 adds
 * nothing.  ws: >= snerf_conf_grad_ws(n) doubles of device scratch, ws_doubles = its length (short = bad argument).  Image index,
 * n = 0 and bad arguments as for snerf_conf_apply.  Linear in the rays: per-slice results add up. */
int snerf_conf_grad(const float* maps, int M, int P, int H, int W, const int* slot_of_image, const float* lambdas, int n_images,
                    const unsigned char* sky, const long* img_dev, int img_host, const long* coords, const float* g_conf, long n,
                    double* ws, long ws_doubles, float* grad_lambdas, void* stream);
/* doubles of scratch snerf_conf_grad needs for n rays */
long snerf_conf_grad_ws(long n);

/* The reprojection confidence maps of one base image on the device: the rgb, ssim and depth modes of Confidence.precompute_conf_map
 * (s-nerf/model/confidence.py:78-112 = get_reproj_conf, model/loss.py:271-327, over reproj_err :218-268, warping :138-179,
 * sample_points :122-135 and utils/pytorch_msssim ssim).  One pass per neighbour, in the order given (select_conf_depends' sel_ids:
 * the LAST neighbour is special): every base pixel is projected into the neighbour with the base depth, base_pose and the general
 * affine inverse of the neighbour's pose (double from the fp32 entries, rounded once); it is in view iff its rounded (rintf, half to
 * even) coordinates lie inside the image, compared as floats (non-finite = out of view; points behind the camera are not rejected).
 * In view: fake = grid_sample of the neighbour image (align_corners = False, zero padding, at u / ((W-1)//2) - 1, v / ((H-1)//2) - 1:
 * the reference's integer division), tgt_depth = the neighbour's depth at the rounded pixel; errors rgb = mean_c |base - fake|, ssim =
 * 1 - mean_c SSIM of the two full masked images (11 x 11 Gaussian, sigma 1.5, zero padding 5, C1 = 0.01^2, C2 = 0.03^2: L = 1, images
 * in [0,1]), depth = |dep - tgt_depth| / max(tgt_depth, 1e-10), flagged where > tau, then clamped to tau.  Per pass and mode
 * (emax - err) / (emax - emin), emax / emin over the pass's in-view pixels (emax == emin: 0 / 0 = NaN, as the reference), is added on
 * the in-view pixels; the result is sum / max(count, 1), and with the depth bit every mode's map is 0 on the pixels in view and over
 * tau in the last pass only.  A pass with no pixel in view is skipped entirely (the reference raises) and is not the last pass.
 * Images smaller than the 11 x 11 window (where the reference shrinks the window) are not the reference's: the window stays 11 x 11,
 * and for H or W < 3, where (W-1)//2 = 0 leaves the sample point undefined, fake is 0.
 * images [N,H,W,3] uint8 (images_u8 = 1: decoded as float32(k / 255.0)) or fp32 in [0,1], depths [N,H,W], poses [N,3,4], intrinsics
 * [N,4] = (cx, cy, fx, fy), all in device memory; neighbours is a HOST array.  modes: bit 0 rgb, 1 ssim, 2 depth; out_* [H,W] fp32,
 * required iff its bit is set.  ws: >= snerf_reproj_conf_ws(H, W) bytes of device scratch, 4-byte aligned.  No host read, no sync, no
 * floating-point atomics: bit-reproducible and capturable in a graph.  n_neighbours = 0 writes zeros.  Bad arguments (a null required
 * pointer, N / H / W < 1, base or a neighbour outside [0,N), n_neighbours < 0 or > 0 with neighbours NULL, modes outside 1..7, an
 * output missing for a set bit, a short or null workspace, tau not finite) return 1 before any launch. */
int snerf_reproj_conf(const void* images, int images_u8, const float* depths, const float* poses, const float* intrinsics, int N, int H,
                      int W, int base, const int* neighbours, int n_neighbours, int modes, float tau, void* ws, long ws_bytes,
                      float* out_rgb, float* out_ssim, float* out_depth, void* stream);
/* bytes of scratch snerf_reproj_conf needs for H x W images (0 for H or W < 1) */
long snerf_reproj_conf_ws(int H, int W);

/* Frame metrics on the device: what image.MetricHarness (s-nerfpp/zipnerf/internal/image.py:110-125: skimage's PSNR of the uint8 RGB
 * images, its SSIM of their 8-bit grey images) and eval.py's mse_to_psnr (s-nerf/eval.py:152) compute per rendered frame, F frames per
 * call.  pred [F,H,W,3] fp32; gt [F,H,W,3] fp32 or uint8 (gt_u8 = 1); out [F,5] DOUBLE: mse_f, psnr_f, mse_u8, psnr_u8, ssim.
 * Quantisation q(x) = trunc(x * 255.f) (one fp32 product, truncated toward zero; below 0 -> 0, above 255 -> 255, NaN -> 0: numpy's
 * cast is undefined outside (-1, 256)); a uint8 gt is used as it is.  mse_f: d = pred - g and d * d as separate fp32 ops, g = gt or
 * float32(k / 255.0) for a uint8 gt, the squares summed in double, over 3 H W; psnr_f = -10 / ln 10 * ln(mse_f).  mse_u8: the squared
 * differences of the quantised samples summed as an integer, over 3 H W; psnr_u8 = 10 log10(255^2 / mse_u8) (+inf for equal images).
 * Grey = (r wr + g wg + b wb + (1 << (shift - 1))) >> shift on the quantised channels, gray_w = {wr, wg, wb, shift} (a HOST array) or
 * NULL for {9798, 19235, 3735, 15}, OpenCV 4's 8-bit RGB2GRAY ({4899, 9617, 1868, 14}: OpenCV 3's).  ssim: skimage's
 * structural_similarity(data_range = 255) defaults on the grey images: 7 x 7 uniform window, K1 = 0.01, K2 = 0.03, sample covariance
 * (49 / 48), a border of 3 cropped; window sums exact in int32, the rest in double, the mean over the (H - 6)(W - 6) cropped pixels.
 * ws: >= snerf_frame_metrics_ws(F, H, W) bytes of device scratch, 8-byte aligned.  No host read, no sync, no atomics: every sum runs in
 * an order that depends on the shape only (bit-reproducible), and the call can be captured in a graph.  Bad arguments (a null pred /
 * gt / ws / out, F < 1 or > 65535, H or W < 7: the window does not fit, where skimage raises; a short or misaligned workspace; a shift
 * outside 1..20, a negative weight or weights whose sum exceeds 1 << shift) return 1 before any launch. */
int snerf_frame_metrics(const float* pred, const void* gt, int gt_u8, int F, int H, int W, const int* gray_w, void* ws, long ws_bytes,
                        double* out, void* stream);
/* bytes of scratch snerf_frame_metrics needs (0 for F < 1 or > 65535, H < 7 or W < 7) */
long snerf_frame_metrics_ws(int F, int H, int W);

/* First-hit ray / triangle-mesh tracer (csrc/meshtrace.hip): what `raytracing.RayTracer(vertices, faces).trace(ray_o, ray_d)` gives
 * s-nerfpp/stage1_code/utils_render.py:839-868 (the mesh depth behind fg_depth of snerf_fg_paste) and stage0_code/utils_render.py:755-776
 * (the instance mask).  That library is not in the reference tree: its behaviour at edges, its normals' orientation and whether it
 * accepts hits beyond its max depth of 100 are NOT pinned.  Defined here: a hit needs 0 < t < t_max with t the ray parameter of the
 * un-normalised direction; the nearest hit wins; a miss has face id -1 and zero position and normal.  The test is watertight (Woop's
 * sheared edge functions, exactly antisymmetric per edge: a ray through a shared edge or a vertex of a closed surface hits).
 *
 * The mesh is handed over ORDERED: faces [F,3] int32 sorted by the caller so that neighbours in the array are neighbours in space (the
 * Morton code of the object-space centroids; any order is correct, a bad one is slow), face_ids [F] int32 = the caller's own id of
 * each ordered face (NULL: the ordered index).  snerf_mesh_prepare applies transform (12 floats in DEVICE memory, a row-major 3 x 4
 * affine map; NULL: none) to vertices [V,3] fp32 and fills ws (>= snerf_mesh_ws_bytes(F) bytes of device memory, 16-byte aligned)
 * with the triangle records and the boxes of the 64-triangle chunks and of the groups of 64 chunks; it is F triangles of work and is
 * repeated for every new transform.  A face with an index outside [0, V), a non-finite transformed vertex or a zero cross product is
 * dropped there (never hit); no vertex is read through an unchecked index.  F = 0 is valid (ws is not touched and may be NULL, here
 * and in the trace entries: everything misses).  Bad arguments (F or V < 0, a null faces / ws, null vertices with V > 0, a short or
 * misaligned ws) return 1 before any launch. */
long snerf_mesh_ws_bytes(int F);
int snerf_mesh_prepare(const float* vertices, int V, const int* faces, const int* face_ids, int F, const float* transform, void* ws,
                       long ws_bytes, void* stream);
/* General rays: rays_o, rays_d [R,3] fp32 -> depth [R] = t of the nearest hit or t_max, and, each optional (NULL), face_id [R] int32,
 * positions [R,3] = o + t d, normals [R,3] = the unit normal (b - a) x (c - a) of the hit face, not turned towards the ray.  64
 * consecutive rays share a wave.  A ray with a non-finite component or a zero direction misses.  flags: bit 0 = no box culling (every
 * chunk is entered: the all-pairs flavour, for measurements), bit 1 = chunks read through wave-uniform loads instead of staged in LDS
 * (same results, slower with culling).  No host read, no atomics; what a ray returns does not depend on the other rays of the call.  R = 0 is valid.  Bad
 * arguments (F or R < 0, t_max not a positive finite number, unknown flag bits, a null rays_o / rays_d / depth, a null or misaligned
 * ws with F > 0) return 1 before any launch. */
int snerf_mesh_trace(const void* ws, int F, const float* rays_o, const float* rays_d, long R, float t_max, int flags, float* depth,
                     int* face_id, float* positions, float* normals, void* stream);
/* Camera rays generated in the kernel, one 8 x 8 pixel tile per wave: pixel (x, y) sends d = (((x + c) - cx) / fx, -(((y + c) - cy) / fy), -1)
 * from the origin, c = 0.5 with pixel_center (stage 0's get_ray_directions) and 0 without (stage 1's get_ray_d_from_xy), in fp32
 * operation by operation as written, so t is the z-depth; the intersection routine is snerf_mesh_trace's (the same bits for the same
 * rays).  mask [H,W,3] uint8 or NULL: only pixels with channel 0 > 0 are traced, the others get depth 0 and hit 0.  depth [H,W] = t of a
 * hit, miss_value on a traced miss (stage 1: t_max = 99, miss_value = 0.1 is `depth[depth >= 99.] = .1`); hit [H,W,3] uint8 (optional)
 * = 255 on a hit (stage 0's mask with t_max = 100).  flags as above.  H = 0 or W = 0 is valid.  Bad arguments (F, H or W < 0, H W >=
 * 2^31, fx or fy zero or not finite, cx or cy not finite, t_max not a positive finite number, unknown flag bits, a null depth, a null
 * or misaligned ws with F > 0) return 1 before any launch. */
int snerf_mesh_trace_pinhole(const void* ws, int F, float fx, float fy, float cx, float cy, int pixel_center, int H, int W,
                             const void* mask, float t_max, float miss_value, int flags, float* depth, void* hit, void* stream);
/* The instance image and mask of s-nerfpp/api_code/mesh_renderer.py:36-88 render(cam) from the prepared mesh: the pixel-centre rays of
 * snerf_mesh_trace_pinhole (pixel_center = 1, no mask; row 0 on top, so the reference's vertical flip has no counterpart) and the same
 * walk, so hit / miss / face are that entry's bits for the same ws, camera and t_max.  nvdiffrast and kaolin are not in the reference
 * tree: their fill rule at an edge and their near plane are NOT pinned.  The winning triangle is intersected once more with the same
 * sheared edge functions; (u, v, w) / ((u + v) + w) are the barycentrics of its vertices (a, b, c), perspective-correct by construction.
 * The attribute source is exactly one of
 *   vertex colours: vertex_color [V,3] fp32 through faces [F,3] int32 (the ORDERED faces snerf_mesh_prepare got);
 *   textures: uvs [U,2] fp32 through face_uvs_idx [F,3] int32 and face_material_idx [F] int32, both in the tracer's order; a uv index
 *     outside [0, U) means uv = (0, 0) (the reference's appended zero row), a material index outside [0, M) leaves the colour 0 with the
 *     mask at 255.  texels: n_texels x (r, g, b, 0) fp32, 16-byte aligned, all materials back to back; materials [M,4] int32, 16-byte
 *     aligned = (texel offset, Hm, Wm, 0) per material, row-major maps, a 1 x 1 map being a constant Kd; an entry that does not lie
 *     inside [0, n_texels) gives colour 0.  The fetch is grid_sample(map, (2u - 1, -(2v - 1)), 'bilinear', align_corners = False,
 *     padding_mode = 'border') in fp32 operation by operation: ix = ((gx + 1) Wm - 1) / 2 clipped to [0, Wm - 1], iy likewise, four
 *     taps accumulated nw, ne, sw, se, a tap outside the map contributing nothing.
 * No attribute is read through an unchecked index.  Outputs, each optional (NULL) but image: image [H,W,3] uint8 = floor(255 clamp(c, 0,
 * 1) + 0.5) (torchvision's save_image; NaN -> 0), image_f [H,W,3] fp32 = the clamped colour (0 on a miss), mask [H,W,3] uint8 = 255 / 0,
 * depth [H,W] fp32 = t (the z-depth) or miss_value, face_id [H,W] int32 in the caller's numbering or -1.
 * validate != 0 applies mesh_renderer.py:44-53: a frame whose mask touches both the first and the last row, or both the first and the
 * last column, or covers more than half of the pixels (as the integer 2 count > H W, where the reference divides twice in fp32) is
 * cleared: image, image_f and mask to 0, depth to miss_value, face_id to -1.  Every wave stores one record (hit count, border bits)
 * with plain stores into scratch (>= snerf_mesh_render_scratch_bytes(H, W) bytes of device memory, 8-byte aligned), a one-block launch
 * reduces them in a fixed order and a finishing launch clears: no host read, no atomics, independent of launch order.  validate = 0
 * skips both launches and does not touch scratch.  flags as for snerf_mesh_trace.  H = 0 or W = 0 is valid; F = 0 is valid (everything
 * misses, the frame is valid, the attribute arguments are not looked at).  Bad arguments (F, H, W, V, U or n_texels < 0, H W >= 2^31,
 * fx or fy zero or not finite, cx or cy not finite, t_max not a positive finite number, unknown flag bits, a null image, with F > 0:
 * both or neither of vertex_color and face_uvs_idx, null faces in colour mode, M < 1 or a null / misaligned table or texel buffer or a
 * null face_material_idx in texture mode, a null or misaligned ws; with validate a null, misaligned or short scratch) return 1 before
 * any launch. */
int snerf_mesh_render_pinhole(const void* ws, int F, float fx, float fy, float cx, float cy, int H, int W, float t_max, float miss_value,
                              int flags, const int* faces, const float* vertex_color, int V, const float* uvs, int U,
                              const int* face_uvs_idx, const int* face_material_idx, const void* texels, long n_texels,
                              const int* materials, int M, int validate, void* scratch, long scratch_bytes, void* image, float* image_f,
                              void* mask, float* depth, int* face_id, void* stream);
/* bytes of scratch the validity rule of snerf_mesh_render_pinhole needs (0 for H or W <= 0) */
long snerf_mesh_render_scratch_bytes(int H, int W);

/* Projected mesh shadows of S-NeRF++ stage 3 (csrc/shadow.hip): s-nerfpp/stage3_code/mesh_shadow.py:21-113 generate_one_shadow for one
 * frame and one instance, with the helpers of stage3_code/utils.py, as three separately callable stages that share one scratch buffer
 * ws (>= snerf_shadow_ws_bytes(H, W, N, r, iter) bytes of device memory, 8-byte aligned; 0 = refused shape).  Images and masks are
 * [H,W,3] uint8; a mask is set where channel 0 is > 0 and is written as 0 / 255 on all three channels (the reference's masks carry one
 * plane three times).  No entry synchronises, allocates or reads a device value on the host; results do not depend on launch order.
 *
 * snerf_shadow_project: utils.py:339-354 process_mesh, :130-154 project_to_ground, :157-168 project, :171-192 points_to_mask.  vertices
 * [N,3] in device memory, fp32 (vertices_f64 = 0) or fp64 (1); all arithmetic is fp64, never contracted.  xf: 28 doubles in HOST memory,
 * read before the call returns: the row-major 3 x 4 placement (Rz(theta) | bbox_center + Rz mesh_bias), the light vector (3), the
 * ground height, the row-major 3 x 4 world-to-pixel matrix P (c2w^-1)[:3].  ground_mode: 0 = the given height; 1 = the reference's
 * `if not ground_height` (None and 0.0 alike): the smallest z of the placed points, found by a two-stage reduction (no atomics); 2 = no
 * ground projection (the reference's check = True, mesh_shadow.py:70-71).  A point is moved by -light (z - ground) / light_z,
 * projected, divided by its third coordinate (no test of its sign), truncated and kept if
 * 0 < x < W and 0 < y < H (strict: column 0 and row 0 are never set).  Divergence: a quotient that is not finite, negative or >= 65536
 * is dropped, where the reference's float -> uint16 cast wraps it.  The splat (plain byte stores of 255 into a zeroed plane of ws) is
 * the input of snerf_shadow_close(mask_in = NULL); mask_out (optional) receives it as an [H,W,3] mask.  N = 0 gives an empty mask.
 *
 * snerf_shadow_close: utils.py:195-211 interpolate = zero-pad by (H, W), cv2.morphologyEx(MORPH_CLOSE, MORPH_RECT (r, r), iterations =
 * iter), crop.  PARITY UNPINNED (cv2 is not available to the build): OpenCV's definition is followed -- dst(x, y) = max (min for the
 * erosion) over 0 <= x', y' < r of src(x + x' - r / 2, y + y' - r / 2), pixels outside the padded image never win, iter dilations and
 * then iter erosions, both with the same un-reflected window (an even r shifts the result).  Runs on bit-packed rows over the image
 * extended by min(iter (r / 2), pad) per side.  mask_in NULL: the splat of the last snerf_shadow_project on this ws.  The closed mask
 * stays in ws for snerf_shadow_fuse(shadow_mask = NULL); mask_out (optional) receives it.  mask_out == mask_in is allowed (the input
 * is packed before anything is written); a partial overlap is refused.  iter = 0 copies.
 *
 * snerf_shadow_fuse: mesh_shadow.py:89-107 blur_shadow, in place on im.  shadow_mask NULL: the closed mask of the last
 * snerf_shadow_close on this ws.  An empty mask leaves im untouched.  Otherwise kw = max(1, (xmax - xmin) / 5), kh likewise from the
 * mask's bounding box (two-stage reduction; written to ws), count = the kw x kh window sum of the 0 / 1 mask with anchor (kw / 2,
 * kh / 2) and BORDER_REFLECT_101 (cv2.blur's definition: PARITY UNPINNED; int32, prefix sums), and per pixel and channel, each step
 * one rounded fp64 operation: b = count * (1.0 / (kw kh)); occ = 255 where b > 0 and not total_mask > 0 (utils.py:214-225
 * check_the_occlusion, per channel), else 0; m = (b * occ) / 255.0; im = (uint8)(im * (1.0 - light_scale * m)), truncating.  check = 1
 * is the reference's check = True (utils.py:248-269 shadow_fuse(im, mask, 1, blur = None)): im[mask > 0] = 0, total_mask unused.
 *
 * snerf_shadow_ws_offset(H, W, which): byte offset in ws of (0) eight int32 = any, kw, kh, xmin, xmax, ymin, ymax, 0 and (1) the
 * counts [H,W] int32, both as the last snerf_shadow_fuse with a non-empty mask left them; -1 for a refused shape or selector.
 * Bad arguments return 1 before any launch: a null vertices (N > 0) / xf / im / total_mask (check = 0) / ws, H or W < 1, H W or the
 * rows / words of the extended bit plane beyond 2^31 - 1, N < 0 or beyond 2^31 - 1, r < 1, iter < 0, vertices_f64 or check other
 * than 0 / 1, ground_mode outside 0..2, light_scale outside [0, 1], a misaligned or short ws (project and fuse need snerf_shadow_ws_bytes(H, W, N, 1, 0), close its own r and iter), an
 * output that overlaps ws or an input, except mask_out == mask_in of snerf_shadow_close. */
long snerf_shadow_ws_bytes(int H, int W, long N, int r, int iter);
long snerf_shadow_ws_offset(int H, int W, int which);
int snerf_shadow_project(const void* vertices, int vertices_f64, long N, const double* xf, int ground_mode, int H, int W, void* mask_out,
                         void* ws, long ws_bytes, void* stream);
int snerf_shadow_close(const void* mask_in, int H, int W, int r, int iter, void* mask_out, void* ws, long ws_bytes, void* stream);
int snerf_shadow_fuse(void* im, const void* total_mask, const void* shadow_mask, int H, int W, double light_scale, int check, void* ws,
                      long ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
